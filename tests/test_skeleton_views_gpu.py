"""Fitting poses to keypoints seen by several cameras inside the projection step on an MI355X (pndf_project_options8 of
include/posendf_amd.h, the several-camera term of csrc/pndf_fk.h and csrc/pndf_skeleton.hip's pndf_skel_enc_rev_views_kernel; DESIGN.md
section 2j "Several cameras"): pndf_skel_project with the 224-byte struct against the numpy restatement (tests/skeleton_views_oracle.py).

1. the stated step: K rounds of pndf_skel_forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last, kp_energy,
   root and bone_scale -- for V = 1, 2, 3 and 8.
   The device against the host twin without a GEMM in the way: a network with d == 0, ten steps, bit for bit.
3. reduction to the pinned calls; 4. skips, the keypoint no view sees; 5. row locality, and the chunk seam at B = 16,520 with tracks of 7.
6. the effect; 7. the refusals, and the persistent engine keeps refusing the struct; the Python layer on cuda; the kernel's symbol.
tests/test_skeleton_views.py holds the host twin to the same statements."""
import ctypes

import numpy as np
import pytest

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
import skeleton_views_oracle as sv
from posendf_amd import synth
from test_skeleton_completion_gpu import cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_length_gpu import UnitLength
from test_skeleton_views import TwinViews, check_driver, check_model_fit_keypoints

pytestmark = pytest.mark.gpu
BAD_ARG = sv.BAD_ARG


class UnitViews(sv.ViewsRunner, UnitLength):
    """pndf_skel_project with the 224-byte struct: poses, mask words, observation, targets [B,V,K,2], confidences [B,V,K], energies, roots
    and scales in device memory; the view table and the rates in host memory"""


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitViews(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", sv.CASES, ids=sko.case_id)
def test_view_steps_are_the_stated_step(torch_cuda, case, act):
    sv.check_stated_step(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("V", sv.VIEW_COUNTS)
@pytest.mark.parametrize("case", sv.CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_under_views_equals_the_twin(torch_cuda, case, V):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: nothing
    depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit -- poses, energies, roots and scales"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    views = sv.make_views(V)
    _, kp = sv.case_kp(case, views, conf=True)
    S = J + len(kp["kpj"])
    track = sdo.clip(case, sv.P, sv.T)
    root = si.make_roots(sv.B, 37)
    dev, cpu = UnitViews(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinViews(parents, "lrelu", sd, encoder=case[1])
    common = dict(views=views, rho=si.RHO, root=root, root_weights=(si.NU_ROT, si.NU_TRANS))
    tracked = dict(opts=dict(step_size=0.5), frames=sv.T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, sv.P, sv.T)),
                   anchor=sk.flat(sdo.make_anchor(track)), mu=sdo.MU)
    for kw, G in ((dict(opts=dict(renormalize="unit")), None), (tracked, sv.P)):
        ln = sl.lengths(None) if G is None else sl.lengths(sl.make_scales(G, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S), (0.5, 2.0))
        got = dev.fit8(sk.flat(track), 10, kp, ln=ln, **common, **kw)
        want = cpu.fit8(sk.flat(track), 10, kp, ln=ln, **common, **kw)
        assert not got[1].any() and not want[1].any() and all(np.isfinite(a).all() for a in got if a is not None) and got[2].any()
        for a, b, name in zip(got, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
            if name != "d_last" and a is not None:      # (d == 0 on both sides, asserted above; its sign is the output layer's, not this feature's)
                sk.assert_same(a, b, sorted(kw) + [V, name])
        assert got[0].tobytes() != sk.flat(track).tobytes() and (got[3] != root).any()


# ------------------------------------------------------------------------------------------ 3. - 4.
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_one_identity_view_and_no_view_are_the_pinned_calls(torch_cuda, case, act):
    assert sv.check_reductions(runner_of(torch_cuda, case, act), case, act) == 0


@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", sv.CASES, ids=sko.case_id)
def test_views_that_take_no_part_are_never_read(torch_cuda, case, act):
    sv.check_skips(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_keypoint_seen_by_no_view_adds_nothing(torch_cuda, case, joint):
    sv.check_unseen_keypoint(runner_of(torch_cuda, case, "lrelu"), case, joint)


# ------------------------------------------------------------------------------------------ 5. row and chunk locality
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose(torch_cuda, case, act):
    sv.check_row_locality(runner_of(torch_cuda, case, act), case, act)


def test_views_follow_the_chunk_seam(torch_cuda):
    """B = 16,520 is more than a chunk: without tracks (seam at 16,384), and with tracks of 7 frames (2,340 whole tracks per chunk, seam at
    16,380, one row of scales each), the poses around the seam, the first 14 and the last 7 equal the same poses run alone, bit for bit --
    a target, confidence, root or scale offset that forgot the chunk or the views' stride would show here"""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitViews(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n, V, Tt = 16520, 3, 7
    views = sv.make_views(V)
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    S = J + K
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(r.uniform(100, 500, (n, V, K, 2)), np.float32)
    conf = r.rand(n, V, K).astype(np.float32)
    conf[r.rand(n, V, K) < 0.1] = 0.0
    root = si.make_roots(n, 37)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    common = dict(opts=dict(renormalize="unit", step_size=0.5), views=views, root_weights=(si.NU_ROT, si.NU_TRANS))
    rates = sl.make_rates(S)
    for kw, g in ((dict(), 1), (dict(frames=Tt, lam=0.5, flags=sdo.FREE_ENDS), Tt)):
        start = sl.make_scales(n // g, S)
        ln = lambda s: sl.lengths(s, sl.NU_LEN, sl.KAPPA, rates, (0.5, 2.0))  # noqa: E731
        out, d, E, rt, sg = run.fit8(q, 2, kp, root=root, ln=ln(start), **common, **kw)
        assert np.isfinite(out).all() and np.isfinite(E).all() and np.isfinite(rt).all() and np.isfinite(sg).all() and (sg != start).any() and (E > 0).any()
        for part in (slice(16373, 16394), slice(0, 14), slice(n - 7, n)):      # (16373 = 7 * 2339: whole tracks on both sides of both seams)
            gs = slice(part.start // g, part.stop // g)
            alone = run.fit8(q[part], 2, dict(kp, Y=kp["Y"][part], conf=conf[part]), root=root[part], ln=ln(start[gs]), **common, **kw)
            for a, b in zip(alone[:4], (out, d, E, rt)):
                assert a.tobytes() == b[part].tobytes(), (sorted(kw), part)
            assert alone[4].tobytes() == sg[gs].tobytes(), (sorted(kw), part, "bone_scale")


# ------------------------------------------------------------------------------------------ 6. the effect
def test_two_views_make_scale_and_depth_observable(torch_cuda):
    parents, sd = sv.effect_inputs()[:2]
    sv.check_effect(UnitViews(torch_cuda, parents, "lrelu", sd))


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing(torch_cuda):
    sv.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


def test_the_persistent_engine_refuses_the_224_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 224-byte struct is
    PNDF_ERR_BAD_ARG, nothing written"""
    torch = torch_cuda
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import Engine
    eng = Engine("lrelu", precision="fp32")
    eng.load_weights(synth.make_weights(0, 2.0, 0.1))
    lib = eng.lib
    n = 8
    q = torch.from_numpy(synth.make_poses(n, seed=5)).cuda()
    out, d = torch.full_like(q, 7.0), torch.full((n,), 7.0, device="cuda:0")
    words = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    views = sv.make_views(2)
    Y, E = torch.full((n, 2, 21, 2), 300.0, device="cuda:0"), torch.full((n,), 7.0, device="cuda:0")
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    b6 = si.c_options6(lib, sk.c_options5(lib, None, Y.data_ptr(), None, E.data_ptr(), rest.ctypes.data, None, None, 21, 0.02), None, sv.UNREAD_CAMERA, 0.0, 0.0,
                       0.0, si.KP_IMAGE)
    big = sv.c_options8(lib, sl.c_options7(lib, b6), views.ctypes.data, 2)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pndf_project_ex(eng.handle, q.data_ptr(), out.data_ptr(), d.data_ptr(), n, 1, ref, st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_complete(eng.handle, q.data_ptr(), words.data_ptr(), out.data_ptr(), d.data_ptr(), n, 1, ref, ws.data_ptr(), st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_complete_step(out.data_ptr(), d.data_ptr(), q.data_ptr(), words.data_ptr(), n, ref, st) == BAD_ARG
    track = torch.full((n // 2, 2, 21, 4), 7.0, device="cuda:0")
    assert lib.pndf_interpolate(eng.handle, q.data_ptr(), q[n // 2:].data_ptr(), None, track.data_ptr(), d.data_ptr(), n // 2, 2, 0, 1, 0.0, ref,
                                ws.data_ptr(), st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_interp_band_step(q.data_ptr(), out.data_ptr(), d.data_ptr(), q.data_ptr(), None, n // 2, 2, 0.0, ref, st) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((d == 7).all()) and bool((track == 7).all()) and bool((E == 7).all())


# ------------------------------------------------------------------------------------------ Python, the kernel
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_views_on_cuda(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    check_model_fit_keypoints(cuda_model(torch_cuda, parents, act, sd), UnitViews(torch_cuda, parents, act, sd), case, "cuda")


def test_keypoint_fitting_driver_takes_views_on_cuda(torch_cuda):
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_driver(cuda_model(torch_cuda, parents, "softplus", sd), "cuda")


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_len_kernel", "pndf_skel_enc_rev_views_kernel"} <= ch.exported_symbols(ge.LIB)
