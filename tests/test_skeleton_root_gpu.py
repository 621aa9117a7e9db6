"""The root's trajectory over the frames of a track inside the projection step on an MI355X (pndf_project_options9 of
include/posendf_amd.h, pndf_fk_root_smooth_step of csrc/pndf_fk.h and csrc/pndf_skeleton.hip's pndf_skel_enc_rev_root_kernel; DESIGN.md
section 2j "Root trajectory"): pndf_skel_project with the 256-byte struct against the numpy restatement (tests/skeleton_root_oracle.py).

1. the stated step: rounds of pndf_skel_forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last, kp_energy,
   root and bone_scale -- with one camera, scales, V = 2 and V = 8; T = 2, 3 and 5; every part; with and without the anchor; 0 .. 3 steps.
2. the device against the host twin without a GEMM in the way: a network with d == 0, ten steps, bit for bit, roots included.
3. the reductions.  4. the refusals; the persistent engine keeps refusing the struct.
5. the chunk seam at B = 16,520 with tracks of 7, for 2 steps and for 3 (the odd count exercises the copy back).
6. the Python layer on cuda; the kernel's symbol.
tests/test_skeleton_root.py holds the host twin to the same statements."""
import ctypes

import numpy as np
import pytest

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
import skeleton_root_oracle as sr
import skeleton_views_oracle as sv
from posendf_amd import synth
from test_skeleton_completion_gpu import cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_root import CASES, TwinRoot, check_fit_clip, check_model_fit_keypoints
from test_skeleton_views_gpu import UnitViews

pytestmark = pytest.mark.gpu
BAD_ARG = sr.BAD_ARG


class UnitRoot(sr.RootRunner, UnitViews):
    """pndf_skel_project with the 256-byte struct: poses, mask words, targets, confidences, energies, roots, the root anchor and scales in
    device memory; the view table and the rates in host memory"""


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitRoot(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_root_steps_are_the_stated_step(torch_cuda, case, term):
    sr.check_stated_step(runner_of(torch_cuda, case, "lrelu"), case, term)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_root_steps_are_the_stated_step_with_views_and_no_scales(torch_cuda, case):
    sr.check_stated_step(runner_of(torch_cuda, case, "lrelu"), case, "views2_plain")


def test_root_steps_are_the_stated_step_with_softplus_and_eight_views(torch_cuda):
    sr.check_stated_step(runner_of(torch_cuda, ("hand", True), "softplus"), ("hand", True), "views8", step_counts=(2, 3))


@pytest.mark.parametrize("term", sr.TERMS)
def test_the_anchor_alone_needs_no_tracks(torch_cuda, term):
    sr.check_anchor_without_tracks(runner_of(torch_cuda, ("hand", True), "lrelu"), ("hand", True), term)


# ------------------------------------------------------------------------------------------ 2. the twin
@pytest.mark.parametrize("term", ("camera", "scales", "views2", "views2_plain", "views8"))
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_with_coupled_roots_equals_the_twin(torch_cuda, case, term):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: nothing
    depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit -- poses, energies, roots and scales"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    dev, cpu = UnitRoot(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinRoot(parents, "lrelu", sd, encoder=case[1])
    for T in sr.FRAMES:
        n = sr.P * T
        kp, views, ln, cam = sr.term_inputs(case, term, n, T)
        track = sdo.clip(case, sr.P, T)
        root = si.make_roots(n, 37)
        kw = dict(opts=dict(step_size=0.5), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, sr.P, T)), views=views, cam=cam,
                  rho=si.RHO, ln=ln, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), root_smooth=(sr.LAM_ROT, sr.LAM_TRANS),
                  root_anchor=sr.make_anchor(root), root_data=(sr.MU_ROT, sr.MU_TRANS))
        got = dev.fit9(sk.flat(track), 10, kp, **kw)
        want = cpu.fit9(sk.flat(track), 10, kp, **kw)
        assert not got[1].any() and not want[1].any() and all(np.isfinite(a).all() for a in got if a is not None) and got[2].any()
        for a, b, name in zip(got, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
            if name != "d_last" and a is not None:      # (d == 0 on both sides, asserted above; its sign is the output layer's, not this feature's)
                sk.assert_same(a, b, (term, T, name))
        assert got[0].tobytes() != sk.flat(track).tobytes() and (got[3] != root).any()


# ------------------------------------------------------------------------------------------ 3. the reductions, locality
@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_reductions_to_the_pinned_calls(torch_cuda, case, term):
    sr.check_reductions(runner_of(torch_cuda, case, "lrelu"), case, term)


@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_roots_stay_in_their_track(torch_cuda, case, term):
    sr.check_locality(runner_of(torch_cuda, case, "lrelu"), case, term)


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing(torch_cuda):
    sr.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


def test_the_persistent_engine_refuses_the_256_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 256-byte struct is
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
    Y, E = torch.full((n, 21, 2), 300.0, device="cuda:0"), torch.full((n,), 7.0, device="cuda:0")
    root = torch.from_numpy(si.make_roots(n, 37)).cuda()
    kept = root.clone()
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    b6 = si.c_options6(lib, sk.c_options5(lib, sdo.c_from(lib, {}, None, 2, 0.0, None, None, 0.0, sdo.FREE_ENDS), Y.data_ptr(), None, E.data_ptr(),
                                          rest.ctypes.data, None, None, 21, 0.02), root.data_ptr(), si.CAMERA, 0.0, 0.0, si.NU_TRANS, si.KP_IMAGE)
    big = sr.c_options9(lib, sv.c_options8(lib, sl.c_options7(lib, b6)), None, 0.0, sr.LAM_TRANS)
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
    assert bool((out == 7).all()) and bool((d == 7).all()) and bool((track == 7).all()) and bool((E == 7).all()) and torch.equal(root, kept)


# ------------------------------------------------------------------------------------------ 5. the chunk seam
@pytest.mark.parametrize("steps", (2, 3))
def test_coupled_roots_follow_the_chunk_seam(torch_cuda, steps):
    """B = 16,520 with tracks of 7 frames is more than a chunk (2,340 whole tracks per chunk, seam at 16,380): the tracks on both sides of
    the seam, the first two and the last one equal the same tracks run alone, bit for bit, roots included -- a root, anchor or second-buffer
    offset that forgot the chunk would show here; the odd step count ends in the second buffer and is copied back chunk by chunk"""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitRoot(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n, Tt = 16520, 7
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(r.uniform(100, 500, (n, K, 2)), np.float32)
    conf = r.rand(n, K).astype(np.float32)
    conf[r.rand(n, K) < 0.1] = 0.0
    root = si.make_roots(n, 37)
    anchor = sr.make_anchor(root)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    kw = dict(opts=dict(renormalize="unit", step_size=0.5), frames=Tt, lam=0.5, flags=sdo.FREE_ENDS, cam=si.cam_of(True, si.RHO), rho=si.RHO,
              root_weights=(si.NU_ROT, si.NU_TRANS), root_smooth=(sr.LAM_ROT, sr.LAM_TRANS), root_data=(sr.MU_ROT, sr.MU_TRANS))
    out, d, E, rt, _ = run.fit9(q, steps, kp, root=root, root_anchor=anchor, **kw)
    assert np.isfinite(out).all() and np.isfinite(E).all() and np.isfinite(rt).all() and (E > 0).any() and (rt != root).all(axis=1).any()
    for part in (slice(16373, 16394), slice(0, 14), slice(n - 7, n)):      # (16373 = 7 * 2339: whole tracks on both sides of the seam)
        alone = run.fit9(q[part], steps, dict(kp, Y=kp["Y"][part], conf=conf[part]), root=root[part], root_anchor=anchor[part], **kw)
        for a, b, name in zip(alone[:4], (out, d, E, rt), ("poses", "d_last", "kp_energy", "root")):
            assert a.tobytes() == b[part].tobytes(), (steps, part, name)


# ------------------------------------------------------------------------------------------ 6. Python, the kernel
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_a_root_trajectory_on_cuda(torch_cuda, case):
    parents, sd = sko.case_network(case, "lrelu")
    check_model_fit_keypoints(cuda_model(torch_cuda, parents, "lrelu", sd), UnitRoot(torch_cuda, parents, "lrelu", sd), case, "cuda")


def test_keypoint_fitting_fit_clip_on_cuda(torch_cuda):
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_fit_clip(cuda_model(torch_cuda, parents, "softplus", sd), "cuda")


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_views_kernel", "pndf_skel_enc_rev_root_kernel"} <= ch.exported_symbols(ge.LIB)
