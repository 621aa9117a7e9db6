"""Fitting bone lengths inside the projection step on an MI355X (pndf_project_options7 of include/posendf_amd.h, the scaled term of
csrc/pndf_fk.h and csrc/pndf_skeleton.hip's pndf_skel_enc_rev_len_kernel and pndf_skel_len_step_kernel; DESIGN.md section 2j "Bone
lengths"): pndf_skel_project with the 208-byte struct against the numpy restatement (tests/skeleton_length_oracle.py).

1. the stated step: K rounds of pndf_skel_forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last, kp_energy,
   root and bone_scale.
2. the device against the host twin without a GEMM in the way: a network with d == 0, ten steps, bit for bit, and the scales moved.
3. the smaller calls; 4. the order of the sum (T = 130: the kernel's workgroup path; T = 2); 5. locality.
6. the chunk seam at B = 16,384 + 136 with per-pose scales and with tracks of 8.
7. tol; 8. the clamp; 9. ten free-running steps, the unit against the fp64 restatement and against the twin.
10. the effect; 11. the refusals, and the persistent engine keeps refusing the struct; 12. the Python layer on cuda; the kernels.
tests/test_skeleton_length.py holds the host twin to the same statements."""
import ctypes

import numpy as np
import pytest

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
from posendf_amd import synth
from test_skeleton_completion_gpu import cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_keypoints import FREE_STEPS
from test_skeleton_keypoints_gpu import UnitRunner
from test_skeleton_length import TwinLength, check_driver, check_model_fit_keypoints, free_gate, free_run

pytestmark = pytest.mark.gpu
BAD_ARG = sl.BAD_ARG


class UnitLength(sl.LengthRunner, si.ImageRunner, UnitRunner):
    """pndf_skel_project with the 208-byte struct: poses, mask words, observation, targets, confidences, energies, roots and scales in device
    memory; the rates in host memory"""


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitLength(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", sl.CASES, ids=sko.case_id)
def test_length_steps_are_the_stated_step(torch_cuda, case, act):
    sl.check_stated_step(runner_of(torch_cuda, case, act), case, act)


# ------------------------------------------------------------------------------------------ 2. device against twin, without a GEMM in the way
@pytest.mark.parametrize("image", [True, False], ids=["image", "3d"])
@pytest.mark.parametrize("case", sl.CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_with_free_lengths_equals_the_twin(torch_cuda, case, image):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: nothing
    depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit -- poses, energies, roots and scales"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    _, kp, _ = si.case_kp(case, image=image, conf=True)
    S = J + len(kp["kpj"])
    track = sdo.clip(case, sl.P, sl.T)
    root = si.make_roots(sl.B, 37)
    dev, cpu = UnitLength(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinLength(parents, "lrelu", sd, encoder=case[1])
    common = dict(cam=si.cam_of(image, si.RHO if image else 0.0), root=root, root_weights=(si.NU_ROT, si.NU_TRANS))
    tracked = dict(opts=dict(step_size=0.5), frames=sl.T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, sl.P, sl.T)),
                   anchor=sk.flat(sdo.make_anchor(track)), mu=sdo.MU)
    for kw, G, per_pose in ((dict(opts=dict(renormalize="unit")), sl.B, False), (tracked, sl.P, False), (tracked, sl.B, True)):
        start = sl.make_scales(G, S)
        ln = sl.lengths(start, sl.NU_LEN, sl.KAPPA, sl.make_rates(S), (0.5, 2.0), per_pose)
        got = dev.fit7(sk.flat(track), 10, kp, ln=ln, **common, **kw)
        want = cpu.fit7(sk.flat(track), 10, kp, ln=ln, **common, **kw)
        assert not got[1].any() and not want[1].any() and all(np.isfinite(a).all() for a in got) and got[2].any()
        for a, b, name in zip(got, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
            if name != "d_last":      # (d == 0 on both sides, asserted above; its sign is the output layer's, not this feature's)
                sk.assert_same(a, b, sorted(kw) + [per_pose, name])
        assert got[0].tobytes() != sk.flat(track).tobytes() and (got[4] != start).any()      # the scales moved


# ------------------------------------------------------------------------------------------ 3. - 5.
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_scales_it_is_the_smaller_call(torch_cuda, case, act):
    sl.check_smaller_calls(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_the_group_sum_runs_in_the_stated_order(torch_cuda, case):
    sl.check_summation_order(runner_of(torch_cuda, case, "lrelu"), case)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("roots5", True), ("hand", False)], ids=sko.case_id)
def test_bad_values_stay_in_their_group_and_idle_scales_stay(torch_cuda, case):
    sl.check_locality(runner_of(torch_cuda, case, "lrelu"), case)


# ------------------------------------------------------------------------------------------ 6. the chunk seam
def test_scales_follow_the_chunk_seam(torch_cuda):
    """B = 16,384 + 136 is more than a chunk: with per-pose scales, and with tracks of 8 frames (2,048 whole tracks per chunk, one row of
    scales each), the poses around the seam, the first 16 and the last 8 equal the same poses run alone, bit for bit, scales included -- a
    scale row, an h row or a distance offset that forgot the chunk would show here"""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitLength(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n = 16384 + 136
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    S = J + K
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(r.uniform(-1.5, 1.5, (n, K, 3)), np.float32)
    conf = r.rand(n, K).astype(np.float32)
    conf[r.rand(n, K) < 0.1] = 0.0
    root = si.make_roots(n, 37, depth=0.0)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    common = dict(opts=dict(renormalize="unit", step_size=0.5), root_weights=(si.NU_ROT, si.NU_TRANS))
    rates = sl.make_rates(S)
    for kw, g in ((dict(), 1), (dict(frames=8, lam=0.5, flags=sdo.FREE_ENDS), 8)):
        start = sl.make_scales(n // g, S)
        ln = lambda s: sl.lengths(s, sl.NU_LEN, sl.KAPPA, rates, (0.5, 2.0))  # noqa: E731
        out, d, E, rt, sg = run.fit7(q, 2, kp, root=root, ln=ln(start), **common, **kw)
        assert np.isfinite(out).all() and np.isfinite(E).all() and np.isfinite(rt).all() and np.isfinite(sg).all() and (sg != start).any()
        for part in (slice(16376, 16392), slice(0, 16), slice(n - 8, n)):
            gs = slice(part.start // g, part.stop // g)
            alone = run.fit7(q[part], 2, dict(kp, Y=kp["Y"][part], conf=conf[part]), root=root[part], ln=ln(start[gs]), **common, **kw)
            for a, b in zip(alone[:4], (out, d, E, rt)):
                assert a.tobytes() == b[part].tobytes(), (sorted(kw), part)
            assert alone[4].tobytes() == sg[gs].tobytes(), (sorted(kw), part, "bone_scale")


# ------------------------------------------------------------------------------------------ 7. - 8.
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_a_group_at_rest_keeps_its_scales(torch_cuda, case, act):
    sl.check_tol(runner_of(torch_cuda, case, act), case)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True)], ids=sko.case_id)
def test_the_clamp_is_exact_and_nan_stays(torch_cuda, case):
    sl.check_clamp(runner_of(torch_cuda, case, "lrelu"), case)


# ------------------------------------------------------------------------------------------ 9. free running
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    got = free_run(UnitLength(torch_cuda, parents, act, sd), case)
    free_gate(got, case, act, f"unit {sko.case_id(case)} {act}")
    cpu = free_run(TwinLength(parents, act, sd), case)
    free_gate(cpu, case, act, f"twin {sko.case_id(case)} {act}")
    free_gate(got, case, act, f"unit against twin {sko.case_id(case)} {act}", ref=cpu)
    assert FREE_STEPS == 10


# ------------------------------------------------------------------------------------------ 10. the effect
@pytest.mark.parametrize("per_pose,image", [(False, False), (True, False), (False, True)], ids=["shared", "per-pose", "image-prior"])
def test_bone_lengths_are_found_from_a_clip(torch_cuda, per_pose, image):
    parents, sd = sl.effect_inputs()[:2]
    sl.check_effect(UnitLength(torch_cuda, parents, "lrelu", sd), per_pose, image)


# ------------------------------------------------------------------------------------------ 11. refusals
def test_refusals_write_nothing(torch_cuda):
    sl.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


def test_the_persistent_engine_refuses_the_208_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 208-byte struct is
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
    Y, E = torch.full((n, 21, 3), 0.5, device="cuda:0"), torch.full((n,), 7.0, device="cuda:0")
    scale_np = sl.make_scales(n, 42)
    scale = torch.from_numpy(scale_np.copy()).cuda()
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    b6 = si.c_options6(lib, sk.c_options5(lib, None, Y.data_ptr(), None, E.data_ptr(), rest.ctypes.data, None, None, 21, 0.02))
    big = sl.c_options7(lib, b6, scale.data_ptr(), None, sl.NU_LEN, sl.KAPPA)
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
    assert scale.cpu().numpy().tobytes() == scale_np.tobytes()


# ------------------------------------------------------------------------------------------ 12. Python
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_scales_on_cuda(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    check_model_fit_keypoints(cuda_model(torch_cuda, parents, act, sd), UnitLength(torch_cuda, parents, act, sd), case, "cuda")


def test_keypoint_fitting_driver_fits_lengths_on_cuda(torch_cuda):
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_driver(cuda_model(torch_cuda, parents, "softplus", sd), "cuda")


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_image_kernel", "pndf_skel_enc_rev_len_kernel", "pndf_skel_len_step_kernel"} <= ch.exported_symbols(ge.LIB)
