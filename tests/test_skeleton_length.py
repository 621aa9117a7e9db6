"""Fitting bone lengths inside the projection step on the host (pndf_project_options7 of include/posendf_amd.h, the scaled term of
csrc/pndf_fk.h; DESIGN.md section 2j "Bone lengths"): the host twin pndf_project_ex_cpu with the 208-byte struct against the numpy
restatement of the scaled tree, the per-frame gradient of the scales, the group's sum in the stated order and the scales' step
(tests/skeleton_length_oracle.py).

0. the restatement itself: its float64 dE/dQ, dE/d(c, s) and dE/dsigma against torch autograd of forward_kinematics(bone_scale=) +
   camera_project, to 1e-9.
1. the stated step: K rounds of the twin's own forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last,
   kp_energy, root and bone_scale -- in 3D and image mode, shared and per pose, with mask, anchor, free ends, a clamp and rates with zeros.
3. the smaller calls; 4. the order of the sum (T = 130 and T = 2); 5. locality; 7. tol; 8. the clamp.
9. free running: ten steps against the fp64 restatement; the scales gated at 4x the float32 restatement's own error.
10. the effect: E falls at every step and every track's scales end nearer the truth than they started.
11. the refusals; the other entry points refuse the 208-byte struct.  12. the ABI, the binding, the Python layer on a cpu model.
Every test but 0 fails on the parent commit, where the 208-byte struct is refused and ProjectOptions7 does not exist.  Runs without a
GPU; tests/test_skeleton_length_gpu.py holds the HIP unit to the same statements (and has 2. and 6.)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
from conftest import outlier_gate, rel_err_rows
from test_skeleton_completion import cpu_model
from test_skeleton_image import with_root
from test_skeleton_keypoints import FREE_STEPS, TOL, TwinRunner

BAD_ARG = sl.BAD_ARG
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TwinLength(sl.LengthRunner, si.ImageRunner, TwinRunner):
    """pndf_project_ex_cpu with the 208-byte struct: every array in host memory"""


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinLength(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 0. the restatement
@pytest.mark.parametrize("image", [False, True], ids=["3d", "image"])
@pytest.mark.parametrize("case", sl.CASES[:5], ids=sko.case_id)
def test_restatement_against_autograd(case, image):
    from posendf_amd import camera_project, forward_kinematics
    n = 8
    parents, kp, _ = si.case_kp(case, n, image=image)
    J, K = len(parents), len(kp["kpj"])
    q = sk.unit_poses(n, J, 3).astype(np.float64) * np.random.RandomState(1).uniform(0.5, 2.0, (n, J, 1))
    conf = np.abs(np.nan_to_num(sk.make_conf(K, n), nan=0.5)).astype(np.float64)
    root = si.make_roots(n, 37).astype(np.float64)
    sigma = sl.make_scales(n, J + K).astype(np.float64)
    cam = si.cam_of(image)
    E, g, gr, h = sl.len_energy_grad(q, parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"].astype(np.float64), conf, root, cam, sigma)
    qt, rt, st = (torch.tensor(a, requires_grad=True) for a in (q, root, sigma))
    C = camera_project(forward_kinematics(qt, parents, torch.tensor(kp["rest"], dtype=torch.float64), kp["kpj"], torch.tensor(kp["kpo"], dtype=torch.float64), st), rt)
    Y = torch.tensor(kp["Y"], dtype=torch.float64)
    if image:
        fx, fy, cx, cy = si.CAMERA
        front = C[..., 2] > 0
        z = torch.where(front, C[..., 2], torch.ones_like(C[..., 2]))
        e = torch.stack([C[..., 0] / z - (Y[..., 0] - cx) / fx, C[..., 1] / z - (Y[..., 1] - cy) / fy], dim=-1)
        sq = torch.where(front, (e * e).sum(-1), torch.zeros_like(z))
    else:
        sq = ((C - Y) ** 2).sum(-1)
    Et = 0.5 * (torch.tensor(conf) * sq).sum(-1)
    Et.sum().backward()
    scale = max(1.0, float(np.abs(h).max()))
    assert np.abs(E - Et.detach().numpy()).max() < 1e-9 * max(1.0, float(E.max()))
    assert np.abs(g - qt.grad.numpy()).max() < 1e-9 * scale and np.abs(gr - rt.grad.numpy()).max() < 1e-9 * scale
    assert np.abs(h - st.grad.numpy()).max() < 1e-9 * scale and np.abs(h).max() > 0


def test_group_sum_order():
    """blocks of 64, then the partials: another order than the plain sequential sum, and the plain sum for n <= 64"""
    r = np.random.RandomState(0)
    h = (r.randn(3, 130, 5) * 10.0 ** r.uniform(-3, 3, (3, 130, 5))).astype(np.float32)
    want = np.zeros((3, 5), np.float32)
    for b in (slice(0, 64), slice(64, 128), slice(128, 130)):
        part = np.zeros((3, 5), np.float32)
        for f in range(b.start, b.stop):
            part = part + h[:, f]
        want = want + part
    assert sl.group_sum(h).tobytes() == want.tobytes() and sl.group_sum(h).tobytes() != sl.group_sum(h, None).tobytes()
    assert sl.group_sum(h[:, :64]).tobytes() == sl.group_sum(h[:, :64], None).tobytes()


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", sl.CASES, ids=sko.case_id)
def test_length_steps_are_the_stated_step(case, act):
    sl.check_stated_step(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 3. - 8.
@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_scales_it_is_the_smaller_call(case, act):
    sl.check_smaller_calls(runner_of(case, act), case, act)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_the_group_sum_runs_in_the_stated_order(case):
    sl.check_summation_order(runner_of(case, "lrelu"), case)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("roots5", True), ("hand", False)], ids=sko.case_id)
def test_bad_values_stay_in_their_group_and_idle_scales_stay(case):
    sl.check_locality(runner_of(case, "lrelu"), case)


@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_a_group_at_rest_keeps_its_scales(case, act):
    sl.check_tol(runner_of(case, act), case)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True)], ids=sko.case_id)
def test_the_clamp_is_exact_and_nan_stays(case):
    sl.check_clamp(runner_of(case, "lrelu"), case)


# ------------------------------------------------------------------------------------------ 9. free running
FREE_KW = dict(smooth=sk.LAMBDA, free_ends=True, renormalize="unit")
FREE_WEIGHTS = (si.NU_ROT, si.NU_TRANS)
SCALE_MARGIN = 4.0      # the margin the project gives the slerp fill: 4x the float32 restatement's own error against fp64


def free_inputs(case):
    """(the noisy clip [6,7,J,4], kp with pixel targets and confidences, the start roots, the start scales [6,S])"""
    x = sdo.noisy_clip(case)
    n = x.shape[0] * x.shape[1]
    parents, kp, _ = si.case_kp(case, n, conf=True)
    return x, kp, si.make_roots(n, 37), sl.make_scales(x.shape[0], len(parents) + len(kp["kpj"]))


@functools.lru_cache(maxsize=None)
def oracle_tracks(case, act):
    """(fp64 rows, fp32 rows, kink margins or None, fp64 scales, fp32 scales) of the numpy restatement after ten steps"""
    parents, sd = sko.case_network(case, act)
    x, kp, root, sg = free_inputs(case)
    ln = sl.lengths(sg, sl.NU_LEN, sl.KAPPA, clamp=(0.5, 2.0))
    q64, _, _, margin, r64, s64 = sl.relax(x, sd, FREE_STEPS, act, parents, kp, si.cam_of(True), ln, root, FREE_WEIGHTS, sl.NU, np.float64, **FREE_KW)
    q32, _, _, _, r32, s32 = sl.relax(x, sd, FREE_STEPS, act, parents, kp, si.cam_of(True), ln, root, FREE_WEIGHTS, sl.NU, np.float32, **FREE_KW)
    return with_root(q64, r64), with_root(q32, r32), (None if act == "softplus" else margin), s64, s32


def scale_error(s, truth):
    return float(np.abs(np.asarray(s, np.float64) - truth).max())


def free_gate(got, case, act, what, ref=None):
    """poses and roots: test_skeleton_image.free_gate's gate (conftest.outlier_gate at 1e-4 against the fp64 restatement, the float32
    restatement's rows or `ref`'s as the reference rows).  The scales: their largest absolute error against the fp64 restatement is at most
    SCALE_MARGIN times the float32 restatement's own on the same inputs.  Measured on the CPU (profiles/skeleton_lengths/free_run.json):
    the float32 restatement's error is 2.34e-7 / 2.58e-7 (hand, lrelu / softplus) and 3.78e-7 / 3.78e-7 (tree32); the twin's is the same."""
    rows_, scales = got
    truth, r32, margin, s64, s32 = oracle_tracks(case, act)
    own = rel_err_rows(r32, truth)
    assert np.isfinite(own).all() and own.max() < 1.0, (what, float(own.max()))
    outlier_gate(own, own, TOL, f"{what}: the float32 restatement itself", margin=margin)
    mine = rel_err_rows(rows_, truth)
    base = own if ref is None else rel_err_rows(ref[0], truth)
    outlier_gate(mine, base, TOL, what, margin=margin)
    own_s, mine_s = scale_error(s32, s64), scale_error(scales, s64)
    print(f"[{what}] scales: max |error| {mine_s:.3e} | the float32 restatement's {own_s:.3e} | per-pose error median {np.median(mine):.2e} max {mine.max():.2e}")
    assert own_s > 0 and mine_s <= SCALE_MARGIN * own_s, (what, mine_s, own_s)
    return own_s, mine_s


def free_run(run, case):
    x, kp, root, sg = free_inputs(case)
    got, d, E, rt, s = run.fit7(sk.flat(x), FREE_STEPS, kp, opts=dict(renormalize="unit"), frames=x.shape[1], lam=sk.LAMBDA, flags=sdo.FREE_ENDS,
                                cam=si.cam_of(True), root=root, root_weights=FREE_WEIGHTS, ln=sl.lengths(sg, sl.NU_LEN, sl.KAPPA, clamp=(0.5, 2.0)))
    assert np.isfinite(got).all() and np.isfinite(d).all() and np.isfinite(E).all() and np.isfinite(rt).all() and np.isfinite(s).all()
    assert (s != sg).any()
    return with_root(got.reshape(x.shape), rt), s


@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(case, act):
    own, mine = free_gate(free_run(runner_of(case, act), case), case, act, f"twin {sko.case_id(case)} {act}")
    recorded = json.load(open(os.path.join(REPO, "profiles", "skeleton_lengths", "free_run.json")))
    assert f"{sko.case_id(case)}-{act}" in recorded["float32_restatement_max_abs_error"]


# ------------------------------------------------------------------------------------------ 10. the effect
@pytest.mark.parametrize("per_pose,image", [(False, False), (True, False), (False, True)], ids=["shared", "per-pose", "image-prior"])
def test_bone_lengths_are_found_from_a_clip(per_pose, image):
    """N = sl.EFFECT_STEPS steps of pure inverse kinematics (3D: kappa = 0) from sigma = 1: E falls at every step and every track's mean
    |sigma - true| ends below its start.  With per-pose scales E falls.  In image mode with a free translation the overall scale trades
    against depth and is unobservable: that variant uses kappa > 0 and asserts only that E falls."""
    parents, sd = sl.effect_inputs()[:2]
    sl.check_effect(TwinLength(parents, "lrelu", sd), per_pose, image)


# ------------------------------------------------------------------------------------------ 11. refusals
def test_refusals_write_nothing():
    sl.check_refusals(runner_of(("hand", True), "lrelu"))


def test_the_other_entry_points_refuse_the_208_byte_struct():
    """every other function with a pndf_project_options parameter: a 208-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers; the persistent engine's entry points are in the GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    rest, Y, E = np.zeros((21, 3), np.float32), np.full((4, 21, 3), 0.5, np.float32), np.full(4, 7.0, np.float32)
    scale = sl.make_scales(4, 42)
    kept = scale.copy()
    b6 = si.c_options6(lib, sk.c_options5(lib, None, Y.ctypes.data, None, E.ctypes.data, rest.ctypes.data, None, None, 21, 0.02))
    big = sl.c_options7(lib, b6, scale.ctypes.data, None, sl.NU_LEN, sl.KAPPA)
    out, d = np.full_like(q, 7.0), np.full(8, 7.0, np.float32)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    track = np.full((2, 2, 21, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q[2:].ctypes.data, None, track.ctypes.data, d.ctypes.data, 2, 2, 0, 1, 0.0, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_complete_step(out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 4, ref, None) == BAD_ARG
    assert lib.pndf_interp_band_step(q.ctypes.data, out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 2, 2, 0.0, ref, None) == BAD_ARG
    assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(track == 7.0) and np.all(E == 7.0) and scale.tobytes() == kept.tobytes()
    # the twin that takes it does, on this 21-joint handle too: the SMPL table with the joints as keypoints
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and scale.tobytes() != kept.tobytes()


# ------------------------------------------------------------------------------------------ 12. the library, the ABI, Python
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert {"pndf_skel_enc_rev_len_kernel", "pndf_skel_len_step_kernel"} <= ch.exported_symbols(ge.LIB)
    o7 = abi.ProjectOptions7
    assert ctypes.sizeof(o7) == 208 and engine.ProjectOptions7 is o7 and abi.LEN_PER_POSE == 1
    assert (o7.base6.offset, o7.bone_scale.offset, o7.len_rate.offset, o7.nu_len.offset, o7.kappa.offset, o7.len_min.offset, o7.len_max.offset, o7.len_flags.offset,
            o7.reserved3.offset) == (0, 168, 176, 184, 188, 192, 196, 200, 204)
    lib = engine.load_library()
    o = engine.project_options7(lib, 64, 7, smooth=0.25, kp_target_ptr=512, rest_ptr=4096, n_keypoints=20, kp_weight=0.02, step_size=0.5, renorm="unit",
                                root_ptr=32768, root_weights=(0.25, 0.5), camera=(500.0, 480.0, 320.0, 240.0), rho=0.125, bone_scale_ptr=65536,
                                len_rate=[1.0, 0.0, 0.5], len_weight=0.75, len_prior=0.375, len_range=(0.5, 2.0), per_pose_lengths=True)
    b = o.base6.base5.base4.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, o.base6.base5.base4.base3.frames, o.base6.base5.kp_target, o.base6.base5.rest, o.base6.base5.n_keypoints) == (208, 0.5, 1, 7, 512, 4096, 20)
    assert (o.base6.root, o.base6.fx, o.base6.rho, o.base6.nu_rot, o.base6.nu_trans, o.base6.kp_flags) == (32768, 500.0, 0.125, 0.25, 0.5, 1)
    assert (o.bone_scale, o.nu_len, o.kappa, o.len_min, o.len_max, o.len_flags, o.reserved3) == (65536, 0.75, 0.375, 0.5, 2.0, 1, 0)
    assert list((ctypes.c_float * 3).from_address(o.len_rate)) == [1.0, 0.0, 0.5]
    o = engine.project_options7(lib, None, 0)
    assert (o.base6.base5.base4.base3.base2.base.struct_size, o.bone_scale, o.len_rate, o.nu_len, o.kappa, o.len_min, o.len_max, o.len_flags) == (208, None, None, 0.0, 0.0, 0.0, 0.0, 0)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sl.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "skel" in n and ("len" in n or "scale" in n)]
    assert not [h for h in abi.HEADERS if "len" in h or "scale" in h]


def test_forward_kinematics_with_scales():
    from posendf_amd import forward_kinematics
    from posendf_amd.engine import PndfError
    for name in ("hand", "tree32", "roots5"):
        parents = sko.SKELETONS[name]
        J = len(parents)
        rest, kpj, kpo = sk.tables(parents)
        K = len(kpj)
        for dt in (torch.float32, torch.float64):
            q = torch.from_numpy(sk.unit_poses(12, J, 3)).to(dt)
            args = (parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
            plain = forward_kinematics(q, *args)
            for shape in ((J + K,), (12, J + K)):
                assert torch.equal(forward_kinematics(q, *args, bone_scale=torch.ones(shape)), plain)      # bit for bit
        sigma = sl.make_scales(12, J + K).astype(np.float64)
        scaled_rest = [[sigma[:, j] * np.float64(rest[j][x]) for x in range(3)] for j in range(J)]
        _, _, _, G, p = sk._forward(q.numpy().astype(np.float64), parents, scaled_rest)
        want = np.stack([np.stack([p[a][x] + sigma[:, J + k] * sk.dot3(G[a][3 * x], np.float64(o[0]), G[a][3 * x + 1], np.float64(o[1]), G[a][3 * x + 2], np.float64(o[2]))
                                   for x in range(3)], axis=-1) for k, (a, o) in enumerate(zip(kpj, kpo))], axis=1)
        got = forward_kinematics(q.double(), *args, bone_scale=torch.from_numpy(sigma))
        assert np.abs(got.numpy() - want).max() < 1e-12
        with pytest.raises(PndfError):
            forward_kinematics(q, *args, bone_scale=torch.ones(J + K - 1))


@pytest.mark.parametrize("act", sl.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_scales_on_cpu(case, act):
    check_model_fit_keypoints(cpu_model(sko.case_network(case, act)[0], act, sko.case_network(case, act)[1]), runner_of(case, act), case, "cpu")


def check_model_fit_keypoints(net, run, case, device):
    """fit_keypoints(bone_scale=, return_scale=True) equals the raw call, bit for bit, shared and per pose; the inputs are not written"""
    from posendf_amd.engine import PndfError
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    _, kp, _ = si.case_kp(case, image=False, conf=True)
    S = J + len(kp["kpj"])
    q_np = sk.flat(sdo.clip(case, sl.P, sl.T))
    root_np = si.make_roots(sl.B, 37)
    rates = sl.make_rates(S)
    to = lambda a: torch.from_numpy(np.array(a)).to(device)  # noqa: E731
    q, Y, c, root = to(q_np), to(kp["Y"]), to(kp["conf"]), to(root_np)
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    weights = (si.NU_ROT, si.NU_TRANS)
    for per_pose in (False, True):
        start = sl.make_scales(sl.B if per_pose else sl.P, S)
        want = run.fit7(q_np, sl.K_STEPS, kp, opts=dict(renormalize="unit"), frames=sl.T, lam=0.5, flags=sdo.FREE_ENDS, root=root_np, root_weights=weights,
                        ln=sl.lengths(start, sl.NU_LEN, sl.KAPPA, rates, (0.5, 2.0), per_pose))
        sg = to(start)
        out, d, E, rt, s = net.fit_keypoints(q, Y, rest, steps=sl.K_STEPS, conf=c, renormalize="unit", frames=sl.T, smooth=0.5, free_ends=True, return_energy=True,
                                             root=root, root_weights=weights, return_root=True, bone_scale=sg, scale_weight=sl.NU_LEN, scale_prior=sl.KAPPA,
                                             scale_rates=rates, scale_range=(0.5, 2.0), per_pose_scale=per_pose, return_scale=True, **tables)
        assert s.device.type == device and s.shape == start.shape
        for a, b in zip((out, d, E, rt, s), want):
            assert a.cpu().numpy().tobytes() == b.tobytes(), per_pose
        assert s.cpu().numpy().tobytes() != start.tobytes() and sg.cpu().numpy().tobytes() == start.tobytes()      # the input is not written
    # scales [S] are every group's start; without bone_scale a positive weight starts at ones; return_scale alone gives ones
    a = net.fit_keypoints(q, Y, rest, steps=2, conf=c, bone_scale=to(start[0]), scale_weight=sl.NU_LEN, return_scale=True, **tables)
    b = net.fit_keypoints(q, Y, rest, steps=2, conf=c, bone_scale=to(start[:1]).expand(sl.B, S), scale_weight=sl.NU_LEN, return_scale=True, **tables)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = net.fit_keypoints(q, Y, rest, steps=2, conf=c, scale_weight=sl.NU_LEN, return_scale=True, **tables)
    b = net.fit_keypoints(q, Y, rest, steps=2, conf=c, bone_scale=torch.ones(S), scale_weight=sl.NU_LEN, return_scale=True, **tables)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[2], torch.ones_like(a[2]))
    a = net.fit_keypoints(q, Y, rest, steps=2, conf=c, **tables)
    b = net.fit_keypoints(q, Y, rest, steps=2, conf=c, return_scale=True, **tables)
    assert torch.equal(a[0], b[0]) and torch.equal(b[2], torch.ones(sl.B, S, device=b[2].device))
    e = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, bone_scale=torch.ones(S), scale_weight=sl.NU_LEN, return_scale=True, **tables)
    assert e[0].shape == (0, J, 4) and e[2].shape == (0, S)
    for kw in (dict(bone_scale=torch.ones(S - 1)), dict(bone_scale=torch.ones(sl.B, S, dtype=torch.int64)), dict(scale_weight=-1.0), dict(scale_prior=float("nan")),
               dict(scale_range=(0.0, 2.0)), dict(scale_range=(1.0,)), dict(scale_rates=-torch.ones(S)), dict(scale_rates=torch.ones(S + 1))):
        args = dict(bone_scale=to(start[0]), scale_weight=sl.NU_LEN)
        args.update(kw)
        with pytest.raises(PndfError):
            net.fit_keypoints(q, Y, rest, steps=1, conf=c, **args, **tables)


def check_driver(net, device):
    """KeypointFitting.fit(fit_lengths=True) on targets made with other bone lengths: the scales of the chosen hypothesis come back, moved and
    inside their range, and the energy it reports is that of the pose and the scales it returns"""
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    S = J + len(kpj)
    clean = net.project(torch.from_numpy(sk.unit_poses(12, J, 7)).to(device), steps=20, renormalize="unit")[0]
    true_scale = torch.from_numpy(sl.make_scales(12, S, 67)).to(device)
    Y = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo), bone_scale=true_scale)
    driver = KeypointFitting(net, body_model=None, device=device)
    kw = dict(rest=torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo), hypotheses=4, iterations=3,
              steps_per_iter=10, seed=0)
    pose, energy, dist, start_energy, scale = driver.fit(Y, fit_lengths=True, **kw)
    assert pose.shape == (12, J, 4) and scale.shape == (12, S) and scale.device.type == device
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(scale).all()) and bool((scale >= 0.5).all()) and bool((scale <= 2.0).all())
    assert not torch.equal(scale, torch.ones_like(scale))
    fixed = driver.fit(Y, **kw)
    assert len(fixed) == 4 and torch.equal(fixed[3], start_energy)
    assert float(energy.median()) < float(start_energy.median())      # (30 untuned steps: no claim against the fit with fixed lengths)
    # the energy it reports is the energy of the pose and the scales it returns
    Pk = posendf_amd.forward_kinematics(pose, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo), bone_scale=scale)
    assert torch.allclose(energy, 0.5 * ((Pk - Y) ** 2).sum((-1, -2)), rtol=1e-3, atol=1e-7)


def test_keypoint_fitting_driver_fits_lengths_on_a_hand():
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_driver(cpu_model(parents, "softplus", sd), "cpu")


def test_keypoint_fitting_main_takes_fit_lengths(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    _, kp, _ = si.case_kp(case, 5, image=False)
    np.savez(tmp_path / "kp.npz", keypoints=kp["Y"], rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo)
    pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2",
                         "--iterations", "2", "--steps_per_iter", "3", "--fit-lengths", "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == (5, len(parents), 4) and np.array_equal(f["pose"], pose.numpy())
        assert f["scale"].shape == (5, len(parents) + len(kpj)) and not np.array_equal(f["scale"], np.ones_like(f["scale"]))
