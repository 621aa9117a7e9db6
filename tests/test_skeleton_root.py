"""The root's trajectory over the frames of a track inside the projection step, on the host (pndf_project_options9 of
include/posendf_amd.h, pndf_fk_root_smooth_step of csrc/pndf_fk.h; DESIGN.md section 2j "Root trajectory"): the host twin
pndf_project_ex_cpu with the 256-byte struct against the numpy restatement (tests/skeleton_root_oracle.py).

1. the stated step: rounds of the twin's own forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last,
   kp_energy, root and bone_scale -- with one camera, scales and V = 2; T = 2, 3 and 5; rotation only, translation only and both; with and
   without the anchor; 0, 1, 2 and 3 steps (both parities of the root buffer).
2. the reductions: lambda 0 without an anchor is the 224-byte call, nu = 0 the 72-byte call, steps == 0 leaves the root, equal roots give
   the uncoupled step's values.
3. locality: a NaN root stays in its track, an anchor whose mu is 0 is never read, a part with nu == 0 keeps its bits.
4. the refusals, the ABI, the other entry points.  5. the effect, on the float64 restatement alone.  6. the Python layer on a cpu model.
Every test but 5 fails on the parent commit, where the 256-byte struct is refused and fit_keypoints has no root_smooth.  Runs without a
GPU; tests/test_skeleton_root_gpu.py holds the HIP unit to the same statements (and has the chunk seam)."""
import ctypes
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
import skeleton_root_oracle as sr
import skeleton_views_oracle as sv
from test_skeleton_completion import cpu_model
from test_skeleton_views import TwinViews

BAD_ARG = sr.BAD_ARG
CASES = [("hand", True), ("tree32", True), ("one", True), ("hand", False)]


class TwinRoot(sr.RootRunner, TwinViews):
    """pndf_project_ex_cpu with the 256-byte struct: every array in host memory"""


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinRoot(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_root_steps_are_the_stated_step(case, term):
    sr.check_stated_step(runner_of(case, "lrelu"), case, term)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_root_steps_are_the_stated_step_with_views_and_no_scales(case):
    sr.check_stated_step(runner_of(case, "lrelu"), case, "views2_plain")


def test_root_steps_are_the_stated_step_with_softplus_and_eight_views():
    sr.check_stated_step(runner_of(("hand", True), "softplus"), ("hand", True), "views8", step_counts=(2, 3))


@pytest.mark.parametrize("term", sr.TERMS)
def test_the_anchor_alone_needs_no_tracks(term):
    sr.check_anchor_without_tracks(runner_of(("hand", True), "lrelu"), ("hand", True), term)


# ------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_reductions_to_the_pinned_calls(case, term):
    sr.check_reductions(runner_of(case, "lrelu"), case, term)


# ------------------------------------------------------------------------------------------ 3. locality
@pytest.mark.parametrize("term", sr.TERMS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_roots_stay_in_their_track(case, term):
    sr.check_locality(runner_of(case, "lrelu"), case, term)


# ------------------------------------------------------------------------------------------ 4. refusals, ABI
def test_refusals_write_nothing():
    sr.check_refusals(runner_of(("hand", True), "lrelu"))


def test_the_other_entry_points_refuse_the_256_byte_struct():
    """every other function with a pndf_project_options parameter: a 256-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers; the persistent engine's entry points are in the GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    rest, Y, E = np.zeros((21, 3), np.float32), np.full((4, 21, 2), 300.0, np.float32), np.full(4, 7.0, np.float32)
    root = si.make_roots(4, 37)
    b6 = si.c_options6(lib, sk.c_options5(lib, sdo.c_from(lib, {}, None, 2, 0.0, None, None, 0.0, sdo.FREE_ENDS), Y.ctypes.data, None, E.ctypes.data,
                                          rest.ctypes.data, None, None, 21, 0.02), root.ctypes.data, si.CAMERA, 0.0, 0.0, si.NU_TRANS, si.KP_IMAGE)
    big = sr.c_options9(lib, sv.c_options8(lib, sl.c_options7(lib, b6)), None, 0.0, sr.LAM_TRANS)
    out, d = np.full_like(q, 7.0), np.full(8, 7.0, np.float32)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    track = np.full((2, 2, 21, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q[2:].ctypes.data, None, track.ctypes.data, d.ctypes.data, 2, 2, 0, 1, 0.0, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_complete_step(out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 4, ref, None) == BAD_ARG
    assert lib.pndf_interp_band_step(q.ctypes.data, out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 2, 2, 0.0, ref, None) == BAD_ARG
    assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(track == 7.0) and np.all(E == 7.0)
    # the twin that takes it does, on this 21-joint handle too: the SMPL table with the joints as keypoints, two tracks of two frames
    kept = root.copy()
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0, lib.pndf_cpu_last_error(eng.handle)
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and root.tobytes() != kept.tobytes()


def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_root_kernel" in ch.exported_symbols(ge.LIB)
    o9 = abi.ProjectOptions9
    assert ctypes.sizeof(o9) == 256 and engine.ProjectOptions9 is o9
    assert (o9.base8.offset, o9.root_anchor.offset, o9.lambda_rot.offset, o9.lambda_trans.offset, o9.mu_rot.offset, o9.mu_trans.offset,
            o9.reserved5.offset) == (0, 224, 232, 236, 240, 244, 248)
    lib = engine.load_library()
    table = sv.make_views(3)
    o = engine.project_options9(lib, 64, 7, smooth=0.25, kp_target_ptr=512, rest_ptr=4096, n_keypoints=20, kp_weight=0.02, step_size=0.5, renorm="unit",
                                root_ptr=32768, root_weights=(0.25, 0.5), rho=0.125, bone_scale_ptr=65536, len_weight=0.75, len_rate=[0.5] * 35, views=table,
                                root_smooth=(0.375, 0.25), root_anchor_ptr=131072, root_data=(0.125, 0.0625))
    b = o.base8.base7.base6.base5.base4.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, o.base8.base7.base6.base5.base4.base3.frames, o.base8.base7.base6.base5.kp_target) == (256, 0.5, 1, 7, 512)
    assert (o.base8.base7.base6.root, o.base8.base7.bone_scale, o.base8.n_views, o.root_anchor, o.lambda_rot, o.lambda_trans, o.mu_rot, o.mu_trans,
            o.reserved5) == (32768, 65536, 3, 131072, 0.375, 0.25, 0.125, 0.0625, 0)
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * 48).from_address(o.base8.views)).reshape(3, 16), table)
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * 35).from_address(o.base8.base7.len_rate)), np.full(35, 0.5, np.float32))
    o = engine.project_options9(lib, None, 0)
    assert (o.base8.base7.base6.base5.base4.base3.base2.base.struct_size, o.root_anchor, o.lambda_rot, o.mu_trans, o.reserved5) == (256, None, 0.0, 0.0, 0)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sr.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "root" in n]
    assert not [h for h in abi.HEADERS if "root" in h]
    assert not [h for h in os.listdir(os.path.join(ge.REPO, "include")) if "root" in h]


# ------------------------------------------------------------------------------------------ 5. the effect
def test_coupling_smooths_the_fitted_depth():
    """On the float64 restatement alone (the one test that passes without the feature): a 15-joint hand on a smooth root path, one camera,
    pixel noise of 1.5 px, 24 frames, 150 steps, the root's translation free and (coupled) lambda_trans = 0.5.  The RMS second difference
    of the fitted depth s_z along the clip is smaller with the coupling; no ratio is fixed.  The figures of this fixture are recorded in
    profiles/skeleton_root/effect.json and DESIGN.md section 2j "Root trajectory"."""
    got = sr.oracle_effect()
    print(json.dumps(got))
    assert all(np.isfinite(v) for v in got.values())
    assert got["rms_coupled"] < got["rms_uncoupled"]
    recorded = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "skeleton_root", "effect.json")
    with open(recorded) as f:
        want = json.load(f)
    for key, value in got.items():
        assert abs(want[key] - value) <= 1e-3 * abs(value), (key, want[key], value)      # the record is this fixture's (float64; 1e-3 leaves room for a BLAS)


# ------------------------------------------------------------------------------------------ 6. the Python layer
def check_model_fit_keypoints(net, run, case, device):
    """fit_keypoints(root_smooth=, root_anchor=, root_data=) equals the raw call, bit for bit; the defaults equal today's call"""
    from posendf_amd.engine import PndfError
    T = 5
    n = sr.P * T
    kp, views, ln, cam = sr.term_inputs(case, "scales", n, T)
    q_np = sk.flat(sdo.clip(case, sr.P, T))
    root_np = si.make_roots(n, 37)
    anchor_np = sr.make_anchor(root_np)
    to = lambda a: torch.from_numpy(np.array(a)).to(device)  # noqa: E731
    q, Y, c, root, anchor = to(q_np), to(kp["Y"]), to(kp["conf"]), to(root_np), to(anchor_np)
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    weights = (si.NU_ROT, si.NU_TRANS)
    common = dict(conf=c, renormalize="unit", frames=T, smooth=0.5, free_ends=True, return_energy=True, root=root, root_weights=weights, return_root=True,
                  bone_scale=to(ln["scale"]), scale_weight=sl.NU_LEN, scale_prior=sl.KAPPA, scale_rates=torch.from_numpy(ln["rate"]), return_scale=True,
                  rho=si.RHO, camera=si.CAMERA, **tables)
    raw = dict(opts=dict(renormalize="unit"), frames=T, lam=0.5, flags=sdo.FREE_ENDS, root=root_np, root_weights=weights, ln=ln, cam=cam, rho=si.RHO)
    for steps in (2, 3):
        want = run.fit9(q_np, steps, kp, root_smooth=(sr.LAM_ROT, sr.LAM_TRANS), root_anchor=anchor_np, root_data=(sr.MU_ROT, sr.MU_TRANS), **raw)
        got = net.fit_keypoints(q, Y, rest, steps=steps, root_smooth=(sr.LAM_ROT, sr.LAM_TRANS), root_anchor=anchor, root_data=(sr.MU_ROT, sr.MU_TRANS), **common)
        for a, b in zip(got, want):
            assert a.device.type == device and a.cpu().numpy().tobytes() == b.tobytes()
    assert root.cpu().numpy().tobytes() == root_np.tobytes() and anchor.cpu().numpy().tobytes() == anchor_np.tobytes()      # the inputs are not written
    today = run.fit8(q_np, 3, kp, **raw)
    got = net.fit_keypoints(q, Y, rest, steps=3, **common)
    for a, b in zip(got, today):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    e = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, camera=si.CAMERA, root_smooth=(0.5, 0.5), **tables)
    assert e[0].shape == (0, q.shape[1], 4)
    for kw in (dict(root_smooth=(0.5,)), dict(root_data=(0.5, 0.5)), dict(root_anchor=anchor[:-1]), dict(root_smooth=(1.5, 0.0)), dict(root_anchor=anchor),
               dict(root_smooth=(0.5, 0.5), frames=None, free_ends=False, bone_scale=None, return_scale=False)):
        args = dict(common)
        args.update(kw)
        with pytest.raises(PndfError):
            net.fit_keypoints(q, Y, rest, steps=1, **args)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_a_root_trajectory_on_cpu(case):
    parents, sd = sko.case_network(case, "lrelu")
    check_model_fit_keypoints(cpu_model(parents, "lrelu", sd), runner_of(case, "lrelu"), case, "cpu")


def check_fit_clip(net, device):
    """KeypointFitting.fit_clip on pixels of one camera: the stated shapes, the roots passed through and moved, scales with fit_lengths"""
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    Pn, T = 2, 4
    clean = net.project(torch.from_numpy(sk.unit_poses(Pn * T, J, 7)).to(device), steps=20, renormalize="unit")[0]
    true_root = torch.from_numpy(si.make_roots(Pn * T, 43, depth=si.EFFECT_DEPTH)).to(device)
    Pk = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    Y = posendf_amd.camera_project(Pk, true_root, camera=si.CAMERA)
    start_root = true_root.clone()
    start_root[:, 4:] += 0.2
    kw = dict(keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo), hypotheses=3, iterations=2, steps_per_iter=5, seed=0, weight=0.1,
              root=start_root, root_weights=(0.0, 0.1), camera=si.CAMERA, clip_steps=7, smooth=0.25, root_smooth=(0.0, 0.5))
    driver = KeypointFitting(net, body_model=None, device=device)
    pose, energy, dist, root = driver.fit_clip(Y, torch.from_numpy(rest), T, **kw)
    assert pose.shape == (Pn * T, J, 4) and energy.shape == (Pn * T,) and dist.shape == (Pn * T,) and root.shape == (Pn * T, 7)
    assert root.device.type == device and bool(torch.isfinite(pose).all()) and bool(torch.isfinite(root).all())
    assert torch.equal(root[:, :4], start_root[:, :4]) and not torch.equal(root[:, 4:], start_root[:, 4:])      # nu_rot = 0: the rotation is passed through
    out = driver.fit_clip(Y, torch.from_numpy(rest), T, fit_lengths=True, **kw)
    assert len(out) == 5 and out[4].shape == (Pn, J + len(kpj)) and bool(torch.isfinite(out[4]).all())
    with pytest.raises(ValueError):
        driver.fit_clip(Y[:-1], torch.from_numpy(rest), T, **kw)
    # the defaults alone are a working call: 3D targets, no camera, no root -- nothing to couple, the identity placement comes back
    small = dict(hypotheses=2, iterations=1, steps_per_iter=3, seed=0, clip_steps=3)
    pose, energy, dist, root = driver.fit_clip(Pk, torch.from_numpy(rest), T, keypoint_joints=kw["keypoint_joints"], keypoint_offsets=kw["keypoint_offsets"], **small)
    identity = torch.zeros(Pn * T, 7, device=root.device)
    identity[:, 0] = 1.0
    assert pose.shape == (Pn * T, J, 4) and torch.equal(root, identity) and bool(torch.isfinite(energy).all())
    # a camera and no root: stage 2 takes the identity placement of stage 1; with a held root (the default weights) it stays, with a free
    # translation the default root_smooth couples it
    tables = dict(keypoint_joints=kw["keypoint_joints"], keypoint_offsets=kw["keypoint_offsets"])
    held = driver.fit_clip(Y, torch.from_numpy(rest), T, camera=si.CAMERA, **tables, **small)
    assert torch.equal(held[3], identity)
    held = driver.fit_clip(Y, torch.from_numpy(rest), T, camera=si.CAMERA, root=start_root, **tables, **small)
    assert torch.equal(held[3], start_root)      # root= given, root_weights left at (0, 0): the coupling of the held parts is dropped
    free = driver.fit_clip(Y, torch.from_numpy(rest), T, camera=si.CAMERA, root=start_root, root_weights=(0.0, 0.1), **tables, **small)
    assert torch.equal(free[3][:, :4], start_root[:, :4]) and not torch.equal(free[3][:, 4:], start_root[:, 4:])
    uncoupled = driver.fit_clip(Y, torch.from_numpy(rest), T, camera=si.CAMERA, root=start_root, root_weights=(0.0, 0.1), root_smooth=(0.0, 0.0), **tables, **small)
    assert not torch.equal(free[3], uncoupled[3])      # the default root_smooth took part


def test_keypoint_fitting_fit_clip_on_a_hand():
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_fit_clip(cpu_model(parents, "softplus", sd), "cpu")


def test_keypoint_fitting_main_takes_a_clip(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    _, kp, _ = si.case_kp(case, 6, image=True)
    np.savez(tmp_path / "kp.npz", keypoints=kp["Y"], rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo, root=si.make_roots(6, 37), camera=np.array(si.CAMERA))
    pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2",
                         "--iterations", "2", "--steps_per_iter", "3", "--root_weights", "0.0", "0.1",
                         "--clip", "3", "--root_smooth", "0.0", "0.5", "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == (6, len(parents), 4) and np.array_equal(f["pose"], pose.numpy()) and f["root"].shape == (6, 7)
    assert bool(torch.isfinite(energy).all())
    # --clip T alone, on 3D keypoints and on pixels with a root: the defaults are a working call
    np.savez(tmp_path / "kp3.npz", keypoints=np.ascontiguousarray(si.case_kp(case, 6, image=False)[1]["Y"]), rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo)
    for name in ("kp3.npz", "kp.npz"):
        pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / name), "--hypotheses", "2",
                             "--iterations", "1", "--steps_per_iter", "2", "--clip", "3"])
        assert pose.shape == (6, len(parents), 4) and bool(torch.isfinite(energy).all())


def test_project_options8_keeps_its_rates_alive():
    """project_options8 copies the struct project_options7 returns; the rates that struct owns (host memory behind a plain address) must
    live as long as the copy"""
    import gc
    from posendf_amd import engine
    lib = engine.load_library()
    rates = [0.25 + i for i in range(35)]
    o = engine.project_options8(lib, None, 0, len_rate=rates, views=sv.make_views(2))
    gc.collect()
    junk = [(ctypes.c_float * 35)(*([7.0] * 35)) for _ in range(64)]      # (what would land in a freed block of the same size)
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * 35).from_address(o.base7.len_rate)), np.asarray(rates, np.float32)) and junk
