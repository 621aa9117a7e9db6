"""Fitting poses to keypoints seen by several cameras inside the projection step, on the host (pndf_project_options8 of
include/posendf_amd.h, the several-camera term of csrc/pndf_fk.h; DESIGN.md section 2j "Several cameras"): the host twin
pndf_project_ex_cpu with the 224-byte struct against the numpy restatement (tests/skeleton_views_oracle.py).

1. the stated step: K rounds of the twin's own forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last,
   kp_energy, root and bone_scale -- for V = 1, 2, 3 and 8, with and without root, rho, confidences, scales (per track and per pose),
   tracks with free ends, mask and anchor.
2. the restatement itself: its float64 dE/dQ, dE/d(c, s) and dE/dsigma against torch autograd of the written energy, to 1e-9 (the one
   test that passes without the feature).
3. reduction: V = 1 with R = I, t = 0 and the camera's intrinsics is the 208-byte call; n_views = 0 is the 208-byte call; nu = 0 is the
   72-byte call and neither targets nor confidences are read.
4. skips: a view with a zero, negative or NaN confidence is never read; a keypoint behind one camera and seen by another; a keypoint seen
   by no view adds nothing; permuting the views changes the float64 restatement only through the order of the sums.
5. row locality.  6. the effect.  7. the refusals, the ABI, the binding, the other entry points, the Python layer on a cpu model.
Every test but 2 and the view-order check of 4 (both run on the restatement alone) fails on the parent commit, where the 224-byte
struct is refused and ProjectOptions8 does not exist.  Runs without a
GPU; tests/test_skeleton_views_gpu.py holds the HIP unit to the same statements (and has the chunk seam)."""
import ctypes

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
import skeleton_views_oracle as sv
from test_skeleton_completion import cpu_model
from test_skeleton_length import TwinLength

BAD_ARG = sv.BAD_ARG


class TwinViews(sv.ViewsRunner, TwinLength):
    """pndf_project_ex_cpu with the 224-byte struct: every array in host memory"""


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinViews(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", sv.CASES, ids=sko.case_id)
def test_view_steps_are_the_stated_step(case, act):
    sv.check_stated_step(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 2. the restatement
@pytest.mark.parametrize("V", sv.VIEW_COUNTS)
@pytest.mark.parametrize("case", sv.CASES[:5], ids=sko.case_id)
def test_restatement_against_autograd(case, V):
    from posendf_amd import camera_project, forward_kinematics
    n = 8
    views = sv.make_views(V)
    parents, kp = sv.case_kp(case, views, n)
    J, K = len(parents), len(kp["kpj"])
    q = sk.unit_poses(n, J, 3).astype(np.float64) * np.random.RandomState(1).uniform(0.5, 2.0, (n, J, 1))
    conf = np.abs(np.nan_to_num(sv.make_view_conf(K, n, V), nan=0.5)).astype(np.float64)
    root = si.make_roots(n, 37).astype(np.float64)
    sigma = sl.make_scales(n, J + K).astype(np.float64)
    Y = kp["Y"].astype(np.float64)
    for rho in (0.0, si.RHO):
        E, g, gr, h = sv.views_energy_grad(q, parents, kp["rest"], kp["kpj"], kp["kpo"], Y, conf, root, rho, views, sigma)
        qt, rt, st = (torch.tensor(a, requires_grad=True) for a in (q, root, sigma))
        Wk = camera_project(forward_kinematics(qt, parents, torch.tensor(kp["rest"], dtype=torch.float64), kp["kpj"], torch.tensor(kp["kpo"], dtype=torch.float64), st), rt)
        vt = torch.tensor(views, dtype=torch.float64)
        C = torch.einsum("vxy,bky->bvkx", vt[:, 4:13].reshape(V, 3, 3), Wk) + vt[None, :, None, 13:16]
        front = C[..., 2] > 0
        z = torch.where(front, C[..., 2], torch.ones_like(C[..., 2]))
        e = C[..., :2] / z[..., None] - (torch.tensor(Y) - vt[None, :, None, 2:4]) / vt[None, :, None, 0:2]
        ee = e * e
        cost = ee if rho == 0 else np.float64(np.float32(rho)) ** 2 * ee / (ee + np.float64(np.float32(rho)) ** 2)
        sq = torch.where(front, cost.sum(-1), torch.zeros_like(z))
        Et = 0.5 * (torch.tensor(conf) * sq).sum((-1, -2))
        Et.sum().backward()
        scale = max(1.0, float(np.abs(h).max()))
        assert np.abs(E - Et.detach().numpy()).max() < 1e-9 * max(1.0, float(E.max()))
        assert np.abs(g - qt.grad.numpy()).max() < 1e-9 * scale and np.abs(gr - rt.grad.numpy()).max() < 1e-9 * scale
        assert np.abs(h - st.grad.numpy()).max() < 1e-9 * scale and np.abs(h).max() > 0 and np.abs(g).max() > 0


# ------------------------------------------------------------------------------------------ 3. reduction
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_one_identity_view_and_no_view_are_the_pinned_calls(case, act):
    """(on these fixtures no entry differs by the sign of a zero: the count the check returns is asserted to be 0, so the comparison is by
    bytes throughout)"""
    assert sv.check_reductions(runner_of(case, act), case, act) == 0


# ------------------------------------------------------------------------------------------ 4. skips
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", sv.CASES, ids=sko.case_id)
def test_views_that_take_no_part_are_never_read(case, act):
    sv.check_skips(runner_of(case, act), case, act)


@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_keypoint_seen_by_no_view_adds_nothing(case, joint):
    sv.check_unseen_keypoint(runner_of(case, "lrelu"), case, joint)


@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_view_order_matters_only_through_the_sums(case):
    sv.check_view_order(case)


# ------------------------------------------------------------------------------------------ 5. locality
@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose(case, act):
    sv.check_row_locality(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 6. the effect
def test_two_views_make_scale_and_depth_observable():
    parents, sd = sv.effect_inputs()[:2]
    sv.check_effect(TwinViews(parents, "lrelu", sd))


# ------------------------------------------------------------------------------------------ 7. refusals, ABI, Python
def test_refusals_write_nothing():
    sv.check_refusals(runner_of(("hand", True), "lrelu"))


def test_the_other_entry_points_refuse_the_224_byte_struct():
    """every other function with a pndf_project_options parameter: a 224-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is -- the
    21-joint functions that refuse a 208-byte struct refuse this one too.  Here the host twins and the two stateless helpers; the
    persistent engine's entry points are in the GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    views = sv.make_views(2)
    rest, Y, E = np.zeros((21, 3), np.float32), np.full((4, 2, 21, 2), 300.0, np.float32), np.full(4, 7.0, np.float32)
    root = si.make_roots(4, 37)
    b6 = si.c_options6(lib, sk.c_options5(lib, None, Y.ctypes.data, None, E.ctypes.data, rest.ctypes.data, None, None, 21, 0.02), root.ctypes.data,
                       sv.UNREAD_CAMERA, 0.0, 0.0, si.NU_TRANS, si.KP_IMAGE)
    big = sv.c_options8(lib, sl.c_options7(lib, b6), views.ctypes.data, 2)
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
    # the twin that takes it does, on this 21-joint handle too: the SMPL table with the joints as keypoints
    kept = root.copy()
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0, lib.pndf_cpu_last_error(eng.handle)
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and root.tobytes() != kept.tobytes()


def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_views_kernel" in ch.exported_symbols(ge.LIB)
    o8 = abi.ProjectOptions8
    assert ctypes.sizeof(o8) == 224 and engine.ProjectOptions8 is o8 and abi.MAX_VIEWS == 8
    assert (o8.base7.offset, o8.views.offset, o8.n_views.offset, o8.reserved4.offset) == (0, 208, 216, 220)
    lib = engine.load_library()
    table = sv.make_views(3)
    o = engine.project_options8(lib, 64, 7, smooth=0.25, kp_target_ptr=512, rest_ptr=4096, n_keypoints=20, kp_weight=0.02, step_size=0.5, renorm="unit",
                                root_ptr=32768, root_weights=(0.25, 0.5), rho=0.125, bone_scale_ptr=65536, len_weight=0.75, views=table)
    b = o.base7.base6.base5.base4.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, o.base7.base6.base5.base4.base3.frames, o.base7.base6.base5.kp_target, o.base7.base6.base5.n_keypoints) == (224, 0.5, 1, 7, 512, 20)
    assert (o.base7.base6.root, o.base7.base6.rho, o.base7.base6.kp_flags, o.base7.bone_scale, o.base7.nu_len, o.n_views, o.reserved4) == (32768, 0.125, 1, 65536, 0.75, 3, 0)
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * 48).from_address(o.views)).reshape(3, 16), table)
    o = engine.project_options8(lib, None, 0)
    assert (o.base7.base6.base5.base4.base3.base2.base.struct_size, o.views, o.n_views, o.reserved4, o.base7.base6.kp_flags) == (224, None, 0, 0, 0)
    # a sequence of (K, R, t) with K a matrix or (fx, fy, cx, cy) is the same table
    seq = [((np.array([[r[0], 0, r[2]], [0, r[1], r[3]], [0, 0, 1]]) if i % 2 else tuple(r[:4])), r[4:13].reshape(3, 3), r[13:]) for i, r in enumerate(table)]
    assert np.array_equal(engine.view_table(seq), table) and np.array_equal(engine.view_table(torch.from_numpy(table)), table)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sv.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "view" in n]
    assert not [h for h in abi.HEADERS if "view" in h]


def test_camera_project_with_views():
    from posendf_amd import camera_project, forward_kinematics
    from posendf_amd.engine import PndfError
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    rest, kpj, kpo = sk.tables(parents)
    views = sv.make_views(3)
    q = torch.from_numpy(sk.unit_poses(12, J, 3)).double()
    root = torch.from_numpy(si.make_roots(12, 37)).double()
    Pk = forward_kinematics(q, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    pix = camera_project(Pk, root, views=views)
    want, _ = sv.project(camera_project(Pk, root).numpy(), views)
    assert pix.shape == (12, 3, len(kpj), 2) and np.abs(pix.numpy() - want).max() < 1e-9
    one = camera_project(Pk, root, views=sv.identity_view())
    assert np.abs(one[:, 0].numpy() - camera_project(Pk, root, camera=si.CAMERA).numpy()).max() < 1e-9
    with pytest.raises(PndfError):
        camera_project(Pk, root, camera=si.CAMERA, views=views)


def check_model_fit_keypoints(net, run, case, device):
    """fit_keypoints(views=) equals the raw call, bit for bit, from a [V,16] table and from a sequence of (K, R, t); conf broadcasts;
    camera= together with views= is an error"""
    from posendf_amd.engine import PndfError
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    V = 3
    views = sv.make_views(V)
    _, kp = sv.case_kp(case, views, conf=True)
    K = len(kp["kpj"])
    S = J + K
    q_np = sk.flat(sdo.clip(case, sv.P, sv.T))
    root_np = si.make_roots(sv.B, 37)
    start = sl.make_scales(sv.P, S)
    to = lambda a: torch.from_numpy(np.array(a)).to(device)  # noqa: E731
    q, Y, c, root = to(q_np), to(kp["Y"]), to(kp["conf"]), to(root_np)
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    weights = (si.NU_ROT, si.NU_TRANS)
    want = run.fit8(q_np, sv.K_STEPS, kp, views=views, rho=si.RHO, opts=dict(renormalize="unit"), frames=sv.T, lam=0.5, flags=sdo.FREE_ENDS, root=root_np,
                    root_weights=weights, ln=sl.lengths(start, sl.NU_LEN, sl.KAPPA))
    seq = [(tuple(r[:4]), r[4:13].reshape(3, 3), r[13:]) for r in views]
    for given in (views, seq, torch.from_numpy(views)):
        got = net.fit_keypoints(q, Y, rest, steps=sv.K_STEPS, conf=c, renormalize="unit", frames=sv.T, smooth=0.5, free_ends=True, return_energy=True,
                                root=root, root_weights=weights, return_root=True, bone_scale=to(start), scale_weight=sl.NU_LEN, scale_prior=sl.KAPPA,
                                return_scale=True, rho=si.RHO, views=given, **tables)
        for a, b in zip(got, want):
            assert a.device.type == device and a.cpu().numpy().tobytes() == b.tobytes()
    assert root.cpu().numpy().tobytes() == root_np.tobytes() and Y.cpu().numpy().tobytes() == kp["Y"].tobytes()      # the inputs are not written
    ones = np.ones((sv.B, V, K), np.float32)
    full = dict(kp, Y=np.nan_to_num(kp["Y"], nan=300.0))
    a = net.fit_keypoints(q, to(full["Y"]), rest, steps=2, conf=torch.ones(K), views=views, root=root, **tables)
    b = net.fit_keypoints(q, to(full["Y"]), rest, steps=2, conf=to(ones), views=views, root=root, **tables)
    c2 = net.fit_keypoints(q, to(full["Y"]), rest, steps=2, conf=torch.ones(V, K), views=views, root=root, **tables)
    d = net.fit_keypoints(q, to(full["Y"]), rest, steps=2, views=views, root=root, **tables)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, c2)) and all(torch.equal(x, y) for x, y in zip(a, d))
    e = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, views=views, **tables)
    assert e[0].shape == (0, J, 4)
    for kw in (dict(camera=si.CAMERA), dict(views=np.zeros((0, 16), np.float32)), dict(views=sv.make_views(8)[:, :15]), dict(views=np.tile(views, (3, 1))),
               dict(conf=torch.ones(sv.B, K)), dict(views=np.where(np.arange(16) == 0, -1.0, views).astype(np.float32))):
        args = dict(views=views, conf=c)
        args.update(kw)
        with pytest.raises(PndfError):
            net.fit_keypoints(q, Y, rest, steps=1, root=root, **args, **tables)
    with pytest.raises(PndfError):
        net.fit_keypoints(q, Y[:, 0], rest, steps=1, views=views, **tables)


@pytest.mark.parametrize("act", sv.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_views_on_cpu(case, act):
    parents, sd = sko.case_network(case, act)
    check_model_fit_keypoints(cpu_model(parents, act, sd), runner_of(case, act), case, "cpu")


def check_driver(net, device):
    """KeypointFitting.fit(views=) on pixels of two cameras: the root of the chosen hypothesis comes back moved, and the energy it reports
    is keypoint_energy(views=) of the pose and the root it returns"""
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting, keypoint_energy
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    views = sv.effect_views()
    clean = net.project(torch.from_numpy(sk.unit_poses(6, J, 7)).to(device), steps=20, renormalize="unit")[0]
    true_root = torch.from_numpy(si.make_roots(6, 43, depth=si.EFFECT_DEPTH)).to(device)
    Pk = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    Y = posendf_amd.camera_project(Pk, true_root, views=views)
    assert Y.shape == (6, 2, len(kpj), 2)
    start_root = true_root.clone()
    start_root[:, 4:] += 0.2
    driver = KeypointFitting(net, body_model=None, device=device)
    kw = dict(rest=torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo), hypotheses=4, iterations=2,
              steps_per_iter=10, seed=0, weight=0.1, root=start_root, root_weights=(0.0, 0.1))
    pose, energy, dist, start_energy, root = driver.fit(Y, views=views, **kw)
    assert pose.shape == (6, J, 4) and root.shape == (6, 7) and root.device.type == device
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(root).all()) and not torch.equal(root, start_root)
    assert float(energy.median()) < float(start_energy.median())      # (20 untuned steps: no further claim)
    again = keypoint_energy(pose, Y, parents, torch.from_numpy(rest).to(device), None, kpj, torch.from_numpy(kpo).to(device), root, views=views)
    assert torch.allclose(energy, again, rtol=1e-3, atol=1e-7)
    with pytest.raises(ValueError):
        driver.fit(Y, views=views, camera=si.CAMERA, **kw)


def test_keypoint_fitting_driver_takes_views_on_a_hand():
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_driver(cpu_model(parents, "softplus", sd), "cpu")


def test_keypoint_fitting_main_takes_views(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    views = sv.make_views(2)
    _, kp = sv.case_kp(case, views, 5)
    Km = np.zeros((2, 3, 3), np.float32)
    Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = views[:, 0], views[:, 1], views[:, 2], views[:, 3], 1.0
    np.savez(tmp_path / "views.npz", K=Km, R=views[:, 4:13].reshape(2, 3, 3), t=views[:, 13:])
    np.savez(tmp_path / "kp.npz", keypoints=kp["Y"], rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo, root=si.make_roots(5, 37))
    pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2",
                         "--iterations", "2", "--steps_per_iter", "3", "--views", str(tmp_path / "views.npz"), "--root_weights", "0.0", "0.1",
                         "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == (5, len(parents), 4) and np.array_equal(f["pose"], pose.numpy()) and f["root"].shape == (5, 7)
    assert bool(torch.isfinite(energy).all())
