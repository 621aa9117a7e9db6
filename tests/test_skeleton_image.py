"""Fitting other skeletons to 2D keypoints on the host (pndf_project_options6 of include/posendf_amd.h, the camera term of csrc/pndf_fk.h;
DESIGN.md section 2j "Image fitting"): the host twin pndf_project_ex_cpu with the 168-byte struct against the numpy restatement of the
root's placement, both residual kinds, their reverse and the root's step (tests/skeleton_image_oracle.py).

1. the restatement itself: its float64 dE/dQ, dE/dc and dE/ds against torch autograd of forward_kinematics + camera_project, to 1e-9.
2. the stated step: K rounds of the twin's own forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last,
   kp_energy and root -- for every option set, both residual kinds, rho 0 and > 0, with and without a root, root weights, a mask,
   confidences, tracks, free ends and the quaternion anchor.
4. it is the smaller call: the 128-byte call's bytes, the 72-byte call's bytes; a NaN root nobody reads; a root with zero weights.
5. skips: keypoints without confidence, and a keypoint behind the camera, are keypoints left out.
6. locality: a joint without a keypoint in its subtree; bad rows at B = 300 stay in their pose and in their root row.
8. free-running: ten steps with prior, coupling, image term and a free root against the fp64 restatement under the project's gate.
9. the effect: a pose and a root that generate their own pixels are found again -- the energy falls at every step.
10. the refusals, each naming its field and writing nothing; the other entry points keep refusing the larger struct.
11. the struct as a C caller writes it, the binding; `camera_project`, `SkeletonPoseNDF.fit_keypoints(camera=, root=)` and the driver on
    a cpu model.
Every test but the first fails on the parent commit, where the 168-byte struct is refused (or the Python names do not exist).  Runs
without a GPU; tests/test_skeleton_image_gpu.py holds the HIP unit to the same statements (and has 3. and 7.)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko
from conftest import outlier_gate, rel_err_rows
from test_skeleton_completion import cpu_model
from test_skeleton_keypoints import FREE_STEPS, TOL, TwinRunner, rows

BAD_ARG = si.BAD_ARG


class TwinImage(si.ImageRunner, TwinRunner):
    """pndf_project_ex_cpu with the 168-byte struct: every array in host memory"""


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinImage(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("image,rho", [(False, 0.0), (True, 0.0), (True, si.RHO)], ids=["3d", "image", "image-rho"])
@pytest.mark.parametrize("case", si.CASES[:4], ids=sko.case_id)
def test_restatement_against_autograd(case, image, rho):
    from posendf_amd import camera_project, forward_kinematics
    n = 8
    parents, kp, _ = si.case_kp(case, n, image=image)
    J, K = len(parents), len(kp["kpj"])
    q = sk.unit_poses(n, J, 3).astype(np.float64) * np.random.RandomState(1).uniform(0.5, 2.0, (n, J, 1))      # raw quaternions: not unit
    conf = np.abs(np.nan_to_num(sk.make_conf(K, n), nan=0.5)).astype(np.float64)                               # zeros stay
    root = si.make_roots(n, 37).astype(np.float64)
    root[0, 4:] = (0.0, 0.0, -3.0)      # a pose behind its camera: keypoints with C_z <= 0
    root[1, :4] = np.array([1.0, 0.3, -0.2, 0.1]) * 2e-13      # the clamped norm: c^ = c / 1e-12, the map is linear there
    Y = kp["Y"].astype(np.float64)
    cam = si.cam_of(image, rho)
    E, g, gr = si.camera_energy_grad(q, parents, kp["rest"], kp["kpj"], kp["kpo"], Y, conf, root, cam)
    qt, rt = torch.tensor(q, requires_grad=True), torch.tensor(root, requires_grad=True)
    Pk = forward_kinematics(qt, parents, torch.tensor(kp["rest"], dtype=torch.float64), kp["kpj"], torch.tensor(kp["kpo"], dtype=torch.float64))
    C = camera_project(Pk, rt)
    assert np.abs(C.detach().numpy() - si.place(sk.positions(q, parents, kp["rest"], kp["kpj"], kp["kpo"]), root)[0]).max() < 1e-12
    w, Yt = torch.tensor(conf), torch.tensor(Y)
    if image:
        front = C[..., 2] > 0
        assert bool((~front).any()) and bool(front.any())
        fx, fy, cx, cy = si.CAMERA
        pix = camera_project(Pk, rt, si.CAMERA)
        assert np.allclose(pix.detach().numpy()[front.numpy()], si.pixels(C.detach().numpy())[front.numpy()], rtol=1e-12)
        e = torch.stack([(pix[..., 0] - Yt[..., 0]) / fx, (pix[..., 1] - Yt[..., 1]) / fy], dim=-1)
        cost = e * e if rho == 0 else rho ** 2 * e * e / (e * e + rho ** 2)
        per = torch.where(front, cost.sum(-1), torch.zeros_like(cost[..., 0]))
    else:
        per = ((C - Yt) ** 2).sum(-1)
    Et = 0.5 * (w * per).sum(-1)
    gq, groot = torch.autograd.grad(Et.sum(), (qt, rt))
    assert np.abs(E - Et.detach().numpy()).max() <= 1e-9 * np.abs(E).max()
    for mine, theirs, what in ((g, gq.numpy(), "dE/dQ"), (gr[:, :4], groot.numpy()[:, :4], "dE/dc"), (gr[:, 4:], groot.numpy()[:, 4:], "dE/ds")):
        assert np.isfinite(mine).all() and np.abs(theirs).max() > 0, what
        assert np.abs(mine - theirs).max() <= 1e-9 * np.abs(theirs).max(), (what, float(np.abs(mine - theirs).max()), float(np.abs(theirs).max()))
    # float32 is the same code: close to the truth
    E32, g32, gr32 = si.camera_energy_grad(q.astype(np.float32), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], conf.astype(np.float32),
                                           root.astype(np.float32), cam)
    assert E32.dtype == np.float32 and np.abs(g32 - g).max() <= 1e-3 * np.abs(g).max() and np.abs(gr32 - gr).max() <= 1e-3 * np.abs(gr).max()


# ------------------------------------------------------------------------------------------ 2. the stated step
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", si.CASES, ids=sko.case_id)
def test_image_steps_are_the_stated_step(case, act):
    si.check_stated_step(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 4. the smaller calls
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_camera_and_root_it_is_the_smaller_call(case, act):
    si.check_smaller_calls(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 5. skips
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", si.CASES, ids=sko.case_id)
def test_skipped_keypoints_are_keypoints_left_out(case, act):
    si.check_skips(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 6. locality
@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_joint_without_a_keypoint_below_it_is_not_moved(case, joint):
    si.check_subtree_locality(runner_of(case, "lrelu"), case, joint)


@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose_and_root_row(case, act):
    si.check_row_locality(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 8. free running
def free_inputs(case):
    """(the noisy clip [6,7,J,4], kp with pixel targets and confidences, the start roots)"""
    x = sdo.noisy_clip(case)
    n = x.shape[0] * x.shape[1]
    _, kp, _ = si.case_kp(case, n, conf=True)
    return x, kp, si.make_roots(n, 37)


FREE_KW = dict(smooth=sk.LAMBDA, free_ends=True, renormalize="unit")
FREE_WEIGHTS = (si.NU_ROT, si.NU_TRANS)


@functools.lru_cache(maxsize=None)
def oracle_tracks(case, act):
    """(fp64 rows, fp32 rows, kink margins along the fp64 trajectory or None) of the numpy restatement after ten steps: a row is a pose and
    its root"""
    parents, sd = sko.case_network(case, act)
    x, kp, root = free_inputs(case)
    q64, _, _, margin, r64 = si.relax(x, sd, FREE_STEPS, act, parents, kp, si.cam_of(True), root, FREE_WEIGHTS, si.NU, np.float64, **FREE_KW)
    q32, _, _, _, r32 = si.relax(x, sd, FREE_STEPS, act, parents, kp, si.cam_of(True), root, FREE_WEIGHTS, si.NU, np.float32, **FREE_KW)
    return with_root(q64, r64), with_root(q32, r32), (None if act == "softplus" else margin)


def with_root(track, root):
    return np.concatenate([rows(track), np.asarray(root)], axis=1)


def free_gate(got, case, act, what, ref=None):
    """the free_gate of tests/test_skeleton_keypoints.py, applied as it is there, on this feature's oracle rows (pose and root):
    conftest.outlier_gate at 1e-4 on every frame against the fp64 restatement, the float32 restatement's rows (or `ref`'s) as the reference
    rows, after the float32 restatement alone is shown to stay inside the gate's exemption caps"""
    truth, r32, margin = oracle_tracks(case, act)
    own = rel_err_rows(r32, truth)
    assert np.isfinite(own).all() and own.max() < 1.0, (what, float(own.max()))
    outlier_gate(own, own, TOL, f"{what}: the float32 restatement itself", margin=margin)
    mine = rel_err_rows(got, truth)
    base = own if ref is None else rel_err_rows(ref, truth)
    print(f"[{what}] per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference rows median {np.median(base):.2e} max {base.max():.2e}")
    outlier_gate(mine, base, TOL, what, margin=margin)


def free_run(run, case):
    x, kp, root = free_inputs(case)
    got, d, E, rt = run.fit6(sk.flat(x), FREE_STEPS, kp, opts=dict(renormalize="unit"), frames=x.shape[1], lam=sk.LAMBDA, flags=sdo.FREE_ENDS,
                             cam=si.cam_of(True), root=root, root_weights=FREE_WEIGHTS)
    assert np.isfinite(got).all() and np.isfinite(d).all() and np.isfinite(E).all() and np.isfinite(rt).all()
    return with_root(got.reshape(x.shape), rt)


@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(case, act):
    free_gate(free_run(runner_of(case, act), case), case, act, f"twin {sko.case_id(case)} {act}")


# ------------------------------------------------------------------------------------------ 9. the effect
def test_a_pose_and_root_are_found_from_their_own_pixels():
    parents, sd, _, _, _ = si.effect_inputs()
    si.check_effect(TwinImage(parents, "lrelu", sd))


# ------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_write_nothing():
    si.check_refusals(runner_of(("hand", True), "lrelu"))


def test_the_other_entry_points_refuse_the_168_byte_struct():
    """every other function with a pndf_project_options parameter: a 168-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
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
    kept = root.copy()
    big = si.c_options6(lib, sk.c_options5(lib, None, Y.ctypes.data, None, E.ctypes.data, rest.ctypes.data, None, None, 21, 0.02), root.ctypes.data,
                        si.CAMERA, 0.0, si.NU_ROT, si.NU_TRANS, si.KP_IMAGE)
    out, d = np.full_like(q, 7.0), np.full(8, 7.0, np.float32)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    track = np.full((2, 2, 21, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q[2:].ctypes.data, None, track.ctypes.data, d.ctypes.data, 2, 2, 0, 1, 0.0, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_complete_step(out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 4, ref, None) == BAD_ARG
    assert lib.pndf_interp_band_step(q.ctypes.data, out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 2, 2, 0.0, ref, None) == BAD_ARG
    assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(track == 7.0) and np.all(E == 7.0) and root.tobytes() == kept.tobytes()
    # the twin that takes it does, on this 21-joint handle too: the SMPL table with the joints as keypoints
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and root.tobytes() != kept.tobytes()


# ------------------------------------------------------------------------------------------ 11. the library, the ABI, Python
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_image_kernel" in ch.exported_symbols(ge.LIB)
    o6 = abi.ProjectOptions6
    assert ctypes.sizeof(o6) == 168 and engine.ProjectOptions6 is o6 and abi.KP_IMAGE == 1
    assert (o6.base5.offset, o6.root.offset, o6.fx.offset, o6.fy.offset, o6.cx.offset, o6.cy.offset, o6.rho.offset, o6.nu_rot.offset, o6.nu_trans.offset,
            o6.kp_flags.offset) == (0, 128, 136, 140, 144, 148, 152, 156, 160, 164)
    lib = engine.load_library()
    o = engine.project_options6(lib, 64, 7, smooth=0.25, kp_target_ptr=512, rest_ptr=4096, n_keypoints=20, kp_weight=0.02, step_size=0.5, renorm="unit",
                                root_ptr=32768, root_weights=(0.25, 0.5), camera=(500.0, 480.0, 320.0, 240.0), rho=0.125)
    b = o.base5.base4.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, o.base5.base4.base3.frames, o.base5.kp_target, o.base5.rest, o.base5.n_keypoints) == (168, 0.5, 1, 7, 512, 4096, 20)
    assert (o.root, o.fx, o.fy, o.cx, o.cy, o.rho, o.nu_rot, o.nu_trans, o.kp_flags) == (32768, 500.0, 480.0, 320.0, 240.0, 0.125, 0.25, 0.5, 1)
    o = engine.project_options6(lib, None, 0)
    assert (o.base5.base4.base3.base2.base.struct_size, o.root, o.kp_flags, o.nu_rot, o.nu_trans, o.rho) == (168, None, 0, 0.0, 0.0, 0.0)
    assert engine.project_options6(lib, None, 0, root_ptr=8, camera=(1, 1, 0, 0), image=False).kp_flags == 0
    ok, diagnostics = ch.compiles_as_c99(tmp_path, si.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "skel" in n and ("image" in n or "camera" in n)]
    assert not [h for h in abi.HEADERS if "skel" in h and ("image" in h or "camera" in h)]


def test_camera_project():
    from posendf_amd import camera_project
    from posendf_amd.engine import PndfError
    pts = torch.tensor(np.random.RandomState(0).uniform(-1, 1, (5, 4, 3)))
    assert camera_project(pts) is pts
    ident = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64)
    assert torch.equal(camera_project(pts, ident), pts)
    shift = torch.tensor([2.0, 0, 0, 0, 0.5, -0.5, 4.0], dtype=torch.float64)      # a non-unit quaternion is normalised
    assert torch.allclose(camera_project(pts, shift), pts + shift[4:])
    quarter = torch.tensor([np.sqrt(0.5), 0, 0, np.sqrt(0.5), 0, 0, 0], dtype=torch.float64)      # 90 degrees about z: x -> y
    turned = camera_project(pts, quarter)
    assert torch.allclose(turned[..., 0], -pts[..., 1]) and torch.allclose(turned[..., 1], pts[..., 0]) and torch.allclose(turned[..., 2], pts[..., 2])
    per_pose = torch.tensor(si.make_roots(5, 3), dtype=torch.float64)
    C = camera_project(pts, per_pose)
    assert np.abs(C.numpy() - si.place(pts.numpy(), per_pose.numpy())[0]).max() < 1e-12
    pix = camera_project(pts, per_pose, si.CAMERA)
    assert pix.shape == (5, 4, 2) and np.allclose(pix.numpy(), si.pixels(C.numpy()))
    with pytest.raises(PndfError):
        camera_project(pts[..., :2])
    with pytest.raises(PndfError):
        camera_project(pts, per_pose[:, :6])


@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_a_camera_on_cpu(case, act):
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cpu_model(parents, act, sd)
    run = TwinImage(parents, act, sd)
    _, kp, _ = si.case_kp(case, conf=True)
    K = len(kp["kpj"])
    track = sdo.clip(case, si.P, si.T)
    q_np = sk.flat(track)
    root_np = si.make_roots(si.B, 37)
    q, Y, c, root = torch.from_numpy(q_np.copy()), torch.from_numpy(kp["Y"]), torch.from_numpy(kp["conf"]), torch.from_numpy(root_np.copy())
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    weights = (si.NU_ROT, si.NU_TRANS)
    want, d_want, E_want, r_want = run.fit6(q_np, si.K_STEPS, kp, opts=dict(renormalize="unit"), nu=0.05, cam=si.cam_of(True, si.RHO), root=root_np, root_weights=weights)
    out, d, E, rt = net.fit_keypoints(q, Y, rest, steps=si.K_STEPS, weight=0.05, conf=c, renormalize="unit", return_energy=True, camera=si.CAMERA, rho=si.RHO,
                                      root=root, root_weights=weights, return_root=True, **tables)
    assert out.shape == (si.B, J, 4) and d.shape == (si.B, 1) and E.shape == (si.B,) and rt.shape == (si.B, 7)
    assert out.numpy().tobytes() == want.tobytes() and d.numpy().tobytes() == d_want.tobytes() and E.numpy().tobytes() == E_want.tobytes()
    assert rt.numpy().tobytes() == r_want.tobytes() and rt.numpy().tobytes() != root_np.tobytes()
    assert q.numpy().tobytes() == q_np.tobytes() and root.numpy().tobytes() == root_np.tobytes()      # the inputs are not written
    # a root [7] is the same root for every pose; 3D targets with a root; tracks, a mask and the anchor ride along
    one = root[3]
    a = net.fit_keypoints(q, Y, rest, steps=2, conf=c, camera=si.CAMERA, root=one, root_weights=weights, return_root=True, **tables)
    b = net.fit_keypoints(q, Y, rest, steps=2, conf=c, camera=si.CAMERA, root=one.expand(si.B, 7), root_weights=weights, return_root=True, **tables)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and one.numpy().tobytes() == root_np[3].tobytes()
    _, kp3, _ = si.case_kp(case, image=False, conf=True)
    mask = sdo.make_mask(J, si.P, si.T)
    want, _, E_want, r_want = run.fit6(q_np, si.K_STEPS, kp3, words=sk.pack(mask), frames=si.T, lam=0.5, flags=sdo.FREE_ENDS, anchor=q_np, mu=0.25,
                                       cam=si.cam_of(False), root=root_np, root_weights=weights)
    out, E, rt = net.fit_keypoints(q, torch.from_numpy(kp3["Y"]), rest, steps=si.K_STEPS, conf=c, observed=torch.from_numpy(mask.reshape(-1, J)), frames=si.T,
                                   smooth=0.5, anchor=q, data=0.25, free_ends=True, return_dist=False, return_energy=True, root=root, root_weights=weights,
                                   return_root=True, **tables)
    assert out.numpy().tobytes() == want.tobytes() and E.numpy().tobytes() == E_want.tobytes() and rt.numpy().tobytes() == r_want.tobytes()
    # the defaults reproduce the call without a camera; return_root without a root is the identity placement
    Yc = torch.from_numpy(sk.targets(parents))
    a = net.fit_keypoints(q, Yc, rest, steps=2, **tables)
    b = net.fit_keypoints(q, Yc, rest, steps=2, return_root=True, **tables)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[2], torch.tensor([1.0, 0, 0, 0, 0, 0, 0]).expand(si.B, 7))
    # steps = 0 and the empty batch
    s, ds, Es, rs = net.fit_keypoints(q, Y, rest, steps=0, return_energy=True, camera=si.CAMERA, root=root, root_weights=weights, return_root=True, **tables)
    assert torch.equal(s, q) and not bool(ds.any()) and not bool(Es.any()) and torch.equal(rs, root)
    e, de, re = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, camera=si.CAMERA, root=root[:0], root_weights=weights, return_root=True, **tables)
    assert e.shape == (0, J, 4) and de.shape == (0, 1) and re.shape == (0, 7)
    # the energy it returns is the energy of forward_kinematics + camera_project at the input of the last step
    from posendf_amd import camera_project, forward_kinematics
    cc = c.abs().nan_to_num(0.5)
    Yf = torch.from_numpy(si.case_kp(case)[1]["Y"])
    _, E1 = net.fit_keypoints(q, Yf, rest, steps=1, conf=cc, return_dist=False, return_energy=True, camera=si.CAMERA, root=root, **tables)
    Pk = forward_kinematics(q.double(), parents, rest.double(), kp["kpj"], torch.from_numpy(kp["kpo"]).double())
    C = camera_project(Pk, root.double())
    pix = camera_project(Pk, root.double(), si.CAMERA)
    e = (pix - Yf.double()) / torch.tensor(si.CAMERA[:2], dtype=torch.float64)
    E_ref = 0.5 * (cc.double() * torch.where(C[..., 2] > 0, (e * e).sum(-1), torch.zeros(si.B, K, dtype=torch.float64))).sum(-1)
    assert torch.allclose(E1.double(), E_ref, rtol=1e-4)
    # wrong shapes and values
    for kw in (dict(targets=Y[:, :, :1]), dict(root=root[:-1]), dict(root=root[:, :6]), dict(root=torch.zeros(si.B, 7, dtype=torch.int64)), dict(camera=(1.0, 1.0, 0.0)),
               dict(camera=(0.0, 1.0, 0.0, 0.0)), dict(rho=-1.0), dict(root_weights=(-1.0, 0.0)), dict(root_weights=(0.1,)), dict(root=None, root_weights=(0.1, 0.0))):
        args = dict(targets=Y, rest=rest, conf=None, camera=si.CAMERA, root=root, root_weights=weights, **tables)
        args.update(kw)
        with pytest.raises(PndfError):
            net.fit_keypoints(q, steps=1, **args)
    with pytest.raises(PndfError):      # rho without a camera
        net.fit_keypoints(q, Yc, rest, steps=1, rho=0.5, **tables)


def test_keypoint_fitting_driver_with_a_camera_on_a_hand():
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cpu_model(parents, "softplus", sd)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    clean = net.project(torch.from_numpy(sk.unit_poses(12, J, 7)), steps=20, renormalize="unit")[0]
    truth_root = torch.from_numpy(si.make_roots(12, 43, depth=si.EFFECT_DEPTH))
    Pk = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    Y = posendf_amd.camera_project(Pk, truth_root, si.CAMERA)
    start_root = truth_root.clone()
    start_root[:, 4:] += 0.3 * torch.from_numpy(np.random.RandomState(3).randn(12, 3).astype(np.float32))
    driver = KeypointFitting(net, body_model=None, device="cpu")
    kw = dict(rest=torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo), camera=si.CAMERA, root=start_root,
              root_weights=si.EFFECT_ROOT_WEIGHTS, weight=si.EFFECT_NU)
    pose, energy, dist, start_energy, root = driver.fit(Y, hypotheses=4, iterations=3, steps_per_iter=10, seed=0, **kw)
    assert pose.shape == (12, J, 4) and energy.shape == (12,) and dist.shape == (12,) and start_energy.shape == (12, 4) and root.shape == (12, 7)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(energy).all()) and bool(torch.isfinite(root).all())
    assert float(energy.median()) < float(start_energy.median()), (float(energy.median()), float(start_energy.median()))
    # the energy it reports is the energy of the pose and the root it returns
    pix = posendf_amd.camera_project(posendf_amd.forward_kinematics(pose, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo)), root, si.CAMERA)
    e = (pix - Y) / torch.tensor(si.CAMERA[:2])
    assert torch.allclose(energy, 0.5 * (e * e).sum((-1, -2)), rtol=1e-3, atol=1e-7)
    again = driver.fit(Y, hypotheses=4, iterations=3, steps_per_iter=10, seed=0, **kw)
    assert torch.equal(again[0], pose) and torch.equal(again[4], root)
    assert start_root.numpy().tobytes() != root.numpy().tobytes()


def test_keypoint_fitting_main_takes_a_camera(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    _, kp, _ = si.case_kp(case, 5)
    root = si.make_roots(5, 37)
    np.savez(tmp_path / "kp.npz", keypoints=kp["Y"], rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo, camera=np.asarray(si.CAMERA, np.float32), root=root)
    pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2",
                         "--iterations", "2", "--steps_per_iter", "3", "--root_weights", "0.05", "0.3", "--rho", "0.5", "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == (5, len(parents), 4) and f["energy"].shape == (5,) and np.array_equal(f["pose"], pose.numpy())
        assert f["root"].shape == (5, 7) and not np.array_equal(f["root"], root)
