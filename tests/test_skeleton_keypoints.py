"""3D keypoint fitting for other skeletons on the host (pndf_project_options5 of include/posendf_amd.h, csrc/pndf_fk.h; DESIGN.md section 2j
"Keypoint fitting"): the host twin pndf_project_ex_cpu with the 128-byte struct against the numpy restatement of the kinematics, their
reverse and the fitting step (tests/skeleton_keypoints_oracle.py).

0. the restatement itself: its float64 gradient against torch autograd of posendf_amd.skeleton.forward_kinematics, to 1e-10.
1. the stated step: K rounds of the twin's own forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last and
   kp_energy -- for every option set, with and without a mask, confidences, tracks, free ends and the quaternion anchor.
2. it is the smaller call: kp_target NULL, and nu == 0 with NaN targets, give the bytes of the 72-byte call.
3. confidences: keypoints without confidence and with NaN targets equal the call without them in the tables.
4. locality: a joint without a keypoint in its subtree; a NaN target, a NaN pose and an overflow stay in their own pose.
5. free-running: ten steps with prior, coupling and keypoint term against the fp64 oracle under the project's gate.
6. the effect: pure inverse kinematics on a hand lowers the energy at every step, in the fp64 oracle first.
7. the refusals, each naming its field and writing nothing; the other entry points keep refusing the larger struct.
8. the struct as a C caller writes it, the binding, no new entry point.
9. `forward_kinematics`, `SkeletonPoseNDF.fit_keypoints` and `KeypointFitting` on a cpu model.
Every test fails on the parent commit, where the 128-byte struct is refused (or the Python names do not exist).  Runs without a GPU;
tests/test_skeleton_keypoints_gpu.py holds the HIP unit to the same statements."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_denoise_oracle as sdo
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko
from conftest import outlier_gate, rel_err_rows
from test_skeleton_completion import Twin, cpu_model

BAD_ARG = sk.BAD_ARG
TOL = 1e-4             # the gate of tests/test_skeleton_denoise_gpu.py's free_gate
FREE_STEPS = 10


class TwinRunner(sk.Runner):
    """pndf_project_ex_cpu: every array in host memory"""

    def __init__(self, parents, act, sd, encoder=True):
        self.twin = Twin(parents, act, sd, encoder=encoder)
        self.lib, self.forward, self.forward_grad = self.twin.lib, self.twin.forward, self.twin.forward_grad

    def place(self, a):
        return np.array(a, order="C")

    def addr(self, holder):
        return holder.ctypes.data

    def fetch(self, holder):
        return holder

    def project(self, q, out, d, n, steps, opt):
        return self.lib.pndf_project_ex_cpu(self.twin.h, q, out, d, n, steps, ctypes.byref(opt))

    def last_error(self):
        return self.lib.pndf_cpu_last_error(self.twin.h)


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinRunner(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 0. the restatement
@pytest.mark.parametrize("case", sk.CASES[:4], ids=sko.case_id)
def test_restatement_against_autograd(case):
    from posendf_amd import forward_kinematics
    parents, kp = sk.case_kp(case, 8)
    J = len(parents)
    q = sk.unit_poses(8, J, 3).astype(np.float64) * np.random.RandomState(1).uniform(0.5, 2.0, (8, J, 1))      # raw quaternions: not unit
    conf = np.abs(np.nan_to_num(sk.make_conf(len(kp["kpj"]), 8), nan=0.5)).astype(np.float64)                  # zeros stay
    Y = kp["Y"].astype(np.float64)
    E, g = sk.energy_grad(q, parents, kp["rest"], kp["kpj"], kp["kpo"], Y, conf)
    qt = torch.tensor(q, requires_grad=True)
    Pk = forward_kinematics(qt, parents, torch.tensor(kp["rest"], dtype=torch.float64), kp["kpj"], torch.tensor(kp["kpo"], dtype=torch.float64))
    assert Pk.shape == (8, len(kp["kpj"]), 3)
    assert np.abs(Pk.detach().numpy() - sk.positions(q, parents, kp["rest"], kp["kpj"], kp["kpo"])).max() < 1e-12
    Et = 0.5 * (torch.tensor(conf) * ((Pk - torch.tensor(Y)) ** 2).sum(-1)).sum(-1)
    (gt,) = torch.autograd.grad(Et.sum(), qt)
    assert np.abs(E - Et.detach().numpy()).max() <= 1e-10 * np.abs(E).max()
    assert np.abs(g - gt.numpy()).max() <= 1e-10 * np.abs(gt.numpy()).max()
    # the clamped norm: a zero quaternion is r = 0 and the map is linear there (autograd of clamp_min agrees)
    q0 = q.copy()
    q0[:, J - 1] = 0.0
    _, g0 = sk.energy_grad(q0, parents, kp["rest"], kp["kpj"], kp["kpo"], Y, conf)
    assert np.isfinite(g0).all()
    # float32 is the same code: close to the truth
    E32, g32 = sk.energy_grad(q.astype(np.float32), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], conf.astype(np.float32))
    assert E32.dtype == np.float32 and np.abs(g32 - g).max() <= 1e-4 * np.abs(g).max()


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", sk.CASES, ids=sko.case_id)
def test_fitting_steps_are_the_stated_step(case, act):
    sk.check_stated_step(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 2. the smaller call
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_keypoints_it_is_the_smaller_call(case, act):
    sk.check_smaller_call(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 3. confidences
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", sk.CASES, ids=sko.case_id)
def test_keypoints_without_confidence_are_keypoints_left_out(case, act):
    sk.check_confidences(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 4. locality
@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_joint_without_a_keypoint_below_it_is_not_moved(case, joint):
    sk.check_subtree_locality(runner_of(case, "lrelu"), case, joint)


@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose(case, act):
    sk.check_row_locality(runner_of(case, act), case, act)


# ------------------------------------------------------------------------------------------ 5. free running
def free_inputs(case):
    """(the noisy clip [6,7,J,4], kp with confidences): prior, coupling with free ends and keypoint term"""
    x = sdo.noisy_clip(case)
    _, kp = sk.case_kp(case, x.shape[0] * x.shape[1], conf=True)
    return x, kp


@functools.lru_cache(maxsize=None)
def oracle_tracks(case, act):
    """(fp64 track, fp32 track, kink margins along the fp64 trajectory or None) of the numpy oracle: ten fitting steps"""
    parents, sd = sko.case_network(case, act)
    x, kp = free_inputs(case)
    kw = dict(smooth=sk.LAMBDA, free_ends=True, renormalize="unit")
    q64, _, _, margin = sk.relax(x, sd, FREE_STEPS, act, parents, kp, sk.NU, np.float64, **kw)
    q32, _, _, _ = sk.relax(x, sd, FREE_STEPS, act, parents, kp, sk.NU, np.float32, **kw)
    return q64, q32, (None if act == "softplus" else margin)


def rows(track):
    t = np.asarray(track)
    return t.reshape(t.shape[0] * t.shape[1], -1)


def free_gate(got, case, act, what, ref=None):
    """the free_gate of tests/test_skeleton_denoise_gpu.py, applied as it is there, on this feature's oracle tracks: conftest.outlier_gate
    at 1e-4 on every frame against the fp64 oracle track, the float32 numpy oracle's rows (or `ref`'s) as the reference rows, after the
    float32 oracle alone is shown to stay inside the gate's exemption caps"""
    q64, q32, margin = oracle_tracks(case, act)
    truth = rows(q64)
    own = rel_err_rows(rows(q32), truth)
    assert np.isfinite(own).all() and own.max() < 1.0, (what, float(own.max()))
    outlier_gate(own, own, TOL, f"{what}: the float32 oracle itself", margin=margin)
    mine = rel_err_rows(rows(got), truth)
    base = own if ref is None else rel_err_rows(rows(ref), truth)
    print(f"[{what}] per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference rows median {np.median(base):.2e} max {base.max():.2e}")
    outlier_gate(mine, base, TOL, what, margin=margin)


def free_run(run, case):
    x, kp = free_inputs(case)
    got, d, E = run.fit(sk.flat(x), FREE_STEPS, opts=dict(renormalize="unit"), frames=x.shape[1], lam=sk.LAMBDA, flags=sdo.FREE_ENDS, kp=kp)
    assert np.isfinite(got).all() and np.isfinite(d).all() and np.isfinite(E).all()
    return got.reshape(x.shape)


@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(case, act):
    free_gate(free_run(runner_of(case, act), case), case, act, f"twin {sko.case_id(case)} {act}")


# ------------------------------------------------------------------------------------------ 6. the effect
def test_inverse_kinematics_lowers_the_energy_at_every_step():
    parents, sd, _, _ = sk.effect_inputs()
    sk.check_effect(TwinRunner(parents, "lrelu", sd))
    # recorded, not asserted: with rest offsets in [-1, 1]^3 the fp64 oracle itself does not fall at every step at nu = 0.02 (the reason the
    # check above runs on the shorter bones, and what the default weight of fit_keypoints does not cover)
    rises, poses, worst = sk.oracle_effect_at_full_reach()
    print(f"[effect, rest offsets in [-1, 1]^3] fp64 oracle: {rises} of {49 * sk.B} steps do not fall, poses {poses}, worst E_last / E_0 {worst:.4f}")


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing():
    sk.check_refusals(runner_of(("hand", True), "lrelu"))


def test_the_other_entry_points_refuse_the_128_byte_struct():
    """every other function with a pndf_project_options parameter: a 128-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers; pndf_project_ex, pndf_complete and pndf_interpolate need a device handle and are in the GPU
    file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    rest, Y, E = np.zeros((21, 3), np.float32), np.zeros((4, 21, 3), np.float32), np.full(4, 7.0, np.float32)
    big = sk.c_options5(lib, None, Y.ctypes.data, None, E.ctypes.data, rest.ctypes.data, None, None, 21, 0.02)
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
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0
    assert not np.any(out == 7.0) and not np.any(E == 7.0)


# ------------------------------------------------------------------------------------------ 8. the library and the ABI
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_fit_kernel" in ch.exported_symbols(ge.LIB)
    o5 = abi.ProjectOptions5
    assert ctypes.sizeof(o5) == 128 and engine.ProjectOptions5 is o5
    assert (o5.base4.offset, o5.kp_target.offset, o5.kp_conf.offset, o5.kp_energy.offset, o5.rest.offset, o5.kp_joint.offset, o5.kp_offset.offset,
            o5.n_keypoints.offset, o5.nu.offset) == (0, 72, 80, 88, 96, 104, 112, 120, 124)
    lib = engine.load_library()
    o = engine.project_options5(lib, 64, 7, smooth=0.25, anchor_ptr=128, conf_ptr=256, data=0.5, free_ends=True, kp_target_ptr=512, kp_conf_ptr=1024,
                                kp_energy_ptr=2048, rest_ptr=4096, kp_joint_ptr=8192, kp_offset_ptr=16384, n_keypoints=20, kp_weight=0.02,
                                step_size=0.5, renorm="unit", tol=0.25)
    b = o.base4.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, b.tol, o.base4.base3.base2.observed, o.base4.base3.frames, o.base4.base3.lambda_) == (128, 0.5, 1, 0.25, 64, 7, 0.25)
    assert (o.base4.anchor, o.base4.conf, o.base4.mu, o.base4.flags) == (128, 256, 0.5, 1)
    assert (o.kp_target, o.kp_conf, o.kp_energy, o.rest, o.kp_joint, o.kp_offset, o.n_keypoints) == (512, 1024, 2048, 4096, 8192, 16384, 20)
    assert o.nu == np.float32(0.02)
    o = engine.project_options5(lib, None, 0)
    assert (o.base4.base3.base2.base.struct_size, o.kp_target, o.rest, o.n_keypoints, o.nu) == (128, None, None, 0, 0.0)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sk.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "skel" in n and ("keypoint" in n or "fit" in n)]
    assert not hasattr(lib, "pndf_skel_fit") and not hasattr(lib, "pndf_skel_keypoints")
    assert not [h for h in abi.HEADERS if "skel" in h and ("keypoint" in h or "fit" in h)]


# ------------------------------------------------------------------------------------------ 9. Python
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_on_cpu(case, act):
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cpu_model(parents, act, sd)
    run = TwinRunner(parents, act, sd)
    _, kp = sk.case_kp(case, conf=True)
    K = len(kp["kpj"])
    track = sdo.clip(case, sk.P, sk.T)
    q_np = sk.flat(track)
    mask = sdo.make_mask(J, sk.P, sk.T)
    q, Y, c = torch.from_numpy(q_np.copy()), torch.from_numpy(kp["Y"]), torch.from_numpy(kp["conf"])
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    # the twin's bits through the C struct: without tracks, then a clip with free ends, a mask and the quaternion anchor
    want, d_want, E_want = run.fit(q_np, sk.K_STEPS, opts=dict(renormalize="unit"), kp=kp, nu=0.05)
    out, d, E = net.fit_keypoints(q, Y, rest, steps=sk.K_STEPS, weight=0.05, conf=c, renormalize="unit", return_energy=True, **tables)
    assert out.shape == (sk.B, J, 4) and d.shape == (sk.B, 1) and E.shape == (sk.B,)
    assert out.numpy().tobytes() == want.tobytes() and d.numpy().tobytes() == d_want.tobytes() and E.numpy().tobytes() == E_want.tobytes()
    assert q.numpy().tobytes() == q_np.tobytes()      # the input is not written
    want, d_want, E_want = run.fit(q_np, sk.K_STEPS, words=sk.pack(mask), frames=sk.T, lam=0.5, flags=sdo.FREE_ENDS, anchor=q_np, mu=0.25, kp=kp)
    out, E = net.fit_keypoints(q.reshape(sk.P, sk.T, J, 4), Y, rest, steps=sk.K_STEPS, conf=c, observed=torch.from_numpy(mask.reshape(-1, J)), frames=sk.T,
                               smooth=0.5, anchor=q, data=0.25, free_ends=True, return_dist=False, return_energy=True, **tables)
    assert out.numpy().tobytes() == want.tobytes() and E.numpy().tobytes() == E_want.tobytes()
    assert torch.equal(out[torch.from_numpy(mask.reshape(-1, J))].view(torch.int32), q[torch.from_numpy(mask.reshape(-1, J))].view(torch.int32))
    # the defaults of the tables: keypoint k is joint k; conf [K] is the same confidence for every pose
    Yc = torch.from_numpy(sk.targets(parents))      # (without confidences: no NaN)
    a = net.fit_keypoints(q, Yc[:, :J], rest, steps=2, return_dist=False)
    b = net.fit_keypoints(q, Yc[:, :J], rest, steps=2, keypoint_joints=torch.arange(J), keypoint_offsets=torch.zeros(J, 3), return_dist=False)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a, q)
    one_conf = c[3].abs().nan_to_num(0.5)
    a, da = net.fit_keypoints(q, Yc, rest, steps=2, conf=one_conf, **tables)
    b, db = net.fit_keypoints(q, Yc, rest, steps=2, conf=one_conf.expand(sk.B, K), **tables)
    assert torch.equal(a, b) and torch.equal(da, db) and bool(torch.isfinite(a).all())
    # steps = 0 is the copy, zero distances and zero energies; an empty batch
    s, ds, Es = net.fit_keypoints(q, Y, rest, steps=0, return_energy=True, **tables)
    assert torch.equal(s, q) and not bool(ds.any()) and not bool(Es.any())
    e, de = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, **tables)
    assert e.shape == (0, J, 4) and de.shape == (0, 1)
    # the energy it returns is the energy of forward_kinematics at the input of the last step
    from posendf_amd import forward_kinematics
    one, E1 = net.fit_keypoints(q, Yc, rest, steps=1, conf=c.abs().nan_to_num(0.5), return_dist=False, return_energy=True, **tables)
    Pk = forward_kinematics(q.double(), parents, rest.double(), kp["kpj"], torch.from_numpy(kp["kpo"]).double())
    E_ref = 0.5 * (c.abs().nan_to_num(0.5).double() * ((Pk - Yc.double()) ** 2).sum(-1)).sum(-1)
    assert torch.allclose(E1.double(), E_ref, rtol=1e-4)
    # wrong shapes, dtypes and values
    for kw in (dict(targets=Y[:, :-1]), dict(targets=Y[:-1]), dict(rest=rest[:-1]), dict(conf=torch.zeros(K + 1)), dict(conf=torch.zeros(sk.B, K, dtype=torch.bool)),
               dict(keypoint_offsets=torch.zeros(K + 1, 3)), dict(keypoint_joints=torch.zeros(K, dtype=torch.float32)), dict(anchor=q[:-1]),
               dict(weight=-1.0), dict(weight=float("inf")), dict(keypoint_joints=torch.full((K,), J, dtype=torch.int64)), dict(frames=5)):
        args = dict(targets=Y, rest=rest, conf=None, **tables)
        args.update(kw)
        with pytest.raises(PndfError):
            net.fit_keypoints(q, steps=1, **args)
    with pytest.raises(PndfError):
        net.fit_keypoints(q[..., :3], Y, rest, **tables)
    with pytest.raises(PndfError):
        forward_kinematics(q, parents, rest[:-1])
    with pytest.raises(PndfError):
        forward_kinematics(q, parents, rest, [J])


def test_keypoint_fitting_driver_on_a_hand():
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    assert posendf_amd.KeypointFitting is KeypointFitting and callable(posendf_amd.fit_keypoint_file)
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cpu_model(parents, "softplus", sd)
    rest, kpj, kpo = sk.tables(parents)
    # targets made from on-manifold poses: seeded poses projected onto the model's manifold
    clean = net.project(torch.from_numpy(sk.unit_poses(12, J, 7)), steps=20, renormalize="unit")[0]
    Y = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    driver = KeypointFitting(net, body_model=None, device="cpu")
    kw = dict(rest=torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo))
    pose, energy, dist, start_energy = driver.fit(Y, hypotheses=4, iterations=3, steps_per_iter=10, seed=0, **kw)
    assert pose.shape == (12, J, 4) and energy.shape == (12,) and dist.shape == (12,) and start_energy.shape == (12, 4)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(energy).all())
    # better than its random starts: the median energy falls
    assert float(energy.median()) < float(start_energy.median()), (float(energy.median()), float(start_energy.median()))
    # the energy it reports is the energy of the pose it returns
    Pk = posendf_amd.forward_kinematics(pose, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    assert torch.allclose(energy, 0.5 * ((Pk - Y) ** 2).sum((-1, -2)), rtol=1e-3, atol=1e-6)
    again = driver.fit(Y, hypotheses=4, iterations=3, steps_per_iter=10, seed=0, **kw)
    assert torch.equal(again[0], pose)
    from posendf_amd import PoseNDF, amass_config
    with pytest.raises(TypeError, match="SkeletonPoseNDF"):
        KeypointFitting(PoseNDF(amass_config("lrelu", "cpu")), body_model=None, device="cpu").fit(torch.zeros(1, 21, 3), rest=torch.zeros(21, 3))


def test_keypoint_fitting_main_reads_and_writes_npz(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    Y = sk.targets(parents, 5)
    np.savez(tmp_path / "kp.npz", keypoints=Y, rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo)
    pose, energy = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2",
                         "--iterations", "2", "--steps_per_iter", "3", "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == (5, len(parents), 4) and f["energy"].shape == (5,) and np.array_equal(f["pose"], pose.numpy())
