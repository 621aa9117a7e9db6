"""3D keypoint fitting for other skeletons on an MI355X (pndf_project_options5 of include/posendf_amd.h, csrc/pndf_fk.h and
csrc/pndf_skeleton.hip's pndf_skel_enc_rev_fit_kernel; DESIGN.md section 2j "Keypoint fitting"): pndf_skel_project with the 128-byte struct
against the numpy restatement of the kinematics, their reverse and the fitting step (tests/skeleton_keypoints_oracle.py).

1. the stated step: K rounds of pndf_skel_forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last, kp_energy.
2. the device against the host twin without feeding: a network with d == 0, ten steps of pure inverse kinematics, bit for bit.
3. it is the smaller call; confidences; locality (a subtree without keypoints; bad rows at B = 300, rows in three GEMM tiles).
4. the chunk seam at B = 16,384 + 136 with per-pose targets and confidences.
5. ten free-running steps against the fp64 oracle under the project's gate; the device against the twin.
6. the effect: the energy falls at every step.
7. the refusals; the persistent engine keeps refusing the larger struct.
8. `SkeletonPoseNDF.fit_keypoints` and `KeypointFitting` on cuda; the exported kernel.
tests/test_skeleton_keypoints.py holds the host twin to the same statements."""
import ctypes

import numpy as np
import pytest

import skeleton_denoise_oracle as sdo
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko
from posendf_amd import synth
from test_skeleton_completion_gpu import Unit, cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_keypoints import FREE_STEPS, TwinRunner, free_gate, free_run

pytestmark = pytest.mark.gpu
BAD_ARG = sk.BAD_ARG


class UnitRunner(sk.Runner):
    """pndf_skel_project: poses, mask words, observation, targets, confidences and energies in device memory"""

    def __init__(self, torch, parents, act, sd, encoder=True, hidden=sko.HIDDEN):
        self.torch = torch
        self.unit = Unit(torch, parents, act, sd, encoder=encoder, hidden=hidden)
        self.lib, self.forward, self.forward_grad = self.unit.lib, self.unit.forward, self.unit.forward_grad

    def place(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()

    def addr(self, holder):
        return holder.data_ptr()

    def fetch(self, holder):
        return holder.cpu().numpy()

    def project(self, q, out, d, n, steps, opt):
        ws, size = self.unit.ws(n)
        rc = self.lib.pndf_skel_project(self.unit.h, q, out, d, n, steps, ctypes.byref(opt), ws.data_ptr(), size, self.unit.stream())
        self.torch.cuda.synchronize()
        return rc

    def last_error(self):
        return self.lib.pndf_skel_last_error(self.unit.h)


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitRunner(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", sk.CASES, ids=sko.case_id)
def test_fitting_steps_are_the_stated_step(torch_cuda, case, act):
    sk.check_stated_step(runner_of(torch_cuda, case, act), case, act)


# ------------------------------------------------------------------------------------------ 2. device against twin, without feeding
@pytest.mark.parametrize("case", sk.CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_equals_the_twin(torch_cuda, case):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: the
    descent is exact, nothing depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    _, kp = sk.case_kp(case, conf=True)
    track = sdo.clip(case, sk.P, sk.T)
    dev, cpu = UnitRunner(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinRunner(parents, "lrelu", sd, encoder=case[1])
    for kw in (dict(opts=dict(renormalize="unit")), dict(opts=dict(step_size=0.5), frames=sk.T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, sk.P, sk.T)),
                                                         anchor=sk.flat(sdo.make_anchor(track)), mu=sdo.MU)):
        got, d, E = dev.fit(sk.flat(track), 10, kp=kp, **kw)
        want, d_want, E_want = cpu.fit(sk.flat(track), 10, kp=kp, **kw)
        assert not d.any() and not d_want.any() and np.isfinite(got).all() and np.isfinite(E).all() and E.any()
        sk.assert_same(got, want, sorted(kw))
        sk.assert_same(E, E_want, sorted(kw) + ["kp_energy"])
        assert got.tobytes() != sk.flat(track).tobytes()


# ------------------------------------------------------------------------------------------ 3. the smaller call, confidences, locality
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_keypoints_it_is_the_smaller_call(torch_cuda, case, act):
    sk.check_smaller_call(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", sk.CASES, ids=sko.case_id)
def test_keypoints_without_confidence_are_keypoints_left_out(torch_cuda, case, act):
    sk.check_confidences(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_joint_without_a_keypoint_below_it_is_not_moved(torch_cuda, case, joint):
    sk.check_subtree_locality(runner_of(torch_cuda, case, "lrelu"), case, joint)


@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose(torch_cuda, case, act):
    sk.check_row_locality(runner_of(torch_cuda, case, act), case, act)


# ------------------------------------------------------------------------------------------ 4. the chunk seam
def test_targets_and_confidences_follow_the_chunk_seam(torch_cuda):
    """B = 16,384 + 136 is more than a chunk: with per-pose distinct targets and confidences the poses on both sides of the seam equal the
    same poses run alone -- a target, confidence or energy offset that forgot the chunk would show here.  With tracks of 8 frames the
    chunk is 16,384 poses too (2,048 whole tracks)."""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitRunner(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n = 16384 + 136
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(r.uniform(-2, 2, (n, K, 3)), np.float32)
    conf = r.rand(n, K).astype(np.float32)
    conf[r.rand(n, K) < 0.1] = 0.0
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    opts = dict(renormalize="unit", step_size=0.5)
    for kw in (dict(), dict(frames=8, lam=0.5, flags=sdo.FREE_ENDS)):
        out, d, E = run.fit(q, 2, opts=opts, kp=kp, **kw)
        assert np.isfinite(out).all() and np.isfinite(E).all()
        for part in (slice(16376, 16392), slice(0, 16), slice(n - 8, n)):
            alone, d_alone, E_alone = run.fit(q[part], 2, opts=opts, kp=dict(kp, Y=kp["Y"][part], conf=conf[part]), **kw)
            assert alone.tobytes() == out[part].tobytes() and d_alone.tobytes() == d[part].tobytes() and E_alone.tobytes() == E[part].tobytes(), (sorted(kw), part)
    out, d, E = run.fit(q, 2, opts=opts, kp=kp)      # without tracks the call may run in place
    inp, d_inp, E_inp = run.fit(q, 2, opts=opts, kp=kp, in_place=True)
    assert inp.tobytes() == out.tobytes() and d_inp.tobytes() == d.tobytes() and E_inp.tobytes() == E.tobytes()


# ------------------------------------------------------------------------------------------ 5. free running
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    got = free_run(UnitRunner(torch_cuda, parents, act, sd), case)
    free_gate(got, case, act, f"unit {sko.case_id(case)} {act}")
    cpu = free_run(TwinRunner(parents, act, sd), case)
    free_gate(cpu, case, act, f"twin {sko.case_id(case)} {act}")
    free_gate(got, case, act, f"unit against twin {sko.case_id(case)} {act}", ref=cpu)
    assert FREE_STEPS == 10


# ------------------------------------------------------------------------------------------ 6. the effect
def test_inverse_kinematics_lowers_the_energy_at_every_step(torch_cuda):
    parents, sd, _, _ = sk.effect_inputs()
    sk.check_effect(UnitRunner(torch_cuda, parents, "lrelu", sd))


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing(torch_cuda):
    sk.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


def test_the_persistent_engine_refuses_the_128_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 128-byte struct is
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
    Y, E = torch.zeros((n, 21, 3), device="cuda:0"), torch.full((n,), 7.0, device="cuda:0")
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    big = sk.c_options5(lib, None, Y.data_ptr(), None, E.data_ptr(), rest.ctypes.data, None, None, 21, 0.02)
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


# ------------------------------------------------------------------------------------------ 8. Python
@pytest.mark.parametrize("act", sk.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_on_cuda(torch_cuda, case, act):
    torch = torch_cuda
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cuda_model(torch, parents, act, sd)
    run = UnitRunner(torch, parents, act, sd)
    _, kp = sk.case_kp(case, conf=True)
    track = sdo.clip(case, sk.P, sk.T)
    q_np = sk.flat(track)
    mask = sdo.make_mask(J, sk.P, sk.T).reshape(-1, J)
    q, Y, c = torch.from_numpy(q_np.copy()).cuda(), torch.from_numpy(kp["Y"]).cuda(), torch.from_numpy(kp["conf"]).cuda()
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    want, d_want, E_want = run.fit(q_np, sk.K_STEPS, opts=dict(renormalize="unit"), kp=kp, nu=0.05)
    out, d, E = net.fit_keypoints(q, Y, rest, steps=sk.K_STEPS, weight=0.05, conf=c, renormalize="unit", return_energy=True, **tables)
    assert out.is_cuda and out.shape == (sk.B, J, 4) and d.shape == (sk.B, 1) and E.shape == (sk.B,)
    assert out.cpu().numpy().tobytes() == want.tobytes() and d.cpu().numpy().tobytes() == d_want.tobytes() and E.cpu().numpy().tobytes() == E_want.tobytes()
    assert q.cpu().numpy().tobytes() == q_np.tobytes()      # the input is not written
    want, d_want, E_want = run.fit(q_np, sk.K_STEPS, words=sk.pack(mask), frames=sk.T, lam=0.5, flags=sdo.FREE_ENDS, anchor=q_np, mu=0.25, kp=kp)
    out, E = net.fit_keypoints(q, Y, rest, steps=sk.K_STEPS, conf=c, observed=torch.from_numpy(mask), frames=sk.T, smooth=0.5, anchor=q, data=0.25,
                               free_ends=True, return_dist=False, return_energy=True, **tables)
    assert out.cpu().numpy().tobytes() == want.tobytes() and E.cpu().numpy().tobytes() == E_want.tobytes()
    # tables given as cuda tensors are brought to the host; a second stream gives the same bits
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again, E_again = net.fit_keypoints(q, Y, rest.cuda(), steps=sk.K_STEPS, conf=c, observed=torch.from_numpy(mask), frames=sk.T, smooth=0.5, anchor=q,
                                           data=0.25, free_ends=True, return_dist=False, return_energy=True, keypoint_joints=tables["keypoint_joints"].cuda(),
                                           keypoint_offsets=tables["keypoint_offsets"].cuda())
    side.synchronize()
    assert torch.equal(again.view(torch.int32), out.view(torch.int32)) and torch.equal(E_again.view(torch.int32), E.view(torch.int32))
    e, de = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, **tables)
    assert e.shape == (0, J, 4) and de.shape == (0, 1)
    with pytest.raises(PndfError):
        net.fit_keypoints(q, Y[:, :-1], rest, **tables)
    with pytest.raises(PndfError):
        net.fit_keypoints(q, Y, rest, weight=-1.0, **tables)


def test_where_tensors_may_live(torch_cuda):
    """per-pose tensors (poses, targets, conf, anchor, observed) are taken from the model's device and from the cpu; a cuda tensor handed to
    a `train.device: cpu` model raises.  The small tables are host tables and are taken from anywhere."""
    torch = torch_cuda
    from posendf_amd.engine import PndfError
    from test_skeleton_completion import cpu_model
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    J = len(parents)
    _, kp = sk.case_kp(case)
    K = len(kp["kpj"])
    q = torch.from_numpy(sk.flat(sdo.clip(case, sk.P, sk.T)))
    Y, rest = torch.from_numpy(kp["Y"]), torch.from_numpy(kp["rest"])
    conf = torch.full((sk.B, K), 0.5)
    mask = torch.from_numpy(sdo.make_mask(J, sk.P, sk.T).reshape(-1, J))
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    kw = dict(steps=2, conf=conf, anchor=q, data=0.25, observed=mask, return_energy=True)
    # refused: anything per pose on the GPU for a model on the cpu -- and nothing is computed on the way
    host = cpu_model(parents, "lrelu", sd)
    want = host.fit_keypoints(q, Y, rest, **kw, **tables)
    for name in ("poses", "targets", "conf", "anchor", "observed"):
        args = dict(poses=q, targets=Y, **kw)
        args[name] = args[name].cuda()
        with pytest.raises(PndfError, match=f"{name} lives on cuda"):
            host.fit_keypoints(args.pop("poses"), args.pop("targets"), rest, **args, **tables)
    # accepted on the cpu model: the tables from the GPU
    got = host.fit_keypoints(q, Y, rest.cuda(), **kw, **{k: v.cuda() for k, v in tables.items()})
    assert all(not t.is_cuda and torch.equal(a, t) for a, t in zip(want, got))
    # accepted on the cuda model: every per-pose tensor from the cpu, from the GPU, or mixed -- the same bits, results on the GPU
    net = cuda_model(torch, parents, "lrelu", sd)
    on_gpu = net.fit_keypoints(q.cuda(), Y.cuda(), rest, **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}, **tables)
    from_cpu = net.fit_keypoints(q, Y, rest, **kw, **tables)
    mixed = net.fit_keypoints(q.cuda(), Y, rest.cuda(), **dict(kw, conf=conf.cuda()), **tables)
    for other in (from_cpu, mixed):
        assert all(t.is_cuda and torch.equal(a.view(torch.int32), t.view(torch.int32)) for a, t in zip(on_gpu, other))


def test_keypoint_fitting_driver_on_a_hand(torch_cuda):
    torch = torch_cuda
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cuda_model(torch, parents, "softplus", sd)
    rest, kpj, kpo = sk.tables(parents)
    clean = net.project(torch.from_numpy(sk.unit_poses(12, J, 7)), steps=20, renormalize="unit")[0]
    Y = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    driver = KeypointFitting(net, body_model=None, device="cuda:0")
    pose, energy, dist, start_energy = driver.fit(Y, torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo),
                                                  hypotheses=4, iterations=3, steps_per_iter=10, seed=0)
    assert pose.is_cuda and pose.shape == (12, J, 4) and start_energy.shape == (12, 4) and bool(torch.isfinite(pose).all())
    assert float(energy.median()) < float(start_energy.median()), (float(energy.median()), float(start_energy.median()))


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_kernel", "pndf_skel_enc_rev_track_kernel", "pndf_skel_enc_rev_denoise_kernel", "pndf_skel_enc_rev_fit_kernel"} <= ch.exported_symbols(ge.LIB)
