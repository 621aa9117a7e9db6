"""Fitting other skeletons to 2D keypoints on an MI355X (pndf_project_options6 of include/posendf_amd.h, the camera term of csrc/pndf_fk.h
and csrc/pndf_skeleton.hip's pndf_skel_enc_rev_image_kernel; DESIGN.md section 2j "Image fitting"): pndf_skel_project with the 168-byte
struct against the numpy restatement (tests/skeleton_image_oracle.py).

2. the stated step: K rounds of pndf_skel_forward_grad + the float32 restatement equal the call, bit for bit -- poses, d_last, kp_energy
   and root.
3. the device against the host twin without feeding: a network with d == 0, ten steps of pure inverse kinematics with a free root, bit
   for bit, in image and 3D mode, with and without tracks, mask and anchor.
4. it is the smaller call; 5. skips; 6. locality (a subtree without keypoints; bad rows at B = 300).
7. the chunk seam at B = 16,384 + 136 with per-pose pixel targets, confidences and roots.
8. ten free-running steps against the fp64 restatement under the project's gate; the device against the twin.
9. the effect: the energy falls at every step.
10. the refusals; the persistent engine keeps refusing the larger struct.
11. `SkeletonPoseNDF.fit_keypoints(camera=, root=)` and `KeypointFitting` on cuda; the exported kernel.
tests/test_skeleton_image.py holds the host twin to the same statements."""
import ctypes

import numpy as np
import pytest

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko
from posendf_amd import synth
from test_skeleton_completion_gpu import cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_image import FREE_WEIGHTS, TwinImage, free_gate, free_run
from test_skeleton_keypoints import FREE_STEPS
from test_skeleton_keypoints_gpu import UnitRunner

pytestmark = pytest.mark.gpu
BAD_ARG = si.BAD_ARG


class UnitImage(si.ImageRunner, UnitRunner):
    """pndf_skel_project with the 168-byte struct: poses, mask words, observation, targets, confidences, energies and roots in device
    memory"""


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitImage(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 2. the stated step
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", si.CASES, ids=sko.case_id)
def test_image_steps_are_the_stated_step(torch_cuda, case, act):
    si.check_stated_step(runner_of(torch_cuda, case, act), case, act)


# ------------------------------------------------------------------------------------------ 3. device against twin, without feeding
@pytest.mark.parametrize("image", [True, False], ids=["image", "3d"])
@pytest.mark.parametrize("case", si.CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_with_a_free_root_equals_the_twin(torch_cuda, case, image):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: nothing
    depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit -- poses, energies and roots"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    _, kp, _ = si.case_kp(case, image=image, conf=True)
    track = sdo.clip(case, si.P, si.T)
    root = si.make_roots(si.B, 37)
    dev, cpu = UnitImage(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinImage(parents, "lrelu", sd, encoder=case[1])
    common = dict(cam=si.cam_of(image, si.RHO if image else 0.0), root=root, root_weights=(si.NU_ROT, si.NU_TRANS))
    for kw in (dict(opts=dict(renormalize="unit")), dict(opts=dict(step_size=0.5), frames=si.T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, si.P, si.T)),
                                                         anchor=sk.flat(sdo.make_anchor(track)), mu=sdo.MU)):
        got, d, E, rt = dev.fit6(sk.flat(track), 10, kp, **common, **kw)
        want, d_want, E_want, r_want = cpu.fit6(sk.flat(track), 10, kp, **common, **kw)
        assert not d.any() and not d_want.any() and np.isfinite(got).all() and np.isfinite(E).all() and E.any() and np.isfinite(rt).all()
        sk.assert_same(got, want, sorted(kw))
        sk.assert_same(E, E_want, sorted(kw) + ["kp_energy"])
        sk.assert_same(rt, r_want, sorted(kw) + ["root"])
        assert got.tobytes() != sk.flat(track).tobytes() and rt.tobytes() != root.tobytes()


# ------------------------------------------------------------------------------------------ 4. - 6.
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_camera_and_root_it_is_the_smaller_call(torch_cuda, case, act):
    si.check_smaller_calls(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", si.CASES, ids=sko.case_id)
def test_skipped_keypoints_are_keypoints_left_out(torch_cuda, case, act):
    si.check_skips(runner_of(torch_cuda, case, act), case, act)


@pytest.mark.parametrize("case,joint", [(("hand", True), 4), (("tree32", True), 7), (("chain32", True), 9), (("hand", False), 13)],
                         ids=["hand", "tree32", "chain32", "hand-noenc"])
def test_a_joint_without_a_keypoint_below_it_is_not_moved(torch_cuda, case, joint):
    si.check_subtree_locality(runner_of(torch_cuda, case, "lrelu"), case, joint)


@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_bad_rows_stay_in_their_pose_and_root_row(torch_cuda, case, act):
    si.check_row_locality(runner_of(torch_cuda, case, act), case, act)


# ------------------------------------------------------------------------------------------ 7. the chunk seam
def test_pixels_confidences_and_roots_follow_the_chunk_seam(torch_cuda):
    """B = 16,384 + 136 is more than a chunk: with per-pose distinct pixel targets, confidences and roots the poses on both sides of the
    seam equal the same poses run alone -- a root, [K,2] target, confidence or energy offset that forgot the chunk would show here.  With
    tracks of 8 frames the chunk is 16,384 poses too (2,048 whole tracks)."""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitImage(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n = 16384 + 136
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(np.asarray(si.CAMERA[2:]) + r.uniform(-200, 200, (n, K, 2)), np.float32)
    conf = r.rand(n, K).astype(np.float32)
    conf[r.rand(n, K) < 0.1] = 0.0
    root = si.make_roots(n, 37)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    common = dict(opts=dict(renormalize="unit", step_size=0.5), cam=si.cam_of(True, si.RHO), root_weights=(si.NU_ROT, si.NU_TRANS))
    for kw in (dict(), dict(frames=8, lam=0.5, flags=sdo.FREE_ENDS)):
        out, d, E, rt = run.fit6(q, 2, kp, root=root, **common, **kw)
        assert np.isfinite(out).all() and np.isfinite(E).all() and np.isfinite(rt).all()
        for part in (slice(16376, 16392), slice(0, 16), slice(n - 8, n)):
            alone = run.fit6(q[part], 2, dict(kp, Y=kp["Y"][part], conf=conf[part]), root=root[part], **common, **kw)
            for a, b in zip(alone, (out, d, E, rt)):
                assert a.tobytes() == b[part].tobytes(), (sorted(kw), part)
    inp = run.fit6(q, 2, kp, root=root, in_place=True, **common)      # without tracks the call may run in place
    for a, b in zip(inp, run.fit6(q, 2, kp, root=root, **common)):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ 8. free running
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    got = free_run(UnitImage(torch_cuda, parents, act, sd), case)
    free_gate(got, case, act, f"unit {sko.case_id(case)} {act}")
    cpu = free_run(TwinImage(parents, act, sd), case)
    free_gate(cpu, case, act, f"twin {sko.case_id(case)} {act}")
    free_gate(got, case, act, f"unit against twin {sko.case_id(case)} {act}", ref=cpu)
    assert FREE_STEPS == 10 and any(FREE_WEIGHTS)


# ------------------------------------------------------------------------------------------ 9. the effect
def test_a_pose_and_root_are_found_from_their_own_pixels(torch_cuda):
    parents, sd, _, _, _ = si.effect_inputs()
    si.check_effect(UnitImage(torch_cuda, parents, "lrelu", sd))


# ------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_write_nothing(torch_cuda):
    si.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


def test_the_persistent_engine_refuses_the_168_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 168-byte struct is
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
    root_np = si.make_roots(n, 37)
    root = torch.from_numpy(root_np.copy()).cuda()
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    big = si.c_options6(lib, sk.c_options5(lib, None, Y.data_ptr(), None, E.data_ptr(), rest.ctypes.data, None, None, 21, 0.02), root.data_ptr(), si.CAMERA, 0.0,
                        si.NU_ROT, si.NU_TRANS, si.KP_IMAGE)
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
    assert root.cpu().numpy().tobytes() == root_np.tobytes()


# ------------------------------------------------------------------------------------------ 11. Python
@pytest.mark.parametrize("act", si.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_fit_keypoints_with_a_camera_on_cuda(torch_cuda, case, act):
    torch = torch_cuda
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cuda_model(torch, parents, act, sd)
    run = UnitImage(torch, parents, act, sd)
    _, kp, _ = si.case_kp(case, conf=True)
    track = sdo.clip(case, si.P, si.T)
    q_np = sk.flat(track)
    root_np = si.make_roots(si.B, 37)
    mask = sdo.make_mask(J, si.P, si.T).reshape(-1, J)
    q, Y, c = torch.from_numpy(q_np.copy()).cuda(), torch.from_numpy(kp["Y"]).cuda(), torch.from_numpy(kp["conf"]).cuda()
    root = torch.from_numpy(root_np.copy()).cuda()
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    weights = (si.NU_ROT, si.NU_TRANS)
    want, d_want, E_want, r_want = run.fit6(q_np, si.K_STEPS, kp, opts=dict(renormalize="unit"), nu=0.05, cam=si.cam_of(True, si.RHO), root=root_np, root_weights=weights)
    out, d, E, rt = net.fit_keypoints(q, Y, rest, steps=si.K_STEPS, weight=0.05, conf=c, renormalize="unit", return_energy=True, camera=si.CAMERA, rho=si.RHO,
                                      root=root, root_weights=weights, return_root=True, **tables)
    assert out.is_cuda and rt.is_cuda and out.shape == (si.B, J, 4) and rt.shape == (si.B, 7)
    assert out.cpu().numpy().tobytes() == want.tobytes() and d.cpu().numpy().tobytes() == d_want.tobytes() and E.cpu().numpy().tobytes() == E_want.tobytes()
    assert rt.cpu().numpy().tobytes() == r_want.tobytes() and rt.cpu().numpy().tobytes() != root_np.tobytes()
    assert q.cpu().numpy().tobytes() == q_np.tobytes() and root.cpu().numpy().tobytes() == root_np.tobytes()      # the inputs are not written
    kw = dict(steps=si.K_STEPS, conf=c, observed=torch.from_numpy(mask), frames=si.T, smooth=0.5, anchor=q, data=0.25, free_ends=True, return_dist=False,
              return_energy=True, camera=si.CAMERA, root_weights=weights, return_root=True)
    want, _, E_want, r_want = run.fit6(q_np, si.K_STEPS, kp, words=sk.pack(mask), frames=si.T, lam=0.5, flags=sdo.FREE_ENDS, anchor=q_np, mu=0.25,
                                       cam=si.cam_of(True), root=root_np, root_weights=weights)
    out, E, rt = net.fit_keypoints(q, Y, rest, root=root, **kw, **tables)
    assert out.cpu().numpy().tobytes() == want.tobytes() and E.cpu().numpy().tobytes() == E_want.tobytes() and rt.cpu().numpy().tobytes() == r_want.tobytes()
    # a root from the cpu is copied to the model's device; a second stream gives the same bits
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again, E_again, r_again = net.fit_keypoints(q, Y, rest, root=torch.from_numpy(root_np.copy()), **kw, **tables)
    side.synchronize()
    assert r_again.is_cuda
    for a, b in ((again, out), (E_again, E), (r_again, rt)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    e, de, re = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, camera=si.CAMERA, root=root[:0], root_weights=weights, return_root=True, **tables)
    assert e.shape == (0, J, 4) and de.shape == (0, 1) and re.shape == (0, 7)
    with pytest.raises(PndfError):
        net.fit_keypoints(q, Y, rest, camera=si.CAMERA, root=root[:, :6], **tables)
    with pytest.raises(PndfError):
        net.fit_keypoints(q, Y, rest, camera=si.CAMERA, root=root, root_weights=(-1.0, 0.0), **tables)


def test_a_root_on_another_device_raises(torch_cuda):
    """`root` is a per-pose tensor: a cuda root handed to a `train.device: cpu` model raises, as the poses do"""
    torch = torch_cuda
    from posendf_amd.engine import PndfError
    from test_skeleton_completion import cpu_model
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    _, kp, _ = si.case_kp(case)
    q = torch.from_numpy(sk.flat(sdo.clip(case, si.P, si.T)))
    Y, rest, root = torch.from_numpy(kp["Y"]), torch.from_numpy(kp["rest"]), torch.from_numpy(si.make_roots(si.B, 37))
    tables = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    host = cpu_model(parents, "lrelu", sd)
    with pytest.raises(PndfError, match="root lives on cuda"):
        host.fit_keypoints(q, Y, rest, steps=1, camera=si.CAMERA, root=root.cuda(), **tables)
    want = host.fit_keypoints(q, Y, rest, steps=2, camera=si.CAMERA, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), return_root=True, **tables)
    assert all(not t.is_cuda for t in want)


def test_keypoint_fitting_driver_with_a_camera_on_a_hand(torch_cuda):
    torch = torch_cuda
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cuda_model(torch, parents, "softplus", sd)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    clean = net.project(torch.from_numpy(sk.unit_poses(12, J, 7)), steps=20, renormalize="unit")[0]
    truth_root = torch.from_numpy(si.make_roots(12, 43, depth=si.EFFECT_DEPTH)).cuda()
    Y = posendf_amd.camera_project(posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo)), truth_root, si.CAMERA)
    start_root = truth_root.clone()
    start_root[:, 4:] += 0.3 * torch.from_numpy(np.random.RandomState(3).randn(12, 3).astype(np.float32)).cuda()
    driver = KeypointFitting(net, body_model=None, device="cuda:0")
    pose, energy, dist, start_energy, root = driver.fit(Y, torch.from_numpy(rest), keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo),
                                                        hypotheses=4, iterations=3, steps_per_iter=10, seed=0, camera=si.CAMERA, root=start_root,
                                                        root_weights=si.EFFECT_ROOT_WEIGHTS, weight=si.EFFECT_NU)
    assert pose.is_cuda and root.is_cuda and pose.shape == (12, J, 4) and root.shape == (12, 7) and start_energy.shape == (12, 4)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(root).all())
    assert float(energy.median()) < float(start_energy.median()), (float(energy.median()), float(start_energy.median()))


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_kernel", "pndf_skel_enc_rev_track_kernel", "pndf_skel_enc_rev_denoise_kernel", "pndf_skel_enc_rev_fit_kernel",
            "pndf_skel_enc_rev_image_kernel"} <= ch.exported_symbols(ge.LIB)
