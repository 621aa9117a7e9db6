"""Moving cameras inside the projection step, on the host (pndf_project_options10 of include/posendf_amd.h, pndf_fk_cams_energy_grad of
csrc/pndf_fk.h; DESIGN.md section 2j "Moving cameras"): the host twin pndf_project_ex_cpu with the 280-byte struct against the numpy
restatement (tests/skeleton_cams_oracle.py).

0. the restatement: the all-poses form the checks use equals the several-camera restatement applied pose by pose, bit for bit (this one
   runs on the restatement alone and passes without the feature).
1. the reduction: tables whose every block is one [V,16] table give the bytes of the 224 / 256-byte call with that table.
2. the stated step: blocks that differ per pose, both layouts, scales, the root in place and out of place, 0 .. 3 steps.
3. locality.  4. the skip: fx or fy not positive switches a view off before anything of it is read.
7. the refusals, the ABI, the other entry points.  8. the Python layer on a cpu model, the command line, the keep-alive of the table.
9. the effect, on the float64 restatement alone (passes without the feature).
Every test but 0 and 9 fails on the parent commit, where the 280-byte struct is refused and fit_keypoints takes no 3-D views.  Runs without
a GPU; tests/test_skeleton_cams_gpu.py holds the HIP unit to the same statements (and has the twin comparison and the chunk seam)."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_cams_oracle as sc
import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
import skeleton_root_oracle as sr
import skeleton_views_oracle as sv
from test_skeleton_completion import cpu_model
from test_skeleton_root import TwinRoot

BAD_ARG = sc.BAD_ARG
CASES = [("hand", True), ("tree32", True)]


class TwinCams(sc.CamsRunner, TwinRoot):
    """pndf_project_ex_cpu with the 280-byte struct: every array, the view table included, in host memory"""


def runner_of(case, act):
    parents, sd = sko.case_network(case, act)
    return TwinCams(parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 0. the restatement
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
def test_restatement_is_the_several_camera_one_pose_by_pose(V):
    case = ("hand", True)
    n = 9
    tables = sc.make_tables(n, V, 3)
    tables[2, 0, 0] = 0.0
    tables[5, V - 1, 1] = np.nan
    tables[7, :, 0] = -1.0      # every view of pose 7
    parents, kp = sc.case_kp(case, tables, conf=True)
    q = sk.unit_poses(n, len(parents), 5)
    root = si.make_roots(n, 37)
    sigma = sl.make_scales(n, len(parents) + len(kp["kpj"]))
    for rt, sg in ((root, sigma), (None, None)):
        views, kp_ = sc.stated(tables, kp)
        got = sv.views_energy_grad(q, parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp_["conf"], rt, si.RHO, views, sg)
        want = sc.energy_grad_by_pose(q, parents, kp, tables, rt, si.RHO, sg)
        for a, b, name in zip(got, want, ("E", "dQ", "droot", "h")):
            sc.same_bytes(a, b, (V, name))
        every_view_off = ~sc.on_views(tables).any(axis=1)
        assert every_view_off[7] and not got[0][every_view_off].any() and not got[1][every_view_off].any() and got[0][~every_view_off].all()


# ------------------------------------------------------------------------------------------ 1. the reduction
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_equal_blocks_are_the_static_call(case, V):
    sc.check_reduction_to_static(runner_of(case, "lrelu"), case, V)


# ------------------------------------------------------------------------------------------ 2. the stated step
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_moving_cameras_are_the_stated_step(case, V):
    sc.check_stated_step(runner_of(case, "lrelu"), case, V)


def test_moving_cameras_are_the_stated_step_with_softplus():
    sc.check_stated_step(runner_of(("hand", True), "softplus"), ("hand", True), 2, step_counts=(2, 3))


# ------------------------------------------------------------------------------------------ 3. locality, 4. the skip
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_a_block_is_its_pose_s_alone(case, V):
    sc.check_locality(runner_of(case, "lrelu"), case, V)


@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_a_focal_length_that_is_not_positive_switches_the_view_off(case, V):
    sc.check_skip(runner_of(case, "lrelu"), case, V)


# ------------------------------------------------------------------------------------------ 7. refusals, ABI
def test_refusals_write_nothing():
    sc.check_refusals(runner_of(("hand", True), "lrelu"))


@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_the_struct_without_a_table_is_the_256_byte_call(case):
    sc.check_empty_struct(runner_of(case, "lrelu"), case)


def big_struct(lib, Y_ptr, E_ptr, rest, root_ptr, table_ptr):
    """a 280-byte struct for a 21-joint handle: two tracks of two frames, the joints as keypoints, one moving view"""
    b6 = si.c_options6(lib, sk.c_options5(lib, sdo.c_from(lib, {}, None, 2, 0.0, None, None, 0.0, sdo.FREE_ENDS), Y_ptr, None, E_ptr, rest.ctypes.data, None, None,
                                          21, 0.02), root_ptr, sv.UNREAD_CAMERA, 0.0, 0.0, si.NU_TRANS, si.KP_IMAGE)
    return sc.c_options10(lib, sr.c_options9(lib, sv.c_options8(lib, sl.c_options7(lib, b6)), None, 0.0, sr.LAM_TRANS), table_ptr, 1, 0)


def test_the_other_entry_points_refuse_the_280_byte_struct():
    """every other function with a pndf_project_options parameter: a 280-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers; the persistent engine's entry points are in the GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    rest, Y, E = np.zeros((21, 3), np.float32), np.full((4, 1, 21, 2), 300.0, np.float32), np.full(4, 7.0, np.float32)
    root = si.make_roots(4, 37)
    table = np.ascontiguousarray(np.tile(sv.identity_view(), (4, 1, 1)))
    big = big_struct(lib, Y.ctypes.data, E.ctypes.data, rest, root.ctypes.data, table.ctypes.data)
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
    # the twin that takes it does, on this 21-joint handle too
    kept = root.copy()
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0, lib.pndf_cpu_last_error(eng.handle)
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and root.tobytes() != kept.tobytes()


def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_cams_kernel" in ch.exported_symbols(ge.LIB)
    o10 = abi.ProjectOptions10
    assert ctypes.sizeof(o10) == 280 and engine.ProjectOptions10 is o10 and abi.VIEWS_PER_FRAME == 1
    assert (o10.base9.offset, o10.pose_views.offset, o10.n_pose_views.offset, o10.view_flags.offset, o10.reserved6.offset) == (0, 256, 264, 268, 272)
    lib = engine.load_library()
    table = sc.make_tables(7, 3, 7)
    o = engine.project_options10(lib, 64, 7, smooth=0.25, kp_target_ptr=512, rest_ptr=4096, n_keypoints=20, kp_weight=0.02, step_size=0.5, renorm="unit",
                                 root_ptr=32768, root_weights=(0.25, 0.5), rho=0.125, root_smooth=(0.375, 0.25), pose_views=table, views_per_frame=True)
    b = o.base9.base8.base7.base6.base5.base4.base3.base2.base
    assert (b.struct_size, b.step_size, o.base9.base8.base7.base6.base5.base4.base3.frames, o.base9.base8.base7.base6.kp_flags) == (280, 0.5, 7, 1)
    assert (o.base9.base8.views, o.base9.base8.n_views, o.base9.lambda_rot, o.n_pose_views, o.view_flags, o.reserved6) == (None, 0, 0.375, 3, 1, 0)
    assert o.pose_views % 16 == 0
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * table.size).from_address(o.pose_views)).reshape(table.shape), table)
    o = engine.project_options10(lib, None, 0)
    assert (o.base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size, o.pose_views, o.n_pose_views, o.view_flags, o.reserved6) == (280, None, 0, 0, 0)
    with pytest.raises(engine.PndfError):
        engine.project_options10(lib, None, 0, pose_views=table[0])
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sc.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "cams" in n or "pose_views" in n]
    assert not [h for h in abi.HEADERS if "cams" in h]
    assert not [h for h in os.listdir(os.path.join(ge.REPO, "include")) if "cams" in h]


def test_project_options10_keeps_its_table_alive():
    """the struct holds a plain address into the table's storage: the options object must own the table, or a caller who builds the
    options and drops the tensor reads freed memory"""
    from posendf_amd import engine
    lib = engine.load_library()
    want = sc.make_tables(6, 2, 3)
    table = torch.from_numpy(want.copy())
    o = engine.project_options10(lib, None, 0, pose_views=table)
    del table
    gc.collect()
    junk = [torch.full((6, 2, 16), 7.0) for _ in range(64)]      # (what would land in a freed block of the same size)
    assert np.array_equal(np.ctypeslib.as_array((ctypes.c_float * want.size).from_address(o.pose_views)).reshape(want.shape), want) and junk
    # and the call reads it: the twin with the dropped tensor's struct equals the twin with a table that lives
    case = ("hand", True)
    run = runner_of(case, "lrelu")
    _, kp = sc.case_kp(case, want)
    q = sk.unit_poses(6, len(sko.SKELETONS["hand"]), 5)
    alive = run.fit10(q, 2, kp, pose_views=want, rho=si.RHO)

    def make10(at, o9):
        held = torch.from_numpy(want.copy())
        struct = engine.project_options10(lib, None, 0, pose_views=held)
        del held
        gc.collect()
        o10 = sc.c_options10(lib, o9, struct.pose_views, struct.n_pose_views, struct.view_flags)
        o10._owner = struct
        return o10
    junk = [torch.full((6, 2, 16), 7.0) for _ in range(64)]
    rc, out, d, E, _, _ = run.run10(q, 2, kp, pose_views=want, rho=si.RHO, make10=make10)
    assert rc == 0 and out.tobytes() == alive[0].tobytes() and E.tobytes() == alive[2].tobytes() and junk


# ------------------------------------------------------------------------------------------ 8. the Python layer
def check_model_fit_keypoints(net, run, case, device):
    """fit_keypoints(views=[B,V,16]) and (views=[T,V,16], frames=T) equal the raw call, bit for bit; camera_project with a batched table
    gives the pixels of the oracle"""
    import posendf_amd
    from posendf_amd.engine import PndfError
    T, V = 5, 2
    n = sc.P * T
    tables = sc.make_tables(n, V, T)
    tables[3, 1, 0] = 0.0      # a camera without a calibration in one frame
    parents, kp = sc.case_kp(case, tables, conf=True)
    ln = sc.scales_of(case, kp, n, T)
    q_np = sk.flat(sdo.clip(case, sc.P, T))
    root_np = si.make_roots(n, 37)
    to = lambda a: torch.from_numpy(np.array(a)).to(device)  # noqa: E731
    q, Y, c, root = to(q_np), to(kp["Y"]), to(kp["conf"]), to(root_np)
    tb = dict(keypoint_joints=torch.from_numpy(kp["kpj"]), keypoint_offsets=torch.from_numpy(kp["kpo"]))
    rest = torch.from_numpy(kp["rest"])
    common = dict(conf=c, renormalize="unit", frames=T, smooth=0.5, free_ends=True, return_energy=True, root=root, root_weights=sc.WEIGHTS, return_root=True,
                  bone_scale=to(ln["scale"]), scale_weight=sl.NU_LEN, scale_prior=sl.KAPPA, scale_rates=torch.from_numpy(ln["rate"]), return_scale=True,
                  rho=si.RHO, **tb)
    raw = dict(opts=dict(renormalize="unit"), frames=T, lam=0.5, flags=sdo.FREE_ENDS, root=root_np, root_weights=sc.WEIGHTS, ln=ln, rho=si.RHO)
    for steps in (2, 3):
        for coupled in ({}, dict(root_smooth=sc.COUPLED["root_smooth"])):
            want = run.fit10(q_np, steps, kp, pose_views=tables, **coupled, **raw)
            got = net.fit_keypoints(q, Y, rest, steps=steps, views=tables if steps == 2 else to(tables), **coupled, **common)
            for a, b in zip(got, want):
                assert a.device.type == device and a.cpu().numpy().tobytes() == b.tobytes()
            want = run.fit10(q_np, steps, kp, pose_views=tables[:T], per_frame=True, **coupled, **raw)
            got = net.fit_keypoints(q, Y, rest, steps=steps, views=to(tables[:T]).double(), **coupled, **common)
            for a, b in zip(got, want):
                assert a.cpu().numpy().tobytes() == b.tobytes()
    # B == frames: per pose and per frame mean the same
    one = slice(0, T)
    a = net.fit_keypoints(q[one], Y[one], rest, steps=2, views=tables[one], **dict(common, conf=c[one], root=root[one], bone_scale=to(ln["scale"][:1])))
    b = run.fit10(q_np[one], 2, dict(kp, Y=kp["Y"][one], conf=kp["conf"][one]), pose_views=tables[one], **dict(raw, root=root_np[one], ln=dict(ln, scale=ln["scale"][:1])))
    assert a[0].cpu().numpy().tobytes() == b[0].tobytes()
    # a 2-D table goes the old way
    static = sv.make_views(V)
    want = run.fit9(q_np, 2, kp, views=static, cam=si.cam_of(True, si.RHO, sv.UNREAD_CAMERA), **raw)
    got = net.fit_keypoints(q, Y, rest, steps=2, views=static, **common)
    for a, b in zip(got, want):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    e = net.fit_keypoints(q[:0], Y[:0], rest, steps=2, views=to(tables[:0]), **tb)
    assert e[0].shape == (0, q.shape[1], 4)
    for kw in (dict(views=tables[:4]), dict(views=tables[:T], frames=None, smooth=0.0, free_ends=False), dict(views=tables[:, :, :15]),
               dict(views=np.zeros((n, 9, 16), np.float32)), dict(views=torch.zeros(n, V, 16, dtype=torch.int32)), dict(views=tables, camera=si.CAMERA)):
        args = dict(common)
        args.update(kw)
        with pytest.raises(PndfError) as err:
            net.fit_keypoints(q, Y, rest, steps=1, **args)
        if kw.get("views") is not None and tuple(kw["views"].shape) == (4, V, 16):
            assert f"[4,{V},16]" in str(err.value) and f"[{n},{V},16]" in str(err.value)
    # camera_project with a table per pose: the oracle's pixels (float64), and the broadcast over leading dimensions
    pose64 = torch.from_numpy(sk.unit_poses(n, len(parents), 31)).double()
    Pk = posendf_amd.forward_kinematics(pose64, parents, rest.double(), kp["kpj"], torch.from_numpy(kp["kpo"]).double())
    clean = sc.case_kp(case, tables)[1]["Y"]
    ok = tables.copy()
    ok[3, 1, 0] = sc.make_tables(n, V, T)[3, 1, 0]
    pix = posendf_amd.camera_project(Pk, torch.from_numpy(si.make_roots(n, 29)).double(), views=torch.from_numpy(ok).double())
    assert pix.shape == (n, V, len(kp["kpj"]), 2)
    want = sc.case_kp(case, ok)[1]["Y"]
    assert np.allclose(pix.numpy(), want, rtol=1e-5, atol=1e-3) and clean.shape == want.shape
    wide = posendf_amd.camera_project(Pk.reshape(sc.P, T, -1, 3), torch.from_numpy(si.make_roots(n, 29)).double().reshape(sc.P, T, 7), views=ok[:T])
    again = posendf_amd.camera_project(Pk, torch.from_numpy(si.make_roots(n, 29)).double(), views=np.tile(ok[:T], (sc.P, 1, 1)))
    assert wide.shape == (sc.P, T, V, len(kp["kpj"]), 2) and torch.equal(wide.reshape(again.shape), again)


@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_model_fit_keypoints_with_moving_cameras_on_cpu(case):
    parents, sd = sko.case_network(case, "lrelu")
    check_model_fit_keypoints(cpu_model(parents, "lrelu", sd), runner_of(case, "lrelu"), case, "cpu")


def check_drivers(net, device):
    """KeypointFitting.fit(views=[N,V,16]) and fit_clip(views=[T,V,16] / [P*T,V,16]) on a moving rig: shapes, finite results, the energy
    lowered, and the two forms of the clip's table agree"""
    import posendf_amd
    from posendf_amd.keypoint_fitting import KeypointFitting, keypoint_energy
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    Pn, T, V = 2, 4, 2
    path = sc.make_tables(T, V, T)
    tables = np.tile(path, (Pn, 1, 1))
    clean = net.project(torch.from_numpy(sk.unit_poses(Pn * T, J, 7)).to(device), steps=20, renormalize="unit")[0]
    true_root = torch.from_numpy(si.make_roots(Pn * T, 43, depth=si.EFFECT_DEPTH)).to(device)
    Pk = posendf_amd.forward_kinematics(clean, parents, torch.from_numpy(rest), kpj, torch.from_numpy(kpo))
    Y = posendf_amd.camera_project(Pk, true_root, views=torch.from_numpy(tables).to(device))
    assert Y.shape == (Pn * T, V, len(kpj), 2)
    start_root = true_root.clone()
    start_root[:, 4:] += 0.2
    kw = dict(keypoint_joints=torch.from_numpy(kpj), keypoint_offsets=torch.from_numpy(kpo), hypotheses=3, iterations=2, steps_per_iter=5, seed=0, weight=0.1,
              root=start_root, root_weights=(0.0, 0.1))
    driver = KeypointFitting(net, body_model=None, device=device)
    pose, energy, dist, start, root = driver.fit(Y, torch.from_numpy(rest), views=tables, **kw)
    assert pose.shape == (Pn * T, J, 4) and root.shape == (Pn * T, 7) and bool(torch.isfinite(pose).all()) and bool(torch.isfinite(root).all())
    assert float(energy.median()) < float(start.median())
    # the energy the driver reports is the statement's, with the table of every target
    again = keypoint_energy(pose, Y, parents, torch.from_numpy(rest).to(device), None, kw["keypoint_joints"], torch.from_numpy(kpo).to(device), root, views=torch.from_numpy(tables).to(device))
    assert torch.allclose(again, energy, rtol=1e-4, atol=1e-7)
    with pytest.raises(ValueError):
        driver.fit(Y, torch.from_numpy(rest), views=tables[:-1], **kw)
    clip = dict(kw, clip_steps=7, smooth=0.25, root_smooth=(0.0, 0.5))
    a = driver.fit_clip(Y, torch.from_numpy(rest), T, views=path, **clip)
    b = driver.fit_clip(Y, torch.from_numpy(rest), T, views=torch.from_numpy(tables), **clip)
    assert a[0].shape == (Pn * T, J, 4) and a[3].shape == (Pn * T, 7) and bool(torch.isfinite(a[0]).all())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[3][:, 4:], start_root[:, 4:])


def test_keypoint_fitting_drivers_with_a_moving_rig():
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_drivers(cpu_model(parents, "softplus", sd), "cpu")


def test_keypoint_fitting_main_takes_moving_views(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.keypoint_fitting import main, view_tables
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    rest, kpj, kpo = sk.tables(parents)
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    N, V, T = 6, 2, 3
    tables = sc.make_tables(N, V, T)
    _, kp = sc.case_kp(case, tables)
    K4, R, t = tables[:, :, :4], tables[:, :, 4:13].reshape(N, V, 3, 3), tables[:, :, 13:]
    K33 = np.zeros((N, V, 3, 3), np.float32)
    K33[..., 0, 0], K33[..., 1, 1], K33[..., 0, 2], K33[..., 1, 2], K33[..., 2, 2] = K4[..., 0], K4[..., 1], K4[..., 2], K4[..., 3], 1.0
    assert np.array_equal(view_tables(K4, R, t), tables) and np.array_equal(view_tables(K33, R, t), tables)
    with pytest.raises(ValueError):
        view_tables(K4, R[:, :1], t)
    np.savez(tmp_path / "kp.npz", keypoints=kp["Y"], rest=rest, keypoint_joints=kpj, keypoint_offsets=kpo, root=si.make_roots(N, 37))
    np.savez(tmp_path / "moving4.npz", K=K4, R=R, t=t)
    np.savez(tmp_path / "moving33.npz", K=K33, R=R, t=t)
    np.savez(tmp_path / "path.npz", K=K4[:T], R=R[:T], t=t[:T])
    base = ["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-kf", str(tmp_path / "kp.npz"), "--hypotheses", "2", "--iterations", "2",
            "--steps_per_iter", "3", "--root_weights", "0.0", "0.1"]
    a = main(base + ["--views", str(tmp_path / "moving4.npz"), "--out", str(tmp_path / "out.npz")])
    b = main(base + ["--views", str(tmp_path / "moving33.npz")])
    assert a[0].shape == (N, len(parents), 4) and torch.equal(a[0], b[0]) and bool(torch.isfinite(a[1]).all())
    with np.load(tmp_path / "out.npz") as f:
        assert np.array_equal(f["pose"], a[0].numpy()) and f["root"].shape == (N, 7)
    # with --clip T: a table per frame of the file, or one path for every clip
    for name in ("moving4.npz", "path.npz"):
        pose, energy = main(base + ["--views", str(tmp_path / name), "--clip", str(T), "--root_smooth", "0.0", "0.5"])
        assert pose.shape == (N, len(parents), 4) and bool(torch.isfinite(energy).all())


# ------------------------------------------------------------------------------------------ 9. the effect
def test_moving_tables_recover_the_world_root():
    """On the float64 restatement alone (passes without the feature): a 15-joint hand moves in a world frame, seen by a two-camera rig that
    moves 1.2 units along x and turns 0.35 rad about y over 24 frames; pixel noise of 1.5 px; the schedule of
    profiles/skeleton_root/effect.json (150 steps, nu 0.05, the root's translation free with 0.05 and coupled with 0.5 in BOTH fits).
    The rig's displacement is several times what the pixel noise can move a fitted root: at the hand's depth of about 6 units and a
    focal length of 500 px, 1.5 px of noise on one keypoint is 0.018 units across the optical axis and, over the rig's 0.12 baseline,
    about 0.9 units along it -- for ONE keypoint; averaged over 20 keypoints and two views, about 0.15.  The rig moves 1.2: eight times
    that.  The condition is the order alone: the RMS error of the fitted world root translation is smaller with the table of every
    frame than with frame 0's table frozen.  The figures of this fixture are recorded in profiles/skeleton_cams/effect.json."""
    got = sc.oracle_effect()
    print(json.dumps(got))
    assert all(np.isfinite(v) for v in got.values())
    assert got["rms_moving"] < got["rms_frozen"]
    recorded = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "skeleton_cams", "effect.json")
    with open(recorded) as f:
        want = json.load(f)
    for key, value in got.items():
        assert abs(want[key] - value) <= 1e-3 * abs(value), (key, want[key], value)      # the record is this fixture's (float64; 1e-3 leaves room for a BLAS)
