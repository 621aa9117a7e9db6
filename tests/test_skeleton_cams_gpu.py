"""Moving cameras inside the projection step on an MI355X (pndf_project_options10 of include/posendf_amd.h, pndf_fk_cams_energy_grad of
csrc/pndf_fk.h and csrc/pndf_skeleton.hip's pndf_skel_enc_rev_cams_kernel; DESIGN.md section 2j "Moving cameras"): pndf_skel_project with
the 280-byte struct and the view table in device memory against the numpy restatement (tests/skeleton_cams_oracle.py).

1. the reduction: tables whose every block is one [V,16] table give the bytes of the 224 / 256-byte call with that table.
2. the stated step: blocks that differ per pose, both layouts, scales, the root in place and out of place, 0 .. 3 steps.
3. locality.  4. the skip.
5. the device against the host twin without a GEMM in the way: a network with d == 0, ten steps, bit for bit, roots and scales included,
   V = 2 and 8, both layouts.
6. the chunk seam at B = 16,520 with tracks of 7, V = 2: the per-pose table must follow the chunk, the per-frame table must not.
7. the refusals; the persistent engine keeps refusing the struct.  8. the Python layer on cuda; the kernel's symbol.
tests/test_skeleton_cams.py holds the host twin to the same statements.  Every test here fails on the parent commit."""
import ctypes

import numpy as np
import pytest

import skeleton_cams_oracle as sc
import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko
import skeleton_root_oracle as sr
from posendf_amd import synth
from test_skeleton_cams import CASES, TwinCams, big_struct, check_drivers, check_model_fit_keypoints
from test_skeleton_completion_gpu import cuda_model, torch_cuda  # noqa: F401  (torch_cuda: the fixture)
from test_skeleton_root_gpu import UnitRoot

pytestmark = pytest.mark.gpu
BAD_ARG = sc.BAD_ARG


class UnitCams(sc.CamsRunner, UnitRoot):
    """pndf_skel_project with the 280-byte struct: poses, mask words, targets, confidences, energies, roots, the root anchor, scales and
    the view table in device memory; the rates in host memory"""


def runner_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return UnitCams(torch, parents, act, sd, encoder=case[1])


# ------------------------------------------------------------------------------------------ 1. the reduction
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_equal_blocks_are_the_static_call(torch_cuda, case, V):
    sc.check_reduction_to_static(runner_of(torch_cuda, case, "lrelu"), case, V)


# ------------------------------------------------------------------------------------------ 2. the stated step
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_moving_cameras_are_the_stated_step(torch_cuda, case, V):
    sc.check_stated_step(runner_of(torch_cuda, case, "lrelu"), case, V)


def test_moving_cameras_are_the_stated_step_with_softplus(torch_cuda):
    sc.check_stated_step(runner_of(torch_cuda, ("hand", True), "softplus"), ("hand", True), 2, step_counts=(2, 3))


# ------------------------------------------------------------------------------------------ 3. locality, 4. the skip
@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_a_block_is_its_pose_s_alone(torch_cuda, case, V):
    sc.check_locality(runner_of(torch_cuda, case, "lrelu"), case, V)


@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_a_focal_length_that_is_not_positive_switches_the_view_off(torch_cuda, case, V):
    sc.check_skip(runner_of(torch_cuda, case, "lrelu"), case, V)


# ------------------------------------------------------------------------------------------ 5. the twin
@pytest.mark.parametrize("per_frame", (False, True), ids=("per_pose", "per_frame"))
@pytest.mark.parametrize("V", (2, 8))
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_pure_inverse_kinematics_with_moving_cameras_equals_the_twin(torch_cuda, case, V, per_frame):
    """behind an output bias of -1e3 a relu-family network gives d == 0 and a zero gradient exactly, on the device and on the host: nothing
    depends on a GEMM's sum order, and ten steps of the unit equal ten steps of the twin bit for bit -- poses, energies, roots and scales"""
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    dev, cpu = UnitCams(torch_cuda, parents, "lrelu", sd, encoder=case[1]), TwinCams(parents, "lrelu", sd, encoder=case[1])
    for T in sc.FRAMES:
        n = sc.P * T
        tables = sc.make_tables(T if per_frame else n, V, T)
        tables[0, V - 1, 0] = 0.0      # one camera has no calibration in one block
        _, kp = sc.case_kp(case, sc.blocks_of(tables, n), conf=True)
        track = sdo.clip(case, sc.P, T)
        root = si.make_roots(n, 37)
        for coupled in (False, True):
            kw = dict(opts=dict(step_size=0.5), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, words=sk.pack(sdo.make_mask(J, sc.P, T)), rho=si.RHO,
                      ln=sc.scales_of(case, kp, n, T), root=root, root_weights=sc.WEIGHTS, pose_views=tables, per_frame=per_frame)
            if coupled:
                kw.update(sc.COUPLED, root_anchor=sr.make_anchor(root))
            got = dev.fit10(sk.flat(track), 10, kp, **kw)
            want = cpu.fit10(sk.flat(track), 10, kp, **kw)
            assert not got[1].any() and not want[1].any() and all(np.isfinite(a).all() for a in got) and got[2].any()
            for a, b, name in zip(got, want, sc.NAMES):
                if name != "d_last":      # (d == 0 on both sides, asserted above; its sign is the output layer's, not this feature's)
                    sk.assert_same(a, b, (V, T, per_frame, coupled, name))
            assert got[0].tobytes() != sk.flat(track).tobytes() and (got[3] != root).any()


# ------------------------------------------------------------------------------------------ 6. the chunk seam
@pytest.mark.parametrize("steps", (2, 3))
def test_tables_follow_the_chunk_seam(torch_cuda, steps):
    """B = 16,520 with tracks of 7 frames is more than a chunk (2,340 whole tracks per chunk, seam at 16,380), V = 2.  The tracks on both
    sides of the seam, the first two and the last one equal the float32 restatement with their own blocks, bit for bit, roots included: a
    per-pose table whose offset forgot the chunk would give the second chunk the first one's blocks, a per-frame table to which the chunk
    offset was applied would read behind the path.  The odd step count ends in the second root buffer."""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    run = UnitCams(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n, Tt, V = 16520, 7, 2
    rest, kpj, kpo = sk.tables(parents)
    K = len(kpj)
    q = synth.make_poses(n, seed=5, signed=True, num_joints=J)
    r = np.random.RandomState(9)
    Y = np.ascontiguousarray(r.uniform(100, 500, (n, V, K, 2)), np.float32)
    conf = r.rand(n, V, K).astype(np.float32)
    conf[r.rand(n, V, K) < 0.1] = 0.0
    root = si.make_roots(n, 37)
    anchor = sr.make_anchor(root)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=sk.missing(Y, conf), conf=conf)
    path = sc.make_tables(Tt, V, Tt)
    jitter = (1.0 + 0.02 * r.randn(n, V, 16)).astype(np.float32)      # every pose another block: a block of the wrong pose shows
    per_pose = np.ascontiguousarray(sc.blocks_of(path, n) * jitter)
    call = dict(opts=dict(renormalize="unit", step_size=0.5), frames=Tt, lam=0.5, flags=sdo.FREE_ENDS, rho=si.RHO, root_weights=sc.WEIGHTS, **sc.COUPLED)
    for tables, per_frame in ((per_pose, False), (path, True)):
        out, d, E, rt, _ = run.fit10(q, steps, kp, pose_views=tables, per_frame=per_frame, root=root, root_anchor=anchor, **call)
        assert np.isfinite(out).all() and np.isfinite(E).all() and np.isfinite(rt).all() and (E > 0).any() and (rt != root).all(axis=1).any()
        blocks = sc.blocks_of(tables, n)
        for part in (slice(16373, 16394), slice(0, 14), slice(n - 7, n)):      # (16373 = 7 * 2339: whole tracks on both sides of the seam)
            track = q[part].reshape(-1, Tt, J, 4)
            want = sc.rounds(run.forward_grad, track, steps, parents, dict(kp, Y=kp["Y"][part], conf=conf[part]), blocks[part], si.RHO, None, root[part],
                             sc.WEIGHTS, sc.COUPLED, anchor[part], free_ends=True, smooth=0.5, renormalize="unit", step_size=0.5)
            for a, b, name in zip(want[:4], (out, d, E, rt), sc.NAMES):
                assert np.ascontiguousarray(a, np.float32).reshape(b[part].shape).tobytes() == b[part].tobytes(), (steps, per_frame, part, name)


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing(torch_cuda):
    sc.check_refusals(runner_of(torch_cuda, ("hand", True), "lrelu"))


@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_the_struct_without_a_table_is_the_256_byte_call(torch_cuda, case):
    sc.check_empty_struct(runner_of(torch_cuda, case, "lrelu"), case)


def test_the_persistent_engine_refuses_the_280_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 280-byte struct is
    PNDF_ERR_BAD_ARG, nothing written"""
    torch = torch_cuda
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import Engine
    import skeleton_views_oracle as sv
    eng = Engine("lrelu", precision="fp32")
    eng.load_weights(synth.make_weights(0, 2.0, 0.1))
    lib = eng.lib
    n = 8
    q = torch.from_numpy(synth.make_poses(n, seed=5)).cuda()
    out, d = torch.full_like(q, 7.0), torch.full((n,), 7.0, device="cuda:0")
    words = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    Y, E = torch.full((n, 1, 21, 2), 300.0, device="cuda:0"), torch.full((n,), 7.0, device="cuda:0")
    root = torch.from_numpy(si.make_roots(n, 37)).cuda()
    table = torch.from_numpy(np.ascontiguousarray(np.tile(sv.identity_view(), (n, 1, 1)))).cuda()
    kept = root.clone()
    rest = np.zeros((21, 3), np.float32)
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    big = big_struct(lib, Y.data_ptr(), E.data_ptr(), rest, root.data_ptr(), table.data_ptr())
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


# ------------------------------------------------------------------------------------------ 8. Python, the kernel
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_model_fit_keypoints_with_moving_cameras_on_cuda(torch_cuda, case):
    parents, sd = sko.case_network(case, "lrelu")
    check_model_fit_keypoints(cuda_model(torch_cuda, parents, "lrelu", sd), UnitCams(torch_cuda, parents, "lrelu", sd), case, "cuda")


def test_keypoint_fitting_drivers_with_a_moving_rig_on_cuda(torch_cuda):
    parents, sd = sko.case_network(("hand", True), "softplus")
    check_drivers(cuda_model(torch_cuda, parents, "softplus", sd), "cuda")


def test_the_options_keep_a_device_table_alive(torch_cuda):
    """build the options around a device tensor, drop the tensor, collect, allocate over it, call: the result is the call's with a table that
    lives"""
    import gc
    torch = torch_cuda
    from posendf_amd import engine
    case = ("hand", True)
    run = runner_of(torch, case, "lrelu")
    want = sc.make_tables(6, 2, 3)
    _, kp = sc.case_kp(case, want)
    q = sk.unit_poses(6, len(sko.SKELETONS["hand"]), 5)
    alive = run.fit10(q, 2, kp, pose_views=want, rho=si.RHO)

    def make10(at, o9):
        held = torch.from_numpy(want.copy()).cuda()
        struct = engine.project_options10(run.lib, None, 0, pose_views=held)
        del held
        gc.collect()
        junk = [torch.full((6, 2, 16), 7.0, device="cuda:0") for _ in range(64)]      # (what the caching allocator would hand out of a freed block)
        o10 = sc.c_options10(run.lib, o9, struct.pose_views, struct.n_pose_views, struct.view_flags)
        o10._owner = (struct, junk)
        return o10
    rc, out, d, E, _, _ = run.run10(q, 2, kp, pose_views=want, rho=si.RHO, make10=make10)
    assert rc == 0 and out.tobytes() == alive[0].tobytes() and E.tobytes() == alive[2].tobytes()


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_views_kernel", "pndf_skel_enc_rev_root_kernel", "pndf_skel_enc_rev_cams_kernel"} <= ch.exported_symbols(ge.LIB)
