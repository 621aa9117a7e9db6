"""Pose completion on the device (include/posendf_amd_completion.h; DESIGN.md section 2 "Pose completion").

9.  the step kernel alone (`pndf_complete_step`) against the numpy float32 masked step (tests/completion_oracle.py), bit for bit, on
    crafted d and dq.
10. `net.complete` against the replay -- k rounds of the engine's own forward + gradient launch with the masked step applied on the
    host --, bit for bit, on every kernel family.
11. `observed=None` against `net.project`, bit for bit, on every family; through the facade and through `pndf_complete(opt = NULL)`.
12. ten free-running masked steps against the vectors the real reference produced (tests/golden/completion.npz), under the gate of
    tests/test_project_options_gpu.py check 8; device and host twin under the same gate.
13. invariants: observed joints keep their bits, an all-observed pose is unchanged and reports its own distance.
14. the `PoseCompletion` driver, and one call on a non-default stream.

Bit for bit: equal bit patterns; where the specification gives a NaN the result is a NaN (the payload of a propagated NaN is the
processor's choice and no part of the step's definition).  Held joints are compared as bit patterns without that allowance.
"""
import ctypes
import functools

import numpy as np
import pytest

import completion_oracle as co
from conftest import outlier_gate, rel_err_rows
from test_project_options_gpu import FAMILIES, forward_grad, network, poses

pytestmark = pytest.mark.gpu
TOL = 1e-4
SETS = list(co.OPTION_SETS)


def same_bits(got, want):
    """[...] float32: equal bit patterns, or a NaN where a NaN is specified -> bool array"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what):
    ok = same_bits(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:6].tolist())


def to_device_words(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).cuda()


def median_tol(eng, q_np):
    d0, _ = forward_grad(eng, q_np)
    return float(np.median(d0[np.isfinite(d0)]))


def replay(eng, q_np, observed, steps, **opts):
    """-> {k: (q after k steps, d of step k)}: the engine's forward + gradient launch, the numpy float32 masked step on the host"""
    cur, out = np.array(q_np, np.float32).reshape(-1, 21, 4), {}
    for k in range(1, steps + 1):
        d, dq = forward_grad(eng, cur)
        cur = np.ascontiguousarray(co.step_masked(cur, d, dq, observed, **opts))
        out[k] = (cur.copy(), d.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("B", [1, 52, 65])
def test_step_kernel_equals_the_numpy_step(B):
    """9. B = 1: one lane group; B = 52: the fixture's poses; B = 65: 1365 lanes = five full blocks of 256 and a ragged sixth.
    Crafted: random d and dq, a NaN d, d on both sides of the tolerance and exactly on it, a zero quaternion with a zero gradient
    under renormalisation, a NaN and a zero quaternion in held joints.  With the mask, without one, with bits 21..31 all set."""
    import torch
    _, eng = network("fp32-lrelu")
    rng = np.random.RandomState(17 + B)
    q = poses(B).copy()
    d = np.abs(rng.randn(B)).astype(np.float32) * 0.3
    dq = rng.randn(B, 21, 4).astype(np.float32)
    mask = co.make_mask(B)
    tol = float(np.median(d))
    if B > 1:
        d[2] = np.float32(tol)                     # exactly on it: not below, so it moves
        d[3] = np.float32(np.nan)                  # never frozen
        d[4] = np.float32(0.0)                     # below any tolerance; without one the step is q - 0
        free, held = int(np.flatnonzero(~mask[5])[0]), np.flatnonzero(mask[5])
        q[5, free], dq[5, free] = 0.0, 0.0         # u = 0: the clamp keeps it zero
        q[5, held[0]] = np.float32(np.nan)         # held joints are not even read for the update
        q[5, held[1]] = 0.0
        assert (d < tol).sum() >= 5 and (d > tol).sum() >= 5
    st = torch.cuda.current_stream().cuda_stream
    d_dev, dq_dev = torch.from_numpy(d).cuda(), torch.from_numpy(dq).cuda()
    high = np.uint32(0xFFE00000)
    for name in SETS:
        step_size, renorm = co.OPTION_SETS[name]
        o = dict(step_size=step_size, renormalize=renorm, tol=tol if name == "unit_tol" else 0.0)
        for observed, words in ((mask, co.pack(mask)), (np.zeros_like(mask), None), (mask, co.pack(mask) | high),
                                (np.zeros_like(mask), np.full(B, high, np.uint32))):
            want = co.step_masked(q, d, dq, observed, **o)
            q_dev = torch.from_numpy(q.copy()).cuda()
            w_dev = None if words is None else to_device_words(words)
            eng.complete_step(q_dev.data_ptr(), d_dev.data_ptr(), dq_dev.data_ptr(), None if w_dev is None else w_dev.data_ptr(), B, st,
                              step_size=step_size, renorm=renorm, tol=o["tol"])
            got = q_dev.cpu().numpy()
            assert_same(got, want, (B, name, words is None))
            assert (got.view(np.uint32)[observed] == q.view(np.uint32)[observed]).all(), (B, name)
            if B > 1 and name == "unit_tol":
                assert got[4].tobytes() == q[4].tobytes() and got[2].tobytes() != q[2].tobytes()
            if B > 1 and renorm is not None and o["tol"] == 0.0:
                assert not got[5, free].any() and np.isnan(got[3][~observed[3]]).all()
    # the inputs of the step are read-only
    assert d_dev.cpu().numpy().tobytes() == d.tobytes() and dq_dev.cpu().numpy().tobytes() == dq.tobytes()
    # refused: nothing is written
    from posendf_amd.engine import PndfError
    q_dev = torch.full((B, 21, 4), 7.0, device="cuda:0")
    for kwargs, ptr in ((dict(step_size=0.0), q_dev.data_ptr()), (dict(tol=-1.0), q_dev.data_ptr()), ({}, q_dev.data_ptr() + 4)):
        with pytest.raises(PndfError, match="pndf_complete_step failed"):
            eng.complete_step(ptr, d_dev.data_ptr(), dq_dev.data_ptr(), None, B, st, **kwargs)
    torch.cuda.synchronize()
    assert bool((q_dev == 7.0).all())


# --------------------------------------------------------------------------------------------------------------- 10
@pytest.mark.parametrize("name", ["half_flip", "unit_tol"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_complete_equals_the_replay(family, name):
    """10. B = 52: one ragged workgroup of the fused kernels; B = 65: a second one with a single pose.  unit_tol: the median of the
    initial d on this network, so about half of the poses rest."""
    import torch
    net, eng = network(family)
    step_size, renorm = co.OPTION_SETS[name]
    for B in (52, 65):
        q_np, mask = poses(B), co.make_mask(B)
        tol = median_tol(eng, q_np) if name == "unit_tol" else 0.0
        o = dict(step_size=step_size, renormalize=renorm, tol=tol)
        want = replay(eng, q_np, mask, 3, **o)
        q = torch.from_numpy(q_np.copy()).cuda()
        for k in (1, 3):
            got, dl = net.complete(q, torch.from_numpy(mask), steps=k, **o)
            assert_same(got.cpu().numpy(), want[k][0], (family, name, B, k, "poses"))
            assert_same(dl.cpu().numpy().reshape(-1), want[k][1], (family, name, B, k, "d_last"))
            assert (got.cpu().numpy().view(np.uint32)[mask] == q_np.view(np.uint32)[mask]).all()
        assert q.cpu().numpy().tobytes() == q_np.tobytes()      # the input is not written


# --------------------------------------------------------------------------------------------------------------- 11
@pytest.mark.parametrize("family", list(FAMILIES))
def test_no_mask_is_the_projection(family):
    """11. B = 65 x 10 steps, every option set through the facade; pndf_complete with opt = NULL and observed = NULL / all-zero words
    against pndf_project; q_out aliasing q_in; a refused call leaves a 7.0-filled output untouched"""
    import torch
    from posendf_amd.engine import ProjectOptions
    net, eng = network(family)
    B = 65
    q = torch.from_numpy(poses(B)).cuda()
    for name in SETS:
        step_size, renorm = co.OPTION_SETS[name]
        o = dict(step_size=step_size, renormalize=renorm, tol=median_tol(eng, poses(B)) if name == "unit_tol" else 0.0)
        a, da = net.project(q, steps=10, **o)
        for observed in (None, torch.zeros(21, dtype=torch.bool)):
            b, db = net.complete(q, observed, steps=10, **o)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(da.view(torch.int32), db.view(torch.int32)), (family, name)
    a, da = net.project(q, steps=10)
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(eng.complete_workspace_floats(B), device="cuda:0")
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    for words in (None, zeros.data_ptr()):
        out, dl = torch.full_like(q, 7.0), torch.full((B,), 7.0, device="cuda:0")
        assert eng.lib.pndf_complete(eng.handle, q.data_ptr(), words, out.data_ptr(), dl.data_ptr(), B, 10, None, ws.data_ptr(), st) == 0
        assert torch.equal(out.view(torch.int32), a.view(torch.int32)) and torch.equal(dl.view(torch.int32), da.view(-1).view(torch.int32))
    inplace = q.clone()
    assert eng.lib.pndf_complete(eng.handle, inplace.data_ptr(), None, inplace.data_ptr(), None, B, 10, None, ws.data_ptr(), st) == 0
    assert torch.equal(inplace.view(torch.int32), a.view(torch.int32))
    # steps = 0: the poses pass through, d_last is zeroed, as pndf_project_ex
    out, dl = torch.full_like(q, 7.0), torch.full((B,), 7.0, device="cuda:0")
    assert eng.lib.pndf_complete(eng.handle, q.data_ptr(), None, out.data_ptr(), dl.data_ptr(), B, 0, None, ws.data_ptr(), st) == 0
    assert torch.equal(out.view(torch.int32), q.view(torch.int32)) and bool((dl == 0).all())
    # refused calls launch and write nothing
    bad_opt = ProjectOptions()
    eng.lib.pndf_default_project_options(ctypes.byref(bad_opt))
    bad_opt.step_size = 0.0
    out, dl = torch.full_like(q, 7.0), torch.full((B,), 7.0, device="cuda:0")
    good = dict(q=q.data_ptr(), words=zeros.data_ptr(), out=out.data_ptr(), dl=dl.data_ptr(), B=B, steps=10, opt=None, ws=ws.data_ptr())
    bad = {"options": dict(opt=ctypes.byref(bad_opt)), "null workspace": dict(ws=None), "misaligned workspace": dict(ws=ws.data_ptr() + 4),
           "null q_in": dict(q=None), "null q_out": dict(out=None), "misaligned q_out": dict(out=out.data_ptr() + 4),
           "misaligned mask": dict(words=zeros.data_ptr() + 2), "negative B": dict(B=-1), "negative steps": dict(steps=-1)}
    for what, change in bad.items():
        c = {**good, **change}
        rc = eng.lib.pndf_complete(eng.handle, c["q"], c["words"], c["out"], c["dl"], c["B"], c["steps"], c["opt"], c["ws"], st)
        assert rc == -1 and eng.lib.pndf_last_error(eng.handle), (what, rc)
    assert eng.lib.pndf_complete(eng.handle, None, None, None, None, 0, 10, None, None, st) == 0      # B = 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dl == 7.0).all())


# --------------------------------------------------------------------------------------------------------------- 12
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(co.FIXTURE))


@functools.lru_cache(maxsize=None)
def kink_margin(act, name):
    """along the MASKED fp64 trajectory; shared by the families of one activation"""
    fx = fixture()
    return co.kink_margin_along(fx["q"], co.weights(), fx["observed"], co.STEPS, act, **co.options(name, act))


@functools.lru_cache(maxsize=None)
def host_twin_result(act, name):
    from posendf_amd.engine import CpuEngine
    fx = fixture()
    host = CpuEngine(act)
    host.load_weights(co.weights())
    o = co.options(name, act)
    q0, words = np.ascontiguousarray(fx["q"]), co.pack(fx["observed"])
    twin = np.empty_like(q0)
    host.complete(q0.ctypes.data, words.ctypes.data, twin.ctypes.data, None, len(q0), co.STEPS, step_size=o["step_size"],
                  renorm=o["renormalize"], tol=o["tol"])
    return twin


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", ["fp32-lrelu", "fp32-softplus", "f16x3-lrelu", "f16x3-softplus"])
def test_ten_masked_steps_against_the_reference_run(family, name):
    """12. free running: outlier_gate on rel_err_rows at 1e-4 against the fixture's fp64 result, the fixture's own fp32 rows as the
    reference rows, the kink margins of the masked fp64 trajectory for lrelu -- gate, arguments and families of
    tests/test_project_options_gpu.py check 8"""
    import torch
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    got, _ = net.complete(torch.from_numpy(fx["q"]).cuda(), torch.from_numpy(fx["observed"]), steps=co.STEPS, **co.options(name, act))
    truth = fx[f"{act}_{name}_q10_f64"]
    mine, ref = rel_err_rows(got.cpu().numpy(), truth), rel_err_rows(fx[f"{act}_{name}_q10_f32"], truth)
    print(f"[{family} {name}] q10 per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference fp32 median {np.median(ref):.2e} max {ref.max():.2e}")
    outlier_gate(mine, ref, TOL, f"{family} {name} q10", margin=kink_margin(act, name))


@pytest.mark.parametrize("family,name", [("fp32-lrelu", "half_flip"), ("f16x3-softplus", "unit_tol")])
def test_device_and_host_twin_under_the_same_gate(family, name):
    """12. the host twin against the fixture under the gate above, and the device against the host twin (check 9 of
    tests/test_project_options_gpu.py: truth = the fixture's fp64 result)"""
    import torch
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    truth = fx[f"{act}_{name}_q10_f64"]
    twin = host_twin_result(act, name)
    margin = kink_margin(act, name)
    outlier_gate(rel_err_rows(twin, truth), rel_err_rows(fx[f"{act}_{name}_q10_f32"], truth), TOL, f"host twin {act} {name} q10", margin=margin)
    got, _ = net.complete(torch.from_numpy(fx["q"]).cuda(), torch.from_numpy(fx["observed"]), steps=co.STEPS, **co.options(name, act))
    outlier_gate(rel_err_rows(got.cpu().numpy(), truth), rel_err_rows(twin, truth), TOL, f"{family} {name} device vs host twin", margin=margin)


# --------------------------------------------------------------------------------------------------------------- 13
@pytest.mark.parametrize("family", ["f16x3-lrelu", "f16x3-softplus"])
def test_invariants_on_the_device(family):
    """13. B = 65 x 10 steps: observed joints are the input's bits (a NaN and a zero quaternion among them); the all-observed poses
    (rows 1 and 53) come back unchanged with d_last = a forward of them"""
    import torch
    net, eng = network(family)
    B = 65
    q_np, mask = poses(B).copy(), co.make_mask(B)
    nan_pose, zero_pose = 6, 7
    q_np[nan_pose, np.flatnonzero(mask[nan_pose])[0]] = np.float32(np.nan)
    q_np[zero_pose, np.flatnonzero(mask[zero_pose])[0]] = 0.0
    q = torch.from_numpy(q_np).cuda()
    d0 = net(q, train=False)["dist_pred"].cpu().numpy().reshape(-1)
    rows = np.flatnonzero(mask.all(axis=1))
    assert rows.tolist() == [co.ALL_OBSERVED, co.ALL_OBSERVED + 52]
    for name in ("plain", "half_flip", "unit_tol"):
        o = co.options(name, FAMILIES[family][1])
        got, dl = net.complete(q, torch.from_numpy(mask), steps=10, **o)
        got, dl = got.cpu().numpy(), dl.cpu().numpy().reshape(-1)
        assert (got.view(np.uint32)[mask] == q_np.view(np.uint32)[mask]).all(), (family, name)
        assert got[rows].tobytes() == q_np[rows].tobytes() and dl[rows].tobytes() == d0[rows].tobytes(), (family, name)
        others = np.arange(B) != nan_pose
        assert np.isnan(got[nan_pose][~mask[nan_pose]]).all() and np.isfinite(got[others]).all() and np.isfinite(dl[others]).all()
        free = ~mask[others]
        assert (got[others].view(np.uint32)[free] != q_np[others].view(np.uint32)[free]).any(axis=-1).mean() > (0.3 if name == "unit_tol" else 0.9)


# --------------------------------------------------------------------------------------------------------------- 14
def test_pose_completion_driver_on_the_device():
    """14. hypotheses = 4 at B = 13: 52 poses through one call; what tests/test_completion.py check 8 checks; and one call on a
    non-default stream gives the same bits"""
    import torch
    from test_completion import check_pose_completion
    net, eng = network("f16x3-lrelu")
    pc, q, m = check_pose_completion(net, "cuda:0", B=13, K=4)
    want, dwant, bwant, _ = pc.complete(q, m, hypotheses=4, generator=torch.Generator().manual_seed(9), steps=5, renormalize="unit_flip", select="best")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, dgot, bgot, _ = pc.complete(q, m, hypotheses=4, generator=torch.Generator().manual_seed(9), steps=5, renormalize="unit_flip", select="best")
    side.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(dgot.view(torch.int32), dwant.view(torch.int32))
    assert torch.equal(bgot, bwant) and bool((got[..., 0] >= 0)[~m[:, None].expand(13, 4, 21).cuda()].all())
    # with a body model (the 500-vertex synthetic one of smoke()): the meshes before / after, as SamplePose returns them
    from posendf_amd import BodyModel, PoseCompletion, synth
    from posendf_amd.sample_poses import quaternion_to_axis_angle
    bm = BodyModel(synth.make_body_model(V=500, seed=3, extra=(7, 123, 499)), device="cuda:0")
    pcb = PoseCompletion(net, body_model=bm, device="cuda:0")
    kw = dict(hypotheses=4, steps=5, renormalize="unit_flip")
    hyp, _, meshes = pcb.complete(q, m, generator=torch.Generator().manual_seed(9), **kw)
    assert torch.equal(hyp.view(torch.int32), want.view(torch.int32))
    assert meshes["vertices"].shape == meshes["vertices_init"].shape == (52, 500, 3) and meshes["pose"].shape == meshes["pose_init"].shape == (52, 69)
    assert torch.equal(meshes["pose"][:, :63], quaternion_to_axis_angle(hyp.reshape(52, 21, 4)).reshape(52, 63)) and bool(torch.isfinite(meshes["vertices"]).all())
    hyp, _, best, meshes = pcb.complete(q, m, generator=torch.Generator().manual_seed(9), select="best", **kw)
    chosen = hyp[torch.arange(13, device="cuda:0"), best]
    assert meshes["vertices"].shape == (13, 500, 3) and torch.equal(meshes["pose"][:, :63], quaternion_to_axis_angle(chosen).reshape(13, 63))
    assert not torch.equal(meshes["vertices"], meshes["vertices_init"])
