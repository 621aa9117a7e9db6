"""Pose interpolation for other skeletons on an MI355X (pndf_project_options3 of include/posendf_amd.h, csrc/pndf_skeleton.hip; DESIGN.md
section 2j): pndf_skel_project with tracks against the numpy statement of the fill and of the band step
(tests/skeleton_interpolation_oracle.py).

1. coupling off: lambda 0 and PNDF_TRACK_GIVEN is the pndf_project_options2 call whose end-frame words are all ones, frames 0 the 32-byte
   call, bit for bit.
2. coupling on: K steps at lambda 0.5 equal K rounds of pndf_skel_forward_grad + the numpy band step, bit for bit, for every option
   set, with and without a mask; held joints keep their bits, a NaN and a zero quaternion included.  42 tracks of 7 frames = 294 lanes:
   two workgroups of the encoder kernels, track 36 across their border.
3. the fill kernel: nlerp to the bit, slerp within four times the float32 error of the formula; T = 2.
4. the refusals; the persistent engine keeps refusing the larger struct.
5. the chunk seam: T = 7 and 2,342 tracks, so a chunk holds 16,380 poses, not 16,384.
6. ten free-running steps against the fp64 oracle under conftest's outlier_gate at 1e-4.
7. `SkeletonPoseNDF.interpolate` and `PoseInterpolation` on cuda; a cuda and a cpu model under the same gate; evenness.
tests/test_skeleton_interpolation.py holds the host twin to the same statements."""
import ctypes
import functools
import math

import numpy as np
import pytest

import interpolation_oracle as io
import skeleton_completion_oracle as sco
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from conftest import outlier_gate, rel_err_rows
from posendf_amd import synth
from test_skeleton_completion_gpu import Unit, cuda_model, torch_cuda, unit_of  # noqa: F401  (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
BAD_ARG = sio.BAD_ARG
P, T, K = 42, sio.T, sio.K      # 294 poses
TOL = 1e-4
FREE_STEPS = 10


flat = sio.flat


def tracked(unit, q, steps, words, opts=None, frames=T, lam=0.0, fill=sio.GIVEN):
    rc, out, d = unit.call(q, steps, lambda at: sio.c_from(unit.lib, opts or {}, at, frames, lam, fill), words)
    assert rc == 0, unit.lib.pndf_skel_last_error(unit.h)
    return out, d


# ------------------------------------------------------------------------------------------ 1. coupling off
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_coupling_off_is_the_masked_call(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    q = flat(sio.given_track(case, P, T))
    mask = sio.case_mask(J, P, T)
    assert J < 32 or mask[1, 1, 31]
    tol = float(np.median(unit.forward(q)))
    for name in sio.OPTION_SETS:
        opts = sio.options(name, tol)
        for m in (None, mask):
            words = None if m is None else sio.pack(m)
            want, d_want = unit.masked(q, K, sio.end_words(m, J, P, T), opts)
            got, d_got = tracked(unit, q, K, words, opts)
            assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), (name, m is None)
            track, given = got.reshape(P, T, J, 4), q.reshape(P, T, J, 4)
            assert track[:, 0].tobytes() == given[:, 0].tobytes() and track[:, -1].tobytes() == given[:, -1].tobytes()
            # frames = 0: the 32-byte call
            small, d_small = unit.masked(q, K, words, opts)
            zero, d_zero = tracked(unit, q, K, words, opts, frames=0)
            assert zero.tobytes() == small.tobytes() and d_zero.tobytes() == d_small.tobytes(), (name, m is None)
    if J > 1:
        assert not np.array_equal(got, q)


# ------------------------------------------------------------------------------------------ 2. coupling on
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_coupled_steps_are_the_stated_step(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    mask = sio.case_mask(J, P, T)
    words = sio.pack(mask)
    clean = sio.given_track(case, P, T)
    odd, places = sio.odd_track(case, mask, P, T)
    tol = float(np.median(unit.forward(flat(clean))))
    held = mask.copy()
    held[:, 0] = held[:, -1] = True
    for name in sio.OPTION_SETS:
        opts = sio.options(name, tol)
        for track, m in ((clean, None), (clean, mask), (odd, mask)):
            want, dk = sio.rounds(unit.forward_grad, track, m, K, sio.LAMBDA, **opts)
            got, dl = tracked(unit, flat(track), K, None if m is None else words, opts, lam=sio.LAMBDA)
            sio.assert_same(got.reshape(track.shape), want, (name, m is None))
            sio.assert_same(dl, dk, (name, "d_last"))
            h = held if m is not None else (held & ~mask)
            assert got.reshape(track.shape)[h].tobytes() == track[h].tobytes(), name
        for at in places:      # (the odd track came last)
            assert got.reshape(odd.shape)[at].tobytes() == odd[at].tobytes()
    off, _ = tracked(unit, flat(clean), K, words, opts, lam=0.0)
    on, _ = tracked(unit, flat(clean), K, words, opts, lam=sio.LAMBDA)
    assert on.tobytes() != off.tobytes()      # the coupling does something


# ------------------------------------------------------------------------------------------ 3. the fill
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_fill(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    a, b = sio.make_pairs(case)
    x = sio.ends_of(a, b, T)
    want = sio.fill(a, b, T, "nlerp", np.float32)
    got, d = tracked(unit, flat(x), 0, None, fill=sio.NLERP)
    sio.assert_same(got.reshape(want.shape), want, "nlerp")
    assert not d.any()
    y = x.copy()      # only the end frames of the input are read
    y[:, 1:-1] = np.float32(np.nan)
    again, _ = tracked(unit, flat(y), 0, None, fill=sio.NLERP)
    assert again.tobytes() == got.tobytes()
    # slerp: within four times the float32 error of the formula on these inputs, measured here on the host
    s32, s64 = sio.fill(a, b, T, "slerp", np.float32), sio.fill(a, b, T, "slerp", np.float64)
    measured = float(np.abs(s32.astype(np.float64) - s64).max())
    sl, d = tracked(unit, flat(x), 0, None, lam=0.5, fill=sio.SLERP)
    sl = sl.reshape(s64.shape)
    err = float(np.abs(sl.astype(np.float64) - s64).max())
    print(f"[fill {sko.case_id(case)}] numpy float32 slerp against fp64 {measured:.3e}, device against fp64 {err:.3e}, bound {4 * measured:.3e}")
    assert err <= 4 * measured and not d.any()
    for out in (got.reshape(want.shape), sl):
        assert out[:, 0].tobytes() == a.tobytes() and out[:, -1].tobytes() == want[:, -1].tobytes()
    # T = 2: a and aligned b, untouched by any step
    two = sio.ends_of(a, b, 2)
    for fill in (sio.SLERP, sio.NLERP):
        for steps in (2, 3):      # both parities of the buffer swap
            out, d2 = tracked(unit, flat(two), steps, None, dict(renormalize="unit"), frames=2, lam=0.5, fill=fill)
            out = out.reshape(two.shape)
            assert out[:, 0].tobytes() == a.tobytes() and out[:, 1].tobytes() == io.align(a, b).tobytes()
            assert np.isfinite(d2).all()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing(torch_cuda):
    unit, J = unit_of(torch_cuda, ("hand", True), "lrelu")
    lib = unit.lib
    q = flat(sio.given_track(("hand", True), 2, 4))      # 8 poses
    words = np.zeros(9, np.uint32)

    def refused(make_opt, field, **kw):
        rc, out, d = unit.call(q, 2, make_opt, words, **kw)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_skel_last_error(unit.h), (field, lib.pndf_skel_last_error(unit.h))
        if kw:
            assert out.tobytes() == q.tobytes(), field
        else:
            assert np.all(out == 7.0), field
        assert np.all(d == 7.0), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 64):
        refused(lambda at, size=size: sio.c_options3(lib, at, 4, size=size), "struct_size")
    refused(lambda at: sio.c_options3(lib, at, 4, reserved2=1), "reserved2")
    for frames in (1, -1, 16385, 3, 5, 16):      # B = 8
        refused(lambda at, frames=frames: sio.c_options3(lib, at, frames), "frames")
    for lam in (-0.1, 1.5, math.nan):
        refused(lambda at, lam=lam: sio.c_options3(lib, at, 4, lam), "lambda")
    for fill in (3, -1):
        refused(lambda at, fill=fill: sio.c_options3(lib, at, 4, 0.5, fill), "fill")
    refused(lambda at: sio.c_options3(lib, at, 0, 0.5), "lambda")
    refused(lambda at: sio.c_options3(lib, at, 0, 0.0, sio.SLERP), "fill")
    refused(lambda at: sio.c_options3(lib, at, 4, 0.5), "q_out", in_place=True)
    refused(lambda at: sio.c_options3(lib, at, 4, reserved=1), "reserved")
    refused(lambda at: sio.c_options3(lib, at + 2, 4), "observed")
    for field, kw in (("step_size", dict(step_size=0.0)), ("tol", dict(tol=math.nan)), ("renorm", dict(renorm=3))):
        refused(lambda at, kw=kw: sco.c_options(lib, **kw), field)
        text = lib.pndf_skel_last_error(unit.h)
        refused(lambda at, kw=kw: sio.c_options3(lib, at, 4, **kw), field)
        assert lib.pndf_skel_last_error(unit.h) == text      # refused as in a 16-byte struct: the same text
    # q_out overlapping q_in by all but one pose
    torch = torch_cuda
    buf = torch.cat([torch.from_numpy(q), torch.full((1,) + q.shape[1:], 7.0)]).cuda()
    before = buf.cpu().numpy().copy()
    d = torch.full((8,), 7.0, device="cuda:0")
    ws, n = unit.ws(8)
    opt = sio.c_options3(lib, None, 4, 0.5)
    rc = lib.pndf_skel_project(unit.h, buf.data_ptr(), buf[1:].data_ptr(), d.data_ptr(), 8, 2, ctypes.byref(opt), ws.data_ptr(), n, unit.stream())
    torch.cuda.synchronize()
    assert rc == BAD_ARG and b"q_out" in lib.pndf_skel_last_error(unit.h)
    assert buf.cpu().numpy().tobytes() == before.tobytes() and bool((d == 7).all())
    rc, out, _ = unit.call(q, 2, lambda at: sio.c_options3(lib, at, 4, 0.5, sio.SLERP), words)
    assert rc == 0 and not np.any(out == 7.0)


def test_the_persistent_engine_refuses_the_48_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 48-byte struct is
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
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    big = sio.c_options3(lib, words.data_ptr(), 2)
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
    assert bool((out == 7).all()) and bool((d == 7).all()) and bool((track == 7).all())


# ------------------------------------------------------------------------------------------ 5. the chunk seam
def test_tracks_do_not_straddle_the_chunk_seam(torch_cuda):
    """T = 7 and P = 2,342: B = 16,394 is more than a chunk of 16,384, and the track-aligned chunk is 16,380 poses = 2,340 tracks.
    Tracks 2,339 (the last of the first chunk) and 2,340 (the first of the second) equal the same two tracks run alone; two runs of
    the big call are bit-identical."""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    unit = Unit(torch_cuda, parents, "softplus", sd, hidden=(32,))
    Pn, Tn = 2342, 7
    assert Pn * Tn == 16394 and (16384 // Tn) * Tn == 16380 == 2340 * Tn
    ends = synth.make_poses(2 * Pn, seed=5, signed=True, num_joints=J)
    x = sio.ends_of(ends[:Pn], ends[Pn:], Tn)
    mask = sio.make_mask(J, Pn, Tn)
    mask[2339, 1:-1] = mask[1, 1:-1]
    mask[2340, 1:-1] = mask[4, 1:-1]
    words = sio.pack(mask)
    opts = dict(renormalize="unit", step_size=0.5)
    for steps in (2, 3):      # both parities of the buffer swap
        out, d = tracked(unit, flat(x), steps, words, opts, frames=Tn, lam=0.5, fill=sio.SLERP)
        again, d_again = tracked(unit, flat(x), steps, words, opts, frames=Tn, lam=0.5, fill=sio.SLERP)
        assert again.tobytes() == out.tobytes() and d_again.tobytes() == d.tobytes()
        out, d = out.reshape(Pn, Tn, J, 4), d.reshape(Pn, Tn)
        assert np.isfinite(out).all() and np.isfinite(d).all()
        pair = slice(2339, 2341)
        alone, d_alone = tracked(unit, flat(x[pair]), steps, words.reshape(Pn, Tn)[pair].reshape(-1), opts, frames=Tn, lam=0.5, fill=sio.SLERP)
        assert alone.tobytes() == out[pair].tobytes() and d_alone.tobytes() == d[pair].tobytes(), steps
        first, d_first = tracked(unit, flat(x[:40]), steps, words[:40 * Tn], opts, frames=Tn, lam=0.5, fill=sio.SLERP)
        assert first.tobytes() == out[:40].tobytes() and d_first.tobytes() == d[:40].tobytes(), steps
        held = mask.copy()
        held[:, 0] = held[:, -1] = True
        start, _ = tracked(unit, flat(x), 0, None, frames=Tn, fill=sio.SLERP)
        assert out[held].tobytes() == start.reshape(out.shape)[held].tobytes() and not np.array_equal(out[~held], start.reshape(out.shape)[~held])


# ------------------------------------------------------------------------------------------ 6. free running
@functools.lru_cache(maxsize=None)
def oracle_tracks(case, act, smooth):
    """(fp64 track, fp32 track, kink margins of the interior frames along the fp64 trajectory or None) of the numpy oracle: the pairs of
    make_pairs, slerp, ten steps, unit quaternions"""
    parents, sd = sko.case_network(case, act)
    a, b = sio.make_pairs(case)
    q64, _, margin = sio.interpolate(a, b, sio.T, sd, FREE_STEPS, act, parents, smooth=smooth, dtype=np.float64, renormalize="unit")
    q32, _, _ = sio.interpolate(a, b, sio.T, sd, FREE_STEPS, act, parents, smooth=smooth, dtype=np.float32, renormalize="unit")
    margin = None if act == "softplus" else margin.reshape(sio.P, sio.T)[:, 1:-1].reshape(-1)
    return q64, q32, margin


def free_gate(got, case, act, smooth, what, ref=None):
    """conftest.outlier_gate at 1e-4 on the interior frames against the fp64 oracle track, the float32 numpy oracle's rows (or `ref`'s) as
    the reference rows.  The gate's exemption caps are conditions, not measurements: first the float32 oracle alone is shown to stay
    inside them on these inputs (finite, every row below 100 %, and through the gate against itself)."""
    q64, q32, margin = oracle_tracks(case, act, smooth)
    truth = sio.inner(q64)
    own = rel_err_rows(sio.inner(q32), truth)
    assert np.isfinite(own).all() and own.max() < 1.0, (what, float(own.max()))
    outlier_gate(own, own, TOL, f"{what}: the float32 oracle itself", margin=margin)
    mine = rel_err_rows(sio.inner(got), truth)
    rows = own if ref is None else rel_err_rows(sio.inner(ref), truth)
    print(f"[{what}] per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference rows median {np.median(rows):.2e} max {rows.max():.2e}")
    outlier_gate(mine, rows, TOL, what, margin=margin)


@pytest.mark.parametrize("smooth", (0.0, 0.5))
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(torch_cuda, case, act, smooth):
    unit, J = unit_of(torch_cuda, case, act)
    a, b = sio.make_pairs(case)
    got, d = tracked(unit, flat(sio.ends_of(a, b, sio.T)), FREE_STEPS, None, dict(renormalize="unit"), frames=sio.T, lam=smooth, fill=sio.SLERP)
    got = got.reshape(sio.P, sio.T, J, 4)
    assert got[:, 0].tobytes() == a.tobytes() and got[:, -1].tobytes() == io.align(a, b).tobytes() and np.isfinite(d).all()
    free_gate(got, case, act, smooth, f"unit {sko.case_id(case)} {act} lambda {smooth}")


# ------------------------------------------------------------------------------------------ 7. Python
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_interpolate_on_cuda(torch_cuda, case, act):
    torch = torch_cuda
    from test_skeleton_completion import cpu_model
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cuda_model(torch, parents, act, sd)
    unit = Unit(torch, parents, act, sd)
    a_np, b_np = sio.make_pairs(case)
    a, b = torch.from_numpy(a_np.copy()).cuda(), torch.from_numpy(b_np.copy()).cuda()
    mask = sio.make_mask(J)
    m = torch.from_numpy(mask)
    # the unit's bits through the C struct: one engine call
    want, d_want = tracked(unit, flat(sio.ends_of(a_np, b_np, sio.T)), K, sio.pack(mask), dict(renormalize="unit"), frames=sio.T, lam=0.5, fill=sio.SLERP)
    track, d = net.interpolate(a, b, sio.T, steps=K, smooth=0.5, observed=m)
    assert track.is_cuda and track.shape == (sio.P, sio.T, J, 4) and d.shape == (sio.P, sio.T)
    assert track.cpu().numpy().tobytes() == want.tobytes() and d.cpu().numpy().tobytes() == d_want.tobytes()
    assert track[:, 0].cpu().numpy().tobytes() == a_np.tobytes() and track[:, -1].cpu().numpy().tobytes() == io.align(a_np, b_np).tobytes()
    assert a.cpu().numpy().tobytes() == a_np.tobytes() and b.cpu().numpy().tobytes() == b_np.tobytes()      # the inputs are not written
    start = net.interpolate(a, b, sio.T, steps=0, return_dist=False)
    assert torch.equal(track.cpu()[m].view(torch.int32), start.cpu()[m].view(torch.int32))
    x, dx = net.interpolate(a, b, sio.T, steps=2, observed=m[1], mode="nlerp")
    y, dy = net.interpolate(a.cpu(), b.cpu(), sio.T, steps=2, observed=m[1].expand(sio.P, sio.T, J), mode="nlerp")
    assert torch.equal(x, y) and torch.equal(dx, dy)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again, d_again = net.interpolate(a, b, sio.T, steps=K, smooth=0.5, observed=m)
    side.synchronize()
    assert torch.equal(again.view(torch.int32), track.view(torch.int32)) and torch.equal(d_again.view(torch.int32), d.view(torch.int32))
    e, de = net.interpolate(a[:0], b[:0], sio.T, steps=2)
    assert e.shape == (0, sio.T, J, 4) and de.shape == (0, sio.T)
    # ten free-running steps: the cuda model under the gate, and against a cpu model under the same gate
    host = cpu_model(parents, act, sd)
    for smooth in (0.0, 0.5):
        dev = net.interpolate(a, b, sio.T, steps=FREE_STEPS, smooth=smooth, return_dist=False).cpu().numpy()
        cpu = host.interpolate(a.cpu(), b.cpu(), sio.T, steps=FREE_STEPS, smooth=smooth, return_dist=False).numpy()
        what = f"model {sko.case_id(case)} {act} lambda {smooth}"
        free_gate(cpu, case, act, smooth, f"cpu {what}")
        free_gate(dev, case, act, smooth, f"cuda {what}")
        free_gate(dev, case, act, smooth, f"cuda against cpu {what}", ref=cpu)


def test_pose_interpolation_driver_on_a_hand(torch_cuda):
    torch = torch_cuda
    from posendf_amd.pose_interpolation import PoseInterpolation
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cuda_model(torch, parents, "softplus", sd)
    a, b = (torch.from_numpy(x) for x in sio.make_pairs(case))
    driver = PoseInterpolation(net, body_model=None, device="cuda:0")
    track, dist, meshes = driver.interpolate(a, b, sio.T, steps=5)
    want, d_want = net.interpolate(a, b, sio.T, steps=5, smooth=0.5)
    assert track.is_cuda and track.shape == (sio.P, sio.T, J, 4) and dist.shape == (sio.P, sio.T) and not meshes
    assert torch.equal(track, want) and torch.equal(dist, d_want) and bool(torch.isfinite(dist).all())
    assert torch.equal(track[:, 0].cpu(), a)


@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_coupling_evens_the_track(torch_cuda, case, act):
    """T = 7, 50 steps, renormalize="unit", slerp: smooth=0.5 gives every pair a smaller longest-to-mean segment ratio and a shorter path
    than smooth=0 -- in the fp64 oracle first, then on the cuda model's output"""
    torch = torch_cuda
    r0, l0 = sio.oracle_evenness(case, act, 0.0)
    r5, l5 = sio.oracle_evenness(case, act, 0.5)
    assert (r5 < r0).all() and (l5 < l0).all(), (r0, r5, l0, l5)
    parents, sd = sko.case_network(case, act)
    net = cuda_model(torch, parents, act, sd)
    a, b = (torch.from_numpy(x) for x in sio.make_pairs(case))
    m0, m5 = (sio.evenness(net.interpolate(a, b, sio.T, steps=sio.EVEN_STEPS, smooth=s, return_dist=False).cpu().numpy()) for s in (0.0, 0.5))
    print(f"[evenness {sko.case_id(case)} {act}] cuda: ratio {m5[0].min():.2f} - {m5[0].max():.2f} against {m0[0].min():.2f} - {m0[0].max():.2f}, "
          f"path {m5[1].min():.1f} - {m5[1].max():.1f} against {m0[1].min():.1f} - {m0[1].max():.1f}")
    assert (m5[0] < m0[0]).all() and (m5[1] < m0[1]).all(), (m0, m5)
