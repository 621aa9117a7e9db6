"""Pose interpolation on the device (include/posendf_amd_interpolation.h; DESIGN.md section 2 "Pose interpolation").

1. the fill kernel alone (`pndf_interp_fill`): nlerp against the numpy float32 fill (tests/interpolation_oracle.py) bit for bit,
   slerp against the fp64 evaluation of the same formula within a bound taken from the float32 error of that formula.
2. the band kernel alone (`pndf_interp_band_step`) against the numpy float32 band step, bit for bit, on crafted d and dq; pair
   isolation; lambda == 0 against `pndf_complete_step`.
3. `net.interpolate` against the replay -- the device's own nlerp fill, then k rounds of the engine's own forward + gradient launch
   with the numpy float32 band step applied on the host --, bit for bit, on every kernel family.
4. smooth = 0 against `net.complete` on the filled track with the end frames observed, bit for bit, on every family.
5. ten free-running steps against the vectors the real reference produced (tests/golden/interpolation.npz), under the gate of
   tests/test_completion_gpu.py check 12; device and host twin under the same gate.
6. the `PoseInterpolation` driver, and one call on a non-default stream.

Shapes (P, T): (1,2) no interior frame; (1,3) one; (5,7) = 735 lanes, two full blocks of 256 and a ragged third; (13,5) = 1365
lanes, and 65 poses for the engine: a full 64-pose workgroup of the fused kernels plus one pose.

Bit for bit: equal bit patterns; where the specification gives a NaN the result is a NaN.  Held quaternions are compared as bit
patterns without that allowance.
"""
import functools

import numpy as np
import pytest

import interpolation_oracle as io
from conftest import outlier_gate, rel_err_rows
from test_completion_gpu import assert_same, to_device_words
from test_project_options_gpu import FAMILIES, forward_grad, median_tol, network, poses

pytestmark = pytest.mark.gpu
TOL = 1e-4
SETS = list(io.OPTION_SETS)
SHAPES = [(1, 2), (1, 3), (5, 7), (13, 5)]
# Crafted joints of pair 0 (every shape has one): (joint, what)
SAME, OPPOSITE, ORTHOGONAL, ZERO_A, ZERO_BOTH, NAN_A = 2, 3, 4, 5, 6, 7
# Largest |float32 - float64| over the components of the slerp fill of `pairs(P)` evaluated by numpy, over SHAPES (measured on the
# host by `slerp_float32_error`, which the test repeats): the float32 error of the FORMULA on these inputs, whoever evaluates it.
# Measured: 0 at (1,2), 9.86e-08 at (1,3) and (13,5), 1.116e-07 at (5,7) -- about one ulp of 1.0.
SLERP_FLOAT32_ERROR = 1.12e-7
SLERP_DEVICE_BOUND = 4 * SLERP_FLOAT32_ERROR


@functools.lru_cache(maxsize=None)
def pairs(P):
    """(a, b) [P,21,4]: poses 0 .. P-1 and the signed poses 24 .. 24+P-1 of the projection-options inputs, with the crafted joints
    in pair 0: b == a, b == -a, b orthogonal to a (an exactly zero dot product), a zero, both zero, a NaN component in a"""
    q = poses(52)
    a, b = q[:P].copy(), q[24:24 + P].copy()
    b[0, SAME] = a[0, SAME]
    b[0, OPPOSITE] = -a[0, OPPOSITE]
    x, y, z, w = a[0, ORTHOGONAL]
    b[0, ORTHOGONAL] = (-y, x, -w, z)
    a[0, ZERO_A] = 0.0
    a[0, ZERO_BOTH] = b[0, ZERO_BOTH] = 0.0
    a[0, NAN_A, 2] = np.float32(np.nan)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def slerp_float32_error(P, T):
    """max |numpy float32 - numpy float64| over the finite components of the slerp fill of pairs(P)"""
    a, b = pairs(P)
    f32, f64 = io.fill(a, b, T, "slerp", np.float32), io.fill(a, b, T, "slerp", np.float64)
    ok = np.isfinite(f64)
    assert (np.isnan(f32) == np.isnan(f64)).all()
    return float(np.abs(f32[ok].astype(np.float64) - f64[ok]).max()) if T > 2 else 0.0


def device_fill(eng, a, b, T, mode):
    import torch
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    track = torch.full((len(a), T, 21, 4), 7.0, device="cuda:0")
    eng.interp_fill(a_dev.data_ptr(), b_dev.data_ptr(), track.data_ptr(), len(a), T, torch.cuda.current_stream().cuda_stream, mode=mode)
    out = track.cpu().numpy()
    assert a_dev.cpu().numpy().tobytes() == a.tobytes() and b_dev.cpu().numpy().tobytes() == b.tobytes()      # read-only
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("P,T", SHAPES)
def test_fill_kernel(P, T):
    """1. nlerp: the numpy float32 fill bit for bit.  Both modes: frame 0 is the bits of a, frame T-1 the bits of +-b with the
    oracle's sign; the NaN of joint NAN_A stays in that joint's track.  slerp: |device - fp64 numpy| <= SLERP_DEVICE_BOUND =
    4.48e-7, four times SLERP_FLOAT32_ERROR = 1.12e-7 -- the error of the numpy float32 evaluation of the same formula against the fp64 one on these
    inputs, measured on the host (independent of the device code; re-measured here and held to the recorded figure); the factor
    four is for the few-ulp gap between the device's sinf / atan2f and libm's.  The crafted joints whose oracle takes no
    trigonometric branch (b == a, b == -a, both zero: theta = 0) are exact, the NaN joint is NaN."""
    from posendf_amd.engine import PndfError
    import torch
    _, eng = network("fp32-lrelu")
    a, b = pairs(P)
    want = io.fill(a, b, T, "nlerp", np.float32)
    got = device_fill(eng, a, b, T, "nlerp")
    assert_same(got, want, (P, T, "nlerp"))
    measured = slerp_float32_error(P, T)
    print(f"[fill {P}x{T}] numpy float32 slerp against fp64: {measured:.3e} (recorded {SLERP_FLOAT32_ERROR:.3e}, device bound {SLERP_DEVICE_BOUND:.3e})")
    assert measured <= SLERP_FLOAT32_ERROR
    s32, s64 = io.fill(a, b, T, "slerp", np.float32), io.fill(a, b, T, "slerp", np.float64)
    sl = device_fill(eng, a, b, T, "slerp")
    for out in (got, sl):
        assert out[:, 0].view(np.uint32).tobytes() == a.view(np.uint32).tobytes()
        assert out[:, -1].view(np.uint32).tobytes() == want[:, -1].view(np.uint32).tobytes()
        assert np.isnan(out[0, 1:-1, NAN_A]).all()
        rest = np.ones((P, T, 21), bool)
        rest[0, :, NAN_A] = False
        assert np.isfinite(out[rest]).all()
    ok = np.isfinite(s64)
    err = float(np.abs(sl[ok].astype(np.float64) - s64[ok]).max())
    print(f"[fill {P}x{T}] device slerp against fp64: {err:.3e}")
    assert err <= SLERP_DEVICE_BOUND
    for j in (SAME, OPPOSITE, ZERO_BOTH):
        assert sl[0, :, j].tobytes() == s32[0, :, j].tobytes(), j
    assert not sl[0, :, ZERO_BOTH].any()
    # refused: nothing is written
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(a).cuda()
    track = torch.full((P, T, 21, 4), 7.0, device="cuda:0")
    for args in ((x.data_ptr(), x.data_ptr(), track.data_ptr() + 4, P, T), (x.data_ptr() + 8, x.data_ptr(), track.data_ptr(), P, T),
                 (x.data_ptr(), None, track.data_ptr(), P, T), (x.data_ptr(), x.data_ptr(), track.data_ptr(), P, 1),
                 (x.data_ptr(), x.data_ptr(), track.data_ptr(), -1, T)):
        with pytest.raises(PndfError, match="pndf_interp_fill failed"):
            eng.interp_fill(*args, st)
    assert eng.lib.pndf_interp_fill(x.data_ptr(), x.data_ptr(), track.data_ptr(), P, T, 2, st) == -1
    torch.cuda.synchronize()
    assert bool((track == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 2
def band_inputs(P, T):
    """-> q [P,T,21,4] (the nlerp fill of pairs(P), jittered so that no frame is special), d [P*T], dq, mask [P,T,21], tol, and
    the crafted places {name: index}"""
    rng = np.random.RandomState(23 + 100 * P + T)
    a, b = pairs(P)
    a, b = a.copy(), b.copy()
    a[0, NAN_A] = poses(52)[0, NAN_A]      # (the NaNs of this check are placed below)
    q = io.fill(a, b, T, "nlerp", np.float32) + (0.05 * rng.randn(P, T, 21, 4)).astype(np.float32)
    B = P * T
    d = (np.abs(rng.randn(B)) * 0.3).astype(np.float32)
    dq = rng.randn(P, T, 21, 4).astype(np.float32)
    mask = io.make_mask(P, T)
    if P > 1:      # make_mask observes pairs 1 and 4; (13,5) and (5,7) have both
        assert mask[1, 1:-1].any() and mask[4, 1:-1].any()
    else:
        mask[0, 1:-1] = np.random.RandomState(7).rand(T - 2, 21) < 1.0 / 3.0
    tol = float(np.median(d))
    where = {}
    if T >= 5:
        f = lambda p, k: p * T + k      # noqa: E731
        d[f(0, 1)] = np.float32(tol)               # exactly on it: not below, so it moves
        d[f(0, 2)] = np.float32(np.nan)            # never frozen
        d[f(0, 3)] = np.float32(0.0)               # below any tolerance; without one the step is q - 0
        free = int(np.flatnonzero(~mask[1, 2])[0])
        q[1, 2, free], dq[1, 2, free] = 0.0, 0.0   # u = 0 (+ the coupling): the clamp keeps a zero quaternion zero
        held = np.flatnonzero(mask[1, 1])
        q[1, 1, held[0]] = np.float32(np.nan)      # a held joint is copied, whatever it holds
        q[2, 0, 9] = np.float32(np.nan)            # an end frame likewise; its neighbour reads it only when lambda > 0
        q[2, T - 1, 10, 3] = np.float32(np.nan)
        where = dict(on_tol=f(0, 1), nan_d=f(0, 2), zero_d=f(0, 3), zero_quat=(1, 2, free), held_nan=(1, 1, int(held[0])))
        assert (d < tol).sum() >= 5 and (d > tol).sum() >= 5
    return np.ascontiguousarray(q), d, dq, mask, tol, where


@pytest.mark.parametrize("P,T", SHAPES)
def test_band_kernel_equals_the_numpy_step(P, T):
    """2. every option set x lambda in {0, 0.5, 1} x {mask, no mask, mask with bits 21..31 set, no mask with only those bits}.
    Crafted (T >= 5): d exactly on the tolerance, NaN and 0; a zero quaternion with a zero gradient; a NaN in a held joint and in
    both end frames of a pair (with lambda == 0 it reaches no other quaternion).  (1,2): the output is the input."""
    import torch
    from posendf_amd.engine import PndfError
    _, eng = network("fp32-lrelu")
    q, d, dq, mask, tol, where = band_inputs(P, T)
    B = P * T
    st = torch.cuda.current_stream().cuda_stream
    q_dev, d_dev, dq_dev = torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(dq).cuda()
    high = np.uint32(0xFFE00000)
    none = np.zeros_like(mask)
    ends = np.zeros_like(mask)
    ends[:, 0] = ends[:, -1] = True

    def run(lam, words, o, src=q_dev):
        out = torch.full((P, T, 21, 4), 7.0, device="cuda:0")
        w_dev = None if words is None else to_device_words(words)
        eng.interp_band_step(src.data_ptr(), out.data_ptr(), d_dev.data_ptr(), dq_dev.data_ptr(), None if w_dev is None else w_dev.data_ptr(),
                             P, T, st, smooth=lam, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
        return out.cpu().numpy()

    for name in SETS:
        step_size, renorm = io.OPTION_SETS[name]
        o = dict(step_size=step_size, renormalize=renorm, tol=tol if name == "unit_tol" else 0.0)
        for lam in (0.0, 0.5, 1.0):
            for observed, words in ((mask, io.pack(mask)), (none, None), (mask, io.pack(mask) | high), (none, np.full(B, high, np.uint32))):
                want = io.band_step(q, d, dq, observed, lam, **o)
                got = run(lam, words, o)
                assert_same(got, want, (P, T, name, lam, words is None))
                held = observed | ends
                assert (got.view(np.uint32)[held] == q.view(np.uint32)[held]).all(), (P, T, name, lam)
                if T == 2:
                    assert got.tobytes() == q.tobytes()
                if where and name == "unit_tol":
                    k = where["zero_d"] % T
                    assert (got[0, k][~observed[0, k]] == q[0, k][~observed[0, k]]).all()      # rests
                    k = where["on_tol"] % T
                    assert (got[0, k] != q[0, k]).any()                                          # moves
                if where and lam == 0.0:
                    k = where["nan_d"] % T      # a NaN d is never below the tolerance: the free joints of its frame take the NaN
                    assert np.isnan(got[0, k][~observed[0, k]]).all()
                    quiet = np.ones((P, T, 21), bool)      # ... and no NaN leaves the quaternion it was put in
                    quiet[0, k] = False
                    quiet[2, 0, 9] = quiet[2, T - 1, 10] = quiet[where["held_nan"]] = False
                    assert np.isfinite(got[quiet]).all(), (name, words is None)
                    assert not got[where["zero_quat"]].any()      # 0 - step_size (d 0) = 0, and 0 / 1e-12 = 0
        # lambda == 0: pndf_complete_step on the same buffers with the end frames observed as well
        for observed in (mask, none):
            inplace = torch.from_numpy(q.copy()).cuda()
            w_dev = to_device_words(io.pack(observed | ends))
            eng.complete_step(inplace.data_ptr(), d_dev.data_ptr(), dq_dev.data_ptr(), w_dev.data_ptr(), B, st, step_size=o["step_size"],
                              renorm=o["renormalize"], tol=o["tol"])
            assert_same(run(0.0, None if observed is none else io.pack(observed), o), inplace.cpu().numpy(), (P, T, name, "complete_step"))
    # pair isolation: every frame of pair 3 changed, the output bits of pairs 2 and 4 are not
    if P >= 5:
        o = dict(step_size=0.5, renormalize="unit_flip", tol=0.0)
        base = run(0.5, io.pack(mask), o)
        q2 = q.copy()
        q2[3] = poses(52)[30:30 + T] * np.float32(-1.5)
        other = run(0.5, io.pack(mask), o, src=torch.from_numpy(q2).cuda())
        assert other[[2, 4]].view(np.uint32).tobytes() == base[[2, 4]].view(np.uint32).tobytes()
        assert other[3].tobytes() != base[3].tobytes() and other[:3].view(np.uint32).tobytes() == base[:3].view(np.uint32).tobytes()
    # the inputs of the step are read-only
    assert q_dev.cpu().numpy().view(np.uint32).tobytes() == q.view(np.uint32).tobytes()
    assert d_dev.cpu().numpy().view(np.uint32).tobytes() == d.view(np.uint32).tobytes() and dq_dev.cpu().numpy().tobytes() == dq.tobytes()
    # refused: nothing is written
    out = torch.full((P, T, 21, 4), 7.0, device="cuda:0")
    good = dict(q=q_dev.data_ptr(), out=out.data_ptr(), d=d_dev.data_ptr(), dq=dq_dev.data_ptr(), P=P, T=T, kw={})
    bad = {"q_out == q_in": dict(q=out.data_ptr()), "misaligned q_out": dict(out=out.data_ptr() + 4), "null d": dict(d=None),
           "misaligned dq": dict(dq=dq_dev.data_ptr() + 8), "T = 1": dict(T=1), "negative P": dict(P=-1), "lambda > 1": dict(kw=dict(smooth=1.5)),
           "lambda < 0": dict(kw=dict(smooth=-0.5)), "lambda NaN": dict(kw=dict(smooth=float("nan"))), "step_size 0": dict(kw=dict(step_size=0.0)),
           "tol < 0": dict(kw=dict(tol=-1.0))}
    for what, change in bad.items():
        c = {**good, **change}
        with pytest.raises(PndfError, match="pndf_interp_band_step failed"):
            eng.interp_band_step(c["q"], c["out"], c["d"], c["dq"], None, c["P"], c["T"], st, **c["kw"])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 3
def replay(eng, track0, observed, steps, smooth, **opts):
    """-> {k: (track after k steps, d of step k)}: the engine's forward + gradient launch, the numpy float32 band step on the host"""
    cur, out = np.array(track0, np.float32), {}
    for k in range(1, steps + 1):
        d, dq = forward_grad(eng, cur.reshape(-1, 21, 4))
        cur = np.ascontiguousarray(io.band_step(cur, d, dq, observed, smooth, **opts))
        out[k] = (cur.copy(), d.copy())
    return out


def clean_pairs(P):
    """pairs(P) without the NaN component (a NaN joint poisons the distance of its whole pose)"""
    a, b = pairs(P)
    a = a.copy()
    a[0, NAN_A] = poses(52)[0, NAN_A]
    return a, b


@pytest.mark.parametrize("smooth", io.SMOOTHS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_interpolate_equals_the_replay(family, smooth):
    """3. P x T = 13 x 5 = 65 poses, steps 1, 2, 3 (both parities of the buffer swap), the option set half_flip without a mask and
    unit_tol (the median of the initial d on this network) with one; the inputs are not written; a non-default stream gives the
    same bits"""
    import torch
    net, eng = network(family)
    P, T = 13, 5
    a_np, b_np = clean_pairs(P)
    a, b = torch.from_numpy(a_np.copy()).cuda(), torch.from_numpy(b_np.copy()).cuda()
    fill = device_fill(eng, a_np, b_np, T, "nlerp")
    assert_same(fill, io.fill(a_np, b_np, T, "nlerp", np.float32), (family, "fill"))
    start, d0 = net.interpolate(a, b, T, steps=0, mode="nlerp")
    assert start.cpu().numpy().tobytes() == fill.tobytes() and not bool(d0.any())
    mask = io.make_mask(P, T)
    for name, m in (("half_flip", None), ("unit_tol", mask)):
        step_size, renorm = io.OPTION_SETS[name]
        o = dict(step_size=step_size, renormalize=renorm, tol=median_tol(eng, fill.reshape(-1, 21, 4)) if name == "unit_tol" else 0.0)
        want = replay(eng, fill, m, 3, smooth, **o)
        obs = None if m is None else torch.from_numpy(m)
        for k in (1, 2, 3):
            got, dl = net.interpolate(a, b, T, steps=k, smooth=smooth, mode="nlerp", observed=obs, **o)
            assert_same(got.cpu().numpy(), want[k][0], (family, name, smooth, k, "track"))
            assert_same(dl.cpu().numpy().reshape(-1), want[k][1], (family, name, smooth, k, "d_last"))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again, dl2 = net.interpolate(a, b, T, steps=3, smooth=smooth, mode="nlerp", observed=obs, **o)
        side.synchronize()
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)) and torch.equal(dl2.view(torch.int32), dl.view(torch.int32))
    assert a.cpu().numpy().tobytes() == a_np.tobytes() and b.cpu().numpy().tobytes() == b_np.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", list(FAMILIES))
def test_no_coupling_is_the_completion(family):
    """4. smooth = 0 at 13 x 5 x 10 steps: `net.complete` on the filled track (the default slerp fill) with the end frames
    observed -- and, with a mask, its joints as well --, bit for bit, for every option set; refused calls write nothing"""
    import torch
    net, eng = network(family)
    P, T = 13, 5
    a_np, b_np = clean_pairs(P)
    a, b = torch.from_numpy(a_np).cuda(), torch.from_numpy(b_np).cuda()
    fill = net.interpolate(a, b, T, steps=0, return_dist=False)
    ends = torch.zeros(P, T, 21, dtype=torch.bool)
    ends[:, 0] = ends[:, -1] = True
    mask = torch.from_numpy(io.make_mask(P, T))
    tol = median_tol(eng, fill.cpu().numpy().reshape(-1, 21, 4))
    for name in SETS:
        step_size, renorm = io.OPTION_SETS[name]
        o = dict(step_size=step_size, renormalize=renorm, tol=tol if name == "unit_tol" else 0.0)
        for m in (None, mask):
            want, dw = net.complete(fill.reshape(-1, 21, 4), (ends if m is None else ends | m).reshape(-1, 21), steps=10, **o)
            got, dg = net.interpolate(a, b, T, steps=10, smooth=0.0, observed=m, **o)
            assert torch.equal(got.reshape(-1, 21, 4).view(torch.int32), want.view(torch.int32)), (family, name, m is None)
            assert torch.equal(dg.reshape(-1).view(torch.int32), dw.reshape(-1).view(torch.int32)), (family, name, m is None)
    # refused calls launch and write nothing
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(eng.interpolate_workspace(P, T), device="cuda:0")
    out, dl = torch.full((P, T, 21, 4), 7.0, device="cuda:0"), torch.full((P * T,), 7.0, device="cuda:0")
    words = torch.zeros(P * T, dtype=torch.int32, device="cuda:0")
    good = dict(a=a.data_ptr(), b=b.data_ptr(), words=words.data_ptr(), out=out.data_ptr(), dl=dl.data_ptr(), P=P, T=T, mode=0, steps=3, lam=0.5,
                ws=ws.data_ptr())
    bad = {"null workspace": dict(ws=None), "misaligned workspace": dict(ws=ws.data_ptr() + 4), "null a": dict(a=None), "null b": dict(b=None),
           "null track": dict(out=None), "misaligned track": dict(out=out.data_ptr() + 4), "misaligned mask": dict(words=words.data_ptr() + 2),
           "misaligned d_last": dict(dl=dl.data_ptr() + 2), "negative P": dict(P=-1), "T = 1": dict(T=1), "negative steps": dict(steps=-1),
           "mode 2": dict(mode=2), "lambda > 1": dict(lam=1.5), "lambda NaN": dict(lam=float("nan")),
           "P * T too large": dict(P=((0x7fffffff * 256) // 21) // T + 1)}
    for what, change in bad.items():
        c = {**good, **change}
        rc = eng.lib.pndf_interpolate(eng.handle, c["a"], c["b"], c["words"], c["out"], c["dl"], c["P"], c["T"], c["mode"], c["steps"], c["lam"],
                                      None, c["ws"], st)
        assert rc == -1 and eng.lib.pndf_last_error(eng.handle), (what, rc)
    assert eng.lib.pndf_interpolate(eng.handle, None, None, None, None, None, 0, T, 0, 3, 0.5, None, None, st) == 0      # P = 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dl == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 5
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(io.FIXTURE))


def inner(track):
    return np.asarray(track)[:, 1:-1].reshape(-1, 84)


@functools.lru_cache(maxsize=None)
def kink_margin(act, name, smooth):
    """along the fp64 trajectory of the band, interior frames; shared by the families of one activation"""
    fx = fixture()
    m = io.kink_margin_along(io.fill(fx["a"], fx["b"], io.T, "slerp", np.float64), io.weights(), io.STEPS, act, smooth=smooth, **io.options(name, act))
    return None if m is None else m.reshape(io.P, io.T)[:, 1:-1].reshape(-1)


@functools.lru_cache(maxsize=None)
def host_twin_result(act, name, smooth):
    from posendf_amd.engine import CpuEngine
    fx = fixture()
    host = CpuEngine(act)
    host.load_weights(io.weights())
    o = io.options(name, act)
    a, b = np.ascontiguousarray(fx["a"]), np.ascontiguousarray(fx["b"])
    twin = np.empty((io.P, io.T, 21, 4), np.float32)
    host.interpolate(a.ctypes.data, b.ctypes.data, None, twin.ctypes.data, None, io.P, io.T, io.STEPS, smooth=smooth, step_size=o["step_size"],
                     renorm=o["renormalize"], tol=o["tol"])
    return twin


@pytest.mark.parametrize("smooth", io.SMOOTHS)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", ["fp32-lrelu", "fp32-softplus", "f16x3-lrelu", "f16x3-softplus"])
def test_ten_steps_against_the_reference_run(family, name, smooth):
    """5. free running, the default slerp fill: outlier_gate on rel_err_rows at 1e-4 against the fixture's fp64 result, the
    fixture's own fp32 rows as the reference rows (they pass their own gate on these pairs: tests/test_interpolation.py check 2),
    the kink margins of the band's fp64 trajectory for lrelu -- the gate of tests/test_completion_gpu.py check 12.  The rows are
    the interior frames; the end frames are the inputs' bits."""
    import torch
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    k = f"{act}_{name}_s{int(smooth * 10)}"
    got, _ = net.interpolate(torch.from_numpy(fx["a"]).cuda(), torch.from_numpy(fx["b"]).cuda(), io.T, steps=io.STEPS, smooth=smooth, **io.options(name, act))
    got = got.cpu().numpy()
    truth = fx[f"{k}_q10_f64"].reshape(-1, 84)
    mine, ref = rel_err_rows(inner(got), truth), rel_err_rows(fx[f"{k}_q10_f32"].reshape(-1, 84), truth)
    print(f"[{family} {k}] q10 per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference fp32 median {np.median(ref):.2e} max {ref.max():.2e}")
    outlier_gate(mine, ref, TOL, f"{family} {k} q10", margin=kink_margin(act, name, smooth))
    assert got[:, 0].tobytes() == fx["a"].tobytes() and np.array_equal(np.abs(got[:, -1]), np.abs(fx["b"]))


@pytest.mark.parametrize("family,name,smooth", [("fp32-lrelu", "half_flip", 0.5), ("f16x3-softplus", "unit_tol", 0.0), ("f16x3-lrelu", "unit", 0.5)])
def test_device_and_host_twin_under_the_same_gate(family, name, smooth):
    """5. the host twin against the fixture under the gate above, and the device against the host twin (truth = the fixture's
    fp64 result)"""
    import torch
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    k = f"{act}_{name}_s{int(smooth * 10)}"
    truth = fx[f"{k}_q10_f64"].reshape(-1, 84)
    twin = host_twin_result(act, name, smooth)
    margin = kink_margin(act, name, smooth)
    outlier_gate(rel_err_rows(inner(twin), truth), rel_err_rows(fx[f"{k}_q10_f32"].reshape(-1, 84), truth), TOL, f"host twin {k} q10", margin=margin)
    got, _ = net.interpolate(torch.from_numpy(fx["a"]).cuda(), torch.from_numpy(fx["b"]).cuda(), io.T, steps=io.STEPS, smooth=smooth, **io.options(name, act))
    outlier_gate(rel_err_rows(inner(got.cpu().numpy()), truth), rel_err_rows(inner(twin), truth), TOL, f"{family} {k} device vs host twin", margin=margin)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_pose_interpolation_driver_on_the_device():
    """6. (P, T) = (4, 9): what tests/test_interpolation.py check 8 checks; one call on a non-default stream gives the same bits;
    with a body model the meshes of the filled and of the relaxed track"""
    import torch
    from test_interpolation import check_pose_interpolation
    net, _ = network("f16x3-lrelu")
    pi, a, b = check_pose_interpolation(net, "cuda:0", P=4, T=9)
    want, dwant, _ = pi.interpolate(a, b, 9, steps=5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, dgot, _ = pi.interpolate(a, b, 9, steps=5)
    side.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(dgot.view(torch.int32), dwant.view(torch.int32))
    from posendf_amd import BodyModel, PoseInterpolation, synth
    from posendf_amd.sample_poses import quaternion_to_axis_angle
    bm = BodyModel(synth.make_body_model(V=500, seed=3, extra=(7, 123, 499)), device="cuda:0")
    track, _, meshes = PoseInterpolation(net, body_model=bm, device="cuda:0").interpolate(a, b, 9, steps=5)
    assert torch.equal(track.view(torch.int32), want.view(torch.int32))
    assert meshes["vertices"].shape == meshes["vertices_init"].shape == (36, 500, 3) and meshes["pose"].shape == meshes["pose_init"].shape == (36, 69)
    assert torch.equal(meshes["pose"][:, :63], quaternion_to_axis_angle(track.reshape(36, 21, 4)).reshape(36, 63))
    assert bool(torch.isfinite(meshes["vertices"]).all()) and not torch.equal(meshes["vertices"], meshes["vertices_init"])
