"""Pose interpolation on the host (include/posendf_amd_interpolation.h; DESIGN.md section 2 "Pose interpolation"): the fill and the
band step in numpy (tests/interpolation_oracle.py) against the vectors the real reference produced with the two restated around it
(tests/golden/make_golden_interpolation.py), the host twin `pndf_interpolate_cpu` bit for bit against a replay around
`pndf_forward_grad_cpu`, no coupling == `pndf_complete_cpu` with the end frames observed, the validation, the companion header
against its signature table, and the `PoseInterpolation` driver.  Runs without a GPU; tests/test_interpolation_gpu.py holds the
device to the same."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cabi_headers as ch
import interpolation_oracle as io
from conftest import outlier_gate, rel_err_rows
from test_completion import cpu_engine, cpu_net

TOL = 1e-4
SETS = list(io.OPTION_SETS)
HEADER = "posendf_amd_interpolation.h"
P, T = io.P, io.T


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(io.FIXTURE))


@pytest.fixture(scope="module")
def sd():
    return io.weights()


def inner(track):
    """[P,T,21,4] -> the interior frames as rows [P*(T-2), 84] (what the fixture stores)"""
    track = np.asarray(track)
    return track[:, 1:-1].reshape(-1, 84)


def key(act, name, smooth):
    return f"{act}_{name}_s{int(smooth * 10)}"


def run_twin(eng, a, b, T, steps, observed=None, mode="nlerp", smooth=0.0, **o):
    """pndf_interpolate_cpu through CpuEngine.interpolate -> (track [P,T,21,4], d_last [P*T]); observed: bool [P,T,21] or None"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    track, dl = np.full((len(a), T, 21, 4), 7.0, np.float32), np.full(len(a) * T, 7.0, np.float32)
    words = None if observed is None else io.pack(observed)
    eng.interpolate(a.ctypes.data, b.ctypes.data, None if words is None else words.ctypes.data, track.ctypes.data, dl.ctypes.data, len(a), T,
                    steps, mode=mode, smooth=smooth, step_size=o.get("step_size", 1.0), renorm=o.get("renormalize"), tol=o.get("tol", 0.0))
    return track, dl


def test_fixture_inputs_are_the_helper_s(fixture):
    io.check_inputs()
    a, b = io.make_pairs()
    assert np.array_equal(fixture["a"], a) and np.array_equal(fixture["b"], b) and int(fixture["frames"]) == T
    assert io.pack(io.make_mask()).shape == (P * T,) and (io.pack(io.make_mask()) >> 21 == 0).all()
    for act in io.ACTS:
        assert float(fixture[f"tol_{act}"]) == io.options("unit_tol", act)["tol"]


def test_fill_oracle_equals_the_reference_run(fixture):
    """1. the slerp fill: the fp64 helper against the torch restatement to rounding; the float32 helper within the float32 error
    of the formula (sin / atan2 of numpy against torch's: a few ulp of operands of order one); the nlerp fill is unit, starts at
    a and ends at +-b"""
    a, b = io.make_pairs()
    f64 = io.fill(a, b, T, "slerp", np.float64)
    assert np.abs(inner(f64) - fixture["fill_f64"].reshape(-1, 84)).max() <= 1e-14
    f32 = io.fill(a, b, T, "slerp", np.float32)
    assert f32.dtype == np.float32 and np.abs(inner(f32) - fixture["fill_f32"].reshape(-1, 84)).max() <= 16 * 2.0 ** -24
    for mode in ("slerp", "nlerp"):
        t = io.fill(a, b, T, mode, np.float32)
        assert t[:, 0].tobytes() == a.tobytes() and np.array_equal(np.abs(t[:, -1]), np.abs(b)) and (t[:, -1] != b).any()
        assert np.abs(np.linalg.norm(t[:, 1:-1].astype(np.float64), axis=-1) - 1).max() <= 2 * 2.0 ** -23
    # the two modes agree to second order in the angle step and are evenly spaced to within the chord / arc difference
    seg = io.segment_lengths(f64)
    assert np.abs(seg / seg.mean(axis=1, keepdims=True) - 1).max() < 1e-6


@pytest.mark.parametrize("smooth", io.SMOOTHS)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("act", io.ACTS)
def test_oracle_equals_the_reference_run(fixture, sd, act, name, smooth):
    """2. fp64: the helper IS the reference-run band to rounding (1e-12 relative); fp32: outlier_gate against the fixture's fp64
    result with the fixture's own fp32 rows as the reference rows -- which pass their own gate on these pairs"""
    o, a, b = io.options(name, act), fixture["a"], fixture["b"]
    k = key(act, name, smooth)
    _, tr64, s64 = io.interpolate(a, b, T, sd, 10, act, smooth=smooth, dtype=np.float64, snap_at=(1, 10), **o)
    for step in (1, 10):
        if f"{k}_q{step}_f64" not in fixture:
            assert step == 1 and smooth == 0
            continue
        truth = fixture[f"{k}_q{step}_f64"].reshape(-1, 84)
        err = float(rel_err_rows(inner(s64[step]), truth, floor_frac=0.0).max())
        print(f"[oracle f64 {k}] q{step} worst per-pose relative error {err:.2e}")
        assert err <= 1e-12, (step, err)
    t64 = fixture[f"{k}_dtrace_f64"]
    assert np.abs(tr64.reshape(10, P, T)[:, :, 1:-1] - t64).max() <= 1e-12 * np.abs(t64).max()
    truth = fixture[f"{k}_q10_f64"].reshape(-1, 84)
    ref = rel_err_rows(fixture[f"{k}_q10_f32"].reshape(-1, 84), truth)
    print(f"[reference fp32 {k}] q10 per-pose error: median {np.median(ref):.2e} max {ref.max():.2e}")
    margin = io.kink_margin_along(io.fill(a, b, T, "slerp", np.float64), sd, 10, act, smooth=smooth, **o)
    margin = None if margin is None else margin.reshape(P, T)[:, 1:-1].reshape(-1)
    outlier_gate(ref, ref, TOL, f"reference fp32 {k} q10", margin=margin)
    out32, _, _ = io.interpolate(a, b, T, sd, 10, act, smooth=smooth, dtype=np.float32, **o)
    assert out32.dtype == np.float32
    outlier_gate(rel_err_rows(inner(out32), truth), ref, TOL, f"oracle f32 {k} q10", margin=margin)
    # the host twin (slerp, the default) under the same gate
    twin, _ = run_twin(cpu_engine(act, sd), a, b, T, 10, mode="slerp", smooth=smooth, **o)
    outlier_gate(rel_err_rows(inner(twin), truth), ref, TOL, f"host twin {k} q10", margin=margin)
    assert twin[:, 0].tobytes() == a.tobytes() and twin[:, -1].tobytes() == out32[:, -1].tobytes()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("smooth", io.SMOOTHS)
@pytest.mark.parametrize("act", io.ACTS)
def test_host_twin_equals_the_replay_bit_for_bit(sd, act, smooth, masked):
    """3. pndf_interpolate_cpu(nlerp) == the numpy float32 fill, then `steps` rounds of pndf_forward_grad_cpu + band_step in numpy
    float32, for 0, 1, 2 and 3 steps (both parities of the buffer swap) and every option set"""
    eng = cpu_engine(act, sd)
    a, b = io.make_pairs()
    m = io.make_mask() if masked else None
    fill = io.fill(a, b, T, "nlerp", np.float32)
    B = P * T
    for name in SETS:
        o = io.options(name, act)
        cur, d = fill.copy(), np.zeros(B, np.float32)
        track, dl = run_twin(eng, a, b, T, 0, m, smooth=smooth, **o)
        assert track.tobytes() == fill.tobytes() and not dl.any(), name
        for steps in (1, 2, 3):
            dq = np.empty_like(cur)
            eng.forward_grad(cur.ctypes.data, None, d.ctypes.data, dq.ctypes.data, B)
            cur = np.ascontiguousarray(io.band_step(cur, d, dq, m, smooth, **o))
            track, dl = run_twin(eng, a, b, T, steps, m, smooth=smooth, **o)
            assert track.tobytes() == cur.tobytes(), (name, steps, int((track.view(np.uint32) != cur.view(np.uint32)).sum()))
            assert dl.tobytes() == d.tobytes(), (name, steps)
            if masked:
                assert (track.view(np.uint32)[m] == fill.view(np.uint32)[m]).all()


@pytest.mark.parametrize("act", io.ACTS)
def test_no_coupling_is_the_completion(sd, act):
    """4. smooth = 0, no mask: bit-equal to pndf_complete_cpu on the filled track with frames 0 and T-1 fully observed; with a
    mask: with the mask's joints observed as well.  Through the C ABI and through PoseNDF.interpolate on a cpu config."""
    eng = cpu_engine(act, sd)
    net = cpu_net(act, sd)
    a, b = io.make_pairs()
    ends = np.zeros((P, T, 21), bool)
    ends[:, 0] = ends[:, -1] = True
    for mode in ("nlerp", "slerp"):
        fill, _ = run_twin(eng, a, b, T, 0, mode=mode)
        for name in SETS:
            o = io.options(name, act)
            for m in (None, io.make_mask()):
                words = io.pack(ends if m is None else (ends | m))
                want, dw = np.empty_like(fill), np.empty(P * T, np.float32)
                eng.complete(fill.ctypes.data, words.ctypes.data, want.ctypes.data, dw.ctypes.data, P * T, 10, step_size=o["step_size"],
                             renorm=o["renormalize"], tol=o["tol"])
                track, dl = run_twin(eng, a, b, T, 10, m, mode=mode, smooth=0.0, **o)
                assert track.tobytes() == want.tobytes() and dl.tobytes() == dw.tobytes(), (mode, name, m is None)
                got, dg = net.interpolate(torch.from_numpy(a), torch.from_numpy(b), T, steps=10, mode=mode,
                                          observed=None if m is None else torch.from_numpy(m), **o)
                assert got.shape == (P, T, 21, 4) and dg.shape == (P, T)
                assert got.numpy().tobytes() == want.tobytes() and dg.numpy().tobytes() == dw.tobytes(), (mode, name)


def test_bad_arguments_are_refused(sd):
    """5. each bad argument: PNDF_ERR_BAD_ARG, a text, and untouched output buffers"""
    from posendf_amd.engine import PndfError, ProjectOptions
    eng = cpu_engine("lrelu", sd)
    lib = eng.lib
    a, b = io.make_pairs()
    words = io.pack(io.make_mask())

    def c_options(step_size=1.0, renorm=0, tol=0.0, size=None):
        o = ProjectOptions()
        lib.pndf_default_project_options(ctypes.byref(o))
        o.step_size, o.renorm, o.tol = step_size, renorm, tol
        if size is not None:
            o.struct_size = size
        return o

    out, dl = np.full((P, T, 21, 4), 7.0, np.float32), np.full(P * T, 7.0, np.float32)
    good = dict(a=a.ctypes.data, b=b.ctypes.data, obs=words.ctypes.data, out=out.ctypes.data, dl=dl.ctypes.data, P=P, T=T, mode=1, steps=2,
                lam=0.5, opt=None)
    big = ((0x7fffffff * 256) // 21) // T + 1
    bad = {"struct_size 0": dict(opt=c_options(size=0)), "step_size 0": dict(opt=c_options(step_size=0.0)),
           "step_size NaN": dict(opt=c_options(step_size=math.nan)), "tol < 0": dict(opt=c_options(tol=-1e-3)),
           "renorm 3": dict(opt=c_options(renorm=3)), "null a": dict(a=None), "null b": dict(b=None), "null track": dict(out=None),
           "misaligned a": dict(a=a.ctypes.data + 2), "misaligned b": dict(b=b.ctypes.data + 1), "misaligned track": dict(out=out.ctypes.data + 2),
           "misaligned observed": dict(obs=words.ctypes.data + 2), "misaligned d_last": dict(dl=dl.ctypes.data + 2),
           "T = 1": dict(T=1), "T = 0": dict(T=0), "T < 0": dict(T=-3), "negative P": dict(P=-1), "negative steps": dict(steps=-1),
           "P * T too large": dict(P=big), "mode 2": dict(mode=2), "mode -1": dict(mode=-1), "lambda < 0": dict(lam=-0.25),
           "lambda > 1": dict(lam=1.5), "lambda NaN": dict(lam=math.nan), "lambda inf": dict(lam=math.inf)}
    for what, change in bad.items():
        c = {**good, **change}
        opt = None if c["opt"] is None else ctypes.byref(c["opt"])
        rc = lib.pndf_interpolate_cpu(eng.handle, c["a"], c["b"], c["obs"], c["out"], c["dl"], c["P"], c["T"], c["mode"], c["steps"], c["lam"], opt)
        assert rc == -1, (what, rc)
        assert lib.pndf_cpu_last_error(eng.handle), what
        assert np.all(out == 7.0) and np.all(dl == 7.0), what
    g = good
    assert lib.pndf_interpolate_cpu(None, g["a"], g["b"], g["obs"], g["out"], g["dl"], P, T, 1, 2, 0.5, None) == -1
    # the option texts are pndf_project_ex_cpu's
    o = c_options(step_size=-0.5)
    assert lib.pndf_interpolate_cpu(eng.handle, g["a"], g["b"], g["obs"], g["out"], g["dl"], P, T, 1, 2, 0.5, ctypes.byref(o)) == -1
    assert b"step_size" in lib.pndf_cpu_last_error(eng.handle)
    # P = 0 is a no-op (null pointers allowed); d_last and observed may be NULL; lambda 0 and 1 are the ends of the range
    assert lib.pndf_interpolate_cpu(eng.handle, None, None, None, None, None, 0, T, 0, 5, 0.0, None) == 0
    for lam in (0.0, 1.0):
        assert lib.pndf_interpolate_cpu(eng.handle, g["a"], g["b"], None, g["out"], None, P, T, 0, 1, lam, None) == 0
    assert not np.all(out == 7.0) and np.isfinite(out).all() and np.all(dl == 7.0)
    # the stateless entry points refuse before any device is looked for; the workspace is d + dq + a pose buffer on 16-byte boundaries
    ws = lib.pndf_interpolate_workspace_floats
    assert ws(0, 2) == 0 and ws(-1, 2) == -1 and ws(1, 1) == -1 and ws(big, T) == -1
    for p, t in ((1, 2), (1, 3), (5, 7), (13, 5), (4096, 16)):
        assert ws(p, t) == -(-p * t // 4) * 4 + 2 * 84 * p * t
    assert lib.pndf_interp_fill(None, None, None, 0, 2, 0, None) == 0
    for args in ((None, None, None, 4, 2, 0, None), (None, None, None, 0, 1, 0, None), (None, None, None, -1, 2, 0, None),
                 (None, None, None, 0, 2, 2, None), (None, None, None, big, T, 0, None)):
        assert lib.pndf_interp_fill(*args) == -1, args
    assert lib.pndf_interp_band_step(None, None, None, None, None, 0, 2, 0.5, None, None) == 0
    x = out.ctypes.data      # (host memory: refused before it would be looked at)
    for args in ((None, None, None, None, None, 4, 2, 0.5, None, None), (None, None, None, None, None, 0, 1, 0.5, None, None),
                 (None, None, None, None, None, 0, 2, -0.5, None, None), (None, None, None, None, None, 0, 2, math.nan, None, None),
                 (None, None, None, None, None, 0, 2, 1.25, None, None), (None, None, None, None, None, -1, 2, 0.5, None, None),
                 (None, None, None, None, None, 0, 2, 0.5, ctypes.byref(c_options(renorm=7)), None),
                 (x, x, x, x, None, P, T, 0.5, None, None), (x, x + 4, x, x, None, P, T, 0.5, None, None)):
        assert lib.pndf_interp_band_step(*args) == -1, args
    assert lib.pndf_interpolate(None, None, None, None, None, None, 0, 2, 0, 0, 0.0, None, None, None) == -1
    # the Python wrappers raise
    with pytest.raises(PndfError, match="lambda"):
        eng.interpolate(g["a"], g["b"], None, g["out"], g["dl"], P, T, 2, smooth=2.0)
    with pytest.raises(PndfError, match="mode"):
        eng.interpolate(g["a"], g["b"], None, g["out"], g["dl"], P, T, 2, mode="squad")
    with pytest.raises(PndfError, match="renormalisation"):
        eng.interpolate(g["a"], g["b"], None, g["out"], g["dl"], P, T, 2, renorm="sphere")
    net = cpu_net("lrelu", sd)
    qa, qb = torch.from_numpy(a), torch.from_numpy(b)
    with pytest.raises(PndfError, match="two frames"):
        net.interpolate(qa, qb, 1)
    with pytest.raises(PndfError, match="pose_b"):
        net.interpolate(qa, qb[:3], T)
    with pytest.raises(PndfError, match="shape"):
        net.interpolate(qa, qb, T, observed=torch.zeros(3, 21, dtype=torch.bool))
    with pytest.raises(PndfError, match="bool"):
        net.interpolate(qa, qb, T, observed=torch.zeros(T, 21))


def test_crafted_joints_on_the_host(sd):
    """6. b == a, b == -a, a zero quaternion, both zero, a NaN joint: the fill's interior frames are the numpy float32 oracle's in
    both modes wherever it takes no trigonometric branch, bit for bit, and the NaN stays in its own joint's track"""
    eng = cpu_engine("lrelu", sd)
    a, b = (x.copy() for x in io.make_pairs())
    b[0, 3] = a[0, 3]
    b[0, 4] = -a[0, 4]
    a[1, 2] = 0.0
    a[2, 6] = b[2, 6] = 0.0
    a[3, 7, 1] = np.nan
    exact = [(0, 3), (0, 4), (2, 6)]
    for mode in ("slerp", "nlerp"):
        want = io.fill(a, b, T, mode, np.float32)
        got, _ = run_twin(eng, a, b, T, 0, mode=mode)
        for p, j in exact:
            assert got[p, :, j].tobytes() == want[p, :, j].tobytes(), (mode, p, j)
        assert np.isnan(got[3, 1:-1, 7]).all() and np.isnan(want[3, 1:-1, 7]).all()
        rest = np.ones((P, 21), bool)
        rest[3, 7] = False
        assert np.isfinite(got[np.broadcast_to(rest[:, None], (P, T, 21))]).all()
        assert got[:, 0].tobytes() == a.tobytes() and got[:, -1].tobytes() == want[:, -1].tobytes()
        assert not got[2, :, 6].any()      # 0 / 1e-12: the clamp keeps a zero quaternion zero
        if mode == "nlerp":
            assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
        else:
            ok = ~np.isnan(want)
            assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= 16 * 2.0 ** -24


# ---- 7. the companion header: what is its own (its table, binding, symbols and C99 build: tests/test_cabi.py, for every header alike)
def test_interpolation_table_matches_its_header(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import abi, engine
    protos = ch.prototypes(HEADER)
    assert list(protos) == ["pndf_interp_fill", "pndf_interp_band_step", "pndf_interpolate_workspace_floats", "pndf_interpolate",
                            "pndf_interpolate_cpu"]
    assert [len(abi.HEADERS[HEADER][n][1]) for n in protos] == [7, 10, 2, 14, 12]
    assert {"pndf_interp_fill_kernel", "pndf_interp_band_kernel"} <= ch.exported_symbols(ge.LIB)
    assert engine.INTERP_MODES == {"slerp": 0, "nlerp": 1}
    public = ch.header_text(HEADER)
    assert "debug" not in public.lower() and '#include "posendf_amd.h"' in public
    assert "PNDF_INTERP_SLERP = 0" in public and "PNDF_INTERP_NLERP = 1" in public
    ok, diagnostics = ch.compiles_as_c99(tmp_path, f'#include "{HEADER}"\nint main(void) {{ return PNDF_INTERP_NLERP == 1 ? 0 : 1; }}\n')
    assert ok, diagnostics


# ---- 8. the driver
def check_pose_interpolation(net, device, P=4, T=9, steps=5):
    """shared with tests/test_interpolation_gpu.py: shapes, the end frames' bits, d_last of an end frame == a forward of it,
    segment_lengths == the numpy oracle's, a single pair given as [21,4], steps = 0 == the fill"""
    from posendf_amd import PoseInterpolation
    from posendf_amd.pose_interpolation import segment_lengths
    a_np, b_np = (x[:P] for x in io.make_pairs())
    a, b = torch.from_numpy(a_np.copy()), torch.from_numpy(b_np.copy())
    pi = PoseInterpolation(net, device=device)
    track, dist, meshes = pi.interpolate(a, b, T, steps=steps)
    assert track.shape == (P, T, 21, 4) and dist.shape == (P, T) and meshes == {} and track.device.type == torch.device(device).type
    t = track.cpu().numpy()
    want_end = io.fill(a_np, b_np, T, "nlerp", np.float32)[:, -1]
    assert t[:, 0].tobytes() == a_np.tobytes() and t[:, -1].tobytes() == want_end.tobytes()
    assert a.numpy().tobytes() == a_np.tobytes() and b.numpy().tobytes() == b_np.tobytes()      # the inputs are not written
    d_all = net(track.reshape(-1, 21, 4), train=False)["dist_pred"].detach().reshape(P, T)      # (the end frames never moved)
    assert torch.equal(dist[:, [0, -1]].view(torch.int32), d_all[:, [0, -1]].view(torch.int32))
    assert np.isfinite(t).all() and np.abs(np.linalg.norm(t[:, 1:-1].astype(np.float64), axis=-1) - 1).max() <= 2 * 2.0 ** -23
    seg = segment_lengths(track)
    assert seg.shape == (P, T - 1)
    want = io.segment_lengths(t)
    # float32 acos of a dot product within 2^-24 of 1 is off by up to sqrt(2 * 2^-24): twice that for each of the 21 joints
    assert np.abs(seg.cpu().numpy() - want).max() <= 21 * 2 * math.sqrt(2 * 2.0 ** -24)
    flipped = t.copy()
    flipped[:, ::2] *= -1      # the sign of a quaternion does not matter
    assert np.allclose(segment_lengths(torch.from_numpy(flipped)).numpy(), segment_lengths(torch.from_numpy(t)).numpy(), rtol=0, atol=1e-5)
    # the coupling reaches the step; steps = 0 is the fill; one pair as [21,4]
    loose, _, _ = pi.interpolate(a, b, T, steps=steps, smooth=0.0)
    assert not torch.equal(loose, track) and torch.equal(loose[:, [0, -1]].view(torch.int32), track[:, [0, -1]].view(torch.int32))
    start, d0, _ = pi.interpolate(a, b, T, steps=0, mode="nlerp")
    assert start.cpu().numpy().tobytes() == io.fill(a_np, b_np, T, "nlerp", np.float32).tobytes() and not bool(d0.any())
    one, d1, _ = pi.interpolate(a[0], b[0], 2, steps=3)
    assert one.shape == (1, 2, 21, 4) and d1.shape == (1, 2) and one.cpu().numpy().tobytes() == t[:1, [0, -1]].tobytes()
    return pi, a, b


def test_pose_interpolation_driver_cpu(sd):
    """8. PoseInterpolation on a cpu config"""
    import posendf_amd
    assert "PoseInterpolation" in posendf_amd.__all__
    check_pose_interpolation(cpu_net("lrelu", sd), "cpu")
