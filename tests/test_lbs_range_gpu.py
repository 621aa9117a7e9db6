"""GPU tests of the body-model kernels (posendf_amd/csrc/pndf_lbs.hip) at the ends of the ranges their split-precision operand
scales rest on (csrc/pndf_lbs_scales.h): heavy-tailed models in three length units, degenerate models, term weights six decades
apart through terms_grad(coefs=...), poses at |R - I| = 2, past pi and at the tiny-angle end, nearly coinciding frames and a
non-finite frame (tests/lbs_stress.py).  tests/test_lbs_range.py checks the bounds themselves on the host; here the kernels run.

Oracle: oracle/lbs_np.py in fp64 (parity unpinned, as in tests/test_lbs_gpu.py).  The gates are that module's, for both
arithmetics ("f16x3" and "fp32"):
  forward   vertices, Jtr, joints_of: error relative to the largest fp64 entry < 1e-5
  gradient  per sequence err < max(1e-4, 8 ref), ref = the fp32 oracle's own error against fp64 on the same input (printed)
and next to them the marginal gates of tests/lbs_gates.py: every vertex, joint and frame on its own against eight draws of the
kernel's reference arithmetic (float32; for "f16x3" the split arithmetic at the library's scales), made once per case.
Shapes: V = 41 (three vertex groups, the last one padded) and 137; S = 2, T = 17 (a chunk boundary with a shared frame, two
sequences in one workgroup quad)."""
import numpy as np
import pytest
import torch

import lbs_gates
from lbs_stress import COEFS, SATURATING_TWINS, UNITS, stress_model, stress_theta
from oracle import lbs_np

pytestmark = pytest.mark.gpu
TOL = 1e-4
S, T = 2, 17
PRECISIONS = ("f16x3", "fp32")
_BANK, _ORACLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _shared():
    """the BodyModel instances and the oracle's results, each made once and shared by every test of the module"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    yield
    _BANK.clear()
    _ORACLE.clear()


def bank(precision, V=137, unit=1.0, kind="smpl_like"):
    key = (precision, V, unit, kind)
    if key not in _BANK:
        from posendf_amd import BodyModel
        m = stress_model(V, 9, unit=unit, kind=kind)
        _BANK[key] = (m, BodyModel(m, device="cuda:0", precision=precision))
    return _BANK[key]


def once(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _theta0(th):
    return th + np.random.default_rng(1).normal(size=th.shape).astype(np.float32) * 0.05


def check_forward(tag, key, m, bm, th):
    """vertices, Jtr and joints_of of all S * T frames; where the fp64 oracle is non-finite the kernels are, entry by entry,
    and nowhere else.  Returns the finite-frame mask."""
    flat = th.reshape(-1, 69)
    with np.errstate(invalid="ignore"):
        V64, J64 = once(("fwd",) + key, lambda: lbs_np.lbs(flat, m))
    out = bm(pose_body=torch.from_numpy(flat))
    v, j, jo = out.vertices.cpu().numpy(), out.Jtr.cpu().numpy(), bm.joints_of(torch.from_numpy(flat)).cpu().numpy()
    assert np.array_equal(np.isfinite(v), np.isfinite(V64)) and np.array_equal(np.isfinite(j), np.isfinite(J64)), tag
    assert np.array_equal(np.isfinite(jo), np.isfinite(J64)), tag
    ok = np.isfinite(V64).all((1, 2)) & np.isfinite(J64).all((1, 2))
    ev, ej, eo = (float(np.abs(a[ok] - b[ok]).max() / np.abs(b[ok]).max()) for a, b in ((v, V64), (j, J64), (jo, J64)))
    print(f"LBS range forward {tag}: verts {ev:.2e}  Jtr {ej:.2e}  joints_of {eo:.2e}")
    assert ev < 1e-5 and ej < 1e-5 and eo < 1e-5, tag

    def envelope(precision):
        return lambda: lbs_gates.envelope(lbs_gates.forward_ref(m, lbs_gates.arithmetic(precision, m)), [flat], (V64, J64))
    env_v, env_j = once(("fwd env", bm.precision) + key, envelope(bm.precision))
    env_o = once(("fwd env", "fp32") + key, envelope("fp32"))[1]      # joints_of runs on the fp32 VALU under either setting
    lbs_gates.gate(f"range forward {tag} verts", v, V64, env_v, lbs_gates.VERTICES, ok)
    lbs_gates.gate(f"range forward {tag} Jtr", j, J64, env_j, lbs_gates.JOINTS, ok)
    lbs_gates.gate(f"range forward {tag} joints_of", jo, J64, env_o, lbs_gates.JOINTS, ok)
    return ok.reshape(th.shape[:2])


def check_gradient(tag, key, m, bm, th, it=0, coefs=None, data=True):
    """terms_grad against body_terms, per sequence: the rows the fp64 oracle makes non-finite are non-finite, every other row is
    finite and inside the gate.  Returns the oracle's non-finite rows per sequence."""
    th0 = _theta0(th)
    j0 = bm.joints_of(torch.from_numpy(th0)) if data else None
    g = bm.terms_grad(torch.from_numpy(th).cuda(), j0, it, coefs=coefs).cpu().numpy()

    def oracle():
        rows = []
        for s in range(th.shape[0]):
            with np.errstate(invalid="ignore", divide="ignore"):
                J0 = lbs_np.lbs(th0[s], m)[1] if data else None
                g64, _ = lbs_np.body_terms(th[s], J0, m, it, coefs=coefs)
                g32, _ = lbs_np.body_terms(th[s], None if J0 is None else J0.astype(np.float32), m, it, np.float32, coefs=coefs)
            rows.append((g64, g32))
        return rows
    rows = once(("grad", it, coefs, data) + key, oracle)

    def envelope():
        weights = coefs if coefs is not None else lbs_gates.schedule_coefs(it)
        hook = lbs_gates.arithmetic(bm.precision, m, th.shape[1], weights if data else (weights[0], 0.0))
        with np.errstate(invalid="ignore"):
            J0 = np.stack([lbs_np.lbs(th0[s], m)[1] for s in range(th.shape[0])]).astype(np.float32) if data else None
        x64 = np.stack([g64 for g64, _ in rows]).reshape(th.shape[:2] + (23, 3))
        return x64, lbs_gates.envelope(lbs_gates.terms_ref(m, it, coefs, hook), [th, J0], x64)
    x64, env = once(("grad env", bm.precision, it, coefs, data) + key, envelope)
    lbs_gates.gate(f"range grad {tag}", g.reshape(x64.shape), x64, env, lbs_gates.GRADIENT, np.isfinite(x64).all((2, 3)))
    bad_rows = []
    for s, (g64, g32) in enumerate(rows):
        good = np.isfinite(g64).all(1)
        assert not np.isfinite(g64[~good]).any()                     # (the oracle's non-finite rows are non-finite throughout)
        assert np.isfinite(g[s][good]).all() and not np.isfinite(g[s][~good]).any(), (tag, s, np.flatnonzero(~good))
        scale = max(np.abs(g64[good]).max(), 1e-30)
        err, ref = np.abs(g[s][good] - g64[good]).max() / scale, np.abs(g32[good] - g64[good]).max() / scale
        arm = "1e-4" if err < TOL or 8 * ref <= TOL else "8 ref"
        print(f"LBS range grad {tag} seq {s}: err {err:.2e} (fp32 oracle ref {ref:.2e}) |g| {scale:.2e} gate arm {arm}"
              + (f" non-finite rows {np.flatnonzero(~good).tolist()}" if not good.all() else ""))
        assert err < max(TOL, 8 * ref), (tag, s, err, ref)
        bad_rows.append(np.flatnonzero(~good).tolist())
    return bad_rows


# ---- 1. length units and dynamic range
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("V", [41, 137])
@pytest.mark.parametrize("unit", UNITS)
def test_units_and_dynamic_range(precision, V, unit):
    m, bm = bank(precision, V, unit)
    th = stress_theta(S, T, 4, "ordinary")
    tag, key = f"{precision} V={V} unit={unit:g} ordinary", (V, unit, "smpl_like", "ordinary")
    assert check_forward(tag, key, m, bm, th).all()
    assert check_gradient(tag + " it=2", key, m, bm, th, it=2) == [[], []]


# ---- 2. term weights
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("coefs", COEFS)
def test_coefs_set_the_reverse_operand_scales(precision, coefs):
    """terms_grad(coefs=...) = pndf_lbs_terms_grad_w: the weights set g_scale and x_scale.  (c, 0): no data term, joints0 may
    be None, and a single frame has no pair: its gradient is exactly zero."""
    m, bm = bank(precision)
    th = stress_theta(S, T, 4, "ordinary")
    data = coefs[1] != 0
    bad = check_gradient(f"{precision} coefs={coefs}", (137, 1.0, "smpl_like", "ordinary"), m, bm, th, it=1 if data else 0, coefs=coefs, data=data)
    assert bad == [[], []]
    if not data:
        g1 = bm.terms_grad(torch.from_numpy(th[:, :1].copy()).cuda(), None, 0, coefs=coefs)
        assert g1.shape == (S, 1, 69) and torch.count_nonzero(g1) == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("it", [0, 1, 9])
def test_builtin_schedule(precision, it):
    m, bm = bank(precision)
    th = stress_theta(S, T, 4, "ordinary")
    assert check_gradient(f"{precision} it={it}", (137, 1.0, "smpl_like", "ordinary"), m, bm, th, it=it, data=it > 0) == [[], []]


# ---- 3. pose range
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("V", [41, 137])
@pytest.mark.parametrize("motion", ["wide", "saturating"])
def test_pose_range(precision, V, motion):
    """angles past pi; every joint at exactly pi (|R - I| = 2), 2 pi, 3 pi, 1e-4, 1e-7 and 0.  The two identical frames of
    "saturating" give the reference's NaN rows (no epsilon under the root) and only those."""
    m, bm = bank(precision, V)
    th = stress_theta(S, T, 4, motion)
    tag, key = f"{precision} V={V} {motion}", (V, 1.0, "smpl_like", motion)
    assert check_forward(tag, key, m, bm, th).all()
    bad = check_gradient(tag + " it=1", key, m, bm, th, it=1)
    assert bad == ([list(SATURATING_TWINS)] * S if motion == "saturating" else [[], []])


# ---- 4. degenerate models
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["no_correctives", "rigid"])
def test_degenerate_models(precision, kind):
    """posedirs = 0 (p_scale from a clamped zero bound: ~2^112) and one-hot skinning weights: finite, inside the same gates"""
    m, bm = bank(precision, 137, 1.0, kind)
    th = stress_theta(S, T, 4, "ordinary")
    tag, key = f"{precision} {kind}", (137, 1.0, kind, "ordinary")
    assert check_forward(tag, key, m, bm, th).all()
    assert check_gradient(tag + " it=1", key, m, bm, th, it=1) == [[], []]


def test_no_correctives_both_arithmetics_agree():
    flat = torch.from_numpy(stress_theta(S, T, 4, "ordinary").reshape(-1, 69))
    a, b = (bank(p, 137, 1.0, "no_correctives")[1](pose_body=flat) for p in PRECISIONS)
    for x, y in ((a.vertices, b.vertices), (a.Jtr, b.Jtr)):
        e = ((x - y).abs().max() / y.abs().max()).item()
        print(f"LBS range no_correctives f16x3 vs fp32: {e:.2e}")
        assert e < 2e-6


# ---- 5. a non-finite frame stays where the mathematics puts it
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("what", ["nan_frame", "inf_entry"])
def test_nonfinite_frame_stays_in_its_rows(precision, what):
    """frame 15 of sequence 0 = the frame its two chunks share (T = 17); sequence 1 sits in the same workgroup quad.  Forward:
    frame 15 alone is touched, entry by entry as in the oracle.  Gradient: the temporal term couples neighbours, so rows 14,
    15, 16 of sequence 0 are non-finite; every other row and all of sequence 1 are finite and inside the gate."""
    m, bm = bank(precision)
    th = stress_theta(S, T, 4, "ordinary")
    if what == "nan_frame":
        th[0, 15, :] = np.nan
    else:
        th[0, 15, 40] = np.inf
    tag, key = f"{precision} {what}", (137, 1.0, "smpl_like", what)
    ok = check_forward(tag, key, m, bm, th)
    assert not ok[0, 15] and ok.sum() == S * T - 1
    assert check_gradient(tag + " it=1", key, m, bm, th, it=1) == [[14, 15, 16], []]


# ---- 6. nearly coinciding frames
@pytest.mark.parametrize("precision", PRECISIONS)
def test_slow_motion(precision):
    """steps of 1e-3 rad: V[t] - V[t+1] cancels three digits; the fp32 oracle's own error `ref` is printed with the result"""
    m, bm = bank(precision)
    th = stress_theta(S, T, 4, "slow")
    assert check_gradient(f"{precision} slow it=1", (137, 1.0, "smpl_like", "slow"), m, bm, th, it=1) == [[], []]
