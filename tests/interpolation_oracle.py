"""Test helper (not a test module) for pose interpolation (include/posendf_amd_interpolation.h; DESIGN.md section 2 "Pose
interpolation"): the fill and the band step in numpy, the free-running oracle built on oracle.posendf_np.forward_grad, and the
inputs, mask and option sets of the reference-run fixture tests/golden/interpolation.npz.

Everything is generic in dtype.  numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so
`fill(mode="nlerp")` and `band_step` in float32 ARE the specification the kernels and the host twin are held to bit for bit;
`fill(mode="slerp")` calls sin and atan2, which differ by a few ulp between implementations, and is held to a tolerance."""
import functools
import os

import numpy as np

import completion_oracle as co
import project_options_oracle as poo
from oracle import posendf_np as onp

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interpolation.npz")
ACTS = poo.ACTS
STEPS = 10
P, T = 6, 7
SMOOTHS = (0.0, 0.5)
OPTION_SETS = co.OPTION_SETS      # name -> (step_size, renormalize); "unit_tol": the tolerance of tests/golden/project_options.npz
MASKED_PAIRS = (1, 4)


def make_pairs():
    """(a, b) [6,21,4] each: poses 0..5 and poses 24..29 of the projection-options fixture.  The b poses are signed, so the
    alignment of the fill flips some of their joints."""
    q = poo.make_inputs()
    return np.ascontiguousarray(q[:P]), np.ascontiguousarray(q[poo.NPOSE:poo.NPOSE + P])


def weights():
    return poo.weights()


def make_mask(P=P, T=T):
    """bool [P,T,21], True = observed: about a third of the joints of the interior frames of pairs 1 and 4 (those that exist)"""
    m = np.zeros((P, T, 21), bool)
    draw = np.random.RandomState(7).rand(len(MASKED_PAIRS), T, 21) < 1.0 / 3.0
    for row, p in enumerate(MASKED_PAIRS):
        if p < P:
            m[p, 1:T - 1] = draw[row, 1:T - 1]
    return m


def pack(mask):
    """bool [P,T,21] -> uint32 [P*T], bit j = joint j (the `observed` argument of pndf_interpolate)"""
    return co.pack(np.asarray(mask, bool).reshape(-1, 21))


def options(name, act):
    """step options of an option set, as keyword arguments of PoseNDF.interpolate (and of band_step)"""
    return co.options(name, act)


def dot4(x, y):
    return ((x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]) + x[..., 3] * y[..., 3]


def align(q, n):
    """n, negated per quaternion where <q, n> < 0 (a NaN dot product does not flip)"""
    with np.errstate(all="ignore"):
        return np.where((dot4(q, n) < 0)[..., None], -n, n)


def unit(u):
    """u / max(|u|, 1e-12) per quaternion: the renormalisation of poo.step"""
    dt = u.dtype.type
    with np.errstate(all="ignore"):
        n = np.sqrt(dot4(u, u))
        den = np.where(n < dt(1e-12), dt(1e-12), n)
        return u / den[..., None]


def fill(a, b, T, mode="slerp", dtype=np.float32):
    """a, b [P,21,4] -> the filled track [P,T,21,4] in `dtype`"""
    assert T >= 2 and mode in ("slerp", "nlerp")
    dt = np.dtype(dtype).type
    a = np.asarray(a, dtype=dtype).reshape(-1, 21, 4)
    b = np.asarray(b, dtype=dtype).reshape(-1, 21, 4)
    bp = align(a, b)
    track = np.empty((len(a), T, 21, 4), dtype)
    track[:, 0], track[:, T - 1] = a, bp
    with np.errstate(all="ignore"):
        if mode == "slerp":
            dm, dp = a - bp, a + bp
            s, p = np.sqrt(dot4(dm, dm)), np.sqrt(dot4(dp, dp))
            theta = dt(2) * np.arctan2(s, p)
            sn = np.sin(theta)
        for k in range(1, T - 1):
            t = dt(k) / dt(T - 1)
            wa, wb = dt(1) - t, t
            if mode == "slerp":
                ok = sn > 0
                den = np.where(ok, sn, dt(1))
                wa = np.where(ok, np.sin(wa * theta) / den, wa)[..., None]
                wb = np.where(ok, np.sin(t * theta) / den, wb)[..., None]
            track[:, k] = unit(wa * a + wb * bp)
    assert track.dtype == np.dtype(dtype)
    return track


def band_step(q, d, g, observed=None, smooth=0.0, step_size=1.0, renormalize=None, tol=0.0):
    """One band step on the track q [P,T,21,4] in q's dtype from d [P*T] and g [P,T,21,4]; observed: bool [P,T,21] or None.
    Returns the new track (q is not modified)."""
    dt = q.dtype.type
    Pn, Tn = q.shape[:2]
    assert q.shape == (Pn, Tn, 21, 4) and Tn >= 2 and 0.0 <= smooth <= 1.0
    g = np.asarray(g, dtype=dt).reshape(q.shape)
    d = np.asarray(d, dtype=dt).reshape(Pn, Tn, 1, 1)
    held = np.zeros((Pn, Tn, 21), bool) if observed is None else np.asarray(observed, bool).reshape(Pn, Tn, 21).copy()
    held[:, 0] = held[:, Tn - 1] = True
    out = q.copy()
    if Tn == 2:
        return out
    Q, G, dist = q[:, 1:-1], g[:, 1:-1], d[:, 1:-1]
    with np.errstate(all="ignore"):
        p = dist * G
        s = dt(step_size) * p
        u = Q - s
        if smooth > 0:
            nm, np_ = align(Q, q[:, :-2]), align(Q, q[:, 2:])
            h = dt(0.5) * (nm + np_)
            m = h - Q
            u = u + dt(smooth) * m
        if renormalize is not None:
            assert renormalize in ("unit", "unit_flip"), renormalize
            u = unit(u)
            if renormalize == "unit_flip":
                u = np.where(u[..., :1] < 0, -u, u)
        if tol > 0:
            u = np.where(dist < dt(tol), Q, u)      # a NaN d compares false: not frozen
    out[:, 1:-1] = np.where(held[:, 1:-1, :, None], Q, u)
    assert out.dtype == q.dtype
    return out


def relax(track, sd, steps, act, observed=None, smooth=0.0, dtype=np.float32, snap_at=(), **opts):
    """`steps` times forward_grad + band_step on a filled track.  Returns (track, d trace [steps, P*T], {k: track after k steps})."""
    q = np.asarray(track, dtype=dtype)
    trace, snaps = [], {}
    for it in range(steps):
        d, g = onp.forward_grad(q.reshape(-1, 21, 4), sd, act, dtype=dtype)
        q = band_step(q, d, g, observed, smooth, **opts)
        trace.append(np.asarray(d).reshape(-1).copy())
        if it + 1 in snap_at:
            snaps[it + 1] = q.copy()
    return q, (np.stack(trace) if trace else np.zeros((0, q.shape[0] * q.shape[1]), dtype)), snaps


def interpolate(a, b, T, sd, steps, act, mode="slerp", observed=None, smooth=0.0, dtype=np.float32, snap_at=(), **opts):
    """Free-running oracle: fill, then relax"""
    return relax(fill(a, b, T, mode, dtype), sd, steps, act, observed, smooth, dtype, snap_at, **opts)


def kink_margin_along(track, sd, steps, act, observed=None, smooth=0.0, **opts):
    """`margin` argument of conftest.outlier_gate: the smallest kink margin each pose of the track meets at the iterates before
    each of the `steps` updates of the band's fp64 trajectory; None for softplus, which has no kinks"""
    if act == "softplus":
        return None
    q = np.asarray(track, dtype=np.float64)
    margin = np.full(q.shape[0] * q.shape[1], np.inf)
    for _ in range(steps):
        flat = q.reshape(-1, 21, 4)
        margin = np.minimum(margin, onp.kink_margin(flat, sd, act))
        d, g = onp.forward_grad(flat, sd, act, dtype=np.float64)
        q = band_step(q, d, g, observed, smooth, **opts)
    return margin


def segment_lengths(track):
    """[P,T,21,4] -> [P,T-1] in float64: the sum over the joints of 2 acos(min(|<q_k, q_k+1>|, 1))"""
    t = np.asarray(track, np.float64)
    dots = np.minimum(np.abs((t[:, :-1] * t[:, 1:]).sum(-1)), 1.0)
    return (2.0 * np.arccos(dots)).sum(-1)


@functools.lru_cache(maxsize=None)
def _evenness(act, smooth):
    a, b = make_pairs()
    out, trace, _ = interpolate(a, b, T, weights(), 50, act, smooth=smooth, dtype=np.float64, **options("unit", act))
    assert np.isfinite(out).all() and np.isfinite(trace).all()
    seg = segment_lengths(out)
    return seg.max(axis=1) / seg.mean(axis=1), seg.sum(axis=1)


def check_inputs():
    """In fp64, with these inputs: every option set and both couplings stay finite for both activations over ten steps, with and
    without the mask; and with renormalize="unit", 50 steps and no mask the coupling 0.5 gives every pair a smaller
    longest-to-mean segment ratio and a shorter path than no coupling."""
    a, b = make_pairs()
    m, sd = make_mask(), weights()
    assert a.shape == b.shape == (P, 21, 4) and m.shape == (P, T, 21)
    flipped = dot4(a, b) < 0
    assert 0.1 < flipped.mean() < 0.9      # the alignment has work to do
    inner = m[list(MASKED_PAIRS), 1:T - 1]
    assert 0.2 < inner.mean() < 0.45 and not m[:, 0].any() and not m[:, T - 1].any() and m.sum() == inner.sum()
    for act in ACTS:
        for name in OPTION_SETS:
            for smooth in SMOOTHS:
                for mask in (None, m):
                    out, trace, _ = interpolate(a, b, T, sd, STEPS, act, observed=mask, smooth=smooth, dtype=np.float64, **options(name, act))
                    assert np.isfinite(out).all() and np.isfinite(trace).all(), (act, name, smooth)
        r0, l0 = _evenness(act, 0.0)
        r5, l5 = _evenness(act, 0.5)
        assert (r5 < r0).all() and (l5 < l0).all(), (act, r0, r5, l0, l5)
