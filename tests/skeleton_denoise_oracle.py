"""Test helper (not a test module) for motion denoising on other skeletons (pndf_project_options4 of include/posendf_amd.h; DESIGN.md
section 2j "Motion denoising"): the numpy statement of the denoising step -- the descent, the neighbour coupling with free or held end
frames, the data term towards the observation, the finish -- for any joint count, in float32 and float64; the free-running oracle on
tests/skeleton_oracle.py's forward_grad; the noisy clips, confidences and masks; the raw C struct and the C99 snippet.  It reuses the
tracks, masks, cases and option sets of tests/skeleton_interpolation_oracle.py.  Shared by tests/test_skeleton_denoise.py (host twin)
and tests/test_skeleton_denoise_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `denoise_step` in float32 IS the
specification both implementations are held to bit for bit."""
import ctypes
import functools

import numpy as np

import skeleton_completion_oracle as sco
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from interpolation_oracle import align, dot4, unit

BAD_ARG = sio.BAD_ARG
FREE_ENDS = 1                      # PNDF_TRACK_FREE_ENDS
CASES = sio.CASES
ACTS = sio.ACTS
OPTION_SETS = sio.OPTION_SETS
options = sio.options
flat = sio.flat
assert_same = sio.assert_same
pack = sio.pack
P, T = 3, 5                        # 15 poses
K = 3
LAMBDA = 0.5
MU = 0.25


def clip(case, P=P, T=T):
    """[P,T,J,4]: the case's poses read as P tracks of T frames (unrelated frames: what a bit-for-bit check of one step wants)"""
    return sio.given_track(case, P, T)


def make_conf(J, P=P, T=T, seed=11):
    """float32 [P,T,J] in (0, 1], with zeros (about one joint in six), one negative value and one NaN: a joint whose confidence is not
    positive takes no data term and its anchor is not read"""
    r = np.random.RandomState(seed)
    c = (0.05 + 0.95 * r.rand(P, T, J)).astype(np.float32)
    c[r.rand(P, T, J) < 1.0 / 6.0] = 0.0
    c[0, 0, 0] = 0.0               # an end frame, which FREE_ENDS frees
    c[P - 1, T - 1, J - 1] = np.float32(-0.5)
    c[P - 1, 1 % T, 0] = np.float32(np.nan)
    return c


def make_anchor(track, conf=None, seed=13):
    """the observation of a clip: the clip itself plus a small offset (so the data term has work to do from the first step), every other
    joint negated (the alignment has work to do); where `conf` is not positive the anchor is NaN -- a missing detection"""
    r = np.random.RandomState(seed)
    a = (track + np.float32(0.05) * r.randn(*track.shape).astype(np.float32)).astype(np.float32)
    a[:, :, 1::2] = -a[:, :, 1::2]
    a[1::2, :, 0] = -a[1::2, :, 0]      # (one joint: every other track)
    if conf is not None:
        with np.errstate(invalid="ignore"):
            a[~(conf > 0)] = np.float32(np.nan)
    return np.ascontiguousarray(a)


def make_mask(J, P=P, T=T, seed=7):
    """bool [P,T,J], True = held: about a third of the joints of track 1, end frames included (FREE_ENDS leaves the mask in force there)"""
    m = np.zeros((P, T, J), bool)
    if P > 1:
        m[1] = np.random.RandomState(seed).rand(T, J) < 1.0 / 3.0
        m[1, 0, 0] = True
        if J == 32:
            m[1, 1 % T, 31] = True     # the sign bit of a word read as int32
    return m


# ---------------------------------------------------------------- the step
def denoise_step(q, d, g, anchor=None, conf=None, mu=0.0, observed=None, smooth=0.0, free_ends=False, frames=None, step_size=1.0,
                 renormalize=None, tol=0.0):
    """One denoising step on q [P,T,J,4] in q's dtype from d [P*T] and g [P,T,J,4].  `frames`: None = the T of q (tracks); 0 = no
    tracks (every pose on its own: no coupling, no end frames).  anchor [P,T,J,4] or None, conf [P,T,J] or None (ones), observed
    bool [P,T,J] or None.  Returns the new track (q is not modified)."""
    dt = q.dtype.type
    Pn, Tn, J = q.shape[:3]
    frames = Tn if frames is None else frames
    assert q.shape == (Pn, Tn, J, 4) and frames in (0, Tn) and 0.0 <= smooth <= 1.0 and 0.0 <= mu <= 1.0
    assert frames or (smooth == 0.0 and not free_ends)
    g = np.asarray(g, dtype=dt).reshape(q.shape)
    dist = np.asarray(d, dtype=dt).reshape(Pn, Tn, 1, 1)
    held = np.zeros((Pn, Tn, J), bool) if observed is None else np.asarray(observed, bool).reshape(Pn, Tn, J).copy()
    if frames and not free_ends:
        held[:, 0] = held[:, Tn - 1] = True
    with np.errstate(all="ignore"):
        # 1. descend
        p = dist * g
        s = dt(step_size) * p
        u = q - s
        # 2. coupling
        if frames and smooth > 0:
            lam = dt(smooth)
            if Tn > 2:
                Q = q[:, 1:-1]
                am, ap = align(Q, q[:, :-2]), align(Q, q[:, 2:])
                h = dt(0.5) * (am + ap)
                m = h - Q
                u[:, 1:-1] = u[:, 1:-1] + lam * m
            if free_ends:
                for k, n in ((0, 1), (Tn - 1, Tn - 2)):
                    Q = q[:, k]
                    an = align(Q, q[:, n])
                    m = an - Q
                    h = dt(0.5) * m
                    u[:, k] = u[:, k] + lam * h
        # 3. data term
        if anchor is not None and mu != 0:
            w = np.full((Pn, Tn, J), dt(mu), dtype=q.dtype) if conf is None else dt(mu) * np.asarray(conf, dtype=q.dtype).reshape(Pn, Tn, J)
            on = w > 0
            A = np.where(on[..., None], np.asarray(anchor, dtype=q.dtype).reshape(q.shape), dt(0))      # the anchor is not read otherwise
            aa = align(q, A)
            m = aa - q
            wm = np.where(on, w, dt(0))[..., None] * m
            u = np.where(on[..., None], u + wm, u)
        # 4. finish
        if renormalize is not None:
            assert renormalize in ("unit", "unit_flip"), renormalize
            u = unit(u)
            if renormalize == "unit_flip":
                u = np.where(u[..., :1] < 0, -u, u)
        if tol > 0:
            u = np.where(dist < dt(tol), q, u)      # a NaN d compares false: not frozen
    out = np.where(held[..., None], q, u)
    assert out.dtype == q.dtype
    return out


def rounds(forward_grad, track, steps, **kw):
    """`steps` rounds of { forward_grad(q [B,J,4]) -> (d [B], dq [B,J,4]) of the engine under test ; denoise_step in float32 } ->
    (track, d of the last round)"""
    cur, d = np.ascontiguousarray(track, np.float32).copy(), np.zeros(track.shape[0] * track.shape[1], np.float32)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        cur = np.ascontiguousarray(denoise_step(cur, d, g, **kw), np.float32)
    return cur, d


def relax(track, sd, steps, act, parents, dtype=np.float32, **kw):
    """free-running oracle: `steps` times skeleton_oracle's forward_grad + denoise_step in `dtype` -> (track, d of the last step [P*T],
    the smallest kink margin every pose met at the iterates before the updates [P*T])"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    d = np.zeros((q.shape[0] * q.shape[1], 1), dtype)
    margin = np.full(q.shape[0] * q.shape[1], np.inf)
    for _ in range(steps):
        d, g, m, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        margin = np.minimum(margin, m)
        q = denoise_step(q, d, g, **kw)
    return q, np.asarray(d).reshape(-1), margin


# ---------------------------------------------------------------- the effects
def noisy_clip(case, P=sio.P, T=sio.T, sigma=0.05, seed=17):
    """a smooth clip plus noise -> (noisy [P,T,J,4] float32, unit per joint): the slerp track between the pairs of
    skeleton_interpolation_oracle.make_pairs, every joint plus sigma * N(0, 1) per component and renormalised.  The fill aligns b to a, so
    consecutive frames lie in one hemisphere and plain differences measure the motion."""
    a, b = sio.make_pairs(case, P)
    clean = sio.fill(a, b, T, "slerp", np.float64)
    x = clean + sigma * np.random.RandomState(seed).randn(*clean.shape)
    x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    return np.ascontiguousarray(x, np.float32)


def angle_to(track, anchor):
    """mean over every joint of the rotation angle 2 acos(min(|<q, a>|, 1)) in float64"""
    t, a = np.asarray(track, np.float64), np.asarray(anchor, np.float64)
    t = t / np.sqrt((t * t).sum(-1, keepdims=True))
    a = a / np.sqrt((a * a).sum(-1, keepdims=True))
    return float((2.0 * np.arccos(np.minimum(np.abs((t * a).sum(-1)), 1.0))).mean())


def second_difference(track):
    """sum over the interior frames, joints and components of (q_k-1 - 2 q_k + q_k+1)^2 in float64"""
    t = np.asarray(track, np.float64)
    dd = t[:, :-2] - 2.0 * t[:, 1:-1] + t[:, 2:]
    return float((dd * dd).sum())


EFFECT_STEPS = 10


@functools.lru_cache(maxsize=None)
def oracle_effect(case, act, smooth, mu):
    """(angle to the observation, second difference) of the fp64 oracle after EFFECT_STEPS free-running steps on noisy_clip(case), the
    clip its own anchor, free ends, unit quaternions"""
    parents, sd = sko.case_network(case, act)
    x = noisy_clip(case)
    out, d, _ = relax(x, sd, EFFECT_STEPS, act, parents, dtype=np.float64, anchor=x, mu=mu, smooth=smooth, free_ends=True, renormalize="unit")
    assert np.isfinite(out).all() and np.isfinite(d).all()
    return angle_to(out, x), second_difference(out)


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options4(lib, observed=None, frames=0, lam=0.0, fill=sio.GIVEN, anchor=None, conf=None, mu=0.0, flags=0, size=None, **kw):
    """a pndf_project_options4 (72 bytes) filled the documented way; observed / anchor / conf: addresses or None; **kw: c_options3's"""
    from posendf_amd.abi import ProjectOptions4
    o = ProjectOptions4()
    o.base3 = sio.c_options3(lib, observed, frames, lam, fill, **kw)
    o.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.anchor, o.conf, o.mu, o.flags = anchor, conf, mu, flags
    return o


def c_from(lib, opts, observed=None, frames=0, lam=0.0, anchor=None, conf=None, mu=0.0, flags=0, fill=sio.GIVEN):
    """the 72-byte struct of keyword options (those of denoise_step)"""
    return c_options4(lib, observed, frames, lam, fill, anchor, conf, mu, flags, step_size=opts.get("step_size", 1.0),
                      renorm=sco.RENORM[opts.get("renormalize")], tol=opts.get("tol", 0.0))


# what a caller of the C header writes: the snippet of the documentation, as strict C99
C99_SNIPPET = """#include "posendf_amd_skeleton.h"
int main(void) {
    static const uint32_t mask[4] = {0u, 0x80000001u, 0u, 0u};
    static const float noisy[4 * 2 * 4] = {0};
    static const float conf[4 * 2] = {0};
    pndf_project_options4 o;
    pndf_default_project_options(&o.base3.base2.base);
    o.base3.base2.base.struct_size = sizeof o;
    o.base3.base2.observed = mask;
    o.base3.base2.reserved = 0;
    o.base3.frames = 4;
    o.base3.lambda = 0.5f;
    o.base3.fill = PNDF_TRACK_GIVEN;
    o.base3.reserved2 = 0;
    o.anchor = noisy;
    o.conf = conf;
    o.mu = 0.25f;
    o.flags = PNDF_TRACK_FREE_ENDS;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 72) + (int)(sizeof(pndf_project_options3) != 48) + (int)(PNDF_TRACK_FREE_ENDS != 1);
}
"""
