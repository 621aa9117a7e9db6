"""Test helper (not a test module) for pose interpolation on other skeletons (pndf_project_options3 of include/posendf_amd.h; DESIGN.md
section 2j): the fill and the band step of tests/interpolation_oracle.py restated for any joint count J, the free-running oracle on
tests/skeleton_oracle.py's forward_grad (pinned against the reference's own modules by the skeleton fixtures), the tracks, masks and
option sets, the raw C struct of the refusal tests and the evenness inputs.  Shared by tests/test_skeleton_interpolation.py (host twin)
and tests/test_skeleton_interpolation_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `fill(mode="nlerp")` and `band_step`
in float32 ARE the specification both implementations are held to bit for bit; `fill(mode="slerp")` calls sin and atan2, which differ
by a few ulp between implementations, and is held to a tolerance."""
import ctypes
import functools

import numpy as np

import completion_oracle as co
import skeleton_completion_oracle as sco
import skeleton_oracle as sko
from interpolation_oracle import align, dot4, unit

BAD_ARG, UNSUPPORTED = sco.BAD_ARG, sco.UNSUPPORTED
GIVEN, SLERP, NLERP = 0, 1, 2      # PNDF_TRACK_*
FILLS = {"given": GIVEN, "slerp": SLERP, "nlerp": NLERP}
CASES = sco.CASES                  # hand, tree32, one, roots5, chain32, the encoder-less hand
ACTS = sko.CASE_ACTS
OPTION_SETS = co.OPTION_SETS       # name -> (step_size, renormalize); "unit_tol" takes a tolerance besides
P, T = 6, 7                        # 42 poses
K = 3                              # steps of the stated-step checks
LAMBDA = 0.5
MASKED_PAIRS = (1, 4)


def options(name, tol):
    """the step options of an option set as keyword arguments of band_step; `tol`: the tolerance of "unit_tol" """
    step_size, renorm = OPTION_SETS[name]
    return dict(step_size=step_size, renormalize=renorm, tol=float(tol) if name == "unit_tol" else 0.0)


def given_track(case, P=P, T=T):
    """[P,T,J,4]: the case's poses (skeleton_oracle.case_poses) read as P tracks of T frames -- unrelated frames, which is what a
    bit-for-bit check of one step wants"""
    q = sko.case_poses(case, P * T)
    return np.ascontiguousarray(q.reshape(P, T, q.shape[1], 4))


def make_pairs(case, P=P):
    """(a, b) [P,J,4] each, unit per joint: poses 0 .. P-1 and poses 24 .. 24+P-1 of case_poses(case, 48), the b poses times the signs
    RandomState(3).rand(P, J, 1) < 0.5, so the alignment of the fill flips some of their joints"""
    q = sko.case_poses(case, 48).astype(np.float64)
    q = (q / np.sqrt((q * q).sum(-1, keepdims=True))).astype(np.float32)
    J = q.shape[1]
    sign = np.where(np.random.RandomState(3).rand(P, J, 1) < 0.5, np.float32(-1), np.float32(1))
    return np.ascontiguousarray(q[:P]), np.ascontiguousarray(q[24:24 + P] * sign)


def ends_of(a, b, T):
    """the input of a filled call: [P,T,J,4] with a in frame 0 and b in frame T-1; the frames between them hold 7.0 and are never read"""
    x = np.full((len(a), T) + a.shape[1:], 7.0, np.float32)
    x[:, 0], x[:, T - 1] = a, b
    return x


def make_mask(J, P=P, T=T, seed=7):
    """bool [P,T,J], True = observed: about a third of the joints of the interior frames of pairs 1 and 4 (those that exist); with 32
    joints joint 31 -- the sign bit of a word read as int32 -- is observed in frame 1 of pair 1"""
    m = np.zeros((P, T, J), bool)
    draw = np.random.RandomState(seed).rand(len(MASKED_PAIRS), T, J) < 1.0 / 3.0
    for row, p in enumerate(MASKED_PAIRS):
        if p < P:
            m[p, 1:T - 1] = draw[row, 1:T - 1]
    if J == 32 and P > 1 and T > 2:
        m[1, 1, 31] = True
    return m


def flat(track):
    """[P,T,J,4] -> the poses [P*T,J,4] as the entry points take them"""
    return np.ascontiguousarray(track, np.float32).reshape((-1,) + track.shape[2:])


def case_mask(J, P=P, T=T):
    """make_mask with a held joint in frame 2 of pair 1 and frame 3 of pair 4, where odd_track puts its odd values"""
    m = make_mask(J, P, T)
    if not (m[1, 2].any() and m[4, 3].any()):      # few joints: hold joint 0 there
        m[1, 2, 0] = m[4, 3, 0] = True
    return m


def odd_track(case, mask, P=P, T=T):
    """the given track of a case with a NaN of a non-default payload in one held joint, a zero quaternion in another and a zero
    quaternion in an end frame -> (track, the three places)"""
    q = given_track(case, P, T).copy()
    j1, j2 = int(np.flatnonzero(mask[1, 2])[0]), int(np.flatnonzero(mask[4, 3])[0])
    q.view(np.uint32)[1, 2, j1, 1] = 0x7FC12345
    q[4, 3, j2] = 0.0
    q[2, 0, 0] = 0.0
    return q, ((1, 2, j1), (4, 3, j2), (2, 0, 0))


def pack(mask):
    """bool [P,T,J] -> uint32 [P*T], bit j = joint j"""
    mask = np.asarray(mask, bool)
    return sco.pack(mask.reshape(-1, mask.shape[-1]))


def end_words(observed, J, P=P, T=T):
    """the words of the pndf_project_options2 call that a track call with lambda 0 and PNDF_TRACK_GIVEN equals: all ones in the end frames"""
    w = (np.zeros(P * T, np.uint32) if observed is None else pack(observed)).reshape(P, T).copy()
    w[:, 0] = w[:, T - 1] = 0xFFFFFFFF
    return np.ascontiguousarray(w.reshape(-1))


# ---------------------------------------------------------------- the arithmetic, any J
def fill(a, b, T, mode="slerp", dtype=np.float32):
    """a, b [P,J,4] -> the filled track [P,T,J,4] in `dtype`: interpolation_oracle.fill without its 21"""
    assert T >= 2 and mode in ("slerp", "nlerp")
    dt = np.dtype(dtype).type
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    assert a.ndim == 3 and a.shape == b.shape and a.shape[2] == 4
    bp = align(a, b)
    track = np.empty((len(a), T) + a.shape[1:], dtype)
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
    """One band step on the track q [P,T,J,4] in q's dtype from d [P*T] and g [P,T,J,4]; observed: bool [P,T,J] or None.  Returns
    the new track (q is not modified): interpolation_oracle.band_step without its 21."""
    dt = q.dtype.type
    Pn, Tn, J = q.shape[:3]
    assert q.shape == (Pn, Tn, J, 4) and Tn >= 2 and 0.0 <= smooth <= 1.0
    g = np.asarray(g, dtype=dt).reshape(q.shape)
    d = np.asarray(d, dtype=dt).reshape(Pn, Tn, 1, 1)
    held = np.zeros((Pn, Tn, J), bool) if observed is None else np.asarray(observed, bool).reshape(Pn, Tn, J).copy()
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


def rounds(forward_grad, track, observed, steps, smooth, **opts):
    """`steps` rounds of { forward_grad(q [B,J,4]) -> (d [B], dq [B,J,4]) of the engine under test ; band_step in float32 } ->
    (track, d of the last round)"""
    cur, d = np.ascontiguousarray(track, np.float32).copy(), np.zeros(track.shape[0] * track.shape[1], np.float32)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        cur = np.ascontiguousarray(band_step(cur, d, g, observed, smooth, **opts), np.float32)
    return cur, d


def relax(track, sd, steps, act, parents, observed=None, smooth=0.0, dtype=np.float32, **opts):
    """free-running oracle: `steps` times skeleton_oracle.forward_grad + band_step -> (track, d of the last step [P*T], the smallest
    kink margin every pose met at the iterates before the updates [P*T])"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    d = np.zeros((q.shape[0] * q.shape[1], 1), dtype)
    margin = np.full(q.shape[0] * q.shape[1], np.inf)
    for _ in range(steps):
        d, g, m, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        margin = np.minimum(margin, m)
        q = band_step(q, d, g, observed, smooth, **opts)
    return q, np.asarray(d).reshape(-1), margin


def interpolate(a, b, T, sd, steps, act, parents, mode="slerp", observed=None, smooth=0.0, dtype=np.float32, **opts):
    """free-running oracle: fill, then relax"""
    return relax(fill(a, b, T, mode, dtype), sd, steps, act, parents, observed, smooth, dtype, **opts)


def assert_same(got, want, what=""):
    """equal bit patterns; where the specification gives a NaN the result is a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def inner(track):
    """the interior frames of a track as rows [P (T-2), 4 J]"""
    t = np.asarray(track)
    return t[:, 1:-1].reshape(-1, t.shape[2] * 4)


# ---------------------------------------------------------------- evenness
def segment_lengths(track):
    """[P,T,J,4] -> [P,T-1] in float64: the sum over the joints of 2 acos(min(|<q_k, q_k+1>|, 1))"""
    t = np.asarray(track, np.float64)
    dots = np.minimum(np.abs((t[:, :-1] * t[:, 1:]).sum(-1)), 1.0)
    return (2.0 * np.arccos(dots)).sum(-1)


def evenness(track):
    """(longest-to-mean segment ratio [P], path length [P]) of a track"""
    seg = segment_lengths(track)
    return seg.max(axis=1) / seg.mean(axis=1), seg.sum(axis=1)


EVEN_STEPS = 50


@functools.lru_cache(maxsize=None)
def oracle_evenness(case, act, smooth):
    """of the fp64 oracle on make_pairs(case): T = 7, 50 steps, renormalize="unit", slerp"""
    parents, sd = sko.case_network(case, act)
    a, b = make_pairs(case)
    out, d, _ = interpolate(a, b, T, sd, EVEN_STEPS, act, parents, smooth=smooth, dtype=np.float64, renormalize="unit")
    assert np.isfinite(out).all() and np.isfinite(d).all()
    return evenness(out)


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options3(lib, observed=None, frames=0, lam=0.0, fill=GIVEN, reserved2=0, size=None, step_size=1.0, renorm=0, tol=0.0, reserved=0):
    """a pndf_project_options3 (48 bytes) filled the documented way; `observed`: an address or None"""
    from posendf_amd.abi import ProjectOptions3
    o = ProjectOptions3()
    lib.pndf_default_project_options(ctypes.byref(o.base2.base))
    o.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.base2.base.step_size, o.base2.base.renorm, o.base2.base.tol = step_size, renorm, tol
    o.base2.observed, o.base2.reserved = observed, reserved
    o.frames, o.lambda_, o.fill, o.reserved2 = frames, lam, fill, reserved2
    return o


def c_from(lib, opts, observed=None, frames=0, lam=0.0, fill=GIVEN):
    """the 48-byte struct of keyword options (those of band_step)"""
    return c_options3(lib, observed, frames, lam, fill, step_size=opts.get("step_size", 1.0), renorm=sco.RENORM[opts.get("renormalize")],
                      tol=opts.get("tol", 0.0))


# what a caller of the C header writes: the snippet of the documentation, as strict C99
C99_SNIPPET = """#include "posendf_amd_skeleton.h"
int main(void) {
    static const uint32_t mask[4] = {0u, 0x80000001u, 0u, 0u};
    pndf_project_options3 o;
    pndf_default_project_options(&o.base2.base);
    o.base2.base.struct_size = sizeof o;
    o.base2.observed = mask;
    o.base2.reserved = 0;
    o.frames = 4;
    o.lambda = 0.5f;
    o.fill = PNDF_TRACK_SLERP;
    o.reserved2 = 0;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 48) + (int)(sizeof(pndf_project_options2) != 32) + (int)(PNDF_TRACK_GIVEN != 0 || PNDF_TRACK_NLERP != 2);
}
"""
