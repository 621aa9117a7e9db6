"""Body models and motions that reach the ends of the ranges the split-precision body-model kernels' operand scales rest on
(posendf_amd/csrc/pndf_lbs_scales.h) -- a helper of tests/test_lbs_range.py and tests/test_lbs_range_gpu.py, no tests in it.

`synth.make_body_model` (shared with the benchmarks, left alone) draws one length unit, Gaussian pose dirs of one magnitude,
skinning weights in [0.05, 1], a dense joint regressor and zero betas.  A real SMPL file is heavy-tailed in all of these."""
import numpy as np

from posendf_amd.synth import make_body_model

KINDS = ("smpl_like", "no_correctives", "rigid")
UNITS = (1e-3, 1.0, 1e3)
MOTIONS = ("ordinary", "wide", "slow", "saturating")
COEFS = ((10.0, 0.0), (1e-3, 1e3), (1e3, 1e-3), (20.0, 50.0))      # (temporal, data) weights handed to terms_grad(coefs=...)
# "saturating": the two frames that are identical on purpose (the reference's NaN rows: no epsilon under the root)
SATURATING_TWINS = (10, 11)


def stress_model(V, seed, unit=1.0, kind="smpl_like", extra=None):
    """The dict of synth.make_body_model with SMPL's dynamic range; deterministic in `seed`.
    smpl_like       pose dirs x 10^U(-6, 1) entrywise, about half of them zero, largest entry ~1 cm; four skinning influences
                    per vertex drawn as 10^U(-7, 0) and normalised; <= 8 non-zeros per row of the (convex) joint regressor;
                    betas of a few sigma
    no_correctives  the same with posedirs = 0 (the packer's scale for P comes from a clamped zero bound)
    rigid           the same with one-hot skinning weights
    `unit` multiplies v_template, shapedirs and posedirs: 1e-3 / 1 / 1e3 = the model in kilometres / metres / millimetres."""
    if kind not in KINDS:
        raise ValueError(kind)
    if extra is None:
        extra = (3, V // 2, V - 1)
    m = dict(make_body_model(V=V, seed=seed, extra=extra))
    rng = np.random.default_rng([seed, 7919])
    J = len(m["parents"])
    pd = np.asarray(m["posedirs"], np.float64) * 10.0 ** rng.uniform(-6, 1, size=m["posedirs"].shape)
    pd[rng.random(pd.shape) < 0.5] = 0.0
    pd *= 0.01 / np.abs(pd).max()
    w = np.zeros((V, J))
    for v in range(V):
        idx = rng.choice(J, 4, replace=False)
        w[v, idx] = 10.0 ** rng.uniform(-7, 0, size=4)
    w /= w.sum(1, keepdims=True)
    jr = np.zeros((J, V))
    for j in range(J):
        idx = rng.choice(V, min(8, V), replace=False)
        jr[j, idx] = rng.random(len(idx)) ** 4 + 1e-3
    jr /= jr.sum(1, keepdims=True)
    betas = np.zeros(len(m["betas"]))
    betas[:3], betas[-1] = (2.5, -3.0, 1.5), -2.0
    if kind == "no_correctives":
        pd[:] = 0.0
    if kind == "rigid":
        one = np.zeros_like(w)
        one[np.arange(V), w.argmax(1)] = 1.0
        w = one
    u = np.float64(unit)
    m.update(v_template=(np.asarray(m["v_template"], np.float64) * u).astype(np.float32),
             shapedirs=(np.asarray(m["shapedirs"], np.float64) * u).astype(np.float32),
             posedirs=(pd * u).astype(np.float32), lbs_weights=w.astype(np.float32), J_regressor=jr.astype(np.float32),
             betas=betas.astype(np.float32))
    return m


_X, _Y, _Z, _D = 0, 1, 2, 3
_PI = np.pi
# (angle, axis) per frame: neighbours are never the same rotation (pi and 3 pi about one axis, or two of 0, 2 pi, 1e-4, 1e-7)
# except frames 10 and 11, which are the same frame
_SATURATING = ((_PI, _X), (2 * _PI, _X), (_PI, _Y), (1e-4, _Y), (_PI, _Z), (3 * _PI, _Y), (_PI, _D), (1e-7, _Z), (_PI, _X),
               (0.0, _X), (_PI, _Y), (_PI, _Y), (2 * _PI, _Z), (_PI, _Z), (3 * _PI, _X), (_PI, _D), (1e-4, _D))
assert _SATURATING[SATURATING_TWINS[0]] == _SATURATING[SATURATING_TWINS[1]]


def stress_theta(S, T, seed, motion):
    """theta [S, T, 69] float32.
    ordinary    a random walk of step 0.03 rad around a pose of amplitude 0.3 (the motions of tests/test_lbs_gpu.py)
    wide        step 0.3 around amplitude 3.0: angles wrap past pi
    slow        step 1e-3: neighbouring frames nearly coincide
    saturating  every joint of a frame at one exact special angle: pi about x, y, z and (1, 1, 1) / sqrt 3 (|R - I| = 2, the
                bound the pose feature's scale rests on), 2 pi and 3 pi, 1e-4 and 1e-7 (the tiny-angle end of the Rodrigues
                reverse pass), one all-zero frame, and frames SATURATING_TWINS identical; sequence s turns the axes s places on"""
    rng = np.random.default_rng([seed, S, T])
    if motion in ("ordinary", "wide", "slow"):
        amp, step = {"ordinary": (0.3, 0.03), "wide": (3.0, 0.3), "slow": (0.3, 1e-3)}[motion]
        th = np.cumsum(rng.normal(size=(S, T, 69)) * step, axis=1) + rng.normal(size=(S, 1, 69)) * amp
        if motion == "ordinary":
            th[0, min(2, T - 1), 6:9] = 0.0                     # a zero rotation
        return th.astype(np.float32)
    if motion != "saturating":
        raise ValueError(motion)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [3 ** -0.5] * 3])
    th = np.zeros((S, T, 23, 3))
    for s in range(S):
        for t in range(T):
            angle, axis = _SATURATING[t % len(_SATURATING)]
            th[s, t] = angle * axes[(axis + s) % 4]
    return th.reshape(S, T, 69).astype(np.float32)
