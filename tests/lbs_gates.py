"""Marginal gates of the body-model tests (tests/test_lbs_gpu.py, tests/test_lbs_range_gpu.py, tests/test_lbs_range.py) -- a
helper, no tests in it.

The older gates of those modules divide the largest error of a whole [T, 69] gradient or [N, V, 3] vertex block by the largest
entry of the block, and compare with a fixed number (1e-5 forward, max(1e-4, 8 ref) gradient).  Here every joint, every vertex
and every frame is held on its own, at the error the REFERENCE ARITHMETIC itself makes there:

  envelope   the reference arithmetic evaluated DRAWS times on inputs perturbed by a relative 2^-23 (one fp32 rounding, the
             convention of conftest.fp32_noise; the same seeded draws everywhere): elementwise max |ref_k - x64| against the
             fp64 oracle.  The reference arithmetic is oracle/lbs_np.py in float32 -- for the fp32 kernels, the joints-only
             forward and the general reverse pass -- and the same with its four contractions in the split kernels' stated
             arithmetic (lbs_np.split_contractions at the scales pndf_debug_lbs_scales reads out) for the f16x3 kernels.
  marginals  gradient [S, T, 23, 3]: every (sequence, joint) over all frames, every (sequence, frame) over all joints;
             Jtr and vertices [N, K, 3]: every joint / vertex over all frames, every frame over all joints / vertices.
  gate       max |got - x64| over m  <=  FACTOR x max over the draws of max |ref_k - x64| over m  +  FLOOR x max |x64| over m
             FACTOR = 8: the `8 ref` of the older gradient gate and conftest.pose_gate's default factor.  FLOOR = 2^-22: four
             units in the last place of an fp32 result of the marginal's size, for a marginal on which every draw happens
             to be exact.  A marginal that is zero in fp64 and in every draw has bound 0: the result there must be zero.
Rows (frames) the fp64 oracle makes non-finite are left out of every marginal (`ok`); that they are non-finite in the result
too, and no others, is asserted by the callers as before.  The reference is always an argument, never the result under test."""
import numpy as np

from oracle import lbs_np

DRAWS, FACTOR, FLOOR, SEED = 8, 8.0, 2.0 ** -22, 1
GRADIENT = {"joint": (1, 3), "frame": (2, 3)}         # axes reduced, of [S, T, 23, 3]
JOINTS = {"joint": (0, 2), "frame": (1, 2)}           # of [N, 45, 3]
VERTICES = {"vertex": (0, 2), "frame": (1, 2)}        # of [N, V, 3]
RATIOS = []      # (what, kind, worst ratio) of every gate() of the process, in call order


def perturbed(inputs, k):
    """draw k of the inputs (None stays None): float32, every entry times 1 + e, |e| <= 2^-23"""
    out = []
    for i, x in enumerate(inputs):
        if x is not None:
            x = np.asarray(x, np.float32)
            x = (x * (1 + np.random.default_rng([SEED, k, i]).uniform(-2.0 ** -23, 2.0 ** -23, x.shape))).astype(np.float32)
        out.append(x)
    return out


def envelope(ref, inputs, x64, draws=range(DRAWS)):
    """elementwise max over the draws of |ref(*perturbed inputs) - x64|; `ref` returns one array or a tuple of them, `x64`
    likewise; returns the like"""
    single = not isinstance(x64, (tuple, list))
    truth = [x64] if single else list(x64)
    env = [np.zeros(np.shape(t)) for t in truth]
    for k in draws:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            r = ref(*perturbed(inputs, k))
            r = [r] if single else list(r)
            env = [np.fmax(e, np.abs(np.asarray(rk, np.float64) - t)) for e, rk, t in zip(env, r, truth)]
    return env[0] if single else tuple(env)


def marginal_ratios(got, x64, env, kinds, ok=None):
    """{kind: worst error / bound over the marginals of that kind}; `ok` [leading axes]: the rows that count"""
    got, x64, env = np.asarray(got, np.float64), np.asarray(x64, np.float64), np.asarray(env, np.float64)
    assert got.shape == x64.shape == env.shape, (got.shape, x64.shape, env.shape)
    with np.errstate(invalid="ignore"):
        err, size = np.abs(got - x64), np.abs(x64)
    if ok is not None:
        keep = np.asarray(ok, bool).reshape(np.shape(ok) + (1,) * (got.ndim - np.ndim(ok)))
        err, size, env = (np.where(keep, a, 0.0) for a in (err, size, env))
    worst = {}
    for kind, axes in kinds.items():
        e, bound = err.max(axes), FACTOR * env.max(axes) + FLOOR * size.max(axes)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(e == 0, 0.0, e / bound)      # (error on a zero bound: inf; a non-finite result: nan)
        worst[kind] = float(ratio.max()) if ratio.size else 0.0
    return worst


def gate(what, got, x64, env, kinds, ok=None):
    """marginal_ratios, printed, recorded in RATIOS and asserted: every marginal inside its bound"""
    worst = marginal_ratios(got, x64, env, kinds, ok)
    print(f"[lbs_gate {what}] " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "  (error / bound, 1 = at the gate)")
    RATIOS.extend((what, k, v) for k, v in worst.items())
    for kind, v in worst.items():
        assert v <= 1.0, (what, kind, v)
    return worst


# ---------------------------------------------------------------- the reference arithmetics
def schedule_coefs(it):
    """pndf_lbs_terms_grad: temp 10 (1 + it), data 100 / (1 + it) for it > 0, formed in float"""
    return float(np.float32(10) * np.float32(1 + it)), float(np.float32(100) / np.float32(1 + it)) if it > 0 else 0.0


def arithmetic(precision, model, T=2, coefs=(0.0, 0.0)):
    """the `contract` hook of the reference arithmetic: None (float32 throughout) for "fp32", the split arithmetic at the
    library's own scales for this model, sequence length and term weights for "f16x3" """
    if precision == "fp32":
        return None
    assert precision == "f16x3", precision
    from posendf_amd import engine
    from test_lbs_oracle import _pack
    from test_lbs_range import read_scales, term_weights
    return lbs_np.split_contractions(read_scales(engine.load_library(), _pack(model), *term_weights(model, T, coefs)))


def forward_ref(model, contract=None):
    """theta [N, 69] -> (vertices, joints) in float32"""
    return lambda theta: lbs_np.lbs(theta, model, np.float32, contract=contract)


def terms_ref(model, it, coefs=None, contract=None, dtype=np.float32):
    """theta [S, T, 69], joints0 [S, T, nj, 3] or None -> the gradient of body_terms [S, T, 23, 3], sequence by sequence"""
    def ref(theta, joints0):
        rows = [lbs_np.body_terms(theta[s], None if joints0 is None else np.asarray(joints0[s], dtype), model, it, dtype, coefs=coefs,
                                  contract=contract)[0] for s in range(theta.shape[0])]
        return np.stack(rows).reshape(theta.shape[0], theta.shape[1], 23, 3)
    return ref


def vjp_ref(model, dtype=np.float32):
    """theta [N, 69], g_verts, g_joints -> lbs_vjp [1, N, 23, 3] (the general reverse pass: fp32 under either setting)"""
    def ref(theta, g_verts, g_joints):
        cache = lbs_np.lbs(theta, model, dtype, keep=True)[2]
        return lbs_np.lbs_vjp(model, cache, g_verts, g_joints, dtype).reshape(1, theta.shape[0], 23, 3)
    return ref
