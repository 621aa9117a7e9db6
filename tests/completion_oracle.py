"""Test helper (not a test module) for pose completion (include/posendf_amd_completion.h; DESIGN.md section 2 "Pose completion"): the
masked step in numpy, the free-running oracle built on oracle.posendf_np.forward_grad, and the inputs, mask and option sets of the
reference-run fixture tests/golden/completion.npz.

The masked step is the step of tests/project_options_oracle.py on the joints that are not observed and the input's bits on those
that are; in float32 it IS the specification the step kernel and the host twin are held to bit for bit."""
import functools
import os

import numpy as np

import project_options_oracle as poo
from oracle import posendf_np as onp

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "completion.npz")
ACTS = poo.ACTS
STEPS = 10
# name -> (step_size, renormalize); "unit_tol" adds the tolerance of tests/golden/project_options.npz (key tol_<act>)
OPTION_SETS = {**poo.OPTION_SETS, "plain": (1.0, None)}
ALL_FREE, ALL_OBSERVED = 0, 1      # poses (rows of the mask) with no joint / every joint observed


def make_inputs():
    """the 52 poses of the projection-options fixture (24 + 24 signed + 4 edge poses)"""
    return poo.make_inputs()


def weights():
    return poo.weights()


def make_mask(B=52):
    """bool [B,21], True = observed: about half of the joints of every pose; pose 0 has none observed, pose 1 all of them.  B > 52
    tiles the 52 rows."""
    m = np.random.RandomState(5).rand(52, 21) < 0.5
    m[ALL_FREE] = False
    m[ALL_OBSERVED] = True
    reps = -(-B // 52)
    return np.ascontiguousarray(np.tile(m, (reps, 1))[:B])


def pack(mask):
    """bool [B,21] -> uint32 [B], bit j = joint j (the `observed` argument of pndf_complete)"""
    mask = np.asarray(mask, bool).reshape(-1, 21)
    return np.ascontiguousarray((mask.astype(np.uint32) << np.arange(21, dtype=np.uint32)).sum(axis=1, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _tols():
    fx = np.load(poo.FIXTURE)
    return {act: float(fx[f"tol_{act}"]) for act in ACTS}


def options(name, act):
    """keyword arguments of PoseNDF.complete (and of step_masked) for an option set"""
    step_size, renorm = OPTION_SETS[name]
    return dict(step_size=step_size, renormalize=renorm, tol=_tols()[act] if name == "unit_tol" else 0.0)


def step_masked(q, d, g, observed, **opts):
    """One masked step on q [B,21,4] in q's dtype: observed [B,21] bool joints keep their bits, the others take poo.step."""
    q = q.reshape(-1, 21, 4)
    observed = np.asarray(observed, bool).reshape(-1, 21)
    return np.where(observed[..., None], q, poo.step(q, d, g, **opts))


def complete(q, sd, observed, steps, act, dtype=np.float32, snap_at=(), **opts):
    """Free-running oracle: `steps` times forward_grad + step_masked.  Returns (q_out, d trace [steps, B], {k: q after k steps})."""
    q = np.asarray(q, dtype=dtype).reshape(-1, 21, 4)
    trace, snaps = [], {}
    for it in range(steps):
        d, g = onp.forward_grad(q, sd, act, dtype=dtype)
        q = step_masked(q, d, g, observed, **opts)
        trace.append(np.asarray(d).reshape(-1).copy())
        if it + 1 in snap_at:
            snaps[it + 1] = q.copy()
    return q, np.stack(trace), snaps


def kink_margin_along(q, sd, observed, steps, act, **opts):
    """poo.kink_margin_along for the masked trajectory: the smallest kink margin each pose meets at the iterates before each of the
    `steps` updates of its fp64 trajectory; None for softplus"""
    if act == "softplus":
        return None
    q = np.asarray(q, dtype=np.float64).reshape(-1, 21, 4)
    margin = np.full(len(q), np.inf)
    for _ in range(steps):
        margin = np.minimum(margin, onp.kink_margin(q, sd, act))
        d, g = onp.forward_grad(q, sd, act, dtype=np.float64)
        q = step_masked(q, d, g, observed, **opts)
    return margin


def check_inputs():
    """In fp64, with these inputs: ten masked steps stay finite for every pose, both activations and every option set, and the
    all-observed pose keeps a constant distance (it never moves)."""
    q, sd, m = make_inputs(), weights(), make_mask()
    assert q.shape == (52, 21, 4) and m.shape == (52, 21) and not m[ALL_FREE].any() and m[ALL_OBSERVED].all()
    assert 0.4 < m[2:].mean() < 0.6 and m[2:].any(axis=1).all() and not m[2:].all(axis=1).any()
    for act in ACTS:
        for name in OPTION_SETS:
            out, trace, _ = complete(q, sd, m, STEPS, act, dtype=np.float64, **options(name, act))
            assert np.isfinite(out).all() and np.isfinite(trace).all(), (act, name)
            assert (trace[:, ALL_OBSERVED] == trace[0, ALL_OBSERVED]).all(), (act, name)
            assert (out[m] == q.astype(np.float64)[m]).all(), (act, name)
