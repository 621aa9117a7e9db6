"""Test helper (not a test module) for the step options of `project` (include/posendf_amd.h pndf_project_options; DESIGN.md section 1
"The projection step"): the numpy statement sequence of one step, the free-running oracle built on
oracle.posendf_np.forward_grad, and the inputs / option sets of the reference-run fixture tests/golden/project_options.npz.

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `step` in float32 IS the
specification the device function and the host twin are held to bit for bit."""
import os

import numpy as np

from oracle import posendf_np as onp
from posendf_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "project_options.npz")
ACTS = ("lrelu", "softplus")
REGIME = dict(seed=0, gain=2.0, out_bias=0.1)      # "live" of tests/golden/make_golden.py
NPOSE = 24
# name -> (step_size, renormalize); the fourth set adds tol = the median of the initial d of its activation (fixture key tol_<act>)
OPTION_SETS = {"unit": (1.0, "unit"), "half_flip": (0.5, "unit_flip"), "half": (0.5, None), "unit_tol": (1.0, "unit")}
N_EDGE = 4
ZERO_QUAT = (2 * NPOSE + 3, 5)      # (pose, joint) of the edge pose with one zero quaternion


def make_inputs():
    """24 poses of seed 11, 24 signed poses of seed 12 and the four edge poses of tests/golden/make_golden.py:make_inputs: 52 in all"""
    q = np.concatenate([synth.make_poses(NPOSE, seed=11), synth.make_poses(NPOSE, seed=12, signed=True)])
    edge = synth.make_poses(N_EDGE, seed=13, signed=True)
    edge[0, :, 2] = 0.0            # zero component column -> eps clamp of F.normalize
    edge[1] *= 1e-3                # tiny pose
    edge[2, :, :] = edge[2, 0:1, :]  # all joints equal
    edge[3, 5, :] = 0.0            # one zero quaternion
    return np.concatenate([q, edge]).astype(np.float32)


def weights():
    return synth.make_weights(**REGIME)


def options(name, fixture, act):
    """keyword arguments of PoseNDF.project for an option set"""
    step_size, renorm = OPTION_SETS[name]
    tol = float(fixture[f"tol_{act}"]) if name == "unit_tol" else 0.0
    return dict(step_size=step_size, renormalize=renorm, tol=tol)


def step(q, d, g, step_size=1.0, renormalize=None, tol=0.0):
    """One step on q [B,21,4], d [B] or [B,1], g [B,21,4], in q's dtype; returns the new poses (q is not modified)."""
    dt = q.dtype.type
    q = q.reshape(-1, 21, 4)
    g = np.asarray(g, dtype=dt).reshape(-1, 21, 4)
    d = np.asarray(d, dtype=dt).reshape(-1, 1, 1)
    with np.errstate(all="ignore"):
        p = d * g
        s = dt(step_size) * p
        u = q - s
        if renormalize is not None:
            assert renormalize in ("unit", "unit_flip"), renormalize
            ss = ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]) + u[..., 3] * u[..., 3]
            n = np.sqrt(ss)
            den = np.where(n < dt(1e-12), dt(1e-12), n)      # clamp_min: a NaN norm stays NaN
            u = u / den[..., None]
            if renormalize == "unit_flip":
                u = np.where(u[..., :1] < 0, -u, u)
        if tol > 0:
            u = np.where(d < dt(tol), q, u)      # a NaN d compares false: not frozen
    assert u.dtype == q.dtype
    return u


def project(q, sd, steps, act, dtype=np.float32, snap_at=(), **opts):
    """Free-running oracle: `steps` times forward_grad + step.  Returns (q_out, d trace [steps, B], {k: q after k steps})."""
    q = np.asarray(q, dtype=dtype).reshape(-1, 21, 4)
    trace, snaps = [], {}
    for it in range(steps):
        d, g = onp.forward_grad(q, sd, act, dtype=dtype)
        q = step(q, d, g, **opts)
        trace.append(np.asarray(d).reshape(-1).copy())
        if it + 1 in snap_at:
            snaps[it + 1] = q.copy()
    return q, np.stack(trace), snaps


def kink_margin_along(q, sd, steps, act, **opts):
    """`margin` argument of conftest.outlier_gate for a free-running projection with options: the smallest kink margin
    (oracle.posendf_np.kink_margin) each pose meets at the iterates BEFORE each of the `steps` updates of its fp64 trajectory -- what
    conftest.traj_margin is for the plain loop.  None for softplus, which has no kinks."""
    if act == "softplus":
        return None
    q = np.asarray(q, dtype=np.float64).reshape(-1, 21, 4)
    margin = np.full(len(q), np.inf)
    for _ in range(steps):
        margin = np.minimum(margin, onp.kink_margin(q, sd, act))
        d, g = onp.forward_grad(q, sd, act, dtype=np.float64)
        q = step(q, d, g, **opts)
    return margin
