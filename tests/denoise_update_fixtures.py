"""Shared by tests/test_denoise_update_gpu.py: seeded inputs of ONE launch of pndf_denoise_update_kernel with the kernel's edges
planted, the loss weights of the two schedules rounded as the C ABI receives them, and the fp64 / fp32 results of
oracle/denoise_np.update_step, computed once per case and handed out read-only.  numpy only: nothing here needs a GPU."""
from __future__ import annotations

import functools

import numpy as np

from oracle import denoise_np as dn

LR = float(np.float32(0.02))                 # what a c_float argument of 0.02 holds: the same value on both sides
ONE_MINUS_BETA1 = np.float32(1.0 - 0.9)      # the kernel's fp32 constant (csrc/pndf_adam.h): m_out = fl(this * g) from zero moments
# (S, T): no temporal term | smallest with a neighbour | one workgroup of 11 frames exactly | the seams 10|11 and 21|22 | the c
# reduction with a second addend in one thread | with several addends per thread
SHAPES = [(1, 1), (2, 2), (3, 11), (2, 12), (1, 23), (2, 257), (1, 600)]
SCHEDULE_ITS = [("motion_denoise", 0), ("motion_denoise", 2), ("partial_observation", 0), ("partial_observation", 2)]
PLANTED_ANGLES = (1e-7, 9.9e-7, 1.1e-6, 1e-4, 3.1, 4.0)      # around the small-angle switch at 1e-6, and beyond pi


def weights(schedule, it):
    """(prior_coef, prior_power, temp_coef, data_coef) of the schedule, the coefficients rounded to the fp32 the C ABI carries"""
    from posendf_amd.motion_denoise import iteration_coefs
    pc, pp, tc, dc = iteration_coefs(schedule, it)
    return float(np.float32(pc)), pp, float(np.float32(tc)), float(np.float32(dc))


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(S, T, k, seed=0):
    """fp32 buffers of one launch.  theta: a random walk per sequence; theta0 = theta + N(0, 0.05); d ~ U(0.01, 0.2); dq ~ N(0, 1);
    g_body ~ N(0, 5); moments zero at k = 1, else mutually consistent (m = +-a U(0.1, 1), v = a^2 U(0.5, 2), a = 10^U(-3, 5)):
    with unrelated moments the "update" is a hundred radians.  Planted in sequence 0 (frame 0 unless said): joint 2 of frame
    min(2, T - 1) with zero rotation; joints 4..9 with the angles PLANTED_ANGLES; joint 10 identical in frames 0 and 1 (T > 1) and
    joint 12 identical in frames 10 and 11, across the workgroup seam (T > 11); joint 11 equal to its theta0."""
    rng = np.random.default_rng([seed, S, T, k])
    th = np.cumsum(rng.normal(size=(S, T, 69)) * 0.03, axis=1) + rng.normal(size=(S, 1, 69)) * 0.3
    th[0, min(2, T - 1), 6:9] = 0.0
    for j, ang in zip(range(4, 10), PLANTED_ANGLES):
        axis = rng.normal(size=3)
        th[0, 0, 3 * j:3 * j + 3] = axis / np.linalg.norm(axis) * ang
    if T > 1:
        th[0, 1, 30:33] = th[0, 0, 30:33]
    if T > 11:
        th[0, 11, 36:39] = th[0, 10, 36:39]
    th = th.astype(np.float32)
    th0 = (th + rng.normal(size=th.shape) * 0.05).astype(np.float32)
    th0[0, 0, 33:36] = th[0, 0, 33:36]
    out = {"theta": th, "theta0": th0, "d": rng.uniform(0.01, 0.2, (S, T)).astype(np.float32),
           "dq": rng.normal(size=(S, T, 21, 4)).astype(np.float32), "g_body": (rng.normal(size=th.shape) * 5.0).astype(np.float32)}
    if k == 1:
        out["m"], out["v"] = np.zeros_like(th), np.zeros_like(th)
    else:
        a = 10.0 ** rng.uniform(-3, 5, th.shape)
        out["m"] = (rng.choice([-1.0, 1.0], th.shape) * a * rng.uniform(0.1, 1.0, th.shape)).astype(np.float32)
        out["v"] = (a * a * rng.uniform(0.5, 2.0, th.shape)).astype(np.float32)
    ang = np.linalg.norm(th[0, 0].astype(np.float64).reshape(23, 3)[4:10], axis=-1)
    assert np.allclose(ang, PLANTED_ANGLES, rtol=1e-6) and (ang[:2] < 1e-6).all() and (ang[2:] > 1e-6).all()
    return {name: _frozen(a) for name, a in out.items()}


@functools.lru_cache(maxsize=None)
def oracle(S, T, k, w, body, dtype=np.float64, seed=0):
    """update_step on inputs(S, T, k, seed) under the weights tuple w: (g, theta_out, m_out, v_out, q_next), read-only"""
    x = inputs(S, T, k, seed)
    res = dn.update_step(x["theta"], x["theta0"], x["d"], x["dq"], x["m"], x["v"], w, k, LR, x["g_body"] if body else None, dtype)
    return tuple(_frozen(a) for a in res)


def rel_max(a, b):
    """max |a - b| / max |b|: the project's usual error of an array against its reference"""
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def rel_norm(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))
