"""Pin oracle/denoise_np.py (the checker of the fused motion-denoise step) on vectors produced by the imported reference
network inside the reference's optimisation loop (tests/golden/make_golden_denoise.py).  CPU only."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_weights
from oracle import denoise_np as dn


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "denoise_live.npz")))


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_loop_matches_reference_fp64(gold, act):
    sd = golden_weights("live")
    _, hist = dn.optimize(gold["theta0"].astype(np.float64), sd, iterations=2, steps_per_iter=4, act=act, trace=True)
    want = gold[f"{act}_theta_f64"]
    for k, th in enumerate(hist):
        err = np.abs(th - want[k]).max()
        assert err < 1e-9, (k, err)
    assert np.array_equal(hist[-1][:, 63:], gold["theta0"][:, 63:].astype(np.float64))     # hand joints never move


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_weighted_terms_match_reference(gold, act):
    sd = golden_weights("live")
    th = gold["theta0"].astype(np.float64)
    for it, prev in [(0, None), (1, 3)]:
        cur = th if prev is None else gold[f"{act}_theta_f64"][prev]
        _, terms = dn.step_gradient(cur, th, sd, it, act)
        ref = gold[f"{act}_terms_f64"][0 if prev is None else prev + 1]      # sorted keys: data, pose_pr, temp
        for name, val in zip(sorted(terms), ref):
            assert abs(terms[name] - val) <= 1e-9 * abs(val), (name, terms[name], val)


def test_fp32_loop_stays_close_to_fp64(gold):
    """Adam turns a gradient into a step of ~lr regardless of its size, so fp32 rounding is not amplified: the fp32
    loop tracks the fp64 one (the envelope the GPU tests use for the engine-backed loops)."""
    sd = golden_weights("live")
    out = dn.optimize(gold["theta0"], sd, iterations=2, steps_per_iter=4, dtype=np.float32)
    ref32, ref64 = gold["lrelu_theta_f32"][-1], gold["lrelu_theta_f64"][-1]
    assert np.abs(out - ref64).max() < 5e-4 and np.abs(ref32 - ref64).max() < 5e-4


def test_aa2quat_jacobian_finite_difference():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(50, 3)) * 0.7
    a[0] = 0.0
    gq = rng.normal(size=(50, 4))
    an = dn.aa2quat_vjp(a, gq)
    h = 1e-6
    for e in range(3):
        da = np.zeros_like(a)
        da[:, e] = h
        fd = ((dn.axis_angle_to_quaternion(a + da)[0] - dn.axis_angle_to_quaternion(a - da)[0]) / (2 * h) * gq).sum(-1)
        assert np.allclose(fd[1:], an[1:, e], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("schedule", ["motion_denoise", "partial_observation"])
def test_update_step_replays_the_pinned_loop(schedule):
    """update_step (one kernel launch's arithmetic, d and dq given) against optimize, which the tests above pin to the
    reference's trajectory: the same steps replayed with d, dq from the oracle network and m, v carried, 1e-12 absolute."""
    from oracle import posendf_np as onp
    from posendf_amd.motion_denoise import iteration_coefs
    sd = golden_weights("live")
    rng = np.random.default_rng(3)
    th0 = np.cumsum(rng.normal(size=(2, 5, 69)) * 0.03, axis=1) + rng.normal(size=(2, 1, 69)) * 0.3
    _, hist = dn.optimize(th0, sd, iterations=2, steps_per_iter=2, trace=True, schedule=schedule)
    th, m, v, k = th0.copy(), np.zeros_like(th0), np.zeros_like(th0), 0
    for it in range(2):
        for _ in range(2):
            k += 1
            q = dn.axis_angle_to_quaternion(th.reshape(2, 5, 23, 3)[:, :, :21])[0]
            d, dq = onp.forward_grad(q.reshape(10, 21, 4), sd, "lrelu", 100.0, np.float64)
            g, th, m, v, qn = dn.update_step(th, th0, d.reshape(2, 5), dq.reshape(2, 5, 21, 4), m, v,
                                             iteration_coefs(schedule, it), k, 0.02)
            err = np.abs(th - hist[k - 1]).max()
            assert err <= 1e-12, (schedule, k, err)
            assert np.array_equal(qn, dn.axis_angle_to_quaternion(th.reshape(2, 5, 23, 3)[:, :, :21])[0])
            assert not g[:, :, 63:].any() and not m[:, :, 63:].any()          # hand joints: zero gradient, zero moments
    assert k == 4 and np.abs(th - th0).max() > 0.02


@pytest.mark.parametrize("weights", [(1e7 / 3, 2, 30.0, 100.0 / 3), (100.0 / 3, 1, 300.0, 10.0 / 3), (1e7, 2, 10.0, 0.0)])
def test_update_step_gradient_against_autograd(weights):
    """update_step's g against torch autograd of the scalar objective it differentiates: d, dq constant, the distance linearised
    around the current pose, c = mean_t (d + <dq, q(theta) - q(theta_now)>), prior prior_coef c^p, plus the surrogates."""
    import torch
    from posendf_amd.motion_denoise import axis_angle_to_quaternion
    rng = np.random.default_rng(11)
    S, T = 2, 6
    th_np = np.cumsum(rng.normal(size=(S, T, 69)) * 0.03, axis=1) + rng.normal(size=(S, 1, 69)) * 0.3
    th0 = torch.from_numpy(th_np + rng.normal(size=th_np.shape) * 0.05)
    d, dq = torch.from_numpy(rng.uniform(0.01, 0.2, (S, T))), torch.from_numpy(rng.normal(size=(S, T, 21, 4)))
    pc, pp, tc, dc = weights
    th = torch.from_numpy(th_np).requires_grad_(True)
    a = th.reshape(S, T, 23, 3)[:, :, :21]
    q = axis_angle_to_quaternion(a)
    c = (d + (dq * (q - q.detach())).sum(dim=(-1, -2))).mean(dim=1)
    norm = lambda x: torch.sqrt((x * x).sum(dim=-1) + dn.SURROGATE_EPS).mean(dim=(1, 2))      # noqa: E731
    loss = pc * c ** pp + tc * norm(a[:, :-1] - a[:, 1:])
    if dc:
        loss = loss + dc * norm(a - th0.reshape(S, T, 23, 3)[:, :, :21])
    loss.sum().backward()
    z = np.zeros_like(th_np)
    g = dn.update_step(th_np, th0.numpy(), d.numpy(), dq.numpy(), z, z, weights, 1, 0.02)[0]
    err = np.abs(g - th.grad.numpy()).max() / np.abs(g).max()
    assert err < 1e-9, err
    # the body-model form: the given gradient on all 23 joints, no surrogate
    gb = rng.normal(size=th_np.shape) * 5.0
    th.grad = None
    q = axis_angle_to_quaternion(th.reshape(S, T, 23, 3)[:, :, :21])
    c = (d + (dq * (q - q.detach())).sum(dim=(-1, -2))).mean(dim=1)
    ((pc * c ** pp).sum() + (th * torch.from_numpy(gb)).sum()).backward()
    g = dn.update_step(th_np, th0.numpy(), d.numpy(), dq.numpy(), z, z, weights, 1, 0.02, g_body=gb)[0]
    err = np.abs(g - th.grad.numpy()).max() / np.abs(g).max()
    assert err < 1e-9, err
