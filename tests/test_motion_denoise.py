"""Motion-denoise driver: CPU checks of the host logic, GPU parity of the optimisation loop
against the same loop around the PyTorch-CPU oracle network.  These are LOOP tests: they see the update kernel through Adam, which
hides the gradient's scale, and compare final poses only.  The kernel-level checks -- one launch of pndf_denoise_update_kernel on
buffers of the test's own making: gradient, moments, update and next quaternions against oracle/denoise_np.update_step and
torch.optim.Adam, the three C entry points, the kernel's edges -- are in tests/test_denoise_update_gpu.py."""
import numpy as np
import pytest
import torch

from conftest import golden_weights


def test_axis_angle_to_quaternion_convention():
    from posendf_amd.motion_denoise import axis_angle_to_quaternion
    aa = torch.tensor([[0.0, 0.0, 0.0], [np.pi, 0.0, 0.0], [0.0, np.pi / 2, 0.0], [1e-8, 0.0, 0.0]], dtype=torch.float64)
    q = axis_angle_to_quaternion(aa)
    assert torch.allclose(q[0], torch.tensor([1.0, 0, 0, 0], dtype=torch.float64))
    assert torch.allclose(q[1], torch.tensor([0.0, 1, 0, 0], dtype=torch.float64), atol=1e-12)
    s = np.sin(np.pi / 4)
    assert torch.allclose(q[2], torch.tensor([s, 0, s, 0], dtype=torch.float64))
    assert torch.allclose(q[3], torch.tensor([1.0, 5e-9, 0, 0], dtype=torch.float64))
    x = torch.randn(100, 3, dtype=torch.float64)
    assert torch.allclose(axis_angle_to_quaternion(x).norm(dim=-1), torch.ones(100, dtype=torch.float64))
    # gradient through the small-angle branch is finite
    z = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    axis_angle_to_quaternion(z).sum().backward()
    assert torch.isfinite(z.grad).all()


def test_weight_schedule_matches_reference_formulas():
    from posendf_amd.motion_denoise import loss_weights
    w = loss_weights()
    c = torch.tensor(0.03)
    for it in (0, 1, 4, 9):
        assert torch.isclose(w["temp"](c, it), 10.0 * c * (1 + it))
        assert torch.isclose(w["data"](c, it), 100.0 * c / (1 + it))
        assert torch.isclose(w["pose_pr"](c, it), 1e7 * c * c / (1 + it))


class _OraclePrior(torch.nn.Module):
    """The oracle network behind the reference's call signature (checker only)."""

    def __init__(self, act, sd):
        super().__init__()
        from oracle.posendf_torch import RefNet
        self.net = RefNet(act)
        self.net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})

    def forward(self, pose, train=False):
        return {"dist_pred": self.net(pose)}


def _noisy_sequences(S, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    walk = torch.cumsum(0.02 * torch.randn(S, T, 69, generator=g), dim=1) + 0.3 * torch.randn(S, 1, 69, generator=g)
    return walk + 0.1 * torch.randn(S, T, 69, generator=g)


def test_loop_runs_on_cpu_with_oracle_prior():
    from posendf_amd.motion_denoise import MotionDenoise
    md = MotionDenoise(_OraclePrior("lrelu", golden_weights("live")), device="cpu")
    noisy = _noisy_sequences(2, 8)
    out, hist = md.denoise(noisy, iterations=2, steps_per_iter=3)
    assert out.shape == noisy.shape and len(hist) == 6
    assert "data" not in hist[0] and "data" in hist[-1]                # data term only for it > 0 (:92)
    assert hist[2]["pose_pr"] < hist[0]["pose_pr"]                     # the (dominant) prior term is descended


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_denoise_matches_oracle_loop(precision):
    """Same optimisation loop, pose prior from the HIP engine vs from the PyTorch-CPU oracle network."""
    from posendf_amd import PoseNDF, amass_config
    from posendf_amd.motion_denoise import MotionDenoise
    sd = golden_weights("live")
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    noisy = _noisy_sequences(3, 12, seed=1)
    got, h_gpu = MotionDenoise(net, device="cuda:0").denoise(noisy, iterations=2, steps_per_iter=10)
    ref, h_cpu = MotionDenoise(_OraclePrior("lrelu", sd), device="cpu").denoise(noisy, iterations=2, steps_per_iter=10)
    assert abs(h_gpu[0]["pose_pr"] - h_cpu[0]["pose_pr"]) < 1e-5 * abs(h_cpu[0]["pose_pr"]) + 1e-8
    # Adam normalises gradients, so tiny gradient differences are not amplified; 20 steps stay close
    err = (got.cpu() - ref).abs().max().item()
    assert err < 2e-3, err
    moved = (ref - noisy).abs().max().item()
    assert moved > 0.05 and err < 0.05 * moved


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_fused_step_matches_autograd_driver(precision):
    """optimize(fused=True) -- engine launch + pndf_denoise_update, no PyTorch in the loop -- against the autograd
    driver around the same engine: same terms, same Adam; differences are rounding order only."""
    from posendf_amd import PoseNDF, amass_config
    from posendf_amd.motion_denoise import MotionDenoise
    sd = golden_weights("live")
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    noisy = _noisy_sequences(5, 31, seed=3)
    noisy[0, 3, 6:9] = 0.0                                   # a zero rotation: small-angle branch and its Jacobian
    md = MotionDenoise(net, device="cuda:0")
    # one step: the update is lr * sign-like, so compare the step itself tightly
    a1, _ = md.denoise(noisy, iterations=1, steps_per_iter=1, record=False)
    f1, _ = md.denoise(noisy, iterations=1, steps_per_iter=1, fused=True)
    assert (a1 - f1).abs().max().item() < 2e-4               # Adam's first step is lr * g / (|g| + eps): +-lr unless g ~ 0
    ref, _ = md.denoise(noisy, iterations=2, steps_per_iter=10, record=False)
    got, _ = md.denoise(noisy, iterations=2, steps_per_iter=10, fused=True)
    assert torch.isfinite(got).all()
    # 20 steps: d d / d q is discontinuous at activation kinks and Adam turns a flipped gradient component into a
    # +-lr step, so a few elements drift apart; the bulk must agree to rounding
    diff = (got - ref).abs().flatten()
    moved = (ref.cpu() - noisy).abs().max().item()
    print(f"fused vs autograd driver after 20 steps: median {diff.median().item():.2e} p99 "
          f"{diff.kthvalue(int(0.99 * diff.numel())).values.item():.2e} max {diff.max().item():.2e} (moved {moved:.2f})")
    assert diff.median().item() < 1e-5
    assert (diff > 1e-3).float().mean().item() < 0.01
    assert diff.max().item() < 0.1 * moved
    assert torch.equal(got[..., 63:].cpu(), noisy[..., 63:])  # hand joints: no term, Adam leaves them in place


@pytest.mark.gpu
def test_aa2quat_kernel_matches_restatement():
    import ctypes
    from posendf_amd.engine import load_library
    from posendf_amd.motion_denoise import axis_angle_to_quaternion
    lib = load_library()
    theta = (0.8 * torch.randn(257, 69)).cuda()
    theta[5, 0:3] = 0.0
    theta[6, 3:6] = 1e-8
    q = torch.empty(257, 21, 4, device="cuda")
    assert lib.pndf_aa2quat(theta.data_ptr(), q.data_ptr(), 257, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    want = axis_angle_to_quaternion(theta.reshape(257, 23, 3)[:, :21])
    assert torch.allclose(q, want, atol=2e-7, rtol=1e-6)


# ---------------------------------------------------------------- round 2: independent oracle, cfg-5 size, body model
def _gold():
    import os
    from conftest import GOLDEN
    return dict(np.load(os.path.join(GOLDEN, "denoise_live.npz")))


def _engine_net(act, precision, sd=None):
    from posendf_amd import PoseNDF, amass_config
    cfg = amass_config(act, "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in (sd or golden_weights("live")).items()})
    return net.eval()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "autograd"])
@pytest.mark.parametrize("act,precision", [("lrelu", "fp32"), ("lrelu", "f16x3"), ("softplus", "f16x3")])
def test_denoise_matches_reference_loop(act, precision, fused):
    """Both product loops -- the fused HIP step (pndf_aa2quat + pndf_forward_grad + pndf_denoise_update) and the autograd
    driver -- against the trajectory that the imported reference network produced inside the reference's optimisation
    loop (tests/golden/make_golden_denoise.py: torch autograd + torch.optim.Adam, fp64), and against the numpy oracle of
    the step (oracle/denoise_np.py, pinned on the same vectors)."""
    from oracle import denoise_np as dn
    from posendf_amd.motion_denoise import MotionDenoise
    g = _gold()
    md = MotionDenoise(_engine_net(act, precision), device="cuda:0")
    theta0 = torch.from_numpy(g["theta0"])
    # first step: Adam's bias-corrected first update is lr * g / (|g| + eps), i.e. -+lr for every element with a gradient
    one, _ = md.denoise(theta0, iterations=1, steps_per_iter=1, fused=fused, record=False)
    want1 = g[f"{act}_theta_f64"][0]
    assert np.abs(one.cpu().numpy() - want1).max() < 1e-5
    out, _ = md.denoise(theta0, iterations=2, steps_per_iter=4, fused=fused, record=False)
    want = g[f"{act}_theta_f64"][-1]
    err = np.abs(out.cpu().numpy() - want)
    ref_err = np.abs(g[f"{act}_theta_f32"][-1] - want)            # the reference loop's own fp32 run
    moved = np.abs(want - g["theta0"]).max()
    print(f"{act} {precision} fused={fused}: max err {err.max():.2e} median {np.median(err):.2e} | reference fp32 loop "
          f"{ref_err.max():.2e} | moved {moved:.3f}")
    assert np.median(err) < 1e-6 and err.max() < max(5e-4, 4 * ref_err.max())
    assert np.array_equal(out.cpu().numpy()[:, 63:], g["theta0"][:, 63:])        # hand joints: no term, never move
    # the numpy oracle of the loop in fp32 lands in the same envelope
    o32 = dn.optimize(g["theta0"], golden_weights("live"), iterations=2, steps_per_iter=4, act=act, dtype=np.float32)
    assert np.abs(o32 - want).max() < max(5e-4, 4 * ref_err.max())


@pytest.mark.gpu
def test_denoise_config5_size():
    """BASELINE.json configs[4]: 512 sequences x 300 frames (one GPU holds all of them here; 8 GPUs shard whole
    sequences).  A few Adam steps of the fused loop at full size: finite, sequences independent (a permuted batch gives
    the permuted result bit for bit), agreement with the autograd driver, and one sequence against the numpy oracle."""
    from oracle import denoise_np as dn
    from posendf_amd.motion_denoise import MotionDenoise
    S, T, steps = 512, 300, 3
    sd = golden_weights("live")
    md = MotionDenoise(_engine_net("lrelu", "f16x3", sd), device="cuda:0")
    noisy = _noisy_sequences(S, T, seed=7)
    out, _ = md.denoise(noisy, iterations=1, steps_per_iter=steps, fused=True)
    assert out.shape == (S, T, 69) and torch.isfinite(out).all()
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(1))
    out_p, _ = md.denoise(noisy[perm], iterations=1, steps_per_iter=steps, fused=True)
    assert torch.equal(out[perm.cuda()], out_p)
    auto, _ = md.denoise(noisy[:16], iterations=1, steps_per_iter=steps, fused=False, record=False)
    diff = (auto - out[:16]).abs()
    assert diff.median().item() < 1e-6 and (diff > 1e-3).float().mean().item() < 0.01
    s = 37
    want = dn.optimize(noisy[s].numpy().astype(np.float64), sd, iterations=1, steps_per_iter=steps)
    err = np.abs(out[s].cpu().numpy() - want)
    assert np.median(err) < 1e-6 and (err > 1e-3).mean() < 0.01, (np.median(err), err.max())
    # second outer iteration switches the data term on (:92) and changes the weights
    out2, _ = md.denoise(noisy[:64], iterations=2, steps_per_iter=2, fused=True)
    want2 = dn.optimize(noisy[5].numpy().astype(np.float64), sd, iterations=2, steps_per_iter=2)
    err2 = np.abs(out2[5].cpu().numpy() - want2)
    assert np.median(err2) < 1e-6 and (err2 > 1e-3).mean() < 0.01


class _LinearBlendBody:
    """A small differentiable stand-in for the SMPL body model of experiments/body_model.py:11-53 (third-party code +
    licensed model files, not available offline): 40 "vertices" and 24 "joints" as fixed random linear blends of the
    joint rotation matrices' first columns -- enough to exercise the body-model terms of the objective
    (motion_denoise.py:86-94: vertex temporal term, joint data term) end to end."""

    def __init__(self, device, dtype=torch.float32, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.wv = (torch.randn(63, 40 * 3, generator=g) / 8).to(device, dtype)
        self.wj = (torch.randn(63, 24 * 3, generator=g) / 8).to(device, dtype)

    def __call__(self, pose_body):                       # [N,69] -> (vertices [N,40,3], joints [N,24,3])
        x = torch.sin(pose_body[:, :63])
        return (x @ self.wv).reshape(-1, 40, 3), (x @ self.wj).reshape(-1, 24, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_body_model_terms_are_pluggable(precision):
    """a user-supplied differentiable body model drives the temporal / data terms; the pose prior still
    comes from the HIP engine through its autograd contract.  Checked against the same loop around the PyTorch-CPU
    oracle network (reference arithmetic), and against the loop WITHOUT the body model (the terms must matter)."""
    from posendf_amd.motion_denoise import MotionDenoise
    sd = golden_weights("live")
    net = _engine_net("lrelu", precision, sd)
    noisy = _noisy_sequences(2, 10, seed=11)
    got, h = MotionDenoise(net, body_model=_LinearBlendBody("cuda:0"), device="cuda:0").denoise(
        noisy, iterations=2, steps_per_iter=5)
    ref, h_ref = MotionDenoise(_OraclePrior("lrelu", sd), body_model=_LinearBlendBody("cpu"), device="cpu").denoise(
        noisy, iterations=2, steps_per_iter=5)
    assert "temp" in h[0] and "data" in h[-1] and abs(h[0]["temp"] - h_ref[0]["temp"]) < 1e-5 * abs(h_ref[0]["temp"])
    err = (got.cpu() - ref).abs()
    assert err.median().item() < 1e-5 and err.max().item() < 5e-3, (err.median().item(), err.max().item())
    plain, _ = MotionDenoise(net, device="cuda:0").denoise(noisy, iterations=2, steps_per_iter=5, record=False)
    # the body-model terms changed the solution (slightly: the prior's 1e7 weight dominates every Adam step)
    assert (plain.cpu() - got.cpu()).abs().max().item() > 2e-5
    with pytest.raises(ValueError):
        MotionDenoise(net, body_model=_LinearBlendBody("cuda:0"), device="cuda:0").denoise(noisy, fused=True)


def test_optimize_calls_a_plain_callable_positionally():
    """optimize() must call a user's body model the way _geometry does: positionally -- a callable whose
    parameter is not named `pose_body` used to run the whole optimisation and then fail in the final v2v computation."""
    from posendf_amd.motion_denoise import MotionDenoise
    inner = _LinearBlendBody("cpu")

    def body(theta):                                     # positional, another parameter name
        return inner(theta)
    md = MotionDenoise(_OraclePrior("lrelu", golden_weights("live")), body_model=body, device="cpu")
    v2v = md.optimize(_noisy_sequences(1, 6, seed=4)[0], iterations=1, steps_per_iter=2)
    assert v2v.shape == () and np.isfinite(v2v) and v2v >= 0


def test_body_model_hook_cpu():
    """The body-model plumbing itself, without a GPU: gradients of the vertex / joint terms reach the poses."""
    from posendf_amd.motion_denoise import MotionDenoise
    md = MotionDenoise(_OraclePrior("lrelu", golden_weights("live")), body_model=_LinearBlendBody("cpu"), device="cpu")
    pose = _noisy_sequences(1, 6, seed=2).requires_grad_(True)
    with torch.no_grad():
        _, init_j = md._geometry(pose)
    loss = md.losses(pose, init_j + 0.01, it=1)
    assert set(loss) == {"pose_pr", "temp", "data"}
    (loss["temp"].sum() + loss["data"].sum()).backward()
    assert pose.grad[..., :63].abs().min().item() > 0 and torch.all(pose.grad[..., 63:] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3])
def test_very_short_sequences(T):
    """one, two and three frames: no temporal neighbour / one / both; fused step and autograd driver agree and stay finite
    (a one-frame sequence has no temporal term here; the reference's mean over an empty difference is NaN)"""
    import torch
    from posendf_amd import PoseNDF, amass_config, synth
    from posendf_amd.motion_denoise import MotionDenoise
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": "fp32"}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0, 2.0, 0.1).items()})
    net.eval()
    rng = np.random.default_rng(7)
    noisy = torch.from_numpy(rng.normal(scale=0.3, size=(4, T, 69)).astype(np.float32)).cuda()
    md = MotionDenoise(net)
    a, _ = md.denoise(noisy, iterations=2, steps_per_iter=3, fused=False)
    b, _ = md.denoise(noisy, iterations=2, steps_per_iter=3, fused=True)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert (a - b).abs().max().item() < 2e-4, (a - b).abs().max().item()


def test_partial_observation_schedule_matches_reference_formulas():
    """experiments/partial_observation.py:29-35: the copy of the loop with other weights -- pose prior LINEAR in c."""
    from posendf_amd.motion_denoise import iteration_coefs, loss_weights
    w = loss_weights("partial_observation")
    c = torch.tensor(0.03)
    for it in (0, 1, 4, 9):
        assert torch.isclose(w["temp"](c, it), 10.0 ** 2 * c * (1 + it))
        assert torch.isclose(w["data"](c, it), 10.0 ** 1 * c / (1 + it))
        assert torch.isclose(w["pose_pr"](c, it), 10.0 ** 2 * c / (1 + it))
        pc, pp, tc, dc = iteration_coefs("partial_observation", it)
        assert pp == 1 and abs(pc - 100.0 / (1 + it)) < 1e-9 and abs(tc - 100.0 * (1 + it)) < 1e-9
        assert dc == (10.0 / (1 + it) if it > 0 else 0.0)
    pc, pp, tc, dc = iteration_coefs("motion_denoise", 3)
    assert (pc, pp, tc, dc) == (1e7 / 4, 2, 40.0, 25.0)


def test_oracle_step_gradient_under_the_partial_observation_schedule():
    """numpy oracle of the step against torch autograd of the same objective (pose prior from the oracle network)."""
    from oracle import denoise_np
    from posendf_amd.motion_denoise import MotionDenoise
    sd = golden_weights("live")
    th0 = _noisy_sequences(1, 7, seed=5)[0].double()
    th = (th0 + 0.01 * torch.randn(7, 69, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).requires_grad_(True)
    md = MotionDenoise(_OraclePrior("lrelu", sd).double(), device="cpu", schedule="partial_observation")
    loss = md.losses(th[None], th0[None].reshape(1, 7, 23, 3)[:, :, :21], 2)
    md.total(loss, 2).sum().backward()
    g, _ = denoise_np.step_gradient(th.detach().numpy(), th0.numpy(), sd, 2, schedule="partial_observation")
    assert np.abs(g - th.grad.numpy()).max() < 1e-8 * np.abs(g).max()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_fused_partial_observation_schedule_matches_oracle(precision):
    """optimize(fused=True) under partial_observation.py's weights (pndf_denoise_update_w: linear pose prior) against the
    numpy oracle of the loop."""
    from oracle import denoise_np
    from posendf_amd import PoseNDF, amass_config
    from posendf_amd.motion_denoise import MotionDenoise
    sd = golden_weights("live")
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    noisy = _noisy_sequences(3, 14, seed=8)
    md = MotionDenoise(net, device="cuda:0", schedule="partial_observation")
    got, _ = md.denoise(noisy, iterations=2, steps_per_iter=4, fused=True)
    ref = denoise_np.optimize(noisy.numpy(), sd, iterations=2, steps_per_iter=4, schedule="partial_observation")
    diff = np.abs(got.cpu().numpy() - ref)
    assert np.median(diff) < 1e-5 and (diff > 1e-3).mean() < 0.01, (np.median(diff), diff.max())
    other, _ = MotionDenoise(net, device="cuda:0").denoise(noisy, iterations=2, steps_per_iter=4, fused=True)
    assert (other - got).abs().max().item() > 1e-3          # the two schedules are different objectives
    auto, _ = md.denoise(noisy, iterations=2, steps_per_iter=4, record=False)
    d2 = (auto - got).abs().flatten()
    assert d2.median().item() < 1e-5 and (d2 > 1e-3).float().mean().item() < 0.01


def test_quaternion_to_axis_angle_inverts_axis_angle_to_quaternion():
    from posendf_amd.motion_denoise import axis_angle_to_quaternion
    from posendf_amd.sample_poses import quaternion_to_axis_angle
    g = torch.Generator().manual_seed(0)
    aa = torch.randn(200, 3, dtype=torch.float64, generator=g)
    aa = aa / aa.norm(dim=-1, keepdim=True) * (torch.rand(200, 1, dtype=torch.float64, generator=g) * 3.0)      # angles < pi
    aa[0] = 0.0
    aa[1] = torch.tensor([1e-9, 0.0, 0.0])
    back = quaternion_to_axis_angle(axis_angle_to_quaternion(aa))
    assert torch.allclose(back, aa, atol=1e-12)
    assert torch.allclose(quaternion_to_axis_angle(torch.tensor([[0.0, 1.0, 0.0, 0.0]], dtype=torch.float64)),
                          torch.tensor([[np.pi, 0.0, 0.0]], dtype=torch.float64))


def test_load_motion_npz_pads_hand_joints(tmp_path):
    from posendf_amd.motion_denoise import load_motion_npz
    body = np.random.default_rng(0).normal(size=(9, 63)).astype(np.float32)
    np.savez(tmp_path / "m.npz", pose_body=body)
    th = load_motion_npz(tmp_path / "m.npz", device="cpu")
    assert th.shape == (9, 69) and torch.equal(th[:, :63], torch.from_numpy(body)) and (th[:, 63:] == 0).all()
    np.savez(tmp_path / "bad.npz", pose_body=body[:, :60])
    with pytest.raises(ValueError):
        load_motion_npz(tmp_path / "bad.npz", device="cpu")


def test_reference_argument_order_is_drop_in():
    """experiments/motion_denoise.py:21,58,151-152 verbatim: `MotionDenoise(net, body_model=body_model, batch_size=len(noisy_poses),
    out_path=out_path)` then `v2v_err = motion_denoiser.optimize(noisy_poses, gt_poses)` -- second positional argument of
    `optimize` is the ground truth, the result is the v2v error in cm as a numpy scalar.  CPU: the oracle
    network and a small differentiable body stand-in; the batched form lives behind `denoise`."""
    import inspect
    from posendf_amd.motion_denoise import MotionDenoise
    assert list(inspect.signature(MotionDenoise.__init__).parameters)[:8] == [
        "self", "posendf", "body_model", "out_path", "debug", "device", "batch_size", "gender"]
    assert list(inspect.signature(MotionDenoise.optimize).parameters)[:5] == [
        "self", "noisy_poses", "gt_poses", "iterations", "steps_per_iter"]
    net = _OraclePrior("lrelu", golden_weights("live"))
    body = _LinearBlendBody("cpu")
    gt_poses = _noisy_sequences(1, 8, seed=21)[0] * 0.3
    noisy_poses = gt_poses + 0.05 * torch.randn(8, 69, generator=torch.Generator().manual_seed(3))
    # the reference's own call shapes: positional out_path / debug / device, keyword body_model / batch_size
    motion_denoiser = MotionDenoise(net, body, "/tmp/unused_out_path", False, "cpu", len(noisy_poses), "male")
    v2v_err = motion_denoiser.optimize(noisy_poses, gt_poses, 2, 3)
    assert isinstance(v2v_err, np.ndarray) and v2v_err.shape == () and np.isfinite(v2v_err) and v2v_err > 0
    out = motion_denoiser.last_poses
    assert out.shape == (8, 69)
    want = torch.mean(torch.sqrt(torch.sum((body(out)[0] - body(gt_poses)[0]) ** 2, dim=2))) * 100.0       # :117-118
    assert abs(float(v2v_err) - float(want)) < 1e-6 * float(want)
    # the same poses as the batched entry point produces
    ref, _ = MotionDenoise(net, body_model=body, device="cpu").denoise(noisy_poses, iterations=2, steps_per_iter=3, record=False)
    assert torch.equal(ref, out)
    # without ground truth the error is measured against the noisy input's meshes (:110)
    v_in = MotionDenoise(net, body_model=body, batch_size=8, out_path="x", device="cpu").optimize(noisy_poses, None, 1, 2)
    assert np.isfinite(v_in) and v_in > 0
    with pytest.raises(ValueError):
        MotionDenoise(net, device="cpu").optimize(noisy_poses)
