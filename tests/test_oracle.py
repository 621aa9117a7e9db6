"""Pin the numpy oracle (oracle/posendf_np.py) against vectors produced by the real reference
(tests/golden/make_golden.py).  CPU only.  Tolerances: single-step quantities 2e-5 relative in fp32
(both sides are fp32 with different summation orders), 1e-9 in fp64."""
import numpy as np
import pytest

from conftest import LITE_REGIMES, d_err, d_rows, fp32_noise, pose_gate, rel_err, rel_err_rows
from oracle import posendf_np as onp


def kink_exempt(g, sd, act):
    """relu family: poses with a pre-activation within 1e-5 (relative) of a kink may flip a derivative"""
    return None if act == "softplus" else onp.kink_margin(g["q"], sd, act) < 1e-5


def test_single_step_fp32(golden_case):
    act, regime, g, sd = golden_case
    dbg = {}
    d, dq = onp.forward_grad(g["q"], sd, act, debug=dbg)
    assert rel_err(dbg["n"], g["n_f32"]) < 1e-5
    assert rel_err(dbg["feat"], g["feat_f32"]) < 1e-5
    if regime in LITE_REGIMES:
        # ill-conditioned weight sets: two fp32 evaluations (numpy here, torch in the fixture) legitimately differ by more
        # than 2e-5 on the poses whose d is a small difference of large terms -- each is held, pose by pose, to the fp32
        # sensitivity of the arithmetic (conftest.fp32_noise), both against the reference's fp64 run
        sig_d, sig_g, _, _ = fp32_noise(g["q"], sd, act)
        pose_gate(d_rows(d, g["d_f64"]), sig_d, "oracle d")
        pose_gate(d_rows(g["d_f32"], g["d_f64"]), sig_d, "reference d")
        ex = kink_exempt(g, sd, act)
        pose_gate(rel_err_rows(dq, g["dq_f64"]), sig_g, "oracle dq", exempt=ex)
        pose_gate(rel_err_rows(g["dq_f32"], g["dq_f64"]), sig_g, "reference dq", exempt=ex)
    else:
        assert d_err(d, g["d_f32"]) < 2e-5
        assert rel_err(dq, g["dq_f32"]) < 5e-5
        assert d_err(onp.forward(g["q"], sd, act), g["d_f32"]) < 2e-5
    # clipped poses are clipped on both sides, and their gradient is exactly zero
    if act != "softplus":
        z = g["d_f32"][:, 0] == 0
        assert np.array_equal(d[:, 0] == 0, z)
        assert np.all(dq[z] == 0)


def test_single_step_fp64(golden_case):
    act, regime, g, sd = golden_case
    d, dq = onp.forward_grad(g["q"], sd, act, dtype=np.float64)
    assert d_err(d, g["d_f64"]) < 1e-9
    assert rel_err(dq, g["dq_f64"]) < 1e-9


def test_autograd_contract(golden_case):
    act, regime, g, sd = golden_case
    _, gp = onp.forward_grad(g["q"], sd, act, grad_out=g["grad_out"])
    if regime in LITE_REGIMES:
        truth = g["dq_f64"] * g["grad_out"].reshape(-1, 1, 1)
        _, sig_g, _, _ = fp32_noise(g["q"], sd, act)
        ex = kink_exempt(g, sd, act)
        pose_gate(rel_err_rows(gp, truth), sig_g, "oracle grad_pose", exempt=ex)
        pose_gate(rel_err_rows(g["grad_pose_f32"], truth), sig_g, "reference grad_pose", exempt=ex)
    else:
        assert rel_err(gp, g["grad_pose_f32"]) < 5e-5


def test_pose_prior_objective(golden_case):
    act, regime, g, sd = golden_case
    if regime in LITE_REGIMES:
        pytest.skip("lite fixture: no pose-prior vectors")
    for it in (0, 3):
        obj, grad = onp.pose_prior_objective(g["q"], sd, it, act)
        assert abs(obj - g[f"prior_obj_it{it}"]) <= 2e-5 * abs(g[f"prior_obj_it{it}"])
        assert rel_err(grad, g[f"prior_grad_it{it}"]) < 1e-4


def test_projection_fp64(golden_case):
    """fp64 trajectories agree to ~1e-9 unless a ReLU/LeakyReLU kink is crossed within rounding."""
    act, regime, g, sd = golden_case
    last = 10 if regime in LITE_REGIMES else 100
    q, d, tr = onp.project(g["q"], sd, steps=last, act=act, dtype=np.float64, trace=True)
    e = np.abs(q - g[f"q{last}_f64"]).reshape(len(q), -1).max(1) / np.abs(g[f"q{last}_f64"]).max()
    assert np.median(e) < 1e-9
    assert (e > 1e-6).mean() <= 0.03
    assert rel_err(tr[0], g["dtrace_f64"][0]) < 1e-9


def test_projection_fp32_envelope(golden_case):
    """Free-running fp32 vs the reference's fp64 truth: the reference's own fp32 run sets the envelope
    (SURVEY.md section 7 'hard parts'); the oracle must be no worse than 2x + slack."""
    act, regime, g, sd = golden_case
    for steps in ((1, 10) if regime in LITE_REGIMES else (1, 10, 100)):
        q, _ = onp.project(g["q"], sd, steps=steps, act=act)
        truth = g[f"q{steps}_f64"]
        scale = np.abs(truth).max()
        mine = np.abs(q - truth).reshape(len(q), -1).max(1) / scale
        ref = np.abs(g[f"q{steps}_f32"] - truth).reshape(len(q), -1).max(1) / scale
        assert np.median(mine) < 1e-5
        assert (mine > 1e-4).mean() <= 2 * (ref > 1e-4).mean() + 0.03, (steps, mine.max(), ref.max())


def test_per_pose_independence():
    from conftest import golden_weights
    from posendf_amd import synth
    sd = golden_weights("mixed")
    q = synth.make_poses(64, seed=3, signed=True)
    d, dq = onp.forward_grad(q, sd)
    perm = np.random.default_rng(0).permutation(64)
    d2, dq2 = onp.forward_grad(q[perm], sd)
    assert np.allclose(d[perm], d2, rtol=1e-6, atol=1e-7)
    assert np.allclose(dq[perm], dq2, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_gradient_finite_difference(act):
    from conftest import golden_weights
    from posendf_amd import synth
    sd = golden_weights("live")
    q = synth.make_poses(4, seed=4, signed=True).astype(np.float64)
    d, dq = onp.forward_grad(q, sd, act, dtype=np.float64)
    rng = np.random.default_rng(1)
    for _ in range(6):
        v = rng.normal(size=q.shape)
        h = 1e-6
        fd = (onp.forward(q + h * v, sd, act, dtype=np.float64) - onp.forward(q - h * v, sd, act, dtype=np.float64)) / (2 * h)
        an = (dq * v).reshape(4, -1).sum(1)
        assert np.allclose(fd[:, 0], an, rtol=2e-4, atol=1e-9)


def test_activation_string_grammar():
    """"trunk[@beta]/encoder[@beta]" (onp.parse_act): model.DFNet.act / beta and model.StrEnc.act / beta travel in the one `act`
    string that every oracle function and every gate helper takes; a side without "@" takes the `beta` argument, one side is both"""
    p = onp.parse_act
    assert p("lrelu") == ("lrelu", 100.0, "lrelu", 100.0) and p("softplus", 7.0) == ("softplus", 7.0, "softplus", 7.0)
    assert p("softplus/lrelu") == ("softplus", 100.0, "lrelu", 100.0) and p("relu/softplus", 3.0) == ("relu", 3.0, "softplus", 3.0)
    assert p("softplus@10") == ("softplus", 10.0, "softplus", 10.0)
    assert p("softplus@100/softplus@7") == ("softplus", 100.0, "softplus", 7.0)
    assert p("relu/softplus@1000", 5.0) == ("relu", 5.0, "softplus", 1000.0)
    assert p("softplus@2.5/lrelu", 9.0) == ("softplus", 2.5, "lrelu", 9.0)
    assert [onp.act_family(a) for a in ("softplus@10", "relu/softplus@1000", "softplus@100/softplus@7")] == \
        ["softplus", "relu/softplus", "softplus/softplus"]
    for bad in ("", "tanh", "relu/", "/relu", "relu/lrelu/relu", "softplus@", "softplus@x", "softplus@0", "softplus@-1",
                "softplus@inf", "softplus@nan", "softplus@1@2", "Softplus", "relu /lrelu"):
        with pytest.raises(ValueError):
            p(bad)
    # the betas reach the arithmetic: "name@b" is beta=b, a bare name is bit-identical to what it always was
    from conftest import golden_weights
    from posendf_amd import synth
    sd = golden_weights("live")
    q = synth.make_poses(16, seed=3)
    for act, beta, same in (("softplus", 100.0, "softplus@100"), ("softplus", 7.0, "softplus@7/softplus@7"),
                            ("softplus/lrelu", 3.0, "softplus@3/lrelu"), ("lrelu", 100.0, "lrelu/lrelu@5")):
        for dtype in (np.float32, np.float64):
            a, b = onp.forward_grad(q, sd, act, beta, dtype), onp.forward_grad(q, sd, same, dtype=dtype)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (act, beta, same)
    # ... and each side's beta reaches its own side only
    d_t, _ = onp.forward_grad(q, sd, "softplus@7/softplus", dtype=np.float64)
    d_e, _ = onp.forward_grad(q, sd, "softplus/softplus@7", dtype=np.float64)
    f = onp.encoder_forward(onp.normalize_joint_axis(q.astype(np.float64))[0], sd, "softplus", 7.0)
    assert np.array_equal(d_e, onp.dfnet_forward(f, sd, "softplus", 100.0))
    f = onp.encoder_forward(onp.normalize_joint_axis(q.astype(np.float64))[0], sd, "softplus", 100.0)
    assert np.array_equal(d_t, onp.dfnet_forward(f, sd, "softplus", 7.0))
