"""The training objective on the HIP engine (opt['engine']['train'] = 'hip', csrc/pndf_train.hip) on an MI355X: losses and every
weight gradient against the reference's fp64 vectors (tests/golden/train_*.npz) and against the stock path in fp64 on the same
GPU, the reference trainer's Adam loop, determinism and the edges.  Reads only fixtures and synth (the reference is not here).

Tolerance rule (per loss, per gradient tensor or digest): relative error in the tensor norm <= max(1e-4, 4 x the error of the
reference arithmetic's own fp32 run against its fp64 run)."""
import numpy as np
import pytest
import torch

import train_fixtures as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _gate(what, mine, ref32, ref64, failures, floor=0.0):
    """`floor`: least norm of the denominator -- a gradient whose terms cancel to (exactly) zero in fp64 keeps an fp32 rounding
    residue in any fp32 evaluation (B = 1: -1 + 3 x 1/3), so it is held to an absolute bound instead"""
    tol = max(1e-4, 4.0 * _rel(ref32, ref64))
    a, b = np.asarray(mine, np.float64), np.asarray(ref64, np.float64)
    err = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor, 1e-30))
    if not err <= tol:
        failures.append((what, err, tol))
    return err


def _model(act, sd, hidden, loss="l1", backend="hip", dtype=torch.float32, enc_act=None, beta=None, enc_beta=None):
    from posendf_amd import PoseNDF
    net = PoseNDF(tf.config(act, hidden, loss, DEV, train_backend=backend, enc_act=enc_act, beta=beta, enc_beta=enc_beta)).to(dtype)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()})
    return net


def _run(net, q, gt, qm, eikonal, dtype=torch.float32):
    t = lambda a: torch.as_tensor(np.asarray(a)).to(device=DEV, dtype=dtype)      # noqa: E731
    return tf.run_objective(net, t(q), t(gt), t(qm), eikonal)


def _compare_full(tag, act, sd, hidden, q, gt, qm, eikonal, loss="l1", enc_act=None, beta=None, enc_beta=None):
    """HIP fp32 against the stock path in fp64 on the GPU, with the stock fp32 run as the envelope"""
    kw = dict(enc_act=enc_act, beta=beta, enc_beta=enc_beta)
    l_h, g_h, _ = _run(_model(act, sd, hidden, loss, **kw), q, gt, qm, eikonal)
    l_32, g_32, _ = _run(_model(act, sd, hidden, loss, "torch", **kw), q, gt, qm, eikonal)
    l_64, g_64, _ = _run(_model(act, sd, hidden, loss, "torch", torch.float64, **kw), q, gt, qm, eikonal, torch.float64)
    assert set(l_h) == set(l_64)
    failures, worst = [], 0.0
    for k in l_64:
        worst = max(worst, _gate(f"{tag} loss {k}", l_h[k], l_32[k], l_64[k], failures))
    floor = 1e-3 * max(np.linalg.norm(g) for g in g_64.values())     # absolute bound: 1e-7 of the step's largest gradient
    for k in g_64:
        worst = max(worst, _gate(f"{tag} grad {k}", g_h[k], g_32[k], g_64[k], failures, floor))
    print(f"[train {tag}] worst relative error {worst:.2e}")
    assert not failures, failures[:8]
    return l_h, g_h


@pytest.mark.parametrize("name", list(tf.CASES))
def test_fixture(name):
    z = dict(np.load(tf.fixture_path(name)))
    act, weights, loss, eikonal = tf.CASES[name]
    sd, hidden = tf.case_weights(weights)
    losses, grads, _ = _run(_model(act, sd, hidden, loss), z["q"], z["dist_gt"], z["q_man"], eikonal)
    failures, worst = [], 0.0
    for i, k in enumerate(tf.LOSS_KEYS):
        if np.isnan(z["losses_f64"][i]):
            assert k not in losses
            continue
        worst = max(worst, _gate(f"loss {k}", losses[k], z["losses_f32"][i], z["losses_f64"][i], failures))
    for k, g in grads.items():
        for part, v in tf.digest(k, g, hidden).items():
            sfx = f"::{part}" if part else ""
            worst = max(worst, _gate(k + sfx, v, z[f"g_f32::{k}{sfx}"], z[f"g_f64::{k}{sfx}"], failures))
    print(f"[train fixture {name}] worst relative error {worst:.2e}")
    assert not failures, failures[:8]


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_reference_batch(act):
    """B = Bm = 20,000 (configs/amass.yaml: 4 files x 5,000 poses) on amass.yaml dims, eikonal on: every full gradient"""
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    q, qm = synth.make_poses(20000, seed=5), synth.make_poses(20000, seed=6)
    gt = np.random.default_rng(7).uniform(0.0, 0.5, 20000).astype(np.float32)
    _compare_full(f"B=20000 {act}", act, sd, hidden, q, gt, qm, 1.0)


def test_dropin_adam_loop():
    """The reference trainer's step structure (train_posendf.py:93-99): zero_grad, model(...), weighted sum (1/1/1), backward,
    Adam(lr 1e-5, weight_decay 1e-4) -- 5 steps at B = Bm = 2,048.  The HIP loop's parameters may differ from the fp64 stock loop's
    by at most 2x what the fp32 stock loop's do, plus 1e-9."""
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    batches = [(synth.make_poses(2048, seed=100 + s), np.random.default_rng(200 + s).uniform(0, 0.5, 2048).astype(np.float32),
                synth.make_poses(2048, seed=300 + s)) for s in range(5)]
    finals = {}
    for tag, backend, dtype in (("hip", "hip", torch.float32), ("f32", "torch", torch.float32), ("f64", "torch", torch.float64)):
        net = _model("lrelu", sd, hidden, "l1", backend, dtype)
        opt = torch.optim.Adam(net.parameters(), lr=1e-5, weight_decay=1e-4)
        for q, gt, qm in batches:
            tf.run_objective(net, *(torch.as_tensor(a).to(device=DEV, dtype=dtype) for a in (q, gt, qm)), 1.0)
            opt.step()
        finals[tag] = {k: p.detach().double().cpu().numpy() for k, p in net.named_parameters()}
    bad = []
    for k in finals["f64"]:
        d_h = np.linalg.norm(finals["hip"][k] - finals["f64"][k])
        d_32 = np.linalg.norm(finals["f32"][k] - finals["f64"][k])
        if not d_h <= 2.0 * d_32 + 1e-9:
            bad.append((k, d_h, d_32))
    assert not bad, bad[:8]


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_two_calls_are_bit_identical(act):
    sd, hidden = tf.case_weights("live")
    q, gt, qm = tf.case_inputs()
    net = _model(act, sd, hidden)
    l1, g1, _ = _run(net, q, gt, qm, 1.0)
    l2, g2, _ = _run(net, q, gt, qm, 1.0)
    assert l1 == l2
    assert all(np.array_equal(g1[k], g2[k]) for k in g1)


@pytest.mark.parametrize("B,Bm", [(1, 3), (63, 40), (65, 130), (1000, 777)])
def test_batch_edges(B, Bm):
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    q, qm = synth.make_poses(B, seed=11), synth.make_poses(Bm, seed=12)
    gt = np.random.default_rng(13).uniform(0, 0.5, B).astype(np.float32)
    for act in ("lrelu", "softplus"):
        _compare_full(f"B={B} Bm={Bm} {act}", act, sd, hidden, q, gt, qm, 1.0)


def test_zero_quaternion_column():
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    q, qm = synth.make_poses(64, seed=21), synth.make_poses(48, seed=22)
    q[3, :, 2] = 0.0                     # one component zero on all 21 joints: the normalisation clamps at eps
    gt = np.random.default_rng(23).uniform(0, 0.5, 64).astype(np.float32)
    for act in ("relu", "softplus"):
        _compare_full(f"zero column {act}", act, sd, hidden, q, gt, qm, 1.0)


def test_poses_at_distance_zero():
    """relu family: a pose with d = 0 gives no gradient and 1 per joint to the eikonal loss (all poses here)"""
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    sd = dict(sd)
    sd[f"dfnet.lin{len(hidden)}.bias"] = np.full_like(sd[f"dfnet.lin{len(hidden)}.bias"], -1e3)
    q, qm = synth.make_poses(100, seed=31), synth.make_poses(70, seed=32)
    gt = np.random.default_rng(33).uniform(0, 0.5, 100).astype(np.float32)
    losses, grads = _compare_full("d = 0", "lrelu", sd, hidden, q, gt, qm, 1.0)
    assert losses["eikonal"] == 1.0 and losses["man_loss"] == 0.0
    assert all(not g.any() for g in grads.values())


def test_eikonal_off_returns_dist_only():
    sd, hidden = tf.case_weights("live")
    q, gt, qm = tf.case_inputs()
    net = _model("softplus", sd, hidden)
    loss, ld = net(torch.from_numpy(q).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(qm).to(DEV), train=True, eikonal=0.0)
    assert set(ld) == {"dist"} and ld["dist"] is loss
    _compare_full("eikonal off", "softplus", sd, hidden, q, gt, qm, 0.0)


@pytest.mark.parametrize("act,hidden,enc_act", [("lrelu", [64], None), ("softplus", [96, 128, 64, 200, 64, 32, 16], None),
                                                ("relu", [1024, 1024], None), ("softplus", [256, 128], "lrelu"),
                                                ("lrelu", [128, 96], "softplus")])
def test_other_networks(act, hidden, enc_act):
    from posendf_amd import synth
    sd = synth.make_weights(3, 2.0, 0.1, dims=(126, *hidden, 1))
    q, qm = synth.make_poses(300, seed=41), synth.make_poses(200, seed=42)
    gt = np.random.default_rng(43).uniform(0, 0.5, 300).astype(np.float32)
    _compare_full(f"{act} {hidden} enc {enc_act}", act, sd, hidden, q, gt, qm, 1.0, enc_act=enc_act)


@pytest.mark.parametrize("act,enc_act,beta,enc_beta", [
    ("softplus", None, 1.0, None), ("softplus", None, 1000.0, None),          # the trunk's beta, the encoder's equal to it
    ("softplus", "softplus", 100.0, 7.0), ("softplus", "softplus", 10.0, 1000.0),      # the encoder's own beta
    ("relu", "softplus", None, 1000.0), ("relu", "softplus", None, 7.0),       # a Softplus encoder of its own beta behind a ReLU trunk
    ("lrelu", "relu", None, None), ("relu", "lrelu", None, None)])             # the two slopes, both ways round
def test_activation_pairs_and_betas(act, enc_act, beta, enc_beta):
    """model.StrEnc.act / beta against model.DFNet.act / beta: each side's activation, slope and beta must reach that side's
    forward, reverse and double-backward (eikonal) arithmetic.  amass.yaml's dims, ragged B / Bm, the eikonal term on."""
    from posendf_amd import synth
    sd, hidden = tf.case_weights("live")
    q, qm = synth.make_poses(300, seed=51), synth.make_poses(200, seed=52)
    gt = np.random.default_rng(53).uniform(0, 0.5, 300).astype(np.float32)
    _compare_full(f"{act}@{beta} enc {enc_act}@{enc_beta}", act, sd, hidden, q, gt, qm, 1.0, enc_act=enc_act, beta=beta, enc_beta=enc_beta)


def test_opt_in_path_uses_the_hip_objective():
    sd, hidden = tf.case_weights("live")
    q, gt, qm = (torch.from_numpy(a).to(DEV) for a in tf.case_inputs())
    loss, ld = _model("lrelu", sd, hidden)(q, gt, qm, train=True, eikonal=1.0)
    assert type(loss.grad_fn).__name__ == "TrainObjectiveBackward"
    assert ld["dist"] is loss and set(ld) == {"dist", "man_loss", "eikonal"}
    loss_t, _ = _model("lrelu", sd, hidden, backend="torch")(q.clone(), gt, qm, train=True, eikonal=1.0)
    assert type(loss_t.grad_fn).__name__ != "TrainObjectiveBackward"
