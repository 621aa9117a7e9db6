"""Shared by tests/golden/make_golden_train.py, tests/test_train_objective.py and tests/test_train_gpu.py: the cases of the
training-objective fixtures (tests/golden/train_*.npz), their inputs, the digests that stand in for the large weight gradients,
and the fp64 oracle -- torch autograd in float64 of this repository's own module tree, i.e. the facade's stock train=True code."""
from __future__ import annotations

import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

B, BM = 509, 383                          # ragged noisy / manifold batches
N_ENTRIES = 1024                          # seeded entries kept of each large weight gradient
# name: (activation, weights, train.loss_type, eikonal weight).  The activation string is oracle.posendf_np.parse_act's:
# "DFNet.act[@DFNet.beta]/StrEnc.act[@StrEnc.beta]", one side for both, beta 100 where no "@" says otherwise
CASES = {
    "lrelu_live": ("lrelu", "live", "l1", 1.0),
    "relu_live": ("relu", "live", "l1", 1.0),
    "softplus_live": ("softplus", "live", "l1", 1.0),
    "trained_lrelu": ("lrelu", "trained_lrelu", "l1", 1.0),
    "lrelu_noeik": ("lrelu", "live", "l1", 0.0),
    "softplus_l2": ("softplus", "live", "l2", 1.0),
    "softplus_encb7": ("softplus@100/softplus@7", "live", "l1", 1.0),      # the encoder's beta alone differs
    "relu_lreluenc": ("relu/lrelu", "live", "l1", 1.0),                    # the encoder's LeakyReLU slope behind a slope-0 trunk
    "softplus_b10": ("softplus@10", "live", "l1", 1.0),                    # beta != 100 on both sides
}
LOSS_KEYS = ("dist", "man_loss", "eikonal")


def fixture_path(name):
    return os.path.join(GOLDEN, f"train_{name}.npz")


def case_weights(weights):
    """(state dict of fp32 numpy arrays, hidden widths)"""
    from posendf_amd import synth
    if weights == "live":
        return synth.make_weights(0, 2.0, 0.1), list(synth.DFNET_DIMS[1:-1])
    z = np.load(os.path.join(GOLDEN, "trained_lrelu.npz"))
    return {k[3:]: z[k].astype(np.float32) for k in z.files if k.startswith("w::")}, [int(w) for w in z["hidden"]]


def case_inputs():
    """noisy poses [B,21,4], labels [B], manifold poses [Bm,21,4] (float32)"""
    from posendf_amd import synth
    q = synth.make_poses(B, seed=71)
    qm = synth.make_poses(BM, seed=72)
    gt = np.random.default_rng(73).uniform(0.0, 0.5, B).astype(np.float32)
    return q, gt, qm


def is_large(key, hidden):
    """lin0 .. lin(L-2) weights are stored as digests; everything else in full"""
    return key.startswith("dfnet.lin") and key.endswith(".weight") and int(key[9:].split(".")[0]) < len(hidden)


def entry_index(key, shape):
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    return np.sort(rng.choice(int(np.prod(shape)), size=min(N_ENTRIES, int(np.prod(shape))), replace=False))


def digest(key, g, hidden):
    """{name: array} standing in for the gradient g of parameter `key` (float64 computations of whatever precision g has)"""
    g = np.asarray(g)
    if not is_large(key, hidden):
        return {"": g}
    g64 = g.astype(np.float64)
    return {"fro": np.array(np.sqrt((g64 ** 2).sum())), "rows": g64.sum(1), "cols": g64.sum(0),
            "vals": g.reshape(-1)[entry_index(key, g.shape)]}


def sides(act, enc_act=None, beta=None, enc_beta=None):
    """(DFNet.act, DFNet.beta, StrEnc.act, StrEnc.beta) of an activation string; `beta` stands for the beta of a side without "@",
    `enc_act` / `enc_beta` replace the encoder's"""
    from oracle.posendf_np import parse_act
    trunk, tbeta, eact, ebeta = parse_act(act, 100.0 if beta is None else float(beta))
    return trunk, tbeta, (eact if enc_act is None else enc_act), (ebeta if enc_beta is None else float(enc_beta))


def config(act, hidden, loss, device, train_backend="torch", enc_act=None, beta=None, enc_beta=None):
    from posendf_amd import amass_config
    trunk, tbeta, eact, ebeta = sides(act, enc_act, beta, enc_beta)
    cfg = amass_config(trunk, device)
    cfg["model"]["DFNet"]["dims"] = list(hidden)
    cfg["model"]["DFNet"]["beta"] = tbeta
    cfg["model"]["StrEnc"]["act"] = eact
    cfg["model"]["StrEnc"]["beta"] = ebeta
    cfg["train"]["loss_type"] = loss
    cfg["engine"] = {"train": train_backend}
    return cfg


def run_objective(net, q, gt, qm, eikonal):
    """one training step's objective and gradients the way the reference's trainer forms them (loss weights 1/1/1):
    (losses {key: float}, grads {state-dict key: numpy array}, loss_dict)"""
    net.zero_grad(set_to_none=True)
    _, ld = net(q, gt, qm, train=True, eikonal=eikonal)
    total = 0.0
    for k in ld:
        total = total + 1.0 * ld[k]
    total.backward()
    losses = {k: float(v.detach()) for k, v in ld.items()}
    grads = {k: p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape)) for k, p in net.named_parameters()}
    return losses, grads, ld


def oracle64(act, weights, loss, eikonal, q, gt, qm, device="cpu", hidden=None, sd=None, enc_act=None):
    """the fp64 oracle: the facade's stock train=True path in float64"""
    import torch
    from posendf_amd import PoseNDF
    if sd is None:
        sd, hidden = case_weights(weights)
    net = PoseNDF(config(act, hidden, loss, device, enc_act=enc_act)).double()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items()})
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(device)      # noqa: E731
    losses, grads, _ = run_objective(net, t(q), t(gt), t(qm), eikonal)
    return losses, grads
