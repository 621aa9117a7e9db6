#!/usr/bin/env python3
"""Fixtures of the training objective (model/posendf.py:62-99, train=True), produced with the REAL reference (dev container only).

For every case of tests/train_fixtures.py -- {lrelu, relu, softplus} x configs/amass.yaml dims x the `live` synthetic weights, the
narrow lrelu network the reference trained (trained_lrelu.npz), one `eikonal: 0` case, one `l2` case, and three whose model.StrEnc.act /
beta or model.DFNet.beta are not configs/amass.yaml's (train_fixtures.sides) -- the imported reference
`PoseNDF` runs the trainer's step structure (model/train_posendf.py:93-98: forward, loss weights 1/1/1, backward) on B = 509 noisy
poses with seeded labels and Bm = 383 manifold poses, in fp32 and in fp64.  Stored: the inputs, the activations and betas the
reference's config held, the losses (NaN where the reference returns no such key) and every weight gradient -- the encoder, all
biases and the last layer in full; the large weights lin0 .. lin5 as Frobenius norm, row sums, column sums and 1,024 seeded entries
(train_fixtures.digest).

Nothing of the reference is copied: only inputs and outputs (data).  One thread, so that a rerun gives bit-equal arrays.
Usage:  python tests/golden/make_golden_train.py [case ...]      (writes tests/golden/train_<case>.npz)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("POSENDF_REFERENCE", "/root/reference")

sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
import train_fixtures as tf       # noqa: E402


def _import_reference():
    ipdb = types.ModuleType("ipdb")
    ipdb.set_trace = lambda *a, **k: None
    sys.modules.setdefault("ipdb", ipdb)
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from configs.config import load_config          # (reference)
    from model.posendf import PoseNDF               # (reference)
    return load_config, PoseNDF


def ref_config(act, hidden, loss):
    load_config, _ = _import_reference()
    opt = load_config(os.path.join(REF, "configs", "amass.yaml"))
    opt["train"]["device"] = "cpu"
    opt["train"]["loss_type"] = loss
    trunk, beta, enc_act, enc_beta = tf.sides(act)
    opt["model"]["DFNet"]["act"] = trunk
    opt["model"]["DFNet"]["beta"] = beta
    opt["model"]["StrEnc"]["act"] = enc_act
    opt["model"]["StrEnc"]["beta"] = enc_beta
    opt["model"]["DFNet"]["dims"] = list(hidden)
    return opt


def ref_step(act, hidden, loss, eikonal, sd, dtype, q, gt, qm):
    _, PoseNDF = _import_reference()
    opt = ref_config(act, hidden, loss)
    net = PoseNDF(opt).to(dtype)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()})
    net.train()
    net.zero_grad()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
    _, ld = net(t(q), t(gt), t(qm), eikonal=eikonal)
    total = 0.0
    for k in ld:                                                 # train_posendf.py:95-97, loss weights 1/1/1
        total = total + 1.0 * ld[k]
    total.backward()
    losses = np.array([float(ld[k].detach()) if k in ld else np.nan for k in tf.LOSS_KEYS])
    grads = {k: p.grad.detach().numpy() for k, p in net.named_parameters()}
    return losses, grads


def make(name):
    act, weights, loss, eikonal = tf.CASES[name]
    sd, hidden = tf.case_weights(weights)
    q, gt, qm = tf.case_inputs()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {"q": q, "dist_gt": gt, "q_man": qm, "act": np.array(act), "weights": np.array(weights), "loss_type": np.array(loss),
               "eikonal": np.array(eikonal), "hidden": np.array(hidden, np.int32)}
        m = ref_config(act, hidden, loss)["model"]
        out.update({"dfnet_act": np.array(m["DFNet"]["act"]), "dfnet_beta": np.array(float(m["DFNet"]["beta"])),
                    "strenc_act": np.array(m["StrEnc"]["act"]), "strenc_beta": np.array(float(m["StrEnc"]["beta"]))})
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            losses, grads = ref_step(act, hidden, loss, eikonal, sd, dtype, q, gt, qm)
            out[f"losses_{tag}"] = losses
            for k, g in grads.items():
                for part, v in tf.digest(k, g, hidden).items():
                    out[f"g_{tag}::{k}" + (f"::{part}" if part else "")] = np.asarray(v)
        out["torch_version"] = np.array(torch.__version__)
    finally:
        torch.set_num_threads(threads)
    return out


if __name__ == "__main__":
    for name in (sys.argv[1:] or tf.CASES):
        res = make(name)
        path = tf.fixture_path(name)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path) // 1024, "KiB", "losses f64", res["losses_f64"])
