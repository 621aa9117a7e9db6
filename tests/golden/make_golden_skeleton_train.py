#!/usr/bin/env python3
"""Generate tests/golden/skeleton_train_<skeleton>_<act>.npz: the training objective on other skeletons, computed with the REAL
reference's classes (include/posendf_amd_skeleton_train.h).

The reference's PoseNDF.forward reshapes to (-1, 21, 4) (model/posendf.py:64,80) and cannot train another skeleton.  Its pieces
can: with `get_parent_mapping` patched as model.network.net_modules sees it (as tests/golden/make_golden_skeleton.py does), the
reference's own StructureEncoder and DFNet build the network of any parent table, and its own `gradient` gives the eikonal term.
This script composes the three into the statements of model/posendf.py:71-96 with J joints in place of 21, runs the trainer's step
structure (model/train_posendf.py:93-98: loss weights 1/1/1, backward) for the 15-joint hand and the 32-joint branching tree, each
with lrelu and softplus (beta 100), hidden [64, 48], on B = 509 noisy poses with seeded labels and Bm = 383 manifold poses, in fp32
and fp64, and stores the inputs, the three losses and EVERY weight gradient in full (the network is small).

The weight seed is the first of 0, 1, 2, ... with at most a quarter of the noisy poses clipped in the fp64 run
(skeleton_train_fixtures.pick_seed); it is stored.

Needs the reference; nothing of the reference is copied into the repository, only inputs and outputs (data).  One thread, so that a
rerun gives bit-equal arrays.
Usage:  python tests/golden/make_golden_skeleton_train.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("POSENDF_REFERENCE", "/root/reference")

# --- stubs for arithmetic-free imports (reference model/posendf.py:5,9), as in make_golden.py
ipdb = types.ModuleType("ipdb")
ipdb.set_trace = lambda *a, **k: None
sys.modules["ipdb"] = ipdb
tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
sys.modules["torch.utils.tensorboard"] = tb
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

import model.network.net_modules as ref_modules      # noqa: E402  (reference)
from model.posendf import gradient as ref_gradient   # noqa: E402  (reference)

import skeleton_oracle as sko                         # noqa: E402  (this repo: tables, inputs and names only)
import skeleton_train_fixtures as stf                 # noqa: E402

TABLES = {"hand": sko.HAND, "tree32": sko.TREE32}


def ref_network(parents, act, sd, dtype):
    """the reference's own StructureEncoder and DFNet along `parents`"""
    ref_modules.get_parent_mapping = lambda model_type: list(parents)      # as model.network.net_modules sees it
    enc = ref_modules.StructureEncoder({"act": act, "beta": 100.0})
    dfnet = ref_modules.DFNet({"in_dim": 6 * len(parents), "dims": list(stf.HIDDEN), "act": act, "beta": 100.0, "num_layers": None})
    net = torch.nn.ModuleDict({"enc": enc, "dfnet": dfnet})
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dtype).train()


def ref_step(net, J, q, gt, qm):
    """model/posendf.py:71-96 on the reference's modules with J joints, then train_posendf.py:95-98"""
    net.zero_grad()
    pose = q.reshape(-1, J, 4)
    pose.requires_grad = True
    dist_pred = net["dfnet"](net["enc"](torch.nn.functional.normalize(pose, dim=1)))
    dist_man = net["dfnet"](net["enc"](qm.reshape(-1, J, 4)))
    ld = {"dist": torch.nn.L1Loss()(dist_pred[:, 0], gt.reshape(-1)), "man_loss": dist_man.abs().mean(),
          "eikonal": ((ref_gradient(pose, dist_pred).norm(2, dim=-1) - 1) ** 2).mean()}
    total = 0.0
    for k in ld:
        total = total + 1.0 * ld[k]
    total.backward()
    return np.array([float(ld[k].detach()) for k in stf.LOSS_KEYS]), {k: p.grad.detach().numpy() for k, p in net.named_parameters()}


def one(skel, act):
    parents = TABLES[skel]
    q, gt, qm = stf.inputs(parents)
    seed, sd = stf.pick_seed(parents, act, q)
    out = {"q": q, "dist_gt": gt, "q_man": qm, "seed": np.array(seed), "parents": np.array(parents, np.int32),
           "hidden": np.array(stf.HIDDEN, np.int32), "torch_version": np.array(torch.__version__)}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
        losses, grads = ref_step(ref_network(parents, act, sd, dtype), len(parents), t(q), t(gt), t(qm))
        assert np.isfinite(losses).all() and all(np.isfinite(g).all() for g in grads.values()), (skel, act, tag)
        out[f"losses_{tag}"] = losses
        for k, g in grads.items():
            out[f"g_{tag}::{k}"] = g
    assert set(grads) == set(sd)
    path = stf.fixture_path(skel, act)
    np.savez_compressed(path, **out)
    print(f"{path}: seed {seed}, losses f64 {out['losses_f64']}, {os.path.getsize(path) // 1024} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(1)
    for skel, act in stf.FIXTURE_CASES:
        one(skel, act)
