#!/usr/bin/env python3
"""Generate tests/golden/skeleton_<skeleton>_<act>.npz by RUNNING THE REAL REFERENCE on other skeletons
(include/posendf_amd_skeleton.h).

The reference prints "Model hierarchy not defined" for anything other than 'smpl', but its StructureEncoder and DFNet are generic: with
`get_parent_mapping` patched as model.network.net_modules sees it, the reference's own classes build the chain of bone MLPs of any
parent table.  Per case -- the 15-joint hand and a 32-joint branching tree, each with lrelu and softplus (beta 100), hidden [64, 48] --
the weights of posendf_amd.synth.make_weights(parents=...) are loaded into them and, for 48 poses of synth.make_poses, recorded in
fp32 and fp64: d and dq by torch.autograd (the arithmetic of model/posendf.py:71-76 and gradient(), :18-27), the poses after 3 plain
steps of experiments/sample_poses.py:67-74, and the state-dict key names and shapes.

The weight seed is the first of 0, 1, 2, ... with at most a quarter of the 48 poses clipped in the fp64 run -- d == 0 behind the output
ReLU, d <= softplus(0) behind Softplus, which never returns 0 -- (a network clipped to zero tests nothing); the script asserts it.

Needs the reference, like make_golden.py; nothing of the reference is copied into the repository, only inputs and outputs (data).
Usage:  python tests/golden/make_golden_skeleton.py
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

import skeleton_oracle as sko                         # noqa: E402  (this repo: tables, inputs and names only)

# the 32-joint branching tree, written out: joint 0 has the three children 1, 2, 3; 0-1-4-5-6-7-8-9 is a chain of depth 7
TREE32 = (-1, 0, 0, 0, 1, 4, 5, 6, 7, 8, 2, 10, 10, 3, 13, 14, 14, 9, 9, 11, 12, 15, 16, -1, 23, 24, 24, 25, 26, 27, 28, 29)
assert TREE32 == sko.TREE32 and TREE32.count(0) == 3
TABLES = {"hand": sko.HAND, "tree32": TREE32}


def ref_network(parents, act, sd, dtype):
    """the reference's own StructureEncoder and DFNet along `parents`"""
    ref_modules.get_parent_mapping = lambda model_type: list(parents)      # as model.network.net_modules sees it
    enc = ref_modules.StructureEncoder({"act": act, "beta": 100.0})
    dfnet = ref_modules.DFNet({"in_dim": 6 * len(parents), "dims": list(sko.HIDDEN), "act": act, "beta": 100.0, "num_layers": None})
    net = torch.nn.ModuleDict({"enc": enc, "dfnet": dfnet})
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dtype).eval()


def dist_grad(net, q):
    q = q.clone().requires_grad_(True)
    x = torch.nn.functional.normalize(q, dim=1)            # model/posendf.py:71
    d = net["dfnet"](net["enc"](x))
    (g,) = torch.autograd.grad(d, q, grad_outputs=torch.ones_like(d))      # gradient(), model/posendf.py:18-27
    return d.detach(), g.detach()


def project(net, q, steps):
    for _ in range(steps):                                 # experiments/sample_poses.py:67-74
        d, g = dist_grad(net, q)
        q = q - (d * g.reshape(len(q), -1)).reshape(q.shape)
    return q


def one(skel, act):
    parents = TABLES[skel]
    q_np = sko.poses(parents)
    for seed in range(64):
        sd = sko.network(parents, seed)
        d64, _ = dist_grad(ref_network(parents, act, sd, torch.float64), torch.from_numpy(q_np).double())
        if sko.clipped(d64.numpy(), act) * 4 <= len(q_np):
            break
    assert sko.clipped(d64.numpy(), act) * 4 <= len(q_np) and int((d64 == 0).sum()) * 4 <= len(q_np), (skel, act, "no seed keeps three quarters of the poses off the clip")
    out = {"q": q_np, "seed": np.array(seed), "parents": np.array(parents, np.int32)}
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        net = ref_network(parents, act, sd, dtype)
        q = torch.from_numpy(q_np).to(dtype)
        d, g = dist_grad(net, q)
        q3 = project(net, q, sko.STEPS)
        assert torch.isfinite(d).all() and torch.isfinite(g).all() and torch.isfinite(q3).all(), (skel, act, tag)
        out[f"d_{tag}"], out[f"dq_{tag}"], out[f"q3_{tag}"] = d.numpy(), g.numpy(), q3.numpy()
    keys = list(net.state_dict().keys())
    out["keys"] = np.array(keys)
    out["shapes"] = np.array([",".join(str(n) for n in net.state_dict()[k].shape) for k in keys])
    path = sko.fixture_path(skel, act)
    np.savez_compressed(path, **out)
    print(f"{path}: seed {seed}, {sko.clipped(out['d_f64'], act)} of {len(q_np)} poses clipped, mean d {float(out['d_f64'].mean()):.3f}, "
          f"{os.path.getsize(path) // 1024} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(8)
    for skel, act in sko.FIXTURE_CASES:
        one(skel, act)
