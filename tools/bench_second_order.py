#!/usr/bin/env python3
"""`pndf_second_order` (csrc/pndf_second_order.hip; PoseNDF.hvp: d, grad d, <v, grad d> and w_d grad d + w_t H v in one call) against
the stock PyTorch-ROCm modules' double backward (normalize -> encoder -> DFNet, autograd.grad with create_graph=True, then
autograd.grad of sum(w_d d + w_t <v, grad d>)) on the same GPU in the same run: configs/amass.yaml dims, lrelu and softplus,
B = 4,096 and 65,536, fp32 on both sides.  The two contestants alternate call by call; each call is timed with HIP events around
work that ends in a synchronise; medians and minima over --steps calls after --warmup.  The FLOP count is the trunk's matrix passes
per pose (softplus: forward, tangent forward and the two adjoint chains = 4; relu family: forward and one adjoint chain = 2) at
2 FLOP per multiply-add.  One JSON line per case; --out writes the list (profiles/second_order/bench.json).
usage: python tools/bench_second_order.py [--steps 20] [--warmup 3] [--acts lrelu softplus] [--batches 4096 65536] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import PoseNDF, amass_config, synth  # noqa: E402
from posendf_amd.modules import DFNet, StructureEncoder  # noqa: E402

FP32_PEAK = 157.3e12
DEV = "cuda:0"


def stock_call(enc, dfnet, q, v, w_d, w_t):
    q = q.clone().requires_grad_(True)
    d = dfnet(enc(torch.nn.functional.normalize(q, dim=1)))
    (g,) = torch.autograd.grad(d.sum(), q, create_graph=True)
    t = (v * g).sum(dim=(1, 2))
    (out,) = torch.autograd.grad((w_d * d[:, 0] + w_t * t).sum(), q)
    return d.detach(), g.detach(), t.detach(), out


def timed_pair(calls, steps, warmup):
    """the contestants alternate; per-call times in ms, {name: [..]}"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(steps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--acts", nargs="+", default=["lrelu", "softplus"])
    ap.add_argument("--batches", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_second_order.py measures on the GPU"
    dims = synth.DFNET_DIMS
    macs = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    sd = synth.make_weights(0, 2.0, 0.1)
    results = []
    for act in a.acts:
        cfg = amass_config(act, DEV)
        net = PoseNDF(cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.eval()
        enc, dfnet = StructureEncoder(cfg["model"]["StrEnc"]).to(DEV), DFNet(cfg["model"]["DFNet"]).to(DEV)
        enc.load_state_dict(net.enc.state_dict())
        dfnet.load_state_dict(net.dfnet.state_dict())
        for B in a.batches:
            rs = np.random.RandomState(B)
            q = torch.from_numpy(synth.make_poses(B, seed=1, signed=True)).to(DEV)
            v = torch.from_numpy(rs.normal(size=(B, 21, 4)).astype(np.float32)).to(DEV)
            w_d = torch.from_numpy(rs.uniform(0.5, 1.5, B).astype(np.float32)).to(DEV)
            w_t = torch.from_numpy(rs.uniform(0.5, 1.5, B).astype(np.float32)).to(DEV)
            hip = net.hvp(q, v, w_d, w_t)
            ref = stock_call(enc, dfnet, q, v, w_d, w_t)
            agree = float((hip[3] - ref[3]).abs().max() / ref[3].abs().max())      # two fp32 evaluations: rounding, and kinks (relu family)
            ms = timed_pair({"hip": lambda: net.hvp(q, v, w_d, w_t), "stock": lambda: stock_call(enc, dfnet, q, v, w_d, w_t)}, a.steps, a.warmup)
            passes = 4 if act == "softplus" else 2
            flop = 2.0 * passes * macs * B
            med = {k: float(np.median(x)) for k, x in ms.items()}
            res = {"act": act, "B": B, "steps": a.steps, "warmup": a.warmup, "trunk_macs_per_pass": macs, "trunk_passes": passes,
                   "flop_per_call": flop, "hip_ms_median": med["hip"], "hip_ms_min": float(np.min(ms["hip"])),
                   "stock_ms_median": med["stock"], "stock_ms_min": float(np.min(ms["stock"])),
                   "speedup_median": med["stock"] / med["hip"], "hip_tflops_median": flop / med["hip"] / 1e9,
                   "hip_fraction_of_fp32_peak": flop / (med["hip"] * 1e-3) / FP32_PEAK,
                   "out_max_abs_difference_over_max_abs": agree,
                   "workspace_MB": net._so_engines[0].workspace_floats(B) * 4 / 1e6}
            print(json.dumps(res), flush=True)
            results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
