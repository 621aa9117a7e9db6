#!/usr/bin/env python3
"""One training step of the reference's trainer (model/train_posendf.py:93-98: zero_grad, model(...), loss weights 1/1/1, backward)
on configs/amass.yaml dims, B = Bm = 20,000 (amass.yaml: 4 files x 5,000 poses), eikonal on, L1 loss: the HIP objective
(opt['engine']['train'] = 'hip', csrc/pndf_train.hip) against the stock PyTorch-ROCm path (the facade default, fp32) on the same
GPU.  Objective forward + backward timed with HIP events, median and minimum over --steps steps after --warmup; the FLOP count is
10 trunk matrix passes per noisy + manifold pose pair (7 for the noisy pose, 3 for the manifold pose) at 2 FLOP per multiply-add.
One JSON line per activation.  --skeleton NAME (a name of posendf_amd.SKELETONS) times the same step of `SkeletonPoseNDF` on that
joint tree (include/posendf_amd_skeleton_train.h) instead of `PoseNDF`; --reps R repeats the timed block R times, the arms
alternating, and reports every repetition's median and their spread (max - min).
usage: python tools/bench_train.py [--steps 20] [--warmup 3] [--reps 1] [--hip-only] [--acts lrelu softplus] [--skeleton hand]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import SKELETONS, PoseNDF, SkeletonPoseNDF, amass_config, skeleton_config, synth  # noqa: E402

FP32_PEAK = 157.3e12


def model(act, backend, skeleton=None):
    if skeleton is None:
        cfg = amass_config(act, "cuda:0")
        cfg["engine"] = {"train": backend}
        net = PoseNDF(cfg)
        sd = synth.make_weights(0, 2.0, 0.1)
    else:
        parents = SKELETONS[skeleton]
        cfg = skeleton_config(skeleton, act, "cuda:0")
        cfg["engine"] = {"train": backend}
        net = SkeletonPoseNDF(cfg)
        sd = synth.make_weights(0, 2.0, 0.1, dims=synth.skeleton_dims(parents, synth.DFNET_DIMS[1:-1], True), parents=tuple(parents))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.train()


def step(net, q, gt, qm):
    net.zero_grad(set_to_none=True)
    _, ld = net(q, gt, qm, train=True, eikonal=1.0)
    loss = 0.0
    for k in ld:
        loss = loss + 1.0 * ld[k]
    loss.backward()


def timed(net, q, gt, qm, steps, warmup):
    for _ in range(warmup):
        step(net, q.clone(), gt, qm)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        qs = q.clone()          # the stock path marks the caller's pose tensor requires_grad: a fresh leaf per step
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(net, qs, gt, qm)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--acts", nargs="+", default=["lrelu", "softplus"])
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--skeleton", choices=sorted(SKELETONS), default=None, help="time SkeletonPoseNDF on this joint tree instead of PoseNDF")
    ap.add_argument("--reps", type=int, default=1, help="repetitions of the timed block, the arms alternating")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train.py measures on the GPU"
    B = Bm = a.batch
    J = 21 if a.skeleton is None else len(SKELETONS[a.skeleton])
    dims = (6 * J,) + tuple(synth.DFNET_DIMS[1:])
    macs = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    flop = 2.0 * 10 * macs * B
    q = torch.from_numpy(synth.make_poses(B, seed=1, num_joints=J)).cuda()
    qm = torch.from_numpy(synth.make_poses(Bm, seed=2, num_joints=J)).cuda()
    gt = torch.from_numpy(np.random.default_rng(3).uniform(0, 0.5, B).astype(np.float32)).cuda()
    for act in a.acts:
        res = {"act": act, "B": B, "Bm": Bm, "eikonal": 1.0, "loss": "l1", "steps": a.steps, "warmup": a.warmup,
               "trunk_macs_per_pass": macs, "flop_per_step": flop}
        if a.skeleton is not None:
            res.update(skeleton=a.skeleton, num_joints=J)
        arms = {"hip": model(act, "hip", a.skeleton)}
        if not a.hip_only:
            arms["stock"] = model(act, "torch", a.skeleton)
        runs = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, net in arms.items():
                runs[name].append(timed(net, q, gt, qm, a.steps, a.warmup))
        med, mn = float(np.median([r[0] for r in runs["hip"]])), min(r[1] for r in runs["hip"])
        res.update(hip_ms_median=med, hip_ms_min=mn, hip_tflops_median=flop / med / 1e9,
                   hip_fraction_of_fp32_peak=flop / (med * 1e-3) / FP32_PEAK)
        if not a.hip_only:
            smed, smn = float(np.median([r[0] for r in runs["stock"]])), min(r[1] for r in runs["stock"])
            res.update(stock_ms_median=smed, stock_ms_min=smn, speedup_median=smed / med)
        if a.reps > 1:
            res["reps"] = a.reps
            for name, rr in runs.items():
                meds = [r[0] for r in rr]
                res.update({f"{name}_ms_medians": meds, f"{name}_ms_spread": max(meds) - min(meds)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
