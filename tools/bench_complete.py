#!/usr/bin/env python3
"""Pose completion against the persistent projection launch (DESIGN.md section 2 "Pose completion"): milliseconds per call of
`PoseNDF.complete(observed=None)`, of `complete` with half of the joints observed, and of `PoseNDF.project` with the same step
options -- f16x3, lrelu and softplus, B = 4,096 and 65,536 x 100 steps.  `complete` is 2 launches per step (pndf_forward_grad +
the masked step kernel), `project` one persistent launch for all steps; `project` is code this feature does not touch.

The three calls alternate inside every repetition (same box, same minute); a call is timed with device events around it and the
median over the repetitions is reported, with the spread.  Before timing, complete(observed=None) is compared with project bit
for bit at the timed size.
usage: python tools/bench_complete.py [--out profiles/completion/bench.json] [--reps 7] [--steps 100]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import PoseNDF, amass_config, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "completion", "bench.json"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
args = ap.parse_args()

assert torch.cuda.is_available(), "tools/bench_complete.py measures on the GPU only"
dev = torch.device("cuda:0")
OPTS = dict(step_size=1.0, renormalize="unit", tol=0.0)      # unit joint quaternions after every step: what a completion caller asks for
sd = synth.make_weights(0, 2.0, 0.1)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
for act in ("lrelu", "softplus"):
    cfg = amass_config(act, "cuda:0")
    cfg["engine"] = {"precision": "f16x3"}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    for B in args.batches:
        q = torch.from_numpy(synth.make_poses(B, seed=1234)).to(dev)
        half = torch.from_numpy(np.random.RandomState(5).rand(B, 21) < 0.5).to(dev)
        calls = {"project": lambda: net.project(q, steps=args.steps, **OPTS),
                 "complete_none": lambda: net.complete(q, None, steps=args.steps, **OPTS),
                 "complete_half": lambda: net.complete(q, half, steps=args.steps, **OPTS)}
        a, da = calls["project"]()
        b, db = calls["complete_none"]()
        calls["complete_half"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(da.view(torch.int32), db.view(torch.int32)))
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                ms[k].append(event_ms(fn))
        row = {"act": act, "precision": "f16x3", "kernel": net._engine_for(dev).kernel_name(), "batch": B, "steps": args.steps,
               "options": OPTS, "reps": args.reps, "complete_none_equals_project_bit_for_bit": same}
        for k, v in ms.items():
            row[f"{k}_ms"] = float(np.median(v))
            row[f"{k}_ms_min_max"] = [float(min(v)), float(max(v))]
        row["ratio_complete_none_over_project"] = row["complete_none_ms"] / row["project_ms"]
        row["ratio_complete_half_over_project"] = row["complete_half_ms"] / row["project_ms"]
        row["complete_none_us_per_step"] = row["complete_none_ms"] / args.steps * 1e3
        row["project_us_per_step"] = row["project_ms"] / args.steps * 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows}, f, indent=1)
    f.write("\n")
