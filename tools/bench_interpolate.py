#!/usr/bin/env python3
"""Pose interpolation against pose completion (DESIGN.md section 2 "Pose interpolation"): milliseconds per call of
`PoseNDF.interpolate` with the neighbour coupling off (smooth = 0) and on (smooth = 0.5), and of `PoseNDF.complete` on the same
number of poses with the same step options -- f16x3, lrelu and softplus, P x T = 4,096 and 65,536 poses with T = 16 frames, 100
steps.  Both are 2 launches per step (pndf_forward_grad + one element-wise kernel); `interpolate` adds the fill launch and, with
the coupling on, two more 16-byte loads per free lane of its step kernel.  `complete` is code this feature does not touch.

The three calls alternate inside every repetition (same box, same minute); a call is timed with device events around it and the
median over the repetitions is reported, with the spread.  Before timing, interpolate(smooth=0) is compared bit for bit with
complete on the filled track with the end frames observed, at the timed size.

The band kernel's own time and its share of the HBM roof come from a separate `rocprofv3 --kernel-trace --stats` run of this
script (`--reps 1`), not from here: bytes per lane are counted as in csrc/pndf_interp.hip's header (a held lane 16 B in + 16 B out,
a free lane with the coupling on four 16-byte loads, d and the store).
usage: python tools/bench_interpolate.py [--out profiles/interpolation/bench.json] [--reps 7] [--steps 100] [--frames 16]"""
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
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "interpolation", "bench.json"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--frames", type=int, default=16)
ap.add_argument("--poses", type=int, nargs="+", default=[4096, 65536], help="P x T of a call (multiples of --frames)")
args = ap.parse_args()

assert torch.cuda.is_available(), "tools/bench_interpolate.py measures on the GPU only"
dev = torch.device("cuda:0")
OPTS = dict(step_size=1.0, renormalize="unit", tol=0.0)
T = args.frames
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
    for B in args.poses:
        assert B % T == 0, (B, T)
        P = B // T
        a = torch.from_numpy(synth.make_poses(P, seed=1234)).to(dev)
        b = torch.from_numpy(synth.make_poses(P, seed=4321, signed=True)).to(dev)
        fill = net.interpolate(a, b, T, steps=0, return_dist=False).reshape(B, 21, 4)
        ends = torch.zeros(P, T, 21, dtype=torch.bool, device=dev)
        ends[:, 0] = ends[:, -1] = True
        ends = ends.reshape(B, 21)
        calls = {"complete": lambda: net.complete(fill, ends, steps=args.steps, **OPTS),
                 "interpolate_smooth0": lambda: net.interpolate(a, b, T, steps=args.steps, smooth=0.0, **OPTS),
                 "interpolate_smooth05": lambda: net.interpolate(a, b, T, steps=args.steps, smooth=0.5, **OPTS)}
        c, dc = calls["complete"]()
        i0, d0 = calls["interpolate_smooth0"]()
        calls["interpolate_smooth05"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(c.view(torch.int32), i0.reshape(B, 21, 4).view(torch.int32))
                    and torch.equal(dc.reshape(-1).view(torch.int32), d0.reshape(-1).view(torch.int32)))
        ms = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, fn in calls.items():
                ms[k].append(event_ms(fn))
        row = {"act": act, "precision": "f16x3", "kernel": net._engine_for(dev).kernel_name(), "pairs": P, "frames": T, "poses": B,
               "steps": args.steps, "options": OPTS, "reps": args.reps, "interpolate_smooth0_equals_complete_bit_for_bit": same}
        for k, v in ms.items():
            row[f"{k}_ms"] = float(np.median(v))
            row[f"{k}_ms_min_max"] = [float(min(v)), float(max(v))]
        row["ratio_smooth0_over_complete"] = row["interpolate_smooth0_ms"] / row["complete_ms"]
        row["ratio_smooth05_over_complete"] = row["interpolate_smooth05_ms"] / row["complete_ms"]
        row["interpolate_smooth05_us_per_step"] = row["interpolate_smooth05_ms"] / args.steps * 1e3
        row["complete_us_per_step"] = row["complete_ms"] / args.steps * 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows}, f, indent=1)
    f.write("\n")
