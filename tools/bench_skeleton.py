#!/usr/bin/env python3
"""Time per projection step of the skeleton unit (csrc/pndf_skeleton.hip; posendf_amd.SkeletonEngine) on the GPU, in one run:
  hand   the 15-joint hand with configs/amass.yaml's hidden widths: the unit against a PyTorch-ROCm loop over the stock modules
         (normalize -> encoder -> DFNet, autograd.grad, q <- q - d grad);
  smpl   the SMPL table with configs/amass.yaml's dims: the unit against the runtime-planned exact-fp32 engine (precision fp32,
         PNDF_FORCE_GENERIC=1 while the engine is created: pndf_generic on amass.yaml itself, one persistent launch per call)
         and against the same PyTorch-ROCm loop.
B = 4,096 and 65,536, 10 steps per call, lrelu and softplus, fp32 everywhere.  The contestants alternate call by call; each call is
timed with HIP events around work that ends in a synchronise; medians, minima and the spread (max / min) over --reps calls after
--warmup; the shader clock is read from the device properties and noted, not set.  One JSON line per case; --out writes the list
(profiles/skeleton/bench.json).
usage: python tools/bench_skeleton.py [--reps 10] [--warmup 2] [--steps 10] [--acts lrelu softplus] [--batches 4096 65536] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import amass_config, synth  # noqa: E402
from posendf_amd.engine import Engine, SkeletonEngine  # noqa: E402
from posendf_amd.modules import DFNet, StructureEncoder  # noqa: E402
from posendf_amd.skeleton import SKELETONS  # noqa: E402

DEV = "cuda:0"
HIDDEN = list(synth.DFNET_DIMS[1:-1])


def torch_loop(enc, dfnet, q, steps):
    for _ in range(steps):
        q = q.detach().requires_grad_(True)
        d = dfnet(enc(torch.nn.functional.normalize(q, dim=1)))
        (g,) = torch.autograd.grad(d.sum(), q)
        q = q - d.detach().reshape(-1, 1, 1) * g
    return q.detach()


def timed(calls, reps, warmup):
    """the contestants alternate; per-call times in ms, {name: [..]}"""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--acts", nargs="+", default=["lrelu", "softplus"])
    ap.add_argument("--batches", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_skeleton.py measures on the GPU"
    st = torch.cuda.current_stream().cuda_stream
    results = []
    for skel in ("hand", "smpl"):
        parents = SKELETONS[skel]
        J = len(parents)
        dims = synth.skeleton_dims(parents, HIDDEN)
        sd = synth.make_weights(0, 2.0, 0.1, dims=dims, parents=parents)
        macs = sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
        for act in a.acts:
            unit = SkeletonEngine(parents, act, hidden=HIDDEN)
            unit.load_weights(sd)
            cfg = amass_config(act, DEV)
            enc = StructureEncoder(dict(cfg["model"]["StrEnc"], parent_mapping=list(parents))).to(DEV)
            dfnet = DFNet(dict(cfg["model"]["DFNet"], in_dim=dims[0])).to(DEV)
            enc.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("enc.")})
            dfnet.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("dfnet.")})
            generic = None
            if skel == "smpl":
                os.environ["PNDF_FORCE_GENERIC"] = "1"
                try:
                    generic = Engine(act, precision="fp32")
                finally:
                    del os.environ["PNDF_FORCE_GENERIC"]
                generic.load_weights(sd)
            for B in a.batches:
                q = torch.from_numpy(synth.make_poses(B, seed=1, num_joints=J)).to(DEV)
                out, d = torch.empty_like(q), torch.empty(B, device=DEV)
                n = unit.workspace_bytes(B)
                ws = torch.empty(n, dtype=torch.uint8, device=DEV)
                calls = {"unit": lambda: unit.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, a.steps, ws.data_ptr(), n, st),
                         "torch": lambda: torch_loop(enc, dfnet, q, a.steps)}
                calls["unit"]()
                ref = torch_loop(enc, dfnet, q, a.steps)
                agree = float((out - ref).abs().max() / ref.abs().max())      # two fp32 evaluations: rounding, and kinks (relu family)
                names = {"unit": "pndf_skel_project"}
                if generic is not None:
                    out_g, d_g = torch.empty_like(q), torch.empty(B, device=DEV)
                    calls["generic"] = lambda: generic.project(q.data_ptr(), out_g.data_ptr(), d_g.data_ptr(), B, a.steps, st)
                    names["generic"] = generic.kernel_name()
                ms = timed(calls, a.reps, a.warmup)
                per_step = {k: float(np.median(x)) / a.steps for k, x in ms.items()}
                res = {"skeleton": skel, "joints": J, "act": act, "B": B, "steps_per_call": a.steps, "reps": a.reps, "warmup": a.warmup,
                       "dims": list(dims), "launches_per_step": 2 + 2 * (len(dims) - 1), "kernels": names,
                       "ms_per_step_median": per_step, "ms_per_step_min": {k: float(np.min(x)) / a.steps for k, x in ms.items()},
                       "spread_max_over_min": {k: float(np.max(x) / np.min(x)) for k, x in ms.items()},
                       "unit_over_torch": per_step["unit"] / per_step["torch"],
                       "unit_over_generic": per_step["unit"] / per_step["generic"] if generic is not None else None,
                       "unit_trunk_tflops": 2.0 * 2 * macs * B / (per_step["unit"] * 1e-3) / 1e12,
                       "projected_max_abs_difference_over_max_abs_vs_torch": agree, "workspace_MB": n / 1e6}
                print(json.dumps(res), flush=True)
                results.append(res)
    if a.out:
        prop = torch.cuda.get_device_properties(0)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "compute_units": prop.multi_processor_count,
                       "max_shader_clock_mhz": getattr(prop, "clock_rate", 0) / 1e3, "clocks": "as found, not set", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
