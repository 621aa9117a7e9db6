#!/usr/bin/env python3
"""Image fitting (posendf_amd.image_fitting.ImageFit, csrc/pndf_keypoints.hip): time per Adam step of stage 1 (translation and
orientation: 3 launches) and of stage 2 (pose and orientation: 6 launches) of the fused driver at S x T = 512 x 1 (images) and
512 x 300 (videos), SMPL-sized synthetic body model (6,890 vertices, 45 joints), and the same stage-2 step through stock
PyTorch-ROCm autograd on the same GPU (oracle/lbs_torch.torch_lbs + oracle/posendf_torch.RefNet + torch.optim.Adam, fp32).
The PyTorch body model is kept to at most 1,200 frames per call -- bench.py's limit for that restatement (larger calls have
ended in a memory fault inside PyTorch) --, so for 512 x 300 the comparator runs 4 x 300 frames and is compared per frame.
HIP events, warm-up, median of --reps windows of --steps steps.  One JSON line per shape.

The keypoint kernel's own time comes from a kernel trace, a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o image_fit -- python tools/bench_image_fit.py --shapes 512x300 --no-torch
    python tools/bench_image_fit.py --kernel-stats DIR/.../image_fit_kernel_stats.csv --shapes 512x300
The second command prints the kernel's share of the traced kernel time and its fraction of the HBM roof from the bytes the
kernel needs: 36 J + 60 per frame with every output (stage 2 writes no translation gradient and no terms: 36 J + 40).
usage: python tools/bench_image_fit.py [--shapes 512x1 512x300] [--steps 20] [--reps 5] [--no-torch] [--out FILE]"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import BodyModel, ImageFit, PoseNDF, amass_config, synth  # noqa: E402
from posendf_amd.image_fitting import _FusedFit  # noqa: E402

PEAK_HBM = 8.0e12            # bytes/s (MI355X)
TORCH_MAX_FRAMES = 1200
J = 45


def kernel_bytes(N, stage):
    """what pndf_keypoint_terms_grad has to move: joints and keypoints in (24 J), g_joints out (12 J), orient + transl in (24),
    g_orient out (12); stage 1 adds g_transl (12) and drops g_joints"""
    return N * ((24 * J + 24 + 12 + 12) if stage == 1 else (36 * J + 24 + 12))


def timed(step, steps, reps):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms)), [float(x) for x in ms]


def make_inputs(S, T, m, seed=0):
    """keypoints [S,T,45,3]: the projection of smooth random poses at depth ~10 plus 2 px of noise, 10 % of the confidences 0"""
    from posendf_amd.image_fitting import PerspectiveCamera, project
    g = torch.Generator().manual_seed(seed)
    N = S * T
    th = (torch.cumsum(0.03 * torch.randn(S, T, 69, generator=g), 1) + 0.15 * torch.randn(S, 1, 69, generator=g)).reshape(N, 69)
    r = 0.15 * torch.randn(N, 3, generator=g)
    t = torch.tensor([0.0, 0.0, 10.0]) + torch.randn(N, 3, generator=g) * torch.tensor([0.2, 0.2, 0.4])
    bm = BodyModel(m, device="cuda:0")
    uv = project(bm.joints_of(th), r.cuda(), t.cuda(), PerspectiveCamera(), posed=False)[1].cpu()
    conf = (torch.rand(N, J, 1, generator=g) > 0.1).float() * (0.5 + 0.5 * torch.rand(N, J, 1, generator=g))
    return bm, torch.cat([uv + 2.0 * torch.randn(N, J, 2, generator=g), conf], -1).reshape(S, T, J, 3)


def torch_stage2(net, m, kp, S, T):
    """the stage-2 step as stock PyTorch-ROCm executes it: returns (step function, tensors it optimises)"""
    from oracle.lbs_torch import torch_lbs
    N = S * T
    dev = kp.device
    kp = kp.reshape(N, J, 3)
    pose = torch.zeros(N, 69, device=dev, requires_grad=True)
    orient = torch.zeros(N, 3, device=dev, requires_grad=True)
    transl = torch.tensor([0.0, 0.0, 10.0], device=dev).repeat(N, 1)
    opt = torch.optim.Adam([pose, orient], 0.02, betas=(0.9, 0.999))
    keep = kp[..., 2] != 0
    kxy = torch.where(keep[..., None], kp[..., :2], torch.zeros_like(kp[..., :2]))
    eye = torch.eye(3, device=dev)

    def step():
        opt.zero_grad()
        ang = torch.norm(pose.reshape(N, 23, 3)[:, :21], dim=-1, keepdim=True)
        small = ang < 1e-6
        k = torch.where(small, 0.5 - ang * ang / 48.0, torch.sin(0.5 * ang) / torch.where(small, torch.ones_like(ang), ang))
        d = net(torch.cat([torch.cos(0.5 * ang), pose.reshape(N, 23, 3)[:, :21] * k], -1)).reshape(S, T)
        joints = torch_lbs(pose, m, torch.float32)[1]
        angle = torch.norm(orient + 1e-8, dim=1, keepdim=True)
        n = orient / angle
        z = torch.zeros_like(n[:, 0])
        K = torch.stack([z, -n[:, 2], n[:, 1], n[:, 2], z, -n[:, 0], -n[:, 1], n[:, 0], z], 1).view(N, 3, 3)
        R = eye + torch.sin(angle)[:, None] * K + (1 - torch.cos(angle))[:, None] * (K @ K)
        J0 = joints[:, :1].detach()
        p = (joints - J0) @ R.transpose(1, 2) + J0 + transl[:, None]
        e = kxy - 5000.0 * p[..., :2] / p[..., 2:3]
        E = (kp[..., 2:3] ** 2 * e * e).sum()
        (100.0 * d.mean(1).sum() + 10.0 * E).backward()
        opt.step()
    return step, (pose, orient)


def stats_report(path, shapes):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    mine = [r for r in rows if "pndf_keypoint_terms_grad_kernel" in r["Name"]]
    if not mine:
        raise SystemExit(f"{path}: no pndf_keypoint_terms_grad_kernel row")
    S, T = shapes[-1]
    N = S * T
    out = {"tool": "bench_image_fit", "kernel_stats": path, "kernel": "pndf_keypoint_terms_grad_kernel", "shape": f"{S}x{T}",
           "calls": sum(int(r["Calls"]) for r in mine), "share_of_traced_kernel_time": sum(float(r["TotalDurationNs"]) for r in mine) / total,
           "min_us": min(float(r["MinNs"]) for r in mine) * 1e-3, "average_us": float(mine[0]["AverageNs"]) * 1e-3,
           "max_us": max(float(r["MaxNs"]) for r in mine) * 1e-3}
    for stage in (1, 2):
        b = kernel_bytes(N, stage)
        out[f"stage{stage}_bytes"] = b
        out[f"stage{stage}_least_us_at_hbm_roof"] = b / PEAK_HBM * 1e6
    # the trace mixes both stages' calls: the average call against the larger (stage-2) byte count bounds the fraction from above,
    # against the smaller one from below
    out["fraction_of_hbm_roof_average_call"] = [kernel_bytes(N, 1) / PEAK_HBM / (out["average_us"] * 1e-6),
                                                kernel_bytes(N, 2) / PEAK_HBM / (out["average_us"] * 1e-6)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["512x1", "512x300"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a traced run of this tool: report the kernel's share")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes]
    if a.kernel_stats:
        return stats_report(a.kernel_stats, shapes)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_fit.py needs a GPU")
    sd = synth.make_weights(0, 2.0, 0.1)
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": a.precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    m = synth.make_body_model(seed=11)
    for S, T in shapes:
        N = S * T
        bm, kp = make_inputs(S, T, m)
        fit = ImageFit(net, bm, device="cuda:0", batch_size=N)
        run = _FusedFit(fit, *fit._prepare(kp, None)[:7])
        k = [0]

        def stage1():
            k[0] += 1
            run.stage1_step(k[0])
        ms1, all1 = timed(stage1, a.steps, a.reps)
        run.begin_stage2()
        k[0] = 0

        def stage2():
            k[0] += 1
            run.stage2_step(k[0], 0)
        ms2, all2 = timed(stage2, a.steps, a.reps)
        ok = bool(torch.isfinite(run.bufs[0]).all() and torch.isfinite(run.orient).all() and torch.isfinite(run.transl).all())
        rec = {"tool": "bench_image_fit", "S": S, "T": T, "frames": N, "joints": J, "vertices": bm.num_vertices, "precision": a.precision,
               "steps_per_window": a.steps, "stage1_ms_per_step": ms1, "stage1_ms_windows": all1, "stage1_launches": 3,
               "stage2_ms_per_step": ms2, "stage2_ms_windows": all2, "stage2_launches": 6, "stage2_frames_per_s": N / (ms2 * 1e-3),
               "finite": ok, "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        if not a.no_torch:
            from oracle.posendf_torch import RefNet
            St = S if N <= TORCH_MAX_FRAMES else max(1, TORCH_MAX_FRAMES // T)
            ref = RefNet("lrelu").cuda()
            ref.load_state_dict({k_: torch.from_numpy(v) for k_, v in sd.items()})
            for p in ref.parameters():
                p.requires_grad_(False)
            step, _ = torch_stage2(ref, m, kp[:St].cuda(), St, T)
            mst, allt = timed(step, max(2, a.steps // 4), max(2, a.reps // 2))
            rec.update({"torch_stage2_sequences": St, "torch_stage2_frames": St * T, "torch_stage2_ms_per_step": mst, "torch_stage2_ms_windows": allt,
                        "stage2_speedup_per_frame_vs_torch": (mst / (St * T)) / (ms2 / N)})
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del run, fit, bm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
