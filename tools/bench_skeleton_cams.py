#!/usr/bin/env python3
"""Moving cameras inside the projection step of the skeleton unit (csrc/pndf_skeleton.hip, pndf_fk_cams_energy_grad of csrc/pndf_fk.h,
pndf_project_options10): what a view table per pose or per frame in device memory -- pndf_skel_enc_rev_cams_kernel in place of the views /
root kernel -- costs.  Two comparisons on the GPU, the hand and a 32-joint tree with configs/amass.yaml's hidden widths, tracks of T = 16
frames, P * T = 4,096 and 65,536 poses, 10 steps per call, K = J keypoints on the joints plus one tip per leaf, medians of --reps calls
after --warmup:

  (a) this build against another build (--against LIBRARY, e.g. the parent commit's, loaded through PNDF_LIBRARY): the nine kinds of
      call that the other build has too -- plain, masked (pndf_project_options2), tracked (pndf_project_options3), denoising
      (pndf_project_options4), 3D fitting (pndf_project_options5), image fitting (pndf_project_options6), length fitting
      (pndf_project_options7), views (pndf_project_options8: V = 2) and the root trajectory (pndf_project_options9: the views call
      without scales, root_smooth = (0.25, 0.25)) --, one process per library, the processes alternating --rounds times in one run.  All
      nine run kernels this build does not change.  The other build is the yardstick: the margin is the spread (max / min) of ITS
      process medians over the rounds.
  (b) the moving-table call against the static-views call in this build, for V = 1, 2 and 8, on the same poses with every block equal to
      the static table (the two compute the same bits): the table per pose [B,V,16] and per frame [T,V,16], each without and with the
      root's coupling (root_smooth = (0.25, 0.25)), alternating call by call inside each process of this build, in a loop of its own
      behind the calls of (a).  The moving call reloads a row per (keypoint, view): 64 V K bytes requested per pose and step, of which
      64 V are new to the caches; the static call reads its table from the kernel's arguments.

Each call is timed with HIP events around work that ends in a synchronise; the shader clock is as found, not set.  A worker process
(--worker) prints one JSON line per case; the driver collects them and --out writes the summary (profiles/skeleton_cams/bench.json).
No PyTorch-ROCm loop is timed: there is none that does this work.
usage: python tools/bench_skeleton_cams.py --against PARENT_LIBRARY.so [--rounds 3] [--reps 10] [--warmup 2]
                                            [--steps 10] [--frames 16] [--timeout 240] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# 32 joints: three children under joint 0, a chain of depth 7, further branches and a second root (the tree of tests/skeleton_oracle.py)
TREE32 = (-1, 0, 0, 0, 1, 4, 5, 6, 7, 8, 2, 10, 10, 3, 13, 14, 14, 9, 9, 11, 12, 15, 16, -1, 23, 24, 24, 25, 26, 27, 28, 29)
DEV = "cuda:0"
OLD = ("plain", "masked", "tracked", "denoise", "fit", "image", "length", "views", "root")
VIEW_COUNTS = (1, 2, 8)
FORMS = ("static", "per_pose", "per_frame")
SMOOTH = (0.25, 0.25)
NEW = tuple(f"v{V}_{form}{tail}" for V in VIEW_COUNTS for tail in ("", "_coupled") for form in FORMS)


def view_rows(V):
    """[V,16]: V cameras eight units from the point (0, 0, 8) the roots sit around, spread over a turn"""
    table = np.zeros((V, 16), np.float32)
    for v in range(V):
        ang = 2.0 * np.pi * v / (V + 1)
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        table[v] = np.concatenate([[500.0, 480.0, 320.0, 240.0], R.reshape(9), np.array([0.0, 0.0, 8.0]) - R @ np.array([0.0, 0.0, 8.0])])
    return table


def worker(a):
    """one process, one library (PNDF_LIBRARY or the package's): every case, the contestants alternating call by call"""
    import torch
    from posendf_amd import synth
    from posendf_amd.engine import SkeletonEngine
    from posendf_amd.skeleton import SKELETONS
    assert torch.cuda.is_available(), "bench_skeleton_cams.py measures on the GPU"
    hidden = list(synth.DFNET_DIMS[1:-1])
    st = torch.cuda.current_stream().cuda_stream
    for skel, parents in (("hand", SKELETONS["hand"]), ("tree32", TREE32)):
        J = len(parents)
        sd = synth.make_weights(0, 2.0, 0.1, dims=synth.skeleton_dims(parents, hidden), parents=parents)
        for act in a.acts:
            unit = SkeletonEngine(parents, act, hidden=hidden)
            unit.load_weights(sd)
            for B in a.batches:
                q = torch.from_numpy(synth.make_poses(B, seed=1, num_joints=J)).to(DEV)
                out, d = torch.empty_like(q), torch.empty(B, device=DEV)
                n = unit.workspace_bytes(B)
                ws = torch.empty(n, dtype=torch.uint8, device=DEV)
                T = a.frames
                assert B % T == 0
                kw = dict(frames=T, smooth=0.5)
                r = np.random.RandomState(5)
                c = r.rand(B, J).astype(np.float32)
                c[r.rand(B, J) < 0.1] = 0.0      # a tenth of the detections missing
                conf = torch.from_numpy(c).to(DEV)
                words = torch.from_numpy((r.rand(B) * 2 ** J).astype(np.int64).astype(np.uint32).view(np.int32)).to(DEV)      # about half the joints held
                dk = dict(anchor_ptr=q.data_ptr(), conf_ptr=conf.data_ptr(), data=0.25, free_ends=True, **kw)
                tips = [j for j in range(J) if j not in parents]
                K = J + len(tips)
                rest = np.ascontiguousarray(r.uniform(-1, 1, (J, 3)), np.float32)
                kpj = np.asarray(list(range(J)) + tips, np.int32)
                kpo = np.ascontiguousarray(np.concatenate([np.zeros((J, 3)), r.uniform(-1, 1, (len(tips), 3))]), np.float32)
                y = torch.from_numpy(np.ascontiguousarray(r.uniform(-2, 2, (B, K, 3)), np.float32)).to(DEV)
                kc = r.rand(B, K).astype(np.float32)
                kc[r.rand(B, K) < 0.1] = 0.0
                kconf, energy = torch.from_numpy(kc).to(DEV), torch.empty(B, device=DEV)
                tables = dict(kp_conf_ptr=kconf.data_ptr(), kp_energy_ptr=energy.data_ptr(), rest_ptr=rest.ctypes.data, kp_joint_ptr=kpj.ctypes.data,
                              kp_offset_ptr=kpo.ctypes.data, n_keypoints=K, kp_weight=0.02)
                fk = dict(kp_target_ptr=y.data_ptr(), **tables)

                def call(**opts):
                    return lambda: unit.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, a.steps, ws.data_ptr(), n, st, **opts)

                pix = torch.from_numpy(np.ascontiguousarray(np.asarray([320.0, 240.0]) + r.uniform(-200, 200, (B, K, 2)), np.float32)).to(DEV)
                # a root per pose, eight units in front of the camera: written by every step, so each call starts from a fresh copy
                root0 = np.zeros((B, 7), np.float32)
                root0[:, 0] = 1.0
                root0[:, 1:4] = 0.15 * r.randn(B, 3)
                root0[:, 4:] = r.uniform(-1, 1, (B, 3)) + np.asarray([0.0, 0.0, 8.0])
                root_start, root = torch.from_numpy(root0).to(DEV), torch.empty(B, 7, device=DEV)
                ik = dict(kp_target_ptr=pix.data_ptr(), **tables, root_ptr=root.data_ptr(), root_weights=(0.05, 0.3), camera=(500.0, 480.0, 320.0, 240.0))

                def fresh(fn):
                    def run():
                        root.copy_(root_start)      # (a 1.8 MB copy at B = 65,536 inside the timed region: under 0.1 % of a call)
                        fn()
                    return run
                S = J + K
                scale0 = r.uniform(0.8, 1.25, (B, S)).astype(np.float32)      # written by every step: each call starts from a fresh copy
                scale_start, scale = torch.from_numpy(scale0).to(DEV), torch.empty(B, S, device=DEV)
                lk = dict(bone_scale_ptr=scale.data_ptr(), len_weight=0.05, len_prior=0.1, len_range=(0.5, 2.0))

                def fresh_scale(fn, rows):
                    def run():
                        scale[:rows].copy_(scale_start[:rows])
                        fn()
                    return run
                vmax = max(VIEW_COUNTS)
                vpix_all = np.ascontiguousarray(np.asarray([320.0, 240.0]) + r.uniform(-200, 200, (B, vmax, K, 2)), np.float32)
                vc_all = r.rand(B, vmax, K).astype(np.float32)
                vc_all[r.rand(B, vmax, K) < 0.1] = 0.0
                keep = []      # (the device arrays behind the addresses below)

                def views_call(V):
                    vpix = torch.from_numpy(np.ascontiguousarray(vpix_all[:, :V])).to(DEV)
                    vconf = torch.from_numpy(np.ascontiguousarray(vc_all[:, :V])).to(DEV)
                    keep.extend([vpix, vconf])
                    vk = dict(ik, kp_target_ptr=vpix.data_ptr(), kp_conf_ptr=vconf.data_ptr())
                    vk.pop("camera")
                    return vk
                v2 = views_call(2)
                # comparison (a): the same nine calls in the same order in both builds; comparison (b) is a loop of its own behind it
                groups = [{"plain": call(), "masked": call(observed_ptr=words.data_ptr()), "tracked": call(**kw), "denoise": call(**dk), "fit": call(**dk, **fk),
                           "image": fresh(call(**dk, **ik)), "length": fresh_scale(fresh(call(**dk, **ik, **lk)), B // T),
                           "views": fresh_scale(fresh(call(**dk, **v2, views=view_rows(2), **lk)), B // T),
                           "root": fresh(call(**dk, **v2, views=view_rows(2), root_smooth=SMOOTH))}]
                if a.moving:
                    moving = {}
                    for V in VIEW_COUNTS:
                        vk = views_call(V)
                        rows = view_rows(V)
                        per_pose = torch.from_numpy(np.ascontiguousarray(np.tile(rows, (B, 1, 1)))).to(DEV)
                        per_frame = torch.from_numpy(np.ascontiguousarray(np.tile(rows, (T, 1, 1)))).to(DEV)
                        for tail, extra in (("", {}), ("_coupled", dict(root_smooth=SMOOTH))):
                            moving[f"v{V}_static{tail}"] = fresh(call(**dk, **vk, views=rows, **extra))
                            moving[f"v{V}_per_pose{tail}"] = fresh(call(**dk, **vk, pose_views=per_pose, **extra))
                            moving[f"v{V}_per_frame{tail}"] = fresh(call(**dk, **vk, pose_views=per_frame, views_per_frame=True, **extra))
                    groups.append(moving)
                ms = {}
                for calls in groups:
                    for _ in range(a.warmup):
                        for fn in calls.values():
                            fn()
                    torch.cuda.synchronize()
                    ms.update({k: [] for k in calls})
                    for _ in range(a.reps):
                        for k, fn in calls.items():
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            torch.cuda.synchronize()
                            ms[k].append(e0.elapsed_time(e1))
                print(json.dumps({"skeleton": skel, "joints": J, "keypoints": K, "act": act, "B": B,
                                  "ms_per_step_median": {k: float(np.median(x)) / a.steps for k, x in ms.items()},
                                  "ms_per_step_min": {k: float(np.min(x)) / a.steps for k, x in ms.items()},
                                  "spread_max_over_min": {k: float(np.max(x) / np.min(x)) for k, x in ms.items()}}), flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                      "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}), flush=True)


def run_worker(a, library, moving):
    """a fresh process under its own time limit; its JSON lines.  A process that fails ends the run: nothing more is started."""
    env = dict(os.environ)
    env.pop("PNDF_LIBRARY", None)
    if library:
        env["PNDF_LIBRARY"] = os.path.abspath(library)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--warmup", str(a.warmup), "--steps", str(a.steps),
           "--acts", *a.acts, "--frames", str(a.frames), "--batches", *[str(b) for b in a.batches]] + (["--moving"] if moving else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"worker with {library or 'this build'} ended with status {r.returncode}: the run stops here")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--moving", action="store_true", help="(worker) also time the moving-table calls: needs a build with pndf_project_options10")
    ap.add_argument("--frames", type=int, default=16, help="T: frames of a track")
    ap.add_argument("--against", default=None, help="the library of the other build (the yardstick of comparison (a))")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one worker process may take")
    ap.add_argument("--acts", nargs="+", default=["lrelu"])
    ap.add_argument("--batches", nargs="+", type=int, default=[4096, 65536])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    runs = {"against": [], "this": []}
    device = None
    for i in range(a.rounds):      # the processes alternate: the other build first
        if a.against:
            runs["against"].append(run_worker(a, a.against, moving=False)[:-1])
            print(f"[round {i + 1} of {a.rounds}] the other build's process is done", file=sys.stderr, flush=True)
        lines = run_worker(a, None, moving=True)
        print(f"[round {i + 1} of {a.rounds}] this build's process is done", file=sys.stderr, flush=True)
        runs["this"].append(lines[:-1])
        device = lines[-1]
    results = []
    for i, case in enumerate(runs["this"][0]):
        mine = [r[i]["ms_per_step_median"] for r in runs["this"]]
        res = {k: case[k] for k in ("skeleton", "joints", "keypoints", "act", "B")}
        for k in OLD + NEW:
            res[f"this_build_{k}_ms_per_step"] = [m[k] for m in mine]
        res["within_call_spread_max_over_min"] = [r[i]["spread_max_over_min"] for r in runs["this"]]
        med = {k: float(np.median(res[f"this_build_{k}_ms_per_step"])) for k in OLD + NEW}
        for V in VIEW_COUNTS:
            for tail in ("", "_coupled"):
                for form in FORMS[1:]:
                    res[f"b_v{V}_{form}{tail}_over_static"] = med[f"v{V}_{form}{tail}"] / med[f"v{V}_static{tail}"]
                    res[f"b_v{V}_{form}{tail}_minus_static_ms_per_step"] = med[f"v{V}_{form}{tail}"] - med[f"v{V}_static{tail}"]
            res[f"b_v{V}_table_bytes_per_pose_and_step_first_touch"] = 64 * V
            res[f"b_v{V}_table_bytes_per_pose_and_step_requested"] = 64 * V * case["keypoints"]
        if a.against:
            for k in OLD:
                other = [r[i]["ms_per_step_median"][k] for r in runs["against"]]
                res[f"other_build_{k}_ms_per_step"] = other
                res[f"other_build_{k}_spread_max_over_min"] = float(np.max(other) / np.min(other))
                res[f"a_this_over_other_{k}"] = med[k] / float(np.median(other))
                res[f"a_{k}_inside_the_other_builds_spread"] = bool(med[k] <= float(np.max(other)))
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({**(device or {}), "clocks": "as found, not set", "steps_per_call": a.steps, "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
                       "rounds": a.rounds, "acts": a.acts, "against": os.path.basename(a.against) if a.against else None,
                       "what": "(a) the plain, masked, tracked (lambda 0.5), denoising (anchor, confidences, mu 0.25, free ends), 3D fitting (K = J + one "
                               "tip per leaf keypoints, confidences, nu 0.02), image fitting (pixel targets, a camera, a free root, nu_rot 0.05, nu_trans "
                               "0.3), length fitting (one row of S = J + K scales per track, nu_len 0.05, kappa 0.1, clamp 0.5 .. 2), views (the length "
                               "call with V = 2) and root (the views call without scales, root_smooth = (0.25, 0.25)) calls, this build over the other "
                               "build, one process per library, alternating; (b) the views call without scales for V = 1, 2 and 8 with its table given "
                               "per pose [B,V,16] and per frame [T,V,16] in device memory (pndf_project_options10: pndf_skel_enc_rev_cams_kernel, the "
                               "row of a view reloaded per (keypoint, view): 64 V K bytes requested per pose and step, 64 V of them first touches) over "
                               "the same call with the static table of pndf_project_options8, every block equal to that table, without and with the "
                               "root's coupling, alternating call by call inside this build's processes",
                       "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
