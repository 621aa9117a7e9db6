"""Online training data on the GPU (posendf_amd.online, csrc/pndf_online.hip): what a regenerated pool costs.

  sampler   pndf_online_sample alone, P = 65,536 and 1,048,576 poses over a manifold of N = 1,048,576: time per launch, the bytes
            the algorithm needs (672 per pose: one 336-byte row read, one written; src and group are not asked for) and their
            share of the HBM roof the project's other benches use.  The gather's sector waste is not counted, so the share is a
            lower bound of the traffic.
  refresh   OnlinePoseDataset.refresh -- the sampler plus pndf_knn_search in chunks -- at P = 200,000 (40 virtual files of 5,000
            rows), N = 1,048,576, k = 5, geo.
  step      the file-based Trainer.step() at amass.yaml's batch (4 x 5,000), measured in the same run, and next to it the
            refresh amortised over the steps it serves: a pool of 40 files is 10 steps per epoch, times refresh_every = 1 and 10.

Every window is timed with device events around a loop that ends in a synchronise, after a warm-up of the same shape; three
windows each, median and spread reported.  One JSON document, printed and written to --out.  --num_joints J (1 .. 32) measures the
sampler (32 J bytes per pose) and the refresh for poses of J joints (include/posendf_amd_skeleton_data.h); with another J than 21 the
step rows, which are the 21-joint trainer's, are left out.
usage: python tools/bench_online.py [--out profiles/online/bench.json] [--steps 100] [--warmup 10] [--num_joints 21]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import amass_config, engine, synth  # noqa: E402
from posendf_amd.online import OnlineOptions, OnlinePoseDataset  # noqa: E402
from posendf_amd.trainer import PoseDataset, Trainer  # noqa: E402

DEV = "cuda:0"
HBM_ROOF = 6.3e12        # achievable bytes per second of an MI355X (8.0e12 on paper): tools/bench_trainer.py's
N_MAN = 1 << 20
ITEMS, NUM_PTS, K, ROWS = 4, 5000, 5, 2000
POOL_FILES, POOL_ROWS = 40, 5000
WINDOWS = 3


def unit_poses(n, seed, J=21):
    """seeded unit quaternions [n,J,4] made on the device (a million poses from the host generator take longer than the bench)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(n, J, 4, device=DEV, generator=g)
    return q / q.norm(dim=2, keepdim=True)


def loop_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def windows(fn, target_s=0.5, least=20, most=20000):
    """warm up, size the window to about target_s, time WINDOWS of them: (median ms, [ms per window], reps)"""
    est = loop_ms(fn, least)
    reps = int(min(most, max(least, target_s * 1e3 / max(est, 1e-6))))
    loop_ms(fn, max(least, reps // 10))
    ms = [loop_ms(fn, reps) for _ in range(WINDOWS)]
    return float(np.median(ms)), ms, reps


def bench_sampler(man, lib):
    out = []
    opt = OnlineOptions().opts(seed=1, draw=0, lib=lib)
    st = torch.cuda.current_stream().cuda_stream
    J = man.shape[1]
    for P in (1 << 16, 1 << 20):
        q = torch.empty(P, J, 4, device=DEV)
        fn = lambda: engine.online_sample(man.data_ptr(), man.shape[0], 0, P, opt, q.data_ptr(), None, None, st, lib, J)      # noqa: E731
        med, ms, reps = windows(fn)
        nbytes = 32 * J * P
        out.append({"what": "pndf_online_sample alone" if J == 21 else "pndf_skel_online_sample alone", "num_joints": J, "P": P, "N": man.shape[0], "launch_us_median": 1e3 * med,
                    "launch_us_windows": [1e3 * m for m in ms], "launches_per_window": reps, "counted_bytes": nbytes,
                    "counted_bytes_per_s": nbytes / (med * 1e-3), "fraction_of_hbm_roof": nbytes / (med * 1e-3) / HBM_ROOF,
                    "hbm_roof_bytes_per_s": HBM_ROOF, "bound": "bytes (HBM); the gather's sector waste is not counted"})
        assert bool(torch.isfinite(q).all())
    return out


def bench_refresh(man):
    ds = OnlinePoseDataset.from_manifold([man.cpu().numpy()], POOL_FILES, POOL_ROWS, OnlineOptions(k=K, metric="geo"), device=DEV,
                                         num_joints=man.shape[1])
    draw = [0]

    def fn():
        ds.refresh(draw[0], 1)
        draw[0] += 1
    med, ms, reps = windows(fn, target_s=2.0, least=2, most=20)
    P = POOL_FILES * POOL_ROWS
    assert bool(torch.isfinite(ds.dist).all()) and bool((ds.nn_idx >= 0).all())
    return {"what": "OnlinePoseDataset.refresh: sampler + pndf_knn_search", "num_joints": ds.num_joints, "P": P, "N": man.shape[0], "k": K,
            "metric": "geo", "chunk": ds.chunk, "refresh_ms_median": med, "refresh_ms_windows": ms, "refreshes_per_window": reps,
            "pairs_per_s": P * man.shape[0] / (med * 1e-3), "resident_bytes": ds.nbytes}


def bench_step(steps, warmup, root):
    files = ITEMS * (warmup + steps)          # one epoch = the warm-up and one window (tools/bench_trainer.py's data set shape)
    rng = np.random.default_rng(0)
    pose = rng.standard_normal(size=(files, ROWS, 21, 4), dtype=np.float32)
    pose /= np.linalg.norm(pose, axis=3, keepdims=True)
    man = pose[:64].copy()
    dist = rng.uniform(0.0, 0.5, (files, ROWS, K)).astype(np.float32)
    ds = PoseDataset.from_arrays(list(pose), list(dist), list(man), device=DEV)
    cfg = amass_config("lrelu", DEV)
    cfg["train"].update(batch_size=ITEMS, optimizer_param=1e-5, continue_train=False, eikonal=1.0)
    cfg["data"] = {"flip": False, "num_pts": NUM_PTS}
    cfg["experiment"]["root_dir"] = root
    t = Trainer(cfg, seed=0, dataset=ds)
    t.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0, 2.0, 0.1).items()})
    ms = []
    for w in range(WINDOWS):
        t.begin_epoch(w)
        loop_ms(t.step, warmup)
        ms.append(loop_ms(t.step, steps))
        assert np.isfinite(t.read_log()).all()
    return {"what": "file-based Trainer.step(), lrelu, eikonal on", "B": t.B, "Bm": t.B, "step_ms_median": float(np.median(ms)),
            "step_ms_windows": ms, "steps_per_window": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "online", "bench.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--root", default=os.path.join(REPO, "build", "bench_online"), help="experiment directory of the trainer")
    ap.add_argument("--num_joints", type=int, default=21)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_online.py measures on the GPU"
    lib = engine.load_library()
    man = unit_poses(N_MAN, seed=2, J=a.num_joints)
    doc = {"device": torch.cuda.get_device_name(0), "library": lib.pndf_version().decode(), "sampler": bench_sampler(man, lib),
           "refresh": bench_refresh(man)}
    del man
    torch.cuda.empty_cache()
    if a.num_joints == 21:
        doc["step"] = bench_step(a.steps, a.warmup, a.root)
        steps_per_epoch = POOL_FILES // ITEMS
        doc["amortised"] = [{"refresh_every": r, "steps_per_pool": steps_per_epoch * r,
                             "refresh_ms_per_step": doc["refresh"]["refresh_ms_median"] / (steps_per_epoch * r),
                             "step_ms": doc["step"]["step_ms_median"],
                             "refresh_over_step": doc["refresh"]["refresh_ms_median"] / (steps_per_epoch * r) / doc["step"]["step_ms_median"]}
                            for r in (1, 10)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
