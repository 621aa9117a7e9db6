#!/usr/bin/env python3
"""One optimiser step of training, end to end, on configs/amass.yaml dims, 4 items x 5,000 poses (B = Bm = 20,000), eikonal on:

  arm A  the composition without posendf_amd.trainer: a device-resident data set indexed with torch (row indices drawn on the
         device), opt['engine']['train'] = 'hip' through autograd (zero_grad, model(...), the weighted sum, backward) and
         torch.optim.Adam(lr 1e-5, weight_decay 1e-4);
  arm B  posendf_amd.trainer.Trainer.step(): pndf_train_batch, pndf_train_forward, pndf_train_backward, pndf_adam_step.

Each run of an arm is ONE loop of --steps steps after --warmup, timed with HIP events around the whole loop; the arms alternate in
one process (A B A B), two runs each, so the A-to-A difference is the spread.  Requirement: B's median step time is not above
A's by more than that spread (exit status 1 otherwise); any gain is reported only.  For B the batch kernel and the optimiser
kernel are also timed alone (back to back, so their working sets stay in the Infinity Cache where they fit), with their bytes per
second against the HBM roof.  One JSON line per arm and activation, appended to --out.
usage: python tools/bench_trainer.py [--steps 100] [--warmup 10] [--acts lrelu softplus] [--out profiles/trainer/step.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from posendf_amd import PoseNDF, amass_config, engine, synth  # noqa: E402
from posendf_amd.trainer import PoseDataset, Trainer  # noqa: E402

DEV = "cuda:0"
HBM_ROOF = 6.3e12        # achievable bytes per second of an MI355X (8.0e12 on paper)
ITEMS, NUM_PTS, K, ROWS = 4, 5000, 5, 2000


def dataset(files):
    rng = np.random.default_rng(0)
    pose = synth.make_poses(files * ROWS, seed=1, signed=True).reshape(files, ROWS, 21, 4)
    man = synth.make_poses(64 * ROWS, seed=2, signed=True).reshape(64, ROWS, 21, 4)
    dist = rng.uniform(0.0, 0.5, (files, ROWS, K)).astype(np.float32)
    return PoseDataset.from_arrays(list(pose), list(dist), list(man), device=DEV)


def config(act, root):
    cfg = amass_config(act, DEV)
    cfg["train"].update(batch_size=ITEMS, optimizer_param=1e-5, continue_train=False, eikonal=1.0)
    cfg["data"] = {"flip": False, "num_pts": NUM_PTS}
    cfg["experiment"]["root_dir"] = root
    return cfg


def loop_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


class ArmA:
    def __init__(self, act, ds):
        cfg = amass_config(act, DEV)
        cfg["engine"] = {"train": "hip"}
        self.net = PoseNDF(cfg)
        self.net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0, 2.0, 0.1).items()})
        self.net.train()
        self.opt = torch.optim.Adam(self.net.parameters(), lr=1e-5, weight_decay=1e-4)
        self.ds, self.B = ds, ITEMS * NUM_PTS
        self.gen = torch.Generator(device=DEV).manual_seed(0)

    def step(self):
        ds = self.ds
        rows = torch.randint(0, ds.pose.shape[0], (self.B,), device=DEV, generator=self.gen)
        mrows = torch.randint(0, ds.man.shape[0], (self.B,), device=DEV, generator=self.gen)
        pose, gt, man = ds.pose[rows], ds.dist[rows].mean(1), ds.man[mrows]
        self.opt.zero_grad()
        _, ld = self.net(pose, gt, man, eikonal=1.0)
        loss = 0.0
        for k in ld.keys():
            loss += 1.0 * ld[k]
        loss.backward()
        self.opt.step()


def kernels_alone(t, reps=200):
    ds, st = t.dataset, torch.cuda.current_stream().cuda_stream
    batch = lambda: engine.train_batch(ds.pose.data_ptr(), ds.dist.data_ptr(), ds.man.data_ptr(), ds.file_off_t.data_ptr(),      # noqa: E731
                                       ds.man_off_t.data_ptr(), t._item_file.data_ptr(), t._item_man.data_ptr(), t._words.data_ptr(),
                                       ds.F, ds.Fm, ds.k, ITEMS, NUM_PTS, 0, t._q.data_ptr(), t._gt.data_ptr(), t._qm.data_ptr(), st, t.lib)
    m, v = torch.zeros_like(t.flat_m), torch.zeros_like(t.flat_v)
    p = t.flat_p.clone()      # copies: the trainer's own state is left alone
    adam = lambda: engine.adam_step(p.data_ptr(), t.flat_g.data_ptr(), m.data_ptr(), v.data_ptr(), t.n_flat, 1, 1e-5, 0.9, 0.999,      # noqa: E731
                                    1e-8, 1e-4, st, t.lib)
    out = {}
    for name, fn, nbytes in (("batch", batch, t.B * (2 * 2 * 336 + 4 * ds.k + 4 + 2 * 4)), ("adam", adam, 7 * 4 * t.n_flat)):
        loop_ms(fn, 20)
        ms = loop_ms(fn, reps)
        out[f"{name}_us"] = 1e3 * ms
        out[f"{name}_bytes"] = nbytes
        out[f"{name}_fraction_of_hbm_roof"] = nbytes / (ms * 1e-3) / HBM_ROOF
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--acts", nargs="+", default=["lrelu", "softplus"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trainer", "step.jsonl"))
    ap.add_argument("--root", default=os.path.join(REPO, "build", "bench_trainer"), help="experiment directory of arm B's trainer")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trainer.py measures on the GPU"
    assert a.steps >= 100, "a timing window needs at least 100 steps"
    runs = 2
    ds = dataset(ITEMS * (a.warmup + a.steps) * runs)          # one epoch serves both runs of arm B
    ok = True
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for act in a.acts:
        arm_a = ArmA(act, ds)
        t = Trainer(config(act, a.root), seed=0, dataset=ds)
        t.model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(0, 2.0, 0.1).items()})
        t.begin_epoch(0)
        ms = {"A": [], "B": []}
        for _ in range(runs):                                    # A B A B
            for name, fn in (("A", arm_a.step), ("B", t.step)):
                loop_ms(fn, a.warmup)
                ms[name].append(loop_ms(fn, a.steps))
        spread = abs(ms["A"][0] - ms["A"][1])
        med_a, med_b = float(np.median(ms["A"])), float(np.median(ms["B"]))
        met = med_b <= med_a + spread
        ok = ok and met
        log = t.read_log()
        assert np.isfinite(log).all()
        common = {"act": act, "B": t.B, "Bm": t.B, "eikonal": 1.0, "steps_per_run": a.steps, "warmup": a.warmup, "runs": runs}
        lines = [dict(common, arm="A", what="torch indexing + engine.train hip through autograd + torch.optim.Adam",
                      step_ms_runs=ms["A"], step_ms_median=med_a, a_to_a_spread_ms=spread),
                 dict(common, arm="B", what="Trainer.step()", step_ms_runs=ms["B"], step_ms_median=med_b,
                      b_over_a=med_b / med_a, requirement_met=bool(met), **kernels_alone(t))]
        with open(a.out, "a") as f:
            for ln in lines:
                print(json.dumps(ln), flush=True)
                f.write(json.dumps(ln) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
