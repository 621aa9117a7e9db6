#!/usr/bin/env python3
"""Fixtures of the training trajectory (model/train_posendf.py:87-110), produced with the REAL reference (dev container only).

For every case of tests/trainer_fixtures.py -- lrelu for 10 steps, softplus for 20, one case with `data.flip`, one with
`train.eikonal: 0`; configs/amass.yaml dims, the `live` synthetic weights, B = Bm = 512 -- the imported reference `PoseNDF` runs the
six statements of train_posendf.py:93-99 (zero_grad, model(...), the weighted sum, backward, optimizer.step) with
torch.optim.Adam(lr=1e-5, weight_decay=1e-4) (train_posendf.py:30), in fp32 and in fp64, on the batches that
`posendf_amd.trainer.Trainer.batch_rows` names in the synthetic directory of trainer_fixtures (rebuilt here with numpy: rows,
the labels' mean, the flip of both batches).  Stored: the per-step losses (NaN where the reference returns no such key), the
final parameters (the large weights through train_fixtures.digest) and both Adam moments (the large weights as Frobenius norm
and 1,024 seeded entries).

Nothing of the reference is copied: only outputs (data).  One thread, so that a rerun gives bit-equal arrays.
Usage:  python tests/golden/make_golden_trainer.py [case ...]      (writes tests/golden/trainer_<case>.npz)
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import train_fixtures as tf             # noqa: E402
import trainer_fixtures as trf          # noqa: E402
from make_golden_train import _import_reference, ref_config      # noqa: E402


def numpy_batch(ds, rows, man_rows, flip):
    """load_data.py:49-61 on the concatenated data set, with the flip on both batches"""
    pose, dist, man = ds.pose.numpy()[rows], ds.dist.numpy()[rows], ds.man.numpy()[man_rows]
    if flip:
        pose = np.where(pose[..., :1] < 0, -pose, pose)
        man = np.where(man[..., :1] < 0, -man, man)
    return pose, dist.astype(np.float64).mean(1), man


def make(name):
    from posendf_amd.trainer import Trainer
    act, steps, flip, eikonal = trf.CASES[name]
    sd, hidden = tf.case_weights("live")
    _, PoseNDF = _import_reference()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {"act": np.array(act), "steps": np.array(steps), "flip": np.array(flip), "eikonal": np.array(eikonal),
           "torch_version": np.array(torch.__version__)}
    try:
        with tempfile.TemporaryDirectory() as root:
            trf.write_dirs(root)
            sampler = Trainer(trf.config(root, act, "cpu", flip, eikonal), seed=0)
            per = sampler.steps_per_epoch
            batches = [numpy_batch(sampler.dataset, *sampler.batch_rows(s // per, s % per), flip) for s in range(steps)]
        weight = {"dist": 1.0, "man_loss": 1.0, "eikonal": eikonal}
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            net = PoseNDF(ref_config(act, hidden, "l1")).to(dtype)
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()})
            opt = torch.optim.Adam(net.parameters(), lr=trf.LR, weight_decay=1e-4)          # train_posendf.py:30
            net.train()
            losses = np.full((steps, 3), np.nan)
            for s, (q, gt, qm) in enumerate(batches):
                t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
                opt.zero_grad()                                               # train_posendf.py:93-99
                _, ld = net(t(q), t(gt), t(qm), eikonal=eikonal)
                loss = 0.0
                for k in ld.keys():
                    loss += weight[k] * ld[k]
                loss.backward()
                opt.step()
                for c, k in enumerate(tf.LOSS_KEYS):
                    if k in ld:
                        losses[s, c] = float(ld[k].detach())
            out[f"losses_{tag}"] = losses
            for k, p in net.named_parameters():
                st = opt.state[p]
                for pre, x, full in (("p", p, True), ("m", st["exp_avg"], False), ("v", st["exp_avg_sq"], False)):
                    for part, v in trf.state_digest(k, x.detach().numpy(), hidden, full).items():
                        out[f"{tag}::{pre}::{k}" + (f"::{part}" if part else "")] = np.asarray(v)
    finally:
        torch.set_num_threads(threads)
    return out


if __name__ == "__main__":
    for name in (sys.argv[1:] or trf.CASES):
        res = make(name)
        path = trf.fixture_path(name)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path) // 1024, "KiB", "last losses f64", res["losses_f64"][-1])
