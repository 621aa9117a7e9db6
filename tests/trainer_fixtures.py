"""Shared by tests/golden/make_golden_trainer.py, tests/test_trainer.py and tests/test_trainer_gpu.py: a small synthetic training
directory written from seeds (what posendf_amd.traindata.generate leaves behind: <data>/<dataset>/*.npz with `pose`, `dist`;
<manifold>/<dataset>/*.npz with `pose`), the trainer configs of the golden trajectories and the trajectory rule."""
from __future__ import annotations

import os

import numpy as np

import train_fixtures as tf

K = 5
# rows per data file / manifold file of each "dataset": unequal on purpose
DATA_ROWS = {"setA": (700, 333, 1024, 90, 1500), "setB": (512, 257, 64, 801)}
MAN_ROWS = {"setA": (400, 150, 90), "setB": (1000, 77)}
# name: (activation, steps, data.flip, train.eikonal) -- configs/amass.yaml dims, B = Bm = 512 (batch_size 2 x num_pts 256),
# Adam(lr 1e-5, weight_decay 1e-4), `live` synthetic weights
CASES = {
    "lrelu": ("lrelu", 10, False, 1.0),
    "softplus": ("softplus", 20, False, 1.0),
    "lrelu_flip": ("lrelu", 10, True, 1.0),
    "lrelu_noeik": ("lrelu", 10, False, 0.0),
}
BATCH_SIZE, NUM_PTS, LR = 2, 256, 1e-5


def fixture_path(name):
    return os.path.join(tf.GOLDEN, f"trainer_{name}.npz")


def arrays(signed=True, k=K, data_rows=None, man_rows=None):
    """({dataset: [(pose, dist), ...]}, {dataset: [pose, ...]}) from seeds: poses from synth.make_poses (signed, so that the
    flip has work to do), labels uniform in [0, 0.5)"""
    from posendf_amd import synth
    data, man = {}, {}
    seed = 1000
    for ds, rows in (data_rows or DATA_ROWS).items():
        data[ds] = []
        for n in rows:
            seed += 1
            data[ds].append((synth.make_poses(n, seed=seed, signed=signed),
                             np.random.default_rng(seed + 5000).uniform(0.0, 0.5, (n, k)).astype(np.float32)))
    for ds, rows in (man_rows or MAN_ROWS).items():
        man[ds] = []
        for n in rows:
            seed += 1
            man[ds].append(synth.make_poses(n, seed=seed, signed=signed))
    return data, man


def write_dirs(root, **kw):
    """writes <root>/data and <root>/manifold; returns (data_dir, amass_dir)"""
    data, man = arrays(**kw)
    data_dir, amass_dir = os.path.join(str(root), "data"), os.path.join(str(root), "manifold")
    for ds, files in data.items():
        os.makedirs(os.path.join(data_dir, ds), exist_ok=True)
        for i, (p, d) in enumerate(files):
            np.savez(os.path.join(data_dir, ds, f"seq{i:03d}.npz"), pose=p, dist=d)
    for ds, files in man.items():
        os.makedirs(os.path.join(amass_dir, ds), exist_ok=True)
        for i, p in enumerate(files):
            np.savez(os.path.join(amass_dir, ds, f"man{i:03d}.npz"), pose=p)
    return data_dir, amass_dir


def config(root, act="lrelu", device="cpu", flip=False, eikonal=1.0, batch_size=BATCH_SIZE, num_pts=NUM_PTS, lr=LR,
           continue_train=False, max_epoch=2, dirs=None):
    from posendf_amd import amass_config
    data_dir, amass_dir = dirs or (os.path.join(str(root), "data"), os.path.join(str(root), "manifold"))
    cfg = amass_config(act, device)
    cfg["data"] = {"data_dir": data_dir, "amass_dir": amass_dir, "flip": flip, "num_pts": num_pts}
    cfg["experiment"]["root_dir"] = os.path.join(str(root), "exp")
    cfg["train"].update(batch_size=batch_size, optimizer_param=lr, continue_train=continue_train, max_epoch=max_epoch,
                        eikonal=eikonal)
    return cfg


def load_live(trainer):
    """the `live` synthetic weights (train_fixtures) into a trainer's model, in place"""
    import torch
    sd, _ = tf.case_weights("live")
    trainer.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def state_digest(key, x, hidden, full=True):
    """train_fixtures.digest for parameters (full=True); for the Adam moments the large weights keep `fro` and `vals` only"""
    d = tf.digest(key, x, hidden)
    if not full and "" not in d:
        d = {"fro": d["fro"], "vals": d["vals"]}
    return d


def torch_adam(p, g, m, v, step, dtype, lr, wd, device):
    """ONE step of torch.optim.Adam on `device` in `dtype` from the numpy buffers p, g, m, v (m, v: the state a loop would hold
    before step `step`; ignored at step 1): [p, exp_avg, exp_avg_sq] as fp64 numpy arrays.  The yardstick of both optimiser
    kernels (tests/test_trainer_gpu.py, tests/test_denoise_update_gpu.py)."""
    import torch
    P = torch.from_numpy(p).to(device, dtype).requires_grad_(True)
    opt = torch.optim.Adam([P], lr=lr, weight_decay=wd)
    if step > 1:
        opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m).to(device, dtype),
                        "exp_avg_sq": torch.from_numpy(v).to(device, dtype)}
    P.grad = torch.from_numpy(g).to(device, dtype)
    opt.step()
    st = opt.state[P]
    assert float(st["step"]) == step
    return [x.detach().double().cpu().numpy() for x in (P, st["exp_avg"], st["exp_avg_sq"])]


def adam_state(trainer):
    """{state-dict key: (exp_avg, exp_avg_sq)} as numpy arrays, from optimizer_state_dict()"""
    st = trainer.optimizer_state_dict()["state"]
    return {k: (st[i]["exp_avg"].detach().cpu().numpy(), st[i]["exp_avg_sq"].detach().cpu().numpy())
            for i, (k, _) in enumerate(trainer.model.named_parameters())}


def check_trajectory(z, params, moments, hidden, what):
    """The trajectory rule: per parameter tensor (per digest part of the large ones) |mine - f64| <= 2 |f32 - f64| + 1e-9, the
    same for both Adam moments.  `z`: the golden file; params {key: array}; moments from adam_state().
    The Frobenius norm of a large tensor is ONE number, and the error of one number against its own fp32 run is luck (the
    fp32 run's may cancel to nothing), so it gets the envelope of the tensor it stands for: |d fro| <= |d W| (Cauchy-Schwarz),
    and |f32 - f64| over the whole tensor is estimated from the digest's 1,024 seeded entries as sqrt(numel / 1024) times
    theirs."""
    from posendf_amd import synth
    numel = {k: int(np.prod(s)) for k, s in synth.state_dict_shapes((126, *hidden, 1)).items()}
    bad = []
    for k, p in params.items():
        sets = [("p", state_digest(k, p, hidden))]
        if moments is not None:
            sets += [("m", state_digest(k, moments[k][0], hidden, False)), ("v", state_digest(k, moments[k][1], hidden, False))]
        for tag, dig in sets:
            for part, v in dig.items():
                name = f"{tag}::{k}" + (f"::{part}" if part else "")
                f32, f64 = z[f"f32::{name}"].astype(np.float64), z[f"f64::{name}"].astype(np.float64)
                mine = np.linalg.norm(np.asarray(v, np.float64) - f64)
                env = np.linalg.norm(f32 - f64)
                if part == "fro":
                    vals = f"{tag}::{k}::vals"
                    n_vals = z[f"f64::{vals}"].size
                    env = np.sqrt(numel[k] / n_vals) * np.linalg.norm(z[f"f32::{vals}"].astype(np.float64) - z[f"f64::{vals}"])
                if not mine <= 2.0 * env + 1e-9:
                    bad.append((name, float(mine), float(env)))
    assert not bad, (what, len(bad), bad[:8])


def loss_tolerance(l32, l64):
    """the per-loss rule of tests/test_train_gpu.py: relative error <= max(1e-4, 4 x the reference's own fp32 error)"""
    return max(1e-4, 4.0 * abs(float(l32) - float(l64)) / max(abs(float(l64)), 1e-30))


def trainer(root, seed=0, **kw):
    from posendf_amd.trainer import Trainer
    return Trainer(config(root, **kw), seed=seed)


def params(t):
    return {k: p.detach().cpu().numpy().copy() for k, p in t.model.named_parameters()}


def run_case(root, name, device):
    """the trainer on a golden case: (trainer, per-step losses [steps, 3])"""
    act, steps, flip, eikonal = CASES[name]
    t = trainer(root, act=act, device=device, flip=flip, eikonal=eikonal)
    load_live(t)
    logs = []
    for s in range(steps):
        if s % t.steps_per_epoch == 0:
            if s:
                logs.append(t.read_log())
            t.begin_epoch(s // t.steps_per_epoch)
        t.step()
    logs.append(t.read_log()[:(steps - 1) % t.steps_per_epoch + 1])
    return t, np.concatenate(logs)


def check_case(name, t, losses):
    z = np.load(fixture_path(name))
    _, hidden = tf.case_weights("live")
    bad = []
    for s in range(len(losses)):
        for c, k in enumerate(tf.LOSS_KEYS):
            l32, l64 = z["losses_f32"][s, c], z["losses_f64"][s, c]
            if np.isnan(l64):
                continue
            err = abs(float(losses[s, c]) - l64) / abs(l64)
            if not err <= loss_tolerance(l32, l64):
                bad.append((s, k, err, loss_tolerance(l32, l64)))
    assert not bad, bad[:8]
    assert t.iter_nums == int(z["steps"])
    check_trajectory(z, params(t), adam_state(t), hidden, name)
