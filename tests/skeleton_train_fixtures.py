"""Test helper (not a test module) for training other skeletons (include/posendf_amd_skeleton_train.h): shared by
tests/golden/make_golden_skeleton_train.py, tests/test_skeleton_train.py and tests/test_skeleton_train_gpu.py.

The tables and synthetic networks are tests/skeleton_oracle.py's, the ragged batch (B = 509, Bm = 383: four full 192-pose encoder
workgroups and one of 124 columns), the step structure and the loss keys tests/train_fixtures.py's, the tolerance rule
tests/test_train_gpu.py's.  The oracle is the model's own stock train=True path in float64: the reference's statement with J in place
of 21, pinned against the reference's own classes by the fixtures tests/golden/skeleton_train_<skeleton>_<act>.npz."""
from __future__ import annotations

import os

import numpy as np

import skeleton_oracle as sko
import train_fixtures as tf

B, BM = tf.B, tf.BM
LOSS_KEYS = tf.LOSS_KEYS
HIDDEN = sko.HIDDEN
SKELETONS = sko.SKELETONS
FIXTURE_CASES = sko.FIXTURE_CASES      # (hand | tree32) x (lrelu | softplus)


def fixture_path(skel, act):
    return os.path.join(sko.GOLDEN, f"skeleton_train_{skel}_{act}.npz")


def inputs(parents, b=B, bm=BM, seed=71):
    """noisy poses [b,J,4], labels [b], manifold poses [bm,J,4] (float32); for one joint signed poses -- normalising over a joint axis
    of length one leaves the signs only (skeleton_oracle.case_poses)"""
    from posendf_amd import synth
    J = len(parents)
    q = synth.make_poses(b, seed=seed, signed=J == 1, num_joints=J)
    qm = synth.make_poses(bm, seed=seed + 1, signed=J == 1, num_joints=J)
    gt = np.random.default_rng(seed + 2).uniform(0.0, 0.5, b).astype(np.float32)
    return q, gt, qm


def pick_seed(parents, act, q, hidden=HIDDEN, first=0):
    """The first weight seed from `first` on that leaves at most a quarter of the noisy poses clipped in the fp64 oracle and gives
    them more than one distance (the rule of tests/golden/make_golden_skeleton.py): a network clipped to zero trains on nothing"""
    for seed in range(first, first + 64):
        sd = sko.network(parents, seed, hidden=hidden)
        d = sko.forward(q, sd, act, parents, np.float64).reshape(-1)
        if sko.clipped(d, act.split("/")[0].split("@")[0]) * 4 <= len(q) and float(np.median(d)) > float(d.min()):
            return seed, sd
    raise AssertionError(f"no seed keeps {len(parents)} joints {act} off d == 0")


_NETS = {}


def case_network(skel, act, hidden=HIDDEN):
    """(parents, weights) of a case: the fixture's seed for a fixture case; elsewhere pick_seed from 7 on"""
    key = (skel, act, tuple(hidden))
    if key not in _NETS:
        parents = SKELETONS[skel]
        if (skel, act) in FIXTURE_CASES and tuple(hidden) == tuple(HIDDEN):
            sd = sko.network(parents, int(np.load(fixture_path(skel, act))["seed"]))
        else:
            _, sd = pick_seed(parents, act, inputs(parents)[0], hidden, first=7)
        _NETS[key] = (parents, sd)
    return _NETS[key]


def config(parents, act, hidden, loss="l1", device="cpu", train_backend="torch", enc_act=None, beta=None, enc_beta=None):
    """configs/amass.yaml with the skeleton `parents`: train_fixtures.config for a parent table"""
    from posendf_amd import skeleton_config
    trunk, tbeta, eact, ebeta = tf.sides(act, enc_act, beta, enc_beta)
    cfg = skeleton_config(list(parents), trunk, device, hidden=hidden)
    cfg["model"]["DFNet"]["beta"] = tbeta
    cfg["model"]["StrEnc"]["act"] = eact
    cfg["model"]["StrEnc"]["beta"] = ebeta
    cfg["train"]["loss_type"] = loss
    cfg["engine"] = {"train": train_backend}
    return cfg


def model(parents, act, sd, hidden=HIDDEN, loss="l1", backend="torch", dtype=None, device="cpu", **kw):
    import torch
    from posendf_amd import SkeletonPoseNDF
    dtype = torch.float32 if dtype is None else dtype
    net = SkeletonPoseNDF(config(parents, act, hidden, loss, device, train_backend=backend, **kw)).to(dtype)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()})
    return net


def run(net, q, gt, qm, eikonal, dtype=None, device="cpu"):
    """train_fixtures.run_objective on numpy inputs: (losses, grads, loss_dict)"""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    t = lambda a: torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype)      # noqa: E731
    return tf.run_objective(net, t(q), t(gt), t(qm), eikonal)


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor, 1e-30))


def gate(what, mine, ref32, ref64, failures, floor=0.0):
    """The rule of tests/test_train_gpu.py: relative error in the tensor norm <= max(1e-4, 4 x the stock fp32 run's error against the
    stock fp64 run); `floor`: the least norm of the denominator, for gradients whose terms cancel"""
    tol = max(1e-4, 4.0 * rel(ref32, ref64))
    err = rel(mine, ref64, floor)
    if not err <= tol:
        failures.append((what, err, tol))
    return err


def check(tag, mine, ref32, ref64, gradients=True):
    """every loss and (with `gradients`) every gradient tensor of `mine` = (losses, grads) under the rule; the absolute floor is 1e-3 x
    the largest gradient norm of the fp64 run"""
    (l_h, g_h), (l_32, g_32), (l_64, g_64) = mine, ref32, ref64
    assert set(l_h) == set(l_64), (tag, set(l_h), set(l_64))
    failures, worst = [], 0.0
    for k in l_64:
        print(f"[skeleton train {tag}] loss {k}: hip {l_h[k]!r} f32 {l_32[k]!r} f64 {l_64[k]!r}")
        worst = max(worst, gate(f"{tag} loss {k}", l_h[k], l_32[k], l_64[k], failures))
    if gradients:
        floor = 1e-3 * max(np.linalg.norm(g) for g in g_64.values())
        assert set(g_h) == set(g_64)
        for k in g_64:
            worst = max(worst, gate(f"{tag} grad {k}", g_h[k], g_32[k], g_64[k], failures, floor))
    print(f"[skeleton train {tag}] worst relative error {worst:.2e}")
    assert not failures, failures[:8]


# ---- the trainer on the 15-joint hand: a small synthetic training directory held in arrays
K = 5
LR = 1e-5


def hand_arrays(files, rows, man_files=3, seed=4000):
    """(poses, dists, mans): `files` data files of `rows` signed hand poses with k = 5 labels, `man_files` manifold files"""
    from posendf_amd import synth
    J = len(sko.HAND)
    poses = [synth.make_poses(rows + 7 * i, seed=seed + i, signed=True, num_joints=J) for i in range(files)]
    dists = [np.random.default_rng(seed + 100 + i).uniform(0.0, 0.5, (len(p), K)).astype(np.float32) for i, p in enumerate(poses)]
    mans = [synth.make_poses(rows + 11 * i, seed=seed + 200 + i, signed=True, num_joints=J) for i in range(man_files)]
    return poses, dists, mans


def trainer_config(root, act="lrelu", device="cpu", hidden=HIDDEN, batch_size=3, num_pts=16, continue_train=False, eikonal=1.0,
                   parents="hand"):
    from posendf_amd import skeleton_config
    cfg = skeleton_config(parents, act, device, hidden=hidden)
    cfg["data"] = {"data_dir": None, "amass_dir": None, "flip": False, "num_pts": num_pts}
    cfg["experiment"]["root_dir"] = os.path.join(str(root), "exp")
    cfg["train"].update(batch_size=batch_size, optimizer_param=LR, continue_train=continue_train, max_epoch=2, eikonal=eikonal)
    return cfg


def hand_trainer(root, files, rows, seed=0, **kw):
    from posendf_amd.trainer import PoseDataset, Trainer
    device = kw.get("device", "cpu")
    ds = PoseDataset.from_arrays(*hand_arrays(files, rows), device=device, num_joints=len(sko.HAND))
    return Trainer(trainer_config(root, **kw), seed=seed, dataset=ds)


def stock_loop(t, cfg, sd, steps, dtype, device):
    """train_posendf.py:93-99 with a stock SkeletonPoseNDF + torch.optim.Adam(lr, weight_decay 1e-4) on the batches of trainer `t`:
    (params, losses [steps, 3])"""
    import torch
    from posendf_amd import SkeletonPoseNDF
    cfg = dict(cfg, engine={"train": "torch"})
    net = SkeletonPoseNDF(cfg).to(dtype)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()})
    opt = torch.optim.Adam(net.parameters(), lr=LR, weight_decay=1e-4)
    losses = np.zeros((steps, 3))
    for s in range(steps):
        pose, gt, man = t.batch(s // t.steps_per_epoch, s % t.steps_per_epoch)
        opt.zero_grad()
        _, ld = net(pose.to(dtype), gt.to(dtype), man.to(dtype), train=True, eikonal=1.0)
        loss = 0.0
        for k in ld.keys():
            loss += 1.0 * ld[k]
        loss.backward()
        opt.step()
        losses[s] = [float(ld[k].detach()) for k in LOSS_KEYS]
    return {k: p.detach().double().cpu().numpy() for k, p in net.named_parameters()}, losses
