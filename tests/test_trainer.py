"""posendf_amd.trainer without a GPU: the loader and the sampler, the cpu backend against the reference's training trajectories
(tests/golden/trainer_*.npz, tests/golden/make_golden_trainer.py) and the checkpoints.  Reads only fixtures and seeded synthetic
data (tests/trainer_fixtures.py).

Trajectory rule (the one tests/test_train_gpu.py::test_dropin_adam_loop uses): per parameter tensor
|mine - f64| <= 2 |f32 - f64| + 1e-9 with the reference's own fp32 and fp64 runs; per-step losses: relative error <=
max(1e-4, 4 x the reference's own fp32 error)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_fixtures as tf
import trainer_fixtures as trf
from conftest import REPO


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture()
def root(tmp_path, lib):
    trf.write_dirs(tmp_path)
    return tmp_path


def _trainer(root, seed=0, **kw):
    from posendf_amd.trainer import Trainer
    return Trainer(trf.config(root, **kw), seed=seed)


def _params(t):
    return {k: p.detach().cpu().numpy().copy() for k, p in t.model.named_parameters()}


def _same(a, b):
    assert a.keys() == b.keys()
    assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])][:5]


# ---- loader and sampler ----------------------------------------------------------------------------------------------------
def test_dataset_reads_what_traindata_writes(root):
    from posendf_amd.trainer import PoseDataset
    ds = PoseDataset(os.path.join(root, "data"), os.path.join(root, "manifold"))
    rows = [n for r in trf.DATA_ROWS.values() for n in r]
    mrows = [n for r in trf.MAN_ROWS.values() for n in r]
    assert ds.F == len(rows) and ds.Fm == len(mrows) and ds.k == trf.K
    assert list(np.diff(ds.file_off)) == rows and list(np.diff(ds.man_off)) == mrows
    assert ds.pose.shape == (sum(rows), 21, 4) and ds.dist.shape == (sum(rows), trf.K) and ds.man.shape == (sum(mrows), 21, 4)
    data, man = trf.arrays()
    assert np.array_equal(ds.pose[:700].numpy(), data["setA"][0][0]) and np.array_equal(ds.man[-77:].numpy(), man["setB"][1])
    only = PoseDataset(os.path.join(root, "data"), os.path.join(root, "manifold"), datasets=["setB"])
    assert only.F == len(trf.DATA_ROWS["setB"]) and only.Fm == len(trf.MAN_ROWS["setB"])
    assert ds.nbytes == 4 * (sum(rows) * (84 + trf.K) + sum(mrows) * 84) + 8 * (ds.F + ds.Fm + 2)


def test_batch_rows(root):
    t = _trainer(root)
    ds = t.dataset
    assert t.steps_per_epoch == ds.F // trf.BATCH_SIZE == 4
    seen = []
    for step in range(t.steps_per_epoch):
        rows, man_rows = t.batch_rows(3, step)
        assert rows.dtype == np.int64 and rows.shape == man_rows.shape == (trf.BATCH_SIZE * trf.NUM_PTS,)
        for item in range(trf.BATCH_SIZE):
            r = rows[item * trf.NUM_PTS:(item + 1) * trf.NUM_PTS]
            f = np.searchsorted(ds.file_off, r[0], side="right") - 1
            assert (r >= ds.file_off[f]).all() and (r < ds.file_off[f + 1]).all()      # inside ONE file
            seen.append(int(f))
            m = man_rows[item * trf.NUM_PTS:(item + 1) * trf.NUM_PTS]
            fm = np.searchsorted(ds.man_off, m[0], side="right") - 1
            assert (m >= ds.man_off[fm]).all() and (m < ds.man_off[fm + 1]).all()
    assert len(set(seen)) == len(seen) == t.steps_per_epoch * trf.BATCH_SIZE           # every file at most once per epoch
    with pytest.raises(IndexError):
        t.batch_rows(0, t.steps_per_epoch)
    # a pure function of (seed, epoch, step)
    again = _trainer(root)
    for e, s in ((0, 0), (3, 2), (0, 0), (7, 3)):
        a, b = t.batch_rows(e, s), again.batch_rows(e, s)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(t.batch_rows(0, 0)[0], t.batch_rows(1, 0)[0])
    assert not np.array_equal(t.batch_rows(0, 0)[0], _trainer(root, seed=1).batch_rows(0, 0)[0])
    # the epochs permute the files: over a few epochs the dropped file changes
    assert len({tuple(sorted(set(np.searchsorted(ds.file_off, np.concatenate([t.batch_rows(e, s)[0] for s in range(4)]), side="right"))))
                for e in range(8)}) > 1


def test_batch_matches_numpy(root):
    for flip in (False, True):
        t = _trainer(root, flip=flip)
        rows, man_rows = t.batch_rows(1, 2)
        pose, gt, man = t.batch(1, 2)
        ds = t.dataset
        p, m = ds.pose.numpy()[rows], ds.man.numpy()[man_rows]
        if flip:
            p, m = np.where(p[..., :1] < 0, -p, p), np.where(m[..., :1] < 0, -m, m)
            assert (pose[..., 0] >= 0).all() and (man[..., 0] >= 0).all() and (ds.pose[rows][..., 0] < 0).any()
        assert np.array_equal(pose.numpy(), p) and np.array_equal(man.numpy(), m)
        u = trf.K * 2.0 ** -24
        mean = ds.dist.numpy()[rows].astype(np.float64).mean(1)
        assert (np.abs(gt.numpy() - mean) <= u / (1 - u) * mean).all()


@pytest.mark.parametrize("what", ["ragged_k", "empty", "pose_shape", "dist_rows", "no_dist"])
def test_bad_files_are_refused_by_name(root, what):
    from posendf_amd.trainer import PoseDataset
    from posendf_amd import synth
    bad = os.path.join(root, "data", "setB", "zz_bad.npz")
    pose, dist = synth.make_poses(10, seed=1), np.zeros((10, trf.K), np.float32)
    if what == "ragged_k":
        np.savez(bad, pose=pose, dist=np.zeros((10, trf.K + 1), np.float32))
    elif what == "empty":
        np.savez(bad, pose=pose[:0], dist=dist[:0])
    elif what == "pose_shape":
        np.savez(bad, pose=pose.reshape(10, 84), dist=dist)
    elif what == "dist_rows":
        np.savez(bad, pose=pose, dist=dist[:9])
    else:
        np.savez(bad, pose=pose)
    with pytest.raises(ValueError, match="zz_bad.npz"):
        PoseDataset(os.path.join(root, "data"), os.path.join(root, "manifold"))
    os.remove(bad)
    badm = os.path.join(root, "manifold", "setA", "zz_badman.npz")
    np.savez(badm, pose=pose[:0] if what == "empty" else pose.reshape(10, 84))
    with pytest.raises(ValueError, match="zz_badman.npz"):
        PoseDataset(os.path.join(root, "data"), os.path.join(root, "manifold"))


def test_too_few_files_for_a_step(root):
    with pytest.raises(ValueError, match="batch_size"):
        _trainer(root, batch_size=10)


def test_experiment_directory_uses_the_reference_formula(root):
    t = _trainer(root)
    assert t.exp_name == "main_lrelu_l1_1e-05_dist1.0_eik1.0"
    assert os.path.isdir(os.path.join(root, "exp", t.exp_name, "checkpoints"))
    assert _trainer(root, flip=True, act="softplus", eikonal=0.0).exp_name == "flip_main_softplus_l1_1e-05_dist1.0_eik0.0"


# ---- the reference's trajectories ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(trf.CASES))
def test_reference_trajectory_cpu(root, name):
    t, losses = trf.run_case(root, name, "cpu")
    trf.check_case(name, t, losses)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
SMALL = dict(num_pts=32)      # the checkpoint tests compare bits, not accuracy: small batches keep them quick


def test_resume_is_bit_identical(tmp_path, lib):
    a, b = tmp_path / "a", tmp_path / "b"
    trf.write_dirs(a)
    trf.write_dirs(b)
    straight = _trainer(a, **SMALL)
    r0 = straight.train_model(0)
    r1 = straight.train_model(1)
    first = _trainer(b, **SMALL)
    assert first.train_model(0) == r0
    del first
    resumed = _trainer(b, continue_train=True, **SMALL)
    assert resumed.ep == 1 and resumed.iter_nums == straight.steps_per_epoch
    assert resumed.train_model(resumed.ep) == r1
    _same(_params(straight), _params(resumed))
    ma, mb = trf.adam_state(straight), trf.adam_state(resumed)
    assert all(np.array_equal(ma[k][0], mb[k][0]) and np.array_equal(ma[k][1], mb[k][1]) for k in ma)
    assert np.isfinite(r1[0]) and np.isfinite(r1[1])
    # without continue_train a new trainer starts over, with it and no checkpoint too
    assert _trainer(b, **SMALL).ep == 0
    c = tmp_path / "c"
    trf.write_dirs(c)
    assert _trainer(c, continue_train=True, **SMALL).ep == 0


def _stock(root, trainer_like, sd=None):
    """a stock PoseNDF + torch.optim.Adam as the reference's trainer builds them (train_posendf.py:29-30)"""
    from posendf_amd import PoseNDF
    net = PoseNDF(trf.config(root, **SMALL))
    if sd is not None:
        net.load_state_dict(sd)
    return net, torch.optim.Adam(net.parameters(), lr=trf.LR, weight_decay=1e-4)


def _stock_epoch(net, opt, sampler, ep):
    for s in range(sampler.steps_per_epoch):
        pose, gt, man = sampler.batch(ep, s)
        opt.zero_grad()
        _, ld = net(pose, gt, man, eikonal=1.0)
        loss = 0.0
        for k in ld.keys():
            loss += 1.0 * ld[k]
        loss.backward()
        opt.step()


def test_checkpoint_loads_into_a_stock_loop_and_continues_identically(root):
    t = _trainer(root, **SMALL)
    t.train_model(0)
    path = os.path.join(t.checkpoint_path, "checkpoint_epoch_best.tar")
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict"} and ck["epoch"] == 0
    with open(path, "rb") as f:
        assert f.read(2) != b"PK"                                   # the legacy serialisation, not a zip archive
    net, opt = _stock(root, t, ck["model_state_dict"])
    opt.load_state_dict(ck["optimizer_state_dict"])
    _stock_epoch(net, opt, t, 1)
    t.train_model(1)
    _same(_params(t), {k: p.detach().numpy() for k, p in net.named_parameters()})


@pytest.mark.parametrize("step_as_number", [False, True])
def test_stock_checkpoint_resumes_in_the_trainer(root, step_as_number):
    sampler = _trainer(root, **SMALL)
    net, opt = _stock(root, sampler, sampler.model.state_dict())
    _stock_epoch(net, opt, sampler, 0)
    osd = opt.state_dict()
    if step_as_number:                                              # checkpoints of older torch versions hold plain ints
        osd = {"state": {i: dict(s, step=int(s["step"])) for i, s in osd["state"].items()}, "param_groups": osd["param_groups"]}
    torch.save({"epoch": 0, "model_state_dict": net.state_dict(), "optimizer_state_dict": osd},
               os.path.join(sampler.checkpoint_path, "checkpoint_epoch_best.tar"), _use_new_zipfile_serialization=False)
    resumed = _trainer(root, continue_train=True, **SMALL)
    assert resumed.ep == 1 and resumed.iter_nums == sampler.steps_per_epoch
    resumed.train_model(1)
    _stock_epoch(net, opt, sampler, 1)
    _same(_params(resumed), {k: p.detach().numpy() for k, p in net.named_parameters()})


def test_best_previous_rotation_and_summary(root):
    t = _trainer(root, **SMALL)
    best = os.path.join(t.checkpoint_path, "checkpoint_epoch_best.tar")
    prev = os.path.join(t.checkpoint_path, "checkpoint_epoch_previous.tar")
    t.train_model(0)
    assert os.path.exists(best) and not os.path.exists(prev)
    t.train_model(1)
    t.train_model(2)
    assert torch.load(best, map_location="cpu")["epoch"] == 2 and torch.load(prev, map_location="cpu")["epoch"] == 1
    lines = [json.loads(ln) for ln in open(os.path.join(t.exp_path, "summary.jsonl"))]
    assert [ln["epoch"] for ln in lines] == [0, 1, 2] and [ln["iter"] for ln in lines] == [4, 8, 12]
    assert set(lines[0]) == {"epoch", "iter", "train/loss_dist", "train/loss_man_loss", "train/loss_eikonal", "train/epoch"}
    assert all(np.isfinite(v) for ln in lines for v in ln.values())
    noeik = _trainer(root, eikonal=0.0, **SMALL)
    last, mean = noeik.train_model(0)
    line = json.loads(open(os.path.join(noeik.exp_path, "summary.jsonl")).readlines()[-1])
    assert set(line) == {"epoch", "iter", "train/loss_dist", "train/epoch"} and abs(line["train/loss_dist"] - last) < 1e-7


def test_cli_runs_two_epochs_on_cpu(root):
    import yaml
    cfg = trf.config(root, continue_train=True, max_epoch=5, **SMALL)
    path = os.path.join(root, "cfg.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "posendf_amd.trainer", "--config", path, "--max_epoch", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(root))
    assert r.returncode == 0, r.stderr
    exp = os.path.join(root, "exp", "main_lrelu_l1_1e-05_dist1.0_eik1.0")
    assert os.path.exists(os.path.join(exp, "config.yaml"))
    assert torch.load(os.path.join(exp, "checkpoints", "checkpoint_epoch_best.tar"), map_location="cpu")["epoch"] == 1
    assert os.path.exists(os.path.join(exp, "checkpoints", "checkpoint_epoch_previous.tar"))
    assert len(open(os.path.join(exp, "summary.jsonl")).readlines()) == 2
    # a second invocation resumes: nothing is left below max_epoch 2, one more epoch below 3
    assert subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(root)).returncode == 0
    assert len(open(os.path.join(exp, "summary.jsonl")).readlines()) == 2
    r = subprocess.run(cmd[:-1] + ["3"], capture_output=True, text=True, env=env, cwd=str(root))
    assert r.returncode == 0, r.stderr
    assert [json.loads(ln)["epoch"] for ln in open(os.path.join(exp, "summary.jsonl"))] == [0, 1, 2]

