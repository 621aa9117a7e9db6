"""Training PoseNDF end to end: the counterpart of the reference's `python trainer.py --config=...` (trainer.py:11-25,
model/train_posendf.py:15-176 `PoseNDF_trainer`, model/load_data.py:18-86 `PoseData`).

    python -m posendf_amd.trainer --config cfg.yaml [--max_epoch N]

reads what `posendf_amd.traindata.generate` writes (`data.data_dir`: <dataset>/*.npz with `pose` [n,21,4] and `dist` [n,k];
`data.amass_dir`: <dataset>/*.npz with `pose`), trains `PoseNDF(opt)` with Adam(lr = train.optimizer_param, weight_decay 1e-4)
and writes the reference's checkpoints (<root_dir>/<exp_name>/checkpoints/checkpoint_epoch_best.tar, the one before kept as
..._previous.tar; legacy serialisation; keys epoch / model_state_dict / optimizer_state_dict), so either side loads the other's.

The backend follows `train.device`, there is no option for it:
  * cuda: the data set lives on the device; parameters, gradients and both Adam moments each live in ONE flat fp32 buffer
    (state-dict order, every tensor on a 16-byte boundary, zero pads) of which the model's parameters are views.  A step is four
    calls of the C ABI -- pndf_train_batch, pndf_train_forward, pndf_train_backward, pndf_adam_step (csrc/pndf_optim.hip,
    csrc/pndf_train.hip) -- with no autograd, allocation, synchronisation or host-to-device copy inside an epoch; the losses of
    a step go to one row of a per-epoch device log that `train_model` reads back once.  No fallback: PndfError without the
    library, a gfx950 device or the structure encoder.
  * cpu: torch indexing, the stock `forward(train=True)` and `torch.optim.Adam`.

Epochs, as the reference's DataLoader(shuffle=True, drop_last=True): a permutation of the data files is cut into
F // batch_size steps of batch_size items; every item gets one uniformly drawn manifold file and `data.num_pts` (5000, which the
reference hard-codes) rows with replacement from its data file and from its manifold file.  All draws of epoch `ep` come from
np.random.RandomState(epoch_seed(seed, ep)) -- the legacy generator, whose stream is frozen -- in this order: permutation(F);
randint(0, Fm, items); randint(0, 2^32, (items, 2, num_pts), uint32) raw words; row = first + (word * len >> 32).  They are made
on the host when the epoch begins and uploaded once, so the cpu and cuda trainers see the same batches, `batch_rows` rebuilds
any batch, and a resume at an epoch boundary continues bit for bit.

Differences from the reference, on purpose:
  * load_data.py:63 flips `poses` where it means `amass_poses`, so with `data.flip` its manifold batch is a copy of the noisy
    poses; here the flip applies to the manifold poses themselves (also listed in posendf_amd/traindata.py);
  * the row draws are words scaled by the file length (bias below len / 2^32 per row), not np.random.randint's rejection
    sampling, and they are seeded: the reference's workers seed numpy from os.urandom;
  * the checkpoint's `epoch` is the epoch just trained, as in the reference, but a resume continues with the NEXT epoch; the
    reference's loop (trainer.py:21) trains the stored epoch a second time;
  * scalars go to <exp>/summary.jsonl (one JSON line per epoch), not to TensorBoard;
  * the data set is resident in memory (device memory on cuda): one that does not fit is refused with the byte count;
  * `data.online` (posendf_amd.online) replaces the frozen sample files by a pool that is redrawn and relabelled on the device
    every `refresh_every` epochs; without it every code path is the file-based one;
  * another skeleton: when `model.StrEnc.parent_mapping` is set (a list or a name of posendf_amd.SKELETONS) the model is
    `SkeletonPoseNDF(opt)`, the files hold `pose` [n,J,4] for its J joints and the cuda backend runs the same four calls on a plan
    of include/posendf_amd_skeleton_train.h.  Online data for it is passed as `dataset=OnlinePoseDataset(..., num_joints=J)`
    (include/posendf_amd_skeleton_data.h); the config mapping `data.online` builds the 21-joint pool only and is refused on
    another table than SMPL's.
"""
from __future__ import annotations

import argparse
import ctypes
import glob
import json
import os
import shutil

import numpy as np
import torch

from .engine import PndfError, TrainEngine, adam_step, load_library, skel_train_batch, state_dict_order, stream_handle
from .facade import PoseNDF
from .synth import PARENT as SMPL_PARENT
from .train import LOSS_CODES

LOSS_KEYS = ("dist", "man_loss", "eikonal")
WEIGHT_DECAY = 1e-4                      # train_posendf.py:30
BETAS, EPS = (0.9, 0.999), 1e-8          # torch.optim.Adam's defaults, which the reference keeps


def epoch_seed(seed: int, epoch: int) -> int:
    """the RandomState seed of all draws of one epoch: a function of (seed, epoch) only"""
    return (int(seed) * 1000003 + int(epoch) * 7919 + 12345) % (2 ** 32)


def _subdirs(root, datasets):
    if not datasets:
        datasets = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
    return list(datasets)


class PoseDataset:
    """Every `<data_dir>/<dataset>/*.npz` (keys `pose` [n,J,4], `dist` [n,k]) and `<amass_dir>/<dataset>/*.npz` (key `pose`),
    concatenated once and kept on `device`: pose [N,J,4], dist [N,k], man [M,J,4] fp32, file_off [F+1], man_off [Fm+1] int64, for
    poses of J = `num_joints` joints (21: SMPL).  `datasets` defaults to every subdirectory (as traindata.database_files).  Files are
    refused by name when `pose` is not [n,J,4], when `dist` does not have one row per pose or has another k than the first file,
    and when they are empty (the sampler cannot draw from them)."""
    num_joints = 21      # (of a data set that sets none)

    def __init__(self, data_dir, amass_dir, datasets=None, device="cpu", num_joints=21):
        self.num_joints = int(num_joints)
        files, man_files = [], []
        for ds in _subdirs(data_dir, datasets):
            files += sorted(glob.glob(os.path.join(data_dir, ds, "*.npz")))
        for ds in _subdirs(amass_dir, datasets):
            man_files += sorted(glob.glob(os.path.join(amass_dir, ds, "*.npz")))
        if not files:
            raise FileNotFoundError(f"no data files <dataset>/*.npz under {data_dir}")
        if not man_files:
            raise FileNotFoundError(f"no manifold files <dataset>/*.npz under {amass_dir}")
        poses, dists, mans = [], [], []
        for f in files:
            with np.load(f) as z:
                if "pose" not in z.files or "dist" not in z.files:
                    raise ValueError(f"{f}: a data file holds `pose` and `dist`, this one {sorted(z.files)}")
                poses.append(self._pose(f, z["pose"], self.num_joints))
                d = np.asarray(z["dist"])
                if d.ndim != 2 or len(d) != len(poses[-1]) or d.shape[1] < 1:
                    raise ValueError(f"{f}: dist is {d.shape}, expected [{len(poses[-1])}, k]")
                if dists and d.shape[1] != dists[0].shape[1]:
                    raise ValueError(f"{f}: dist has k = {d.shape[1]}, {files[0]} has k = {dists[0].shape[1]}")
                dists.append(np.ascontiguousarray(d, dtype=np.float32))
        for f in man_files:
            with np.load(f) as z:
                if "pose" not in z.files:
                    raise ValueError(f"{f}: a manifold file holds `pose`, this one {sorted(z.files)}")
                mans.append(self._pose(f, z["pose"], self.num_joints))
        self._init(poses, dists, mans, device, files, man_files)

    @classmethod
    def from_arrays(cls, poses, dists, mans, device="cpu", num_joints=21):
        """the same from lists of arrays, one entry per file (tests, benchmarks)"""
        self = cls.__new__(cls)
        self.num_joints = int(num_joints)
        names = [f"<data {i}>" for i in range(len(poses))]
        mnames = [f"<manifold {i}>" for i in range(len(mans))]
        poses = [cls._pose(n, p, self.num_joints) for n, p in zip(names, poses)]
        mans = [cls._pose(n, p, self.num_joints) for n, p in zip(mnames, mans)]
        dists = [np.ascontiguousarray(d, dtype=np.float32) for d in dists]
        for n, p, d in zip(names, poses, dists):
            if d.ndim != 2 or len(d) != len(p) or d.shape[1] != dists[0].shape[1] or d.shape[1] < 1:
                raise ValueError(f"{n}: dist is {d.shape}, expected [{len(p)}, {dists[0].shape[1] if dists[0].ndim == 2 else 'k'}]")
        self._init(poses, dists, mans, device, names, mnames)
        return self

    @staticmethod
    def _pose(name, p, num_joints=21):
        p = np.asarray(p)
        if p.ndim != 3 or p.shape[1:] != (num_joints, 4):
            raise ValueError(f"{name}: pose is {p.shape}, expected [n, {num_joints}, 4]")
        if len(p) == 0:
            raise ValueError(f"{name}: an empty file cannot be sampled")
        if len(p) >= 2 ** 32:
            raise ValueError(f"{name}: {len(p)} rows, the sampler draws 32-bit words")
        return np.ascontiguousarray(p, dtype=np.float32)

    def _init(self, poses, dists, mans, device, files, man_files):
        self.files, self.man_files = list(files), list(man_files)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.k = int(dists[0].shape[1])
        self.file_off = np.concatenate([[0], np.cumsum([len(p) for p in poses])]).astype(np.int64)
        self.man_off = np.concatenate([[0], np.cumsum([len(p) for p in mans])]).astype(np.int64)
        N, M = int(self.file_off[-1]), int(self.man_off[-1])
        nq = 4 * self.num_joints
        self.nbytes = 4 * (N * nq + N * self.k + M * nq) + 8 * (len(self.file_off) + len(self.man_off))
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            if self.nbytes > free:
                raise MemoryError(f"the data set needs {self.nbytes} bytes on {self.device}, {free} are free: a data set larger "
                                  "than device memory is not supported")
        self.pose = torch.from_numpy(np.concatenate(poses)).to(self.device)
        self.dist = torch.from_numpy(np.concatenate(dists)).to(self.device)
        self.man = torch.from_numpy(np.concatenate(mans)).to(self.device)
        self.file_off_t = torch.from_numpy(self.file_off).to(self.device)
        self.man_off_t = torch.from_numpy(self.man_off).to(self.device)

    @property
    def F(self):
        return len(self.file_off) - 1

    @property
    def Fm(self):
        return len(self.man_off) - 1


def mean_labels(d):
    """np.mean(dist, axis=1) of load_data.py:53 as the batch kernel forms it: fp32, summed in index order, divided by k"""
    acc = d[:, 0].clone()
    for c in range(1, d.shape[1]):
        acc += d[:, c]
    return acc / float(d.shape[1])


def quat_flip(q):
    """load_data.py:12-16: every joint quaternion whose real part is < 0, negated"""
    return torch.where(q[..., :1] < 0, -q, q)


class Trainer:
    """`PoseNDF_trainer(opt)` (train_posendf.py:15-176).  Reads train.{device, batch_size, optimizer_param, continue_train,
    max_epoch, loss_type, man_loss, dist, eikonal}, data.{data_dir, amass_dir, flip (False), num_pts (5000)} and
    experiment.{root_dir, exp_name}; `seed` feeds the initial weights and, with the epoch, every draw of the sampler.
    `dataset`: a PoseDataset to train on instead of the directories of `opt['data']`.

    Another skeleton: with `model.StrEnc.parent_mapping` (a list, or a name of posendf_amd.SKELETONS) the model is
    `SkeletonPoseNDF(opt)` and the data set holds poses of its J joints; without the key nothing changes.

    Online data (posendf_amd.online): with the mapping `data.online` = {files, rows, refresh_every (epochs, default 1), sigmas,
    shares, noise, k, metric, weighted} -- or an `OnlinePoseDataset` passed as `dataset` -- the noisy poses are a pool of files x
    rows poses drawn from `data.amass_dir` and labelled on the device; `data.data_dir` is not read.  `begin_epoch(epoch)` makes
    pool `epoch // refresh_every` of the trainer's seed resident when it is not; the pool is a pure function of (seed, draw,
    manifold, options), so a resume regenerates it and continues bit for bit.  The experiment name gains the prefix `online_`."""

    def __init__(self, opt, seed=0, dataset=None):
        tr, data = opt["train"], opt.get("data") or {}
        self.opt = opt
        self.seed = int(seed)
        self.device = torch.device(tr["device"])
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.batch_size = int(tr["batch_size"])
        self.learning_rate = float(tr["optimizer_param"])
        self.max_epoch = int(tr.get("max_epoch", 0))
        self.flip = bool(data.get("flip", False))
        self.num_pts = int(data.get("num_pts", 5000))
        self.loss = tr["loss_type"]
        self.loss_weight = {"man_loss": float(tr["man_loss"]), "dist": float(tr["dist"]), "eikonal": float(tr["eikonal"])}
        self.eikonal = self.loss_weight["eikonal"] > 0.0
        # with eikonal off the reference's model returns (loss, {'dist': loss}): the objective is `dist` alone
        self.keys = LOSS_KEYS if self.eikonal else ("dist",)
        # train_posendf.py:58-62
        name = "{}_{}_{}_{}_dist{}_eik{}".format(opt["experiment"]["exp_name"], opt["model"]["DFNet"]["act"], self.loss,
                                                 tr["optimizer_param"], tr["dist"], tr["eikonal"])
        online = data.get("online")
        self.online = online is not None or hasattr(dataset, "refresh")
        self.refresh_every = int((online or {}).get("refresh_every", 1))
        if self.refresh_every < 1:
            raise ValueError(f"data.online.refresh_every = {self.refresh_every}: a pool lasts one epoch or more")
        if self.online:
            name = "online_{}".format(name)      # the two data sources keep their checkpoints apart
        self.exp_name = "flip_{}".format(name) if self.flip else name
        self.exp_path = "{}/{}/".format(opt["experiment"]["root_dir"], self.exp_name)
        self.checkpoint_path = self.exp_path + "checkpoints/"
        os.makedirs(self.checkpoint_path, exist_ok=True)

        with torch.random.fork_rng(devices=[]):        # the initial weights: a function of `seed`, the global stream untouched
            torch.manual_seed(self.seed)
            if "parent_mapping" in opt["model"]["StrEnc"]:
                from .skeleton import SkeletonPoseNDF
                self.model = SkeletonPoseNDF(opt).to(self.device)
            else:
                self.model = PoseNDF(opt).to(self.device)
        self.num_joints = self.model.num_joints
        if online is not None and tuple(self.model.parents) != tuple(SMPL_PARENT):
            raise PndfError(f"`data.online` in a config builds the 21-joint pool only, this model has the {self.num_joints}-joint table "
                            f"{list(self.model.parents)}: pass its pool as dataset=OnlinePoseDataset(..., num_joints={self.num_joints})")
        self.hip = self.device.type == "cuda"
        if self.hip and self.model.enc is None:
            raise PndfError("training on cuda needs the structure encoder (model.StrEnc.use: True), as opt['engine']['train'] = 'hip'")
        if dataset is None and online is not None:
            dataset = self._online_dataset(data, online)
        self.dataset = dataset if dataset is not None else PoseDataset(data["data_dir"], data["amass_dir"], data.get("datasets"),
                                                                        self.device, self.num_joints)
        if self.dataset.num_joints != self.num_joints:
            raise ValueError(f"the data set holds poses of {self.dataset.num_joints} joints, the model has {self.num_joints}")
        if self.dataset.device != self.device:
            raise ValueError(f"the data set is on {self.dataset.device}, the trainer on {self.device}")
        if self.dataset.F < self.batch_size:
            raise ValueError(f"{self.dataset.F} data files give no step of batch_size {self.batch_size} (drop_last)")
        self.steps_per_epoch = self.dataset.F // self.batch_size
        self.items = self.steps_per_epoch * self.batch_size
        self.B = self.batch_size * self.num_pts
        self.iter_nums = 0          # optimiser steps so far (train_posendf.py:102), the Adam step count
        self.ep = 0                 # the next epoch to train
        self._draws = None          # (epoch, perm, man_files, words) of the epoch in flight
        self._cursor = None         # (epoch, next step)
        self._log = None
        if self.hip:
            self._init_hip()
        else:
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=self.learning_rate, weight_decay=WEIGHT_DECAY)
            self._log = np.zeros((self.steps_per_epoch, 3), np.float32)
        if tr.get("continue_train"):
            self.ep = self.load_checkpoint()

    # ---- the cuda backend's buffers ---------------------------------------------------------------
    def _init_hip(self):
        m, dev = self.model, self.device
        self.lib = load_library()
        named = dict(m.named_parameters())
        skel = m._net_kw.get("parents")      # SkeletonPoseNDF: its table; PoseNDF: None, the SMPL plan of pndf_train_create
        self._keys = state_dict_order(True, len(m._hidden) + 1, parents=skel)
        if set(self._keys) != set(named):
            raise PndfError("the model's parameters are not the reference's state dict")
        self._offsets, n = [], 0
        for k in self._keys:
            self._offsets.append(n)
            n += -(-named[k].numel() // 4) * 4      # every tensor on a 16-byte boundary
        self.n_flat = n
        self.flat_p, self.flat_g, self.flat_m, self.flat_v = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
        self._params = []
        for k, o in zip(self._keys, self._offsets):
            p = named[k]
            if p.dtype != torch.float32:
                raise PndfError(f"{k} is {p.dtype}: the trainer keeps fp32 parameters")
            view = self.flat_p[o:o + p.numel()].view(p.shape)
            view.copy_(p.detach())
            p.data = view                             # the model's parameters are views into the flat buffer from here on
            self._params.append(p)
        self._ptrs = [p.data_ptr() for p in self._params]
        tab = ctypes.c_void_p * len(self._keys)
        self._wtab = tab(*self._ptrs)
        self._gtab = tab(*[self.flat_g.data_ptr() + 4 * o for o in self._offsets])
        self._engine = TrainEngine(m._act, m._beta, dev.index, lib=self.lib, hidden=m._hidden, enc_act=m._enc_act, enc_beta=m._enc_beta,
                                   parents=skel)
        self._ws = torch.empty(self._engine.workspace_floats(self.B, self.B, self.eikonal), dtype=torch.float32, device=dev)
        self._q = torch.empty(self.B, self.num_joints, 4, dtype=torch.float32, device=dev)
        self._qm = torch.empty(self.B, self.num_joints, 4, dtype=torch.float32, device=dev)
        self._gt = torch.empty(self.B, dtype=torch.float32, device=dev)
        self._upstream = torch.tensor([self.loss_weight[k] for k in LOSS_KEYS], dtype=torch.float32, device=dev)
        self._log_dev = torch.zeros(self.steps_per_epoch, 3, dtype=torch.float32, device=dev)
        # the epoch's draws on the device, written once per epoch
        self._item_file = torch.zeros(self.items, dtype=torch.int32, device=dev)
        self._item_man = torch.zeros(self.items, dtype=torch.int32, device=dev)
        self._words = torch.zeros(self.items, 2, self.num_pts, dtype=torch.int32, device=dev)      # uint32 bit patterns

    def _online_dataset(self, data, online):
        """the OnlinePoseDataset of `data.online` over `data.amass_dir`"""
        from .online import OnlineOptions, OnlinePoseDataset
        known = {"files", "rows", "refresh_every", "sigmas", "shares", "noise", "k", "metric", "weighted", "chunk"}
        if set(online) - known:
            raise ValueError(f"data.online: unknown keys {sorted(set(online) - known)} (known: {sorted(known)})")
        if "files" not in online or "rows" not in online:
            raise ValueError("data.online needs `files` and `rows`: the pool is files x rows noisy poses")
        kw = {k: online[k] for k in ("noise", "k", "metric", "weighted") if k in online}
        for k in ("sigmas", "shares"):
            if k in online:
                kw[k] = tuple(float(x) for x in online[k])
        extra = {"chunk": int(online["chunk"])} if "chunk" in online else {}
        return OnlinePoseDataset(data["amass_dir"], int(online["files"]), int(online["rows"]), OnlineOptions(**kw), data.get("datasets"),
                                 self.device, **extra)

    def _ensure_pool(self, epoch):
        """online data: the pool of `epoch` resident (a no-op when it is, and for a file-based data set)"""
        if self.online:
            draw = int(epoch) // self.refresh_every
            if self.dataset.draw != draw or self.dataset.seed != self.seed:
                self.dataset.refresh(draw, self.seed)

    def _check_homes(self):
        """the parameters must still be the views the kernels update"""
        for k, p, ptr in zip(self._keys, self._params, self._ptrs):
            if p.data_ptr() != ptr:
                raise PndfError(f"{k} no longer lives in the trainer's flat parameter buffer (re-homed by .to(), an assignment or "
                                "load_state_dict(assign=True)): build a new Trainer")

    def _stale_inference(self):
        """The facade's fingerprint is (data_ptr, _version) of every parameter and an update by the optimiser kernel changes
        neither: mark the cached inference engines stale, so that forward(train=False) / project() re-pack the weights."""
        for entry in self.model._engines.values():
            entry[1] = None

    # ---- the sampler -----------------------------------------------------------------------------
    def _epoch_draws(self, epoch):
        if self._draws is None or self._draws[0] != epoch:
            rng = np.random.RandomState(epoch_seed(self.seed, epoch))
            perm = rng.permutation(self.dataset.F)[:self.items].astype(np.int32)
            man = rng.randint(0, self.dataset.Fm, self.items).astype(np.int32)
            words = rng.randint(0, 2 ** 32, size=(self.items, 2, self.num_pts), dtype=np.uint32)
            self._draws = (epoch, perm, man, words)
        return self._draws[1:]

    def batch_rows(self, epoch, step):
        """(rows [B], man_rows [Bm]) int64: the rows of dataset.pose / dataset.dist and of dataset.man that step `step` of epoch
        `epoch` trains on.  A pure function of (seed, epoch, step) and the data set's file lengths."""
        if not 0 <= step < self.steps_per_epoch:
            raise IndexError(f"step {step} of {self.steps_per_epoch}")
        perm, man, words = self._epoch_draws(epoch)
        s = slice(step * self.batch_size, (step + 1) * self.batch_size)
        out = []
        for files, off, side in ((perm[s], self.dataset.file_off, 0), (man[s], self.dataset.man_off, 1)):
            first = off[files].astype(np.uint64)[:, None]
            length = (off[files + 1] - off[files]).astype(np.uint64)[:, None]
            out.append((first + ((words[s, side].astype(np.uint64) * length) >> np.uint64(32))).astype(np.int64).reshape(-1))
        return out[0], out[1]

    def begin_epoch(self, epoch):
        """draws the epoch on the host and (cuda) uploads it: the only host-to-device copy of the epoch"""
        perm, man, words = self._epoch_draws(epoch)
        self._ensure_pool(epoch)
        if self.hip:
            self._item_file.copy_(torch.from_numpy(perm))
            self._item_man.copy_(torch.from_numpy(man))
            self._words.copy_(torch.from_numpy(words.view(np.int32)))
            self._log_dev.zero_()
        else:
            self._log[:] = 0
        self._cursor = [epoch, 0]

    # ---- one optimiser step ------------------------------------------------------------------------
    def step(self):
        """train_posendf.py:93-99 for the next batch of the epoch in flight (begin_epoch(self.ep) when there is none)"""
        if self._cursor is None:
            self.begin_epoch(self.ep)
        epoch, i = self._cursor
        if i >= self.steps_per_epoch:
            raise IndexError(f"epoch {epoch} has {self.steps_per_epoch} steps: begin_epoch() starts the next one")
        self._ensure_pool(epoch)      # (online data: batch() of another epoch may have swapped the pool since begin_epoch)
        if self.hip:
            self._step_hip(i)
        else:
            self._step_torch(epoch, i)
        self._cursor[1] = i + 1
        self.iter_nums += 1

    def _step_hip(self, i):
        ds, bs = self.dataset, self.batch_size
        self._check_homes()
        stream = stream_handle(self.device)
        skel_train_batch(ds.pose.data_ptr(), ds.dist.data_ptr(), ds.man.data_ptr(), ds.file_off_t.data_ptr(), ds.man_off_t.data_ptr(),
                         self._item_file.data_ptr() + 4 * i * bs, self._item_man.data_ptr() + 4 * i * bs,
                         self._words.data_ptr() + 4 * i * bs * 2 * self.num_pts, ds.F, ds.Fm, ds.k, bs, self.num_pts, self.flip,
                         self.num_joints, self._q.data_ptr(), self._gt.data_ptr(), self._qm.data_ptr(), stream, self.lib)
        ws = self._ws.data_ptr()
        self._engine.forward(self._wtab, self._q.data_ptr(), self._gt.data_ptr(), self._qm.data_ptr(), self.B, self.B,
                             LOSS_CODES[self.loss], self.eikonal, self._log_dev.data_ptr() + 12 * i, ws, stream)
        self._engine.backward(self._wtab, self._upstream.data_ptr(), self._gtab, ws, stream)      # gradients written, not added
        adam_step(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.flat_m.data_ptr(), self.flat_v.data_ptr(), self.n_flat,
                  self.iter_nums + 1, self.learning_rate, BETAS[0], BETAS[1], EPS, WEIGHT_DECAY, stream, self.lib)
        self._stale_inference()

    def batch(self, epoch, step):
        """the batch of (epoch, step) with torch indexing, on the trainer's device: (pose [B,J,4], dist_gt [B], man [B,J,4])"""
        rows, man_rows = self.batch_rows(epoch, step)
        self._ensure_pool(epoch)
        ds = self.dataset
        rows, man_rows = torch.from_numpy(rows).to(self.device), torch.from_numpy(man_rows).to(self.device)
        pose, man = ds.pose[rows], ds.man[man_rows]
        if self.flip:
            pose, man = quat_flip(pose), quat_flip(man)
        return pose, mean_labels(ds.dist[rows]), man

    def _step_torch(self, epoch, i):
        pose, gt, man = self.batch(epoch, i)
        self.model.train()
        self.optimizer.zero_grad()
        _, ld = self.model(pose, gt, man, train=True, eikonal=self.loss_weight["eikonal"])
        loss = 0.0
        for k in ld.keys():
            loss += self.loss_weight[k] * ld[k]
        loss.backward()
        self.optimizer.step()
        for c, k in enumerate(LOSS_KEYS):
            self._log[i, c] = float(ld[k].detach()) if k in ld else 0.0

    # ---- one epoch -----------------------------------------------------------------------------------
    def read_log(self):
        """the per-step losses [steps, 3] (dist, man_loss, eikonal) of the epoch in flight; on cuda this synchronises"""
        return self._log_dev.cpu().numpy() if self.hip else self._log.copy()

    def total_loss(self, row):
        """train_posendf.py:95-97 on one row of the log, in fp32 like the reference's tensors"""
        total = np.float32(0.0)
        for c, k in enumerate(LOSS_KEYS):
            if k in self.keys:
                total = np.float32(total + np.float32(self.loss_weight[k]) * np.float32(row[c]))
        return total

    def train_model(self, ep=None):
        """one epoch, its summary line and its checkpoint: (loss of the last step, mean loss of the epoch) as floats"""
        ep = self.ep if ep is None else int(ep)
        self.begin_epoch(ep)
        for _ in range(self.steps_per_epoch):
            self.step()
        log = self.read_log()                          # the epoch's only synchronisation
        totals = [self.total_loss(r) for r in log]
        mean = float(np.float32(sum(np.float32(t) * np.float32(self.batch_size) for t in totals)
                                / np.float32(self.batch_size * len(totals))))      # AverageMeter (train_posendf.py:101)
        line = {"epoch": ep, "iter": self.iter_nums}
        for c, k in enumerate(LOSS_KEYS):
            if k in self.keys:
                line[f"train/loss_{k}"] = float(log[-1, c])      # train_posendf.py:104-105: the last step's
        line["train/epoch"] = mean                              # :106
        with open(self.exp_path + "summary.jsonl", "a") as f:
            f.write(json.dumps(line) + "\n")
        self.save_checkpoint(ep)
        self.ep = ep + 1
        self._cursor = None
        return float(totals[-1]), mean

    # ---- checkpoints (train_posendf.py:147-176) ----------------------------------------------------------
    def optimizer_state_dict(self):
        """the layout of torch.optim.Adam.state_dict(): per-parameter step / exp_avg / exp_avg_sq in model.parameters() order
        and one param group"""
        if not self.hip:
            return self.optimizer.state_dict()
        params = list(self.model.parameters())
        groups = torch.optim.Adam(params, lr=self.learning_rate, betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY).state_dict()["param_groups"]
        state = {}
        if self.iter_nums > 0:
            home = {id(p): o for p, o in zip(self._params, self._offsets)}
            for i, p in enumerate(params):
                o = home[id(p)]
                state[i] = {"step": torch.tensor(float(self.iter_nums)),
                            "exp_avg": self.flat_m[o:o + p.numel()].view(p.shape).clone(),
                            "exp_avg_sq": self.flat_v[o:o + p.numel()].view(p.shape).clone()}
        return {"state": state, "param_groups": groups}

    def load_optimizer_state_dict(self, sd):
        state = {int(i): dict(s) for i, s in sd["state"].items()}
        steps = {int(float(s["step"])) for s in state.values()}          # a tensor or a number
        if len(steps) > 1:
            raise ValueError(f"the parameters of this optimiser state have different step counts {sorted(steps)}")
        if not self.hip:
            for s in state.values():
                s["step"] = torch.as_tensor(float(s["step"]), dtype=torch.float32)
            self.optimizer.load_state_dict({"state": state, "param_groups": sd["param_groups"]})
            for g in self.optimizer.param_groups:      # the config decides the rate, as the reference's constructor does
                g["lr"] = self.learning_rate
        else:
            params = list(self.model.parameters())
            if state and sorted(state) != list(range(len(params))):
                raise ValueError(f"optimiser state for {len(state)} parameters, the model has {len(params)}")
            home = {id(p): o for p, o in zip(self._params, self._offsets)}
            self.flat_m.zero_()
            self.flat_v.zero_()
            for i, s in state.items():
                p = params[i]
                o = home[id(p)]
                self.flat_m[o:o + p.numel()].view(p.shape).copy_(s["exp_avg"])
                self.flat_v[o:o + p.numel()].view(p.shape).copy_(s["exp_avg_sq"])
        self.iter_nums = steps.pop() if steps else 0

    def save_checkpoint(self, epoch):
        path = self.checkpoint_path + "checkpoint_epoch_best.tar"
        if os.path.exists(path):
            shutil.copyfile(path, self.checkpoint_path + "checkpoint_epoch_previous.tar")      # (the file name only, whatever the path holds)
        torch.save({"epoch": epoch, "model_state_dict": self.model.state_dict(), "optimizer_state_dict": self.optimizer_state_dict()},
                   path, _use_new_zipfile_serialization=False)

    def load_checkpoint(self):
        """loads checkpoint_epoch_best.tar when there is one: the next epoch to train (0 without a checkpoint)"""
        path = self.checkpoint_path + "checkpoint_epoch_best.tar"
        if not os.path.exists(path):
            print("No checkpoints found at {}".format(self.checkpoint_path))
            return 0
        ck = torch.load(path, map_location=self.device)
        self.model.load_state_dict(ck["model_state_dict"])          # copies in place: the views stay
        if self.hip:
            self._check_homes()
            self._stale_inference()
        self.load_optimizer_state_dict(ck["optimizer_state_dict"])
        print("Loaded checkpoint from: {}".format(path))
        return int(ck["epoch"]) + 1


def train(opt, config_file=None, seed=0):
    """trainer.py:11-25: the config copied next to the checkpoints, then epochs ep .. max_epoch"""
    trainer = Trainer(opt, seed=seed)
    if config_file:
        shutil.copyfile(config_file, trainer.exp_path + "config.yaml")
    for ep in range(trainer.ep, trainer.max_epoch):
        loss, mean = trainer.train_model(ep)
        print("train/epoch", mean, ep)
    return trainer


def main(argv=None):
    from .config import load_config
    ap = argparse.ArgumentParser(description="Train PoseNDF.")
    ap.add_argument("--config", "-c", required=True, help="path to the config file (configs/amass.yaml's keys)")
    ap.add_argument("--max_epoch", type=int, default=None, help="overrides train.max_epoch")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    opt = load_config(a.config)
    if a.max_epoch is not None:
        opt["train"]["max_epoch"] = a.max_epoch
    train(opt, a.config, a.seed)


if __name__ == "__main__":
    main()
