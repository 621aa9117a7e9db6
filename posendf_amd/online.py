"""Online training data: noisy poses drawn from the pose manifold on the device and labelled on the fly with their exact distance to
it -- what the reference sketches in model/load_data.py:89-135 (`PoseData_online`, marked "not used") and could not afford.

    q, src, group = sample_noisy(man[N,21,4], count, seed=0, draw=0)        # csrc/pndf_online.hip; the host twin for a cpu tensor
    ds = OnlinePoseDataset(amass_dir, files=40, rows=5000, device="cuda:0") # a pool of files x rows noisy poses over <amass_dir>
    ds.refresh(draw=3, seed=0)                                              # pose <- the sampler, dist <- pndf_knn_search
    Trainer(opt, dataset=ds)        # or `data.online: {files, rows, refresh_every, ...}` in the config (posendf_amd.trainer)

Another skeleton: `num_joints=J` (1 .. 32) on sample_noisy, OnlinePoseDataset and .from_manifold draws and labels poses [.., J, 4]
(include/posendf_amd_skeleton_data.h); a J-joint data set goes to the trainer as `dataset=`.

A pool is a pure function of (seed, draw, options, manifold): pose i takes the manifold row, the sigma group and the noise that
the Philox4x32-10 blocks with counter (i, block, draw) and key `seed` give it (include/posendf_amd_online.h), so any chunking
produces the same bits and a pool is regenerated, not stored.  `OnlinePoseDataset` holds the pool in the buffers `Trainer` and
pndf_train_batch already read -- pose [F*R,21,4], dist [F*R,k], file_off -- with virtual file f owning poses f*R .. (f+1)*R - 1,
so the optimiser step is the file-based one, untouched.

Differences from data/create_data.py, on purpose: the noise is drawn per pose and per component (:89 shares one rand(21, 4)
across a whole sigma group); the group of a pose is drawn (shares are probabilities, not exact counts); noise="symmetric"
(2 u - 1) exists next to the reference's "uniform" (u in [0, 1), biased towards +); the labels are the exact k nearest of the
whole manifold, as posendf_amd.traindata's.
"""
from __future__ import annotations

import glob
import os
from dataclasses import dataclass

import numpy as np
import torch

from .dist_utils import JOINT_RANK
from .engine import PndfError, load_library, online_opts, online_sample, online_sample_cpu, stream_handle
from .traindata import SAMPLE_DISTRIBUTION, SIGMA
from .trainer import PoseDataset, _subdirs

KNN_TILE_BYTES, KNN_TILE = 5376, 16      # csrc/pndf_knn.hip: the packed index is whole tiles of 16 poses (21 joints)


def knn_tile_bytes(num_joints=21):
    """one packed tile of the index: J joints x 4 components x 16 poses, fp32"""
    return 256 * int(num_joints)


def _check_joints(num_joints, weighted=False):
    J = int(num_joints)
    if not 1 <= J <= 32:
        raise ValueError(f"num_joints = {J}: the sampler and the index take 1 .. 32 joints")
    if weighted and J != 21:
        raise ValueError(f"OnlineOptions.weighted is the joint-rank vector of the 21 SMPL joints, not of {J}")
    return J


@dataclass(frozen=True)
class OnlineOptions:
    """What a pool is drawn and labelled with: noise scales and their shares (create_data.py:49-50), the noise mode, and the k,
    metric and joint weighting of the labels (posendf_amd.knn.PoseIndex)."""
    sigmas: tuple = SIGMA
    shares: tuple = SAMPLE_DISTRIBUTION
    noise: str = "uniform"
    k: int = 5
    metric: str = "geo"
    weighted: bool = False

    def opts(self, seed=0, draw=0, lib=None):
        """the pndf_online_opts of pool (seed, draw)"""
        return online_opts(self.sigmas, self.shares, self.noise, seed, draw, lib)


def _sample_into(man, first, count, opt, q, src, group, lib=None):
    """pool poses first .. first + count - 1 into q (and src, group: tensors or None) on man's device, on the current stream;
    man [N,J,4] gives the joint count"""
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    J = man.shape[1]
    if man.device.type == "cuda":
        with torch.cuda.device(man.device):
            online_sample(man.data_ptr(), man.shape[0], first, count, opt, q.data_ptr(), ptr(src), ptr(group), stream_handle(man.device), lib, J)
    else:
        online_sample_cpu(man.data_ptr(), man.shape[0], first, count, opt, q.data_ptr(), ptr(src), ptr(group), lib, J)


def sample_noisy(man, count, *, first=0, seed=0, draw=0, options=None, num_joints=21):
    """-> (q float32 [count,J,4], src int64 [count], group int32 [count]) on `man`'s device: poses first .. first + count - 1
    of pool (seed, draw) over the manifold man [N,J,4], J = `num_joints`.  On cuda this is pndf_online_sample (J = 21) or
    pndf_skel_online_sample on the current stream (no synchronisation); on cpu the host twin, the same bits."""
    options = options or OnlineOptions()
    J = _check_joints(num_joints)
    man = torch.as_tensor(man).to(torch.float32).reshape(-1, J, 4).contiguous()
    count = int(count)
    if count < 0:
        raise PndfError(f"count = {count}")
    q = torch.empty(count, J, 4, dtype=torch.float32, device=man.device)
    src = torch.empty(count, dtype=torch.int64, device=man.device)
    group = torch.empty(count, dtype=torch.int32, device=man.device)
    if count:
        _sample_into(man, int(first), count, options.opts(seed, draw), q, src, group)
    return q, src, group


def _joint_weights(weighted, device, dtype):
    if not weighted:
        return None
    rank = torch.tensor(JOINT_RANK, dtype=torch.float32)
    return torch.nn.functional.normalize(rank, dim=0).to(device, dtype)                # dist_utils.py:18,41


def host_labels(queries, man, k, metric, weighted, vals, idx, budget=2 ** 18):
    """dist_utils.geo / euc over the whole manifold and the k smallest, restated with torch on the host in fp64 (rounded to fp32
    at the end), about `budget` pairs at a time: ascending, ties to the lower row, a NaN distance last.  Slow -- a [chunk, M, J]
    intermediate and a full sort per chunk -- and meant for small sets.  Any joint count J = man.shape[1]; `weighted` (the SMPL
    joint ranks) with 21 only."""
    _check_joints(man.shape[1], weighted)
    m = man.to(torch.float64)
    w = _joint_weights(weighted, man.device, torch.float64)
    step = max(1, budget // max(len(m), 1))
    for s in range(0, len(queries), step):
        n = queries[s:s + step].to(torch.float64)[:, None]                             # [c,1,J,4]
        if metric == "geo":
            per_joint = 1.0 - torch.einsum("cjd,mjd->cmj", n[:, 0], m).abs()
        elif metric == "euc":
            per_joint = (n - m[None]).pow(2).sum(dim=3).sqrt()
        else:
            raise PndfError(f"unknown metric {metric!r} (geo, euc)")
        d = (per_joint * w).sum(dim=2) if w is not None else per_joint.mean(dim=2)
        v, i = torch.sort(d, dim=1, stable=True)
        vals[s:s + step] = v[:, :k].to(torch.float32)
        i = i[:, :k]
        idx[s:s + step] = torch.where(torch.isnan(v[:, :k]), torch.full_like(i, -1), i)


class OnlinePoseDataset(PoseDataset):
    """A `PoseDataset` whose noisy poses and labels are generated, not loaded: built from the manifold files alone
    (`<amass_dir>/<dataset>/*.npz`, key `pose`), it exposes what `Trainer` and pndf_train_batch read -- pose [F*R,J,4], dist
    [F*R,k], man [M,J,4], file_off, man_off (and their device copies file_off_t, man_off_t), k, F, Fm, nbytes, device, num_joints
    -- with `files` virtual data files of `rows` poses each and J = `num_joints` joints (21: SMPL; any of 1 .. 32).  `refresh(draw, seed)` rewrites pose, src, group (the manifold row and the
    sigma group every pose came from) and dist, nn_idx (the exact k nearest manifold rows) in place; `draw` and `seed` record
    which pool is resident (None before the first refresh).

    On cuda the data set keeps one PoseIndex over the manifold and one search workspace sized for its query chunk (`chunk`
    poses per pndf_knn_search); refresh allocates nothing, copies nothing from the host and does not synchronise: 1 + 2 per
    chunk launches on the current stream.  On cpu refresh runs the host twin of the sampler and `host_labels`, which is slow and
    meant for small sets.  Refused: k > min(16, M), rows >= 2^32, and on cuda a pool + manifold + index + workspace larger than the
    free device memory (the message gives the byte count)."""

    def __init__(self, amass_dir, files, rows, options=None, datasets=None, device="cpu", chunk=65536, num_joints=21):
        J = _check_joints(num_joints)
        man_files = []
        for ds in _subdirs(amass_dir, datasets):
            man_files += sorted(glob.glob(os.path.join(amass_dir, ds, "*.npz")))
        if not man_files:
            raise FileNotFoundError(f"no manifold files <dataset>/*.npz under {amass_dir}")
        mans = []
        for f in man_files:
            with np.load(f) as z:
                if "pose" not in z.files:
                    raise ValueError(f"{f}: a manifold file holds `pose`, this one {sorted(z.files)}")
                mans.append(self._pose(f, z["pose"], J))
        self._init_online(mans, man_files, files, rows, options, device, chunk, J)

    @classmethod
    def from_manifold(cls, mans, files, rows, options=None, device="cpu", chunk=65536, num_joints=21):
        """the same from a list of arrays [n,J,4], one entry per manifold file (tests, benchmarks)"""
        self = cls.__new__(cls)
        J = _check_joints(num_joints)
        names = [f"<manifold {i}>" for i in range(len(mans))]
        self._init_online([cls._pose(n, p, J) for n, p in zip(names, mans)], names, files, rows, options, device, chunk, J)
        return self

    def _init_online(self, mans, man_files, files, rows, options, device, chunk, num_joints=21):
        self.options = options or OnlineOptions()
        J = self.num_joints = _check_joints(num_joints, self.options.weighted)
        F, R, k = int(files), int(rows), int(self.options.k)
        if F < 1 or R < 1:
            raise ValueError(f"an online pool needs files >= 1 and rows >= 1, got {F} x {R}")
        if R >= 2 ** 32:
            raise ValueError(f"rows = {R}: the trainer's sampler draws 32-bit words")
        self.man_files = list(man_files)
        self.files = [f"<online {i}>" for i in range(F)]
        self.rows = R
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.man_off = np.concatenate([[0], np.cumsum([len(p) for p in mans])]).astype(np.int64)
        self.file_off = (np.arange(F + 1, dtype=np.int64) * R)
        P, M = F * R, int(self.man_off[-1])
        if M >= 2 ** 31:
            raise ValueError(f"the manifold holds {M} poses, the index and the sampler take fewer than 2^31")
        if not 1 <= k <= min(16, M):
            raise ValueError(f"k = {k}: the labels are the 1 .. min(16, M = {M}) nearest manifold poses")
        if self.options.metric not in ("geo", "euc"):
            raise PndfError(f"unknown metric {self.options.metric!r} (geo, euc)")
        self.k = k
        self.chunk = max(1, min(int(chunk), P))
        self._lib = load_library()
        self.options.opts(0, 0, self._lib)                       # refuses bad sigmas / shares / noise here, not at the first refresh
        self.nbytes = 4 * (P * 4 * J + P * k + M * 4 * J) + 8 * (P * k + P) + 4 * P + 8 * (len(self.file_off) + len(self.man_off))
        hip = self.device.type == "cuda"
        if hip:
            # the plan of a search depends on its query count: the workspace must hold a full chunk and the last, shorter one
            sizes = sorted({self.chunk, P % self.chunk} - {0})
            index_bytes = -(-M // KNN_TILE) * knn_tile_bytes(J)
            ws_bound = max(self._plan_bytes(Q, M, k) for Q in sizes)
            need = self.nbytes + index_bytes + ws_bound
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > free:
                raise MemoryError(f"the online pool, the manifold, its index and the search workspace need {need} bytes on {self.device}, "
                                  f"{free} are free: a data set larger than device memory is not supported")
        dev = self.device
        self.man = torch.from_numpy(np.concatenate(mans)).to(dev)
        self.pose = torch.zeros(P, J, 4, dtype=torch.float32, device=dev)
        self.dist = torch.zeros(P, k, dtype=torch.float32, device=dev)
        self.nn_idx = torch.zeros(P, k, dtype=torch.int64, device=dev)
        self.src = torch.zeros(P, dtype=torch.int64, device=dev)
        self.group = torch.zeros(P, dtype=torch.int32, device=dev)
        self.file_off_t = torch.from_numpy(self.file_off).to(dev)
        self.man_off_t = torch.from_numpy(self.man_off).to(dev)
        self.draw = self.seed = None
        self._index = self._ws = None
        if hip:
            from .knn import PoseIndex
            self._index = PoseIndex(self.man, metric=self.options.metric, weighted=self.options.weighted, device=dev, num_joints=J)._index
            ws = max(self._index.workspace_bytes(Q, k) for Q in sizes)
            self._ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=dev)
            self.nbytes += index_bytes + ws

    @staticmethod
    def _plan_bytes(Q, M, k):
        """an upper bound of pndf_knn_workspace_bytes before the index exists: at most 2,048 + Q / 128 (query block, split) pairs
        of 128 queries x 16 slots x 8 bytes"""
        return (2048 + -(-Q // 128)) * 128 * 16 * 8

    def refresh(self, draw, seed=0):
        """pose, src, group <- pool (seed, draw); dist, nn_idx <- its exact k nearest manifold poses.  On cuda: enqueued on the
        current stream, nothing allocated, nothing copied from the host, no synchronisation."""
        draw, seed = int(draw), int(seed)
        P = self.pose.shape[0]
        opt = self.options.opts(seed, draw, self._lib)
        _sample_into(self.man, 0, P, opt, self.pose, self.src, self.group, self._lib)
        if self._index is not None:
            with torch.cuda.device(self.device):
                stream = stream_handle(self.device)
                for s in range(0, P, self.chunk):
                    c = min(self.chunk, P - s)
                    self._index.search(self.pose.data_ptr() + 16 * self.num_joints * s, c, self.k, self.dist.data_ptr() + 4 * self.k * s,
                                       self.nn_idx.data_ptr() + 8 * self.k * s, self._ws.data_ptr(), stream)
        else:
            host_labels(self.pose, self.man, self.k, self.options.metric, self.options.weighted, self.dist, self.nn_idx)
        self.draw, self.seed = draw, seed
