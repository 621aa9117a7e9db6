"""Exact k-nearest-pose search on the HIP engine (csrc/pndf_knn.hip, `pndf_knn_*` of include/posendf_amd.h): the search the
reference's data/prepare_traindata.py runs as a FAISS joint-space prefilter (`faiss_model.search`, :152) followed by the exact
geodesic top-k among the candidates (`dist_calc`, :159), done here exactly over the whole database:

    index = PoseIndex(poses[N,21,4], metric="geo")      # or "euc"; weighted=True uses the joint-rank weights
    vals, idx = index.search(queries[Q,21,4], k=5)      # float32 [Q,k] ascending, int64 [Q,k]
    hand = PoseIndex(poses[N,15,4], num_joints=15)      # any joint count 1 .. 32 (include/posendf_amd_skeleton_data.h);
                                                        # weights=[J positive floats] in place of the default 1/J each

The metric and the semantics are those of `dist_utils.geo / euc` (pndf_quat_topk): ties go to the lower database index, a NaN
distance is never selected (missing slots: NaN / -1), 1 <= k <= min(16, N).  The index owns a packed copy of the poses, so
the tensor it was built from may be freed or overwritten afterwards.  No CPU fallback.
"""
from __future__ import annotations

import torch

from .dist_utils import JOINT_RANK
from .engine import KnnIndex, PndfError, stream_handle


def joint_weights(num_joints: int, weighted: bool = False, weights=None):
    """The per-joint weights of a distance over `num_joints` joints as a list of floats, or None for the default 1 / J each:
    `weighted` = the L2-normalised SMPL joint ranks (dist_utils.py:18,41; 21 joints only), `weights` = J positive finite
    floats of the caller's.  ValueError for a joint count outside 1 .. 32, both at once, `weighted` with another joint count
    than 21, a wrong length or a weight that is not finite and > 0."""
    J = int(num_joints)
    if not 1 <= J <= 32:
        raise ValueError(f"num_joints = {J}: the index takes 1 .. 32 joints")
    if weighted and weights is not None:
        raise ValueError("weighted=True is the SMPL joint-rank vector: pass it or `weights`, not both")
    if weighted:
        if J != 21:
            raise ValueError(f"weighted=True is the joint-rank vector of the 21 SMPL joints; with num_joints = {J} pass `weights`")
        rank = torch.tensor(JOINT_RANK, dtype=torch.float32)
        return torch.nn.functional.normalize(rank, dim=0).tolist()                 # dist_utils.py:18,41
    if weights is None:
        return None
    w = [float(x) for x in torch.as_tensor(weights, dtype=torch.float32).reshape(-1).tolist()]
    if len(w) != J:
        raise ValueError(f"{len(w)} weights for {J} joints")
    if not all(x > 0.0 and x != float("inf") for x in w):
        raise ValueError("joint weights must be finite and > 0")
    return w


class PoseIndex:
    def __init__(self, poses, metric: str = "geo", weighted: bool = False, device="cuda:0", num_joints: int = 21, weights=None):
        J = int(num_joints)
        w = joint_weights(J, weighted, weights)      # (the argument refusals come before the device is touched)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PndfError(f"PoseIndex runs on a gfx950 device, not {self.device} (no CPU fallback)")
        p = torch.as_tensor(poses).to(self.device, torch.float32).reshape(-1, J, 4).contiguous()
        self.metric = metric
        self.weighted = weighted
        self.num_joints = J
        self.weights = w
        with torch.cuda.device(self.device):
            self._index = KnnIndex(p.data_ptr(), p.shape[0], metric, w, stream_handle(self.device), num_joints=J)

    def __len__(self) -> int:
        return self._index.size()

    def search(self, queries, k: int = 5):
        """-> (vals float32 [Q,k], idx int64 [Q,k]) on the index's device, enqueued on the current stream."""
        q = torch.as_tensor(queries).to(self.device, torch.float32).reshape(-1, self.num_joints, 4).contiguous()
        Q = q.shape[0]
        k = int(k)
        with torch.cuda.device(self.device):
            nbytes = self._index.workspace_bytes(Q, k)
            vals = torch.empty(Q, k, dtype=torch.float32, device=self.device)
            idx = torch.empty(Q, k, dtype=torch.int64, device=self.device)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
            self._index.search(q.data_ptr(), Q, k, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), stream_handle(self.device))
        return vals, idx
