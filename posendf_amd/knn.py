"""Exact k-nearest-pose search on the HIP engine (csrc/pndf_knn.hip, `pndf_knn_*` of include/posendf_amd.h): the search the
reference's data/prepare_traindata.py runs as a FAISS joint-space prefilter (`faiss_model.search`, :152) followed by the exact
geodesic top-k among the candidates (`dist_calc`, :159), done here exactly over the whole database:

    index = PoseIndex(poses[N,21,4], metric="geo")      # or "euc"; weighted=True uses the joint-rank weights
    vals, idx = index.search(queries[Q,21,4], k=5)      # float32 [Q,k] ascending, int64 [Q,k]

The metric and the semantics are those of `dist_utils.geo / euc` (pndf_quat_topk): ties go to the lower database index, a NaN
distance is never selected (missing slots: NaN / -1), 1 <= k <= min(16, N).  The index owns a packed copy of the poses, so
the tensor it was built from may be freed or overwritten afterwards.  No CPU fallback.
"""
from __future__ import annotations

import torch

from .dist_utils import JOINT_RANK
from .engine import KnnIndex, PndfError, stream_handle


class PoseIndex:
    def __init__(self, poses, metric: str = "geo", weighted: bool = False, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PndfError(f"PoseIndex runs on a gfx950 device, not {self.device} (no CPU fallback)")
        p = torch.as_tensor(poses).to(self.device, torch.float32).reshape(-1, 21, 4).contiguous()
        self.metric = metric
        self.weighted = weighted
        w = None
        if weighted:
            rank = torch.tensor(JOINT_RANK, dtype=torch.float32)
            w = torch.nn.functional.normalize(rank, dim=0).tolist()                # dist_utils.py:18,41
        with torch.cuda.device(self.device):
            self._index = KnnIndex(p.data_ptr(), p.shape[0], metric, w, stream_handle(self.device))

    def __len__(self) -> int:
        return self._index.size()

    def search(self, queries, k: int = 5):
        """-> (vals float32 [Q,k], idx int64 [Q,k]) on the index's device, enqueued on the current stream."""
        q = torch.as_tensor(queries).to(self.device, torch.float32).reshape(-1, 21, 4).contiguous()
        Q = q.shape[0]
        k = int(k)
        with torch.cuda.device(self.device):
            nbytes = self._index.workspace_bytes(Q, k)
            vals = torch.empty(Q, k, dtype=torch.float32, device=self.device)
            idx = torch.empty(Q, k, dtype=torch.int64, device=self.device)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
            self._index.search(q.data_ptr(), Q, k, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), stream_handle(self.device))
        return vals, idx
