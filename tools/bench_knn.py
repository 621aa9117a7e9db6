#!/usr/bin/env python3
"""Exact k-nearest-pose search (posendf_amd.knn.PoseIndex, csrc/pndf_knn.hip): pairs/s and FLOP/s of geo and euc, weighted and
unweighted, k = 5, at Q = 65,536 x N = 1,048,576 and the reference's per-file shape Q = 100,000 x N = 4,194,304, against a
chunked PyTorch-ROCm restatement (einsum / broadcast difference + topk) on the same GPU and the same inputs.  HIP events, one
warm-up, median of --reps timed calls.  The PyTorch comparator materialises [q, n, 21] blocks and is timed on the first
--torch_queries queries against the whole database (its time scales with the number of pairs); the two must agree on those
queries.  One JSON line per case.  --num_joints J (1 .. 32) measures the J-joint index (include/posendf_amd_skeleton_data.h), unweighted
only: the joint ranks are SMPL's.   usage: python tools/bench_knn.py [--reps 3] [--shapes 65536x1048576 100000x4194304] [--num_joints 21]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from posendf_amd.dist_utils import JOINT_RANK  # noqa: E402
from posendf_amd.knn import PoseIndex  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
FLOP_PER_JOINT = 8           # per pair and joint: 4 multiply-adds + |.| + weight + sum (168 per pair at 21 joints)


def weights(weighted, J=21):
    if weighted:
        return torch.nn.functional.normalize(torch.tensor(JOINT_RANK, dtype=torch.float32), dim=0).cuda()
    return torch.full((J,), 1.0 / J, device="cuda")


def torch_knn(db, q, k, metric, weighted, cq=512, cn=131072):
    """the PyTorch-ROCm restatement: per block [cq, cn, J] of per-joint terms, weighted sum, running topk"""
    w = weights(weighted, db.shape[1])
    vals, idx = [], []
    for s in range(0, len(q), cq):
        qc = q[s:s + cq]
        bv = torch.full((len(qc), k), float("inf"), device="cuda")
        bi = torch.zeros((len(qc), k), dtype=torch.int64, device="cuda")
        for n0 in range(0, len(db), cn):
            dc = db[n0:n0 + cn]
            if metric == "geo":
                t = 1 - torch.einsum("qjc,njc->qnj", qc, dc).abs()
            else:
                t = (qc[:, None] - dc[None]).square().sum(-1).sqrt()
            d = (t * w).sum(-1)
            v, i = torch.topk(torch.cat([bv, d], 1), k, dim=1, largest=False)
            ci = torch.cat([bi, torch.arange(n0, n0 + len(dc), device="cuda").expand(len(qc), -1)], 1)
            bv, bi = v, torch.gather(ci, 1, i)
        vals.append(bv)
        idx.append(bi)
    return torch.cat(vals), torch.cat(idx)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=["65536x1048576", "100000x4194304"])
    ap.add_argument("--metrics", nargs="*", default=["geo", "euc"])
    ap.add_argument("--torch_queries", type=int, default=1024)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--num_joints", type=int, default=21)
    a = ap.parse_args()
    J = a.num_joints
    g = torch.Generator(device="cuda").manual_seed(0)
    for shape in a.shapes:
        Q, N = (int(x) for x in shape.split("x"))
        db = torch.rand(N, J, 4, device="cuda", generator=g) * 2 - 1
        db /= db.norm(dim=2, keepdim=True)
        q = db[torch.randint(0, N, (Q,), device="cuda", generator=g)] + 0.05 * torch.randn(Q, J, 4, device="cuda", generator=g)
        q /= q.norm(dim=2, keepdim=True)
        for metric in a.metrics:
            for weighted in ((False, True) if J == 21 else (False,)):
                index = PoseIndex(db, metric=metric, weighted=weighted, num_joints=J)
                k = 5
                out = {}
                t, ts = timed(lambda: out.update(r=index.search(q, k)), a.reps)
                vals, idx = out["r"]
                nq = min(a.torch_queries, Q)
                tt, _ = timed(lambda: out.update(t=torch_knn(db, q[:nq], k, metric, weighted)), 1)
                tv, ti = out["t"]
                dv = float((tv - vals[:nq]).abs().max())
                same = float((ti == idx[:nq]).all(1).float().mean())
                pairs = Q * N
                rec = {"tool": "bench_knn", "metric": metric, "weighted": weighted, "num_joints": J, "Q": Q, "N": N, "k": k, "seconds": t,
                       "seconds_all": ts, "pairs_per_s": pairs / t}
                if metric == "geo":
                    rec["flop_per_s"] = pairs * FLOP_PER_JOINT * J / t
                    rec["fraction_of_fp32_mfma_peak"] = pairs * FLOP_PER_JOINT * J / t / PEAK_FP32_MFMA
                rec.update({"torch_queries": nq, "torch_seconds": tt, "torch_pairs_per_s": nq * N / tt,
                            "speedup_vs_torch": (nq * N / tt) and (pairs / t) / (nq * N / tt),
                            "torch_max_abs_diff": dv, "torch_rows_same_idx": same})
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                assert dv < 1e-5, dv
                del index
        del db, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
