"""Test helper (not a test module) for the training data of other skeletons (include/posendf_amd_skeleton_data.h; DESIGN.md section
2u): shared by tests/golden/make_golden_skeleton_knn.py, tests/test_skeleton_data.py and tests/test_skeleton_data_gpu.py.

The inputs are tests/knn_oracle.knn_inputs generalised to J joints, the distance matrix is restated in fp64 for J joints and any weight
vector, the acceptance is tests/knn_oracle.check_knn as it is; the sampler is tests/online_oracle.sample restated for J joints (block
1 + j for joint j), with that module's Philox.  The skeletons are tests/skeleton_oracle.py's."""
import ctypes

import numpy as np

import knn_oracle as ko
import online_oracle as oo
import skeleton_oracle as sko

JOINTS = {name: len(parents) for name, parents in sko.SKELETONS.items()}      # hand 15, tree32 / chain32 32, one 1, roots5 5
HAND_J = len(sko.HAND)
OK, BAD_ARG, NO_DEVICE = 0, -1, -6


# ---- the search --------------------------------------------------------------------------------------------------------------------
def knn_inputs(Q: int, N: int, J: int, seed: int):
    """knn_oracle.knn_inputs for J joints -> (queries [Q,J,4], database [N,J,4]) float32; the same arrays for J = 21"""
    from posendf_amd import synth
    db = synth.make_poses(N, seed=seed, signed=True, num_joints=J)
    rng = np.random.default_rng([seed, 7])
    src = rng.integers(0, N, Q)
    scale = rng.choice([0.01, 0.05, 0.2, 1.0], size=(Q, 1, 1))
    q = db[src].astype(np.float64) + scale * rng.normal(size=(Q, J, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    return q.astype(np.float32), db


def all_distances(queries, db, metric, weights=None, budget=2 ** 18):
    """fp64 distances of every query [Q,J,4] to every database pose [N,J,4] -> [Q,N]: sum_j w_j (1 - |<q_j, p_j>|) (geo) or
    sum_j w_j ||q_j - p_j|| (euc), w_j = 1 / J (the mean) without `weights`"""
    q, p = np.asarray(queries, np.float64), np.asarray(db, np.float64)
    J = q.shape[1]
    w = None if weights is None else np.asarray(weights, np.float32).astype(np.float64).reshape(J)      # the index holds fp32 weights
    out = np.empty((len(q), len(p)), np.float64)
    step = max(1, budget // max(len(p), 1))
    for s in range(0, len(q), step):
        n = q[s:s + step, None]
        if metric == "geo":
            per_joint = 1.0 - np.abs(np.einsum("cjd,mjd->cmj", n[:, 0], p))
        elif metric == "euc":
            d = n - p[None]
            per_joint = np.sqrt((d * d).sum(axis=3))
        else:
            raise ValueError(metric)
        out[s:s + step] = per_joint.mean(axis=2) if w is None else (per_joint * w).sum(axis=2)
    return out


def clear_rows(D, k, gap=1e-6):
    """the rows check_knn compares neighbour sets on: the oracle's k-th and (k+1)-th distances differ by more than `gap`"""
    if D.shape[1] <= k:
        return np.ones(len(D), bool)
    srt = np.partition(D, k, axis=1)[:, :k + 1]
    srt.sort(axis=1)
    return srt[:, k] - srt[:, k - 1] > gap


def check_case(results, D):
    """One case = one (J, Q, N, metric) with its searches `results` = [(vals, idx, k), ...]: knn_oracle.check_knn as it is on every
    search, under the condition that its gap rule skips at most 1 in 64 of the case's rows (Q per k).  Measured on the fp64 oracle
    alone over the cases of tests/test_skeleton_data_gpu.py: one row skipped in two of them -- J = 15, 130 x 4097, euc, k = 16 (1 of
    390 rows) and J = 2, 33 x 1000, euc, k = 16 (1 of 99) -- and none elsewhere."""
    skipped = sum(int((~clear_rows(D, k)).sum()) for _, _, k in results)
    rows = len(D) * len(results)
    assert skipped * 64 <= rows, (skipped, rows)
    for vals, idx, k in results:
        ko.check_knn(vals, idx, D, k)


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def manifold(N, J, seed=21):
    from posendf_amd import synth
    return synth.make_poses(N, seed=seed, signed=True, num_joints=J)


def sample(man, first, count, seed, draw, sigmas, cum, noise):
    """online_oracle.sample for man [N,J,4] -> (q float32 [count,J,4], src, group): fp64, rounded once at the end"""
    man = np.asarray(man, np.float32)
    J = man.shape[1]
    src, group = oo.picks(len(man), first, count, seed, draw, cum)
    idx = np.int64(first) + np.arange(count, dtype=np.int64)
    w = oo.blocks(seed, draw, idx[:, None], 1 + np.arange(J)[None, :])               # [count, J, 4]
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    n = 2.0 * u - 1.0 if noise else u
    sig = np.asarray(sigmas, np.float32).astype(np.float64)[group]
    Q = man[src].astype(np.float64)
    x = Q + sig[:, None, None] * n
    s = (x * x).sum(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((s > 0) & np.isfinite(s), x / np.sqrt(s), Q)
    return out.astype(np.float32), src, group


def oracle_of(man, first, count, opt):
    n = opt.n_sigma
    return sample(man, first, count, opt.seed, opt.draw, list(opt.sigma[:n]), list(opt.cum[:n]), opt.noise)


def skel_twin(lib, man, first, count, opt):
    """pndf_skel_online_sample_cpu over man [N,J,4] -> (q, src, group); the buffers start poisoned"""
    J = man.shape[1]
    q = np.full((count, J, 4), 7.0, np.float32)
    src = np.full(count, -5, np.int64)
    group = np.full(count, -5, np.int32)
    rc = lib.pndf_skel_online_sample_cpu(man.ctypes.data, len(man), J, first, count, ctypes.byref(opt), q.ctypes.data, src.ctypes.data,
                                         group.ctypes.data)
    assert rc == 0, (rc, lib.pndf_cpu_last_error(None))
    return q, src, group


def same_bits(a, b):
    """(q, src, group) triples: every array bit for bit"""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and x.shape == y.shape
               for x, y in zip(a, b))


# ---- the hand's online data set and trainer --------------------------------------------------------------------------------------
def hand_manifolds(rows=(200, 100), seed=4200):
    return [manifold(n, HAND_J, seed + i) for i, n in enumerate(rows)]


def hand_online_trainer(root, device="cpu", files=3, rows=48, seed=0, engine_train=None, **kw):
    """Trainer on the 15-joint hand (tests/skeleton_train_fixtures.trainer_config) over an OnlinePoseDataset passed as dataset="""
    import skeleton_train_fixtures as stf
    from posendf_amd.online import OnlinePoseDataset
    from posendf_amd.trainer import Trainer
    ds = OnlinePoseDataset.from_manifold(hand_manifolds(), files, rows, device=device, num_joints=HAND_J)
    cfg = stf.trainer_config(root, device=device, **kw)
    if engine_train:
        cfg["engine"] = {"train": engine_train}
    return Trainer(cfg, seed=seed, dataset=ds)
