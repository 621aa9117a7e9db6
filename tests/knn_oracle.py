"""Test helper (not a test module) for the exact k-nearest-pose search (posendf_amd.knn, csrc/pndf_knn.hip) and the training-data
generator (posendf_amd.traindata): seeded inputs, and the brute-force oracle built on oracle.quat_dist_np.pose_distances."""
import numpy as np

from oracle.quat_dist_np import pose_distances
from posendf_amd import synth


def knn_inputs(Q: int, N: int, seed: int):
    """-> (queries [Q,21,4], database [N,21,4]) float32: full-sphere unit quaternions; every query is a database pose with noise
    of a seeded scale (some close, some far), so the nearest distances spread from near 0 to the bulk."""
    db = synth.make_poses(N, seed=seed, signed=True)
    rng = np.random.default_rng([seed, 7])
    src = rng.integers(0, N, Q)
    scale = rng.choice([0.01, 0.05, 0.2, 1.0], size=(Q, 1, 1))
    q = db[src].astype(np.float64) + scale * rng.normal(size=(Q, 21, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    return q.astype(np.float32), db


def all_distances(queries, db, metric, weighted, budget=2 ** 18):
    """fp64 distances of every query to every database pose: [Q,N] (pose_distances on blocks of about `budget` pairs)"""
    Q, N = len(queries), len(db)
    out = np.empty((Q, N), np.float64)
    step = max(1, budget // max(N, 1))
    for s in range(0, Q, step):
        q = queries[s:s + step]
        for n0 in range(0, N, budget):
            v = np.broadcast_to(db[None, n0:n0 + budget], (len(q),) + db[n0:n0 + budget].shape)
            out[s:s + step, n0:n0 + budget] = pose_distances(q, v, metric, weighted, dtype=np.float64)
    return out


def brute_force(D, k):
    """-> (values [Q,k], indices [Q,k]) of a distance matrix: ascending, ties to the lower index, NaN last"""
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(D, order, axis=1), order


def check_knn(vals, idx, D, k, rtol=5e-6, atol=5e-7, gap=1e-6):
    """The acceptance of the search against the fp64 distance matrix D: values within rtol / atol, every returned index has its
    returned value, and the neighbour set is the oracle's wherever the oracle's k-th and (k+1)-th distances differ by > gap."""
    vals, idx = np.asarray(vals), np.asarray(idx)
    want_v, want_i = brute_force(D, k)
    assert vals.shape == want_v.shape and idx.shape == want_i.shape
    np.testing.assert_allclose(vals, want_v, rtol=rtol, atol=atol)
    np.testing.assert_allclose(np.take_along_axis(D, idx, axis=1), vals, rtol=rtol, atol=atol)
    if D.shape[1] > k:
        srt = np.partition(D, k, axis=1)[:, :k + 1]
        srt.sort(axis=1)
        clear = srt[:, k] - srt[:, k - 1] > gap
    else:
        clear = np.ones(len(D), bool)
    for r in np.nonzero(clear)[0]:
        assert set(idx[r].tolist()) == set(want_i[r].tolist()), r


def make_pose_body(n: int, seed: int, width: int = 63) -> np.ndarray:
    """A synthetic VPoser-style `pose_body` array [n, width] float32 (axis-angle, smooth in time like a motion sequence)"""
    rng = np.random.default_rng([seed, 11])
    walk = np.cumsum(rng.normal(scale=0.05, size=(n, width)), axis=0)
    return (0.4 * rng.normal(size=(1, width)) + walk).astype(np.float32)
