"""Training data for PoseNDF on the GPU: the replacement of the reference's data/prepare_traindata.py.

    python -m posendf_amd.traindata --raw_data <dir> --out_dir <dir> --seq_file <dataset>/<seq>.npz [--manifold_dir <dir>]

Database: every `<raw_data>/<dataset>/*.npz` of the named datasets (`--datasets`, default every subdirectory), key `pose_body`
(axis-angle [n,63] or [n,69]; the first 21 joints), converted to quaternions.  Queries: noisy poses drawn from the sequence file
exactly as data/create_data.py:PoseData.__getitem__ (:82-94, mode='query') draws them, `--runs` items of `--num_samples` poses.
Labels: the exact k nearest database poses of every query under the reference's metric (posendf_amd.knn.PoseIndex).  Output
`<out_dir>/<seq_file>` holds what model/load_data.py:44-71 reads: `pose` [n,21,4], `dist` [n,k], `nn_pose` [n,k,21,3] (the
neighbours' axis-angle, as the reference stores it), plus `nn_idx` [n,k] int64.  `--manifold_dir` also writes every database
file's quaternions under key `pose` (`man_poses` of load_data.py:57-61).

Another skeleton: `--num_joints J` (1 .. 32) reads the first 3 J columns of `pose_body` as J axis-angle joints and writes `pose`
[n,J,4], `nn_pose` [n,k,J,3]: the files `PoseDataset(num_joints=J)` loads.  With 21 the numpy stream and the output are what they
were.

Kept from the reference's sampler, on purpose:
  * one `rand(21, 4)` draw per sigma group is added to every pose of the group: the noise is shared within a group;
  * the noise is U[0, 1) (`np.random.rand`), not zero-mean;
  * the reference's 12-worker DataLoader has no `worker_init_fn`, so its workers repeat one numpy stream; here every item is
    drawn from one seeded stream (`--seed`), in order.
Difference: the reference's labels are the top-k among 500 candidates of a FAISS search in SMPL joint space (that prefilter
needs the SMPL model files and is out of scope); these are the exact top-k over the whole database, so per query each of our k
distances is <= the reference's.
Difference on the reading side (posendf_amd.trainer): with `data.flip` the reference's loader (model/load_data.py:63) flips
the noisy poses where it means the manifold poses, so its manifold batch becomes a copy of the noisy one; the trainer here flips
the manifold poses themselves.
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np

SIGMA = (0.01, 0.05, 0.1, 0.25, 0.5)                     # create_data.py:49
SAMPLE_DISTRIBUTION = (0.2, 0.2, 0.2, 0.2, 0.2)          # create_data.py:50


def group_sizes(num_samples: int) -> np.ndarray:
    """rint(num_samples * 0.2) poses per sigma group (create_data.py:53); refuses a count whose shares do not add up, which
    the reference's own assert (:94) rejects."""
    sizes = np.rint(num_samples * np.array(SAMPLE_DISTRIBUTION)).astype(np.uint32)
    if int(sizes.sum()) != int(num_samples):
        raise ValueError(f"num_samples = {num_samples}: the five groups of rint({num_samples} * 0.2) = {int(sizes[0])} poses "
                         f"add up to {int(sizes.sum())}, not {num_samples} (the reference asserts the same); use a multiple of 5")
    return sizes


def sample_queries(quat_pose: np.ndarray, num_samples: int, rng: np.random.RandomState) -> np.ndarray:
    """One item of create_data.py:PoseData.__getitem__ in mode 'query' (:82-94): quat_pose float32 [n,J,4] -> float64
    [num_samples,J,4], consuming `rng` in the reference's order (one rand(J, 4) per sigma group; J = 21 there)."""
    out = []
    for i, num in enumerate(group_sizes(num_samples)):
        indices = rng.randint(0, len(quat_pose), num)
        sampled = quat_pose[indices] + SIGMA[i] * rng.rand(quat_pose.shape[1], 4)
        sampled = sampled / np.linalg.norm(sampled, axis=2, keepdims=True)
        out.extend(sampled)
    return np.array(out)


def aa_to_quat(aa: np.ndarray):
    """axis-angle [n,J,3] -> quaternions [n,J,4] (real part first) with the engine's conversion (motion_denoise), on the
    host in float32 as the reference converts (create_data.py:33-37)"""
    import torch
    from .motion_denoise import axis_angle_to_quaternion
    return axis_angle_to_quaternion(torch.from_numpy(np.ascontiguousarray(aa, dtype=np.float32)))


def load_pose_body(path: str, num_joints: int = 21) -> np.ndarray:
    """`pose_body` of a VPoser-style file -> float32 [n,J,3] (the first 3 J values; 63 for the 21 joints of create_data.py:72-73)"""
    J = int(num_joints)
    if not 1 <= J <= 32:
        raise ValueError(f"num_joints = {J}: 1 .. 32 joints")
    p = np.load(path)["pose_body"].astype(np.float32)
    if p.ndim != 2 or p.shape[1] < 3 * J:
        raise ValueError(f"{path}: pose_body is {p.shape}, {J} joints need [n, >= {3 * J}]")
    p = p[:, :3 * J]
    return p.reshape(len(p), J, 3)


def database_files(raw_data: str, datasets=None):
    if not datasets:
        datasets = sorted(d for d in os.listdir(raw_data) if os.path.isdir(os.path.join(raw_data, d)))
    files = []
    for ds in datasets:
        files += sorted(glob.glob(os.path.join(raw_data, ds, "*.npz")))
    return files


def make_queries(seq_file: str, num_samples: int, runs: int, seed: int, num_joints: int = 21) -> np.ndarray:
    """`runs` items of the reference's sampler from one seeded stream -> float64 [runs * num_samples, J, 4]"""
    group_sizes(num_samples)
    quat = aa_to_quat(load_pose_body(seq_file, num_joints)).numpy()
    rng = np.random.RandomState(seed)
    return np.concatenate([sample_queries(quat, num_samples, rng) for _ in range(runs)], axis=0)


def generate(raw_data, out_dir, seq_file, metric="geo", num_samples=100, k_dist=5, batch_size=65536, runs=1000, seed=0,
             weighted=False, datasets=None, manifold_dir=None, device="cuda:0", num_joints=21):
    """Writes <out_dir>/<seq_file> (and, with manifold_dir, the database's quaternions); returns the output path."""
    import torch
    from .knn import PoseIndex, joint_weights
    joint_weights(num_joints, weighted)      # refuses --weighted with another joint count than 21 before anything is read
    seq_path = os.path.join(raw_data, seq_file)
    if not os.path.exists(seq_path):
        raise FileNotFoundError(f"missing sequence file {seq_path}")
    queries = make_queries(seq_path, num_samples, runs, seed, num_joints)
    files = database_files(raw_data, datasets)
    if not files:
        raise FileNotFoundError(f"no database files <dataset>/*.npz under {raw_data}")
    aa = [load_pose_body(f, num_joints) for f in files]
    db_aa = np.concatenate(aa, axis=0)
    db_q = aa_to_quat(db_aa).numpy()
    if manifold_dir:
        o = 0
        for f, a in zip(files, aa):
            dst = os.path.join(manifold_dir, os.path.relpath(f, raw_data))
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            np.savez(dst, pose=db_q[o:o + len(a)])
            o += len(a)
    index = PoseIndex(db_q, metric=metric, weighted=weighted, device=device, num_joints=num_joints)
    del db_q
    pose = queries.astype(np.float32)
    dist = np.empty((len(pose), k_dist), np.float32)
    nn_idx = np.empty((len(pose), k_dist), np.int64)
    for s in range(0, len(pose), batch_size):
        v, i = index.search(torch.from_numpy(pose[s:s + batch_size]), k_dist)
        dist[s:s + batch_size] = v.cpu().numpy()
        nn_idx[s:s + batch_size] = i.cpu().numpy()
    nn_pose = db_aa[np.maximum(nn_idx, 0)]
    nn_pose[nn_idx < 0] = np.nan
    out = os.path.join(out_dir, seq_file)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    np.savez(out, pose=pose, dist=dist, nn_pose=nn_pose.astype(np.float32), nn_idx=nn_idx)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="PoseNDF training data: noisy poses and their exact k nearest database poses")
    ap.add_argument("-rd", "--raw_data", required=True, help="<raw_data>/<dataset>/*.npz with key pose_body")
    ap.add_argument("-od", "--out_dir", required=True)
    ap.add_argument("-sf", "--seq_file", required=True, help="the query sequence, relative to --raw_data")
    ap.add_argument("-m", "--metric", default="geo", choices=("geo", "euc"))
    ap.add_argument("-n", "--num_samples", type=int, default=100, help="poses per item (a multiple of 5)")
    ap.add_argument("-k", "--k_dist", type=int, default=5, help="nearest neighbours per query (1 .. 16)")
    ap.add_argument("-bs", "--batch_size", type=int, default=65536, help="queries per search call")
    ap.add_argument("--runs", type=int, default=1000, help="items drawn from the sequence (create_data.py:45)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weighted", action="store_true", help="joint-rank weights (dist_utils.py:17-18)")
    ap.add_argument("--datasets", nargs="*", default=None, help="database subdirectories of --raw_data (default: all)")
    ap.add_argument("--manifold_dir", default=None, help="also write each database file's quaternions (key pose) here")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--num_joints", type=int, default=21, help="joints per pose (1 .. 32): the first 3 J columns of pose_body")
    a = ap.parse_args(argv)
    out = generate(a.raw_data, a.out_dir, a.seq_file, a.metric, a.num_samples, a.k_dist, a.batch_size, a.runs, a.seed,
                   a.weighted, a.datasets, a.manifold_dir, a.device, a.num_joints)
    print("wrote", out)


if __name__ == "__main__":
    main()
