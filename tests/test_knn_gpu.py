"""GPU checks of the exact k-nearest-pose search (posendf_amd.knn.PoseIndex, csrc/pndf_knn.hip) against the reference's vectors
and the fp64 brute force, its edge cases and its plan independence, and of the training-data generator end to end."""
import os

import numpy as np
import pytest

from knn_oracle import all_distances, check_knn, knn_inputs, make_pose_body

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
VARIANTS = [("geo", False), ("geo", True), ("euc", False), ("euc", True)]


def _index(db, metric="geo", weighted=False):
    from posendf_amd.knn import PoseIndex
    return PoseIndex(db, metric=metric, weighted=weighted, device="cuda:0")


def _search(index, q, k):
    v, i = index.search(q, k)
    assert v.dtype.is_floating_point and str(i.dtype) == "torch.int64"
    return v.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("metric,weighted", VARIANTS)
def test_matches_reference_vectors(metric, weighted):
    g = np.load(os.path.join(HERE, "golden", "knn_ref.npz"))
    tag = f"{metric}_{'w' if weighted else 'u'}"
    q, db = knn_inputs(16, 2000, 5)
    v, i = _search(_index(db, metric, weighted), q, 5)
    ref_v, ref_i = g[tag + "_val"], g[tag + "_idx"]
    np.testing.assert_allclose(v, ref_v, rtol=5e-6, atol=5e-7)
    distinct = np.ones_like(ref_i, dtype=bool)
    distinct[:, 1:] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    distinct[:, :-1] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    assert (i[distinct] == ref_i[distinct]).all()


@pytest.mark.parametrize("Q,N", [(1, 1), (1, 17), (15, 1000), (17, 4097), (300, 50000), (3, 1000003)])
@pytest.mark.parametrize("metric,weighted", VARIANTS)
def test_matches_fp64_brute_force(Q, N, metric, weighted):
    q, db = knn_inputs(Q, N, seed=Q + N)
    D = all_distances(q, db, metric, weighted)
    index = _index(db, metric, weighted)
    assert len(index) == N
    for k in (1, 5, 16):
        if k > N:
            continue
        v, i = _search(index, q, k)
        check_knn(v, i, D, k)


def test_planted_poses():
    """exact copies (0), antipodal copies (geo 0, euc 2/21 per joint), duplicates (the lower index wins)"""
    q, db = knn_inputs(4, 5000, seed=9)
    db = db.copy()
    db[4321] = q[0]
    db[77] = q[1]
    db[4000] = q[1]                      # duplicate: 77 wins
    db[1234] = -q[2]                     # antipodal
    db[4999] = q[3]
    for metric in ("geo", "euc"):
        v, i = _search(_index(db, metric), q, 3)
        assert i[0, 0] == 4321 and i[1, 0] == 77 and i[1, 1] == 4000 and i[3, 0] == 4999
        assert np.abs(v[[0, 1, 3], 0]).max() < 1e-6 and v[1, 1] == v[1, 0]
        if metric == "geo":
            assert i[2, 0] == 1234 and abs(v[2, 0]) < 1e-6


def test_planted_poses_past_2gb():
    """N x 336 B > 2^31: 64-bit offsets; copies at the last indices are found"""
    import torch
    N, Q = 6_600_000, 8
    g = torch.Generator(device="cuda").manual_seed(3)
    db = torch.rand(N, 21, 4, device="cuda", generator=g) * 2 - 1
    db = db / db.norm(dim=2, keepdim=True)
    q = db[torch.arange(Q, device="cuda") * 1000].flip(2)           # new poses
    targets = [N - 1, N - 2, N - 17, N - 100, 3, N // 2, N - 5, N - 3]
    db[targets] = q
    for metric in ("geo", "euc"):
        index = _index(db, metric)
        v, i = _search(index, q, 2)
        assert i[:, 0].tolist() == targets and np.abs(v[:, 0]).max() < 1e-6
        assert (i[:, 1] != i[:, 0]).all()
        del index


def test_edge_cases():
    import torch
    from posendf_amd.engine import PndfError
    q, db = knn_inputs(6, 12, seed=4)
    db = db.copy()
    db[5] = np.nan
    db[7, 3] = np.nan
    D = all_distances(q, db, "geo", False)
    v, i = _search(_index(db), q, 12)           # k = N: every finite pose, then NaN / -1
    assert (i[:, :10] >= 0).all() and not np.isin(i[:, :10], [5, 7]).any()
    assert np.isnan(v[:, 10:]).all() and (i[:, 10:] == -1).all()
    fin = np.isfinite(D)
    check_knn(v[:, :10], i[:, :10], np.where(fin, D, np.inf), 10)
    q2, db2 = knn_inputs(3, 16, seed=2)
    index = _index(db2, "euc")
    v, i = _search(index, q2, 16)
    assert (np.sort(i, axis=1) == np.arange(16)).all()
    v0, i0 = index.search(torch.empty(0, 21, 4), 5)          # Q = 0
    assert v0.shape == (0, 5) and i0.shape == (0, 5)
    for k in (17, 0, -1):
        with pytest.raises(PndfError):
            index.search(q2, k)
    with pytest.raises(PndfError):
        _index(db2[:4]).search(q2, 5)                        # k > N


def test_plan_independence():
    import torch
    q, db = knn_inputs(4096, 1_000_003, seed=8)
    for metric in ("geo", "euc"):
        index = _index(db, metric)
        v, i = _search(index, q, 5)
        v2, i2 = _search(index, q, 5)
        assert (v.view(np.uint32) == v2.view(np.uint32)).all() and (i == i2).all()
        parts = [_search(index, q[s:s + 1000], 5) for s in range(0, len(q), 1000)]
        assert (np.concatenate([p[0] for p in parts]).view(np.uint32) == v.view(np.uint32)).all()
        assert (np.concatenate([p[1] for p in parts]) == i).all()
        for r in range(0, 4096, 64):                         # Q = 1: the widest database split
            v1, i1 = _search(index, q[r:r + 1], 5)
            assert (v1.view(np.uint32) == v[r:r + 1].view(np.uint32)).all() and (i1 == i[r:r + 1]).all()
        torch.cuda.synchronize()


def test_index_owns_its_copy_and_streams():
    import torch
    q, db = knn_inputs(40, 3000, seed=6)
    src = torch.from_numpy(db).cuda()
    from posendf_amd.knn import PoseIndex
    index = PoseIndex(src, metric="geo")
    src.fill_(0.5)                                           # the caller overwrites its tensor
    del src
    D = all_distances(q, db, "geo", False)
    v, i = _search(index, q, 5)
    check_knn(v, i, D, 5)
    s = torch.cuda.Stream()
    qt = torch.from_numpy(q).cuda()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s):
        vs, is_ = index.search(qt, 5)
    s.synchronize()
    assert (vs.cpu().numpy() == v).all() and (is_.cpu().numpy() == i).all()


def test_traindata_end_to_end(tmp_path):
    import subprocess
    import sys
    import torch
    raw = tmp_path / "raw"
    for ds, files in (("DS_A", 2), ("DS_B", 1)):
        os.makedirs(raw / ds)
        for f in range(files):
            np.savez(raw / ds / f"seq{f}.npz", pose_body=make_pose_body(400 + 50 * f, seed=10 * len(ds) + f, width=69 if f else 63))
    out, man = tmp_path / "out", tmp_path / "man"
    repo = os.path.dirname(HERE)
    cmd = [sys.executable, "-m", "posendf_amd.traindata", "--raw_data", str(raw), "--out_dir", str(out), "--seq_file", "DS_A/seq0.npz",
           "--num_samples", "45", "--runs", "20", "--seed", "3", "--batch_size", "300", "--manifold_dir", str(man)]
    r = subprocess.run(cmd, cwd=repo, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    f = np.load(out / "DS_A" / "seq0.npz")
    n = 45 * 20
    assert f["pose"].shape == (n, 21, 4) and f["pose"].dtype == np.float32
    assert f["dist"].shape == (n, 5) and f["dist"].dtype == np.float32
    assert f["nn_pose"].shape == (n, 5, 21, 3) and f["nn_idx"].shape == (n, 5) and f["nn_idx"].dtype == np.int64
    from posendf_amd import traindata
    files = traindata.database_files(str(raw))
    db_aa = np.concatenate([traindata.load_pose_body(p) for p in files])
    db = traindata.aa_to_quat(db_aa).numpy()
    rows = np.arange(0, n, 37)
    D = all_distances(f["pose"][rows], db, "geo", False)
    check_knn(f["dist"][rows], f["nn_idx"][rows], D, 5)
    assert (f["nn_pose"] == db_aa[f["nn_idx"]]).all()
    mans = sorted(str(p) for p in man.rglob("*.npz"))
    assert len(mans) == 3
    man_poses = np.concatenate([np.load(p)["pose"] for p in mans])
    assert man_poses.shape == (len(db), 21, 4)
    # one training step consumes pose, mean(dist, 1) and the manifold poses (model/load_data.py:49-61)
    from posendf_amd import engine, synth
    from posendf_amd.train import TrainObjective
    eng = engine.TrainEngine("softplus", 100.0)
    sd = synth.make_weights(0, 2.0, 0.1)
    params = [torch.from_numpy(sd[key]).cuda().requires_grad_(True) for key in engine.state_dict_order()]
    B = 256
    pose = torch.from_numpy(f["pose"][:B]).cuda()
    dist = torch.from_numpy(f["dist"][:B].mean(1)).cuda()
    mp = torch.from_numpy(man_poses[:B]).cuda()
    losses = TrainObjective.apply(eng, pose, dist, mp, 0, True, *params)
    sum(losses).backward()
    assert all(torch.isfinite(p.grad).all() for p in params)
