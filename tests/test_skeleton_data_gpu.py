"""Training data for other skeletons on an MI355X (include/posendf_amd_skeleton_data.h): the J-joint search
against the fp64 brute force and the reference's vectors, the 21-joint instantiation against pndf_knn_create bit for bit, planted
poses, plan independence, the J-joint sampler against its host twin, and the online hand data set, its trainer and the generator end
to end.  Helpers: tests/skeleton_data_oracle.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_oracle as ko
import online_oracle as oo
import skeleton_data_oracle as sdo

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
JOINT_COUNTS = (1, 2, 15, 20, 22, 32)      # every width class of csrc/pndf_knn.hip (8, 16, 24, 32), their ends, both sides of 21
SHAPES = ((1, 1), (1, 17), (33, 1000), (130, 4097))
KS = (1, 5, 16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _index(db, J, metric="geo", weights=None):
    from posendf_amd.knn import PoseIndex
    return PoseIndex(db, metric=metric, device=DEV, num_joints=J, weights=weights)


def _search(index, q, k):
    v, i = index.search(q, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == (len(q), k) and i.shape == (len(q), k)
    return v.cpu().numpy(), i.cpu().numpy()


def bits(v):
    return np.ascontiguousarray(v).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. the search against the fp64 brute force
@pytest.mark.parametrize("metric", ("geo", "euc"))
@pytest.mark.parametrize("Q,N", SHAPES)
@pytest.mark.parametrize("J", JOINT_COUNTS)
def test_matches_fp64_brute_force(J, Q, N, metric):
    q, db = sdo.knn_inputs(Q, N, J, seed=Q + N)
    D = sdo.all_distances(q, db, metric)
    index = _index(db, J, metric)
    assert len(index) == N and index.num_joints == J
    sdo.check_case([_search(index, q, k) + (k,) for k in KS if k <= N], D)


@pytest.mark.parametrize("metric", ("geo", "euc"))
def test_explicit_weights_on_the_hand(metric):
    q, db = sdo.knn_inputs(130, 4097, 15, seed=130 + 4097)
    w = np.random.default_rng(15).uniform(0.02, 0.3, 15).astype(np.float32)
    D = sdo.all_distances(q, db, metric, weights=w)
    assert np.abs(D - sdo.all_distances(q, db, metric)).max() > 1e-2      # (not the default weighting)
    index = _index(db, 15, metric, weights=w)
    sdo.check_case([_search(index, q, k) + (k,) for k in KS], D)


# ------------------------------------------------------------------------------------------ 2. the reference's vectors
@pytest.mark.parametrize("metric", ("geo", "euc"))
@pytest.mark.parametrize("J", (15, 32))
def test_matches_reference_vectors(J, metric):
    """tests/test_knn_gpu.py::test_matches_reference_vectors for J joints (tests/golden/make_golden_skeleton_knn.py)"""
    g = np.load(os.path.join(HERE, "golden", "skeleton_knn_ref.npz"))
    q, db = sdo.knn_inputs(16, 2000, J, 5)
    v, i = _search(_index(db, J, metric), q, 5)
    ref_v, ref_i = g[f"{metric}_u_{J}_val"], g[f"{metric}_u_{J}_idx"]
    np.testing.assert_allclose(v, ref_v, rtol=5e-6, atol=5e-7)
    distinct = np.ones_like(ref_i, dtype=bool)
    distinct[:, 1:] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    distinct[:, :-1] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    assert (i[distinct] == ref_i[distinct]).all()


# ------------------------------------------------------------------------------------------ 3. 21 joints: the two entry points
def _raw_search(lib, create, db_t, q_t, k):
    """an index made by `create(&handle)` searched through pndf_knn_search -> (vals, idx) tensors"""
    h = ctypes.c_void_p()
    assert create(ctypes.byref(h)) == 0, lib.pndf_knn_last_error(None)
    try:
        Q = len(q_t)
        n = lib.pndf_knn_workspace_bytes(h, Q, k)
        assert n >= 0 and lib.pndf_knn_size(h) == len(db_t)
        ws = torch.empty(max(n, 16), dtype=torch.uint8, device=DEV)
        vals = torch.empty(Q, k, dtype=torch.float32, device=DEV)
        idx = torch.empty(Q, k, dtype=torch.int64, device=DEV)
        rc = lib.pndf_knn_search(h, q_t.data_ptr(), Q, k, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), stream())
        assert rc == 0, lib.pndf_knn_last_error(h)
        torch.cuda.synchronize()
        return vals, idx
    finally:
        lib.pndf_knn_destroy(h)


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("metric", (0, 1), ids=("geo", "euc"))
def test_21_joints_equal_pndf_knn_create(lib, metric, weighted):
    from posendf_amd.knn import joint_weights
    q, db = ko.knn_inputs(130, 4097, seed=130 + 4097)
    assert np.array_equal(q, sdo.knn_inputs(130, 4097, 21, seed=130 + 4097)[0])
    db_t, q_t = torch.from_numpy(db).to(DEV), torch.from_numpy(q).to(DEV)
    w = (ctypes.c_float * 21)(*joint_weights(21, True)) if weighted else None
    for k in KS:
        old = _raw_search(lib, lambda h: lib.pndf_knn_create(h, db_t.data_ptr(), len(db), metric, w, stream()), db_t, q_t, k)
        new = _raw_search(lib, lambda h: lib.pndf_skel_knn_create(h, db_t.data_ptr(), len(db), 21, metric, w, stream()), db_t, q_t, k)
        assert torch.equal(old[0].view(torch.int32), new[0].view(torch.int32)) and torch.equal(old[1], new[1]), k
        assert torch.equal(old[0], new[0])


# ------------------------------------------------------------------------------------------ 4. planted poses, plan independence
def test_planted_poses_on_the_hand():
    """an exact copy gives 0, an antipodal copy geo 0, a duplicate goes to the lower index, a NaN pose is never selected, k = N"""
    q, db = sdo.knn_inputs(4, 5000, 15, seed=9)
    db = db.copy()
    db[4321] = q[0]
    db[77] = q[1]
    db[4000] = q[1]                      # duplicate: 77 wins
    db[1234] = -q[2]                     # antipodal
    db[4999] = q[3]
    db[4998] = np.nan
    db[16, 14, 3] = np.nan
    for metric in ("geo", "euc"):
        v, i = _search(_index(db, 15, metric), q, 3)
        assert i[0, 0] == 4321 and i[1, 0] == 77 and i[1, 1] == 4000 and i[3, 0] == 4999
        assert np.abs(v[[0, 1, 3], 0]).max() < 1e-6 and v[1, 1] == v[1, 0]
        if metric == "geo":
            assert i[2, 0] == 1234 and abs(v[2, 0]) < 1e-6
    q2, db2 = sdo.knn_inputs(6, 12, 15, seed=4)
    db2 = db2.copy()
    db2[5] = np.nan
    db2[7, 3] = np.nan
    D = sdo.all_distances(q2, db2, "geo")
    v, i = _search(_index(db2, 15), q2, 12)           # k = N: every finite pose, then NaN / -1
    assert (i[:, :10] >= 0).all() and not np.isin(i[:, :10], [5, 7]).any()
    assert np.isnan(v[:, 10:]).all() and (i[:, 10:] == -1).all()
    ko.check_knn(v[:, :10], i[:, :10], np.where(np.isfinite(D), D, np.inf), 10)
    v, i = _search(_index(db2[:5], 15, "euc"), q2, 5)
    assert (np.sort(i, axis=1) == np.arange(5)).all()


@pytest.mark.parametrize("metric", ("geo", "euc"))
def test_plan_independence_at_32_joints(metric):
    q, db = sdo.knn_inputs(130, 4097, 32, seed=130 + 4097)
    index = _index(db, 32, metric)
    for k in (5, 16):
        v, i = _search(index, q, k)
        for chunk in (1, 7):
            parts = [_search(index, q[s:s + chunk], k) for s in range(0, len(q), chunk)]
            assert np.array_equal(bits(np.concatenate([p[0] for p in parts])), bits(v)), (k, chunk)
            assert np.array_equal(np.concatenate([p[1] for p in parts]), i), (k, chunk)


# ------------------------------------------------------------------------------------------ 5. the sampler
def device_sample(lib, man_t, first, count, opt, J=None):
    """pndf_skel_online_sample (J given) or pndf_online_sample over the device manifold -> (q, src, group) numpy; poisoned buffers"""
    width = man_t.shape[1]
    q = torch.full((count, width, 4), 7.0, dtype=torch.float32, device=DEV)
    src = torch.full((count,), -5, dtype=torch.int64, device=DEV)
    group = torch.full((count,), -5, dtype=torch.int32, device=DEV)
    if J is None:
        rc = lib.pndf_online_sample(man_t.data_ptr(), len(man_t), first, count, ctypes.byref(opt), q.data_ptr(), src.data_ptr(),
                                    group.data_ptr(), stream())
    else:
        rc = lib.pndf_skel_online_sample(man_t.data_ptr(), len(man_t), J, first, count, ctypes.byref(opt), q.data_ptr(), src.data_ptr(),
                                         group.data_ptr(), stream())
    assert rc == 0, lib.pndf_last_error(None)
    torch.cuda.synchronize()
    return q.cpu().numpy(), src.cpu().numpy(), group.cpu().numpy()


@pytest.mark.parametrize("J", (1, 15, 21, 32))
def test_sampler_equals_its_host_twin(lib, J):
    """1,003 poses: for every J a last workgroup of 256 joint quaternions that is partly filled"""
    man = sdo.manifold(1000, J)
    man_t = torch.from_numpy(man).to(DEV)
    assert (1003 * J) % 256
    for noise, n_sigma, first in ((0, 5, 0), (1, 16, 2 ** 32 - 3)):
        opt = oo.case_options(n_sigma, noise, seed=99 + J, draw=4)
        got = device_sample(lib, man_t, first, 1003, opt, J)
        assert sdo.same_bits(got, sdo.skel_twin(lib, man, first, 1003, opt)), (noise, first)
        if J == 21:
            assert sdo.same_bits(got, device_sample(lib, man_t, first, 1003, opt)), (noise, first)


def test_sample_noisy_on_the_device(lib):
    from posendf_amd import sample_noisy
    man = sdo.manifold(300, 15)
    q, src, group = sample_noisy(torch.from_numpy(man).to(DEV), 77, first=3, seed=5, draw=2, num_joints=15)
    h = sample_noisy(torch.from_numpy(man), 77, first=3, seed=5, draw=2, num_joints=15)
    assert q.is_cuda and sdo.same_bits((q.cpu().numpy(), src.cpu().numpy(), group.cpu().numpy()), [t.numpy() for t in h])


# ------------------------------------------------------------------------------------------ 6. end to end
def test_online_hand_dataset_on_the_device():
    from posendf_amd import OnlinePoseDataset
    from posendf_amd.online import knn_tile_bytes
    mans = sdo.hand_manifolds()
    ds = OnlinePoseDataset.from_manifold(mans, 4, 250, device=DEV, num_joints=15, chunk=300)      # chunks of 300, 300, 300, 100
    cpu = OnlinePoseDataset.from_manifold(mans, 4, 250, device="cpu", num_joints=15)
    assert ds.num_joints == 15 and ds.pose.shape == (1000, 15, 4) and ds.pose.is_cuda
    assert ds.nbytes >= cpu.nbytes + -(-300 // 16) * knn_tile_bytes(15) and knn_tile_bytes(15) == 15 * 4 * 16 * 4
    ds.refresh(2, seed=5)
    cpu.refresh(2, seed=5)
    torch.cuda.synchronize()
    assert sdo.same_bits([t.cpu().numpy() for t in (ds.pose, ds.src, ds.group)], [t.numpy() for t in (cpu.pose, cpu.src, cpu.group)])
    D = sdo.all_distances(cpu.pose.numpy(), np.concatenate(mans), "geo")
    ko.check_knn(ds.dist.cpu().numpy(), ds.nn_idx.cpu().numpy(), D, 5)
    ko.check_knn(cpu.dist.numpy(), cpu.nn_idx.numpy(), D, 5)


def test_hip_trainer_on_an_online_hand_pool(tmp_path):
    import trainer_fixtures as trf
    from posendf_amd import OnlinePoseDataset
    runs = []
    for name in ("a", "b"):
        t = sdo.hand_online_trainer(tmp_path / name, device=DEV, seed=3, engine_train="hip")
        assert t.hip and t.num_joints == 15 and isinstance(t.dataset, OnlinePoseDataset) and t.dataset.pose.is_cuda
        start = trf.params(t)
        t.train_model()
        pool0 = t.dataset.pose.clone()
        t.train_model()
        assert t.iter_nums == 2 and t.dataset.draw == 1 and not torch.equal(pool0, t.dataset.pose)
        runs.append(trf.params(t))
    assert all(np.array_equal(bits(runs[0][k]), bits(runs[1][k])) for k in runs[0])
    assert not np.array_equal(runs[0]["dfnet.lin0.weight"], start["dfnet.lin0.weight"])


def test_traindata_generate_on_the_hand(tmp_path):
    from posendf_amd import traindata
    from posendf_amd.trainer import PoseDataset
    raw = tmp_path / "raw"
    for ds, files in (("DS_A", 2), ("DS_B", 1)):
        os.makedirs(raw / ds)
        for f in range(files):
            np.savez(raw / ds / f"seq{f}.npz", pose_body=ko.make_pose_body(400 + 50 * f, seed=10 * len(ds) + f, width=45))
    out, man = tmp_path / "out", tmp_path / "man"
    path = traindata.generate(str(raw), str(out), "DS_A/seq0.npz", num_samples=45, runs=20, seed=3, batch_size=300, manifold_dir=str(man),
                              device=DEV, num_joints=15)
    f = np.load(path)
    n = 45 * 20
    assert f["pose"].shape == (n, 15, 4) and f["pose"].dtype == np.float32 and f["dist"].shape == (n, 5)
    assert f["nn_pose"].shape == (n, 5, 15, 3) and f["nn_idx"].shape == (n, 5) and f["nn_idx"].dtype == np.int64
    files = traindata.database_files(str(raw))
    db_aa = np.concatenate([traindata.load_pose_body(p, 15) for p in files])
    db_q = traindata.aa_to_quat(db_aa).numpy()
    assert np.array_equal(f["pose"], traindata.make_queries(files[0], 45, 20, 3, 15).astype(np.float32))
    ko.check_knn(f["dist"], f["nn_idx"], sdo.all_distances(f["pose"], db_q, "geo"), 5)
    assert np.array_equal(f["nn_pose"], db_aa[f["nn_idx"]])
    ds = PoseDataset(str(out), str(man), device="cpu", num_joints=15)
    assert ds.num_joints == 15 and ds.pose.shape == (n, 15, 4) and ds.man.shape == (len(db_q), 15, 4) and ds.k == 5
