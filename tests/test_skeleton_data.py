"""Training data for other skeletons (include/posendf_amd_skeleton_data.h), the parts that run without a GPU: the
header against the signature table, the joint-count refusals, the host twin of the J-joint sampler (against the 21-joint entry point
bit for bit, against the fp64 restatement of tests/skeleton_data_oracle.py for other J, chunk independence), the cpu
`OnlinePoseDataset(num_joints=15)` and the trainer on it, the traindata helpers and what `PoseIndex` refuses before it touches a
device.  tests/test_skeleton_data_gpu.py holds the kernels to the same."""
import ctypes

import numpy as np
import pytest
import torch

import cabi_headers as ch
import knn_oracle as ko
import online_oracle as oo
import skeleton_data_oracle as sdo
import trainer_fixtures as trf

BAD_ARG = sdo.BAD_ARG


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


# ------------------------------------------------------------------------------------------ 1. the header
def test_header_matches_the_signature_table(tmp_path):
    """each call takes its 21-joint form's parameters with num_joints after N, the build watches the header, and the calls in C; the
    header against its table is tests/test_cabi.py's"""
    import __graft_entry__ as ge
    from posendf_amd import abi
    mine = abi.HEADERS["posendf_amd_skeleton_data.h"]
    for skel, smpl, header in (("pndf_skel_knn_create", "pndf_knn_create", "posendf_amd.h"),
                               ("pndf_skel_online_sample", "pndf_online_sample", "posendf_amd_online.h"),
                               ("pndf_skel_online_sample_cpu", "pndf_online_sample_cpu", "posendf_amd_online.h")):
        smpl_args = abi.HEADERS[header][smpl][1]
        at = smpl_args.index(ctypes.c_int64) + 1
        assert list(mine[skel][1]) == list(smpl_args[:at]) + [ctypes.c_int32] + list(smpl_args[at:])
    assert "posendf_amd_skeleton_data.h" in " ".join(ge.HIP_DEPS)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, '#include "posendf_amd_skeleton_data.h"\nint main(void) { pndf_knn_handle h = 0; pndf_online_opts o; '
                                         'return pndf_skel_knn_create(&h, 0, 1, 15, 0, 0, 0) + pndf_skel_online_sample(0, 1, 15, 0, 0, &o, 0, 0, 0, 0) + '
                                         'pndf_skel_online_sample_cpu(0, 1, 15, 0, 0, &o, 0, 0, 0); }\n')
    assert ok, diagnostics


# ------------------------------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("J", (0, 33, -1))
def test_joint_count_is_refused_before_pointers_are_read(lib, J):
    """every pointer is the address 16, which nothing may read or write: the joint count decides first"""
    bad = ctypes.c_void_p(16)
    handle_at = ctypes.cast(bad, ctypes.POINTER(ctypes.c_void_p))
    opt_at = ctypes.cast(bad, ctypes.POINTER(type(oo.case_options(5, 0, 0, 0))))
    assert lib.pndf_skel_knn_create(handle_at, bad, 100, J, 0, bad, None) == BAD_ARG
    assert b"num_joints" in lib.pndf_knn_last_error(None)
    assert lib.pndf_skel_online_sample(bad, 100, J, 0, 10, opt_at, bad, bad, bad, None) == BAD_ARG
    assert b"num_joints" in lib.pndf_last_error(None)
    assert lib.pndf_skel_online_sample_cpu(bad, 100, J, 0, 10, opt_at, bad, bad, bad) == BAD_ARG
    assert b"num_joints" in lib.pndf_cpu_last_error(None)


def test_the_other_refusals_are_the_21_joint_ones(lib):
    """with a joint count in range the texts of pndf_online_sample_cpu, under the new name"""
    man = sdo.manifold(10, 15)
    q = np.zeros((4, 15, 4), np.float32)
    opt = oo.case_options(5, 0, 1, 0)
    for args, word in (((man.ctypes.data, 0, 15, 0, 4, ctypes.byref(opt), q.ctypes.data, None, None), b"manifold"),
                       ((man.ctypes.data, 10, 15, -1, 4, ctypes.byref(opt), q.ctypes.data, None, None), b"negative"),
                       ((man.ctypes.data, 10, 15, 0, (2 ** 31 - 1) * 256 // 15 + 1, ctypes.byref(opt), q.ctypes.data, None, None), b"grid"),
                       ((None, 10, 15, 0, 4, ctypes.byref(opt), q.ctypes.data, None, None), b"null")):
        assert lib.pndf_skel_online_sample_cpu(*args) == BAD_ARG
        text = lib.pndf_cpu_last_error(None)
        assert text.startswith(b"pndf_skel_online_sample_cpu: ") and word in text, text
    # the bound of the grid is a function of J: this count is refused at 21 joints and is a no-op question at 15
    count = (2 ** 31 - 1) * 256 // 21 + 1
    assert lib.pndf_online_sample_cpu(man.ctypes.data, 10, 0, count, ctypes.byref(opt), q.ctypes.data, None, None) == BAD_ARG
    assert b"grid" in lib.pndf_cpu_last_error(None)
    assert lib.pndf_skel_online_sample_cpu(man.ctypes.data, 10, 15, 0, 0, ctypes.byref(opt), None, None, None) == 0


# ------------------------------------------------------------------------------------------ 3. the host twin
@pytest.mark.parametrize("n_sigma", (1, 16))
@pytest.mark.parametrize("noise", (0, 1))
def test_21_joints_equal_the_21_joint_entry_point(lib, noise, n_sigma):
    man = oo.manifold(1000)
    opt = oo.case_options(n_sigma, noise, seed=0x0123456789ABCDEF + n_sigma, draw=3 + noise)
    for first in (0, 2 ** 32 - 3, 2 ** 32 + 5, 2 ** 40 + 1):
        for count in (1, 65, 300):
            q = np.full((count, 21, 4), 7.0, np.float32)
            src = np.full(count, -5, np.int64)
            group = np.full(count, -5, np.int32)
            rc = lib.pndf_online_sample_cpu(man.ctypes.data, len(man), first, count, ctypes.byref(opt), q.ctypes.data, src.ctypes.data,
                                            group.ctypes.data)
            assert rc == 0
            assert sdo.same_bits(sdo.skel_twin(lib, man, first, count, opt), (q, src, group)), (first, count)


@pytest.mark.parametrize("J", (1, 15, 32))
def test_host_twin_against_the_oracle(lib, J):
    """the tolerance of tests/test_online.py's 21-joint twin (online_oracle.POSE_TOL / UNIT_TOL: per component, independent of J)"""
    worst = 0.0
    for N in (1, 1000):
        man = sdo.manifold(N, J)
        for noise in (0, 1):
            for n_sigma in (1, 5, 16):
                opt = oo.case_options(n_sigma, noise, seed=0x0123456789ABCDEF + N + J, draw=7 + n_sigma)
                for first in oo.FIRSTS:
                    for count in (1, 65, 1000):
                        q, src, group = sdo.skel_twin(lib, man, first, count, opt)
                        q_o, src_o, group_o = sdo.oracle_of(man, first, count, opt)
                        assert q.shape == (count, J, 4)
                        assert np.array_equal(src, src_o) and np.array_equal(group, group_o), (N, noise, first, count)
                        assert 0 <= src.min() and src.max() < N and 0 <= group.min() and group.max() < n_sigma
                        err = float(np.abs(q.astype(np.float64) - q_o).max())
                        unit = float(np.abs(np.linalg.norm(q.astype(np.float64), axis=2) - 1.0).max())
                        worst = max(worst, err)
                        assert err <= oo.POSE_TOL and unit <= oo.UNIT_TOL, (N, noise, first, count, err, unit)
    print(f"[skeleton data] host twin against the fp64 oracle, J = {J}: largest error {worst:.2e}")


def test_joints_draw_their_own_blocks(lib):
    """joint j of a J-joint pose draws block 1 + j whatever J is: over a manifold whose joints are all one quaternion, the first 15
    joints of the 32-joint pool are the 15-joint pool"""
    quat = sdo.manifold(50, 1)
    opt = oo.case_options(5, 1, seed=5, draw=1)
    q15 = sdo.skel_twin(lib, np.ascontiguousarray(np.repeat(quat, 15, axis=1)), 7, 100, opt)
    q32 = sdo.skel_twin(lib, np.ascontiguousarray(np.repeat(quat, 32, axis=1)), 7, 100, opt)
    assert np.array_equal(q32[0][:, :15].view(np.uint32), q15[0].view(np.uint32))
    assert np.array_equal(q32[1], q15[1]) and np.array_equal(q32[2], q15[2])


@pytest.mark.parametrize("J", (15, 32))
def test_chunk_independence(lib, J):
    man = sdo.manifold(1000, J)
    opt = oo.case_options(5, 1, seed=11, draw=2)
    first = 2 ** 32 - 500
    whole = sdo.skel_twin(lib, man, first, 1000, opt)
    for chunk in (500, 7, 333):
        parts = [sdo.skel_twin(lib, man, first + s, min(chunk, 1000 - s), opt) for s in range(0, 1000, chunk)]
        assert sdo.same_bits([np.concatenate([p[c] for p in parts]) for c in range(3)], whole), chunk


def test_sample_noisy_on_the_host(lib):
    from posendf_amd import sample_noisy
    from posendf_amd.online import OnlineOptions
    man = sdo.manifold(300, 15)
    q, src, group = sample_noisy(torch.from_numpy(man), 77, first=3, seed=5, draw=2, num_joints=15)
    opt = OnlineOptions().opts(5, 2)
    assert q.shape == (77, 15, 4)
    assert sdo.same_bits((q.numpy(), src.numpy(), group.numpy()), sdo.skel_twin(lib, man, 3, 77, opt))
    with pytest.raises(ValueError, match="num_joints"):
        sample_noisy(torch.from_numpy(man), 4, num_joints=33)


# ------------------------------------------------------------------------------------------ 4. the cpu data set
F, R, K = 3, 48, 5


def pool_bits(ds):
    return [t.clone().numpy() for t in (ds.pose, ds.src, ds.group, ds.dist, ds.nn_idx)]


@pytest.mark.parametrize("metric", ("geo", "euc"))
def test_cpu_dataset_on_the_hand(lib, metric):
    from posendf_amd import OnlinePoseDataset, PoseDataset
    from posendf_amd.online import OnlineOptions
    mans = sdo.hand_manifolds()
    ds = OnlinePoseDataset.from_manifold(mans, F, R, OnlineOptions(metric=metric, noise="symmetric"), device="cpu", num_joints=15)
    assert isinstance(ds, PoseDataset) and ds.num_joints == 15 and ds.F == F and ds.Fm == 2 and ds.k == K and ds.draw is None
    P, M, J = F * R, 300, 15
    assert ds.pose.shape == (P, J, 4) and ds.dist.shape == (P, K) and ds.nn_idx.shape == (P, K) and ds.man.shape == (M, J, 4)
    assert ds.src.shape == (P,) and ds.group.shape == (P,)
    assert ds.file_off.tolist() == [0, 48, 96, 144] and ds.man_off.tolist() == [0, 200, 300]
    assert ds.nbytes == 4 * (P * 4 * J + P * K + M * 4 * J) + 8 * (P * K + P) + 4 * P + 8 * (4 + 3)
    ds.refresh(3, seed=9)
    assert ds.draw == 3 and ds.seed == 9
    man = np.concatenate(mans)
    want = sdo.skel_twin(lib, man, 0, P, ds.options.opts(9, 3))
    assert sdo.same_bits((ds.pose.numpy(), ds.src.numpy(), ds.group.numpy()), want)
    D = sdo.all_distances(ds.pose.numpy(), man, metric)
    ko.check_knn(ds.dist.numpy(), ds.nn_idx.numpy(), D, K)
    a = pool_bits(ds)
    ds.refresh(4, seed=9)
    assert not np.array_equal(a[0], ds.pose.numpy())
    ds.refresh(3, seed=9)
    assert all(np.array_equal(x, y) for x, y in zip(a, pool_bits(ds)))


def test_cpu_dataset_refusals():
    from posendf_amd import OnlinePoseDataset
    from posendf_amd.online import OnlineOptions
    with pytest.raises(ValueError, match=r"<manifold 1>.*15"):
        OnlinePoseDataset.from_manifold([sdo.manifold(20, 15), oo.manifold(20)], F, R, device="cpu", num_joints=15)
    with pytest.raises(ValueError, match="21 SMPL joints"):
        OnlinePoseDataset.from_manifold(sdo.hand_manifolds(), F, R, OnlineOptions(weighted=True), device="cpu", num_joints=15)
    for J in (0, 33):
        with pytest.raises(ValueError, match="num_joints"):
            OnlinePoseDataset.from_manifold(sdo.hand_manifolds(), F, R, device="cpu", num_joints=J)


def test_manifold_files_of_another_width_name_the_file(tmp_path):
    from posendf_amd import OnlinePoseDataset
    amass_dir, _ = oo.write_manifold(tmp_path)      # 21-joint files
    with pytest.raises(ValueError, match=r"man000\.npz.*15"):
        OnlinePoseDataset(amass_dir, F, R, device="cpu", num_joints=15)


# ------------------------------------------------------------------------------------------ 5. the trainer, cpu backend
def test_cpu_trainer_on_an_online_hand_pool(tmp_path):
    from posendf_amd import OnlinePoseDataset, SkeletonPoseNDF
    t = sdo.hand_online_trainer(tmp_path / "a", seed=2)
    assert isinstance(t.model, SkeletonPoseNDF) and isinstance(t.dataset, OnlinePoseDataset) and t.num_joints == 15
    assert t.online and t.refresh_every == 1 and t.exp_name.startswith("online_") and t.dataset.draw is None
    t.begin_epoch(0)
    first = pool_bits(t.dataset)
    assert t.dataset.draw == 0 and t.dataset.seed == 2
    t.begin_epoch(1)
    assert t.dataset.draw == 1 and not np.array_equal(first[0], t.dataset.pose.numpy())
    pose, gt, man = t.batch(0, 0)
    assert pose.shape == (t.B, 15, 4) and man.shape == (t.B, 15, 4) and t.dataset.draw == 0
    rows, _ = t.batch_rows(0, 0)
    assert np.array_equal(pose.numpy(), first[0][rows])
    a = sdo.hand_online_trainer(tmp_path / "b", seed=2)
    b = sdo.hand_online_trainer(tmp_path / "c", seed=2)
    start = trf.params(a)
    for x in (a, b):
        x.train_model()
        x.train_model()
        assert x.iter_nums == 2 and x.dataset.draw == 1
    pa, pb = trf.params(a), trf.params(b)
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    assert not np.array_equal(pa["dfnet.lin0.weight"], start["dfnet.lin0.weight"])


def test_trainer_refuses_a_pool_of_another_joint_count(tmp_path):
    import skeleton_train_fixtures as stf
    from posendf_amd import OnlinePoseDataset
    from posendf_amd.trainer import Trainer
    ds = OnlinePoseDataset.from_manifold([oo.manifold(100)], 3, 48, device="cpu")
    with pytest.raises(ValueError, match="21 joints, the model has 15"):
        Trainer(stf.trainer_config(tmp_path), seed=0, dataset=ds)
    # the config mapping stays the 21-joint pool (tests/test_skeleton_train.py pins the refusal): its text says where the J-joint one goes
    from posendf_amd.engine import PndfError
    cfg = stf.trainer_config(tmp_path)
    cfg["data"]["online"] = {"files": 3, "rows": 16}
    with pytest.raises(PndfError, match=r"num_joints=15"):
        Trainer(cfg, seed=0)


# ------------------------------------------------------------------------------------------ 6. traindata
def _parent_sample_queries(quat_pose, num_samples, rng):
    """traindata.sample_queries as it was with 21 joints only, restated"""
    from posendf_amd.traindata import SIGMA, group_sizes
    out = []
    for i, num in enumerate(group_sizes(num_samples)):
        indices = rng.randint(0, len(quat_pose), num)
        sampled = quat_pose[indices] + SIGMA[i] * rng.rand(21, 4)
        sampled = sampled / np.linalg.norm(sampled, axis=2, keepdims=True)
        out.extend(sampled)
    return np.array(out)


def test_traindata_helpers(tmp_path):
    from posendf_amd import traindata
    quat = oo.manifold(300)
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    mine = np.concatenate([traindata.sample_queries(quat, 100, a) for _ in range(3)])
    want = np.concatenate([_parent_sample_queries(quat, 100, b) for _ in range(3)])
    assert mine.dtype == want.dtype and np.array_equal(mine, want)
    assert a.randint(0, 2 ** 31) == b.randint(0, 2 ** 31)      # the streams stand at the same place
    hand = traindata.sample_queries(sdo.manifold(300, 15), 100, np.random.RandomState(7))
    assert hand.shape == (100, 15, 4) and np.abs(np.linalg.norm(hand, axis=2) - 1.0).max() <= 1e-12
    body = ko.make_pose_body(40, seed=3, width=45)
    path = str(tmp_path / "seq.npz")
    np.savez(path, pose_body=body)
    assert np.array_equal(traindata.load_pose_body(path, 15), body.reshape(40, 15, 3))
    assert np.array_equal(traindata.load_pose_body(path, 10), body[:, :30].reshape(40, 10, 3))
    with pytest.raises(ValueError, match=r"seq\.npz.*45"):
        traindata.load_pose_body(path, 21)
    q = traindata.make_queries(path, 10, 4, seed=1, num_joints=15)
    assert q.shape == (40, 15, 4)
    wide = str(tmp_path / "wide.npz")
    np.savez(wide, pose_body=ko.make_pose_body(40, seed=3, width=69))
    assert np.array_equal(traindata.load_pose_body(wide), np.load(wide)["pose_body"][:, :63].reshape(40, 21, 3))
    assert traindata.main.__module__ == "posendf_amd.traindata"
    with pytest.raises(ValueError, match="21 SMPL joints"):
        traindata.generate(str(tmp_path), str(tmp_path / "out"), "seq.npz", weighted=True, num_joints=15)


# ------------------------------------------------------------------------------------------ 7. PoseIndex
def test_pose_index_refuses_arguments_before_the_device(monkeypatch):
    from posendf_amd import PoseIndex, knn

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(knn, "KnnIndex", no_device)      # (without a device the copy of the poses fails before it, not with ValueError)
    poses = torch.from_numpy(sdo.manifold(8, 15))
    with pytest.raises(ValueError, match="21 SMPL joints"):
        PoseIndex(poses, weighted=True, num_joints=15)
    with pytest.raises(ValueError, match="14 weights for 15 joints"):
        PoseIndex(poses, num_joints=15, weights=[1.0] * 14)
    with pytest.raises(ValueError, match="not both"):
        PoseIndex(torch.from_numpy(oo.manifold(8)), weighted=True, weights=[1.0] * 21)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and > 0"):
            PoseIndex(poses, num_joints=15, weights=[1.0] * 14 + [bad])
    for J in (0, 33):
        with pytest.raises(ValueError, match="1 .. 32"):
            PoseIndex(poses, num_joints=J)
