"""CPU checks of the exact k-nearest-pose search and the training-data generator (posendf_amd.knn, posendf_amd.traindata): the
query sampler and the brute-force oracle against vectors produced by the reference itself, and the C ABI's refusals that need
no device."""
import ctypes
import os

import numpy as np
import pytest

from knn_oracle import all_distances, brute_force, knn_inputs, make_pose_body

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("num_samples", [100, 45])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sampler_matches_reference(num_samples, seed):
    """tests/golden/make_golden_traindata.py: create_data.py PoseData.__getitem__ (mode 'query') under np.random.seed(seed),
    two items from one stream, on the same synthetic sequence"""
    from posendf_amd import traindata
    g = np.load(os.path.join(HERE, "golden", "traindata_sampler.npz"))[f"pose_n{num_samples}_s{seed}"]
    quat = traindata.aa_to_quat(make_pose_body(300, 3, 69)[:, :63].reshape(-1, 21, 3)).numpy()
    rng = np.random.RandomState(seed)
    got = np.stack([traindata.sample_queries(quat, num_samples, rng) for _ in range(2)])
    assert got.shape == g.shape == (2, num_samples, 21, 4) and got.dtype == np.float64
    np.testing.assert_allclose(got, g, rtol=0, atol=1e-12)


def test_sampler_refuses_shares_that_do_not_add_up():
    from posendf_amd import traindata
    assert traindata.group_sizes(100).tolist() == [20] * 5 and traindata.group_sizes(45).tolist() == [9] * 5
    with pytest.raises(ValueError, match="add up"):
        traindata.group_sizes(37)
    quat = traindata.aa_to_quat(make_pose_body(20, 1).reshape(-1, 21, 3)).numpy()
    with pytest.raises(ValueError, match="37"):
        traindata.sample_queries(quat, 37, np.random.RandomState(0))


@pytest.mark.parametrize("metric", ["geo", "euc"])
@pytest.mark.parametrize("weighted", [False, True])
def test_oracle_matches_reference_vectors(metric, weighted):
    """tests/golden/make_golden_knn.py: the reference's dist_calc with the whole database as every query's candidate list"""
    g = np.load(os.path.join(HERE, "golden", "knn_ref.npz"))
    tag = f"{metric}_{'w' if weighted else 'u'}"
    q, db = knn_inputs(16, 2000, 5)
    val, idx = brute_force(all_distances(q, db, metric, weighted), 5)
    ref_v, ref_i = g[tag + "_val"], g[tag + "_idx"]
    np.testing.assert_allclose(val, ref_v, rtol=2e-6, atol=2e-7)
    distinct = np.ones_like(ref_i, dtype=bool)                 # indices wherever the reference's values are distinct
    distinct[:, 1:] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    distinct[:, :-1] &= np.abs(ref_v[:, 1:] - ref_v[:, :-1]) > 1e-6
    assert distinct.mean() > 0.9
    assert (idx[distinct] == ref_i[distinct]).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def test_knn_refusals_without_a_device(lib):
    vals = np.empty(16, np.float32)
    idx = np.empty(16, np.int64)
    q = np.zeros(84 * 4 + 4, np.float32)
    qa = q.ctypes.data + (-q.ctypes.data) % 16          # 16-byte aligned
    v, i = vals.ctypes.data, idx.ctypes.data
    for k in (0, 17, -1):
        assert lib.pndf_knn_search(None, qa, 1, k, v, i, None, None) == -1
        assert b"k must be in 1 .. 16" in lib.pndf_knn_last_error(None)
    assert lib.pndf_knn_search(None, qa, -1, 5, v, i, None, None) == -1
    assert b"Q must be" in lib.pndf_knn_last_error(None)
    assert lib.pndf_knn_search(None, qa + 4, 1, 5, v, i, None, None) == -1
    assert b"misaligned" in lib.pndf_knn_last_error(None)
    assert lib.pndf_knn_search(None, qa, 1, 5, v + 2, i, None, None) == -1
    assert lib.pndf_knn_search(None, qa, 1, 5, v, i + 4, None, None) == -1
    assert b"misaligned" in lib.pndf_knn_last_error(None)
    assert lib.pndf_knn_search(None, qa, 1, 5, v, i, None, None) == -1
    assert b"null index handle" in lib.pndf_knn_last_error(None)
    assert lib.pndf_knn_size(None) == -1 and lib.pndf_knn_workspace_bytes(None, 4, 5) == -1
    assert lib.pndf_knn_destroy(None) == 0
    h = ctypes.c_void_p()
    assert lib.pndf_knn_create(ctypes.byref(h), qa, 1, 7, None, None) == -4              # unknown metric
    assert lib.pndf_knn_create(ctypes.byref(h), qa, 0, 0, None, None) == -1              # N < 1
    assert lib.pndf_knn_create(ctypes.byref(h), qa, 1 << 31, 0, None, None) == -4        # N >= 2^31
    assert lib.pndf_knn_create(ctypes.byref(h), None, 4, 0, None, None) == -1
    assert lib.pndf_knn_create(ctypes.byref(h), qa + 4, 1, 0, None, None) == -1          # misaligned
    w = (ctypes.c_float * 21)(*([1.0] * 20 + [0.0]))
    assert lib.pndf_knn_create(ctypes.byref(h), qa, 1, 0, w, None) == -1                 # a joint weight <= 0
    assert b"weights" in lib.pndf_knn_last_error(None)
    assert not h.value


def test_knn_index_is_never_on_the_cpu():
    from posendf_amd.engine import PndfError
    from posendf_amd.knn import PoseIndex
    with pytest.raises(PndfError):
        PoseIndex(np.zeros((4, 21, 4), np.float32), device="cpu")
