"""Online training data on the device (csrc/pndf_online.hip, posendf_amd.online): the sampler kernel against the numpy
oracle and the host twin, chunk independence, `OnlinePoseDataset.refresh` against `PoseIndex.search`, the search oracle and the cpu
data set, the cuda `Trainer` on `data.online` (determinism, resume, refresh cadence, losses against the cpu trainer, inference
after training), and refresh's promise to allocate nothing and not to wait for the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_oracle as ko
import online_oracle as oo
import trainer_fixtures as trf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_sample(lib, man_t, first, count, opt):
    """pndf_online_sample into poisoned buffers -> (q, src, group) as numpy arrays"""
    from posendf_amd import engine
    q = torch.full((count, 21, 4), 7.0, device=DEV)
    src = torch.full((count,), -5, dtype=torch.int64, device=DEV)
    group = torch.full((count,), -5, dtype=torch.int32, device=DEV)
    engine.online_sample(man_t.data_ptr(), man_t.shape[0], first, count, opt, q.data_ptr(), src.data_ptr(), group.data_ptr(), stream(), lib)
    return q.cpu().numpy(), src.cpu().numpy(), group.cpu().numpy()


def host_sample(lib, man, first, count, opt):
    from posendf_amd import engine
    q, src, group = np.empty((count, 21, 4), np.float32), np.empty(count, np.int64), np.empty(count, np.int32)
    engine.online_sample_cpu(man.ctypes.data, len(man), first, count, opt, q.ctypes.data, src.ctypes.data, group.ctypes.data, lib)
    return q, src, group


def check_against_oracle_and_twin(lib, man, man_t, first, count, opt, what):
    q, src, group = device_sample(lib, man_t, first, count, opt)
    q_o, src_o, group_o = oo.oracle_of(man, first, count, opt)
    q_h, src_h, group_h = host_sample(lib, man, first, count, opt)
    assert np.array_equal(src, src_o) and np.array_equal(group, group_o), what
    assert np.array_equal(src, src_h) and np.array_equal(group, group_h), what
    err = float(np.abs(q.astype(np.float64) - q_o).max())
    err_h = float(np.abs(q.astype(np.float64) - q_h).max())
    unit = float(np.abs(np.linalg.norm(q.astype(np.float64), axis=2) - 1.0).max())
    assert err <= oo.POSE_TOL and err_h <= oo.POSE_TOL and unit <= oo.UNIT_TOL, (what, err, err_h, unit)
    return err, err_h


# ---- 1. the kernel against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sigma", oo.N_SIGMAS)
@pytest.mark.parametrize("N", oo.SIZES_N)
def test_kernel_against_the_oracle(lib, N, n_sigma):
    man = oo.manifold(N)
    man_t = torch.from_numpy(man).to(DEV)
    worst = worst_h = 0.0
    for noise in (0, 1):
        opt = oo.case_options(n_sigma, noise, seed=0x0123456789ABCDEF + N, draw=7 + n_sigma)
        for first in oo.FIRSTS:
            for count in oo.COUNTS:
                e, eh = check_against_oracle_and_twin(lib, man, man_t, first, count, opt, (noise, first, count))
                worst, worst_h = max(worst, e), max(worst_h, eh)
    print(f"[online] kernel, N = {N}, {n_sigma} groups: largest error against the fp64 oracle {worst:.2e}, against the host twin {worst_h:.2e}")


@pytest.mark.parametrize("n_sigma,noise,first", [(5, 0, 0), (16, 1, 2 ** 32 - 3)])
def test_kernel_many_workgroups_and_tail(lib, n_sigma, noise, first):
    """100,003 poses: 8,204 workgroups, the last one partly filled"""
    man = oo.manifold(1000)
    opt = oo.case_options(n_sigma, noise, seed=99, draw=4)
    e, eh = check_against_oracle_and_twin(lib, man, torch.from_numpy(man).to(DEV), first, 100_003, opt, (n_sigma, noise, first))
    print(f"[online] kernel, 100,003 poses: largest error against the fp64 oracle {e:.2e}, against the host twin {eh:.2e}")


# ---- 2. chunk independence, refusals, the no-op -------------------------------------------------------------------------------------
def test_chunk_independence_on_the_device(lib):
    from posendf_amd import engine
    man = oo.manifold(1000)
    man_t = torch.from_numpy(man).to(DEV)
    opt = oo.case_options(5, 1, seed=11, draw=2)
    first = 2 ** 32 - 500
    whole = device_sample(lib, man_t, first, 1000, opt)
    for chunk in (7, 333):
        q = torch.full((1000, 21, 4), 7.0, device=DEV)
        src = torch.full((1000,), -5, dtype=torch.int64, device=DEV)
        group = torch.full((1000,), -5, dtype=torch.int32, device=DEV)
        for s in range(0, 1000, chunk):
            c = min(chunk, 1000 - s)
            engine.online_sample(man_t.data_ptr(), 1000, first + s, c, opt, q.data_ptr() + 336 * s, src.data_ptr() + 8 * s,
                                 group.data_ptr() + 4 * s, stream(), lib)
        assert np.array_equal(q.cpu().numpy().view(np.uint32), whole[0].view(np.uint32)), chunk
        assert np.array_equal(src.cpu().numpy(), whole[1]) and np.array_equal(group.cpu().numpy(), whole[2]), chunk
    # NULL src / group: the same poses
    q = torch.empty(1000, 21, 4, device=DEV)
    engine.online_sample(man_t.data_ptr(), 1000, first, 1000, opt, q.data_ptr(), None, None, stream(), lib)
    assert np.array_equal(q.cpu().numpy().view(np.uint32), whole[0].view(np.uint32))
    # a misaligned q is refused, nothing is written; count == 0 leaves a poisoned buffer untouched
    poison = torch.full((16, 21, 4), 7.0, device=DEV)
    ref = ctypes.byref(opt)
    assert lib.pndf_online_sample(man_t.data_ptr(), 1000, 0, 8, ref, poison.data_ptr() + 4, None, None, stream()) == BAD_ARG
    assert "16-byte" in lib.pndf_last_error(None).decode()
    assert lib.pndf_online_sample(man_t.data_ptr() + 8, 1000, 0, 8, ref, poison.data_ptr(), None, None, stream()) == BAD_ARG
    assert lib.pndf_online_sample(man_t.data_ptr(), 1000, 0, 0, ref, poison.data_ptr(), None, None, stream()) == 0
    torch.cuda.synchronize()
    assert bool((poison == 7.0).all())


# ---- 3. refresh on the device ----------------------------------------------------------------------------------------------------
P_FILES, P_ROWS, POOL_SEED, POOL_DRAW = 4, 250, 5, 2
_POOL = {}


def pool_reference(metric=None):
    """computed once and left alone: the manifold, the cpu data set's pool (default options but symmetric noise), and per
    metric the fp64 distance matrix of that pool to the manifold"""
    from posendf_amd import OnlineOptions, OnlinePoseDataset
    if "man" not in _POOL:
        _POOL["man"] = oo.manifold(1000, seed=41)
        cpu = OnlinePoseDataset.from_manifold([_POOL["man"]], P_FILES, P_ROWS, OnlineOptions(noise="symmetric", k=1), device="cpu")
        cpu.refresh(POOL_DRAW, POOL_SEED)
        _POOL["pose"], _POOL["src"] = cpu.pose.numpy().copy(), cpu.src.numpy().copy()
    if metric is not None and metric not in _POOL:
        _POOL[metric] = ko.all_distances(_POOL["pose"], _POOL["man"], metric, False)
    return _POOL


@pytest.mark.parametrize("metric", ["geo", "euc"])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_refresh_on_the_device(lib, k, metric):
    from posendf_amd import OnlineOptions, OnlinePoseDataset, PoseIndex
    ref = pool_reference(metric)
    options = OnlineOptions(noise="symmetric", k=k, metric=metric)
    ds = OnlinePoseDataset.from_manifold([ref["man"]], P_FILES, P_ROWS, options, device=DEV)
    assert ds.device == torch.device(DEV) and ds.pose.shape == (1000, 21, 4) and ds.dist.shape == (1000, k) and ds.draw is None
    ds.refresh(POOL_DRAW, POOL_SEED)
    assert ds.draw == POOL_DRAW and ds.seed == POOL_SEED
    pose, dist, idx = ds.pose.cpu().numpy(), ds.dist.cpu().numpy(), ds.nn_idx.cpu().numpy()
    # the pool is the cpu data set's
    assert float(np.abs(pose - ref["pose"]).max()) <= oo.POSE_TOL and np.array_equal(ds.src.cpu().numpy(), ref["src"])
    # the labels are PoseIndex.search's, bit for bit
    vals, nn = PoseIndex(ref["man"], metric=metric, device=DEV).search(ds.pose, k)
    assert torch.equal(vals, ds.dist) and torch.equal(nn, ds.nn_idx)
    # ... and the search oracle's on the device's own pool (the cpu pool may differ from it by a rounding)
    D = ref[metric] if np.array_equal(pose, ref["pose"]) else ko.all_distances(pose, ref["man"], metric, False)
    ko.check_knn(dist, idx, D, k)
    # the query chunk does not change a bit
    small = OnlinePoseDataset.from_manifold([ref["man"]], P_FILES, P_ROWS, options, device=DEV, chunk=64)
    small.refresh(POOL_DRAW, POOL_SEED)
    assert torch.equal(small.pose, ds.pose) and torch.equal(small.dist, ds.dist) and torch.equal(small.nn_idx, ds.nn_idx)
    assert torch.equal(small.src, ds.src) and torch.equal(small.group, ds.group)


def test_dataset_refuses_what_does_not_fit(lib):
    from posendf_amd import OnlineOptions, OnlinePoseDataset
    with pytest.raises(MemoryError, match=r"need \d+ bytes"):
        OnlinePoseDataset.from_manifold([oo.manifold(100)], 4096, 2 ** 22, OnlineOptions(k=1), device=DEV)      # a 5.8 TB pool


# ---- 4. the trainer on cuda ----------------------------------------------------------------------------------------------------------
F, R, NUM_PTS = 4, 256, 64


def gpu_trainer(root, seed=0, device=DEV, live=True, **kw):
    from posendf_amd.trainer import Trainer
    if not os.path.isdir(os.path.join(str(root), "manifold")):
        oo.write_manifold(root)
    t = Trainer(oo.online_config(root, device, F, R, NUM_PTS, **kw), seed=seed)
    if live and not kw.get("continue_train"):
        trf.load_live(t)
    return t


def _same(a, b):
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_trainer_same_seed_same_bits_and_resume(tmp_path, lib):
    one, two = gpu_trainer(tmp_path / "a", seed=3), gpu_trainer(tmp_path / "b", seed=3)
    assert one.hip and one.online and one.exp_name.startswith("online_") and one.steps_per_epoch == 2
    r = [(one.train_model(e), two.train_model(e)) for e in range(2)]
    assert all(x == y for x, y in r) and all(np.isfinite(x).all() for x, _ in r)
    _same(trf.params(one), trf.params(two))
    ma, mb = trf.adam_state(one), trf.adam_state(two)
    assert all(np.array_equal(ma[k][0], mb[k][0]) and np.array_equal(ma[k][1], mb[k][1]) for k in ma)
    first = gpu_trainer(tmp_path / "c", seed=3)
    assert first.train_model(0) == r[0][0]
    del first
    resumed = gpu_trainer(tmp_path / "c", seed=3, continue_train=True)
    assert resumed.ep == 1 and resumed.iter_nums == one.steps_per_epoch and resumed.dataset.draw is None
    assert resumed.train_model(1) == r[1][0] and resumed.dataset.draw == 1
    _same(trf.params(one), trf.params(resumed))
    mc = trf.adam_state(resumed)
    assert all(np.array_equal(ma[k][0], mc[k][0]) and np.array_equal(ma[k][1], mc[k][1]) for k in ma)


def test_trainer_keeps_a_pool_for_refresh_every_epochs(tmp_path, lib):
    t = gpu_trainer(tmp_path, seed=1, refresh_every=2)
    pools = []
    for ep in range(3):
        t.train_model(ep)
        assert t.dataset.draw == ep // 2
        pools.append((t.dataset.pose.clone(), t.dataset.dist.clone()))
    assert torch.equal(pools[0][0], pools[1][0]) and torch.equal(pools[0][1], pools[1][1])
    assert not torch.equal(pools[1][0], pools[2][0]) and not torch.equal(pools[1][1], pools[2][1])


def test_trainer_losses_against_the_cpu_trainer_and_inference(tmp_path, lib):
    """one epoch, the same seed: the cuda trainer (HIP sampler, search and step) against the cpu trainer (host twin, torch labels,
    stock forward and torch.optim.Adam), per step and per loss within the relative bound of tests/test_trainer_gpu.py's
    comparison with the stock loop (trainer_fixtures.loss_tolerance: 1e-4 where the fp32 loop is itself that good)"""
    from posendf_amd import PoseNDF, synth
    gpu, cpu = gpu_trainer(tmp_path / "g", seed=6), gpu_trainer(tmp_path / "c", seed=6, device="cpu")
    q = torch.from_numpy(synth.make_poses(200, seed=9)).to(DEV)
    for t in (gpu, cpu):
        t.begin_epoch(0)
        for _ in range(t.steps_per_epoch):
            t.step()
    assert float((gpu.dataset.pose.cpu() - cpu.dataset.pose).abs().max()) <= oo.POSE_TOL and torch.equal(gpu.dataset.src.cpu(), cpu.dataset.src)
    lg, lc = gpu.read_log(), cpu.read_log()
    tol = trf.loss_tolerance(1.0, 1.0)
    rel = np.where(lg == lc, 0.0, np.abs(lg - lc) / np.maximum(np.abs(lc), 1e-30))
    print(f"[online] cuda against cpu trainer, per-step losses {lc.tolist()}: largest relative difference {rel.max():.2e} (bound {tol:.0e})")
    assert np.isfinite(lg).all() and (rel <= tol).all(), (lg, lc)
    # project() after training sees the updated weights (a learning rate large enough for one step to show in fp32 distances)
    p0, _ = gpu.model.project(q, 3)
    gpu.learning_rate = 1e-3
    gpu.begin_epoch(1)
    gpu.step()
    p1, _ = gpu.model.project(q, 3)
    fresh = PoseNDF(oo.online_config(tmp_path / "g", DEV, F, R, NUM_PTS))
    fresh.load_state_dict({k: v.clone() for k, v in gpu.model.state_dict().items()})
    p2, _ = fresh.project(q, 3)
    assert torch.equal(p1, p2) and not torch.equal(p0, p1)


# ---- 5. refresh allocates nothing and does not wait ------------------------------------------------------------------------------
def test_refresh_allocates_nothing_and_does_not_synchronise(lib):
    from posendf_amd import OnlineOptions, OnlinePoseDataset
    ds = OnlinePoseDataset.from_manifold([oo.manifold(1000, seed=41)], 4, 1000, OnlineOptions(), device=DEV, chunk=1024)
    ds.refresh(0, 1)
    a, b = torch.randn(4096, 4096, device=DEV), torch.randn(4096, 4096, device=DEV)
    for _ in range(3):
        a @ b                                # (the product is dropped at once: its block goes back to torch's cache)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    busy = torch.cuda.Event()
    for _ in range(60):                      # some tens of milliseconds of matrix products queued in front of the refresh
        a @ b
    busy.record()
    ds.refresh(1, 1)
    returned_early = not busy.query()        # the call came back while the work queued before it was still running
    after = torch.cuda.memory_allocated()
    torch.cuda.synchronize()
    assert after == before and ds.draw == 1, (before, after)
    print(f"[online] refresh returned with earlier work still queued: {returned_early}")
    assert returned_early
