"""Online training data on the host (include/posendf_amd_online.h, posendf_amd.online): Philox4x32-10 against its known
answers, the host twin `pndf_online_sample_cpu` against the numpy oracle (tests/online_oracle.py), chunk independence, the
distribution of rows and groups, the companion header against its signature table and every refusal, and the cpu
`OnlinePoseDataset` / `Trainer` -- pure pools, exact labels, refresh cadence, determinism and resume.  Runs without a GPU;
tests/test_online_gpu.py holds the kernel and the device data set to the same."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cabi_headers as ch
import knn_oracle as ko
import online_oracle as oo
import trainer_fixtures as trf

BAD_ARG, NO_DEVICE = -1, -6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def twin(lib, man, first, count, opt, want_src=True, want_group=True):
    """pndf_online_sample_cpu -> (q, src or None, group or None); the buffers start poisoned"""
    q = np.full((count, 21, 4), 7.0, np.float32)
    src = np.full(count, -5, np.int64) if want_src else None
    group = np.full(count, -5, np.int32) if want_group else None
    rc = lib.pndf_online_sample_cpu(man.ctypes.data, len(man), first, count, ctypes.byref(opt), q.ctypes.data,
                                    None if src is None else src.ctypes.data, None if group is None else group.ctypes.data)
    assert rc == 0, (rc, lib.pndf_cpu_last_error(None))
    return q, src, group


# ---- 1. Philox ----------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, out in oo.KNOWN_ANSWERS:
        assert oo.philox_scalar(ctr, key) == out
        assert tuple(int(w) for w in oo.philox(np.array(ctr), np.array(key))) == out


def test_vectorised_philox_against_the_scalar_one():
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    got = oo.philox(ctr, key)
    for r in range(1000):
        assert tuple(int(w) for w in got[r]) == oo.philox_scalar(ctr[r], key[r]), r


# ---- 2. the host twin against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sigma", oo.N_SIGMAS)
@pytest.mark.parametrize("N", oo.SIZES_N)
def test_host_twin_against_the_oracle(lib, N, n_sigma):
    man = oo.manifold(N)
    worst = 0.0
    for noise in (0, 1):
        opt = oo.case_options(n_sigma, noise, seed=0x0123456789ABCDEF + N, draw=7 + n_sigma)
        for first in oo.FIRSTS:
            for count in oo.COUNTS:
                q, src, group = twin(lib, man, first, count, opt)
                q_o, src_o, group_o = oo.oracle_of(man, first, count, opt)
                assert np.array_equal(src, src_o) and np.array_equal(group, group_o), (noise, first, count)
                assert 0 <= src.min() and src.max() < N and 0 <= group.min() and group.max() < n_sigma
                err = float(np.abs(q.astype(np.float64) - q_o).max())
                unit = float(np.abs(np.linalg.norm(q.astype(np.float64), axis=2) - 1.0).max())
                worst = max(worst, err)
                assert err <= oo.POSE_TOL and unit <= oo.UNIT_TOL, (noise, first, count, err, unit)
    print(f"[online] host twin against the fp64 oracle, N = {N}, {n_sigma} groups: largest error {worst:.2e}")


def test_src_and_group_may_be_null(lib):
    man = oo.manifold(1000)
    opt = oo.case_options(5, 0, seed=3, draw=1)
    full = twin(lib, man, 5, 65, opt)
    for want_src, want_group in ((False, True), (True, False), (False, False)):
        q, src, group = twin(lib, man, 5, 65, opt, want_src, want_group)
        assert np.array_equal(q.view(np.uint32), full[0].view(np.uint32))
        assert src is None or np.array_equal(src, full[1])
        assert group is None or np.array_equal(group, full[2])


def test_degenerate_and_nan_rows(lib):
    """a zero row with sigma 0 has squared norm 0 and comes back unchanged; a NaN row gives a NaN pose"""
    from posendf_amd import engine
    man = oo.manifold(3).copy()
    man[0] = 0.0
    man[1, 4] = np.nan
    opt = engine.online_opts([0.0], [1.0], "uniform", seed=1, draw=0)
    q, src, _ = twin(lib, man, 0, 200, opt)
    assert set(src.tolist()) == {0, 1, 2}
    assert (q[src == 0] == 0.0).all()
    assert np.isnan(q[src == 1][:, 4]).all() and np.isfinite(q[src == 1][:, :4]).all()
    assert np.abs(q[src == 2] - oo.oracle_of(man, 0, 200, opt)[0][src == 2]).max() <= oo.POSE_TOL


# ---- 3. chunk independence -------------------------------------------------------------------------------------------------------
def test_chunk_independence(lib):
    man = oo.manifold(1000)
    opt = oo.case_options(5, 1, seed=11, draw=2)
    first = 2 ** 32 - 500
    whole = twin(lib, man, first, 1000, opt)
    for chunk in (1, 7, 333):
        parts = [twin(lib, man, first + s, min(chunk, 1000 - s), opt) for s in range(0, 1000, chunk)]
        for c in range(3):
            got = np.concatenate([p[c] for p in parts])
            assert np.array_equal(got.view(np.uint32) if c == 0 else got, whole[c].view(np.uint32) if c == 0 else whole[c]), (chunk, c)


# ---- 4. distribution -------------------------------------------------------------------------------------------------------------
DIST_SEED = 0      # chosen on the oracle (the first seed tried).  The bound on a share, 0.2 +- 0.005, is about four standard deviations
#                    of a binomial at 100,000 draws (sqrt(0.2 * 0.8 / 1e5) = 1.26e-3): a seed that fails the oracle is replaced, the bound is not


def test_distribution(lib):
    from posendf_amd import engine
    opt = engine.OnlineOpts()
    assert lib.pndf_online_default_opts(ctypes.byref(opt)) == 0
    assert opt.n_sigma == 5 and opt.noise == 0 and opt.seed == 0 and opt.draw == 0
    assert np.array_equal(np.array(opt.sigma[:5]), np.array(oo.DEFAULT_SIGMAS, np.float32))
    assert opt.cum[4] == 0xFFFFFFFF and all(abs((opt.cum[g] + 1) / 2 ** 32 - 0.2 * (g + 1)) < 1e-9 for g in range(5))
    opt.seed = DIST_SEED
    count, N = 100_000, 1000
    for name, (src, group) in (("oracle", oo.picks(N, 0, count, opt.seed, opt.draw, list(opt.cum[:5]))),
                               ("twin", twin(lib, oo.manifold(N), 0, count, opt)[1:])):
        share = np.bincount(group, minlength=5) / count
        print(f"[online] {name}: group shares {share.tolist()}, rows drawn {len(np.unique(src))} of {N}")
        assert (np.abs(share - 0.2) <= 0.005).all(), (name, share)
        assert len(np.unique(src)) == N, name


def test_shares_make_the_thresholds(lib):
    from posendf_amd import engine
    opt = engine.online_opts([0.1, 0.2, 0.3], [0.5, 0.25, 0.25])
    assert [opt.cum[g] for g in range(3)] == [0x7FFFFFFF, 0xBFFFFFFF, 0xFFFFFFFF]
    opt = engine.online_opts([0.1], [3.0])
    assert opt.cum[0] == 0xFFFFFFFF
    opt = engine.online_opts(np.linspace(0.1, 0.2, 16), [1.0] * 16)
    assert [opt.cum[g] for g in range(16)] == [(g + 1) * 2 ** 28 - 1 for g in range(16)]
    # thirds: 2^32 = 3 * 1431655765 + 1, the one left over goes to the first of the equal remainders
    opt = engine.online_opts([0.1, 0.2, 0.3], [1.0, 1.0, 1.0])
    assert [opt.cum[g] for g in range(3)] == [1431655765, 2 * 1431655765 + 0, 0xFFFFFFFF]
    for bad in ([0.5, 0.0, 0.5], [0.5, -1.0, 0.5], [0.5, float("nan"), 0.5], [0.5, float("inf"), 0.5], [1.0, 1e-12, 1.0]):
        o = engine.OnlineOpts()
        o.n_sigma = 3
        assert lib.pndf_online_shares(ctypes.byref(o), (ctypes.c_float * 3)(*bad)) == BAD_ARG, bad
        assert b"share" in lib.pndf_cpu_last_error(None)
    o = engine.OnlineOpts()
    for n in (0, 17, -1):
        o.n_sigma = n
        assert lib.pndf_online_shares(ctypes.byref(o), (ctypes.c_float * 16)(*([1.0] * 16))) == BAD_ARG
    o.n_sigma = 2
    assert lib.pndf_online_shares(ctypes.byref(o), None) == BAD_ARG and lib.pndf_online_shares(None, None) == BAD_ARG
    assert lib.pndf_online_default_opts(None) == BAD_ARG


# ---- 5. ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_matches_the_signature_table(lib):
    """what is the online header's own (its table, binding and symbols: tests/test_cabi.py, for every header alike): every entry point
    returns a status, posendf_amd.h names none of them, the build knows the sources, the options structure has the header's size"""
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    header = "posendf_amd_online.h"
    assert all(ret == "int" and abi.HEADERS[header][name][0] is ctypes.c_int for name, (ret, _) in ch.prototypes(header).items())
    main = ch.header_text("posendf_amd.h")
    assert not any(n in main for n in abi.exports(header))
    assert "pndf_online.hip" in ge.PRODUCT_SOURCES and "pndf_online.h" in ge.HIP_DEPS
    assert ctypes.sizeof(engine.OnlineOpts) == 152      # 8 + 4 + 4 + 4 + 64 + 64, padded to the struct's 8-byte alignment


def test_header_compiles_as_plain_c(tmp_path):
    ok, diagnostics = ch.compiles_as_c99(tmp_path, '#include "posendf_amd_online.h"\nint use(void) { pndf_online_opts o; '
                                         "o.n_sigma = PNDF_ONLINE_MAX_SIGMA; return (int)sizeof(o) + o.n_sigma + PNDF_ONLINE_SYMMETRIC; }\n")
    assert ok, diagnostics


def _refusals(opt_of):
    """(what, kwargs of a call that is otherwise fine) for every refusal of the sampler's entry points"""
    def opt(**kw):
        o = opt_of()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(o, k)[v[0]] = v[1]
            else:
                setattr(o, k, v)
        return o
    return [
        ("N < 1", dict(N=0)), ("N < 1", dict(N=-4)), ("N >= 2^31", dict(N=2 ** 31)),
        ("negative count", dict(count=-1)), ("negative first", dict(first=-1)), ("first + count", dict(first=2 ** 63 - 3, count=8)),
        ("n_sigma 0", dict(opt=opt(n_sigma=0))), ("n_sigma 17", dict(opt=opt(n_sigma=17))),
        ("negative sigma", dict(opt=opt(sigma=(2, -0.1)))), ("inf sigma", dict(opt=opt(sigma=(0, float("inf"))))),
        ("nan sigma", dict(opt=opt(sigma=(4, float("nan"))))),
        ("non-monotone cum", dict(opt=opt(cum=(1, 5)))), ("last cum", dict(opt=opt(cum=(4, 0xFFFFFFFE)))),
        ("noise 2", dict(opt=opt(noise=2))), ("noise -1", dict(opt=opt(noise=-1))),
        ("null opt", dict(opt=None)), ("null man_db", dict(man=None)), ("null q", dict(q=None)),
        ("misaligned src", dict(src=4)), ("misaligned group", dict(group=2)),
    ]


def test_refusals(lib):
    """every refusal returns PNDF_ERR_BAD_ARG with its text on the error channel: pndf_cpu_last_error(NULL) for the host twin,
    pndf_last_error(NULL) for pndf_online_sample, whose argument checks come before it looks for a device"""
    from posendf_amd import engine

    def default():
        o = engine.OnlineOpts()
        assert lib.pndf_online_default_opts(ctypes.byref(o)) == 0
        return o

    man = oo.manifold(8)
    buf = np.zeros(8 * 84 + 64, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16                    # a 16-byte aligned q for 8 poses
    man16 = np.zeros(8 * 84 + 64, np.float32)
    mbase = man16.ctypes.data + (-man16.ctypes.data) % 16
    ctypes.memmove(mbase, man.ctypes.data, man.nbytes)
    src, group = np.zeros(9, np.int64), np.zeros(9, np.int32)
    for what, kw in _refusals(default):
        a = dict(man=mbase, N=8, first=0, count=8, opt=default(), q=base, src=src.ctypes.data, group=group.ctypes.data)
        if "src" in kw or "group" in kw:
            kw = {k: a[k] + v for k, v in kw.items()}
        a.update(kw)
        ref = None if a["opt"] is None else ctypes.byref(a["opt"])
        for fn, err, extra in ((lib.pndf_online_sample_cpu, lib.pndf_cpu_last_error, ()), (lib.pndf_online_sample, lib.pndf_last_error, (None,))):
            rc = fn(a["man"], a["N"], a["first"], a["count"], ref, a["q"], a["src"], a["group"], *extra)
            text = err(None).decode()
            assert rc == BAD_ARG and text.startswith(fn.__name__ + ": ") and len(text) > len(fn.__name__) + 4, (what, fn.__name__, rc, text)
    # the kernel moves 16-byte vectors: a 4-byte aligned q or man_db is refused by the device entry point alone
    o = default()
    for m, q in ((mbase + 4, base), (mbase, base + 8)):
        assert lib.pndf_online_sample(m, 8, 0, 1, ctypes.byref(o), q, None, None, None) == BAD_ARG
        assert "16-byte" in lib.pndf_last_error(None).decode()
    assert lib.pndf_online_sample_cpu(mbase + 2, 8, 0, 1, ctypes.byref(o), base, None, None) == BAD_ARG
    # count == 0 is a no-op, whatever the pointers
    assert lib.pndf_online_sample_cpu(None, 8, 0, 0, ctypes.byref(o), None, None, None) == 0
    assert lib.pndf_online_sample(None, 8, 0, 0, ctypes.byref(o), None, None, None, None) == 0
    # a fine call of the device entry point: a loud error without a device, and host memory is not device memory with one
    rc = lib.pndf_online_sample(mbase, 8, 0, 8, ctypes.byref(o), base, None, None, None)
    if not torch.cuda.is_available():
        assert rc == NO_DEVICE and "no HIP device" in lib.pndf_last_error(None).decode()
        with pytest.raises(engine.PndfError):
            engine.online_sample(mbase, 8, 0, 8, o, base)
    else:
        assert rc == BAD_ARG and "device memory" in lib.pndf_last_error(None).decode()
    with pytest.raises(engine.PndfError):
        engine.online_opts([0.1, 0.2], [1.0])
    with pytest.raises(engine.PndfError):
        engine.online_opts([0.1], [1.0], noise="gauss")


# ---- 6. the cpu data set and trainer ---------------------------------------------------------------------------------------------
F, R, NUM_PTS = 4, 50, 16


def cpu_dataset(root, **kw):
    from posendf_amd import OnlineOptions, OnlinePoseDataset
    amass_dir, mans = oo.write_manifold(root)
    return OnlinePoseDataset(amass_dir, files=F, rows=R, options=OnlineOptions(**kw), device="cpu"), np.concatenate(mans)


def pool_bits(ds):
    return [t.detach().cpu().numpy().copy() for t in (ds.pose, ds.dist, ds.src, ds.group, ds.nn_idx)]


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("metric,weighted,k", [("geo", False, 5), ("euc", True, 3)])
def test_cpu_dataset_pools_and_labels(tmp_path, metric, weighted, k):
    from posendf_amd import PoseDataset, sample_noisy
    ds, man = cpu_dataset(tmp_path, metric=metric, weighted=weighted, k=k, noise="symmetric")
    assert isinstance(ds, PoseDataset) and ds.F == F and ds.Fm == 2 and ds.k == k and ds.draw is None
    assert ds.pose.shape == (F * R, 21, 4) and ds.dist.shape == (F * R, k) and ds.man.shape == (300, 21, 4)
    assert ds.file_off.tolist() == [0, 50, 100, 150, 200] and ds.man_off.tolist() == [0, 200, 300]
    assert ds.file_off_t.tolist() == ds.file_off.tolist() and ds.man_off_t.tolist() == ds.man_off.tolist() and ds.nbytes > 0
    ds.refresh(3, seed=9)
    a = pool_bits(ds)
    assert ds.draw == 3 and ds.seed == 9
    ds.refresh(4, seed=9)
    b = pool_bits(ds)
    ds.refresh(3, seed=10)
    c = pool_bits(ds)
    ds.refresh(3, seed=9)
    assert same(pool_bits(ds), a) and not same(a, b) and not same(a, c)
    # the pool is sample_noisy's, any part of it
    q, src, group = sample_noisy(ds.man, 70, first=60, seed=9, draw=3, options=ds.options)
    assert np.array_equal(q.numpy().view(np.uint32), a[0][60:130].view(np.uint32)) and np.array_equal(src.numpy(), a[2][60:130])
    assert np.array_equal(group.numpy(), a[3][60:130])
    q_o, src_o, group_o = oo.oracle_of(man, 0, F * R, ds.options.opts(9, 3))
    assert np.abs(a[0] - q_o).max() <= oo.POSE_TOL and np.array_equal(a[2], src_o) and np.array_equal(a[3], group_o)
    # the labels: the exact k nearest of the whole manifold, within the search oracle's own bound
    D = ko.all_distances(a[0], man, metric, weighted)
    ko.check_knn(a[1], a[4], D, k)


def test_dataset_refusals(tmp_path):
    from posendf_amd import OnlineOptions, OnlinePoseDataset
    mans = [oo.manifold(10)]
    with pytest.raises(ValueError, match="k = 11"):
        OnlinePoseDataset.from_manifold(mans, 2, 5, OnlineOptions(k=11))
    with pytest.raises(ValueError, match="k = 17"):
        OnlinePoseDataset.from_manifold([oo.manifold(40)], 2, 5, OnlineOptions(k=17))
    with pytest.raises(ValueError, match="32-bit"):
        OnlinePoseDataset.from_manifold(mans, 1, 2 ** 32, OnlineOptions(k=1))
    with pytest.raises(FileNotFoundError):
        OnlinePoseDataset(str(tmp_path), 2, 5)
    with pytest.raises(Exception):
        OnlinePoseDataset.from_manifold(mans, 2, 5, OnlineOptions(sigmas=(0.1, 0.2), shares=(1.0,)))


def cpu_trainer(root, seed=0, **kw):
    from posendf_amd.trainer import Trainer
    if not os.path.isdir(os.path.join(str(root), "manifold")):
        oo.write_manifold(root)
    t = Trainer(oo.online_config(root, "cpu", F, R, NUM_PTS, **kw), seed=seed)
    if not kw.get("continue_train"):
        trf.load_live(t)
    return t


def test_trainer_refreshes_with_the_draw(tmp_path):
    from posendf_amd import OnlinePoseDataset
    t = cpu_trainer(tmp_path, seed=4, refresh_every=2)
    assert isinstance(t.dataset, OnlinePoseDataset) and t.exp_name.startswith("online_") and t.steps_per_epoch == 2
    assert t.dataset.draw is None
    pools = []
    for ep in range(5):
        t.begin_epoch(ep)
        assert t.dataset.draw == ep // 2 and t.dataset.seed == 4
        pools.append(pool_bits(t.dataset))
    assert same(pools[0], pools[1]) and same(pools[2], pools[3])
    assert not same(pools[1], pools[2]) and not same(pools[3], pools[4]) and not same(pools[0], pools[4])
    # batch() of an epoch whose pool is not resident regenerates it
    pose, gt, man = t.batch(0, 1)
    rows, _ = t.batch_rows(0, 1)
    assert t.dataset.draw == 0 and np.array_equal(pose.numpy(), pools[0][0][rows])
    t.step()                               # ... and the epoch in flight (4) gets its own pool back before it trains on
    assert t.dataset.draw == 2 and same(pool_bits(t.dataset), pools[4])
    with pytest.raises(ValueError):
        cpu_trainer(tmp_path / "bad", refresh_every=0)


def test_trainer_same_seed_same_bits_and_resume(tmp_path):
    a = cpu_trainer(tmp_path / "a", seed=2)
    b = cpu_trainer(tmp_path / "b", seed=2)
    for t in (a, b):
        t.train_model()
        t.train_model()
    pa, pb = trf.params(a), trf.params(b)
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    assert a.iter_nums == 4 and a.dataset.draw == 1
    # resume after epoch 0
    c = cpu_trainer(tmp_path / "c", seed=2)
    c.train_model()
    d = cpu_trainer(tmp_path / "c", seed=2, continue_train=True)
    assert d.ep == 1 and d.iter_nums == 2
    d.train_model()
    pd, ma, md = trf.params(d), trf.adam_state(a), trf.adam_state(d)
    assert all(np.array_equal(pa[k], pd[k]) for k in pa)
    assert all(np.array_equal(ma[k][0], md[k][0]) and np.array_equal(ma[k][1], md[k][1]) for k in ma)
    # another seed trains on another pool
    e = cpu_trainer(tmp_path / "e", seed=3)
    e.begin_epoch(0)
    a.begin_epoch(0)
    assert not np.array_equal(e.dataset.pose.numpy(), a.dataset.pose.numpy())


def test_config_without_online_is_the_file_based_data_set(tmp_path):
    from posendf_amd import OnlinePoseDataset, PoseDataset
    from posendf_amd.trainer import Trainer
    trf.write_dirs(tmp_path)
    t = Trainer(trf.config(tmp_path, num_pts=NUM_PTS), seed=0)
    assert type(t.dataset) is PoseDataset and not isinstance(t.dataset, OnlinePoseDataset)
    assert not t.online and "online" not in t.exp_name
    t.begin_epoch(0)
    t.step()
    # an OnlinePoseDataset passed in is trained on as well, with the prefix
    ds = OnlinePoseDataset.from_manifold([oo.manifold(300)], F, R)
    t2 = Trainer(trf.config(tmp_path / "x", num_pts=NUM_PTS), seed=1, dataset=ds)
    assert t2.online and t2.exp_name.startswith("online_") and t2.refresh_every == 1
    t2.begin_epoch(3)
    assert ds.draw == 3 and ds.seed == 1
    t2.step()


# ---- 7. the labels mean something --------------------------------------------------------------------------------------------------
def test_labels_grow_with_sigma():
    """1,000 poses per sigma of the defaults, symmetric noise, over 2,000 seeded poses: the mean label is strictly increasing in
    sigma -- on the oracle alone first, then on the library's sampler and labels"""
    from posendf_amd import OnlineOptions
    from posendf_amd.online import host_labels, sample_noisy
    man = oo.manifold(2000, seed=77)
    means_o, means = [], []
    for g, sigma in enumerate(oo.DEFAULT_SIGMAS):
        q_o, _, _ = oo.sample(man, 0, 1000, 5, g, [sigma], [0xFFFFFFFF], 1)
        D = ko.all_distances(q_o, man, "geo", False)
        means_o.append(float(ko.brute_force(D, 5)[0].mean()))
        q, _, group = sample_noisy(torch.from_numpy(man), 1000, seed=5, draw=g,
                                   options=OnlineOptions(sigmas=(sigma,), shares=(1.0,), noise="symmetric"))
        assert int(group.max()) == 0
        vals, idx = torch.empty(1000, 5), torch.empty(1000, 5, dtype=torch.int64)
        host_labels(q, torch.from_numpy(man), 5, "geo", False, vals, idx)
        means.append(float(vals.double().mean()))
    print(f"[online] mean label per sigma: oracle {means_o}, library {means}")
    assert all(a < b for a, b in zip(means_o, means_o[1:])), means_o
    assert all(a < b for a, b in zip(means, means[1:])), means
    assert np.allclose(means, means_o, rtol=1e-5)
