"""posendf_amd.trainer on an MI355X: the optimiser kernel against torch.optim.Adam, the batch kernel against numpy, the cuda
trainer against the reference's trajectories (tests/golden/trainer_*.npz) and against an fp64 stock loop on the same GPU,
determinism, resume, the inference paths after a step, and the pipeline raw poses -> training data -> training -> checkpoint ->
project().  Reads only fixtures and seeded synthetic data (the reference is not here).

Bounds: pndf_adam_step -- per buffer (p, exp_avg, exp_avg_sq) the error against torch's fp64 result in the norm over the buffer
is <= 2 x the error of torch's own fp32 result; pndf_train_batch -- poses bit-equal, the labels' mean within k u / (1 - k u),
u = 2^-24, of the fp64 mean (k non-negative addends and one division); trajectories -- tests/test_trainer.py's rules."""
import os

import numpy as np
import pytest
import torch

import train_fixtures as tf
import trainer_fixtures as trf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


@pytest.fixture()
def root(tmp_path, lib):
    trf.write_dirs(tmp_path)
    return tmp_path


def _same(a, b):
    assert a.keys() == b.keys()
    assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])][:5]


# ---- pndf_adam_step ----------------------------------------------------------------------------------------------------------
def _model_layout():
    """(n, pad mask) of the flat buffer of configs/amass.yaml's model: state-dict order, every tensor on a 16-byte boundary"""
    from posendf_amd import synth
    sizes = [int(np.prod(s)) for s in synth.state_dict_shapes().values()]
    mask, n = [], 0
    for s in sizes:
        padded = -(-s // 4) * 4
        mask += [False] * s + [True] * (padded - s)
        n += padded
    return n, np.array(mask)


def _adam_inputs(n, step, pad=None, seed=0):
    rng = np.random.default_rng([seed, n, step])
    sign = lambda: rng.choice([-1.0, 1.0], n)                            # noqa: E731
    p = rng.uniform(-0.5, 0.5, n)
    g = sign() * 10.0 ** rng.uniform(-6, 0, n)                             # magnitudes 1e-6 .. 1
    if step == 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = sign() * 10.0 ** rng.uniform(-6, 0, n)
        v = (10.0 ** rng.uniform(-6, 0, n)) ** 2
    out = [a.astype(np.float32) for a in (p, g, m, v)]
    if pad is not None:
        for a in out:
            a[pad] = 0.0
    return out


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("size", [1000, 1003, "model"])
def test_adam_step_against_torch(lib, size, step):
    from posendf_amd import engine
    lr, wd = 1e-5, 1e-4                                                    # train_posendf.py:30
    n, pad = _model_layout() if size == "model" else (size, None)
    p, g, m, v = _adam_inputs(n, step, pad)
    t32 = trf.torch_adam(p, g, m, v, step, torch.float32, lr, wd, DEV)
    t64 = trf.torch_adam(p, g, m, v, step, torch.float64, lr, wd, DEV)
    guard = 8                                                              # floats behind the buffer that no call may touch
    runs = []
    for _ in range(2):
        bufs = [torch.full((n + guard,), 7.0, dtype=torch.float32, device=DEV) for _ in range(4)]
        for b, a in zip(bufs, (p, g, m, v)):
            b[:n] = torch.from_numpy(a)
        engine.adam_step(*[b.data_ptr() for b in bufs], n, step, lr, 0.9, 0.999, 1e-8, wd, torch.cuda.current_stream().cuda_stream, lib)
        torch.cuda.synchronize()
        assert all(bool((b[n:] == 7.0).all()) for b in bufs)
        assert np.array_equal(bufs[1][:n].cpu().numpy(), g)              # the gradients are read only
        runs.append([bufs[i][:n].cpu().numpy() for i in (0, 2, 3)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))              # the same inputs give the same bits
    for name, mine, a32, a64 in zip(("p", "exp_avg", "exp_avg_sq"), runs[0], t32, t64):
        e_mine, e_32 = np.linalg.norm(mine.astype(np.float64) - a64), np.linalg.norm(a32 - a64)
        print(f"[adam n={n} step={step}] {name}: |mine - f64| = {e_mine:.3e}, |torch f32 - f64| = {e_32:.3e}, ratio {e_mine / e_32:.3f}")
        assert e_32 > 0.0
        assert e_mine <= 2.0 * e_32, (name, e_mine, e_32)
        assert not np.array_equal(mine, (p, m, v)[("p", "exp_avg", "exp_avg_sq").index(name)])
        if pad is not None:
            assert not mine[pad].any()                                    # the pads stay exactly zero


def test_adam_step_refuses_bad_arguments(lib):
    from posendf_amd import engine
    bufs = [torch.zeros(64, dtype=torch.float32, device=DEV) for _ in range(4)]
    ptr = [b.data_ptr() for b in bufs]
    call = lambda p, n, step, b1=0.9: lib.pndf_adam_step(*p, n, step, 1e-5, b1, 0.999, 1e-8, 1e-4, None)      # noqa: E731
    assert call(ptr, 64, 0) == -1 and call(ptr, 64, -3) == -1 and call(ptr, -1, 1) == -1
    assert call([None] + ptr[1:], 64, 1) == -1 and call(ptr[:3] + [None], 64, 1) == -1
    assert call([ptr[0] + 4] + ptr[1:], 60, 1) == -1 and call(ptr[:2] + [ptr[2] + 8, ptr[3]], 60, 1) == -1
    assert call(ptr, 64, 1, 1.0) == -1
    assert call([None] * 4, 0, 1) == 0 and call(ptr, 0, 1) == 0            # n == 0: a no-op
    torch.cuda.synchronize()
    assert all(not b.any() for b in bufs)
    with pytest.raises(engine.PndfError):
        engine.adam_step(*ptr, 64, 0, 1e-5, lib=lib)
    assert call(ptr, 64, 1) == 0
    torch.cuda.synchronize()


# ---- pndf_train_batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,num_pts,flip", [(5, 70, 0), (5, 70, 1), (1, 64, 1), (16, 1, 0), (16, 333, 1)])
def test_train_batch_against_numpy(lib, k, num_pts, flip):
    from posendf_amd import engine, synth
    rows, mrows = (40, 1, 1000, 1, 257), (1, 300, 17)                       # one-row files among them
    rng = np.random.default_rng([k, num_pts, flip])
    pose = synth.make_poses(sum(rows), seed=3, signed=True)
    man = synth.make_poses(sum(mrows), seed=4, signed=True)
    dist = rng.uniform(0.0, 0.5, (sum(rows), k)).astype(np.float32)
    off, moff = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), np.concatenate([[0], np.cumsum(mrows)]).astype(np.int64)
    item_file = np.array([2, 1, 4, 0, 3, 2], np.int32)                       # a file may serve two items of one call
    item_man = np.array([1, 0, 2, 2, 1, 0], np.int32)
    items = len(item_file)
    words = rng.integers(0, 2 ** 32, (items, 2, num_pts), dtype=np.uint64).astype(np.uint32)
    words[:, :, 0] = 0                                                       # the first row of a file ...
    words[:, :, -1] = 2 ** 32 - 1                                            # ... and the last one
    want_rows = []
    for side, (files, o) in enumerate(((item_file, off), (item_man, moff))):
        first, length = o[files].astype(np.uint64)[:, None], (o[files + 1] - o[files]).astype(np.uint64)[:, None]
        want_rows.append((first + ((words[:, side].astype(np.uint64) * length) >> np.uint64(32))).astype(np.int64))
    assert (want_rows[0][:, -1] == off[item_file + 1] - 1).all() and (want_rows[1][:, -1] == moff[item_man + 1] - 1).all()
    if num_pts > 1:
        assert (want_rows[0][:, 0] == off[item_file]).all() and (want_rows[1][:, 0] == moff[item_man]).all()
    r, rm = want_rows[0].reshape(-1), want_rows[1].reshape(-1)
    q_want, qm_want = pose[r], man[rm]
    if flip:
        q_want, qm_want = np.where(q_want[..., :1] < 0, -q_want, q_want), np.where(qm_want[..., :1] < 0, -qm_want, qm_want)
        assert (pose[r][..., 0] < 0).any() and (man[rm][..., 0] < 0).any()
    mean = dist[r].astype(np.float64).mean(1)

    dev = lambda a: torch.from_numpy(a).to(DEV)                             # noqa: E731
    t = [dev(a) for a in (pose, dist, man, off, moff, item_file, item_man, words.view(np.int32))]
    P = items * num_pts
    guard = 4
    q = torch.full((P + guard, 21, 4), 7.0, dtype=torch.float32, device=DEV)
    qm = torch.full((P + guard, 21, 4), 7.0, dtype=torch.float32, device=DEV)
    gt = torch.full((P + guard,), 7.0, dtype=torch.float32, device=DEV)
    engine.train_batch(*[x.data_ptr() for x in t], len(rows), len(mrows), k, items, num_pts, flip, q.data_ptr(), gt.data_ptr(),
                       qm.data_ptr(), torch.cuda.current_stream().cuda_stream, lib)
    torch.cuda.synchronize()
    assert bool((q[P:] == 7.0).all()) and bool((qm[P:] == 7.0).all()) and bool((gt[P:] == 7.0).all())
    assert np.array_equal(q[:P].cpu().numpy(), q_want) and np.array_equal(qm[:P].cpu().numpy(), qm_want)
    u = k * 2.0 ** -24
    err = np.abs(gt[:P].cpu().numpy().astype(np.float64) - mean)
    print(f"[batch k={k} num_pts={num_pts}] labels: worst error / bound = {(err / (u / (1 - u) * mean)).max():.3f}")
    assert (err <= u / (1 - u) * mean).all()


def test_train_batch_refuses_bad_arguments(lib):
    bufs = [torch.zeros(84 * 8, dtype=torch.float32, device=DEV) for _ in range(6)]
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device=DEV)
    files = torch.zeros(2, dtype=torch.int32, device=DEV)
    words = torch.zeros(2 * 2 * 3, dtype=torch.int32, device=DEV)
    pose, dist, man, q, gt, qm = [b.data_ptr() for b in bufs]

    def call(pose=pose, q=q, gt=gt, F=2, Fm=2, k=5, items=2, num_pts=3, off_ptr=off.data_ptr()):
        return lib.pndf_train_batch(pose, dist, man, off_ptr, off.data_ptr(), files.data_ptr(), files.data_ptr(), words.data_ptr(),
                                    F, Fm, k, items, num_pts, 0, q, gt, qm, None)
    assert call(F=0) == -1 and call(Fm=0) == -1 and call(k=0) == -1 and call(items=-1) == -1 and call(num_pts=-1) == -1
    assert call(pose=None) == -1 and call(q=None) == -1 and call(off_ptr=None) == -1
    assert call(pose=pose + 4) == -1 and call(q=q + 8) == -1 and call(gt=gt + 4) == -1
    assert call(items=0) == 0 and call(num_pts=0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    # an item that names a file outside the table is not sampled: NaN, nothing read
    files[1] = 9
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs[3][3 * 84:6 * 84]).all()) and bool(torch.isnan(bufs[4][3:6]).all()) and not bool(torch.isnan(bufs[3][:3 * 84]).any())


def test_empty_files_are_refused_at_load_time(lib):
    from posendf_amd import synth
    from posendf_amd.trainer import PoseDataset
    p = synth.make_poses(8, seed=1)
    d = np.zeros((8, 5), np.float32)
    with pytest.raises(ValueError, match="<data 1>.*empty"):
        PoseDataset.from_arrays([p, p[:0]], [d, d[:0]], [p], device=DEV)
    with pytest.raises(ValueError, match="<manifold 0>.*empty"):
        PoseDataset.from_arrays([p], [d], [p[:0]], device=DEV)


def test_a_data_set_larger_than_device_memory_is_refused(lib, monkeypatch):
    from posendf_amd import synth
    from posendf_amd.trainer import PoseDataset
    p = synth.make_poses(8, seed=1)
    d = np.zeros((8, 5), np.float32)
    need = 4 * (8 * 84 + 8 * 5 + 8 * 84) + 8 * 4
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need - 1, 1 << 40))
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        PoseDataset.from_arrays([p], [d], [p], device=DEV)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need, 1 << 40))
    assert PoseDataset.from_arrays([p], [d], [p], device=DEV).nbytes == need


# ---- trajectories --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(trf.CASES))
def test_reference_trajectory(root, name):
    t, losses = trf.run_case(root, name, DEV)
    assert t.hip
    trf.check_case(name, t, losses)


def _stock_loop(t, act, steps, dtype):
    """train_posendf.py:93-99 with a stock PoseNDF + torch.optim.Adam on the batches batch_rows names: (params, losses)"""
    from posendf_amd import PoseNDF
    sd, hidden = tf.case_weights("live")
    net = PoseNDF(tf.config(act, hidden, "l1", DEV)).to(dtype)
    net.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()})
    opt = torch.optim.Adam(net.parameters(), lr=trf.LR, weight_decay=1e-4)
    losses = np.zeros((steps, 3))
    for s in range(steps):
        pose, gt, man = t.batch(s // t.steps_per_epoch, s % t.steps_per_epoch)
        opt.zero_grad()
        _, ld = net(pose.to(dtype), gt.to(dtype), man.to(dtype), eikonal=1.0)
        loss = 0.0
        for k in ld.keys():
            loss += 1.0 * ld[k]
        loss.backward()
        opt.step()
        losses[s] = [float(ld[k].detach()) for k in tf.LOSS_KEYS]
    return {k: p.detach().double().cpu().numpy() for k, p in net.named_parameters()}, losses


@pytest.mark.parametrize("act,steps", [("lrelu", 10), ("softplus", 20)])
def test_trajectory_against_fp64_stock_loop(root, act, steps):
    """configs/amass.yaml dims, B = Bm = 2,048 (4 files x 512 poses), lr 1e-5"""
    t = trf.trainer(root, act=act, device=DEV, batch_size=4, num_pts=512)
    trf.load_live(t)
    assert t.B == 2048
    logs = []
    for s in range(steps):
        if s % t.steps_per_epoch == 0:
            if s:
                logs.append(t.read_log())
            t.begin_epoch(s // t.steps_per_epoch)
        t.step()
    logs.append(t.read_log()[:(steps - 1) % t.steps_per_epoch + 1])
    mine, losses = trf.params(t), np.concatenate(logs)
    p32, l32 = _stock_loop(t, act, steps, torch.float32)
    p64, l64 = _stock_loop(t, act, steps, torch.float64)
    bad, worst = [], 0.0
    for k in p64:
        d_h, d_32 = np.linalg.norm(mine[k] - p64[k]), np.linalg.norm(p32[k] - p64[k])
        worst = max(worst, d_h / max(d_32, 1e-30))
        if not d_h <= 2.0 * d_32 + 1e-9:
            bad.append((k, d_h, d_32))
    print(f"[trajectory {act} {steps} steps] worst |hip - f64| / |f32 - f64| over the parameter tensors: {worst:.3f}")
    assert not bad, bad[:8]
    lbad = [(s, c, losses[s, c], l64[s, c]) for s in range(steps) for c in range(3)
            if not abs(losses[s, c] - l64[s, c]) / abs(l64[s, c]) <= trf.loss_tolerance(l32[s, c], l64[s, c])]
    assert not lbad, lbad[:8]


# ---- determinism, resume, inference ----------------------------------------------------------------------------------------------
SMALL = dict(num_pts=96, device=DEV)


def test_same_seed_same_bits_and_resume(tmp_path, lib):
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        trf.write_dirs(d)
    one, two = trf.trainer(a, seed=3, **SMALL), trf.trainer(b, seed=3, **SMALL)
    r = [(one.train_model(e), two.train_model(e)) for e in range(2)]
    assert all(x == y for x, y in r) and all(np.isfinite(x).all() for x, _ in r)
    _same(trf.params(one), trf.params(two))
    other = trf.trainer(c, seed=4, **SMALL)
    assert not np.array_equal(trf.params(other)["dfnet.lin0.weight"], trf.params(trf.trainer(c, seed=3, **SMALL))["dfnet.lin0.weight"])
    # one epoch + checkpoint + a new trainer with continue_train + one epoch
    first = trf.trainer(c, seed=3, **SMALL)
    assert first.train_model(0) == r[0][0]
    del first
    resumed = trf.trainer(c, seed=3, continue_train=True, **SMALL)
    assert resumed.ep == 1 and resumed.iter_nums == one.steps_per_epoch
    assert resumed.train_model(1) == r[1][0]
    _same(trf.params(one), trf.params(resumed))
    ma, mb = trf.adam_state(one), trf.adam_state(resumed)
    assert all(np.array_equal(ma[k][0], mb[k][0]) and np.array_equal(ma[k][1], mb[k][1]) for k in ma)


def test_checkpoints_cross_the_backends(tmp_path, lib):
    """a checkpoint of the cuda trainer continues in a stock PoseNDF + torch.optim.Adam, and the cpu trainer's in the cuda one"""
    from posendf_amd import PoseNDF
    a = tmp_path / "a"
    trf.write_dirs(a)
    t = trf.trainer(a, **SMALL)
    t.train_model(0)
    ck = torch.load(os.path.join(t.checkpoint_path, "checkpoint_epoch_best.tar"), map_location=DEV)
    net = PoseNDF(trf.config(a, **SMALL))
    net.load_state_dict(ck["model_state_dict"])
    opt = torch.optim.Adam(net.parameters(), lr=trf.LR, weight_decay=1e-4)
    opt.load_state_dict(ck["optimizer_state_dict"])
    assert all(float(s["step"]) == t.steps_per_epoch for s in opt.state.values()) and len(opt.state) == 98
    pose, gt, man = t.batch(1, 0)
    opt.zero_grad()
    _, ld = net(pose, gt, man, eikonal=1.0)
    sum(ld.values()).backward()
    opt.step()                                                             # (runs: the state has torch's layout)
    b = tmp_path / "b"
    trf.write_dirs(b)
    cpu = trf.trainer(b, num_pts=96, device="cpu")
    cpu.train_model(0)
    gpu = trf.trainer(b, continue_train=True, **SMALL)
    assert gpu.ep == 1 and gpu.iter_nums == cpu.steps_per_epoch
    _same(trf.params(cpu), trf.params(gpu))
    mc, mg = trf.adam_state(cpu), trf.adam_state(gpu)
    assert all(np.array_equal(mc[k][1], mg[k][1]) for k in mc)
    assert np.isfinite(gpu.train_model(1)).all()


def test_inference_sees_the_update(root):
    from posendf_amd import PoseNDF, synth
    t = trf.trainer(root, **SMALL)
    trf.load_live(t)
    q = torch.from_numpy(synth.make_poses(300, seed=9)).to(DEV)
    d0 = t.model(q, train=False)["dist_pred"].clone()
    p0, _ = t.model.project(q, 3)
    # a learning rate large enough for one step to show in fp32 distances
    t.learning_rate = 1e-3
    t.step()
    d1 = t.model(q, train=False)["dist_pred"].clone()
    p1, _ = t.model.project(q, 3)
    fresh = PoseNDF(trf.config(root, **SMALL))
    fresh.load_state_dict({k: v.clone() for k, v in t.model.state_dict().items()})
    d2 = fresh(q, train=False)["dist_pred"]
    p2, _ = fresh.project(q, 3)
    assert torch.equal(d1, d2) and torch.equal(p1, p2)
    assert not torch.equal(d0, d1) and not torch.equal(p0, p1)
    # the parameters are views into the flat buffer; a re-homed one is refused
    assert all(p.data_ptr() == t.flat_p.data_ptr() + 4 * o for p, o in zip(t._params, t._offsets))
    t.model.dfnet.lin6.bias.data = t.model.dfnet.lin6.bias.data.clone()
    from posendf_amd.engine import PndfError
    with pytest.raises(PndfError, match="dfnet.lin6.bias"):
        t.step()


def test_raw_poses_to_projection(tmp_path, lib):
    """traindata.generate on a tiny raw directory, two epochs of training, the checkpoint loaded by PoseNDF, project()"""
    from knn_oracle import make_pose_body
    from posendf_amd import PoseNDF, synth, traindata
    raw, out, man = tmp_path / "raw", tmp_path / "out", tmp_path / "man"
    for ds, files in (("DS_A", 3), ("DS_B", 2)):
        os.makedirs(raw / ds)
        for f in range(files):
            np.savez(raw / ds / f"seq{f}.npz", pose_body=make_pose_body(300 + 40 * f, seed=10 * len(ds) + f + (ds == "DS_B")))
    for ds, files in (("DS_A", 3), ("DS_B", 2)):
        for f in range(files):
            traindata.generate(str(raw), str(out), f"{ds}/seq{f}.npz", num_samples=50, runs=6, seed=f, manifold_dir=str(man), device=DEV)
    cfg = trf.config(tmp_path, device=DEV, num_pts=128, dirs=(str(out), str(man)))
    from posendf_amd.trainer import Trainer
    t = Trainer(cfg, seed=0)
    assert t.dataset.F == 5 and t.dataset.Fm == 5 and t.dataset.k == 5
    res = [t.train_model(e) for e in range(2)]
    assert np.isfinite(res).all()
    best = os.path.join(t.checkpoint_path, "checkpoint_epoch_best.tar")
    assert os.path.exists(best) and os.path.exists(os.path.join(t.checkpoint_path, "checkpoint_epoch_previous.tar"))
    assert os.path.exists(os.path.join(t.exp_path, "summary.jsonl"))
    net = PoseNDF(cfg)
    net.load_state_dict(torch.load(best, map_location=DEV)["model_state_dict"])
    net.eval()
    qp, d = net.project(torch.from_numpy(synth.make_poses(64, seed=2)), steps=3)
    assert qp.shape == (64, 21, 4) and d.shape == (64, 1) and bool(torch.isfinite(qp).all()) and bool(torch.isfinite(d).all())
