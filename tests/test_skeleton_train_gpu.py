"""Training other skeletons on an MI355X (include/posendf_amd_skeleton_train.h): the HIP objective and every
weight gradient of `SkeletonPoseNDF` with opt['engine']['train'] = 'hip' against the model's own stock path in float64 on the same
GPU, the fixtures of tests/golden/skeleton_train_*.npz, the SMPL table against a pndf_train_create handle, determinism, the batch
kernel for any joint count and the cuda trainer on the 15-joint hand.  Reads only fixtures and synth (the reference is not here).

Tolerance rule (tests/test_train_gpu.py's; per loss, per gradient tensor): relative error in the tensor norm <= max(1e-4, 4 x the
stock fp32 run's error against the stock fp64 run); a tensor whose terms cancel is held to 1e-3 x the largest gradient norm."""
import ctypes
import os

import numpy as np
import pytest
import torch

import skeleton_oracle as sko
import skeleton_train_fixtures as stf
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


def _three(parents, act, sd, q, gt, qm, eikonal, hidden=stf.HIDDEN, loss="l1", **kw):
    """(losses, grads) of the HIP run, the stock fp32 run and the stock fp64 run on the GPU"""
    out = []
    for backend, dtype in (("hip", torch.float32), ("torch", torch.float32), ("torch", torch.float64)):
        net = stf.model(parents, act, sd, hidden, loss, backend, dtype, DEV, **kw)
        out.append(stf.run(net, q, gt, qm, eikonal, dtype, DEV)[:2])
    return out


def _compare(tag, parents, act, sd, q, gt, qm, eikonal=1.0, gradients=True, **kw):
    mine, r32, r64 = _three(parents, act, sd, q, gt, qm, eikonal, **kw)
    stf.check(tag, mine, r32, r64, gradients)
    return mine, r32, r64


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["lrelu", "softplus"])
@pytest.mark.parametrize("skel", ["hand", "tree32", "roots5", "chain32"])
def test_parity(skel, act):
    """B = 509, Bm = 383, eikonal on: every loss and every gradient tensor; the fixture cases also against the reference's values"""
    parents, sd = stf.case_network(skel, act)
    q, gt, qm = stf.inputs(parents)
    (l_h, g_h), _, _ = _compare(f"{skel} {act}", parents, act, sd, q, gt, qm)
    assert len(g_h) == 4 * len(parents) + 2 * (len(stf.HIDDEN) + 1)
    if (skel, act) in stf.FIXTURE_CASES:
        z = np.load(stf.fixture_path(skel, act))
        z32 = ({k: z["losses_f32"][i] for i, k in enumerate(stf.LOSS_KEYS)}, {k: z[f"g_f32::{k}"] for k in g_h})
        z64 = ({k: z["losses_f64"][i] for i, k in enumerate(stf.LOSS_KEYS)}, {k: z[f"g_f64::{k}"] for k in g_h})
        stf.check(f"{skel} {act} fixture", (l_h, g_h), z32, z64)


def test_one_joint():
    """Eikonal off: full parity.  Eikonal on: normalising over a one-joint axis leaves signs and the true input gradient is zero, so
    the eikonal seed's direction is rounding noise in any fp32 run: the three losses under the rule (which
    puts `eikonal` within 1e-4 of 1), every gradient finite, the gradients not gated"""
    parents, sd = stf.case_network("one", "lrelu")
    q, gt, qm = stf.inputs(parents)
    _compare("one, eikonal off", parents, "lrelu", sd, q, gt, qm, eikonal=0.0)
    (l_h, g_h), _, _ = _compare("one, eikonal on", parents, "lrelu", sd, q, gt, qm, eikonal=1.0, gradients=False)
    assert abs(l_h["eikonal"] - 1.0) <= 1e-4
    assert all(np.isfinite(g).all() for g in g_h.values())


@pytest.mark.parametrize("variant", ["softplus/lrelu", "lrelu/softplus@7", "l2", "noeik"])
def test_variants_on_the_hand(variant):
    parents = sko.HAND
    q, gt, qm = stf.inputs(parents)
    if variant in ("l2", "noeik"):
        _, sd = stf.case_network("hand", "softplus")
        mine, _, _ = _compare(f"hand {variant}", parents, "softplus", sd, q, gt, qm, eikonal=0.0 if variant == "noeik" else 1.0,
                              loss="l2" if variant == "l2" else "l1")
        if variant == "noeik":      # the loss dict is {"dist"} alone (checked by stf.check against the stock run), and so is the gradient
            assert set(mine[0]) == {"dist"}
            net = stf.model(parents, "softplus", sd, backend="hip", device=DEV)
            t = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
            loss, ld = net(t(q), t(gt), t(qm), train=True, eikonal=0.0)
            assert set(ld) == {"dist"} and ld["dist"] is loss
    else:
        _, sd = stf.case_network("hand", variant)
        _compare(f"hand {variant}", parents, variant, sd, q, gt, qm)


@pytest.mark.parametrize("B,Bm", [(1, 3), (63, 40), (192, 193)])
def test_batch_edges(B, Bm):
    """(192, 193): 385 primal columns, so the encoder's reverse runs a workgroup with one active lane; 577 columns of the NT GEMM"""
    parents, sd = stf.case_network("hand", "softplus")
    q, gt, qm = stf.inputs(parents, B, Bm, seed=11)
    _compare(f"hand B={B} Bm={Bm}", parents, "softplus", sd, q, gt, qm)


def test_split_k():
    """configs/amass.yaml's hidden widths at B = Bm = 2,048: several K slabs per weight gradient, a 90-row first layer against 128-wide
    tiles"""
    from posendf_amd import synth
    hidden = list(synth.DFNET_DIMS[1:-1])
    parents, sd = stf.case_network("hand", "lrelu", hidden)
    q, gt, qm = stf.inputs(parents, 2048, 2048, seed=31)
    _compare("hand split K", parents, "lrelu", sd, q, gt, qm, hidden=hidden)


@pytest.mark.parametrize("act", ["relu", "softplus"])
def test_zero_quaternion_column(act):
    parents, sd = stf.case_network("hand", act)
    q, gt, qm = stf.inputs(parents, 64, 48, seed=21)
    q[3, :, 2] = 0.0                     # one component zero on all 15 joints: the normalisation clamps at eps
    _compare(f"hand zero column {act}", parents, act, sd, q, gt, qm)


# ---- the SMPL table, determinism, the model path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_smpl_table_gives_the_bits_of_pndf_train_create(act):
    from posendf_amd import PoseNDF, synth
    sd, hidden = tf.case_weights("live")
    q, gt, qm = tf.case_inputs()
    a = PoseNDF(tf.config(act, hidden, "l1", DEV, train_backend="hip"))
    b = stf.model(synth.PARENT, act, sd, hidden, backend="hip", device=DEV)
    a.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    la, ga, _ = stf.run(a, q, gt, qm, 1.0, device=DEV)
    lb, gb, _ = stf.run(b, q, gt, qm, 1.0, device=DEV)
    eng_a, eng_b = a._train_engines[0], b._train_engines[0]
    assert eng_a.parents is None and eng_b.parents == tuple(synth.PARENT)      # pndf_train_create / pndf_skel_train_create
    assert la == lb and len(ga) == 98
    assert all(np.array_equal(ga[k], gb[k]) for k in ga), [k for k in ga if not np.array_equal(ga[k], gb[k])][:5]


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_two_calls_are_bit_identical(act):
    parents, sd = stf.case_network("tree32", act)
    q, gt, qm = stf.inputs(parents)
    net = stf.model(parents, act, sd, backend="hip", device=DEV)
    l1, g1, _ = stf.run(net, q, gt, qm, 1.0, device=DEV)
    l2, g2, _ = stf.run(net, q, gt, qm, 1.0, device=DEV)
    assert l1 == l2 and all(np.array_equal(g1[k], g2[k]) for k in g1)


def test_model_path():
    parents, sd = stf.case_network("hand", "lrelu")
    q, gt, qm = (torch.from_numpy(a).to(DEV) for a in stf.inputs(parents))
    net = stf.model(parents, "lrelu", sd, backend="hip", device=DEV)
    d0 = net(q, train=False)["dist_pred"].clone()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    loss, ld = net(q, gt, qm, train=True, eikonal=1.0)
    assert type(loss.grad_fn).__name__ == "TrainObjectiveBackward"
    assert ld["dist"] is loss and set(ld) == set(stf.LOSS_KEYS)
    sum(ld.values()).backward()
    opt.step()
    d1 = net(q, train=False)["dist_pred"]
    assert bool(torch.isfinite(d1).all()) and not torch.equal(d0, d1)
    loss_t, _ = stf.model(parents, "lrelu", sd, device=DEV)(q.clone(), gt, qm, train=True, eikonal=1.0)
    assert type(loss_t.grad_fn).__name__ != "TrainObjectiveBackward"


# ---- pndf_skel_train_batch -----------------------------------------------------------------------------------------------------------
def _batch_case(J, k, num_pts, flip):
    """the inputs and the numpy statement of tests/test_trainer_gpu.py::test_train_batch_against_numpy for J joints"""
    from posendf_amd import synth
    rows, mrows = (40, 1, 1000, 1, 257), (1, 300, 17)
    rng = np.random.default_rng([k, num_pts, flip])
    pose = synth.make_poses(sum(rows), seed=3, signed=True, num_joints=J)
    man = synth.make_poses(sum(mrows), seed=4, signed=True, num_joints=J)
    dist = rng.uniform(0.0, 0.5, (sum(rows), k)).astype(np.float32)
    off, moff = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), np.concatenate([[0], np.cumsum(mrows)]).astype(np.int64)
    item_file, item_man = np.array([2, 1, 4, 0, 3, 2], np.int32), np.array([1, 0, 2, 2, 1, 0], np.int32)
    words = rng.integers(0, 2 ** 32, (len(item_file), 2, num_pts), dtype=np.uint64).astype(np.uint32)
    words[:, :, 0] = 0
    words[:, :, -1] = 2 ** 32 - 1
    want_rows = []
    for side, (files, o) in enumerate(((item_file, off), (item_man, moff))):
        first, length = o[files].astype(np.uint64)[:, None], (o[files + 1] - o[files]).astype(np.uint64)[:, None]
        want_rows.append((first + ((words[:, side].astype(np.uint64) * length) >> np.uint64(32))).astype(np.int64).reshape(-1))
    r, rm = want_rows
    q_want, qm_want = pose[r], man[rm]
    if flip:
        q_want, qm_want = np.where(q_want[..., :1] < 0, -q_want, q_want), np.where(qm_want[..., :1] < 0, -qm_want, qm_want)
    return (pose, dist, man, off, moff, item_file, item_man, words.view(np.int32)), (len(rows), len(mrows)), q_want, qm_want, dist[r].astype(np.float64).mean(1)


def _run_batch(lib, arrays, counts, J, k, num_pts, flip, skel=True):
    from posendf_amd import engine
    t = [torch.from_numpy(a).to(DEV) for a in arrays]
    P, guard = 6 * num_pts, 4
    q = torch.full((P + guard, J, 4), 7.0, dtype=torch.float32, device=DEV)
    qm = torch.full((P + guard, J, 4), 7.0, dtype=torch.float32, device=DEV)
    gt = torch.full((P + guard,), 7.0, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if skel:
        engine.skel_train_batch(*[x.data_ptr() for x in t], *counts, k, 6, num_pts, flip, J, q.data_ptr(), gt.data_ptr(), qm.data_ptr(), st, lib)
    else:
        engine.train_batch(*[x.data_ptr() for x in t], *counts, k, 6, num_pts, flip, q.data_ptr(), gt.data_ptr(), qm.data_ptr(), st, lib)
    torch.cuda.synchronize()
    assert bool((q[P:] == 7.0).all()) and bool((qm[P:] == 7.0).all()) and bool((gt[P:] == 7.0).all())      # nothing behind the buffers
    return q[:P].cpu().numpy(), qm[:P].cpu().numpy(), gt[:P].cpu().numpy()


@pytest.mark.parametrize("k,num_pts,flip", [(5, 70, 1), (16, 1, 0)])
@pytest.mark.parametrize("J", [1, 15, 32])
def test_skel_train_batch_against_numpy(lib, J, k, num_pts, flip):
    arrays, counts, q_want, qm_want, mean = _batch_case(J, k, num_pts, flip)
    q, qm, gt = _run_batch(lib, arrays, counts, J, k, num_pts, flip)
    assert np.array_equal(q, q_want) and np.array_equal(qm, qm_want)
    u = k * 2.0 ** -24
    assert (np.abs(gt.astype(np.float64) - mean) <= u / (1 - u) * mean).all()


def test_skel_train_batch_with_21_joints_is_train_batch(lib):
    arrays, counts, q_want, _, _ = _batch_case(21, 5, 70, 1)
    a = _run_batch(lib, arrays, counts, 21, 5, 70, 1, skel=True)
    b = _run_batch(lib, arrays, counts, 21, 5, 70, 1, skel=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[0], q_want)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def _load(t, sd):
    t.model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})


def test_trainer_trajectory_against_fp64_stock_loop(tmp_path, lib):
    """the hand, 4 files, batch_size 4, num_pts 128 (B = 512), 10 lrelu steps: tests/test_trainer_gpu.py's rule -- per parameter tensor
    |hip - f64| <= 2 |f32 - f64| + 1e-9, the losses within trainer_fixtures.loss_tolerance"""
    from posendf_amd import SkeletonPoseNDF
    steps = 10
    _, sd = stf.case_network("hand", "lrelu")
    t = stf.hand_trainer(tmp_path, files=4, rows=300, device=DEV, batch_size=4, num_pts=128)
    assert isinstance(t.model, SkeletonPoseNDF) and t.hip and t.B == 512 and t.steps_per_epoch == 1 and t._q.shape == (512, 15, 4)
    assert t._engine.parents == sko.HAND and t._engine.num_joints == 15
    _load(t, sd)
    logs = []
    for s in range(steps):
        t.begin_epoch(s)
        t.step()
        logs.append(t.read_log()[:1])
    mine, losses = trf.params(t), np.concatenate(logs)
    cfg = stf.trainer_config(tmp_path, device=DEV, batch_size=4, num_pts=128)
    p32, l32 = stf.stock_loop(t, cfg, sd, steps, torch.float32, DEV)
    p64, l64 = stf.stock_loop(t, cfg, sd, steps, torch.float64, DEV)
    bad, worst = [], 0.0
    for k in p64:
        d_h, d_32 = np.linalg.norm(mine[k] - p64[k]), np.linalg.norm(p32[k] - p64[k])
        worst = max(worst, d_h / max(d_32, 1e-30))
        if not d_h <= 2.0 * d_32 + 1e-9:
            bad.append((k, d_h, d_32))
    print(f"[hand trajectory {steps} steps] worst |hip - f64| / |f32 - f64| over the parameter tensors: {worst:.3f}")
    assert not bad, bad[:8]
    lbad = [(s, c, losses[s, c], l64[s, c]) for s in range(steps) for c in range(3)
            if not abs(losses[s, c] - l64[s, c]) / abs(l64[s, c]) <= trf.loss_tolerance(l32[s, c], l64[s, c])]
    assert not lbad, lbad[:8]


def test_trainer_same_seed_same_bits_and_resume(tmp_path, lib):
    kw = dict(files=7, rows=60, device=DEV, batch_size=3, num_pts=96)      # two steps per epoch
    one, two = stf.hand_trainer(tmp_path / "a", seed=3, **kw), stf.hand_trainer(tmp_path / "b", seed=3, **kw)
    r = [(one.train_model(e), two.train_model(e)) for e in range(2)]
    assert all(x == y for x, y in r) and all(np.isfinite(x).all() for x, _ in r)
    pa, pb = trf.params(one), trf.params(two)
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    # one epoch + checkpoint + a new trainer with continue_train + one epoch
    first = stf.hand_trainer(tmp_path / "c", seed=3, **kw)
    assert first.train_model(0) == r[0][0]
    del first
    resumed = stf.hand_trainer(tmp_path / "c", seed=3, continue_train=True, **kw)
    assert resumed.ep == 1 and resumed.iter_nums == one.steps_per_epoch == 2
    assert resumed.train_model(1) == r[1][0]
    pc = trf.params(resumed)
    assert all(np.array_equal(pa[k], pc[k]) for k in pa)
    ma, mc = trf.adam_state(one), trf.adam_state(resumed)
    assert all(np.array_equal(ma[k][0], mc[k][0]) and np.array_equal(ma[k][1], mc[k][1]) for k in ma)
