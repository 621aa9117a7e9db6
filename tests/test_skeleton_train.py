"""Training other skeletons (include/posendf_amd_skeleton_train.h), the parts that run without a GPU: the oracle
pinned against the reference's own classes, the header against the signature table, what the new create and the batch call refuse,
the data set's shapes, the model's knob and the trainer's cpu backend on the 15-joint hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cabi_headers as ch
import skeleton_oracle as sko
import skeleton_train_fixtures as stf
import test_net_plan as tnp

OK, BAD_ARG, UNSUPPORTED, NO_DEVICE = 0, -1, -4, -6
ACCEPTED = OK if torch.cuda.is_available() else NO_DEVICE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


# ------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("skel,act", stf.FIXTURE_CASES, ids=[f"{s}-{a}" for s, a in stf.FIXTURE_CASES])
def test_stock_fp64_path_equals_the_reference(skel, act):
    """the stock train=True path of SkeletonPoseNDF in float64 against the reference's own StructureEncoder, DFNet and gradient
    composed for J joints (tests/golden/make_golden_skeleton_train.py): 1e-9 relative, the bound skeleton_oracle holds"""
    z = np.load(stf.fixture_path(skel, act))
    parents, sd = stf.case_network(skel, act)
    assert tuple(z["parents"]) == tuple(parents) and z["q"].shape == (stf.B, len(parents), 4) and z["q_man"].shape == (stf.BM, len(parents), 4)
    q, gt, qm = stf.inputs(parents)
    assert np.array_equal(q, z["q"]) and np.array_equal(gt, z["dist_gt"]) and np.array_equal(qm, z["q_man"])
    net = stf.model(parents, act, sd, dtype=torch.float64)
    losses, grads, _ = stf.run(net, q, gt, qm, 1.0, torch.float64)
    for i, k in enumerate(stf.LOSS_KEYS):
        assert abs(losses[k] - z["losses_f64"][i]) <= 1e-9 * abs(z["losses_f64"][i]), (k, losses[k], z["losses_f64"][i])
    assert set(grads) == {k[len("g_f64::"):] for k in z.files if k.startswith("g_f64::")}
    scale = max(np.linalg.norm(z[f"g_f64::{k}"]) for k in grads)
    for k, g in grads.items():
        assert stf.rel(g, z[f"g_f64::{k}"], 1e-3 * scale) <= 1e-9, k


# ------------------------------------------------------------------------------------------ 2. the header
def test_header_matches_the_signature_table(tmp_path):
    """pndf_skel_train_batch takes pndf_train_batch's parameters with num_joints after `flip`, and the header's types in a C call; the
    header against its table is tests/test_cabi.py's"""
    from posendf_amd import abi
    batch = abi.HEADERS["posendf_amd.h"]["pndf_train_batch"][1]
    skel_batch = abi.HEADERS["posendf_amd_skeleton_train.h"]["pndf_skel_train_batch"][1]
    assert list(skel_batch) == list(batch[:14]) + [ctypes.c_int32] + list(batch[14:])
    ok, diagnostics = ch.compiles_as_c99(tmp_path, '#include "posendf_amd_skeleton_train.h"\nint main(void) { pndf_train_handle h = 0; pndf_config c; '
                                         "return pndf_skel_train_create(&h, &c, 0) + (int)sizeof(pndf_config) * 0; }\n")
    assert ok, diagnostics


# ------------------------------------------------------------------------------------------ 3. refusals
def _skel_train_create(lib, cfg):
    h = ctypes.c_void_p()
    rc = lib.pndf_skel_train_create(ctypes.byref(h), ctypes.byref(cfg), 0)
    text = lib.pndf_train_last_error(None)
    if rc == OK:
        assert h.value and lib.pndf_train_destroy(h) == OK
    else:
        assert not h.value
    return rc, text


@pytest.mark.parametrize("row", tnp.TABLE, ids=[r[0] for r in tnp.TABLE])
def test_create_against_the_single_fault_table(lib, row):
    """tests/test_net_plan.py's table: every row pndf_train_create refuses is refused, except "20 joints", which this create is for"""
    name, fault, want = row
    cfg = tnp.base_config(lib)
    fault(cfg)
    rc, text = _skel_train_create(lib, cfg)
    if name == "20 joints":
        assert rc == ACCEPTED, (rc, text)
        rc_smpl, text_smpl = tnp.run_create(lib, "pndf_train_create", cfg)
        assert rc_smpl == UNSUPPORTED and b"num_joints" in text_smpl
    elif want[0] == UNSUPPORTED:
        assert rc == UNSUPPORTED and text, (name, rc, text)
        assert (rc, text) == tnp.run_create(lib, "pndf_train_create", cfg)
    else:
        assert rc == ACCEPTED, (name, rc, text)


def test_create_other_trees_and_the_encoderless_text(lib):
    from posendf_amd import engine
    for parents, hidden in ((sko.HAND, sko.HIDDEN), (sko.TREE32, [1024]), (sko.ONE, [1]), (sko.CHAIN32, [8] * 7), (sko.ROOTS5, sko.HIDDEN)):
        rc, text = _skel_train_create(lib, engine._network_config(lib, "softplus", 100.0, hidden=list(hidden), parents=parents))
        assert rc == ACCEPTED, (parents, rc, text)
    # the SMPL table is accepted like pndf_train_create's
    assert _skel_train_create(lib, tnp.base_config(lib))[0] == ACCEPTED
    # without the encoder: the text pndf_train_create gives
    rc, text = _skel_train_create(lib, engine._network_config(lib, "lrelu", 100.0, hidden=list(sko.HIDDEN), parents=sko.HAND, encoder=False))
    rc21, text21 = tnp.run_create(lib, "pndf_train_create", engine._network_config(lib, "lrelu", 100.0, encoder=False))
    assert rc == rc21 == UNSUPPORTED and text == text21 and b"structure encoder" in text
    assert lib.pndf_skel_train_create(None, None, 0) == BAD_ARG
    if not torch.cuda.is_available():
        with pytest.raises(engine.PndfError, match="pndf_skel_train_create"):
            engine.TrainEngine("lrelu", hidden=sko.HIDDEN, parents=sko.HAND)


def test_batch_refuses_joint_counts_outside_1_to_32(lib):
    """decided before any pointer is looked at"""
    buf = np.zeros(64, np.float32)
    off = np.array([0, 1], np.int64)
    idx = np.zeros(4, np.int32)
    p = buf.ctypes.data

    def call(nj):
        return lib.pndf_skel_train_batch(p, p, p, off.ctypes.data, off.ctypes.data, idx.ctypes.data, idx.ctypes.data, idx.ctypes.data,
                                         1, 1, 1, 0, 1, 0, nj, p, p, p, None)
    assert call(0) == BAD_ARG and call(33) == BAD_ARG and call(-1) == BAD_ARG
    assert call(1) == OK and call(15) == OK and call(32) == OK      # items == 0: a no-op, nothing launched


# ------------------------------------------------------------------------------------------ 4. the data set
def test_dataset_shapes():
    from posendf_amd import synth
    from posendf_amd.trainer import PoseDataset
    hand = synth.make_poses(8, seed=1, num_joints=15)
    smpl = synth.make_poses(8, seed=1)
    d = np.zeros((8, 5), np.float32)
    ds = PoseDataset.from_arrays([hand, hand], [d, d], [hand], num_joints=15)
    assert ds.num_joints == 15 and ds.pose.shape == (16, 15, 4) and ds.man.shape == (8, 15, 4)
    assert ds.nbytes == 4 * (16 * 60 + 16 * 5 + 8 * 60) + 8 * (3 + 2)
    with pytest.raises(ValueError, match=r"<data 1>.*expected \[n, 15, 4\]"):
        PoseDataset.from_arrays([hand, smpl], [d, d], [hand], num_joints=15)
    with pytest.raises(ValueError, match=r"<manifold 0>.*expected \[n, 15, 4\]"):
        PoseDataset.from_arrays([hand], [d], [hand.reshape(8, 60)], num_joints=15)
    with pytest.raises(ValueError, match=r"<data 0>.*expected \[n, 21, 4\]"):
        PoseDataset.from_arrays([hand], [d], [hand])
    assert PoseDataset.from_arrays([smpl], [d], [smpl]).num_joints == 21


def test_dataset_files_name_the_file(tmp_path):
    from posendf_amd import synth
    from posendf_amd.trainer import PoseDataset
    hand = synth.make_poses(8, seed=1, num_joints=15)
    for sub in ("data/a", "man/a"):
        os.makedirs(tmp_path / sub)
    np.savez(tmp_path / "data/a/s0.npz", pose=hand, dist=np.zeros((8, 5), np.float32))
    np.savez(tmp_path / "man/a/m0.npz", pose=hand)
    ds = PoseDataset(str(tmp_path / "data"), str(tmp_path / "man"), num_joints=15)
    assert ds.pose.shape == (8, 15, 4)
    with pytest.raises(ValueError, match=r"s0\.npz.*expected \[n, 21, 4\]"):
        PoseDataset(str(tmp_path / "data"), str(tmp_path / "man"))


# ------------------------------------------------------------------------------------------ 5. the model's knob
def test_the_train_knob_of_a_skeleton_model():
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    from posendf_amd.engine import PndfError
    cfg = skeleton_config("hand", "lrelu", "cpu", hidden=sko.HIDDEN)
    cfg["engine"] = {"train": "gpu"}
    with pytest.raises(ValueError, match="must be 'torch' or 'hip'"):
        SkeletonPoseNDF(cfg)
    cfg = skeleton_config("hand", "lrelu", "cpu", hidden=sko.HIDDEN, encoder=False)
    cfg["engine"] = {"train": "hip"}
    with pytest.raises(PndfError, match="structure encoder"):
        SkeletonPoseNDF(cfg)
    cfg = skeleton_config("hand", "lrelu", "cpu", hidden=sko.HIDDEN)
    cfg["engine"] = {"train": "hip"}
    net = SkeletonPoseNDF(cfg)      # a cpu model keeps the stock path either way
    q, gt, qm = stf.inputs(sko.HAND, 9, 7)
    loss, ld = net(torch.from_numpy(q), torch.from_numpy(gt), torch.from_numpy(qm), train=True, eikonal=1.0)
    assert type(loss.grad_fn).__name__ != "TrainObjectiveBackward" and set(ld) == set(stf.LOSS_KEYS)


# ------------------------------------------------------------------------------------------ 6. the trainer, cpu backend
def test_cpu_trainer_on_the_hand(tmp_path):
    from posendf_amd import SkeletonPoseNDF
    from posendf_amd.trainer import WEIGHT_DECAY
    t = stf.hand_trainer(tmp_path, files=3, rows=40, seed=5)
    assert isinstance(t.model, SkeletonPoseNDF) and t.num_joints == 15 and not t.hip and t.B == 48 and t.steps_per_epoch == 1
    start = {k: v.clone() for k, v in t.model.state_dict().items()}
    for ep in range(2):
        t.begin_epoch(ep)
        t.step()
    # the hand-written stock loop from the same weights on the same batches
    net = SkeletonPoseNDF(stf.trainer_config(tmp_path))
    net.load_state_dict(start)
    opt = torch.optim.Adam(net.parameters(), lr=stf.LR, weight_decay=WEIGHT_DECAY)
    for ep in range(2):
        pose, gt, man = t.batch(ep, 0)
        assert pose.shape == (48, 15, 4) and man.shape == (48, 15, 4)
        opt.zero_grad()
        _, ld = net(pose, gt, man, train=True, eikonal=1.0)
        loss = 0.0
        for k in ld.keys():
            loss += 1.0 * ld[k]
        loss.backward()
        opt.step()
    mine, want = dict(t.model.named_parameters()), dict(net.named_parameters())
    assert len(mine) == 4 * 15 + 2 * 3
    assert all(torch.equal(mine[k].detach(), want[k].detach()) for k in want)
    assert not torch.equal(mine["dfnet.lin0.weight"].detach(), start["dfnet.lin0.weight"])


def test_online_data_needs_the_smpl_table(tmp_path):
    from posendf_amd.engine import PndfError
    from posendf_amd.trainer import Trainer
    cfg = stf.trainer_config(tmp_path)
    cfg["data"]["online"] = {"files": 3, "rows": 16}
    with pytest.raises(PndfError, match="21-joint"):
        Trainer(cfg, seed=0)
