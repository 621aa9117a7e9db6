"""Other skeletons on the host (include/posendf_amd_skeleton.h): the numpy oracle for any parent table pinned
against oracle.posendf_np (SMPL) and against the reference's own autograd on a hand and a 32-joint tree
(tests/golden/make_golden_skeleton.py); `SkeletonPoseNDF` on a cpu model; the generalised first-order host twins through
`CpuEngine(parents=...)`; the refusals of pndf_skel_create / pndf_cpu_create; the companion header.  Runs without a GPU;
tests/test_skeleton_gpu.py holds the HIP unit to the same gates."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cabi_headers as ch
import skeleton_oracle as sko
from conftest import d_rows, golden_weights, pose_gate, rel_err_rows
from oracle import posendf_np as onp
from posendf_amd import synth

UNSUPPORTED, NO_DEVICE = -4, -6


def load_fixture(skel, act):
    g = dict(np.load(sko.fixture_path(skel, act)))
    parents = tuple(int(p) for p in g["parents"])
    assert parents == sko.SKELETONS[skel]
    return g, parents, sko.network(parents, int(g["seed"]))


# ------------------------------------------------------------------------------------------ 1. the oracle is pinned
@pytest.mark.parametrize("act", ["lrelu", "relu", "softplus"])
def test_oracle_equals_posendf_np_on_the_smpl_table(act):
    sd = golden_weights("live")
    q = synth.make_poses(40, seed=11)
    d0, g0 = onp.forward_grad(q, sd, act, dtype=np.float64)
    d1, g1 = sko.forward_grad(q, sd, act, synth.PARENT, np.float64)
    assert np.abs(d1 - d0).max() <= 1e-12 * max(np.abs(d0).max(), 1.0) and rel_err_rows(g1, g0).max() <= 1e-12
    assert np.array_equal(sko.forward(q, sd, act, synth.PARENT, np.float64), d1)
    q0, dl0 = onp.project(q, sd, steps=3, act=act, dtype=np.float64)
    q1, dl1 = sko.project(q, sd, 3, act, synth.PARENT, np.float64)
    assert rel_err_rows(q1, q0).max() <= 1e-12 and np.abs(dl1 - dl0.reshape(-1)).max() <= 1e-12 * max(np.abs(dl0).max(), 1.0)


@pytest.mark.parametrize("skel,act", sko.FIXTURE_CASES)
def test_oracle_equals_the_reference_on_the_fixtures(skel, act):
    g, parents, sd = load_fixture(skel, act)
    q = g["q"]
    assert np.array_equal(q, sko.poses(parents)) and os.path.getsize(sko.fixture_path(skel, act)) < 1 << 20
    assert int((g["d_f64"] == 0).sum()) * 4 <= len(q)      # the generator's promise: the network is not clipped to zero
    d64, g64 = sko.forward_grad(q, sd, act, parents, np.float64)
    assert np.abs(d64 - g["d_f64"]).max() <= 1e-9 * max(np.abs(g["d_f64"]).max(), 1.0)
    assert rel_err_rows(g64, g["dq_f64"]).max() <= 1e-9
    q3, _ = sko.project(q, sd, sko.STEPS, act, parents, np.float64)
    assert rel_err_rows(q3, g["q3_f64"]).max() <= 1e-9
    # the envelope must not fail the reference itself: its own fp32 run under the gates every implementation is held to
    sko.gate(g["d_f32"], g["dq_f32"], q, sd, act, parents, f"reference fp32 {skel} {act}")


# ------------------------------------------------------------------------------------------ 2. SkeletonPoseNDF on cpu
def cpu_model(parents, act, sd, encoder=True):
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    net = SkeletonPoseNDF(skeleton_config(list(parents), act, "cpu", hidden=sko.HIDDEN, encoder=encoder))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.eval()


@pytest.mark.parametrize("skel,act", sko.FIXTURE_CASES)
def test_model_on_cpu(skel, act):
    g, parents, sd = load_fixture(skel, act)
    net = cpu_model(parents, act, sd)
    mine = net.state_dict()
    assert list(mine.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(n) for n in v.shape) for v in mine.values()] == [str(s) for s in g["shapes"]]
    q = torch.from_numpy(g["q"]).requires_grad_(True)
    d = net(q, train=False)["dist_pred"]
    assert d.shape == (len(g["q"]), 1)
    (dq,) = torch.autograd.grad(d.sum(), q)
    sko.gate(d.detach().numpy(), dq.numpy(), g["q"], sd, act, parents, f"cpu model {skel} {act}")
    with pytest.raises(RuntimeError):      # first order only
        qq = torch.from_numpy(g["q"][:4]).requires_grad_(True)
        (g1,) = torch.autograd.grad(net(qq, train=False)["dist_pred"].sum(), qq, create_graph=True)
        g1.sum().backward()
    q3, dl = net.project(torch.from_numpy(g["q"]), steps=sko.STEPS)
    o3, ol = sko.project(g["q"], sd, sko.STEPS, act, parents, np.float64)
    assert q3.shape == g["q"].shape and dl.shape == (len(g["q"]), 1)
    assert np.median(rel_err_rows(q3.numpy(), o3)) <= 1e-5 and np.median(d_rows(dl.numpy(), ol)) <= 1e-5
    # train=True runs the stock modules: the loss has a gradient for every parameter
    loss, _ = net(torch.from_numpy(g["q"]), dist_gt=torch.zeros(len(g["q"])), man_poses=torch.from_numpy(g["q"]), train=True, eikonal=1.0)
    loss.backward()
    assert all(p.grad is not None for p in net.parameters())


def test_absent_parent_mapping_is_the_smpl_tree():
    from posendf_amd import PoseNDF, SkeletonPoseNDF, amass_config
    from posendf_amd.modules import StructureEncoder
    cfg = amass_config("lrelu", "cpu")
    assert "parent_mapping" not in cfg["model"]["StrEnc"]
    enc = StructureEncoder(cfg["model"]["StrEnc"])
    assert enc.parent_mapping == list(synth.PARENT) and enc.num_joints == 21 and enc.out_dim == 126
    a, b = PoseNDF(cfg).state_dict(), SkeletonPoseNDF(cfg).state_dict()
    assert list(a.keys()) == list(b.keys()) == list(synth.state_dict_shapes().keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) == synth.state_dict_shapes()[k] for k in a)
    hand = StructureEncoder(dict(cfg["model"]["StrEnc"], parent_mapping=list(sko.HAND)))
    assert hand.num_joints == 15 and hand.out_dim == 90
    with pytest.raises(ValueError):
        StructureEncoder(dict(cfg["model"]["StrEnc"], parent_mapping=[-1, 1]))
    # the defaults of synth are unchanged
    assert synth.make_poses(3, seed=2).shape == (3, 21, 4) and synth.make_poses(3, seed=2, num_joints=15).shape == (3, 15, 4)
    assert list(synth.state_dict_shapes(synth.skeleton_dims(sko.HAND, [8]), sko.HAND))[-2:] == ["dfnet.lin1.weight", "dfnet.lin1.bias"]


# ------------------------------------------------------------------------------------------ 3. the host twins
def cpu_engine(parents, act, sd, encoder=True):
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine(act, encoder=encoder, hidden=sko.HIDDEN, parents=parents)
    eng.load_weights(sd)
    return eng


def twin_forward_grad(eng, q, grad_out=None):
    q = np.ascontiguousarray(q, np.float32)
    d, dq = np.full(len(q), 7.0, np.float32), np.full(q.shape, 7.0, np.float32)
    eng.forward_grad(q.ctypes.data, None if grad_out is None else grad_out.ctypes.data, d.ctypes.data, dq.ctypes.data, len(q))
    return d, dq


def twin_project(eng, q, steps, **opts):
    q = np.ascontiguousarray(q, np.float32)
    out, d = np.full(q.shape, 7.0, np.float32), np.full(len(q), 7.0, np.float32)
    eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), steps, step_size=opts.get("step_size", 1.0),
                renorm=opts.get("renormalize"), tol=opts.get("tol", 0.0))
    return out, d


@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", sko.CASES, ids=sko.case_id)
def test_host_twin(case, act):
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    q = sko.case_poses(case)
    eng = cpu_engine(parents, act, sd, encoder=case[1])
    d, dq = twin_forward_grad(eng, q)
    sko.gate(d, dq, q, sd, act, parents, f"host twin {sko.case_id(case)} {act}")
    d_only = np.full(len(q), 7.0, np.float32)
    eng.forward(q.ctypes.data, d_only.ctypes.data, len(q))
    assert d_only.tobytes() == d.tobytes()
    # grad_out scales dq: powers of two, both signs, to the bit
    i = np.arange(len(q))
    go = ((-1.0) ** i * 2.0 ** (i % 5 - 2)).astype(np.float32)
    d2, dq2 = twin_forward_grad(eng, q, go)
    normal = np.abs(dq) > 2.0 ** -100      # (a product that lands among the subnormals is rounded)
    assert d2.tobytes() == d.tobytes() and np.array_equal(dq2[normal], (dq * go[:, None, None])[normal])
    # the step options: K rounds of forward_grad + the numpy statement of the step, to the bit; with a tolerance some poses rest
    tol = float(np.median(d))
    for opts in (dict(), dict(renormalize="unit", tol=tol), dict(renormalize="unit_flip", step_size=0.5, tol=tol)):
        want = q.copy()
        for _ in range(2):
            dk, gk = twin_forward_grad(eng, want)
            want = sko.step(want, dk, gk, J, **opts)
        got, dl = twin_project(eng, q, 2, **opts)
        assert got.tobytes() == want.tobytes() and dl.tobytes() == dk.tobytes(), opts
        if "tol" in opts:
            rest = d < np.float32(tol)
            assert rest.any() and not rest.all()
            assert got[rest].tobytes() == q[rest].tobytes() and not np.array_equal(got[~rest], q[~rest])


def test_the_other_twins_stay_21_joint():
    parents, sd = sko.case_network(("hand", True), "lrelu")
    eng = cpu_engine(parents, "lrelu", sd)
    q = sko.poses(parents, 4)
    out, d = np.empty_like(q), np.empty(4, np.float32)
    lib = eng.lib
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, None, out.ctypes.data, d.ctypes.data, 4, 1, None) == UNSUPPORTED
    assert b"21-joint" in lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_second_order_cpu(eng.handle, q.ctypes.data, q.ctypes.data, None, None, None, None, None, out.ctypes.data, 4) == UNSUPPORTED
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q.ctypes.data, None, out.ctypes.data, None, 1, 2, 0, 0, 0.0, None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ 4. refusals
def hand_config(lib, **kw):
    from posendf_amd import engine
    return engine._network_config(lib, "lrelu", 100.0, hidden=list(sko.HIDDEN), parents=sko.HAND, **kw)


def _bad_configs(lib):
    from posendf_amd import engine
    def edit(field, fn, **kw):
        cfg = hand_config(lib, **kw)
        fn(cfg)
        return field, cfg
    yield edit(b"num_joints", lambda c: setattr(c, "num_joints", 0))
    yield edit(b"num_joints", lambda c: setattr(c, "num_joints", 33))
    yield edit(b"parent", lambda c: c.parent.__setitem__(4, 4))
    yield edit(b"parent", lambda c: c.parent.__setitem__(2, -2))
    yield edit(b"dims[0]", lambda c: c.dims.__setitem__(0, 126))
    yield b"dims", engine._network_config(lib, "lrelu", 100.0, hidden=[8] * 7, parents=sko.HAND)      # (seven hidden layers: accepted below)


def test_create_refusals_name_the_field():
    from posendf_amd import engine
    lib = engine.load_library()
    h = ctypes.c_void_p()
    creates = (("skel", lambda cfg: lib.pndf_skel_create(ctypes.byref(h), ctypes.byref(cfg), 0), lambda: lib.pndf_skel_last_error(None)),
               ("cpu", lambda cfg: lib.pndf_cpu_create(ctypes.byref(h), ctypes.byref(cfg)), lambda: lib.pndf_cpu_last_error(None)))
    for which, create, text in creates:
        for field, cfg in list(_bad_configs(lib))[:-1]:
            assert create(cfg) == UNSUPPORTED and not h, (which, field)
            assert field in text(), (which, field, text())
        cfg = hand_config(lib)      # eight hidden layers
        cfg.n_dims = 10
        for i in range(1, 9):
            cfg.dims[i] = 8
        cfg.dims[9] = 1
        assert create(cfg) == UNSUPPORTED and b"n_dims" in text(), which
    cfg = hand_config(lib, precision="f16x3")
    assert lib.pndf_skel_create(ctypes.byref(h), ctypes.byref(cfg), 0) == UNSUPPORTED and b"precision" in lib.pndf_skel_last_error(None)
    # accepted: the device decides; seven hidden layers, 32 joints, one joint, no encoder
    for cfg in (hand_config(lib), hand_config(lib, encoder=False), list(_bad_configs(lib))[-1][1],
                engine._network_config(lib, "softplus", 100.0, hidden=[1024], parents=sko.TREE32),
                engine._network_config(lib, "relu", 100.0, hidden=[1], parents=sko.ONE)):
        rc = lib.pndf_skel_create(ctypes.byref(h), ctypes.byref(cfg), 0)
        assert rc == (0 if torch.cuda.is_available() else NO_DEVICE), lib.pndf_skel_last_error(None)
        if rc == 0:
            assert lib.pndf_skel_destroy(h) == 0
        h = ctypes.c_void_p()
        assert lib.pndf_cpu_create(ctypes.byref(h), ctypes.byref(cfg)) == 0 and lib.pndf_cpu_destroy(h) == 0
        h = ctypes.c_void_p()
    # the persistent engine keeps refusing another skeleton, and says where to go
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(hand_config(lib)), 0) == UNSUPPORTED
    assert b"pndf_skel_create" in lib.pndf_last_error(None)
    assert lib.pndf_skel_create(None, None, 0) == -1 and lib.pndf_skel_destroy(None) == 0
    assert lib.pndf_skel_workspace_bytes(None, 4) == -1
    assert lib.pndf_skel_forward(None, None, None, 4, None, 0, None) == -1
    if not torch.cuda.is_available():
        with pytest.raises(engine.PndfError):
            engine.SkeletonEngine(sko.HAND, hidden=sko.HIDDEN)


# ------------------------------------------------------------------------------------------ 5. the header
def test_header_matches_the_signature_table(tmp_path):
    """what the skeleton unit adds to the build, and its handle type in a C call; its header against its table is tests/test_cabi.py's"""
    import __graft_entry__ as ge
    from posendf_amd import engine
    assert "pndf_experiment_word_skeleton" in engine.EXPERIMENT_WORDS and "pndf_skeleton.hip" in ge.PRODUCT_SOURCES
    ok, diagnostics = ch.compiles_as_c99(tmp_path, '#include "posendf_amd_skeleton.h"\nint main(void) { pndf_skel_handle h = 0; '
                                         "return pndf_skel_destroy(h) + (int)sizeof(pndf_config) * 0; }\n")
    assert ok, diagnostics
