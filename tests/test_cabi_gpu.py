"""GPU checks of the C ABI's host layer on live handles: a call refused by an argument check leaves its text on the HANDLE
(not in the thread's null-handle slot, csrc/pndf_error.h), and the handle works afterwards exactly as before -- one refusal per
handle family, each at the smallest shape (one pose, one index row, S = T = 1).  Nothing here launches a kernel on bad data: every
refusal comes from a check ahead of the launch.  And the ordering of launches that share a handle's scratch across streams
(csrc/pndf_host.h PndfScratchOrder) on the runtime-planned kernels; tests/test_gpu_parity.py test_side_stream_and_graph_capture
holds the fused ones to the same."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAD_ARG, NO_WEIGHTS = -1, -5


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def _stream():
    from posendf_amd import engine
    return engine.stream_handle(DEV)


def _one_pose(seed=3):
    from posendf_amd import synth
    return torch.from_numpy(synth.make_poses(1, seed=seed)).to(DEV).reshape(1, 84).contiguous()


def _refused(obj, call, code, text):
    """`call()` on the live handle of `obj` returns `code`; `text` is on the handle, the thread's null-handle slot keeps its own"""
    last_error = getattr(obj.lib, obj._last_error)
    null_before = last_error(None)
    assert null_before != b"" and null_before != text      # (the caller left a refused create's text there)
    assert call() == code
    assert last_error(obj.handle) == text, last_error(obj.handle)
    assert last_error(None) == null_before


def _engine_outputs(eng, q):
    d, dq, qp, dl = (torch.empty(1, device=DEV), torch.empty_like(q), torch.empty_like(q), torch.empty(1, device=DEV))
    eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), 1, _stream())
    eng.project(q.data_ptr(), qp.data_ptr(), dl.data_ptr(), 1, 2, _stream())
    torch.cuda.synchronize()
    return d, dq, qp, dl


def test_engine_refusal_stays_on_the_handle(lib):
    """fused fp32 relu kernel: a pose pointer 4 bytes off its 16-byte alignment"""
    from posendf_amd import engine, synth
    assert lib.pndf_create(None, None, 0) == BAD_ARG      # "out is null" in the null-handle slot
    eng = engine.Engine("relu", device=0, lib=lib, precision="fp32")
    eng.load_weights(synth.make_weights(0, 2.0, 0.1))
    assert eng.kernel_name() == "pndf_fused_relu_kernel"
    buf = torch.zeros(88, device=DEV)      # (the misaligned pointer stays inside an allocation; the call never reads it)
    q = _one_pose()
    before = _engine_outputs(eng, q)
    d = torch.empty(1, device=DEV)
    _refused(eng, lambda: lib.pndf_forward(eng.handle, buf.data_ptr() + 4, d.data_ptr(), 1, _stream()), BAD_ARG,
             b"pose buffers must be 16-byte aligned")
    after = _engine_outputs(eng, q)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.isfinite(before[0]).all() and not torch.equal(before[2], q)
    eng.close()


def test_runtime_planned_engine_refusal_stays_on_the_handle(lib):
    """dims 126, 16, 1 (the runtime-planned kernels): pndf_project before pndf_load_weights; once the weights are loaded the
    handle gives the bits of a handle that was never refused"""
    from posendf_amd import engine, synth
    assert lib.pndf_create(None, None, 0) == BAD_ARG
    sd = synth.make_weights(0, 2.0, 0.1, dims=(126, 16, 1))
    q = _one_pose()
    clean = engine.Engine("relu", device=0, lib=lib, precision="fp32", hidden=[16])
    clean.load_weights(sd)
    assert clean.kernel_name() == "pndf_generic_relu_kernel"
    want = _engine_outputs(clean, q)
    eng = engine.Engine("relu", device=0, lib=lib, precision="fp32", hidden=[16])
    qp, dl = torch.empty_like(q), torch.empty(1, device=DEV)
    _refused(eng, lambda: lib.pndf_project(eng.handle, q.data_ptr(), qp.data_ptr(), dl.data_ptr(), 1, 2, _stream()), NO_WEIGHTS,
             b"pndf_load_weights has not been called")
    eng.load_weights(sd)
    got = _engine_outputs(eng, q)
    assert all(torch.equal(a, b) for a, b in zip(want, got)) and torch.isfinite(want[0]).all()
    clean.close()
    eng.close()


def test_knn_refusal_stays_on_the_handle(lib):
    """an index of one pose asked for two neighbours"""
    from posendf_amd import engine
    h = ctypes.c_void_p()
    assert lib.pndf_knn_create(ctypes.byref(h), None, 1, 2, None, None) == -4      # "metric: ..." in the null-handle slot
    db, q = _one_pose(5), _one_pose(6)
    index = engine.KnnIndex(db.data_ptr(), 1, lib=lib, stream=_stream())
    ws = torch.empty(max(index.workspace_bytes(1, 1), 16), dtype=torch.uint8, device=DEV)

    def search():
        vals, idx = torch.full((1, 1), -1.0, device=DEV), torch.full((1, 1), -7, dtype=torch.int64, device=DEV)
        index.search(q.data_ptr(), 1, 1, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        return vals, idx
    before = search()
    vals2, idx2 = torch.empty(1, 2, device=DEV), torch.empty(1, 2, dtype=torch.int64, device=DEV)
    _refused(index, lambda: lib.pndf_knn_search(index.handle, q.data_ptr(), 1, 2, vals2.data_ptr(), idx2.data_ptr(), ws.data_ptr(), _stream()),
             BAD_ARG, b"k = 2 exceeds the index size 1")
    after = search()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert int(before[1][0, 0]) == 0 and float(before[0][0, 0]) >= 0.0
    index.close()


def test_train_refusal_stays_on_the_handle(lib):
    """a loss type that does not exist"""
    from posendf_amd import engine, synth
    h = ctypes.c_void_p()
    assert lib.pndf_train_create(ctypes.byref(h), None, 0) == BAD_ARG      # "out / cfg is null" in the null-handle slot
    sd = synth.make_weights(0, 2.0, 0.1, dims=(126, 16, 1))
    eng = engine.TrainEngine("lrelu", device=0, lib=lib, hidden=[16])
    weights = [torch.from_numpy(sd[k]).to(DEV).contiguous() for k in engine.state_dict_order(True, 2)]
    ptrs = [w.data_ptr() for w in weights]
    q, qm, gt = _one_pose(7), _one_pose(8), torch.full((1,), 0.25, device=DEV)
    ws = torch.empty(eng.workspace_floats(1, 1, False), device=DEV)

    def forward(loss_type):
        losses = torch.full((3,), float("nan"), device=DEV)
        rc = lib.pndf_train_forward(eng.handle, eng._table(ptrs), q.data_ptr(), gt.data_ptr(), qm.data_ptr(), 1, 1, loss_type, 0,
                                    losses.data_ptr(), ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        return rc, losses
    rc, before = forward(0)
    assert rc == 0 and torch.isfinite(before[:2]).all()
    _refused(eng, lambda: forward(2)[0], BAD_ARG, b"loss_type: 0 (l1) or 1 (l2)")
    rc, after = forward(0)
    assert rc == 0 and torch.equal(before, after)
    eng.close()


def test_body_model_refusal_stays_on_the_handle(lib):
    """the 41-vertex synthetic model of tests/test_lbs_gpu.py: a workspace 4 bytes off its 16-byte alignment"""
    from oracle import lbs_np
    from posendf_amd import BodyModel
    h = ctypes.c_void_p()
    assert lib.pndf_lbs_create(ctypes.byref(h), 0, 0, *([None] * 8), 0, 0) == BAD_ARG      # "V < 1" in the null-handle slot
    m = lbs_np.synthetic_model(V=41, seed=5, extra=(3, 17, 40))
    bm = BodyModel(m, device="cuda:0")
    assert bm.lib.pndf_lbs_last_error(None) == lib.pndf_lbs_last_error(None)      # (one library, one slot)
    theta = (torch.from_numpy(np.random.default_rng(2).normal(size=(1, 69)).astype(np.float32)) * 0.2).to(DEV)
    ws = torch.empty(int(lib.pndf_lbs_workspace_floats(bm.handle, 1, 1)) + 4, device=DEV)

    def forward(ws_ptr):
        verts, joints = torch.empty(1, 41, 3, device=DEV), torch.empty(1, 27, 3, device=DEV)
        rc = lib.pndf_lbs_forward(bm.handle, theta.data_ptr(), 1, verts.data_ptr(), joints.data_ptr(), ws_ptr, _stream())
        torch.cuda.synchronize()
        return rc, verts, joints
    rc, v0, j0 = forward(ws.data_ptr())
    assert rc == 0 and torch.isfinite(v0).all() and torch.isfinite(j0).all()
    _refused(bm, lambda: forward(ws.data_ptr() + 4)[0], BAD_ARG, b"workspace must be 16-byte aligned")
    rc, v1, j1 = forward(ws.data_ptr())
    assert rc == 0 and torch.equal(v0, v1) and torch.equal(j0, j1)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_side_stream_on_the_runtime_planned_path(lib, precision):
    """A Softplus network on the runtime-planned kernels (the depth_d4_softplus fixture's), 65 poses = two 64-pose blocks: the
    launches of one handle share its scratch, so a launch on a side stream is ordered behind the default stream's by the handle's
    event -- same bits."""
    from posendf_amd import PoseNDF, synth
    from test_depth import config_for, load_case
    _, hidden, act, enc, sd = load_case("d4_softplus")
    cfg = config_for(hidden, act, enc, "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    q = torch.from_numpy(synth.make_poses(65, seed=9)).cuda()
    ref_q, ref_d = net.project(q, steps=2)
    assert net._engine_for(q.device).kernel_name() == ("pndf_generic_softplus_kernel" if precision == "fp32" else "pndf_generic_split_softplus_kernel")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_q, s_d = net.project(q, steps=2)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(s_q, ref_q) and torch.equal(s_d, ref_d)
    assert torch.isfinite(ref_q).all() and not torch.equal(ref_q, q)
