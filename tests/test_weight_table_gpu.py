"""What the device loaders answer to a weight table that does not fit, on live handles of an MI355X (csrc/pndf_net_plan.h:
pndf_table_fault): pndf_load_weights on the fused and on the runtime-planned kernels and pndf_skel_load_weights
against the faulty tables of tests/weight_table_faults.py.  Every refusal comes from the validation ahead of any copy or launch: it
leaves its text on the handle and the previous weights serving, so forward_grad at B = 65 (one full 64-pose block and a ragged one)
gives the bytes it gave before.  The status codes are literals; nothing here launches on bad data.  The loaders without a device:
tests/test_weight_table.py."""
import numpy as np
import pytest

import weight_table_faults as wtf
from posendf_amd import synth

pytestmark = pytest.mark.gpu
BAD_ARG, BAD_SHAPE = -1, -2
B = 65


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    return torch


def forward_grad(torch, eng, q, skeleton):
    d, dq = torch.full((B,), 7.0, device="cuda:0"), torch.full(q.shape, 7.0, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    if skeleton:
        n = eng.workspace_bytes(B)
        ws = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda:0")
        eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, ws.data_ptr(), n, stream)
    else:
        eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, stream)
    torch.cuda.synchronize()
    return d.cpu().numpy(), dq.cpu().numpy()


def refusals_change_nothing(torch, eng, load, last_error, sd, q, codes, parents=None, skeleton=False):
    q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    eng.load_weights(sd)
    d0, dq0 = forward_grad(torch, eng, q, skeleton)
    assert np.isfinite(d0).all() and np.isfinite(dq0).all() and (d0 > 0).any() and np.abs(dq0).max() > 0
    seen = []
    for fault, keep, tensors, numel, n in wtf.faulty_tables(sd, parents):
        if fault not in codes:
            continue
        seen.append(fault)
        assert load(eng.handle, tensors, numel, n) == codes[fault], fault
        assert last_error(eng.handle), fault
    assert seen == [f for f in wtf.FAULTS if f in codes]
    d1, dq1 = forward_grad(torch, eng, q, skeleton)
    assert d1.tobytes() == d0.tobytes() and dq1.tobytes() == dq0.tobytes()
    eng.close()


ENGINE_CODES = {fault: BAD_SHAPE for fault in wtf.FAULTS}


def test_fused_engine(torch_cuda):
    from posendf_amd import engine
    eng = engine.Engine("lrelu", device=0, precision="fp32")
    refusals_change_nothing(torch_cuda, eng, eng.lib.pndf_load_weights, eng.lib.pndf_last_error, synth.make_weights(0, 2.0, 0.1),
                            synth.make_poses(B, seed=5).reshape(B, 84), ENGINE_CODES)


def test_runtime_planned_engine(torch_cuda):
    from posendf_amd import engine
    eng = engine.Engine("lrelu", device=0, precision="fp32", hidden=[16, 16])
    sd = synth.make_weights(50, 2.5, 0.3, dims=(126, 16, 16, 1))      # (a seed whose small network is not clipped to d = 0 on these poses)
    eng.load_weights(sd)
    assert eng.kernel_name() == "pndf_generic_relu_kernel"
    refusals_change_nothing(torch_cuda, eng, eng.lib.pndf_load_weights, eng.lib.pndf_last_error, sd, synth.make_poses(B, seed=5).reshape(B, 84),
                            ENGINE_CODES)


def test_skeleton_engine(torch_cuda):
    """a null pointer is an argument's fault in this family; a 3-joint tree has no table of SMPL's 14 tensors to be mistaken for"""
    from posendf_amd import engine
    parents = (-1, 0, 0)
    eng = engine.SkeletonEngine(parents, "lrelu", hidden=[8])
    sd = synth.make_weights(0, 2.0, 0.1, dims=synth.skeleton_dims(parents, [8]), parents=parents)
    codes = {fault: BAD_ARG if fault in wtf.NULL_TABLE + wtf.NULL_TENSOR else BAD_SHAPE for fault in wtf.FAULTS if fault != "dfnet-only table"}
    q = np.random.default_rng(5).normal(size=(B, 4 * len(parents))).astype(np.float32)
    refusals_change_nothing(torch_cuda, eng, eng.lib.pndf_skel_load_weights, eng.lib.pndf_skel_last_error, sd, q, codes, parents, skeleton=True)
