"""Other skeletons on an MI355X (include/posendf_amd_skeleton.h, csrc/pndf_skeleton.hip): the HIP unit under the
gates of tests/test_skeleton.py on a hand, a 32-joint tree, one joint, five roots and one chain of 32, with and without the encoder,
at batch sizes on both sides of the 64-lane and the 128-column seams; on the SMPL table under the gates of tests/test_gpu_parity.py;
the fused step against forward_grad + the numpy statement of the step, to the bit; chunk seams, determinism, streams; the argument
checks; `SkeletonPoseNDF` on cuda."""
import ctypes

import numpy as np
import pytest

import skeleton_oracle as sko
from conftest import (d_rows, fp32_noise, golden_weights, load_golden, outlier_gate, pose_gate, rel_err_rows, traj_margin)
from oracle import posendf_np as onp
from posendf_amd import synth

pytestmark = pytest.mark.gpu
BAD_ARG, NO_WEIGHTS = -1, -5
CHUNK = 16384      # SK_CHUNK of csrc/pndf_skeleton.hip


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    return torch


class Unit:
    """pndf_skel_* on cuda:0 with numpy in and out"""

    def __init__(self, torch, parents, act, sd, encoder=True, hidden=sko.HIDDEN):
        from posendf_amd.engine import SkeletonEngine
        self.torch, self.J = torch, len(parents)
        self.eng = SkeletonEngine(parents, act, encoder=encoder, hidden=hidden)
        if sd is not None:
            self.eng.load_weights(sd)

    def ws(self, B):
        n = self.eng.workspace_bytes(B)
        return self.torch.empty(max(n, 16), dtype=self.torch.uint8, device="cuda:0"), n

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    def forward(self, q):
        q, (ws, n) = self.dev(q), self.ws(len(q))
        d = self.torch.full((len(q),), 7.0, device="cuda:0")
        self.eng.forward(q.data_ptr(), d.data_ptr(), len(q), ws.data_ptr(), n, self.torch.cuda.current_stream().cuda_stream)
        return d.cpu().numpy()

    def forward_grad(self, q, grad_out=None, want_d=True):
        q, (ws, n) = self.dev(q), self.ws(len(q))
        d, dq = self.torch.full((len(q),), 7.0, device="cuda:0"), self.torch.full(q.shape, 7.0, device="cuda:0")
        go = None if grad_out is None else self.dev(grad_out)
        self.eng.forward_grad(q.data_ptr(), None if go is None else go.data_ptr(), d.data_ptr() if want_d else None, dq.data_ptr(), len(q),
                              ws.data_ptr(), n, self.torch.cuda.current_stream().cuda_stream)
        return d.cpu().numpy(), dq.cpu().numpy()

    def project(self, q, steps, want_d=True, in_place=False, **opts):
        q, (ws, n) = self.dev(q), self.ws(len(q))
        out = q if in_place else self.torch.full(q.shape, 7.0, device="cuda:0")
        d = self.torch.full((len(q),), 7.0, device="cuda:0")
        self.eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr() if want_d else None, len(q), steps, ws.data_ptr(), n,
                         self.torch.cuda.current_stream().cuda_stream, step_size=opts.get("step_size", 1.0), renorm=opts.get("renormalize"),
                         tol=opts.get("tol", 0.0))
        return out.cpu().numpy(), d.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", sko.CASES, ids=sko.case_id)
def test_unit_meets_the_gates(torch_cuda, case, act):
    """B = 1, 65, 129, 257: a lone column and both sides of the 64-lane and the 128-column seams; 6 J = 6, 30, 90, 192 (4 J = 60, 128
    without the encoder): the GEMM's K tail and its second row tile"""
    parents, sd = sko.case_network(case, act)
    unit = Unit(torch_cuda, parents, act, sd, encoder=case[1])
    for B in (1, 65, 129, 257):
        q = sko.case_poses(case, B)
        d, dq = unit.forward_grad(q)
        sko.gate(d, dq, q, sd, act, parents, f"unit {sko.case_id(case)} {act} B={B}")
        assert unit.forward(q).tobytes() == d.tobytes()
    i = np.arange(len(q))
    go = ((-1.0) ** i * 2.0 ** (i % 5 - 2)).astype(np.float32)
    d2, dq2 = unit.forward_grad(q, go)
    normal = np.abs(dq) > 2.0 ** -100
    assert d2.tobytes() == d.tobytes() and np.array_equal(dq2[normal], (dq * go[:, None, None])[normal])


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_smpl_table_under_the_parity_gates(torch_cuda, act):
    """amass.yaml's dims, conftest's golden weights: the gates tests/test_gpu_parity.py applies to the exact-fp32 kernel"""
    g, sd = load_golden(act, "live"), golden_weights("live")
    unit = Unit(torch_cuda, synth.PARENT, act, sd, hidden=synth.DFNET_DIMS[1:-1])
    d, dq = unit.forward_grad(g["q"])
    sig_d, sig_g, _, _ = fp32_noise(g["q"], sd, act, extra_d=[d_rows(g["d_f32"], g["d_f64"])], extra_g=[rel_err_rows(g["dq_f32"], g["dq_f64"])])
    e_d, e_g = d_rows(d, g["d_f64"]), rel_err_rows(dq, g["dq_f64"])
    ex = None if act == "softplus" else onp.kink_margin(g["q"], sd, act) < 1e-5
    pose_gate(e_d, sig_d, "d")
    pose_gate(e_g, sig_g, "dq", exempt=ex)
    outlier_gate(e_g, rel_err_rows(g["dq_f32"], g["dq_f64"]), 1e-4, "dq", margin=traj_margin(g["q"], sd, act), sigma=sig_g)


# ------------------------------------------------------------------------------------------ 2. the fused step is the stated step
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", False)], ids=sko.case_id)
def test_fused_step_is_the_stated_step(torch_cuda, case, act):
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    unit = Unit(torch_cuda, parents, act, sd, encoder=case[1])
    q = sko.case_poses(case, 129)
    d0, _ = unit.forward_grad(q)
    tol = float(np.median(d0))
    for opts in (dict(), dict(renormalize="unit", step_size=0.5), dict(renormalize="unit_flip", step_size=0.5), dict(renormalize="unit", tol=tol)):
        for K in (1, 3):
            want = q.copy()
            for _ in range(K):
                dk, gk = unit.forward_grad(want)
                want = sko.step(want, dk, gk, J, **opts)
            got, dl = unit.project(q, K, **opts)
            assert got.tobytes() == want.tobytes() and dl.tobytes() == dk.tobytes(), (opts, K)
            assert unit.project(q, K, in_place=True, **opts)[0].tobytes() == want.tobytes(), (opts, K, "in place")
            if "tol" in opts:
                rest = d0 < np.float32(tol)
                assert rest.any() and not rest.all()
                assert got[rest].tobytes() == q[rest].tobytes() and not np.array_equal(got[~rest], q[~rest])
    got, dl = unit.project(q, 0)
    assert got.tobytes() == q.tobytes() and not dl.any()


# ------------------------------------------------------------------------------------------ 3. independence and determinism
def test_chunk_seams_determinism_and_streams(torch_cuda):
    torch = torch_cuda
    parents = sko.HAND
    sd = sko.network(parents, 3, hidden=(32,))
    unit = Unit(torch, parents, "softplus", sd, hidden=(32,))
    B = CHUNK + 37
    q = synth.make_poses(B, seed=5, num_joints=len(parents))
    d, dq = unit.forward_grad(q)
    assert np.isfinite(d).all() and np.isfinite(dq).all() and d.std() > 0
    d2, dq2 = unit.forward_grad(q)
    assert d2.tobytes() == d.tobytes() and dq2.tobytes() == dq.tobytes()
    for part in (slice(0, CHUNK), slice(CHUNK, B)):
        dp, dqp = unit.forward_grad(q[part])
        assert dp.tobytes() == d[part].tobytes() and dqp.tobytes() == dq[part].tobytes()
    p, dl = unit.project(q, 2)
    pp, dlp = unit.project(q[CHUNK - 5:CHUNK + 5], 2)
    assert pp.tobytes() == p[CHUNK - 5:CHUNK + 5].tobytes() and dlp.tobytes() == dl[CHUNK - 5:CHUNK + 5].tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ds, dqs = unit.forward_grad(q)
    side.synchronize()
    assert ds.tobytes() == d.tobytes() and dqs.tobytes() == dq.tobytes()


# ------------------------------------------------------------------------------------------ 4. arguments
def test_arguments(torch_cuda):
    torch = torch_cuda
    parents, sd = sko.case_network(("hand", True), "lrelu")
    unit = Unit(torch, parents, "lrelu", None)
    lib, h = unit.eng.lib, unit.eng.handle
    B = 9
    q = unit.dev(sko.poses(parents, B))
    d, dq, out = torch.full((B,), 7.0, device="cuda:0"), torch.full(q.shape, 7.0, device="cuda:0"), torch.full(q.shape, 7.0, device="cuda:0")
    ws, n = unit.ws(B)
    assert n > 0 and n == unit.eng.workspace_bytes(B) and unit.eng.workspace_bytes(0) == 0 and lib.pndf_skel_workspace_bytes(h, -1) == BAD_ARG
    # before load_weights
    assert lib.pndf_skel_forward(h, q.data_ptr(), d.data_ptr(), B, ws.data_ptr(), n, None) == NO_WEIGHTS
    assert lib.pndf_skel_forward_grad(h, q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, ws.data_ptr(), n, None) == NO_WEIGHTS
    assert lib.pndf_skel_project(h, q.data_ptr(), out.data_ptr(), d.data_ptr(), B, 1, None, ws.data_ptr(), n, None) == NO_WEIGHTS
    assert b"pndf_skel_load_weights" in lib.pndf_skel_last_error(h)
    wrong = dict(sd)
    wrong["dfnet.lin0.weight"] = sd["dfnet.lin0.weight"][:, :-1]
    with pytest.raises(Exception):
        unit.eng.load_weights(wrong)
    unit.eng.load_weights(sd)
    # a workspace one byte short: nothing is launched, the outputs keep their marker
    assert lib.pndf_skel_forward(h, q.data_ptr(), d.data_ptr(), B, ws.data_ptr(), n - 1, None) == BAD_ARG
    assert lib.pndf_skel_forward_grad(h, q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, ws.data_ptr(), n - 1, None) == BAD_ARG
    assert lib.pndf_skel_project(h, q.data_ptr(), out.data_ptr(), d.data_ptr(), B, 1, None, ws.data_ptr(), n - 1, None) == BAD_ARG
    assert b"workspace" in lib.pndf_skel_last_error(h)
    torch.cuda.synchronize()
    assert bool((d == 7).all()) and bool((dq == 7).all()) and bool((out == 7).all())
    # null and misaligned pointers, negative sizes, overlaps, bad options
    assert lib.pndf_skel_forward(h, None, d.data_ptr(), B, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_forward(h, q.data_ptr(), None, B, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_forward(h, q.data_ptr(), d.data_ptr(), -1, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_forward(h, q.data_ptr(), d.data_ptr(), B, None, n, None) == BAD_ARG
    assert lib.pndf_skel_forward(h, q.data_ptr(), d.data_ptr(), B, ws.data_ptr() + 4, n, None) == BAD_ARG
    assert lib.pndf_skel_forward_grad(h, q.data_ptr(), None, d.data_ptr(), None, B, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_forward_grad(h, q.data_ptr(), None, d.data_ptr(), q.data_ptr(), B, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_forward_grad(h, q.data_ptr(), None, d.data_ptr(), dq.data_ptr() + 2, B, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_project(h, q.data_ptr(), None, d.data_ptr(), B, 1, None, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_project(h, q.data_ptr(), out.data_ptr(), d.data_ptr(), B, -1, None, ws.data_ptr(), n, None) == BAD_ARG
    assert lib.pndf_skel_project(h, q.data_ptr(), q.data_ptr() + 16, d.data_ptr(), B - 1, 1, None, ws.data_ptr(), n, None) == BAD_ARG
    from posendf_amd.engine import ProjectOptions
    bad = ProjectOptions()      # zero-initialised: struct_size 0
    assert lib.pndf_skel_project(h, q.data_ptr(), out.data_ptr(), d.data_ptr(), B, 1, ctypes.byref(bad), ws.data_ptr(), n, None) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((d == 7).all()) and bool((dq == 7).all()) and bool((out == 7).all())
    # B == 0 succeeds without a launch; the optional outputs may be null and the others hold the same bits
    assert lib.pndf_skel_forward_grad(h, None, None, None, None, 0, None, 0, None) == 0
    qn = q.cpu().numpy()
    full_d, full_dq = unit.forward_grad(qn)
    d_no, dq_no = unit.forward_grad(qn, want_d=False)
    assert dq_no.tobytes() == full_dq.tobytes() and (d_no == 7).all()
    p, dl = unit.project(qn, 2)
    p_no, dl_no = unit.project(qn, 2, want_d=False)
    assert p_no.tobytes() == p.tobytes() and (dl_no == 7).all() and not (dl == 7).any()


# ------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("act", sko.CASE_ACTS)
def test_model_on_cuda(torch_cuda, act):
    torch = torch_cuda
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    parents, sd = sko.case_network(("hand", True), act)
    net = SkeletonPoseNDF(skeleton_config("hand", act, "cuda:0", hidden=sko.HIDDEN))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    unit = Unit(torch, parents, act, sd)
    qn = sko.poses(parents, 70)
    want_d, want_dq = unit.forward_grad(qn)
    q = torch.from_numpy(qn).cuda().requires_grad_(True)
    d = net(q, train=False)["dist_pred"]
    assert d.shape == (70, 1) and d.detach().cpu().numpy().tobytes() == want_d.tobytes()
    (dq,) = torch.autograd.grad(d.sum(), q, create_graph=True)
    assert dq.cpu().numpy().tobytes() == want_dq.tobytes()
    with pytest.raises(RuntimeError):      # first order only
        q2 = torch.from_numpy(qn).cuda().requires_grad_(True)
        (g1,) = torch.autograd.grad(net(q2, train=False)["dist_pred"].sum(), q2, create_graph=True)
        g1.sum().backward()
    with torch.no_grad():
        assert net(torch.from_numpy(qn), train=False)["dist_pred"].cpu().numpy().tobytes() == want_d.tobytes()
    p, dl = net.project(torch.from_numpy(qn), steps=3, step_size=0.5, renormalize="unit")
    want_p, want_dl = unit.project(qn, 3, step_size=0.5, renormalize="unit")
    assert p.cpu().numpy().tobytes() == want_p.tobytes() and dl.cpu().numpy().reshape(-1).tobytes() == want_dl.tobytes()
    # a replaced parameter and an in-place update both reach the device
    sd2 = sko.network(parents, 11)
    net.dfnet.lin0.weight = torch.nn.Parameter(torch.from_numpy(sd2["dfnet.lin0.weight"]).cuda())
    with torch.no_grad():
        net.enc.net[3].net[0].bias.copy_(torch.from_numpy(sd2["enc.net.3.net.0.bias"]))
    mixed = dict(sd, **{k: sd2[k] for k in ("dfnet.lin0.weight", "enc.net.3.net.0.bias")})
    with torch.no_grad():
        got = net(torch.from_numpy(qn), train=False)["dist_pred"].cpu().numpy().reshape(-1)
    want = Unit(torch, parents, act, mixed).forward(qn)
    assert got.tobytes() == want.tobytes() and got.tobytes() != want_d.tobytes()
