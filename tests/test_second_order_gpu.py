"""The second order of the distance on an MI355X (include/posendf_amd_second_order.h, csrc/pndf_second_order.hip):
`pndf_second_order` against the reference's fp64 vectors and against the stock modules' double backward in fp64 on the same GPU,
determinism and the NULL outputs, the clamp of the normalisation, and the opt-in autograd path of `PoseNDF`; the betas, activation
pairs and widths of second_order_oracle.NETWORKS, and the oracle-free properties (exact linearity in v and in the weights, rows that
stay rows, a distance clamped to zero) that tests/test_second_order.py holds the host twin to.  Reads only fixtures and synth (the
reference is not here).

The gate, everywhere: max abs error over the batch / max abs of the fp64 output <= 4 x the same figure of the reference arithmetic's
own fp32 run (second_order_oracle.gate).  A pose's results do not depend on the batch around it (every GEMM column and every
encoder lane is one pose, summed in a fixed order), so the batch sizes that straddle the 128-column tile, the 256-lane encoder
workgroups and the chunk seam are held to the BITS of the same poses inside one larger batch, and the gate is taken over that larger
batch, where the max over the batch is not the rounding of a single number."""
import numpy as np
import pytest
import torch

import second_order_oracle as soo
from posendf_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 16384     # csrc/pndf_second_order.hip SO_CHUNK


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(soo.FIXTURE))


@pytest.fixture(scope="module")
def sd():
    return soo.weights()


def model(act, sd, hidden=None, enc_act=None, engine=None, device=DEV, beta=None, enc_beta=None):
    from posendf_amd import PoseNDF, amass_config
    cfg = soo.set_network(amass_config(act, device), hidden, enc_act, beta, enc_beta)
    if engine is not None:
        cfg["engine"] = dict(engine)
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net.eval()
    return net


def inputs(B, seed=31, kinks=None):
    """second_order_oracle.batch_inputs (B signed poses, normal directions, weights of both signs; `kinks`: its kink filter) on the GPU"""
    return tuple(torch.from_numpy(a).to(DEV) for a in soo.batch_inputs(B, seed, kinks))


def hvp_np(net, *args):
    return [a.cpu().numpy() for a in net.hvp(*args)]


def stock_gate(tag, net, act, sd, args, hidden=None, enc_act=None, beta=None, enc_beta=None):
    """`net.hvp` against the stock modules' double backward: fp64 as the truth, their fp32 run as the envelope, on this GPU"""
    mine = hvp_np(net, *args)
    m64 = soo.stock_model(act, sd, DEV, torch.float64, hidden, enc_act, beta, enc_beta)
    m32 = soo.stock_model(act, sd, DEV, torch.float32, hidden, enc_act, beta, enc_beta)
    r64 = soo.stock_second_order(m64, *(a.double() for a in args))
    r32 = soo.stock_second_order(m32, *args)
    for name, a, b, c in zip(soo.OUTPUTS, mine, r32, r64):
        soo.gate(a, b.cpu().numpy(), c.cpu().numpy(), f"{tag} {name}")
    return mine


def device_of(net, sd):
    """`pndf_second_order` for a second_order_oracle.NETWORKS entry as `run(q, v, w_d, w_t)` -> [d, g, t, out] in numpy, through
    PoseNDF._second_order on the GPU; and the model"""
    act, beta, enc_act, enc_beta, hidden = net
    m = model(act, sd, hidden, enc_act, beta=beta, enc_beta=enc_beta)

    def run(q, v, w_d, w_t):
        args = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (q, v, w_d, w_t)]
        return [a.cpu().numpy() for a in m._second_order(*args)]
    return run, m


@pytest.mark.parametrize("act", soo.ACTS)
def test_fixture_gate(fixture, sd, act):
    """1. pndf_second_order against the reference's fp64 double backward, the reference's fp32 run as the envelope"""
    net = model(act, sd)
    args = [torch.from_numpy(fixture[k]).to(DEV) for k in ("q", "v", "w_d", "w_t")]
    for name, mine in zip(soo.OUTPUTS, hvp_np(net, *args)):
        soo.gate(mine, fixture[f"{act}_{name}_f32"], fixture[f"{act}_{name}_f64"], f"gpu {act} {name}")


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_stock_fp64_and_batch_seams(sd, act):
    """2. configs/amass.yaml's network at B = 300 against the stock modules in fp64; B = 1, 127, 129 (the 128-column GEMM tile) give
    the bits of the same poses inside the 300"""
    net = model(act, sd)
    args = inputs(300, kinks=(sd, act))
    full = stock_gate(f"stock {act} B=300", net, act, sd, args)
    for B in (1, 127, 129):
        part = hvp_np(net, *(a[:B] for a in args))
        for name, a, b in zip(soo.OUTPUTS, part, full):
            assert a.tobytes() == b[:B].tobytes(), (B, name)


def test_chunk_seam(sd):
    """2. one pose past the chunk: the gate over all 16,385 poses, the first chunk's head and the pose behind the seam bit for bit"""
    net = model("softplus", sd)
    args = inputs(CHUNK + 1, seed=32)
    full = stock_gate(f"stock softplus B={CHUNK + 1}", net, "softplus", sd, args)
    head = hvp_np(net, *(a[:300] for a in args))
    last = hvp_np(net, *(a[CHUNK:] for a in args))
    for name, a, b, c in zip(soo.OUTPUTS, full, head, last):
        assert a[:300].tobytes() == b.tobytes() and a[CHUNK:].tobytes() == c.tobytes(), name


@pytest.mark.parametrize("act,enc_act,hidden", [("softplus", None, [96, 40]), ("lrelu", None, [96, 40]),
                                                ("softplus", None, [128, 96, 64, 72, 64, 48, 40]),
                                                ("softplus", "lrelu", None), ("relu", "softplus", [96, 40])])
def test_other_networks(act, enc_act, hidden):
    """2. widths that are no multiple of 16, seven hidden layers, mixed encoder / trunk activations (a relu trunk behind a softplus
    encoder has a Hessian that lives in the encoder alone), at B = 129"""
    dims = synth.DFNET_DIMS if hidden is None else (126, *hidden, 1)
    sd = synth.make_weights(seed=3, gain=2.0, out_bias=0.1, dims=dims)
    net = model(act, sd, hidden, enc_act)
    stock_gate(f"stock {act}/{enc_act or act} {hidden or 'amass'}", net, act, sd, inputs(129, seed=33, kinks=(sd, f"{act}/{enc_act or act}")), hidden, enc_act)


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_same_bits_and_null_outputs(sd, act):
    """3. two calls give the same bits; every combination of NULL outputs gives the same bits in the outputs it writes"""
    net = model(act, sd)
    q, v, w_d, w_t = inputs(300, seed=34)
    full = [a.clone() for a in net._second_order(q, v, w_d, w_t)]
    again = net._second_order(q, v, w_d, w_t)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for mask in range(16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        outs = net._second_order(q, v, w_d, w_t, want=want)
        for a, b, w in zip(outs, full, want):
            assert (a is None) == (not w) and (a is None or torch.equal(a, b)), mask
    assert torch.equal(net._second_order(q, v, None, None)[3], net._second_order(q, v, torch.zeros_like(w_d), torch.ones_like(w_t))[3])


def test_clamp_is_finite_and_null_out_is_not_written(sd):
    """4. a zero-norm component column gives finite results; a call with `out` = NULL (and d, t NULL) runs and gives g's bits; `out` over
    q or v and a short workspace are refused"""
    from posendf_amd.engine import PndfError
    net = model("softplus", sd)
    q, v, w_d, w_t = inputs(64, seed=35)
    q[3, :, 2] = 0.0
    outs = net._second_order(q, v, w_d, w_t)
    assert all(torch.isfinite(a).all() for a in outs)
    eng = net._so_engines[0]
    named = dict(net.named_parameters())
    from posendf_amd.engine import state_dict_order
    ptrs = [named[k].data_ptr() for k in state_dict_order(True, 7)]
    n = eng.workspace_floats(64)
    ws = torch.empty(n, device=DEV)
    g = torch.empty(64, 21, 4, device=DEV)
    eng.second_order(ptrs, q.data_ptr(), v.data_ptr(), None, None, None, g.data_ptr(), None, None, 64, ws.data_ptr(), n)
    torch.cuda.synchronize()
    assert torch.equal(g, outs[1])      # (a store through the NULL `out` would have faulted: the call coming back with g's bits is the evidence)
    for alias in (q, v):
        with pytest.raises(PndfError, match="alias"):
            eng.second_order(ptrs, q.data_ptr(), v.data_ptr(), None, None, None, None, None, alias.data_ptr(), 64, ws.data_ptr(), n)
    with pytest.raises(PndfError, match="workspace"):
        eng.second_order(ptrs, q.data_ptr(), v.data_ptr(), None, None, None, None, None, g.data_ptr(), 64, ws.data_ptr(), n - 1)
    assert eng.workspace_floats(0) == 0 and eng.workspace_floats(65536) == eng.workspace_floats(CHUNK) < 1 << 28
    eng.second_order(ptrs, None, None, None, None, None, None, None, None, 0, None, 0)      # B = 0: no launch


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_option_on_keeps_first_order_bits_and_runs_the_double_backward(sd, act):
    """5. + 6. with the option on, forward and first-order gradient equal the option-off results bit for bit at the default
    precision, and the double backward that raises without the option runs and equals hvp(q, ones)"""
    off, on = model(act, sd), model(act, sd, engine={"second_order": "hip"})
    q = inputs(129, seed=36)[0]
    qa, qb = q.clone().requires_grad_(True), q.clone().requires_grad_(True)
    da, db = off(qa, train=False)["dist_pred"], on(qb, train=False)["dist_pred"]
    (ga,) = torch.autograd.grad(da.sum(), qa)
    assert torch.equal(da, db) and torch.equal(off(q, train=False)["dist_pred"], on(q, train=False)["dist_pred"])
    qq = q.clone().requires_grad_(True)
    dd = on(qq, train=False)["dist_pred"]
    (g1,) = torch.autograd.grad(dd.sum(), qq, create_graph=True)
    assert torch.equal(g1.detach(), ga)
    g1.sum().backward()
    assert torch.equal(qq.grad, on.hvp(q, torch.ones_like(q))[3])
    with pytest.raises(RuntimeError):      # the default stays as it is
        qq = q.clone().requires_grad_(True)
        (g1,) = torch.autograd.grad(off(qq, train=False)["dist_pred"].sum(), qq, create_graph=True)
        g1.sum().backward()
    with pytest.raises(RuntimeError):      # a third order raises
        qq = q.clone().requires_grad_(True)
        (g1,) = torch.autograd.grad(on(qq, train=False)["dist_pred"].sum(), qq, create_graph=True)
        (g2,) = torch.autograd.grad(g1.sum(), qq, create_graph=True)
        g2.sum().backward()


def unrolled_loop(net, q0, w):
    from posendf_amd import gradient
    q0 = q0.clone().requires_grad_(True)
    q = q0
    for _ in range(soo.LOOP_STEPS):
        pred = net(q, train=False)
        grad = gradient(q, pred["dist_pred"]).reshape(-1, 84)
        q = q - (pred["dist_pred"] * grad).reshape(-1, 21, 4)
    (g0,) = torch.autograd.grad((q * w).sum(), q0)
    return q.detach().cpu().numpy(), g0.detach().cpu().numpy()


@pytest.mark.parametrize("act", soo.LOOP_ACTS)
def test_unrolled_loop_gradient(fixture, sd, act):
    """7. three projection steps with the graph kept, dL/dq0 under the gate with engine.precision fp32; at the default f16x3 the
    figure is printed (DESIGN.md records it), not gated"""
    q0, w = torch.from_numpy(fixture["q"]).to(DEV), torch.from_numpy(fixture["w"]).to(DEV)
    q3, g0 = unrolled_loop(model(act, sd, engine={"second_order": "hip"}), q0, w)
    e = soo.err(g0, fixture[f"loop_{act}_grad_f64"])
    print(f"[second order] gpu {act} loop dL/dq0 at the default f16x3: err {e:.2e} (reference fp32 {soo.err(fixture[f'loop_{act}_grad_f32'], fixture[f'loop_{act}_grad_f64']):.2e}), not gated")
    q3, g0 = unrolled_loop(model(act, sd, engine={"second_order": "hip", "precision": "fp32"}), q0, w)
    soo.gate(q3, fixture[f"loop_{act}_q3_f32"], fixture[f"loop_{act}_q3_f64"], f"gpu {act} fp32 loop q3")
    soo.gate(g0, fixture[f"loop_{act}_grad_f32"], fixture[f"loop_{act}_grad_f64"], f"gpu {act} fp32 loop dL/dq0")


def test_hvp_takes_any_layout_and_dtype(sd):
    """8. a non-contiguous or float64 pose gives what the float32 contiguous copy gives"""
    net = model("softplus", sd)
    q, v, w_d, w_t = inputs(129, seed=37)
    want = net.hvp(q, v, w_d, w_t)
    strided = torch.empty(129, 21, 8, device=DEV)[..., ::2]
    strided.copy_(q)
    assert not strided.is_contiguous()
    for pose, vv in ((strided, v), (q.double(), v.double()), (q.cpu(), v.cpu())):
        got = net.hvp(pose, vv, w_d, w_t)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("net", soo.NETWORKS, ids=soo.network_id)
def test_networks_table(net):
    """9. second_order_oracle.NETWORKS -- betas on either side and both (a factor of the result), activation pairs, a one-unit
    hidden layer (M = 1 forward, K = 1 reverse), odd widths, 1024 x 1024 (eight row tiles, 64 K steps), 129 / 127 -- at B = 129
    under the gate against the stock modules in fp64 on this GPU"""
    act, beta, enc_act, enc_beta, hidden = net
    sd = soo.network_weights(net)
    args = inputs(129, seed=33, kinks=soo.network_kinks(net, sd))
    m = model(act, sd, hidden, enc_act, beta=beta, enc_beta=enc_beta)
    stock_gate(f"stock {soo.network_id(net)}", m, act, sd, args, hidden, enc_act, beta, enc_beta)


@pytest.mark.parametrize("net", soo.LAUNCH_SEQUENCES, ids=soo.network_id)
def test_exact_identities(sd, net):
    """10. v -> 2v, v -> -v, v = 0, w_t = 0 and power-of-two scalings of (w_d, w_t), to the bit at B = 300: the kernels compute the
    formula of their header comment, with nothing of the tangent in the primal chain"""
    soo.check_exact_identities(device_of(net, sd)[0], *soo.batch_inputs(300, seed=38))


@pytest.mark.parametrize("net", soo.LAUNCH_SEQUENCES, ids=soo.network_id)
def test_rows_are_independent(sd, net):
    """11. NaN / Inf poses, a NaN direction, an infinite weight and clamped columns (ordinary float inputs to arithmetic kernels;
    nothing indexes with them) stay in their rows: the GEMM loads zero-fill outside the matrix, not inside it, so a NaN column stays a
    column.  Rows 7, 130 and 257 sit in three 128-column tiles, 127 | 128 | 129 straddle a tile edge"""
    soo.check_rows_are_independent(device_of(net, sd)[0], *soo.batch_inputs(300, seed=38), clamped_column_is_w_d_g=net[0] == "lrelu")


@pytest.mark.parametrize("act", ["lrelu", "relu"])
def test_distance_zero_has_no_derivatives(sd, act):
    """12. an output bias of -1e3 switches the output ReLU off: d, g, t and out are exactly zero at B = 129"""
    sd = dict(sd, **{"dfnet.lin6.bias": np.full_like(sd["dfnet.lin6.bias"], -1e3)})
    soo.check_distance_zero(device_of((act, 100.0, None, None, None), sd)[0], *soo.batch_inputs(129, seed=39))


@pytest.mark.parametrize("net", soo.LAUNCH_SEQUENCES[1:], ids=soo.network_id)
def test_chunk_seam_other_launch_sequences(sd, net):
    """13. the relu-family launch sequence, and `zero_a0` (the encoder kernel clears the primal adjoint of the features itself, no
    trunk pass writes it), across a chunk seam at B = CHUNK + 129: the first 300 poses and the last 129 equal, bit for bit, separate
    calls on those slices made afterwards on the same model -- whose per-stream workspace a smaller call then reuses.  No oracle."""
    run, _ = device_of(net, sd)
    args = soo.batch_inputs(CHUNK + 129, seed=32)
    full = run(*args)
    head = run(*(a[:300] for a in args))
    last = run(*(a[CHUNK:] for a in args))
    assert all(np.isfinite(a).all() for a in full)
    for name, a, b, c in zip(soo.OUTPUTS, full, head, last):
        assert a[:300].tobytes() == b.tobytes(), f"{name}: the chunk's head"
        assert a[CHUNK:].tobytes() == c.tobytes(), f"{name}: behind the seam"


@pytest.mark.parametrize("net", soo.TWIN_AND_DEVICE, ids=soo.network_id)
def test_device_equals_host_twin_under_the_gate(net):
    """14. the device and the host twin held to the same stock fp64 truth (this GPU's) with the same gate, side by side"""
    from posendf_amd.engine import CpuEngine
    act, beta, enc_act, enc_beta, hidden = net
    sd = soo.network_weights(net)
    args = soo.batch_inputs(129, seed=33, kinks=soo.network_kinks(net, sd))
    ref32, ref64 = soo.stock_reference(net, sd, args, DEV)
    dev = soo.gate_all(f"device {soo.network_id(net)}", device_of(net, sd)[0](*args), ref32, ref64)
    eng = CpuEngine(act, beta, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta)
    eng.load_weights(sd)
    twin = [np.empty(s, np.float32) for s in ((129,), (129, 21, 4), (129,), (129, 21, 4))]
    eng.second_order(*(a.ctypes.data for a in (*args, *twin)), 129)
    host = soo.gate_all(f"host twin {soo.network_id(net)}", twin, ref32, ref64)
    for name in soo.OUTPUTS:
        print(f"[second order] {soo.network_id(net)} {name}: device {dev[name]:.2f}  host twin {host[name]:.2f}  (err / stock fp32 err)")
