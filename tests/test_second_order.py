"""The second order of the distance on the host (include/posendf_amd_second_order.h): the host
twin `pndf_second_order_cpu` against the vectors the real reference's double backward produced
(tests/golden/make_golden_second_order.py), the relu family's H v against the closed form of the normalisation's curvature, the NULL
outputs and B = 0, other betas / activation pairs / widths against the stock modules in fp64, the exact identities and the row
isolation that need no oracle, the refusals' codes, the companion header against its signature table, and the opt-in autograd path of `PoseNDF` on a
cpu model.  Runs without a GPU; tests/test_second_order_gpu.py holds the device to the same."""
import ctypes
import os

import numpy as np
import pytest
import torch

import second_order_oracle as soo
from oracle import posendf_np as onp

BAD_ARG, UNSUPPORTED, NO_DEVICE = -1, -4, -6


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(soo.FIXTURE))


@pytest.fixture(scope="module")
def sd():
    return soo.weights()


def cpu_engine(act, sd, **kw):
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine(act, **kw)
    eng.load_weights(sd)
    return eng


def run_twin(eng, q, v, w_d=None, w_t=None, want=(True, True, True, True)):
    """pndf_second_order_cpu through CpuEngine.second_order -> [d, g, t, out], None where not wanted (those buffers keep a marker)"""
    q, v = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(v, np.float32)
    B = len(q)
    outs = [np.full(s, 7.0, np.float32) if w else None for s, w in zip(((B,), (B, 21, 4), (B,), (B, 21, 4)), want)]
    ptr = [None if a is None else a.ctypes.data for a in (w_d, w_t, *outs)]
    eng.second_order(q.ctypes.data, v.ctypes.data, *ptr, B)
    return outs


def cpu_net(act, sd, second_order=None):
    from posendf_amd import PoseNDF, amass_config
    cfg = amass_config(act, "cpu")
    if second_order is not None:
        cfg["engine"] = {"second_order": second_order}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    return net


def test_fixture_inputs_are_the_helper_s(fixture):
    inp = soo.make_inputs()
    for k, a in inp.items():
        assert np.array_equal(fixture[k], a), k
    for k, a in fixture.items():
        if a.dtype.kind == "f":
            assert np.isfinite(a).all(), k
    assert os.path.getsize(soo.FIXTURE) < 1 << 20


def test_header_matches_the_signature_table():
    """what the second order adds to the build; its header against its table is tests/test_cabi.py's, for every header alike"""
    import __graft_entry__ as ge
    from posendf_amd import engine
    assert "pndf_experiment_word_second_order" in engine.EXPERIMENT_WORDS and "pndf_second_order.hip" in ge.PRODUCT_SOURCES


@pytest.mark.parametrize("act", soo.ACTS)
def test_host_twin_meets_the_gate(fixture, sd, act):
    """1. every output within 4 x the reference's own fp32-vs-fp64 error of the reference's fp64 result"""
    eng = cpu_engine(act, sd)
    outs = run_twin(eng, fixture["q"], fixture["v"], fixture["w_d"], fixture["w_t"])
    for name, mine in zip(soo.OUTPUTS, outs):
        soo.gate(mine, fixture[f"{act}_{name}_f32"], fixture[f"{act}_{name}_f64"], f"host twin {act} {name}")


@pytest.mark.parametrize("act", ["lrelu", "relu"])
def test_relu_family_hvp_is_the_curvature(fixture, sd, act):
    """2. sigma'' = 0: out - w_d g = w_t C(q, v, g_x), the closed form in numpy float32 with g_x of the fp32 oracle, to a few ulp of the
    largest entry.  The bound, 16 ulp (2^-23 each): C is linear in g_x, and the twin's g_x and the oracle's are two independent fp32
    evaluations of the same reverse pass, whose sums run over up to 1024 terms: sqrt(1024) * 2^-24 of the largest entry = 16 ulp;
    the closed form's own dozen roundings are inside that.  Measured: 4.7 (lrelu) and 4.5 (relu) ulp."""
    eng = cpu_engine(act, sd)
    q, v, w_d, w_t = (fixture[k] for k in ("q", "v", "w_d", "w_t"))
    _, g, _, out = run_twin(eng, q, v, w_d, w_t)
    dbg = {}
    onp.forward_grad(q, sd, act, dtype=np.float32, debug=dbg)
    c = soo.curvature(q, v, dbg["gn"])
    want = w_t[:, None, None] * c
    assert want.dtype == np.float32
    got = out - w_d[:, None, None] * g
    ulp = 2.0 ** -23
    e = float(np.abs(got - want).max() / np.abs(want).max())
    # with w_d = NULL (0) and w_t = NULL (1) `out` is C itself
    plain = run_twin(eng, q, v)[3]
    e_plain = float(np.abs(plain - c).max() / np.abs(c).max())
    print(f"[second order] {act}: out - w_d g against w_t C: {e / ulp:.1f} ulp of the largest entry; out with NULL weights against C: {e_plain / ulp:.1f} ulp")
    assert e <= 16 * ulp and e_plain <= 16 * ulp, (e / ulp, e_plain / ulp)


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_null_outputs_and_empty_batch(fixture, sd, act):
    """3. every combination of NULL outputs writes the same bits into the outputs it does write; NULL weights are 0 and 1; B = 0 succeeds"""
    eng = cpu_engine(act, sd)
    q, v, w_d, w_t = (fixture[k][:9] for k in ("q", "v", "w_d", "w_t"))
    full = run_twin(eng, q, v, w_d, w_t)
    for mask in range(16):
        want = tuple(bool(mask >> i & 1) for i in range(4))
        outs = run_twin(eng, q, v, w_d, w_t, want)
        for a, b, w in zip(outs, full, want):
            assert (a is None) == (not w) and (a is None or a.tobytes() == b.tobytes()), mask
    zeros, ones = np.zeros(9, np.float32), np.ones(9, np.float32)
    assert run_twin(eng, q, v)[3].tobytes() == run_twin(eng, q, v, zeros, ones)[3].tobytes()
    lib = eng.lib
    assert lib.pndf_second_order_cpu(eng.handle, None, None, None, None, None, None, None, None, 0) == 0
    net = cpu_net(act, sd)
    d, g, t, out = net.hvp(torch.from_numpy(q), torch.from_numpy(v), torch.from_numpy(w_d), torch.from_numpy(w_t))
    assert d.shape == (9, 1) and g.shape == (9, 21, 4) and t.shape == (9, 1) and out.shape == (9, 21, 4)
    for a, b in zip((d, g, t, out), full):
        assert a.numpy().tobytes() == b.tobytes()
    d0, g0, t0, out0 = net.hvp(torch.zeros(0, 21, 4), torch.zeros(0, 21, 4))
    assert d0.shape == (0, 1) and out0.shape == (0, 21, 4)


def test_zero_norm_column_is_finite(fixture, sd):
    """a pose on the clamp of F.normalize (outside the parity contract: the reference's double backward is NaN there) gives finite
    results, and its clamped column carries no curvature"""
    q, v = fixture["q"][:4].copy(), fixture["v"][:4]
    q[1, :, 2] = 0.0
    for act in ("lrelu", "softplus"):
        outs = run_twin(cpu_engine(act, sd), q, v)
        assert all(np.isfinite(a).all() for a in outs), act


def twin_of(net, sd):
    """the host twin of a second_order_oracle.NETWORKS entry as `run(q, v, w_d, w_t)` -> [d, g, t, out]"""
    act, beta, enc_act, enc_beta, hidden = net
    eng = cpu_engine(act, sd, beta=beta, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta)
    return lambda q, v, w_d, w_t: run_twin(eng, q, v, w_d, w_t)


@pytest.mark.parametrize("net", soo.NETWORKS, ids=soo.network_id)
def test_host_twin_other_networks(net):
    """betas (a factor of the result: sigma'' = beta s (1 - s)) on either side and both, activation pairs, one-unit, odd, 1024-wide
    and 129 / 127-wide layers, at B = 129 under the gate against the stock modules in fp64, their fp32 run as the envelope"""
    sd = soo.network_weights(net)
    args = soo.batch_inputs(129, seed=33, kinks=soo.network_kinks(net, sd))
    ref32, ref64 = soo.stock_reference(net, sd, args, "cpu")
    soo.gate_all(f"host twin {soo.network_id(net)}", twin_of(net, sd)(*args), ref32, ref64)


@pytest.mark.parametrize("net", soo.LAUNCH_SEQUENCES, ids=soo.network_id)
def test_exact_identities(sd, net):
    """v -> 2v, v -> -v, v = 0, w_t = 0 and power-of-two scalings of (w_d, w_t), to the bit at B = 300"""
    soo.check_exact_identities(twin_of(net, sd), *soo.batch_inputs(300, seed=38))


@pytest.mark.parametrize("net", soo.LAUNCH_SEQUENCES, ids=soo.network_id)
def test_rows_are_independent(sd, net):
    """NaN / Inf poses, a NaN direction, an infinite weight and clamped columns stay in their rows; for lrelu the clamped column of
    `out` is w_d g: no curvature there"""
    soo.check_rows_are_independent(twin_of(net, sd), *soo.batch_inputs(300, seed=38), clamped_column_is_w_d_g=net[0] == "lrelu")


@pytest.mark.parametrize("act", ["lrelu", "relu"])
def test_distance_zero_has_no_derivatives(sd, act):
    """an output bias of -1e3 switches the output ReLU off: d, g, t and out are exactly zero at B = 129"""
    sd = dict(sd, **{"dfnet.lin6.bias": np.full_like(sd["dfnet.lin6.bias"], -1e3)})
    soo.check_distance_zero(twin_of((act, 100.0, None, None, None), sd), *soo.batch_inputs(129, seed=39))


def test_refusals_return_their_codes(fixture, sd):
    """4. the named codes and a text on the right channel"""
    from posendf_amd import engine
    lib = engine.load_library()
    eng = cpu_engine("lrelu", sd)
    q, v = np.ascontiguousarray(fixture["q"][:4]), np.ascontiguousarray(fixture["v"][:4])
    out = np.empty_like(q)
    call = lib.pndf_second_order_cpu
    assert call(None, q.ctypes.data, v.ctypes.data, None, None, None, None, None, out.ctypes.data, 4) == BAD_ARG
    assert call(eng.handle, q.ctypes.data, None, None, None, None, None, None, out.ctypes.data, 4) == BAD_ARG
    assert call(eng.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, out.ctypes.data, -1) == BAD_ARG
    for alias in (q, v):      # `out` over q or v
        assert call(eng.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, alias.ctypes.data, 4) == BAD_ARG
        assert b"alias" in lib.pndf_cpu_last_error(eng.handle)
    assert call(eng.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, q.ctypes.data + 84 * 4, 4) == BAD_ARG      # a partial overlap
    assert call(eng.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, out.ctypes.data + 2, 4) == BAD_ARG          # misaligned
    assert call(eng.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, out.ctypes.data, 4) == 0
    # without the structure encoder: PNDF_ERR_UNSUPPORTED, on the host twin and -- before any device is looked for -- on the device plan
    noenc = engine.CpuEngine("lrelu", encoder=False)
    assert call(noenc.handle, q.ctypes.data, v.ctypes.data, None, None, None, None, None, out.ctypes.data, 4) == UNSUPPORTED
    cfg = engine._network_config(lib, "lrelu", 100.0, encoder=False)
    h = ctypes.c_void_p()
    assert lib.pndf_so_create(ctypes.byref(h), ctypes.byref(cfg), 0) == UNSUPPORTED and not h
    assert b"structure encoder" in lib.pndf_so_last_error(None)
    cfg = engine._network_config(lib, "lrelu", 100.0, hidden=[64, 2048])
    assert lib.pndf_so_create(ctypes.byref(h), ctypes.byref(cfg), 0) == UNSUPPORTED
    assert lib.pndf_so_create(None, None, 0) == BAD_ARG
    assert lib.pndf_so_workspace_floats(None, 4) == BAD_ARG
    assert lib.pndf_second_order(None, None, None, None, None, None, None, None, None, None, 4, None, 0, None) == BAD_ARG
    assert lib.pndf_so_destroy(None) == 0
    if not torch.cuda.is_available():      # no gfx950 device: a loud error, no fallback
        cfg = engine._network_config(lib, "lrelu", 100.0)
        assert lib.pndf_so_create(ctypes.byref(h), ctypes.byref(cfg), 0) == NO_DEVICE
        with pytest.raises(engine.PndfError):
            engine.SecondOrderEngine("lrelu")
    from posendf_amd import PoseNDF, amass_config
    cfg = amass_config("lrelu", "cpu")
    cfg["engine"] = {"second_order": "torch"}
    with pytest.raises(ValueError):
        PoseNDF(cfg)


def unrolled_loop(net, q0, w):
    """experiments/sample_poses.py:67-74, three steps with the graph kept -> (q3, dL/dq0) for L = sum(q3 * w)"""
    from posendf_amd import gradient
    q0 = q0.clone().requires_grad_(True)
    q = q0
    for _ in range(soo.LOOP_STEPS):
        pred = net(q, train=False)
        grad = gradient(q, pred["dist_pred"]).reshape(-1, 84)
        q = q - (pred["dist_pred"] * grad).reshape(-1, 21, 4)
    (g0,) = torch.autograd.grad((q * w).sum(), q0)
    return q.detach(), g0.detach()


@pytest.mark.parametrize("act", soo.LOOP_ACTS)
def test_cpu_model_differentiates_the_unrolled_loop(fixture, sd, act):
    """5. with the option on, a cpu model backpropagates through three projection steps: dL/dq0 under the gate"""
    net = cpu_net(act, sd, "hip")
    q3, g0 = unrolled_loop(net, torch.from_numpy(fixture["q"]), torch.from_numpy(fixture["w"]))
    soo.gate(q3.numpy(), fixture[f"loop_{act}_q3_f32"], fixture[f"loop_{act}_q3_f64"], f"cpu model {act} loop q3")
    soo.gate(g0.numpy(), fixture[f"loop_{act}_grad_f32"], fixture[f"loop_{act}_grad_f64"], f"cpu model {act} loop dL/dq0")


def test_option_off_raises_and_option_on_stops_at_the_third_order(fixture, sd):
    """6. the default keeps today's RuntimeError on a double backward; with the option on the second order runs, equals hvp(q, ones),
    leaves forward and first-order gradient bit for bit, and a third order raises"""
    q = torch.from_numpy(fixture["q"][:8])
    off, on = cpu_net("softplus", sd), cpu_net("softplus", sd, "hip")
    with pytest.raises(RuntimeError):
        qq = q.clone().requires_grad_(True)
        dd = off(qq, train=False)["dist_pred"]
        (g1,) = torch.autograd.grad(dd.sum(), qq, create_graph=True)
        g1.sum().backward()
    qa, qb = q.clone().requires_grad_(True), q.clone().requires_grad_(True)
    da, db = off(qa, train=False)["dist_pred"], on(qb, train=False)["dist_pred"]
    (ga,) = torch.autograd.grad(da.sum(), qa)
    (gb,) = torch.autograd.grad(db.sum(), qb, create_graph=True)
    assert torch.equal(da, db) and torch.equal(ga, gb.detach()) and gb.requires_grad
    (h,) = torch.autograd.grad(gb.sum(), qb, create_graph=True)
    assert torch.equal(h, on.hvp(q, torch.ones_like(q))[3])
    assert not h.requires_grad
    with pytest.raises(RuntimeError):
        h.sum().backward()
    # the gradient with respect to grad_out: <v, grad d>
    qc = q.clone().requires_grad_(True)
    go = torch.full((8, 1), 0.5, requires_grad=True)
    (gc,) = torch.autograd.grad(on(qc, train=False)["dist_pred"], qc, grad_outputs=go, create_graph=True)
    v = torch.from_numpy(fixture["v"][:8])
    (tgo,) = torch.autograd.grad((gc * v).sum(), go)
    assert torch.equal(tgo, on.hvp(q, v)[2])
