"""Test helper (not a test module) for the second order of the distance (include/posendf_amd_second_order.h): the
inputs of the reference-run fixture tests/golden/second_order.npz, the gate its tests share, the closed form of the normalisation's
curvature in numpy, the stock PyTorch modules' double backward as a same-machine fp64 reference, the table of networks (betas,
activation pairs, widths) and the seeded batches the host twin's and the device's tests share, and the oracle-free checks both run."""
import os

import numpy as np

import completion_oracle as co

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "second_order.npz")
ACTS = ("lrelu", "relu", "softplus")
LOOP_ACTS = ("softplus", "lrelu")
LOOP_STEPS = 3
NPOSE = 48
OUTPUTS = ("d", "g", "t", "out")
GATE = 4.0      # times the reference's own fp32-vs-fp64 error (the motion-denoise gate of DESIGN.md section 2)


def weights():
    return co.weights()


def make_inputs():
    """the first 48 poses of completion_oracle.make_inputs() (none with a zero-norm component column: the reference's double backward
    is NaN there), two seeded normal directions, per-pose weights of both signs away from 0 and 1, and the loop's fixed w"""
    q = np.ascontiguousarray(co.make_inputs()[:NPOSE])
    assert (np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)) > 1e-3).all()
    rs = np.random.RandomState(7)
    v = rs.normal(size=q.shape).astype(np.float32)
    u = rs.normal(size=q.shape).astype(np.float32)
    w_d = (rs.uniform(0.5, 1.5, NPOSE) * np.where(rs.rand(NPOSE) < 0.5, -1, 1)).astype(np.float32)
    w_t = (rs.uniform(0.5, 1.5, NPOSE) * np.where(rs.rand(NPOSE) < 0.5, -1, 1)).astype(np.float32)
    w = rs.normal(size=q.shape).astype(np.float32)
    return dict(q=q, v=v, u=u, w_d=w_d, w_t=w_t, w=w)


def err(x, truth):
    """max abs error over the fixture divided by the max abs of the fp64 output"""
    truth = np.asarray(truth, np.float64)
    return float(np.abs(np.asarray(x, np.float64).reshape(truth.shape) - truth).max() / np.abs(truth).max())


def gate(mine, ref32, truth, what):
    """err(mine) <= 4 x err(the reference's own fp32 result), both against the reference's fp64 result; prints both before it asserts"""
    e_mine, e_ref = err(mine, truth), err(ref32, truth)
    print(f"[second order] {what}: err {e_mine:.2e}  reference fp32 {e_ref:.2e}  ratio {e_mine / max(e_ref, 1e-300):.2f}")
    assert np.isfinite(np.asarray(mine)).all(), what
    assert e_mine <= GATE * e_ref, (what, e_mine, e_ref)
    return e_mine, e_ref


def curvature(q, v, gx):
    """C(q, v, g_x) [B,21,4] in the dtype of q: per component column c with u = q[:, :, c], s = |u|, n = u / s, p = (v_c - n (n . v_c)) / s,
    J g = (g_c - n (n . g_c)) / s:   C_c = -[(g_c . p) n + (n . v_c) J g + (g_c . n) p] / s"""
    dt = q.dtype
    v, gx = np.asarray(v, dt), np.asarray(gx, dt)
    s = np.sqrt((q * q).sum(axis=1, keepdims=True))
    n = q / s
    nv = (n * v).sum(axis=1, keepdims=True)
    ng = (n * gx).sum(axis=1, keepdims=True)
    p = (v - n * nv) / s
    jg = (gx - n * ng) / s
    gp = (gx * p).sum(axis=1, keepdims=True)
    return -(gp * n + nv * jg + ng * p) / s


def set_network(cfg, hidden=None, enc_act=None, beta=None, enc_beta=None):
    """model.DFNet.dims / beta and model.StrEnc.act / beta of a config, the way tests/train_fixtures.config sets them; None keeps
    amass.yaml's, and an encoder beta that is not given follows the trunk's"""
    if hidden is not None:
        cfg["model"]["DFNet"]["dims"] = list(hidden)
    if enc_act is not None:
        cfg["model"]["StrEnc"]["act"] = enc_act
    if beta is not None:
        cfg["model"]["DFNet"]["beta"] = float(beta)
        cfg["model"]["StrEnc"]["beta"] = float(beta)
    if enc_beta is not None:
        cfg["model"]["StrEnc"]["beta"] = float(enc_beta)
    return cfg


# (trunk activation, trunk beta, encoder activation, encoder beta, hidden widths) of the networks the host twin and the device are
# both held to the stock modules on.  None: the encoder's as the trunk's, amass.yaml's widths.  A beta is a factor of the result
# (sigma'' = beta s (1 - s)); the trunk's reaches the GEMM epilogue, the encoder's the bone code, by separate plumbing.  The widths:
# one unit (M = 1 forward, K = 1 reverse), odd widths below the 16-deep K step, eight row tiles and 64 K steps, one past and one
# short of the 128-row tile.  (Seven one-unit softplus layers are left out: in fp64 that network's gradient is 7e-144.)
NETWORKS = (
    ("softplus", 1.0, None, None, None),
    ("softplus", 10.0, None, None, None),
    ("softplus", 1000.0, None, None, None),
    ("softplus", 100.0, "softplus", 7.0, None),
    ("softplus", 10.0, "softplus", 1000.0, None),
    ("relu", 100.0, "softplus", 7.0, None),
    ("relu", 100.0, "softplus", 1000.0, None),
    ("lrelu", 100.0, "relu", None, None),
    ("relu", 100.0, "lrelu", None, None),
    ("softplus", 100.0, None, None, (1,)),
    ("softplus", 100.0, None, None, (17, 33, 65, 31, 15, 1)),
    ("softplus", 100.0, None, None, (1024, 1024)),
    ("lrelu", 100.0, None, None, (1024, 1024)),
    ("softplus", 10.0, None, None, (129, 127)),
)
# the three networks of the exact identities and of the row isolation: one per launch sequence (four passes over the layers, two
# passes and no tangent, two passes with the tangent and the primal chain in the encoder alone: `zero_a0`)
LAUNCH_SEQUENCES = (("softplus", 100.0, None, None, None), ("lrelu", 100.0, None, None, None), ("relu", 100.0, "softplus", 7.0, None))
TWIN_AND_DEVICE = (NETWORKS[2], NETWORKS[5], NETWORKS[13])


def network_id(net):
    act, beta, enc_act, enc_beta, hidden = net
    side = lambda a, b: f"{a}@{b:g}" if a == "softplus" else a      # noqa: E731
    name = side(act, beta)
    if enc_act is not None:
        name += "/" + side(enc_act, beta if enc_beta is None else enc_beta)
    return name + ("" if hidden is None else "-" + "x".join(str(w) for w in hidden))


def network_act_string(net):
    """oracle.posendf_np.parse_act's "DFNet.act@beta/StrEnc.act@beta" of a NETWORKS entry"""
    act, beta, enc_act, enc_beta, _ = net
    return f"{act}@{beta:g}/{act if enc_act is None else enc_act}@{beta if enc_beta is None else enc_beta:g}"


def network_weights(net):
    """the fixture's weights for amass.yaml's widths, seeded ones for any other"""
    from posendf_amd import synth
    hidden = net[4]
    return weights() if hidden is None else synth.make_weights(seed=3, gain=2.0, out_bias=0.1, dims=(126, *hidden, 1))


def network_kinks(net, sd):
    """the `kinks` of batch_inputs: None for a network without a relu-family part"""
    act, _, enc_act, _, _ = net
    return None if act == "softplus" and enc_act in (None, "softplus") else (sd, network_act_string(net))


def batch_inputs(B, seed=31, kinks=None):
    """B signed poses, normal directions and weights of both signs (numpy float32).  `kinks` = (weights, "trunk/encoder" activations)
    of a network with a relu-family part: only poses whose kink margin (oracle.posendf_np.kink_margin: the smallest |pre-activation|
    relative to its layer's largest) is at least 1e-5 -- conftest.outlier_gate's kink_tol -- are taken.  Nearer to a kink two correct
    fp32 evaluations may take different sides of it, and their derivatives then differ by O(1): such a pose measures no arithmetic."""
    from oracle import posendf_np as onp
    from posendf_amd import synth
    rs = np.random.RandomState(seed)
    q = synth.make_poses(2 * B + 8, seed=seed, signed=True).astype(np.float32)
    if kinks is not None:
        q = q[onp.kink_margin(q, *kinks) >= 1e-5]
    q = np.ascontiguousarray(q[:B])
    assert len(q) == B
    v = rs.normal(size=q.shape).astype(np.float32)
    w_d = (rs.uniform(0.5, 1.5, B) * np.where(rs.rand(B) < 0.5, -1, 1)).astype(np.float32)
    w_t = (rs.uniform(0.5, 1.5, B) * np.where(rs.rand(B) < 0.5, -1, 1)).astype(np.float32)
    return q, v, w_d, w_t


def stock_model(act, sd, device, dtype, hidden=None, enc_act=None, beta=None, enc_beta=None):
    """the stock PyTorch modules (posendf_amd.modules, the reference's own layers) with the weights `sd`, in `dtype` on `device`;
    `beta` / `enc_beta`: model.DFNet.beta / model.StrEnc.beta, the encoder's the trunk's where it is not given"""
    import torch
    from posendf_amd import amass_config
    from posendf_amd.modules import DFNet, StructureEncoder
    cfg = amass_config(act, "cpu")
    set_network(cfg, hidden, enc_act, beta, enc_beta)
    enc, dfnet = StructureEncoder(cfg["model"]["StrEnc"]), DFNet(cfg["model"]["DFNet"])
    enc.load_state_dict({k[len("enc."):]: torch.from_numpy(np.asarray(a)) for k, a in sd.items() if k.startswith("enc.")})
    dfnet.load_state_dict({k[len("dfnet."):]: torch.from_numpy(np.asarray(a)) for k, a in sd.items() if k.startswith("dfnet.")})
    return enc.to(device=device, dtype=dtype), dfnet.to(device=device, dtype=dtype)


def stock_second_order(model, q, v, w_d, w_t):
    """(d [B], g, t [B], out) by the stock modules' double backward, in the dtype and on the device of q (torch tensors)"""
    import torch
    enc, dfnet = model
    q = q.clone().requires_grad_(True)
    d = dfnet(enc(torch.nn.functional.normalize(q, dim=1)))
    (g,) = torch.autograd.grad(d.sum(), q, create_graph=True)
    t = (v * g).sum(dim=(1, 2))
    (out,) = torch.autograd.grad((w_d * d[:, 0] + w_t * t).sum(), q)
    return d.detach()[:, 0], g.detach(), t.detach(), out.detach()


def stock_reference(net, sd, args, device):
    """the stock modules' double backward of a NETWORKS entry on `device` for numpy (q, v, w_d, w_t) -> (fp32 results, fp64 results),
    each [d, g, t, out] in numpy: the envelope and the truth of `gate`"""
    import torch
    act, beta, enc_act, enc_beta, hidden = net
    res = []
    for dtype in (torch.float32, torch.float64):
        model = stock_model(act, sd, device, dtype, hidden, enc_act, beta, enc_beta)
        r = stock_second_order(model, *(torch.from_numpy(a).to(device=device, dtype=dtype) for a in args))
        res.append([a.cpu().numpy() for a in r])
    return res


def gate_all(tag, mine, ref32, ref64):
    """`gate` on d, g, t and out -> {output: err / the reference's fp32 err}"""
    ratios = {}
    for name, a, b, c in zip(OUTPUTS, mine, ref32, ref64):
        e_mine, e_ref = gate(a, b, c, f"{tag} {name}")
        ratios[name] = e_mine / e_ref
    return ratios


# ---- oracle-free checks, shared by the host twin's and the device's tests.  `run(q, v, w_d, w_t)` -> [d [B], g, t [B], out] in numpy
# float32 for numpy float32 inputs; w_d / w_t may be None (0 and 1)
def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check_exact_identities(run, q, v, w_d, w_t):
    """Every operation on the tangent chain is linear in v and expf never sees v, and `out` is linear in (w_d, w_t): a scaling by a
    power of two commutes with every rounding, fused or not, as long as nothing underflows.  No tolerance anywhere."""
    B = len(q)
    d, g, t, out = run(q, v, None, None)
    assert all(np.isfinite(a).all() for a in (d, g, t, out))
    # v -> 2 v: the primal chain does not see v
    d2, g2, t2, out2 = run(q, 2.0 * v, None, None)
    assert same_bits(d2, d) and same_bits(g2, g), "v -> 2v changed d or g"
    assert np.array_equal(t2, 2.0 * t) and np.array_equal(out2, 2.0 * out), "v -> 2v did not double t and out"
    # v -> -v
    dn, gn, tn, outn = run(q, -v, None, None)
    assert same_bits(dn, d) and same_bits(gn, g), "v -> -v changed d or g"
    assert np.array_equal(tn, -t) and np.array_equal(outn, -out), "v -> -v did not negate t and out"
    # v = 0: no tangent, out = w_d g (values: a signed zero is allowed)
    wg = w_d[:, None, None] * g
    assert wg.dtype == np.float32
    d0, g0, t0, out0 = run(q, np.zeros_like(v), w_d, w_t)
    assert same_bits(d0, d) and same_bits(g0, g)
    assert np.array_equal(t0, np.zeros(B, np.float32)), "v = 0 left a tangent"
    assert np.array_equal(out0, wg), "v = 0: out is not w_d g"
    # w_t = 0
    dz, gz, tz, outz = run(q, v, w_d, np.zeros_like(w_t))
    assert same_bits(dz, d) and same_bits(gz, g) and same_bits(tz, t)
    assert np.array_equal(outz, wg), "w_t = 0: out is not float32(w_d g)"
    # (w_d, w_t) -> s (w_d, w_t)
    base = run(q, v, w_d, w_t)
    assert same_bits(base[0], d) and same_bits(base[1], g) and same_bits(base[2], t)
    for s in (2.0 ** -40, 2.0 ** 23, -(2.0 ** 31)):
        s = np.float32(s)
        ds, gs, ts, outs = run(q, v, s * w_d, s * w_t)
        assert same_bits(ds, d) and same_bits(gs, g) and same_bits(ts, t), f"scaling the weights by {s} changed d, g or t"
        assert np.array_equal(outs, s * base[3]), f"scaling the weights by {s} did not scale out"


BAD_ROWS = (5, 7, 9, 128, 130, 257)      # 7, 130 and 257 sit in three 128-column GEMM tiles; 127 | 128 | 129 straddle a tile edge


def check_rows_are_independent(run, q, v, w_d, w_t, clamped_column_is_w_d_g):
    """A non-finite or clamped pose, direction or weight stays in its own row: every other row keeps the clean run's bits."""
    B = len(q)
    assert B == 300
    clean = run(q, v, w_d, w_t)
    assert all(np.isfinite(a).all() for a in clean)
    q, v, w_d = q.copy(), v.copy(), w_d.copy()
    q[7] = np.nan
    q[130, 3, 1] = np.inf
    q[257] = 0.0               # every column on the clamp of F.normalize
    q[128, :, 2] = 0.0         # one column on it
    v[5] = np.nan
    w_d[9] = np.inf
    dirty = run(q, v, w_d, w_t)
    keep = np.ones(B, bool)
    keep[list(BAD_ROWS)] = False
    assert keep[127] and keep[129] and keep.sum() == B - len(BAD_ROWS)
    for name, a, b in zip(OUTPUTS, clean, dirty):
        assert same_bits(a[keep], b[keep]), f"{name}: a disturbed row reached another row"
    for name, a, b in zip(OUTPUTS[:3], clean, dirty):      # w_d enters `out` alone
        assert same_bits(a[9], b[9]), f"{name}: w_d reached {name}"
    for row in (128, 257):
        assert all(np.isfinite(a[row]).all() for a in dirty), f"row {row} (clamped columns) is not finite"
    if clamped_column_is_w_d_g:      # sigma'' = 0 everywhere: H v = C, and a clamped column carries no curvature
        g = dirty[1]
        assert np.array_equal(dirty[3][128, :, 2], w_d[128] * g[128, :, 2]), "curvature on a clamped column"
        assert np.abs(g[128, :, 2]).max() > 0


def check_distance_zero(run, q, v, w_d, w_t):
    """behind an output bias of -1e3 the output ReLU is off for every pose: d, g, t and out are all exactly zero"""
    for name, a in zip(OUTPUTS, run(q, v, w_d, w_t)):
        assert np.array_equal(a, np.zeros_like(a)), f"{name} is not zero where the distance is clamped to zero"
