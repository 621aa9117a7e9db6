"""Weight and activation magnitude range of the runtime-planned HIP kernels (csrc/pndf_generic.hip), both forms: the exact fp32 one
and the split-precision one with its own operand scaling (pndf_pack::layer_scale, gen_pose_scale, gen_pose_scale_grad, gen_pow2_rcp).
Cases, rescalings, clamp prediction and gates: tests/depth_range.py; their CPU side: tests/test_depth_range.py.  The numpy oracle
(pinned at these depths by test_depth.test_oracle_is_pinned_at_other_depths) is the reference throughout.
  A  gain and bias sweep                  B  layer outputs rescaled by 1e-6 .. 1e5, jumps of 1e7 between layers
  C  power-of-two rescaling: the same bits on every pose whose scales meet no clamp
  D  the edges: the last 2^k before a clamp engages (gates and bits hold) and the first behind it (finite; recorded, not gated)
  E  grad_outputs of any magnitude        F  a half-precision checkpoint (every lo half of the packed weights zero)"""
import json
import os

import numpy as np
import pytest

import depth_range as dr
from conftest import REPO, d_rows, fp32_noise, rel_err_rows

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "f16x3"]
RESCALE_CASES = [(h, e, a) for h, e in dr.RESCALE_ARCHS for a in dr.RESCALE_ACTS]
EDGES_JSON = os.path.join(REPO, "profiles", "depth_range", "edges.json")


def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X (no CPU fallback exists)"


def _rescale_weights(hidden, enc, act):
    return dr.weights(hidden, enc, act, *dr.RESCALE_REGIME)


_BASE = {}


def _base_run(hidden, enc, act, precision):
    """d and d d/d q of the unrescaled network on the kernel under test: what the rescaled networks are compared with, word for word"""
    key = (tuple(hidden), enc, act, precision)
    if key not in _BASE:
        net = dr.make_net(hidden, act, enc, _rescale_weights(hidden, enc, act), "cuda:0", precision)
        _BASE[key] = dr.single_step(net, dr.poses(), "cuda:0")
    return _BASE[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hidden,enc,act,gain,bias", dr.SWEEP, ids=dr.case_id)
def test_gain_and_bias_sweep(hidden, enc, act, gain, bias, precision):
    """A: gains 0.5 .. 4 (activations and gradients from a hundredth to a hundred times the benchmark network's) on the planner's
    distinct paths: every pose through pose_gate, the 3-step projection through outlier_gate"""
    _gpu()
    dr.check_network(hidden, act, enc, dr.weights(hidden, enc, act, gain, bias), "cuda:0", precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pattern", list(dr.DECIMAL))
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_layer_scale_extremes(hidden, enc, act, pattern, precision):
    """B: the fused kernels' test of the same name on the runtime-planned ones: the per-layer weight scale and the per-pose operand
    scale must keep every operand inside fp16 whatever a layer's size and however it jumps to the next"""
    _gpu()
    sd = dr.rescaled(_rescale_weights(hidden, enc, act), dr.decimal_pattern(pattern, len(hidden)))
    dr.check_network(hidden, act, enc, sd, "cuda:0", precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pattern", list(dr.POW2))
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_power_of_two_rescaling_changes_no_bit(hidden, enc, act, pattern, precision):
    """C: scales that are exact powers of two read off the data cancel a power-of-two rescaling of the layers exactly: d and d d/d q
    of every pose whose scales meet no clamp (depth_range.predicted_clamp) are the unrescaled network's, as uint32 words.  A fixed
    scale, a clamp that engages early or a scale that is no power of two fails at once."""
    _gpu()
    base = _rescale_weights(hidden, enc, act)
    c = dr.pow2_pattern(pattern, len(hidden))
    q = dr.poses()
    free = ~dr.predicted_clamp(q, base, act, c)
    assert free.mean() >= 0.9, float(free.mean())
    d0, g0 = _base_run(hidden, enc, act, precision)
    net = dr.make_net(hidden, act, enc, dr.rescaled(base, c), "cuda:0", precision)
    d1, g1 = dr.single_step(net, q, "cuda:0")
    import torch
    assert net._engine_for(torch.device("cuda:0")).kernel_name() == dr.generic_kernel(act, enc, precision)
    same = dr.same_bits(d0, d1) & dr.same_bits(g0, g1)
    print(f"[pow2 {hidden} {act} {pattern} {precision}] {int(free.sum())} poses free of clamps, {int((~same & free).sum())} of them differ, "
          f"{int((~same & ~free).sum())} of the others")
    assert same[free].all(), (pattern, np.flatnonzero(~same & free)[:8].tolist())


def _record_edge(key, entry):
    os.makedirs(os.path.dirname(EDGES_JSON), exist_ok=True)
    table = json.load(open(EDGES_JSON)) if os.path.exists(EDGES_JSON) else {}
    table[key] = entry
    with open(EDGES_JSON, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("side", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_edges_of_the_scale_range(hidden, enc, act, side, precision):
    """D: uniform 2^k, walked outwards in steps of 8 from 2^+-24 until predicted_clamp engages for most poses.  At the last k before:
    the gates of A and the bits of C.  At the first k behind: finite results; the error against fp64 and whether the bits moved are
    printed and recorded in profiles/depth_range/edges.json (DESIGN.md 2c "Magnitude range" states the edge; no accuracy is asserted)."""
    _gpu()
    import torch
    base = _rescale_weights(hidden, enc, act)
    q = dr.poses()
    last, first = dr.walk_to_edge(q, base, act, side, len(hidden))
    d0, g0 = _base_run(hidden, enc, act, precision)
    # the last k before the edge
    c = dr.uniform(last, len(hidden))
    d1, g1, _ = dr.check_network(hidden, act, enc, dr.rescaled(base, c), "cuda:0", precision)
    free = ~dr.predicted_clamp(q, base, act, c)
    same = dr.same_bits(d0, d1) & dr.same_bits(g0, g1)
    assert same[free].all(), (last, np.flatnonzero(~same & free)[:8].tolist())
    # the first k behind it
    c = dr.uniform(first, len(hidden))
    sd = dr.rescaled(base, c)
    net = dr.make_net(hidden, act, enc, sd, "cuda:0", precision)
    d2, g2 = dr.single_step(net, q, "cuda:0")
    kernel = net._engine_for(torch.device("cuda:0")).kernel_name()
    clamped = dr.predicted_clamp(q, base, act, c)
    _, _, d64, g64 = fp32_noise(q, sd, act)
    finite = bool(np.isfinite(d2).all() and np.isfinite(g2).all())
    with np.errstate(invalid="ignore"):
        e_d, e_g = d_rows(d2, d64), rel_err_rows(g2, g64)
    moved = ~(dr.same_bits(d0, d2) & dr.same_bits(g0, g2))
    entry = {"last_unclamped_log2": last, "first_clamped_log2": first, "kernel": kernel, "poses": len(q), "predicted_clamped": int(clamped.sum()),
             "finite": finite, "poses_whose_bits_moved": int(moved.sum()),
             "d_err_median": float(np.nanmedian(e_d)), "d_err_max": float(np.nanmax(e_d)),
             "dq_err_median": float(np.nanmedian(e_g)), "dq_err_max": float(np.nanmax(e_g))}
    print(f"[edge {hidden} {act} {'up' if side > 0 else 'down'} {precision}] {entry}")
    _record_edge(f"{dr.case_id(hidden)} {act} {'up' if side > 0 else 'down'} {precision}", entry)
    assert finite, entry


@pytest.mark.parametrize("go", [1e-12, -3e9])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_grad_outputs_of_any_magnitude(act, precision, go):
    """E: the upstream gradient multiplies the RESULT of the backward pass, never its fp16 operands: dq(go) = go * dq(1) to one rounding
    (tests/test_gpu_parity.py, the same assertion)"""
    _gpu()
    import torch
    hidden, enc = [384, 384], True
    net = dr.make_net(hidden, act, enc, dr.weights(hidden, enc, act, 2.5, 0.3), "cuda:0", precision)
    qn = dr.poses()
    q = torch.from_numpy(qn).cuda().requires_grad_(True)
    d = net(q, train=False)["dist_pred"]
    (g1,) = torch.autograd.grad(d.sum(), q)
    q2 = torch.from_numpy(qn).cuda().requires_grad_(True)
    (g2,) = torch.autograd.grad(net(q2, train=False)["dist_pred"], q2, grad_outputs=torch.full_like(d, go))
    assert net._engine_for(q.device).kernel_name() == dr.generic_kernel(act, enc, precision)
    ref = g1.double() * go
    err = (g2.double() - ref).abs().amax(dim=(1, 2)) / ref.abs().amax(dim=(1, 2)).clamp_min(1e-300)
    assert float(g1.abs().max()) > 0 and torch.isfinite(g2).all() and float(err.max()) < 3e-7, float(err.max())


@pytest.mark.parametrize("act", ["lrelu", "softplus"])
def test_half_precision_checkpoint(act):
    """F: weights that are fp16 numbers: every lo half of the packed stream is zero (the fused kernels take their two-term form on such
    a table; here the three-term form must simply be right with a term of zeros)"""
    _gpu()
    hidden, enc = [384, 384], True
    sd = {k: v.astype(np.float16).astype(np.float32) for k, v in dr.weights(hidden, enc, act, *dr.RESCALE_REGIME).items()}
    dr.check_network(hidden, act, enc, sd, "cuda:0", "f16x3")
