"""The inputs of tests/test_depth_range_gpu.py, checked where no GPU is needed (the cases, rescalings and gates live in
tests/depth_range.py): every case of the gain and bias sweep has a live network, the fp32 oracle itself passes the gates on every
regime and every rescaled network and is invariant to the bit under the power-of-two rescalings, the clamp prediction follows the
constants of csrc/pndf_generic.hip, and the library's host twins (`train.device: cpu`) meet the same gates."""
import os
import re

import numpy as np
import pytest

import depth_range as dr
from conftest import REPO

SWEEP_ARGS = ("hidden,enc,act,gain,bias", dr.SWEEP)
RESCALE_CASES = [(h, e, a) for h, e in dr.RESCALE_ARCHS for a in dr.RESCALE_ACTS]


def _rescale_weights(hidden, enc, act):
    return dr.weights(hidden, enc, act, *dr.RESCALE_REGIME)


@pytest.mark.parametrize(*SWEEP_ARGS, ids=dr.case_id)
def test_every_sweep_case_is_live_and_the_fp32_oracle_passes_its_gates(hidden, enc, act, gain, bias):
    """a live seed in 50 .. 89 (none: a failure, not a skip), the network still alive on the 200 poses of the GPU test, and the fp32
    oracle against fp64 inside pose_gate: a regime on which the reference arithmetic misses the gate cannot judge a kernel"""
    from oracle import posendf_np as onp
    sd = dr.weights(hidden, enc, act, gain, bias)
    q = dr.poses()
    d32, g32 = onp.forward_grad(q, sd, act)
    assert (d32 > 1e-3).mean() > 0.5, float((d32 > 1e-3).mean())
    assert dr.single_step_gates(d32, g32, q, sd, act, f"oracle {hidden} {act} gain {gain}") <= 1.0


@pytest.mark.parametrize("pattern", list(dr.DECIMAL) + list(dr.POW2))
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_fp32_oracle_passes_its_gates_on_rescaled_networks(hidden, enc, act, pattern):
    from oracle import posendf_np as onp
    base = _rescale_weights(hidden, enc, act)
    c = dr.decimal_pattern(pattern, len(hidden)) if pattern in dr.DECIMAL else dr.pow2_pattern(pattern, len(hidden))
    sd = dr.rescaled(base, c)
    q = dr.poses()
    # the same function in fp64 (2e-6 in d: the decimal factors are rounded to fp32 weights)
    d_base, d_resc = onp.forward(q, base, act, dtype=np.float64), onp.forward(q, sd, act, dtype=np.float64)
    assert np.abs(d_resc - d_base).max() <= 2e-6 * max(np.abs(d_base).max(), 1.0)
    d32, g32 = onp.forward_grad(q, sd, act)
    assert dr.single_step_gates(d32, g32, q, sd, act, f"oracle {hidden} {act} {pattern}") <= 1.0


@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_fp32_oracle_is_bit_invariant_under_power_of_two_rescaling(hidden, enc, act):
    """what the GPU test asks of the kernels holds for the reference arithmetic on EVERY pose, and the clamp prediction leaves at
    least 90 % of the poses to be compared"""
    from oracle import posendf_np as onp
    base = _rescale_weights(hidden, enc, act)
    q = dr.poses()
    d0, g0 = onp.forward_grad(q, base, act)
    assert not dr.predicted_clamp(q, base, act).any()
    for pattern in dr.POW2:
        c = dr.pow2_pattern(pattern, len(hidden))
        d1, g1 = onp.forward_grad(q, dr.rescaled(base, c), act)
        assert dr.same_bits(d0, d1).all() and dr.same_bits(g0, g1).all(), pattern
        assert (~dr.predicted_clamp(q, base, act, c)).mean() >= 0.9, (pattern, float(dr.predicted_clamp(q, base, act, c).mean()))


@pytest.mark.parametrize("side", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_edge_walk_ends_within_ten_steps(hidden, enc, act, side):
    """uniform 2^k outwards from 2^+-24: an edge is found, and at the last k before it the oracle is still bit-invariant"""
    from oracle import posendf_np as onp
    base = _rescale_weights(hidden, enc, act)
    q = dr.poses()
    last, first = dr.walk_to_edge(q, base, act, side, len(hidden))
    assert abs(first - last) == 8 and abs(last) >= 24
    d0, g0 = onp.forward_grad(q, base, act)
    d1, g1 = onp.forward_grad(q, dr.rescaled(base, dr.uniform(last, len(hidden))), act)
    assert dr.same_bits(d0, d1).all() and dr.same_bits(g0, g1).all(), last
    print(f"[edge {hidden} {act} {'up' if side > 0 else 'down'}] last unclamped 2^{last}, first clamped 2^{first}")


def test_clamp_bounds_are_the_kernel_constants():
    """FWD_E / BWD_E restate gen_pose_scale / gen_pose_scale_grad; the bounds follow from them"""
    src = open(os.path.join(REPO, "posendf_amd", "csrc", "pndf_generic.hip")).read()
    clamps = re.findall(r"float (gen_pose_scale\w*)\(float bound\) \{.*?e = e < (\d+)u \? \d+u : \(e > (\d+)u", src, flags=re.S)
    assert {n: (int(a), int(b)) for n, a, b in clamps} == {"gen_pose_scale": dr.FWD_E, "gen_pose_scale_grad": dr.BWD_E}, clamps
    assert dr.clamp_bounds(dr.FWD_E) == (2.0 ** -27, 2.0 ** 53) and dr.clamp_bounds(dr.BWD_E) == (2.0 ** -80, 2.0 ** 53)


def test_predicted_clamp_sees_each_bound():
    """one hidden layer scaled so that its activations (forward) or its adjoints (backward) cross a bound: predicted on that side only
    when the margin is crossed"""
    hidden, enc, act = [384, 384], True, "lrelu"
    base = _rescale_weights(hidden, enc, act)
    q = dr.poses()
    fwd, bwd = dr.operand_maxima(q, base, act)
    assert fwd.shape == (200, 3) and bwd.shape == (200, 2)
    k_hi = int(np.floor(np.log2(2.0 ** 52 / fwd[:, 1].max())))         # every pose's layer-1 input stays below 2^52
    assert not dr.predicted_clamp(q, base, act, (2.0 ** k_hi, 1.0)).any()
    assert dr.predicted_clamp(q, base, act, (2.0 ** (k_hi + 8), 1.0)).any()
    k_lo = int(np.ceil(np.log2(2.0 ** -26 / fwd[:, 1].min())))
    assert not dr.predicted_clamp(q, base, act, (2.0 ** k_lo, 1.0)).any()
    assert dr.predicted_clamp(q, base, act, (2.0 ** (k_lo - 8), 1.0)).any()
    # (the adjoint of a layer's pre-activations is 1 / c_l of the original: under a rescaling the forward bounds are always met
    # first, the backward window being the wider one on both sides)
    assert (bwd[:, 0] * 2.0 ** -k_lo <= 2.0 ** 52).all() and (bwd[:, 0] * 2.0 ** -k_hi >= 2.0 ** -79).all()


@pytest.mark.parametrize(*SWEEP_ARGS, ids=dr.case_id)
def test_host_twins_on_the_regime_sweep(hidden, enc, act, gain, bias):
    dr.check_network(hidden, act, enc, dr.weights(hidden, enc, act, gain, bias), "cpu")


@pytest.mark.parametrize("pattern", list(dr.DECIMAL))
@pytest.mark.parametrize("hidden,enc,act", RESCALE_CASES, ids=dr.case_id)
def test_host_twins_on_rescaled_networks(hidden, enc, act, pattern):
    sd = dr.rescaled(_rescale_weights(hidden, enc, act), dr.decimal_pattern(pattern, len(hidden)))
    dr.check_network(hidden, act, enc, sd, "cpu")
