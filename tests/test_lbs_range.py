"""The a-priori bounds behind the operand scales of the split-precision body-model kernels (posendf_amd/csrc/pndf_lbs_scales.h),
checked with no kernel in the loop: the scales are READ from the library (pndf_debug_lbs_scales: the function pndf_lbs_create and
every launch call), the operands come from the fp64 oracle (oracle/lbs_np.py) at heavy-tailed models, three length units, poses
up to |R - I| = 2 and term weights six decades apart (tests/lbs_stress.py).

  headroom          every operand x its scale is finite and < 2^14 -- the design's own statement ("bound * s in [2^13, 2^14)");
                    an operand above its bound saturates silently on the device (v_cvt_pkrtz rounds toward zero)
  arithmetic model  the four contractions from fp16 hi / lo halves with the three kept products, in float64, against the exact
                    contraction: the split arithmetic's predicted error per length unit, below the gates of the GPU tests
                    (tests/test_lbs_range_gpu.py).  The halves are rounded to nearest (test_lbs_split_layout.split, as the host
                    packer does); the device splits its own operands toward zero, which costs up to 2^-21 more per operand."""
import numpy as np
import pytest

from lbs_stress import COEFS, KINDS, MOTIONS, SATURATING_TWINS, UNITS, stress_model, stress_theta
from oracle import lbs_np
from test_lbs_split_layout import split

S, T = 2, 17
LIMIT = 2.0 ** 14
NAMES = ("p_scale", "w_scale", "a_scale", "g_scale", "x_scale", "max_p", "max_w", "w_rowsum", "vp_bound", "a_bound", "g_bound", "x_bound", "pf_scale")
FORWARD_GATE, GRADIENT_GATE = 1e-5, 1e-4      # tests/test_lbs_gpu.py: forward 1e-5, fused-terms gradient max(1e-4, 8 ref)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def term_weights(model, T, coefs):
    """the weights over the means of the two terms (oracle/lbs_np.body_terms: coef / nrm.size), in float32 like pndf_lbs_terms_grad_w"""
    V, nj = model["v_template"].shape[0], 24 + len(model["extra_joint_vertex"])
    w_temp = np.float32(coefs[0]) / (np.float32(T - 1) * np.float32(V)) if T > 1 else np.float32(0)
    w_data = np.float32(coefs[1]) / (np.float32(T) * np.float32(nj)) if coefs[1] != 0 else np.float32(0)
    return float(w_temp), float(w_data)


def read_scales(lib, packed, w_temp, w_data):
    blob, J, rel = packed
    out = np.zeros(len(NAMES), np.float32)
    V = int((blob[:, 10544:10560].view(np.int32) > -2).sum())
    assert lib.pndf_debug_lbs_scales(V, blob.ctypes.data, J.ctypes.data, rel.ctypes.data, w_temp, w_data, out.ctypes.data) == 0
    return dict(zip(NAMES, out.astype(np.float64)))


def operands(model, theta, joints0, coefs):
    """ONE sequence: the true operands of the four contractions (unscaled), from the fp64 oracle"""
    with np.errstate(invalid="ignore", divide="ignore"):
        _, _, c = lbs_np.body_terms(theta, joints0, model, 1 if coefs[1] != 0 else 0, coefs=coefs, keep=True)
    gV = np.array(c["gV"])
    np.add.at(gV, (slice(None), np.asarray(model["extra_joint_vertex"])), c["gJ"][:, 24:])      # the picked vertices' data term
    A_t = c["G_t"] - (c["G_R"] @ c["J"][None, :, :, None])[..., 0]
    vp1 = np.concatenate([c["v_posed"], np.ones(c["v_posed"].shape[:2] + (1,))], -1)
    return {"pf": c["pf"], "A_R": c["G_R"], "A_t": A_t,
            "g": np.einsum("nvab,nva->nvb", c["T_R"], gV),                # T_R^T d L / d verts
            "x": gV[..., :, None] * vp1[..., None, :], "gV": gV}          # d L / d verts (x) [v_posed, 1]


def test_scale_readout_is_the_packers(lib):
    """the read-out and pndf_lbs_pack_split_host give the same p_scale, w_scale; null pointers and V < 1 are refused"""
    from test_lbs_oracle import _pack
    from test_lbs_split_layout import _pack_split
    m = stress_model(41, 5)
    packed = _pack(m)
    s = read_scales(lib, packed, 0.01, 0.5)
    _, _, p_scale, w_scale = _pack_split(m)
    assert s["p_scale"] == p_scale and s["w_scale"] == w_scale and s["pf_scale"] == 4096.0
    for k in NAMES[:5]:
        assert np.log2(s[k]) % 1 == 0, k
    assert 2.0 ** 12 <= s["max_p"] * s["p_scale"] < 2.0 ** 13 and 2.0 ** 12 <= s["a_bound"] * s["a_scale"] < 2.0 ** 13
    assert 2.0 ** 13 <= s["g_bound"] * s["g_scale"] < LIMIT and 2.0 ** 13 <= s["x_bound"] * s["x_scale"] < LIMIT
    blob, J, rel = packed
    out = np.zeros(len(NAMES), np.float32)
    assert lib.pndf_debug_lbs_scales(0, blob.ctypes.data, J.ctypes.data, rel.ctypes.data, 1.0, 1.0, out.ctypes.data) == -1
    assert lib.pndf_debug_lbs_scales(41, None, J.ctypes.data, rel.ctypes.data, 1.0, 1.0, out.ctypes.data) == -1
    assert lib.pndf_debug_lbs_scales(41, blob.ctypes.data, J.ctypes.data, rel.ctypes.data, 1.0, 1.0, None) == -1


def test_every_operand_stays_below_its_bound(lib):
    """kind x unit x motion x coefs: operand x scale finite and < 2^14.  A condition, not a measurement: the fp64 oracle stays
    inside it or the bound is wrong.  Printed (not gated): per operand class the smallest log2(max |operand x scale|) over
    all cases = how far the a-priori bound overshoots at worst (14 = none)."""
    from test_lbs_oracle import _pack
    lowest, highest = {}, {}
    failures = []
    cases = 0
    for kind in KINDS:
        for unit in UNITS:
            m = stress_model(137, 9, unit=unit, kind=kind)
            packed = _pack(m)
            P = np.asarray(m["posedirs"], np.float64)
            W = np.asarray(m["lbs_weights"], np.float64)
            for motion in MOTIONS:
                th = stress_theta(S, T, 4, motion)
                th0 = th + np.random.default_rng(1).normal(size=th.shape).astype(np.float32) * 0.05
                twins = list(SATURATING_TWINS) if motion == "saturating" else []
                keep = np.setdiff1d(np.arange(T), twins)
                for coefs in COEFS:
                    cases += 1
                    sc = read_scales(lib, packed, *term_weights(m, T, coefs))
                    for s in range(S):
                        _, J0 = lbs_np.lbs(th0[s], m)
                        op = operands(m, th[s], J0, coefs)
                        if twins:      # identical frames: the reference's NaN (no epsilon under the root), there and only there
                            assert np.isnan(op["gV"][twins]).all() and np.isfinite(op["gV"][keep]).all()
                        scaled = {"pf": sc["pf_scale"] * op["pf"], "A_R": sc["a_scale"] * op["A_R"], "A_t": sc["a_scale"] * op["A_t"],
                                  "P": sc["p_scale"] * P, "W": sc["w_scale"] * W,
                                  "g": sc["g_scale"] * op["g"][keep], "x": sc["x_scale"] * op["x"][keep]}
                        for name, x in scaled.items():
                            top = np.abs(x).max()
                            if not (np.isfinite(x).all() and top < LIMIT):
                                failures.append(f"{kind} unit {unit:g} {motion} coefs {coefs} seq {s}: {name} max {top:.6g} (2^{np.log2(top):.2f})")
                            if top > 0:
                                lowest[name] = min(lowest.get(name, np.inf), np.log2(top))
                                highest[name] = max(highest.get(name, -np.inf), np.log2(top))
    print(f"headroom over {cases} cases (kind x unit x motion x coefs), {S} sequences of {T} frames each:")
    for name, lg in lowest.items():
        print(f"  {name:4s} log2(max |operand x scale|): smallest {lg:6.2f}  largest {highest[name]:6.2f}")
    assert cases == len(KINDS) * len(UNITS) * len(MOTIONS) * len(COEFS)
    assert not failures, "\n".join(failures)


def contraction_errors(lib, unit, motion, coefs, products=("hh", "hl", "lh"), V=137):
    """{contraction: error of the split arithmetic relative to the largest exact output entry} at the library's scales"""
    from test_lbs_oracle import _pack
    m = stress_model(V, 9, unit=unit)
    sc = read_scales(lib, _pack(m), *term_weights(m, T, coefs))
    th = stress_theta(1, T, 4, motion)[0]
    _, J0 = lbs_np.lbs(th + np.float32(0.04), m)
    op = operands(m, th, J0, coefs)
    keep = np.setdiff1d(np.arange(T), SATURATING_TWINS if motion == "saturating" else [])
    P = np.asarray(m["posedirs"], np.float64).reshape(207, V, 3)
    W = np.asarray(m["lbs_weights"], np.float64)
    A = np.concatenate([op["A_R"].reshape(T, 24, 9), op["A_t"]], -1)                       # [n, j, 12]
    x = op["x"][keep].reshape(len(keep), V, 12)
    jobs = {"pose blend": ("kvc,nk->nvc", P * sc["p_scale"], op["pf"] * sc["pf_scale"]),
            "skinning": ("vj,nje->nve", W * sc["w_scale"], A * sc["a_scale"]),
            "d/d pose feature": ("kvc,nvc->nk", P * sc["p_scale"], op["g"][keep] * sc["g_scale"]),
            "d/d A": ("vj,nve->nje", W * sc["w_scale"], x * sc["x_scale"])}
    errs = {}
    for name, (spec, a, b) in jobs.items():
        (ah, al), (bh, bl) = split(a), split(b)
        assert np.isfinite(ah).all() and np.isfinite(bh).all(), name      # (fp16 overflow would show as inf here)
        got = sum(np.einsum(spec, u, v) for key, u, v in (("hh", ah, bh), ("hl", ah, bl), ("lh", al, bh)) if key in products)
        want = np.einsum(spec, a, b)
        errs[name] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    return errs


GATES = {"pose blend": FORWARD_GATE, "skinning": FORWARD_GATE, "d/d pose feature": GRADIENT_GATE, "d/d A": GRADIENT_GATE}


@pytest.mark.parametrize("unit", UNITS)
def test_split_arithmetic_predicted_error_is_below_the_gpu_gates(lib, unit):
    """hi hi + hi lo + lo hi at the library's scales, per length unit, ordinary and saturating poses, every coefs pair: strictly
    below the gates the GPU tests hold the kernels to."""
    worst = dict.fromkeys(GATES, 0.0)
    for motion in ("ordinary", "saturating"):
        for coefs in COEFS:
            for name, e in contraction_errors(lib, unit, motion, coefs).items():
                worst[name] = max(worst[name], e)
    print(f"split arithmetic, predicted, unit {unit:g}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e < GATES[name], (unit, name, e)


def test_arithmetic_model_sees_a_dropped_product(lib):
    """the model is sharp: without the lo hi product the predicted error of the forward contractions leaves their gate"""
    e = contraction_errors(lib, 1.0, "ordinary", COEFS[3], products=("hh", "hl"))
    print("split arithmetic without lo hi: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["pose blend"] > FORWARD_GATE and e["skinning"] > FORWARD_GATE
