"""The a-priori bounds behind the operand scales of the split-precision body-model kernels (posendf_amd/csrc/pndf_lbs_scales.h),
checked with no kernel in the loop: the scales are READ from the library (pndf_debug_lbs_scales: the function pndf_lbs_create and
every launch call), the operands come from the fp64 oracle (oracle/lbs_np.py) at heavy-tailed models, three length units, poses
up to |R - I| = 2 and term weights six decades apart (tests/lbs_stress.py).

  headroom          every operand x its scale is finite and < 2^14 -- the design's own statement ("bound * s in [2^13, 2^14)");
                    an operand above its bound saturates silently on the device (v_cvt_pkrtz rounds toward zero)
  arithmetic model  the four contractions from fp16 hi / lo halves with the three kept products, in float64, against the exact
                    contraction: the split arithmetic's predicted error per length unit, below the gates of the GPU tests
                    (tests/test_lbs_range_gpu.py).  The halves are rounded to nearest (test_lbs_split_layout.split, as the host
                    packer does); the device splits its own operands toward zero, which costs up to 2^-21 more per operand.
  marginal gates    tests/lbs_gates.py, the per-joint / per-frame / per-vertex gates of the GPU tests, held here against the
                    oracle's two reference arithmetics (float32, and oracle/lbs_np.split_contractions = the split kernels'
                    stated arithmetic): sound (a ninth draw passes the gate of the other eight) and sharp (a cross product
                    dropped from one contraction leaves it; the older whole-sequence gates let "d/d A" mutants through)."""
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


def contraction_errors(lib, unit, motion, coefs, products=("hh", "hl", "lh"), V=137, full=False):
    """{contraction: error of the split arithmetic relative to the largest exact output entry} at the library's scales;
    full=True: {contraction: (einsum spec, model operand, per-frame operand, its result in scaled units)} and the scales"""
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
    errs, everything = {}, {}
    for name, (spec, a, b) in jobs.items():
        (ah, al), (bh, bl) = split(a), split(b)
        assert np.isfinite(ah).all() and np.isfinite(bh).all(), name      # (fp16 overflow would show as inf here)
        got = sum(np.einsum(spec, u, v) for key, u, v in (("hh", ah, bh), ("hl", ah, bl), ("lh", al, bh)) if key in products)
        want = np.einsum(spec, a, b)
        errs[name] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
        everything[name] = (spec, a, b, got)
    return (everything, sc) if full else errs


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


# ---------------------------------------------------------------- the marginal gates (tests/lbs_gates.py), held on the host
def test_split_halves_follow_the_two_rounding_rules():
    """to nearest = test_lbs_split_layout.split bit for bit; toward zero: |hi| <= |x| always, saturating at 65504, and hi + lo
    within 2^-21 |x| (hi leaves up to 2^-10, lo keeps 11 bits of that)"""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=4000) * 10.0 ** rng.uniform(-3, 4, 4000), [0.0, 65504.0, -65519.9, 70000.0, 2.0 ** -14, -1e-7]])
    for mine, theirs in zip(lbs_np.split_halves(x), split(x[np.abs(x) < 65520])):
        assert np.array_equal(mine[np.abs(x) < 65520], theirs)
    hi, lo = lbs_np.split_halves(x, toward_zero=True)
    assert (np.abs(hi) <= np.abs(x)).all() and np.abs(hi).max() == 65504.0 and (hi * x >= 0).all()
    inside = np.abs(x) <= 65504
    assert (np.abs(hi + lo - x)[inside] <= 2.0 ** -21 * np.abs(x)[inside] + 2.0 ** -25).all()      # (+ half an fp16 subnormal)


@pytest.mark.parametrize("products", [lbs_np.PRODUCTS, ("hh", "hl"), ("hh", "lh")])
def test_split_mode_oracle_reproduces_the_arithmetic_model(lib, products):
    """each of the four contractions of lbs_np.split_contractions, taken alone with both operands rounded to nearest and float64
    accumulation, is contraction_errors' `got` for the same operands and scales (to the summation order); in the device's form
    (float32 operands, per-frame operand split toward zero, float32 accumulation) the full product set stays inside
    (2^-19 + K 2^-24) sum |a| |b|, K the contraction length"""
    jobs, sc = contraction_errors(lib, 1.0, "ordinary", COEFS[3], products=products, full=True)
    assert list(jobs) == list(lbs_np.CONTRACTIONS)
    for name, (spec, a, b, got) in jobs.items():
        sa, sb = (sc[k] for k in lbs_np.CONTRACTIONS[name])
        model64 = lbs_np.split_contractions(sc, {name: products}, device_rounding=False, acc=np.float64)
        mine = model64(name, spec, a / sa, b / sb) * (sa * sb)
        assert np.abs(mine - got).max() <= 1e-12 * np.abs(got).max(), (name, products)
        if products == lbs_np.PRODUCTS:
            K = {"pose blend": 207, "skinning": 24, "d/d pose feature": 3 * 137, "d/d A": 137}[name]
            dev = lbs_np.split_contractions(sc)(name, spec, (a / sa).astype(np.float32), (b / sb).astype(np.float32)).astype(np.float64) * (sa * sb)
            assert dev.dtype == np.float64 and (np.abs(dev - np.einsum(spec, a, b)) <= (2.0 ** -19 + K * 2.0 ** -24) * np.einsum(spec, np.abs(a), np.abs(b))).all(), name


_GATE_CASES = {}


def gate_case(lib, V, unit, motion, coefs=COEFS[3]):
    """model, inputs, fp64 truth and the two reference arithmetics' envelopes (forward and gradient) of one case, made once"""
    import lbs_gates
    key = (V, unit, motion, coefs)
    if key not in _GATE_CASES:
        from test_lbs_oracle import _pack
        m = stress_model(V, 9, unit=unit)
        th = stress_theta(S, T, 4, motion)
        th0 = th + np.random.default_rng(1).normal(size=th.shape).astype(np.float32) * 0.05
        j0 = lbs_np.lbs(th0.reshape(-1, 69), m)[1].astype(np.float32).reshape(S, T, -1, 3)
        flat = th.reshape(-1, 69)
        hooks = {"fp32": None, "f16x3": lbs_np.split_contractions(read_scales(lib, _pack(m), *term_weights(m, T, coefs)))}
        fwd64 = lbs_np.lbs(flat, m)
        grad64 = lbs_gates.terms_ref(m, 1, coefs, dtype=np.float64)(th, j0)
        env = {p: (lbs_gates.envelope(lbs_gates.forward_ref(m, h), [flat], fwd64),
                   lbs_gates.envelope(lbs_gates.terms_ref(m, 1, coefs, h), [th, j0], grad64)) for p, h in hooks.items()}
        _GATE_CASES[key] = dict(m=m, th=th, j0=j0, flat=flat, hooks=hooks, fwd64=fwd64, grad64=grad64, env=env,
                                scales=read_scales(lib, _pack(m), *term_weights(m, T, coefs)))
    return _GATE_CASES[key]


@pytest.mark.parametrize("motion", ["ordinary", "wide", "slow"])
@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("V", [41, 137])
def test_marginal_gate_is_sound(lib, V, unit, motion):
    """a ninth draw of each reference arithmetic passes the gate built from the other eight: forward (vertices, joints) and
    gradient, float32 and split.  A reference that fails its own gate would mean the gate is wrong."""
    import lbs_gates
    c = gate_case(lib, V, unit, motion)
    for p, hook in c["hooks"].items():
        (env_v, env_j), env_g = c["env"][p]
        v9, j9 = lbs_gates.forward_ref(c["m"], hook)(*lbs_gates.perturbed([c["flat"]], lbs_gates.DRAWS))
        g9 = lbs_gates.terms_ref(c["m"], 1, COEFS[3], hook)(*lbs_gates.perturbed([c["th"], c["j0"]], lbs_gates.DRAWS))
        tag = f"ninth draw {p} V={V} unit={unit:g} {motion}"
        lbs_gates.gate(tag + " verts", v9, c["fwd64"][0], env_v, lbs_gates.VERTICES)
        lbs_gates.gate(tag + " joints", j9, c["fwd64"][1], env_j, lbs_gates.JOINTS)
        lbs_gates.gate(tag + " grad", g9, c["grad64"], env_g, lbs_gates.GRADIENT)


MUTANTS = [(name, kept) for name in lbs_np.CONTRACTIONS for kept in (("hh", "hl"), ("hh", "lh"))]
MUTANT_NAMES = {("hh", "hl"): "lo hi", ("hh", "lh"): "hi lo"}      # kept products -> the product left out (model x per-frame operand)


def mutant_table(lib, device_rounding):
    """{mutant: worst error / bound per result over the marginals, and the whole-sequence error against the older gradient gate
    max(1e-4, 8 ref) of tests/test_lbs_range_gpu.check_gradient}: unit 1, ordinary, COEFS[3], V = 137, T = 17"""
    import lbs_gates
    c = gate_case(lib, 137, 1.0, "ordinary")
    (env_v, env_j), env_g = c["env"]["f16x3"]
    ref32 = lbs_gates.terms_ref(c["m"], 1, COEFS[3])(c["th"], c["j0"])
    table = {}
    for name, kept in MUTANTS:
        hook = lbs_np.split_contractions(c["scales"], {name: kept}, device_rounding=device_rounding)
        worst = {}
        if name in ("pose blend", "skinning"):
            v, j = lbs_gates.forward_ref(c["m"], hook)(c["flat"])
            worst["verts"] = max(lbs_gates.marginal_ratios(v, c["fwd64"][0], env_v, lbs_gates.VERTICES).values())
            worst["joints"] = max(lbs_gates.marginal_ratios(j, c["fwd64"][1], env_j, lbs_gates.JOINTS).values())
        g = lbs_gates.terms_ref(c["m"], 1, COEFS[3], hook)(c["th"], c["j0"])
        worst["grad"] = max(lbs_gates.marginal_ratios(g, c["grad64"], env_g, lbs_gates.GRADIENT).values())
        old = []
        for s in range(S):
            scale = np.abs(c["grad64"][s]).max()
            old.append(np.abs(g[s] - c["grad64"][s]).max() / scale / max(GRADIENT_GATE, 8 * np.abs(ref32[s] - c["grad64"][s]).max() / scale))
        worst["old gradient gate"] = float(max(old))
        table[f"{name} without {MUTANT_NAMES[kept]}"] = worst
        print(f"[lbs_gate mutant, halves {'toward zero' if device_rounding else 'to nearest'}] {name:17s} without {MUTANT_NAMES[kept]}: "
              + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return table


ESCAPES = ("d/d pose feature without lo hi", "d/d pose feature without hi lo")


def test_marginal_gate_is_sharp(lib):
    """The split-mode oracle with lo hi or hi lo left out of ONE contraction -- eight mutants; unit 1, ordinary, COEFS[3],
    V = 137, S = 2, T = 17 -- against the gate the GPU tests hold the f16x3 kernels to (envelope: the split arithmetic with the
    device's halves).  Worst error / bound over the marginals (> 1: caught), and the whole-sequence error over the older gradient
    gate max(1e-4, 8 ref) (< 1: that gate lets it through):

                                       per-frame halves toward zero (the device)      both halves to nearest (contraction_errors)
                                       verts   joints  grad    older gradient gate    verts   joints  grad    older gradient gate
      pose blend        without lo hi  2.01    0.593   0.325   0.031                  2.03    0.575   0.328   0.031
      pose blend        without hi lo  4.9     1.08    0.856   0.066                  2.5     0.971   0.962   0.031
      skinning          without lo hi  151     32.3    16.9    1.97                   151     32.3    16.9    1.98
      skinning          without hi lo  335     274     161     9.25                   168     221     190     9.8
      d/d pose feature  without lo hi                  0.124   0.016                                  0.113   0.015
      d/d pose feature  without hi lo                  0.303   0.016                                  0.367   0.016
      d/d A             without lo hi                  3.57    0.205                                  3.57    0.205
      d/d A             without hi lo                  51      2.97                                   7.37    0.407

    Asserted.  Six of the eight mutants leave the gate on at least one marginal, under either rounding of the halves.  The
    acceptance case: "d/d A" without lo hi passes the older gate (0.2 of it) and is 3.6 times over the new one -- a reverse pass
    that had lost a third of its products passed the suite.  "d/d A" without hi lo does the same when the halves are rounded to
    nearest, the arithmetic of contraction_errors; with the device's halves (hi toward zero: the lo half is one-sided and up
    to twice as large) its error is 3e-4 of the largest entry and the older gate caught it as well (2.97), the new one at 51.
    ESCAPES: the two "d/d pose feature" mutants stay inside every marginal (0.11 to 0.37 of the bound).  The pose blend shapes of
    this model reach 1 cm on a skeleton of metres, so what the gradient receives through d/d pose feature is 9e-4 of its
    largest entry and at most 3 % of any joint's, and 2^-11 of that is below the float32 noise of the sum: a gate on
    d L / d theta alone cannot see it at this model.  Recorded in profiles/lbs_gates/ratios.json; nothing is loosened for it."""
    device, nearest = mutant_table(lib, True), mutant_table(lib, False)
    for table in (device, nearest):
        for key, worst in table.items():
            caught = max(v for k, v in worst.items() if k != "old gradient gate") > 1.0
            assert caught == (key not in ESCAPES), (key, worst)
    assert device["d/d A without lo hi"]["old gradient gate"] < 1.0 < device["d/d A without lo hi"]["grad"]
    for key in ("d/d A without lo hi", "d/d A without hi lo"):
        assert nearest[key]["old gradient gate"] < 1.0 < nearest[key]["grad"], (key, nearest[key])
    assert device["d/d A without hi lo"]["grad"] > 1.0 and device["d/d A without hi lo"]["old gradient gate"] > 1.0
    # the unmutated split arithmetic itself is inside every gate
    import lbs_gates
    c = gate_case(lib, 137, 1.0, "ordinary")
    (env_v, env_j), env_g = c["env"]["f16x3"]
    v, j = lbs_gates.forward_ref(c["m"], c["hooks"]["f16x3"])(c["flat"])
    g = lbs_gates.terms_ref(c["m"], 1, COEFS[3], c["hooks"]["f16x3"])(c["th"], c["j0"])
    lbs_gates.gate("split oracle verts", v, c["fwd64"][0], env_v, lbs_gates.VERTICES)
    lbs_gates.gate("split oracle joints", j, c["fwd64"][1], env_j, lbs_gates.JOINTS)
    lbs_gates.gate("split oracle grad", g, c["grad64"], env_g, lbs_gates.GRADIENT)
