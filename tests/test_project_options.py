"""Step options of `project` -- step size, unit-quaternion steps, stop tolerance (include/posendf_amd.h pndf_project_options; DESIGN.md
section 1 "The projection step") -- on the host: the numpy statement of the step (tests/project_options_oracle.py) against the
vectors the real reference produced with the step restated around it (tests/golden/make_golden_project_options.py), the host twin
`pndf_project_ex_cpu` bit for bit against a replay around `pndf_forward_grad_cpu`, the defaults, the validation, and the
properties the options promise.  Runs without a GPU; tests/test_project_options_gpu.py holds the device to the same."""
import ctypes
import math

import numpy as np
import pytest
import torch

import project_options_oracle as poo
from conftest import outlier_gate, rel_err_rows

TOL = 1e-4
SETS = list(poo.OPTION_SETS)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(poo.FIXTURE))


@pytest.fixture(scope="module")
def sd():
    return poo.weights()


def np_opts(name, fixture, act):
    o = poo.options(name, fixture, act)
    return dict(step_size=o["step_size"], renormalize=o["renormalize"], tol=o["tol"])


def cpu_engine(act, sd):
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine(act)
    eng.load_weights(sd)
    return eng


def c_options(lib, step_size=1.0, renorm=0, tol=0.0):
    from posendf_amd.engine import ProjectOptions
    o = ProjectOptions()
    lib.pndf_default_project_options(ctypes.byref(o))
    o.step_size, o.renorm, o.tol = step_size, renorm, tol
    return o


def test_fixture_inputs_are_the_helper_s(fixture):
    assert np.array_equal(fixture["q"], poo.make_inputs()) and len(fixture["q"]) == 2 * poo.NPOSE + poo.N_EDGE == 52
    assert not fixture["q"][poo.ZERO_QUAT].any()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("act", poo.ACTS)
def test_oracle_equals_the_reference_run(fixture, sd, act, name):
    """1. fp64: the helper IS the reference-run step to rounding (1e-12 relative); fp32: within the reference arithmetic's own fp32
    error (outlier_gate against the fixture's fp64 result, the fixture's own fp32 rows as the reference rows)."""
    o = np_opts(name, fixture, act)
    _, tr64, s64 = poo.project(fixture["q"], sd, 10, act, dtype=np.float64, snap_at=(1, 10), **o)
    for k in (1, 10):
        truth = fixture[f"{act}_{name}_q{k}_f64"]
        err = float(rel_err_rows(s64[k], truth, floor_frac=0.0).max())
        print(f"[oracle f64 {act} {name}] q{k} worst per-pose relative error {err:.2e}")
        assert err <= 1e-12, (k, err)
    t64 = fixture[f"{act}_{name}_dtrace_f64"]
    assert np.abs(tr64 - t64).max() <= 1e-12 * np.abs(t64).max()
    _, tr32, s32 = poo.project(fixture["q"], sd, 10, act, dtype=np.float32, snap_at=(1, 10), **o)
    for k in (1, 10):
        truth = fixture[f"{act}_{name}_q{k}_f64"]
        outlier_gate(rel_err_rows(s32[k], truth), rel_err_rows(fixture[f"{act}_{name}_q{k}_f32"], truth), TOL, f"oracle f32 {act} {name} q{k}")


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("act", poo.ACTS)
def test_host_twin_equals_the_replay_bit_for_bit(fixture, sd, act, name):
    """2. pndf_project_ex_cpu == `steps` rounds of pndf_forward_grad_cpu + the numpy float32 statement sequence, for 1, 3, 10 steps"""
    eng = cpu_engine(act, sd)
    o = poo.options(name, fixture, act)
    q0 = np.ascontiguousarray(fixture["q"]).reshape(-1, 21, 4)
    B = len(q0)
    cur, snaps, d = q0.copy(), {}, np.zeros(B, np.float32)
    for it in range(10):
        dq = np.empty_like(cur)
        eng.forward_grad(cur.ctypes.data, None, d.ctypes.data, dq.ctypes.data, B)
        cur = np.ascontiguousarray(poo.step(cur, d, dq, **np_opts(name, fixture, act)))
        snaps[it + 1] = (cur.copy(), d.copy())
    for steps in (1, 3, 10):
        out, dl = np.empty_like(q0), np.empty(B, np.float32)
        eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, steps, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
        want_q, want_d = snaps[steps]
        assert out.tobytes() == want_q.tobytes(), (steps, int((out.view(np.uint32) != want_q.view(np.uint32)).sum()))
        assert dl.tobytes() == want_d.tobytes()


@pytest.mark.parametrize("act", poo.ACTS)
def test_defaults_are_the_plain_projection(fixture, sd, act):
    """3. opt = NULL and the default struct: pndf_project_cpu bit for bit; the same through PoseNDF.project on a cpu config"""
    from posendf_amd import PoseNDF, amass_config
    eng = cpu_engine(act, sd)
    lib = eng.lib
    q0 = np.ascontiguousarray(fixture["q"])
    B = len(q0)
    plain, dp = np.empty_like(q0), np.empty(B, np.float32)
    assert lib.pndf_project_cpu(eng.handle, q0.ctypes.data, plain.ctypes.data, dp.ctypes.data, B, 10) == 0
    default = c_options(lib)
    assert (default.struct_size, default.step_size, default.renorm, default.tol) == (ctypes.sizeof(default), 1.0, 0, 0.0) and ctypes.sizeof(default) == 16
    for opt in (None, ctypes.byref(default)):
        out, dl = np.full_like(q0, 7.0), np.full(B, 7.0, np.float32)
        assert lib.pndf_project_ex_cpu(eng.handle, q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 10, opt) == 0
        assert out.tobytes() == plain.tobytes() and dl.tobytes() == dp.tobytes()
    net = PoseNDF(amass_config(act, "cpu"))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    a, da = net.project(torch.from_numpy(q0), steps=10)
    b, db = net.project(torch.from_numpy(q0), steps=10, step_size=1.0, renormalize=None, tol=0.0)
    assert torch.equal(a, b) and torch.equal(da, db) and a.numpy().tobytes() == plain.tobytes()
    # an option that is set reaches the host twin through the facade
    c, _ = net.project(torch.from_numpy(q0), steps=10, renormalize="unit")
    assert c.numpy().tobytes() != plain.tobytes()


def test_bad_options_are_refused(fixture, sd):
    """4. each bad field: PNDF_ERR_BAD_ARG, a text, and an untouched output buffer"""
    from posendf_amd.engine import PndfError
    eng = cpu_engine("lrelu", sd)
    lib = eng.lib
    q0 = np.ascontiguousarray(fixture["q"])
    B = len(q0)
    bad = {"struct_size 0 (a zero-initialised struct)": dict(size=0), "struct_size 12": dict(size=12),
           "step_size 0": dict(step_size=0.0), "step_size < 0": dict(step_size=-0.5), "step_size inf": dict(step_size=math.inf),
           "step_size NaN": dict(step_size=math.nan), "tol < 0": dict(tol=-1e-3), "tol NaN": dict(tol=math.nan),
           "renorm 3": dict(renorm=3), "renorm -1": dict(renorm=-1)}
    for what, f in bad.items():
        o = c_options(lib, f.get("step_size", 1.0), f.get("renorm", 0), f.get("tol", 0.0))
        if "size" in f:
            o.struct_size = f["size"]
        out, dl = np.full_like(q0, 7.0), np.full(B, 7.0, np.float32)
        rc = lib.pndf_project_ex_cpu(eng.handle, q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 2, ctypes.byref(o))
        assert rc == -1, (what, rc)
        assert lib.pndf_cpu_last_error(eng.handle), what
        assert np.all(out == 7.0) and np.all(dl == 7.0), what
    out, dl = np.full_like(q0, 7.0), np.full(B, 7.0, np.float32)
    with pytest.raises(PndfError, match="step_size"):
        eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 2, step_size=-1.0)
    with pytest.raises(PndfError, match="renormalisation"):
        eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 2, renorm="sphere")
    assert np.all(out == 7.0)
    # tol = +inf is a value like any other: every pose with a distance below it is frozen
    eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 2, tol=math.inf)
    assert out.tobytes() == q0.tobytes()


def joint_norms(q):
    return np.sqrt((np.asarray(q, np.float64) ** 2).sum(axis=-1))


@pytest.mark.parametrize("act", poo.ACTS)
def test_properties_the_options_promise(fixture, sd, act):
    """5. on the host twin's ten-step results for the fixture's poses (the reference-run fixture is held to the same)"""
    eng = cpu_engine(act, sd)
    q0 = np.ascontiguousarray(fixture["q"]).reshape(-1, 21, 4)
    B = len(q0)
    ulp = 2.0 ** -23

    def run(name):
        o = poo.options(name, fixture, act)
        out, dl = np.empty_like(q0), np.empty(B, np.float32)
        eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, B, 10, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
        return out, dl, o

    for source in ("host twin", "fixture"):
        # unit: every joint of every pose has moved and is a unit quaternion; the zero quaternion produced no NaN
        out = run("unit")[0] if source == "host twin" else fixture[f"{act}_unit_q10_f32"]
        assert np.isfinite(out).all(), source
        assert np.abs(joint_norms(out) - 1.0).max() <= 2 * ulp, (source, float(np.abs(joint_norms(out) - 1.0).max()))
        # unit_flip: unit, and w >= 0 everywhere -- and the flip fired: without it some of these joints have w < 0
        out = run("half_flip")[0] if source == "host twin" else fixture[f"{act}_half_flip_q10_f32"]
        assert np.abs(joint_norms(out) - 1.0).max() <= 2 * ulp and (out[..., 0] >= 0).all(), source
        unflipped, _, _ = poo.project(q0, sd, 1, act, step_size=0.5, renormalize="unit")
        assert (unflipped[..., 0] < 0).sum() > 100      # the signed poses: about half of their joints
        # tol: the poses that start below it are their input bit for bit, keep their d at every step (so d_last < tol), and are
        # exactly the unchanged ones; a pose that starts above it moves, and may come to rest later: at any step the poses it
        # leaves unchanged are exactly those with d < tol (checked on the last step of the host twin, whose step 9 we can run)
        o = poo.options("unit_tol", fixture, act)
        tol = np.float32(o["tol"])
        if source == "host twin":
            out, dl, _ = run("unit_tol")
            d0 = np.empty(B, np.float32)
            eng.forward(q0.ctypes.data, d0.ctypes.data, B)
            prev = np.empty_like(q0)
            eng.project(q0.ctypes.data, prev.ctypes.data, None, B, 9, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
            rested = (out.view(np.uint32) == prev.view(np.uint32)).all(axis=(1, 2))
            assert np.array_equal(rested, dl < tol), np.flatnonzero(rested != (dl < tol)).tolist()
        else:
            trace = fixture[f"{act}_unit_tol_dtrace_f32"]
            out, dl, d0 = fixture[f"{act}_unit_tol_q10_f32"], trace[-1], trace[0]
            assert (trace[:, d0 < tol].view(np.uint32) == d0[d0 < tol].view(np.uint32)).all()
        same = (out.view(np.uint32) == q0.view(np.uint32)).all(axis=(1, 2))
        frozen = d0 < tol
        assert np.array_equal(same, frozen), (source, np.flatnonzero(same != frozen).tolist())
        assert (dl[frozen].view(np.uint32) == d0[frozen].view(np.uint32)).all() and (dl[frozen] < tol).all()
        assert 10 <= frozen.sum() <= B - 10, (source, int(frozen.sum()))
        assert np.abs(joint_norms(out[~frozen]) - 1.0).max() <= 2 * ulp      # the moved ones were normalised


def test_a_nan_distance_is_not_frozen(sd):
    """`d < tol` is false for a NaN d: the pose takes the (NaN) update like every other pose, it is not passed through"""
    eng = cpu_engine("lrelu", sd)
    q0 = poo.make_inputs()[:4].copy()
    q0[2, 3, 1] = np.nan
    out, dl = np.empty_like(q0), np.empty(4, np.float32)
    eng.project(q0.ctypes.data, out.ctypes.data, dl.ctypes.data, 4, 1, tol=math.inf)
    assert np.isnan(dl[2]) and np.isnan(out[2]).all() and out[[0, 1, 3]].tobytes() == q0[[0, 1, 3]].tobytes()
