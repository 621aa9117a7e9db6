"""Pose completion on the host (include/posendf_amd_completion.h; DESIGN.md section 2 "Pose completion"): the masked step in numpy
(tests/completion_oracle.py) against the vectors the real reference produced with the masked step restated around it
(tests/golden/make_golden_completion.py), the host twin `pndf_complete_cpu` bit for bit against a replay around
`pndf_forward_grad_cpu`, no-mask == `pndf_project_ex_cpu`, the held joints' bits, the validation, the companion header against its
signature table, and the `PoseCompletion` driver.  Runs without a GPU; tests/test_completion_gpu.py holds the device to the same."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
from conftest import outlier_gate, rel_err_rows

TOL = 1e-4
SETS = list(co.OPTION_SETS)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(co.FIXTURE))


@pytest.fixture(scope="module")
def sd():
    return co.weights()


def cpu_engine(act, sd):
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine(act)
    eng.load_weights(sd)
    return eng


def run_twin(eng, q0, observed, steps, o, alias=False):
    """pndf_complete_cpu through CpuEngine.complete -> (poses, d_last); observed: bool [B,21] or None"""
    q0 = np.ascontiguousarray(q0, np.float32)
    B = len(q0)
    out = q0.copy() if alias else np.full_like(q0, 7.0)
    src = out if alias else q0
    dl = np.full(B, 7.0, np.float32)
    words = None if observed is None else co.pack(observed)
    eng.complete(src.ctypes.data, None if words is None else words.ctypes.data, out.ctypes.data, dl.ctypes.data, B, steps,
                 step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
    return out, dl


def cpu_net(act, sd):
    from posendf_amd import PoseNDF, amass_config
    net = PoseNDF(amass_config(act, "cpu"))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    return net


def test_fixture_inputs_are_the_helper_s(fixture):
    co.check_inputs()
    assert np.array_equal(fixture["q"], co.make_inputs()) and np.array_equal(fixture["observed"], co.make_mask())
    assert co.pack(co.make_mask())[co.ALL_FREE] == 0 and co.pack(co.make_mask())[co.ALL_OBSERVED] == (1 << 21) - 1
    for act in co.ACTS:
        assert float(fixture[f"tol_{act}"]) == co.options("unit_tol", act)["tol"]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("act", co.ACTS)
def test_oracle_equals_the_reference_run(fixture, sd, act, name):
    """1. fp64: the helper IS the reference-run masked step to rounding (1e-12 relative); fp32: the gate of
    tests/test_project_options.py check 1 (outlier_gate against the fixture's fp64 result, the fixture's own fp32 rows as the
    reference rows)."""
    o, m = co.options(name, act), fixture["observed"]
    _, tr64, s64 = co.complete(fixture["q"], sd, m, 10, act, dtype=np.float64, snap_at=(1, 10), **o)
    for k in (1, 10):
        truth = fixture[f"{act}_{name}_q{k}_f64"]
        err = float(rel_err_rows(s64[k], truth, floor_frac=0.0).max())
        print(f"[oracle f64 {act} {name}] q{k} worst per-pose relative error {err:.2e}")
        assert err <= 1e-12, (k, err)
    t64 = fixture[f"{act}_{name}_dtrace_f64"]
    assert np.abs(tr64 - t64).max() <= 1e-12 * np.abs(t64).max()
    _, tr32, s32 = co.complete(fixture["q"], sd, m, 10, act, dtype=np.float32, snap_at=(1, 10), **o)
    for k in (1, 10):
        truth = fixture[f"{act}_{name}_q{k}_f64"]
        outlier_gate(rel_err_rows(s32[k], truth), rel_err_rows(fixture[f"{act}_{name}_q{k}_f32"], truth), TOL, f"oracle f32 {act} {name} q{k}")
    # the reference run itself held the observed joints: they are the input in both precisions
    for tag in ("f32", "f64"):
        assert (fixture[f"{act}_{name}_q10_{tag}"][m] == fixture["q"][m]).all()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("act", co.ACTS)
def test_host_twin_equals_the_replay_bit_for_bit(fixture, sd, act, name):
    """2. pndf_complete_cpu == `steps` rounds of pndf_forward_grad_cpu + step_masked in numpy float32, for 1, 3 and 10 steps, and
    with q_out aliasing q_in"""
    eng = cpu_engine(act, sd)
    o, m = co.options(name, act), fixture["observed"]
    q0 = np.ascontiguousarray(fixture["q"]).reshape(-1, 21, 4)
    B = len(q0)
    cur, snaps, d = q0.copy(), {}, np.zeros(B, np.float32)
    for it in range(10):
        dq = np.empty_like(cur)
        eng.forward_grad(cur.ctypes.data, None, d.ctypes.data, dq.ctypes.data, B)
        cur = np.ascontiguousarray(co.step_masked(cur, d, dq, m, **o))
        snaps[it + 1] = (cur.copy(), d.copy())
    for steps in (1, 3, 10):
        want_q, want_d = snaps[steps]
        for alias in (False, True):
            out, dl = run_twin(eng, q0, m, steps, o, alias=alias)
            assert out.tobytes() == want_q.tobytes(), (steps, alias, int((out.view(np.uint32) != want_q.view(np.uint32)).sum()))
            assert dl.tobytes() == want_d.tobytes(), (steps, alias)


@pytest.mark.parametrize("act", co.ACTS)
def test_no_mask_is_the_projection(fixture, sd, act):
    """3. observed = NULL and an all-zero mask: pndf_project_ex_cpu bit for bit, for every option set; steps = 0 as well; the same
    through PoseNDF.complete on a cpu config"""
    eng = cpu_engine(act, sd)
    q0 = np.ascontiguousarray(fixture["q"])
    B = len(q0)
    net = cpu_net(act, sd)
    none = np.zeros((B, 21), bool)
    for name in SETS:
        o = co.options(name, act)
        for steps in (0, 10):
            want, dw = np.empty_like(q0), np.empty(B, np.float32)
            eng.project(q0.ctypes.data, want.ctypes.data, dw.ctypes.data, B, steps, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
            for observed in (None, none):
                out, dl = run_twin(eng, q0, observed, steps, o)
                assert out.tobytes() == want.tobytes() and dl.tobytes() == dw.tobytes(), (name, steps, observed is None)
        for observed in (None, torch.from_numpy(none), torch.zeros(21, dtype=torch.bool)):
            a, da = net.complete(torch.from_numpy(q0), observed, steps=10, **o)
            assert a.shape == (B, 21, 4) and da.shape == (B, 1)
            assert a.numpy().tobytes() == want.tobytes() and da.numpy().tobytes() == dw.tobytes(), name
    # opt = NULL through the C ABI: the defaults
    plain, dp = np.empty_like(q0), np.empty(B, np.float32)
    assert eng.lib.pndf_project_cpu(eng.handle, q0.ctypes.data, plain.ctypes.data, dp.ctypes.data, B, 10) == 0
    out, dl = np.full_like(q0, 7.0), np.full(B, 7.0, np.float32)
    assert eng.lib.pndf_complete_cpu(eng.handle, q0.ctypes.data, None, out.ctypes.data, dl.ctypes.data, B, 10, None) == 0
    assert out.tobytes() == plain.tobytes() and dl.tobytes() == dp.tobytes()
    # a mask reaches the host twin through the facade; return_dist=False returns the poses alone
    m = torch.from_numpy(fixture["observed"])
    b = net.complete(torch.from_numpy(q0), m, steps=10, return_dist=False)
    want, _ = run_twin(eng, q0, fixture["observed"], 10, co.options("plain", act))
    assert b.numpy().tobytes() == want.tobytes() and want.tobytes() != plain.tobytes()
    one = net.complete(torch.from_numpy(q0), m[5], steps=3, return_dist=False)      # one [21] mask for every pose
    want, _ = run_twin(eng, q0, np.tile(fixture["observed"][5], (B, 1)), 3, co.options("plain", act))
    assert one.numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("act", co.ACTS)
def test_observed_joints_keep_their_bits(fixture, sd, act):
    """4. observed joints of the output are the input's bits, whatever they hold; an all-observed pose comes back unchanged with
    d_last = dist_pred(input)"""
    eng = cpu_engine(act, sd)
    m = fixture["observed"].copy()
    q0 = np.ascontiguousarray(fixture["q"]).copy()
    nan_pose, zero_pose = 6, 7
    jn, jz = int(np.flatnonzero(m[nan_pose])[0]), int(np.flatnonzero(m[zero_pose])[0])
    q0[nan_pose, jn] = np.float32(np.nan)
    q0[nan_pose, jn, 2] = np.float32(-0.0)
    q0[zero_pose, jz] = 0.0
    B = len(q0)
    d0 = np.empty(B, np.float32)
    eng.forward(q0.ctypes.data, d0.ctypes.data, B)
    for name in SETS:
        out, dl = run_twin(eng, q0, m, 10, co.options(name, act))
        assert (out.view(np.uint32)[m] == q0.view(np.uint32)[m]).all(), name
        assert out[co.ALL_OBSERVED].tobytes() == q0[co.ALL_OBSERVED].tobytes() and dl[co.ALL_OBSERVED].tobytes() == d0[co.ALL_OBSERVED].tobytes()
        # the NaN joint poisons the rest of ITS pose (it enters the distance) and nothing else; the zero quaternion is harmless
        assert np.isnan(out[nan_pose][~m[nan_pose]]).all() and np.isnan(dl[nan_pose])
        others = np.arange(B) != nan_pose
        assert np.isfinite(out[others]).all() and np.isfinite(dl[others]).all(), name
        moved = (out.view(np.uint32) != q0.view(np.uint32)).any(axis=-1)
        if name != "unit_tol":
            assert moved[others][~m[others]].mean() > 0.9, name      # the free joints took their step (a pose with d = 0 stays)


def test_bad_arguments_are_refused(fixture, sd):
    """5. each bad argument: PNDF_ERR_BAD_ARG, a text, and an untouched output buffer"""
    from posendf_amd.engine import PndfError, ProjectOptions
    eng = cpu_engine("lrelu", sd)
    lib = eng.lib
    q0 = np.ascontiguousarray(fixture["q"])
    words = co.pack(fixture["observed"])
    B = len(q0)

    def c_options(step_size=1.0, renorm=0, tol=0.0, size=None):
        o = ProjectOptions()
        lib.pndf_default_project_options(ctypes.byref(o))
        o.step_size, o.renorm, o.tol = step_size, renorm, tol
        if size is not None:
            o.struct_size = size
        return o

    out, dl = np.full_like(q0, 7.0), np.full(B, 7.0, np.float32)
    good = dict(q=q0.ctypes.data, obs=words.ctypes.data, out=out.ctypes.data, dl=dl.ctypes.data, B=B, steps=2, opt=None)
    bad = {"struct_size 0": dict(opt=c_options(size=0)), "struct_size 12": dict(opt=c_options(size=12)),
           "step_size 0": dict(opt=c_options(step_size=0.0)), "step_size NaN": dict(opt=c_options(step_size=math.nan)),
           "step_size inf": dict(opt=c_options(step_size=math.inf)), "tol < 0": dict(opt=c_options(tol=-1e-3)),
           "tol NaN": dict(opt=c_options(tol=math.nan)), "renorm 3": dict(opt=c_options(renorm=3)),
           "null q_in": dict(q=None), "null q_out": dict(out=None), "misaligned q_in": dict(q=q0.ctypes.data + 2),
           "misaligned q_out": dict(out=out.ctypes.data + 1), "misaligned observed": dict(obs=words.ctypes.data + 2),
           "misaligned d_last": dict(dl=dl.ctypes.data + 2), "negative B": dict(B=-1), "negative steps": dict(steps=-1)}
    for what, change in bad.items():
        a = {**good, **change}
        opt = None if a["opt"] is None else ctypes.byref(a["opt"])
        rc = lib.pndf_complete_cpu(eng.handle, a["q"], a["obs"], a["out"], a["dl"], a["B"], a["steps"], opt)
        assert rc == -1, (what, rc)
        assert lib.pndf_cpu_last_error(eng.handle), what
        assert np.all(out == 7.0) and np.all(dl == 7.0), what
    assert lib.pndf_complete_cpu(None, good["q"], good["obs"], good["out"], good["dl"], B, 2, None) == -1
    # the option texts are pndf_project_ex_cpu's
    o = c_options(step_size=-0.5)
    assert lib.pndf_complete_cpu(eng.handle, good["q"], good["obs"], good["out"], good["dl"], B, 2, ctypes.byref(o)) == -1
    mine = lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_project_ex_cpu(eng.handle, good["q"], good["out"], good["dl"], B, 2, ctypes.byref(o)) == -1
    assert mine == lib.pndf_cpu_last_error(eng.handle) and b"step_size" in mine
    # B = 0 is a no-op (null pointers allowed), d_last may be NULL
    assert lib.pndf_complete_cpu(eng.handle, None, None, None, None, 0, 5, None) == 0
    assert lib.pndf_complete_cpu(eng.handle, good["q"], good["obs"], good["out"], None, B, 1, None) == 0 and not np.all(out == 7.0)
    # the stateless entry points refuse before any device is looked for; the workspace is d + dq on 16-byte boundaries
    assert lib.pndf_complete_workspace_floats(0) == 0 and lib.pndf_complete_workspace_floats(-1) == -1
    for n in (1, 4, 52, 65):
        assert lib.pndf_complete_workspace_floats(n) == -(-n // 4) * 4 + 84 * n
    assert lib.pndf_complete_step(None, None, None, None, 0, None, None) == 0
    assert lib.pndf_complete_step(None, None, None, None, -1, None, None) == -1
    assert lib.pndf_complete_step(None, None, None, None, 4, None, None) == -1
    assert lib.pndf_complete_step(None, None, None, None, 0, ctypes.byref(c_options(renorm=7)), None) == -1
    assert lib.pndf_complete(None, None, None, None, None, 0, 0, None, None, None) == -1
    # the Python wrappers raise
    with pytest.raises(PndfError, match="step_size"):
        eng.complete(good["q"], good["obs"], good["out"], good["dl"], B, 2, step_size=-1.0)
    with pytest.raises(PndfError, match="renormalisation"):
        eng.complete(good["q"], good["obs"], good["out"], good["dl"], B, 2, renorm="sphere")
    net = cpu_net("lrelu", sd)
    with pytest.raises(PndfError, match="shape"):
        net.complete(torch.from_numpy(q0), torch.zeros(3, 21, dtype=torch.bool), steps=1)
    with pytest.raises(PndfError, match="bool"):
        net.complete(torch.from_numpy(q0), torch.zeros(21), steps=1)


def test_a_nan_distance_is_not_frozen(sd):
    """6. `d < tol` is false for a NaN d: the free joints of the pose take the (NaN) update, its observed joints stay"""
    eng = cpu_engine("lrelu", sd)
    q0 = co.make_inputs()[:4].copy()
    m = co.make_mask()[2:6].copy()      # (none of the special rows)
    free = int(np.flatnonzero(~m[2])[0])
    q0[2, free, 1] = np.nan
    out, dl = run_twin(eng, q0, m, 1, dict(step_size=1.0, renormalize=None, tol=math.inf))
    assert np.isnan(dl[2]) and np.isnan(out[2][~m[2]]).all()
    assert out[2][m[2]].tobytes() == q0[2][m[2]].tobytes() and out[[0, 1, 3]].tobytes() == q0[[0, 1, 3]].tobytes()


# ---- 7. the companion header: what is its own (its table, binding, symbols and C99 build: tests/test_cabi.py, for every header alike)
HEADER = "posendf_amd_completion.h"


def test_completion_table_matches_its_header():
    import __graft_entry__ as ge
    ge.build()
    assert list(ch.prototypes(HEADER)) == ["pndf_complete_step", "pndf_complete_workspace_floats", "pndf_complete", "pndf_complete_cpu"]
    assert "pndf_complete_step_kernel" in ch.exported_symbols(ge.LIB)
    public = ch.header_text(HEADER)
    assert "debug" not in public.lower() and '#include "posendf_amd.h"' in public


# ---- 8. the driver
def check_pose_completion(net, device, B=13, K=4, steps=3):
    """shared with tests/test_completion_gpu.py: shapes, held joints identical across hypotheses, NaN in unobserved inputs harmless
    under fill="random", select="best" == a numpy arg-min with NaN skipped, determinism under a seeded generator"""
    from posendf_amd import PoseCompletion
    from posendf_amd.pose_completion import best_hypothesis
    q = torch.from_numpy(co.make_inputs()[:B].copy())
    m = torch.from_numpy(co.make_mask()[:B])
    pc = PoseCompletion(net, device=device)
    gen = lambda: torch.Generator().manual_seed(3)      # noqa: E731
    poses, dist, meshes = pc.complete(q, m, hypotheses=K, generator=gen(), steps=steps, renormalize="unit")
    assert poses.shape == (B, K, 21, 4) and dist.shape == (B, K) and meshes == {} and poses.device.type == torch.device(device).type
    p, mm = poses.cpu().numpy(), m.numpy()
    for k in range(K):
        assert p[:, k][mm].tobytes() == q.numpy()[mm].tobytes()
    free = ~mm
    free[co.ALL_OBSERVED] = False
    assert np.isfinite(p).all() and (p[:, 0][free] != p[:, 1][free]).any(axis=-1).all()      # the hypotheses differ where they may
    assert (dist.cpu().numpy()[co.ALL_OBSERVED] == dist.cpu().numpy()[co.ALL_OBSERVED, 0]).all()
    # NaN in the unobserved inputs: ignored by fill="random" (same generator, same bits), fatal for fill="given"
    holes = q.clone()
    holes[~m] = float("nan")
    again, dist2, best, _ = pc.complete(holes, m, hypotheses=K, generator=gen(), steps=steps, renormalize="unit", select="best")
    assert torch.equal(again.view(torch.int32), poses.view(torch.int32)) and torch.equal(dist2.view(torch.int32), dist.view(torch.int32))
    given, dgiven, bgiven, _ = pc.complete(holes, m, hypotheses=2, fill="given", steps=1, select="best")
    has_hole = ~m.all(dim=1)
    assert bool(torch.isnan(dgiven.cpu()[has_hole]).all()) and bool((bgiven.cpu()[has_hole] == 0).all())
    assert torch.equal(given[:, 0].view(torch.int32), given[:, 1].view(torch.int32))
    # the arg-min: numpy with NaN skipped, ties to the lower index
    d = dist.cpu().numpy()
    assert best.shape == (B,) and np.array_equal(best.cpu().numpy(), np.argmin(d, axis=1)) and best.cpu().numpy()[co.ALL_OBSERVED] == 0
    crafted = torch.tensor([[2.0, math.nan, 1.0, 1.0], [math.nan, math.nan, math.nan, math.nan], [math.nan, 3.0, math.inf, 3.0],
                            [math.nan, math.inf, math.inf, math.nan]])
    assert best_hypothesis(crafted).tolist() == [2, 0, 1, 1]
    valid = [np.flatnonzero(~np.isnan(r)) for r in crafted.numpy()]      # numpy, NaN skipped (np.nanargmin would turn them into inf)
    assert best_hypothesis(crafted).tolist() == [int(v[np.argmin(r[v])]) if len(v) else 0 for v, r in zip(valid, crafted.numpy())]
    # another seed gives other hypotheses; no generator works too
    other, _, _ = pc.complete(q, m, hypotheses=K, generator=torch.Generator().manual_seed(4), steps=steps, renormalize="unit")
    assert not torch.equal(other, poses)
    one, d1, _ = pc.complete(q, m[3], steps=1)
    assert one.shape == (B, 1, 21, 4) and d1.shape == (B, 1)
    with pytest.raises(ValueError):
        pc.complete(q, m, fill="zeros")
    with pytest.raises(ValueError):
        pc.complete(q, m, select="first")
    return pc, q, m


def test_pose_completion_driver_cpu(sd):
    """8. PoseCompletion on a cpu config"""
    import posendf_amd
    assert "PoseCompletion" in posendf_amd.__all__
    check_pose_completion(cpu_net("lrelu", sd), "cpu")
