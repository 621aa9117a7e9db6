"""Step options of `project` on the device (include/posendf_amd.h pndf_project_ex; DESIGN.md section 1 "The projection step"): every
kernel family that implements the projection loop honours them.

6. replay, bit for bit: `net.project(q, steps=k, **options)` equals k rounds of the engine's own forward + gradient launch with the
   numpy float32 statement sequence of the step (tests/project_options_oracle.py) applied on the host -- the pattern of
   tests/test_reference_callers.py:54-56.  It isolates the step from the network's arithmetic, so it holds at any precision.  The
   plain `project` of the commit before this feature has the same bit-equality against the same replay on every family below
   (measured with this file's replay on that build: profiles/project_options/ab.json "parent_replay"), so no family is gated
   through check 8 instead.
7. the defaults are the plain projection, bit for bit, through the facade and through `pndf_project_ex(opt = NULL)`.
8. ten free-running steps against the vectors the real reference produced with the step restated around it.
9. device == host twin under the same gate.
10. `SamplePose.project(..., renormalize="unit")` returns unit joint quaternions.
"""
import ctypes
import functools

import numpy as np
import pytest

import project_options_oracle as poo
from conftest import outlier_gate, rel_err_rows

pytestmark = pytest.mark.gpu
TOL = 1e-4
SETS = list(poo.OPTION_SETS)

# id -> (kind, act, precision): every kernel family with a projection loop
FAMILIES = {
    "fp32-lrelu": ("amass", "lrelu", "fp32"), "fp32-softplus": ("amass", "softplus", "fp32"),
    "f16x3-lrelu": ("amass", "lrelu", "f16x3"), "f16x3-softplus": ("amass", "softplus", "f16x3"),
    "f16x3-two-term-lrelu": ("half_ckpt", "lrelu", "f16x3"), "f16x3-two-term-softplus": ("half_ckpt", "softplus", "f16x3"),
    "noenc-fp32-softplus": ("noenc", "softplus", "fp32"), "noenc-f16x3-lrelu": ("noenc", "lrelu", "f16x3"),
    "planned-fp32": ("depth", "d4_lrelu", "fp32"), "planned-f16x3": ("depth", "d4_lrelu", "f16x3"),
    "bf16": ("amass", "lrelu", "bf16"), "f16": ("amass", "lrelu", "f16"),
}
KERNELS = {
    "fp32-lrelu": "pndf_fused_relu_kernel", "fp32-softplus": "pndf_fused_softplus_kernel",
    "f16x3-lrelu": "pndf_fused_split_relu_kernel", "f16x3-softplus": "pndf_fused_split_softplus_kernel",
    "f16x3-two-term-lrelu": "pndf_fused_split2_relu_kernel", "f16x3-two-term-softplus": "pndf_fused_split2_softplus_kernel",
    "noenc-fp32-softplus": "pndf_fused_softplus_kernel", "noenc-f16x3-lrelu": "pndf_fused_split_relu_kernel",
    "planned-fp32": "pndf_generic_relu_kernel", "planned-f16x3": "pndf_generic_split_relu_kernel",
    "bf16": "pndf_fused_bf16_relu_kernel", "f16": "pndf_fused_half_relu_kernel",
}


@functools.lru_cache(maxsize=None)
def network(family):
    """(PoseNDF on cuda:0, its engine) of a family, built once per session"""
    import torch
    from posendf_amd import PoseNDF, amass_config, synth
    kind, act, precision = FAMILIES[family]
    if kind == "depth":
        from test_depth import config_for, load_case
        _, hidden, act, enc, sd = load_case(act)
        cfg = config_for(hidden, act, enc, "cuda:0")
    else:
        cfg = amass_config(act, "cuda:0")
        sd = poo.weights()
        if kind == "noenc":
            cfg["model"]["StrEnc"]["use"] = False
            cfg["model"]["DFNet"]["in_dim"] = 84
            sd = synth.make_weights(**poo.REGIME, dims=synth.DFNET_DIMS_NOENC)
        if kind == "half_ckpt":      # a half-precision checkpoint: every lo half of the packed weights is zero -> the two-term kernels
            sd = {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    eng = net._engine_for(torch.device("cuda:0"))
    assert eng.kernel_name() == KERNELS[family], (family, eng.kernel_name())
    return net, eng


@functools.lru_cache(maxsize=None)
def poses(B):
    """the fixture's 52 poses (edge poses included), then seeded signed poses up to B"""
    from posendf_amd import synth
    q = poo.make_inputs()
    if B > len(q):
        q = np.concatenate([q, synth.make_poses(B - len(q), seed=31, signed=True)])
    return np.ascontiguousarray(q[:B])


def forward_grad(eng, q_np):
    """one forward + gradient launch of the engine on host poses -> (d [B], dq [B,21,4]) float32"""
    import torch
    q = torch.from_numpy(np.ascontiguousarray(q_np)).cuda()
    d = torch.empty(len(q_np), device="cuda:0")
    dq = torch.empty_like(q)
    eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), len(q_np), torch.cuda.current_stream().cuda_stream)
    return d.cpu().numpy(), dq.cpu().numpy()


def replay(eng, q_np, steps, **opts):
    """-> {k: (q after k steps, d of step k)}: the engine's forward + gradient, the numpy float32 step on the host"""
    cur, out = np.array(q_np, np.float32).reshape(-1, 21, 4), {}
    for k in range(1, steps + 1):
        d, dq = forward_grad(eng, cur)
        cur = np.ascontiguousarray(poo.step(cur, d, dq, **opts))
        out[k] = (cur.copy(), d.copy())
    return out


def median_tol(eng, q_np):
    """the fourth option set's tolerance for these poses on this network: the median of the initial d, so about half freeze"""
    d0, _ = forward_grad(eng, q_np)
    return float(np.median(d0[np.isfinite(d0)]))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_replay(family, name, B, ks):
    import torch
    net, eng = network(family)
    q_np = poses(B)
    step_size, renorm = poo.OPTION_SETS[name]
    tol = median_tol(eng, q_np) if name == "unit_tol" else 0.0
    want = replay(eng, q_np, max(ks), step_size=step_size, renormalize=renorm, tol=tol)
    q = torch.from_numpy(q_np.copy()).cuda()
    for k in ks:
        got, dl = net.project(q, steps=k, step_size=step_size, renormalize=renorm, tol=tol)
        got, dl = got.cpu().numpy(), dl.cpu().numpy().reshape(-1)
        diff = got.view(np.uint32) != want[k][0].view(np.uint32)
        assert not diff.any(), (family, name, B, k, int(diff.sum()), np.flatnonzero(diff.any(axis=(1, 2)))[:8].tolist())
        assert bits_equal(dl, want[k][1]), (family, name, B, k)
    if name == "unit_tol":      # both populations: poses that never move, poses that do
        frozen = (want[1][0].view(np.uint32) == q_np.view(np.uint32)).all(axis=(1, 2))
        assert 5 <= frozen.sum() <= B - 5, (family, B, int(frozen.sum()))


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_project_with_options_equals_the_replay(family, name):
    """6. B = 52: one ragged workgroup (the fixture's poses, edge poses included); B = 65: a second workgroup with one valid pose"""
    for B in (52, 65):
        check_replay(family, name, B, (1, 3))


@pytest.mark.parametrize("family", ["f16x3-lrelu", "f16x3-softplus", "planned-f16x3"])
def test_replay_on_the_persistent_grid(family):
    """6. B = 16,449 x 2 steps: 258 blocks of 64 -- more than the compute units, so the persistent grids (softplus, runtime-planned)
    walk a second block per workgroup -- with a ragged tail of one pose; the option set that uses every option"""
    check_replay(family, "half_flip", 16449, (2,))
    check_replay(family, "unit_tol", 16449, (2,))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_defaults_are_the_plain_projection(family):
    """7. through the facade, and pndf_project_ex with opt = NULL / the default struct against pndf_project"""
    import torch
    from posendf_amd.engine import ProjectOptions
    net, eng = network(family)
    q = torch.from_numpy(poses(65)).cuda()
    a, da = net.project(q, steps=10)
    b, db = net.project(q, steps=10, step_size=1.0, renormalize=None, tol=0.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(da.view(torch.int32), db.view(torch.int32))
    default = ProjectOptions()
    eng.lib.pndf_default_project_options(ctypes.byref(default))
    st = torch.cuda.current_stream().cuda_stream
    for opt in (None, ctypes.byref(default)):
        out, dl = torch.full_like(q, 7.0), torch.full((65,), 7.0, device="cuda:0")
        assert eng.lib.pndf_project_ex(eng.handle, q.data_ptr(), out.data_ptr(), dl.data_ptr(), 65, 10, opt, st) == 0
        assert torch.equal(out.view(torch.int32), a.view(torch.int32)) and torch.equal(dl.view(torch.int32), da.view(-1).view(torch.int32))
    # a refused struct launches nothing
    default.step_size = 0.0
    out = torch.full_like(q, 7.0)
    assert eng.lib.pndf_project_ex(eng.handle, q.data_ptr(), out.data_ptr(), None, 65, 10, ctypes.byref(default), st) == -1
    assert eng.lib.pndf_last_error(eng.handle) and bool((out == 7.0).all())


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(poo.FIXTURE))


@functools.lru_cache(maxsize=None)
def kink_margin(act, name):
    """shared by the families of one activation: a property of the fp64 trajectory, not of a kernel"""
    fx = fixture()
    return poo.kink_margin_along(fx["q"], poo.weights(), 10, act, **poo.options(name, fx, act))


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("family", ["fp32-lrelu", "fp32-softplus", "f16x3-lrelu", "f16x3-softplus"])
def test_ten_steps_against_the_reference_run(family, name):
    """8. free running, per option set: outlier_gate on rel_err_rows at 1e-4 against the fixture's fp64 result, the fixture's own fp32
    rows as the reference rows (the reference arithmetic's fp32-vs-fp64 error on these inputs after ten steps: median 1.5e-7, max
    5.5e-5, none of the 96 ordinary poses beyond 1e-4 -- the gate's own caps are not what passes this).  lrelu: the gate is given
    the kink margins of the fp64 trajectory, as every free-running test of the plain loop gives it (conftest.traj_margin): with step
    size 0.5 and flips, pose 24 passes within 1.7e-7 (relative) of a LeakyReLU kink, where two correct fp32 evaluations may take
    different branches -- the exact-fp32 kernel does (2.2e-4 on that pose), the reference's own fp32 run happens not to.  Such poses
    stay bounded in number (at most 2 of 52) and below 100 % by the gate."""
    import torch
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    got, _ = net.project(torch.from_numpy(fx["q"]).cuda(), steps=10, **poo.options(name, fx, act))
    truth = fx[f"{act}_{name}_q10_f64"]
    mine, ref = rel_err_rows(got.cpu().numpy(), truth), rel_err_rows(fx[f"{act}_{name}_q10_f32"], truth)
    print(f"[{family} {name}] q10 per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference fp32 median {np.median(ref):.2e} max {ref.max():.2e}")
    outlier_gate(mine, ref, TOL, f"{family} {name} q10", margin=kink_margin(act, name))


@pytest.mark.parametrize("family,name", [("fp32-lrelu", "half_flip"), ("f16x3-softplus", "unit_tol")])
def test_device_equals_the_host_twin(family, name):
    """9. pndf_project_ex against pndf_project_ex_cpu, ten steps, under the gate of check 8 (truth: the fixture's fp64 result)"""
    import torch
    from posendf_amd.engine import CpuEngine
    net, _ = network(family)
    act = FAMILIES[family][1]
    fx = fixture()
    o = poo.options(name, fx, act)
    got, _ = net.project(torch.from_numpy(fx["q"]).cuda(), steps=10, **o)
    host = CpuEngine(act)
    host.load_weights(poo.weights())
    q0 = np.ascontiguousarray(fx["q"])
    twin = np.empty_like(q0)
    host.project(q0.ctypes.data, twin.ctypes.data, None, len(q0), 10, step_size=o["step_size"], renorm=o["renormalize"], tol=o["tol"])
    truth = fx[f"{act}_{name}_q10_f64"]
    outlier_gate(rel_err_rows(got.cpu().numpy(), truth), rel_err_rows(twin, truth), TOL, f"{family} {name} device vs host twin",
                 margin=kink_margin(act, name))


def test_sample_pose_returns_unit_quaternions():
    """10. the caller the option exists for: SamplePose feeds the result to quaternion_to_axis_angle, which assumes unit length"""
    import torch
    from posendf_amd.sample_poses import SamplePose, sample_pose
    net, _ = network("f16x3-lrelu")
    q = torch.from_numpy(poses(65))
    poses_out, dist, _ = SamplePose(net).project(q, steps=10, renormalize="unit")
    norms = poses_out.double().norm(dim=-1)
    assert poses_out.shape == (65, 21, 4) and dist.shape == (65, 1) and float((norms - 1).abs().max()) <= 2 * 2.0 ** -23
    plain, _, _ = SamplePose(net).project(q, steps=10)
    assert float((plain.double().norm(dim=-1) - 1).abs().max()) > 1e-3      # what the bare loop leaves behind
    flipped, _, _ = sample_pose(net, batch_size=8, steps=3, generator=torch.Generator().manual_seed(0), renormalize="unit_flip", step_size=0.5)
    assert bool((flipped[..., 0] >= 0).all()) and float((flipped.double().norm(dim=-1) - 1).abs().max()) <= 2 * 2.0 ** -23
