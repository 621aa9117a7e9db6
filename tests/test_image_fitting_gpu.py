"""GPU tests of image fitting: the keypoint kernels (posendf_amd/csrc/pndf_keypoints.hip, C ABI pndf_keypoint_*) against the
fp64 torch oracle tests/keypoint_oracle.py, their chain with the HIP body model, `keypoint_term` under autograd, and the
fused two-stage driver `ImageFit.optimize` against the oracle's loop.  Parity UNPINNED (the reference script does not run as
written; its camera and robustifier are SMPLify-X's): the oracle restates the mathematics, gates are the project's own --
error against fp64 held to a tolerance and to a multiple of the fp32 oracle's own error."""
import numpy as np
import pytest
import torch

import keypoint_oracle as ko
from oracle import lbs_np
from oracle.lbs_torch import torch_lbs

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _camera(cam):
    from posendf_amd.image_fitting import PerspectiveCamera
    return PerspectiveCamera(rotation=torch.tensor(cam["R"]), focal_length_x=float(cam["fx"]), focal_length_y=float(cam["fy"]),
                             center=torch.tensor([[cam["cx"], cam["cy"]]]))


def _kernel_case(N, J, seed, odd_camera=False):
    """Random joints (no body model): a zero orientation row, a confidence-0 joint, a NaN keypoint at confidence 0, a zero
    joint weight; translations near (0, 0, 10), so every p_z > 0; keypoints = the projection + 60 px of noise (errors on both
    sides of rho = 100).  Everything is rounded to fp32 first: the oracle sees the kernel's inputs."""
    rng = np.random.default_rng(seed)
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    joints = f(rng.normal(size=(N, J, 3)) * 0.4)
    orient = f(rng.normal(size=(N, 3)) * 0.5)
    orient[N // 2] = 0.0
    transl = f(np.array([0.0, 0.0, 10.0]) + rng.normal(size=(N, 3)) * np.array([0.3, 0.3, 0.5]))
    cam = ko.default_camera()
    if odd_camera:
        cam = ko.default_camera(cx=320.0, cy=240.0, R=f(lbs_np.batch_rodrigues(np.array([[0.2, -0.3, 0.25]]))[0]))
    uv = ko.project(torch.tensor(joints), torch.tensor(orient), torch.tensor(transl), cam).numpy()
    kp = np.concatenate([uv + rng.normal(size=uv.shape) * 60.0, rng.uniform(0.3, 1.0, size=(N, J, 1))], -1)
    kp[0, 1, 2] = 0.0                                      # a confidence-0 joint with ordinary coordinates
    kp[N - 1, 5] = (np.nan, np.nan, 0.0)                   # a missing detection
    w = f(rng.uniform(0.5, 1.5, size=J))
    w[3] = 0.0
    return joints, orient, transl, f(kp), w, cam


@pytest.mark.parametrize("rho", [0.0, 100.0])
@pytest.mark.parametrize("N,J", [(1, 27), (5, 27), (67, 45), (2, 69)])
def test_kernel_against_fp64_oracle(N, J, rho):
    """terms, g_joints, g_orient, g_transl: finite and max|a - b| / max|b| <= max(1e-5, 8 x the fp32 oracle's own error).
    A host replay of the kernel's own per-joint and per-frame functions (the same source compiled for the CPU, sums in joint
    order instead of the butterfly) gives 4e-8 .. 2.1e-6 on these eight cases, the fp32 oracle 2e-8 .. 2.1e-6 (largest for
    both: g_joints at N = 67, J = 45, rho = 100).  On an MI355X: not measured yet; the test prints each error next to the
    fp32 oracle's."""
    _need_gpu()
    from posendf_amd.image_fitting import terms_grad
    joints, orient, transl, kp, w, cam = _kernel_case(N, J, seed=100 * N + J, odd_camera=(N == 5))
    kw = dict(data_coef=1.7, rho=rho, depth_coef=3.0, depth_target=9.6)
    want = ko.terms_grad(joints, orient, transl, kp, cam, w, **kw)
    ref32 = ko.terms_grad(joints, orient, transl, kp, cam, w, dtype=torch.float32, **kw)
    got = terms_grad(_cuda(joints), _cuda(orient), _cuda(transl), _cuda(kp), _camera(cam), _cuda(w), **kw)
    for name, g, b, r32 in zip(("terms", "g_joints", "g_orient", "g_transl"), got, want, ref32):
        g = g.cpu().numpy()
        err, ref = _rel(g, b), _rel(r32, b)
        print(f"keypoint kernel N={N} J={J} rho={rho} {name}: err {err:.2e} (fp32 oracle {ref:.2e}) scale {np.abs(b).max():.2e}")
        assert g.shape == b.shape and np.isfinite(g).all(), name
        assert err <= max(1e-5, 8 * ref), (name, err, ref)
    gj = got[1].cpu().numpy()
    assert np.all(gj[0, 1] == 0) and np.all(gj[N - 1, 5] == 0) and np.all(gj[:, 3] == 0)      # skipped joints: exact zeros


def test_kernel_is_deterministic_and_skips_exactly():
    _need_gpu()
    from posendf_amd.image_fitting import terms_grad
    joints, orient, transl, kp, w, cam = _kernel_case(67, 45, seed=7)
    args = [_cuda(x) for x in (joints, orient, transl, kp)]
    camera = _camera(cam)
    kw = dict(data_coef=1.7, rho=100.0, depth_coef=3.0, depth_target=9.6)
    a = terms_grad(*args, camera, _cuda(w), **kw)
    b = terms_grad(*args, camera, _cuda(w), **kw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    kp0 = kp.copy()
    kp0[..., 2] = 0.0                                       # every confidence 0 (coordinates, one of them NaN, stay)
    t, gj, go, gt = (x.cpu().numpy() for x in terms_grad(args[0], args[1], args[2], _cuda(kp0), camera, _cuda(w), **kw))
    assert np.all(t[:, 0] == 0) and np.all(gj == 0) and np.all(go == 0) and np.all(gt[:, :2] == 0)
    dz = transl.astype(np.float32)[:, 2] - np.float32(9.6)
    assert np.array_equal(t[:, 1], dz * dz) and np.array_equal(gt[:, 2], np.float32(3.0) * np.float32(2.0) * dz)      # the depth term alone
    # outputs are optional, and use_conf = 0 reads no confidence
    only = terms_grad(*args, camera, _cuda(w), terms=False, g_joints=False, g_transl=False, **kw)
    assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], a[2])
    ones = kp.copy()
    ones[..., 2] = 1.0
    ones[66, 5, :2] = 0.0
    kp1 = kp.copy()
    kp1[66, 5, :2] = 0.0
    u0 = terms_grad(args[0], args[1], args[2], _cuda(kp1), camera, _cuda(w), use_conf=False, **kw)
    u1 = terms_grad(args[0], args[1], args[2], _cuda(ones), camera, _cuda(w), use_conf=True, **kw)
    for x, y in zip(u0, u1):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def body():
    _need_gpu()
    from posendf_amd import BodyModel, synth
    m = synth.make_body_model(V=500, seed=3)                # 24 joints + 21 picked vertices: J = 45
    bm = BodyModel(m, device="cuda:0")
    assert bm.num_joints == 45
    return m, bm


def _poses(N, seed):
    rng = np.random.default_rng(seed)
    th = (rng.normal(size=(N, 69)) * 0.25).astype(np.float32)
    r = (rng.normal(size=(N, 3)) * 0.6).astype(np.float32)
    r[0] = 0.0
    t = (np.array([0.0, 0.0, 10.0]) + rng.normal(size=(N, 3)) * 0.3).astype(np.float32)
    return th, r, t


@pytest.mark.parametrize("N", [1, 16])
def test_posed_joints_against_lbs_with_global_orient(body, N):
    """pndf_lbs_forward + pndf_keypoint_project(posed) == lbs(theta, global_orient = r) + t; the camera module on CUDA points."""
    from posendf_amd.image_fitting import PerspectiveCamera, project
    m, bm = body
    th, r, t = _poses(N, seed=N)
    joints = bm.joints_of(torch.from_numpy(th))
    posed, uv = project(joints, _cuda(r), _cuda(t), PerspectiveCamera())
    _, J64 = lbs_np.lbs(th, m, global_orient=r)
    want = J64 + t[:, None].astype(np.float64)
    err = _rel(posed.cpu().numpy(), want)
    print(f"posed joints N={N}: err {err:.2e}")
    assert posed.shape == (N, 45, 3) and err < 1e-5
    assert _rel(uv.cpu().numpy(), 5000.0 * want[..., :2] / want[..., 2:]) < 1e-5
    only_uv = project(joints, _cuda(r), _cuda(t), PerspectiveCamera(), posed=False)
    assert only_uv[0] is None and torch.equal(only_uv[1], uv)
    cam = PerspectiveCamera(translation=torch.from_numpy(t[:1]), focal_length_x=1200.0, focal_length_y=1100.0,
                            center=torch.tensor([[320.0, 240.0]])).to("cuda:0")
    pts = torch.from_numpy(want.astype(np.float32)).cuda()
    p = want + t[:1, None].astype(np.float64)
    ref = np.stack([1200.0 * p[..., 0] / p[..., 2] + 320.0, 1100.0 * p[..., 1] / p[..., 2] + 240.0], -1)
    assert _rel(cam(pts).cpu().numpy(), ref) < 1e-5


def _chain_case(m, N, seed):
    th, r, t = _poses(N, seed)
    rng = np.random.default_rng(seed + 1)
    with torch.no_grad():
        uv = ko.project(torch_lbs(torch.tensor(th, dtype=torch.float64), m)[1], torch.tensor(r, dtype=torch.float64),
                        torch.tensor(t, dtype=torch.float64), ko.default_camera()).numpy()
    kp = np.concatenate([uv + rng.normal(size=uv.shape) * 40.0, rng.uniform(0.3, 1.0, size=uv.shape[:2] + (1,))], -1).astype(np.float32)
    kp[0, 7] = (np.nan, np.nan, 0.0)
    return th, r, t, kp


def _oracle_chain(m, th, r, t, kp, rho, dtype):
    x = torch.tensor(th, dtype=dtype, requires_grad=True)
    E, _ = ko.terms(torch_lbs(x, m, dtype)[1], torch.tensor(r, dtype=dtype), torch.tensor(t, dtype=dtype), torch.tensor(kp, dtype=dtype),
                    ko.default_camera(), None, rho)
    E.sum().backward()
    return x.grad.double().numpy()


@pytest.mark.parametrize("rho", [0.0, 100.0])
def test_chain_gradient_through_lbs_backward(body, rho):
    """d(sum E)/d theta = pndf_lbs_backward(g_joints of the keypoint kernel) against autograd through torch_lbs.  The gate is test_fused_terms_gradient's
    (tests/test_lbs_gpu.py): err < max(1e-4, 8 x the fp32 oracle's error).  On an MI355X: not measured yet (printed)."""
    from posendf_amd.image_fitting import PerspectiveCamera, terms_grad
    m, bm = body
    N = 9
    th, r, t, kp = _chain_case(m, N, seed=40)
    theta = _cuda(th)
    joints = bm.joints_of(theta)
    _, gj, _, _ = terms_grad(joints, _cuda(r), _cuda(t), _cuda(kp), PerspectiveCamera(), rho=rho)
    g = torch.empty_like(theta)
    bm._call("pndf_lbs_backward", theta.data_ptr(), None, gj.data_ptr(), N, g.data_ptr(), bm._workspace(1, N, theta.device),
             bm._stream(theta.device))
    g64 = _oracle_chain(m, th, r, t, kp, rho, torch.float64)
    err, ref = _rel(g.cpu().numpy(), g64), _rel(_oracle_chain(m, th, r, t, kp, rho, torch.float32), g64)
    print(f"chain gradient rho={rho}: err {err:.2e} (fp32 oracle {ref:.2e}) |g| {np.abs(g64).max():.2e}")
    assert torch.isfinite(g).all() and err < max(1e-4, 8 * ref)


def test_keypoint_term_autograd_equals_the_kernel(body):
    from posendf_amd import keypoint_term
    from posendf_amd.image_fitting import PerspectiveCamera, terms_grad
    m, bm = body
    N = 9
    th, r, t, kp = _chain_case(m, N, seed=50)
    cam = PerspectiveCamera()
    w = torch.ones(45, device="cuda")
    w[11] = 0.0
    joints = bm.joints_of(_cuda(th))
    for data_coef, depth_w in ((1.0, 0.0), (1.7, 1.5)):
        j, o, tr = (x.clone().requires_grad_(True) for x in (joints, _cuda(r), _cuda(t)))
        E, D = keypoint_term(j, o, tr, _cuda(kp), cam, joint_weight=w, rho=100.0, depth_weight=depth_w, depth_target=9.6)
        (data_coef * E.sum() + D.sum()).backward()
        terms, gj, go, gt = terms_grad(joints, _cuda(r), _cuda(t), _cuda(kp), cam, w, data_coef=data_coef, rho=100.0,
                                       depth_coef=depth_w ** 2, depth_target=9.6)
        assert torch.equal(E, terms[:, 0]) and torch.equal(D, terms[:, 1] * depth_w ** 2)
        for a, b in ((j.grad, gj), (o.grad, go), (tr.grad, gt)):
            if data_coef == 1.0:
                assert torch.equal(a, b)                     # the same launch, unscaled
            else:
                assert _rel(a.cpu().numpy(), b.cpu().numpy().astype(np.float64)) < 1e-5      # scaled after instead of before the sums
    # through the body model: theta.grad is the chain of the test above
    theta = _cuda(th).requires_grad_(True)
    E, _ = keypoint_term(bm(pose_body=theta).Jtr, _cuda(r), _cuda(t), _cuda(kp), cam, rho=100.0)
    E.sum().backward()
    assert _rel(theta.grad.cpu().numpy(), _oracle_chain(m, th, r, t, kp, 100.0, torch.float64)) < 1e-4


_FITS = {}


def _oracle_fit(S, T, rho):
    """the fp64 loop once per (shape, rho): shared by the precisions"""
    key = (S, T, rho)
    if key not in _FITS:
        m, sd, cam, kp, _ = ko.fit_case(S, T, seed=S * 10 + T)
        _FITS[key] = (m, sd, kp, ko.fit(kp, m, sd, cam, iterations=2, steps_per_iter=3, rho=rho))
    return _FITS[key]


def _loop_gate(what, got, ref):
    """tests/test_lbs_gpu.py's loop gate on pose, orientation and translation together"""
    start = [np.zeros_like(ref[0]), np.zeros_like(ref[1]), np.broadcast_to(np.array([0.0, 0.0, 10.0]), ref[2].shape)]
    diff = np.concatenate([np.abs(g.double().cpu().numpy().reshape(r.shape) - r).ravel() for g, r in zip(got, ref)])
    moved = max(np.abs(r - s).max() for r, s in zip(ref, start))
    print(f"{what}: median {np.median(diff):.2e} share > 1e-3 {(diff > 1e-3).mean():.4f} max {diff.max():.2e} moved {moved:.3f}")
    assert np.isfinite(diff).all()
    assert np.median(diff) < 1e-5 and (diff > 1e-3).mean() < 0.01 and diff.max() < 0.5 * moved


@pytest.mark.parametrize("rho", [0.0, 100.0])
@pytest.mark.parametrize("S,T", [(3, 1), (1, 4)])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_fused_fit_matches_oracle_loop(body, precision, S, T, rho):
    """ImageFit.optimize(fused=True), 2 x 3 steps per stage, against the oracle's loop; the autograd driver takes the same steps.
    Inputs: tests/keypoint_oracle.fit_case (the projection of a known pose, orientation and translation + 2 px of noise, 10 %
    missing detections stored as NaN at confidence 0).  On these inputs the oracle loop in fp32 against fp64 (CPU) gives, for
    the four (shape, rho) cases: median 3.3e-9 .. 3.7e-9, share above 1e-3 exactly 0, max 9.1e-7 .. 2.5e-6, moved 0.23 -- a
    margin of more than 2000 x on the median and the whole of the 1 % on the share.  On an MI355X: not measured yet (the gate's figures are printed)."""
    from posendf_amd import ImageFit, PoseNDF, amass_config
    m, bm = body
    m_, sd, kp, ref = _oracle_fit(S, T, rho)
    cfg = amass_config("lrelu", "cuda:0")
    cfg["engine"] = {"precision": precision}
    net = PoseNDF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    fit = ImageFit(net, bm, device="cuda:0", batch_size=S * T, rho=rho)
    keypoints = kp[:, 0] if T == 1 else kp                   # images [S,K,3] / videos [S,T,K,3]
    out = fit.optimize(None, keypoints, iterations=2, steps_per_iter=3)
    lead = (S,) if T == 1 else (S, T)
    assert out["body_pose"].shape == lead + (69,) and out["global_orient"].shape == lead + (3,)
    assert out["translation"].shape == lead + (3,) and out["joints_2d"].shape == lead + (45, 2)
    assert out["body_pose"] is fit.body_pose and out["joints_2d"] is fit.joints_2d
    _loop_gate(f"fused fit {precision} S={S} T={T} rho={rho}", (out["body_pose"], out["global_orient"], out["translation"]), ref[:3])
    for stage, (before, after) in fit.data_terms.items():    # each stage lowers its data term
        assert np.isfinite([before, after]).all() and after < before, (stage, before, after)
    sums = ref[3]
    assert abs(fit.data_terms["stage1"][1] - sums[1]) < 1e-3 * sums[1] and abs(fit.data_terms["stage2"][1] - sums[3]) < 1e-3 * sums[3]
    with torch.no_grad():                                    # joints_2d is the projection of what was returned
        pose, r, t = (torch.tensor(x.reshape(S * T, -1)) for x in ref[:3])
        uv = ko.project(torch_lbs(pose, m)[1], r, t, ko.default_camera()).numpy()
    assert np.abs(out["joints_2d"].double().cpu().numpy().reshape(uv.shape) - uv).max() < 0.05      # pixels; poses agree to ~1e-5 rad
    auto = ImageFit(net, bm, device="cuda:0", batch_size=S * T, rho=rho).optimize(None, keypoints, iterations=2, steps_per_iter=3, fused=False)
    _loop_gate(f"autograd fit {precision} S={S} T={T} rho={rho}", (auto["body_pose"], auto["global_orient"], auto["translation"]), ref[:3])


def test_fit_with_joint_map_and_refusals(body):
    """a detector's 12 keypoints on 12 of the model's joints: the other joints carry confidence 0 and are skipped"""
    from posendf_amd import ImageFit, PoseNDF, amass_config
    m, bm = body
    m_, sd, kp, _ = _oracle_fit(3, 1, 0.0)
    net = PoseNDF(amass_config("lrelu", "cuda:0"))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.eval()
    jm = np.array([9, 12, 2, 5, 1, 4, 7, 16, 18, 20, 30, 44])
    sub = kp[:, 0][:, jm]
    fit = ImageFit(net, bm, device="cuda:0", joint_map=jm)
    out = fit.optimize(None, sub, iterations=1, steps_per_iter=2)
    mask = np.zeros(45)
    mask[jm] = 1.0
    ref = ko.fit(kp, m, sd, ko.default_camera(), iterations=1, steps_per_iter=2, joint_mask=mask)
    _loop_gate("fit with a joint map", (out["body_pose"], out["global_orient"], out["translation"]), ref[:3])
    class Other:                                             # some other body model: the autograd driver's business
        num_joints = 45
    with pytest.raises(ValueError, match="BodyModel"):
        ImageFit(net, Other(), device="cuda:0", joint_map=jm).optimize(None, sub)
    with pytest.raises(ValueError, match="joint_map"):
        ImageFit(net, bm, device="cuda:0").optimize(None, sub)
