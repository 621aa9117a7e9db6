"""CPU-side checks of image fitting (posendf_amd/image_fitting.py, csrc/pndf_keypoints.hip): the identity that lets the keypoint
kernel apply SMPL's global orientation after linear-blend skinning, the oracle's robustifier and skip rule, the keypoint
scattering, shape validation and the argument checks of the C ABI.  No compute call: no device is needed."""
import ctypes

import numpy as np
import pytest
import torch

import keypoint_oracle as ko
from oracle import lbs_np


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def test_global_orientation_is_a_rotation_about_the_rest_root_joint():
    """lbs(theta, global_orient = r) == R(r) (x - J0) + J0 with x computed at global_orient = 0 and J0 = joints[:, 0]: the pose
    feature excludes the root and J0 does not depend on theta.  Both sides are fp64; they differ by the 1e-8 inside
    batch_rodrigues only (rounding of unit-size quantities is 1e-16), so the bound is 1e-8 x the model's size (~ 1)."""
    from posendf_amd import synth
    m = synth.make_body_model(V=500, seed=3)
    rng = np.random.default_rng(0)
    th = rng.normal(size=(6, 69)) * 0.3
    r = rng.normal(size=(6, 3)) * 0.8
    r[2] = 0.0
    _, want = lbs_np.lbs(th, m, global_orient=r)
    _, x = lbs_np.lbs(th, m)
    assert np.array_equal(x[:, 0], np.broadcast_to(x[0, 0], (6, 3)))             # J0 is the same for every pose
    cam = ko.default_camera()
    got = ko.posed_points(torch.tensor(x), torch.tensor(r), torch.zeros(6, 3, dtype=torch.float64), cam).numpy()
    err = np.abs(got - want).max()
    print(f"post-rotation against lbs(global_orient=): max joint difference {err:.2e}")
    assert got.shape == (6, 45, 3) and err < 1e-8
    # and the oracle's Rodrigues is lbs_np's
    assert np.abs(ko.rodrigues(torch.tensor(r)).numpy() - lbs_np.batch_rodrigues(r)).max() < 1e-15


def test_gmof_limits_and_plain_squares():
    e = torch.tensor([-300.0, -3.0, 0.0, 0.5, 40.0, 1e4], dtype=torch.float64)
    assert torch.equal(ko.gmof(e, 0.0), e * e)                                   # rho == 0: the reference's formula as written
    big = ko.gmof(e, 1e9)
    assert torch.allclose(big, e * e, rtol=1e-9)                                 # rho -> inf: squares
    g = ko.gmof(e, 100.0)
    assert (g <= e * e).all() and (g < 100.0 ** 2).all() and g[2] == 0           # bounded by rho^2, below the square
    assert abs(float(ko.gmof(torch.tensor(1e9, dtype=torch.float64), 100.0)) - 1e4) < 1e-6      # e -> inf: rho^2
    assert abs(float(ko.gmof(torch.tensor(100.0, dtype=torch.float64), 100.0)) - 5e3) < 1e-9     # e == rho: rho^2 / 2


def test_oracle_skips_by_zeroing():
    """a confidence-0 keypoint that holds NaN contributes exactly 0 to the term and to every gradient"""
    rng = np.random.default_rng(1)
    N, J = 3, 7
    joints, orient = rng.normal(size=(N, J, 3)) * 0.3, rng.normal(size=(N, 3)) * 0.2
    transl = np.array([0.0, 0.0, 10.0]) + rng.normal(size=(N, 3)) * 0.1
    kp = np.concatenate([rng.normal(size=(N, J, 2)) * 100, rng.uniform(0.5, 1, size=(N, J, 1))], -1)
    w = np.ones(J)
    w[4] = 0.0
    clean = kp.copy()
    clean[1, 2] = (5.0, -7.0, 0.0)
    clean[:, 4, :2] = 1.0
    dirty = clean.copy()
    dirty[1, 2, :2] = np.nan
    dirty[:, 4, :2] = np.inf
    for rho in (0.0, 100.0):
        a = ko.terms_grad(joints, orient, transl, clean, ko.default_camera(), w, rho=rho, depth_coef=2.0, depth_target=9.5)
        b = ko.terms_grad(joints, orient, transl, dirty, ko.default_camera(), w, rho=rho, depth_coef=2.0, depth_target=9.5)
        for x, y in zip(a, b):
            assert np.isfinite(y).all() and np.array_equal(x, y)
        assert np.all(b[1][1, 2] == 0) and np.all(b[1][:, 4] == 0) and np.abs(b[1]).max() > 0


def test_joint_map_scattering_and_refusals():
    from posendf_amd.image_fitting import scatter_keypoints
    kp = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3) + 1
    out, mask = scatter_keypoints(kp, [5, -1, 0, 2], 6)
    assert out.shape == (2, 6, 3) and mask.tolist() == [True, False, True, False, False, True]
    assert torch.equal(out[:, 5], kp[:, 0]) and torch.equal(out[:, 0], kp[:, 2]) and torch.equal(out[:, 2], kp[:, 3])
    assert torch.all(out[:, [1, 3, 4]] == 0)                                     # confidence 0 where there is no keypoint
    same, mask = scatter_keypoints(kp, None, 4)
    assert same is kp and mask.all()
    with pytest.raises(ValueError, match="joint_map"):
        scatter_keypoints(kp, None, 6)                                           # the identity needs K == J
    with pytest.raises(ValueError, match="two keypoints"):
        scatter_keypoints(kp, [1, 1, 0, 2], 6)
    with pytest.raises(ValueError):
        scatter_keypoints(kp, [0, 1, 2], 6)                                      # one entry per keypoint
    with pytest.raises(ValueError):
        scatter_keypoints(kp, [0, 1, 2, 6], 6)                                   # a joint the model does not have
    with pytest.raises(ValueError):
        scatter_keypoints(kp, [0.0, 1.0, 2.0, 3.0], 6)


def test_shape_validation_and_exports():
    import posendf_amd
    from posendf_amd.engine import PndfError
    from posendf_amd.image_fitting import ImageFit, PerspectiveCamera, keypoint_term, terms_grad
    assert posendf_amd.ImageFit is ImageFit and posendf_amd.PerspectiveCamera is PerspectiveCamera
    assert posendf_amd.keypoint_term is keypoint_term

    class Body:
        num_joints = 6
    fit = ImageFit(None, Body(), device="cpu")
    assert (fit.out_path, fit.debug, fit.batch_size, fit.gender, fit.use_joints_conf) == ("./experiment_results/image_fitting", False, 1, "male", True)
    for bad in (np.zeros((2, 6, 2)), np.zeros((6, 3)), np.zeros((1, 2, 3, 6, 3))):
        with pytest.raises(ValueError, match="keypoints"):
            fit._prepare(bad, None)
    with pytest.raises(ValueError, match="joint_map"):
        fit._prepare(np.zeros((2, 5, 3)), None)
    kp, w1, w2, t0, depth, S, T, video = fit._prepare(np.zeros((2, 3, 6, 3)), None)
    assert (S, T, video, depth) == (2, 3, True, 10.0) and kp.shape == (6, 6, 3) and t0.tolist() == [[0.0, 0.0, 10.0]] * 6
    assert w2.tolist() == [1.0] * 6 and w1.tolist() == [0, 0, 1, 0, 0, 1]      # the torso joints the model has (9 and 12 are beyond 6)...
    with pytest.raises(ValueError, match="init_translation"):
        fit._prepare(np.zeros((2, 6, 3)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match="depth"):
        fit._prepare(np.zeros((2, 6, 3)), np.array([[0, 0, 9.0], [0, 0, 11.0]]))
    assert ImageFit(None, Body(), device="cpu", depth_weight=0.0)._prepare(np.zeros((2, 6, 3)), np.array([[0, 0, 9.0], [0, 0, 11.0]]))[3].shape == (2, 3)
    with pytest.raises(ValueError, match="rho"):
        ImageFit(None, Body(), rho=-1.0)
    with pytest.raises(ValueError, match="BodyModel"):                            # the fused driver takes the HIP body model only
        fit.optimize(None, np.zeros((2, 6, 3)), fused=True)
    cam = PerspectiveCamera()
    z = torch.zeros(2, 6, 3)
    with pytest.raises(PndfError, match="HIP kernel only"):
        terms_grad(z, torch.zeros(2, 3), torch.zeros(2, 3), z, cam)


def test_camera_buffers_and_cpu_projection():
    from posendf_amd.engine import PndfError
    from posendf_amd.image_fitting import PerspectiveCamera
    cam = PerspectiveCamera(batch_size=2)
    assert cam.focal_length_x.tolist() == [5000.0, 5000.0] and cam.center.shape == (2, 2) and cam.zero.shape == (2,)
    assert cam.rotation.shape == (2, 3, 3) and cam.translation.shape == (2, 3) and cam.rotation.requires_grad
    s = cam.struct()
    assert (s.fx, s.fy, s.cx, s.cy) == (5000.0, 5000.0, 0.0, 0.0) and list(s.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    rng = np.random.default_rng(2)
    Rc = lbs_np.batch_rodrigues(np.array([[0.1, -0.2, 0.3]]))[0]
    cam = PerspectiveCamera(rotation=torch.tensor(Rc), translation=torch.tensor([[0.1, -0.2, 9.0]]), focal_length_x=1200.0,
                            focal_length_y=1100.0, center=torch.tensor([[320.0, 240.0]]))
    pts = rng.normal(size=(3, 5, 3)) * 0.4
    want = ko.project(torch.tensor(pts), torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0.1, -0.2, 9.0]] * 3, dtype=torch.float64),
                      ko.default_camera(1200.0, 1100.0, 320.0, 240.0, Rc)).numpy()
    got = cam(torch.tensor(pts, dtype=torch.float32)).detach().numpy()
    assert got.shape == (3, 5, 2) and np.abs(got - want).max() < 1e-3             # fp32 pixels of size ~ 500: 1e-7 x 500 x a few operations
    mixed = PerspectiveCamera(batch_size=2, focal_length_x=torch.tensor([1000.0, 1200.0]))
    with pytest.raises(PndfError, match="differ"):
        mixed.struct()


def test_guess_translation_similar_triangles():
    from posendf_amd.image_fitting import guess_translation
    j3 = np.zeros((12 + 1, 3))
    j3[9], j3[12], j3[2], j3[5] = (0.2, 0.5, 0), (-0.2, 0.5, 0), (0.1, 0.0, 0), (-0.1, 0.0, 0)
    depth = np.array([8.0, 12.5])
    kp = 5000.0 * j3[None, :, :2] / depth[:, None, None]
    t = guess_translation(np.concatenate([kp, np.ones((2, 13, 1))], -1), j3, 5000.0)
    assert t.shape == (2, 3) and t.dtype == np.float32 and np.all(t[:, :2] == 0) and np.abs(t[:, 2] - depth).max() < 1e-5


def test_cabi_argument_checks(lib):
    """every refusal happens before anything touches a device"""
    from posendf_amd.engine import Camera, KeypointOpts
    cam = Camera(5000.0, 5000.0, 0.0, 0.0, (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1))
    opt = KeypointOpts(1.0, 0.0, 0.0, 0.0, 1, 0)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data                     # a non-null pointer: never dereferenced by a refused call
    C, O = ctypes.byref(cam), ctypes.byref(opt)
    tg, pj = lib.pndf_keypoint_terms_grad, lib.pndf_keypoint_project
    assert tg(None, None, None, None, None, 0, 4, C, O, None, None, None, None, None) == 0            # N == 0: a no-op
    assert pj(None, None, None, 0, 4, C, None, None, None) == 0
    assert tg(p, p, p, p, None, -1, 4, C, O, p, p, p, p, None) == -1
    assert tg(p, p, p, p, None, 2, 0, C, O, p, p, p, p, None) == -1
    assert tg(p, p, p, p, None, 2, 4, None, O, p, p, p, p, None) == -1
    assert tg(p, p, p, p, None, 2, 4, C, None, p, p, p, p, None) == -1
    for k in range(4):                                                            # each required pointer
        args = [p, p, p, p]
        args[k] = None
        assert tg(*args, None, 2, 4, C, O, p, p, p, p, None) == -1
    for rho in (-1.0, float("nan")):
        bad = KeypointOpts(1.0, rho, 0.0, 0.0, 1, 0)
        assert tg(p, p, p, p, None, 2, 4, C, ctypes.byref(bad), p, p, p, p, None) == -1
        assert tg(None, None, None, None, None, 0, 4, C, ctypes.byref(bad), None, None, None, None, None) == -1
    assert pj(p, p, p, -1, 4, C, p, p, None) == -1 and pj(p, p, p, 2, 0, C, p, p, None) == -1 and pj(p, p, p, 2, 4, None, p, p, None) == -1
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert pj(*args, 2, 4, C, p, p, None) == -1
    assert ctypes.sizeof(Camera) == 52 and ctypes.sizeof(KeypointOpts) == 24      # the layouts of include/posendf_amd.h
