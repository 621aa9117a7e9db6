"""ORACLE (test infrastructure, NOT product code) -- torch restatement of the keypoint term of image fitting and of the two-stage
fitting loop, checker of posendf_amd/csrc/pndf_keypoints.hip and posendf_amd/image_fitting.py.  fp64 by default; `dtype`
= torch.float32 gives the same arithmetic in fp32, which sets the scale of the tests' gates.

Parity status: UNPINNED.  The reference's experiments/image_fitting.py does not run as written and its
camera and robustifier come from SMPLify-X, which is third-party: this restates what the script evidently means (the issue
text of the feature, DESIGN.md "Image fitting").  Built from oracle/lbs_torch.torch_lbs and oracle/posendf_torch.RefNet;
nothing here reads the reference tree.

  R(r)      smplx batch_rodrigues with its 1e-8 (oracle/lbs_np.batch_rodrigues)
  p         Rc (R(r) (x - J0) + J0) + t,  J0 = joints[:, 0] held constant (no gradient through the pivot)
  u, v      fx p_x / p_z + cx,  fy p_y / p_z + cy
  E_n       sum_j (w_j c_nj)^2 [rho(kx - u) + rho(ky - v)],  rho(e) = e^2 or rho^2 e^2 / (e^2 + rho^2)
  D_n       (t_z - depth_target)^2
A joint with w_j c_nj == 0 is skipped BY ZEROING its keypoint before the arithmetic (masking afterwards would leave 0 * NaN in
the gradient).
"""
import numpy as np
import torch

from oracle.lbs_torch import torch_lbs
from oracle.posendf_torch import RefNet

TORSO = (9, 12, 2, 5)


def default_camera(fx=5000.0, fy=5000.0, cx=0.0, cy=0.0, R=None):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, R=np.eye(3) if R is None else np.asarray(R, np.float64))


def rodrigues(r, eps=1e-8):
    angle = torch.sqrt(((r + eps) ** 2).sum(-1, keepdim=True))
    n = r / angle
    s, c = torch.sin(angle)[..., None], torch.cos(angle)[..., None]
    z = torch.zeros_like(n[..., 0])
    K = torch.stack([z, -n[..., 2], n[..., 1], n[..., 2], z, -n[..., 0], -n[..., 1], n[..., 0], z], -1).reshape(r.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=r.dtype) + s * K + (1 - c) * (K @ K)


def posed_points(joints, orient, transl, cam):
    """[N,J,3] camera-space points"""
    J0 = joints[:, :1].detach()
    world = (joints - J0) @ rodrigues(orient).transpose(1, 2) + J0
    return world @ torch.as_tensor(cam["R"], dtype=joints.dtype).T + transl[:, None]


def project(joints, orient, transl, cam):
    p = posed_points(joints, orient, transl, cam)
    return torch.stack([cam["fx"] * p[..., 0] / p[..., 2] + cam["cx"], cam["fy"] * p[..., 1] / p[..., 2] + cam["cy"]], -1)


def gmof(e, rho):
    return e * e if rho == 0 else rho * rho * e * e / (e * e + rho * rho)


def terms(joints, orient, transl, keypoints, cam, joint_weight=None, rho=0.0, use_conf=True, depth_target=0.0):
    """per frame (E [N], D [N])"""
    N, J = joints.shape[:2]
    w = torch.ones(J, dtype=joints.dtype) if joint_weight is None else joint_weight
    wc = w[None] * (keypoints[..., 2] if use_conf else torch.ones_like(keypoints[..., 2]))
    keep = wc != 0
    wc = torch.where(keep, wc, torch.zeros_like(wc))
    kxy = torch.where(keep[..., None], keypoints[..., :2], torch.zeros_like(keypoints[..., :2]))      # zeroed BEFORE the arithmetic
    e = kxy - project(joints, orient, transl, cam)
    E = (wc ** 2 * (gmof(e[..., 0], rho) + gmof(e[..., 1], rho))).sum(1)
    return E, (transl[:, 2] - depth_target) ** 2


def terms_grad(joints, orient, transl, keypoints, cam, joint_weight=None, *, data_coef=1.0, rho=0.0, depth_coef=0.0, depth_target=0.0,
               use_conf=True, dtype=torch.float64):
    """numpy in, numpy (fp64) out: terms [N,2] and d(data_coef sum E + depth_coef sum D) / d(joints, orient, transl), evaluated in
    `dtype`"""
    t = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype)
    j, o, tr = (t(x).requires_grad_(True) for x in (joints, orient, transl))
    E, D = terms(j, o, tr, t(keypoints), cam, t(joint_weight), rho, use_conf, depth_target)
    (data_coef * E.sum() + depth_coef * D.sum()).backward()
    out = [torch.stack([E, D], 1).detach()] + [x.grad if x.grad is not None else torch.zeros_like(x) for x in (j, o, tr)]
    return tuple(x.double().numpy() for x in out)


def axis_angle_to_quaternion(aa):
    """pytorch3d's documented convention (real part first, Taylor series below 1e-6), as posendf_amd.motion_denoise restates it"""
    ang = torch.norm(aa, p=2, dim=-1, keepdim=True)
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48.0, torch.sin(0.5 * ang) / torch.where(small, torch.ones_like(ang), ang))
    return torch.cat([torch.cos(0.5 * ang), aa * k], -1)


def fit(keypoints, model, sd, cam, *, iterations, steps_per_iter, act="lrelu", rho=0.0, use_conf=True, depth_weight=100.0,
        camera_data_weight=1.0, init_translation=(0.0, 0.0, 10.0), joint_mask=None, lr=0.02, dtype=torch.float64):
    """The two-stage loop (module docstring of posendf_amd/image_fitting.py) on keypoints [S,T,J,3].  Returns numpy
    (pose [S,T,69], orient [S,T,3], transl [S,T,3], data sums (before 1, after 1, before 2, after 2))."""
    kp = torch.tensor(np.asarray(keypoints), dtype=dtype)
    S, T, J = kp.shape[:3]
    N = S * T
    kp = kp.reshape(N, J, 3)
    net = RefNet(act).to(dtype)
    net.load_state_dict({k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in sd.items()})
    for p in net.parameters():
        p.requires_grad_(False)
    w2 = torch.ones(J, dtype=dtype) if joint_mask is None else torch.tensor(np.asarray(joint_mask), dtype=dtype)
    w1 = torch.zeros(J, dtype=dtype)
    w1[list(TORSO)] = 1.0
    w1 = w1 * w2
    pose = torch.zeros(N, 69, dtype=dtype, requires_grad=True)
    orient = torch.zeros(N, 3, dtype=dtype, requires_grad=True)
    transl = torch.tensor(np.broadcast_to(np.asarray(init_translation, np.float64), (N, 3)).copy(), dtype=dtype, requires_grad=True)
    depth = float(np.asarray(init_translation, np.float64).reshape(-1, 3)[0, 2])
    lbs_joints = lambda th: torch_lbs(th, model, dtype)[1]
    E_sum = lambda joints, w, r: float(terms(joints, orient, transl, kp, cam, w, r, use_conf)[0].sum())
    with torch.no_grad():
        joints0 = lbs_joints(pose)
        sums = [E_sum(joints0, w1, 0.0)]
    opt = torch.optim.Adam([transl, orient], lr, betas=(0.9, 0.999))
    for it in range(iterations):
        for _ in range(steps_per_iter):
            opt.zero_grad()
            E, D = terms(joints0, orient, transl, kp, cam, w1, 0.0, use_conf, depth)
            (camera_data_weight ** 2 * E.sum() + depth_weight ** 2 * D.sum()).backward()
            opt.step()
    with torch.no_grad():
        sums += [E_sum(joints0, w1, 0.0), E_sum(joints0, w2, rho)]
    transl.requires_grad_(False)
    opt = torch.optim.Adam([pose, orient], lr, betas=(0.9, 0.999))
    for it in range(iterations):
        pc, dc = 1e2 / (1 + it), 1e1 / (1 + it)
        for _ in range(steps_per_iter):
            opt.zero_grad()
            d = net(axis_angle_to_quaternion(pose.reshape(N, 23, 3)[:, :21])).reshape(S, T)
            E, _ = terms(lbs_joints(pose), orient, transl, kp, cam, w2, rho, use_conf)
            (pc * d.mean(1).sum() + dc * E.sum()).backward()
            opt.step()
    with torch.no_grad():
        sums.append(E_sum(lbs_joints(pose), w2, rho))
    out = [x.detach().double().numpy() for x in (pose.reshape(S, T, 69), orient.reshape(S, T, 3), transl.reshape(S, T, 3))]
    return out[0], out[1], out[2], tuple(sums)


def fit_case(S, T, seed=0, V=500, noise=2.0):
    """Inputs of a fit: a 500-vertex synthetic body model (J = 45), the 'live' weights of the prior and keypoints [S,T,45,3] that
    are the projection of a known pose, orientation and translation plus `noise` pixels, confidences in [0.5, 1], and a few
    missing detections (confidence 0, coordinates NaN)."""
    from posendf_amd import synth
    rng = np.random.default_rng(seed)
    m = synth.make_body_model(V=V, seed=3)
    sd = synth.make_weights(0, 2.0, 0.1)
    N = S * T
    th = (np.cumsum(rng.normal(size=(S, T, 69)) * 0.03, axis=1) + rng.normal(size=(S, 1, 69)) * 0.15).reshape(N, 69)
    orient = rng.normal(size=(N, 3)) * 0.15
    transl = np.array([0.0, 0.0, 10.0]) + rng.normal(size=(N, 3)) * np.array([0.2, 0.2, 0.4])
    cam = default_camera()
    with torch.no_grad():
        joints = torch_lbs(torch.tensor(th), m)[1]
        uv = project(joints, torch.tensor(orient), torch.tensor(transl), cam).numpy()
    J = uv.shape[1]
    kp = np.concatenate([uv + rng.normal(size=uv.shape) * noise, rng.uniform(0.5, 1.0, size=(N, J, 1))], -1)
    miss = rng.random((N, J)) < 0.1
    miss[:, list(TORSO)] = False
    kp[miss] = (np.nan, np.nan, 0.0)
    return m, sd, cam, kp.reshape(S, T, J, 3).astype(np.float32), dict(pose=th, orient=orient, transl=transl)
