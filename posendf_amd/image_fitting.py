"""Fitting SMPL poses to 2D keypoints through a perspective camera, with PoseNDF as the pose prior -- the third caller of the
hot path (reference experiments/image_fitting.py; camera experiments/exp_utils.py:68-143).

The reference script does not run as written; what it means is SMPLify-X's two-stage fit with the VPoser
prior replaced by PoseNDF:
    stage 1 (:110-136)  Adam(0.02) over the camera translation and the body's global orientation, pose fixed at zero:
                        camera_data_weight^2 sum E(torso joints 9, 12, 2, 5; rho = 0) + depth_weight^2 sum (t_z - depth)^2
    stage 2 (:139-168)  fresh Adam(0.02) over body pose and global orientation, translation frozen; per sequence
                        1e2 / (1 + it) mean_t d + 10 / (1 + it) sum_t E_t       (weights :36-42; d = the PoseNDF distance)
with E the confidence-weighted, optionally robustified (GMoF) squared reprojection error of csrc/pndf_keypoints.hip.

`ImageFit.optimize(fused=True)` runs both stages with no PyTorch in the loop.  Stage 1 is `pndf_keypoint_terms_grad` and two
`pndf_adam_step` per step (the joints are computed once: the pose is fixed).  Stage 2 is six launches per step and no host
synchronisation: `pndf_forward_grad`, `pndf_lbs_forward` (joints only), `pndf_keypoint_terms_grad`, `pndf_lbs_backward`,
`pndf_denoise_update_w` (axis-angle Jacobian, Adam, next quaternions) and `pndf_adam_step` on the orientation.
`fused=False` takes the same steps through autograd (`keypoint_term`, `BodyModel`, `PoseNDF.forward`, torch.optim.Adam).

The global orientation is SMPL's: a rotation about the rest root joint, applied to the joints by the keypoint kernel
("Image fitting"); `BodyModel` itself stays at zero global orientation.  A joint whose weight or confidence is zero
is skipped, so missing detections may hold NaN.  The betas are fixed at the body model's construction (the reference lists
them among stage 2's variables); the reference's third block (:171-213) is the motion-denoise loop and is served by
`MotionDenoise(schedule="partial_observation")`; rendering and mesh export are out of scope.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .engine import (Camera, DenoiseWeights, KeypointOpts, PndfError, _device_only, aa2quat, adam_step, denoise_update_w,
                     keypoint_project, keypoint_terms_grad, load_library, stream_handle)
from .motion_denoise import axis_angle_to_quaternion

FOCAL_LENGTH = 5000.0                      # image_fitting.py:96, exp_utils.py:70
INIT_JOINTS_IDXS = (9, 12, 2, 5)           # the torso joints of stage 1 (image_fitting.py:30)
TRANS_ESTIMATION = 10.0                    # :32


def _f32(t, device=None):
    """float32, contiguous, (on `device`): what the C ABI's raw pointers need"""
    return t.detach().to(device=device if device is not None else t.device, dtype=torch.float32).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


class PerspectiveCamera(torch.nn.Module):
    """The camera of experiments/exp_utils.py:68-143 (SMPLify-X's): buffers `focal_length_x` / `focal_length_y` [B] (default
    5000), `center` [B,2] (default 0), parameters `rotation` [B,3,3] (default identity) and `translation` [B,3] (default 0).
    `forward(points [N,J,3]) -> [N,J,2]`: u = fx p_x / p_z + cx with p = Rc x + t.

    CUDA points run on `pndf_keypoint_project`.  That call takes ONE set of intrinsics and one rotation (its translation is per
    frame), so the entries of a batched camera must agree there; they are read on the host when the camera is built (and again
    by `refresh()` after the buffers were changed in place).  The kernel call is not recorded by autograd: optimisation goes
    through `keypoint_term`, which is.  CPU points are projected with torch operations."""

    FOCAL_LENGTH = FOCAL_LENGTH

    def __init__(self, rotation=None, translation=None, focal_length_x=None, focal_length_y=None, batch_size=1, center=None,
                 dtype=torch.float32, **kwargs):
        super().__init__()
        self.batch_size, self.dtype = batch_size, dtype

        def focal(f):
            if f is None or isinstance(f, (int, float)):
                return torch.full([batch_size], self.FOCAL_LENGTH if f is None else float(f), dtype=dtype)
            return torch.as_tensor(f, dtype=dtype).reshape(-1)
        self.register_buffer("zero", torch.zeros([batch_size], dtype=dtype))
        self.register_buffer("focal_length_x", focal(focal_length_x))
        self.register_buffer("focal_length_y", focal(focal_length_y))
        self.register_buffer("center", torch.zeros([batch_size, 2], dtype=dtype) if center is None
                             else torch.as_tensor(center, dtype=dtype).reshape(-1, 2))
        if rotation is None:
            rotation = torch.eye(3, dtype=dtype)[None].repeat(batch_size, 1, 1)
        self.rotation = torch.nn.Parameter(torch.as_tensor(rotation, dtype=dtype).reshape(-1, 3, 3).clone(), requires_grad=True)
        if translation is None:
            translation = torch.zeros([batch_size, 3], dtype=dtype)
        self.translation = torch.nn.Parameter(torch.as_tensor(translation, dtype=dtype).reshape(-1, 3).clone(), requires_grad=True)
        self._host = None

    def refresh(self):
        """re-reads intrinsics and rotation to the host (one synchronisation) after they were changed in place"""
        self._host = None
        return self

    def struct(self) -> Camera:
        """the `pndf_camera` of this camera; refuses a batched camera whose entries differ"""
        if self._host is None:
            vals = []
            for name in ("focal_length_x", "focal_length_y"):
                vals.append(getattr(self, name).detach().cpu().double().reshape(-1, 1))
            vals.append(self.center.detach().cpu().double().reshape(-1, 2))
            vals.append(self.rotation.detach().cpu().double().reshape(-1, 9))
            for v in vals:
                if not bool((v == v[:1]).all()):
                    raise PndfError("pndf_keypoint_* take one set of intrinsics and one camera rotation per call: the entries of "
                                    "this batched camera differ (use one camera per group of frames)")
            self._host = (float(vals[0][0, 0]), float(vals[1][0, 0]), float(vals[2][0, 0]), float(vals[2][0, 1]),
                          [float(x) for x in vals[3][0]])
        fx, fy, cx, cy, R = self._host
        return Camera(fx, fy, cx, cy, (ctypes.c_float * 9)(*R))

    def forward(self, points):
        N = points.shape[0]
        t = self.translation
        if t.shape[0] not in (1, N):
            raise ValueError(f"{N} point sets but {t.shape[0]} camera translations")
        if points.device.type != "cuda":
            p = torch.matmul(points, self.rotation.to(points.device).transpose(1, 2)) + t.to(points.device)[:, None]
            f = torch.stack([self.focal_length_x, self.focal_length_y], -1).to(points.device)
            return f[:, None] * p[..., :2] / p[..., 2:3] + self.center.to(points.device)[:, None]
        x = _f32(points)
        zero = torch.zeros(N, 3, device=x.device, dtype=torch.float32)
        return project(x, zero, _f32(t, x.device).expand(N, 3).contiguous(), self)[1]


def project(joints, orient, transl, camera, posed=True, uv=True):
    """`pndf_keypoint_project`: joints [N,J,3] at zero global orientation, orient / transl [N,3] (CUDA, float32, contiguous) ->
    (camera-space points [N,J,3] or None, image points [N,J,2] or None)"""
    _device_only(joints.device, "pndf_keypoint_project")
    N, J = joints.shape[:2]
    po = torch.empty(N, J, 3, device=joints.device, dtype=torch.float32) if posed else None
    out = torch.empty(N, J, 2, device=joints.device, dtype=torch.float32) if uv else None
    keypoint_project(joints.data_ptr(), orient.data_ptr(), transl.data_ptr(), N, J, camera.struct(), _ptr(po), _ptr(out),
                     stream_handle(joints.device))
    return po, out


def terms_grad(joints, orient, transl, keypoints, camera, joint_weight=None, *, data_coef=1.0, rho=0.0, depth_coef=0.0,
               depth_target=0.0, use_conf=True, terms=True, g_joints=True, g_orient=True, g_transl=True, cam=None):
    """`pndf_keypoint_terms_grad` on CUDA float32 contiguous tensors.  Each output argument is True (allocate), a tensor to write
    into, or False / None (not computed).  Returns (terms [N,2], g_joints [N,J,3], g_orient [N,3], g_transl [N,3])."""
    N, J = joints.shape[:2]
    dev = joints.device
    if dev.type != "cuda":
        raise PndfError(f"the keypoint term runs on the HIP kernel only: joints on {dev}")
    if keypoints.shape != (N, J, 3) or orient.shape != (N, 3) or transl.shape != (N, 3):
        raise ValueError(f"joints {tuple(joints.shape)}: keypoints must be [{N},{J},3] and orient / transl [{N},3], got "
                         f"{tuple(keypoints.shape)}, {tuple(orient.shape)}, {tuple(transl.shape)}")
    if joint_weight is not None and joint_weight.shape != (J,):
        raise ValueError(f"joint_weight must be [{J}], got {tuple(joint_weight.shape)}")
    if not rho >= 0:
        raise ValueError(f"rho must be >= 0, got {rho}")
    outs = []
    for want, shape in ((terms, (N, 2)), (g_joints, (N, J, 3)), (g_orient, (N, 3)), (g_transl, (N, 3))):
        if want is True:
            want = torch.empty(shape, device=dev, dtype=torch.float32)
        elif want is False:
            want = None
        outs.append(want)
    cam = cam or camera.struct()
    opt = KeypointOpts(float(data_coef), float(rho), float(depth_coef), float(depth_target), int(bool(use_conf)), 0)
    keypoint_terms_grad(joints.data_ptr(), orient.data_ptr(), transl.data_ptr(), keypoints.data_ptr(), _ptr(joint_weight), N, J, cam, opt,
                        *[_ptr(o) for o in outs], stream_handle(dev))
    return tuple(outs)


class _KeypointTerm(torch.autograd.Function):
    """(E_n, D_n) per frame.  One kernel call in forward computes d E_n / d (joints, orient, transl) as well (a frame's term
    depends on that frame's inputs alone, so backward scales the rows by the upstream gradient); D's gradient is 2 (t_z - target)."""

    @staticmethod
    def forward(ctx, joints, orient, transl, keypoints, camera, joint_weight, rho, use_conf, depth_target):
        dev = joints.device
        j, o, t, k = _f32(joints), _f32(orient, dev), _f32(transl, dev), _f32(keypoints, dev)
        w = None if joint_weight is None else _f32(joint_weight, dev)
        terms, gj, go, gt = terms_grad(j, o, t, k, camera, w, data_coef=1.0, rho=rho, depth_target=depth_target, use_conf=use_conf)
        ctx.save_for_backward(gj, go, gt, t)
        ctx.depth_target = depth_target
        ctx.dtypes = (joints.dtype, orient.dtype, transl.dtype)
        return terms[:, 0].clone(), terms[:, 1].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, gE, gD):
        gj, go, gt, t = ctx.saved_tensors
        gE = gE.float()
        g_t = gt * gE[:, None]
        g_t[:, 2] += gD.float() * 2.0 * (t[:, 2] - ctx.depth_target)
        dj, do, dt = ctx.dtypes
        return (gj * gE[:, None, None]).to(dj), (go * gE[:, None]).to(do), g_t.to(dt), None, None, None, None, None, None


def keypoint_term(joints, orient, transl, keypoints, camera, *, joint_weight=None, rho=0.0, use_conf=True, depth_weight=0.0,
                  depth_target=0.0):
    """The keypoint term on `pndf_keypoint_terms_grad`, differentiable (first order) in `joints` [N,J,3] (at zero global
    orientation, e.g. `BodyModel(...).Jtr`), `orient` [N,3] and `transl` [N,3]; `keypoints` [N,J,3] = (x, y, confidence),
    `camera` a `PerspectiveCamera` (intrinsics and rotation; its own translation is not used), `joint_weight` [J] or None.
    Returns per frame (E [N], D [N]):
        E_n = sum_j (w_j c_nj)^2 [rho(kx - u) + rho(ky - v)]                 (unweighted)
        D_n = depth_weight^2 (t_z - depth_target)^2                          (image_fitting.py:76-80: 0 at the default weight 0)
    A joint with w_j c_nj == 0 is skipped, whatever its keypoint holds."""
    E, D = _KeypointTerm.apply(joints, orient, transl, keypoints, camera, joint_weight, float(rho), bool(use_conf), float(depth_target))
    return E, D * float(depth_weight) ** 2


def scatter_keypoints(keypoints, joint_map, num_joints):
    """keypoints [N,K,3] -> [N,J,3] with keypoint k on model joint joint_map[k] (-1: dropped) and confidence 0 on every joint
    without a keypoint; `joint_map` None is the identity (K == J).  Returns (scattered keypoints, mask [J] of joints that have one)."""
    N, K = keypoints.shape[0], keypoints.shape[1]
    if joint_map is None:
        if K != num_joints:
            raise ValueError(f"{K} keypoints but the body model has {num_joints} joints: pass joint_map (the model joint of every "
                             "keypoint, -1 for none)")
        return keypoints, torch.ones(num_joints, dtype=torch.bool)
    jm = np.asarray(joint_map)
    if jm.shape != (K,) or not np.issubdtype(jm.dtype, np.integer):
        raise ValueError(f"joint_map must be an int array [{K}], got {jm.dtype} {jm.shape}")
    if ((jm < -1) | (jm >= num_joints)).any():
        raise ValueError(f"joint_map entries must be -1 or a joint 0 .. {num_joints - 1}")
    used = jm[jm >= 0]
    if len(np.unique(used)) != len(used):
        raise ValueError("joint_map puts two keypoints on one model joint")
    out = torch.zeros(N, num_joints, 3, dtype=keypoints.dtype, device=keypoints.device)
    src = torch.as_tensor(np.flatnonzero(jm >= 0), device=keypoints.device)
    out[:, torch.as_tensor(used, device=keypoints.device).long()] = keypoints[:, src]
    mask = torch.zeros(num_joints, dtype=torch.bool)
    mask[torch.as_tensor(used).long()] = True
    return out, mask


def guess_translation(keypoints, joints3d, focal, idxs=INIT_JOINTS_IDXS):
    """SMPLify-X's similar-triangles depth guess: t = (0, 0, focal * h3d / h2d) per frame, with h3d / h2d the mean length of the
    torso edges (idxs[0]-idxs[2], idxs[1]-idxs[3]: shoulder to hip on each side) in the model and in the image.  keypoints
    [N,J,>=2], joints3d [N,J,3] or [J,3]; host-side, returns a float32 array [N,3] for `optimize(init_translation=)`."""
    kp = np.asarray(torch.as_tensor(keypoints).detach().cpu(), np.float64)[..., :2]
    j3 = np.asarray(torch.as_tensor(joints3d).detach().cpu(), np.float64)
    j3 = np.broadcast_to(j3, kp.shape[:1] + j3.shape[-2:])
    edges = ((idxs[0], idxs[2]), (idxs[1], idxs[3]))
    h3d = np.mean([np.linalg.norm(j3[:, a] - j3[:, b], axis=-1) for a, b in edges], axis=0)
    h2d = np.mean([np.linalg.norm(kp[:, a] - kp[:, b], axis=-1) for a, b in edges], axis=0)
    t = np.zeros((kp.shape[0], 3), np.float32)
    t[:, 2] = float(focal) * h3d / h2d
    return t


class _FusedFit:
    """The buffers and the two step functions of `ImageFit.optimize(fused=True)`: every step is a fixed sequence of C-ABI calls
    on the current stream, with no host synchronisation and no allocation."""

    def __init__(self, fit, kp, w1, w2, transl, depth, S, T):
        from .body_model import BodyModel
        bm = fit.body_model
        if not isinstance(bm, BodyModel):
            raise ValueError("fused=True needs a posendf_amd.BodyModel (HIP LBS); an arbitrary callable runs through the autograd "
                             "driver (fused=False)")
        dev = kp.device
        if dev.type != "cuda":
            raise ValueError(f"fused=True is the HIP driver: device {dev}; the autograd driver (fused=False) needs CUDA for the "
                             "keypoint term as well")
        if torch.device(dev.type, dev.index or 0) != bm.device:
            raise ValueError(f"fitting on {dev} but the body model lives on {bm.device}: the fused step hands raw pointers to both")
        self.fit, self.bm, self.kp, self.w1, self.w2, self.transl, self.depth, self.S, self.T = fit, bm, kp, w1, w2, transl, depth, S, T
        self.N, self.J = N, J = kp.shape[0], kp.shape[1]
        self.lib = load_library()
        self.eng = fit.pose_prior._engine_for(dev)
        self.st = stream_handle(dev)
        self.cam = fit.camera.struct()
        f32 = dict(device=dev, dtype=torch.float32)
        self.theta0 = torch.zeros(S, T, 69, **f32)                                  # :102
        self.orient = torch.zeros(N, 3, **f32)
        self.g_orient, self.g_transl = torch.empty(N, 3, **f32), torch.empty(N, 3, **f32)
        self.terms = torch.empty(N, 2, **f32)
        self.joints = bm.joints_of(self.theta0)                                     # stage 1: computed once, the pose is fixed
        self.mo, self.vo, self.mt, self.vt = (torch.zeros(N, 3, **f32) for _ in range(4))
        self.bufs = [self.theta0.clone(), torch.empty_like(self.theta0)]
        self.m, self.v = torch.zeros_like(self.theta0), torch.zeros_like(self.theta0)
        self.q, self.dq = torch.empty(N, 21, 4, **f32), torch.empty(N, 21, 4, **f32)
        self.d = torch.empty(N, **f32)
        self.g_joints = torch.empty(N, J, 3, **f32)
        self.g_body = torch.empty_like(self.theta0)
        self.ws = bm._workspace(1, N, dev)

    def _terms_grad(self, w, **kw):
        terms_grad(self.joints, self.orient, self.transl, self.kp, None, w, use_conf=self.fit.use_joints_conf, cam=self.cam, **kw)

    def _adam(self, p, g, m, v, k):
        adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), k, self.fit.LR, stream=self.st, lib=self.lib)

    def data_term(self, w, rho):
        """sum_n E_n of the current state (a 0-d tensor: no synchronisation)"""
        self._terms_grad(w, rho=rho, terms=self.terms, g_joints=False, g_orient=False, g_transl=False)
        return self.terms[:, 0].sum()

    def stage1_step(self, k):
        """three launches: the keypoint and depth terms' gradient, Adam on the translation, Adam on the orientation"""
        fit = self.fit
        self._terms_grad(self.w1, data_coef=fit.camera_data_weight ** 2, rho=0.0, depth_coef=fit.depth_weight ** 2, depth_target=self.depth,
                         terms=False, g_joints=False, g_orient=self.g_orient, g_transl=self.g_transl)
        self._adam(self.transl, self.g_transl, self.mt, self.vt, k)
        self._adam(self.orient, self.g_orient, self.mo, self.vo, k)

    def begin_stage2(self):
        """fresh optimiser state (:144) and the quaternions of the first step"""
        self.mo.zero_()
        self.vo.zero_()
        aa2quat(self.bufs[0].data_ptr(), self.q.data_ptr(), self.N, self.st, self.lib)

    def stage2_step(self, k, it):
        """six launches: distances and their gradient, joints, the keypoint term's gradient, the body model's reverse pass,
        the pose update (axis-angle Jacobian, Adam, next quaternions), Adam on the orientation"""
        bm, st, N = self.bm, self.st, self.N
        pc, dc = self.fit.stage2_coefs(it)
        w = DenoiseWeights(pc, 1, 0.0, 0.0)
        cur, nxt = self.bufs
        self.eng.forward_grad(self.q.data_ptr(), None, self.d.data_ptr(), self.dq.data_ptr(), N, st)
        bm._call("pndf_lbs_forward", cur.data_ptr(), N, None, self.joints.data_ptr(), self.ws, st)
        self._terms_grad(self.w2, data_coef=dc, rho=self.fit.rho, terms=False, g_joints=self.g_joints, g_orient=self.g_orient, g_transl=False)
        bm._call("pndf_lbs_backward", cur.data_ptr(), None, self.g_joints.data_ptr(), N, self.g_body.data_ptr(), self.ws, st)
        denoise_update_w(cur.data_ptr(), nxt.data_ptr(), self.theta0.data_ptr(), self.d.data_ptr(), self.dq.data_ptr(), self.g_body.data_ptr(),
                         self.m.data_ptr(), self.v.data_ptr(), self.q.data_ptr(), self.S, self.T, w, k, self.fit.LR, st, self.lib)
        self._adam(self.orient, self.g_orient, self.mo, self.vo, k)
        self.bufs.reverse()

    def finish(self):
        """joints of the final pose (left in `joints` for data_term) and their projection [N,J,2]"""
        self.bm._call("pndf_lbs_forward", self.bufs[0].data_ptr(), self.N, None, self.joints.data_ptr(), self.ws, self.st)
        return project(self.joints, self.orient, self.transl, self.fit.camera, posed=False)[1]


class ImageFit:
    """Positional arguments are the reference's (experiments/image_fitting.py:22: `ImageFit(posendf, body_model, out_path,
    debug, device, batch_size, gender, use_joints_conf)`); `out_path`, `debug`, `gender` and `batch_size` only feed what is out
    of scope here (mesh export, renderer, the size of the zero betas) and are kept as attributes.  Keyword only: `rho` (the
    robustifier of stage 2; 0 = the reference's plain squares), `depth_weight` and `camera_data_weight` (stage 1),
    `joint_map` (int [K]: the model joint of every keypoint, -1 for none; default: the identity, K == J).  A detector's joint
    table is third-party data and the caller's to supply."""

    LR = 0.02                                                   # :116,144

    def __init__(self, posendf, body_model, out_path="./experiment_results/image_fitting", debug=False, device="cuda:0", batch_size=1,
                 gender="male", use_joints_conf=True, *, rho=0.0, depth_weight=100.0, camera_data_weight=1.0, joint_map=None):
        if not rho >= 0:
            raise ValueError(f"rho must be >= 0, got {rho}")
        self.pose_prior, self.body_model = posendf, body_model
        self.out_path, self.debug, self.device, self.batch_size, self.gender = out_path, debug, device, batch_size, gender
        self.use_joints_conf = use_joints_conf
        self.rho, self.depth_weight, self.camera_data_weight = float(rho), float(depth_weight), float(camera_data_weight)
        self.joint_map = None if joint_map is None else np.asarray(joint_map)
        self.init_joints_idxs = INIT_JOINTS_IDXS
        self.trans_estimation = TRANS_ESTIMATION
        self.camera = PerspectiveCamera(focal_length_x=FOCAL_LENGTH, focal_length_y=FOCAL_LENGTH)      # :96-97
        self.body_pose = self.global_orient = self.translation = self.joints_2d = None
        self.data_terms = None            # sum of E before / after each stage: {'stage1': (before, after), 'stage2': (...)}

    # ---- the schedule ---------------------------------------------------------------------------
    @staticmethod
    def stage2_coefs(it):
        """(prior weight, data weight) of outer iteration `it` (image_fitting.py:36-42: 1e2 / (1 + it), 1e1 / (1 + it))"""
        return 1e2 / (1 + it), 1e1 / (1 + it)

    def _num_joints(self):
        n = getattr(self.body_model, "num_joints", None)
        if n is None:
            raise ValueError("the body model must say how many joints it returns (`num_joints`)")
        return int(n)

    def _prepare(self, keypoints, init_translation):
        kp = torch.as_tensor(keypoints, dtype=torch.float32)
        if kp.dim() not in (3, 4) or kp.shape[-1] != 3:
            raise ValueError(f"keypoints must be [S,K,3] (images) or [S,T,K,3] (videos) with (x, y, confidence), got {tuple(kp.shape)}")
        video = kp.dim() == 4
        S, T = (kp.shape[0], kp.shape[1]) if video else (kp.shape[0], 1)
        N, J = S * T, self._num_joints()
        kp, mask = scatter_keypoints(kp.reshape(N, kp.shape[-2], 3), self.joint_map, J)
        dev = torch.device(self.device)
        kp = kp.to(dev).contiguous()
        w2 = mask.float()
        w1 = torch.zeros(J)
        w1[[i for i in self.init_joints_idxs if i < J]] = 1.0
        w1 = w1 * w2
        if init_translation is None:
            t0 = torch.tensor([0.0, 0.0, self.trans_estimation]).repeat(N, 1)
        else:
            t0 = torch.as_tensor(np.asarray(init_translation), dtype=torch.float32)
            if t0.numel() not in (3, N * 3):
                raise ValueError(f"init_translation must be [3] or [.., 3] for {N} frames, got {tuple(t0.shape)}")
            t0 = t0.reshape(-1, 3).expand(N, 3).clone()
        depth = float(t0[0, 2])
        if self.depth_weight > 0 and not bool((t0[:, 2] == depth).all()):
            raise ValueError("the depth term takes one target depth per call: the z of init_translation differs between frames "
                             "(fit frames of one depth per call, or set depth_weight=0)")
        return kp, w1.to(dev), w2.to(dev), t0.to(dev).contiguous(), depth, S, T, video

    # ---- the fused driver -----------------------------------------------------------------------
    def _optimize_fused(self, kp, w1, w2, transl, depth, S, T, iterations, steps_per_iter):
        run = _FusedFit(self, kp, w1, w2, transl, depth, S, T)
        before1 = run.data_term(w1, 0.0)
        k = 0
        for it in range(iterations):                        # stage 1: translation and orientation on the torso joints (:110-136)
            for _ in range(steps_per_iter):
                k += 1
                run.stage1_step(k)
        after1, before2 = run.data_term(w1, 0.0), run.data_term(w2, self.rho)
        run.begin_stage2()
        k = 0
        for it in range(iterations):                        # stage 2: body pose and orientation on all joints (:139-168)
            for _ in range(steps_per_iter):
                k += 1
                run.stage2_step(k, it)
        uv = run.finish()
        return run.bufs[0].reshape(-1, 69), run.orient, run.transl, uv, (before1, after1, before2, run.data_term(w2, self.rho))

    # ---- the autograd driver --------------------------------------------------------------------
    def _joints(self, pose):
        from .body_model import BodyModel
        if isinstance(self.body_model, BodyModel):
            return self.body_model(pose_body=pose).Jtr
        res = self.body_model(pose)
        return res.Jtr if hasattr(res, "Jtr") else res[1]

    def _optimize_autograd(self, kp, w1, w2, transl, depth, S, T, iterations, steps_per_iter):
        dev = kp.device
        N = kp.shape[0]
        cam = self.camera
        pose = torch.zeros(N, 69, device=dev, requires_grad=True)
        orient = torch.zeros(N, 3, device=dev, requires_grad=True)
        transl = transl.clone().requires_grad_(True)
        cw2 = self.camera_data_weight ** 2

        def term(joints, w, rho, depth_weight=0.0):
            return keypoint_term(joints, orient, transl, kp, cam, joint_weight=w, rho=rho, use_conf=self.use_joints_conf,
                                 depth_weight=depth_weight, depth_target=depth)
        with torch.no_grad():
            joints0 = self._joints(pose)
            before1 = term(joints0, w1, 0.0)[0].sum()
        opt = torch.optim.Adam([transl, orient], self.LR, betas=(0.9, 0.999))         # :115-116
        for it in range(iterations):
            for _ in range(steps_per_iter):
                opt.zero_grad()
                E, D = term(joints0, w1, 0.0, self.depth_weight)
                (cw2 * E.sum() + D.sum()).backward()                                   # :129-131
                opt.step()
        with torch.no_grad():
            after1, before2 = term(joints0, w1, 0.0)[0].sum(), term(joints0, w2, self.rho)[0].sum()
        transl.requires_grad_(False)
        opt = torch.optim.Adam([pose, orient], self.LR, betas=(0.9, 0.999))           # :143-144
        for it in range(iterations):
            pc, dc = self.stage2_coefs(it)
            for _ in range(steps_per_iter):
                opt.zero_grad()
                quat = axis_angle_to_quaternion(pose.reshape(N, 23, 3)[:, :21])         # :157
                dist = self.pose_prior(quat, train=False)["dist_pred"].reshape(S, T)
                E, _ = term(self._joints(pose), w2, self.rho)
                (pc * dist.mean(dim=1).sum() + dc * E.sum()).backward()
                opt.step()
        with torch.no_grad():
            joints = _f32(self._joints(pose))
            after2 = term(joints, w2, self.rho)[0].sum()
            uv = project(joints, _f32(orient), _f32(transl), cam, posed=False)[1]
        return pose.detach(), orient.detach(), transl.detach(), uv, (before1, after1, before2, after2)

    def optimize(self, image, keypoints, iterations=10, steps_per_iter=10, *, fused=True, init_translation=None):
        """The reference's entry point (image_fitting.py:94).  `image` is accepted and unused (rendering is out of scope);
        `keypoints` [S,K,3] (S images) or [S,T,K,3] (S videos of T frames, which share the prior's per-sequence mean as in
        `MotionDenoise`), (x, y, confidence) per keypoint.  Starts from the zero pose, zero orientation and the translation
        (0, 0, 10) -- or `init_translation` ([3] or per frame, e.g. `guess_translation`); the reference's zero translation puts the
        body on the camera plane.  Returns {'body_pose' [.., 69], 'global_orient' [.., 3], 'translation' [.., 3], 'joints_2d'
        [.., J, 2]} with the leading shape of `keypoints`; the same values are kept on the instance."""
        kp, w1, w2, t0, depth, S, T, video = self._prepare(keypoints, init_translation)
        run = self._optimize_fused if fused else self._optimize_autograd
        pose, orient, transl, uv, sums = run(kp, w1, w2, t0, depth, S, T, int(iterations), int(steps_per_iter))
        lead = (S, T) if video else (S,)
        self.body_pose, self.global_orient = pose.reshape(*lead, 69), orient.reshape(*lead, 3)
        self.translation, self.joints_2d = transl.reshape(*lead, 3), uv.reshape(*lead, -1, 2)
        b1, a1, b2, a2 = (float(x) for x in torch.stack(sums).cpu())
        self.data_terms = {"stage1": (b1, a1), "stage2": (b2, a2)}
        return {"body_pose": self.body_pose, "global_orient": self.global_orient, "translation": self.translation,
                "joints_2d": self.joints_2d}
