"""Fitting poses of any joint tree to 3D keypoints: inverse kinematics under the learned prior -- what `ImageFit` (posendf_amd/image_fit.py)
is for a PoseNDF with an SMPL body model and a camera, for a model that has no body model: a hand, an animal rig, a `SkeletonPoseNDF`.  The
joint tree with its rest offsets is the body model; the detections are 3D points in the roots' frame.  Every step of
`SkeletonPoseNDF.fit_keypoints` descends the distance field and the keypoint energy inside the projection step
(pndf_project_options5, include/posendf_amd.h), so all hypotheses of all targets are ONE engine call per outer iteration.

Inverse kinematics from one start can end in a local minimum (a finger folded the wrong way), so `KeypointFitting.fit` runs several random
starts per target and returns, per target, the hypothesis of the lowest `energy + lam * dist`.

With a `camera` the detections are pixels [N,K,2], and with a `root` the tree is placed in the target's frame by a rotation and a
translation per pose that the steps move as well (pndf_project_options6; DESIGN.md section 2j "Image fitting"): a hand tracker's output.
With `views` the detections are pixels [N,V,K,2] of the same frame in V calibrated cameras (pndf_project_options8; DESIGN.md section 2j
"Several cameras"); `--views FILE.npz` on the command line.  With `views` [N,V,16] the cameras move from frame to frame
(pndf_project_options10; DESIGN.md section 2j "Moving cameras"); arrays with a leading frame dimension in FILE.npz select that form.
With `fit_lengths=True` the segment lengths of the subject are unknowns too: a scale per rest offset and per keypoint offset
(pndf_project_options7; DESIGN.md section 2j "Bone lengths").

`KeypointFitting.fit_clip` is the driver for a video: `fit` per frame, then one tracked call that couples the poses and the roots along
the clip (pndf_project_options9; DESIGN.md section 2j "Root trajectory"); `--clip T` and `--root_smooth` on the command line.

`python -m posendf_amd.keypoint_fitting` reads an .npz of targets and writes the fitted poses.
"""
from __future__ import annotations

import torch

from .sample_poses import SamplePose


def keypoint_energy(pose, targets, parents, rest, conf=None, keypoint_joints=None, keypoint_offsets=None, root=None, camera=None, rho=0.0,
                    bone_scale=None, views=None):
    """1/2 sum_k w_k |C_k(pose, root) - targets_k|^2 per pose [...], with `forward_kinematics` and `camera_project`; a keypoint whose
    confidence is not positive (zero, negative, NaN) takes no part, whatever its target holds.  With a `camera` the targets are pixels and
    the residual e is taken in normalised image coordinates, rho(e) = e^2 or (rho > 0) rho^2 e^2 / (e^2 + rho^2) summed over both axes; a
    keypoint that is not in front of the camera takes no part.  With `views` (`SkeletonPoseNDF.fit_keypoints(views=)`) the targets are
    [...,V,K,2], the confidences [...,V,K] and the sum runs over views and keypoints; `views` [...,V,16] with leading dimensions is a table
    per pose (moving cameras), in which a view whose fx or fy is not positive takes no part for that pose"""
    from .engine import view_table
    from .skeleton import camera_project, forward_kinematics
    C = camera_project(forward_kinematics(pose, parents, rest, keypoint_joints, keypoint_offsets, bone_scale), root)
    if views is not None:
        moving = hasattr(views, "shape") and len(views.shape) > 2
        vt = torch.as_tensor(views if moving else view_table(views), dtype=C.dtype, device=C.device)      # [V,16], or [...,V,16]
        C = (vt[..., 4:13].reshape(vt.shape[:-1] + (1, 3, 3)) @ C.unsqueeze(-3).unsqueeze(-1)).squeeze(-1) + vt[..., 13:16].unsqueeze(-2)      # [...,V,K,3]
        focal = vt[..., 0:2].unsqueeze(-2)
        on_view = ((focal[..., 0] > 0) & (focal[..., 1] > 0)).expand(C.shape[:-1])
        focal = torch.where(on_view.unsqueeze(-1), focal, torch.ones_like(focal))
        front = (C[..., 2] > 0) & on_view
        z = torch.where(front, C[..., 2], torch.ones_like(C[..., 2]))
        e = C[..., :2] / z.unsqueeze(-1) - (targets - vt[..., 2:4].unsqueeze(-2)) / focal
        ee = e * e
        cost = ee if not rho else float(rho) ** 2 * ee / (ee + float(rho) ** 2)
        sq = torch.where(front, cost.sum(-1), torch.zeros_like(z))
    elif camera is None:
        res = C - targets
        sq = (res * res).sum(-1)
    else:
        fx, fy, cx, cy = (float(v) for v in camera)
        front = C[..., 2] > 0
        z = torch.where(front, C[..., 2], torch.ones_like(C[..., 2]))
        e = torch.stack([C[..., 0] / z - (targets[..., 0] - cx) / fx, C[..., 1] / z - (targets[..., 1] - cy) / fy], dim=-1)
        ee = e * e
        cost = ee if not rho else float(rho) ** 2 * ee / (ee + float(rho) ** 2)
        sq = torch.where(front, cost.sum(-1), torch.zeros_like(z))
    if conf is not None:
        on = conf > 0
        sq = torch.where(on, conf * torch.where(on, sq, torch.zeros_like(sq)), torch.zeros_like(sq))
    return 0.5 * (sq.sum((-2, -1)) if views is not None else sq.sum(-1))


def view_tables(K, R, t):
    """The view table [N,V,16] float32 of cameras that move from frame to frame (`SkeletonPoseNDF.fit_keypoints` with a 3-D `views`), from
    arrays with a leading frame dimension: K [N,V,3,3] or [N,V,4] = (fx, fy, cx, cy), R [N,V,3,3] and t [N,V,3], world -> camera"""
    import numpy as np
    K, R, t = (np.asarray(v, dtype=np.float64) for v in (K, R, t))
    if K.ndim == 4 and K.shape[2:] == (3, 3):
        K = np.stack([K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]], axis=-1)
    if K.ndim != 3 or K.shape[2] != 4 or R.shape != K.shape[:2] + (3, 3) or t.shape != K.shape[:2] + (3,):
        raise ValueError(f"moving views are K [N,V,3,3] or [N,V,4], R [N,V,3,3] and t [N,V,3], not {K.shape}, {R.shape}, {t.shape}")
    return np.ascontiguousarray(np.concatenate([K, R.reshape(R.shape[:2] + (9,)), t], axis=-1), dtype=np.float32)


class KeypointFitting(SamplePose):
    """KeypointFitting(posendf, body_model=None, device="cuda:0"): SamplePose's constructor, plus `fit` for a model that has a
    `fit_keypoints` method (a SkeletonPoseNDF of any joint tree)"""

    @torch.no_grad()
    def fit(self, targets, rest, conf=None, keypoint_joints=None, keypoint_offsets=None, hypotheses=8, iterations=3, steps_per_iter=30, weight=0.02,
            lam=1.0, seed=None, *, step_size=1.0, renormalize="unit", tol=0.0, camera=None, root=None, root_weights=(0.0, 0.0), rho=0.0,
            fit_lengths=False, length_weight=0.02, length_prior=0.1, length_range=(0.5, 2.0), views=None):
        """targets: [N,K,3] detections (one set of K keypoints per target pose); rest / keypoint_joints / keypoint_offsets / conf: as
        `SkeletonPoseNDF.fit_keypoints` (conf [K] or [N,K]).  Every target gets `hypotheses` random starts (unit quaternions, seeded by
        `seed`); `iterations` engine calls of `steps_per_iter` steps each run all N * hypotheses poses at once, iteration `it` with the
        keypoint weight `weight` and starting from the result of the one before.  The schedule (3 x 30 steps, a constant weight of 0.02,
        lam 1) is UNTUNED: no trained skeleton model exists to tune it on, and the weight is only known to lower the energy of a
        15-joint hand with rest offsets within [-0.75, 0.75]^3 at every step (with offsets within [-1, 1]^3 one start of 48 already
        oscillates: scale it down by the square of the rig's size, `SkeletonPoseNDF.fit_keypoints`).  Returns (pose [N,J,4], energy [N], dist [N], start_energy [N,hypotheses]): per target the
        hypothesis of the lowest energy + lam * dist, its keypoint energy and distance, and the energies of its random starts.
        `camera` = (fx, fy, cx, cy): targets are [N,K,2] pixels; `root` [7] or [N,7]: the placement of the tree in the target's frame, from
        which EVERY hypothesis of a target starts; `root_weights` = (nu_rot, nu_trans) let the steps move it; `rho`: the robustifier of the
        image residual -- all as `SkeletonPoseNDF.fit_keypoints`.  With a camera or a root the result has a fifth entry, the root [N,7] of
        the chosen hypothesis.  The image term's weights are UNTUNED as well and default to a held root: its residual is in normalised
        image coordinates, smaller than the 3D term's by the depth of the rig, so useful weights are larger.  Tried on a 15-joint hand with
        rest offsets within [-0.75, 0.75]^3 about 6 units in front of the camera, pure inverse kinematics, as (weight; nu_rot, nu_trans):
        (2.0; 0.5, 2.0), (1.0; 0.2, 1.0) and (0.5; 0.1, 0.5) make the energy of 45, 19 and 5 starts of 48 rise at some step; (0.3; 0.05, 0.3)
        and (0.1; 0.02, 0.1) lower it at every step for every start.
        `fit_lengths=True` makes the bone lengths unknowns of the fit: every hypothesis carries its own scales [S] (S = J + K, one per rest
        offset and per keypoint offset, `SkeletonPoseNDF.fit_keypoints(bone_scale=, per_pose_scale=True)`), started at ones, stepped with
        `length_weight` under the prior `length_prior` (sigma - 1)^2 / 2 and clamped to `length_range`; the result gains a last entry, the
        scales [N,S] of the chosen hypothesis.  These defaults (0.02, 0.1, (0.5, 2.0)) are UNTUNED: no trained model of another skeleton
        exists to tune them on.  With a camera and a free root translation the overall scale trades against depth and only the prior holds
        it.
        `views` (a [V,16] array or a sequence of (K, R, t): `SkeletonPoseNDF.fit_keypoints(views=)`): targets are [N,V,K,2] pixels of the
        same frame in V calibrated cameras and conf [K], [V,K] or [N,V,K]; the root places the tree in the world frame.  Not with
        `camera`.  The weights tried for one camera are the only ones known; several views add their gradients, so start lower.
        `views` [N,V,16] (a tensor or array): a table per target, for cameras that move from frame to frame (pndf_project_options10); its
        rows are repeated per hypothesis.  A row whose fx or fy is not positive switches its view off for that target."""
        net = self.pose_prior
        if not hasattr(net, "fit_keypoints"):
            raise TypeError(f"{type(net).__name__} has no fit_keypoints(): fitting to 3D keypoints is SkeletonPoseNDF's; a PoseNDF fits 2D "
                            "keypoints through posendf_amd.image_fit.ImageFit and its body model")
        J, H = net.num_joints, int(hypotheses)
        y = targets.to(self.device).float()
        D = 3 if camera is None and views is None else 2
        if camera is not None and views is not None:
            raise ValueError("camera= is the one camera of a fit and views= the several: give one of them")
        if y.dim() != (3 if views is None else 4) or y.shape[-1] != D:
            raise ValueError(f"targets are [N,K,{D}] (with views [N,V,K,2]), not {tuple(targets.shape)}")
        N, K = y.shape[0], y.shape[-2]
        lead = () if views is None else (y.shape[1],)
        if H < 1:
            raise ValueError("at least one hypothesis per target")
        gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
        start = torch.randn((N, H, J, 4), generator=gen)
        start = (start / start.norm(dim=-1, keepdim=True).clamp_min(1e-12)).to(self.device)
        yy = y[:, None].expand(N, H, *lead, K, D).reshape(N * H, *lead, K, D)
        placed = camera is not None or root is not None or views is not None
        rt = None
        if root is not None:
            rt = torch.as_tensor(root).to(self.device).float().expand(N, 7)[:, None].expand(N, H, 7).reshape(N * H, 7).contiguous()
        if views is not None and hasattr(views, "shape") and len(views.shape) == 3:      # a table per target: one copy per hypothesis
            vm = torch.as_tensor(views).to(self.device).float()
            if vm.shape[0] != N or vm.shape[1] != y.shape[1] or vm.shape[2] != 16:
                raise ValueError(f"views with a table per target are [{N},{y.shape[1]},16], not {list(vm.shape)}")
            views = vm[:, None].expand(N, H, vm.shape[1], 16).reshape(N * H, vm.shape[1], 16).contiguous()
        image = dict(camera=camera, rho=rho, root_weights=tuple(root_weights), **({} if views is None else dict(views=views))) if placed else {}
        c = None
        if conf is not None:
            c = torch.as_tensor(conf).to(self.device).float()
            c = c.expand(N, *lead, K)[:, None].expand(N, H, *lead, K).reshape(N * H, *lead, K).contiguous()
        tables = dict(keypoint_joints=keypoint_joints, keypoint_offsets=keypoint_offsets)
        rest_d = torch.as_tensor(rest).to(self.device).float()
        off_d = None if keypoint_offsets is None else torch.as_tensor(keypoint_offsets).to(self.device).float()

        sg = torch.ones(N * H, J + K, device=self.device) if fit_lengths else None
        lengths = dict(scale_weight=length_weight, scale_prior=length_prior, scale_range=length_range, per_pose_scale=True, return_scale=True) if fit_lengths else {}

        def energy_of(q, r):
            return keypoint_energy(q, yy, net.parents, rest_d, c, keypoint_joints, off_d, r, camera, rho, sg, views)

        cur = start.reshape(N * H, J, 4)
        start_energy = energy_of(cur, rt).reshape(N, H)
        for _ in range(int(iterations)):
            cur = net.fit_keypoints(cur, yy, rest, steps=int(steps_per_iter), weight=weight, conf=c, return_dist=False, step_size=step_size,
                                    renormalize=renormalize, tol=tol, **tables, **image, **(dict(root=rt, return_root=True) if rt is not None else {}),
                                    **(dict(bone_scale=sg, **lengths) if fit_lengths else {}))
            if fit_lengths:
                cur, sg = cur[:-1] if rt is not None else cur[0], cur[-1]
            if rt is not None:
                cur, rt = cur
        energy = energy_of(cur, rt).reshape(N, H)
        dist = net.project(cur, steps=1)[1].reshape(N, H) if N else energy      # dist_pred at `cur`: evaluated before the update
        best = (energy + float(lam) * dist).argmin(dim=1)
        pick = torch.arange(N, device=best.device)
        result = (cur.reshape(N, H, J, 4)[pick, best], energy[pick, best], dist[pick, best], start_energy)
        if placed:
            if rt is None:
                rt = torch.zeros(N * H, 7, device=cur.device)
                rt[:, 0] = 1.0
            result += (rt.reshape(N, H, 7)[pick, best],)
        if fit_lengths:
            result += (sg.reshape(N, H, J + K)[pick, best],)
        return result

    @torch.no_grad()
    def fit_clip(self, targets, rest, frames, conf=None, clip_steps=60, smooth=0.25, root_smooth=(0.0, 0.25), root_anchor=None, root_data=(0.0, 0.0),
                 fit_lengths=False, length_weight=0.02, length_prior=0.1, length_range=(0.5, 2.0), **fit):
        """The driver for a video: targets [P*T,K,2] (or [P*T,K,3], or with `views` [P*T,V,K,2]) are P clips of T = `frames` consecutive
        frames each.  Stage 1 is `fit` per frame -- the random hypotheses and the choice by energy + lam * dist, with `**fit` its
        arguments (camera, root, root_weights, views, weight, hypotheses, ...), without bone lengths.  Stage 2 is ONE tracked call of
        `clip_steps` steps over the chosen poses and roots: the joints coupled along the clip with `smooth`, the end frames free, the
        roots coupled with `root_smooth` = (lambda_rot, lambda_trans) and, with `root_anchor` [P*T,7], drawn towards it with `root_data`
        (pndf_project_options9), and with `fit_lengths` one set of scales per clip (`length_weight`, `length_prior`, `length_range` as in
        `fit`).  The root of stage 2 is the one stage 1 returns: the `root` given, stepped, or with a `camera` or `views` and no `root`
        the identity placement; without any of the three there is no root.  A part of the root is coupled (and drawn towards the anchor)
        only where it moves -- there is a root and its `root_weights` entry is positive; the coupling of a held part is dropped, not
        refused, so with the default `root_weights` = (0, 0) the defaults of this method are a call without a root trajectory.
        Returns (pose [P*T,J,4], energy [P*T] and dist [P*T] of the last step, root [P*T,7]: the identity placement when there is none)
        and with `fit_lengths` the scales [P,S].
        `views` [T,V,16] (one camera path for every clip) or [P*T,V,16] (pndf_project_options10): cameras that move from frame to frame;
        stage 1 gets the table of every frame, stage 2 the table as given.
        The reference implementation has no such driver: it fits single frames.  The schedule (60 steps, smooth 0.25, the translation
        coupled with 0.25, the rotation not) is UNTUNED: no trained skeleton model exists to tune it on."""
        net = self.pose_prior
        T = int(frames)
        y = targets.to(self.device).float()
        if T < 2 or y.shape[0] % T != 0:
            raise ValueError(f"targets are P * T frames with T = frames >= 2, not {y.shape[0]} frames with frames = {frames}")
        views = fit.get("views")
        if views is not None and hasattr(views, "shape") and len(views.shape) == 3 and views.shape[0] == T and y.shape[0] != T:
            per_frame = torch.as_tensor(views).float()      # stage 1 fits single frames: every frame of every clip gets its table
            fit = dict(fit, views=per_frame.repeat(y.shape[0] // T, 1, 1))
        first = self.fit(y, rest, conf=conf, **fit)
        if views is not None:
            fit = dict(fit, views=views)
        pose = first[0]
        placed = fit.get("camera") is not None or fit.get("root") is not None or fit.get("views") is not None
        root = first[4] if placed else None      # (the identity placement when a camera or views came without a root)
        step = {k: fit[k] for k in ("keypoint_joints", "keypoint_offsets", "weight", "step_size", "tol", "camera", "rho", "views", "root_weights") if k in fit}
        moves = [root is not None and float(w) > 0.0 for w in fit.get("root_weights", (0.0, 0.0))]
        coupled = tuple(float(v) if m else 0.0 for v, m in zip(root_smooth, moves))
        drawn = tuple(float(v) if m and root_anchor is not None else 0.0 for v, m in zip(root_data, moves))
        c = None if conf is None else torch.as_tensor(conf).to(self.device).float()
        lengths = dict(scale_weight=length_weight, scale_prior=length_prior, scale_range=length_range) if fit_lengths else {}
        out = net.fit_keypoints(pose, y, rest, steps=int(clip_steps), conf=c, frames=T, smooth=smooth, free_ends=True, renormalize=fit.get("renormalize", "unit"),
                                return_dist=True, return_energy=True, return_root=True, return_scale=bool(fit_lengths), root=root, root_smooth=coupled,
                                root_anchor=root_anchor if any(drawn) else None, root_data=drawn, **step, **lengths)
        return (out[0], out[2], out[1].reshape(-1)) + tuple(out[3:])


def fit_keypoint_file(posendf, keypoint_file, device="cuda:0", key="keypoints", clip=0, **kwargs):
    """The targets of an .npz -- `key` [N,K,3], `rest` [J,3], and, if the file has them, `conf` [K] or [N,K], `keypoint_joints` [K],
    `keypoint_offsets` [K,3], `camera` [4] = (fx, fy, cx, cy) (then `key` is [N,K,2] pixels) and `root` [7] or [N,7] -> what
    KeypointFitting.fit returns for them.  With `views=` among the keyword arguments `key` is [N,V,K,2].  With `clip` = T the targets are
    clips of T frames and the result is KeypointFitting.fit_clip's."""
    import numpy as np
    with np.load(keypoint_file) as f:
        y = torch.from_numpy(np.ascontiguousarray(f[key], dtype=np.float32))
        rest = torch.from_numpy(np.ascontiguousarray(f["rest"], dtype=np.float32))
        opt = {}
        if "conf" in f.files:
            opt["conf"] = torch.from_numpy(np.ascontiguousarray(f["conf"], dtype=np.float32))
        if "keypoint_joints" in f.files:
            opt["keypoint_joints"] = torch.from_numpy(np.ascontiguousarray(f["keypoint_joints"], dtype=np.int32))
        if "keypoint_offsets" in f.files:
            opt["keypoint_offsets"] = torch.from_numpy(np.ascontiguousarray(f["keypoint_offsets"], dtype=np.float32))
        if "camera" in f.files:
            opt["camera"] = tuple(float(v) for v in np.asarray(f["camera"]).reshape(-1))
        if "root" in f.files:
            opt["root"] = torch.from_numpy(np.ascontiguousarray(f["root"], dtype=np.float32))
    driver = KeypointFitting(posendf, body_model=None, device=device)
    if clip:
        return driver.fit_clip(y, rest, int(clip), **opt, **kwargs)
    return driver.fit(y, rest, **opt, **kwargs)


def main(argv=None):
    import argparse

    from .config import load_config
    from .skeleton import SkeletonPoseNDF
    ap = argparse.ArgumentParser(description="Fit poses of any joint tree to 3D or 2D keypoints with a SkeletonPoseNDF (schedule untuned).")
    ap.add_argument("--config", "-c", required=True, help="path to the config file (configs/amass.yaml's keys, model.StrEnc.parent_mapping the tree)")
    ap.add_argument("--ckpt_path", "-ckpt", required=True, help="checkpoint of the trained model (key model_state_dict)")
    ap.add_argument("--keypoint_file", "-kf", required=True, help=".npz with keys keypoints [N,K,3], rest [J,3] and optionally conf, keypoint_joints, keypoint_offsets, camera [4] "
                                                                    "(fx, fy, cx, cy: keypoints are [N,K,2] pixels) and root [7] or [N,7]")
    ap.add_argument("--hypotheses", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--steps_per_iter", type=int, default=30)
    ap.add_argument("--weight", type=float, default=0.02, help="weight of the keypoint term (nu)")
    ap.add_argument("--root_weights", type=float, nargs=2, default=(0.0, 0.0), metavar=("NU_ROT", "NU_TRANS"),
                    help="weights of the root's own step (needs a root in the file); 0 holds that part")
    ap.add_argument("--rho", type=float, default=0.0, help="robustifier of the image residual (needs a camera in the file); 0 = squared error")
    ap.add_argument("--fit-lengths", "--fit_lengths", dest="fit_lengths", action="store_true",
                    help="fit a scale per rest offset and per keypoint offset besides (weights untuned); written to the key scale")
    ap.add_argument("--views", default=None, metavar="FILE.npz",
                    help="calibration of several cameras: arrays K [V,3,3] (or [V,4] = fx, fy, cx, cy), R [V,3,3] and t [V,3], world -> camera; "
                         "keypoints are then [N,V,K,2] pixels (not with a camera in the keypoint file).  Arrays with a leading frame dimension "
                         "-- K [N,V,3,3] (or [N,V,4]), R [N,V,3,3], t [N,V,3] -- are cameras that move from frame to frame; with --clip T, N "
                         "is T (one path for every clip) or the number of frames")
    ap.add_argument("--clip", type=int, default=0, metavar="T",
                    help="the keypoints are clips of T consecutive frames each: after the fit per frame one tracked call couples the poses and the "
                         "roots along every clip (KeypointFitting.fit_clip; schedule untuned)")
    ap.add_argument("--root_smooth", type=float, nargs=2, default=None, metavar=("LAM_ROT", "LAM_TRANS"),
                    help="with --clip: the coupling of a frame's root rotation / translation to its neighbour frames', each in [0, 1] (default: "
                         "fit_clip's); a part is coupled only where its --root_weights entry is positive and there is a root or a camera")
    ap.add_argument("--lam", type=float, default=1.0, help="weight of the distance in the choice between hypotheses")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the fitted poses (key pose), their energies (energy) and distances (dist) to this .npz")
    a = ap.parse_args(argv)
    opt = load_config(a.config)
    net = SkeletonPoseNDF(opt)
    net.load_state_dict(torch.load(a.ckpt_path, map_location="cpu")["model_state_dict"])
    net.eval()
    extra = {}
    if any(a.root_weights):
        extra["root_weights"] = tuple(a.root_weights)
    if a.rho:
        extra["rho"] = a.rho
    if a.fit_lengths:
        extra["fit_lengths"] = True
    if a.views:
        import numpy as np
        with np.load(a.views) as f:
            if f["R"].ndim == 4:      # a leading frame dimension: cameras that move from frame to frame
                extra["views"] = view_tables(f["K"], f["R"], f["t"])
            else:
                extra["views"] = [(f["K"][v], f["R"][v], f["t"][v]) for v in range(f["R"].shape[0])]
    if a.root_smooth is not None and not a.clip:
        ap.error("--root_smooth needs --clip T")
    if a.clip:
        if a.root_smooth is not None:
            extra["root_smooth"] = tuple(a.root_smooth)
        pose, energy, dist, *root = fit_keypoint_file(net, a.keypoint_file, device=opt["train"]["device"], clip=a.clip, hypotheses=a.hypotheses,
                                                      iterations=a.iterations, steps_per_iter=a.steps_per_iter, weight=a.weight, lam=a.lam, seed=a.seed, **extra)
        if energy.numel():
            print(f"median keypoint energy {float(energy.median()):.5f}, mean dist {float(dist.mean()):.4f} over clips of {a.clip} frames")
    else:
        pose, energy, dist, start, *root = fit_keypoint_file(net, a.keypoint_file, device=opt["train"]["device"], hypotheses=a.hypotheses, iterations=a.iterations,
                                                             steps_per_iter=a.steps_per_iter, weight=a.weight, lam=a.lam, seed=a.seed, **extra)
        if energy.numel():
            print(f"median keypoint energy {float(energy.median()):.5f} (random starts: {float(start.median()):.5f}), mean dist {float(dist.mean()):.4f}")
    scale = [root.pop()] if a.fit_lengths else []
    if a.out:
        import numpy as np
        np.savez(a.out, pose=pose.cpu().numpy(), energy=energy.cpu().numpy(), dist=dist.cpu().numpy(), **({"root": root[0].cpu().numpy()} if root else {}),
                 **({"scale": scale[0].cpu().numpy()} if scale else {}))
    return pose, energy


if __name__ == "__main__":
    main()
