"""`SkeletonPoseNDF` -- the Pose-NDF model for any joint tree.

The model has nothing SMPL-specific in it: a chain of bone MLPs along a parent table in front of an MLP (reference
model/network/net_modules.py:140-170, :46-72).  `PoseNDF` (posendf_amd.facade) runs the 21-joint table of
get_parent_mapping('smpl') on the persistent kernels; this class takes the table from the config key
`model.StrEnc.parent_mapping` -- the key of the reference's own StructureEncoder.from_cfg -- as a list (-1 = a root, every parent
before its child, 1 .. 32 joints) or as a name of `SKELETONS`, and runs train=False on include/posendf_amd_skeleton.h: the
layer-by-layer HIP unit for a cuda model, the first-order host twins for `train.device: cpu` (posendf_amd.model_base.PoseModel).

`forward(train=True)` runs the stock PyTorch modules unless `opt['engine']['train'] = 'hip'`: then a cuda model's training objective
and every weight gradient come from csrc/pndf_train.hip on a plan of include/posendf_amd_skeleton_train.h for this class's parent
table, with no fallback, and `posendf_amd.trainer.Trainer` trains the skeleton end to end.

`complete(poses, observed)` is pose completion for the model's tree: `project` with the observed joints held, the joint mask inside
the projection step of the unit's last kernel (or of the host twin), handed over in a pndf_project_options2 (include/posendf_amd.h);
`posendf_amd.pose_completion.PoseCompletion` drives it with several hypotheses per pose.  `interpolate(pose_a, pose_b, frames)` is pose
interpolation for the model's tree the same way: the tracks ride in a pndf_project_options3, the fill is one small kernel and the
neighbour coupling sits in the step; `posendf_amd.pose_interpolation.PoseInterpolation` drives it.  `denoise(track)` is motion
denoising in quaternion space -- the pose prior, the neighbour coupling with free end frames and a data term towards the noisy
observation, in a pndf_project_options4 --, which `posendf_amd.pose_denoising.PoseDenoising` drives.  `fit_keypoints(poses, targets,
rest)` is inverse kinematics under the prior -- 3D detections of keypoints attached to the joints, the tree with its rest offsets as the
body model, in a pndf_project_options5 --, which `posendf_amd.keypoint_fitting.KeypointFitting` drives; `forward_kinematics` is the
differentiable torch statement of its kinematics.  With `camera=` the detections are pixels, and with `root=` / `root_weights=` the tree
has a placement in the target's frame that the steps move (a pndf_project_options6; `camera_project` is the torch statement of both).
With `bone_scale=` / `scale_weight=` the segment lengths of the subject are unknowns of the same fit, one set of scales per clip (a
pndf_project_options7; `forward_kinematics(..., bone_scale=)` is the torch statement of the scaled tree).
With `views=` the detections are pixels of the same frame in several calibrated cameras (a pndf_project_options8;
`camera_project(..., views=)` is the torch statement of the pixels).
With `root_smooth=` / `root_anchor=` / `root_data=` the roots of the frames of a track are coupled to their neighbours' and drawn towards an
observed trajectory (a pndf_project_options9).
With a 3-D `views=` [B,V,16] or [frames,V,16] the cameras move from pose to pose or from frame to frame (a pndf_project_options10).
Only the second order stays 21-joint: its C ABI refuses another joint count, and that refusal is pinned.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from .engine import MAX_VIEWS, PndfError, SkeletonEngine, StreamWorkspaces, stream_handle, view_table
from .model_base import PoseModel, _Distance, pack_observed
from .synth import BONE_DIM, FEAT, PARENT

# named parent tables: get_parent_mapping('smpl') of the reference, and a 15-joint hand -- five fingers of three joints each, every
# finger a chain that starts at a root (the wrist is not part of the pose)
SKELETONS = {
    "smpl": tuple(PARENT),
    "hand": (-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13),
}


def parent_table(mapping=None):
    """the parent table of a config value: None (SMPL), a name of SKELETONS or a list"""
    if mapping is None:
        return SKELETONS["smpl"]
    if isinstance(mapping, str):
        if mapping not in SKELETONS:
            raise PndfError(f"unknown skeleton {mapping!r} ({', '.join(SKELETONS)}, or a parent table as a list)")
        return SKELETONS[mapping]
    return tuple(int(p) for p in mapping)


def skeleton_config(parents, act="lrelu", device="cuda", hidden=None, encoder=True, beta=None):
    """configs/amass.yaml with the skeleton `parents` (a name of SKELETONS or a list): model.StrEnc.parent_mapping, model.DFNet.in_dim
    to match, and optionally other hidden widths, no encoder, another Softplus beta"""
    from .config import amass_config
    cfg = amass_config(act, device)
    table = parent_table(parents)
    cfg["model"]["StrEnc"]["parent_mapping"] = list(table)
    cfg["model"]["StrEnc"]["use"] = bool(encoder)
    cfg["model"]["DFNet"]["in_dim"] = len(table) * (FEAT if encoder else BONE_DIM)
    if hidden is not None:
        cfg["model"]["DFNet"]["dims"] = [int(w) for w in hidden]
    if beta is not None:
        cfg["model"]["DFNet"]["beta"] = cfg["model"]["StrEnc"]["beta"] = float(beta)
    return cfg


class SkeletonPoseNDF(PoseModel):
    _hip_path = "unit"

    def __init__(self, opt):
        strenc = opt["model"]["StrEnc"]
        parents = parent_table(strenc.get("parent_mapping"))
        if not 1 <= len(parents) <= 32:
            raise PndfError(f"a skeleton of {len(parents)} joints: 1 .. 32 are implemented")
        dfnet = copy.deepcopy(opt["model"]["DFNet"])
        in_dim = len(parents) * (FEAT if strenc["use"] else BONE_DIM)
        if dfnet.get("in_dim", in_dim) != in_dim:
            raise PndfError(f"model.DFNet.in_dim is {dfnet['in_dim']}; a skeleton of {len(parents)} joints "
                            f"{'with' if strenc['use'] else 'without'} the structure encoder feeds it {in_dim}")
        dfnet["in_dim"] = in_dim
        super().__init__(opt, parents, dict(copy.deepcopy(strenc), parent_mapping=list(parents)), dfnet)
        if self.loss not in ("l1", "l2"):
            self.loss_l1 = nn.L1Loss()
        self._net_kw["parents"] = self.parents
        self._workspaces = StreamWorkspaces(torch.uint8)

    def _new_engine(self, idx):
        return SkeletonEngine(device=idx, **self._net_kw)

    def _engine_args(self, eng, device, B):
        """(workspace pointer, its bytes, stream): this stream's workspace on `device` for B poses"""
        ws = self._workspaces.get(device, max(eng.workspace_bytes(B), 16))
        return ws.data_ptr(), ws.numel(), stream_handle(device)

    def forward(self, pose, dist_gt=None, man_poses=None, train=False, eikonal=0.0):
        pose = pose.to(device=self.device).reshape(-1, self.num_joints, 4)
        if not train:
            return {"dist_pred": _Distance.apply(pose, self)}
        return self._forward_train(pose, dist_gt, man_poses, eikonal)

    @torch.no_grad()
    def complete(self, poses, observed, steps=100, return_dist=True, *, step_size=1.0, renormalize=None, tol=0.0):
        """Pose completion with the contract of `PoseNDF.complete`: `project` with the observed joints held.  `observed` is a bool
        tensor [J] (one mask for every pose) or [B,J], True = the joint's rotation is known and stays as it is, bit for bit (it still
        enters the distance and the gradient of the others); None = no joint is held, which is `project` bit for bit.  The mask rides
        in the projection call itself (pndf_project_options2, include/posendf_amd.h): the unit's last kernel of every step selects
        per joint, so a masked step costs no launch more than an unmasked one; a `train.device: cpu` model runs the host twin.
        Returns and step options: as `project`."""
        q = poses.to(device=self.device).reshape(-1, self.num_joints, 4).float().contiguous()
        B = q.shape[0]
        out = torch.empty_like(q)
        d = torch.empty(B, device=q.device, dtype=torch.float32)
        mask = None if observed is None else pack_observed(observed, B, q.device, self.num_joints)
        eng = self._engine_for(q.device)
        host = q.device.type == "cpu"
        if B or host:       # as `project`
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), *(() if host else self._engine_args(eng, q.device, B)),
                        step_size=step_size, renorm=renormalize, tol=tol, observed_ptr=None if mask is None or B == 0 else mask.data_ptr())
        return (out, d.view(-1, 1)) if return_dist else out

    @torch.no_grad()
    def interpolate(self, pose_a, pose_b, frames, steps=100, smooth=0.0, mode="slerp", observed=None, return_dist=True, *, step_size=1.0,
                    renormalize="unit", tol=0.0):
        """Pose interpolation with the contract of `PoseNDF.interpolate`: a track of `frames` poses from every pose of `pose_a` to the
        matching pose of `pose_b` ([P,J,4] each), relaxed onto the manifold.  Frame 0 is `pose_a`, frame frames-1 is `pose_b` with every
        joint quaternion negated where that is the shorter way round; the frames between them start as the `mode` ("slerp" / "nlerp")
        interpolation of each joint and take `steps` steps of `complete` -- the two end frames and the `observed` joints held, bit for
        bit -- with a neighbour coupling of weight `smooth` in [0, 1] inside the same step.  `observed`: bool [J], [frames,J] (one mask
        per frame, for every pair) or [P,frames,J].  The whole interpolation is ONE engine call: the tracks ride in the projection call
        itself (pndf_project_options3, include/posendf_amd.h), the unit fills a chunk of tracks with one small kernel and couples the
        neighbours in its last kernel of every step, so a step costs no launch more than a projection step; a `train.device: cpu` model
        runs the host twin.  The inputs are not written.  Returns (track [P,frames,J,4], dist [P,frames] of the last iteration); step
        options: as `project`, with unit quaternions as the default."""
        if mode not in ("slerp", "nlerp"):
            raise PndfError(f"unknown interpolation mode {mode!r} ('slerp', 'nlerp')")
        J = self.num_joints
        a = pose_a.to(device=self.device).reshape(-1, J, 4).float()
        b = pose_b.to(device=self.device).reshape(-1, J, 4).float()
        P, T = a.shape[0], int(frames)
        if b.shape[0] != P:
            raise PndfError(f"pose_a holds {P} poses, pose_b {b.shape[0]}")
        if T < 2:
            raise PndfError(f"an interpolation has at least two frames, not {frames}")
        # the call reads frames 0 and T-1 of every track of its input and nothing else of it
        ends = torch.zeros((P, T, J, 4), device=a.device, dtype=torch.float32)
        ends[:, 0], ends[:, T - 1] = a, b
        track = torch.empty_like(ends)
        d = torch.empty((P, T), device=a.device, dtype=torch.float32)
        mask = None
        if observed is not None:
            obs = torch.as_tensor(observed, device=a.device)
            if obs.dtype == torch.bool and obs.shape == (T, J):
                obs = obs.expand(P, T, J)
            if obs.dtype == torch.bool and obs.shape == (P, T, J):
                obs = obs.reshape(P * T, J)
            mask = pack_observed(obs, P * T, a.device, J)
        eng = self._engine_for(a.device)
        host = a.device.type == "cpu"
        B = P * T
        if B or host:       # as `project`
            eng.project(ends.data_ptr(), track.data_ptr(), d.data_ptr(), B, int(steps), *(() if host else self._engine_args(eng, a.device, B)),
                        step_size=step_size, renorm=renormalize, tol=tol, observed_ptr=None if mask is None or B == 0 else mask.data_ptr(),
                        frames=T, smooth=smooth, fill=mode)
        return (track, d) if return_dist else track

    @torch.no_grad()
    def denoise(self, track, steps=100, smooth=0.25, data=0.25, conf=None, observed=None, free_ends=True, return_dist=True, *, step_size=1.0,
                renormalize="unit", tol=0.0, anchor=None):
        """Motion denoising for the model's tree, in quaternion space: `track` [P,T,J,4] (or [T,J,4], one clip) is the noisy observation,
        which is both the start and the anchor.  Every step descends the distance field (the pose prior), couples every frame to its
        neighbour frames with weight `smooth` in [0, 1] (the temporal term) and pulls every joint towards its observation with weight
        `data` * conf in [0, 1] (the data term), all inside the projection step of the unit's last kernel (or of the host twin):
        pndf_project_options4, include/posendf_amd.h.  `conf`: per-joint confidences [J], [T,J] or [P,T,J] (None: ones); a joint whose
        confidence is zero, negative or NaN takes no data term and its observation is not read, so a missing detection may hold NaN --
        but it is still the start of that joint, so give it a finite guess.  `observed`: bool [J], [T,J] or [P,T,J], joints held bit for
        bit.  `free_ends` (default): the first and the last frame are as noisy as the rest and move; False holds them as `interpolate`
        does.  T = 1 runs without tracks, with the data term only.  The whole clip is ONE engine call of 2 + 2 L launches per step and
        the input is not written; a `train.device: cpu` model runs the host twin.  The defaults of `smooth` and `data` are untuned.
        `anchor` (same shape as `track`): the observation where it is not the start -- the later iterations of `PoseDenoising` start
        from the result of the iteration before and stay anchored to the original clip.
        Returns (track [P,T,J,4], dist [P,T] of the last iteration) with the leading axis as given; step options: as `project`, with
        unit quaternions as the default."""
        J = self.num_joints
        x = track.to(device=self.device).float()
        if x.dim() not in (3, 4) or tuple(x.shape[-2:]) != (J, 4):
            raise PndfError(f"a clip is [P,T,{J},4] or [T,{J},4], not {tuple(track.shape)}")
        single = x.dim() == 3
        q = x.reshape((-1,) + tuple(x.shape[-3:])).contiguous()
        P, T = q.shape[0], q.shape[1]
        if T < 1:
            raise PndfError("a clip has at least one frame")
        B = P * T
        if anchor is None:
            seen = q
        else:
            if tuple(anchor.shape) != tuple(track.shape):
                raise PndfError(f"anchor has the clip's shape {tuple(track.shape)}, not {tuple(anchor.shape)}")
            seen = anchor.to(device=self.device).float().reshape(q.shape).contiguous()
        out = torch.empty_like(q)
        d = torch.empty((P, T), device=q.device, dtype=torch.float32)

        def per_joint(value, dtype, what):
            v = torch.as_tensor(value, device=q.device)
            if (dtype == torch.bool) != (v.dtype == torch.bool) or (dtype != torch.bool and not v.is_floating_point()):
                raise PndfError(f"{what} is a {'bool' if dtype == torch.bool else 'floating-point'} tensor, not {v.dtype}")
            if tuple(v.shape) not in ((J,), (T, J), (P, T, J)):
                raise PndfError(f"{what} is [{J}], [{T},{J}] or [{P},{T},{J}], not {tuple(v.shape)}")
            return v.to(dtype).expand(P, T, J).reshape(B, J).contiguous()

        weights = None if conf is None else per_joint(conf, torch.float32, "conf")
        mask = None if observed is None else pack_observed(per_joint(observed, torch.bool, "observed"), B, q.device, J)
        eng = self._engine_for(q.device)
        host = q.device.type == "cpu"
        if B or host:       # as `project`
            tracks = dict(frames=T, smooth=smooth, free_ends=bool(free_ends)) if T >= 2 else {}
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), *(() if host else self._engine_args(eng, q.device, B)),
                        step_size=step_size, renorm=renormalize, tol=tol, observed_ptr=None if mask is None or B == 0 else mask.data_ptr(),
                        anchor_ptr=seen.data_ptr() if B else None, conf_ptr=None if weights is None or B == 0 else weights.data_ptr(), data=data if B else 0.0,
                        **tracks)
        if single:
            out, d = out[0], d[0]
        return (out, d) if return_dist else out

    @torch.no_grad()
    def fit_keypoints(self, poses, targets, rest, steps=100, weight=0.02, conf=None, keypoint_joints=None, keypoint_offsets=None, observed=None,
                      frames=None, smooth=0.0, anchor=None, data=0.0, free_ends=False, return_dist=True, return_energy=False, *, step_size=1.0,
                      renormalize=None, tol=0.0, root=None, root_weights=(0.0, 0.0), camera=None, rho=0.0, return_root=False, bone_scale=None,
                      scale_weight=0.0, scale_prior=0.0, scale_range=None, scale_rates=None, per_pose_scale=False, return_scale=False,
                      views=None, root_smooth=(0.0, 0.0), root_anchor=None, root_data=(0.0, 0.0)):
        """Inverse kinematics under the learned prior, for the model's tree: from the start `poses` [B,J,4], `steps` projection steps that
        also descend E = 1/2 sum_k conf_k |P_k(pose) - targets_k|^2 with weight `weight` (nu), P_k = `forward_kinematics` of the pose.
        `targets` [B,K,3] are 3D detections in the roots' frame; `rest` [J,3] the offsets of the joints from their parents in the rest
        pose; `keypoint_joints` [K] (None: K = J, keypoint k is joint k) and `keypoint_offsets` [K,3] (None: zeros) attach the keypoints;
        `conf` [K] or [B,K]: a keypoint whose confidence is zero, negative or NaN takes no part and its target is not read, so a missing
        detection may hold NaN.  `observed` (bool [J] or [B,J]) joints are held bit for bit and still move their subtree.  `frames` = T >= 2
        reads the poses as B / T clips and couples neighbouring frames with weight `smooth`, the end frames held unless `free_ends`;
        `anchor` [B,J,4] with `data` adds the quaternion data term of `denoise`.  Everything rides in ONE engine call of 2 + 2 L launches
        per step (pndf_project_options5, include/posendf_amd.h): kinematics, residuals and their reverse run inside the unit's last kernel;
        a `train.device: cpu` model runs the host twin.  The inputs are not written.  The default `weight` is untuned: it is the largest of
        the values tried (0.02, 0.05) at which the energy of a 15-joint hand with rest offsets within [-0.75, 0.75]^3 fell at every step of
        pure inverse kinematics; the term is a plain gradient step whose length grows with the square of the bone lengths, and already
        with offsets within [-1, 1]^3 one start of 48 oscillates at 0.02 -- scale `weight` down by the square of the rig's size.
        Where tensors may live: the per-pose tensors `poses`, `targets`, `conf`, `anchor` and `observed` are accepted on the model's device
        and on the cpu (host data is copied to the model's device); a tensor on any other device -- a cuda tensor handed to a
        `train.device: cpu` model, or one on another GPU than the model's -- raises PndfError, since it would mean a silent copy of a whole
        batch off its device.  The small tables `rest`, `keypoint_joints` and `keypoint_offsets` are host tables of the call and are
        accepted from any device.
        Image fitting (pndf_project_options6; DESIGN.md section 2j "Image fitting"): `camera` = (fx, fy, cx, cy) makes `targets` [B,K,2] pixel
        detections of a pinhole camera -- the residual is taken in normalised image coordinates, (C_x / C_z, C_y / C_z) against
        ((u - cx) / fx, (v - cy) / fy), so the energy and `weight` do not depend on the resolution; a keypoint that is not in front of the
        camera takes no part in that step; `rho` > 0 replaces the squared residual by rho^2 e^2 / (e^2 + rho^2).  `root` [B,7] or [7] places
        the tree in the target's frame, C_k = R(c) P_k + s with c = root[:4] (a quaternion, real part first, normalised) and s = root[4:];
        it is per pose, lives where `poses` may live and is cloned.  `root_weights` = (nu_rot, nu_trans) let every step move it along the
        energy's gradient (0: that part is held); the root is not a joint, so neither `observed` nor held end frames hold it.  Without a
        keypoint term (`weight` 0) the root is left as it is.  The default weights are zero; those tried are listed in
        `posendf_amd.keypoint_fitting`.  `camera_project` is the torch statement of C_k and of the pixels.  The defaults are the call
        without a camera, bit for bit.
        Bone lengths (pndf_project_options7; DESIGN.md section 2j "Bone lengths"): `bone_scale` [G,S] or [S], S = J + K, scales the rest
        offset of joint j by bone_scale[..., j] and the local offset of keypoint k by bone_scale[..., J + k]; with `frames` = T >= 2 and
        without `per_pose_scale` there is one row per clip (G = B / T) which all its frames read, otherwise one per pose (G = B).  It lives
        where `poses` may live and is cloned.  `scale_weight` (nu_len) > 0 lets every step move the scales along the gradient of the
        clip's mean energy plus the prior 1/2 `scale_prior` (sigma - 1)^2 (then a missing `bone_scale` starts at ones); `scale_rates` [S]
        multiplies the weight per scale (0 holds that scale); `scale_range` = (lo, hi) clamps them.  Like the root the scales are not
        joints: held joints and held end frames still contribute to their gradient.  With 2D targets and a free root translation the
        overall scale trades against depth and is not observable: use a prior.  The default weights are zero and UNTUNED.
        Several cameras (pndf_project_options8; DESIGN.md section 2j "Several cameras"): `views` -- a [V,16] array (per view fx, fy, cx,
        cy, R row-major, t) or a sequence of (K [3,3] or (fx, fy, cx, cy), R [3,3], t [3]), V <= 8 -- makes `targets` [B,V,K,2] the pixels
        of the same frame in V calibrated cameras and `conf` [K], [V,K] or [B,V,K]; R and t map the world frame, in which `root` places
        the tree, to the camera's (C = R W + t).  A view whose confidence for a keypoint is not positive, or behind which the keypoint
        lies, takes no part for it and its target is not read.  `camera=` together with `views=` is an error.  `camera_project(views=)` is
        the torch statement of the pixels.
        Moving cameras (pndf_project_options10; DESIGN.md section 2j "Moving cameras"): `views` as a 3-D tensor or array is a table per
        pose [B,V,16], or with `frames` a table per frame of a track [frames,V,16] -- one camera path shared by every track; when B ==
        frames the two mean the same.  It is moved to the poses' device as contiguous float32.  A row whose fx or fy is not positive
        (zeros, NaNs) switches its view off for that pose: neither its targets nor its confidences are read.  In a row that is on,
        finite entries are the caller's responsibility: the library cannot look at a table in device memory.
        The root's trajectory (pndf_project_options9; DESIGN.md section 2j "Root trajectory"): `root_smooth` = (lambda_rot, lambda_trans),
        each in [0, 1], couples the root of every frame of a track (`frames`) to the roots of its neighbour frames as `smooth` couples
        the joints, the end frames with their one neighbour whether or not `free_ends` is set; `root_anchor` [B,7] (where `poses` may
        live) is an observed or earlier trajectory and `root_data` = (mu_rot, mu_trans) the weights of the data term towards it.  A part
        needs its `root_weights` entry positive.  The defaults are the call without them, bit for bit, and UNTUNED.
        Returns poses [B,J,4], then dist [B,1] of the last iteration (`return_dist`), then the energy [B] of the last iteration, evaluated
        before its update (`return_energy`), then the final root [B,7] (`return_root`; the identity placement when none was given), then
        the final scales [G,S] (`return_scale`; ones when none were given); step options: as `project`."""
        J = self.num_joints
        home = torch.device(self.device)

        def on_device(value, what):
            # host data and data on the model's device are taken; anything else would be a silent copy of a batch off its device
            t = torch.as_tensor(value)
            there = t.device
            if there.type != "cpu" and (there.type != home.type or (home.index is not None and there.index != home.index)):
                raise PndfError(f"{what} lives on {there}, the model on {home}: per-pose tensors are taken from the model's device or from the cpu")
            return t.to(device=home)

        q = on_device(poses, "poses").float()
        if q.dim() < 2 or tuple(q.shape[-2:]) != (J, 4):
            raise PndfError(f"poses are [B,{J},4], not {tuple(poses.shape)}")
        q = q.reshape(-1, J, 4).contiguous()
        B, dev = q.shape[0], q.device

        def table(value, shape, dtype, what):
            t = torch.as_tensor(value).detach().to("cpu")
            if tuple(t.shape) != shape:
                raise PndfError(f"{what} is {list(shape)}, not {list(t.shape)}")
            return t.to(dtype).contiguous()

        kpj = None if keypoint_joints is None else torch.as_tensor(keypoint_joints).detach().to("cpu")
        if kpj is not None and (kpj.dim() != 1 or kpj.dtype in (torch.bool, torch.float16, torch.float32, torch.float64)):
            raise PndfError(f"keypoint_joints is an integer tensor [K], not {kpj.dtype} {list(kpj.shape)}")
        K = J if kpj is None else int(kpj.shape[0])
        kpj = None if kpj is None else kpj.to(torch.int32).contiguous()
        rest_t = table(rest, (J, 3), torch.float32, "rest")
        kpo = None if keypoint_offsets is None else table(keypoint_offsets, (K, 3), torch.float32, "keypoint_offsets")
        D = 3 if camera is None and views is None else 2
        if camera is not None and views is not None:
            raise PndfError("camera= is the one camera of a fit and views= the several: give one of them")
        if camera is not None and len(tuple(camera)) != 4:
            raise PndfError("camera is (fx, fy, cx, cy)")
        mv = None      # the moving table [B,V,16] or [frames,V,16] of a pndf_project_options10
        if views is not None and hasattr(views, "shape") and len(views.shape) == 3:
            mv = on_device(views, "views")
            if not mv.is_floating_point() or mv.shape[2] != 16:
                raise PndfError(f"views with a block per pose or frame is a floating-point [N,V,16], not {mv.dtype} {list(mv.shape)}")
        vt = None if views is None or mv is not None else view_table(views)
        V = 1 if vt is None else int(vt.shape[0])
        if mv is not None:
            V = int(mv.shape[1])
        several = vt is not None or mv is not None
        if several and not 1 <= V <= MAX_VIEWS:
            raise PndfError(f"views are 1 .. {MAX_VIEWS} rows, not {V}")
        y = on_device(targets, "targets").float()
        if several:
            if y.dim() < 3 or tuple(y.shape[-3:]) != (V, K, 2) or y.numel() != B * V * K * 2:
                raise PndfError(f"targets are [{B},{V},{K},2] with views, not {list(y.shape)}")
            y = y.reshape(B, V, K, 2).contiguous()
        else:
            if y.dim() < 2 or tuple(y.shape[-2:]) != (K, D) or y.numel() != B * K * D:
                raise PndfError(f"targets are [{B},{K},{D}], not {list(y.shape)}")
            y = y.reshape(B, K, D).contiguous()
        place = None
        if root is not None:
            place = on_device(root, "root")
            if not place.is_floating_point() or tuple(place.shape) not in ((7,), (B, 7)):
                raise PndfError(f"root is a floating-point tensor [7] or [{B},7], not {place.dtype} {list(place.shape)}")
            place = place.float().expand(B, 7).contiguous().clone()
        if len(tuple(root_weights)) != 2:
            raise PndfError("root_weights is (nu_rot, nu_trans)")
        if len(tuple(root_smooth)) != 2:
            raise PndfError("root_smooth is (lambda_rot, lambda_trans)")
        if len(tuple(root_data)) != 2:
            raise PndfError("root_data is (mu_rot, mu_trans)")
        track_anchor = None
        if root_anchor is not None:
            track_anchor = on_device(root_anchor, "root_anchor")
            if not track_anchor.is_floating_point() or tuple(track_anchor.shape) != (B, 7):
                raise PndfError(f"root_anchor is a floating-point tensor [{B},7], not {track_anchor.dtype} {list(track_anchor.shape)}")
            track_anchor = track_anchor.float().contiguous()
        root_tracked = track_anchor is not None or any(root_smooth) or any(root_data)
        T = int(frames or 0)
        if T == 1:
            T = 0
        per_frame = False
        if mv is not None:
            N = int(mv.shape[0])
            if N != B and not (T >= 2 and N == T):
                raise PndfError(f"views [{N},{V},16] has neither a block per pose ([{B},{V},16]) nor a block per frame of a track "
                                f"([frames,{V},16] with frames = {T})")
            per_frame = N != B
            mv = mv.float().contiguous()
        S = J + K
        G = B if (per_pose_scale or T < 2) else (B // T if B % T == 0 else -1)
        lengthed = bone_scale is not None or bool(scale_weight) or bool(scale_prior) or scale_range is not None or scale_rates is not None or bool(per_pose_scale)
        scales = None
        if bone_scale is not None:
            scales = on_device(bone_scale, "bone_scale")
            if not scales.is_floating_point() or tuple(scales.shape) not in ((S,), (G, S)):
                raise PndfError(f"bone_scale is a floating-point tensor [{S}] or [{G},{S}], not {scales.dtype} {list(scales.shape)}")
            scales = scales.float().expand(max(G, 0), S).contiguous().clone()
        elif scale_weight and G >= 0:
            scales = torch.ones(G, S, device=home, dtype=torch.float32)
        if scale_range is not None and len(tuple(scale_range)) != 2:
            raise PndfError("scale_range is (lo, hi)")
        rates = None
        if scale_rates is not None:
            rates = table(scale_rates, (S,), torch.float32, "scale_rates").tolist()
        c = None
        if conf is not None:
            c = on_device(conf, "conf")
            if several:
                if not c.is_floating_point() or tuple(c.shape) not in ((K,), (V, K), (B, V, K)):
                    raise PndfError(f"conf is a floating-point tensor [{K}], [{V},{K}] or [{B},{V},{K}] with views, not {c.dtype} {list(c.shape)}")
                c = c.float().expand(B, V, K).contiguous()
            else:
                if not c.is_floating_point() or tuple(c.shape) not in ((K,), (B, K)):
                    raise PndfError(f"conf is a floating-point tensor [{K}] or [{B},{K}], not {c.dtype} {list(c.shape)}")
                c = c.float().expand(B, K).contiguous()
        seen = None
        if anchor is not None:
            seen = on_device(anchor, "anchor").float()
            if seen.numel() != q.numel() or tuple(seen.shape[-2:]) != (J, 4):
                raise PndfError(f"anchor has the poses' shape {list(q.shape)}, not {list(seen.shape)}")
            seen = seen.reshape(q.shape).contiguous()
        out = torch.empty_like(q)
        d = torch.empty(B, device=dev, dtype=torch.float32)
        energy = torch.zeros(B, device=dev, dtype=torch.float32)
        mask = None if observed is None else pack_observed(on_device(observed, "observed"), B, dev, J)
        eng = self._engine_for(dev)
        host = dev.type == "cpu"
        if B or host:       # as `project`
            tracks = dict(frames=T, smooth=smooth, free_ends=bool(free_ends)) if T else {}
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), *(() if host else self._engine_args(eng, dev, B)),
                        step_size=step_size, renorm=renormalize, tol=tol, observed_ptr=None if mask is None or B == 0 else mask.data_ptr(),
                        anchor_ptr=None if seen is None or B == 0 else seen.data_ptr(), data=data if seen is not None and B else 0.0,
                        kp_target_ptr=y.data_ptr() if B else None, kp_conf_ptr=None if c is None or B == 0 else c.data_ptr(),
                        kp_energy_ptr=energy.data_ptr() if B else None, rest_ptr=rest_t.data_ptr(),
                        kp_joint_ptr=None if kpj is None else kpj.data_ptr(), kp_offset_ptr=None if kpo is None else kpo.data_ptr(),
                        n_keypoints=K, kp_weight=weight, **tracks,
                        **(dict(root_ptr=place.data_ptr() if place is not None and B else None, root_weights=tuple(root_weights) if B else (0.0, 0.0), camera=camera, rho=rho)
                           if place is not None or camera is not None or rho or any(root_weights) else {}),
                        **(dict(views=vt) if vt is not None and B else {}),      # (without poses there are no targets for the views to size)
                        **(dict(pose_views=mv, views_per_frame=per_frame) if mv is not None and B else {}),
                        **(dict(root_smooth=tuple(root_smooth) if B else (0.0, 0.0), root_data=tuple(root_data) if B else (0.0, 0.0),
                                root_anchor_ptr=track_anchor.data_ptr() if track_anchor is not None and B else None) if root_tracked else {}),
                        **(dict(bone_scale_ptr=scales.data_ptr() if scales is not None and B else None, len_rate=rates, len_weight=scale_weight if B else 0.0,
                                len_prior=scale_prior, len_range=None if scale_range is None else tuple(scale_range), per_pose_lengths=bool(per_pose_scale))
                           if lengthed else {}))
        if return_scale and scales is None:
            scales = torch.ones(max(G, 0), S, device=dev, dtype=torch.float32)
        if return_root and place is None:
            place = torch.zeros(B, 7, device=dev, dtype=torch.float32)
            place[:, 0] = 1.0
        result = (out,) + ((d.view(-1, 1),) if return_dist else ()) + ((energy,) if return_energy else ()) + ((place,) if return_root else ()) + ((scales,) if return_scale else ())
        return result if len(result) > 1 else out


def forward_kinematics(pose, parents, rest, keypoint_joints=None, keypoint_offsets=None, bone_scale=None):
    """The keypoints of poses on a joint tree, differentiable: pose [...,J,4] (joint quaternions, real part first; each is normalised,
    r = Q / max(|Q|, 1e-12)) -> [...,K,3].  `parents`: the parent table (-1: a root; every parent before its child); `rest` [J,3]: joint j
    relative to its parent in the rest pose (the position of a root); keypoint k sits on joint `keypoint_joints[k]` at the local offset
    `keypoint_offsets[k]` (None: K = J, the joints themselves).  With G_j the global rotation and p_j the position of joint j:
    root G_j = R_j, p_j = t_j; else G_j = G_parent R_j, p_j = p_parent + G_parent t_j; P_k = p_a(k) + G_a(k) o_k.  This is the statement
    `SkeletonPoseNDF.fit_keypoints` (csrc/pndf_fk.h) descends; use it to make targets and to read residuals.  `bone_scale` [...,J+K] or
    [J+K] (None: no scaling, the same bits): joint j's rest offset is scaled by bone_scale[..., j], keypoint k's local offset by
    bone_scale[..., J + k] -- the tree of `fit_keypoints(bone_scale=)`; its leading dimensions broadcast against the pose's."""
    parents = parent_table(parents)
    J = len(parents)
    if tuple(pose.shape[-2:]) != (J, 4):
        raise PndfError(f"pose is [...,{J},4], not {tuple(pose.shape)}")
    rest = torch.as_tensor(rest, dtype=pose.dtype, device=pose.device)
    if tuple(rest.shape) != (J, 3):
        raise PndfError(f"rest is [{J},3], not {tuple(rest.shape)}")
    joints = list(range(J)) if keypoint_joints is None else [int(a) for a in torch.as_tensor(keypoint_joints).reshape(-1).tolist()]
    if any(a < 0 or a >= J for a in joints):
        raise PndfError(f"keypoint_joints lie in 0 .. {J - 1}")
    offsets = None if keypoint_offsets is None else torch.as_tensor(keypoint_offsets, dtype=pose.dtype, device=pose.device)
    if offsets is not None and tuple(offsets.shape) != (len(joints), 3):
        raise PndfError(f"keypoint_offsets is [{len(joints)},3], not {tuple(offsets.shape)}")
    r = pose / pose.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    w, x, y, z = r.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(pose.shape[:-1] + (3, 3))
    sg = None
    if bone_scale is not None:      # a scale commutes with the rotation: sigma (G t) is G (sigma t), and with sigma = 1 the same bits as without
        sg = torch.as_tensor(bone_scale, dtype=pose.dtype, device=pose.device)
        if sg.shape[-1] != J + len(joints):
            raise PndfError(f"bone_scale is [...,{J + len(joints)}], not {tuple(sg.shape)}")
    G, p = [], []
    for j, pa in enumerate(parents):
        if pa < 0:
            G.append(R[..., j, :, :])
            t = rest[j] if sg is None else sg[..., j, None] * rest[j]
            p.append(t.expand(pose.shape[:-2] + (3,)))
        else:
            G.append(G[pa] @ R[..., j, :, :])
            v = (G[pa] @ rest[j].unsqueeze(-1)).squeeze(-1)
            p.append(p[pa] + (v if sg is None else sg[..., j, None] * v))
    out = []
    for k, a in enumerate(joints):
        if offsets is None:
            out.append(p[a])
        else:
            v = (G[a] @ offsets[k].unsqueeze(-1)).squeeze(-1)
            out.append(p[a] + (v if sg is None else sg[..., J + k, None] * v))
    return torch.stack(out, dim=-2)


def camera_project(points, root=None, camera=None, views=None):
    """Keypoints in the target's frame, and their pixels, differentiable: points [...,K,3] (`forward_kinematics`, the roots' frame) ->
    C_k = R(c) P_k + s with `root` [...,7] or [7] = (c: a quaternion, real part first, normalised c / max(|c|, 1e-12); s: a translation),
    or the points themselves when root is None; with `camera` = (fx, fy, cx, cy) the pixels (fx C_x / C_z + cx, fy C_y / C_z + cy)
    [...,K,2] of a pinhole camera that looks along +z.  This is the statement `SkeletonPoseNDF.fit_keypoints(camera=..., root=...)`
    (csrc/pndf_fk.h) descends; use it to make targets and to read residuals.  With `views` ([V,16], or a sequence of (K or (fx, fy, cx, cy),
    R, t): `fit_keypoints(views=)`) the root places the tree in the world frame and the result is [...,V,K,2]: the pixels
    (fx C_x / C_z + cx, fy C_y / C_z + cy) of C = R_v W + t_v in every view.  A `views` tensor or array with leading dimensions,
    [...,V,16], is a table per pose (moving cameras): those dimensions broadcast against the points' and the result is [...,V,K,2]."""
    if camera is not None and views is not None:
        raise PndfError("camera= is the one camera and views= the several: give one of them")
    if points.shape[-1] != 3:
        raise PndfError(f"points are [...,K,3], not {tuple(points.shape)}")
    C = points
    if root is not None:
        root = torch.as_tensor(root, dtype=points.dtype, device=points.device)
        if root.shape[-1] != 7:
            raise PndfError(f"root is [...,7], not {tuple(root.shape)}")
        c, s = root[..., :4], root[..., 4:]
        r = c / c.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
        w, x, y, z = r.unbind(-1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(r.shape[:-1] + (3, 3))
        C = (R.unsqueeze(-3) @ points.unsqueeze(-1)).squeeze(-1) + s.unsqueeze(-2)
    if views is not None and hasattr(views, "shape") and len(views.shape) > 2:
        # moving cameras (`fit_keypoints` with a 3-D views): a table [...,V,16] whose leading dimensions broadcast against the points'
        vt = torch.as_tensor(views, dtype=points.dtype, device=points.device)
        if vt.shape[-1] != 16:
            raise PndfError(f"views with leading dimensions is [...,V,16], not {tuple(vt.shape)}")
        Rv = vt[..., 4:13].reshape(vt.shape[:-1] + (1, 3, 3))                                         # [...,V,1,3,3]
        Cv = (Rv @ C.unsqueeze(-3).unsqueeze(-1)).squeeze(-1) + vt[..., 13:16].unsqueeze(-2)         # [...,V,K,3]
        f, pp = vt[..., 0:2].unsqueeze(-2), vt[..., 2:4].unsqueeze(-2)
        return f * Cv[..., :2] / Cv[..., 2:3] + pp
    if views is not None:
        vt = torch.as_tensor(view_table(views), dtype=points.dtype, device=points.device)      # [V,16]
        Cv = (vt[:, 4:13].reshape(-1, 1, 3, 3) @ C.unsqueeze(-3).unsqueeze(-1)).squeeze(-1) + vt[:, 13:16].unsqueeze(-2)      # [...,V,K,3]
        f, pp = vt[:, 0:2].unsqueeze(-2), vt[:, 2:4].unsqueeze(-2)
        return f * Cv[..., :2] / Cv[..., 2:3] + pp
    if camera is None:
        return C
    fx, fy, cx, cy = (float(v) for v in camera)
    return torch.stack([fx * C[..., 0] / C[..., 2] + cx, fy * C[..., 1] / C[..., 2] + cy], dim=-1)
