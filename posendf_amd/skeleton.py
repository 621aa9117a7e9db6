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
observation, in a pndf_project_options4 --, which `posendf_amd.pose_denoising.PoseDenoising` drives.  The second order stays 21-joint
(DESIGN.md section 8).
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from .engine import PndfError, SkeletonEngine, StreamWorkspaces, stream_handle
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
