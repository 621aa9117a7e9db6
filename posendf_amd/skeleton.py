"""`SkeletonPoseNDF` -- the Pose-NDF model for any joint tree.

The model has nothing SMPL-specific in it: a chain of bone MLPs along a parent table in front of an MLP (reference
model/network/net_modules.py:140-170, :46-72).  `PoseNDF` (posendf_amd.facade) runs the 21-joint table of
get_parent_mapping('smpl') on the persistent kernels; this class takes the table from the config key
`model.StrEnc.parent_mapping` -- the key of the reference's own StructureEncoder.from_cfg -- as a list (-1 = a root, every parent
before its child, 1 .. 32 joints) or as a name of `SKELETONS`, and runs train=False on include/posendf_amd_skeleton.h: the
layer-by-layer HIP unit for a cuda model, the first-order host twins for `train.device: cpu`.  No fallback: a cuda pose runs on
the HIP unit or raises.  Same parameter tree and state-dict keys as the reference (`enc.net.{j}.net.{0,2}`, `dfnet.lin{l}`).

`forward(train=True)` runs the stock PyTorch modules, so another skeleton trains through PyTorch autograd; the HIP training path,
completion, interpolation and the second order stay 21-joint.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .engine import CpuEngine, PndfError, SkeletonEngine, StreamWorkspaces, state_dict_order, stream_handle
from .facade import gradient
from .modules import DFNet, StructureEncoder
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


class _SkeletonDistance(torch.autograd.Function):
    """dist_pred = f(pose) with first-order autograd: backward(g) = g * d dist / d pose, both from one pndf_skel_forward_grad (or
    its host twin); a second derivative raises (once_differentiable)."""

    @staticmethod
    def forward(ctx, pose, owner):
        d, dq = owner._launch(pose, ctx.needs_input_grad[0])
        if dq is not None:
            ctx.save_for_backward(dq)
        ctx.pose_dtype = pose.dtype
        return d

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (dq,) = ctx.saved_tensors
        return (grad_out.reshape(-1, 1, 1).to(dq.dtype) * dq).to(ctx.pose_dtype), None


class SkeletonPoseNDF(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.device = opt["train"]["device"]
        strenc = opt["model"]["StrEnc"]
        self.parents = parent_table(strenc.get("parent_mapping"))
        self.num_joints = len(self.parents)
        if not 1 <= self.num_joints <= 32:
            raise PndfError(f"a skeleton of {self.num_joints} joints: 1 .. 32 are implemented")
        self.enc = None
        if strenc["use"]:
            enc_opt = dict(copy.deepcopy(strenc), parent_mapping=list(self.parents))
            self.enc = StructureEncoder(enc_opt).to(self.device)
        dfnet = copy.deepcopy(opt["model"]["DFNet"])
        in_dim = self.num_joints * (FEAT if self.enc is not None else BONE_DIM)
        if dfnet.get("in_dim", in_dim) != in_dim:
            raise PndfError(f"model.DFNet.in_dim is {dfnet['in_dim']}; a skeleton of {self.num_joints} joints "
                            f"{'with' if self.enc is not None else 'without'} the structure encoder feeds it {in_dim}")
        dfnet["in_dim"] = in_dim
        self.dfnet = DFNet(dfnet).to(self.device)
        self.loss = opt["train"]["loss_type"]
        self.loss_l1 = nn.MSELoss() if self.loss == "l2" else nn.L1Loss()
        self._act = dfnet["act"]
        self._beta = float(dfnet.get("beta", 100.0))
        self._enc_act = strenc["act"] if self.enc is not None else None
        self._enc_beta = float(strenc.get("beta", self._beta)) if self.enc is not None else None
        self._hidden = list(dfnet["dims"])
        self._engines = {}        # device index or "cpu" -> [engine, weight fingerprint]
        self._workspaces = StreamWorkspaces(torch.uint8)

    def train(self, mode=True):
        super().train(mode)
        return self

    # ---- engine plumbing -----------------------------------------------------------------------
    def _fingerprint(self):
        """(storage, version) of every parameter: the weights are uploaded again when it changes, as the facade's does"""
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _engine_for(self, device):
        if device.type not in ("cuda", "cpu"):
            raise PndfError(f"SkeletonPoseNDF inference runs on the HIP unit (cuda) or the host twins (cpu), not on {device}")
        host = device.type == "cpu"
        idx = "cpu" if host else (device.index if device.index is not None else torch.cuda.current_device())
        entry = self._engines.get(idx)
        if entry is None:
            kw = dict(act=self._act, beta=self._beta, encoder=self.enc is not None, hidden=self._hidden, enc_act=self._enc_act,
                      enc_beta=self._enc_beta, parents=self.parents)
            entry = self._engines[idx] = [CpuEngine(**kw) if host else SkeletonEngine(device=idx, **kw), None]
        fp = self._fingerprint()
        if entry[1] != fp:          # first use, load_state_dict, an optimiser step, a replaced Parameter, .to()
            sd = self.state_dict()
            keys = state_dict_order(self.enc is not None, len(self._hidden) + 1, parents=self.parents)
            entry[0].load_weights({k: sd[k].detach().float().cpu().numpy() for k in keys})
            entry[1] = fp
        return entry[0]

    def _workspace(self, eng, q, B):
        """(pointer, bytes) of this stream's workspace on q's device for B poses"""
        ws = self._workspaces.get(q.device, max(eng.workspace_bytes(B), 16))
        return ws.data_ptr(), ws.numel()

    def _poses(self, pose):
        q = pose.detach().to(device=self.device).reshape(-1, self.num_joints, 4)
        if q.dtype != torch.float32 or not q.is_contiguous():
            q = q.float().contiguous()
        return q

    def _launch(self, pose, want_grad):
        """dist_pred [B,1] and, when asked for, d dist / d pose [B,J,4] (else None)"""
        q = self._poses(pose)
        B = q.shape[0]
        d = torch.empty(B, device=q.device, dtype=torch.float32)
        dq = torch.empty_like(q) if want_grad else None
        eng = self._engine_for(q.device)
        if q.device.type == "cpu":
            if want_grad:
                eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B)
            else:
                eng.forward(q.data_ptr(), d.data_ptr(), B)
        elif B:
            ws, nbytes = self._workspace(eng, q, B)
            st = stream_handle(q.device)
            if want_grad:
                eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, ws, nbytes, st)
            else:
                eng.forward(q.data_ptr(), d.data_ptr(), B, ws, nbytes, st)
        return d.view(B, 1), dq

    # ---- reference API -------------------------------------------------------------------------
    def forward(self, pose, dist_gt=None, man_poses=None, train=False, eikonal=0.0):
        J = self.num_joints
        pose = pose.to(device=self.device).reshape(-1, J, 4)
        if not train:
            return {"dist_pred": _SkeletonDistance.apply(pose, self)}
        # ------ the training objective of model/posendf.py:65-99 on the stock modules
        pose.requires_grad = True
        dist_gt = dist_gt.to(device=self.device).reshape(-1)
        x = torch.nn.functional.normalize(pose, dim=1)
        dist_pred = self.dfnet(self.enc(x) if self.enc is not None else x)
        man = man_poses.to(device=self.device).reshape(-1, J, 4)
        dist_man = self.dfnet(self.enc(man) if self.enc is not None else man)
        loss = self.loss_l1(dist_pred[:, 0], dist_gt)
        if eikonal > 0.0:
            eik = ((gradient(pose, dist_pred).norm(2, dim=-1) - 1) ** 2).mean()
            return loss, {"dist": loss, "man_loss": dist_man.abs().mean(), "eikonal": eik}
        return loss, {"dist": loss}

    @torch.no_grad()
    def project(self, poses, steps=100, return_dist=True, *, step_size=1.0, renormalize=None, tol=0.0):
        """`steps` times q <- q - dist_pred(q) * d dist_pred / d q with the meaning and the step options of `PoseNDF.project`.
        Returns (poses [B,J,4], dist [B,1] of the last iteration)."""
        q = self._poses(poses)
        B = q.shape[0]
        out = torch.empty_like(q)
        d = torch.zeros(B, device=q.device, dtype=torch.float32)
        eng = self._engine_for(q.device)
        if q.device.type == "cpu":
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), step_size=step_size, renorm=renormalize, tol=tol)
        elif B:
            ws, nbytes = self._workspace(eng, q, B)
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), ws, nbytes, stream_handle(q.device),
                        step_size=step_size, renorm=renormalize, tol=tol)
        return (out, d.view(-1, 1)) if return_dist else out
