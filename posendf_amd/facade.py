"""`PoseNDF` -- drop-in for the reference class of the same name (reference model/posendf.py:30-101).

Same constructor (`PoseNDF(opt)` reading the keys of configs/amass.yaml that the reference reads) and the same
`forward(pose, dist_gt=None, man_poses=None, train=True, eikonal=0.0)` signature and return values, on the 21-joint table of
get_parent_mapping('smpl'); the model layer it shares with `SkeletonPoseNDF` is posendf_amd.model_base.PoseModel.  A cuda model's
train=False and `project()` run on the fused persistent kernels (include/posendf_amd.h).

`forward(train=True)` runs on the stock PyTorch modules unless `opt['engine']['train'] = 'hip'`: then a cuda model's training
objective and every weight gradient come from csrc/pndf_train.hip (posendf_amd.train.TrainObjective), again with no fallback; the
knob is the model base's.

`hvp(pose, v)` gives the distance, its pose gradient and Hessian-vector products with respect to the pose
(include/posendf_amd_second_order.h); `opt['engine']['second_order'] = 'hip'` makes the train=False gradient itself differentiable
once more through the same entry point (default 'off': a double backward raises).
"""
from __future__ import annotations

import logging
import os
import warnings

import torch
from torch.autograd.function import once_differentiable

from .engine import Engine, PndfError, SecondOrderEngine, StreamWorkspaces, device_index, state_dict_order, stream_handle
from .model_base import PoseModel, _Distance, cached, gradient, pack_observed  # noqa: F401  (`gradient` is part of this module's surface)
from .synth import PARENT


class _Distance2(torch.autograd.Function):
    """`_Distance` for opt['engine']['second_order'] = 'hip': the same launch and the same values, but the backward is itself a
    differentiable function of (pose, grad_out)."""

    @staticmethod
    def forward(ctx, pose, owner):
        d, dq = owner._launch(pose, ctx.needs_input_grad[0])
        if dq is not None:
            ctx.save_for_backward(pose, dq)
        ctx.owner = owner
        return d

    @staticmethod
    def backward(ctx, grad_out):
        pose, dq = ctx.saved_tensors
        return _DistanceGrad.apply(pose, grad_out, dq, ctx.owner), None


class _DistanceGrad(torch.autograd.Function):
    """(pose, grad_out) -> grad_out * d dist / d pose, the value from the forward's launch (`dq`).  Its backward, given the incoming
    v: grad_out * H v for the pose and <v, d dist / d pose> for grad_out, from one pndf_second_order call; a third order raises."""

    @staticmethod
    def forward(ctx, pose, grad_out, dq, owner):
        ctx.save_for_backward(pose, grad_out)
        ctx.owner = owner
        return (grad_out.reshape(-1, 1, 1).to(dq.dtype) * dq).to(pose.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, v):
        pose, grad_out = ctx.saved_tensors
        need_pose, need_go = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        _, _, t, out = ctx.owner._second_order(pose.detach(), v, None, grad_out.detach().reshape(-1), want=(False, False, need_go, need_pose))
        return (out.to(pose.dtype) if need_pose else None, t.reshape(grad_out.shape).to(grad_out.dtype) if need_go else None, None, None)


class PoseNDF(PoseModel):
    def __init__(self, opt):
        super().__init__(opt, PARENT)
        self.batch_size = opt["train"]["batch_size"]
        # engine knob (no reference counterpart): arithmetic of the trunk -- "fp32" (exact fp32 MFMA), "f16x3" (fp16
        # hi/lo split, fp32 accumulate: fp32-class accuracy, same parity gates, ~3x the throughput), "auto" (default:
        # f16x3, or fp32 with a warning when a layer's weights are outside the split's operating range), "f16"
        # / "bf16" (reduced precision, ONE MFMA per product block: the measured comparison points of BASELINE.json configs[2] "fp32 vs
        # bf16", outside the 1e-4 parity bar, relu family only); opt["engine"]["precision"] or $PNDF_PRECISION
        self._precision = (opt.get("engine") or {}).get("precision") or os.environ.get("PNDF_PRECISION", "auto")
        # engine knob (no reference counterpart): "off" (default: the train=False gradient is once differentiable, a double backward
        # raises) or "hip" (it is differentiable once more, through pndf_second_order / its host twin; a third order raises)
        self._second_order_mode = (opt.get("engine") or {}).get("second_order", "off")
        if self._second_order_mode not in ("off", "hip"):
            raise ValueError(f"opt['engine']['second_order'] must be 'off' or 'hip', not {self._second_order_mode!r}")
        if self._second_order_mode == "hip" and self.enc is None:
            raise PndfError("opt['engine']['second_order'] = 'hip' needs the structure encoder (model.StrEnc.use: True)")
        self._so_engines = {}       # device index -> SecondOrderEngine
        self._so_params = None      # (the _param_list it was made from, the Parameters in state-dict order)
        self._so_workspaces = StreamWorkspaces(torch.float32)

    # ---- engine plumbing -----------------------------------------------------------------------
    def _new_engine(self, idx):
        # the plain-f16 / plain-bf16 comparison kernels are relu-family only; fp32 and f16x3 implement all three activations
        prec = "fp32" if (self._act == "softplus" and self._precision in ("f16", "bf16")) else self._precision
        eng = Engine(device=idx, precision="f16x3" if prec == "auto" else prec, **self._net_kw)
        if prec == "auto":      # a drop-in of an fp32 model picks an arithmetic on the caller's behalf: say so, once per engine
            logging.getLogger("posendf_amd").info(
                "PoseNDF on cuda:%s: precision 'auto' runs the split-precision kernels (f16x3: fp32 operands as fp16 hi + lo, "
                "three fp16 MFMAs per product block, fp32 accumulate; same parity gates as the exact kernel); "
                "opt['engine'] = {'precision': 'fp32'} or PNDF_PRECISION=fp32 selects the exact fp32 MFMA kernel", idx)
        return eng

    def _engine_after_refusal(self, eng, err):
        if self._precision != "auto" or eng.precision != "f16x3" or "operating" not in str(err):
            return None
        # both are HIP kernels: this is a choice of arithmetic, not a fallback off the engine
        warnings.warn(f"posendf_amd: {err}; precision 'auto' selects the exact fp32 kernel for this network")
        return Engine(device=eng.device, precision="fp32", **self._net_kw)

    def _engine_args(self, eng, device, B):
        return (stream_handle(device),)

    # ---- reference API -------------------------------------------------------------------------
    def forward(self, pose, dist_gt=None, man_poses=None, train=True, eikonal=0.0):
        pose = pose.to(device=self.device).reshape(-1, self.num_joints, 4)      # posendf.py:64
        if not train:
            fn = _Distance2 if self._second_order_mode == "hip" else _Distance
            return {"dist_pred": fn.apply(pose, self)}             # posendf.py:100-101
        return self._forward_train(pose, dist_gt, man_poses, eikonal)

    # ---- added surface (north_star: `.project` on the model) -------------------------------------
    def _ordered_parameters(self):
        """the live Parameters in state-dict order; the walk of the module tree is cached next to `_fingerprint`'s and rebuilt with it"""
        self._fingerprint()      # validates (or rebuilds) self._param_list by identity
        c = self._so_params
        if c is None or c[0] is None or c[0] is not self._param_list:
            named = dict(self.named_parameters())
            c = self._so_params = (self._param_list, [named[k] for k in state_dict_order(True, len(self._hidden) + 1)])
        return c[1]

    def _second_order(self, q, v, w_d, w_t, want=(True, True, True, True)):
        """pndf_second_order (cuda poses) or its host twin (cpu poses) -> (d [B], g [B,21,4], t [B], out [B,21,4]) in fp32, None
        where `want` is False.  q, v: [B,21,4]; w_d, w_t: [B] or None (0 and 1)."""
        def f32(x):
            return None if x is None else x.detach().to(device=q.device, dtype=torch.float32).contiguous()
        q = f32(q.reshape(-1, self.num_joints, 4))
        B = q.shape[0]
        v = f32(v.reshape(q.shape))
        w_d = f32(w_d if w_d is None else w_d.reshape(B))
        w_t = f32(w_t if w_t is None else w_t.reshape(B))
        shapes = ((B,), q.shape, (B,), q.shape)
        outs = [torch.empty(s, device=q.device, dtype=torch.float32) if w else None for s, w in zip(shapes, want)]
        ptr = [None if x is None or B == 0 else x.data_ptr() for x in (w_d, w_t, *outs)]
        if q.device.type == "cpu":
            self._engine_for(q.device).second_order(q.data_ptr(), v.data_ptr(), *ptr, B)
            return outs
        if q.device.type != "cuda":
            raise PndfError(f"the second order runs on the HIP engine (cuda) or the host twin (cpu), not on {q.device}")
        if self.enc is None:
            raise PndfError("the second order needs the structure encoder (model.StrEnc.use: True)")
        idx = device_index(q.device)
        eng = cached(self._so_engines, idx, lambda: SecondOrderEngine(device=idx, **self._net_kw))
        params = self._ordered_parameters()
        if any(p.device != q.device or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
            raise PndfError("the second order reads the parameters in place: contiguous fp32 on the pose's device")
        n = eng.workspace_floats(B)
        ws = self._so_workspaces.get(q.device, n)
        eng.second_order([p.data_ptr() for p in params], q.data_ptr(), v.data_ptr(), *ptr, B, ws.data_ptr() if n else None, ws.numel(),
                         stream_handle(q.device))
        return outs

    @torch.no_grad()
    def hvp(self, pose, v, w_d=None, w_t=None):
        """Distance, gradient and Hessian-vector product in one call (include/posendf_amd_second_order.h): for poses and
        directions [B,21,4] and per-pose weights w_d (default 0), w_t (default 1) returns (d [B,1], grad [B,21,4] = d d / d pose,
        t [B,1] = <v, grad>, out [B,21,4] = w_d grad + w_t H v) with H the Hessian of the distance in the pose, the weights of the
        network held constant.  Exact fp32 on the HIP engine for cuda poses, the host twin for a `train.device: cpu` model."""
        q = pose.to(device=self.device).reshape(-1, self.num_joints, 4)
        d, g, t, out = self._second_order(q, v, w_d, w_t)
        return d.view(-1, 1), g, t.view(-1, 1), out

    pack_observed = staticmethod(pack_observed)      # the model base's, shared with SkeletonPoseNDF.complete; num_joints defaults to 21

    @torch.no_grad()
    def complete(self, poses, observed, steps=100, return_dist=True, *, step_size=1.0, renormalize=None, tol=0.0):
        """Pose completion: `project` with the observed joints held.  `observed` is a bool tensor [21] (one mask for every pose) or
        [B,21], True = the joint's rotation is known and stays as it is, bit for bit; None = no joint is held, which is `project`
        bit for bit.  Each of the `steps` steps is one forward + gradient launch and one small masked update kernel on the
        caller's stream (include/posendf_amd_completion.h); a `train.device: cpu` model runs the host twin.  Returns and step options:
        as `project`."""
        q = poses.to(device=self.device).reshape(-1, self.num_joints, 4).float().contiguous()
        B = q.shape[0]
        out = torch.empty_like(q)
        d = torch.empty(B, device=q.device, dtype=torch.float32)
        mask = None if observed is None else self.pack_observed(observed, B, q.device, self.num_joints)
        eng = self._engine_for(q.device)
        ws = torch.empty(eng.complete_workspace_floats(B), device=q.device, dtype=torch.float32)
        eng.complete(q.data_ptr(), None if mask is None or B == 0 else mask.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps),
                     ws.data_ptr() if ws.numel() else None, stream_handle(q.device), step_size=step_size, renorm=renormalize, tol=tol)
        return (out, d.view(-1, 1)) if return_dist else out

    @torch.no_grad()
    def interpolate(self, pose_a, pose_b, frames, steps=100, smooth=0.0, mode="slerp", observed=None, return_dist=True, *, step_size=1.0,
                    renormalize="unit", tol=0.0):
        """Pose interpolation: a track of `frames` poses from every pose of `pose_a` to the matching pose of `pose_b` ([P,21,4]
        each), relaxed onto the manifold.  Frame 0 is `pose_a`, frame frames-1 is `pose_b` with every joint quaternion negated
        where that is the shorter way round; the frames between them start as the `mode` ("slerp" / "nlerp") interpolation of each
        joint and take `steps` steps of `complete` -- the two end frames and the `observed` joints held, bit for bit -- with a
        neighbour coupling of weight `smooth` in [0, 1] in the same step, which pulls every frame towards the mean of its two
        neighbours and keeps the track evenly spaced (smooth=0: the frames descend on their own, `complete` bit for bit).
        `observed`: bool [21], [frames,21] (one mask per frame, for every pair) or [P,frames,21].  One fill launch, then per step
        one forward + gradient launch and one band kernel on the caller's stream (include/posendf_amd_interpolation.h); a
        `train.device: cpu` model runs the host twin.  The inputs are not written.  Returns (track [P,frames,21,4], dist
        [P,frames] of the last iteration); step options: as `project`, with unit quaternions as the default."""
        J = self.num_joints
        a = pose_a.to(device=self.device).reshape(-1, J, 4).float().contiguous()
        b = pose_b.to(device=self.device).reshape(-1, J, 4).float().contiguous()
        P, T = a.shape[0], int(frames)
        if b.shape[0] != P:
            raise PndfError(f"pose_a holds {P} poses, pose_b {b.shape[0]}")
        if T < 2:
            raise PndfError(f"an interpolation has at least two frames, not {frames}")
        track = torch.empty((P, T, J, 4), device=a.device, dtype=torch.float32)
        d = torch.empty((P, T), device=a.device, dtype=torch.float32)
        mask = None
        if observed is not None:
            obs = torch.as_tensor(observed, device=a.device)
            if obs.dtype == torch.bool and obs.shape == (T, J):
                obs = obs.expand(P, T, J)
            if obs.dtype == torch.bool and obs.shape == (P, T, J):
                obs = obs.reshape(P * T, J)
            mask = self.pack_observed(obs, P * T, a.device, J)
        eng = self._engine_for(a.device)
        ws = torch.empty(eng.interpolate_workspace(P, T), device=a.device, dtype=torch.float32)
        eng.interpolate(a.data_ptr(), b.data_ptr(), None if mask is None or P == 0 else mask.data_ptr(), track.data_ptr(), d.data_ptr(), P, T,
                        int(steps), ws.data_ptr() if ws.numel() else None, stream_handle(a.device), mode=mode, smooth=smooth,
                        step_size=step_size, renorm=renormalize, tol=tol)
        return (track, d) if return_dist else track
