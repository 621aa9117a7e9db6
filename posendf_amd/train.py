"""The training objective of `PoseNDF.forward(train=True)` / `SkeletonPoseNDF.forward(train=True)` on the HIP engine
(csrc/pndf_train.hip, `pndf_train_*` of include/posendf_amd.h, for another skeleton on a plan of
include/posendf_amd_skeleton_train.h): what `opt['engine']['train'] = 'hip'` routes a cuda model's training step to."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .engine import PndfError, stream_handle

LOSS_CODES = {"l1": 0, "l2": 1}


class TrainObjective(torch.autograd.Function):
    """(dist, man_loss, eikonal) of model/posendf.py:71-97 for noisy poses `pose` with labels `dist_gt` and manifold poses
    `man_poses`, as three 0-dim tensors from ONE forward call of the engine; backward gives every parameter its gradient -- the
    eikonal term's double backward included -- from ONE backward call, with the upstream gradients read on the device (no
    synchronisation).  `params` are the model's parameters in state-dict order, read in place (fp32, contiguous, on the poses'
    device).  Without `eikonal` only `dist` has a gradient, as in the reference's (loss, {'dist': loss}) branch.

    No gradient is returned for the poses, the labels or the manifold poses: the reference's trainer never reads one
    (model/train_posendf.py:92-99 steps the optimiser on the parameters only).  The workspace comes from the torch caching
    allocator and lives until backward."""

    @staticmethod
    def forward(ctx, engine, pose, dist_gt, man_poses, loss_type, eikonal, *params):
        dev = pose.device
        nq = 4 * engine.num_joints
        q = pose.detach().reshape(-1, nq).float().contiguous()
        gt = dist_gt.detach().reshape(-1).float().contiguous()
        qm = man_poses.detach().reshape(-1, nq).float().contiguous()
        B, Bm = q.shape[0], qm.shape[0]
        if gt.numel() != B:
            raise PndfError(f"{gt.numel()} labels for {B} poses")
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise PndfError(f"the HIP training objective takes contiguous fp32 parameters on {dev} (got {p.dtype} on {p.device})")
        ws = torch.empty(engine.workspace_floats(B, Bm, eikonal), dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        engine.forward([p.data_ptr() for p in params], q.data_ptr(), gt.data_ptr(), qm.data_ptr(), B, Bm, loss_type, eikonal,
                       losses.data_ptr(), ws.data_ptr(), stream_handle(dev))
        ctx.engine, ctx.ws = engine, ws
        ctx.save_for_backward(*params)
        return losses[0].clone(), losses[1].clone(), losses[2].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dist, g_man, g_eik):
        params = ctx.saved_tensors
        dev = params[0].device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        up = torch.stack([zero if g is None else g.reshape(()).float() for g in (g_dist, g_man, g_eik)]).contiguous()
        grads = [torch.empty_like(p) for p in params]
        ctx.engine.backward([p.data_ptr() for p in params], up.data_ptr(), [g.data_ptr() for g in grads], ctx.ws.data_ptr(),
                            stream_handle(dev))
        ctx.ws = None
        return (None,) * 6 + tuple(grads)
