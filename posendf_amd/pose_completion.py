"""Pose completion -- the application of the paper that follows pose generation: some of a pose's joint rotations are observed, the
others are occluded or missing, and plausible values for them are found by descending the distance field while the observed joints
stay put.  Modelled on `SamplePose` (posendf_amd/sample_poses.py): the loop is the model's `complete` -- `PoseNDF.complete` for the 21
SMPL joints (per step one forward + gradient launch and one masked update kernel, include/posendf_amd_completion.h),
`SkeletonPoseNDF.complete` for any other joint tree of 1 .. 32 joints, a hand or a rig (the mask inside the projection step,
pndf_project_options2 of include/posendf_amd.h) -- and with a body model the poses before / after are turned into meshes for
inspection.  The body model is SMPL's: a model of another joint count completes poses without one.

The distance field has many local minima around a partial observation, so the usual recipe is several hypotheses per pose: the
unobserved joints are filled with random unit quaternions (the convention of `random_poses`), every hypothesis is completed, and
the one that ends nearest to the manifold is kept.  The fill and the selection happen once per call and are torch ops; all
B * K poses go through ONE `complete` call of the model.
"""
from __future__ import annotations

import torch

from .sample_poses import SamplePose


def best_hypothesis(dist: torch.Tensor) -> torch.Tensor:
    """[B,K] distances -> [B] index of the smallest one per pose; a NaN is never chosen (a row of NaNs gives 0), ties go to the
    lower index."""
    nan = torch.isnan(dist)
    d = torch.where(nan, torch.full_like(dist, float("inf")), dist)
    K = d.shape[1]
    idx = torch.arange(K, device=d.device).expand_as(d)
    hit = (d == d.min(dim=1, keepdim=True).values) & ~nan
    first = torch.where(hit, idx, torch.full_like(idx, K)).min(dim=1).values
    return torch.where(first == K, torch.zeros_like(first), first)


class PoseCompletion(SamplePose):
    """PoseCompletion(posendf, body_model=None, device="cuda:0"): SamplePose's constructor and mesh helper, plus `complete`"""

    @torch.no_grad()
    def complete(self, poses, observed, hypotheses=1, fill="random", select="all", generator=None, steps=100, *, step_size=1.0,
                 renormalize=None, tol=0.0):
        """poses [B,J,4] with J = the model's num_joints (21 for PoseNDF); observed: bool [J] or [B,J], True = the joint is known
        (None: no joint is).  `hypotheses` = K starts per pose.  fill="random": the unobserved joints of every hypothesis are
        normalize(torch.rand(B,K,J,4), dim=-1), drawn on the host from `generator` -- whatever the input holds there (NaN
        included) is ignored; fill="given": every hypothesis starts from the input as it is.  `steps` and the step options are
        those of the model's `complete`.

        Returns (poses [B,K,J,4], dist [B,K] of the last iteration, meshes); with select="best" (poses, dist, best [B], meshes),
        where best[b] is the hypothesis with the smallest distance (`best_hypothesis`).  With a body model, meshes holds
        'pose_init' / 'vertices_init' and 'pose' / 'vertices' / 'joints' of the B * K poses before and after (of the B best ones
        with select="best"); without one it is empty."""
        if fill not in ("random", "given"):
            raise ValueError(f"fill must be 'random' or 'given', not {fill!r}")
        if select not in ("all", "best"):
            raise ValueError(f"select must be 'all' or 'best', not {select!r}")
        K = int(hypotheses)
        if K < 1:
            raise ValueError(f"hypotheses must be at least 1, not {hypotheses}")
        J = self.pose_prior.num_joints
        if self.body_model is not None and J != 21:
            raise ValueError(f"the body model takes SMPL's 21 joints; a model of {J} joints completes poses without one (body_model=None)")
        q = poses.to(self.device).reshape(-1, J, 4).float()
        B = q.shape[0]
        obs = torch.zeros(B, J, dtype=torch.bool, device=q.device) if observed is None else torch.as_tensor(observed, device=q.device)
        if obs.dtype != torch.bool or obs.shape not in ((J,), (B, J)):
            raise ValueError(f"observed must be a bool tensor of shape [{J}] or [{B}, {J}]")
        obs = obs.expand(B, J)
        start = q[:, None].expand(B, K, J, 4)
        if fill == "random":
            rand = torch.nn.functional.normalize(torch.rand((B, K, J, 4), generator=generator), dim=-1).to(q.device)
            start = torch.where(obs[:, None, :, None], start, rand)
        start = start.reshape(B * K, J, 4).contiguous()
        mask = obs[:, None].expand(B, K, J).reshape(B * K, J)
        out, dist = self.pose_prior.complete(start, mask, steps=steps, step_size=step_size, renormalize=renormalize, tol=tol)
        out, dist = out.view(B, K, J, 4), dist.view(B, K)
        start = start.view(B, K, J, 4)
        best = best_hypothesis(dist) if select == "best" else None
        meshes = {}
        if self.body_model is not None:
            pick = (lambda x: x.reshape(B * K, J, 4)) if best is None else (lambda x: x[torch.arange(B, device=x.device), best])
            meshes["pose_init"], meshes["vertices_init"], _ = self._mesh(pick(start))
            meshes["pose"], meshes["vertices"], meshes["joints"] = self._mesh(pick(out))
        return (out, dist, meshes) if best is None else (out, dist, best, meshes)
