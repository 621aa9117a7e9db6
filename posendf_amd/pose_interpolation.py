"""Pose interpolation -- the fifth application of the paper: a plausible motion between two key poses.  The in-betweens start as a
quaternion interpolation of every joint and are relaxed onto the pose manifold as ONE track: the two key poses stay as they are,
every other frame descends the distance field while a neighbour-coupling term keeps the frames evenly spaced.  Modelled on
`PoseCompletion` (posendf_amd/pose_completion.py): the loop is `PoseNDF.interpolate` (one fill launch, then per step one forward +
gradient launch and one band kernel, include/posendf_amd_interpolation.h), and with a body model the track before / after is turned
into meshes for inspection.

The reference's experiments/interpolation.py stops after it has loaded the model; `main()` takes that script's arguments and does
what its last comment announces: read `pose_body` from a motion file, convert axis-angle to quaternions, interpolate between the
first and the last frame.
"""
from __future__ import annotations

import torch

from .sample_poses import SamplePose


def segment_lengths(track: torch.Tensor) -> torch.Tensor:
    """track [P,T,J,4] (any joint count) -> [P,T-1]: the length of every segment of the track in radians, the sum over the joints of the rotation
    angle between consecutive frames, 2 acos(min(|<q_k, q_k+1>|, 1)) (the sign of a quaternion does not matter)."""
    dots = (track[:, :-1] * track[:, 1:]).sum(dim=-1).abs().clamp(max=1.0)
    return (2.0 * torch.acos(dots)).sum(dim=-1)


class PoseInterpolation(SamplePose):
    """PoseInterpolation(posendf, body_model=None, device="cuda:0"): SamplePose's constructor and mesh helper, plus `interpolate`"""

    @torch.no_grad()
    def interpolate(self, pose_a, pose_b, frames, steps=100, smooth=0.5, mode="slerp", observed=None, *, step_size=1.0, renormalize="unit",
                    tol=0.0):
        """pose_a, pose_b: [J,4] or [P,J,4] for the model's J joints (21 for a PoseNDF, the tree's for a SkeletonPoseNDF, which has no
        body model: its meshes are empty); every argument is the model's `interpolate`'s (smooth defaults to the coupling that keeps
        a track even).  Returns (track [P,frames,J,4], dist [P,frames] of the last iteration, meshes).  With a body model, meshes
        holds 'pose_init' / 'vertices_init' of the filled track (steps = 0) and 'pose' / 'vertices' / 'joints' of the relaxed one,
        P * frames rows each; without one it is empty."""
        J = self.pose_prior.num_joints
        if self.body_model is not None and J != 21:
            raise ValueError(f"the body model takes SMPL's 21 joints; a model of {J} joints interpolates without one (body_model=None)")
        a = pose_a.to(self.device).reshape(-1, J, 4).float()
        b = pose_b.to(self.device).reshape(-1, J, 4).float()
        kw = dict(mode=mode, observed=observed, step_size=step_size, renormalize=renormalize, tol=tol)
        track, dist = self.pose_prior.interpolate(a, b, frames, steps=steps, smooth=smooth, **kw)
        meshes = {}
        if self.body_model is not None:
            start = self.pose_prior.interpolate(a, b, frames, steps=0, smooth=smooth, return_dist=False, **kw)
            meshes["pose_init"], meshes["vertices_init"], _ = self._mesh(start.reshape(-1, J, 4))
            meshes["pose"], meshes["vertices"], meshes["joints"] = self._mesh(track.reshape(-1, J, 4))
        return track, dist, meshes


def interpolate_motion_file(posendf, pose_file, frames=16, device="cuda:0", body_model=None, **kwargs):
    """The first and the last frame of the motion file's `pose_body` ([N,63] or [N,69] axis-angle) as key poses -> what
    PoseInterpolation.interpolate returns for them.  On a HIP device the conversion to quaternions is pndf_aa2quat; the host twin
    of the engine has none, so a cpu model converts with motion_denoise.axis_angle_to_quaternion."""
    from .motion_denoise import axis_angle_to_quaternion, load_motion_npz
    theta = load_motion_npz(pose_file, device)[[0, -1]].contiguous()
    if theta.device.type == "cuda":
        from .engine import aa2quat, stream_handle
        keys = torch.empty((2, 21, 4), device=theta.device, dtype=torch.float32)
        aa2quat(theta.data_ptr(), keys.data_ptr(), 2, stream_handle(theta.device))
    else:
        keys = axis_angle_to_quaternion(theta.view(2, 23, 3)[:, :21])
    return PoseInterpolation(posendf, body_model=body_model, device=device).interpolate(keys[0], keys[1], frames, **kwargs)


def main(argv=None):
    import argparse

    from .config import load_config
    from .facade import PoseNDF
    ap = argparse.ArgumentParser(description="Interpolate between the first and the last pose of a motion file using PoseNDF.")
    ap.add_argument("--config", "-c", required=True, help="path to the config file (configs/amass.yaml's keys)")
    ap.add_argument("--ckpt_path", "-ckpt", required=True, help="checkpoint of the trained model (key model_state_dict)")
    ap.add_argument("--pose_file", "-pf", required=True, help=".npz motion file with key pose_body")
    ap.add_argument("--frames", type=int, default=16, help="frames of the track, key poses included")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--smooth", type=float, default=0.5, help="neighbour coupling in [0, 1]")
    ap.add_argument("--out", default=None, help="write the track (key pose) and its distances (key dist) to this .npz")
    a = ap.parse_args(argv)
    opt = load_config(a.config)
    net = PoseNDF(opt)
    net.load_state_dict(torch.load(a.ckpt_path, map_location="cpu")["model_state_dict"])
    net.eval()
    device = opt["train"]["device"]
    track, dist, _ = interpolate_motion_file(net, a.pose_file, frames=a.frames, device=device, steps=a.steps, smooth=a.smooth)
    seg = segment_lengths(track)[0]
    print(f"{a.frames} frames: dist of the interior frames mean {float(dist[0, 1:-1].mean()):.4f}, "
          f"path {float(seg.sum()):.3f} rad, longest / mean segment {float(seg.max() / seg.mean()):.3f}")
    if a.out:
        import numpy as np
        np.savez(a.out, pose=track[0].cpu().numpy(), dist=dist[0].cpu().numpy())
    return track, dist


if __name__ == "__main__":
    main()
