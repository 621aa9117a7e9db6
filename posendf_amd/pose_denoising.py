"""Motion denoising for any joint tree, in quaternion space -- the reference's headline application (experiments/motion_denoise.py: a
pose prior, a temporal term and a data term that ties the result to the noisy observation) for a model that has no body model: a hand,
an animal rig, a `SkeletonPoseNDF`.  `MotionDenoise` (posendf_amd/motion_denoise.py) needs SMPL for its temporal and data terms; here
both live on the joint quaternions and inside the projection step: every step of `SkeletonPoseNDF.denoise` descends the distance field,
couples every frame to its neighbours and pulls every joint towards its observation (pndf_project_options4, include/posendf_amd.h), and a
clip is ONE engine call per outer iteration.

The outer iterations follow the direction of the reference's schedule (motion_denoise.py:29-35: the temporal weight grows, the data
weight falls): iteration `it` runs with the coupling min(1, smooth (1 + it)) and the data weight data / (1 + it), always anchored to the
ORIGINAL observation, starting from the result of the iteration before.

`python -m posendf_amd.pose_denoising` reads an .npz of quaternion tracks and writes the denoised ones.
"""
from __future__ import annotations

import torch

from .sample_poses import SamplePose


def second_difference(track: torch.Tensor) -> torch.Tensor:
    """track [P,T,J,4] -> [P]: the sum over the interior frames, joints and components of (q_k-1 - 2 q_k + q_k+1)^2 with the two
    neighbours negated where that is the shorter way round -- the jitter a temporal term removes; zeros for T < 3."""
    q = track[:, 1:-1]
    if q.shape[1] == 0:
        return track.new_zeros(track.shape[0])
    def near(n):
        return torch.where((q * n).sum(dim=-1, keepdim=True) < 0, -n, n)
    dd = near(track[:, :-2]) - 2.0 * q + near(track[:, 2:])
    return (dd * dd).sum(dim=(1, 2, 3))


class PoseDenoising(SamplePose):
    """PoseDenoising(posendf, body_model=None, device="cuda:0"): SamplePose's constructor, plus `denoise` for a model that has a
    `denoise` method (a SkeletonPoseNDF of any joint tree)"""

    @torch.no_grad()
    def denoise(self, track, conf=None, iterations=5, steps_per_iter=20, smooth=0.2, data=0.5, observed=None, free_ends=True, *, step_size=1.0,
                renormalize="unit", tol=0.0):
        """track: [P,T,J,4] or [T,J,4], the noisy clip; conf: per-joint confidences [J], [T,J] or [P,T,J] (None: ones; a joint with a
        confidence that is not positive takes no data term).  `iterations` engine calls of `steps_per_iter` steps each: iteration `it`
        starts from the result of the one before and runs with the coupling min(1, smooth (1 + it)) and the data weight
        data / (1 + it) towards the original observation.  The defaults (5 x 20 steps, smooth 0.2, data 0.5) are UNTUNED: no trained
        skeleton model exists to tune them on; they only have the direction of the reference's schedule.  Returns (track, dist of the
        last iteration's last step [P,T], history): history is a list of (coupling, data weight, mean dist) per iteration."""
        net = self.pose_prior
        if not hasattr(net, "denoise"):
            raise TypeError(f"{type(net).__name__} has no denoise(): motion denoising in quaternion space is SkeletonPoseNDF's; a PoseNDF "
                            "denoises through posendf_amd.motion_denoise.MotionDenoise and its body model")
        x = track.to(self.device).float()
        single = x.dim() == 3
        noisy = x.reshape((-1,) + tuple(x.shape[-3:])).contiguous()
        P, T = noisy.shape[0], noisy.shape[1]
        cur, dist, history = noisy, torch.zeros((P, T), device=noisy.device), []
        for it in range(int(iterations)):
            lam, mu = min(1.0, float(smooth) * (1 + it)), float(data) / (1 + it)
            cur, dist = net.denoise(cur, steps=int(steps_per_iter), smooth=lam, data=mu, conf=conf, observed=observed, free_ends=free_ends,
                                    step_size=step_size, renormalize=renormalize, tol=tol, anchor=noisy)
            history.append((lam, mu, float(dist.mean()) if dist.numel() else 0.0))
        if single:
            cur, dist = cur[0], dist[0]
        return cur, dist, history


def denoise_track_file(posendf, track_file, device="cuda:0", key="pose", conf_key="conf", **kwargs):
    """The quaternion tracks of an .npz -- `key` [T,J,4] or [P,T,J,4], and `conf_key` (if the file has it) [J], [T,J] or [P,T,J] -> what
    PoseDenoising.denoise returns for them."""
    import numpy as np
    with np.load(track_file) as f:
        track = torch.from_numpy(np.ascontiguousarray(f[key], dtype=np.float32))
        conf = torch.from_numpy(np.ascontiguousarray(f[conf_key], dtype=np.float32)) if conf_key in f.files else None
    return PoseDenoising(posendf, body_model=None, device=device).denoise(track, conf=conf, **kwargs)


def main(argv=None):
    import argparse

    from .config import load_config
    from .skeleton import SkeletonPoseNDF
    ap = argparse.ArgumentParser(description="Denoise quaternion tracks of any joint tree with a SkeletonPoseNDF (defaults untuned).")
    ap.add_argument("--config", "-c", required=True, help="path to the config file (configs/amass.yaml's keys, model.StrEnc.parent_mapping the tree)")
    ap.add_argument("--ckpt_path", "-ckpt", required=True, help="checkpoint of the trained model (key model_state_dict)")
    ap.add_argument("--track_file", "-tf", required=True, help=".npz with key pose [T,J,4] or [P,T,J,4] and optionally conf")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--steps_per_iter", type=int, default=20)
    ap.add_argument("--smooth", type=float, default=0.2, help="neighbour coupling of the first iteration, in [0, 1]")
    ap.add_argument("--data", type=float, default=0.5, help="data weight of the first iteration, in [0, 1]")
    ap.add_argument("--out", default=None, help="write the denoised tracks (key pose) and their distances (key dist) to this .npz")
    a = ap.parse_args(argv)
    opt = load_config(a.config)
    net = SkeletonPoseNDF(opt)
    net.load_state_dict(torch.load(a.ckpt_path, map_location="cpu")["model_state_dict"])
    net.eval()
    device = opt["train"]["device"]
    track, dist, history = denoise_track_file(net, a.track_file, device=device, iterations=a.iterations, steps_per_iter=a.steps_per_iter,
                                              smooth=a.smooth, data=a.data)
    for it, (lam, mu, mean) in enumerate(history):
        print(f"iteration {it}: coupling {lam:.3f}, data weight {mu:.3f}, mean dist {mean:.4f}")
    if a.out:
        import numpy as np
        np.savez(a.out, pose=track.cpu().numpy(), dist=dist.cpu().numpy())
    return track, dist


if __name__ == "__main__":
    main()
