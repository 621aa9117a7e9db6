#!/usr/bin/env python3
"""Generate tests/golden/completion.npz by RUNNING THE REAL REFERENCE: the projection loop of experiments/sample_poses.py:67-74
with the step options of `project` restated around it (tests/golden/make_golden_project_options.py, whose stubs, imports, model
builder and step this file reuses) and, on top, the mask of pose completion: an observed joint keeps the bits it had
(include/posendf_amd_completion.h; DESIGN.md section 2 "Pose completion").

Needs the reference, like make_golden.py; nothing of the reference is copied into the repository, only inputs and outputs (data).
Usage:  python tests/golden/make_golden_completion.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_project_options as mgpo      # noqa: E402  (the reference's PoseNDF / gradient by path, ref_model, step_ref)

import completion_oracle as co                  # noqa: E402  (this repo: inputs, mask, weights and option sets only)

gradient = mgpo.gradient


def complete_ref(net, q0, observed, steps, step_size, renormalize, tol, snap_at=(1, 10)):
    held = torch.from_numpy(observed)[..., None]
    noisy = q0.clone()
    noisy.requires_grad = True
    trace, snaps = [], {}
    for it in range(steps):
        net_pred = net(noisy, train=False)
        grad = gradient(noisy, net_pred["dist_pred"]).reshape(-1, 84)
        cur = noisy.detach()
        moved = mgpo.step_ref(cur, net_pred["dist_pred"].detach()[:, 0], grad.detach(), step_size, renormalize, tol)
        noisy = torch.where(held, cur, moved).detach()
        noisy.requires_grad = True
        trace.append(net_pred["dist_pred"].detach()[:, 0].clone())
        if it + 1 in snap_at:
            snaps[it + 1] = noisy.detach().clone()
    return snaps, torch.stack(trace)


if __name__ == "__main__":
    torch.set_num_threads(8)
    q_np, mask = co.make_inputs(), co.make_mask()
    out = {"q": q_np, "observed": mask}
    for act in co.ACTS:
        nets = {tag: mgpo.ref_model(act, dt) for tag, dt in (("f32", torch.float32), ("f64", torch.float64))}
        out[f"tol_{act}"] = np.float32(co.options("unit_tol", act)["tol"])
        for name in co.OPTION_SETS:
            o = co.options(name, act)
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                snaps, trace = complete_ref(nets[tag], torch.from_numpy(q_np).to(dt), mask, co.STEPS, o["step_size"], o["renormalize"], o["tol"])
                for k, v in snaps.items():
                    out[f"{act}_{name}_q{k}_{tag}"] = v.numpy()
                out[f"{act}_{name}_dtrace_{tag}"] = trace.numpy()
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "completion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")
