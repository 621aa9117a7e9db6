#!/usr/bin/env python3
"""Generate tests/golden/project_options.npz by RUNNING THE REAL REFERENCE: the projection loop of
experiments/sample_poses.py:67-74 (as tests/golden/make_golden.py:project_ref restates it around the imported PoseNDF +
gradient) with the step options of `project` restated around it -- step size, unit-quaternion steps, stop tolerance
(include/posendf_amd.h pndf_project_options; DESIGN.md section 1 "The projection step").

Needs the reference, like make_golden.py, whose stub modules and imports it reuses; the same `synth` weights in regime "live"; nothing of
the reference is copied into the repository, only inputs and outputs (data).
Usage:  python tests/golden/make_golden_project_options.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                         # noqa: E402  (the stubs, the reference's PoseNDF / gradient / load_config by path)

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
import project_options_oracle as poo            # noqa: E402  (this repo: inputs, weights and option sets only)

PoseNDF, gradient, load_config, REF = mg.PoseNDF, mg.gradient, mg.load_config, mg.REF
assert poo.REGIME == mg.REGIMES["live"]

STEPS = 10


def ref_model(act, dtype):
    opt = load_config(os.path.join(REF, "configs", "amass.yaml"))
    opt["train"]["device"] = "cpu"
    opt["model"]["DFNet"]["act"] = act
    opt["model"]["StrEnc"]["act"] = act
    net = PoseNDF(opt)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in poo.weights().items()})
    net.eval()
    return net.to(dtype)


def step_ref(q, d, grad, step_size, renormalize, tol):
    """the step, statement by statement, in the dtype of q (torch rounds every operation on its own)"""
    p = d.reshape(-1, 1, 1) * grad.reshape(-1, 21, 4)
    s = step_size * p
    u = q - s
    if renormalize is not None:
        ss = ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]) + u[..., 3] * u[..., 3]
        n = torch.sqrt(ss)
        u = u / torch.clamp_min(n, 1e-12)[..., None]
        if renormalize == "unit_flip":
            u = torch.where(u[..., :1] < 0, -u, u)
    if tol > 0:
        u = torch.where(d.reshape(-1, 1, 1) < tol, q, u)
    return u


def project_ref(net, q0, steps, step_size, renormalize, tol, snap_at=(1, 10)):
    noisy = q0.clone()
    noisy.requires_grad = True
    trace, snaps = [], {}
    for it in range(steps):
        net_pred = net(noisy, train=False)
        grad = gradient(noisy, net_pred["dist_pred"]).reshape(-1, 84)
        noisy = step_ref(noisy.detach(), net_pred["dist_pred"].detach()[:, 0], grad.detach(), step_size, renormalize, tol).detach()
        noisy.requires_grad = True
        trace.append(net_pred["dist_pred"].detach()[:, 0].clone())
        if it + 1 in snap_at:
            snaps[it + 1] = noisy.detach().clone()
    return snaps, torch.stack(trace)


if __name__ == "__main__":
    torch.set_num_threads(8)
    q_np = poo.make_inputs()
    out = {"q": q_np}
    for act in poo.ACTS:
        nets = {tag: ref_model(act, dt) for tag, dt in (("f32", torch.float32), ("f64", torch.float64))}
        q32 = torch.from_numpy(q_np)
        d0 = nets["f32"](q32, train=False)["dist_pred"].detach()[:, 0].numpy()
        tol = np.float32(np.median(d0))      # about half of the poses start below it and never move
        out[f"tol_{act}"] = tol
        for name, (step_size, renorm) in poo.OPTION_SETS.items():
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                snaps, trace = project_ref(nets[tag], torch.from_numpy(q_np).to(dt), STEPS, step_size, renorm,
                                           float(tol) if name == "unit_tol" else 0.0)
                for k, v in snaps.items():
                    out[f"{act}_{name}_q{k}_{tag}"] = v.numpy()
                out[f"{act}_{name}_dtrace_{tag}"] = trace.numpy()
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "project_options.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB", {a: float(out[f"tol_{a}"]) for a in poo.ACTS})
