#!/usr/bin/env python3
"""Generate tests/golden/interpolation.npz by RUNNING THE REAL REFERENCE: its PoseNDF and `gradient` (imported by path through
tests/golden/make_golden_project_options.py, whose stubs, model builder and step this file reuses) with the fill and the band step
of pose interpolation restated around them in torch (include/posendf_amd_interpolation.h; DESIGN.md section 2 "Pose
interpolation").  The reference's own experiments/interpolation.py stops after loading the model, so there is no loop of its to
restate: what the reference contributes is the distance and its gradient at every iterate.

fp32 and fp64, ten steps, every option set crossed with the couplings 0 and 0.5.  To stay within the size of a committed fixture
only the INTERIOR frames are stored (the end frames are the inputs, held bit for bit): the slerp fill, the track after step 10 in
both precisions, after step 1 in fp64 for the coupling 0.5 (with no coupling the first step is the completion step), and the d
trace of the interior frames.

Needs the reference, like make_golden.py; nothing of the reference is copied into the repository, only inputs and outputs (data).
Usage:  python tests/golden/make_golden_interpolation.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_project_options as mgpo      # noqa: E402  (the reference's PoseNDF / gradient by path, ref_model, step_ref)

import interpolation_oracle as io               # noqa: E402  (this repo: inputs, weights and option sets only)

gradient = mgpo.gradient


def dot4(x, y):
    return ((x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]) + x[..., 3] * y[..., 3]


def align_ref(q, n):
    return torch.where((dot4(q, n) < 0)[..., None], -n, n)


def unit_ref(u):
    return u / torch.clamp_min(torch.sqrt(dot4(u, u)), 1e-12)[..., None]


def fill_ref(a, b, T):
    """the slerp fill, statement by statement, in the dtype of a"""
    bp = align_ref(a, b)
    dm, dp = a - bp, a + bp
    theta = 2 * torch.atan2(torch.sqrt(dot4(dm, dm)), torch.sqrt(dot4(dp, dp)))
    sn = torch.sin(theta)
    ok = sn > 0
    den = torch.where(ok, sn, torch.ones_like(sn))
    frames = [a]
    for k in range(1, T - 1):
        t = torch.tensor(k, dtype=a.dtype) / torch.tensor(T - 1, dtype=a.dtype)
        wa = torch.where(ok, torch.sin((1 - t) * theta) / den, 1 - t)[..., None]
        wb = torch.where(ok, torch.sin(t * theta) / den, t)[..., None]
        frames.append(unit_ref(wa * a + wb * bp))
    frames.append(bp)
    return torch.stack(frames, dim=1)


def band_step_ref(q, d, grad, smooth, step_size, renormalize, tol):
    """one band step on the track q [P,T,21,4]: mgpo.step_ref with the coupling between its update and its renormalisation"""
    Q = q[:, 1:-1]
    dist = d.reshape(q.shape[0], q.shape[1], 1, 1)[:, 1:-1]
    u = Q - step_size * (dist * grad.reshape(q.shape)[:, 1:-1])
    if smooth > 0:
        h = 0.5 * (align_ref(Q, q[:, :-2]) + align_ref(Q, q[:, 2:]))
        u = u + smooth * (h - Q)
    if renormalize is not None:
        u = unit_ref(u)
        if renormalize == "unit_flip":
            u = torch.where(u[..., :1] < 0, -u, u)
    if tol > 0:
        u = torch.where(dist < tol, Q, u)
    return torch.cat([q[:, :1], u, q[:, -1:]], dim=1)


def relax_ref(net, track, steps, smooth, step_size, renormalize, tol, snap_at=(1, 10)):
    cur = track.clone()
    trace, snaps = [], {}
    for it in range(steps):
        noisy = cur.reshape(-1, 21, 4).clone()
        noisy.requires_grad = True
        net_pred = net(noisy, train=False)
        grad = gradient(noisy, net_pred["dist_pred"]).reshape(-1, 84)
        d = net_pred["dist_pred"].detach()[:, 0]
        cur = band_step_ref(cur, d, grad.detach(), smooth, step_size, renormalize, tol).detach()
        trace.append(d.clone())
        if it + 1 in snap_at:
            snaps[it + 1] = cur.clone()
    return snaps, torch.stack(trace)


if __name__ == "__main__":
    torch.set_num_threads(8)
    a_np, b_np = io.make_pairs()
    P, T = io.P, io.T
    out = {"a": a_np, "b": b_np, "frames": np.int32(T)}
    dts = (("f32", torch.float32), ("f64", torch.float64))
    inner = lambda x: np.ascontiguousarray(x.numpy()[:, 1:-1])      # noqa: E731
    for tag, dt in dts:
        out[f"fill_{tag}"] = inner(fill_ref(torch.from_numpy(a_np).to(dt), torch.from_numpy(b_np).to(dt), T))
    for act in io.ACTS:
        nets = {tag: mgpo.ref_model(act, dt) for tag, dt in dts}
        out[f"tol_{act}"] = np.float32(io.options("unit_tol", act)["tol"])
        for name in io.OPTION_SETS:
            o = io.options(name, act)
            for smooth in io.SMOOTHS:
                key = f"{act}_{name}_s{int(smooth * 10)}"
                for tag, dt in dts:
                    track = fill_ref(torch.from_numpy(a_np).to(dt), torch.from_numpy(b_np).to(dt), T)
                    snaps, trace = relax_ref(nets[tag], track, io.STEPS, smooth, o["step_size"], o["renormalize"], o["tol"])
                    out[f"{key}_q10_{tag}"] = inner(snaps[10])
                    if tag == "f64" and smooth > 0:
                        out[f"{key}_q1_{tag}"] = inner(snaps[1])
                    out[f"{key}_dtrace_{tag}"] = np.ascontiguousarray(trace.numpy().reshape(io.STEPS, P, T)[:, :, 1:-1])
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "interpolation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")
