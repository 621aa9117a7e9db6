#!/usr/bin/env python3
"""Generate tests/golden/second_order.npz by RUNNING THE REAL REFERENCE: the double backward of its `gradient()`
(model/posendf.py:18-27 asks for create_graph=True) with respect to the pose, and the unrolled projection loop of
experiments/sample_poses.py:67-74 with the graph kept (include/posendf_amd_second_order.h).

For poses q, directions v and per-pose weights w_d, w_t:  d, g = grad_q d, t = <v, g>, out = grad_q sum(w_d d + w_t t), in fp32 and
fp64, for lrelu, relu and softplus.  The unrolled loop: three steps q <- q - d grad with the graph kept, L = sum(q3 * w), dL/dq0, for
softplus and lrelu.  The generator asserts that every output is finite, that the fp64 H v equals a central difference of grad d, and
that <u, H v> = <v, H u>.

Needs the reference, like make_golden.py, whose stubs and imports it reuses through make_golden_project_options; nothing of the
reference is copied into the repository, only inputs and outputs (data).
Usage:  python tests/golden/make_golden_second_order.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_project_options as mgpo      # noqa: E402  (the reference's PoseNDF / gradient by path, ref_model)

import second_order_oracle as soo               # noqa: E402  (this repo: inputs and names only)

gradient = mgpo.gradient


def second_order_ref(net, q, v, w_d, w_t):
    """(d [B], g, t [B], out) of the reference's autograd in the dtype of q"""
    q = q.clone().requires_grad_(True)
    d = net(q, train=False)["dist_pred"]
    g = gradient(q, d)
    t = (v * g).sum(dim=(1, 2))
    (out,) = torch.autograd.grad((w_d * d[:, 0] + w_t * t).sum(), q)
    return d.detach()[:, 0], g.detach(), t.detach(), out.detach()


def grad_ref(net, q):
    q = q.clone().requires_grad_(True)
    return gradient(q, net(q, train=False)["dist_pred"]).detach()


def loop_ref(net, q0, w):
    """sample_poses.py:67-74, three steps, the graph kept: (q3, dL/dq0) for L = sum(q3 * w)"""
    q0 = q0.clone().requires_grad_(True)
    q = q0
    for _ in range(soo.LOOP_STEPS):
        pred = net(q, train=False)
        grad = gradient(q, pred["dist_pred"]).reshape(-1, 84)
        q = q - (pred["dist_pred"] * grad).reshape(-1, 21, 4)
    (g0,) = torch.autograd.grad((q * w).sum(), q0)
    return q.detach(), g0.detach()


if __name__ == "__main__":
    torch.set_num_threads(8)
    inp = soo.make_inputs()
    out = dict(inp)
    for act in soo.ACTS:
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            net = mgpo.ref_model(act, dt)
            q, v, u, w_d, w_t, w = (torch.from_numpy(inp[k]).to(dt) for k in ("q", "v", "u", "w_d", "w_t", "w"))
            res = second_order_ref(net, q, v, w_d, w_t)
            for name, val in zip(("d", "g", "t", "out"), res):
                assert torch.isfinite(val).all(), (act, tag, name)
                out[f"{act}_{name}_{tag}"] = val.numpy()
            if tag == "f64":
                one, zero = torch.ones_like(w_d), torch.zeros_like(w_d)
                hv = second_order_ref(net, q, v, zero, one)[3]
                hu = second_order_ref(net, q, u, zero, one)[3]
                eps = 1e-7
                fd = (grad_ref(net, q + eps * v) - grad_ref(net, q - eps * v)) / (2 * eps)
                e_fd = float((fd - hv).abs().max() / hv.abs().max())
                lhs, rhs = (u * hv).sum(dim=(1, 2)), (v * hu).sum(dim=(1, 2))
                e_sym = float((lhs - rhs).abs().max() / lhs.abs().max())
                print(f"[{act}] max |Hv| {float(hv.abs().max()):.3f}  central difference {e_fd:.1e}  symmetry {e_sym:.1e}")
                assert e_fd <= 1e-6 and e_sym <= 1e-10, (act, e_fd, e_sym)
            if act in soo.LOOP_ACTS:
                q3, g0 = loop_ref(net, q, w)
                assert torch.isfinite(q3).all() and torch.isfinite(g0).all(), (act, tag)
                out[f"loop_{act}_q3_{tag}"] = q3.numpy()
                out[f"loop_{act}_grad_{tag}"] = g0.numpy()
    out["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(soo.FIXTURE, **out)
    print(soo.FIXTURE, os.path.getsize(soo.FIXTURE) // 1024, "KiB")
