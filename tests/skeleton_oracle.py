"""Test helper (not a test module) for the skeleton unit (include/posendf_amd_skeleton.h): the numpy restatement of
the first-order path for ANY parent table -- forward, forward + gradient, projection --, its fp32 noise envelope, the kink exemption
of the relu family, and the cases and fixtures of tests/test_skeleton.py and tests/test_skeleton_gpu.py.

The activations and the trunk are oracle.posendf_np's (pinned against the reference by tests/test_oracle.py); the normalisation over
the joint axis, the encoder along the parent table and their reverse are restated here with the table as an argument, and pinned
twice: on the SMPL table against oracle.posendf_np, on the fixtures against the reference's own autograd
(tests/golden/make_golden_skeleton.py).  The projection step is tests/project_options_oracle.py's, reshaped to J joints."""
import os

import numpy as np

import project_options_oracle as poo
from conftest import d_rows, rel_err_rows
from oracle import posendf_np as onp
from posendf_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAND = (-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13)
# 32 joints: joint 0 has three children (1, 2, 3); 1-4-5-6-7-8-9 is a chain of depth 7 below it; further branches and a second root
TREE32 = (-1, 0, 0, 0, 1, 4, 5, 6, 7, 8, 2, 10, 10, 3, 13, 14, 14, 9, 9, 11, 12, 15, 16, -1, 23, 24, 24, 25, 26, 27, 28, 29)
CHAIN32 = tuple(range(-1, 31))
ROOTS5 = (-1,) * 5
ONE = (-1,)
SKELETONS = {"hand": HAND, "tree32": TREE32, "one": ONE, "roots5": ROOTS5, "chain32": CHAIN32}
FIXTURE_CASES = [(s, a) for s in ("hand", "tree32") for a in ("lrelu", "softplus")]
HIDDEN = (64, 48)
NPOSE = 48
STEPS = 3


def fixture_path(skel, act):
    return os.path.join(GOLDEN, f"skeleton_{skel}_{act}.npz")


def network(parents, seed, encoder=True, hidden=HIDDEN, gain=2.0, out_bias=0.1):
    """synthetic weights of a DFNet behind the skeleton `parents`"""
    return synth.make_weights(seed, gain, out_bias, dims=synth.skeleton_dims(parents, hidden, encoder), parents=tuple(parents))


def poses(parents, n=NPOSE, seed=21):
    return synth.make_poses(n, seed=seed, num_joints=len(parents))


# ---------------------------------------------------------------- the arithmetic
def _encoder(n, sd, parents, act, beta):
    """net_modules.py:140-170 along `parents`: features [B, 6 J] and the pre-activations of every bone"""
    dt = n.dtype
    feats, cache = [], []
    for j, p in enumerate(parents):
        inp = n[:, j, :] if p == -1 else np.concatenate([n[:, j, :], feats[p]], axis=-1)
        z1 = inp @ np.asarray(sd[f"enc.net.{j}.net.0.weight"], dt).T + np.asarray(sd[f"enc.net.{j}.net.0.bias"], dt)
        z2 = onp._act(z1, act, beta) @ np.asarray(sd[f"enc.net.{j}.net.2.weight"], dt).T + np.asarray(sd[f"enc.net.{j}.net.2.bias"], dt)
        feats.append(onp._act(z2, act, beta))
        cache.append((z1, z2))
    return np.concatenate(feats, axis=-1), cache


def _run(q, sd, act, parents, dtype, grad_out=None, want_grad=True):
    J = len(parents)
    q = np.asarray(q, dtype=dtype).reshape(-1, J, 4)
    act, beta, eact, ebeta = onp.parse_act(act)
    norm = np.sqrt((q * q).sum(axis=1, keepdims=True))      # F.normalize(pose, dim=1): over the joints, per component
    den = np.maximum(norm, dtype(1e-12))
    n = q / den
    enc = onp.has_encoder(sd)
    f, cache = _encoder(n, sd, parents, eact, ebeta) if enc else (n.reshape(len(n), -1), None)
    d, zs = onp.dfnet_forward(f, sd, act, beta, keep=True)
    # oracle.posendf_np.kink_margin: the smallest |pre-activation| of a relu-family unit relative to the largest of its layer
    margin = np.full(len(q), np.inf)
    kinked = list(zs[:-1] if act != "softplus" else ()) + [z for pair in (cache if enc and eact != "softplus" else ()) for z in pair]
    for z in kinked:
        margin = np.minimum(margin, np.abs(z).min(axis=1) / np.maximum(np.abs(z).max(axis=1), 1e-300))
    if not want_grad:
        return d, None, margin, None
    g = np.ones_like(d) if grad_out is None else np.asarray(grad_out, dtype=dtype).reshape(-1, 1)
    g = g * onp._dact(zs[-1], onp._out_kind(act), beta)
    for l in range(len(zs) - 1, -1, -1):
        g = g @ np.asarray(sd[f"dfnet.lin{l}.weight"], dtype)
        if l > 0:
            g = g * onp._dact(zs[l - 1], act, beta)
    if enc:
        gf = [g[:, 6 * j:6 * j + 6].copy() for j in range(J)]
        gn = np.zeros_like(n)
        for j in range(J - 1, -1, -1):      # children before parents
            z1, z2 = cache[j]
            gz2 = gf[j] * onp._dact(z2, eact, ebeta)
            gz1 = (gz2 @ np.asarray(sd[f"enc.net.{j}.net.2.weight"], dtype)) * onp._dact(z1, eact, ebeta)
            gin = gz1 @ np.asarray(sd[f"enc.net.{j}.net.0.weight"], dtype)
            gn[:, j, :] = gin[:, :4]
            if parents[j] != -1:
                gf[parents[j]] = gf[parents[j]] + gin[:, 4:]
    else:
        gn = g.reshape(n.shape)
    live = norm > dtype(1e-12)
    dot = (gn * q).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = np.where(live, q * dot / (den * den * np.where(live, norm, 1)), 0)
    return d, gn / den - corr, margin, np.abs(gn / den).reshape(len(q), -1).max(axis=1)


def forward(q, sd, act, parents, dtype=np.float32):
    """dist_pred [B,1]"""
    return _run(q, sd, act, parents, dtype, want_grad=False)[0]


def forward_grad(q, sd, act, parents, dtype=np.float32, grad_out=None):
    """(d [B,1], dq [B,J,4]) with dq = grad_out * d d / d q"""
    return _run(q, sd, act, parents, dtype, grad_out)[:2]


def step(q, d, g, J, step_size=1.0, renormalize=None, tol=0.0):
    """The stated step of tests/project_options_oracle.py for J joints.  poo.step sees [*, 21, 4] with one d per row: feed it one row per joint quaternion, padded to 21 quaternions with copies"""
    dt = q.dtype
    qj = np.ascontiguousarray(q, dt).reshape(-1, 1, 4)
    gj = np.ascontiguousarray(g, dt).reshape(-1, 1, 4)
    dj = np.repeat(np.asarray(d, dt).reshape(-1), J)
    out = poo.step(np.repeat(qj, 21, axis=1), dj, np.repeat(gj, 21, axis=1), step_size, renormalize, tol)
    return np.ascontiguousarray(out[:, 0, :]).reshape(-1, J, 4)


def project(q, sd, steps, act, parents, dtype=np.float32, **opts):
    """free-running oracle: `steps` times forward_grad + step -> (q_out [B,J,4], d of the last iteration [B])"""
    J = len(parents)
    q = np.asarray(q, dtype=dtype).reshape(-1, J, 4)
    d = np.zeros((len(q), 1), dtype)
    for _ in range(steps):
        d, g = forward_grad(q, sd, act, parents, dtype)
        q = step(q, d, g, J, opts.get("step_size", 1.0), opts.get("renormalize"), opts.get("tol", 0.0))
    return q, np.asarray(d).reshape(-1)


# ---------------------------------------------------------------- the gates' inputs
_MEMO = {}


def grad_rows(a, b, parents, scale):
    """The per-pose error of a gradient: conftest.rel_err_rows -- except for ONE joint.  There normalize(q, dim=1) runs over a joint
    axis of length one, x = sign(q) is piecewise constant and the true gradient is exactly zero: dq = g_x / s - q (g_x . q) / s^3 is
    the difference of two equal terms.  The fp64 run returns its own rounding noise (1e-17), and an error relative to that noise
    measures nothing (the fp32 oracle itself is 1e8 "wrong").  What fp32 can hold there is the cancellation to the rounding of the
    terms that cancel, so the error is taken relative to `scale` = max |g_x / s| of the pose (fp64 run): the same quantity
    rel_err_rows divides by wherever the gradient is not a cancellation."""
    if len(parents) > 1:
        return rel_err_rows(a, b)
    a, b = np.asarray(a, np.float64).reshape(len(scale), -1), np.asarray(b, np.float64).reshape(len(scale), -1)
    return np.abs(a - b).max(axis=1) / np.maximum(scale, 1e-30)


def fp32_noise(q, sd, act, parents, draws=8, seed=1):
    """conftest._fp32_noise for a parent table: per pose, the largest error against the fp64 run over `draws` fp32 evaluations whose
    inputs are perturbed by one fp32 rounding, in the metrics of d_rows / rel_err_rows (grad_rows) -> (sigma_d, sigma_g, d64, g64,
    scale of grad_rows)"""
    key = (np.asarray(q, np.float32).tobytes(), tuple(parents), act, draws, seed, tuple((k, np.asarray(v).tobytes()) for k, v in sorted(sd.items())))
    key = hash(key)
    if key not in _MEMO:
        q = np.asarray(q, dtype=np.float32)
        d64, g64, _, scale = _run(q, sd, act, parents, np.float64)
        rng = np.random.default_rng(seed)
        sig_d, sig_g = [], []
        for _ in range(draws):
            qk = (q * (1 + rng.uniform(-2.0 ** -23, 2.0 ** -23, q.shape))).astype(np.float32)
            d32, g32 = forward_grad(qk, sd, act, parents, np.float32)
            sig_d.append(d_rows(d32, d64))
            sig_g.append(grad_rows(g32, g64, parents, scale))
        _MEMO[key] = (np.max(sig_d, axis=0), np.max(sig_g, axis=0), d64, g64, scale)
    return _MEMO[key]


def kink_exempt(q, sd, act, parents, tol=1e-5):
    """relu family: poses with a pre-activation within `tol` of 0 (relative to its layer's largest) in the fp64 run, where the derivative may legitimately flip (what
    tests/test_depth.py kink_exempt is for the SMPL table); None for softplus"""
    if onp.act_family(act) in ("softplus", "softplus/softplus"):
        return None
    return _run(q, sd, act, parents, np.float64)[2] < tol


def gate(d, dq, q, sd, act, parents, what):
    """the two pose gates every implementation is held to: conftest.pose_gate with its calibrated defaults (factor 8, floor 8e-6)"""
    from conftest import pose_gate
    sig_d, sig_g, d64, g64, scale = fp32_noise(q, sd, act, parents)
    pose_gate(d_rows(np.asarray(d).reshape(-1), d64), sig_d, f"{what} d")
    pose_gate(grad_rows(np.asarray(dq).reshape(len(d64), -1), g64.reshape(len(d64), -1), parents, scale), sig_g, f"{what} dq",
              exempt=kink_exempt(q, sd, act, parents))


# the cases of the host-twin and device tests: (skeleton, encoder); 6 J = 6, 30, 90, 192 (and 4 J without the encoder)
CASES = [("hand", True), ("tree32", True), ("one", True), ("roots5", True), ("chain32", True), ("hand", False), ("tree32", False)]
CASE_ACTS = ("lrelu", "softplus")


def case_id(c):
    return f"{c[0]}{'' if c[1] else '-noenc'}"


def clipped(d, act):
    """the number of poses whose output pre-activation is not positive: d == 0 behind the output ReLU; behind Softplus(beta 100), which
    never returns 0, d <= softplus(0) = ln 2 / 100 (a stricter count than d == 0)"""
    return int((np.asarray(d) <= (np.log(2.0) / 100.0 if act == "softplus" else 0.0)).sum())


def case_poses(case, n=NPOSE):
    """the poses of a case: the fixture's (synth.make_poses, components in [0, 1)); for one joint signed ones -- normalising over a
    joint axis of length one leaves the signs only, and unsigned poses would all be the same input"""
    parents = SKELETONS[case[0]]
    return synth.make_poses(n, seed=21, signed=len(parents) == 1, num_joints=len(parents))


def case_network(case, act):
    """(parents, weights) of a case: the fixture's seed for a fixture case with the encoder; elsewhere the first seed from 7 on that
    leaves at most a quarter of the case's poses clipped in the fp64 oracle and, so that a tolerance can part them, gives them more
    than one distance (the rule of tests/golden/make_golden_skeleton.py)"""
    skel, enc = case
    parents = SKELETONS[skel]
    if enc and (skel, act) in FIXTURE_CASES:
        return parents, network(parents, int(np.load(fixture_path(skel, act))["seed"]), encoder=enc)
    q = case_poses(case)
    for seed in range(7, 71):
        sd = network(parents, seed, encoder=enc)
        d = forward(q, sd, act, parents, np.float64).reshape(-1)
        if clipped(d, act) * 4 <= len(q) and float(np.median(d)) > float(d.min()):
            return parents, sd
    raise AssertionError(f"no seed keeps {case_id(case)} {act} off d == 0")
