"""Test helper (not a test module) for pose completion on other skeletons (pndf_project_options2 of include/posendf_amd.h; DESIGN.md
section 2j): the masked step in numpy -- tests/skeleton_oracle.py's `step` for the free joints and `np.where` on the joint mask for
the held ones --, the masks, the packed words, the option sets, the raw C structs of the refusal tests and the fp32 envelope of a
masked trajectory.  Shared by tests/test_skeleton_completion.py (host twin) and tests/test_skeleton_completion_gpu.py (HIP unit).

In float32 the masked step IS the specification both implementations are held to bit for bit."""
import ctypes

import numpy as np

import skeleton_oracle as sko
from conftest import d_rows, rel_err_rows

BAD_ARG, UNSUPPORTED = -1, -4
STEPS = 3
# the skeleton cases of the stated step: (skeleton, encoder)
CASES = [("hand", True), ("tree32", True), ("one", True), ("roots5", True), ("chain32", True), ("hand", False)]
ALL_FREE, ALL_HELD = 0, 1      # poses (rows of the mask) with no joint / every joint held


def make_mask(B, J, seed=5):
    """bool [B,J], True = held: about half of the joints of every pose; pose 0 has none held, pose 1 all of them; with 32 joints pose 2
    holds joint 31, the sign bit of a word read as int32"""
    m = np.random.RandomState(seed).rand(B, J) < 0.5
    m[ALL_FREE] = False
    m[ALL_HELD] = True
    if J == 32 and B > 2:
        m[2, 31] = True
    return np.ascontiguousarray(m)


def pack(mask):
    """bool [B,J] -> uint32 [B], bit j = joint j: the `observed` words of pndf_project_options2"""
    mask = np.asarray(mask, bool)
    J = mask.shape[1]
    return np.ascontiguousarray((mask.astype(np.uint64) << np.arange(J, dtype=np.uint64)).sum(axis=1).astype(np.uint32))


def option_sets(tol):
    """the three option sets of the stated step: the defaults; unit quaternions with a tolerance; flipped half steps with it"""
    return (dict(), dict(renormalize="unit", tol=tol), dict(renormalize="unit_flip", step_size=0.5, tol=tol))


def step_masked(q, d, g, mask, **opts):
    """one masked step on q [B,J,4] in q's dtype: held joints keep their bits, the others take skeleton_oracle.step"""
    J = mask.shape[1]
    q = q.reshape(-1, J, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        stepped = sko.step(q, d, g, J, opts.get("step_size", 1.0), opts.get("renormalize"), opts.get("tol", 0.0))
    return np.where(np.asarray(mask, bool)[..., None], q, stepped)


def rounds(forward_grad, q, mask, steps, **opts):
    """`steps` rounds of { forward_grad(q) -> (d [B], dq [B,J,4]) of the engine under test ; step_masked } -> (q_out, d of the last round)"""
    want, d = np.ascontiguousarray(q, np.float32).copy(), None
    for _ in range(steps):
        d, g = forward_grad(want)
        want = np.ascontiguousarray(step_masked(want, d, g, mask, **opts), np.float32)
    return want, d


def complete(q, sd, mask, steps, act, parents, dtype=np.float32, **opts):
    """free-running oracle: `steps` times skeleton_oracle.forward_grad + step_masked -> (q_out [B,J,4], d of the last iteration [B])"""
    J = len(parents)
    q = np.asarray(q, dtype=dtype).reshape(-1, J, 4)
    d = np.zeros((len(q), 1), dtype)
    for _ in range(steps):
        d, g = sko.forward_grad(q, sd, act, parents, dtype)
        q = step_masked(q, d, g, mask, **opts)
    return q, np.asarray(d).reshape(-1)


def traj_noise(q, sd, mask, steps, act, parents, draws=4, seed=1, **opts):
    """The fp32 envelope of a masked trajectory, as skeleton_oracle.fp32_noise is the envelope of one evaluation: per pose, the largest
    rel_err_rows (poses) and d_rows (last distance) against the fp64 oracle trajectory over `draws` fp32 oracle trajectories whose free
    joints start one fp32 rounding away (the held joints are not perturbed: they are data) -> (sigma_q [B], sigma_d [B], q64 [B,J,4],
    d64 [B])"""
    q = np.asarray(q, np.float32)
    q64, d64 = complete(q, sd, mask, steps, act, parents, np.float64, **opts)
    rng = np.random.default_rng(seed)
    sig_q, sig_d = [], []
    for _ in range(draws):
        qk = np.where(mask[..., None], q, (q * (1 + rng.uniform(-2.0 ** -23, 2.0 ** -23, q.shape))).astype(np.float32))
        q32, d32 = complete(qk, sd, mask, steps, act, parents, np.float32, **opts)
        sig_q.append(rel_err_rows(q32, q64))
        sig_d.append(d_rows(d32, d64))
    return np.max(sig_q, axis=0), np.max(sig_d, axis=0), q64, d64


def gate(out, d, q, sd, mask, steps, act, parents, what, **opts):
    """conftest.pose_gate (its calibrated factor 8 and floor 8e-6) on the poses and the last distance of a masked projection against
    the fp64 oracle trajectory, the envelope from `traj_noise`, the relu family's kink poses of `kink_exempt_along` exempt: the gate
    skeleton_oracle.gate applies to one evaluation, applied to `steps` of them"""
    from conftest import pose_gate
    sig_q, sig_d, q64, d64 = traj_noise(q, sd, mask, steps, act, parents, **opts)
    exempt = kink_exempt_along(q, sd, mask, steps, act, parents, **opts)
    pose_gate(d_rows(np.asarray(d).reshape(-1), d64), sig_d, f"{what} d", exempt=exempt)
    pose_gate(rel_err_rows(np.asarray(out), q64), sig_q, f"{what} q", exempt=exempt)


def kink_exempt_along(q, sd, mask, steps, act, parents, tol=1e-5, **opts):
    """relu family: the poses that come within `tol` of a kink at an iterate of their masked fp64 trajectory (skeleton_oracle.kink_exempt
    at every step); None for softplus"""
    J = len(parents)
    q = np.asarray(q, np.float64).reshape(-1, J, 4)
    ex = None
    for _ in range(steps):
        e = sko.kink_exempt(q, sd, act, parents, tol)
        if e is None:
            return None
        ex = e if ex is None else ex | e
        d, g = sko.forward_grad(q, sd, act, parents, np.float64)
        q = step_masked(q, d, g, mask, **opts)
    return ex


# ---------------------------------------------------------------- the C structs as a caller of the header writes them
def c_options(lib, step_size=1.0, renorm=0, tol=0.0, size=None):
    """a pndf_project_options (16 bytes) filled through pndf_default_project_options"""
    from posendf_amd.abi import ProjectOptions
    o = ProjectOptions()
    lib.pndf_default_project_options(ctypes.byref(o))
    o.step_size, o.renorm, o.tol = step_size, renorm, tol
    if size is not None:
        o.struct_size = size
    return o


def c_options2(lib, observed=None, step_size=1.0, renorm=0, tol=0.0, size=None, reserved=0):
    """a pndf_project_options2 (32 bytes) filled the documented way; `observed`: an address or None"""
    from posendf_amd.abi import ProjectOptions2
    o = ProjectOptions2()
    lib.pndf_default_project_options(ctypes.byref(o.base))
    o.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.base.step_size, o.base.renorm, o.base.tol = step_size, renorm, tol
    o.observed, o.reserved = observed, reserved
    return o


RENORM = {None: 0, "none": 0, "unit": 1, "unit_flip": 2}


def c_from(lib, opts, observed=None, large=True):
    """the struct of an option set of `option_sets`: the 32-byte one with the mask at `observed`, or the 16-byte one"""
    kw = dict(step_size=opts.get("step_size", 1.0), renorm=RENORM[opts.get("renormalize")], tol=opts.get("tol", 0.0))
    return c_options2(lib, observed, **kw) if large else c_options(lib, **kw)


# what a caller of the C header writes: the snippet of the documentation, as strict C99
C99_SNIPPET = """#include "posendf_amd_skeleton.h"
int main(void) {
    static const uint32_t mask[2] = {0u, 0x80000001u};
    pndf_project_options2 o;
    pndf_default_project_options(&o.base);
    o.base.struct_size = sizeof o;
    o.base.renorm = PNDF_RENORM_UNIT;
    o.observed = mask;
    o.reserved = 0;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 32) + (int)(sizeof(pndf_project_options) != 16);
}
"""
