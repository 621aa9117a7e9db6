"""Test helper (not a test module) for the root's trajectory over the frames of a track inside the projection step
(pndf_project_options9 of include/posendf_amd.h; DESIGN.md section 2j "Root trajectory"): the numpy restatement of csrc/pndf_fk.h's
pndf_fk_root_smooth_step -- the descent, the neighbour coupling with its alignment, the data term towards the anchor and the Jacobi
buffer discipline -- operation for operation, on top of tests/skeleton_views_oracle.py's several-camera term,
tests/skeleton_length_oracle.py's scaled tree and scales' step, tests/skeleton_image_oracle.py's camera term and
tests/skeleton_keypoints_oracle.py's fitting step; the raw C struct; the runner that drives pndf_skel_project or pndf_project_ex_cpu with
it.  Shared by tests/test_skeleton_root.py (host twin) and tests/test_skeleton_root_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `root_smooth_step` in float32 IS the
specification both implementations are held to bit for bit; the same code in float64 is the truth of the effect."""
import ctypes

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
import skeleton_views_oracle as sv

BAD_ARG = sk.BAD_ARG
P = 3
FRAMES = (2, 3, 5)      # both frames are ends; one interior frame; three
NU = sk.NU
LAM_ROT, LAM_TRANS = 0.375, 0.25
MU_ROT, MU_TRANS = 0.125, 0.0625
PARTS = {"rotation": ((si.NU_ROT, 0.0), (LAM_ROT, 0.0), (MU_ROT, 0.0)),
         "translation": ((0.0, si.NU_TRANS), (0.0, LAM_TRANS), (0.0, MU_TRANS)),
         "both": ((si.NU_ROT, si.NU_TRANS), (LAM_ROT, LAM_TRANS), (MU_ROT, MU_TRANS))}      # root_weights, root_smooth, root_data
TERMS = ("camera", "scales", "views2")
flat, pack, ptr, assert_same, same_bytes = sk.flat, sk.pack, sk.ptr, sk.assert_same, si.same_bytes
lengths = sl.lengths


# ---------------------------------------------------------------- csrc/pndf_fk.h's root step, operation for operation
def quat_dot(a, b):
    """((a0 b0 + a1 b1) + a2 b2) + a3 b3 per row"""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]


def align(c, n):
    """n negated where its dot product with c is negative (a NaN dot product does not flip)"""
    with np.errstate(all="ignore"):
        return np.where((quat_dot(c, n) < 0)[:, None], -n, n)


def root_smooth_step(root, groot, nu_rot, nu_trans, d, tol=0.0, frames=0, root_smooth=(0.0, 0.0), anchor=None, root_data=(0.0, 0.0)):
    """pndf_fk_root_smooth_step for every pose, in root's dtype.  root [B,7] is the step's INPUT for every frame (Jacobi: the result is a
    new array, frame k reads rows k - 1 and k + 1 of `root`); frames: T, or 0 (no tracks: no neighbours).  A pose that rests under tol
    keeps its root; a part whose nu is zero keeps its bits and reads nothing."""
    root = np.asarray(root)
    dt = root.dtype.type
    f32 = lambda v: dt(np.float32(v))  # noqa: E731
    Bn = len(root)
    out = root.copy()
    k = np.arange(Bn) % frames if frames else np.zeros(Bn, int)
    has_m = (k > 0) if frames else np.zeros(Bn, bool)
    has_p = (k < frames - 1) if frames else np.zeros(Bn, bool)
    interior, end = has_m & has_p, has_m ^ has_p
    prev, nxt = np.roll(root, 1, axis=0), np.roll(root, -1, axis=0)
    one = np.where(has_m[:, None], prev, nxt)      # an end frame's one neighbour
    lam_r, lam_t = root_smooth
    mu_r, mu_t = root_data
    A = None if anchor is None else np.asarray(anchor, root.dtype)
    with np.errstate(all="ignore"):
        if nu_rot > 0:
            c = root[:, :4]
            u = c - f32(nu_rot) * groot[:, :4]
            if lam_r > 0:
                both = u + f32(lam_r) * ((dt(0.5) * (align(c, prev[:, :4]) + align(c, nxt[:, :4]))) - c)
                single = u + f32(lam_r) * (dt(0.5) * (align(c, one[:, :4]) - c))
                u = np.where(interior[:, None], both, np.where(end[:, None], single, u))
            if mu_r > 0:
                u = u + f32(mu_r) * (align(c, A[:, :4]) - c)
            ch, _ = sk.fk_unit(u)
            out[:, :4] = np.stack(ch, axis=-1)
        if nu_trans > 0:
            s = root[:, 4:]
            u = s - f32(nu_trans) * groot[:, 4:]
            if lam_t > 0:
                both = u + f32(lam_t) * ((dt(0.5) * (prev[:, 4:] + nxt[:, 4:])) - s)
                single = u + f32(lam_t) * (dt(0.5) * (one[:, 4:] - s))
                u = np.where(interior[:, None], both, np.where(end[:, None], single, u))
            if mu_t > 0:
                u = u + f32(mu_t) * (A[:, 4:] - s)
            out[:, 4:] = u
        if tol > 0:
            rests = np.asarray(d, root.dtype).reshape(-1) < dt(tol)
            out = np.where(rests[:, None], root, out)
    assert out.dtype == root.dtype
    return out


def one_step(q, d, g, parents, kp, cam, views, rt, root_weights, sg, ln, group_frames, nu, root_frames, root_smooth, root_anchor, root_data, **kw):
    """one step of the statement at the track q [P,T,J,4] in q's dtype: (q', E, root', scales' or None).  The term is the several-camera
    one with `views`, the scaled one with scales `sg`, the camera term otherwise -- the kernel's choice."""
    dt = q.dtype
    Bn = q.shape[0] * q.shape[1]
    G, n = sl.groups_of(Bn, group_frames, ln["per_pose"])
    fq = q.reshape((-1,) + q.shape[2:])
    sigma = None if sg is None else np.repeat(sg, n, axis=0)
    h = None
    if views is not None:
        E, gk, gr, h = sv.views_energy_grad(fq, parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), rt, cam["rho"], views, sigma)
    elif sg is not None:
        E, gk, gr, h = sl.len_energy_grad(fq, parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), rt, cam, sigma)
    else:
        E, gk, gr = si.camera_energy_grad(fq, parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), rt, cam)
    tol = kw.get("tol", 0.0)
    out = sk.fit_step(q, d, g, gk, nu, **kw)
    if rt is not None and any(root_weights):
        rt = root_smooth_step(rt, gr, root_weights[0], root_weights[1], d, tol, root_frames, root_smooth, root_anchor, root_data)
    if sg is not None and ln["nu_len"] > 0:
        S = sg.shape[1]
        dd = np.asarray(d, dt).reshape(G, n)
        rests = (dd < dt.type(tol)).all(axis=1) if tol > 0 else np.zeros(G, bool)
        rate = np.ones(S, np.float32) if ln["rate"] is None else ln["rate"]
        sg = sl.len_step(sg, sl.group_sum(h.reshape(G, n, S)), n, ln["nu_len"], rate, ln["kappa"], ln["clamp"], rests)
    return out, E, rt, sg


def rounds(forward_grad, track, steps, parents, kp, cam, views=None, ln=None, root=None, root_weights=(0.0, 0.0), nu=NU, frames=None,
           root_smooth=(0.0, 0.0), root_anchor=None, root_data=(0.0, 0.0), **kw):
    """`steps` rounds of { forward_grad of the engine under test ; the float32 restatement } -> (track, d, E of the last round, root, scales).
    The roots are ping-ponged between two arrays as the implementations do: the step's input is never written."""
    ln = ln or lengths(None)
    cur = np.ascontiguousarray(track, np.float32).copy()
    bufs = [None if root is None else np.ascontiguousarray(root, np.float32).copy(), None]
    sg = None if ln["scale"] is None else ln["scale"].copy()
    frames_ = track.shape[1] if frames is None else frames
    d = np.zeros(track.shape[0] * track.shape[1], np.float32)
    E = np.zeros_like(d)
    for s in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        src = bufs[s & 1]
        kept = None if src is None else src.copy()
        cur, E, bufs[(s + 1) & 1], sg = one_step(cur, d, g, parents, kp, cam, views, src, root_weights, sg, ln, frames_, nu, frames_, root_smooth,
                                                  root_anchor, root_data, frames=frames, **kw)
        assert src is None or src.tobytes() == kept.tobytes()      # Jacobi: the input buffer is untouched
        cur = np.ascontiguousarray(cur, np.float32)
    return cur, d, E, bufs[steps & 1], sg


def relax(track, sd, steps, act, parents, kp, cam, views=None, root=None, root_weights=(0.0, 0.0), nu=NU, dtype=np.float64, frames=None,
          root_smooth=(0.0, 0.0), root_anchor=None, root_data=(0.0, 0.0), **kw):
    """the free-running restatement in `dtype` (float64: the truth of the effect) -> (track, E of every step [steps,B], root)"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    rt = None if root is None else np.asarray(root, dtype)
    frames_ = q.shape[1] if frames is None else frames
    Es = []
    ln = lengths(None)
    for _ in range(steps):
        d, g, _, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        q, E, rt, _ = one_step(q, d, g, parents, kp, cam, views, rt, root_weights, None, ln, frames_, nu, frames_, root_smooth, root_anchor, root_data,
                               frames=frames, **kw)
        Es.append(E)
    return q, np.stack(Es), rt


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options9(lib, base8, root_anchor=None, lambda_rot=0.0, lambda_trans=0.0, mu_rot=0.0, mu_trans=0.0, reserved5=0, size=None):
    """a pndf_project_options9 (256 bytes) around a filled ProjectOptions8; root_anchor: an address or None"""
    from posendf_amd.abi import ProjectOptions9
    o = ProjectOptions9()
    o.base8 = base8
    o.base8.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.root_anchor = root_anchor
    o.lambda_rot, o.lambda_trans, o.mu_rot, o.mu_trans, o.reserved5 = lambda_rot, lambda_trans, mu_rot, mu_trans, reserved5
    return o


C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float pixels[4 * 3 * 2] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static float placement[4 * 7] = {1, 0, 0, 0, 0, 0, 5};
    static const float seen[4 * 7] = {1, 0, 0, 0, 0, 0, 5};
    pndf_project_options9 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base8.base7.base6.base5.base4.base3.base2.base);
    o.base8.base7.base6.base5.base4.base3.base2.base.struct_size = sizeof o;
    o.base8.base7.base6.base5.base4.base3.frames = 4;
    o.base8.base7.base6.base5.kp_target = pixels;
    o.base8.base7.base6.base5.rest = rest;
    o.base8.base7.base6.base5.kp_joint = joint;
    o.base8.base7.base6.base5.n_keypoints = 3;
    o.base8.base7.base6.base5.nu = 0.1f;
    o.base8.base7.base6.root = placement;
    o.base8.base7.base6.nu_trans = 0.1f;
    o.base8.base7.base6.fx = o.base8.base7.base6.fy = 500.f;
    o.base8.base7.base6.kp_flags = PNDF_KP_IMAGE;
    o.root_anchor = seen;
    o.lambda_trans = 0.5f;
    o.mu_trans = 0.25f;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 256) + (int)(sizeof(pndf_project_options8) != 224);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class RootRunner:
    """mixed in front of a ViewsRunner: `run` with the 256-byte struct.  -> (status, q_out, d_last, kp_energy, root after the call or None,
    scales after the call or None).  `root_anchor` [n,7] is placed where the poses live."""

    def run9(self, q, steps, kp, root_smooth=(0.0, 0.0), root_anchor=None, root_data=(0.0, 0.0), views=None, make9=None, **kw):
        held = None if root_anchor is None else self.place(np.ascontiguousarray(root_anchor, np.float32))
        table = None if views is None else np.ascontiguousarray(views, np.float32)

        def make8(at, o7):
            at = dict(at, root_anchor=None if held is None else self.addr(held))
            o8 = sv.c_options8(self.lib, o7, ptr(table), 0 if table is None else len(table))
            if make9 is not None:
                return make9(at, o8)
            return c_options9(self.lib, o8, at["root_anchor"], root_smooth[0], root_smooth[1], root_data[0], root_data[1])
        out = self.run8(q, steps, kp, views=views, make8=make8, **kw)
        if held is not None:
            assert self.fetch(held).tobytes() == np.ascontiguousarray(root_anchor, np.float32).tobytes()      # the anchor is never written
        return out

    def fit9(self, q, steps, kp, **kw):
        rc, out, d, E, rt, sg = self.run9(q, steps, kp, **kw)
        assert rc == 0, self.last_error()
        return out, d, E, rt, sg


# ---------------------------------------------------------------- fixtures
def term_inputs(case, term, n, frames, conf=True):
    """(kp, views or None, ln, cam) of a term on n poses in tracks of `frames`: "camera" the one camera of a pndf_project_options6,
    "scales" the same with one row of scales per track, "views2" / "views8" that many cameras and scales, "views2_plain" two cameras and
    no scales (bone_scale == NULL)"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    if term.startswith("views"):
        views = sv.make_views(int(term[5:].split("_")[0]))
        _, kp = sv.case_kp(case, views, n, conf=conf)
        cam = si.cam_of(True, si.RHO, sv.UNREAD_CAMERA)
    else:
        views = None
        _, kp, _ = si.case_kp(case, n, image=True, conf=conf)
        cam = si.cam_of(True, si.RHO)
    ln = lengths(None)
    if term != "camera" and not term.endswith("_plain"):
        S = J + len(kp["kpj"])
        G, _ = sl.groups_of(n, frames, False)
        ln = lengths(sl.make_scales(G, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S))
    return kp, views, ln, cam


def make_anchor(root, seed=53):
    """[n,7] float32: the roots with noise, half of the rotations negated (the alignment has work to do)"""
    r = np.random.RandomState(seed)
    a = np.asarray(root, np.float64) + 0.05 * r.randn(*np.shape(root))
    a[::2, :4] *= -1.0
    return np.ascontiguousarray(a, np.float32)


def check_stated_step(run, case, term, step_counts=(0, 1, 2, 3)):
    """rounds of the runner's own forward_grad + the float32 restatement equal the call with the 256-byte struct, bit for bit: poses, d_last,
    kp_energy, root and bone_scale -- T = 2, 3 and 5, rotation only / translation only / both, with and without the anchor, and every
    step count (both parities of the root buffer)"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    moved = 0
    for T in FRAMES:
        n = P * T
        track = sdo.clip(case, P, T)
        kp, views, ln, cam = term_inputs(case, term, n, T)
        root = si.make_roots(n, 37)
        anchor = make_anchor(root)
        words = pack(sdo.make_mask(J, P, T))
        tol = float(np.median(run.forward(flat(track))))
        for i, (part, (weights, lam, mu)) in enumerate(sorted(PARTS.items())):
            for use_anchor in (False, True):
                name = sorted(sk.OPTION_SETS)[(i + use_anchor) % len(sk.OPTION_SETS)]
                opts = sk.options(name, tol)
                rkw = dict(root_smooth=lam, root_anchor=anchor if use_anchor else None, root_data=mu if use_anchor else (0.0, 0.0))
                for steps in step_counts:
                    what = (term, T, part, use_anchor, name, steps)
                    want, dk, Ek, rk, sk_ = rounds(run.forward_grad, track, steps, parents, kp, cam, views, ln, root, weights, observed=sdo.make_mask(J, P, T),
                                                   free_ends=True, smooth=sk.LAMBDA, **rkw, **opts)
                    got, dl, El, rl, sg = run.fit9(flat(track), steps, kp, opts=opts, words=words, frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, views=views,
                                                   cam=cam, rho=si.RHO, root=root, root_weights=weights, ln=ln, **rkw)
                    assert_same(got.reshape(track.shape), want, what)
                    assert_same(dl, dk, what + ("d_last",))
                    assert_same(El, Ek, what + ("kp_energy",))
                    same_bytes(rl, rk, what + ("root",))
                    if ln["scale"] is not None:
                        assert_same(sg, sk_, what + ("bone_scale",))
                    if steps:
                        moved += int((rl != root).any())
                    else:
                        assert rl.tobytes() == root.tobytes(), what
    assert moved


def check_anchor_without_tracks(run, case, term):
    """frames == 0: no neighbours, the data term towards the anchor alone -- the stated step bit for bit, for 1, 2 and 3 steps"""
    parents = sko.SKELETONS[case[0]]
    n = 10
    track = sdo.clip(case, 2, 5)
    kp, views, ln, cam = term_inputs(case, term, n, 0)
    root = si.make_roots(n, 37)
    anchor = make_anchor(root)
    weights = (si.NU_ROT, si.NU_TRANS)
    opts = dict(step_size=0.5, renormalize="unit", tol=0.0)
    for steps in (1, 2, 3):
        want, dk, Ek, rk, sk_ = rounds(run.forward_grad, track, steps, parents, kp, cam, views, ln, root, weights, frames=0, root_anchor=anchor,
                                       root_data=(MU_ROT, MU_TRANS), **opts)
        got, dl, El, rl, sg = run.fit9(flat(track), steps, kp, opts=opts, views=views, cam=cam, rho=si.RHO, root=root, root_weights=weights, ln=ln,
                                       root_anchor=anchor, root_data=(MU_ROT, MU_TRANS))
        assert_same(got.reshape(track.shape), want, (term, steps))
        assert_same(dl, dk, (term, steps, "d_last"))
        assert_same(El, Ek, (term, steps, "kp_energy"))
        same_bytes(rl, rk, (term, steps, "root"))
        if ln["scale"] is not None:
            assert_same(sg, sk_, (term, steps, "bone_scale"))
        assert (rl != root).any()


def check_reductions(run, case, term):
    """lambda = 0 and no anchor: the 224-byte call's bytes.  nu = 0: the 72-byte call's bytes, root and anchor full of NaN neither read nor
    written.  steps == 0: root untouched.  All roots of a track equal and no anchor: the values of the uncoupled step (array_equal: adding
    +0.0 may change the sign of a zero)."""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    T = 5
    n = P * T
    track = sdo.clip(case, P, T)
    q = flat(track)
    kp, views, ln, cam = term_inputs(case, term, n, T)
    root = si.make_roots(n, 37)
    weights = (si.NU_ROT, si.NU_TRANS)
    kw = dict(opts=dict(renormalize="unit", step_size=0.5), words=pack(sdo.make_mask(J, P, T)), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, cam=cam,
              rho=si.RHO, ln=ln)
    for steps in (1, 2, 3):
        want = run.fit8(q, steps, kp, views=views, root=root, root_weights=weights, **kw)
        got = run.fit9(q, steps, kp, views=views, root=root, root_weights=weights, **kw)
        for a, b, part in zip(got, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
            same_bytes(a, b, (term, steps, "lambda 0", part))
    # all roots of a track equal: the coupling adds exact zeros
    same = np.repeat(root[::T], T, axis=0)
    one = run.fit9(q, 1, kp, views=views, root=same, root_weights=weights, root_smooth=(LAM_ROT, LAM_TRANS), **kw)
    ref = run.fit8(q, 1, kp, views=views, root=same, root_weights=weights, **kw)
    for a, b in zip(one, ref):
        assert (a is None and b is None) or np.array_equal(a, b), (term, "equal roots")
    # nu = 0: nothing of the root or the anchor is read or written
    want4, d4, _ = run.fit(q, 2, small=True, opts=kw["opts"], words=kw["words"], frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS)
    nan_root, nan_anchor = np.full((n, 7), np.nan, np.float32), np.full((n, 7), np.nan, np.float32)
    got, d, E, rt, _ = run.fit9(q, 2, kp, views=views, nu=0.0, root=nan_root, root_weights=weights, root_smooth=(LAM_ROT, LAM_TRANS),
                                root_anchor=nan_anchor, root_data=(MU_ROT, MU_TRANS), **kw)
    assert got.tobytes() == want4.tobytes() and d.tobytes() == d4.tobytes() and not E.any() and rt.tobytes() == nan_root.tobytes()
    # steps == 0
    got = run.fit9(q, 0, kp, views=views, root=root, root_weights=weights, root_smooth=(LAM_ROT, LAM_TRANS), **kw)
    assert got[3].tobytes() == root.tobytes() and got[0].tobytes() == q.tobytes()


def check_locality(run, case, term):
    """a NaN in one track's root stays in that track; a NaN anchor whose mu is 0 is never read; a part with nu == 0 keeps its bits"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    T = 5
    n = P * T
    track = sdo.clip(case, P, T)
    q = flat(track)
    kp, views, ln, cam = term_inputs(case, term, n, T, conf=False)
    root = si.make_roots(n, 37)
    kw = dict(opts=dict(renormalize="unit"), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, cam=cam, rho=si.RHO, ln=ln, views=views)
    both = dict(root_weights=(si.NU_ROT, si.NU_TRANS), root_smooth=(LAM_ROT, LAM_TRANS))
    clean = run.fit9(q, 3, kp, root=root, **both, **kw)
    assert np.isfinite(clean[3]).all()
    bad = root.copy()
    bad[T + 2] = np.nan      # a frame of track 1
    got = run.fit9(q, 3, kp, root=bad, **both, **kw)
    for tr in (0, 2):
        rows = slice(tr * T, (tr + 1) * T)
        assert got[3][rows].tobytes() == clean[3][rows].tobytes() and got[0][rows].tobytes() == clean[0][rows].tobytes(), (term, tr)
    assert np.isnan(got[3][T:2 * T]).all()      # three Jacobi steps carry it to every frame of a track of five ... from its middle
    # the anchor of a part whose mu is 0 is not read: NaN there changes nothing
    anchor = make_anchor(root)
    half = anchor.copy()
    half[:, 4:] = np.nan
    a = run.fit9(q, 2, kp, root=root, root_anchor=anchor, root_data=(MU_ROT, 0.0), **both, **kw)
    b = run.fit9(q, 2, kp, root=root, root_anchor=half, root_data=(MU_ROT, 0.0), **both, **kw)
    assert a[3].tobytes() == b[3].tobytes() and np.isfinite(b[3]).all()
    # a part whose nu is 0 keeps its bits (and reads neither neighbours nor anchor)
    turned = anchor.copy()
    turned[:, :4] = np.nan
    got = run.fit9(q, 3, kp, root=root, root_weights=(0.0, si.NU_TRANS), root_smooth=(0.0, LAM_TRANS), root_anchor=turned, root_data=(0.0, MU_TRANS), **kw)
    assert np.isfinite(got[3]).all()
    assert got[3][:, :4].tobytes() == root[:, :4].tobytes() and (got[3][:, 4:] != root[:, 4:]).any()
    got = run.fit9(q, 3, kp, root=root, root_weights=(si.NU_ROT, 0.0), root_smooth=(LAM_ROT, 0.0), **kw)
    assert got[3][:, 4:].tobytes() == root[:, 4:].tobytes() and (got[3][:, :4] != root[:, :4]).any()


def check_refusals(run, sizes=(241, 248, 255, 257, 264)):
    """every refusal of pndf_project_options9 names its field and writes nothing"""
    case = ("hand", True)
    parents = sko.SKELETONS["hand"]
    J = len(parents)
    T = 5
    n = P * T
    q = flat(sdo.clip(case, P, T))
    kp, views, ln, cam = term_inputs(case, "camera", n, T, conf=False)
    root = si.make_roots(n, 37)
    anchor = make_anchor(root)
    nan = float("nan")

    def refused(field, frames=T, weights=(si.NU_ROT, si.NU_TRANS), with_root=True, use_anchor=True, o8=None, **f):
        def make9(at, base8):
            g = dict(root_anchor=at["root_anchor"], lambda_rot=LAM_ROT if frames else 0.0, lambda_trans=LAM_TRANS if frames else 0.0, mu_rot=MU_ROT,
                     mu_trans=MU_TRANS)
            g.update({k: (v(at) if callable(v) else v) for k, v in f.items()})
            if o8 is not None:
                base8 = o8(at, base8)
            return c_options9(run.lib, base8, **g)
        rc, out, d, E, rt, _ = run.run9(q, 2, kp, root_anchor=anchor if use_anchor else None, root=root if with_root else None, root_weights=weights,
                                        frames=frames, lam=sk.LAMBDA if frames else 0.0, flags=sdo.FREE_ENDS if frames else 0, cam=cam, make9=make9)
        assert rc == BAD_ARG, (field, f, rc)
        assert field.encode() in run.last_error(), (field, run.last_error())
        assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(E == 7.0), field
        assert rt is None or rt.tobytes() == root.tobytes(), field

    for size in sizes:
        refused("struct_size", size=size)
    refused("reserved5", reserved5=1)
    refused("reserved5", reserved5=1 << 40)
    for name in ("lambda_rot", "lambda_trans", "mu_rot", "mu_trans"):
        for v in (-0.125, 1.5, nan):
            refused(name, **{name: v})
    refused("lambda_rot", frames=0, lambda_rot=LAM_ROT)
    refused("lambda_trans", frames=0, lambda_trans=LAM_TRANS)
    refused("lambda_rot", weights=(0.0, si.NU_TRANS), mu_rot=0.0)
    refused("mu_rot", weights=(0.0, si.NU_TRANS), lambda_rot=0.0)
    refused("lambda_trans", weights=(si.NU_ROT, 0.0), mu_trans=0.0)
    refused("mu_trans", weights=(si.NU_ROT, 0.0), lambda_trans=0.0)
    refused("root", with_root=False, weights=(0.0, 0.0), o8=lambda at, b8: (setattr(b8.base7.base6, "nu_rot", si.NU_ROT), setattr(b8.base7.base6, "nu_trans", si.NU_TRANS), b8)[2])
    refused("root_anchor", use_anchor=False)
    refused("root_anchor", mu_rot=0.0, mu_trans=0.0)
    for odd in (1, 2, 3):
        refused("root_anchor", root_anchor=lambda at, odd=odd: at["root_anchor"] + odd)
    refused("root_anchor", root_anchor=lambda at: at["root"])
    refused("root_anchor", root_anchor=lambda at: at["root"] + 4 * (n * 7 - 1))
    refused("root_anchor", root_anchor=lambda at: at["out"])
    refused("root_anchor", root_anchor=lambda at: at["out"] - 4 * (n * 7 - 1))
    # whatever base8 refuses
    refused("reserved4", o8=lambda at, b8: (setattr(b8, "reserved4", 1), b8)[1])
    # (a nu that is NaN or negative is base6's refusal, with base6's text, whatever the lambdas say)
    refused("pndf_project_options6.nu_rot must be finite", o8=lambda at, b8: (setattr(b8.base7.base6, "nu_rot", nan), b8)[1])
    refused("pndf_project_options6.nu_trans must be finite", o8=lambda at, b8: (setattr(b8.base7.base6, "nu_trans", -1.0), b8)[1])


# ---------------------------------------------------------------- the effect, on the float64 restatement alone
EFFECT = dict(T=24, steps=150, noise=1.5, lam=(0.0, 0.5), weights=(0.0, 0.05), nu=0.05, seed=11)


def effect_inputs():
    """a 15-joint hand on a smooth root path seen by one camera: (parents, weights with d == 0, true track [1,T,J,4], kp with noisy pixel
    targets, start roots [T,7], true roots [T,7])"""
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    sd = sk.zero_distance(sd)
    J = len(parents)
    T = EFFECT["T"]
    rest, kpj, kpo = sk.tables(parents)
    rest = rest * np.float32(sk.EFFECT_REACH)
    r = np.random.RandomState(EFFECT["seed"])
    pose = sk.unit_poses(1, J, 7).astype(np.float64)
    track = np.repeat(pose, T, axis=0) + 0.02 * r.randn(T, J, 4)
    track /= np.sqrt((track * track).sum(-1, keepdims=True))
    t = np.linspace(0.0, 1.0, T)
    true_root = np.zeros((T, 7))
    true_root[:, 0] = 1.0
    true_root[:, 4] = 0.3 * np.sin(2 * np.pi * t)
    true_root[:, 5] = 0.2 * t
    true_root[:, 6] = si.EFFECT_DEPTH + 0.5 * np.cos(np.pi * t)
    Pk = sk.positions(track, parents, rest, kpj, kpo)
    C = si.place(Pk, true_root)[0]
    fx, fy, cx, cy = si.CAMERA
    pix = np.stack([fx * C[..., 0] / C[..., 2] + cx, fy * C[..., 1] / C[..., 2] + cy], axis=-1) + EFFECT["noise"] * r.randn(T, len(kpj), 2)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=np.ascontiguousarray(pix, np.float32))
    start = true_root.copy()
    start[:, 6] += 0.3
    return parents, sd, np.ascontiguousarray(track[None], np.float32), kp, np.ascontiguousarray(start, np.float32), true_root


def oracle_effect():
    """-> dict(rms_uncoupled, rms_coupled, energy_uncoupled, energy_coupled): the RMS second difference of the fitted depth s_z along the
    clip and the mean final reprojection energy, with and without the coupling of the root's translation, on the float64 restatement"""
    parents, sd, track, kp, start, _ = effect_inputs()
    cam = si.cam_of(True, 0.0)
    out = {}
    for name, lam in (("uncoupled", (0.0, 0.0)), ("coupled", EFFECT["lam"])):
        _, Es, rt = relax(track, sd, EFFECT["steps"], "lrelu", parents, kp, cam, None, start, EFFECT["weights"], nu=EFFECT["nu"], frames=EFFECT["T"],
                          root_smooth=lam, free_ends=True, smooth=0.0, renormalize="unit")
        z = rt[:, 6]
        out["rms_" + name] = float(np.sqrt(np.mean((z[2:] - 2 * z[1:-1] + z[:-2]) ** 2)))
        out["energy_" + name] = float(Es[-1].mean())
    return out
