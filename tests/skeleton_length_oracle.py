"""Test helper (not a test module) for fitting bone lengths inside the projection step (pndf_project_options7 of include/posendf_amd.h;
DESIGN.md section 2j "Bone lengths"): the numpy restatement of csrc/pndf_fk.h's scaled term -- the tree with its rest offsets and keypoint
offsets scaled, the per-frame gradient of the scales, the sum over the frames of a group in the stated order and the scales' step --
operation for operation, on top of tests/skeleton_image_oracle.py's camera term and tests/skeleton_keypoints_oracle.py's kinematics and
fitting step; the raw C struct; the runner that drives pndf_skel_project or pndf_project_ex_cpu with it.  Shared by
tests/test_skeleton_length.py (host twin) and tests/test_skeleton_length_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `len_energy_grad`, `group_sum` and
`len_step` in float32 ARE the specification both implementations are held to bit for bit; the same code in float64 is the truth."""
import ctypes
import functools

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko

BAD_ARG = sk.BAD_ARG
CASES = [("hand", True), ("tree32", True), ("one", True), ("roots5", True), ("chain32", True), ("hand", False)]
ACTS = sk.ACTS
P, T, B = si.P, si.T, si.B
K_STEPS = sk.K_STEPS
NU = sk.NU
LEN_PER_POSE = 1
NU_LEN, KAPPA = 0.05, 0.1      # the weights of the bit-for-bit checks: any positive values do
BLOCK = 64                     # frames per partial sum (PNDF_FK_LEN_BLOCK)
flat, pack, ptr, assert_same = sk.flat, sk.pack, sk.ptr, sk.assert_same
dot3, fk_unit, fk_rot, fk_quat_adj = sk.dot3, sk.fk_unit, sk.fk_rot, sk.fk_quat_adj
same_bytes, cam_of, make_roots = si.same_bytes, si.cam_of, si.make_roots


# ---------------------------------------------------------------- scales
def make_scales(G, S, seed=47, lo=0.8, hi=1.25):
    """[G,S] float32 scales in [lo, hi]"""
    return np.ascontiguousarray(np.random.RandomState(seed).uniform(lo, hi, (G, S)), np.float32)


def make_rates(S, seed=53):
    """[S] float32 rates in [0.5, 1.5], every fourth one zero (that scale keeps its bits)"""
    r = np.random.RandomState(seed).uniform(0.5, 1.5, S).astype(np.float32)
    r[::4] = 0.0
    return r


def groups_of(n, frames, per_pose):
    """(G, frames per group)"""
    g = 1 if (per_pose or frames < 2) else frames
    return n // g, g


# ---------------------------------------------------------------- csrc/pndf_fk.h's scaled term, operation for operation
def len_energy_grad(q, parents, rest, kpj, kpo, Y, conf=None, root=None, cam=None, sigma=None):
    """pndf_fk_len_energy_grad for every pose of q [B,J,4], in q's dtype: (E [B], dE/dQ [B,J,4], dE/d(c, s) [B,7] or None, h [B,S]).
    sigma [B,S]: the row of every pose's group."""
    cam = cam or cam_of(False)
    q = np.asarray(q)
    dt = q.dtype.type
    Bn, J = q.shape[:2]
    K = len(kpj)
    rest, kpo, Y = np.asarray(rest, q.dtype), np.asarray(kpo, q.dtype), np.asarray(Y, q.dtype)
    sigma = np.asarray(sigma, q.dtype)
    assert sigma.shape == (Bn, J + K)
    fx, fy, cx, cy = (dt(np.float32(v)) for v in cam["camera"])
    zero = np.zeros(Bn, q.dtype)
    with np.errstate(all="ignore"):
        ts = [[sigma[:, j] * rest[j][x] for x in range(3)] for j in range(J)]      # t'_j, per pose
        r, n, R, G, p = sk._forward(q, parents, ts)
        Rc = s = ch = nc = None
        if root is not None:
            root = np.asarray(root, q.dtype)
            ch, nc = fk_unit(root[:, :4])
            Rc = fk_rot(ch)
            s = [root[:, 4 + x] for x in range(3)]
        M = [[zero] * 9 for _ in range(J)]
        ap = [[zero] * 3 for _ in range(J)]
        a_s, AR = [zero] * 3, [zero] * 9
        acc = zero
        h = [zero] * (J + K)
        for k, (a, o) in enumerate(zip(kpj, kpo)):
            w = np.ones(Bn, q.dtype) if conf is None else np.asarray(conf, q.dtype)[:, k]
            on = w > 0
            w = np.where(on, w, dt(0))
            os_ = [sigma[:, J + k] * o[x] for x in range(3)]
            Pk = [p[a][x] + dot3(G[a][3 * x], os_[0], G[a][3 * x + 1], os_[1], G[a][3 * x + 2], os_[2]) for x in range(3)]
            vu = [dot3(G[a][3 * x], o[0], G[a][3 * x + 1], o[1], G[a][3 * x + 2], o[2]) for x in range(3)]
            C = Pk if Rc is None else [dot3(Rc[3 * x], Pk[0], Rc[3 * x + 1], Pk[1], Rc[3 * x + 2], Pk[2]) + s[x] for x in range(3)]
            if cam["image"]:
                on = on & (C[2] > 0)
                y = np.where(on[:, None], Y[:, k], dt(0))
                Cz = np.where(on, C[2], dt(1))
                nu_, nv = C[0] / Cz, C[1] / Cz
                yu, yv = (y[:, 0] - cx) / fx, (y[:, 1] - cy) / fy
                eu, ev = nu_ - yu, nv - yv
                ru, pu = si.robust(eu, cam["rho"])
                rv, pv = si.robust(ev, cam["rho"])
                e = w * (ru + rv)
                tu, tv = pu / Cz, pv / Cz
                tz = -((pu * nu_ + pv * nv) / Cz)
                adj = [w * tu, w * tv, w * tz]
            else:
                y = np.where(on[:, None], Y[:, k], dt(0))
                res = [C[x] - y[:, x] for x in range(3)]
                e = w * dot3(res[0], res[0], res[1], res[1], res[2], res[2])
                adj = [w * res[x] for x in range(3)]
            if Rc is not None:
                for x in range(3):
                    a_s[x] = np.where(on, a_s[x] + adj[x], a_s[x])
                    for c in range(3):
                        AR[3 * x + c] = np.where(on, AR[3 * x + c] + adj[x] * Pk[c], AR[3 * x + c])
            wr = [adj[x] if Rc is None else dot3(Rc[x], adj[0], Rc[3 + x], adj[1], Rc[6 + x], adj[2]) for x in range(3)]
            for x in range(3):
                ap[a][x] = np.where(on, ap[a][x] + wr[x], ap[a][x])
                for c in range(3):
                    M[a][3 * x + c] = np.where(on, M[a][3 * x + c] + wr[x] * os_[c], M[a][3 * x + c])
            h[J + k] = np.where(on, dot3(wr[0], vu[0], wr[1], vu[1], wr[2], vu[2]), dt(0))
            acc = np.where(on, acc + e, acc)
        g = np.zeros_like(q)
        for j in range(J - 1, -1, -1):
            pa, Mj, t, tj = parents[j], M[j], rest[j], ts[j]
            if pa < 0:
                v = [np.full(Bn, t[x], q.dtype) for x in range(3)]
            else:
                Gp = G[pa]
                v = [dot3(Gp[3 * x], t[0], Gp[3 * x + 1], t[1], Gp[3 * x + 2], t[2]) for x in range(3)]
            h[j] = dot3(ap[j][0], v[0], ap[j][1], v[1], ap[j][2], v[2])
            if pa < 0:
                A = Mj
            else:
                A = [dot3(Gp[a], Mj[b], Gp[3 + a], Mj[3 + b], Gp[6 + a], Mj[6 + b]) for a in range(3) for b in range(3)]
                for a in range(3):
                    av = ap[j][a]
                    ap[pa][a] = ap[pa][a] + av
                    for b in range(3):
                        add = av * tj[b] + dot3(Mj[3 * a], R[j][3 * b], Mj[3 * a + 1], R[j][3 * b + 1], Mj[3 * a + 2], R[j][3 * b + 2])
                        M[pa][3 * a + b] = M[pa][3 * a + b] + add
            g[:, j] = fk_quat_adj(A, r[j], n[j])
        groot = None
        if Rc is not None:
            groot = np.concatenate([fk_quat_adj(AR, ch, nc), np.stack(a_s, axis=-1)], axis=-1)
        E = dt(0.5) * acc
        hs = np.stack(h, axis=-1)
    assert E.dtype == q.dtype and g.dtype == q.dtype and hs.dtype == q.dtype
    return E, g, groot, hs


def group_sum(h, block=BLOCK):
    """h [G,n,S] -> H [G,S] in h's dtype: the partial of every block of `block` consecutive frames accumulated in frame order from 0, the
    partials added in block order from 0.  block=None: the plain sequential sum."""
    h = np.asarray(h)
    G, n, S = h.shape
    block = n if block is None else block
    total = np.zeros((G, S), h.dtype)
    with np.errstate(all="ignore"):
        for f0 in range(0, n, block):
            part = np.zeros((G, S), h.dtype)
            for f in range(f0, min(f0 + block, n)):
                part = part + h[:, f]
            total = total + part
    assert total.dtype == h.dtype
    return total


def len_step(sigma, H, n, nu_len, rate, kappa, clamp, rests):
    """pndf_fk_len_step for every group and scale, in sigma's dtype: sigma [G,S], H [G,S], rate [S], rests [G] bool"""
    sigma = np.asarray(sigma)
    dt = sigma.dtype.type
    with np.errstate(all="ignore"):
        w = dt(np.float32(nu_len)) * np.asarray(np.asarray(rate, np.float32), sigma.dtype)
        m = H / dt(n)
        pr = dt(np.float32(kappa)) * (sigma - dt(1))
        gsum = m + pr
        v = sigma - w[None, :] * gsum
        if clamp is not None:
            lo, hi = dt(np.float32(clamp[0])), dt(np.float32(clamp[1]))
            v = np.where(v < lo, lo, np.where(v > hi, hi, v))
        keep = ~(w > 0)[None, :] | np.asarray(rests, bool)[:, None]
        out = np.where(keep, sigma, v)
    assert out.dtype == sigma.dtype
    return out


def lengths(scale, nu_len=0.0, kappa=0.0, rate=None, clamp=None, per_pose=False):
    """the bone-length dict of a call"""
    return dict(scale=None if scale is None else np.ascontiguousarray(scale, np.float32), nu_len=float(nu_len), kappa=float(kappa),
                rate=None if rate is None else np.ascontiguousarray(rate, np.float32), clamp=clamp, per_pose=bool(per_pose))


def one_step(q, d, g, parents, kp, cam, rt, root_weights, sg, ln, group_frames, nu, block=BLOCK, **kw):
    """one step of the statement at the track q [P,T,J,4] in q's dtype: (q', E, root', scales', h)"""
    dt = q.dtype
    Bn = q.shape[0] * q.shape[1]
    G, n = groups_of(Bn, group_frames, ln["per_pose"])
    S = sg.shape[1]
    E, gk, gr, h = len_energy_grad(q.reshape((-1,) + q.shape[2:]), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), rt, cam,
                                   np.repeat(sg, n, axis=0))
    tol = kw.get("tol", 0.0)
    out = sk.fit_step(q, d, g, gk, nu, **kw)
    if rt is not None and any(root_weights):
        rt = si.root_step(rt, gr, root_weights[0], root_weights[1], d, tol)
    if ln["nu_len"] > 0:
        dd = np.asarray(d, dt).reshape(G, n)
        rests = (dd < dt.type(tol)).all(axis=1) if tol > 0 else np.zeros(G, bool)
        rate = np.ones(S, np.float32) if ln["rate"] is None else ln["rate"]
        sg = len_step(sg, group_sum(h.reshape(G, n, S), block), n, ln["nu_len"], rate, ln["kappa"], ln["clamp"], rests)
    return out, E, rt, sg, h


def rounds(forward_grad, track, steps, parents, kp, cam, ln, root=None, root_weights=(0.0, 0.0), nu=NU, frames=None, block=BLOCK, **kw):
    """`steps` rounds of { forward_grad of the engine under test ; the float32 restatement } -> (track, d, E of the last round, root, scales)"""
    cur = np.ascontiguousarray(track, np.float32).copy()
    rt = None if root is None else np.ascontiguousarray(root, np.float32).copy()
    sg = ln["scale"].copy()
    frames_ = track.shape[1] if frames is None else frames
    d = np.zeros(track.shape[0] * track.shape[1], np.float32)
    E = np.zeros_like(d)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        cur, E, rt, sg, _ = one_step(cur, d, g, parents, kp, cam, rt, root_weights, sg, ln, frames_, nu, block, frames=frames, **kw)
        cur = np.ascontiguousarray(cur, np.float32)
    return cur, d, E, rt, sg


def relax(track, sd, steps, act, parents, kp, cam, ln, root=None, root_weights=(0.0, 0.0), nu=NU, dtype=np.float32, history=False, frames=None,
          **kw):
    """free-running oracle in `dtype` -> (track, d of the last step, E of the last step or (history) of every step, margins, root, scales or
    (history) the scales after every step)"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    rt = None if root is None else np.asarray(root, dtype)
    sg = np.asarray(ln["scale"], dtype)
    frames_ = q.shape[1] if frames is None else frames
    nq = q.shape[0] * q.shape[1]
    d, E, margin, Es, Ss = np.zeros((nq, 1), dtype), np.zeros(nq, dtype), np.full(nq, np.inf), [], []
    for _ in range(steps):
        d, g, m, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        margin = np.minimum(margin, m)
        q, E, rt, sg, _ = one_step(q, d, g, parents, kp, cam, rt, root_weights, sg, ln, frames_, nu, frames=frames, **kw)
        Es.append(E)
        Ss.append(sg)
    return q, np.asarray(d).reshape(-1), (np.stack(Es) if history else E), margin, rt, (np.stack(Ss) if history else sg)


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options7(lib, base6, bone_scale=None, len_rate=None, nu_len=0.0, kappa=0.0, len_min=0.0, len_max=0.0, len_flags=0, reserved3=0, size=None):
    """a pndf_project_options7 (208 bytes) around a filled ProjectOptions6; bone_scale, len_rate: addresses or None"""
    from posendf_amd.abi import ProjectOptions7
    o = ProjectOptions7()
    o.base6 = base6
    o.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.bone_scale, o.len_rate = bone_scale, len_rate
    o.nu_len, o.kappa, o.len_min, o.len_max, o.len_flags, o.reserved3 = nu_len, kappa, len_min, len_max, len_flags, reserved3
    return o


C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float points[4 * 3 * 3] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static float scales[2 * 5] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    static const float rates[5] = {1, 1, 0, 1, 1};
    pndf_project_options7 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base6.base5.base4.base3.base2.base);
    o.base6.base5.base4.base3.base2.base.struct_size = sizeof o;
    o.base6.base5.base4.base3.frames = 2;
    o.base6.base5.base4.base3.fill = PNDF_TRACK_GIVEN;
    o.base6.base5.kp_target = points;
    o.base6.base5.rest = rest;
    o.base6.base5.kp_joint = joint;
    o.base6.base5.n_keypoints = 3;
    o.base6.base5.nu = 0.02f;
    o.bone_scale = scales;
    o.len_rate = rates;
    o.nu_len = 0.05f;
    o.kappa = 0.1f;
    o.len_min = 0.5f;
    o.len_max = 2.f;
    o.len_flags = PNDF_LEN_PER_POSE;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 208) + (int)(sizeof(pndf_project_options6) != 168);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class LengthRunner:
    """mixed in front of a skeleton_keypoints_oracle.Runner (TwinRunner, UnitRunner): `run` with the 208-byte struct.  -> (status, q_out,
    d_last, kp_energy, root after the call or None, scales after the call or None)"""

    def run7(self, q, steps, kp, ln=None, cam=None, root=None, root_weights=(0.0, 0.0), nu=NU, opts=None, words=None, frames=0, lam=0.0,
             anchor=None, aconf=None, mu=0.0, flags=0, in_place=False, make=None):
        q = np.ascontiguousarray(q, np.float32)
        n = len(q)
        cam = cam or cam_of(False)
        ln = ln or lengths(None)
        held = {"q": self.place(q)}
        if words is not None:
            held["words"] = self.place(np.ascontiguousarray(words, np.uint32).view(np.int32))
        for name, a in (("anchor", anchor), ("aconf", aconf), ("Y", kp["Y"]), ("conf", kp.get("conf")), ("root", root), ("scale", ln["scale"])):
            if a is not None:
                held[name] = self.place(np.ascontiguousarray(a, np.float32))
        held["out"] = held["q"] if in_place else self.filled(q.shape)
        held["d"], held["E"] = self.filled((n,)), self.filled((n,))
        at = {k: self.addr(v) for k, v in held.items()}
        base = sdo.c_from(self.lib, opts or {}, at.get("words"), frames, lam, at.get("anchor"), at.get("aconf"), mu, flags)
        base5 = sk.c_options5(self.lib, base, at["Y"], at.get("conf"), at["E"], ptr(kp["rest"]), ptr(kp.get("kpj")), ptr(kp.get("kpo")),
                              kp["K"] if "K" in kp else len(kp["kpj"]), nu)
        base6 = si.c_options6(self.lib, base5, at.get("root"), cam["camera"], cam["rho"], root_weights[0], root_weights[1], si.KP_IMAGE if cam["image"] else 0)
        if make is not None:
            opt = make(at, base6)
        else:
            clamp = ln["clamp"] or (0.0, 0.0)
            opt = c_options7(self.lib, base6, at.get("scale"), ptr(ln["rate"]), ln["nu_len"], ln["kappa"], clamp[0], clamp[1],
                             LEN_PER_POSE if ln["per_pose"] else 0)
        rc = self.project(at["q"], at["out"], at["d"], n, steps, opt)
        return (rc, self.fetch(held["out"]), self.fetch(held["d"]), self.fetch(held["E"]), (self.fetch(held["root"]) if "root" in held else None),
                (self.fetch(held["scale"]) if "scale" in held else None))

    def fit7(self, q, steps, kp, **kw):
        rc, out, d, E, rt, sg = self.run7(q, steps, kp, **kw)
        assert rc == 0, self.last_error()
        return out, d, E, rt, sg


# (image, root given, root weights, mask, keypoint confidences, tracks: None / "held" / "free", the quaternion anchor, per-pose scales,
#  rates with zeros, clamp)
VARIANTS = [(False, False, (0.0, 0.0), False, False, "held", False, False, False, None),
            (True, True, (si.NU_ROT, si.NU_TRANS), True, True, "free", True, False, True, None),
            (True, True, (0.0, si.NU_TRANS), False, True, "held", True, True, True, (0.9, 1.1)),
            (False, True, (si.NU_ROT, 0.0), True, False, None, False, False, True, None),
            (True, False, (0.0, 0.0), False, True, None, True, True, False, (0.5, 2.0)),
            (False, False, (0.0, 0.0), True, True, "free", False, True, True, None)]


def check_stated_step(run, case, act):
    """K_STEPS rounds of the runner's own forward_grad + the float32 restatement equal the call with the 208-byte struct, bit for bit:
    poses, d_last, kp_energy, root and bone_scale, for every option set and every variant"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    track = sdo.clip(case, P, T)
    mask = sdo.make_mask(J, P, T)
    words = pack(mask)
    aconf = sdo.make_conf(J, P, T)
    start_root = make_roots(B, 37)
    tol = float(np.median(run.forward(flat(track))))
    for name in sk.OPTION_SETS:
        opts = sk.options(name, tol)
        for image, use_root, weights, use_mask, use_conf, tracks, use_anchor, per_pose, use_rates, clamp in VARIANTS:
            what = (name, image, use_root, weights, use_mask, use_conf, tracks, use_anchor, per_pose, use_rates, clamp)
            _, kp, _ = si.case_kp(case, image=image, conf=use_conf)
            S = J + len(kp["kpj"])
            cam = cam_of(image, si.RHO if image else 0.0)
            root = start_root if use_root else None
            G, _ = groups_of(B, T if tracks else 0, per_pose)
            start = make_scales(G, S)
            rate = make_rates(S) if use_rates else None
            ln = lengths(start, NU_LEN, KAPPA, rate, clamp, per_pose)
            m = mask if use_mask else None
            anchor = sdo.make_anchor(track, aconf) if use_anchor else None
            step_kw = dict(observed=m, free_ends=tracks == "free", frames=None if tracks else 0, smooth=sk.LAMBDA if tracks else 0.0, **opts)
            if use_anchor:
                step_kw.update(anchor=anchor, conf=aconf, mu=sdo.MU)
            want, dk, Ek, rk, sk_ = rounds(run.forward_grad, track, K_STEPS, parents, kp, cam, ln, root, weights, **step_kw)
            call_kw = dict(opts=opts, words=words if use_mask else None, frames=T if tracks else 0, lam=sk.LAMBDA if tracks else 0.0,
                           flags=sdo.FREE_ENDS if tracks == "free" else 0, cam=cam, root=root, root_weights=weights, ln=ln)
            if use_anchor:
                call_kw.update(anchor=flat(anchor), aconf=aconf.reshape(-1, J), mu=sdo.MU)
            got, dl, El, rl, sl = run.fit7(flat(track), K_STEPS, kp, **call_kw)
            assert_same(got.reshape(track.shape), want, what)
            assert_same(dl, dk, what + ("d_last",))
            assert_same(El, Ek, what + ("kp_energy",))
            same_bytes(rl, rk, what + ("root",))
            assert_same(sl, sk_, what + ("bone_scale",))
            if use_rates:
                assert sl[:, ::4].tobytes() == start[:, ::4].tobytes(), what      # rate 0: the scale keeps its bits
            assert (sl != start).any(), what
            if not tracks:
                again = run.fit7(flat(track), K_STEPS, kp, in_place=True, **call_kw)
                for a, b in zip(again, (got, dl, El, rl, sl)):
                    same_bytes(a, b, what + ("in place",))


def check_smaller_calls(run, case, act):
    """bone_scale NULL: the bytes of the 168-byte call.  Every scale 1.0f and nu_len == 0: those bytes too, and the buffer is not written.
    kp_target NULL or nu == 0: the bytes of the 72-byte call, and scales and root full of NaN are neither read nor written.  steps == 0
    leaves bone_scale untouched."""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    track = sdo.clip(case, P, T)
    q = flat(track)
    words = pack(sdo.make_mask(J, P, T))
    anchor = flat(sdo.make_anchor(track))
    root = make_roots(B, 37)
    tol = float(np.median(run.forward(q)))
    for name in sk.OPTION_SETS:
        opts = sk.options(name, tol)
        for image in (False, True):
            _, kp, _ = si.case_kp(case, image=image, conf=True)
            K = len(kp["kpj"])
            S = J + K
            cam = cam_of(image, si.RHO if image else 0.0)
            for frames, lam, flags, w, akw in ((0, 0.0, 0, None, dict()), (T, sk.LAMBDA, sdo.FREE_ENDS, words, dict(anchor=anchor, mu=sdo.MU)),
                                               (T, sk.LAMBDA, 0, None, dict())):
                kw = dict(opts=opts, words=w, frames=frames, lam=lam, flags=flags, **akw)
                what = (name, image, frames, flags, sorted(akw))
                for rkw in (dict(), dict(root=root, root_weights=(si.NU_ROT, si.NU_TRANS))):
                    want = run.fit6(q, K_STEPS, kp, cam=cam, **rkw, **kw)
                    got = run.fit7(q, K_STEPS, kp, cam=cam, ln=lengths(None, kappa=KAPPA), **rkw, **kw)
                    for a, b in zip(got[:4], want):
                        same_bytes(a, b, what + ("NULL",))
                    for per_pose in (False, True):
                        G, _ = groups_of(B, frames, per_pose)
                        ones = np.ones((G, S), np.float32)
                        got = run.fit7(q, K_STEPS, kp, cam=cam, ln=lengths(ones, 0.0, KAPPA, make_rates(S), (0.5, 2.0), per_pose), **rkw, **kw)
                        for a, b in zip(got[:4], want):
                            same_bytes(a, b, what + ("ones", per_pose))
                        assert got[4].tobytes() == ones.tobytes(), what
                want4, d4, _ = run.fit(q, K_STEPS, small=True, **kw)
                nan_kp = dict(kp, Y=np.full_like(kp["Y"], np.nan), conf=np.full((B, K), np.nan, np.float32))
                nan_root, nan_scale = np.full((B, 7), np.nan, np.float32), np.full((B, S), np.nan, np.float32)
                ln = lengths(nan_scale, NU_LEN, KAPPA, None, None, True)
                no_target = lambda at, b6: c_options7(run.lib, si.c_options6(run.lib, sk.c_options5(run.lib, b6.base5.base4, None, at.get("conf"), at["E"],  # noqa: E731
                                                      ptr(kp["rest"]), ptr(kp["kpj"]), ptr(kp["kpo"]), K, NU), at["root"], si.CAMERA, 0.0, si.NU_ROT, si.NU_TRANS,
                                                      si.KP_IMAGE if image else 0), at["scale"], None, NU_LEN, KAPPA, 0.0, 0.0, LEN_PER_POSE)
                for variant in (dict(make=no_target), dict(nu=0.0, cam=cam, root_weights=(si.NU_ROT, si.NU_TRANS))):
                    got, d, E, rt, sg = run.fit7(q, K_STEPS, nan_kp, root=nan_root, ln=ln, **kw, **variant)
                    assert got.tobytes() == want4.tobytes() and d.tobytes() == d4.tobytes() and not E.any(), what + (sorted(variant),)
                    assert rt.tobytes() == nan_root.tobytes() and sg.tobytes() == nan_scale.tobytes(), what
    _, kp, _ = si.case_kp(case, image=False)
    start = make_scales(B, J + len(kp["kpj"]))
    got, d, E, _, sg = run.fit7(q, 0, kp, ln=lengths(start, NU_LEN, KAPPA))
    assert got.tobytes() == q.tobytes() and not d.any() and not E.any() and sg.tobytes() == start.tobytes()


# ---------------------------------------------------------------- the order of the group's sum
ORDER_T = (130, 2)      # blocks of 64, 64 and 2; and the plain sequential sum
ORDER_NU_LEN = 1e-2     # a last-bit difference of H reaches the scale only when w * H / n is of the scale's own size: on order_inputs the plain
                        # sequential sum changes 17 of 105 (hand) and 35 of 216 (tree32) scales after two steps at this weight, 1 and 4 at 1e-3


def order_inputs(case, frames, seed=61):
    """three tracks of `frames` frames with distinct per-frame 3D targets whose size differs from frame to frame by orders of magnitude, so
    that the per-frame h differ in magnitude and another order of additions gives other bits"""
    parents, kp = sk.case_kp(case, 3 * frames)
    J = len(parents)
    r = np.random.RandomState(seed)
    q = sk.unit_poses(3 * frames, J, seed).reshape(3, frames, J, 4)
    mag = (10.0 ** r.uniform(-2, 2, (3 * frames, 1, 1))).astype(np.float32)
    kp = dict(kp, Y=np.ascontiguousarray(kp["Y"] * mag + r.randn(*kp["Y"].shape).astype(np.float32) * mag, np.float32))
    return parents, kp, np.ascontiguousarray(q, np.float32)


def check_summation_order(run, case):
    """two steps bit for bit against the restatement with the stated order; for T = 130 the plain sequential sum gives other scales"""
    for frames in ORDER_T:
        parents, kp, track = order_inputs(case, frames)
        S = len(parents) + len(kp["kpj"])
        ln = lengths(make_scales(3, S), ORDER_NU_LEN, KAPPA)
        kw = dict(smooth=0.25, free_ends=True, renormalize="unit")
        want = rounds(run.forward_grad, track, 2, parents, kp, cam_of(False), ln, nu=1e-4, **kw)
        got = run.fit7(flat(track), 2, kp, ln=ln, nu=1e-4, opts=dict(renormalize="unit"), frames=frames, lam=0.25, flags=sdo.FREE_ENDS)
        assert_same(got[0].reshape(track.shape), want[0], (frames, "poses"))
        assert_same(got[4], want[4], (frames, "bone_scale"))
        assert np.isfinite(got[4]).all() and (got[4] != ln["scale"]).any()
        if frames > BLOCK:
            plain = rounds(run.forward_grad, track, 2, parents, kp, cam_of(False), ln, nu=1e-4, block=None, **kw)
            assert plain[4].tobytes() != want[4].tobytes(), "the plain sequential sum gives the same bits: the inputs do not tell the orders apart"


# ---------------------------------------------------------------- locality
def check_locality(run, case):
    """a NaN in one group's scale row, or in one frame's target, stays in that group's rows; a scale whose subtree carries no keypoint takes
    h == 0: with kappa == 0 it keeps its value, with rate == 0 its bits"""
    parents, kp, _ = si.case_kp(case, image=False)
    J, K = len(parents), len(kp["kpj"])
    S = J + K
    track = sdo.clip(case, P, T)
    q = flat(track)
    start = make_scales(P, S)
    kw = dict(opts=dict(renormalize="unit"), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS)
    clean = run.fit7(q, K_STEPS, kp, ln=lengths(start, NU_LEN, KAPPA), **kw)
    assert all(np.isfinite(a).all() for a in clean if a is not None)
    bad_scale = start.copy()
    bad_scale[1, 3 % S] = np.nan
    bad_Y = kp["Y"].copy()
    bad_Y[2 * T + 1, 0, 1] = np.nan
    got = run.fit7(q, K_STEPS, dict(kp, Y=bad_Y), ln=lengths(bad_scale, NU_LEN, KAPPA), **kw)
    rows_ok = np.ones(B, bool)
    rows_ok[T:3 * T] = False
    assert got[0][rows_ok].tobytes() == clean[0][rows_ok].tobytes() and got[2][rows_ok].tobytes() == clean[2][rows_ok].tobytes()
    groups_ok = np.ones(P, bool)
    groups_ok[1:3] = False
    assert got[4][groups_ok].tobytes() == clean[4][groups_ok].tobytes()
    assert np.isnan(got[4][1]).any() and np.isnan(got[4][2]).any()
    # one keypoint, on joint `a`: the scales of the joints outside a's chain of ancestors and of nothing else see h == 0
    a = J - 1
    chain, j = [], a
    while j >= 0:
        chain.append(j)
        j = parents[j]
    others = [j for j in range(J) if j not in chain]
    one = dict(rest=kp["rest"], kpj=np.asarray([a], np.int32), kpo=np.asarray([[0.3, -0.2, 0.5]], np.float32), Y=np.ascontiguousarray(kp["Y"][:, :1]))
    start1 = make_scales(P, J + 1)
    got = run.fit7(q, K_STEPS, one, ln=lengths(start1, NU_LEN, 0.0), **kw)
    assert (got[4][:, chain] != start1[:, chain]).any() and (got[4][:, J] != start1[:, J]).all()
    assert others
    assert (got[4][:, others] == start1[:, others]).all()      # h == 0 and kappa == 0: v = sigma - w * (0 / n + 0 * ..) = sigma
    moved = run.fit7(q, K_STEPS, one, ln=lengths(start1, NU_LEN, KAPPA), **kw)
    assert (moved[4][:, others] != start1[:, others]).any()      # (with a prior they do move)
    rate = np.ones(J + 1, np.float32)
    rate[others] = 0.0
    held = run.fit7(q, K_STEPS, one, ln=lengths(start1, NU_LEN, KAPPA, rate), **kw)
    assert held[4][:, others].tobytes() == start1[:, others].tobytes()


def check_tol(run, case):
    """with tol between the distances of two groups: a group whose frames all rest keeps its scale bits; a group with one moving frame
    steps"""
    parents, kp, _ = si.case_kp(case, image=False)
    J = len(parents)
    S = J + len(kp["kpj"])
    q = flat(sdo.clip(case, P, T))
    d = np.asarray(run.forward_grad(q)[0], np.float32).reshape(P, T)      # one step: the distances of the call are those of its input
    order = np.sort(d.max(axis=1))
    start = make_scales(P, S)
    kw = dict(frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, ln=lengths(start, NU_LEN, KAPPA))
    tol = float(np.nextafter(order[len(order) // 2], np.float32(np.inf)))      # every frame of about half of the tracks rests
    got = run.fit7(q, 1, kp, opts=dict(tol=tol), **kw)
    rests = (d < np.float32(tol)).all(axis=1)
    assert rests.any() and not rests.all(), (rests, order)
    assert got[4][rests].tobytes() == start[rests].tobytes() and (got[4][~rests] != start[~rests]).any(axis=1).all()
    some = (d < np.float32(tol)).any(axis=1) & ~rests      # a group with frames at rest and one that moves: it steps
    assert some.any()


def check_clamp(run, case):
    """a scale driven past len_max lands on it exactly, one driven below len_min on that; NaN stays NaN"""
    parents, kp, _ = si.case_kp(case, image=False)
    J = len(parents)
    S = J + len(kp["kpj"])
    q = flat(sdo.clip(case, P, T))
    start = make_scales(B, S, lo=0.95, hi=1.05)
    start[3, 1 % S] = np.nan
    free = run.fit7(q, 2, kp, ln=lengths(start, 5.0, 0.0, per_pose=True))[4]
    got = run.fit7(q, 2, kp, ln=lengths(start, 5.0, 0.0, clamp=(0.9, 1.1), per_pose=True))[4]
    ok = ~np.isnan(got)
    assert np.isnan(got[3, 1 % S]) and (got[ok] >= np.float32(0.9)).all() and (got[ok] <= np.float32(1.1)).all()
    assert (got == np.float32(1.1)).any() and (got == np.float32(0.9)).any() and (np.nan_to_num(free) > 1.1).any() and (np.nan_to_num(free) < 0.9).any()


# ---------------------------------------------------------------- the effect: a clip whose subject has other bone lengths
EFFECT_P, EFFECT_T = 4, 7
EFFECT_STEPS = 100            # N: recorded from the fp64 restatement (oracle_effect asserts both conditions for every track)
EFFECT_NU, EFFECT_NU_LEN = 0.02, 0.02
EFFECT_NOISE = 0.1


def effect_inputs(act="lrelu", image=False):
    """(parents, weights with d == 0, start track [P,T,J,4], kp with targets, true scales [P,S], start root or None): forward kinematics of
    the effect's hand with true scales in [0.8, 1.25], one set per track (float64, rounded once); the start is the pose plus EFFECT_NOISE *
    N(0, 1) per component, renormalised, and sigma = 1"""
    parents, sd, _, kp = sk.effect_inputs(act)
    J, K = len(parents), len(kp["kpj"])
    n = EFFECT_P * EFFECT_T
    truth = sk.unit_poses(n, J, 31).astype(np.float64)
    true_scale = make_scales(EFFECT_P, J + K, 67).astype(np.float64)
    per = np.repeat(true_scale, EFFECT_T, axis=0)
    rest = [[per[:, j] * np.float64(kp["rest"][j][x]) for x in range(3)] for j in range(J)]
    _, _, _, Gm, p = sk._forward(truth, parents, rest)
    Pk = np.stack([np.stack([p[a][x] + dot3(Gm[a][3 * x], per[:, J + k] * np.float64(o[0]), Gm[a][3 * x + 1], per[:, J + k] * np.float64(o[1]),
                                            Gm[a][3 * x + 2], per[:, J + k] * np.float64(o[2])) for x in range(3)], axis=-1)
                   for k, (a, o) in enumerate(zip(kp["kpj"], kp["kpo"]))], axis=1)
    root = None
    if image:
        root = make_roots(n, 43, depth=si.EFFECT_DEPTH)
        C, _, _, _ = si.place(Pk, root.astype(np.float64))
        assert (C[..., 2] > 1.0).all()
        Pk = si.pixels(C)
    kp = dict(kp, Y=np.ascontiguousarray(Pk, np.float32))
    r = np.random.RandomState(41)
    x = truth + EFFECT_NOISE * r.randn(*truth.shape)
    x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    return parents, sd, np.ascontiguousarray(x.reshape(EFFECT_P, EFFECT_T, J, 4), np.float32), kp, true_scale, root


EFFECT_KW = dict(smooth=0.0, free_ends=True, renormalize="unit")
IMAGE_EFFECT = dict(nu=0.3, nu_len=0.3, kappa=0.05, steps=30)


def effect_met(E, scales, true_scale, per_pose=False):
    """E [steps,B] falls at every step in total per track; every track's mean |sigma - true| ends below its start (shared scales)"""
    E = np.asarray(E, np.float64)
    Et = E.reshape(E.shape[0], EFFECT_P, -1).sum(axis=2)
    ok = bool((np.diff(Et, axis=0) < 0).all())
    if per_pose or true_scale is None:
        return ok
    first = np.abs(1.0 - true_scale).mean(axis=1)
    last = np.abs(np.asarray(scales[-1], np.float64) - true_scale).mean(axis=1)
    return ok and bool((last < first).all())


@functools.lru_cache(maxsize=None)
def oracle_effect(per_pose=False, image=False):
    """the fp64 restatement on effect_inputs meets both conditions for every track: (E [steps,B], scales [steps,G,S])"""
    parents, sd, x, kp, true_scale, root = effect_inputs(image=image)
    S = true_scale.shape[1]
    G = x.shape[0] * x.shape[1] if per_pose else EFFECT_P
    f = IMAGE_EFFECT if image else dict(nu=EFFECT_NU, nu_len=EFFECT_NU_LEN, kappa=0.0, steps=EFFECT_STEPS)
    ln = lengths(np.ones((G, S), np.float32), f["nu_len"], f["kappa"], per_pose=per_pose)
    _, d, E, _, _, Ss = relax(x, sd, f["steps"], "lrelu", parents, kp, cam_of(image), ln, root, (0.0, si.EFFECT_ROOT_WEIGHTS[1]) if image else (0.0, 0.0),
                              f["nu"], np.float64, history=True, **EFFECT_KW)
    assert not d.any()      # d == 0 exactly: pure inverse kinematics
    first = np.abs(1.0 - true_scale).mean(axis=1)
    last = np.abs(Ss[-1] - true_scale).mean(axis=1) if not per_pose else None
    print(f"[effect per_pose={per_pose} image={image}] fp64: E_last / E_0 {E[-1].sum() / E[0].sum():.4f}; mean |sigma - true| per track {first} -> {last}")
    assert effect_met(E, Ss, None if image else true_scale, per_pose), (per_pose, image)
    return E, Ss


def check_effect(run, per_pose=False, image=False):
    """the runner's kp_energy over chained one-step calls falls at every step as the fp64 restatement's does, every track's scales end
    nearer the truth than they started, and the chained calls are the one call, bit for bit"""
    oracle_effect(per_pose, image)
    parents, _, x, kp, true_scale, root = effect_inputs(image=image)
    S = true_scale.shape[1]
    n = EFFECT_P * EFFECT_T
    f = IMAGE_EFFECT if image else dict(nu=EFFECT_NU, nu_len=EFFECT_NU_LEN, kappa=0.0, steps=EFFECT_STEPS)
    start = np.ones((n if per_pose else EFFECT_P, S), np.float32)
    kw = dict(opts=dict(renormalize="unit"), frames=EFFECT_T, lam=0.0, flags=sdo.FREE_ENDS, cam=cam_of(image), nu=f["nu"],
              root_weights=(0.0, si.EFFECT_ROOT_WEIGHTS[1]) if image else (0.0, 0.0))
    cur, rt, sg, Es, Ss = flat(x), root, start, [], []
    for _ in range(f["steps"]):
        cur, d, E, rt, sg = run.fit7(cur, 1, kp, root=rt, ln=lengths(sg, f["nu_len"], f["kappa"], per_pose=per_pose), **kw)
        assert not d.any()
        Es.append(E)
        Ss.append(sg)
    assert effect_met(np.stack(Es), Ss, None if image else true_scale, per_pose)
    once = run.fit7(flat(x), f["steps"], kp, root=root, ln=lengths(start, f["nu_len"], f["kappa"], per_pose=per_pose), **kw)
    assert once[0].tobytes() == cur.tobytes() and once[2].tobytes() == Es[-1].tobytes() and once[4].tobytes() == sg.tobytes()
    same_bytes(once[3], rt, "root")


# ---------------------------------------------------------------- refusals
def check_refusals(run):
    """every refusal of pndf_project_options7 names its field and writes nothing"""
    import math
    case = ("hand", True)
    n = 8
    parents, kp, _ = si.case_kp(case, n, image=False)
    kp = dict(kp, conf=np.ones((n, len(kp["kpj"])), np.float32))
    J, K = len(parents), len(kp["kpj"])
    S = J + K
    q = sko.case_poses(case, n)
    root = make_roots(n, 37)
    start = make_scales(n, S)
    rates = np.ones(S, np.float32)
    lib = run.lib

    def struct(at, b6, **kw):
        f = dict(bone_scale=at["scale"], len_rate=ptr(rates), nu_len=NU_LEN, kappa=KAPPA, len_min=0.5, len_max=2.0, len_flags=0)
        f.update({k: (v(at) if callable(v) else v) for k, v in kw.items()})
        return c_options7(lib, b6, **f)

    def refused(field, in_place=False, anchor=None, b6=None, **kw):
        rc, out, d, E, rt, sg = run.run7(q, 2, kp, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), ln=lengths(start), in_place=in_place, anchor=anchor,
                                         mu=0.5 if anchor is not None else 0.0,
                                         make=lambda at, base6: struct(at, base6 if b6 is None else b6(at, base6), **kw))
        text = run.last_error()
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in text, (field, text)
        assert (out.tobytes() == q.tobytes() if in_place else np.all(out == 7.0)) and np.all(d == 7.0) and np.all(E == 7.0), field
        assert rt.tobytes() == root.tobytes() and sg.tobytes() == start.tobytes(), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 56, 64, 71, 73, 80, 127, 129, 136, 160, 167, 169, 176, 200, 207, 209, 216):
        refused("struct_size", size=size)
    for bad in (1, 7, 1 << 31):
        refused("reserved3", reserved3=bad)
    for bits in (2, 3, 1 << 31):
        refused("len_flags", len_flags=bits)
    for bad in (-0.01, math.nan, math.inf, -math.inf):
        refused("nu_len", nu_len=bad)
        refused("kappa", kappa=bad)
    for lo, hi, field in ((0.0, 2.0, "len_min"), (0.5, 0.0, "len_max"), (-0.5, 2.0, "len_min"), (math.nan, 2.0, "len_min"), (math.inf, math.inf, "len_min"),
                          (0.5, math.nan, "len_max"), (0.5, math.inf, "len_max"), (1.5, 1.0, "len_max")):
        refused(field, len_min=lo, len_max=hi)
    for i, bad in ((0, -1.0), (S - 1, math.nan), (J, math.inf)):
        r = rates.copy()
        r[i] = bad
        refused("len_rate", len_rate=ptr(r))
    refused("len_rate", len_rate=ptr(rates) + 2)
    refused("bone_scale", bone_scale=None)
    for odd in (1, 2, 3):
        refused("bone_scale", bone_scale=lambda at: at["scale"] + odd)
    # bone_scale overlapping q_out (its first and its last float), q_in, root, anchor, conf, kp_target, kp_conf, kp_energy; read-only too
    refused("bone_scale", bone_scale=lambda at: at["out"])
    refused("bone_scale", bone_scale=lambda at: at["out"] + 4 * (n * J * 4 - 1))
    refused("bone_scale", bone_scale=lambda at: at["out"] - 4 * (n * S - 1))
    refused("bone_scale", bone_scale=lambda at: at["out"], nu_len=0.0)
    for name in ("q", "root", "anchor", "Y", "conf", "E"):
        refused("bone_scale", bone_scale=lambda at, name=name: at[name], anchor=q)
    aconf = np.ones((n, J), np.float32)

    def with_conf(at, base6):
        held = run.place(aconf)
        with_conf.keep = held
        base6.base5.base4.conf = run.addr(held)
        with_conf.addr = run.addr(held)
        return base6
    refused("bone_scale", b6=with_conf, anchor=q, bone_scale=lambda at: with_conf.addr)
    # everything base6 refuses
    def bad_rho(at, base6):
        base6.rho = -1.0
        return base6
    refused("rho", b6=bad_rho)
    def bad_nu(at, base6):
        base6.base5.nu = -1.0
        return base6
    refused("nu", b6=bad_nu)
    def bad_root(at, base6):
        base6.root = None
        return base6
    refused("root", b6=bad_root)
    # a good struct after all that; PNDF_LEN_PER_POSE without tracks is accepted and says what holds there anyway
    for flags_ in (0, LEN_PER_POSE):
        rc, out, d, E, rt, sg = run.run7(q, 2, kp, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), ln=lengths(start),
                                         make=lambda at, b6: struct(at, b6, len_flags=flags_))
        assert rc == 0, run.last_error()
        assert not np.any(out == 7.0) and not np.any(E == 7.0) and (sg != start).any() and (sg >= 0.5).all() and (sg <= 2.0).all()
