"""Test helper (not a test module) for fitting poses to keypoints seen by several cameras inside the projection step
(pndf_project_options8 of include/posendf_amd.h; DESIGN.md section 2j "Several cameras"): the numpy restatement of csrc/pndf_fk.h's
several-camera term -- the world frame, the view loop in view order, the skip rule and the world-frame adjoint -- operation for operation,
on top of tests/skeleton_length_oracle.py's scaled tree and scales' step, tests/skeleton_image_oracle.py's robustifier and root step and
tests/skeleton_keypoints_oracle.py's kinematics and fitting step; the raw C struct; the runner that drives pndf_skel_project or
pndf_project_ex_cpu with it.  Shared by tests/test_skeleton_views.py (host twin) and tests/test_skeleton_views_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `views_energy_grad` in float32 IS the
specification both implementations are held to bit for bit; the same code in float64 is the truth."""
import ctypes
import functools

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko

BAD_ARG = sk.BAD_ARG
CASES = sl.CASES      # the 15-joint hand, the 32-joint tree, one joint, five roots, a chain of 32, the encoder-less hand
ACTS = sk.ACTS
P, T, B = si.P, si.T, si.B
K_STEPS = sk.K_STEPS
NU = sk.NU
MAX_VIEWS = 8
VIEW_COUNTS = (1, 2, 3, 8)
flat, pack, ptr, assert_same = sk.flat, sk.pack, sk.ptr, sk.assert_same
dot3, fk_unit, fk_rot, fk_quat_adj = sk.dot3, sk.fk_unit, sk.fk_rot, sk.fk_quat_adj
same_bytes, make_roots = si.same_bytes, si.make_roots
lengths = sl.lengths
UNREAD_CAMERA = (0.0, -3.0, float("nan"), float("inf"))      # base6's intrinsics with views: not read, so not refused either


# ---------------------------------------------------------------- views and targets
def make_views(V, seed=71, centre_depth=si.DEPTH, skew=0.02, spread=None):
    """[V,16] float32: view v looks at the point (0, 0, centre_depth) of the world frame from the distance si.DEPTH, turned about the
    world's y axis by v * spread (default: a full turn over V + 1 views, so no two views coincide and none looks from behind at exactly
    180 degrees) and a little about x; intrinsics near si.CAMERA; `skew` * N(0, 1) on every entry of R_v: the term takes any matrix"""
    r = np.random.RandomState(seed)
    spread = 2.0 * np.pi / (V + 1) if spread is None else spread
    rows = []
    for v in range(V):
        a, b = v * spread, 0.1 * r.randn()
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Rx @ Ry + skew * r.randn(3, 3)
        t = np.array([0.0, 0.0, si.DEPTH]) - R @ np.array([0.0, 0.0, centre_depth])
        K = np.array(si.CAMERA) * r.uniform(0.8, 1.25, 4)
        rows.append(np.concatenate([K, R.reshape(9), t]))
    return np.ascontiguousarray(np.stack(rows), np.float32)


def identity_view(camera=si.CAMERA):
    """[1,16]: R = I, t = 0 and the intrinsics `camera`: the one camera of a pndf_project_options6"""
    return np.ascontiguousarray([list(camera) + [1, 0, 0, 0, 1, 0, 0, 0, 1] + [0, 0, 0]], np.float32)


def project(Wk, views):
    """pixels [B,V,K,2] and camera-frame depths [B,V,K] of world points Wk [B,K,3] in Wk's dtype (the truth of the targets: plain
    arithmetic, not the stated order)"""
    vt = np.asarray(views, Wk.dtype)
    R, t = vt[:, 4:13].reshape(-1, 3, 3), vt[:, 13:16]
    C = np.einsum("vxy,bky->bvkx", R, Wk) + t[None, :, None, :]
    with np.errstate(all="ignore"):
        pix = vt[None, :, None, 0:2] * C[..., :2] / C[..., 2:3] + vt[None, :, None, 2:4]
    return pix, C[..., 2]


def make_view_conf(K, n, V, seed=19):
    """[n,V,K] float32: sk.make_conf's mixture (zeros, a negative value, a NaN) over views and keypoints"""
    return np.ascontiguousarray(sk.make_conf(K, n * V, seed).reshape(n, V, K))


def case_kp(case, views, n=B, conf=False, rooted=True, root_seed=29, nan_missing=True):
    """(parents, kp): sk.case_kp's tables; Y [n,V,K,2] are the pixels in `views` of the keypoints of seeded unit poses placed in the world
    frame by make_roots(seed=root_seed) (rooted) or left in the tree's frame (float64, rounded once); conf [n,V,K]"""
    parents, kp = sk.case_kp(case, n)
    Pk = sk.positions(sk.unit_poses(n, len(parents), 31).astype(np.float64), parents, kp["rest"], kp["kpj"], kp["kpo"])
    Wk = si.place(Pk, make_roots(n, root_seed).astype(np.float64))[0] if rooted else Pk
    kp["Y"] = np.ascontiguousarray(project(Wk, views)[0], np.float32)
    if conf:
        kp["conf"] = make_view_conf(len(kp["kpj"]), n, len(views))
        if nan_missing:
            kp["Y"] = sk.missing(kp["Y"], kp["conf"])
    return parents, kp


# ---------------------------------------------------------------- csrc/pndf_fk.h's several-camera term, operation for operation
def views_energy_grad(q, parents, rest, kpj, kpo, Y, conf=None, root=None, rho=0.0, views=None, sigma=None):
    """pndf_fk_views_energy_grad for every pose of q [B,J,4], in q's dtype: (E [B], dE/dQ [B,J,4], dE/d(c, s) [B,7] or None, h [B,S]).
    Y [B,V,K,2], conf [B,V,K] or None, views [V,16], sigma [B,S] (the row of every pose's group) or None (all ones: a product with 1 is
    exact, so the same bits as no product)."""
    q = np.asarray(q)
    dt = q.dtype.type
    Bn, J = q.shape[:2]
    K = len(kpj)
    V = len(views)
    rest, kpo, Y = np.asarray(rest, q.dtype), np.asarray(kpo, q.dtype), np.asarray(Y, q.dtype)
    assert Y.shape == (Bn, V, K, 2)
    vt = np.asarray(np.asarray(views, np.float32), q.dtype)
    sigma = np.ones((Bn, J + K), q.dtype) if sigma is None else np.asarray(sigma, q.dtype)
    assert sigma.shape == (Bn, J + K)
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
            os_ = [sigma[:, J + k] * o[x] for x in range(3)]
            Pk = [p[a][x] + dot3(G[a][3 * x], os_[0], G[a][3 * x + 1], os_[1], G[a][3 * x + 2], os_[2]) for x in range(3)]
            vu = [dot3(G[a][3 * x], o[0], G[a][3 * x + 1], o[1], G[a][3 * x + 2], o[2]) for x in range(3)]
            Wd = Pk if Rc is None else [dot3(Rc[3 * x], Pk[0], Rc[3 * x + 1], Pk[1], Rc[3 * x + 2], Pk[2]) + s[x] for x in range(3)]
            aW = [zero] * 3
            seen = np.zeros(Bn, bool)
            for v in range(V):
                fx, fy, cx, cy = vt[v, 0], vt[v, 1], vt[v, 2], vt[v, 3]
                Rv, tv = vt[v, 4:13], vt[v, 13:16]
                w = np.ones(Bn, q.dtype) if conf is None else np.asarray(conf, q.dtype)[:, v, k]
                on = w > 0
                w = np.where(on, w, dt(0))
                C = [dot3(Rv[3 * x], Wd[0], Rv[3 * x + 1], Wd[1], Rv[3 * x + 2], Wd[2]) + tv[x] for x in range(3)]
                on = on & (C[2] > 0)
                y = np.where(on[:, None], Y[:, v, k], dt(0))      # the target of a view that takes no part is not read
                Cz = np.where(on, C[2], dt(1))
                nu_, nv = C[0] / Cz, C[1] / Cz
                yu, yv = (y[:, 0] - cx) / fx, (y[:, 1] - cy) / fy
                eu, ev = nu_ - yu, nv - yv
                ru, pu = si.robust(eu, rho)
                rv, pv = si.robust(ev, rho)
                e = w * (ru + rv)
                acc = np.where(on, acc + e, acc)
                tu, tv_ = pu / Cz, pv / Cz
                tz = -((pu * nu_ + pv * nv) / Cz)
                adj = [w * tu, w * tv_, w * tz]
                for x in range(3):      # R_v^T a, accumulated in view order from 0
                    aW[x] = np.where(on, aW[x] + dot3(Rv[x], adj[0], Rv[3 + x], adj[1], Rv[6 + x], adj[2]), aW[x])
                seen = seen | on
            if Rc is not None:
                for x in range(3):
                    a_s[x] = np.where(seen, a_s[x] + aW[x], a_s[x])
                    for c in range(3):
                        AR[3 * x + c] = np.where(seen, AR[3 * x + c] + aW[x] * Pk[c], AR[3 * x + c])
            wr = [aW[x] if Rc is None else dot3(Rc[x], aW[0], Rc[3 + x], aW[1], Rc[6 + x], aW[2]) for x in range(3)]
            for x in range(3):
                ap[a][x] = np.where(seen, ap[a][x] + wr[x], ap[a][x])
                for c in range(3):
                    M[a][3 * x + c] = np.where(seen, M[a][3 * x + c] + wr[x] * os_[c], M[a][3 * x + c])
            h[J + k] = np.where(seen, dot3(wr[0], vu[0], wr[1], vu[1], wr[2], vu[2]), dt(0))
        g = np.zeros_like(q)
        for j in range(J - 1, -1, -1):
            pa, Mj, t, tj = parents[j], M[j], rest[j], ts[j]
            if pa < 0:
                v_ = [np.full(Bn, t[x], q.dtype) for x in range(3)]
            else:
                Gp = G[pa]
                v_ = [dot3(Gp[3 * x], t[0], Gp[3 * x + 1], t[1], Gp[3 * x + 2], t[2]) for x in range(3)]
            h[j] = dot3(ap[j][0], v_[0], ap[j][1], v_[1], ap[j][2], v_[2])
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


def one_step(q, d, g, parents, kp, views, rho, rt, root_weights, sg, ln, group_frames, nu, **kw):
    """one step of the statement at the track q [P,T,J,4] in q's dtype: (q', E, root', scales' or None, h).  sg None: no scales."""
    dt = q.dtype
    Bn = q.shape[0] * q.shape[1]
    G, n = sl.groups_of(Bn, group_frames, ln["per_pose"])
    E, gk, gr, h = views_energy_grad(q.reshape((-1,) + q.shape[2:]), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), rt, rho, views,
                                     None if sg is None else np.repeat(sg, n, axis=0))
    tol = kw.get("tol", 0.0)
    out = sk.fit_step(q, d, g, gk, nu, **kw)
    if rt is not None and any(root_weights):
        rt = si.root_step(rt, gr, root_weights[0], root_weights[1], d, tol)
    if sg is not None and ln["nu_len"] > 0:
        S = sg.shape[1]
        dd = np.asarray(d, dt).reshape(G, n)
        rests = (dd < dt.type(tol)).all(axis=1) if tol > 0 else np.zeros(G, bool)
        rate = np.ones(S, np.float32) if ln["rate"] is None else ln["rate"]
        sg = sl.len_step(sg, sl.group_sum(h.reshape(G, n, S)), n, ln["nu_len"], rate, ln["kappa"], ln["clamp"], rests)
    return out, E, rt, sg, h


def rounds(forward_grad, track, steps, parents, kp, views, rho=0.0, ln=None, root=None, root_weights=(0.0, 0.0), nu=NU, frames=None, **kw):
    """`steps` rounds of { forward_grad of the engine under test ; the float32 restatement } -> (track, d, E of the last round, root, scales)"""
    ln = ln or lengths(None)
    cur = np.ascontiguousarray(track, np.float32).copy()
    rt = None if root is None else np.ascontiguousarray(root, np.float32).copy()
    sg = None if ln["scale"] is None else ln["scale"].copy()
    frames_ = track.shape[1] if frames is None else frames
    d = np.zeros(track.shape[0] * track.shape[1], np.float32)
    E = np.zeros_like(d)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        cur, E, rt, sg, _ = one_step(cur, d, g, parents, kp, views, rho, rt, root_weights, sg, ln, frames_, nu, frames=frames, **kw)
        cur = np.ascontiguousarray(cur, np.float32)
    return cur, d, E, rt, sg


def relax(track, sd, steps, act, parents, kp, views, rho=0.0, ln=None, root=None, root_weights=(0.0, 0.0), nu=NU, dtype=np.float64, frames=None, **kw):
    """free-running oracle in `dtype` -> (track, d of the last step, E of every step [steps,B], the root after every step, the scales after
    every step or None)"""
    ln = ln or lengths(None)
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    rt = None if root is None else np.asarray(root, dtype)
    sg = None if ln["scale"] is None else np.asarray(ln["scale"], dtype)
    frames_ = q.shape[1] if frames is None else frames
    d, Es, Rs, Ss = None, [], [], []
    for _ in range(steps):
        d, g, _, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        q, E, rt, sg, _ = one_step(q, d, g, parents, kp, views, rho, rt, root_weights, sg, ln, frames_, nu, frames=frames, **kw)
        Es.append(E)
        Rs.append(rt)
        Ss.append(sg)
    return q, np.asarray(d).reshape(-1), np.stack(Es), Rs, (None if sg is None else np.stack(Ss))


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options8(lib, base7, views=None, n_views=0, reserved4=0, size=None):
    """a pndf_project_options8 (224 bytes) around a filled ProjectOptions7; views: an address or None"""
    from posendf_amd.abi import ProjectOptions8
    o = ProjectOptions8()
    o.base7 = base7
    o.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.views, o.n_views, o.reserved4 = views, n_views, reserved4
    return o


C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float pixels[4 * 2 * 3 * 2] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static float placement[4 * 7] = {1, 0, 0, 0, 0, 0, 5};
    static const float views[2 * 16] = {500, 500, 320, 240, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0,
                                        500, 500, 320, 240, 0, 0, -1, 0, 1, 0, 1, 0, 0, 5, 0, 5};
    pndf_project_options8 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base7.base6.base5.base4.base3.base2.base);
    o.base7.base6.base5.base4.base3.base2.base.struct_size = sizeof o;
    o.base7.base6.base5.kp_target = pixels;
    o.base7.base6.base5.rest = rest;
    o.base7.base6.base5.kp_joint = joint;
    o.base7.base6.base5.n_keypoints = 3;
    o.base7.base6.base5.nu = 0.1f;
    o.base7.base6.root = placement;
    o.base7.base6.nu_trans = 0.1f;
    o.base7.base6.kp_flags = PNDF_KP_IMAGE;
    o.views = views;
    o.n_views = 2;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 224) + (int)(sizeof(pndf_project_options7) != 208) + (int)(PNDF_FK_MAX_VIEWS != 8);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class ViewsRunner:
    """mixed in front of a LengthRunner: `run` with the 224-byte struct.  -> (status, q_out, d_last, kp_energy, root after the call or None,
    scales after the call or None).  kp["Y"] is [n,V,K,2], kp["conf"] [n,V,K]; `views` [V,16] float32 stays in host memory."""

    def run8(self, q, steps, kp, views=None, rho=0.0, ln=None, cam=None, make8=None, **kw):
        ln_ = ln or lengths(None)
        table = None if views is None else np.ascontiguousarray(views, np.float32)
        cam = cam or si.cam_of(True, rho, UNREAD_CAMERA if table is not None else si.CAMERA)

        def make(at, base6):
            clamp = ln_["clamp"] or (0.0, 0.0)
            o7 = sl.c_options7(self.lib, base6, at.get("scale"), ptr(ln_["rate"]), ln_["nu_len"], ln_["kappa"], clamp[0], clamp[1],
                               sl.LEN_PER_POSE if ln_["per_pose"] else 0)
            if make8 is not None:
                return make8(at, o7)
            return c_options8(self.lib, o7, ptr(table), 0 if table is None else len(table))
        return self.run7(q, steps, kp, ln=ln_, cam=cam, make=make, **kw)      # (`table` lives in the closure until the call is over)

    def fit8(self, q, steps, kp, **kw):
        rc, out, d, E, rt, sg = self.run8(q, steps, kp, **kw)
        assert rc == 0, self.last_error()
        return out, d, E, rt, sg


# (V, root given, root weights, rho, confidences, scales: None / "track" / "pose", tracks: None / "held" / "free", mask, the quaternion anchor)
VARIANTS = [(1, False, (0.0, 0.0), 0.0, False, None, None, False, False),
            (2, True, (si.NU_ROT, si.NU_TRANS), si.RHO, True, "track", "free", True, True),
            (3, True, (0.0, si.NU_TRANS), 0.0, True, "pose", "held", False, True),
            (8, True, (si.NU_ROT, 0.0), si.RHO, False, None, None, True, False),
            (2, False, (0.0, 0.0), 0.0, True, "pose", None, False, True),
            (8, True, (si.NU_ROT, si.NU_TRANS), 0.0, True, "track", "free", True, False),
            (3, True, (si.NU_ROT, si.NU_TRANS), si.RHO, False, None, "held", False, False)]


def check_stated_step(run, case, act):
    """K_STEPS rounds of the runner's own forward_grad + the float32 restatement equal the call with the 224-byte struct, bit for bit:
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
        for V, use_root, weights, rho, use_conf, scales, tracks, use_mask, use_anchor in VARIANTS:
            what = (name, V, use_root, weights, rho, use_conf, scales, tracks, use_mask, use_anchor)
            views = make_views(V, centre_depth=si.DEPTH if use_root else 0.0)
            _, kp = case_kp(case, views, conf=use_conf, rooted=use_root)
            S = J + len(kp["kpj"])
            root = start_root if use_root else None
            ln = lengths(None)
            if scales:
                G, _ = sl.groups_of(B, T if tracks else 0, scales == "pose")
                ln = lengths(sl.make_scales(G, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S), None, scales == "pose")
            m = mask if use_mask else None
            anchor = sdo.make_anchor(track, aconf) if use_anchor else None
            step_kw = dict(observed=m, free_ends=tracks == "free", frames=None if tracks else 0, smooth=sk.LAMBDA if tracks else 0.0, **opts)
            if use_anchor:
                step_kw.update(anchor=anchor, conf=aconf, mu=sdo.MU)
            want, dk, Ek, rk, sk_ = rounds(run.forward_grad, track, K_STEPS, parents, kp, views, rho, ln, root, weights, **step_kw)
            call_kw = dict(opts=opts, words=words if use_mask else None, frames=T if tracks else 0, lam=sk.LAMBDA if tracks else 0.0,
                           flags=sdo.FREE_ENDS if tracks == "free" else 0, views=views, rho=rho, root=root, root_weights=weights, ln=ln)
            if use_anchor:
                call_kw.update(anchor=flat(anchor), aconf=aconf.reshape(-1, J), mu=sdo.MU)
            got, dl, El, rl, sg = run.fit8(flat(track), K_STEPS, kp, **call_kw)
            assert_same(got.reshape(track.shape), want, what)
            assert_same(dl, dk, what + ("d_last",))
            assert_same(El, Ek, what + ("kp_energy",))
            assert (El > 0).any(), what
            same_bytes(rl, rk, what + ("root",))
            if scales:
                assert_same(sg, sk_, what + ("bone_scale",))
                assert (sg != ln["scale"]).any(), what
            if any(weights):
                assert (rl != root).any(), what
            if not tracks:
                again = run.fit8(flat(track), K_STEPS, kp, in_place=True, **call_kw)
                for a, b in zip(again, (got, dl, El, rl, sg)):
                    same_bytes(a, b, what + ("in place",))


# ---------------------------------------------------------------- reduction to the pinned calls
def check_reductions(run, case, act):
    """V = 1 with R = I, t = 0 and CAMERA's intrinsics: the bytes of the 208-byte call with that camera (entries that differ are compared
    by value and must be zeros of either sign: the identity products turn -0 into +0).  n_views = 0: the 208-byte call's bytes.  nu = 0:
    the 72-byte call's bytes, targets and confidences full of NaN never read, root and scales neither read nor written."""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    track = sdo.clip(case, P, T)
    q = flat(track)
    words = pack(sdo.make_mask(J, P, T))
    anchor = flat(sdo.make_anchor(track))
    root = make_roots(B, 37)
    tol = float(np.median(run.forward(q)))
    _, kp1, _ = si.case_kp(case, image=True, conf=True)
    K = len(kp1["kpj"])
    S = J + K
    kpv = dict(kp1, Y=np.ascontiguousarray(kp1["Y"][:, None]), conf=np.ascontiguousarray(kp1["conf"][:, None]))
    zeros_of_either_sign = 0
    for name in sk.OPTION_SETS:
        opts = sk.options(name, tol)
        for frames, lam, flags, w, akw in ((0, 0.0, 0, None, dict()), (T, sk.LAMBDA, sdo.FREE_ENDS, words, dict(anchor=anchor, mu=sdo.MU))):
            kw = dict(opts=opts, words=w, frames=frames, lam=lam, flags=flags, **akw)
            for rkw in (dict(), dict(root=root, root_weights=(si.NU_ROT, si.NU_TRANS))):
                for scaled in (False, True):
                    what = (name, frames, sorted(rkw), scaled)
                    G, _ = sl.groups_of(B, frames, False)
                    ln = lengths(sl.make_scales(G, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S)) if scaled else lengths(None)
                    cam = si.cam_of(True, si.RHO)
                    want = run.fit7(q, K_STEPS, kp1, cam=cam, ln=ln, **rkw, **kw)
                    got = run.fit8(q, K_STEPS, kpv, views=identity_view(), rho=si.RHO, ln=ln, **rkw, **kw)
                    for a, b, part in zip(got, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
                        if a is None and b is None:
                            continue
                        if a.tobytes() != b.tobytes():
                            differ = a.view(np.uint32) != b.view(np.uint32)
                            assert (a[differ] == 0).all() and (b[differ] == 0).all(), what + (part,)
                            zeros_of_either_sign += int(differ.sum())
                    none = run.fit8(q, K_STEPS, kp1, views=None, cam=cam, ln=ln, **rkw, **kw)      # n_views = 0, views = NULL
                    for a, b, part in zip(none, want, ("poses", "d_last", "kp_energy", "root", "bone_scale")):
                        same_bytes(a, b, what + ("n_views 0", part))
            want4, d4, _ = run.fit(q, K_STEPS, small=True, **kw)
            for V in (1, 3):
                nan_kp = dict(kp1, Y=np.full((B, V, K, 2), np.nan, np.float32), conf=np.full((B, V, K), np.nan, np.float32))
                nan_root, nan_scale = np.full((B, 7), np.nan, np.float32), np.full((B, S), np.nan, np.float32)
                got, d, E, rt, sg = run.fit8(q, K_STEPS, nan_kp, views=make_views(V), nu=0.0, root=nan_root, root_weights=(si.NU_ROT, si.NU_TRANS),
                                             ln=lengths(nan_scale, sl.NU_LEN, sl.KAPPA, None, None, True), **kw)
                assert got.tobytes() == want4.tobytes() and d.tobytes() == d4.tobytes() and not E.any(), (name, frames, V)
                assert rt.tobytes() == nan_root.tobytes() and sg.tobytes() == nan_scale.tobytes(), (name, frames, V)
    return zeros_of_either_sign


# ---------------------------------------------------------------- skips
def check_skips(run, case, act):
    """a view whose confidence is 0, negative or NaN is never read: NaN-filled targets leave the bits of the call with that view's
    confidence zero and finite targets; a view with every confidence zero leaves the bits of the call without that view in the table; a
    keypoint behind one camera while seen by another equals, at one step, the call with that view's confidence for it zero"""
    V = 3
    views = make_views(V)
    parents, kp = case_kp(case, views, conf=True, nan_missing=False)
    J, K = len(parents), len(kp["kpj"])
    q = flat(sdo.clip(case, P, T))
    root = make_roots(B, 37)
    S = J + K
    ln = lengths(sl.make_scales(B, S), sl.NU_LEN, sl.KAPPA, None, None, True)
    kw = dict(opts=dict(renormalize="unit"), rho=si.RHO, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), ln=ln)
    conf = np.abs(np.nan_to_num(kp["conf"], nan=0.5)) + np.float32(0.05)      # every view sees every keypoint
    bad = conf.copy()
    bad[:, 1, 0::3], bad[:, 1, 1::3], bad[:, 1, 2::3] = np.float32(0.0), np.float32(-0.25), np.float32(np.nan)      # view 1 sees nothing
    bad[:, 0, 0] = np.float32(np.nan)
    Y = kp["Y"].copy()
    with np.errstate(invalid="ignore"):
        Y[~(bad > 0)] = np.nan
    quiet = np.where(bad > 0, bad, np.float32(0.0)).astype(np.float32)
    got = run.fit8(q, K_STEPS, dict(kp, Y=Y, conf=bad), views=views, **kw)
    want = run.fit8(q, K_STEPS, dict(kp, conf=quiet), views=views, **kw)
    assert all(np.isfinite(a).all() for a in got) and (got[2] > 0).any()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    keep = [0, 2]
    less = run.fit8(q, K_STEPS, dict(kp, Y=np.ascontiguousarray(kp["Y"][:, keep]), conf=np.ascontiguousarray(quiet[:, keep])), views=views[keep], **kw)
    for a, b in zip(got, less):
        assert a.tobytes() == b.tobytes()
    full = run.fit8(q, K_STEPS, dict(kp, conf=conf), views=views, **kw)
    assert full[0].tobytes() != got[0].tobytes()      # (the view does count when it sees)
    # behind one camera, seen by the other: two views that look at the scene from opposite sides of a keypoint far down the tree's -z
    if K < 2:
        return
    qi = q.copy()
    qi[:, :, :] = np.float32([1, 0, 0, 0])      # every joint at rest: global rotations are the identity, offsets are in the tree's frame
    far = dict(kp, kpo=kp["kpo"].copy())
    far["kpo"][K - 1] = np.float32([0.0, 0.0, -30.0])
    two = make_views(2, spread=np.pi, skew=0.0)      # view 1 looks back at view 0 through the scene
    Pk = sk.positions(qi.astype(np.float64), parents, far["rest"], far["kpj"], far["kpo"])
    depth = project(si.place(Pk, root.astype(np.float64))[0], two)[1]
    assert (depth[:, 0, K - 1] < -5.0).all() and (depth[:, 1, K - 1] > 5.0).all()
    ones = np.ones((B, 2, K), np.float32)
    blind = ones.copy()
    blind[:, 0, K - 1] = 0.0
    Y2 = np.ascontiguousarray(project(si.place(Pk, make_roots(B, 29).astype(np.float64))[0], two)[0], np.float32)
    Y2nan = Y2.copy()
    Y2nan[:, 0, K - 1] = np.nan
    got = run.fit8(qi, 1, dict(far, Y=Y2nan, conf=ones), views=two, **kw)
    want = run.fit8(qi, 1, dict(far, Y=Y2, conf=blind), views=two, **kw)
    assert all(np.isfinite(a).all() for a in got)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    gone = blind.copy()
    gone[:, 1, K - 1] = 0.0
    without = run.fit8(qi, 1, dict(far, Y=Y2, conf=gone), views=two, **kw)
    assert without[2].tobytes() != want[2].tobytes()      # (the other camera does see it)


def check_unseen_keypoint(run, case, joint):
    """one keypoint, on `joint`, seen by no view (behind one camera, zero confidence in the other): energy 0, root and scales keep their
    bits and every joint ends with the bytes of the call without a keypoint term -- the subtree's gradient is exactly zero.  Seen by one
    view it moves the joints of its chain, and only those."""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    rest, _, _ = sk.tables(parents)
    qi = flat(sdo.clip(case, P, T))
    two = make_views(2, spread=np.pi, skew=0.0)      # view 1 looks back at view 0 through the point (0, 0, DEPTH)
    kp = dict(rest=rest, kpj=np.asarray([joint], np.int32), kpo=np.asarray([[0.3, -0.2, 0.5]], np.float32),
              Y=np.ascontiguousarray(np.random.RandomState(2).uniform(100, 500, (B, 2, 1, 2)), np.float32))
    root = make_roots(B, 37, depth=-20.0)      # the whole tree far behind view 0, and so in front of view 1
    Pk = sk.positions(qi.astype(np.float64), parents, kp["rest"], kp["kpj"], kp["kpo"])
    depth = project(si.place(Pk, root.astype(np.float64))[0], two)[1]
    assert (depth[:, 0, 0] < -5.0).all() and (depth[:, 1, 0] > 5.0).all()
    start = sl.make_scales(B, J + 1)
    opts = dict(renormalize="unit", step_size=0.5)
    kw = dict(opts=opts, views=two, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), nu=1.0, ln=lengths(start, sl.NU_LEN, 0.0, None, None, True))
    plain, d_plain, _ = run.fit(qi, 1, opts=opts, small=True)
    conf = np.ones((B, 2, 1), np.float32)
    conf[:, 1] = 0.0
    got, d, E, rt, sg = run.fit8(qi, 1, dict(kp, conf=conf), **kw)
    assert got.tobytes() == plain.tobytes() and d.tobytes() == d_plain.tobytes() and not E.any()
    # dE/ds == 0: s - nu_trans * 0 keeps its bits (the quaternion is renormalised by its own step); h == 0 and kappa == 0: v = sigma - w * 0
    assert rt[:, 4:].tobytes() == root[:, 4:].tobytes() and (sg == start).all()
    chain, j = [], joint
    while j >= 0:
        chain.append(j)
        j = parents[j]
    others = [j for j in range(J) if j not in chain]
    got, d, E, rt, sg = run.fit8(qi, 1, dict(kp, conf=np.ones((B, 2, 1), np.float32)), **kw)
    assert (E > 0).all() and (rt != root).any(axis=-1).all() and (got[:, chain] != plain[:, chain]).any()
    assert got[:, others].tobytes() == plain[:, others].tobytes()


def check_view_order(case):
    """permuting the views together with their targets and confidences changes the result only through the order of the sums: the float64
    restatement agrees to 1e-12 of the gradient's size (asserted on the oracle, not as bits on the device)"""
    V = 8
    views = make_views(V)
    parents, kp = case_kp(case, views, n=12, conf=True, nan_missing=False)
    J, K = len(parents), len(kp["kpj"])
    q = sk.unit_poses(12, J, 3).astype(np.float64)
    root = make_roots(12, 37).astype(np.float64)
    sigma = sl.make_scales(12, J + K).astype(np.float64)
    perm = np.random.RandomState(3).permutation(V)
    assert (perm != np.arange(V)).any()
    args = (q, parents, kp["rest"], kp["kpj"], kp["kpo"])
    a = views_energy_grad(*args, kp["Y"].astype(np.float64), kp["conf"].astype(np.float64), root, si.RHO, views, sigma)
    b = views_energy_grad(*args, kp["Y"][:, perm].astype(np.float64), kp["conf"][:, perm].astype(np.float64), root, si.RHO, views[perm], sigma)
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, float(np.abs(x).max()))
    assert np.abs(a[1]).max() > 0


# ---------------------------------------------------------------- row and chunk locality
BAD_ROWS = si.BAD_ROWS      # 5, 7, 9, 128, 130, 257


def check_row_locality(run, case, act):
    """B = 300: a NaN pose, a NaN root, an infinite target and a NaN scale row stay in their own pose"""
    n = 300
    V = 3
    views = make_views(V)
    parents, kp = case_kp(case, views, n)
    J = len(parents)
    S = J + len(kp["kpj"])
    q = sko.case_poses(case, n)
    root = make_roots(n, 37)
    start = sl.make_scales(n, S)
    bad_q, bad_Y, bad_root, bad_scale = q.copy(), kp["Y"].copy(), root.copy(), start.copy()
    bad_q[7, 0, 2] = bad_q[130] = np.nan
    bad_root[5, 1] = bad_root[128] = np.nan
    bad_Y[9, 1], bad_Y[257, 2, 1] = np.float32(np.inf), np.float32(-np.inf)
    bad_scale[9, 0] = np.nan
    kw = dict(opts=dict(renormalize="unit"), views=views, root_weights=(si.NU_ROT, si.NU_TRANS))
    ln = lambda s: lengths(s, sl.NU_LEN, sl.KAPPA, None, None, True)  # noqa: E731
    clean = run.fit8(q, K_STEPS, kp, root=root, ln=ln(start), **kw)
    got = run.fit8(bad_q, K_STEPS, dict(kp, Y=bad_Y), root=bad_root, ln=ln(bad_scale), **kw)
    keep = np.ones(n, bool)
    keep[list(BAD_ROWS)] = False
    assert all(np.isfinite(a).all() for a in clean)
    for row in BAD_ROWS:      # the bad values did arrive
        assert got[0][row].tobytes() != clean[0][row].tobytes() or got[3][row].tobytes() != clean[3][row].tobytes(), row
    for a, b in zip(got, clean):
        assert a[keep].tobytes() == b[keep].tobytes()
    for part in (slice(0, 16), slice(120, 136), slice(n - 8, n)):      # a row's result does not depend on its batch
        alone = run.fit8(q[part], K_STEPS, dict(kp, Y=kp["Y"][part]), root=root[part], ln=ln(start[part]), **kw)
        for a, b in zip(alone, clean):
            assert a.tobytes() == b[part].tobytes(), part


# ---------------------------------------------------------------- the effect: two cameras make depth and scale observable
EFFECT_N = 16
EFFECT_STEPS = 200
EFFECT_SCALE = 1.2                   # every scale of the start is this common factor; the truth is 1
EFFECT_SHIFT = 1.0                   # the start root is the true one moved this far along the first view's optical axis
EFFECT_NOISE = 0.05
EFFECT_NU, EFFECT_NU_TRANS, EFFECT_NU_LEN = 0.15, 0.15, 0.075
EFFECT_SCALE_MARGIN, EFFECT_DEPTH_MARGIN = 0.9, 0.15      # from the fp64 oracle's figures in oracle_effect's docstring: it shows 0.853 and 0.081


def effect_views():
    """two views at the distance si.EFFECT_DEPTH from the scene's centre whose optical axes are 90 degrees apart, orthonormal"""
    rows = []
    for a in (0.0, 0.5 * np.pi):
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([0.0, 0.0, si.EFFECT_DEPTH]) - R @ np.array([0.0, 0.0, si.EFFECT_DEPTH])
        rows.append(np.concatenate([np.array(si.CAMERA), R.reshape(9), t]))
    return np.ascontiguousarray(np.stack(rows), np.float32)


def effect_inputs(act="lrelu"):
    """(parents, weights with d == 0, start poses [N,J,4], start roots [N,7], kp with pixels of both views [N,2,K,2], true roots [N,7]): a
    true pose, a true root (translation about (0, 0, EFFECT_DEPTH), so the hand sits at the centre both views look at) and unit scales
    generate the pixels (float64, rounded once).  The start: the pose plus EFFECT_NOISE * N(0, 1) per component, renormalised; the root's
    translation moved by EFFECT_SHIFT along the first view's axis (+z); every scale EFFECT_SCALE."""
    parents, sd, _, kp = sk.effect_inputs(act)
    J = len(parents)
    n = EFFECT_N
    truth = sk.unit_poses(n, J, 31).astype(np.float64)
    true_root = make_roots(n, 43, depth=si.EFFECT_DEPTH).astype(np.float64)
    true_root[:, 4:6] *= 0.25
    Wk = si.place(sk.positions(truth, parents, kp["rest"], kp["kpj"], kp["kpo"]), true_root)[0]
    views = effect_views()
    pix, depth = project(Wk, views)
    assert (depth > 1.0).all()
    kp = dict(kp, Y=np.ascontiguousarray(pix, np.float32))
    r = np.random.RandomState(41)
    x = truth + EFFECT_NOISE * r.randn(*truth.shape)
    x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    rt = true_root.copy()
    rt[:, 6] += EFFECT_SHIFT
    return parents, sd, np.ascontiguousarray(x, np.float32), np.ascontiguousarray(rt, np.float32), kp, true_root


def effect_call(n_views):
    """(views, kp restricted to the first n_views views)"""
    parents, sd, x, rt, kp, true_root = effect_inputs()
    views = effect_views()[:n_views]
    return views, dict(kp, Y=np.ascontiguousarray(kp["Y"][:, :n_views]))


def effect_errors(scales, roots, true_root):
    """(mean |sigma - 1| per pose, |s_z - true| per pose) of the last step"""
    return np.abs(np.asarray(scales, np.float64) - 1.0).mean(axis=1), np.abs(np.asarray(roots, np.float64)[:, 6] - true_root[:, 6])


@functools.lru_cache(maxsize=None)
def oracle_effect(n_views):
    """the fp64 restatement on effect_inputs with the first `n_views` views, kappa = 0, root translation and scales free ->
    (E [steps,N], final scale error [N], final depth error [N]).
    Weights tried on this float64 restatement, 200 steps, as (nu; nu_trans; nu_len) -> with both views: whether si.falls(E) holds, the median
    over the poses of the final mean |sigma - 1| (start 0.2) and of the final |s_z - true| (start 1.0); with the first view alone the same
    two figures (falls(E) held with one view at every weight tried):
      (0.3; 0.3; 0.3)      no: 188 rising steps in 3 poses    0.1365  0.0494      one view 0.1940  1.0316
      (0.2; 0.2; 0.1)      no: 28 rising steps in 1 pose      0.1628  0.0657      one view 0.1971  1.0305
      (0.15; 0.15; 0.075)  falls                              0.1685  0.0827      one view 0.1975  1.0264
      (0.1; 0.1; 0.05)     falls                              0.1755  0.1073      one view 0.1979  1.0218
      (0.05; 0.05; 0.02)   falls                              0.1877  0.1594      one view 0.1988  1.0154
      (0.1; 0.2; 0.1)      falls                              0.1590  0.0581      one view 0.1963  1.0392
      (0.1; 0.1; 0.1)      falls                              0.1611  0.1141      one view 0.1961  1.0201
      (0.1; 0.1; 0.2)      falls                              0.1440  0.1188      one view 0.1935  1.0171
      (0.1; 0.1; 0.4)      falls                              0.1353  0.1306      one view 0.1900  1.0132
    The check runs at (0.15; 0.15; 0.075), the largest of the family 2 : 2 : 1 at which every step falls.  With both views the depth returns
    (1.0 -> 0.083) and the common scale moves towards the truth (0.2 -> 0.1685, slowly: a fixed-step descent, and the scale trades against
    the pose); with the first view alone the depth does not return (1.0 -> 1.026) and the scale barely moves (0.2 -> 0.1975): the
    ambiguity the README names.  Ratios two views / one view: scale 0.853, depth 0.081; the gates are 0.9 and 0.15."""
    parents, sd, x, rt, kp, true_root = effect_inputs()
    views, kpv = effect_call(n_views)
    S = len(parents) + len(kp["kpj"])
    ln = lengths(np.full((EFFECT_N, S), EFFECT_SCALE, np.float32), EFFECT_NU_LEN, 0.0, None, None, True)
    _, d, E, Rs, Ss = relax(x[None], sd, EFFECT_STEPS, "lrelu", parents, kpv, views, 0.0, ln, rt, (0.0, EFFECT_NU_TRANS), EFFECT_NU, np.float64,
                            frames=0, renormalize="unit")
    assert not d.any()      # d == 0 exactly: pure inverse kinematics
    es, ez = effect_errors(Ss[-1], Rs[-1], true_root)
    print(f"[views effect V={n_views}] fp64: E_last / E_0 median {np.median(E[-1] / E[0]):.4g} worst {(E[-1] / E[0]).max():.4g}; steps that do not fall "
          f"{int((np.diff(E, axis=0) >= 0).sum())}; mean |sigma - 1| {EFFECT_SCALE - 1:.3f} -> median {np.median(es):.4f} worst {es.max():.4f}; "
          f"|s_z - true| {EFFECT_SHIFT} -> median {np.median(ez):.4f} worst {ez.max():.4f}")
    return E, es, ez


def check_effect(run):
    """the oracle's own assertions, then the runner: kp_energy over chained one-step calls falls with both views; the two-view final scale
    error lies below the one-view final scale error by the oracle's margin; the chained calls are the one call, bit for bit"""
    E2, es2, ez2 = oracle_effect(2)
    E1, es1, ez1 = oracle_effect(1)
    assert si.falls(E2) and si.falls(E1)
    assert np.median(es2) < EFFECT_SCALE_MARGIN * np.median(es1) and np.median(ez2) < EFFECT_DEPTH_MARGIN * np.median(ez1)
    assert np.median(ez1) > 0.9 * EFFECT_SHIFT      # with one view the depth does not return
    parents, _, x, rt, kp, true_root = effect_inputs()
    S = len(parents) + len(kp["kpj"])
    start = np.full((EFFECT_N, S), EFFECT_SCALE, np.float32)
    final = {}
    for n_views in (2, 1):
        views, kpv = effect_call(n_views)
        kw = dict(opts=dict(renormalize="unit"), views=views, root_weights=(0.0, EFFECT_NU_TRANS), nu=EFFECT_NU)
        ln = lambda s: lengths(s, EFFECT_NU_LEN, 0.0, None, None, True)  # noqa: E731
        cur, root, sg, Es = x, rt, start, []
        for _ in range(EFFECT_STEPS):
            cur, d, E, root, sg = run.fit8(cur, 1, kpv, root=root, ln=ln(sg), **kw)
            assert not d.any()
            Es.append(E)
        final[n_views] = effect_errors(sg, root, true_root)
        print(f"[views effect V={n_views}] kp_energy: E_last / E_0 median {np.median(Es[-1] / Es[0]):.4g}; mean |sigma - 1| median {np.median(final[n_views][0]):.4f}; "
              f"|s_z - true| median {np.median(final[n_views][1]):.4f}")
        assert si.falls(np.stack(Es)), n_views      # (the oracle's does with one view as well: the energy falls, the depth does not return)
        once = run.fit8(x, EFFECT_STEPS, kpv, root=rt, ln=ln(start), **kw)
        assert once[0].tobytes() == cur.tobytes() and once[2].tobytes() == Es[-1].tobytes() and once[3].tobytes() == root.tobytes()
        assert once[4].tobytes() == sg.tobytes()
    assert np.median(final[2][0]) < EFFECT_SCALE_MARGIN * np.median(final[1][0])
    assert np.median(final[2][1]) < EFFECT_DEPTH_MARGIN * np.median(final[1][1])
    assert np.median(final[1][1]) > 0.9 * EFFECT_SHIFT


# ---------------------------------------------------------------- refusals
def check_refusals(run):
    """every refusal of pndf_project_options8 names its field and writes nothing"""
    import math
    case = ("hand", True)
    n = 8
    V = 3
    views = make_views(V)
    parents, kp = case_kp(case, views, n)
    J, K = len(parents), len(kp["kpj"])
    kp = dict(kp, conf=np.ones((n, V, K), np.float32))
    S = J + K
    q = sko.case_poses(case, n)
    root = make_roots(n, 37)
    start = sl.make_scales(n, S)
    lib = run.lib
    keep = []

    def table(edit=None):
        t = views.copy()
        if edit:
            edit(t)
        keep.append(t)
        return ptr(t)

    def refused(field, in_place=False, b7=None, image=True, **kw):
        def make8(at, o7):
            f = dict(views=table(), n_views=V)
            f.update({k: (v(at) if callable(v) else v) for k, v in kw.items()})
            return c_options8(lib, o7 if b7 is None else b7(at, o7), **f)
        rc, out, d, E, rt, sg = run.run8(q, 2, kp, views=views, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), ln=lengths(start, sl.NU_LEN, sl.KAPPA),
                                         in_place=in_place, make8=make8, cam=si.cam_of(image, 0.0, UNREAD_CAMERA if image else si.CAMERA))
        text = run.last_error()
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in text, (field, text)
        assert (out.tobytes() == q.tobytes() if in_place else np.all(out == 7.0)) and np.all(d == 7.0) and np.all(E == 7.0), field
        assert rt.tobytes() == root.tobytes() and sg.tobytes() == start.tobytes(), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 56, 64, 71, 73, 80, 127, 129, 136, 160, 167, 169, 176, 200, 207, 209, 216, 223, 225, 232, 240):
        refused("struct_size", size=size)
    for bad in (1, 7, 1 << 31):
        refused("reserved4", reserved4=bad)
    for bad in (-1, 9, 64, -(1 << 31)):
        refused("n_views must lie in", n_views=bad)
    refused("views must not be NULL", views=None)              # views NULL with n_views > 0
    refused("n_views must be positive", n_views=0)             # views given with n_views 0
    refused("kp_flags", image=False)          # n_views > 0 without PNDF_KP_IMAGE

    def no_target(at, o7):
        o7.base6.base5.kp_target = None
        return o7
    refused("kp_target", b7=no_target)
    for v, i, bad, field in ((0, 0, 0.0, "fx"), (1, 0, -500.0, "fx"), (2, 0, math.nan, "fx"), (0, 0, math.inf, "fx"), (2, 1, 0.0, "fy"), (0, 1, -math.inf, "fy"),
                             (1, 1, math.nan, "fy")):
        refused(field, views=table(lambda t: t.__setitem__((v, i), bad)))
    for v, i, bad in ((0, 2, math.nan), (1, 3, math.inf), (2, 4, math.nan), (0, 12, -math.inf), (2, 15, math.nan), (1, 13, math.inf)):
        refused("views has an entry that is not finite", views=table(lambda t: t.__setitem__((v, i), bad)))
    for odd in (1, 2, 3):
        refused("views must be 4-byte aligned", views=table() + odd)
    # the new extents of kp_target [n,V,K,2] and kp_conf [n,V,K] in the overlap checks: q_out laid over the last float of either is refused
    # (with the extents of one view it would not be)
    refused("kp_target", b7=lambda at, o7: (setattr(o7.base6.base5, "kp_target", at["out"] - 4 * (n * V * K * 2 - 1)), o7)[1])
    refused("kp_conf", b7=lambda at, o7: (setattr(o7.base6.base5, "kp_conf", at["out"] - 4 * (n * V * K - 1)), o7)[1])
    refused("bone_scale", b7=lambda at, o7: (setattr(o7, "bone_scale", at["Y"] + 4 * (n * V * K * 2 - 1)), o7)[1])

    # whatever base7 refuses
    def bad_kappa(at, o7):
        o7.kappa = -1.0
        return o7
    refused("kappa", b7=bad_kappa)

    def bad_rho(at, o7):
        o7.base6.rho = -1.0
        return o7
    refused("rho", b7=bad_rho)

    def bad_nu(at, o7):
        o7.base6.base5.nu = math.nan
        return o7
    refused("nu", b7=bad_nu)
    # a good struct after all that
    rc, out, d, E, rt, sg = run.run8(q, 2, kp, views=views, root=root, root_weights=(si.NU_ROT, si.NU_TRANS), ln=lengths(start, sl.NU_LEN, sl.KAPPA))
    assert rc == 0, run.last_error()
    assert not np.any(out == 7.0) and not np.any(E == 7.0) and (sg != start).any() and (rt != root).any()
