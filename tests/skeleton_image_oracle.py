"""Test helper (not a test module) for fitting other skeletons to 2D keypoints (pndf_project_options6 of include/posendf_amd.h; DESIGN.md
section 2j "Image fitting"): the numpy restatement of the camera term of csrc/pndf_fk.h -- the root's placement, both residual kinds, the
adjoint into the tree, the root's adjoints and the root's step -- operation for operation, for a batch of poses, on top of
tests/skeleton_keypoints_oracle.py's kinematics and fitting step; the roots, cameras and pixel targets of the tests; the raw C struct;
the runner that drives pndf_skel_project or pndf_project_ex_cpu with it.  Shared by tests/test_skeleton_image.py (host twin) and
tests/test_skeleton_image_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `camera_energy_grad` and `root_step` in
float32 ARE the specification both implementations are held to bit for bit; the same code in float64 is the truth (its gradients are
pinned against torch autograd of forward_kinematics + camera_project by tests/test_skeleton_image.py)."""
import ctypes
import functools

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_keypoints_oracle as sk
import skeleton_oracle as sko

BAD_ARG = sk.BAD_ARG
CASES = sk.CASES
ACTS = sk.ACTS
P, T, B = sk.P, sk.T, sk.B
K_STEPS = sk.K_STEPS
NU = sk.NU
KP_IMAGE = 1
CAMERA = (500.0, 480.0, 320.0, 240.0)      # fx, fy, cx, cy
RHO = 0.25
NU_ROT, NU_TRANS = 0.05, 0.1               # the root weights of the bit-for-bit checks: any positive values do
DEPTH = 8.0                                # the roots' mean distance along the optical axis: most keypoints lie in front of the camera
flat, pack, ptr, assert_same = sk.flat, sk.pack, sk.ptr, sk.assert_same
dot3, dot4, fk_unit, fk_rot, fk_quat_adj = sk.dot3, sk.dot4, sk.fk_unit, sk.fk_rot, sk.fk_quat_adj


# ---------------------------------------------------------------- roots and targets
def make_roots(n=B, seed=23, depth=DEPTH):
    """[n,7] float32: a raw (not unit) quaternion near the identity (vector part 0.15 * N(0, 1): about 30 degrees), and a translation
    (+-1, +-1, depth +- 1)"""
    r = np.random.RandomState(seed)
    c = np.concatenate([np.ones((n, 1)), 0.15 * r.randn(n, 3)], axis=1) * r.uniform(0.5, 2.0, (n, 1))
    s = np.stack([r.uniform(-1, 1, n), r.uniform(-1, 1, n), depth + r.uniform(-1, 1, n)], axis=1)
    return np.ascontiguousarray(np.concatenate([c, s], axis=1), np.float32)


def place(Pk, root):
    """C [B,K,3] = R(c^) P + s in P's dtype, operation for operation (root None: P itself) -> (C, Rc or None, c^, n)"""
    if root is None:
        return Pk, None, None, None
    root = np.asarray(root, Pk.dtype)
    ch, n = fk_unit(root[:, :4])
    Rc = fk_rot(ch)
    C = np.stack([dot3(Rc[3 * x][:, None], Pk[..., 0], Rc[3 * x + 1][:, None], Pk[..., 1], Rc[3 * x + 2][:, None], Pk[..., 2]) + root[:, 4 + x][:, None]
                  for x in range(3)], axis=-1)
    return C, Rc, ch, n


def pixels(C, camera=CAMERA):
    fx, fy, cx, cy = camera
    with np.errstate(all="ignore"):
        return np.stack([fx * C[..., 0] / C[..., 2] + cx, fy * C[..., 1] / C[..., 2] + cy], axis=-1)


def case_kp(case, n=B, image=True, conf=False, root_seed=29, nan_missing=True):
    """(parents, kp, the roots the targets were made with): sk.case_kp's tables; the targets are the keypoints of seeded unit poses placed
    by make_roots(seed=root_seed) (float64, rounded once) -- as pixels of CAMERA (image) or as 3D points in the target's frame"""
    parents, kp = sk.case_kp(case, n)
    truth_root = make_roots(n, root_seed)
    Pk = sk.positions(sk.unit_poses(n, len(parents), 31).astype(np.float64), parents, kp["rest"], kp["kpj"], kp["kpo"])
    C, _, _, _ = place(Pk, truth_root.astype(np.float64))
    kp["Y"] = np.ascontiguousarray(pixels(C) if image else C, np.float32)
    if conf:
        kp["conf"] = sk.make_conf(len(kp["kpj"]), n)
        if nan_missing:
            kp["Y"] = sk.missing(kp["Y"], kp["conf"])
    return parents, kp, truth_root


def cam_of(image=True, rho=0.0, camera=CAMERA):
    """the camera dict of a call: image (bool), rho, camera"""
    return dict(image=bool(image), rho=float(rho), camera=tuple(camera))


# ---------------------------------------------------------------- csrc/pndf_fk.h's camera term, operation for operation
def robust(e, rho):
    """(rho(e), psi(e)) in e's dtype"""
    dt = e.dtype.type
    ee = e * e
    if rho == 0:
        return ee, e
    r2 = dt(np.float32(rho)) * dt(np.float32(rho))
    d = ee + r2
    return (r2 * ee) / d, (e * (r2 * r2)) / (d * d)


def camera_energy_grad(q, parents, rest, kpj, kpo, Y, conf=None, root=None, cam=None):
    """pndf_fk_camera_energy_grad for every pose of q [B,J,4], in q's dtype: (E [B], dE/dQ [B,J,4], dE/d(c, s) [B,7] or None without a
    root).  Y [B,K,3] or (cam['image']) [B,K,2] pixels; conf [B,K] or None; root [B,7] or None.  A keypoint whose confidence is not
    positive, or (image) whose C_z > 0 is false, takes no part."""
    cam = cam or cam_of(False)
    q = np.asarray(q)
    dt = q.dtype.type
    Bn, J = q.shape[:2]
    rest, kpo, Y = np.asarray(rest, q.dtype), np.asarray(kpo, q.dtype), np.asarray(Y, q.dtype)
    fx, fy, cx, cy = (dt(np.float32(v)) for v in cam["camera"])
    zero = np.zeros(Bn, q.dtype)
    with np.errstate(all="ignore"):
        r, n, R, G, p = sk._forward(q, parents, rest)
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
        for k, (a, o) in enumerate(zip(kpj, kpo)):
            w = np.ones(Bn, q.dtype) if conf is None else np.asarray(conf, q.dtype)[:, k]
            on = w > 0
            w = np.where(on, w, dt(0))
            Pk = [p[a][x] + dot3(G[a][3 * x], o[0], G[a][3 * x + 1], o[1], G[a][3 * x + 2], o[2]) for x in range(3)]
            C = Pk if Rc is None else [dot3(Rc[3 * x], Pk[0], Rc[3 * x + 1], Pk[1], Rc[3 * x + 2], Pk[2]) + s[x] for x in range(3)]
            if cam["image"]:
                on = on & (C[2] > 0)
                y = np.where(on[:, None], Y[:, k], dt(0))
                Cz = np.where(on, C[2], dt(1))
                nu_, nv = C[0] / Cz, C[1] / Cz
                yu, yv = (y[:, 0] - cx) / fx, (y[:, 1] - cy) / fy
                eu, ev = nu_ - yu, nv - yv
                ru, pu = robust(eu, cam["rho"])
                rv, pv = robust(ev, cam["rho"])
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
            for x in range(3):
                wr = adj[x] if Rc is None else dot3(Rc[x], adj[0], Rc[3 + x], adj[1], Rc[6 + x], adj[2])
                ap[a][x] = np.where(on, ap[a][x] + wr, ap[a][x])
                for c in range(3):
                    M[a][3 * x + c] = np.where(on, M[a][3 * x + c] + wr * o[c], M[a][3 * x + c])
            acc = np.where(on, acc + e, acc)
        g = np.zeros_like(q)
        for j in range(J - 1, -1, -1):
            pa, Mj, t = parents[j], M[j], rest[j]
            if pa < 0:
                A = Mj
            else:
                Gp = G[pa]
                A = [dot3(Gp[a], Mj[b], Gp[3 + a], Mj[3 + b], Gp[6 + a], Mj[6 + b]) for a in range(3) for b in range(3)]
                for a in range(3):
                    av = ap[j][a]
                    ap[pa][a] = ap[pa][a] + av
                    for b in range(3):
                        add = av * t[b] + dot3(Mj[3 * a], R[j][3 * b], Mj[3 * a + 1], R[j][3 * b + 1], Mj[3 * a + 2], R[j][3 * b + 2])
                        M[pa][3 * a + b] = M[pa][3 * a + b] + add
            g[:, j] = fk_quat_adj(A, r[j], n[j])
        groot = None
        if Rc is not None:
            groot = np.concatenate([fk_quat_adj(AR, ch, nc), np.stack(a_s, axis=-1)], axis=-1)
        E = dt(0.5) * acc
    assert E.dtype == q.dtype and g.dtype == q.dtype and (groot is None or groot.dtype == q.dtype)
    return E, g, groot


def root_step(root, groot, nu_rot, nu_trans, d, tol=0.0):
    """pndf_fk_root_step for every pose, in root's dtype: a pose that rests under tol keeps its root; a part whose weight is zero keeps its
    bits"""
    root = np.asarray(root)
    dt = root.dtype.type
    out = root.copy()
    with np.errstate(all="ignore"):
        if nu_rot > 0:
            u = root[:, :4] - dt(np.float32(nu_rot)) * groot[:, :4]
            ch, _ = fk_unit(u)
            out[:, :4] = np.stack(ch, axis=-1)
        if nu_trans > 0:
            out[:, 4:] = root[:, 4:] - dt(np.float32(nu_trans)) * groot[:, 4:]
        if tol > 0:
            rests = np.asarray(d, root.dtype).reshape(-1) < dt(tol)
            out = np.where(rests[:, None], root, out)
    assert out.dtype == root.dtype
    return out


def term(cur, parents, kp, root, cam):
    return camera_energy_grad(cur.reshape((-1,) + cur.shape[2:]), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"), root, cam)


def rounds(forward_grad, track, steps, parents, kp, cam, root=None, root_weights=(0.0, 0.0), nu=NU, **kw):
    """`steps` rounds of { forward_grad of the engine under test ; camera_energy_grad, sk.fit_step and root_step in float32 } ->
    (track, d of the last round, E of the last round, root)"""
    cur = np.ascontiguousarray(track, np.float32).copy()
    rt = None if root is None else np.ascontiguousarray(root, np.float32).copy()
    d = np.zeros(track.shape[0] * track.shape[1], np.float32)
    E = np.zeros_like(d)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        E, gk, gr = term(cur, parents, kp, rt, cam)
        cur = np.ascontiguousarray(sk.fit_step(cur, d, g, gk, nu, **kw), np.float32)
        if rt is not None and any(root_weights):
            rt = root_step(rt, gr, root_weights[0], root_weights[1], d, kw.get("tol", 0.0))
    return cur, d, E, rt


def relax(track, sd, steps, act, parents, kp, cam, root=None, root_weights=(0.0, 0.0), nu=NU, dtype=np.float32, history=False, **kw):
    """free-running oracle in `dtype` -> (track, d of the last step, E of the last step or (history) of every step, margins, root)"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    rt = None if root is None else np.asarray(root, dtype)
    n = q.shape[0] * q.shape[1]
    d, E, margin, Es = np.zeros((n, 1), dtype), np.zeros(n, dtype), np.full(n, np.inf), []
    for _ in range(steps):
        d, g, m, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        margin = np.minimum(margin, m)
        E, gk, gr = term(q, parents, kp, rt, cam)
        Es.append(E)
        q = sk.fit_step(q, d, g, gk, nu, **kw)
        if rt is not None and any(root_weights):
            rt = root_step(rt, gr, root_weights[0], root_weights[1], d, kw.get("tol", 0.0))
    return q, np.asarray(d).reshape(-1), (np.stack(Es) if history else E), margin, rt


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options6(lib, base5, root=None, camera=None, rho=0.0, nu_rot=0.0, nu_trans=0.0, kp_flags=0, size=None):
    """a pndf_project_options6 (168 bytes) around a filled ProjectOptions5; root: an address or None"""
    from posendf_amd.abi import ProjectOptions6
    o = ProjectOptions6()
    o.base5 = base5
    o.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.root = root
    if camera is not None:
        o.fx, o.fy, o.cx, o.cy = camera
    o.rho, o.nu_rot, o.nu_trans, o.kp_flags = rho, nu_rot, nu_trans, kp_flags
    return o


C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float pixels[2 * 3 * 2] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static float placement[2 * 7] = {1, 0, 0, 0, 0, 0, 5, 1, 0, 0, 0, 0, 0, 5};
    pndf_project_options6 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base5.base4.base3.base2.base);
    o.base5.base4.base3.base2.base.struct_size = sizeof o;
    o.base5.base4.base3.fill = PNDF_TRACK_GIVEN;
    o.base5.kp_target = pixels;
    o.base5.rest = rest;
    o.base5.kp_joint = joint;
    o.base5.n_keypoints = 3;
    o.base5.nu = 0.02f;
    o.root = placement;
    o.fx = o.fy = 500.f;
    o.cx = 320.f;
    o.cy = 240.f;
    o.rho = 0.f;
    o.nu_rot = 0.02f;
    o.nu_trans = 0.02f;
    o.kp_flags = PNDF_KP_IMAGE;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 168) + (int)(sizeof(pndf_project_options5) != 128);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class ImageRunner:
    """mixed in front of a skeleton_keypoints_oracle.Runner (TwinRunner, UnitRunner): `run` with the 168-byte struct.  -> (status, q_out,
    d_last, kp_energy, root after the call or None)"""

    def run6(self, q, steps, kp, cam=None, root=None, root_weights=(0.0, 0.0), nu=NU, opts=None, words=None, frames=0, lam=0.0, anchor=None,
             aconf=None, mu=0.0, flags=0, in_place=False, make=None):
        q = np.ascontiguousarray(q, np.float32)
        n = len(q)
        cam = cam or cam_of(False)
        held = {"q": self.place(q)}
        if words is not None:
            held["words"] = self.place(np.ascontiguousarray(words, np.uint32).view(np.int32))
        for name, a in (("anchor", anchor), ("aconf", aconf), ("Y", kp["Y"]), ("conf", kp.get("conf")), ("root", root)):
            if a is not None:
                held[name] = self.place(np.ascontiguousarray(a, np.float32))
        held["out"] = held["q"] if in_place else self.filled(q.shape)
        held["d"], held["E"] = self.filled((n,)), self.filled((n,))
        at = {k: self.addr(v) for k, v in held.items()}
        base = sdo.c_from(self.lib, opts or {}, at.get("words"), frames, lam, at.get("anchor"), at.get("aconf"), mu, flags)
        base5 = sk.c_options5(self.lib, base, at["Y"], at.get("conf"), at["E"], ptr(kp["rest"]), ptr(kp.get("kpj")), ptr(kp.get("kpo")),
                              kp["K"] if "K" in kp else len(kp["kpj"]), nu)
        if make is not None:
            opt = make(at, base5)
        else:
            opt = c_options6(self.lib, base5, at.get("root"), cam["camera"], cam["rho"], root_weights[0], root_weights[1], KP_IMAGE if cam["image"] else 0)
        rc = self.project(at["q"], at["out"], at["d"], n, steps, opt)
        return rc, self.fetch(held["out"]), self.fetch(held["d"]), self.fetch(held["E"]), (self.fetch(held["root"]) if "root" in held else None)

    def fit6(self, q, steps, kp, **kw):
        rc, out, d, E, rt = self.run6(q, steps, kp, **kw)
        assert rc == 0, self.last_error()
        return out, d, E, rt


def same_bytes(got, want, what):
    assert (got is None) == (want is None), what
    if got is not None:
        assert_same(np.asarray(got), np.asarray(want), what)


# (image, rho, root given, root weights, mask, keypoint confidences, tracks: None / "held" / "free", the quaternion anchor)
VARIANTS = [(True, 0.0, True, (NU_ROT, NU_TRANS), False, False, None, False),
            (True, RHO, True, (NU_ROT, NU_TRANS), True, True, "free", True),
            (True, 0.0, True, (0.0, NU_TRANS), False, True, "held", True),
            (True, RHO, False, (0.0, 0.0), True, False, None, False),
            (False, 0.0, True, (NU_ROT, NU_TRANS), True, True, "held", False),
            (False, 0.0, True, (NU_ROT, 0.0), False, False, "free", True),
            (False, 0.0, True, (0.0, 0.0), False, True, None, False)]


def check_stated_step(run, case, act):
    """K_STEPS rounds of the runner's own forward_grad + the float32 restatement equal the call with the 168-byte struct, bit for bit:
    poses, d_last, kp_energy and root, for every option set and every variant; a root with zero weights keeps its bytes"""
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
        for image, rho, use_root, weights, use_mask, use_conf, tracks, use_anchor in VARIANTS:
            what = (name, image, rho, use_root, weights, use_mask, use_conf, tracks, use_anchor)
            _, kp, _ = case_kp(case, image=image, conf=use_conf)
            cam = cam_of(image, rho)
            root = start_root if use_root else None
            m = mask if use_mask else None
            anchor = sdo.make_anchor(track, aconf) if use_anchor else None
            step_kw = dict(observed=m, free_ends=tracks == "free", frames=None if tracks else 0, smooth=sk.LAMBDA if tracks else 0.0, **opts)
            if use_anchor:
                step_kw.update(anchor=anchor, conf=aconf, mu=sdo.MU)
            want, dk, Ek, rk = rounds(run.forward_grad, track, K_STEPS, parents, kp, cam, root, weights, **step_kw)
            call_kw = dict(opts=opts, words=words if use_mask else None, frames=T if tracks else 0, lam=sk.LAMBDA if tracks else 0.0,
                           flags=sdo.FREE_ENDS if tracks == "free" else 0, cam=cam, root=root, root_weights=weights)
            if use_anchor:
                call_kw.update(anchor=flat(anchor), aconf=aconf.reshape(-1, J), mu=sdo.MU)
            got, dl, El, rl = run.fit6(flat(track), K_STEPS, kp, **call_kw)
            assert_same(got.reshape(track.shape), want, what)
            assert_same(dl, dk, what + ("d_last",))
            assert_same(El, Ek, what + ("kp_energy",))
            same_bytes(rl, rk, what + ("root",))
            if use_root and not any(weights):
                assert rl.tobytes() == start_root.tobytes(), what
            if use_root and weights[0] == 0:
                assert rl[:, :4].tobytes() == start_root[:, :4].tobytes(), what
            if use_root and any(weights):
                assert rl.tobytes() != start_root.tobytes(), what
            if not tracks:
                again, d_again, E_again, r_again = run.fit6(flat(track), K_STEPS, kp, in_place=True, **call_kw)
                assert again.tobytes() == got.tobytes() and d_again.tobytes() == dl.tobytes() and E_again.tobytes() == El.tobytes(), what + ("in place",)
                same_bytes(r_again, rl, what + ("in place", "root"))


def check_smaller_calls(run, case, act):
    """root NULL, kp_flags 0, zero root weights: the bytes of the 128-byte call.  kp_target NULL or nu == 0 with zero root weights: the
    bytes of the 72-byte call, and a root full of NaN is neither read nor written.  A root with zero weights is not written."""
    parents, kp = sk.case_kp(case)
    J, K = len(parents), len(kp["kpj"])
    track = sdo.clip(case, P, T)
    q = flat(track)
    words = pack(sdo.make_mask(J, P, T))
    anchor = flat(sdo.make_anchor(track))
    nan_root = np.full((B, 7), np.nan, np.float32)
    tol = float(np.median(run.forward(q)))
    for name in sk.OPTION_SETS:
        opts = sk.options(name, tol)
        for w in (None, words):
            for frames, lam, flags in ((0, 0.0, 0), (T, sk.LAMBDA, sdo.FREE_ENDS)):
                for akw in (dict(), dict(anchor=anchor, mu=sdo.MU)):
                    kw = dict(opts=opts, words=w, frames=frames, lam=lam, flags=flags, **akw)
                    what = (name, w is None, frames, sorted(akw))
                    want5, d5, E5 = run.fit(q, K_STEPS, kp=kp, **kw)
                    got, d, E, _ = run.fit6(q, K_STEPS, kp, **kw)
                    assert got.tobytes() == want5.tobytes() and d.tobytes() == d5.tobytes() and E.tobytes() == E5.tobytes(), what
                    want4, d4, _ = run.fit(q, K_STEPS, small=True, **kw)
                    nan_kp = dict(kp, Y=np.full((B, K, 2), np.nan, np.float32), conf=np.full((B, K), np.nan, np.float32))
                    no_target = lambda at, b5: c_options6(run.lib, sk.c_options5(run.lib, b5.base4, None, at.get("conf"), at["E"], ptr(kp["rest"]),  # noqa: E731
                                                                                  ptr(kp["kpj"]), ptr(kp["kpo"]), K, NU), at["root"], CAMERA, RHO, 0.0, 0.0, KP_IMAGE)
                    for variant in (dict(make=no_target), dict(nu=0.0, cam=cam_of(True, RHO))):
                        got, d, E, rt = run.fit6(q, K_STEPS, nan_kp, root=nan_root, **kw, **variant)
                        assert got.tobytes() == want4.tobytes() and d.tobytes() == d4.tobytes() and not E.any(), what + (sorted(variant),)
                        assert rt.tobytes() == nan_root.tobytes(), what
    # without a keypoint term there is no energy for the root to descend: positive root weights leave it as it is, too
    want4, d4, _ = run.fit(q, K_STEPS, small=True)
    _, kpi, _ = case_kp(case)
    root = make_roots(B, 37)
    got, d, E, rt = run.fit6(q, K_STEPS, kpi, nu=0.0, cam=cam_of(True), root=root, root_weights=(NU_ROT, NU_TRANS))
    assert got.tobytes() == want4.tobytes() and d.tobytes() == d4.tobytes() and not E.any() and rt.tobytes() == root.tobytes()
    # a root with zero weights is read and not written
    _, kpi, _ = case_kp(case)
    root = make_roots(B, 37)
    _, _, E, rt = run.fit6(q, K_STEPS, kpi, cam=cam_of(True), root=root)
    _, _, E_none, _ = run.fit6(q, K_STEPS, kpi, cam=cam_of(True))
    assert rt.tobytes() == root.tobytes() and E.tobytes() != E_none.tobytes()


def check_skips(run, case, act):
    """keypoints whose confidence is 0, negative or NaN with NaN targets equal the call without them in the tables; so does, at one step,
    a keypoint behind the camera (its offset moved far behind it), bit for bit"""
    parents, kp, _ = case_kp(case, conf=True, nan_missing=False)
    J, K = len(parents), len(kp["kpj"])
    q = flat(sdo.clip(case, P, T))
    root = make_roots(B, 37)
    cam = cam_of(True, RHO)
    conf = np.abs(np.nan_to_num(kp["conf"], nan=0.5)) + np.float32(0.05)
    off = sorted({0, K - 1}) if K > 2 else [0]
    for k, bad in zip(off, (0.0, np.nan)):
        conf[:, k] = np.float32(bad)
    Y = kp["Y"].copy()
    Y[:, off] = np.nan
    keep = [k for k in range(K) if k not in off]
    less = dict(rest=kp["rest"], kpj=np.ascontiguousarray(kp["kpj"][keep]), kpo=np.ascontiguousarray(kp["kpo"][keep]),
                Y=np.ascontiguousarray(Y[:, keep]), conf=np.ascontiguousarray(conf[:, keep]))
    kw = dict(opts=dict(renormalize="unit"), cam=cam, root=root, root_weights=(NU_ROT, NU_TRANS))
    got = run.fit6(q, K_STEPS, dict(kp, Y=Y, conf=conf), **kw)
    want = run.fit6(q, K_STEPS, less, **kw)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all() and np.isfinite(got[3]).all() and (got[2] > 0).any()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    if len(keep) < 2:
        return
    # behind the camera: every joint at rest, so offsets are in the tree's frame, and the last kept keypoint's offset 100 units down the
    # tree's -z; the roots turn the tree by well under 90 degrees and sit about DEPTH in front, so that keypoint is behind every camera
    qi = q.copy()
    qi[:, :, :] = np.float32([1, 0, 0, 0])      # every joint at rest: global rotations are the identity, offsets are in the tree's frame
    far = dict(less, kpo=less["kpo"].copy())
    far["kpo"][-1] = np.float32([0.0, 0.0, -100.0])
    fewer = dict(rest=less["rest"], kpj=np.ascontiguousarray(less["kpj"][:-1]), kpo=np.ascontiguousarray(less["kpo"][:-1]),
                 Y=np.ascontiguousarray(less["Y"][:, :-1]), conf=np.ascontiguousarray(less["conf"][:, :-1]))
    Pk = sk.positions(qi.astype(np.float64), parents, far["rest"], far["kpj"], far["kpo"])
    assert (place(Pk, root.astype(np.float64))[0][:, -1, 2] < -10.0).all()
    got = run.fit6(qi, 1, far, **kw)
    want = run.fit6(qi, 1, fewer, **kw)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    with_it = run.fit6(qi, 1, dict(far, kpo=less["kpo"]), **kw)      # (in front of the camera the same keypoint does count)
    assert with_it[2].tobytes() != want[2].tobytes()


def check_subtree_locality(run, case, joint):
    """one keypoint, on `joint`, under a camera and a free root: every joint that is not `joint` or one of its ancestors ends with the
    bytes of the call without the keypoint term"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    rest, _, _ = sk.tables(parents)
    q = flat(sdo.clip(case, P, T))
    kp = dict(rest=rest, kpj=np.asarray([joint], np.int32), kpo=np.asarray([[0.3, -0.2, 0.5]], np.float32),
              Y=np.ascontiguousarray(np.random.RandomState(2).uniform(100, 500, (B, 1, 2)), np.float32))
    chain, j = [], joint
    while j >= 0:
        chain.append(j)
        j = parents[j]
    others = [j for j in range(J) if j not in chain]
    assert others and len(chain) > 1
    opts = dict(renormalize="unit", step_size=0.5)
    root = make_roots(B, 37, depth=30.0)      # every keypoint in front of the camera
    plain, d_plain, _ = run.fit(q, 1, opts=opts, small=True)
    got, d, E, rt = run.fit6(q, 1, kp, opts=opts, cam=cam_of(True), root=root, root_weights=(NU_ROT, NU_TRANS), nu=1.0)
    assert got[:, others].tobytes() == plain[:, others].tobytes() and d.tobytes() == d_plain.tobytes()
    assert (got[:, chain] != plain[:, chain]).any(axis=-1).all() and (E > 0).all() and (rt != root).any(axis=-1).all()


BAD_ROWS = sk.BAD_ROWS      # 5, 7, 9, 128, 130, 257


def check_row_locality(run, case, act):
    """B = 300: a NaN pose, a NaN root, an infinite target stay in their own pose and in their own root row"""
    n = 300
    parents, kp, _ = case_kp(case, n)
    q = sko.case_poses(case, n)
    root = make_roots(n, 37)
    bad_q, bad_Y, bad_root = q.copy(), kp["Y"].copy(), root.copy()
    bad_q[7, 0, 2] = bad_q[130] = np.nan
    bad_root[5, 1] = bad_root[128] = np.nan
    bad_Y[9], bad_Y[257, 1] = np.float32(np.inf), np.float32(-np.inf)
    kw = dict(opts=dict(renormalize="unit"), cam=cam_of(True), root_weights=(NU_ROT, NU_TRANS))
    clean = run.fit6(q, K_STEPS, kp, root=root, **kw)
    got = run.fit6(bad_q, K_STEPS, dict(kp, Y=bad_Y), root=bad_root, **kw)
    keep = np.ones(n, bool)
    keep[list(BAD_ROWS)] = False
    assert all(np.isfinite(a).all() for a in clean)
    for row in BAD_ROWS:      # the bad values did arrive
        assert got[0][row].tobytes() != clean[0][row].tobytes() or got[3][row].tobytes() != clean[3][row].tobytes(), row
    for a, b in zip(got, clean):
        assert a[keep].tobytes() == b[keep].tobytes()


# ---------------------------------------------------------------- the effect: pure inverse kinematics of a hand seen by a camera
EFFECT_STEPS, EFFECT_NOISE, EFFECT_ROOT_NOISE = 50, 0.2, (0.05, 0.3)
EFFECT_NU, EFFECT_ROOT_WEIGHTS, EFFECT_DEPTH = 0.3, (0.05, 0.3), 6.0


def effect_inputs(act="lrelu"):
    """(parents, weights with d == 0, start poses [B,J,4], start roots [B,7], kp with pixel targets): a pose and a root generate their own
    pixels (float64, rounded once); the start is the pose plus EFFECT_NOISE * N(0, 1) per component, renormalised, and the root with its
    quaternion perturbed by EFFECT_ROOT_NOISE[0] * N(0, 1) and its translation by EFFECT_ROOT_NOISE[1] * N(0, 1).  The hand has
    sk.EFFECT_REACH's shorter bones.  The residual is in normalised image coordinates at depth about EFFECT_DEPTH, so its gradients are
    smaller than the 3D term's by the depth and its curvature by the depth squared: the weights are larger than the 3D term's 0.02.
    Weights tried on the float64 restatement, as (nu; nu_rot, nu_trans) -> poses of 48 whose energy rises at some step of 50:
    (2.0; 0.5, 2.0) 45, (1.0; 0.2, 1.0) 19, (0.5; 0.1, 0.5) 5, (0.3; 0.05, 0.3) none (E_last / E_0 median 0.022, worst 0.23),
    (0.1; 0.02, 0.1) none (median 0.063, worst 0.38).  The check runs at (0.3; 0.05, 0.3), the largest at which every step falls."""
    parents, sd, _, kp = sk.effect_inputs(act)
    J = len(parents)
    truth = sk.unit_poses(B, J, 31).astype(np.float64)
    truth_root = make_roots(B, 43, depth=EFFECT_DEPTH).astype(np.float64)
    C, _, _, _ = place(sk.positions(truth, parents, kp["rest"], kp["kpj"], kp["kpo"]), truth_root)
    assert (C[..., 2] > 1.0).all()
    kp = dict(kp, Y=np.ascontiguousarray(pixels(C), np.float32))
    r = np.random.RandomState(41)
    x = truth + EFFECT_NOISE * r.randn(*truth.shape)
    x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    rt = truth_root.copy()
    rt[:, :4] += EFFECT_ROOT_NOISE[0] * r.randn(B, 4)
    rt[:, 4:] += EFFECT_ROOT_NOISE[1] * r.randn(B, 3)
    return parents, sd, np.ascontiguousarray(x, np.float32), np.ascontiguousarray(rt, np.float32), kp


def falls(E):
    """E [steps, B]: E falls at every step for every pose, and for the median pose it ends below a tenth of its start (a fixed-step
    descent: how far a pose gets in 50 steps depends on its conditioning, that it falls does not)"""
    E = np.asarray(E, np.float64)
    return bool((np.diff(E, axis=0) < 0).all() and np.median(E[-1] / E[0]) < 0.1)


def oracle_history(nu=EFFECT_NU, weights=EFFECT_ROOT_WEIGHTS, act="lrelu"):
    parents, sd, x, rt, kp = effect_inputs(act)
    _, d, E, _, _ = relax(x[None], sd, EFFECT_STEPS, act, parents, kp, cam_of(True), rt, weights, nu, np.float64, history=True, frames=0, renormalize="unit")
    assert not d.any()      # d == 0 exactly: pure inverse kinematics
    return E


@functools.lru_cache(maxsize=None)
def oracle_effect(act="lrelu"):
    """E of every step of the fp64 oracle [EFFECT_STEPS, B] on effect_inputs; asserted to fall"""
    E = oracle_history(act=act)
    ratio = E[-1] / E[0]
    print(f"[effect] fp64 oracle: E_last / E_0 median {np.median(ratio):.4f} worst {ratio.max():.4f}; steps that do not fall {(np.diff(E, axis=0) >= 0).sum()}")
    assert falls(E), (float(np.median(ratio)), float(ratio.max()), int((np.diff(E, axis=0) >= 0).sum()))
    return E


def check_effect(run):
    """the runner's kp_energy over EFFECT_STEPS chained one-step calls falls as the fp64 oracle's does, and the chained calls are the one
    call of EFFECT_STEPS steps, bit for bit -- poses, energy and root"""
    oracle_effect()
    _, _, x, rt, kp = effect_inputs()
    kw = dict(opts=dict(renormalize="unit"), cam=cam_of(True), root_weights=EFFECT_ROOT_WEIGHTS, nu=EFFECT_NU)
    cur, root, Es = x, rt, []
    for _ in range(EFFECT_STEPS):
        cur, d, E, root = run.fit6(cur, 1, kp, root=root, **kw)
        assert not d.any()
        Es.append(E)
    ratio = Es[-1] / Es[0]
    print(f"[effect] kp_energy: E_last / E_0 median {np.median(ratio):.4f} worst {ratio.max():.4f}")
    assert falls(np.stack(Es)), (float(np.median(ratio)), float(ratio.max()))
    once, _, E_once, root_once = run.fit6(x, EFFECT_STEPS, kp, root=rt, **kw)
    assert once.tobytes() == cur.tobytes() and E_once.tobytes() == Es[-1].tobytes() and root_once.tobytes() == root.tobytes()


# ---------------------------------------------------------------- refusals
def check_refusals(run):
    """every refusal of pndf_project_options6 names its field and writes nothing"""
    import math
    case = ("hand", True)
    n = 8
    parents, kp, _ = case_kp(case, n)
    kp = dict(kp, conf=np.ones((n, len(kp["kpj"])), np.float32))
    J, K = len(parents), len(kp["kpj"])
    q = sko.case_poses(case, n)
    root = make_roots(n, 37)
    lib = run.lib

    def struct(at, b5, **kw):
        f = dict(root=at["root"], camera=CAMERA, rho=0.0, nu_rot=NU_ROT, nu_trans=NU_TRANS, kp_flags=KP_IMAGE)
        f.update({k: (v(at) if callable(v) else v) for k, v in kw.items()})
        return c_options6(lib, b5, **f)

    def refused(field, in_place=False, anchor=None, b5=None, **kw):
        rc, out, d, E, rt = run.run6(q, 2, kp, root=root, in_place=in_place, anchor=anchor, mu=0.5 if anchor is not None else 0.0,
                                     make=lambda at, base5: struct(at, base5 if b5 is None else b5(at, base5), **kw))
        text = run.last_error()
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in text, (field, text)
        assert (out.tobytes() == q.tobytes() if in_place else np.all(out == 7.0)) and np.all(d == 7.0) and np.all(E == 7.0), field
        assert rt.tobytes() == root.tobytes(), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 56, 64, 71, 73, 80, 127, 129, 136, 160, 167, 169, 176):
        refused("struct_size", size=size)
    for bits in (2, 3, 1 << 31):
        refused("kp_flags", kp_flags=bits)
    for bad in (-0.01, math.nan, math.inf, -math.inf):
        refused("rho", rho=bad)
        refused("nu_rot", nu_rot=bad)
        refused("nu_trans", nu_trans=bad)
    refused("rho", rho=0.5, kp_flags=0)
    for bad in (0.0, -1.0, math.nan, math.inf):
        refused("fx", camera=(bad, 480.0, 320.0, 240.0))
        refused("fy", camera=(500.0, bad, 320.0, 240.0))
    for bad in (math.nan, math.inf, -math.inf):
        refused("cx", camera=(500.0, 480.0, bad, 240.0))
        refused("cy", camera=(500.0, 480.0, 320.0, bad))
    refused("root", root=None)
    refused("root", root=None, nu_rot=0.0)
    refused("root", root=None, nu_trans=0.0)
    for odd in (1, 2, 3):
        refused("root", root=lambda at: at["root"] + odd)
    # root overlapping q_out: always; its first and its last float
    refused("root", root=lambda at: at["out"])
    refused("root", root=lambda at: at["out"] + 4 * (n * J * 4 - 1))
    refused("root", root=lambda at: at["out"] - 4 * (n * 7 - 1))
    refused("root", root=lambda at: at["out"], nu_rot=0.0, nu_trans=0.0)
    # with a positive root weight: q_in, anchor, conf, kp_target, kp_conf, kp_energy
    for name in ("q", "anchor", "Y", "conf", "E"):
        refused("root", root=lambda at, name=name: at[name], anchor=q)
    aconf = np.ones((n, J), np.float32)

    def with_conf(at, base5):
        held = run.place(aconf)
        with_conf.keep = held
        base5.base4.conf = run.addr(held)
        with_conf.addr = run.addr(held)
        return base5
    refused("root", b5=with_conf, anchor=q, root=lambda at: with_conf.addr)
    # everything base5 refuses
    def bad_nu(at, base5):
        base5.nu = -1.0
        return base5
    refused("nu", b5=bad_nu)
    def bad_K(at, base5):
        base5.n_keypoints = 65
        return base5
    refused("n_keypoints", b5=bad_K)
    def bad_mu(at, base5):
        base5.base4.mu = 1.5
        return base5
    refused("mu", b5=bad_mu, anchor=q)
    # a good struct after all that: with zero root weights the root may share memory with what is only read (here: the anchor's place)
    rc, out, d, E, rt = run.run6(q, 2, kp, cam=cam_of(True), root=root, root_weights=(NU_ROT, NU_TRANS))
    assert rc == 0 and not np.any(out == 7.0) and not np.any(E == 7.0) and rt.tobytes() != root.tobytes()
    rc, out, d, E, rt = run.run6(q, 2, kp, root=root, make=lambda at, b5: struct(at, b5, root=at["Y"], nu_rot=0.0, nu_trans=0.0))
    assert rc == 0, run.last_error()
