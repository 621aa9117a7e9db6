"""Test helper (not a test module) for 3D keypoint fitting on other skeletons (pndf_project_options5 of include/posendf_amd.h; DESIGN.md
section 2j "Keypoint fitting"): the numpy restatement of csrc/pndf_fk.h -- forward kinematics of a joint tree, the keypoint energy, the
reverse accumulation and the quaternion Jacobian -- operation for operation, for a batch of poses; the fitting step, which extends
tests/skeleton_denoise_oracle.py's denoising step by the term nu * dE/dQ in front of the finish; the free-running oracle; the keypoint
tables, targets and confidences of the tests; the raw C struct and the C99 snippet.  Shared by tests/test_skeleton_keypoints.py (host
twin) and tests/test_skeleton_keypoints_gpu.py (HIP unit).

numpy rounds every operation to the array's dtype and never contracts a multiply into an add, so `energy_grad` and `fit_step` in float32
ARE the specification both implementations are held to bit for bit; the same code in float64 is the truth (its gradient is pinned
against torch autograd of posendf_amd.skeleton.forward_kinematics by tests/test_skeleton_keypoints.py)."""
import ctypes
import functools

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from interpolation_oracle import unit

BAD_ARG = sdo.BAD_ARG
CASES = [("hand", True), ("tree32", True), ("one", True), ("chain32", True), ("hand", False)]
ACTS = sdo.ACTS
OPTION_SETS = sdo.OPTION_SETS
options = sdo.options
flat = sdo.flat
assert_same = sdo.assert_same
pack = sdo.pack
P, T = 6, 8                        # 48 poses
B = P * T
K_STEPS = 3
NU = 0.02


# ---------------------------------------------------------------- the tables
def leaves(parents):
    return [j for j in range(len(parents)) if j not in parents]


@functools.lru_cache(maxsize=None)
def _tables(parents, seed):
    r = np.random.RandomState(seed)
    J = len(parents)
    tips = leaves(parents)
    rest = r.uniform(-1.0, 1.0, (J, 3)).astype(np.float32)
    kpj = np.asarray(list(range(J)) + tips, np.int32)
    kpo = np.concatenate([np.zeros((J, 3), np.float32), r.uniform(-1.0, 1.0, (len(tips), 3)).astype(np.float32)])
    return rest, kpj, np.ascontiguousarray(kpo)


def tables(parents, seed=5):
    """(rest [J,3], kp_joint [K], kp_offset [K,3]): seeded rest offsets in [-1, 1]^3; the keypoints are the J joints (offset zero) plus
    one tip with a seeded offset in [-1, 1]^3 on every leaf"""
    rest, kpj, kpo = _tables(tuple(parents), seed)
    return rest.copy(), kpj.copy(), kpo.copy()


def unit_poses(n, J, seed):
    """[n,J,4] float32, unit per joint, signed"""
    x = np.random.RandomState(seed).randn(n, J, 4)
    return np.ascontiguousarray(x / np.sqrt((x * x).sum(-1, keepdims=True)), np.float32)


def targets(parents, n=B, seed=31):
    """[n,K,3] float32: the keypoints of seeded unit poses under tables(parents) (float64 kinematics, rounded once)"""
    rest, kpj, kpo = tables(parents)
    return np.ascontiguousarray(positions(unit_poses(n, len(parents), seed).astype(np.float64), parents, rest, kpj, kpo), np.float32)


def make_conf(K, n=B, seed=19):
    """float32 [n,K] in (0, 1] with zeros (about one keypoint in six), one negative value and one NaN"""
    r = np.random.RandomState(seed)
    c = (0.05 + 0.95 * r.rand(n, K)).astype(np.float32)
    c[r.rand(n, K) < 1.0 / 6.0] = 0.0
    c[0, 0] = 0.0
    c[n - 1, K - 1] = np.float32(-0.5)
    c[1 % n, 0] = np.float32(np.nan)
    return c


def missing(target, conf):
    """the targets with NaN wherever the confidence is not positive: a missing detection"""
    y = target.copy()
    with np.errstate(invalid="ignore"):
        y[~(conf > 0)] = np.float32(np.nan)
    return y


# ---------------------------------------------------------------- csrc/pndf_fk.h, operation for operation
def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def dot4(x, y):
    return ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]


def fk_unit(Q):
    """Q [B,4] -> (r: list of four [B], n [B])"""
    dt = Q.dtype.type
    c = [Q[:, i] for i in range(4)]
    n = np.sqrt(dot4(c, c))
    den = np.where(n < dt(1e-12), dt(1e-12), n)
    return [ci / den for ci in c], n


def fk_rot(r):
    dt = r[0].dtype.type
    w, x, y, z = r
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    one, two = dt(1), dt(2)
    R = [None] * 9
    R[0] = one - two * (yy + zz)
    R[4] = one - two * (xx + zz)
    R[8] = one - two * (xx + yy)
    R[1] = two * (xy - wz)
    R[3] = two * (xy + wz)
    R[2] = two * (xz + wy)
    R[6] = two * (xz - wy)
    R[5] = two * (yz - wx)
    R[7] = two * (yz + wx)
    return R


def fk_quat_adj(A, r, n):
    dt = n.dtype.type
    two = dt(2)
    w, x, y, z = r
    d0, d1, d2 = A[7] - A[5], A[2] - A[6], A[3] - A[1]
    s01, s02, s12 = A[1] + A[3], A[2] + A[6], A[5] + A[7]
    t0, t1, t2 = A[4] + A[8], A[0] + A[8], A[0] + A[4]
    gr = [None] * 4
    gr[0] = two * dot3(x, d0, y, d1, z, d2)
    cx, cy, cz = x * t0, y * t1, z * t2
    gr[1] = two * (dot3(w, d0, y, s01, z, s02) - two * cx)
    gr[2] = two * (dot3(w, d1, x, s01, z, s12) - two * cy)
    gr[3] = two * (dot3(w, d2, x, s02, y, s12) - two * cz)
    clamped = n < dt(1e-12)
    dot = dot4(r, gr)
    return np.stack([np.where(clamped, gr[c] / dt(1e-12), (gr[c] - r[c] * dot) / n) for c in range(4)], axis=-1)


def _forward(q, parents, rest):
    """per joint: r, n, R (nine [B]), G (nine [B]), p (three [B])"""
    Bn, J = q.shape[:2]
    r, n, R, G, p = [None] * J, [None] * J, [None] * J, [None] * J, [None] * J
    for j in range(J):
        r[j], n[j] = fk_unit(q[:, j])
        R[j] = fk_rot(r[j])
        t = rest[j]
        pa = parents[j]
        if pa < 0:
            G[j] = list(R[j])
            p[j] = [np.full(Bn, t[a], q.dtype) for a in range(3)]
        else:
            Gp = G[pa]
            G[j] = [dot3(Gp[3 * a], R[j][b], Gp[3 * a + 1], R[j][3 + b], Gp[3 * a + 2], R[j][6 + b]) for a in range(3) for b in range(3)]
            p[j] = [p[pa][a] + dot3(Gp[3 * a], t[0], Gp[3 * a + 1], t[1], Gp[3 * a + 2], t[2]) for a in range(3)]
    return r, n, R, G, p


def positions(q, parents, rest, kpj, kpo):
    """the keypoints P [B,K,3] of the poses q [B,J,4] in q's dtype"""
    q = np.asarray(q)
    rest, kpo = np.asarray(rest, q.dtype), np.asarray(kpo, q.dtype)
    with np.errstate(all="ignore"):
        _, _, _, G, p = _forward(q, parents, rest)
        out = [[p[a][x] + dot3(G[a][3 * x], o[0], G[a][3 * x + 1], o[1], G[a][3 * x + 2], o[2]) for x in range(3)] for a, o in zip(kpj, kpo)]
    return np.stack([np.stack(row, axis=-1) for row in out], axis=1)


def energy_grad(q, parents, rest, kpj, kpo, Y, conf=None):
    """pndf_fk_energy_grad for every pose of q [B,J,4], in q's dtype: (E [B], dE/dQ [B,J,4]).  Y [B,K,3], conf [B,K] or None (ones); a
    keypoint whose confidence is not positive takes no part and its target is not looked at."""
    q = np.asarray(q)
    dt = q.dtype.type
    Bn, J = q.shape[:2]
    rest, kpo, Y = np.asarray(rest, q.dtype), np.asarray(kpo, q.dtype), np.asarray(Y, q.dtype)
    zero = np.zeros(Bn, q.dtype)
    with np.errstate(all="ignore"):
        r, n, R, G, p = _forward(q, parents, rest)
        M = [[zero] * 9 for _ in range(J)]
        ap = [[zero] * 3 for _ in range(J)]
        acc = zero
        for k, (a, o) in enumerate(zip(kpj, kpo)):
            w = np.ones(Bn, q.dtype) if conf is None else np.asarray(conf, q.dtype)[:, k]
            on = w > 0
            w = np.where(on, w, dt(0))
            y = np.where(on[:, None], Y[:, k], dt(0))
            res = [(p[a][x] + dot3(G[a][3 * x], o[0], G[a][3 * x + 1], o[1], G[a][3 * x + 2], o[2])) - y[:, x] for x in range(3)]
            e = w * dot3(res[0], res[0], res[1], res[1], res[2], res[2])
            for x in range(3):
                wr = w * res[x]
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
        E = dt(0.5) * acc
    assert E.dtype == q.dtype and g.dtype == q.dtype
    return E, g


# ---------------------------------------------------------------- the step
def fit_step(q, d, g, gk, nu, observed=None, free_ends=False, frames=None, renormalize=None, tol=0.0, **kw):
    """One fitting step on q [P,T,J,4] in q's dtype: skeleton_denoise_oracle.denoise_step's descent, coupling and data term (**kw: anchor,
    conf, mu, smooth, step_size), then u <- u - nu * gk with gk = dE/dQ [P*T,J,4] at q, then the finish; held joints keep q."""
    dt = q.dtype.type
    Pn, Tn, J = q.shape[:3]
    frames = Tn if frames is None else frames
    u = sdo.denoise_step(q, d, g, observed=None, free_ends=free_ends, frames=frames, renormalize=None, tol=0.0, **kw)
    dist = np.asarray(d, dtype=q.dtype).reshape(Pn, Tn, 1, 1)
    held = np.zeros((Pn, Tn, J), bool) if observed is None else np.asarray(observed, bool).reshape(Pn, Tn, J).copy()
    if frames and not free_ends:
        held[:, 0] = held[:, Tn - 1] = True
    with np.errstate(all="ignore"):
        s = dt(nu) * np.asarray(gk, q.dtype).reshape(q.shape)
        u = u - s
        if renormalize is not None:
            assert renormalize in ("unit", "unit_flip"), renormalize
            u = unit(u)
            if renormalize == "unit_flip":
                u = np.where(u[..., :1] < 0, -u, u)
        if tol > 0:
            u = np.where(dist < dt(tol), q, u)
    out = np.where(held[..., None], q, u)
    assert out.dtype == q.dtype
    return out


def term(cur, parents, kp):
    """(E [P*T], dE/dQ [P*T,J,4]) of the keypoint dict kp = dict(rest, kpj, kpo, Y, conf) at the track `cur`"""
    return energy_grad(cur.reshape((-1,) + cur.shape[2:]), parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"], kp.get("conf"))


def rounds(forward_grad, track, steps, parents, kp, nu=NU, **kw):
    """`steps` rounds of { forward_grad(q [B,J,4]) -> (d, dq) of the engine under test ; energy_grad and fit_step in float32 } ->
    (track, d of the last round, E of the last round)"""
    cur = np.ascontiguousarray(track, np.float32).copy()
    d = np.zeros(track.shape[0] * track.shape[1], np.float32)
    E = np.zeros_like(d)
    for _ in range(steps):
        d, g = forward_grad(cur.reshape((-1,) + cur.shape[2:]))
        E, gk = term(cur, parents, kp)
        cur = np.ascontiguousarray(fit_step(cur, d, g, gk, nu, **kw), np.float32)
    return cur, d, E


def relax(track, sd, steps, act, parents, kp, nu=NU, dtype=np.float32, history=False, **kw):
    """free-running oracle: `steps` times skeleton_oracle's forward_grad + energy_grad + fit_step in `dtype` -> (track, d of the last step,
    E of the last step, the smallest kink margin every pose met); history=True: E of every step [steps, P*T] in place of the last"""
    J = len(parents)
    q = np.asarray(track, dtype=dtype)
    n = q.shape[0] * q.shape[1]
    d, E, margin, Es = np.zeros((n, 1), dtype), np.zeros(n, dtype), np.full(n, np.inf), []
    for _ in range(steps):
        d, g, m, _ = sko._run(q.reshape(-1, J, 4), sd, act, parents, dtype)
        margin = np.minimum(margin, m)
        E, gk = term(q, parents, kp)
        Es.append(E)
        q = fit_step(q, d, g, gk, nu, **kw)
    return q, np.asarray(d).reshape(-1), (np.stack(Es) if history else E), margin


def zero_distance(sd):
    """the weights with an output bias of -1e3: behind a relu-family output d == 0 exactly and its gradient too, so the descent is exact
    and a call is pure inverse kinematics (check_distance_zero's trick)"""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    last = max(int(k.split("lin")[1].split(".")[0]) for k in out if k.startswith("dfnet.lin"))
    out[f"dfnet.lin{last}.bias"] = np.full_like(out[f"dfnet.lin{last}.bias"], -1e3)
    return out


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def ptr(a):
    return None if a is None else a.ctypes.data


def c_options5(lib, base=None, target=None, conf=None, energy=None, rest=None, kpj=None, kpo=None, K=0, nu=0.0, size=None, **kw):
    """a pndf_project_options5 (128 bytes); `base`: a filled ProjectOptions4 (default: skeleton_denoise_oracle.c_options4(lib, **kw)); the
    other arguments are addresses (or None), K and nu"""
    from posendf_amd.abi import ProjectOptions5
    o = ProjectOptions5()
    o.base4 = sdo.c_options4(lib, **kw) if base is None else base
    o.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.kp_target, o.kp_conf, o.kp_energy, o.rest, o.kp_joint, o.kp_offset, o.n_keypoints, o.nu = target, conf, energy, rest, kpj, kpo, K, nu
    return o


def c_fit(lib, base, kp, energy=None, nu=NU, target=None, conf=None):
    """the 128-byte struct around the 72-byte `base` for the keypoint dict `kp` (host arrays; `target` / `conf`: addresses that replace
    kp's, for device memory)"""
    return c_options5(lib, base, ptr(kp["Y"]) if target is None else target, (ptr(kp.get("conf")) if conf is None else conf), energy,
                      ptr(kp["rest"]), ptr(kp["kpj"]), ptr(kp["kpo"]), len(kp["kpj"]), nu)


# what a caller of the C header writes: the snippet of the documentation, as strict C99
C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float detections[2 * 3 * 3] = {0};
    static const float conf[2 * 3] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static const float offset[3 * 3] = {0};
    static float energy[2];
    pndf_project_options5 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base4.base3.base2.base);
    o.base4.base3.base2.base.struct_size = sizeof o;
    o.base4.base3.fill = PNDF_TRACK_GIVEN;
    o.kp_target = detections;
    o.kp_conf = conf;
    o.kp_energy = energy;
    o.rest = rest;
    o.kp_joint = joint;
    o.kp_offset = offset;
    o.n_keypoints = 3;
    o.nu = 0.02f;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 128) + (int)(sizeof(pndf_project_options4) != 72);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class Runner:
    """pndf_skel_project (device memory) or pndf_project_ex_cpu (host memory) with numpy in and out.  A subclass says where arrays live:
    place(array) -> holder, addr(holder), fetch(holder) -> numpy, project(q, out, d addresses, n, steps, struct) -> status, last_error(),
    forward(q), forward_grad(q).  The host tables rest / kp_joint / kp_offset are numpy arrays in both."""
    lib = None

    def filled(self, shape, value=7.0):
        return self.place(np.full(shape, value, np.float32))

    def run(self, q, steps, opts=None, words=None, frames=0, lam=0.0, anchor=None, aconf=None, mu=0.0, flags=0, kp=None, nu=NU, in_place=False,
            small=False, make=None):
        """-> (status, q_out, d_last, kp_energy or None); the outputs are prefilled with 7.0.  `small`: the 72-byte struct in place of the
        128-byte one.  `make(addresses: dict, base: the 72-byte struct) -> struct` replaces the struct."""
        q = np.ascontiguousarray(q, np.float32)
        n = len(q)
        held = {"q": self.place(q)}
        if words is not None:
            held["words"] = self.place(np.ascontiguousarray(words, np.uint32).view(np.int32))
        for name, a in (("anchor", anchor), ("aconf", aconf), ("Y", None if kp is None else kp["Y"]), ("conf", None if kp is None else kp.get("conf"))):
            if a is not None:
                held[name] = self.place(np.ascontiguousarray(a, np.float32))
        held["out"] = held["q"] if in_place else self.filled(q.shape)
        held["d"], held["E"] = self.filled((n,)), self.filled((n,))
        at = {k: self.addr(v) for k, v in held.items()}
        base = sdo.c_from(self.lib, opts or {}, at.get("words"), frames, lam, at.get("anchor"), at.get("aconf"), mu, flags)
        if make is not None:
            opt = make(at, base)
        elif small:
            opt = base
        elif kp is None:
            opt = c_options5(self.lib, base, energy=at["E"])
        else:
            opt = c_options5(self.lib, base, at["Y"], at.get("conf"), at["E"], ptr(kp["rest"]), ptr(kp.get("kpj")), ptr(kp.get("kpo")),
                             kp["K"] if "K" in kp else len(kp["kpj"]), nu)
        rc = self.project(at["q"], at["out"], at["d"], n, steps, opt)
        return rc, self.fetch(held["out"]), self.fetch(held["d"]), (None if small else self.fetch(held["E"]))

    def fit(self, q, steps, **kw):
        rc, out, d, E = self.run(q, steps, **kw)
        assert rc == 0, self.last_error()
        return out, d, E


def case_kp(case, n=B, conf=False, nan_missing=True):
    """the keypoint dict of a case: tables(parents), the targets of seeded unit poses and (conf=True) confidences with NaN targets where
    the confidence is not positive"""
    parents = sko.SKELETONS[case[0]]
    rest, kpj, kpo = tables(parents)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=targets(parents, n))
    if conf:
        kp["conf"] = make_conf(len(kpj), n)
        if nan_missing:
            kp["Y"] = missing(kp["Y"], kp["conf"])
    return parents, kp


# (mask, keypoint confidences, tracks: None / "held" / "free" end frames, the quaternion anchor) of the stated-step checks
VARIANTS = [(False, False, None, False), (True, True, "free", True), (False, True, "held", True), (True, False, "held", False),
            (False, False, "free", False), (True, True, None, True)]


def check_stated_step(run, case, act):
    """K_STEPS rounds of the runner's own forward_grad + the float32 restatement equal the call with the 128-byte struct, bit for bit:
    poses, d_last and kp_energy, for every option set and every variant; held joints and held end frames keep their bytes"""
    parents, _ = case_kp(case)
    J = len(parents)
    track = sdo.clip(case, P, T)
    mask = sdo.make_mask(J, P, T)
    words = pack(mask)
    aconf = sdo.make_conf(J, P, T)
    tol = float(np.median(run.forward(flat(track))))
    for name in OPTION_SETS:
        opts = options(name, tol)
        for use_mask, use_conf, tracks, use_anchor in VARIANTS:
            what = (name, use_mask, use_conf, tracks, use_anchor)
            _, kp = case_kp(case, conf=use_conf)
            if use_conf:
                with np.errstate(invalid="ignore"):
                    c = kp["conf"]
                    assert (c == 0).any() and (c < 0).any() and np.isnan(c).any() and np.isnan(kp["Y"][~(c > 0)]).all()
            m = mask if use_mask else None
            anchor = sdo.make_anchor(track, aconf) if use_anchor else None
            step_kw = dict(observed=m, free_ends=tracks == "free", frames=None if tracks else 0, smooth=LAMBDA if tracks else 0.0, **opts)
            if use_anchor:
                step_kw.update(anchor=anchor, conf=aconf, mu=sdo.MU)
            want, dk, Ek = rounds(run.forward_grad, track, K_STEPS, parents, kp, **step_kw)
            call_kw = dict(opts=opts, words=words if use_mask else None, frames=T if tracks else 0, lam=LAMBDA if tracks else 0.0,
                           flags=sdo.FREE_ENDS if tracks == "free" else 0, kp=kp)
            if use_anchor:
                call_kw.update(anchor=flat(anchor), aconf=aconf.reshape(-1, J), mu=sdo.MU)
            got, dl, El = run.fit(flat(track), K_STEPS, **call_kw)
            assert_same(got.reshape(track.shape), want, what)
            assert_same(dl, dk, what + ("d_last",))
            assert_same(El, Ek, what + ("kp_energy",))
            held = mask.copy() if use_mask else np.zeros_like(mask)
            if tracks == "held":
                held[:, 0] = held[:, -1] = True
            assert got.reshape(track.shape)[held].tobytes() == track[held].tobytes(), what
            if not tracks:      # a lane (a pose) reads only its own pose: in place
                again, d_again, E_again = run.fit(flat(track), K_STEPS, in_place=True, **call_kw)
                assert again.tobytes() == got.tobytes() and d_again.tobytes() == dl.tobytes() and E_again.tobytes() == El.tobytes(), what + ("in place",)


LAMBDA = sdo.LAMBDA


def check_smaller_call(run, case, act):
    """kp_target NULL, and nu == 0 with targets and confidences full of NaN: the bytes of the 72-byte call, poses and d_last, with and
    without tracks, a mask and an anchor, in place where that is allowed; kp_energy is zero"""
    parents, kp = case_kp(case)
    J, K = len(parents), len(kp["kpj"])
    track = sdo.clip(case, P, T)
    q = flat(track)
    words = pack(sdo.make_mask(J, P, T))
    nan_kp = dict(kp, Y=np.full((B, K, 3), np.nan, np.float32), conf=np.full((B, K), np.nan, np.float32))
    anchor = flat(sdo.make_anchor(track))
    tol = float(np.median(run.forward(q)))
    for name in OPTION_SETS:
        opts = options(name, tol)
        for w in (None, words):
            for frames, lam, flags in ((0, 0.0, 0), (T, LAMBDA, 0), (T, LAMBDA, sdo.FREE_ENDS)):
                for akw in (dict(), dict(anchor=anchor, mu=sdo.MU)):
                    kw = dict(opts=opts, words=w, frames=frames, lam=lam, flags=flags, **akw)
                    what = (name, w is None, frames, flags, sorted(akw))
                    want, d_want, _ = run.fit(q, K_STEPS, small=True, **kw)
                    for places in ((False, True) if frames == 0 else (False,)):
                        no_target = lambda at, base: c_options5(run.lib, base, None, at.get("conf"), at["E"], ptr(kp["rest"]), ptr(kp["kpj"]), ptr(kp["kpo"]), K, NU)  # noqa: E731
                        for variant in (dict(kp=None), dict(kp=nan_kp, make=no_target), dict(kp=nan_kp, nu=0.0)):
                            got, d_got, E = run.fit(q, K_STEPS, in_place=places, **kw, **variant)
                            assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), what + (places, sorted(variant))
                            assert not E.any(), what


def check_confidences(run, case, act):
    """three keypoints whose confidence is 0, negative and NaN in every pose and whose targets are NaN: finite results, and the bytes of
    the call with those keypoints taken out of the tables"""
    parents, kp = case_kp(case, conf=True, nan_missing=False)
    J, K = len(parents), len(kp["kpj"])
    q = flat(sdo.clip(case, P, T))
    off = sorted({0, K // 2, K - 1})
    conf = np.abs(np.nan_to_num(kp["conf"], nan=0.5)) + np.float32(0.05)
    for k, bad in zip(off, (0.0, -1.0, np.nan)):
        conf[:, k] = np.float32(bad)
    Y = kp["Y"].copy()
    Y[:, off] = np.nan
    keep = [k for k in range(K) if k not in off]
    if not keep:      # one joint: two keypoints
        off, keep = off[:1], [k for k in range(K) if k != off[0]]
        conf[:, keep] = np.float32(0.7)
        Y[:, keep] = kp["Y"][:, keep]
    full = dict(kp, Y=Y, conf=conf)
    less = dict(rest=kp["rest"], kpj=np.ascontiguousarray(kp["kpj"][keep]), kpo=np.ascontiguousarray(kp["kpo"][keep]),
                Y=np.ascontiguousarray(Y[:, keep]), conf=np.ascontiguousarray(conf[:, keep]))
    opts = dict(renormalize="unit")
    got, d, E = run.fit(q, K_STEPS, opts=opts, kp=full)
    want, d_want, E_want = run.fit(q, K_STEPS, opts=opts, kp=less)
    assert np.isfinite(got).all() and np.isfinite(d).all() and np.isfinite(E).all() and (E > 0).all()
    assert got.tobytes() == want.tobytes() and d.tobytes() == d_want.tobytes() and E.tobytes() == E_want.tobytes()


def check_subtree_locality(run, case, joint):
    """one keypoint, on `joint`: every joint that is not `joint` or one of its ancestors ends with the bytes of the call without the
    keypoint term; `joint` and its ancestors do not"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    rest, _, _ = tables(parents)
    q = flat(sdo.clip(case, P, T))
    kp = dict(rest=rest, kpj=np.asarray([joint], np.int32), kpo=np.asarray([[0.3, -0.2, 0.5]], np.float32),
              Y=np.ascontiguousarray(np.random.RandomState(2).uniform(-1, 1, (B, 1, 3)), np.float32))
    chain, j = [], joint
    while j >= 0:
        chain.append(j)
        j = parents[j]
    others = [j for j in range(J) if j not in chain]
    assert others and len(chain) > 1
    opts = dict(renormalize="unit", step_size=0.5)
    plain, d_plain, _ = run.fit(q, 1, opts=opts, small=True)
    got, d, E = run.fit(q, 1, opts=opts, kp=kp)
    assert got[:, others].tobytes() == plain[:, others].tobytes() and d.tobytes() == d_plain.tobytes()
    assert (got[:, chain] != plain[:, chain]).any(axis=-1).all()


BAD_ROWS = (5, 7, 9, 128, 130, 257)      # 7, 130 and 257 sit in three 128-column GEMM tiles (second_order_oracle.BAD_ROWS)


def check_row_locality(run, case, act):
    """B = 300: a NaN target with positive confidence, a NaN pose and a row whose nu-scaled gradient overflows stay in their own pose --
    every other row has the bytes it has when those rows hold ordinary values"""
    n = 300
    parents, kp = case_kp(case, n)
    q = sko.case_poses(case, n)
    bad_q, bad_Y = q.copy(), kp["Y"].copy()
    bad_Y[5, 0, 1] = bad_Y[128, -1] = np.nan
    bad_q[7, 0, 2] = bad_q[130] = np.nan
    bad_Y[9], bad_Y[257, 1] = np.float32(3e38), np.float32(-3e38)      # (keypoint 1: joint 1, which joint 0 carries)
    opts = dict(renormalize="unit")
    clean, d_clean, E_clean = run.fit(q, K_STEPS, opts=opts, kp=kp)
    got, d, E = run.fit(bad_q, K_STEPS, opts=opts, kp=dict(kp, Y=bad_Y))
    keep = np.ones(n, bool)
    keep[list(BAD_ROWS)] = False
    assert np.isfinite(clean).all()
    for row in BAD_ROWS:      # the bad values did arrive: every such row differs from its clean run
        assert got[row].tobytes() != clean[row].tobytes(), row
    assert not np.isfinite(E[[9, 257]]).any()      # the overflow
    assert got[keep].tobytes() == clean[keep].tobytes() and d[keep].tobytes() == d_clean[keep].tobytes() and E[keep].tobytes() == E_clean[keep].tobytes()


# ---------------------------------------------------------------- the effect: pure inverse kinematics on a hand
EFFECT_CASE, EFFECT_STEPS, EFFECT_NOISE = ("hand", True), 50, 0.3


EFFECT_REACH = 0.75      # the rest offsets of the effect's hand lie in [-0.75, 0.75]^3


def effect_inputs(act="lrelu", reach=EFFECT_REACH):
    """(parents, weights with d == 0, start [B,J,4], kp): the targets are the keypoints of seeded unit poses, the start those poses plus
    EFFECT_NOISE * N(0, 1) per component, renormalised.  The step nu * dE/dQ is a gradient step whose length grows with the square of the
    bone lengths; it lowers E only while nu times the curvature of E stays below 2.  With rest offsets in [-1, 1]^3 one of the 48 poses
    sits beyond that in the float64 oracle (E alternates from step 19 on, +0.3 % .. +2 % every other step), with [-0.75, 0.75]^3 none
    does, so the hand of this check has the shorter bones; nu, the noise and the step count stay as they are."""
    parents, sd = sko.case_network(EFFECT_CASE, act)
    _, kp = case_kp(EFFECT_CASE)
    kp["rest"] = np.ascontiguousarray(kp["rest"] * np.float32(reach), np.float32)
    kp["Y"] = np.ascontiguousarray(positions(unit_poses(B, len(parents), 31).astype(np.float64), parents, kp["rest"], kp["kpj"], kp["kpo"]), np.float32)
    truth = unit_poses(B, len(parents), 31).astype(np.float64)      # the poses behind targets()
    x = truth + EFFECT_NOISE * np.random.RandomState(41).randn(*truth.shape)
    x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    return parents, zero_distance(sd), np.ascontiguousarray(x, np.float32), kp


def falls(E):
    """E [steps, B]: E falls at every step for every pose and ends below a tenth of its start"""
    E = np.asarray(E, np.float64)
    return bool((np.diff(E, axis=0) < 0).all() and (E[-1] < 0.1 * E[0]).all())


@functools.lru_cache(maxsize=None)
def oracle_effect(act="lrelu"):
    """E of every step of the fp64 oracle [EFFECT_STEPS, B] on effect_inputs, nu = NU, unit quaternions; asserted to fall"""
    parents, sd, x, kp = effect_inputs(act)
    _, d, E, _ = relax(x[None], sd, EFFECT_STEPS, act, parents, kp, NU, np.float64, history=True, frames=0, renormalize="unit")
    assert not d.any()      # d == 0 exactly: pure inverse kinematics
    ratio = E[-1] / E[0]
    print(f"[effect] fp64 oracle: E_last / E_0 median {np.median(ratio):.4f} worst {ratio.max():.4f}; steps that do not fall {(np.diff(E, axis=0) >= 0).sum()}")
    assert falls(E), (float(np.median(ratio)), float(ratio.max()), int((np.diff(E, axis=0) >= 0).sum()))
    return E


def oracle_effect_at_full_reach(act="lrelu"):
    """the recorded case, not asserted: the same run with rest offsets in [-1, 1]^3 -> (steps of 49 x 48 at which E does not fall, the
    poses they belong to, the worst E_last / E_0)"""
    parents, sd, x, kp = effect_inputs(act, reach=1.0)
    _, _, E, _ = relax(x[None], sd, EFFECT_STEPS, act, parents, kp, NU, np.float64, history=True, frames=0, renormalize="unit")
    up = np.argwhere(np.diff(E, axis=0) >= 0)
    return len(up), sorted(set(up[:, 1].tolist())), float((E[-1] / E[0]).max())


def check_effect(run):
    """the runner's kp_energy over EFFECT_STEPS chained one-step calls falls as the fp64 oracle's does, and the chained calls are the
    one call of EFFECT_STEPS steps, bit for bit"""
    oracle_effect()
    _, _, x, kp = effect_inputs()
    cur, Es = x, []
    for _ in range(EFFECT_STEPS):
        cur, d, E = run.fit(cur, 1, opts=dict(renormalize="unit"), kp=kp)
        assert not d.any()
        Es.append(E)
    ratio = Es[-1] / Es[0]
    print(f"[effect] kp_energy: E_last / E_0 median {np.median(ratio):.4f} worst {ratio.max():.4f}")
    assert falls(np.stack(Es)), (float(np.median(ratio)), float(ratio.max()))
    once, _, E_once = run.fit(x, EFFECT_STEPS, opts=dict(renormalize="unit"), kp=kp)
    assert once.tobytes() == cur.tobytes() and E_once.tobytes() == Es[-1].tobytes()


# ---------------------------------------------------------------- refusals
def check_refusals(run):
    """every refusal of pndf_project_options5 names its field and writes nothing"""
    import math
    case = ("hand", True)
    parents, kp = case_kp(case, 9)
    J, K = len(parents), len(kp["kpj"])
    q = flat(sio.given_track(case, 2, 4))      # 8 poses
    lib = run.lib
    rest, kpj, kpo = kp["rest"], kp["kpj"], kp["kpo"]

    def struct(at, base, **kw):
        f = dict(target=at["Y"], conf=at.get("conf"), energy=at["E"], rest=ptr(rest), kpj=ptr(kpj), kpo=ptr(kpo), K=K, nu=NU)
        f.update(kw)
        return c_options5(lib, base, **f)

    def refused(field, in_place=False, frames=0, lam=0.0, **kw):
        rc, out, d, E = run.run(q, 2, kp=dict(kp, conf=np.ones((9, K), np.float32)), frames=frames, lam=lam, in_place=in_place,
                                make=lambda at, base: struct(at, base, **{k: (v(at) if callable(v) else v) for k, v in kw.items()}))
        text = run.last_error()
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in text, (field, text)
        assert (out.tobytes() == q.tobytes() if in_place else np.all(out == 7.0)) and np.all(d == 7.0) and np.all(E == 7.0), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 56, 64, 71, 73, 80, 127, 129):
        refused("struct_size", size=size)
    for nu in (-0.01, math.nan, math.inf, -math.inf):
        refused("nu", nu=nu)
    for bad in (0, -1, 65, 1 << 20):
        refused("n_keypoints", K=bad)
    refused("rest", rest=None)
    refused("kp_joint", kpj=None)                          # K = 20 keypoints on J = 15 joints
    refused("kp_joint", kpj=None, K=J - 1)
    for where, value in ((0, -1), (K - 1, J), (3, 1 << 30)):
        wrong = kpj.copy()
        wrong[where] = value
        refused("kp_joint", kpj=ptr(wrong))
    for value in (np.nan, np.inf, -np.inf):
        wrong = rest.copy()
        wrong[J - 1, 2] = value
        refused("rest", rest=ptr(wrong))
        wrong = kpo.copy()
        wrong[K - 1, 0] = value
        refused("kp_offset", kpo=ptr(wrong))
    for odd in (1, 2, 3):
        refused("kp_target", target=lambda at: at["Y"] + odd)
        refused("kp_conf", conf=lambda at: at["conf"] + odd)
        refused("kp_energy", energy=lambda at: at["E"] + odd)
        refused("rest", rest=ptr(rest) + odd)
        refused("kp_joint", kpj=ptr(kpj) + odd)
        refused("kp_offset", kpo=ptr(kpo) + odd)
    # kp_energy or kp_target (or kp_conf) overlapping q_out
    refused("kp_energy", energy=lambda at: at["out"])
    refused("kp_energy", energy=lambda at: at["out"] + 4 * (8 * J * 4 - 1))
    refused("kp_target", target=lambda at: at["out"])
    refused("kp_conf", conf=lambda at: at["out"] + 16)
    refused("kp_target", target=lambda at: at["out"], nu=0.0)      # without a term too: the struct names the arrays
    refused("kp_conf", conf=lambda at: at["out"] + 16, nu=0.0)
    # anything refused in base4
    for field, bad in (("mu", dict(mu=1.5)), ("flags", dict(flags=2)), ("frames", dict(frames=3)), ("lambda", dict(frames=4, lam=1.5))):
        rc, out, d, E = run.run(q, 2, kp=kp, make=lambda at, base: struct(at, sdo.c_options4(lib, None, bad.get("frames", 0), bad.get("lam", 0.0),
                                                                                              anchor=at["q"], mu=bad.get("mu", 0.5), flags=bad.get("flags", 0))))
        assert rc == BAD_ARG and field.encode() in run.last_error() and np.all(out == 7.0) and np.all(d == 7.0) and np.all(E == 7.0), field
    for field, bad in (("reserved2", dict(reserved2=1)), ("reserved", dict(reserved=1)), ("step_size", dict(step_size=0.0)), ("tol", dict(tol=math.nan)),
                       ("renorm", dict(renorm=3))):
        rc, out, d, E = run.run(q, 2, kp=kp, make=lambda at, base: struct(at, sdo.c_options4(lib, **bad)))
        assert rc == BAD_ARG and field.encode() in run.last_error() and np.all(out == 7.0) and np.all(d == 7.0) and np.all(E == 7.0), field
    refused("q_out", in_place=True, frames=4, lam=0.5)      # with tracks q_out stays apart from q_in
    # a good struct after all that; keypoint k is joint k when kp_joint is NULL and K == J
    rc, out, d, E = run.run(q, 2, kp=kp, frames=4, lam=0.5)
    assert rc == 0 and not np.any(out == 7.0) and not np.any(E == 7.0)
    ident = dict(rest=rest, kpj=np.arange(J, dtype=np.int32), kpo=np.zeros((J, 3), np.float32), Y=np.ascontiguousarray(kp["Y"][:, :J]))
    want, d_want, E_want = run.fit(q, 2, kp=ident)
    got, d_got, E_got = run.fit(q, 2, kp=dict(rest=rest, Y=ident["Y"], K=J))
    assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes() and E_got.tobytes() == E_want.tobytes()
