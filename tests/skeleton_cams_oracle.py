"""Test helper (not a test module) for moving cameras inside the projection step (pndf_project_options10 of include/posendf_amd.h; DESIGN.md
section 2j "Moving cameras"): a view table per pose [B,V,16], or per frame of a track [T,V,16], in device memory.

The float32 restatement of record is the several-camera restatement that exists (tests/skeleton_views_oracle.py's views_energy_grad,
imported, not copied) applied pose by pose with that pose's block, plus the focal-length skip: a view whose fx > 0 && fy > 0 is false
takes no part for that pose and nothing of it is read.  `energy_grad_by_pose` is that sentence literally.  `stated` is the same
arithmetic for all poses at once: views_energy_grad works elementwise over the poses and indexes its table as vt[v, i], so a table
turned to [V,16,B] gives every pose its own entries, and a view that is skipped is a view whose confidence is zero -- which that
restatement already takes out before anything of the view is used.  tests/test_skeleton_cams.py holds the two to each other bit for bit.
On top: tests/skeleton_root_oracle.py's rounds (the root stepped out of place, coupled) and skeleton_views_oracle's (in place); the raw C
struct; the runner for pndf_skel_project and pndf_project_ex_cpu.  Shared by tests/test_skeleton_cams.py (host twin) and
tests/test_skeleton_cams_gpu.py (HIP unit)."""
import ctypes

import numpy as np

import skeleton_denoise_oracle as sdo
import skeleton_image_oracle as si
import skeleton_keypoints_oracle as sk
import skeleton_length_oracle as sl
import skeleton_oracle as sko
import skeleton_root_oracle as sr
import skeleton_views_oracle as sv

BAD_ARG = sk.BAD_ARG
VIEWS_PER_FRAME = 1
P = sr.P
FRAMES = sr.FRAMES
VIEW_COUNTS = (1, 2, 8)
WEIGHTS = (si.NU_ROT, si.NU_TRANS)
COUPLED = dict(root_smooth=(sr.LAM_ROT, sr.LAM_TRANS), root_data=(sr.MU_ROT, sr.MU_TRANS))
flat, pack, ptr, assert_same, same_bytes = sk.flat, sk.pack, sk.ptr, sk.assert_same, si.same_bytes
lengths = sl.lengths
NAMES = ("poses", "d_last", "kp_energy", "root", "bone_scale")


# ---------------------------------------------------------------- tables and targets
def make_tables(n, V, frames=0, seed=83):
    """[n,V,16] float32: sv.make_views(V) carried along a path -- block b is the rig turned about the world's y axis and moved, further
    with every frame (b % frames, or b) and differently per track, with intrinsics that vary a few percent from block to block (a zoom)"""
    r = np.random.RandomState(seed)
    base = sv.make_views(V).astype(np.float64)
    out = np.empty((n, V, 16))
    for b in range(n):
        k, tr = (b % frames, b // frames) if frames else (b, 0)
        a = 0.04 * (k + 1) * (1.0 + 0.5 * tr) + 0.01 * r.randn()
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        shift = np.array([0.05 * (k + 1), -0.03 * (k + 1) * (1 + tr), 0.04 * k]) + 0.01 * r.randn(3)
        for v in range(V):
            R = base[v, 4:13].reshape(3, 3) @ Ry
            out[b, v] = np.concatenate([base[v, :4] * r.uniform(0.95, 1.05, 4), R.reshape(9), base[v, 13:16] + shift])
    return np.ascontiguousarray(out, np.float32)


def blocks_of(tables, n):
    """the block of every pose [n,V,16]: the table itself, or a table per frame [T,V,16] repeated along the tracks"""
    tables = np.asarray(tables)
    assert n % len(tables) == 0
    return np.ascontiguousarray(np.tile(tables, (n // len(tables), 1, 1)))


def project(Wk, blocks):
    """pixels [B,V,K,2] of world points Wk [B,K,3] in every pose's own views (plain float64 arithmetic: the truth of the targets)"""
    return np.concatenate([sv.project(Wk[b:b + 1], blocks[b])[0] for b in range(len(Wk))], axis=0)


def case_kp(case, blocks, conf=False, root_seed=29):
    """(parents, kp): sv.case_kp with every pose seen by its own block"""
    n = len(blocks)
    parents, kp = sk.case_kp(case, n)
    Pk = sk.positions(sk.unit_poses(n, len(parents), 31).astype(np.float64), parents, kp["rest"], kp["kpj"], kp["kpo"])
    Wk = si.place(Pk, si.make_roots(n, root_seed).astype(np.float64))[0]
    kp["Y"] = np.ascontiguousarray(project(Wk, blocks.astype(np.float64)), np.float32)
    if conf:
        kp["conf"] = sv.make_view_conf(len(kp["kpj"]), n, blocks.shape[1])
        kp["Y"] = sk.missing(kp["Y"], kp["conf"])
    return parents, kp


# ---------------------------------------------------------------- the restatement
def on_views(blocks):
    """[n,V] bool: fx > 0 && fy > 0 (false for a NaN)"""
    with np.errstate(all="ignore"):
        return (blocks[:, :, 0] > 0) & (blocks[:, :, 1] > 0)


def stated(blocks, kp):
    """(views, kp) for sv.views_energy_grad / sv.rounds / sr.rounds: the table turned to [V,16,n] so that vt[v, i] is every pose's own entry,
    and the confidences of a skipped view set to zero (ones with zeros when the call has no confidences: a product with 1 is exact)"""
    blocks = np.asarray(blocks, np.float32)
    n, V = blocks.shape[:2]
    K = len(kp["kpj"])
    conf = kp.get("conf")
    conf = np.ones((n, V, K), np.float32) if conf is None else np.asarray(conf, np.float32)
    conf = np.where(on_views(blocks)[:, :, None], conf, np.float32(0))
    return np.ascontiguousarray(blocks.transpose(1, 2, 0)), dict(kp, conf=np.ascontiguousarray(conf, np.float32))


def energy_grad_by_pose(q, parents, kp, blocks, root=None, rho=0.0, sigma=None):
    """the restatement of record, literally: sv.views_energy_grad pose by pose with that pose's block [V,16]; a skipped view is left out of
    the pose's call altogether -- its row, its targets and its confidences are not even passed -> (E, dE/dQ, dE/d(c, s) or None, h)"""
    out = []
    on = on_views(np.asarray(blocks, np.float32))
    for b in range(len(q)):
        keep = np.flatnonzero(on[b])
        one = slice(b, b + 1)
        conf = None if kp.get("conf") is None else kp["conf"][one][:, keep]
        out.append(sv.views_energy_grad(q[one], parents, kp["rest"], kp["kpj"], kp["kpo"], kp["Y"][one][:, keep], conf, None if root is None else root[one],
                                        rho, blocks[b][keep], None if sigma is None else sigma[one]))
    return tuple(None if parts[0] is None else np.concatenate(parts, axis=0) for parts in zip(*out))


def rounds(forward_grad, track, steps, parents, kp, blocks, rho=0.0, ln=None, root=None, root_weights=(0.0, 0.0), coupled=None, root_anchor=None,
           frames=None, **kw):
    """`steps` rounds of { forward_grad of the engine under test ; the float32 restatement } -> (track, d, E, root, scales).  coupled: None
    (the root stepped in place: sv.rounds) or dict(root_smooth=, root_data=) (out of place: sr.rounds)"""
    views, kp_ = stated(blocks, kp)
    if coupled is None:
        return sv.rounds(forward_grad, track, steps, parents, kp_, views, rho, ln, root, root_weights, frames=frames, **kw)
    return sr.rounds(forward_grad, track, steps, parents, kp_, si.cam_of(True, rho), views, ln, root, root_weights, frames=frames,
                     root_smooth=coupled["root_smooth"], root_anchor=root_anchor, root_data=coupled["root_data"] if root_anchor is not None else (0.0, 0.0), **kw)


# ---------------------------------------------------------------- the C struct as a caller of the header writes it
def c_options10(lib, base9, pose_views=None, n_pose_views=0, view_flags=0, reserved6=0, size=None):
    """a pndf_project_options10 (280 bytes) around a filled ProjectOptions9; pose_views: an address or None"""
    from posendf_amd.abi import ProjectOptions10
    o = ProjectOptions10()
    o.base9 = base9
    o.base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(o) if size is None else size
    o.pose_views, o.n_pose_views, o.view_flags, o.reserved6 = pose_views, n_pose_views, view_flags, reserved6
    return o


C99_SNIPPET = """#include <string.h>
#include "posendf_amd_skeleton.h"
int main(void) {
    static const float pixels[4 * 2 * 3 * 2] = {0};
    static const float rest[2 * 3] = {0};
    static const int32_t joint[3] = {0, 1, 1};
    static float placement[4 * 7] = {1, 0, 0, 0, 0, 0, 5};
    static const float path[2 * 2 * 16] __attribute__((aligned(16))) = {500, 500, 320, 240, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0,
                                                                        500, 500, 320, 240, 0, 0, -1, 0, 1, 0, 1, 0, 0, 5, 0, 5};
    pndf_project_options10 o;
    memset(&o, 0, sizeof o);
    pndf_default_project_options(&o.base9.base8.base7.base6.base5.base4.base3.base2.base);
    o.base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = sizeof o;
    o.base9.base8.base7.base6.base5.base4.base3.frames = 2;
    o.base9.base8.base7.base6.base5.kp_target = pixels;
    o.base9.base8.base7.base6.base5.rest = rest;
    o.base9.base8.base7.base6.base5.kp_joint = joint;
    o.base9.base8.base7.base6.base5.n_keypoints = 3;
    o.base9.base8.base7.base6.base5.nu = 0.1f;
    o.base9.base8.base7.base6.root = placement;
    o.base9.base8.base7.base6.nu_trans = 0.1f;
    o.base9.base8.base7.base6.kp_flags = PNDF_KP_IMAGE;
    o.base9.lambda_trans = 0.5f;
    o.pose_views = path;
    o.n_pose_views = 2;
    o.view_flags = PNDF_VIEWS_PER_FRAME;
    return pndf_project_ex_cpu(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o) + pndf_skel_project(0, 0, 0, 0, 0, 1, (const pndf_project_options*)&o, 0, 0, 0)
           + (int)(sizeof o != 280) + (int)(sizeof(pndf_project_options9) != 256) + (int)(PNDF_VIEWS_PER_FRAME != 1);
}
"""


# ---------------------------------------------------------------- one face for the two entry points
class CamsRunner:
    """mixed in front of a RootRunner: `run` with the 280-byte struct.  -> (status, q_out, d_last, kp_energy, root after the call or None,
    scales after the call or None).  `pose_views` [n,V,16] or (per_frame) [T,V,16] is placed where the poses live; the intrinsics of base6
    hold sv.UNREAD_CAMERA."""

    def run10(self, q, steps, kp, pose_views=None, per_frame=False, rho=0.0, root_smooth=(0.0, 0.0), root_anchor=None, root_data=(0.0, 0.0), make10=None,
              **kw):
        table = None if pose_views is None else np.ascontiguousarray(pose_views, np.float32)
        held = None if table is None else self.place(table)
        assert held is None or self.addr(held) % 16 == 0

        def make9(at, o8):
            at = dict(at, pose_views=None if held is None else self.addr(held))
            o9 = sr.c_options9(self.lib, o8, at["root_anchor"], root_smooth[0], root_smooth[1], root_data[0], root_data[1])
            if make10 is not None:
                return make10(at, o9)
            return c_options10(self.lib, o9, at["pose_views"], 0 if table is None else table.shape[1], VIEWS_PER_FRAME if per_frame else 0)
        kw.setdefault("cam", si.cam_of(True, rho, sv.UNREAD_CAMERA if table is not None else si.CAMERA))
        out = self.run9(q, steps, kp, root_anchor=root_anchor, make9=make9, rho=rho, **kw)
        if held is not None:
            assert self.fetch(held).tobytes() == table.tobytes()      # the table is never written
        return out

    def fit10(self, q, steps, kp, **kw):
        rc, out, d, E, rt, sg = self.run10(q, steps, kp, **kw)
        assert rc == 0, self.last_error()
        return out, d, E, rt, sg


# ---------------------------------------------------------------- fixtures and shared checks
def scales_of(case, kp, n, frames, on=True):
    if not on:
        return lengths(None)
    S = len(sko.SKELETONS[case[0]]) + len(kp["kpj"])
    G, _ = sl.groups_of(n, frames, False)
    return lengths(sl.make_scales(G, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S))


def variants():
    """(scales, root coupling and anchor) of the grids"""
    return [(False, False), (True, False), (False, True), (True, True)]


def check_reduction_to_static(run, case, V):
    """a per-pose table and a per-frame table whose every block is one [V,16] table give the bytes of the 224 / 256-byte call with that
    table: poses, d_last, kp_energy, root and bone_scale -- with and without scales, with and without the root's coupling and anchor, an
    even and an odd step count"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    views = sv.make_views(V)
    for T in FRAMES:
        n = P * T
        track = sdo.clip(case, P, T)
        q = flat(track)
        _, kp = sv.case_kp(case, views, n, conf=True)
        root = si.make_roots(n, 37)
        anchor = sr.make_anchor(root)
        for scaled, coupled in variants():
            ln = scales_of(case, kp, n, T, scaled)
            kw = dict(opts=dict(renormalize="unit", step_size=0.5), words=pack(sdo.make_mask(J, P, T)), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS,
                      rho=si.RHO, ln=ln, root=root, root_weights=WEIGHTS)
            if coupled:
                kw.update(COUPLED, root_anchor=anchor)
            for steps in (2, 3):
                want = run.fit9(q, steps, kp, views=views, cam=si.cam_of(True, si.RHO, sv.UNREAD_CAMERA), **kw)
                per_pose = run.fit10(q, steps, kp, pose_views=np.tile(views, (n, 1, 1)), **kw)
                per_frame = run.fit10(q, steps, kp, pose_views=np.tile(views, (T, 1, 1)), per_frame=True, **kw)
                for a, b, c, name in zip(per_pose, per_frame, want, NAMES):
                    same_bytes(a, c, (V, T, scaled, coupled, steps, "per pose", name))
                    same_bytes(b, c, (V, T, scaled, coupled, steps, "per frame", name))
                assert (want[3] != root).any()


def check_stated_step(run, case, V, step_counts=(0, 1, 2, 3)):
    """blocks that differ per pose (a rig turning and moving along the frames, differently per track, with a zoom): rounds of the runner's
    own forward_grad + the float32 restatement equal the call bit for bit; PNDF_VIEWS_PER_FRAME equals the restatement with the
    [T,V,16] table repeated for every track"""
    parents = sko.SKELETONS[case[0]]
    J = len(parents)
    moved = 0
    for T in FRAMES:
        n = P * T
        track = sdo.clip(case, P, T)
        q = flat(track)
        root = si.make_roots(n, 37)
        anchor = sr.make_anchor(root)
        words = pack(sdo.make_mask(J, P, T))
        tol = float(np.median(run.forward(q)))
        for per_frame in (False, True):
            tables = make_tables(T if per_frame else n, V, T)
            blocks = blocks_of(tables, n)
            _, kp = case_kp(case, blocks, conf=True)
            for i, (scaled, coupled) in enumerate(variants()):
                ln = scales_of(case, kp, n, T, scaled)
                name = sorted(sk.OPTION_SETS)[(i + per_frame) % len(sk.OPTION_SETS)]
                opts = sk.options(name, tol)
                for steps in step_counts:
                    what = (V, T, per_frame, scaled, coupled, name, steps)
                    want = rounds(run.forward_grad, track, steps, parents, kp, blocks, si.RHO, ln, root, WEIGHTS, COUPLED if coupled else None,
                                  anchor if coupled else None, observed=sdo.make_mask(J, P, T), free_ends=True, smooth=sk.LAMBDA, **opts)
                    got = run.fit10(q, steps, kp, pose_views=tables, per_frame=per_frame, opts=opts, words=words, frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS,
                                    rho=si.RHO, ln=ln, root=root, root_weights=WEIGHTS, **(dict(COUPLED, root_anchor=anchor) if coupled else {}))
                    assert_same(got[0].reshape(track.shape), want[0], what)
                    for a, b, part in list(zip(got, want, NAMES))[1:]:
                        same_bytes(a, b, what + (part,))
                    moved += int(steps > 0 and (got[3] != root).any())
    assert moved


def check_locality(run, case, V):
    """without tracks a pose's block is that pose's alone: another block for pose c changes pose c's outputs and no other pose's.  With
    tracks coupled by lambda: one step equals the restatement."""
    parents = sko.SKELETONS[case[0]]
    T = 5
    n = P * T
    track = sdo.clip(case, P, T)
    q = flat(track)
    tables = make_tables(n, V, T)
    _, kp = case_kp(case, tables, conf=True)
    root = si.make_roots(n, 37)
    ln = scales_of(case, kp, n, 0, True)      # without tracks: a row of scales per pose
    kw = dict(opts=dict(renormalize="unit", step_size=0.5), rho=si.RHO, ln=ln, root=root, root_weights=WEIGHTS)
    clean = run.fit10(q, 3, kp, pose_views=tables, **kw)
    c = 7
    other = tables.copy()
    other[c] = make_tables(n, V, T, seed=5)[(c + 3) % n]
    got = run.fit10(q, 3, kp, pose_views=other, **kw)
    rest = np.arange(n) != c
    for a, b, name in zip(got, clean, NAMES):
        assert a[rest].tobytes() == b[rest].tobytes(), (V, name, "another pose changed")
        if name != "d_last":      # (the distance of the last step's input differs only once the pose has moved: 3 steps)
            assert a[c].tobytes() != b[c].tobytes(), (V, name, "the pose did not change")
    ln = scales_of(case, kp, n, T, True)
    tr = dict(kw, ln=ln, frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS)
    want = rounds(run.forward_grad, track, 1, parents, kp, other, si.RHO, ln, root, WEIGHTS, COUPLED, free_ends=True, smooth=sk.LAMBDA, renormalize="unit",
                  step_size=0.5)
    got = run.fit10(q, 1, kp, pose_views=other, root_smooth=COUPLED["root_smooth"], **tr)
    assert_same(got[0].reshape(track.shape), want[0], (V, "tracks"))
    for a, b, part in list(zip(got, want, NAMES))[1:]:
        same_bytes(a, b, (V, "tracks", part))


def check_skip(run, case, V):
    """a view whose fx is 0, whose fy is negative, whose fx is NaN, and a row of zeros whose targets and confidences hold NaN: the outputs
    are those of the call with valid rows and that view's confidences zero for that pose, and nothing is NaN.  Every view of a pose
    skipped: its energy is 0 and its pose takes the step of the prior alone."""
    parents = sko.SKELETONS[case[0]]
    T = 5
    n = P * T
    track = sdo.clip(case, P, T)
    q = flat(track)
    tables = make_tables(n, V, T)
    _, kp = case_kp(case, tables, conf=False)
    K = len(kp["kpj"])
    r = np.random.RandomState(3)
    conf = np.ascontiguousarray(r.uniform(0.25, 1.0, (n, V, K)), np.float32)
    root = si.make_roots(n, 37)
    ln = scales_of(case, kp, n, T, True)
    kw = dict(opts=dict(renormalize="unit", step_size=0.5), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, rho=si.RHO, ln=ln, root=root, root_weights=WEIGHTS,
              root_smooth=COUPLED["root_smooth"])
    bad, off, Y = tables.copy(), conf.copy(), kp["Y"].copy()
    edits = [(1, 0, lambda row: row.__setitem__(0, 0.0)), (4, V - 1, lambda row: row.__setitem__(1, -500.0)), (8, V // 2, lambda row: row.__setitem__(0, np.nan)),
             (11, 0, lambda row: row.__setitem__(slice(None), 0.0))]
    for pose, v, edit in edits:
        edit(bad[pose, v])
        off[pose, v] = 0.0
    bad_conf = conf.copy()
    bad_conf[11, 0] = np.nan
    Y[11, 0] = np.nan
    for v in range(V):      # every view of pose 13
        bad[13, v, :2] = (0.0, np.nan) if v % 2 else (-1.0, 300.0)
        bad[13, v, 4:] = np.nan
        off[13, v] = 0.0
    Y[13] = np.nan
    bad_conf[13] = np.nan
    for steps in (1, 2, 3):
        want = run.fit10(q, steps, dict(kp, conf=off), pose_views=tables, **kw)
        got = run.fit10(q, steps, dict(kp, Y=Y, conf=bad_conf), pose_views=bad, **kw)
        for a, b, name in zip(got, want, NAMES):
            same_bytes(a, b, (V, steps, name))
            assert np.isfinite(a).all(), (V, steps, name)
    # the restatement says the same
    want = rounds(run.forward_grad, track, 2, parents, dict(kp, Y=Y, conf=bad_conf), bad, si.RHO, ln, root, WEIGHTS, dict(COUPLED, root_data=(0.0, 0.0)),
                  free_ends=True, smooth=sk.LAMBDA, renormalize="unit", step_size=0.5)
    got = run.fit10(q, 2, dict(kp, Y=Y, conf=bad_conf), pose_views=bad, **kw)
    assert_same(got[0].reshape(track.shape), want[0], (V, "restated"))
    # every view skipped: E = 0, and with the track's other poses left out (no tracks) the pose takes the 72-byte call's step
    alone = dict(opts=kw["opts"], rho=si.RHO, root=root[13:14], root_weights=WEIGHTS)
    out, d, E, rt, _ = run.fit10(q[13:14], 2, dict(kp, Y=Y[13:14], conf=bad_conf[13:14]), pose_views=bad[13:14], **alone)
    prior, dp, _ = run.fit(q[13:14], 2, small=True, opts=kw["opts"])
    assert not E.any() and out.tobytes() == prior.tobytes() and d.tobytes() == dp.tobytes() and np.isfinite(rt).all()


def check_refusals(run, sizes=(257, 264, 272, 279, 281, 288)):
    """every refusal of pndf_project_options10 names its field and writes nothing"""
    case = ("hand", True)
    T = 5
    n = P * T
    q = flat(sdo.clip(case, P, T))
    V = 2
    tables = make_tables(n, V, T)
    _, kp = case_kp(case, tables)
    root = si.make_roots(n, 37)
    S = len(sko.SKELETONS["hand"]) + len(kp["kpj"])
    ln = lengths(sl.make_scales(P, S), sl.NU_LEN, sl.KAPPA, sl.make_rates(S))
    static = sv.make_views(V)

    def refused(field, frames=T, o9=None, table=tables, **f):
        def make10(at, base9):
            g = dict(pose_views=at["pose_views"], n_pose_views=V, view_flags=0)
            g.update({k: (v(at) if callable(v) else v) for k, v in f.items()})
            if o9 is not None:
                base9 = o9(at, base9)
            return c_options10(run.lib, base9, **g)
        rc, out, d, E, rt, sg = run.run10(q, 2, kp, pose_views=table, root=root, root_weights=WEIGHTS, frames=frames, lam=sk.LAMBDA if frames else 0.0,
                                          flags=sdo.FREE_ENDS if frames else 0, ln=ln if frames else lengths(None), make10=make10)
        assert rc == BAD_ARG, (field, f, rc)
        assert field.encode() in run.last_error(), (field, run.last_error())
        assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(E == 7.0), field
        assert rt.tobytes() == root.tobytes() and (sg is None or sg.tobytes() == ln["scale"].tobytes()), field

    for size in sizes:
        refused("struct_size", size=size)
    refused("reserved6", reserved6=1)
    refused("reserved6", reserved6=1 << 40)
    refused("view_flags", view_flags=2)
    refused("view_flags", view_flags=VIEWS_PER_FRAME | 0x80000000)
    refused("n_pose_views", n_pose_views=0)
    refused("n_pose_views", n_pose_views=9)
    refused("n_pose_views", n_pose_views=-1)
    refused("pose_views", pose_views=None)
    refused("view_flags", pose_views=None, n_pose_views=0, view_flags=VIEWS_PER_FRAME)
    refused("PNDF_VIEWS_PER_FRAME", frames=0, view_flags=VIEWS_PER_FRAME)
    for odd in (4, 8, 12, 1):
        refused("pose_views must be 16-byte aligned", pose_views=lambda at, odd=odd: at["pose_views"] + odd)
    # one table or the other
    held = np.ascontiguousarray(static)

    def both(at, b9):
        b9.base8.views, b9.base8.n_views = held.ctypes.data, V
        return b9
    refused("one table or the other", o9=both)
    refused("PNDF_KP_IMAGE", o9=lambda at, b9: (setattr(b9.base8.base7.base6, "kp_flags", 0), b9)[1])
    refused("kp_target", o9=lambda at, b9: (setattr(b9.base8.base7.base6.base5, "kp_target", None), b9)[1])
    # overlaps: q_out, the root (it is stepped), the scales (they are stepped)
    floats = n * V * 16
    refused("pose_views must not overlap q_out", pose_views=lambda at: at["out"])
    refused("pose_views must not overlap q_out", pose_views=lambda at: at["out"] - 4 * (floats - 4))
    # (a table of one view per frame is 320 bytes: it fits inside the root's 420 and the scales' 420, whatever lies beside them)
    inside = dict(n_pose_views=1, view_flags=VIEWS_PER_FRAME)
    refused("pose_views must not overlap pndf_project_options6.root", pose_views=lambda at: at["root"] + (-at["root"]) % 16, **inside)
    refused("pose_views must not overlap pndf_project_options7.bone_scale", pose_views=lambda at: at["scale"] + (-at["scale"]) % 16, **inside)
    # whatever base9 refuses
    refused("reserved5", o9=lambda at, b9: (setattr(b9, "reserved5", 1), b9)[1])
    refused("reserved4", o9=lambda at, b9: (setattr(b9.base8, "reserved4", 1), b9)[1])


def check_empty_struct(run, case):
    """a 280-byte struct without a table is the 256-byte call, bit for bit"""
    T = 5
    n = P * T
    q = flat(sdo.clip(case, P, T))
    kp, views, ln, cam = sr.term_inputs(case, "views2", n, T)
    root = si.make_roots(n, 37)
    kw = dict(opts=dict(renormalize="unit"), frames=T, lam=sk.LAMBDA, flags=sdo.FREE_ENDS, views=views, cam=cam, rho=si.RHO, ln=ln, root=root,
              root_weights=WEIGHTS, root_anchor=sr.make_anchor(root), **COUPLED)
    for steps in (2, 3):
        for a, b, name in zip(run.fit10(q, steps, kp, **kw), run.fit9(q, steps, kp, **kw), NAMES):
            same_bytes(a, b, (steps, name))


# ---------------------------------------------------------------- the effect, on the float64 restatement alone
EFFECT = dict(T=24, steps=150, noise=1.5, lam=(0.0, 0.5), weights=(0.0, 0.05), nu=0.05, seed=11, V=2, rig_shift=1.2, rig_turn=0.35)


def effect_inputs():
    """a 15-joint hand that moves in a world frame, seen by a two-camera rig (a headset: two views 0.12 apart) that translates by
    `rig_shift` along x and turns by `rig_turn` rad about y over the clip: (parents, weights with d == 0, true track [1,T,J,4], kp with
    noisy pixel targets [T,2,K,2], the true tables [T,2,16], start roots [T,7], true roots [T,7]).  The schedule is
    profiles/skeleton_root/effect.json's."""
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
    tables = np.zeros((T, EFFECT["V"], 16))
    for k in range(T):
        a = EFFECT["rig_turn"] * t[k]
        R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])      # world -> rig
        centre = np.array([EFFECT["rig_shift"] * t[k], 0.0, 0.0])                              # the rig's position in the world
        for v in range(EFFECT["V"]):
            eye = np.array([(v - 0.5) * 0.12, 0.0, 0.0])                                       # the camera's position in the rig
            tables[k, v] = np.concatenate([si.CAMERA, R.reshape(9), -(R @ centre) - eye])
    Pk = sk.positions(track, parents, rest, kpj, kpo)
    Wk = si.place(Pk, true_root)[0]
    pix = project(Wk, tables) + EFFECT["noise"] * r.randn(T, EFFECT["V"], len(kpj), 2)
    kp = dict(rest=rest, kpj=kpj, kpo=kpo, Y=np.ascontiguousarray(pix, np.float32))
    start = true_root.copy()
    start[:, 6] += 0.3
    return parents, sd, np.ascontiguousarray(track[None], np.float32), kp, np.ascontiguousarray(tables, np.float32), np.ascontiguousarray(start, np.float32), true_root


def oracle_effect():
    """-> dict(rms_moving, rms_frozen, energy_moving, energy_frozen): the RMS error of the fitted world root translation over the clip and
    the mean final reprojection energy, fitted with the true table of every frame and with frame 0's table for every frame (what a caller
    of the 256-byte struct can do), the root's translation coupled in both, on the float64 restatement"""
    parents, sd, track, kp, tables, start, true_root = effect_inputs()
    T = EFFECT["T"]
    out = {}
    for name, blocks in (("moving", tables), ("frozen", np.tile(tables[:1], (T, 1, 1)))):
        views, kp_ = stated(blocks, kp)
        _, Es, rt = sr.relax(track, sd, EFFECT["steps"], "lrelu", parents, kp_, si.cam_of(True, 0.0), views, start, EFFECT["weights"], nu=EFFECT["nu"], frames=T,
                             root_smooth=EFFECT["lam"], free_ends=True, smooth=0.0, renormalize="unit")
        out["rms_" + name] = float(np.sqrt(np.mean(((rt[:, 4:] - true_root[:, 4:]) ** 2).sum(-1))))
        out["energy_" + name] = float(Es[-1].mean())
    return out
