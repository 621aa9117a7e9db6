"""Motion denoising for other skeletons on an MI355X (pndf_project_options4 of include/posendf_amd.h, csrc/pndf_skeleton.hip; DESIGN.md
section 2j "Motion denoising"): pndf_skel_project with an observation and free end frames against the numpy statement of the denoising
step (tests/skeleton_denoise_oracle.py).

1. the stated step: K rounds of pndf_skel_forward_grad + the numpy step equal the call with the 72-byte struct, bit for bit, for every
   option set, with and without a mask, confidences and free end frames, with tracks and without.  42 tracks of 7 frames = 294 lanes:
   two workgroups of the encoder kernels, track 36 across their border.
2. same bits: anchor NULL and flags 0 is the 48-byte call, mu 0 with anchors of NaN too, without tracks the 32-byte call; one step.
3. the chunk seam: T = 7 and 2,342 tracks with anchors, confidences and free ends; in place without tracks.
4. the refusals; the persistent engine keeps refusing the larger struct.
5. ten free-running steps against the fp64 oracle under conftest's outlier_gate at 1e-4; the device against the twin.
6. `SkeletonPoseNDF.denoise` and `PoseDenoising` on cuda; the exported kernel.
tests/test_skeleton_denoise.py holds the host twin to the same statements."""
import ctypes
import functools
import math

import numpy as np
import pytest

import skeleton_completion_oracle as sco
import skeleton_denoise_oracle as sdo
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from conftest import outlier_gate, rel_err_rows
from posendf_amd import synth
from test_skeleton_completion_gpu import Unit, cuda_model, torch_cuda, unit_of  # noqa: F401  (torch_cuda: the fixture)

pytestmark = pytest.mark.gpu
BAD_ARG = sdo.BAD_ARG
P, T, K = 42, sio.T, sdo.K      # 294 poses
TOL = 1e-4
FREE_STEPS = 10
CASES = sdo.CASES + [c for c in sko.CASES if c not in sdo.CASES]      # the second encoder-less case, ("tree32", False), besides
VARIANTS = [(False, False, False), (True, True, True), (False, True, True), (True, False, False), (False, False, True)]
flat = sdo.flat


def denoise_call(unit, q, steps, words=None, opts=None, frames=T, lam=0.0, anchor=None, conf=None, mu=0.0, flags=0, in_place=False, make=None):
    """(status, q_out, d_last) of pndf_skel_project with a 72-byte struct; q, words, anchor and conf go to the device; the outputs are
    prefilled with 7.0.  `make(words address, anchor address, conf address)`: the struct, where it is not c_from's."""
    torch = unit.torch
    dq, (ws, n) = unit.dev(q), unit.ws(len(q))
    w = None if words is None else unit.words(words)
    a = None if anchor is None else unit.dev(anchor)
    c = None if conf is None else unit.dev(conf)
    at = [None if t is None else t.data_ptr() for t in (w, a, c)]
    opt = make(*at) if make else sdo.c_from(unit.lib, opts or {}, at[0], frames, lam, at[1], at[2], mu, flags)
    out = dq if in_place else torch.full(dq.shape, 7.0, device="cuda:0")
    d = torch.full((len(q),), 7.0, device="cuda:0")
    rc = unit.lib.pndf_skel_project(unit.h, dq.data_ptr(), out.data_ptr(), d.data_ptr(), len(q), steps, ctypes.byref(opt), ws.data_ptr(), n, unit.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), d.cpu().numpy()


def denoised(unit, q, steps, words=None, opts=None, **kw):
    rc, out, d = denoise_call(unit, q, steps, words, opts, **kw)
    assert rc == 0, unit.lib.pndf_skel_last_error(unit.h)
    return out, d


def tracked(unit, q, steps, words, opts=None, frames=T, lam=0.0):
    rc, out, d = unit.call(q, steps, lambda at: sio.c_from(unit.lib, opts or {}, at, frames, lam), words)
    assert rc == 0, unit.lib.pndf_skel_last_error(unit.h)
    return out, d


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", CASES, ids=sko.case_id)
def test_denoising_steps_are_the_stated_step(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    track = sdo.clip(case, P, T)
    mask = sdo.make_mask(J, P, T)
    words = sdo.pack(mask)
    conf = sdo.make_conf(J, P, T)
    tol = float(np.median(unit.forward(flat(track))))
    for name in sdo.OPTION_SETS:
        opts = sdo.options(name, tol)
        for use_mask, use_conf, free in VARIANTS:
            m, c = (mask if use_mask else None), (conf if use_conf else None)
            anchor = sdo.make_anchor(track, c)
            what = (name, use_mask, use_conf, free)
            want, dk = sdo.rounds(unit.forward_grad, track, K, anchor=anchor, conf=c, mu=sdo.MU, observed=m, smooth=sdo.LAMBDA, free_ends=free, **opts)
            got, dl = denoised(unit, flat(track), K, words if use_mask else None, opts, lam=sdo.LAMBDA, anchor=flat(anchor),
                               conf=None if c is None else c.reshape(-1, J), mu=sdo.MU, flags=sdo.FREE_ENDS if free else 0)
            sdo.assert_same(got.reshape(track.shape), want, what)
            sdo.assert_same(dl, dk, what + ("d_last",))
            held = mask.copy() if use_mask else np.zeros_like(mask)
            if not free:
                held[:, 0] = held[:, -1] = True
            assert got.reshape(track.shape)[held].tobytes() == track[held].tobytes(), what
            if free:
                continue
            want, dk = sdo.rounds(unit.forward_grad, track, K, anchor=anchor, conf=c, mu=sdo.MU, observed=m, frames=0, **opts)
            kw = dict(frames=0, anchor=flat(anchor), conf=None if c is None else c.reshape(-1, J), mu=sdo.MU)
            got, dl = denoised(unit, flat(track), K, words if use_mask else None, opts, **kw)
            sdo.assert_same(got.reshape(track.shape), want, what + ("no tracks",))
            sdo.assert_same(dl, dk, what + ("no tracks", "d_last"))
            again, d_again = denoised(unit, flat(track), K, words if use_mask else None, opts, in_place=True, **kw)      # a lane reads only its own pose
            assert again.tobytes() == got.tobytes() and d_again.tobytes() == dl.tobytes(), what + ("in place",)


# ------------------------------------------------------------------------------------------ 2. same bits, one step
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_an_observation_it_is_the_smaller_call(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    q = flat(sdo.clip(case, P, T))
    words = sdo.pack(sdo.make_mask(J, P, T))
    nan = np.full(q.shape, np.nan, np.float32)
    conf = sdo.make_conf(J, P, T).reshape(-1, J)
    tol = float(np.median(unit.forward(q)))
    for name in sdo.OPTION_SETS:
        opts = sdo.options(name, tol)
        for w in (None, words):
            for lam in (0.0, sdo.LAMBDA):
                want, d_want = tracked(unit, q, K, w, opts, lam=lam)
                for kw in (dict(), dict(anchor=nan), dict(anchor=nan, conf=conf)):      # mu == 0: the anchors are never read
                    got, d_got = denoised(unit, q, K, w, opts, lam=lam, **kw)
                    assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), (name, w is None, lam, sorted(kw))
            small, d_small = unit.masked(q, K, w, opts)      # tracks off, free ends off, mu 0: the 32-byte call
            for kw in (dict(), dict(anchor=nan)):
                got, d_got = denoised(unit, q, K, w, opts, frames=0, **kw)
                assert got.tobytes() == small.tobytes() and d_got.tobytes() == d_small.tobytes(), (name, w is None, sorted(kw))


@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_one_step(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    track = sdo.clip(case, P, T)
    q = flat(track)
    mask = sdo.make_mask(J, P, T)
    words = sdo.pack(mask)
    opts = dict(renormalize="unit")
    anchor = sdo.make_anchor(track)
    plain, _ = tracked(unit, q, 1, words, opts, lam=sdo.LAMBDA)
    plain = plain.reshape(track.shape)
    conf = np.ones((P, T, J), np.float32)
    off = np.zeros((P, T, J), bool)
    off[0, 2, 0], off[2, 1, J - 1], off[40, 3, J // 2] = True, True, True      # (track 40: the second workgroup)
    conf[0, 2, 0], conf[2, 1, J - 1], conf[40, 3, J // 2] = 0.0, np.nan, -1.0
    a = anchor.copy()
    a[off] = np.nan
    got, d = denoised(unit, q, 1, words, opts, lam=sdo.LAMBDA, anchor=flat(a), conf=conf.reshape(-1, J), mu=sdo.MU)
    got = got.reshape(track.shape)
    assert np.isfinite(got).all() and np.isfinite(d).all()
    assert got[off].tobytes() == plain[off].tobytes()      # no confidence: the bits of the unanchored call, the NaN anchor not read
    interior = np.zeros((P, T, J), bool)
    interior[:, 1:-1] = True
    pulled = interior & ~off & ~mask
    assert (got[pulled] != plain[pulled]).any(axis=-1).all()
    assert mask.any() and got[mask].tobytes() == track[mask].tobytes()
    assert got[:, 0].tobytes() == track[:, 0].tobytes() and got[:, -1].tobytes() == track[:, -1].tobytes()
    for kw in (dict(), dict(anchor=flat(anchor), mu=sdo.MU)):
        free, d = denoised(unit, q, 1, words, opts, lam=sdo.LAMBDA, flags=sdo.FREE_ENDS, **kw)
        free = free.reshape(track.shape)
        ends = ~interior & ~mask
        assert (free[ends] != track[ends]).any(axis=-1).all() and free[mask].tobytes() == track[mask].tobytes()
        if not kw:
            assert free[:, 1:-1].tobytes() == plain[:, 1:-1].tobytes()


# ------------------------------------------------------------------------------------------ 3. the chunk seam
def test_anchors_and_confidences_follow_the_chunk_seam(torch_cuda):
    """T = 7 and P = 2,342: B = 16,394 is more than a chunk of 16,384, and the track-aligned chunk is 16,380 poses = 2,340 tracks.
    With anchors, confidences and free ends, tracks 2,339 (the last of the first chunk) and 2,340 (the first of the second) equal the
    same two tracks run alone -- an anchor or confidence offset that forgot the chunk would show here; two runs of the big call are
    bit-identical."""
    parents = sko.HAND
    J = len(parents)
    sd = sko.network(parents, 3, hidden=(32,))
    unit = Unit(torch_cuda, parents, "softplus", sd, hidden=(32,))
    Pn, Tn = 2342, 7
    assert Pn * Tn == 16394 and (16384 // Tn) * Tn == 16380 == 2340 * Tn
    x = synth.make_poses(Pn * Tn, seed=5, signed=True, num_joints=J).reshape(Pn, Tn, J, 4)
    r = np.random.RandomState(9)
    conf = r.rand(Pn, Tn, J).astype(np.float32)
    conf[r.rand(Pn, Tn, J) < 0.1] = 0.0
    anchor = sdo.make_anchor(x, conf, seed=3)
    mask = np.zeros((Pn, Tn, J), bool)
    mask[2339], mask[2340] = sdo.make_mask(J, 2, Tn)[1], sdo.make_mask(J, 2, Tn, seed=8)[1]
    words = sdo.pack(mask)
    opts = dict(renormalize="unit", step_size=0.5)
    kw = dict(frames=Tn, lam=0.5, mu=0.25, flags=sdo.FREE_ENDS)
    for steps in (2, 3):      # both parities of the buffer swap
        out, d = denoised(unit, flat(x), steps, words, opts, anchor=flat(anchor), conf=conf.reshape(-1, J), **kw)
        again, d_again = denoised(unit, flat(x), steps, words, opts, anchor=flat(anchor), conf=conf.reshape(-1, J), **kw)
        assert again.tobytes() == out.tobytes() and d_again.tobytes() == d.tobytes()
        out, d = out.reshape(Pn, Tn, J, 4), d.reshape(Pn, Tn)
        assert np.isfinite(out).all() and np.isfinite(d).all()
        for part in (slice(2339, 2341), slice(0, 40), slice(2341, 2342)):
            alone, d_alone = denoised(unit, flat(x[part]), steps, words.reshape(Pn, Tn)[part].reshape(-1), opts, anchor=flat(anchor[part]),
                                      conf=conf[part].reshape(-1, J), **kw)
            assert alone.tobytes() == out[part].tobytes() and d_alone.tobytes() == d[part].tobytes(), (steps, part)
        assert out[mask].tobytes() == x[mask].tobytes() and not np.array_equal(out[:, 0], x[:, 0])
    # without tracks the seam is at 16,384: poses 16,383 and 16,384 alone equal the big call, in place too
    q = flat(x)
    kw = dict(frames=0, mu=0.25, anchor=flat(anchor), conf=conf.reshape(-1, J))
    out, d = denoised(unit, q, 2, None, opts, **kw)
    pair = slice(16383, 16385)
    alone, d_alone = denoised(unit, q[pair], 2, None, opts, frames=0, mu=0.25, anchor=flat(anchor)[pair], conf=conf.reshape(-1, J)[pair])
    assert alone.tobytes() == out[pair].tobytes() and d_alone.tobytes() == d[pair].tobytes()
    inp, d_inp = denoised(unit, q, 2, None, opts, in_place=True, **kw)
    assert inp.tobytes() == out.tobytes() and d_inp.tobytes() == d.tobytes()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing(torch_cuda):
    torch = torch_cuda
    unit, J = unit_of(torch, ("hand", True), "lrelu")
    lib = unit.lib
    q = flat(sio.given_track(("hand", True), 2, 4))      # 8 poses
    words = np.zeros(9, np.uint32)
    anchor = np.concatenate([q, q[:1]])
    conf = np.ones((9, J), np.float32)

    def refused(make, field, **kw):
        rc, out, d = denoise_call(unit, q, 2, words, anchor=anchor, conf=conf, make=make, **kw)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_skel_last_error(unit.h), (field, lib.pndf_skel_last_error(unit.h))
        assert (out.tobytes() == q.tobytes() if kw else np.all(out == 7.0)) and np.all(d == 7.0), field

    for size in (71, 73, 0, 56, 64, 80):
        refused(lambda at, an, cf, size=size: sdo.c_options4(lib, at, 4, anchor=an, mu=0.5, size=size), "struct_size")
    for mu in (-0.1, 1.5, math.nan):
        refused(lambda at, an, cf, mu=mu: sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=mu), "mu")
    for flags in (2, 0x80000000):
        refused(lambda at, an, cf, flags=flags: sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5, flags=flags), "flags")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=None, mu=0.5), "anchor")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=None, conf=cf), "anchor")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an + 2, mu=0.5), "anchor")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an, conf=cf + 1, mu=0.5), "conf")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 0, 0.0, flags=sdo.FREE_ENDS), "FREE_ENDS")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, sio.SLERP, flags=sdo.FREE_ENDS), "fill")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5), "q_out", in_place=True)
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 3, 0.5, anchor=an, mu=0.5), "frames")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5, reserved2=1), "reserved2")
    refused(lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5, step_size=0.0), "step_size")
    # anchor or conf overlapping q_out: whole and by one pose
    dq = torch.from_numpy(q).cuda()
    ws, n = unit.ws(8)
    for which, shift in (("anchor", 0), ("anchor", 1), ("conf", 0)):
        buf = torch.full((9,) + q.shape[1:], 7.0, device="cuda:0")
        d = torch.full((8,), 7.0, device="cuda:0")
        side = torch.from_numpy(anchor).cuda()
        opt = sdo.c_options4(lib, None, 4, 0.5, anchor=buf[shift:].data_ptr() if which == "anchor" else side.data_ptr(),
                             conf=buf.data_ptr() if which == "conf" else None, mu=0.5)
        rc = lib.pndf_skel_project(unit.h, dq.data_ptr(), buf.data_ptr(), d.data_ptr(), 8, 2, ctypes.byref(opt), ws.data_ptr(), n, unit.stream())
        torch.cuda.synchronize()
        text = lib.pndf_skel_last_error(unit.h)
        assert rc == BAD_ARG and which.encode() in text and b"q_out" in text and bool((buf == 7).all()) and bool((d == 7).all()), (which, shift, text)
    rc, out, _ = denoise_call(unit, q, 2, words, anchor=anchor, conf=conf, make=lambda at, an, cf: sdo.c_options4(lib, at, 4, 0.5, anchor=an, conf=cf, mu=0.5,
                                                                                                                  flags=sdo.FREE_ENDS))
    assert rc == 0 and not np.any(out == 7.0)


def test_the_persistent_engine_refuses_the_72_byte_struct(torch_cuda):
    """pndf_project_ex, pndf_complete, pndf_interpolate and the two step helpers on a pndf_create handle: a 72-byte struct is
    PNDF_ERR_BAD_ARG, nothing written"""
    torch = torch_cuda
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import Engine
    eng = Engine("lrelu", precision="fp32")
    eng.load_weights(synth.make_weights(0, 2.0, 0.1))
    lib = eng.lib
    n = 8
    q = torch.from_numpy(synth.make_poses(n, seed=5)).cuda()
    out, d = torch.full_like(q, 7.0), torch.full((n,), 7.0, device="cuda:0")
    words = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(max(eng.complete_workspace_floats(n), eng.interpolate_workspace(n // 2, 2), 4), device="cuda:0")
    big = sdo.c_options4(lib, words.data_ptr(), 2, anchor=q.data_ptr(), mu=0.5)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pndf_project_ex(eng.handle, q.data_ptr(), out.data_ptr(), d.data_ptr(), n, 1, ref, st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_complete(eng.handle, q.data_ptr(), words.data_ptr(), out.data_ptr(), d.data_ptr(), n, 1, ref, ws.data_ptr(), st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_complete_step(out.data_ptr(), d.data_ptr(), q.data_ptr(), words.data_ptr(), n, ref, st) == BAD_ARG
    track = torch.full((n // 2, 2, 21, 4), 7.0, device="cuda:0")
    assert lib.pndf_interpolate(eng.handle, q.data_ptr(), q[n // 2:].data_ptr(), None, track.data_ptr(), d.data_ptr(), n // 2, 2, 0, 1, 0.0, ref,
                                ws.data_ptr(), st) == BAD_ARG
    assert b"struct_size" in lib.pndf_last_error(eng.handle)
    assert lib.pndf_interp_band_step(q.data_ptr(), out.data_ptr(), d.data_ptr(), q.data_ptr(), None, n // 2, 2, 0.0, ref, st) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((d == 7).all()) and bool((track == 7).all())


# ------------------------------------------------------------------------------------------ 5. free running
def free_inputs(case):
    """(the noisy clip [6,7,J,4], its confidences): the clip is its own anchor, so every confidence's anchor is finite"""
    x = sdo.noisy_clip(case)
    return x, sdo.make_conf(x.shape[2], x.shape[0], x.shape[1])


@functools.lru_cache(maxsize=None)
def oracle_tracks(case, act):
    """(fp64 track, fp32 track, kink margins along the fp64 trajectory or None) of the numpy oracle: ten denoising steps on the noisy
    clip with confidences, free ends, lambda 0.5, mu 0.25, unit quaternions"""
    parents, sd = sko.case_network(case, act)
    x, conf = free_inputs(case)
    kw = dict(anchor=x, conf=conf, mu=sdo.MU, smooth=sdo.LAMBDA, free_ends=True, renormalize="unit")
    q64, _, margin = sdo.relax(x, sd, FREE_STEPS, act, parents, dtype=np.float64, **kw)
    q32, _, _ = sdo.relax(x, sd, FREE_STEPS, act, parents, dtype=np.float32, **kw)
    return q64, q32, (None if act == "softplus" else margin)


def rows(track):
    t = np.asarray(track)
    return t.reshape(t.shape[0] * t.shape[1], -1)      # every frame moves: the end frames are free


def free_gate(got, case, act, what, ref=None):
    """conftest.outlier_gate at 1e-4 on every frame against the fp64 oracle track, the float32 numpy oracle's rows (or `ref`'s) as the
    reference rows.  The gate's exemption caps are conditions, not measurements: first the float32 oracle alone is shown to stay inside
    them on these inputs (finite, every row below 100 %, and through the gate against itself)."""
    q64, q32, margin = oracle_tracks(case, act)
    truth = rows(q64)
    own = rel_err_rows(rows(q32), truth)
    assert np.isfinite(own).all() and own.max() < 1.0, (what, float(own.max()))
    outlier_gate(own, own, TOL, f"{what}: the float32 oracle itself", margin=margin)
    mine = rel_err_rows(rows(got), truth)
    base = own if ref is None else rel_err_rows(rows(ref), truth)
    print(f"[{what}] per-pose error: median {np.median(mine):.2e} max {mine.max():.2e} | reference rows median {np.median(base):.2e} max {base.max():.2e}")
    outlier_gate(mine, base, TOL, what, margin=margin)


@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_ten_free_running_steps(torch_cuda, case, act):
    from test_skeleton_completion import twin_of
    unit, J = unit_of(torch_cuda, case, act)
    x, conf = free_inputs(case)
    kw = dict(frames=x.shape[1], lam=sdo.LAMBDA, mu=sdo.MU, flags=sdo.FREE_ENDS)
    got, d = denoised(unit, flat(x), FREE_STEPS, None, dict(renormalize="unit"), anchor=flat(x), conf=conf.reshape(-1, J), **kw)
    assert np.isfinite(got).all() and np.isfinite(d).all()
    got = got.reshape(x.shape)
    free_gate(got, case, act, f"unit {sko.case_id(case)} {act}")
    # the device against the twin, under the same gate
    twin, _ = twin_of(case, act)
    q, c = flat(x), np.ascontiguousarray(conf.reshape(-1, J))
    cpu, _ = twin.project(q, FREE_STEPS, sdo.c_from(twin.lib, dict(renormalize="unit"), None, x.shape[1], sdo.LAMBDA, q.ctypes.data, c.ctypes.data, sdo.MU,
                                                    sdo.FREE_ENDS))
    free_gate(cpu.reshape(x.shape), case, act, f"twin {sko.case_id(case)} {act}")
    free_gate(got, case, act, f"unit against twin {sko.case_id(case)} {act}", ref=cpu.reshape(x.shape))


# ------------------------------------------------------------------------------------------ 6. Python
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_denoise_on_cuda(torch_cuda, case, act):
    torch = torch_cuda
    from test_skeleton_completion import cpu_model
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cuda_model(torch, parents, act, sd)
    unit = Unit(torch, parents, act, sd)
    x_np, conf = free_inputs(case)
    Pn, Tn = x_np.shape[:2]
    mask = sdo.make_mask(J, Pn, Tn)
    x, c, m = torch.from_numpy(x_np.copy()).cuda(), torch.from_numpy(conf).cuda(), torch.from_numpy(mask)
    # the unit's bits through the C struct: one engine call, the input its own anchor
    want, d_want = denoised(unit, flat(x_np), K, sdo.pack(mask), dict(renormalize="unit"), frames=Tn, lam=0.5, anchor=flat(x_np), conf=conf.reshape(-1, J),
                            mu=0.25, flags=sdo.FREE_ENDS)
    track, d = net.denoise(x, steps=K, smooth=0.5, data=0.25, conf=c, observed=m)
    assert track.is_cuda and track.shape == (Pn, Tn, J, 4) and d.shape == (Pn, Tn)
    assert track.cpu().numpy().tobytes() == want.tobytes() and d.cpu().numpy().tobytes() == d_want.tobytes()
    assert x.cpu().numpy().tobytes() == x_np.tobytes()      # the input is not written
    assert torch.equal(track.cpu()[m].view(torch.int32), torch.from_numpy(x_np)[m].view(torch.int32))
    held = net.denoise(x, steps=K, smooth=0.5, data=0.25, free_ends=False, return_dist=False)
    assert torch.equal(held[:, 0], x[:, 0]) and torch.equal(held[:, -1], x[:, -1]) and not torch.equal(track[:, 0], x[:, 0])
    a, da = net.denoise(x, steps=2, conf=c[1, 2])
    b, db = net.denoise(x, steps=2, conf=c[1, 2].expand(Pn, Tn, J))
    assert torch.equal(a, b) and torch.equal(da, db)
    one, d_one = net.denoise(x[1], steps=2, conf=c[1])
    assert one.shape == (Tn, J, 4) and torch.equal(one, net.denoise(x, steps=2, conf=c[1], return_dist=False)[1])
    # T = 1: no tracks, the data term only -- the 72-byte call with frames 0
    frame = x[:, :1].contiguous()
    f_np = flat(frame.cpu().numpy())
    want, d_want = denoised(unit, f_np, K, None, dict(renormalize="unit"), frames=0, anchor=f_np, mu=0.25)
    got, dg = net.denoise(frame, steps=K, smooth=0.5, data=0.25)
    assert got.cpu().numpy().tobytes() == want.tobytes() and dg.cpu().numpy().reshape(-1).tobytes() == d_want.tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again, d_again = net.denoise(x, steps=K, smooth=0.5, data=0.25, conf=c, observed=m)
    side.synchronize()
    assert torch.equal(again.view(torch.int32), track.view(torch.int32)) and torch.equal(d_again.view(torch.int32), d.view(torch.int32))
    e, de = net.denoise(x[:0], steps=2)
    assert e.shape == (0, Tn, J, 4) and de.shape == (0, Tn)
    # ten free-running steps: the cuda model and a cpu model under the gate, and one against the other
    host = cpu_model(parents, act, sd)
    kw = dict(steps=FREE_STEPS, smooth=sdo.LAMBDA, data=sdo.MU, return_dist=False)
    dev = net.denoise(x, conf=c, **kw).cpu().numpy()
    cpu = host.denoise(x.cpu(), conf=c.cpu(), **kw).numpy()
    what = f"model {sko.case_id(case)} {act}"
    free_gate(cpu, case, act, f"cpu {what}")
    free_gate(dev, case, act, f"cuda {what}")
    free_gate(dev, case, act, f"cuda against cpu {what}", ref=cpu)


def test_pose_denoising_driver_on_a_hand(torch_cuda):
    torch = torch_cuda
    from posendf_amd.pose_denoising import PoseDenoising
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cuda_model(torch, parents, "softplus", sd)
    x_np, conf = free_inputs(case)
    x, c = torch.from_numpy(x_np), torch.from_numpy(np.abs(conf))
    driver = PoseDenoising(net, body_model=None, device="cuda:0")
    track, dist, history = driver.denoise(x, conf=c, iterations=3, steps_per_iter=3, smooth=0.4, data=0.5)
    assert track.is_cuda and track.shape == x.shape and dist.shape == x.shape[:2] and bool(torch.isfinite(track).all()) and bool(torch.isfinite(dist).all())
    assert [(lam, mu) for lam, mu, _ in history] == [(0.4, 0.5), (0.8, 0.25), (1.0, 0.5 / 3)]
    cur = x.cuda()
    for lam, mu, _ in history:
        cur, d = net.denoise(cur, steps=3, smooth=lam, data=mu, conf=c, anchor=x)
    assert torch.equal(track, cur) and torch.equal(dist, d)


def test_exported_symbols():
    import __graft_entry__ as ge
    import cabi_headers as ch
    assert {"pndf_skel_enc_rev_kernel", "pndf_skel_enc_rev_track_kernel", "pndf_skel_enc_rev_denoise_kernel"} <= ch.exported_symbols(ge.LIB)
