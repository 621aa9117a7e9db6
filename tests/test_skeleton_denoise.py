"""Motion denoising for other skeletons on the host (pndf_project_options4 of include/posendf_amd.h; DESIGN.md section 2j "Motion
denoising"): the host twin pndf_project_ex_cpu with an observation and free end frames against the numpy statement of the denoising step
(tests/skeleton_denoise_oracle.py).

1. the stated step: K rounds of the twin's own forward_grad + the numpy step equal the call, bit for bit, for every option set, with and
   without a mask, confidences and free end frames, with tracks and without.
2. same bits: anchor NULL and flags 0 is the 48-byte call; mu 0 with anchors of NaN too; without tracks, free ends and mu the 32-byte call.
3. one step: a joint without confidence ignores its (NaN) anchor, a held joint keeps its bits, free end frames move and held ones do not.
4. the refusals, each naming its field and writing nothing; the other entry points keep refusing the larger struct.
5. the effects, first on the float64 numpy oracle alone, then on the twin: the data term keeps the result nearer the observation, the
   coupling lowers the second difference.
6. the struct as a C caller writes it, the binding, no new entry point.
7. `SkeletonPoseNDF.denoise` and `PoseDenoising` on a cpu model.
Runs without a GPU; tests/test_skeleton_denoise_gpu.py holds the HIP unit to the same statements."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_completion_oracle as sco
import skeleton_denoise_oracle as sdo
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from test_skeleton_completion import Twin, cpu_model, twin_of

BAD_ARG = sdo.BAD_ARG
P, T, K = sdo.P, sdo.T, sdo.K
B = P * T
flat = sdo.flat

# (mask, confidences, free end frames) of the stated-step checks
VARIANTS = [(False, False, False), (True, True, True), (False, True, True), (True, False, False), (False, False, True)]


def ptr(a):
    return None if a is None else a.ctypes.data


# ------------------------------------------------------------------------------------------ 1. the stated step
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", sdo.CASES, ids=sko.case_id)
def test_denoising_steps_are_the_stated_step(case, act):
    twin, J = twin_of(case, act)
    track = sdo.clip(case)
    mask = sdo.make_mask(J)
    words = sdo.pack(mask)
    conf = sdo.make_conf(J)
    with np.errstate(invalid="ignore"):
        assert (conf == 0).any() and (conf < 0).any() and np.isnan(conf).any() and (conf > 0).any()
    tol = float(np.median(twin.forward(flat(track))))
    for name in sdo.OPTION_SETS:
        opts = sdo.options(name, tol)
        for use_mask, use_conf, free in VARIANTS:
            m, c = (mask if use_mask else None), (conf if use_conf else None)
            anchor = sdo.make_anchor(track, c)
            assert (c is None) == bool(np.isfinite(anchor).all())      # a joint without confidence has a NaN anchor
            what = (name, use_mask, use_conf, free)
            # with tracks
            want, dk = sdo.rounds(twin.forward_grad, track, K, anchor=anchor, conf=c, mu=sdo.MU, observed=m, smooth=sdo.LAMBDA, free_ends=free, **opts)
            got, dl = twin.project(flat(track), K, sdo.c_from(twin.lib, opts, ptr(words) if use_mask else None, T, sdo.LAMBDA, ptr(anchor), ptr(c), sdo.MU,
                                                              sdo.FREE_ENDS if free else 0))
            sdo.assert_same(got.reshape(track.shape), want, what)
            sdo.assert_same(dl, dk, what + ("d_last",))
            held = mask.copy() if use_mask else np.zeros_like(mask)
            if not free:
                held[:, 0] = held[:, -1] = True
            assert got.reshape(track.shape)[held].tobytes() == track[held].tobytes(), what
            if free:
                continue
            # without tracks: every pose on its own, the data term only
            want, dk = sdo.rounds(twin.forward_grad, track, K, anchor=anchor, conf=c, mu=sdo.MU, observed=m, frames=0, **opts)
            got, dl = twin.project(flat(track), K, sdo.c_from(twin.lib, opts, ptr(words) if use_mask else None, 0, 0.0, ptr(anchor), ptr(c), sdo.MU))
            sdo.assert_same(got.reshape(track.shape), want, what + ("no tracks",))
            sdo.assert_same(dl, dk, what + ("no tracks", "d_last"))
            again, d_again = twin.project(flat(track), K, sdo.c_from(twin.lib, opts, ptr(words) if use_mask else None, 0, 0.0, ptr(anchor), ptr(c), sdo.MU),
                                          in_place=True)
            assert again.tobytes() == got.tobytes() and d_again.tobytes() == dl.tobytes(), what + ("in place",)


# ------------------------------------------------------------------------------------------ 2. same bits
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_without_an_observation_it_is_the_smaller_call(case, act):
    twin, J = twin_of(case, act)
    lib = twin.lib
    q = flat(sdo.clip(case))
    words = sdo.pack(sdo.make_mask(J))
    nan = np.full(q.shape, np.nan, np.float32)
    conf = sdo.make_conf(J)
    tol = float(np.median(twin.forward(q)))
    for name in sdo.OPTION_SETS:
        opts = sdo.options(name, tol)
        for w in (None, words):
            for lam in (0.0, sdo.LAMBDA):
                want, d_want = twin.project(q, K, sio.c_from(lib, opts, ptr(w), frames=T, lam=lam))
                for kw in (dict(), dict(anchor=ptr(nan)), dict(anchor=ptr(nan), conf=ptr(conf))):      # mu == 0: the anchors are never read
                    got, d_got = twin.project(q, K, sdo.c_from(lib, opts, ptr(w), T, lam, **kw))
                    assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), (name, w is None, lam, sorted(kw))
            # tracks off, free ends off, mu 0: the 32-byte call
            small, d_small = twin.project(q, K, sco.c_from(lib, opts, ptr(w)))
            for kw in (dict(), dict(anchor=ptr(nan))):
                got, d_got = twin.project(q, K, sdo.c_from(lib, opts, ptr(w), 0, 0.0, **kw))
                assert got.tobytes() == small.tobytes() and d_got.tobytes() == d_small.tobytes(), (name, w is None, sorted(kw))


# ------------------------------------------------------------------------------------------ 3. one step
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_one_step(case, act):
    twin, J = twin_of(case, act)
    lib = twin.lib
    track = sdo.clip(case)
    q = flat(track)
    mask = sdo.make_mask(J)
    words = sdo.pack(mask)
    opts = dict(renormalize="unit")
    anchor = sdo.make_anchor(track)
    plain, _ = twin.project(q, 1, sio.c_from(lib, opts, ptr(words), frames=T, lam=sdo.LAMBDA))
    plain = plain.reshape(track.shape)
    # a joint with conf == 0, negative or NaN and a NaN anchor takes exactly the bits of the unanchored call; the others do not
    conf = np.ones((P, T, J), np.float32)
    off = np.zeros((P, T, J), bool)
    off[0, 2, 0], off[2, 1, J - 1], off[2, 3, J // 2] = True, True, True
    conf[0, 2, 0], conf[2, 1, J - 1], conf[2, 3, J // 2] = 0.0, np.nan, -1.0
    a = anchor.copy()
    a[off] = np.nan
    got, d = twin.project(q, 1, sdo.c_from(lib, opts, ptr(words), T, sdo.LAMBDA, ptr(a), ptr(conf), sdo.MU))
    got = got.reshape(track.shape)
    assert np.isfinite(got).all() and np.isfinite(d).all()
    assert got[off].tobytes() == plain[off].tobytes()
    interior = np.zeros((P, T, J), bool)
    interior[:, 1:-1] = True
    pulled = interior & ~off & ~mask
    assert (got[pulled] != plain[pulled]).any(axis=-1).all()
    # a held joint keeps its bits, and so do the end frames without FREE_ENDS
    assert mask.any() and got[mask].tobytes() == track[mask].tobytes()
    assert got[:, 0].tobytes() == track[:, 0].tobytes() and got[:, -1].tobytes() == track[:, -1].tobytes()
    # under FREE_ENDS the end frames move (every joint the mask does not hold), with and without an anchor
    for kw in (dict(), dict(anchor=ptr(anchor), mu=sdo.MU)):
        free, d = twin.project(q, 1, sdo.c_from(lib, opts, ptr(words), T, sdo.LAMBDA, flags=sdo.FREE_ENDS, **kw))
        free = free.reshape(track.shape)
        ends = ~interior & ~mask
        assert (free[ends] != track[ends]).any(axis=-1).all() and free[mask].tobytes() == track[mask].tobytes()
        if not kw:      # the interior frames of the first step do not see the ends move: a Jacobi update
            assert free[:, 1:-1].tobytes() == plain[:, 1:-1].tobytes()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing():
    twin, J = twin_of(("hand", True), "lrelu")
    lib = twin.lib
    q = flat(sio.given_track(("hand", True), 2, 4))      # 8 poses
    words = np.zeros(9, np.uint32)
    anchor = np.concatenate([q, q[:1]])
    conf = np.ones((9, J), np.float32)
    at, an, cf = words.ctypes.data, anchor.ctypes.data, conf.ctypes.data

    def refused(opt, field, **kw):
        rc, out, d = twin.call(q, 2, opt, **kw)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_cpu_last_error(twin.h), (field, lib.pndf_cpu_last_error(twin.h))
        assert np.all(out == 7.0) and np.all(d == 7.0), field

    for size in (71, 73, 0, 56, 64, 80):
        refused(sdo.c_options4(lib, at, 4, anchor=an, mu=0.5, size=size), "struct_size")
    for mu in (-0.1, 1.5, math.nan, math.inf):
        refused(sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=mu), "mu")
    for flags in (2, 3, 0x80000000):
        refused(sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5, flags=flags), "flags")
    refused(sdo.c_options4(lib, at, 4, 0.5, anchor=None, mu=0.5), "anchor")
    refused(sdo.c_options4(lib, at, 4, 0.5, anchor=None, conf=cf), "anchor")
    for odd in (1, 2, 3):
        refused(sdo.c_options4(lib, at, 4, 0.5, anchor=an + odd, mu=0.5), "anchor")
        refused(sdo.c_options4(lib, at, 4, 0.5, anchor=an, conf=cf + odd, mu=0.5), "conf")
    refused(sdo.c_options4(lib, at, 0, 0.0, flags=sdo.FREE_ENDS), "FREE_ENDS")
    refused(sdo.c_options4(lib, at, 0, 0.0, flags=sdo.FREE_ENDS), "frames")
    for fill in (sio.SLERP, sio.NLERP):
        refused(sdo.c_options4(lib, at, 4, 0.5, fill, flags=sdo.FREE_ENDS), "FREE_ENDS")
        refused(sdo.c_options4(lib, at, 4, 0.5, fill, flags=sdo.FREE_ENDS), "fill")
    # anchor or conf overlapping q_out: whole and by one pose
    d = np.full(8, 7.0, np.float32)
    for steps_kw, field in ((dict(anchor="out"), "anchor"), (dict(anchor="out1"), "anchor"), (dict(conf="out"), "conf")):
        buf = np.full((9,) + q.shape[1:], 7.0, np.float32)
        where = {"out": buf.ctypes.data, "out1": buf[1:].ctypes.data}
        opt = sdo.c_options4(lib, at, 4, 0.5, anchor=where.get(steps_kw.get("anchor"), an), conf=where.get(steps_kw.get("conf")), mu=0.5)
        assert lib.pndf_project_ex_cpu(twin.h, q.ctypes.data, buf.ctypes.data, d.ctypes.data, 8, 2, ctypes.byref(opt)) == BAD_ARG, steps_kw
        text = lib.pndf_cpu_last_error(twin.h)
        assert field.encode() in text and b"q_out" in text and np.all(buf == 7.0) and np.all(d == 7.0), (steps_kw, text)
    # in place without tracks: the anchor must lie elsewhere
    rc, out, d2 = twin.call(q, 2, sdo.c_options4(lib, at, 0, 0.0, anchor=an, mu=0.5), in_place=True)
    assert rc == 0 and np.isfinite(out).all()
    # everything base3 already refuses, with the text of the smaller structs
    for field, kw in (("reserved2", dict(reserved2=1)), ("reserved", dict(reserved=1)), ("step_size", dict(step_size=0.0)), ("tol", dict(tol=math.nan)),
                      ("renorm", dict(renorm=3))):
        rc, _, _ = twin.call(q, 2, sio.c_options3(lib, at, 4, **kw))
        text = lib.pndf_cpu_last_error(twin.h)
        refused(sdo.c_options4(lib, at, 4, anchor=an, mu=0.5, **kw), field)
        assert rc == BAD_ARG and lib.pndf_cpu_last_error(twin.h) == text
    for frames, lam, field in ((3, 0.0, "frames"), (1, 0.0, "frames"), (4, 1.5, "lambda"), (0, 0.5, "lambda")):
        refused(sdo.c_options4(lib, at, frames, lam, anchor=an, mu=0.5), field)
    rc, out, d2 = twin.call(q, 2, sdo.c_options4(lib, at, 4, 0.5, anchor=an, mu=0.5), in_place=True)      # with tracks q_out stays apart from q_in
    assert rc == BAD_ARG and b"q_out" in lib.pndf_cpu_last_error(twin.h) and out.tobytes() == q.tobytes() and np.all(d2 == 7.0)
    # a good struct after all that, and the Python layer
    rc, out, _ = twin.call(q, 2, sdo.c_options4(lib, at, 4, 0.5, anchor=an, conf=cf, mu=0.5, flags=sdo.FREE_ENDS))
    assert rc == 0 and not np.any(out == 7.0)
    from posendf_amd.engine import PndfError
    out, d = np.full_like(q, 7.0), np.full(len(q), 7.0, np.float32)
    for field, kw in (("mu", dict(frames=4, anchor_ptr=an, data=2.0)), ("anchor", dict(frames=4, data=0.5)), ("anchor", dict(frames=4, conf_ptr=cf)),
                      ("FREE_ENDS", dict(free_ends=True)), ("frames", dict(frames=3, anchor_ptr=an, data=0.5))):
        with pytest.raises(PndfError, match=field):
            twin.eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), 2, **kw)
    assert np.all(out == 7.0) and np.all(d == 7.0)


def test_the_other_entry_points_refuse_the_72_byte_struct():
    """every other function with a pndf_project_options parameter: a 72-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers; pndf_project_ex, pndf_complete and pndf_interpolate need a device handle and are in the
    GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    big = sdo.c_options4(lib, words.ctypes.data, 2, anchor=q.ctypes.data, mu=0.5)
    out, d = np.full_like(q, 7.0), np.full(8, 7.0, np.float32)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(ProjectOptions))
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    track = np.full((2, 2, 21, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q[2:].ctypes.data, None, track.ctypes.data, d.ctypes.data, 2, 2, 0, 1, 0.0, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    assert lib.pndf_complete_step(out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 4, ref, None) == BAD_ARG
    assert lib.pndf_interp_band_step(q.ctypes.data, out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 2, 2, 0.0, ref, None) == BAD_ARG
    assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(track == 7.0)
    # the twin that takes it does, on this 21-joint handle too
    assert lib.pndf_project_ex_cpu(eng.handle, q.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(big)) == 0
    assert not np.any(out == 7.0)


# ------------------------------------------------------------------------------------------ 5. the effects
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_the_terms_do_what_they_are_for(case, act):
    """ten free-running steps on a noisy clip, free ends, unit quaternions: with mu > 0 the mean per-joint angle to the observation is
    smaller than with mu = 0; with lambda > 0 the summed second difference is smaller than with lambda = 0 -- in the fp64 oracle
    first, then on the model's output"""
    a_free, s_rough = sdo.oracle_effect(case, act, 0.0, 0.0)
    a_tied, _ = sdo.oracle_effect(case, act, 0.0, sdo.MU)
    _, s_smooth = sdo.oracle_effect(case, act, sdo.LAMBDA, 0.0)
    a_both, s_both = sdo.oracle_effect(case, act, sdo.LAMBDA, sdo.MU)
    _, s_data = sdo.oracle_effect(case, act, 0.0, sdo.MU)
    a_smooth, _ = sdo.oracle_effect(case, act, sdo.LAMBDA, 0.0)
    print(f"[effects {sko.case_id(case)} {act}] fp64 oracle: angle to the observation {a_tied:.4f} (mu {sdo.MU}) against {a_free:.4f} (mu 0); "
          f"second difference {s_smooth:.4f} (lambda {sdo.LAMBDA}) against {s_rough:.4f} (lambda 0); both terms {a_both:.4f} / {s_both:.4f}")
    assert a_tied < a_free and s_smooth < s_rough and a_both < a_smooth and s_both < s_data
    parents, sd = sko.case_network(case, act)
    net = cpu_model(parents, act, sd)
    x = torch.from_numpy(sdo.noisy_clip(case))

    def run(smooth, data):
        out = net.denoise(x, steps=sdo.EFFECT_STEPS, smooth=smooth, data=data, return_dist=False).numpy()
        return sdo.angle_to(out, x.numpy()), sdo.second_difference(out)

    (m_free, r_rough), (m_tied, r_data), (m_smooth, r_smooth), (m_both, r_both) = run(0.0, 0.0), run(0.0, sdo.MU), run(sdo.LAMBDA, 0.0), run(sdo.LAMBDA, sdo.MU)
    assert m_tied < m_free and r_smooth < r_rough and m_both < m_smooth and r_both < r_data, (m_free, m_tied, m_smooth, m_both, r_rough, r_data, r_smooth, r_both)


# ------------------------------------------------------------------------------------------ 6. the library and the ABI
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_denoise_kernel" in ch.exported_symbols(ge.LIB)
    o4 = abi.ProjectOptions4
    assert ctypes.sizeof(o4) == 72 and engine.ProjectOptions4 is o4
    assert (o4.base3.offset, o4.anchor.offset, o4.conf.offset, o4.mu.offset, o4.flags.offset) == (0, 48, 56, 64, 68)
    assert abi.TRACK_FREE_ENDS == sdo.FREE_ENDS == 1
    lib = engine.load_library()
    o = engine.project_options4(lib, 64, 7, smooth=0.25, anchor_ptr=128, conf_ptr=256, data=0.5, free_ends=True, step_size=0.5, renorm="unit", tol=0.25)
    b = o.base3.base2.base
    assert (b.struct_size, b.step_size, b.renorm, b.tol, o.base3.base2.observed, o.base3.base2.reserved) == (72, 0.5, 1, 0.25, 64, 0)
    assert (o.base3.frames, o.base3.lambda_, o.base3.fill, o.base3.reserved2) == (7, 0.25, sio.GIVEN, 0)
    assert (o.anchor, o.conf, o.mu, o.flags) == (128, 256, 0.5, 1)
    o = engine.project_options4(lib, None, 0)
    assert (o.base3.base2.base.struct_size, o.anchor, o.conf, o.mu, o.flags) == (72, None, None, 0.0, 0)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sdo.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "denoise" in n and "skel" in n] and not hasattr(lib, "pndf_skel_denoise")
    assert not [h for h in abi.HEADERS if "denoise" in h and "skel" in h]


# ------------------------------------------------------------------------------------------ 7. Python
@pytest.mark.parametrize("act", sdo.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_denoise_on_cpu(case, act):
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cpu_model(parents, act, sd)
    twin = Twin(parents, act, sd)
    x_np = sdo.noisy_clip(case, P, T)
    x = torch.from_numpy(x_np.copy())
    mask, conf = sdo.make_mask(J), sdo.make_conf(J)
    words = sdo.pack(mask)
    # the twin's bits through the C struct: one engine call, the input its own anchor
    q = flat(x_np)
    want, d_want = twin.project(q, K, sdo.c_options4(twin.lib, ptr(words), T, 0.5, anchor=ptr(q), conf=ptr(conf), mu=0.25, flags=sdo.FREE_ENDS, renorm=1))
    track, d = net.denoise(x, steps=K, smooth=0.5, data=0.25, conf=torch.from_numpy(conf), observed=torch.from_numpy(mask))
    assert track.shape == (P, T, J, 4) and d.shape == (P, T)
    assert track.numpy().tobytes() == want.tobytes() and d.numpy().tobytes() == d_want.tobytes()
    assert x.numpy().tobytes() == x_np.tobytes()      # the input is not written
    assert net.denoise(x, steps=K, smooth=0.5, data=0.25, conf=torch.from_numpy(conf), observed=torch.from_numpy(mask), return_dist=False).numpy().tobytes() == want.tobytes()
    m = torch.from_numpy(mask)
    assert torch.equal(track[m].view(torch.int32), x[m].view(torch.int32))
    # held end frames
    want, d_want = twin.project(q, K, sdo.c_options4(twin.lib, None, T, 0.5, anchor=ptr(q), mu=0.25, renorm=1))
    held, dh = net.denoise(x, steps=K, smooth=0.5, data=0.25, free_ends=False)
    assert held.numpy().tobytes() == want.tobytes() and dh.numpy().tobytes() == d_want.tobytes()
    assert torch.equal(held[:, 0], x[:, 0]) and torch.equal(held[:, -1], x[:, -1]) and not torch.equal(track[:, 0], x[:, 0])
    # the shapes of conf and observed: [J], [T,J], [P,T,J]
    c = torch.from_numpy(conf)
    for small, full in ((c[1, 2], c[1, 2].expand(P, T, J)), (c[1], c[1].expand(P, T, J))):
        a, da = net.denoise(x, steps=2, conf=small)
        b, db = net.denoise(x, steps=2, conf=full)
        assert torch.equal(a, b) and torch.equal(da, db)
    for small, full in ((m[1, 2], m[1, 2].expand(P, T, J)), (m[1], m[1].expand(P, T, J))):
        a, _ = net.denoise(x, steps=2, observed=small)
        b, _ = net.denoise(x, steps=2, observed=full)
        assert torch.equal(a, b)
    # one clip [T,J,4]
    one, d_one = net.denoise(x[1], steps=2, conf=c[1])
    many, d_many = net.denoise(x, steps=2, conf=c[1])
    assert one.shape == (T, J, 4) and d_one.shape == (T,) and torch.equal(one, many[1]) and torch.equal(d_one, d_many[1])
    # T = 1: no tracks, the data term only
    frame = x[:, :1].contiguous()
    want, d_want = twin.project(flat(frame.numpy()), K, sdo.c_options4(twin.lib, None, 0, 0.0, anchor=ptr(flat(frame.numpy())), mu=0.25, renorm=1))
    got, dg = net.denoise(frame, steps=K, smooth=0.5, data=0.25)
    assert got.shape == (P, 1, J, 4) and got.numpy().tobytes() == want.tobytes() and dg.numpy().reshape(-1).tobytes() == d_want.tobytes()
    # steps = 0 is the copy and zero distances; wrong arguments; an empty batch
    s, ds = net.denoise(x, steps=0)
    assert torch.equal(s, x) and not bool(ds.any())
    for kw in (dict(smooth=1.5), dict(data=-0.5), dict(conf=torch.zeros(T, J + 1)), dict(conf=torch.zeros(P, T, J, dtype=torch.bool)),
               dict(observed=torch.zeros(P, T, J)), dict(observed=torch.zeros(T + 1, J, dtype=torch.bool)), dict(anchor=x[:, :2])):
        with pytest.raises(PndfError):
            net.denoise(x, **kw)
    with pytest.raises(PndfError):
        net.denoise(x[..., :3])
    e, de = net.denoise(x[:0], steps=2)
    assert e.shape == (0, T, J, 4) and de.shape == (0, T)


def test_pose_denoising_driver_on_a_hand():
    import posendf_amd
    from posendf_amd.pose_denoising import PoseDenoising, second_difference
    assert posendf_amd.PoseDenoising is PoseDenoising and callable(posendf_amd.denoise_track_file)
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cpu_model(parents, "softplus", sd)
    x = torch.from_numpy(sdo.noisy_clip(case, P, T))
    conf = torch.from_numpy(np.abs(sdo.make_conf(J)))
    driver = PoseDenoising(net, body_model=None, device="cpu")
    track, dist, history = driver.denoise(x, conf=conf, iterations=3, steps_per_iter=2, smooth=0.4, data=0.5)
    assert track.shape == (P, T, J, 4) and dist.shape == (P, T) and bool(torch.isfinite(track).all()) and bool(torch.isfinite(dist).all())
    # the schedule: the coupling up (capped at 1), the data weight down, always anchored to the original clip
    assert [(lam, mu) for lam, mu, _ in history] == [(0.4, 0.5), (0.8, 0.25), (1.0, 0.5 / 3)]
    cur = x
    for lam, mu, _ in history:
        cur, d = net.denoise(cur, steps=2, smooth=lam, data=mu, conf=conf, anchor=x)
    assert torch.equal(track, cur) and torch.equal(dist, d)
    one, d_one, _ = driver.denoise(x[0], conf=conf[0], iterations=3, steps_per_iter=2, smooth=0.4, data=0.5)
    assert one.shape == (T, J, 4) and torch.equal(one, track[0]) and torch.equal(d_one, dist[0])
    sec = second_difference(track)      # J-agnostic, against the oracle's on an aligned clip
    assert sec.shape == (P,) and np.allclose(float(sec.sum()), sdo.second_difference(track.numpy()), rtol=1e-4)
    from posendf_amd import PoseNDF, amass_config
    with pytest.raises(TypeError, match="SkeletonPoseNDF"):
        PoseDenoising(PoseNDF(amass_config("lrelu", "cpu")), body_model=None, device="cpu").denoise(torch.zeros(1, 3, 21, 4))


def test_pose_denoising_main_reads_and_writes_npz(tmp_path):
    import yaml
    from posendf_amd import skeleton_config
    from posendf_amd.pose_denoising import main
    case = ("hand", True)
    parents, sd = sko.case_network(case, "lrelu")
    cfg = skeleton_config(list(parents), "lrelu", "cpu", hidden=sko.HIDDEN)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "ckpt.tar")
    x = sdo.noisy_clip(case, P, T)
    np.savez(tmp_path / "clip.npz", pose=x, conf=np.ones(len(parents), np.float32))
    track, dist = main(["-c", str(tmp_path / "cfg.yaml"), "-ckpt", str(tmp_path / "ckpt.tar"), "-tf", str(tmp_path / "clip.npz"), "--iterations", "2",
                        "--steps_per_iter", "2", "--out", str(tmp_path / "out.npz")])
    with np.load(tmp_path / "out.npz") as f:
        assert f["pose"].shape == x.shape and f["dist"].shape == (P, T) and np.array_equal(f["pose"], track.numpy())
    net = cpu_model(parents, "lrelu", sd)
    want, _, _ = __import__("posendf_amd").PoseDenoising(net, body_model=None, device="cpu").denoise(torch.from_numpy(x), conf=torch.ones(len(parents)),
                                                                                                 iterations=2, steps_per_iter=2)
    assert torch.equal(track, want)
