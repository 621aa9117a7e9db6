"""Pose interpolation for other skeletons on the host (pndf_project_options3 of include/posendf_amd.h): the host twin
pndf_project_ex_cpu with tracks against the numpy statement of the fill and of the band step (tests/skeleton_interpolation_oracle.py).

1. coupling off: lambda 0 and PNDF_TRACK_GIVEN is the pndf_project_options2 call whose end-frame words are all ones, frames 0 the 32-byte
   call, bit for bit.
2. coupling on: K steps at lambda 0.5 equal K rounds of forward_grad + the numpy band step, bit for bit, for every option set, with and
   without a mask; held joints keep their bits, a NaN and a zero quaternion included.
3. the fill: nlerp to the bit, slerp within four times the float32 error of the formula; T = 2.
4. the refusals, each naming its field and writing nothing; the other entry points keep refusing the larger struct.
5. on a 21-joint handle the call equals pndf_interpolate_cpu bit for bit; pndf_interpolate_cpu keeps refusing a skeleton handle.
6. `SkeletonPoseNDF.interpolate` and `PoseInterpolation` on a cpu model, and the evenness the coupling buys.
7. the struct as a C caller writes it.
Runs without a GPU; tests/test_skeleton_interpolation_gpu.py holds the HIP unit to the same statements."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import interpolation_oracle as io
import skeleton_completion_oracle as sco
import skeleton_interpolation_oracle as sio
import skeleton_oracle as sko
from test_skeleton_completion import Twin, cpu_model, twin_of

BAD_ARG, UNSUPPORTED = sio.BAD_ARG, sio.UNSUPPORTED
P, T, K = sio.P, sio.T, sio.K
B = P * T


flat = sio.flat


# ------------------------------------------------------------------------------------------ 1. coupling off
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_coupling_off_is_the_masked_call(case, act):
    twin, J = twin_of(case, act)
    q = flat(sio.given_track(case))
    mask = sio.case_mask(J)
    assert J < 32 or mask[1, 1, 31]
    tol = float(np.median(twin.forward(q)))
    for name in sio.OPTION_SETS:
        opts = sio.options(name, tol)
        for m in (None, mask):
            words = None if m is None else sio.pack(m)
            ends = sio.end_words(m, J)
            want, d_want = twin.project(q, K, sco.c_from(twin.lib, opts, ends.ctypes.data))
            got, d_got = twin.project(q, K, sio.c_from(twin.lib, opts, None if words is None else words.ctypes.data, frames=T))
            assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), (name, m is None)
            track = got.reshape(P, T, J, 4)
            assert track[:, 0].tobytes() == q.reshape(P, T, J, 4)[:, 0].tobytes() and track[:, -1].tobytes() == q.reshape(P, T, J, 4)[:, -1].tobytes()
            # frames = 0: the 32-byte call
            small, d_small = twin.project(q, K, sco.c_from(twin.lib, opts, None if words is None else words.ctypes.data))
            zero, d_zero = twin.project(q, K, sio.c_from(twin.lib, opts, None if words is None else words.ctypes.data, frames=0))
            assert zero.tobytes() == small.tobytes() and d_zero.tobytes() == d_small.tobytes(), (name, m is None)
    if J > 1:
        assert not np.array_equal(got, q)


# ------------------------------------------------------------------------------------------ 2. coupling on
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_coupled_steps_are_the_stated_step(case, act):
    twin, J = twin_of(case, act)
    mask = sio.case_mask(J)
    words = sio.pack(mask)
    clean = sio.given_track(case)
    odd, places = sio.odd_track(case, mask)
    tol = float(np.median(twin.forward(flat(clean))))
    held = mask.copy()
    held[:, 0] = held[:, -1] = True
    for name in sio.OPTION_SETS:
        opts = sio.options(name, tol)
        for track, m in ((clean, None), (clean, mask), (odd, mask)):
            want, dk = sio.rounds(twin.forward_grad, track, m, K, sio.LAMBDA, **opts)
            got, dl = twin.project(flat(track), K, sio.c_from(twin.lib, opts, None if m is None else words.ctypes.data, frames=T, lam=sio.LAMBDA))
            sio.assert_same(got.reshape(track.shape), want, (name, m is None))
            sio.assert_same(dl, dk, (name, "d_last"))
            h = held if m is not None else (held & ~mask)
            assert got.reshape(track.shape)[h].tobytes() == track[h].tobytes(), name
        for at in places:      # (the odd track came last)
            assert got.reshape(odd.shape)[at].tobytes() == odd[at].tobytes()
    # the coupling does something: the same call with lambda 0 gives other bits
    off, _ = twin.project(flat(clean), K, sio.c_from(twin.lib, opts, words.ctypes.data, frames=T, lam=0.0))
    on, _ = twin.project(flat(clean), K, sio.c_from(twin.lib, opts, words.ctypes.data, frames=T, lam=sio.LAMBDA))
    assert on.tobytes() != off.tobytes()


# ------------------------------------------------------------------------------------------ 3. the fill
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", sio.CASES, ids=sko.case_id)
def test_fill(case, act):
    twin, J = twin_of(case, act)
    a, b = sio.make_pairs(case)
    assert 0 < (io.dot4(a, b) < 0).sum() < a.shape[0] * J or J == 1      # the alignment has work to do
    x = sio.ends_of(a, b, T)
    want = sio.fill(a, b, T, "nlerp", np.float32)
    got, d = twin.project(flat(x), 0, sio.c_options3(twin.lib, None, T, 0.0, sio.NLERP))
    sio.assert_same(got.reshape(want.shape), want, "nlerp")
    assert not d.any()
    # only the end frames of the input are read
    y = x.copy()
    y[:, 1:-1] = np.float32(np.nan)
    again, _ = twin.project(flat(y), 0, sio.c_options3(twin.lib, None, T, 0.0, sio.NLERP))
    assert again.tobytes() == got.tobytes()
    # slerp: within four times the float32 error of the formula on these inputs, measured here
    s32, s64 = sio.fill(a, b, T, "slerp", np.float32), sio.fill(a, b, T, "slerp", np.float64)
    measured = float(np.abs(s32.astype(np.float64) - s64).max())
    sl, d = twin.project(flat(x), 0, sio.c_options3(twin.lib, None, T, 0.5, sio.SLERP))
    sl = sl.reshape(s64.shape)
    err = float(np.abs(sl.astype(np.float64) - s64).max())
    print(f"[fill {sko.case_id(case)}] numpy float32 slerp against fp64 {measured:.3e}, twin against fp64 {err:.3e}, bound {4 * measured:.3e}")
    assert err <= 4 * measured and not d.any()
    for out in (got.reshape(want.shape), sl):
        assert out[:, 0].tobytes() == a.tobytes() and out[:, -1].tobytes() == want[:, -1].tobytes()
    # T = 2: a and aligned b, untouched by any step
    two = sio.ends_of(a, b, 2)
    for fill in (sio.SLERP, sio.NLERP):
        out, d2 = twin.project(flat(two), 3, sio.c_options3(twin.lib, None, 2, 0.5, fill, renorm=1))
        out = out.reshape(two.shape)
        assert out[:, 0].tobytes() == a.tobytes() and out[:, 1].tobytes() == io.align(a, b).tobytes()
        assert np.isfinite(d2).all()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing():
    twin, J = twin_of(("hand", True), "lrelu")
    lib = twin.lib
    q = flat(sio.given_track(("hand", True), 2, 4))      # 8 poses
    words = np.zeros(9, np.uint32)
    at = words.ctypes.data

    def refused(opt, field, **kw):
        rc, out, d = twin.call(q, 2, opt, **kw)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_cpu_last_error(twin.h), (field, lib.pndf_cpu_last_error(twin.h))
        if not kw:
            assert np.all(out == 7.0), field
        assert np.all(d == 7.0), field

    for size in (0, 12, 20, 31, 33, 40, 47, 49, 64):
        refused(sio.c_options3(lib, at, 4, size=size), "struct_size")
    refused(sio.c_options3(lib, at, 4, reserved2=1), "reserved2")
    refused(sio.c_options3(lib, at, 0, reserved2=-1), "reserved2")
    for frames in (1, -1, -4, 16385, 2 ** 31 - 1):
        refused(sio.c_options3(lib, at, frames), "frames")
    for frames in (3, 5, 16):      # B = 8
        refused(sio.c_options3(lib, at, frames), "frames")
    for lam in (-0.1, 1.5, math.nan, math.inf):
        refused(sio.c_options3(lib, at, 4, lam), "lambda")
    for fill in (3, -1):
        refused(sio.c_options3(lib, at, 4, 0.5, fill), "fill")
    refused(sio.c_options3(lib, at, 0, 0.5), "lambda")
    refused(sio.c_options3(lib, at, 0, 0.0, sio.SLERP), "fill")
    refused(sio.c_options3(lib, at, 4, 0.5), "q_out", in_place=True)
    assert q.tobytes() == flat(sio.given_track(("hand", True), 2, 4)).tobytes()
    # q_out overlapping q_in by all but one pose
    buf = np.concatenate([q, np.full((1,) + q.shape[1:], 7.0, np.float32)])
    d = np.full(8, 7.0, np.float32)
    before = buf.copy()
    opt = sio.c_options3(lib, at, 4, 0.5)
    assert lib.pndf_project_ex_cpu(twin.h, buf.ctypes.data, buf[1:].ctypes.data, d.ctypes.data, 8, 2, ctypes.byref(opt)) == BAD_ARG
    assert b"q_out" in lib.pndf_cpu_last_error(twin.h) and buf.tobytes() == before.tobytes() and np.all(d == 7.0)
    # everything base2 already refuses, with the text of the smaller structs
    refused(sio.c_options3(lib, at, 4, reserved=1), "reserved")
    for odd in (1, 2, 3):
        refused(sio.c_options3(lib, at + odd, 4), "observed")
    for field, kw in (("step_size", dict(step_size=0.0)), ("step_size", dict(step_size=math.nan)), ("tol", dict(tol=-1e-3)), ("tol", dict(tol=math.nan)),
                      ("renorm", dict(renorm=3))):
        rc, _, _ = twin.call(q, 2, sco.c_options(lib, **kw))
        text = lib.pndf_cpu_last_error(twin.h)
        refused(sio.c_options3(lib, at, 4, **kw), field)
        assert rc == BAD_ARG and lib.pndf_cpu_last_error(twin.h) == text
    # a good struct after all that, and the Python layer
    rc, out, _ = twin.call(q, 2, sio.c_options3(lib, at, 4, 0.5, sio.SLERP))
    assert rc == 0 and not np.any(out == 7.0)
    from posendf_amd.engine import PndfError
    out, d = np.full_like(q, 7.0), np.full(len(q), 7.0, np.float32)
    for field, kw in (("frames", dict(frames=3)), ("lambda", dict(frames=4, smooth=2.0)), ("lambda", dict(smooth=0.5)), ("fill", dict(fill="slerp")),
                      ("step_size", dict(frames=4, step_size=-1.0))):
        with pytest.raises(PndfError, match=field):
            twin.eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), 2, **kw)
    with pytest.raises(PndfError, match="fill"):
        twin.eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), 2, frames=4, fill="cubic")
    assert np.all(out == 7.0) and np.all(d == 7.0)


def test_the_other_entry_points_refuse_the_48_byte_struct():
    """every other function with a pndf_project_options parameter: a 48-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here the
    host twins and the two stateless helpers, which decide it before a device is looked for; pndf_project_ex, pndf_complete and
    pndf_interpolate need a device handle and are in the GPU file."""
    from posendf_amd.abi import ProjectOptions
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    big = sio.c_options3(lib, words.ctypes.data, 2)
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


# ------------------------------------------------------------------------------------------ 5. the 21-joint handle
@pytest.mark.parametrize("encoder", [True, False], ids=["enc", "noenc"])
@pytest.mark.parametrize("act", co.ACTS)
def test_smpl_table_equals_pndf_interpolate_cpu(act, encoder):
    from posendf_amd import synth
    from posendf_amd.engine import CpuEngine
    a, b = io.make_pairs()
    Pn, Tn = io.P, io.T
    mask = io.make_mask()
    words = io.pack(mask)
    assert np.array_equal(words, sio.pack(mask))
    eng = CpuEngine(act, encoder=encoder, hidden=None if encoder else sko.HIDDEN)
    eng.load_weights(co.weights() if encoder else sko.network(synth.PARENT, 7, encoder=False))
    x = flat(sio.ends_of(a, b, Tn))
    n = Pn * Tn
    for mode, steps, lam, m in [(mode, steps, lam, m) for mode in ("slerp", "nlerp") for steps in (0, 1, 4) for lam in (0.0, 0.5) for m in (None, words)]:
        want, d_want = np.full((n, 21, 4), 7.0, np.float32), np.full(n, 7.0, np.float32)
        eng.interpolate(a.ctypes.data, b.ctypes.data, None if m is None else m.ctypes.data, want.ctypes.data, d_want.ctypes.data, Pn, Tn, steps, mode=mode,
                        smooth=lam, renorm="unit")
        got, d_got = np.full((n, 21, 4), 7.0, np.float32), np.full(n, 7.0, np.float32)
        eng.project(x.ctypes.data, got.ctypes.data, d_got.ctypes.data, n, steps, renorm="unit", observed_ptr=None if m is None else m.ctypes.data,
                    frames=Tn, smooth=lam, fill=mode)
        assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes(), (mode, steps, lam, m is None)
    assert not np.array_equal(got, x)


def test_pndf_interpolate_cpu_still_refuses_a_skeleton_handle():
    twin, J = twin_of(("hand", True), "lrelu")
    lib, h = twin.lib, twin.h
    q = sko.poses(sko.HAND, 4)
    out = np.full((4, J, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(h, q.ctypes.data, q[2:].ctypes.data, None, out.ctypes.data, None, 2, 2, 0, 1, 0.5, None) == UNSUPPORTED
    text = lib.pndf_cpu_last_error(h)
    assert b"21-joint" in text and b"pndf_project_options3" in text and np.all(out == 7.0)


# ------------------------------------------------------------------------------------------ 6. Python
@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_interpolate_on_cpu(case, act):
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cpu_model(parents, act, sd)
    twin = Twin(parents, act, sd)
    a_np, b_np = sio.make_pairs(case)
    a, b = torch.from_numpy(a_np.copy()), torch.from_numpy(b_np.copy())
    mask = sio.make_mask(J)
    words = sio.pack(mask)
    # the twin's bits through the C struct: one engine call
    want, d_want = twin.project(flat(sio.ends_of(a_np, b_np, T)), K, sio.c_options3(twin.lib, words.ctypes.data, T, 0.5, sio.SLERP, renorm=1))
    track, d = net.interpolate(a, b, T, steps=K, smooth=0.5, observed=torch.from_numpy(mask))
    assert track.shape == (P, T, J, 4) and d.shape == (P, T)
    assert track.numpy().tobytes() == want.tobytes() and d.numpy().tobytes() == d_want.tobytes()
    assert track[:, 0].numpy().tobytes() == a_np.tobytes() and track[:, -1].numpy().tobytes() == io.align(a_np, b_np).tobytes()
    assert a.numpy().tobytes() == a_np.tobytes() and b.numpy().tobytes() == b_np.tobytes()
    assert net.interpolate(a, b, T, steps=K, smooth=0.5, observed=torch.from_numpy(mask), return_dist=False).numpy().tobytes() == want.tobytes()
    # the observed joints are the fill's, bit for bit
    start = net.interpolate(a, b, T, steps=0, return_dist=False)
    m = torch.from_numpy(mask)
    assert torch.equal(track[m].view(torch.int32), start[m].view(torch.int32))
    # [T,J] and [J] masks
    one = m[1]
    x, dx = net.interpolate(a, b, T, steps=2, observed=one, mode="nlerp")
    y, dy = net.interpolate(a, b, T, steps=2, observed=one.expand(P, T, J), mode="nlerp")
    assert torch.equal(x, y) and torch.equal(dx, dy)
    x, _ = net.interpolate(a, b, T, steps=2, observed=one[2])
    y, _ = net.interpolate(a, b, T, steps=2, observed=one[2].expand(P, T, J))
    assert torch.equal(x, y)
    # steps = 0 is the fill and zero distances; wrong arguments
    s, ds = net.interpolate(a, b, T, steps=0, mode="nlerp")
    sio.assert_same(s.numpy(), sio.fill(a_np, b_np, T, "nlerp"), "fill")
    assert not bool(ds.any())
    for kw in (dict(frames=1), dict(frames=T, mode="cubic"), dict(frames=T, smooth=1.5), dict(frames=T, observed=torch.zeros(T, J + 1, dtype=torch.bool)),
               dict(frames=T, observed=torch.zeros(P, T, J))):
        with pytest.raises(PndfError):
            net.interpolate(a, b, **kw)
    with pytest.raises(PndfError):
        net.interpolate(a, b[:2], T)
    e, de = net.interpolate(a[:0], b[:0], T, steps=2)
    assert e.shape == (0, T, J, 4) and de.shape == (0, T)


def test_pose_interpolation_driver_on_a_hand():
    from posendf_amd.pose_interpolation import PoseInterpolation, segment_lengths
    case = ("hand", True)
    parents, sd = sko.case_network(case, "softplus")
    J = len(parents)
    net = cpu_model(parents, "softplus", sd)
    a_np, b_np = sio.make_pairs(case)
    a, b = torch.from_numpy(a_np), torch.from_numpy(b_np)
    driver = PoseInterpolation(net, body_model=None, device="cpu")
    track, dist, meshes = driver.interpolate(a, b, T, steps=5)
    want, d_want = net.interpolate(a, b, T, steps=5, smooth=0.5)
    assert track.shape == (P, T, J, 4) and dist.shape == (P, T) and not meshes
    assert torch.equal(track, want) and torch.equal(dist, d_want) and bool(torch.isfinite(dist).all())
    one, _, _ = driver.interpolate(a[0], b[0], T, steps=5)
    assert torch.equal(one, track[:1])
    seg = segment_lengths(track)      # J-agnostic: the oracle's, for 15 joints
    assert seg.shape == (P, T - 1) and np.allclose(seg.numpy(), sio.segment_lengths(track.numpy()), rtol=1e-3, atol=1e-3)
    with pytest.raises(ValueError, match="21"):
        PoseInterpolation(net, body_model=object(), device="cpu").interpolate(a, b, T)


@pytest.mark.parametrize("act", sio.ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_coupling_evens_the_track(case, act):
    """T = 7, 50 steps, renormalize="unit", slerp: smooth=0.5 gives every pair a smaller longest-to-mean segment ratio and a shorter path
    than smooth=0 -- in the fp64 oracle first, then on the model's output"""
    r0, l0 = sio.oracle_evenness(case, act, 0.0)
    r5, l5 = sio.oracle_evenness(case, act, 0.5)
    print(f"[evenness {sko.case_id(case)} {act}] fp64 oracle: ratio {r5.min():.2f} - {r5.max():.2f} against {r0.min():.2f} - {r0.max():.2f}, "
          f"path {l5.min():.1f} - {l5.max():.1f} against {l0.min():.1f} - {l0.max():.1f}")
    assert (r5 < r0).all() and (l5 < l0).all(), (r0, r5, l0, l5)
    parents, sd = sko.case_network(case, act)
    net = cpu_model(parents, act, sd)
    a, b = (torch.from_numpy(x) for x in sio.make_pairs(case))
    m0, m5 = (sio.evenness(net.interpolate(a, b, T, steps=sio.EVEN_STEPS, smooth=s, return_dist=False).numpy()) for s in (0.0, 0.5))
    assert (m5[0] < m0[0]).all() and (m5[1] < m0[1]).all(), (m0, m5)


# ------------------------------------------------------------------------------------------ 7. the library and the ABI
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert {"pndf_skel_enc_rev_kernel", "pndf_skel_fill_kernel"} <= ch.exported_symbols(ge.LIB)
    assert ctypes.sizeof(abi.ProjectOptions3) == 48 and engine.ProjectOptions3 is abi.ProjectOptions3
    o3 = abi.ProjectOptions3
    assert (o3.base2.offset, o3.frames.offset, o3.lambda_.offset, o3.fill.offset, o3.reserved2.offset) == (0, 32, 36, 40, 44)
    lib = engine.load_library()
    o = engine.project_options3(lib, 64, 7, smooth=0.25, fill="nlerp", step_size=0.5, renorm="unit", tol=0.25)
    assert (o.base2.base.struct_size, o.base2.base.step_size, o.base2.base.renorm, o.base2.base.tol, o.base2.observed, o.base2.reserved) == (48, 0.5, 1, 0.25, 64, 0)
    assert (o.frames, o.lambda_, o.fill, o.reserved2) == (7, 0.25, sio.NLERP, 0)
    o = engine.project_options3(lib, None, 3)
    assert (o.base2.base.struct_size, o.base2.observed, o.frames, o.lambda_, o.fill) == (48, None, 3, 0.0, sio.GIVEN)
    assert abi.TRACK_FILLS == sio.FILLS
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sio.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point and no new header
    assert not [n for n in abi.PRODUCT_EXPORTS if "interpolate" in n and "skel" in n] and not hasattr(lib, "pndf_skel_interpolate")
