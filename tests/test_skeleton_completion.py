"""Pose completion for other skeletons on the host (pndf_project_options2 of include/posendf_amd.h): the host
twin pndf_project_ex_cpu with a joint mask against the numpy statement of the masked step, to the bit; no mask = the call without
one; every joint held; the SMPL table against pndf_complete_cpu; in place; the refusals; `SkeletonPoseNDF.complete` and
`PoseCompletion` on a cpu model; the library's symbols and the struct as a C caller writes it.  Runs without a GPU;
tests/test_skeleton_completion_gpu.py holds the HIP unit to the same statements."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cabi_headers as ch
import completion_oracle as co
import skeleton_completion_oracle as sco
import skeleton_oracle as sko

BAD_ARG, UNSUPPORTED = sco.BAD_ARG, sco.UNSUPPORTED
B = sko.NPOSE      # 48


class Twin:
    """pndf_*_cpu of one network with numpy in and out; `opt`: a ctypes struct (either size), or None"""

    def __init__(self, parents, act, sd, encoder=True, hidden=sko.HIDDEN):
        from posendf_amd.engine import CpuEngine
        self.eng = CpuEngine(act, encoder=encoder, hidden=hidden, parents=parents)
        self.eng.load_weights(sd)
        self.lib, self.h = self.eng.lib, self.eng.handle

    def forward_grad(self, q):
        q = np.ascontiguousarray(q, np.float32)
        d, dq = np.full(len(q), 7.0, np.float32), np.full(q.shape, 7.0, np.float32)
        self.eng.forward_grad(q.ctypes.data, None, d.ctypes.data, dq.ctypes.data, len(q))
        return d, dq

    def forward(self, q):
        q = np.ascontiguousarray(q, np.float32)
        d = np.full(len(q), 7.0, np.float32)
        self.eng.forward(q.ctypes.data, d.ctypes.data, len(q))
        return d

    def call(self, q, steps, opt, in_place=False):
        """(status, q_out, d_last) of pndf_project_ex_cpu; the outputs are prefilled with 7.0"""
        q = np.array(q, np.float32, order="C")
        out = q if in_place else np.full(q.shape, 7.0, np.float32)
        d = np.full(len(q), 7.0, np.float32)
        rc = self.lib.pndf_project_ex_cpu(self.h, q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), steps,
                                          None if opt is None else ctypes.byref(opt))
        return rc, out, d

    def project(self, q, steps, opt, in_place=False):
        rc, out, d = self.call(q, steps, opt, in_place)
        assert rc == 0, self.lib.pndf_cpu_last_error(self.h)
        return out, d


def twin_of(case, act):
    parents, sd = sko.case_network(case, act)
    return Twin(parents, act, sd, encoder=case[1]), len(parents)


# ------------------------------------------------------------------------------------------ 1. the masked step is the stated step
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", sco.CASES, ids=sko.case_id)
def test_masked_steps_are_the_stated_step(case, act):
    twin, J = twin_of(case, act)
    q = sko.case_poses(case, B)
    mask = sco.make_mask(B, J)
    words = sco.pack(mask)
    assert not mask[sco.ALL_FREE].any() and mask[sco.ALL_HELD].all() and (J < 32 or (words >> 31).any())
    d0 = twin.forward(q)
    tol = float(np.median(d0))
    for opts in sco.option_sets(tol):
        want, dk = sco.rounds(twin.forward_grad, q, mask, sco.STEPS, **opts)
        got, dl = twin.project(q, sco.STEPS, sco.c_from(twin.lib, opts, words.ctypes.data))
        assert got.tobytes() == want.tobytes() and dl.tobytes() == dk.tobytes(), opts
        assert got[mask].tobytes() == q[mask].tobytes(), opts
        if "tol" in opts:
            rest = d0 < np.float32(tol)
            assert rest.any() and not rest.all()
            assert got[rest].tobytes() == q[rest].tobytes()
        moved = (d0 > 0) & (~rest if "tol" in opts else True)      # (d == 0 behind the output ReLU: a step of length zero)
        free = moved[:, None] & ~mask
        if J > 1:      # every free joint of a pose that does not rest moves (one joint: the true gradient is zero, skeleton_oracle.grad_rows)
            assert free.any() and (got[free] != q[free]).any(axis=-1).all(), opts


# ------------------------------------------------------------------------------------------ 2. no mask means today's call
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("hand", False)], ids=sko.case_id)
def test_no_mask_is_the_call_without_one(case, act):
    twin, J = twin_of(case, act)
    q = sko.case_poses(case, B)
    zeros = np.zeros(B, np.uint32)
    tol = float(np.median(twin.forward(q)))
    for opts in sco.option_sets(tol):
        small, d_small = twin.project(q, sco.STEPS, sco.c_from(twin.lib, opts, large=False))
        for observed in (None, zeros.ctypes.data):
            big, d_big = twin.project(q, sco.STEPS, sco.c_from(twin.lib, opts, observed))
            assert big.tobytes() == small.tobytes() and d_big.tobytes() == d_small.tobytes(), (opts, observed)
        if not opts:
            null, d_null = twin.project(q, sco.STEPS, None)
            assert null.tobytes() == small.tobytes() and d_null.tobytes() == d_small.tobytes()
            assert not np.array_equal(small, q)


# ------------------------------------------------------------------------------------------ 3. every joint held
def odd_poses(case, J):
    """the poses of a case with a NaN of a non-default payload in pose 5, a signalling one in pose 6 and a zero quaternion in pose 7"""
    q = sko.case_poses(case, B).copy()
    bits = q.view(np.uint32)
    bits[5, J // 2, 1] = 0x7FC12345
    bits[6, 0, 3] = 0xFF812345
    q[7, J - 1] = 0.0
    return q


@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True), ("one", True), ("hand", False)], ids=sko.case_id)
def test_all_joints_held(case, act):
    twin, J = twin_of(case, act)
    q = odd_poses(case, J)
    words = np.full(B, 0xFFFFFFFF, np.uint32)      # bits J .. 31 are ignored
    tol = float(np.median(twin.forward(sko.case_poses(case, B))))
    d_fwd = twin.forward(q)
    assert np.isnan(d_fwd[5:7]).all() and np.isfinite(np.delete(d_fwd, (5, 6))).all()
    for opts in sco.option_sets(tol):
        got, dl = twin.project(q, sco.STEPS, sco.c_from(twin.lib, opts, words.ctypes.data))
        assert got.tobytes() == q.tobytes(), opts
        fin = np.isfinite(d_fwd)
        assert dl[fin].tobytes() == d_fwd[fin].tobytes() and np.isnan(dl[~fin]).all(), opts


@pytest.mark.parametrize("act", sko.CASE_ACTS)
def test_a_nan_in_a_held_joint_stays_in_its_pose(act):
    case = ("tree32", True)
    twin, J = twin_of(case, act)
    q = sko.case_poses(case, B)
    mask = sco.make_mask(B, J)
    j = int(np.flatnonzero(mask[5])[0])
    bad = q.copy()
    bad.view(np.uint32)[5, j, 2] = 0x7FC12345
    words = sco.pack(mask)
    opt = sco.c_options2(twin.lib, words.ctypes.data)
    clean, d_clean = twin.project(q, sco.STEPS, opt)
    got, dl = twin.project(bad, sco.STEPS, opt)
    others = np.arange(B) != 5
    assert got[others].tobytes() == clean[others].tobytes() and dl[others].tobytes() == d_clean[others].tobytes()
    assert got[5][mask[5]].tobytes() == bad[5][mask[5]].tobytes() and np.isnan(dl[5])


# ------------------------------------------------------------------------------------------ 4. the SMPL table: pndf_complete_cpu
@pytest.mark.parametrize("name", ["plain", "unit"])
@pytest.mark.parametrize("act", co.ACTS)
def test_smpl_table_equals_pndf_complete_cpu(act, name):
    from posendf_amd import synth
    from posendf_amd.engine import CpuEngine
    q, mask = np.ascontiguousarray(co.make_inputs(), np.float32), co.make_mask()
    words = co.pack(mask)
    assert np.array_equal(words, sco.pack(mask))
    eng = CpuEngine(act)
    eng.load_weights(co.weights())
    opts = co.options(name, act)
    want, d_want = np.full_like(q, 7.0), np.full(len(q), 7.0, np.float32)
    eng.complete(q.ctypes.data, words.ctypes.data, want.ctypes.data, d_want.ctypes.data, len(q), sco.STEPS, step_size=opts["step_size"],
                 renorm=opts["renormalize"], tol=opts["tol"])
    got, d_got = np.full_like(q, 7.0), np.full(len(q), 7.0, np.float32)
    eng.project(q.ctypes.data, got.ctypes.data, d_got.ctypes.data, len(q), sco.STEPS, step_size=opts["step_size"], renorm=opts["renormalize"],
                tol=opts["tol"], observed_ptr=words.ctypes.data)
    assert got.tobytes() == want.tobytes() and d_got.tobytes() == d_want.tobytes()
    assert got[mask].tobytes() == q[mask].tobytes() and not np.array_equal(got, q) and len(synth.PARENT) == mask.shape[1]
    # the encoder-less 21-joint model takes the mask too
    sd = sko.network(synth.PARENT, 7, encoder=False)
    twin = Twin(None, act, sd, encoder=False)
    out, _ = twin.project(q, 2, sco.c_options2(twin.lib, words.ctypes.data))
    ref, _ = sco.rounds(twin.forward_grad, q, mask, 2)
    assert out.tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------ 6. in place
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", False)], ids=sko.case_id)
def test_in_place_equals_out_of_place(case, act):
    parents = sko.SKELETONS[case[0]]
    twin = Twin(parents, act, sko.network(parents, 9, encoder=case[1]), encoder=case[1])
    J = len(parents)
    q = sko.case_poses(case, B)
    words = sco.pack(sco.make_mask(B, J))
    for opts in sco.option_sets(float(np.median(twin.forward(q)))):
        opt = sco.c_from(twin.lib, opts, words.ctypes.data)
        out, d = twin.project(q, sco.STEPS, opt)
        same, d_same = twin.project(q, sco.STEPS, opt, in_place=True)
        assert same.tobytes() == out.tobytes() and d_same.tobytes() == d.tobytes(), opts


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing():
    twin, J = twin_of(("hand", True), "lrelu")
    lib = twin.lib
    q = sko.case_poses(("hand", True), 8)
    words = np.zeros(9, np.uint32)
    at = words.ctypes.data

    def refused(opt, field):
        rc, out, d = twin.call(q, 2, opt)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_cpu_last_error(twin.h), (field, lib.pndf_cpu_last_error(twin.h))
        assert np.all(out == 7.0) and np.all(d == 7.0), field

    for size in (0, 12, 20, 31, 33):
        refused(sco.c_options2(lib, at, size=size), "struct_size")
        refused(sco.c_options(lib, size=size), "struct_size")
    refused(sco.c_options2(lib, at, reserved=1), "reserved")
    refused(sco.c_options2(lib, None, reserved=1 << 40), "reserved")
    for odd in (1, 2, 3):
        refused(sco.c_options2(lib, at + odd), "observed")
    for field, kw in (("step_size", dict(step_size=0.0)), ("step_size", dict(step_size=-0.5)), ("step_size", dict(step_size=math.inf)),
                      ("step_size", dict(step_size=math.nan)), ("tol", dict(tol=-1e-3)), ("tol", dict(tol=math.nan)), ("renorm", dict(renorm=3)),
                      ("renorm", dict(renorm=-1))):
        refused(sco.c_options2(lib, at, **kw), field)
        small = sco.c_options(lib, **kw)
        rc, _, _ = twin.call(q, 2, small)
        text = lib.pndf_cpu_last_error(twin.h)
        rc2, _, _ = twin.call(q, 2, sco.c_options2(lib, at, **kw))
        assert rc == rc2 == BAD_ARG and lib.pndf_cpu_last_error(twin.h) == text      # refused as in a 16-byte struct: the same text
    # a good struct after all that
    assert twin.call(q, 2, sco.c_options2(lib, at))[0] == 0
    # the Python layer
    from posendf_amd.engine import PndfError
    out, d = np.full_like(q, 7.0), np.full(len(q), 7.0, np.float32)
    with pytest.raises(PndfError, match="observed"):
        twin.eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), 2, observed_ptr=at + 2)
    with pytest.raises(PndfError, match="step_size"):
        twin.eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), 2, observed_ptr=at, step_size=-1.0)
    assert np.all(out == 7.0) and np.all(d == 7.0)


def test_the_other_entry_points_keep_refusing_the_larger_struct():
    """every other function with a pndf_project_options parameter: a 32-byte struct is PNDF_ERR_BAD_ARG as any size but 16 is.  Here
    the host twins and the two stateless helpers, which decide it before a device is looked for; pndf_project_ex needs a device
    handle and is in the GPU file."""
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("lrelu")
    eng.load_weights(co.weights())
    lib = eng.lib
    q = np.ascontiguousarray(co.make_inputs()[:4], np.float32)
    words = np.zeros(8, np.uint32)
    big = sco.c_options2(lib, words.ctypes.data)
    ok = sco.c_options(lib)
    out, d = np.full_like(q, 7.0), np.full(8, 7.0, np.float32)
    ref = ctypes.cast(ctypes.byref(big), ctypes.POINTER(type(ok)))
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    track = np.full((2, 2, 21, 4), 7.0, np.float32)
    assert lib.pndf_interpolate_cpu(eng.handle, q.ctypes.data, q[2:].ctypes.data, None, track.ctypes.data, d.ctypes.data, 2, 2, 0, 1, 0.0, ref) == BAD_ARG
    assert b"struct_size" in lib.pndf_cpu_last_error(eng.handle)
    assert np.all(out == 7.0) and np.all(d == 7.0) and np.all(track == 7.0)
    # the stateless helpers: the options are checked first, host addresses are never read
    assert lib.pndf_complete_step(out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 4, ref, None) == BAD_ARG
    assert lib.pndf_interp_band_step(q.ctypes.data, out.ctypes.data, d.ctypes.data, q.ctypes.data, None, 2, 2, 0.0, ref, None) == BAD_ARG
    assert np.all(out == 7.0) and np.all(d == 7.0)
    # with the 16-byte struct the host twins run
    assert lib.pndf_complete_cpu(eng.handle, q.ctypes.data, words.ctypes.data, out.ctypes.data, d.ctypes.data, 4, 1, ctypes.byref(ok)) == 0


def test_the_other_twins_still_refuse_a_skeleton_handle():
    """the three calls of tests/test_skeleton.py::test_the_other_twins_stay_21_joint: completion for a skeleton is the options struct,
    not pndf_complete_cpu"""
    twin, J = twin_of(("hand", True), "lrelu")
    lib, h = twin.lib, twin.h
    q = sko.poses(sko.HAND, 4)
    out, d = np.empty_like(q), np.empty(4, np.float32)
    assert lib.pndf_complete_cpu(h, q.ctypes.data, None, out.ctypes.data, d.ctypes.data, 4, 1, None) == UNSUPPORTED
    assert b"21-joint" in lib.pndf_cpu_last_error(h) and b"pndf_project_options2" in lib.pndf_cpu_last_error(h)
    assert lib.pndf_second_order_cpu(h, q.ctypes.data, q.ctypes.data, None, None, None, None, None, out.ctypes.data, 4) == UNSUPPORTED
    assert lib.pndf_interpolate_cpu(h, q.ctypes.data, q.ctypes.data, None, out.ctypes.data, None, 1, 2, 0, 0, 0.0, None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ 8. Python
def cpu_model(parents, act, sd, encoder=True):
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    net = SkeletonPoseNDF(skeleton_config(list(parents), act, "cpu", hidden=sko.HIDDEN, encoder=encoder))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.eval()


@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_complete_on_cpu(case, act):
    from posendf_amd import PoseNDF
    from posendf_amd.engine import PndfError
    from posendf_amd.model_base import pack_observed
    parents, sd = sko.case_network(case, act)
    J = len(parents)
    net = cpu_model(parents, act, sd)
    q = torch.from_numpy(sko.case_poses(case, B))
    mask = sco.make_mask(B, J)
    # the packed words, joint 31 included
    words = pack_observed(torch.from_numpy(mask), B, "cpu", J)
    assert words.dtype == torch.int32 and np.array_equal(words.numpy().view(np.uint32), sco.pack(mask))
    assert PoseNDF.pack_observed is pack_observed
    # None is project
    p, dp = net.project(q, steps=sco.STEPS, renormalize="unit")
    c, dc = net.complete(q, None, steps=sco.STEPS, renormalize="unit")
    assert torch.equal(p, c) and torch.equal(dp, dc)
    # a [B,J] mask against the twin through the C struct; held joints equal the input, free joints differ
    twin = Twin(parents, act, sd)
    packed = sco.pack(mask)      # (kept alive: the struct holds its address)
    want, d_want = twin.project(q.numpy(), sco.STEPS, sco.c_options2(twin.lib, packed.ctypes.data))
    out, d = net.complete(q, torch.from_numpy(mask), steps=sco.STEPS)
    assert out.shape == (B, J, 4) and d.shape == (B, 1)
    assert out.numpy().tobytes() == want.tobytes() and d.numpy().reshape(-1).tobytes() == d_want.tobytes()
    m = torch.from_numpy(mask)
    free = ~m & torch.from_numpy(twin.forward(q.numpy()) > 0)[:, None]      # (d == 0 behind the output ReLU: a step of length zero)
    assert torch.equal(out[m], q[m]) and bool(free.any()) and bool((out[free] != q[free]).any(dim=-1).all())
    assert net.complete(q, m, steps=sco.STEPS, return_dist=False).numpy().tobytes() == want.tobytes()
    # a [J] mask is the same mask for every pose
    one = torch.from_numpy(mask[2])
    a, da = net.complete(q, one, steps=2, step_size=0.5, renormalize="unit_flip")
    b, db = net.complete(q, one.expand(B, J), steps=2, step_size=0.5, renormalize="unit_flip")
    assert torch.equal(a, b) and torch.equal(da, db) and torch.equal(a[:, one], q[:, one])
    if J == 32:
        assert bool(one[31]) and int(words[2]) < 0
    # wrong shapes and dtypes, an empty batch
    for wrong in (torch.zeros(J + 1, dtype=torch.bool), torch.zeros(B - 1, J, dtype=torch.bool), torch.zeros(B, J), torch.zeros(B, J, dtype=torch.int32)):
        with pytest.raises(PndfError):
            net.complete(q, wrong, steps=1)
    e, de = net.complete(q[:0], torch.zeros(0, J, dtype=torch.bool), steps=2)
    assert e.shape == (0, J, 4) and de.shape == (0, 1)
    e, de = net.complete(q[:0], one, steps=2)
    assert e.shape == (0, J, 4) and de.shape == (0, 1)


@pytest.mark.parametrize("select", ["all", "best"])
def test_pose_completion_driver_on_a_hand(select):
    from posendf_amd.pose_completion import PoseCompletion, best_hypothesis
    parents, sd = sko.case_network(("hand", True), "softplus")
    J, K, n = len(parents), 3, 10
    net = cpu_model(parents, "softplus", sd)
    driver = PoseCompletion(net, body_model=None, device="cpu")
    q = torch.from_numpy(sko.case_poses(("hand", True), n))
    q[3, 4] = float("nan")      # an unobserved joint may hold anything: it is filled
    obs = torch.from_numpy(sco.make_mask(n, J))
    obs[3, 4] = False
    res = driver.complete(q, obs, hypotheses=K, fill="random", select=select, generator=torch.Generator().manual_seed(3), steps=sco.STEPS,
                          renormalize="unit")
    out, dist, meshes = res[0], res[1], res[-1]
    assert out.shape == (n, K, J, 4) and dist.shape == (n, K) and meshes == {} and bool(torch.isfinite(dist).all())
    if select == "best":
        assert len(res) == 4 and torch.equal(res[2], best_hypothesis(dist))
    else:
        assert len(res) == 3
    for k in range(K):      # observed joints: the input's, in every hypothesis
        assert torch.equal(out[:, k][obs], q[obs])
    free = ~obs
    assert not torch.equal(out[:, 0][free], out[:, 1][free])      # the hypotheses start apart
    again = driver.complete(q, obs, hypotheses=K, fill="random", select=select, generator=torch.Generator().manual_seed(3), steps=sco.STEPS,
                            renormalize="unit")
    assert torch.equal(again[0], out) and torch.equal(again[1], dist)
    # one mask for every pose, and the body model is SMPL's
    out1 = driver.complete(q[:2], obs[0] | obs[2], hypotheses=2, fill="given", steps=1)[0]
    assert out1.shape == (2, 2, J, 4)
    with pytest.raises(ValueError, match="21"):
        PoseCompletion(net, body_model=object(), device="cpu").complete(q, obs)


# ------------------------------------------------------------------------------------------ 9. the library and the ABI
def test_library_symbols_and_abi(tmp_path):
    import __graft_entry__ as ge
    from posendf_amd import abi, engine
    assert "pndf_skel_enc_rev_kernel" in ch.exported_symbols(ge.LIB)
    assert ctypes.sizeof(abi.ProjectOptions2) == 32 and ctypes.sizeof(abi.ProjectOptions) == 16 and engine.ProjectOptions2 is abi.ProjectOptions2
    assert (abi.ProjectOptions2.base.offset, abi.ProjectOptions2.observed.offset, abi.ProjectOptions2.reserved.offset) == (0, 16, 24)
    lib = engine.load_library()
    o = engine.project_options2(lib, 64, step_size=0.5, renorm="unit", tol=0.25)
    assert (o.base.struct_size, o.base.step_size, o.base.renorm, o.base.tol, o.observed, o.reserved) == (32, 0.5, 1, 0.25, 64, 0)
    o = engine.project_options2(lib, None)
    assert (o.base.struct_size, o.base.step_size, o.base.renorm, o.base.tol, o.observed, o.reserved) == (32, 1.0, 0, 0.0, None, 0)
    ok, diagnostics = ch.compiles_as_c99(tmp_path, sco.C99_SNIPPET)
    assert ok, diagnostics
    # no new entry point: the two that take the struct are the ones the headers had
    assert "pndf_skel_complete" not in abi.PRODUCT_EXPORTS and not hasattr(lib, "pndf_skel_complete")
