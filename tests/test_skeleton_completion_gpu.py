"""Pose completion for other skeletons on an MI355X (pndf_project_options2 of include/posendf_amd.h, csrc/pndf_skeleton.hip; DESIGN.md
section 2j): pndf_skel_project with a joint mask against forward_grad + the numpy statement of the masked step, to the bit; no mask =
the call without one; every joint held; batch independence across the chunk seam; in place; the refusals; `SkeletonPoseNDF.complete`
and `PoseCompletion` on cuda.  tests/test_skeleton_completion.py holds the host twin to the same statements."""
import ctypes
import math

import numpy as np
import pytest

import skeleton_completion_oracle as sco
import skeleton_oracle as sko
from posendf_amd import synth

pytestmark = pytest.mark.gpu
BAD_ARG = sco.BAD_ARG
CHUNK = 16384      # SK_CHUNK of csrc/pndf_skeleton.hip
B = 300            # one encoder workgroup of 256 lanes and an edge


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    return torch


class Unit:
    """pndf_skel_* on cuda:0 with numpy in and out; the options as the C structs of skeleton_completion_oracle"""

    def __init__(self, torch, parents, act, sd, encoder=True, hidden=sko.HIDDEN):
        from posendf_amd.engine import SkeletonEngine
        self.torch, self.J = torch, len(parents)
        self.eng = SkeletonEngine(parents, act, encoder=encoder, hidden=hidden)
        self.eng.load_weights(sd)
        self.lib, self.h = self.eng.lib, self.eng.handle

    def ws(self, n_poses):
        n = self.eng.workspace_bytes(n_poses)
        return self.torch.empty(max(n, 16), dtype=self.torch.uint8, device="cuda:0"), n

    def dev(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()

    def words(self, w):
        """uint32 words -> a device tensor that holds their bits (int32)"""
        return self.dev(np.ascontiguousarray(w, np.uint32).view(np.int32), np.int32)

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def forward(self, q):
        q, (ws, n) = self.dev(q), self.ws(len(q))
        d = self.torch.full((len(q),), 7.0, device="cuda:0")
        self.eng.forward(q.data_ptr(), d.data_ptr(), len(q), ws.data_ptr(), n, self.stream())
        return d.cpu().numpy()

    def forward_grad(self, q):
        q, (ws, n) = self.dev(q), self.ws(len(q))
        d, dq = self.torch.full((len(q),), 7.0, device="cuda:0"), self.torch.full(q.shape, 7.0, device="cuda:0")
        self.eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), len(q), ws.data_ptr(), n, self.stream())
        return d.cpu().numpy(), dq.cpu().numpy()

    def call(self, q, steps, make_opt, words=None, in_place=False):
        """(status, q_out, d_last) of pndf_skel_project; `make_opt(address of the device words or None)` -> a ctypes struct or None;
        the outputs are prefilled with 7.0"""
        q, (ws, n) = self.dev(q), self.ws(len(q))
        w = None if words is None else self.words(words)
        opt = make_opt(None if w is None else w.data_ptr())
        out = q if in_place else self.torch.full(q.shape, 7.0, device="cuda:0")
        d = self.torch.full((len(q),), 7.0, device="cuda:0")
        rc = self.lib.pndf_skel_project(self.h, q.data_ptr(), out.data_ptr(), d.data_ptr(), len(q), steps, None if opt is None else ctypes.byref(opt),
                                        ws.data_ptr(), n, self.stream())
        self.torch.cuda.synchronize()
        return rc, out.cpu().numpy(), d.cpu().numpy()

    def masked(self, q, steps, words, opts=None, in_place=False):
        rc, out, d = self.call(q, steps, lambda at: sco.c_from(self.lib, opts or {}, at), words, in_place)
        assert rc == 0, self.lib.pndf_skel_last_error(self.h)
        return out, d


def unit_of(torch, case, act):
    parents, sd = sko.case_network(case, act)
    return Unit(torch, parents, act, sd, encoder=case[1]), len(parents)


# ------------------------------------------------------------------------------------------ 1. the masked step is the stated step
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", sco.CASES, ids=sko.case_id)
def test_masked_steps_are_the_stated_step(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    q = sko.case_poses(case, B)
    mask = sco.make_mask(B, J)
    words = sco.pack(mask)
    assert not mask[sco.ALL_FREE].any() and mask[sco.ALL_HELD].all() and (J < 32 or (words >> 31).any())
    d0 = unit.forward(q)
    tol = float(np.median(d0))
    for opts in sco.option_sets(tol):
        want, dk = sco.rounds(unit.forward_grad, q, mask, sco.STEPS, **opts)
        got, dl = unit.masked(q, sco.STEPS, words, opts)
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
def test_no_mask_is_the_call_without_one(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    q = sko.case_poses(case, B)
    tol = float(np.median(unit.forward(q)))
    for opts in sco.option_sets(tol):
        rc, small, d_small = unit.call(q, sco.STEPS, lambda at: sco.c_from(unit.lib, opts, large=False))
        assert rc == 0
        for words in (None, np.zeros(B, np.uint32)):
            big, d_big = unit.masked(q, sco.STEPS, words, opts)
            assert big.tobytes() == small.tobytes() and d_big.tobytes() == d_small.tobytes(), (opts, words is None)
        if not opts:
            rc, null, d_null = unit.call(q, sco.STEPS, lambda at: None)
            assert rc == 0 and null.tobytes() == small.tobytes() and d_null.tobytes() == d_small.tobytes()
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
def test_all_joints_held(torch_cuda, case, act):
    unit, J = unit_of(torch_cuda, case, act)
    q = odd_poses(case, J)
    words = np.full(B, 0xFFFFFFFF, np.uint32)      # bits J .. 31 are ignored
    tol = float(np.median(unit.forward(sko.case_poses(case, B))))
    d_fwd = unit.forward(q)
    fin = np.isfinite(d_fwd)      # (what a NaN pose's distance is, is the forward's business: d_last is held to it)
    assert np.delete(fin, (5, 6)).all()
    for opts in sco.option_sets(tol):
        got, dl = unit.masked(q, sco.STEPS, words, opts)
        assert got.tobytes() == q.tobytes(), opts
        assert dl[fin].tobytes() == d_fwd[fin].tobytes() and np.isnan(dl[~fin]).all(), opts
        same, _ = unit.masked(q, sco.STEPS, words, opts, in_place=True)
        assert same.tobytes() == q.tobytes(), opts


@pytest.mark.parametrize("act", sko.CASE_ACTS)
def test_a_nan_in_a_held_joint_stays_in_its_pose(torch_cuda, act):
    case = ("tree32", True)
    unit, J = unit_of(torch_cuda, case, act)
    q = sko.case_poses(case, B)
    mask = sco.make_mask(B, J)
    j = int(np.flatnonzero(mask[5])[0])
    bad = q.copy()
    bad.view(np.uint32)[5, j, 2] = 0x7FC12345
    words = sco.pack(mask)
    clean, d_clean = unit.masked(q, sco.STEPS, words)
    got, dl = unit.masked(bad, sco.STEPS, words)
    others = np.arange(B) != 5
    assert got[others].tobytes() == clean[others].tobytes() and dl[others].tobytes() == d_clean[others].tobytes()
    assert got[5][mask[5]].tobytes() == bad[5][mask[5]].tobytes()


# ------------------------------------------------------------------------------------------ 5. batch independence across the chunk seam
def test_batch_independence_across_the_chunk_seam(torch_cuda):
    parents = sko.HAND
    sd = sko.network(parents, 3, hidden=(32,))
    unit = Unit(torch_cuda, parents, "softplus", sd, hidden=(32,))
    n = CHUNK + 129      # 16,513: the second chunk holds 129 poses
    q = synth.make_poses(n, seed=5, num_joints=len(parents))
    mask = sco.make_mask(n, len(parents))
    words = sco.pack(mask)
    opts = dict(renormalize="unit", step_size=0.5)
    out, d = unit.masked(q, 2, words, opts)
    assert np.isfinite(out).all() and out[mask].tobytes() == q[mask].tobytes() and not np.array_equal(out[~mask], q[~mask])
    again, d_again = unit.masked(q, 2, words, opts)
    assert again.tobytes() == out.tobytes() and d_again.tobytes() == d.tobytes()
    for part in (slice(0, 300), slice(n - 129, n)):
        po, pd = unit.masked(q[part], 2, words[part], opts)
        assert po.tobytes() == out[part].tobytes() and pd.tobytes() == d[part].tobytes(), part
    # the mask of the second chunk is the second chunk's: shifting the words by one pose changes its result
    shifted, _ = unit.masked(q, 2, np.roll(words, 1), opts)
    assert shifted[n - 129:].tobytes() != out[n - 129:].tobytes()


# ------------------------------------------------------------------------------------------ 6. in place
@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", False)], ids=sko.case_id)
def test_in_place_equals_out_of_place(torch_cuda, case, act):
    parents = sko.SKELETONS[case[0]]
    unit = Unit(torch_cuda, parents, act, sko.network(parents, 9, encoder=case[1]), encoder=case[1])
    q = sko.case_poses(case, B)
    words = sco.pack(sco.make_mask(B, len(parents)))
    for opts in sco.option_sets(float(np.median(unit.forward(q)))):
        out, d = unit.masked(q, sco.STEPS, words, opts)
        same, d_same = unit.masked(q, sco.STEPS, words, opts, in_place=True)
        assert same.tobytes() == out.tobytes() and d_same.tobytes() == d.tobytes(), opts


# ------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_write_nothing(torch_cuda):
    unit, J = unit_of(torch_cuda, ("hand", True), "lrelu")
    lib = unit.lib
    q = sko.case_poses(("hand", True), 9)
    words = np.zeros(9, np.uint32)

    def refused(make_opt, field, q_in=q):
        rc, out, d = unit.call(q_in, 2, make_opt, words)
        assert rc == BAD_ARG, (field, rc)
        assert field.encode() in lib.pndf_skel_last_error(unit.h), (field, lib.pndf_skel_last_error(unit.h))
        assert np.all(out == 7.0) and np.all(d == 7.0), field

    for size in (0, 12, 20, 31, 33):
        refused(lambda at, size=size: sco.c_options2(lib, at, size=size), "struct_size")
        refused(lambda at, size=size: sco.c_options(lib, size=size), "struct_size")
    refused(lambda at: sco.c_options2(lib, at, reserved=1), "reserved")
    for odd in (1, 2, 3):
        refused(lambda at, odd=odd: sco.c_options2(lib, at + odd), "observed")
    for field, kw in (("step_size", dict(step_size=0.0)), ("step_size", dict(step_size=math.inf)), ("step_size", dict(step_size=math.nan)),
                      ("tol", dict(tol=-1e-3)), ("tol", dict(tol=math.nan)), ("renorm", dict(renorm=3)), ("renorm", dict(renorm=-1))):
        refused(lambda at, kw=kw: sco.c_options(lib, **kw), field)
        text = lib.pndf_skel_last_error(unit.h)
        refused(lambda at, kw=kw: sco.c_options2(lib, at, **kw), field)
        assert lib.pndf_skel_last_error(unit.h) == text      # refused as in a 16-byte struct: the same text
    rc, out, _ = unit.call(q, 2, lambda at: sco.c_options2(lib, at), words)
    assert rc == 0 and not np.any(out == 7.0)


def test_the_persistent_engine_keeps_refusing_the_larger_struct(torch_cuda):
    """pndf_project_ex, pndf_complete and pndf_interpolate on a pndf_create handle: a 32-byte struct is PNDF_ERR_BAD_ARG, nothing written"""
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
    big = sco.c_options2(lib, words.data_ptr())
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
    assert lib.pndf_interp_band_step(q.data_ptr(), out.data_ptr(), d.data_ptr(), q.data_ptr(), None, n // 2, 2, 0.0, ref, st) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((d == 7).all()) and bool((track == 7).all())
    # the 16-byte struct runs
    ok = sco.c_options(lib, renorm=1)
    assert lib.pndf_project_ex(eng.handle, q.data_ptr(), out.data_ptr(), d.data_ptr(), n, 1, ctypes.byref(ok), st) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7).any())


# ------------------------------------------------------------------------------------------ 8. Python
def cuda_model(torch, parents, act, sd):
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    net = SkeletonPoseNDF(skeleton_config(list(parents), act, "cuda:0", hidden=sko.HIDDEN))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.eval()


@pytest.mark.parametrize("act", sko.CASE_ACTS)
@pytest.mark.parametrize("case", [("hand", True), ("tree32", True)], ids=sko.case_id)
def test_model_complete_on_cuda(torch_cuda, case, act):
    torch = torch_cuda
    from posendf_amd.engine import PndfError
    parents, sd = sko.case_network(case, act)
    J, n = len(parents), 70
    net = cuda_model(torch, parents, act, sd)
    unit = Unit(torch, parents, act, sd)
    qn = sko.case_poses(case, n)
    q = torch.from_numpy(qn)
    mask = sco.make_mask(n, J)
    m = torch.from_numpy(mask)
    # None is project
    p, dp = net.project(q, steps=sco.STEPS, renormalize="unit")
    c, dc = net.complete(q, None, steps=sco.STEPS, renormalize="unit")
    assert c.is_cuda and torch.equal(p, c) and torch.equal(dp, dc)
    # a [B,J] mask (joint 31 held in pose 2 of the 32-joint tree): the unit's bits; held joints equal the input, free joints differ
    opts = dict(renormalize="unit", step_size=0.5)
    want, d_want = unit.masked(qn, sco.STEPS, sco.pack(mask), opts)
    out, d = net.complete(q, m, steps=sco.STEPS, **opts)
    assert out.shape == (n, J, 4) and d.shape == (n, 1) and (J < 32 or mask[2, 31])
    assert out.cpu().numpy().tobytes() == want.tobytes() and d.cpu().numpy().reshape(-1).tobytes() == d_want.tobytes()
    assert torch.equal(out.cpu()[m], q[m]) and bool((out.cpu()[~m] != q[~m]).any(dim=-1).all())
    assert torch.equal(net.complete(q.cuda(), m.cuda(), steps=sco.STEPS, return_dist=False, **opts), out)
    # under the pose gates against the oracle's fp64 trajectory
    sco.gate(out.cpu().numpy(), d.cpu().numpy(), qn, sd, mask, sco.STEPS, act, parents, f"cuda complete {sko.case_id(case)} {act}", **opts)
    plain, d_plain = net.complete(q, m, steps=sco.STEPS)
    sco.gate(plain.cpu().numpy(), d_plain.cpu().numpy(), qn, sd, mask, sco.STEPS, act, parents, f"cuda complete {sko.case_id(case)} {act} plain")
    # a [J] mask is the same mask for every pose
    one = m[2]
    a, da = net.complete(q, one, steps=2, step_size=0.5, renormalize="unit_flip")
    b, db = net.complete(q, one.expand(n, J), steps=2, step_size=0.5, renormalize="unit_flip")
    assert torch.equal(a, b) and torch.equal(da, db) and torch.equal(a.cpu()[:, one], q[:, one])
    # wrong shapes and dtypes, an empty batch
    for wrong in (torch.zeros(J + 1, dtype=torch.bool), torch.zeros(n - 1, J, dtype=torch.bool), torch.zeros(n, J), torch.zeros(n, J, dtype=torch.int32)):
        with pytest.raises(PndfError):
            net.complete(q, wrong, steps=1)
    e, de = net.complete(q[:0], torch.zeros(0, J, dtype=torch.bool), steps=2)
    assert e.shape == (0, J, 4) and de.shape == (0, 1)


@pytest.mark.parametrize("select", ["all", "best"])
def test_pose_completion_driver_on_a_hand(torch_cuda, select):
    torch = torch_cuda
    from posendf_amd.pose_completion import PoseCompletion, best_hypothesis
    parents, sd = sko.case_network(("hand", True), "softplus")
    J, K, n = len(parents), 3, 10
    net = cuda_model(torch, parents, "softplus", sd)
    driver = PoseCompletion(net, body_model=None, device="cuda:0")
    q = torch.from_numpy(sko.case_poses(("hand", True), n))
    q[3, 4] = float("nan")      # an unobserved joint may hold anything: it is filled
    obs = torch.from_numpy(sco.make_mask(n, J))
    obs[3, 4] = False
    res = driver.complete(q, obs, hypotheses=K, fill="random", select=select, generator=torch.Generator().manual_seed(3), steps=sco.STEPS,
                          renormalize="unit")
    out, dist, meshes = res[0].cpu(), res[1].cpu(), res[-1]
    assert out.shape == (n, K, J, 4) and dist.shape == (n, K) and meshes == {} and bool(torch.isfinite(dist).all())
    if select == "best":
        assert len(res) == 4 and torch.equal(res[2].cpu(), best_hypothesis(dist))
    else:
        assert len(res) == 3
    for k in range(K):      # observed joints: the input's, in every hypothesis
        assert torch.equal(out[:, k][obs], q[obs])
    assert not torch.equal(out[:, 0][~obs], out[:, 1][~obs])      # the hypotheses start apart
