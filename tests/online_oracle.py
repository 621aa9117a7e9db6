"""Test helper (not a test module) for the online sampler (include/posendf_amd_online.h, posendf_amd.online): a vectorised numpy
Philox4x32-10, a scalar pure-Python one to hold it to, and the sampler restated in numpy -- words and integers exact, the pose
arithmetic in fp64 and rounded to fp32 at the end.  Written from the description of the stream, not from
the C++."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# counter, key -> output (the known answers of the Philox4x32-10 reference implementation)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

DEFAULT_SIGMAS = (0.01, 0.05, 0.1, 0.25, 0.5)


def philox_scalar(ctr, key):
    """one block with Python integers: (c0, c1, c2, c3), (k0, k1) -> four words"""
    c0, c1, c2, c3 = (int(c) for c in ctr)
    k0, k1 = (int(k) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other) of unsigned words -> [..., 4] uint32"""
    ctr = np.asarray(ctr, np.uint64)
    key = np.asarray(key, np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., n], shape).copy() for n in range(4)]
    k = [np.broadcast_to(key[..., n], shape).copy() for n in range(2)]
    m = np.uint64(MASK)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]        # < 2^64: both factors are below 2^32
        c = [(p1 >> s) ^ c[1] ^ k[0], p1 & m, (p0 >> s) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + np.uint64(W0)) & m, (k[1] + np.uint64(W1)) & m]
    return np.stack(c, axis=-1).astype(np.uint32)


def blocks(seed, draw, index, block):
    """the words of `block` (an int or an array broadcast against `index`) of the pool poses `index` (int64 array)"""
    index, block = np.broadcast_arrays(np.asarray(index, np.int64).astype(np.uint64), np.asarray(block, np.uint64))
    ctr = np.stack([index & np.uint64(MASK), index >> np.uint64(32), block, np.full(index.shape, int(draw) & MASK, np.uint64)], axis=-1)
    key = np.array([int(seed) & MASK, (int(seed) >> 32) & MASK], np.uint64)
    return philox(ctr, key)


def picks(N, first, count, seed, draw, cum):
    """-> (src int64 [count], group int32 [count]) of pool poses first .. first + count - 1"""
    idx = np.int64(first) + np.arange(count, dtype=np.int64)
    w = blocks(seed, draw, idx, 0).astype(np.uint64)
    src = ((w[:, 0] * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    group = np.searchsorted(np.asarray(cum, np.uint64), w[:, 1], side="left").astype(np.int32)      # the first g with w1 <= cum[g]
    return src, group


def sample(man, first, count, seed, draw, sigmas, cum, noise):
    """-> (q float32 [count,21,4], src, group): the sampler in fp64, rounded once at the end.  `noise`: 0 uniform, 1 symmetric"""
    man = np.asarray(man, np.float32)
    src, group = picks(len(man), first, count, seed, draw, cum)
    idx = np.int64(first) + np.arange(count, dtype=np.int64)
    w = blocks(seed, draw, idx[:, None], 1 + np.arange(21)[None, :])                 # [count, 21, 4]
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    n = 2.0 * u - 1.0 if noise else u
    sig = np.asarray(sigmas, np.float32).astype(np.float64)[group]                  # the options hold fp32 sigmas
    Q = man[src].astype(np.float64)
    x = Q + sig[:, None, None] * n
    s = (x * x).sum(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((s > 0) & np.isfinite(s), x / np.sqrt(s), Q)
    return out.astype(np.float32), src, group


# ---- shared by tests/test_online.py and tests/test_online_gpu.py ---------------------------------------------------------------
POSE_TOL = 5e-7      # |kernel or twin - fp64 oracle| per component: components are at most 1 in magnitude; one fma, four products, three
#                      sums, one sqrt and one divide each round at 2^-24 relative: at most 8 * 2^-24 = 4.8e-7
UNIT_TOL = 2e-7      # | |q| - 1 | of every output quaternion
SIZES_N = (1, 3, 1000)
COUNTS = (1, 63, 64, 65, 1000)
FIRSTS = (0, 5, 2 ** 32 - 3)      # the last: the high counter word becomes non-zero inside a 7-pose call
N_SIGMAS = (1, 5, 16)


def case_options(n_sigma, noise, seed, draw):
    """engine.OnlineOpts of a test case: 1, 5 (the defaults) or 16 sigma groups with seeded unequal shares"""
    from posendf_amd import engine
    if n_sigma == 5:
        sigmas, shares = DEFAULT_SIGMAS, (0.2,) * 5
    else:
        rng = np.random.default_rng([n_sigma, 3])
        sigmas, shares = np.linspace(0.01, 0.5, n_sigma), rng.uniform(0.5, 2.0, n_sigma)
    return engine.online_opts(sigmas, shares, ("uniform", "symmetric")[noise], seed, draw)


def oracle_of(man, first, count, opt):
    n = opt.n_sigma
    return sample(man, first, count, opt.seed, opt.draw, list(opt.sigma[:n]), list(opt.cum[:n]), opt.noise)


def manifold(N, seed=21):
    from posendf_amd import synth
    return synth.make_poses(N, seed=seed, signed=True)


def write_manifold(root, rows=(200, 100), seed=31):
    """<root>/manifold/setA/man*.npz with seeded unit poses: the amass_dir of the trainer tests; -> (amass_dir, list of arrays)"""
    import os
    amass_dir = os.path.join(str(root), "manifold")
    os.makedirs(os.path.join(amass_dir, "setA"), exist_ok=True)
    mans = [manifold(n, seed + i) for i, n in enumerate(rows)]
    for i, p in enumerate(mans):
        np.savez(os.path.join(amass_dir, "setA", f"man{i:03d}.npz"), pose=p)
    return amass_dir, mans


def online_config(root, device, files, rows, num_pts, refresh_every=1, batch_size=2, continue_train=False, online=None, **kw):
    """trainer_fixtures.config with `data.online` over <root>/manifold (write_manifold) and no data_dir"""
    import os
    import trainer_fixtures as trf
    cfg = trf.config(root, device=device, batch_size=batch_size, num_pts=num_pts, continue_train=continue_train, **kw)
    cfg["data"] = {"amass_dir": os.path.join(str(root), "manifold"), "flip": False, "num_pts": num_pts,
                   "online": dict({"files": files, "rows": rows, "refresh_every": refresh_every}, **(online or {}))}
    return cfg
