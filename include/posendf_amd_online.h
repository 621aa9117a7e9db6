/* posendf_amd_online.h -- online training data: noisy poses drawn from a pose manifold on the device, counter-based.
 *
 * Companion of posendf_amd.h (same library).  A pool of noisy poses is a pure function of (seed, draw, options, man_db): pose i
 * of the pool takes a manifold row, a sigma group and 84 noise values from Philox4x32-10 blocks whose counter names the pose,
 * so any part of a pool can be produced by any call, in any order, and holds the same bits.  pndf_knn_search then labels the
 * pool with its exact distances to the manifold (posendf_amd/online.py).  DESIGN.md section 2n.
 *
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key
 * (seed & 0xffffffff, seed >> 32), counter (i & 0xffffffff, i >> 32, block, draw) for pool index i.
 *   block 0      word 0: source row  src = (uint64) w0 * N >> 32  (bias below N / 2^32)
 *                word 1: sigma group = the first g with w1 <= cum[g]
 *   block 1 + j  the four noise words of joint j:  u = (w >> 8) * 2^-24 in [0, 1);
 *                noise 0 (PNDF_ONLINE_UNIFORM): n = u, the reference's np.random.rand (data/create_data.py:89, biased towards +);
 *                noise 1 (PNDF_ONLINE_SYMMETRIC): n = 2 u - 1
 * The pose, per joint quaternion Q of row src: x_c = fma(sigma[group], n_c, Q_c), s = ((x0 x0 + x1 x1) + x2 x2) + x3 x3 (every
 * operation rounded to fp32 on its own), out = x / sqrt(s); where s is 0 or not finite, out = Q.  A NaN row gives a NaN pose.
 * The noise is drawn per pose and per component: create_data.py:89 shares one rand(21, 4) across a whole sigma group.
 *
 * Conventions: those of posendf_amd.h -- contiguous fp32, poses [.., 21, 4]; q and man_db 16-byte aligned DEVICE pointers, src
 * 8-byte and group 4-byte aligned (the host twin: HOST pointers, naturally aligned); work is enqueued on `stream` (a hipStream_t
 * passed as void*; NULL = the default stream) and the call returns without synchronising, allocating or freeing anything; it
 * runs on the device of `q` and restores the caller's current device; return value 0 on success, a negative pndf_status
 * otherwise.  There is no handle: the text of a refusal is left in the calling thread's slot, pndf_last_error(NULL) for
 * pndf_online_sample and pndf_cpu_last_error(NULL) for the three host functions.
 *
 * Poses of another joint count than 21: pndf_skel_online_sample / pndf_skel_online_sample_cpu of posendf_amd_skeleton_data.h.
 */
#ifndef POSENDF_AMD_ONLINE_H
#define POSENDF_AMD_ONLINE_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum pndf_online_noise { PNDF_ONLINE_UNIFORM = 0, PNDF_ONLINE_SYMMETRIC = 1 };

#define PNDF_ONLINE_MAX_SIGMA 16

/* seed and draw (the generation of the pool) select the stream; n_sigma groups in 1 .. 16, each with its noise scale sigma[g]
 * (finite, >= 0) and its cumulative threshold cum[g] (non-decreasing, cum[n_sigma - 1] == 0xffffffff): group g is drawn with
 * probability (cum[g] - cum[g - 1]) / 2^32.  Entries from n_sigma on are ignored. */
typedef struct pndf_online_opts {
    uint64_t seed; uint32_t draw; int32_t noise; int32_t n_sigma;
    float sigma[16]; uint32_t cum[16];
} pndf_online_opts;

/* data/create_data.py:51-52: sigma 0.01, 0.05, 0.1, 0.25, 0.5 with equal shares, uniform noise, seed 0, draw 0 */
int pndf_online_default_opts(pndf_online_opts* opt);

/* Host: opt->cum from opt->n_sigma shares (finite, > 0; they need not sum to 1).  The 2^32 values of a word are divided among
 * the groups by the largest-remainder rule (ties to the lower group) and cum[g] = the values of groups 0 .. g, minus 1, so the
 * last threshold is 2^32 - 1.  PNDF_ERR_BAD_ARG for a null pointer, n_sigma outside 1 .. 16, a share that is not finite and
 * > 0 or that is too small to receive one value of 2^32. */
int pndf_online_shares(pndf_online_opts* opt, const float* shares);

/* q [count,21,4] <- poses first .. first + count - 1 of the pool over man_db [N,21,4]; src [count] (may be NULL) <- their
 * source rows, group [count] (may be NULL) <- their sigma groups.  The bits of pose i depend on (seed, draw, i, the options,
 * man_db) only.  One launch.  PNDF_ERR_BAD_ARG with nothing launched for N < 1 or N >= 2^31, a negative count or first (or
 * first + count beyond int64, or a count beyond the grid of the kernel), n_sigma outside 1 .. 16, a sigma that is negative or
 * not finite, a cum that decreases or does not end in 0xffffffff, a noise that is not a pndf_online_noise, a null or misaligned
 * pointer, a q that is not device memory; count == 0 is a no-op; PNDF_ERR_NO_DEVICE without a HIP device. */
int pndf_online_sample(const float* man_db, int64_t N, int64_t first, int64_t count, const pndf_online_opts* opt, float* q,
                       int64_t* src /* may be NULL */, int32_t* group /* may be NULL */, void* stream);

/* Host twin (HOST pointers, no stream): the same expression, the same bits. */
int pndf_online_sample_cpu(const float* man_db, int64_t N, int64_t first, int64_t count, const pndf_online_opts* opt, float* q,
                           int64_t* src, int32_t* group);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_ONLINE_H */
