// The online sampler's expression for ONE joint quaternion of one pool pose (include/posendf_amd_online.h),
// written once for the device and the host: the kernel (pndf_online.hip) and the host twin (pndf_cpu.cpp, compiled without a
// device pass) both call these functions, which is why they agree bit for bit.  Integer work is exact; every floating-point
// operation is rounded to fp32 on its own, in the order written (contraction off in every body, the one fused operation is an
// explicit fmaf).  The header needs no HIP runtime header before it.
//   pndf_philox4x32_10      the counter-based generator: ten rounds, the key bumped by the Weyl constants between rounds
//   pndf_online_pick        block 0 of pose i: the source row and the sigma group
//   pndf_online_quat        block 1 + j of pose i: the four noise values of joint j, the step off the manifold, the unit norm
// and, host only, what both entry points refuse and the thresholds that pndf_online_shares makes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/posendf_amd_online.h"
#include "pndf_step.h"

PNDF_HD void pndf_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// block `block` of pool pose i
PNDF_HD void pndf_online_block(uint64_t seed, uint32_t draw, int64_t i, uint32_t block, uint32_t w[4]) {
    const uint32_t ctr[4] = {(uint32_t)((uint64_t)i & 0xffffffffu), (uint32_t)((uint64_t)i >> 32), block, draw};
    const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    pndf_philox4x32_10(ctr, key, w);
}

// The source row in [0, N) and the sigma group of pose i.  The group is the first g with w1 <= cum[g]: cum does not decrease
// and ends in 0xffffffff, so that is the number of thresholds below w1.  The loops run over all 16 slots with the count as a
// guard, so that a kernel reads the option struct with constant offsets only.
PNDF_HD void pndf_online_pick(const pndf_online_opts& o, int64_t i, int64_t N, int64_t* src, int32_t* group, float* sigma) {
    uint32_t w[4];
    pndf_online_block(o.seed, o.draw, i, 0u, w);
    *src = (int64_t)(((uint64_t)w[0] * (uint64_t)N) >> 32);
    int32_t g = 0;
#pragma unroll
    for (int c = 0; c < PNDF_ONLINE_MAX_SIGMA - 1; ++c) g += (c < o.n_sigma - 1 && w[1] > o.cum[c]) ? 1 : 0;
    float s = o.sigma[0];
#pragma unroll
    for (int c = 1; c < PNDF_ONLINE_MAX_SIGMA; ++c) s = (g >= c) ? o.sigma[c] : s;
    *group = g;
    *sigma = s;
}

// out = unit(Q + sigma n) for joint j of pose i; Q as it came where the squared norm is 0 or not finite
PNDF_HD void pndf_online_quat(uint64_t seed, uint32_t draw, int64_t i, int j, int noise, float sigma, const float* Q, float* out) {
#pragma clang fp contract(off)
    uint32_t w[4];
    pndf_online_block(seed, draw, i, 1u + (uint32_t)j, w);
    float x[4];
    for (int c = 0; c < 4; ++c) {
        const float u = (float)(w[c] >> 8) * 5.9604644775390625e-08f;      // 2^-24: exact, in [0, 1)
        const float n = noise ? 2.0f * u - 1.0f : u;                       // exact: 2 u has 24 bits, 2 u - 1 at most 24
        x[c] = fmaf(sigma, n, Q[c]);
    }
    const float s = pndf_quat_dot(x, x);
    const bool ok = s > 0.0f && s < INFINITY;                              // false for 0, inf and NaN
    const float r = sqrtf(s);
    for (int c = 0; c < 4; ++c) out[c] = ok ? x[c] / r : Q[c];
}

// ------------------------------------------------------------------ host only: the refusals, the thresholds
// (plain inline functions: host code in every translation unit)
// the grid of the kernel: one lane per joint quaternion, 256 lanes per block
constexpr int PNDF_ONLINE_MAX_JOINTS = 32;
inline int64_t pndf_online_max_count(int num_joints) { return ((int64_t)0x7fffffff * 256) / num_joints; }

// why a call of pndf_online_sample / pndf_online_sample_cpu (num_joints 21) or of their pndf_skel_ forms is refused, or nullptr;
// `vec_align`: the alignment of q and man_db.  The joint count is looked at before any pointer.
inline const char* pndf_online_check(const float* man_db, int64_t N, int num_joints, int64_t first, int64_t count, const pndf_online_opts* o, const float* q,
                                     const int64_t* src, const int32_t* group, uintptr_t vec_align) {
    if (num_joints < 1 || num_joints > PNDF_ONLINE_MAX_JOINTS) return "num_joints must be in 1 .. 32";
    if (N < 1 || N >= ((int64_t)1 << 31)) return "the manifold needs 1 <= N < 2^31 poses";
    if (count < 0 || first < 0) return "negative count or first";
    if (first > INT64_MAX - count) return "first + count is beyond int64";
    if (count > pndf_online_max_count(num_joints)) return "count is beyond the grid of the kernel";
    if (!o) return "opt is null";
    if (o->n_sigma < 1 || o->n_sigma > PNDF_ONLINE_MAX_SIGMA) return "n_sigma must be in 1 .. 16";
    for (int g = 0; g < o->n_sigma; ++g) {
        if (!(o->sigma[g] >= 0.0f && o->sigma[g] < INFINITY)) return "every sigma must be finite and >= 0";
        if (g && o->cum[g] < o->cum[g - 1]) return "cum must not decrease";
    }
    if (o->cum[o->n_sigma - 1] != 0xffffffffu) return "the last cum must be 0xffffffff";
    if (o->noise != PNDF_ONLINE_UNIFORM && o->noise != PNDF_ONLINE_SYMMETRIC) return "noise: 0 = uniform or 1 = symmetric";
    if (count == 0) return nullptr;      // a no-op: the pointers are not looked at
    if (!man_db || !q) return "man_db / q is null";
    if (((uintptr_t)man_db | (uintptr_t)q) & (vec_align - 1)) return vec_align == 16 ? "man_db and q must be 16-byte aligned" : "misaligned man_db or q";
    if (((uintptr_t)src & 7) || ((uintptr_t)group & 3)) return "misaligned src or group";
    return nullptr;
}

// cum[0 .. n) from n shares (see the header), or the reason of the refusal
inline const char* pndf_online_thresholds(int n, const float* shares, uint32_t* cum) {
    if (n < 1 || n > PNDF_ONLINE_MAX_SIGMA) return "n_sigma must be in 1 .. 16";
    if (!shares) return "shares is null";
    double total = 0.0;
    for (int g = 0; g < n; ++g) {
        if (!(shares[g] > 0.0f && shares[g] < INFINITY)) return "every share must be finite and > 0";
        total += (double)shares[g];
    }
    uint64_t count[PNDF_ONLINE_MAX_SIGMA], given = 0;
    double rest[PNDF_ONLINE_MAX_SIGMA];
    for (int g = 0; g < n; ++g) {
        const double ideal = (double)shares[g] / total * 4294967296.0;
        double whole = floor(ideal);
        if (whole > 4294967296.0) whole = 4294967296.0;
        count[g] = (uint64_t)whole;
        rest[g] = ideal - whole;
        given += count[g];
    }
    // the double arithmetic can leave the floors a few values short of (rarely beyond) 2^32: hand them out (take them back) by remainder
    while (given < 4294967296ull) {
        int best = 0;
        for (int g = 1; g < n; ++g)
            if (rest[g] > rest[best]) best = g;
        ++count[best], ++given;
        rest[best] -= 1.0;
    }
    while (given > 4294967296ull) {
        int best = -1;
        for (int g = 0; g < n; ++g)
            if (count[g] > 1 && (best < 0 || rest[g] < rest[best])) best = g;
        if (best < 0) return "shares too uneven for 32-bit thresholds";
        --count[best], --given;
        rest[best] += 1.0;
    }
    uint64_t acc = 0;
    for (int g = 0; g < n; ++g) {
        if (count[g] < 1) return "a share is too small to receive one of the 2^32 values of a word";
        acc += count[g];
        cum[g] = (uint32_t)(acc - 1);
    }
    return nullptr;
}
