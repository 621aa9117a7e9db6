// Exact k-nearest-pose search over a pose database (the search stage of the reference's data/prepare_traindata.py:152-159,
// with the whole database as every query's candidate list): for Q query poses [Q,J,4] and an index of N poses of J joints
// (1 .. 32, a property of the index: 21 for pndf_knn_create, any for pndf_skel_knn_create of
// include/posendf_amd_skeleton_data.h), the k smallest of
//   geo: sum_j w_j (1 - |<q_j, p_j>|)        euc: sum_j w_j ||q_j - p_j||_2
// (w_j = 1/J, or the caller's: the L2-normalised joint ranks of SMPL), the metric and semantics of pndf_quat_topk.
//
// Layout.  The index packs the database once into joint-major 16-pose tiles: tile t = J joints x 4 components x 16 poses
// (256 J bytes; 5,376 B at 21), element [t][j][c][m] = pose 16t+m, joint j, component c.  Poses past N are NaN, so their
// distance is NaN and never selected.  One joint of one tile is 64 consecutive floats: lane l of a wave loads element l, which
// is exactly the A operand A[m = l&15][c = l>>4] of v_mfma_f32_16x16x4_f32.
//
// The joint count in the kernels.  Every per-joint register array is sized by a compile-time bound JP and indexed by unrolled
// loops only; the kernels are instantiated for the width classes JP = 8, 16, 24, 32, where joint j of the unrolled sequence runs
// under the wave-uniform guard j < J (J a kernel argument), and for JP = 21, where J is the constant 21 and the guard folds
// away: the 21-joint instantiation is the expression sequence it was before the other joint counts existed.
//
// geo (MFMA).  A = 16 database poses (rows), B = 16 queries (columns) with w_j folded in; one MFMA per joint and query group
// gives the 16x16 block of w_j <q_j, p_j>.  Lane l holds column l&15 (one query) and rows 4(l>>4)+r (four poses), adds
// w_j - |d| per joint in joint order 0..J-1: a pair gets the same bits wherever it lands in the plan.  A wave owns 2 groups
// (32 queries), a workgroup of 4 waves 128 queries; the 4 waves read the same tile (L1 hits after the first).
// euc (VALU).  The direct-difference form sqrt(sum_c (q_c - p_c)^2), never the expansion |q|^2 + |p|^2 - 2<q,p> (which
// cancels for near-identical joints).  A lane owns one query; a workgroup of 128 stages 4 tiles in LDS and reads each pose
// as broadcast float4s.
//
// Selection.  Every lane keeps a sorted (value, index) list of KM = pow2 >= k entries per query in registers; a candidate
// that fails `value <= list[KM-1]` costs that one compare (NaN fails it).  Order: value ascending, then index: ties go to the
// lower index.  geo merges the 4 lanes that share a query with shuffles; each (query block, database split) workgroup writes
// one partial list per query to the caller's workspace, and pndf_knn_merge_kernel reduces the partial lists of a query in one
// wave.  The k smallest under a strict total order do not depend on how the database was split: results are bit-identical
// for every plan.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/posendf_amd.h"
#include "../../include/posendf_amd_skeleton_data.h"
#include "pndf_host.h"

struct pndf_knn_index {
    int device = -1;
    int64_t N = 0, T = 0;
    int32_t metric = 0;
    int32_t J = 21;
    float w[32];
    float* db = nullptr;
    std::string err;
};

namespace {
constexpr int MAX_J = 32, EXACT_J = 21, TILE = 16, QPB = 128, MAX_K = 16, EUC_CHUNK = 4;
constexpr int SENT = 0x7fffffff;                     // empty slot: sorts after every real index (N < 2^31)
constexpr int TARGET_WGS = 2048;                     // 8 workgroups per CU of a 256-CU part
constexpr int64_t MIN_TILES_PER_SPLIT = 16;
typedef float f4 __attribute__((ext_vector_type(4)));

struct KnnArgs {
    const float* db;     // packed tiles
    const float* q;      // [Q,J,4]
    float* pv;           // partial lists [S][Q][KM]
    int* pi;
    int64_t Q, T, tps, S, qb;
    int32_t J;
    float w[MAX_J];
};

// the joint count of an instantiation: the constant 21 in the exact one, the argument (<= JP) in a width class
template <int JP>
__device__ __forceinline__ int joint_count(const KnnArgs& a) { return JP == EXACT_J ? EXACT_J : a.J; }

struct MergeArgs {
    const float* pv;
    const int* pi;
    float* vals;
    long long* idx;
    int64_t Q, S;
    int k;
};

__device__ __forceinline__ bool before(float v, int i, float ov, int oi) { return v < ov || (v == ov && i < oi); }

template <int KM>
__device__ __forceinline__ void init_list(float (&lv)[KM], int (&li)[KM]) {
#pragma unroll
    for (int s = 0; s < KM; ++s) { lv[s] = __builtin_inff(); li[s] = SENT; }
}

// candidate (v, i) into the sorted list: replaces the last entry, then one bubble pass
template <int KM>
__device__ __forceinline__ void offer(float (&lv)[KM], int (&li)[KM], float v, int i) {
    if (!(v <= lv[KM - 1])) return;                  // the threshold test (NaN fails it)
    if (!before(v, i, lv[KM - 1], li[KM - 1])) return;
    lv[KM - 1] = v;
    li[KM - 1] = i;
#pragma unroll
    for (int s = KM - 1; s > 0; --s) {
        if (before(lv[s], li[s], lv[s - 1], li[s - 1])) {
            const float tv = lv[s]; lv[s] = lv[s - 1]; lv[s - 1] = tv;
            const int ti = li[s]; li[s] = li[s - 1]; li[s - 1] = ti;
        }
    }
}

// merges the lists of the lanes l ^ {off_lo .. 32} (powers of two): KM rounds of "smallest head wins, the winner pops";
// afterwards every lane of the group holds the merged list.  Real indices are unique across the group; lanes whose heads are
// empty all "win" and pop an empty slot, which changes nothing.  Uniform control flow only.
template <int KM>
__device__ __forceinline__ void merge_lanes(float (&lv)[KM], int (&li)[KM], int off_lo) {
    float rv[KM];
    int ri[KM];
#pragma unroll
    for (int r = 0; r < KM; ++r) {
        float v = lv[0];
        int i = li[0];
        for (int off = off_lo; off < 64; off <<= 1) {
            const float ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(i, off);
            if (before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        rv[r] = v;
        ri[r] = i;
        if (li[0] == i) {
#pragma unroll
            for (int s = 0; s + 1 < KM; ++s) { lv[s] = lv[s + 1]; li[s] = li[s + 1]; }
            lv[KM - 1] = __builtin_inff();
            li[KM - 1] = SENT;
        }
    }
#pragma unroll
    for (int r = 0; r < KM; ++r) { lv[r] = rv[r]; li[r] = ri[r]; }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) pndf_knn_pack_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                        int64_t N, int J, int64_t n_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out) return;
    const int tile_floats = J * 4 * TILE;
    const int64_t t = e / tile_floats;
    const int r = (int)(e - t * tile_floats);
    const int j = r >> 6, c = (r >> 4) & 3, m = r & 15;
    const int64_t n = t * TILE + m;
    dst[e] = n < N ? src[(n * J + j) * 4 + c] : __builtin_nanf("");
}

template <int JP, int KM>
__global__ void __launch_bounds__(256) pndf_knn_geo_kernel(KnnArgs a) {
    constexpr int G = 2;                              // query groups of 16 per wave
    const int J = joint_count<JP>(a), tile_floats = J * 4 * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int64_t split = blockIdx.x / a.qb, qblock = blockIdx.x - split * a.qb;
    float bq[G][JP];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t qi = qblock * QPB + wave * (16 * G) + g * 16 + col;
#pragma unroll
        for (int j = 0; j < JP; ++j) bq[g][j] = (j < J && qi < a.Q) ? a.w[j] * a.q[(qi * J + j) * 4 + kq] : 0.f;
    }
    float lv[G][KM];
    int li[G][KM];
#pragma unroll
    for (int g = 0; g < G; ++g) init_list<KM>(lv[g], li[g]);
    const int64_t t0 = split * a.tps, t1 = min(t0 + a.tps, a.T);
    const float* db = a.db + lane;
    float pa[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) pa[j] = j < J ? db[t0 * tile_floats + j * 64] : 0.f;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t tn = t + 1 < t1 ? t + 1 : t;   // the next tile's loads go out before this tile's MFMAs
        float pn[JP];
#pragma unroll
        for (int j = 0; j < JP; ++j) pn[j] = j < J ? db[tn * tile_floats + j * 64] : 0.f;
        f4 s[G];
#pragma unroll
        for (int g = 0; g < G; ++g) s[g] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < JP; ++j) {
            if (j < J) {                              // (wave-uniform; constant in the 21-joint instantiation)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const f4 d = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[j], bq[g][j], f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[g][r] += a.w[j] - fabsf(d[r]);
                }
            }
        }
        const int64_t base = t * TILE + 4 * kq;      // (padding poses are NaN: never taken)
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) offer<KM>(lv[g], li[g], s[g][r], (int)(base + r));
        }
#pragma unroll
        for (int j = 0; j < JP; ++j) pa[j] = pn[j];
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        merge_lanes<KM>(lv[g], li[g], 16);
        const int64_t qi = qblock * QPB + wave * (16 * G) + g * 16 + col;
        if (kq == 0 && qi < a.Q) {
            const int64_t o = (split * a.Q + qi) * KM;
#pragma unroll
            for (int r = 0; r < KM; ++r) { a.pv[o + r] = lv[g][r]; a.pi[o + r] = li[g][r]; }
        }
    }
}

template <int JP, int KM>
__global__ void __launch_bounds__(QPB) pndf_knn_euc_kernel(KnnArgs a) {
    __shared__ f4 sp[EUC_CHUNK * TILE][JP];           // 21,504 B at 21, 32 KB at 32
    const int tid = threadIdx.x;
    const int J = joint_count<JP>(a), tile_floats = J * 4 * TILE;
    const int64_t split = blockIdx.x / a.qb, qblock = blockIdx.x - split * a.qb;
    const int64_t qi = qblock * QPB + tid;
    f4 qq[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) qq[j] = (j < J && qi < a.Q) ? ((const f4*)a.q)[qi * J + j] : f4{0.f, 0.f, 0.f, 0.f};
    float lv[KM];
    int li[KM];
    init_list<KM>(lv, li);
    const int64_t t0 = split * a.tps, t1 = min(t0 + a.tps, a.T);
    for (int64_t t = t0; t < t1; t += EUC_CHUNK) {
        const int nt = (int)min((int64_t)EUC_CHUNK, t1 - t);
        __syncthreads();
        const float* src = a.db + t * tile_floats;
        for (int e = tid; e < nt * tile_floats; e += QPB) {
            const int tt = e / tile_floats, r = e - tt * tile_floats;
            const int j = r >> 6, c = (r >> 4) & 3, m = r & 15;
            ((float*)&sp[tt * TILE + m][j])[c] = src[e];
        }
        __syncthreads();
        const int64_t base = t * TILE;
        for (int p = 0; p < nt * TILE; ++p) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < JP; ++j) {
                if (j < J) {
                    const f4 v = sp[p][j], q = qq[j];
                    const float dx = q.x - v.x, dy = q.y - v.y, dz = q.z - v.z, dw = q.w - v.w;
                    s += sqrtf(dx * dx + dy * dy + dz * dz + dw * dw) * a.w[j];
                }
            }
            offer<KM>(lv, li, s, (int)(base + p));
        }
    }
    if (qi < a.Q) {
        const int64_t o = (split * a.Q + qi) * KM;
#pragma unroll
        for (int r = 0; r < KM; ++r) { a.pv[o + r] = lv[r]; a.pi[o + r] = li[r]; }
    }
}

// one wave per query: every lane offers its strided share of the S partial lists, then the 64 lanes merge
template <int KM>
__global__ void __launch_bounds__(256) pndf_knn_merge_kernel(MergeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= a.Q) return;                            // (uniform per wave)
    float lv[KM];
    int li[KM];
    init_list<KM>(lv, li);
    const int64_t n = a.S * KM;
    for (int64_t c = lane; c < n; c += 64) {
        const int64_t s = c / KM, r = c - s * KM;
        const int64_t o = (s * a.Q + qi) * KM + r;
        offer<KM>(lv, li, a.pv[o], a.pi[o]);
    }
    merge_lanes<KM>(lv, li, 1);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < KM; ++r) {
            if (r < a.k) {
                const bool found = li[r] != SENT;     // fewer than k finite distances: NaN / -1
                a.vals[qi * a.k + r] = found ? lv[r] : __builtin_nanf("");
                a.idx[qi * a.k + r] = found ? (long long)li[r] : -1ll;
            }
        }
    }
}

namespace {
struct Plan {
    int KM;
    int64_t qb, S, tps;
};

// depends on (Q, N, k) only: query blocks of 128 x database splits of whole tiles, about TARGET_WGS workgroups in all, at
// least MIN_TILES_PER_SPLIT tiles per split
Plan make_plan(int64_t Q, int64_t N, int k) {
    Plan p;
    p.KM = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
    const int64_t T = (N + TILE - 1) / TILE;
    p.qb = (Q + QPB - 1) / QPB;
    int64_t S = (TARGET_WGS + p.qb - 1) / p.qb;
    S = std::min(S, (T + MIN_TILES_PER_SPLIT - 1) / MIN_TILES_PER_SPLIT);
    S = std::max<int64_t>(S, 1);
    p.tps = (T + S - 1) / S;
    p.S = (T + p.tps - 1) / p.tps;
    return p;
}

int64_t workspace_bytes(int64_t Q, int64_t N, int k) {
    const Plan p = make_plan(Q, N, k);
    return p.S * Q * p.KM * 8;
}

template <int JP, int KM>
void launch_search(const pndf_knn_index* h, const KnnArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)(a.S * a.qb);
    if (h->metric == 0) hipLaunchKernelGGL((pndf_knn_geo_kernel<JP, KM>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pndf_knn_euc_kernel<JP, KM>), dim3(grid), dim3(QPB), 0, st, a);
}

// the instantiation of a joint count: 21 has its own, every other one the smallest width class that holds it
template <int KM>
void launch(const pndf_knn_index* h, const KnnArgs& a, const MergeArgs& m, hipStream_t st) {
    if (h->J == EXACT_J) launch_search<EXACT_J, KM>(h, a, st);
    else if (h->J <= 8) launch_search<8, KM>(h, a, st);
    else if (h->J <= 16) launch_search<16, KM>(h, a, st);
    else if (h->J <= 24) launch_search<24, KM>(h, a, st);
    else launch_search<MAX_J, KM>(h, a, st);
    hipLaunchKernelGGL(pndf_knn_merge_kernel<KM>, dim3((unsigned)((m.Q + 3) / 4)), dim3(256), 0, st, m);
}
}  // namespace

extern "C" const char* pndf_knn_last_error(pndf_knn_handle h) { return pndf_last_error_of(h); }

static int knn_create(pndf_knn_handle* out, const float* poses, int64_t N, int J, int32_t metric, const float* weights, void* stream) {
    if (!out) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (metric != 0 && metric != 1) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_UNSUPPORTED, "metric: 0 = geo or 1 = euc");
    if (N < 1) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "the index needs N >= 1 poses");
    if (N >= ((int64_t)1 << 31)) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_UNSUPPORTED, "N must be below 2^31");
    if (!poses) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "poses is null");
    if ((uintptr_t)poses & 15) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "poses must be 16-byte aligned");
    if (weights)
        for (int j = 0; j < J; ++j)
            if (!(weights[j] > 0.f) || !std::isfinite(weights[j]))
                return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "joint weights must be finite and > 0");
    const PndfDeviceCheck any = pndf_check_gfx950(PNDF_ANY_DEVICE, "the pose index");
    if (any.code != PNDF_OK) return pndf_fail<pndf_knn_index>(nullptr, any.code, any.text);
    const int device = pndf_pointer_device(poses);
    if (device < 0) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "poses is not device memory");
    const PndfDeviceCheck dev = pndf_check_gfx950(device, "the pose index");
    if (dev.code != PNDF_OK) return pndf_fail<pndf_knn_index>(nullptr, dev.code, dev.text);
    DeviceGuard guard(device);
    if (!guard.ok) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_HIP, "hipSetDevice failed");
    pndf_knn_index* h = new pndf_knn_index();
    h->device = device;
    h->N = N;
    h->T = (N + TILE - 1) / TILE;
    h->metric = metric;
    h->J = J;
    for (int j = 0; j < MAX_J; ++j) h->w[j] = j >= J ? 0.f : weights ? weights[j] : 1.0f / (float)J;
    const int64_t n_out = h->T * (J * 4 * TILE);
    if (hipMalloc((void**)&h->db, (size_t)n_out * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_HIP, "hipMalloc of the packed index (" + std::to_string(n_out * 4) + " B) failed");
    }
    hipLaunchKernelGGL(pndf_knn_pack_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, poses,
                       h->db, N, J, n_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);      // the caller may free or overwrite `poses` next
    if (e != hipSuccess) {
        const std::string msg = std::string("packing the index: ") + hipGetErrorString(e);
        (void)hipFree(h->db);
        delete h;
        return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_HIP, msg);
    }
    *out = h;
    return PNDF_OK;
}

extern "C" int pndf_knn_create(pndf_knn_handle* out, const float* poses, int64_t N, int32_t metric, const float* weights,
                               void* stream) {
    return knn_create(out, poses, N, EXACT_J, metric, weights, stream);
}

// include/posendf_amd_skeleton_data.h
extern "C" int pndf_skel_knn_create(pndf_knn_handle* out, const float* poses, int64_t N, int32_t num_joints, int32_t metric,
                                    const float* weights, void* stream) {
    if (num_joints < 1 || num_joints > MAX_J)         // (before any pointer is looked at, `out` among them)
        return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "num_joints must be in 1 .. 32, got " + std::to_string(num_joints));
    return knn_create(out, poses, N, num_joints, metric, weights, stream);
}

extern "C" int pndf_knn_destroy(pndf_knn_handle h) {
    if (!h) return PNDF_OK;
    {
        DeviceGuard guard(h->device);
        if (h->db) (void)hipFree(h->db);
    }
    delete h;
    return PNDF_OK;
}

extern "C" int64_t pndf_knn_size(pndf_knn_handle h) { return h ? h->N : -1; }

extern "C" int64_t pndf_knn_workspace_bytes(pndf_knn_handle h, int64_t Q, int32_t k) {
    if (!h || Q < 0 || k < 1 || k > MAX_K || k > h->N) return PNDF_ERR_BAD_ARG;
    return Q == 0 ? 0 : workspace_bytes(Q, h->N, k);
}

extern "C" int pndf_knn_search(pndf_knn_handle h, const float* q, int64_t Q, int32_t k, float* vals, long long* idx,
                               void* workspace, void* stream) {
    PndfRange range("pndf_knn_search");
    if (k < 1 || k > MAX_K) return pndf_fail(h, PNDF_ERR_BAD_ARG, "k must be in 1 .. 16, got " + std::to_string(k));
    if (Q < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "Q must be >= 0");
    if (((uintptr_t)q & 15) || ((uintptr_t)vals & 3) || ((uintptr_t)idx & 7) || ((uintptr_t)workspace & 15))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pointer: q and workspace 16 B, vals 4 B, idx 8 B");
    if (!h) return pndf_fail<pndf_knn_index>(nullptr, PNDF_ERR_BAD_ARG, "null index handle");
    if (k > h->N)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "k = " + std::to_string(k) + " exceeds the index size " + std::to_string(h->N));
    if (Q == 0) return PNDF_OK;
    if (!q || !vals || !idx || !workspace) return pndf_fail(h, PNDF_ERR_BAD_ARG, "q, vals, idx and workspace must be non-null");
    if (Q >= ((int64_t)1 << 31)) return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "Q must be below 2^31 per call");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    const Plan p = make_plan(Q, h->N, k);
    KnnArgs a;
    a.db = h->db; a.q = q;
    a.pv = (float*)workspace;
    a.pi = (int*)((char*)workspace + p.S * Q * p.KM * 4);
    a.Q = Q; a.T = h->T; a.tps = p.tps; a.S = p.S; a.qb = p.qb;
    a.J = h->J;
    for (int j = 0; j < MAX_J; ++j) a.w[j] = h->w[j];
    MergeArgs m;
    m.pv = a.pv; m.pi = a.pi; m.vals = vals; m.idx = idx; m.Q = Q; m.S = p.S; m.k = k;
    const hipStream_t st = (hipStream_t)stream;
    switch (p.KM) {
        case 1: launch<1>(h, a, m, st); break;
        case 2: launch<2>(h, a, m, st); break;
        case 4: launch<4>(h, a, m, st); break;
        case 8: launch<8>(h, a, m, st); break;
        default: launch<16>(h, a, m, st); break;
    }
    return pndf_check_launch(h, "pndf_knn_search");
}
