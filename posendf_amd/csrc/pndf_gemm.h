// The 128 x 128 fp32 MFMA GEMM with its epilogues and the activation with its two derivatives, shared by the layer-by-layer
// units csrc/pndf_train.hip (the training objective), csrc/pndf_second_order.hip (Hessian-vector products of the distance) and
// csrc/pndf_skeleton.hip (the first order for any joint tree).  Device code in an unnamed namespace: every translation unit that
// includes it instantiates its own kernels from it under its own extern "C" names.  Host side, at the end: the one GEMM launcher
// over a unit's kernels, and the trunk's forward and first-order reverse as launch sequences over the plan of pndf_net_plan.h.
// The structure encoder of those units is in pndf_bone.h, which includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "../../include/posendf_amd.h"
#include "pndf_net_plan.h"

namespace {

constexpr float LRELU_SLOPE = 0.01f;       // nn.LeakyReLU()
constexpr float SP_THRESHOLD = 20.f;       // nn.Softplus(threshold=20)

// GEMM tiling: a 128 x 128 output tile per 256-thread workgroup, K steps of 16, each wave a 64 x 64 quarter as 4 x 4 blocks of
// the 16x16x4 fp32 MFMA.  LDS rows padded to 144 floats: the four k-rows one fragment read touches fall on distinct banks.
constexpr int TM = 128, TN = 128, TK = 16, LDS_LD = 144;

enum { EPI_STORE = 0, EPI_FWD = 1, EPI_TAN = 2, EPI_MUL = 3 };

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    int64_t lda, ldb, ldc;
    int M, N, K, kc;          // kc: K range of one blockIdx.z (split-K)
    int64_t slab;             // C offset per blockIdx.z
    int epi, act, out_layer;
    float beta;
    const float* bias;
    float* D1;                // sigma'(z)                     [M][ld1]
    float* D2;                // sigma'' (then sigma'' zdot)   [M][ld2], columns < nB only
    const float* X;           // EPI_MUL: cross term added on columns < nB
    int64_t ld1, ld2, ldx;
    int64_t nB;
    int64_t np_split;         // EPI_MUL: columns >= np_split read sigma' at (column - np_split)
};

__device__ __forceinline__ void act_eval(int act, float beta, bool out, float z, float& a, float& d1, float& d2) {
    if (act == PNDF_ACT_SOFTPLUS) {
        const float bz = beta * z;
        if (bz > SP_THRESHOLD) {
            a = z; d1 = 1.f; d2 = 0.f;
        } else {
            const float e = expf(bz);
            a = log1pf(e) / beta;
            const float s = e / (e + 1.f);
            d1 = s;
            d2 = beta * s * (1.f - s);
        }
    } else if (act == PNDF_ACT_RELU || out) {
        a = z > 0.f ? z : 0.f; d1 = z > 0.f ? 1.f : 0.f; d2 = 0.f;
    } else {
        a = z > 0.f ? z : LRELU_SLOPE * z; d1 = z > 0.f ? 1.f : LRELU_SLOPE; d2 = 0.f;
    }
}

// C(m, n) = sum_k A(m, k) B(k, n).  A_KC: A(m, k) = A[m lda + k] (else A[k lda + m]);  B_KC: B(k, n) = B[n ldb + k] (else
// B[k ldb + n]).  Every load outside [0, M) x [kbeg, kend) x [0, N) reads zero; every store is bounds checked.
template <int A_KC, int B_KC>
__device__ __forceinline__ void gemm_body(const GemmArgs& g) {
    __shared__ float As[TK][LDS_LD];
    __shared__ float Bs[TK][LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w & 1, wn = w >> 1;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int kbeg = blockIdx.z * g.kc;
    const int kend = min(g.K, kbeg + g.kc);
    float ra[8], rb[8];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int mm = A_KC ? (tid >> 4) + 16 * i : (tid & 127);
            const int ka = A_KC ? (tid & 15) : (tid >> 7) + 2 * i;
            const int m = m0 + mm, k = k0 + ka;
            ra[i] = (m < g.M && k < kend) ? (A_KC ? g.A[(int64_t)m * g.lda + k] : g.A[(int64_t)k * g.lda + m]) : 0.f;
            const int nn = B_KC ? (tid >> 4) + 16 * i : (tid & 127);
            const int kb = B_KC ? (tid & 15) : (tid >> 7) + 2 * i;
            const int n = n0 + nn, kk = k0 + kb;
            rb[i] = (n < g.N && kk < kend) ? (B_KC ? g.B[(int64_t)n * g.ldb + kk] : g.B[(int64_t)kk * g.ldb + n]) : 0.f;
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += TK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[A_KC ? (tid & 15) : (tid >> 7) + 2 * i][A_KC ? (tid >> 4) + 16 * i : (tid & 127)] = ra[i];
            Bs[B_KC ? (tid & 15) : (tid >> 7) + 2 * i][B_KC ? (tid >> 4) + 16 * i : (tid & 127)] = rb[i];
        }
        __syncthreads();
        if (k0 + TK < kend) load(k0 + TK);
#pragma unroll
        for (int s = 0; s < TK / 4; ++s) {
            float a[4], b[4];
            const int kr = s * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = As[kr][wm * 64 + i * 16 + (lane & 15)];
                b[i] = Bs[kr][wn * 64 + i * 16 + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float* C = g.C + (int64_t)blockIdx.z * g.slab;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                const int col = n0 + wn * 64 + j * 16 + (lane & 15);
                if (row >= g.M || col >= g.N) continue;
                const float v = acc[i][j][r];
                float* out = C + (int64_t)row * g.ldc + col;
                if (g.epi == EPI_STORE) {
                    *out = v;
                } else if (g.epi == EPI_FWD) {
                    float a, d1, d2;
                    act_eval(g.act, g.beta, g.out_layer != 0, v + g.bias[row], a, d1, d2);
                    *out = a;
                    g.D1[(int64_t)row * g.ld1 + col] = d1;
                    if (g.D2 && col < g.nB) g.D2[(int64_t)row * g.ld2 + col] = d2;
                } else if (g.epi == EPI_TAN) {      // tangent forward (v = zdot) and tangent reverse (v = adotbar)
                    *out = v * g.D1[(int64_t)row * g.ld1 + col];
                    if (g.D2) {
                        float* d2 = g.D2 + (int64_t)row * g.ld2 + col;
                        *d2 = v * *d2;
                    }
                } else {                            // EPI_MUL: v sigma' (+ the cross term); raw without sigma'
                    float o = v;
                    if (g.D1) o *= g.D1[(int64_t)row * g.ld1 + (col >= g.np_split ? col - g.np_split : col)];
                    if (g.X && col < g.nB) o += g.X[(int64_t)row * g.ldx + col];
                    *out = o;
                }
            }
}

inline GemmArgs gemm_args(const float* A, int64_t lda, const float* Bp, int64_t ldb, float* C, int64_t ldc, int M, int N, int K) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = Bp; g.ldb = ldb; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.kc = K;
    g.np_split = INT64_MAX;
    return g;
}

inline int64_t align64(int64_t x) { return (x + 63) / 64 * 64; }
inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------------------ host side
// a workspace or a weight blob carved into regions of floats, every region 256-byte aligned
struct Carver {
    int64_t o = 0;
    int64_t take(int64_t n) { const int64_t at = o; o += align64(n); return at; }
};

// A unit's own instances of gemm_body under its own extern "C" names (the profiles name them); nt: training alone has one.
struct GemmKernels {
    void (*nn)(GemmArgs);
    void (*tn)(GemmArgs);
    void (*nt)(GemmArgs);
};
enum { GEMM_NN, GEMM_TN, GEMM_NT };
inline void launch_gemm(const GemmKernels& k, int kind, const GemmArgs& g, int splits, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0) return;
    const dim3 grid((g.N + TN - 1) / TN, (g.M + TM - 1) / TM, splits);
    void (*kernel)(GemmArgs) = kind == GEMM_NN ? k.nn : kind == GEMM_TN ? k.tn : k.nt;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, g);
}

// trunk layer t: W[t] weight [dims[t+1]][dims[t]], b[t] bias
struct TrunkWeights {
    const float* W[PNDF_NET_MAX_LIN];
    const float* b[PNDF_NET_MAX_LIN];
};
// ... from a caller's tensor table, the trunk's 2 L tensors in state-dict order
inline TrunkWeights trunk_weights(const LayerNet& net, const float* const* tensors) {
    TrunkWeights w{};
    for (int t = 0; t < net.L; ++t) { w.W[t] = tensors[2 * t]; w.b[t] = tensors[2 * t + 1]; }
    return w;
}

// The buffers of one pass over the trunk for a chunk of n columns, every matrix [features][ld]
struct TrunkBuffers {
    const float* in;                   // the trunk's input [dims[0]][ld]
    float* P[2];                       // the ping-pong buffers every pass over the layers runs through [maxw][ld]
    float* D1[PNDF_NET_MAX_LIN];       // sigma' of layer t [dims[t+1]][ld]
    float* D2[PNDF_NET_MAX_LIN];       // null, or sigma'' of layer t, then what the tangent passes leave there (a dual trunk)
    float *out, *din;                  // the output row [ld]; the reverse's result, the adjoint of the input [dims[0]][ld]
    int64_t ld;
    int n;
};

// forward: layer t reads in / P[(t-1)&1] and writes P[t&1], epilogue bias + sigma with sigma' (and sigma'') kept; the output row
// goes to `out`
inline void trunk_forward(const GemmKernels& k, const LayerNet& net, const TrunkWeights& w, const TrunkBuffers& b, hipStream_t st) {
    const int L = net.L;
    for (int t = 0; t < L; ++t) {
        GemmArgs a = gemm_args(w.W[t], net.dims[t], t == 0 ? b.in : b.P[(t - 1) & 1], b.ld, t == L - 1 ? b.out : b.P[t & 1], b.ld,
                               net.dims[t + 1], b.n, net.dims[t]);
        a.epi = EPI_FWD; a.act = net.act; a.beta = net.beta; a.out_layer = t == L - 1; a.bias = w.b[t];
        a.D1 = b.D1[t]; a.ld1 = b.ld;
        if (b.D2[t]) { a.D2 = b.D2[t]; a.ld2 = b.ld; a.nB = b.n; }
        launch_gemm(k, GEMM_NN, a, 1, st);
    }
}

// The first-order reverse from sigma' of the output (the seed 1): layer t's input adjoint, * sigma' of layer t-1, down to `din`.
// In a dual trunk this is the adjoint chain of the tangent, and adotbar sigma'' zdot replaces sigma'' zdot in D2 on the way.
inline void trunk_reverse(const GemmKernels& k, const LayerNet& net, const TrunkWeights& w, const TrunkBuffers& b, hipStream_t st) {
    const float* U = b.D1[net.L - 1];
    for (int t = net.L - 1; t >= 0; --t) {
        float* o = t == 0 ? b.din : b.P[t & 1];
        GemmArgs a = gemm_args(w.W[t], net.dims[t], U, b.ld, o, b.ld, net.dims[t], b.n, net.dims[t + 1]);
        a.epi = (t > 0 && b.D2[t - 1]) ? EPI_TAN : EPI_MUL;
        if (t > 0) { a.D1 = b.D1[t - 1]; a.ld1 = b.ld; }
        if (a.epi == EPI_TAN) { a.D2 = b.D2[t - 1]; a.ld2 = b.ld; }
        launch_gemm(k, GEMM_TN, a, 1, st);
        U = o;
    }
}

}  // namespace
