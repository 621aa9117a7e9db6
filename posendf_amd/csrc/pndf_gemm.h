// The 128 x 128 fp32 MFMA GEMM with its epilogues and the activation with its two derivatives, shared by the layer-by-layer
// units csrc/pndf_train.hip (the training objective) and csrc/pndf_second_order.hip (Hessian-vector products of the distance).
// The structure encoder and the network plan of those units are in pndf_bone.h, which includes this header.  Device code in an
// unnamed namespace: every translation unit that includes it instantiates its own kernels from it under its own extern "C" names.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "../../include/posendf_amd.h"

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

}  // namespace
