// PoseNDF's training objective and its weight gradients on gfx950 (model/posendf.py:62-99, the train=True branch that
// model/train_posendf.py:87-96 runs every step).
//
// Layer by layer over the whole batch, activations in HBM: the weight gradients are reductions over every pose, which a
// persistent per-pose kernel cannot hold.  Every activation matrix is [features][columns] (the pose index contiguous) with the
// columns ordered  [ noisy primal (B) | manifold primal (Bm) | noisy tangent (B) ].
//   forward : encoder (noisy: x = normalize(q, dim=1); manifold: raw q) -> NN GEMMs over the B + Bm primal columns, epilogue
//             bias + sigma, stores a, sigma' and (softplus) sigma'';  the losses.
//   eikonal : input gradient of the noisy batch (TN GEMMs, epilogue * sigma'), encoder backward, G = J_N^T g_x, the seed
//             Gbar = (2 / JB)(|G_j| - 1) G_j / |G_j|, xdot = J_N Gbar, tangent encoder, tangent NN GEMMs (no bias, epilogue
//             * sigma'; softplus: sigma'' zdot kept for the reverse).
//   backward: one reverse pass over the dual network.  Seeds on the output, then per layer  Wbar = [zbar|zdotbar][a|adot]^T
//             (NT GEMM, K split in a fixed way, partial slabs, a second launch sums them in order), bbar = row sums over the
//             primal columns, [abar|adotbar] = W^T [zbar|zdotbar] (TN GEMM) with zbar = abar sigma' + adotbar zdot sigma''
//             and zdotbar = adotbar sigma' in the epilogue; the J bone MLPs of the encoder last, lanes owning poses, their
//             weight gradients summed per workgroup (fixed order) and then over workgroups (fixed order).
// Shared with pndf_second_order.hip and pndf_skeleton.hip: the GEMM, its epilogues, the activation and the launcher (pndf_gemm.h);
// the dual-number bone ("The dual-number bone") and the pieces of the normalisation (pndf_bone.h); the
// host's description of the network, LayerNet (pndf_net_plan.h).  Here: the encoder's kernels around the bone with the LDS
// reduction of its weight gradient, the eikonal seed, the losses, the reverse's seeds and sums, and this unit's own launch
// sequences: column ranges of one [primal | tangent] matrix per layer, two leading dimensions, no ping-pong.
// Arithmetic: exact fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 accumulate.  No float atomics, no communication between
// workgroups inside a launch: two calls with the same inputs give the same bits.
// The skeleton is a run-time value (include/posendf_amd_skeleton_train.h): J = 1 .. 32 joints, the parent table and every bone's
// offset in the packed encoder from the plan.  A parent's features and adjoints are read back from the [6 J][ld] matrices, never
// from a per-thread array indexed by the parent, so the encoder kernels use no scratch memory.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <string>
#include <unordered_map>

#include "../../include/posendf_amd_skeleton_train.h"
#include "pndf_experiment.h"
#include "pndf_bone.h"
#include "pndf_host.h"

PNDF_EXPORT_EXPERIMENT_WORD(train)

namespace {

constexpr int SPLIT_TARGET_WGS = 1024;     // split-K target of the weight-gradient GEMM: a constant, never the device's occupancy
constexpr int ENC_WG = 192;                // poses per workgroup of the encoder's dual reverse (>= 176, the largest bone)
constexpr int ENC_VEC = 72;                // per-pose vectors the encoder's reduction reads from LDS
constexpr int ENC_LDS_LD = ENC_WG + 1;

enum { LOSS_L1 = 0, LOSS_L2 = 1 };

using EncTable = PtrTableOf<MAX_ENC_TENSORS>;      // the encoder's tensors of up to 32 joints; 4 J of them live

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pndf_train_gemm_nn_kernel(GemmArgs g) { gemm_body<1, 0>(g); }
extern "C" __global__ void __launch_bounds__(256) pndf_train_gemm_tn_kernel(GemmArgs g) { gemm_body<0, 0>(g); }
extern "C" __global__ void __launch_bounds__(256) pndf_train_gemm_nt_kernel(GemmArgs g) { gemm_body<1, 1>(g); }

namespace {

// ---- encoder: J bone MLPs (pndf_bone.h), the weights packed in state-dict order into one flat array
struct EncArgs {
    const float* wenc;        // packed encoder weights
    const float* q;           // noisy poses [B][4 J]
    const float* qm;          // manifold poses [Bm][4 J]
    const float* dgt;         // labels [B]
    float* X;                 // network input per primal column [4 J][np]: normalised noisy poses, raw manifold poses
    float* dgt_copy;          // [B]
    float* act0;              // encoder output [6 J][ncols]
    float* U0;                // d dist / d act0 of the noisy columns [6 J][B]
    float* Xd;                // x gradient, then Gbar, then xdot [4 J][B]
    float* eikp;              // per pose: sum_j (|G_j| - 1)^2 [B]
    float* abar;              // adjoint of act0 [6 J][ncols] (backward: accumulated in place)
    float* part;              // per-workgroup encoder weight-gradient partials [wgs][n_params]
    int64_t B, Bm, np, ncols;
    int act, eik, n_params, nj;
    float beta;
    int parent[MAXJ];
    int off[MAXJ];
};

// bone j's input on primal column c (X and the parent's rows of act0), and its tangent on noisy column c (xdot in Xd and the
// parent's rows of act0's tangent columns)
template <int FIN>
__device__ __forceinline__ void load_in(const EncArgs& e, int j, int64_t c, float* in) {
    bone_load<FIN>(e.X, e.np, e.act0, e.ncols, e.parent, j, c, in);
}
template <int FIN>
__device__ __forceinline__ void load_in_tan(const EncArgs& e, int j, int64_t c, float* ind) {
    bone_load<FIN>(e.Xd, e.B, e.act0 + e.np, e.ncols, e.parent, j, c, ind);
}

template <int FIN>
__device__ __forceinline__ void enc_fwd_bone(const EncArgs& e, int j, int64_t c) {
    float in[FIN];
    BoneDual b;
    load_in<FIN>(e, j, c, in);
    bone_fwd<FIN>(e, e.wenc + e.off[j], in, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) e.act0[(int64_t)(j * FEAT + i) * e.ncols + c] = b.ao[i];
}

// first-order reverse of one bone (input gradient of the noisy batch): the gradient on act0's rows of bone j (U0) -> the x
// gradient (Xd) and the parent's feature gradient (accumulated into U0).  The dual reverse without its primal chain.
template <int FIN>
__device__ __forceinline__ void enc_grad_bone(const EncArgs& e, int j, int64_t c) {
    const float* w = e.wenc + e.off[j];
    float in[FIN], adb[FEAT];
    BoneDual b;
    BoneAdj r;
    load_in<FIN>(e, j, c, in);
    bone_fwd<FIN>(e, w, in, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) adb[i] = e.U0[(int64_t)(j * FEAT + i) * e.B + c];
    bone_dual_rev<FIN, false>(w, b, nullptr, adb, r);
#pragma unroll
    for (int m = 0; m < FIN; ++m) {
        float s, sd;
        bone_input_adj<FIN, false>(w, r, m, s, sd);
        if (m < BONE) e.Xd[(int64_t)(j * BONE + m) * e.B + c] = sd;
        else e.U0[(int64_t)(e.parent[j] * FEAT + (m - BONE)) * e.B + c] += sd;
    }
}

// tangent forward of one bone along xdot
template <int FIN>
__device__ __forceinline__ void enc_tan_bone(const EncArgs& e, int j, int64_t c) {
    const float* w = e.wenc + e.off[j];
    float in[FIN], ind[FIN];
    BoneDual b;
    load_in<FIN>(e, j, c, in);
    load_in_tan<FIN>(e, j, c, ind);
    bone_fwd<FIN>(e, w, in, b);
    bone_tan<FIN>(w, ind, true, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) e.act0[(int64_t)(j * FEAT + i) * e.ncols + e.np + c] = b.oz[i] * b.d1o[i];
}

// dual reverse of one bone for one pose: the primal and tangent adjoints of the bone's output (abar, in place) -> the parent's,
// and the per-pose vectors whose outer products make the bone's weight gradient (to LDS, column `lane`; zeros on an idle lane)
template <int FIN>
__device__ __forceinline__ void enc_rev_bone(const EncArgs& e, int j, int64_t c, bool active, bool tangent,
                                             float (*sv)[ENC_LDS_LD], int lane) {
    float in[HID] = {}, ind[HID] = {};
    BoneDual b = {};
    BoneAdj r = {};
    if (active) {
        const float* w = e.wenc + e.off[j];
        const int64_t tc = e.np + c;
        load_in<FIN>(e, j, c, in);
        if (tangent) load_in_tan<FIN>(e, j, c, ind);
        bone_fwd<FIN>(e, w, in, b);
        bone_tan<FIN>(w, ind, true, b);      // a lane without a tangent runs it on ind = 0: a per-lane branch here spills 42 VGPRs
        float ab[FEAT], adb[FEAT];
#pragma unroll
        for (int i = 0; i < FEAT; ++i) {
            ab[i] = e.abar[(int64_t)(j * FEAT + i) * e.ncols + c];
            adb[i] = tangent ? e.abar[(int64_t)(j * FEAT + i) * e.ncols + tc] : 0.f;
        }
        bone_dual_rev<FIN, true, 0x20>(w, b, ab, adb, r);      // 0x20: this unit's rounding of zob (pndf_bone.h)
        if (FIN > BONE) {
            const int p = e.parent[j];
#pragma unroll
            for (int m = BONE; m < FIN; ++m) {      // the parent's adjoints; the weight gradient does not need those of x
                float s, sd;
                bone_input_adj<FIN, true>(w, r, m, s, sd);
                e.abar[(int64_t)(p * FEAT + (m - BONE)) * e.ncols + c] += s;
                if (tangent) e.abar[(int64_t)(p * FEAT + (m - BONE)) * e.ncols + tc] += sd;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < HID; ++k) {
        sv[k][lane] = in[k];
        sv[10 + k][lane] = ind[k];
        sv[20 + k][lane] = r.zhb[k];
        sv[30 + k][lane] = r.zhdb[k];
        sv[40 + k][lane] = b.ah[k];
        sv[50 + k][lane] = b.ahd[k];
    }
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        sv[60 + i][lane] = r.zob[i];
        sv[66 + i][lane] = r.zodb[i];
    }
}

// parameter t of a bone (state-dict order inside the bone), summed over the workgroup's poses in order
template <int FIN>
__device__ __forceinline__ float enc_param_sum(float (*sv)[ENC_LDS_LD], int t) {
    float s = 0.f;
    if (t < HID * FIN) {
        const int i = t / FIN, k = t % FIN;
        for (int l = 0; l < ENC_WG; ++l) s = fmaf(sv[30 + i][l], sv[10 + k][l], fmaf(sv[20 + i][l], sv[k][l], s));
    } else if (t < HID * FIN + HID) {
        const int i = t - HID * FIN;
        for (int l = 0; l < ENC_WG; ++l) s += sv[20 + i][l];
    } else if (t < HID * FIN + HID + FEAT * HID) {
        const int u = t - HID * FIN - HID, i = u / HID, k = u % HID;
        for (int l = 0; l < ENC_WG; ++l) s = fmaf(sv[66 + i][l], sv[50 + k][l], fmaf(sv[60 + i][l], sv[40 + k][l], s));
    } else {
        const int i = t - HID * FIN - HID - FEAT * HID;
        for (int l = 0; l < ENC_WG; ++l) s += sv[60 + i][l];
    }
    return s;
}

}  // namespace

// encoder forward over the primal columns; the noisy ones normalised over the joint axis first (F.normalize(q, dim=1))
extern "C" __global__ void __launch_bounds__(256) pndf_train_enc_fwd_kernel(EncArgs e) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.np) return;
    const int nq = e.nj * BONE;
    if (c < e.B) {
        const float* q = e.q + c * nq;
        float nrm[BONE];
        pose_col_norms(q, e.nj, nrm);
        for (int j = 0; j < e.nj; ++j)
#pragma unroll
            for (int k = 0; k < BONE; ++k) e.X[(int64_t)(j * BONE + k) * e.np + c] = norm_x(q[j * BONE + k], nrm[k]);
        e.dgt_copy[c] = e.dgt[c];
    } else {
        const float* q = e.qm + (c - e.B) * nq;
        for (int f = 0; f < nq; ++f) e.X[(int64_t)f * e.np + c] = q[f];
    }
    for (int j = 0; j < e.nj; ++j) {
        if (e.parent[j] < 0) enc_fwd_bone<BONE>(e, j, c);
        else enc_fwd_bone<BONE + FEAT>(e, j, c);
    }
}

// noisy columns: encoder backward of the input gradient, G = J_N^T g_x, the eikonal partial sums and seed, xdot = J_N Gbar, and
// the tangent encoder forward into act0's tangent columns
extern "C" __global__ void __launch_bounds__(256) pndf_train_enc_eik_kernel(EncArgs e) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.B) return;
    for (int j = e.nj - 1; j >= 0; --j) {
        if (e.parent[j] < 0) enc_grad_bone<BONE>(e, j, c);
        else enc_grad_bone<BONE + FEAT>(e, j, c);
    }
    const float* q = e.q + c * (e.nj * BONE);
    float nrm[BONE], s[BONE] = {0.f, 0.f, 0.f, 0.f};
    bool live[BONE];
    pose_col_norms(q, e.nj, nrm);
#pragma unroll
    for (int k = 0; k < BONE; ++k) live[k] = nrm[k] >= NORM_EPS;
    for (int j = 0; j < e.nj; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) s[k] = fmaf(e.X[(int64_t)(j * BONE + k) * e.np + c], e.Xd[(int64_t)(j * BONE + k) * e.B + c], s[k]);
    const float coef = 2.f / ((float)e.nj * (float)e.B);
    float eik = 0.f, t[BONE] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < e.nj; ++j) {
        float G[BONE], x[BONE], n2 = 0.f;
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            x[k] = e.X[(int64_t)(j * BONE + k) * e.np + c];
            const float gx = e.Xd[(int64_t)(j * BONE + k) * e.B + c];
            G[k] = norm_jvp(gx, x[k], s[k], nrm[k], live[k]);
            n2 = fmaf(G[k], G[k], n2);
        }
        const float n = sqrtf(n2);
        eik = fmaf(n - 1.f, n - 1.f, eik);
        const float f = n > 0.f ? coef * (n - 1.f) / n : 0.f;
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const float gb = f * G[k];
            e.Xd[(int64_t)(j * BONE + k) * e.B + c] = gb;
            t[k] = fmaf(x[k], gb, t[k]);
        }
    }
    e.eikp[c] = eik;
    for (int j = 0; j < e.nj; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            float* p = e.Xd + (int64_t)(j * BONE + k) * e.B + c;
            const float x = e.X[(int64_t)(j * BONE + k) * e.np + c];
            *p = norm_jvp(*p, x, t[k], nrm[k], live[k]);
        }
    for (int j = 0; j < e.nj; ++j) {
        if (e.parent[j] < 0) enc_tan_bone<BONE>(e, j, c);
        else enc_tan_bone<BONE + FEAT>(e, j, c);
    }
}

// dual reverse of the encoder: lanes own poses (the noisy ones, and the manifold ones when the eikonal term is on); per bone
// the workgroup's weight-gradient partial sums go to `part` (one row per workgroup)
extern "C" __global__ void __launch_bounds__(ENC_WG) pndf_train_enc_rev_kernel(EncArgs e) {
    __shared__ float sv[ENC_VEC][ENC_LDS_LD];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * ENC_WG + lane;
    const int64_t P = e.eik ? e.np : e.B;
    const bool active = c < P, tangent = e.eik && c < e.B;
    float* part = e.part + (int64_t)blockIdx.x * e.n_params;
    for (int j = e.nj - 1; j >= 0; --j) {
        const bool root = e.parent[j] < 0;
        if (root) enc_rev_bone<BONE>(e, j, c, active, tangent, sv, lane);
        else enc_rev_bone<BONE + FEAT>(e, j, c, active, tangent, sv, lane);
        __syncthreads();
        const int size = root ? HID * BONE + HID + FEAT * HID + FEAT : HID * (BONE + FEAT) + HID + FEAT * HID + FEAT;
        if (lane < size) part[e.off[j] + lane] = root ? enc_param_sum<BONE>(sv, lane) : enc_param_sum<BONE + FEAT>(sv, lane);
        __syncthreads();
    }
}

// the caller's 4 J encoder tensors (nt of them) -> one flat array
extern "C" __global__ void __launch_bounds__(256) pndf_train_enc_pack_kernel(EncTable t, int nt, float* dst) {
    enc_pack_body(t, nt, dst);
}

// per-workgroup partials -> the caller's 4 J encoder gradient tensors, summed over workgroups in order
extern "C" __global__ void __launch_bounds__(256) pndf_train_enc_reduce_kernel(EncTable t, int nt, const float* part, int wgs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t.off[nt];
    if (i >= n) return;
    float s = 0.f;
    for (int w = 0; w < wgs; ++w) s += part[(int64_t)w * n + i];
    int k = 0;
    while (t.off[k + 1] <= i) ++k;
    t.p[k][i - t.off[k]] = s;
}

// split-K slabs -> the weight gradient, summed over the slabs in order
extern "C" __global__ void __launch_bounds__(256) pndf_train_slab_reduce_kernel(const float* slab, int S, int64_t n, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int z = 0; z < S; ++z) s += slab[(int64_t)z * n + i];
    out[i] = s;
}

// bias gradient: row sums over the primal columns, one workgroup per row, a fixed-order tree
extern "C" __global__ void __launch_bounds__(256) pndf_train_row_sum_kernel(const float* Z, int64_t ld, int64_t ncols, float* out) {
    __shared__ float red[256];
    const float* z = Z + (int64_t)blockIdx.x * ld;
    float s = 0.f;
    for (int64_t c = threadIdx.x; c < ncols; c += 256) s += z[c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// the three losses: one workgroup, fp64 partial sums in a fixed order
extern "C" __global__ void __launch_bounds__(256) pndf_train_loss_kernel(const float* d, const float* dgt, const float* eikp, int64_t B,
                                                                         int64_t Bm, int nj, int loss_type, int eik, float* losses) {
    __shared__ double red[3][256];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t c = threadIdx.x; c < B; c += 256) {
        const double r = (double)d[c] - (double)dgt[c];
        s0 += loss_type == LOSS_L2 ? r * r : fabs(r);
        if (eik) s2 += (double)eikp[c];
    }
    for (int64_t c = threadIdx.x; c < Bm; c += 256) s1 += fabs((double)d[B + c]);
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        losses[0] = (float)(red[0][0] / (double)B);
        losses[1] = (float)(red[1][0] / (double)Bm);
        losses[2] = eik ? (float)(red[2][0] / ((double)nj * (double)B)) : 0.f;
    }
}

// seeds of the reverse pass on the output layer (width 1): zbar on the primal columns, zdotbar on the tangent columns
extern "C" __global__ void __launch_bounds__(256) pndf_train_head_kernel(const float* d, const float* dgt, const float* D1, const float* D2,
                                                                         const float* up, int64_t B, int64_t Bm, int loss_type, int eik,
                                                                         float* zbar) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t np = B + Bm, n = eik ? np + B : B;
    if (c >= n) return;
    const float g_dist = up[0], g_man = up[1], g_eik = up[2];
    float z;
    if (c < B) {
        const float r = d[c] - dgt[c];
        const float dl = loss_type == LOSS_L2 ? 2.f * r / (float)B : (float)((r > 0.f) - (r < 0.f)) / (float)B;
        z = g_dist * dl * D1[c];
        if (D2) z += g_eik * D2[c];
    } else if (c < np) {
        const float m = d[c];
        z = g_man * ((float)((m > 0.f) - (m < 0.f)) / (float)Bm) * D1[c];
    } else {
        z = g_eik * D1[c - np];
    }
    zbar[c] = z;
}

// ------------------------------------------------------------------------------------------------------------ host side
namespace {

struct Shape {
    int64_t B = 0, Bm = 0;
    int loss_type = 0, eik = 0;
};

// workspace layout in floats (every region 256-byte aligned)
struct Layout {
    int64_t np, ncols, nrev;
    int64_t wenc, X, dgt, act[MAX_LIN + 1], D1[MAX_LIN], D2[MAX_LIN], Xd, eikp, Z[2], slab, part;
    int split[MAX_LIN], kc[MAX_LIN];
    int enc_wgs;
    int64_t total;
};

}  // namespace

struct pndf_train_plan : LayerNet {
    std::mutex mu;
    std::unordered_map<const void*, Shape> shapes;      // workspace -> the shape of the forward that filled it
    std::string err;
};

namespace {

Layout make_layout(const pndf_train_plan* h, int64_t B, int64_t Bm, int eik) {
    Layout l{};
    l.np = B + Bm;
    l.ncols = eik ? l.np + B : l.np;
    l.nrev = eik ? l.ncols : B;
    Carver c;
    l.wenc = c.take(h->enc_params);
    l.X = c.take((int64_t)h->nj * BONE * l.np);
    l.dgt = c.take(B);
    for (int t = 0; t <= h->L; ++t) l.act[t] = c.take((int64_t)h->dims[t] * l.ncols);
    for (int t = 0; t < h->L; ++t) l.D1[t] = c.take((int64_t)h->dims[t + 1] * l.np);
    for (int t = 0; t < h->L; ++t) l.D2[t] = (eik && h->act == PNDF_ACT_SOFTPLUS) ? c.take((int64_t)h->dims[t + 1] * B) : -1;
    l.Xd = eik ? c.take((int64_t)h->nj * BONE * B) : -1;
    l.eikp = eik ? c.take(B) : -1;
    // the two ping-pong adjoint buffers of the reverse pass; the forward's input-gradient pass uses the same memory
    l.Z[0] = c.take((int64_t)h->maxw * l.ncols);
    l.Z[1] = c.take((int64_t)h->maxw * l.ncols);
    int64_t slab = 0;
    for (int t = 0; t < h->L; ++t) {
        // K split of the weight-gradient GEMM: a function of the shapes only, never of the device's occupancy
        const int64_t M = h->dims[t + 1], N = h->dims[t];
        const int64_t tiles = ((M + TM - 1) / TM) * ((N + TN - 1) / TN);
        int64_t S = (SPLIT_TARGET_WGS + tiles - 1) / tiles;
        const int64_t smax = (l.nrev + 255) / 256;
        if (S > smax) S = smax;
        if (S < 1) S = 1;
        int64_t kc = (l.nrev + S - 1) / S;
        kc = (kc + TK - 1) / TK * TK;
        S = (l.nrev + kc - 1) / kc;
        l.split[t] = (int)S;
        l.kc[t] = (int)kc;
        if (S * M * N > slab) slab = S * M * N;
    }
    l.slab = c.take(slab);
    const int64_t P = eik ? l.np : B;
    l.enc_wgs = (int)((P + ENC_WG - 1) / ENC_WG);
    l.part = c.take((int64_t)l.enc_wgs * h->enc_params);
    l.total = c.o;
    return l;
}

const GemmKernels TRAIN_GEMM = {pndf_train_gemm_nn_kernel, pndf_train_gemm_tn_kernel, pndf_train_gemm_nt_kernel};

EncArgs enc_args(const pndf_train_plan* h, const Layout& l, float* ws, int64_t B, int64_t Bm, int eik) {
    EncArgs e;
    memset(&e, 0, sizeof(e));
    e.wenc = ws + l.wenc;
    e.X = ws + l.X;
    e.dgt_copy = ws + l.dgt;
    e.act0 = ws + l.act[0];
    e.U0 = ws + l.Z[0];
    e.Xd = eik ? ws + l.Xd : nullptr;
    e.eikp = eik ? ws + l.eikp : nullptr;
    e.part = ws + l.part;
    e.B = B; e.Bm = Bm; e.np = l.np; e.ncols = l.ncols;
    e.act = h->enc_act; e.beta = h->enc_beta; e.eik = eik; e.n_params = h->enc_params; e.nj = h->nj;
    for (int j = 0; j < h->nj; ++j) { e.parent[j] = h->parent[j]; e.off[j] = h->enc_off[j]; }
    return e;
}

}  // namespace

extern "C" const char* pndf_train_last_error(pndf_train_handle h) { return pndf_last_error_of(h); }

namespace {

const char* const NO_ENCODER = "training needs the structure encoder (model.StrEnc.use: True, dims[0] = 126): the reference's train=True "
                               "branch cannot run without it either (man_pose_in is unbound)";

// the two creates: one plan, refusals before a device is looked for; `any_tree`: every joint tree of pndf_net_plan.h, not SMPL's 21 alone
int train_create(pndf_train_handle* out, const pndf_config* cfg, int device, bool any_tree) {
    if (!out || !cfg) return pndf_fail<pndf_train_plan>(nullptr, PNDF_ERR_BAD_ARG, "out / cfg is null");
    *out = nullptr;
    if (const char* why = layer_network_refusal(cfg, NO_ENCODER, any_tree)) return pndf_fail<pndf_train_plan>(nullptr, PNDF_ERR_UNSUPPORTED, why);
    const PndfDeviceCheck dev = pndf_check_gfx950(device, "training");
    if (dev.code != PNDF_OK) return pndf_fail<pndf_train_plan>(nullptr, dev.code, dev.text);
    pndf_train_plan* h = new pndf_train_plan();
    layer_net_init(*h, cfg, device);
    *out = h;
    return PNDF_OK;
}

}  // namespace

extern "C" int pndf_train_create(pndf_train_handle* out, const pndf_config* cfg, int device) { return train_create(out, cfg, device, false); }

extern "C" int pndf_skel_train_create(pndf_train_handle* out, const pndf_config* cfg, int device) { return train_create(out, cfg, device, true); }

extern "C" int pndf_train_destroy(pndf_train_handle h) {
    delete h;
    return PNDF_OK;
}

extern "C" int64_t pndf_train_workspace_floats(pndf_train_handle h, int64_t B, int64_t Bm, int32_t eikonal) {
    if (!h || B < 1 || Bm < 1) return PNDF_ERR_BAD_ARG;
    return make_layout(h, B, Bm, eikonal ? 1 : 0).total;
}

extern "C" int pndf_train_forward(pndf_train_handle h, const float* const* weights, const float* q, const float* dist_gt,
                                  const float* q_man, int64_t B, int64_t Bm, int32_t loss_type, int32_t eikonal, float* losses,
                                  void* workspace, void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!weights || !q || !dist_gt || !q_man || !losses || !workspace) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pointer");
    if (B < 1 || Bm < 1) return pndf_fail(h, PNDF_ERR_BAD_ARG, "B and Bm must be >= 1");
    if (loss_type != LOSS_L1 && loss_type != LOSS_L2) return pndf_fail(h, PNDF_ERR_BAD_ARG, "loss_type: 0 (l1) or 1 (l2)");
    if (((uintptr_t)workspace & 15) != 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "workspace must be 16-byte aligned");
    if (const PndfTableFault f = pndf_table_fault(*h, weights)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "weights: " + f.text());
    PndfRange range("pndf_train_forward");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    const int eik = eikonal ? 1 : 0;
    const Layout l = make_layout(h, B, Bm, eik);
    {
        std::lock_guard<std::mutex> lk(h->mu);
        Shape s;
        s.B = B; s.Bm = Bm; s.loss_type = loss_type; s.eik = eik;
        h->shapes[workspace] = s;
    }
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int nt = 4 * h->nj;      // the encoder's tensors, in front of the trunk's
    const TrunkWeights w = trunk_weights(*h, weights + nt);
    const bool sp = h->act == PNDF_ACT_SOFTPLUS;

    hipLaunchKernelGGL(pndf_train_enc_pack_kernel, dim3(blocks(h->enc_params)), dim3(256), 0, st, ptr_table<MAX_ENC_TENSORS>(*h, weights), nt, ws + l.wenc);
    EncArgs e = enc_args(h, l, ws, B, Bm, eik);
    e.q = q; e.qm = q_man; e.dgt = dist_gt;
    hipLaunchKernelGGL(pndf_train_enc_fwd_kernel, dim3(blocks(l.np)), dim3(256), 0, st, e);
    // 1. forward over the primal columns
    for (int t = 0; t < h->L; ++t) {
        GemmArgs g = gemm_args(w.W[t], h->dims[t], ws + l.act[t], l.ncols, ws + l.act[t + 1], l.ncols, h->dims[t + 1], (int)l.np,
                               h->dims[t]);
        g.epi = EPI_FWD; g.act = h->act; g.beta = h->beta; g.out_layer = t == h->L - 1; g.bias = w.b[t];
        g.D1 = ws + l.D1[t]; g.ld1 = l.np;
        if (l.D2[t] >= 0) { g.D2 = ws + l.D2[t]; g.ld2 = B; g.nB = B; }
        launch_gemm(TRAIN_GEMM, GEMM_NN, g, 1, st);
    }
    if (eik) {
        // 2. input gradient of the noisy batch: u_t = (W_t^T u_{t+1}) sigma'_{t-1}, from sigma' of the output; ends in Z[0] = U0
        const float* U = ws + l.D1[h->L - 1];
        int64_t ldu = l.np;
        for (int t = h->L - 1; t >= 0; --t) {
            float* out = ws + l.Z[t & 1];
            GemmArgs g = gemm_args(w.W[t], h->dims[t], U, ldu, out, B, h->dims[t], (int)B, h->dims[t + 1]);
            g.epi = EPI_MUL;
            if (t > 0) { g.D1 = ws + l.D1[t - 1]; g.ld1 = l.np; }
            launch_gemm(TRAIN_GEMM, GEMM_TN, g, 1, st);
            U = out;
            ldu = B;
        }
        // 3. encoder backward, the eikonal seed, xdot and the tangent encoder
        hipLaunchKernelGGL(pndf_train_enc_eik_kernel, dim3(blocks(B)), dim3(256), 0, st, e);
        // 4. tangent forward
        for (int t = 0; t < h->L; ++t) {
            GemmArgs g = gemm_args(w.W[t], h->dims[t], ws + l.act[t] + l.np, l.ncols, ws + l.act[t + 1] + l.np, l.ncols,
                                   h->dims[t + 1], (int)B, h->dims[t]);
            g.epi = EPI_TAN; g.D1 = ws + l.D1[t]; g.ld1 = l.np;
            if (sp) { g.D2 = ws + l.D2[t]; g.ld2 = B; }
            launch_gemm(TRAIN_GEMM, GEMM_NN, g, 1, st);
        }
    }
    hipLaunchKernelGGL(pndf_train_loss_kernel, dim3(1), dim3(256), 0, st, ws + l.act[h->L], ws + l.dgt, eik ? ws + l.eikp : nullptr,
                       B, Bm, h->nj, (int)loss_type, eik, losses);
    return pndf_check_launch(h, "pndf_train_forward");
}

extern "C" int pndf_train_backward(pndf_train_handle h, const float* const* weights, const float* upstream, float* const* grads,
                                   void* workspace, void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!weights || !upstream || !grads || !workspace) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pointer");
    Shape s;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto it = h->shapes.find(workspace);
        if (it == h->shapes.end()) return pndf_fail(h, PNDF_ERR_BAD_ARG, "workspace was not filled by pndf_train_forward of this handle");
        s = it->second;
    }
    if (const PndfTableFault f = pndf_table_fault(*h, weights)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "weights: " + f.text());
    if (const PndfTableFault f = pndf_table_fault(*h, grads)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "grads: " + f.text());
    PndfRange range("pndf_train_backward");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    const int64_t B = s.B, Bm = s.Bm;
    const int eik = s.eik;
    const Layout l = make_layout(h, B, Bm, eik);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const int nt = 4 * h->nj;      // the encoder's tensors, in front of the trunk's
    const TrunkWeights w = trunk_weights(*h, weights + nt);
    float* const* G = grads + nt;
    const bool cross = eik && h->act == PNDF_ACT_SOFTPLUS;
    const int64_t npr = eik ? l.np : B;          // primal columns of the reverse pass

    hipLaunchKernelGGL(pndf_train_enc_pack_kernel, dim3(blocks(h->enc_params)), dim3(256), 0, st, ptr_table<MAX_ENC_TENSORS>(*h, weights), nt, ws + l.wenc);
    const int L = h->L;
    int zi = 0;
    hipLaunchKernelGGL(pndf_train_head_kernel, dim3(blocks(l.nrev)), dim3(256), 0, st, ws + l.act[L], ws + l.dgt, ws + l.D1[L - 1],
                       cross ? ws + l.D2[L - 1] : nullptr, upstream, B, Bm, s.loss_type, eik, ws + l.Z[zi]);
    for (int t = L - 1; t >= 0; --t) {
        const float* Zb = ws + l.Z[zi];
        const int M = h->dims[t + 1], N = h->dims[t];
        // weight gradient: [zbar|zdotbar] [a|adot]^T over every column of the reverse pass, K split, the slabs summed in order
        GemmArgs g = gemm_args(Zb, l.ncols, ws + l.act[t], l.ncols, ws + l.slab, N, M, N, (int)l.nrev);
        g.epi = EPI_STORE; g.kc = l.kc[t]; g.slab = (int64_t)M * N;
        launch_gemm(TRAIN_GEMM, GEMM_NT, g, l.split[t], st);
        hipLaunchKernelGGL(pndf_train_slab_reduce_kernel, dim3(blocks((int64_t)M * N)), dim3(256), 0, st, ws + l.slab, l.split[t],
                           (int64_t)M * N, G[2 * t]);
        hipLaunchKernelGGL(pndf_train_row_sum_kernel, dim3(M), dim3(256), 0, st, Zb, l.ncols, npr, G[2 * t + 1]);
        // adjoint of the layer's input
        float* out = ws + l.Z[zi ^ 1];
        if (t > 0 && cross) {
            // softplus: the tangent columns first (adotbar sigma'' zdot replaces sigma'' zdot), then the primal ones add it
            GemmArgs gt = gemm_args(w.W[t], N, Zb + l.np, l.ncols, out + l.np, l.ncols, N, (int)B, M);
            gt.epi = EPI_TAN; gt.D1 = ws + l.D1[t - 1]; gt.ld1 = l.np; gt.D2 = ws + l.D2[t - 1]; gt.ld2 = B;
            launch_gemm(TRAIN_GEMM, GEMM_TN, gt, 1, st);
            GemmArgs gp = gemm_args(w.W[t], N, Zb, l.ncols, out, l.ncols, N, (int)l.np, M);
            gp.epi = EPI_MUL; gp.D1 = ws + l.D1[t - 1]; gp.ld1 = l.np; gp.X = ws + l.D2[t - 1]; gp.ldx = B; gp.nB = B;
            launch_gemm(TRAIN_GEMM, GEMM_TN, gp, 1, st);
        } else {
            GemmArgs gr = gemm_args(w.W[t], N, Zb, l.ncols, out, l.ncols, N, (int)l.nrev, M);
            gr.epi = EPI_MUL;
            if (t > 0) { gr.D1 = ws + l.D1[t - 1]; gr.ld1 = l.np; gr.np_split = l.np; }
            launch_gemm(TRAIN_GEMM, GEMM_TN, gr, 1, st);
        }
        zi ^= 1;
    }
    // the encoder: dual reverse per pose, partials per workgroup, then the ordered sum into the caller's tensors
    EncArgs e = enc_args(h, l, ws, B, Bm, eik);
    e.abar = ws + l.Z[zi];
    hipLaunchKernelGGL(pndf_train_enc_rev_kernel, dim3(l.enc_wgs), dim3(ENC_WG), 0, st, e);
    hipLaunchKernelGGL(pndf_train_enc_reduce_kernel, dim3(blocks(h->enc_params)), dim3(256), 0, st, ptr_table<MAX_ENC_TENSORS>(*h, grads), nt, ws + l.part,
                       l.enc_wgs);
    return pndf_check_launch(h, "pndf_train_backward");
}
