// Second order of the distance on gfx950 (include/posendf_amd_second_order.h): for poses q, directions v and per-pose weights
// w_d, w_t one call gives  d(q),  g = grad_q d,  t = <v, g>  and  out = grad_q (w_d d + w_t <v, grad_q d>) = w_d g + w_t H v.
// The weights of the network are constants here (the train=False path): this is the double backward of
// model/posendf.py:18-27,62-76,100-101 with respect to the pose alone.
//
// With x = normalize(q, dim=1) and f the encoder plus trunk:  g = J_N g_x,  xdot = J_N v,  H v = J_N (hess f xdot) + C(q, v, g_x),
// C the curvature of the normalisation.  hess f xdot comes from the dual-number network csrc/pndf_train.hip differentiates the
// eikonal term through, seeded with dbar = 0, ddotbar = 1: the adjoint chain of the tangent is the first-order reverse (it gives
// g_x), the adjoint chain of the primal carries the sigma'' cross terms ("The dual-number bone").
// Shared with pndf_train.hip and pndf_skeleton.hip: the GEMM with its epilogues and the activation, the GEMM launcher and the
// trunk's forward and first-order reverse as launch sequences (pndf_gemm.h); the dual-number bone and the pieces of the
// normalisation (pndf_bone.h); the host's description of the network, LayerNet (pndf_net_plan.h).  Here: the two encoder kernels
// around the bone, the curvature of the normalisation with the four outputs, the tangent forward and the primal adjoint chain of
// a softplus trunk, the chunked call.
//
// Layer by layer over a chunk of SO_CHUNK poses, every activation matrix [features][columns] (the pose index contiguous) in the
// caller's workspace; the chunk is a function of B only and bounds the workspace (0.53 GB for configs/amass.yaml with softplus):
//   pndf_so_enc_fwd_kernel   lanes own poses: x, xdot, the encoder and its tangent
//   trunk forward            NN GEMMs, epilogue bias + sigma, stores sigma' and (softplus) sigma''
//   softplus trunk only      tangent forward (NN, * sigma', sigma'' zdot kept), the tangent's adjoint chain (TN, * sigma',
//                            adotbar sigma'' zdot kept), the primal's adjoint chain (TN, * sigma' + the kept cross term)
//   relu family trunk        sigma'' = 0: the first-order reverse alone (TN, * sigma'); the primal adjoint of the features is zero
//   pndf_so_enc_rev_kernel   lanes own poses: both adjoint chains through the 21 bone MLPs (no weight gradient, so no
//                            reduction), then the normalisation: g, t, J_N xbar + C, the four outputs
// A relu-family network (trunk and encoder) has hess f = 0: H v = C, and the tangent and the primal chain are skipped everywhere.
// Arithmetic: exact fp32 MFMA (v_mfma_f32_16x16x4_f32), fp32 accumulate.  No float atomics, no communication between workgroups
// inside a launch: two calls with the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/posendf_amd_second_order.h"
#include "pndf_experiment.h"
#include "pndf_bone.h"
#include "pndf_host.h"

PNDF_EXPORT_EXPERIMENT_WORD(second_order)

namespace {

// Poses per pass over the layers: a constant, so the chunk seams depend on B only.  Measured at B = 65,536 on amass.yaml's dims
// (lrelu / softplus, ms per call; profiles/second_order/chunk_sweep.jsonl): 4,096 -> 20.9 / 44.2, 8,192 -> 11.4 / 24.5, 16,384 -> 7.75 / 17.6.  A 4,096-column chunk would keep its
// 133 MB inside the last-level cache, but the 128 x 128 GEMM tile then fills half of the 256 CUs on the 512-row layers with one
// workgroup each; 16,384 columns give every layer at least two workgroups per CU, and that outweighs the cache.
constexpr int64_t SO_CHUNK = 16384;

struct SoArgs {
    const float* wenc;        // packed encoder weights
    const float* q;           // the chunk's poses [n][84]
    const float* v;           // the chunk's directions [n][84]
    const float* w_d;         // [n] or null (0)
    const float* w_t;         // [n] or null (1)
    float* d_out;             // [n] or null
    float* g_out;             // [n][84] or null
    float* t_out;             // [n] or null
    float* h_out;             // [n][84] or null
    float* X;                 // normalised poses [84][ld]
    float* Xd;                // xdot = J_N v [84][ld]                                   (dual only)
    float* act0;              // encoder output [126][ld]
    float* tan0;              // its tangent [126][ld]                                    (dual only)
    float* U0;                // adjoint of the tangent features = d d / d act0 [126][ld], accumulated in place
    float* A0;                // adjoint of the primal features [126][ld], accumulated in place  (dual only)
    float* Gx;                // g_x [84][ld]
    float* Xb;                // xbar = hess f xdot [84][ld]                              (dual only)
    const float* dist;        // the trunk's output row [ld]
    int64_t n, ld;
    int act, dual, zero_a0;   // act / beta: the encoder's; dual: the network has a softplus; zero_a0: no trunk pass writes A0
    float beta;
    int parent[NJ];
    int off[NJ];
};

// bone j's input on column c: its own normalised quaternion and its parent's feature; `tan`: the tangents of both
template <int FIN>
__device__ __forceinline__ void so_load_in(const SoArgs& e, int j, int64_t c, bool tan, float* in) {
    bone_load<FIN>(tan ? e.Xd : e.X, e.ld, tan ? e.tan0 : e.act0, e.ld, e.parent, j, c, in);
}

// primal and (dual) tangent forward of one bone
template <int FIN>
__device__ __forceinline__ void so_fwd_bone(const SoArgs& e, int j, int64_t c) {
    const float* w = e.wenc + e.off[j];
    float in[FIN], ind[FIN];
    BoneDual b;
    so_load_in<FIN>(e, j, c, false, in);
    bone_fwd<FIN>(e, w, in, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) e.act0[(int64_t)(j * FEAT + i) * e.ld + c] = b.ao[i];
    if (!e.dual) return;
    so_load_in<FIN>(e, j, c, true, ind);
    bone_tan<FIN>(w, ind, true, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) e.tan0[(int64_t)(j * FEAT + i) * e.ld + c] = b.oz[i] * b.d1o[i];
}

// reverse of one bone for one pose.  The tangent's adjoint (U0 -> Gx, the parent's rows of U0) is the first-order reverse; with
// DUAL the primal's adjoint (A0 -> Xb, the parent's rows of A0) runs next to it with the sigma'' cross terms.
template <int FIN, bool DUAL>
__device__ __forceinline__ void so_rev_bone(const SoArgs& e, int j, int64_t c) {
    const float* w = e.wenc + e.off[j];
    float in[FIN], ind[FIN], ab[FEAT], adb[FEAT];
    BoneDual b;
    BoneAdj r;
    so_load_in<FIN>(e, j, c, false, in);
    bone_fwd<FIN>(e, w, in, b);
    if (DUAL) so_load_in<FIN>(e, j, c, true, ind);
    bone_tan<FIN>(w, ind, DUAL, b);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        adb[i] = e.U0[(int64_t)(j * FEAT + i) * e.ld + c];
        if (DUAL) ab[i] = e.A0[(int64_t)(j * FEAT + i) * e.ld + c];
    }
    bone_dual_rev<FIN, DUAL>(w, b, ab, adb, r);
#pragma unroll
    for (int m = 0; m < FIN; ++m) {
        float s, sd;
        bone_input_adj<FIN, DUAL>(w, r, m, s, sd);
        if (m < BONE) {
            e.Gx[(int64_t)(j * BONE + m) * e.ld + c] = sd;
            if (DUAL) e.Xb[(int64_t)(j * BONE + m) * e.ld + c] = s;
        } else {
            const int64_t at = (int64_t)(e.parent[j] * FEAT + (m - BONE)) * e.ld + c;
            e.U0[at] += sd;
            if (DUAL) e.A0[at] += s;
        }
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pndf_so_gemm_nn_kernel(GemmArgs g) { gemm_body<1, 0>(g); }
extern "C" __global__ void __launch_bounds__(256) pndf_so_gemm_tn_kernel(GemmArgs g) { gemm_body<0, 0>(g); }

// the caller's 84 encoder tensors -> one flat array
extern "C" __global__ void __launch_bounds__(256) pndf_so_enc_pack_kernel(PtrTable t, float* dst) { enc_pack_body(t, ENC_TENSORS, dst); }

// x = normalize(q, dim=1) (over the joint axis, per quaternion component), xdot = J_N v, the encoder and its tangent
extern "C" __global__ void __launch_bounds__(256) pndf_so_enc_fwd_kernel(SoArgs e) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.n) return;
    const float* q = e.q + c * POSE;
    const float* v = e.v + c * POSE;
    float nrm[BONE], a[BONE] = {0.f, 0.f, 0.f, 0.f};
    pose_col_norms(q, NJ, nrm);
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const float x = norm_x(q[j * BONE + k], nrm[k]);
            e.X[(int64_t)(j * BONE + k) * e.ld + c] = x;
            a[k] = fmaf(x, v[j * BONE + k], a[k]);
        }
    if (e.dual) {
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < BONE; ++k) {
                const float x = e.X[(int64_t)(j * BONE + k) * e.ld + c];
                e.Xd[(int64_t)(j * BONE + k) * e.ld + c] = norm_jvp(v[j * BONE + k], x, a[k], nrm[k], nrm[k] > NORM_EPS);
            }
    }
    for (int j = 0; j < NJ; ++j) {
        if (e.parent[j] < 0) so_fwd_bone<BONE>(e, j, c);
        else so_fwd_bone<BONE + FEAT>(e, j, c);
    }
    if (e.zero_a0)
        for (int f = 0; f < ENC_IN; ++f) e.A0[(int64_t)f * e.ld + c] = 0.f;
}

// both adjoint chains through the encoder, then the normalisation and the four outputs.  Per component column k with s = |q_k|,
// n = q_k / s, p = J v_k, g = J g_k (J = (I - n n^T) / s):   H v = J xbar_k - [(g_k . p) n + (n . v_k) g + (g_k . n) p] / s;
// where the norm is clamped the normalisation is linear: J = I / eps and no curvature.
extern "C" __global__ void __launch_bounds__(256) pndf_so_enc_rev_kernel(SoArgs e) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.n) return;
    for (int j = NJ - 1; j >= 0; --j) {
        const bool root = e.parent[j] < 0;      // without a softplus the primal chain is compiled out, not run on zeros
        if (e.dual) root ? so_rev_bone<BONE, true>(e, j, c) : so_rev_bone<BONE + FEAT, true>(e, j, c);
        else root ? so_rev_bone<BONE, false>(e, j, c) : so_rev_bone<BONE + FEAT, false>(e, j, c);
    }
    const float* q = e.q + c * POSE;
    const float* v = e.v + c * POSE;
    float s[BONE], a[BONE] = {0.f, 0.f, 0.f, 0.f}, b[BONE] = {0.f, 0.f, 0.f, 0.f}, xe[BONE] = {0.f, 0.f, 0.f, 0.f};
    pose_col_norms(q, NJ, s);
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const int64_t at = (int64_t)(j * BONE + k) * e.ld + c;
            const float x = e.X[at];
            a[k] = fmaf(x, v[j * BONE + k], a[k]);
            b[k] = fmaf(x, e.Gx[at], b[k]);
            if (e.dual) xe[k] = fmaf(x, e.Xb[at], xe[k]);
        }
    float gp[BONE] = {0.f, 0.f, 0.f, 0.f};
    bool live[BONE];
#pragma unroll
    for (int k = 0; k < BONE; ++k) live[k] = s[k] > NORM_EPS;
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const int64_t at = (int64_t)(j * BONE + k) * e.ld + c;
            const float p = (v[j * BONE + k] - e.X[at] * a[k]) / s[k];
            if (live[k]) gp[k] = fmaf(e.Gx[at], p, gp[k]);
        }
    const float wd = e.w_d ? e.w_d[c] : 0.f, wt = e.w_t ? e.w_t[c] : 1.f;
    float t = 0.f;
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const int64_t at = (int64_t)(j * BONE + k) * e.ld + c;
            const float x = e.X[at], gx = e.Gx[at], vv = v[j * BONE + k];
            const float xb = e.dual ? e.Xb[at] : 0.f;
            float g, hv;
            if (live[k]) {
                const float p = (vv - x * a[k]) / s[k];
                g = (gx - x * b[k]) / s[k];
                hv = (xb - x * xe[k]) / s[k] - (gp[k] * x + a[k] * g + b[k] * p) / s[k];
            } else {
                g = gx / NORM_EPS;
                hv = xb / NORM_EPS;
            }
            t = fmaf(vv, g, t);
            if (e.g_out) e.g_out[c * POSE + j * BONE + k] = g;
            if (e.h_out) e.h_out[c * POSE + j * BONE + k] = wd * g + wt * hv;
        }
    if (e.t_out) e.t_out[c] = t;
    if (e.d_out) e.d_out[c] = e.dist[c];
}

// ------------------------------------------------------------------------------------------------------------ host side
struct pndf_so_plan : LayerNet {
    bool dual_trunk = false, dual = false;      // softplus trunk; a softplus anywhere
    std::string err;
};

namespace {

// workspace layout in floats (every region 256-byte aligned); nc: the columns of a chunk
struct SoLayout {
    int64_t nc;
    int64_t wenc, X, Xd, act0, tan0, U0, A0, Gx, Xb, dist, D1[MAX_LIN], D2[MAX_LIN], P[2];
    int64_t total;
};

SoLayout so_layout(const pndf_so_plan* h, int64_t B) {
    SoLayout l{};
    l.nc = B < SO_CHUNK ? B : SO_CHUNK;
    Carver c;
    l.wenc = c.take(h->enc_params);
    l.X = c.take(POSE * l.nc);
    l.Xd = h->dual ? c.take(POSE * l.nc) : -1;
    l.act0 = c.take(ENC_IN * l.nc);
    l.tan0 = h->dual ? c.take(ENC_IN * l.nc) : -1;
    l.U0 = c.take(ENC_IN * l.nc);
    l.A0 = h->dual ? c.take(ENC_IN * l.nc) : -1;
    l.Gx = c.take(POSE * l.nc);
    l.Xb = h->dual ? c.take(POSE * l.nc) : -1;
    l.dist = c.take(l.nc);
    for (int t = 0; t < h->L; ++t) l.D1[t] = c.take((int64_t)h->dims[t + 1] * l.nc);
    for (int t = 0; t < h->L; ++t) l.D2[t] = h->dual_trunk ? c.take((int64_t)h->dims[t + 1] * l.nc) : -1;
    // the two ping-pong buffers every pass over the layers runs through
    l.P[0] = c.take((int64_t)h->maxw * l.nc);
    l.P[1] = c.take((int64_t)h->maxw * l.nc);
    l.total = c.o;
    return l;
}

const GemmKernels SO_GEMM = {pndf_so_gemm_nn_kernel, pndf_so_gemm_tn_kernel, nullptr};

}  // namespace

extern "C" const char* pndf_so_last_error(pndf_so_handle h) { return pndf_last_error_of(h); }

extern "C" int pndf_so_create(pndf_so_handle* out, const pndf_config* cfg, int device) {
    if (!out || !cfg) return pndf_fail<pndf_so_plan>(nullptr, PNDF_ERR_BAD_ARG, "out / cfg is null");
    *out = nullptr;
    if (const char* why = layer_network_refusal(cfg, "the second order needs the structure encoder (model.StrEnc.use: True, dims[0] = 126)"))
        return pndf_fail<pndf_so_plan>(nullptr, PNDF_ERR_UNSUPPORTED, why);
    const PndfDeviceCheck dev = pndf_check_gfx950(device, "the second order");
    if (dev.code != PNDF_OK) return pndf_fail<pndf_so_plan>(nullptr, dev.code, dev.text);
    pndf_so_plan* h = new pndf_so_plan();
    layer_net_init(*h, cfg, device);
    h->dual_trunk = h->act == PNDF_ACT_SOFTPLUS;
    h->dual = h->dual_trunk || h->enc_act == PNDF_ACT_SOFTPLUS;
    *out = h;
    return PNDF_OK;
}

extern "C" int pndf_so_destroy(pndf_so_handle h) {
    delete h;
    return PNDF_OK;
}

extern "C" int64_t pndf_so_workspace_floats(pndf_so_handle h, int64_t B) {
    if (!h || B < 0) return PNDF_ERR_BAD_ARG;
    return B == 0 ? 0 : so_layout(h, B).total;
}

extern "C" int pndf_second_order(pndf_so_handle h, const float* const* weights, const float* q, const float* v, const float* w_d,
                                 const float* w_t, float* d, float* g, float* t, float* out, int64_t B, void* workspace,
                                 int64_t workspace_floats, void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (B < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative batch");
    if (B == 0) return PNDF_OK;
    if (!weights || !q || !v) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pointer");
    if (((uintptr_t)q | (uintptr_t)v | (uintptr_t)w_d | (uintptr_t)w_t | (uintptr_t)d | (uintptr_t)g | (uintptr_t)t | (uintptr_t)out) & 3)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose, direction, weight or output buffer");
    if (overlaps(out, q, B * POSE) || overlaps(out, v, B * POSE) || overlaps(g, q, B * POSE) || overlaps(g, v, B * POSE) || overlaps(g, out, B * POSE))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "out and g must not alias q, v or each other");
    const SoLayout l = so_layout(h, B);
    if (const int rc = pndf_check_workspace(h, workspace, workspace_floats, l.total, "floats", "pndf_so_workspace_floats"); rc != PNDF_OK) return rc;
    if (const PndfTableFault f = pndf_table_fault(*h, weights)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "weights: " + f.text());
    PndfRange range("pndf_second_order");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const TrunkWeights w = trunk_weights(*h, weights + ENC_TENSORS);
    const int L = h->L;
    const int64_t ld = l.nc;
    TrunkBuffers b{};
    b.in = ws + l.act0; b.P[0] = ws + l.P[0]; b.P[1] = ws + l.P[1]; b.out = ws + l.dist; b.din = ws + l.U0;
    b.ld = ld;
    for (int tt = 0; tt < L; ++tt) { b.D1[tt] = ws + l.D1[tt]; b.D2[tt] = h->dual_trunk ? ws + l.D2[tt] : nullptr; }

    hipLaunchKernelGGL(pndf_so_enc_pack_kernel, dim3(blocks(h->enc_params)), dim3(256), 0, st, ptr_table(*h, weights), ws + l.wenc);

    SoArgs e;
    memset(&e, 0, sizeof(e));
    e.wenc = ws + l.wenc;
    e.X = ws + l.X; e.act0 = ws + l.act0; e.U0 = ws + l.U0; e.Gx = ws + l.Gx; e.dist = ws + l.dist;
    if (h->dual) { e.Xd = ws + l.Xd; e.tan0 = ws + l.tan0; e.A0 = ws + l.A0; e.Xb = ws + l.Xb; }
    e.ld = ld;
    e.act = h->enc_act; e.beta = h->enc_beta; e.dual = h->dual ? 1 : 0; e.zero_a0 = (h->dual && !h->dual_trunk) ? 1 : 0;
    for (int j = 0; j < NJ; ++j) { e.parent[j] = h->parent[j]; e.off[j] = h->enc_off[j]; }

    for (int64_t c0 = 0; c0 < B; c0 += l.nc) {
        const int n = (int)(B - c0 < l.nc ? B - c0 : l.nc);
        e.n = n;
        e.q = q + c0 * POSE; e.v = v + c0 * POSE;
        e.w_d = w_d ? w_d + c0 : nullptr; e.w_t = w_t ? w_t + c0 : nullptr;
        e.d_out = d ? d + c0 : nullptr; e.g_out = g ? g + c0 * POSE : nullptr;
        e.t_out = t ? t + c0 : nullptr; e.h_out = out ? out + c0 * POSE : nullptr;
        hipLaunchKernelGGL(pndf_so_enc_fwd_kernel, dim3(blocks(n)), dim3(256), 0, st, e);
        b.n = n;
        trunk_forward(SO_GEMM, *h, w, b, st);      // 1. sigma' kept, and (softplus) sigma''
        if (h->dual_trunk) {
            // 2. tangent forward: adot = sigma' zdot; sigma'' zdot replaces sigma''
            for (int tt = 0; tt < L; ++tt) {
                GemmArgs a = gemm_args(w.W[tt], h->dims[tt], tt == 0 ? ws + l.tan0 : ws + l.P[(tt - 1) & 1], ld, ws + l.P[tt & 1], ld,
                                       h->dims[tt + 1], n, h->dims[tt]);
                a.epi = EPI_TAN; a.D1 = ws + l.D1[tt]; a.ld1 = ld; a.D2 = ws + l.D2[tt]; a.ld2 = ld;
                launch_gemm(SO_GEMM, GEMM_NN, a, 1, st);
            }
        }
        // 3. the tangent's adjoint chain from zdotbar = sigma' of the output (seed ddotbar = 1): the first-order reverse.  Softplus:
        //    adotbar sigma'' zdot replaces sigma'' zdot on the way
        trunk_reverse(SO_GEMM, *h, w, b, st);
        if (h->dual_trunk) {
            // 4. the primal's adjoint chain from zbar = sigma'' zdot of the output (seed dbar = 0): abar sigma' + the kept cross term
            const float* Z = ws + l.D2[L - 1];
            for (int tt = L - 1; tt >= 0; --tt) {
                float* o = tt == 0 ? ws + l.A0 : ws + l.P[tt & 1];
                GemmArgs a = gemm_args(w.W[tt], h->dims[tt], Z, ld, o, ld, h->dims[tt], n, h->dims[tt + 1]);
                a.epi = EPI_MUL;
                if (tt > 0) { a.D1 = ws + l.D1[tt - 1]; a.ld1 = ld; a.X = ws + l.D2[tt - 1]; a.ldx = ld; a.nB = n; }
                launch_gemm(SO_GEMM, GEMM_TN, a, 1, st);
                Z = o;
            }
        }
        hipLaunchKernelGGL(pndf_so_enc_rev_kernel, dim3(blocks(n)), dim3(256), 0, st, e);
    }
    return pndf_check_launch(h, "pndf_second_order");
}
