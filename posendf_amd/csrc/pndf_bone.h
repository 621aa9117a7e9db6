// The structure encoder of the layer-by-layer units (csrc/pndf_train.hip, csrc/pndf_second_order.hip, csrc/pndf_skeleton.hip), on
// top of pndf_gemm.h.  Device side: one bone MLP as a dual number (its input gather, its forward with the tangent, its reverse with
// the primal and the tangent adjoint: DESIGN.md section 2s, "The dual-number bone"), the pieces of normalize(q, dim=1), the table
// of the encoder's 4 J tensors.  Host side: what training and the second order refuse of a network and ask of its tensors; the
// plan itself, LayerNet, is pndf_net_plan.h's.  Each unit keeps what is its own: training the LDS reduction of the weight
// gradient, the second order the curvature of the normalisation and the 21 joints its kernels are compiled for; training and the
// skeleton unit take the joint count at run time.  Everything is in an unnamed namespace, instantiated per translation unit as in
// pndf_gemm.h.
#pragma once
#include "pndf_gemm.h"
#include "pndf_net_plan.h"

namespace {

constexpr int NJ = 21, FEAT = 6, HID = 10, BONE = 4;      // NJ and what follows from it: the SMPL table, for the second order
constexpr int ENC_IN = NJ * FEAT;          // 126: the encoder's output, the trunk's input
constexpr int POSE = NJ * BONE;            // 84
constexpr int MAX_LIN = PNDF_NET_MAX_LIN;  // 1 .. 7 hidden layers -> 2 .. 8 linear layers
constexpr int ENC_TENSORS = 4 * NJ;        // 84
constexpr int MAXJ = PNDF_SKEL_MAX_JOINTS; // the units that take the joint count at run time: 1 .. 32 joints
constexpr int MAX_ENC_TENSORS = 4 * MAXJ;  // 128
constexpr float NORM_EPS = 1e-12f;         // F.normalize

// ---- encoder: one bone MLP per joint (4 | 10 -> 10 -> 6), the weights packed in state-dict order into one flat array
template <int FIN>
__device__ __forceinline__ void bone_lin0(const float* w, const float* in, float* zh, bool bias) {
#pragma unroll
    for (int i = 0; i < HID; ++i) {
        float s = bias ? w[HID * FIN + i] : 0.f;
#pragma unroll
        for (int k = 0; k < FIN; ++k) s = fmaf(w[i * FIN + k], in[k], s);
        zh[i] = s;
    }
}
template <int FIN>
__device__ __forceinline__ const float* bone_w2(const float* w) { return w + HID * FIN + HID; }

// bone j's input on column `col`: its own four rows of x (row stride ldx) and its parent's six feature rows of f (row stride ldf)
template <int FIN>
__device__ __forceinline__ void bone_load(const float* x, int64_t ldx, const float* f, int64_t ldf, const int* parent, int j,
                                          int64_t col, float* out) {
#pragma unroll
    for (int k = 0; k < BONE; ++k) out[k] = x[(int64_t)(j * BONE + k) * ldx + col];
    if (FIN > BONE) {
        const int p = parent[j];
#pragma unroll
        for (int i = 0; i < FIN - BONE; ++i) out[BONE + i] = f[(int64_t)(p * FEAT + i) * ldf + col];
    }
}

// One bone at one pose as a dual number: the primal's activations with sigma' and sigma'' of both layers, and along the tangent
// of the input the pre-activations hz (hidden) and oz (output) and the hidden tangent ahd = sigma'h hz.  The tangent of the bone's
// output is oz sigma'o.
struct BoneDual {
    float ah[HID], d1h[HID], d2h[HID], ao[FEAT], d1o[FEAT], d2o[FEAT];
    float hz[HID], ahd[HID], oz[FEAT];
};

// The dual forward of one bone in its two steps, so that a caller can store the primal's output before it gathers the tangent's
// input.  The primal from `in` (E: the kernel's argument struct, for its act and beta) ...
template <int FIN, class E>
__device__ __forceinline__ void bone_fwd(const E& e, const float* w, const float* in, BoneDual& b) {
    float zh[HID];
    bone_lin0<FIN>(w, in, zh, true);
#pragma unroll
    for (int i = 0; i < HID; ++i) act_eval(e.act, e.beta, false, zh[i], b.ah[i], b.d1h[i], b.d2h[i]);
    const float* w2 = bone_w2<FIN>(w);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        float s = w2[FEAT * HID + i];
#pragma unroll
        for (int k = 0; k < HID; ++k) s = fmaf(w2[i * HID + k], b.ah[k], s);
        act_eval(e.act, e.beta, false, s, b.ao[i], b.d1o[i], b.d2o[i]);
    }
}
// ... then, with `tangent`, the tangent along `ind`; without it +0 and no product formed
template <int FIN>
__device__ __forceinline__ void bone_tan(const float* w, const float* ind, bool tangent, BoneDual& b) {
#pragma unroll
    for (int k = 0; k < HID; ++k) b.hz[k] = b.ahd[k] = 0.f;
#pragma unroll
    for (int i = 0; i < FEAT; ++i) b.oz[i] = 0.f;
    if (!tangent) return;
    const float* w2 = bone_w2<FIN>(w);
    bone_lin0<FIN>(w, ind, b.hz, false);
#pragma unroll
    for (int k = 0; k < HID; ++k) b.ahd[k] = b.d1h[k] * b.hz[k];
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < HID; ++k) s = fmaf(w2[i * HID + k], b.ahd[k], s);
        b.oz[i] = s;
    }
}

// the adjoints of one bone's pre-activations, output (zo) and hidden (zh), primal (..b) and tangent (..db)
struct BoneAdj {
    float zob[FEAT], zodb[FEAT], zhb[HID], zhdb[HID];
};

// Dual reverse of one bone ("The dual-number bone") from the adjoints ab (primal) and adb (tangent) of its
// six outputs.  Without PRIMAL the ab chain is compiled out (ab is not read, zob and zhb stay unwritten): what is left is the
// first-order reverse, the chain a network without a second derivative needs.
// The rounding of the two sums is pinned (one fma, the other product rounded first), no longer left to -ffp-contract: zhb takes
// the cross term's last product into the fma.  For zob the two units' own copies had been compiled differently, the second order
// like zhb in all six outputs, training in the last output only (the other five fuse ab sigma'o instead).  Bit i of FUSE_CROSS
// keeps that choice for output i, so that both units compute the bits they did; one mask for both would move training's.
template <int FIN, bool PRIMAL, unsigned FUSE_CROSS = 0x3f>
__device__ __forceinline__ void bone_dual_rev(const float* w, const BoneDual& b, const float* ab, const float* adb, BoneAdj& r) {
#pragma clang fp contract(off)
    const float* w2 = bone_w2<FIN>(w);
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        const float cross = adb[i] * b.oz[i];
        if (PRIMAL) r.zob[i] = (FUSE_CROSS >> i & 1) ? fmaf(cross, b.d2o[i], ab[i] * b.d1o[i]) : fmaf(ab[i], b.d1o[i], cross * b.d2o[i]);
        r.zodb[i] = adb[i] * b.d1o[i];
    }
#pragma unroll
    for (int k = 0; k < HID; ++k) {
        float s = 0.f, sd = 0.f;
#pragma unroll
        for (int i = 0; i < FEAT; ++i) {
            if (PRIMAL) s = fmaf(w2[i * HID + k], r.zob[i], s);
            sd = fmaf(w2[i * HID + k], r.zodb[i], sd);
        }
        if (PRIMAL) r.zhb[k] = fmaf(sd * b.hz[k], b.d2h[k], s * b.d1h[k]);
        r.zhdb[k] = sd * b.d1h[k];
    }
}
// ... and the adjoints of input m, s the primal's and sd the tangent's: the caller's loop, which stores each pair as it comes
template <int FIN, bool PRIMAL>
__device__ __forceinline__ void bone_input_adj(const float* w, const BoneAdj& r, int m, float& s, float& sd) {
    s = 0.f;
    sd = 0.f;
#pragma unroll
    for (int k = 0; k < HID; ++k) {
        if (PRIMAL) s = fmaf(w[k * FIN + m], r.zhb[k], s);
        sd = fmaf(w[k * FIN + m], r.zhdb[k], sd);
    }
}

// ---- x = normalize(q, dim=1): over the joint axis, per quaternion component k (a column of nj joints)
// the norms of a pose's four columns, the joints summed in index order
__device__ __forceinline__ void pose_col_norms(const float* q, int nj, float* nrm) {
    float n2[BONE] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nj; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) n2[k] = fmaf(q[j * BONE + k], q[j * BONE + k], n2[k]);
#pragma unroll
    for (int k = 0; k < BONE; ++k) nrm[k] = sqrtf(n2[k]);
}
__device__ __forceinline__ float norm_x(float q, float nrm) { return q / fmaxf(nrm, NORM_EPS); }
// J_N v = (v - x (x . v)) / |q_k| with a = x . v over the column; v / eps where the norm is clamped.  `live` is the caller's:
// training tests nrm >= NORM_EPS, the second order nrm > NORM_EPS.  They part at nrm == eps exactly, where one comparison for
// both would change the bits of one of them.
__device__ __forceinline__ float norm_jvp(float v, float x, float a, float nrm, bool live) {
    return live ? (v - x * a) / nrm : v / NORM_EPS;
}

// ---- the caller's encoder tensors and their offsets in the flat array: a table of NT entries of which the first n are live
// (n = NT = 84 in the second order; training sizes it for 32 joints and takes n = 4 J from the plan)
template <int NT>
struct PtrTableOf {
    float* p[NT];
    int off[NT + 1];
};
using PtrTable = PtrTableOf<ENC_TENSORS>;

template <int NT>
__device__ __forceinline__ void enc_pack_body(const PtrTableOf<NT>& t, int n, float* dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.off[n]) return;
    int k = 0;
    while (t.off[k + 1] <= i) ++k;
    dst[i] = t.p[k][i - t.off[k]];
}

// ------------------------------------------------------------------------------------------------------------ host side
// The networks training and the second order run: what pndf_net_plan.h accepts, with the structure encoder and -- unless
// `any_tree`, the training plans of posendf_amd_skeleton_train.h -- the 21 joints the second order's kernels are compiled for.
// Null, or why `cfg` is PNDF_ERR_UNSUPPORTED; `no_encoder`: the caller's text for a network without it.
inline const char* layer_network_refusal(const pndf_config* cfg, const char* no_encoder, bool any_tree = false) {
    if (const char* why = pndf_skeleton_refusal(cfg)) return why;
    if (!any_tree && cfg->num_joints != NJ)
        return "num_joints must be 21 (pndf_skel_create of posendf_amd_skeleton.h and pndf_skel_train_create of "
               "posendf_amd_skeleton_train.h take any joint tree)";
    if (cfg->dims[0] != FEAT * cfg->num_joints) return no_encoder;
    return pndf_dfnet_refusal(cfg);
}

// the encoder's 4 J tensors among the caller's `tensors` (weights, or gradients to write); the entries past them are null and
// their offsets the end of the packed encoder
template <int NT = ENC_TENSORS>
inline PtrTableOf<NT> ptr_table(const LayerNet& n, const float* const* tensors) {
    PtrTableOf<NT> t;
    const int live = 4 * n.nj;
    for (int k = 0; k < NT; ++k) t.p[k] = k < live ? const_cast<float*>(tensors[k]) : nullptr;
    for (int k = 0; k <= NT; ++k) t.off[k] = n.enc_tensor_off[k < live ? k : live];
    return t;
}

}  // namespace
