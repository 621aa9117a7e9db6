// Operand scales of the split-precision body-model kernels (pndf_lbs.hip), host side: ONE function chooses all of them, for
// pndf_lbs_create (the model's part, once), for every launch (the term weights' part) and for the read-out of
// include/posendf_amd_debug.h (pndf_debug_lbs_scales), which tests/test_lbs_range.py holds against the fp64 oracle's operands.
//
// No scale is measured at run time: each is a power of two derived from an a-priori bound of its operand,
//   operand                              scale               bound
//   pose blend shapes P, weights W       p_scale, w_scale    largest |entry| of the packed model          -> [2^12, 2^13)
//   pose feature R - I                   PNDF_LBS_PF_SCALE   |R - I| <= 2                                 -> <= 2^13
//   joint transforms A = [G_R | A_t]     a_scale             max(1, sum of the bone lengths + max |J|)    -> [2^12, 2^13)
//   T_R^T d L / d verts                  g_scale             3 max_v sum_j |W| (2 w_temp + w_data)        -> [2^13, 2^14)
//   d L / d verts (x) [v_posed, 1]       x_scale             (2 w_temp + w_data) max(1, vp_bound)         -> [2^13, 2^14)
// with |d L / d verts| <= 2 w_temp + w_data per component (two pairs share a vertex; the data term touches the picked
// vertices) and |v_posed| <= vp_bound = max_v,c |v_shaped| + 2 sum_k |P|.  An operand above its bound would saturate silently
// (the device-side split rounds toward zero), one far below it loses its lo half to fp16 subnormals.
#pragma once
#include <cmath>

#include "pndf_lbs_split.h"

// power of two s with bound * s in [2^13, 2^14): the operand's hi half cannot overflow (65504), and values down to 2^-16 of
// the bound keep a normal lo half.  Clamped: a zero bound must not turn into an infinite factor.
static inline float pndf_lbs_scale_for(float bound) {
    if (!(bound > 1e-30f)) bound = 1e-30f;
    if (bound > 1e30f) bound = 1e30f;
    return std::ldexp(1.0f, 13 - std::ilogb(bound));
}

struct PndfLbsScales {
    float p_scale = 1.f, w_scale = 1.f, a_scale = 1.f;      // the model's part: set once
    float g_scale = 1.f, x_scale = 1.f;                     // the term weights' part: set per launch
    // the bounds they come from
    float max_p = 0.f, max_w = 0.f;   // largest |entry| of P and of W
    float w_rowsum = 1.f;             // max_v sum_j |W[v, j]|, at least 1e-6                  (bounds |T_R^T g|)
    float vp_bound = 1.f;             // max_v,c |v_shaped| + 2 sum_k |posedirs|, at least 1   (bounds |v_posed|)
    float a_bound = 1.f;              // max(1, sum of the bone lengths + max_j |J_j|)          (bounds |A|)
    float g_bound = 0.f, x_bound = 0.f;
    float pf_scale = PNDF_LBS_PF_SCALE;      // the pose feature's: a constant
};
constexpr int PNDF_LBS_SCALES_FLOATS = 13;      // pndf_debug_lbs_scales: the fields above in this order

// `blob` (pndf_lbs_pack_host: [NG][PNDF_LBS_BLOB_FLOATS]) with the rest joints `J`, `rel` [24][3]: the model's part is
// (re)computed; blob == nullptr keeps it.  The weights' part is computed from s's bounds either way; w_temp, w_data are the
// weights over the means (pndf_lbs_terms_grad_w), 0 where no term runs.
static inline void pndf_lbs_select_scales(PndfLbsScales& s, const float* blob, int NG, const float* J, const float* rel,
                                          float w_temp, float w_data) {
    constexpr int NJ = PNDF_LBS_J, PF = PNDF_LBS_PF, GV = PNDF_LBS_GV, C_STRIDE = PNDF_LBS_PF * PNDF_LBS_GV;
    if (blob) {
        float maxP = 0.f, maxW = 0.f, rowsum = 0.f, vpb = 0.f;
        for (int grp = 0; grp < NG; ++grp) {
            const float* b = blob + (size_t)grp * PNDF_LBS_BLOB_FLOATS;
            for (int vi = 0; vi < GV; ++vi) {
                float ws = 0.f;
                for (int j = 0; j < NJ; ++j) {
                    const float w = std::fabs(b[PNDF_LBS_BLOB_W + j * GV + vi]);
                    ws += w;
                    maxW = std::fmax(maxW, w);
                }
                rowsum = std::fmax(rowsum, ws);
                for (int c = 0; c < 3; ++c) {
                    float ps = 0.f;
                    for (int k = 0; k < PF; ++k) {
                        const float pv = std::fabs(b[PNDF_LBS_BLOB_P + c * C_STRIDE + k * GV + vi]);
                        ps += pv;
                        maxP = std::fmax(maxP, pv);
                    }
                    vpb = std::fmax(vpb, std::fabs(b[PNDF_LBS_BLOB_VS + c * GV + vi]) + 2.0f * ps);      // |R - I| <= 2
                }
            }
        }
        float extent = 0.f, maxJ = 0.f;      // |G_t[j]| <= sum of the bone lengths, |A_t| <= |G_t| + |J|
        for (int j = 0; j < NJ; ++j) {
            extent += std::sqrt(rel[3 * j] * rel[3 * j] + rel[3 * j + 1] * rel[3 * j + 1] + rel[3 * j + 2] * rel[3 * j + 2]);
            maxJ = std::fmax(maxJ, std::sqrt(J[3 * j] * J[3 * j] + J[3 * j + 1] * J[3 * j + 1] + J[3 * j + 2] * J[3 * j + 2]));
        }
        s.max_p = maxP;
        s.max_w = maxW;
        s.w_rowsum = std::fmax(rowsum, 1e-6f);
        s.vp_bound = std::fmax(vpb, 1.0f);
        s.a_bound = std::fmax(1.0f, extent + maxJ);
        s.p_scale = pndf_lbs_scale_for(maxP) * 0.5f;
        s.w_scale = pndf_lbs_scale_for(maxW) * 0.5f;
        s.a_scale = pndf_lbs_scale_for(s.a_bound) * 0.5f;
    }
    const float gb = 2.0f * std::fabs(w_temp) + std::fabs(w_data);
    s.g_bound = 3.0f * s.w_rowsum * gb;
    s.x_bound = gb * s.vp_bound;
    s.g_scale = pndf_lbs_scale_for(s.g_bound);
    s.x_scale = pndf_lbs_scale_for(s.x_bound);
}
