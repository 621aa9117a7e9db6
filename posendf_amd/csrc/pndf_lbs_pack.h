// Host side of the body model (pndf_lbs.hip) that needs no device: the packers behind pndf_lbs_pack_host and
// pndf_lbs_pack_split_host, and the picked-joint table of the joints-only forward.  Plain C++17, no HIP: pndf_lbs_create runs
// all of it before its first device call, and tests/host/lbs_pack_check.cpp checks it as a stand-alone host program.
#pragma once
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../include/posendf_amd.h"
#include "pndf_args.h"
#include "pndf_lbs_scales.h"
#include "pndf_lbs_split.h"

namespace pndf_lbs {

constexpr int NJ = PNDF_LBS_J, PF = PNDF_LBS_PF, GV = PNDF_LBS_GV, BLOB = PNDF_LBS_BLOB_FLOATS;
constexpr int C_STRIDE = PF * GV;          // floats per component of P in a blob (3328)
constexpr int PICK_FLOATS = 3 + NJ + 3 * 9 * (NJ - 1);      // per picked vertex: v_shaped [3] | weights [24] | pose blend shapes [207][3]

// fp32 -> fp16 bits, round to nearest even (host side of the split: any hi + lo = x decomposition serves the kernels)
static inline uint16_t f32_to_f16(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                          // >= 65520: inf
    if (x < 0x38800000u) {                                                            // below 2^-14: subnormal, units of 2^-24
        float af;
        memcpy(&af, &x, 4);
        return (uint16_t)(sign | (uint16_t)std::nearbyint((double)af * 16777216.0));
    }
    uint32_t h = (((x >> 23) - 112u) << 10) | ((x & 0x7fffffu) >> 13);
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;                           // (a carry runs into the exponent)
    return (uint16_t)(sign | h);
}
static inline float f16_to_f32(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 1023;
    const float v = (e == 0) ? std::ldexp((float)m, -24) : std::ldexp((float)(m | 1024), e - 25);
    return (h & 0x8000u) ? -v : v;
}

// the split-precision model from the fp32 one (same [row][16 v] order inside a plane)
static inline void lbs_pack_split(const float* blob, int NG, float p_scale, float w_scale, uint8_t* out) {
    memset(out, 0, (size_t)NG * PNDF_LBS_SB_BYTES);
    for (int grp = 0; grp < NG; ++grp) {
        const float* b = blob + (size_t)grp * BLOB;
        uint8_t* o = out + (size_t)grp * PNDF_LBS_SB_BYTES;
        auto put = [&](int hi_off, int lo_off, int row, int vi, float x) {
            const uint16_t h = f32_to_f16(x);
            const uint16_t l = f32_to_f16(x - f16_to_f32(h));
            memcpy(o + hi_off + pndf_lbs_sb_at(row, vi), &h, 2);
            memcpy(o + lo_off + pndf_lbs_sb_at(row, vi), &l, 2);
        };
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < PF; ++k)
                for (int vi = 0; vi < GV; ++vi)
                    put(PNDF_LBS_SB_PH + c * PNDF_LBS_SB_PLANE, PNDF_LBS_SB_PL + c * PNDF_LBS_SB_PLANE, k, vi,
                        b[PNDF_LBS_BLOB_P + c * C_STRIDE + k * GV + vi] * p_scale);
        for (int j = 0; j < 32; ++j)
            for (int vi = 0; vi < GV; ++vi)
                put(PNDF_LBS_SB_WH, PNDF_LBS_SB_WL, j, vi, b[PNDF_LBS_BLOB_W + j * GV + vi] * w_scale);
        memcpy(o + PNDF_LBS_SB_VS, b + PNDF_LBS_BLOB_VS, 3 * GV * 4);
        memcpy(o + PNDF_LBS_SB_FL, b + PNDF_LBS_BLOB_FL, GV * 4);
    }
}

// pndf_lbs_pack_host: the model in MFMA tile order + the rest joints.  `J_out` (72 floats) and `rel_out` (72 floats) may be
// null.  Returns 0 or a negative pndf_status; a refusal writes nothing.
static inline int lbs_pack(int32_t V, int32_t NB, const float* v_template, const float* shapedirs, const float* betas,
                           const float* posedirs, const float* J_regressor, const int32_t* parents, const float* lbs_weights,
                           const int32_t* extra_joint_vertex, int32_t n_extra, float* blob, float* J_out, float* rel_out) {
    if (V < 1 || NB < 0 || !v_template || !posedirs || !J_regressor || !parents || !lbs_weights || !blob) return PNDF_ERR_BAD_ARG;
    if (NB > 0 && (!shapedirs || !betas)) return PNDF_ERR_BAD_ARG;
    if (n_extra < 0 || n_extra > PNDF_LBS_MAX_EXTRA || (n_extra > 0 && !extra_joint_vertex)) return PNDF_ERR_BAD_ARG;
    if (parents[0] >= 0) return PNDF_ERR_UNSUPPORTED;
    for (int j = 1; j < NJ; ++j)
        if (parents[j] < 0 || parents[j] >= j) return PNDF_ERR_UNSUPPORTED;      // parents precede their children (SMPL)
    for (int e = 0; e < n_extra; ++e)
        if (extra_joint_vertex[e] < 0 || extra_joint_vertex[e] >= V) return PNDF_ERR_BAD_ARG;
    // v_shaped = v_template + blend_shapes(betas, shapedirs); J = J_regressor v_shaped   (smplx lbs(), first two steps)
    std::vector<float> vsh((size_t)V * 3);
    for (int i = 0; i < V * 3; ++i) {
        double acc = v_template[i];
        for (int l = 0; l < NB; ++l) acc += (double)shapedirs[(size_t)i * NB + l] * betas[l];
        vsh[i] = (float)acc;
    }
    float J[NJ][3];
    for (int j = 0; j < NJ; ++j)
        for (int e = 0; e < 3; ++e) {
            double acc = 0.0;
            for (int v = 0; v < V; ++v) acc += (double)J_regressor[(size_t)j * V + v] * vsh[(size_t)v * 3 + e];
            J[j][e] = (float)acc;
        }
    const int NG = (V + GV - 1) / GV;
    std::vector<int> flag((size_t)NG * GV, -2);
    for (int v = 0; v < V; ++v) flag[v] = -1;
    // The vertex kernels find a vertex-picked joint through this per-vertex flag, i.e. one joint per vertex: a vertex named
    // twice would leave the earlier joint's row unwritten (smplx's VertexJointSelector is an index_select and would serve
    // both).  SMPL's own table has no duplicates; anything else is refused rather than half served.
    for (int e = 0; e < n_extra; ++e) {
        if (flag[extra_joint_vertex[e]] >= 0) return PNDF_ERR_BAD_ARG;
        flag[extra_joint_vertex[e]] = e;
    }
    for (int j = 0; j < NJ; ++j)
        for (int e = 0; e < 3; ++e) {
            if (J_out) J_out[3 * j + e] = J[j][e];
            if (rel_out) rel_out[3 * j + e] = (j == 0) ? J[j][e] : J[j][e] - J[parents[j]][e];
        }
    memset(blob, 0, (size_t)NG * BLOB * sizeof(float));
    const int npf = 9 * (NJ - 1);
    for (int grp = 0; grp < NG; ++grp) {
        float* b = blob + (size_t)grp * BLOB;
        for (int vi = 0; vi < GV; ++vi) {
            const int v = grp * GV + vi;
            ((int*)(b + PNDF_LBS_BLOB_FL))[vi] = flag[(size_t)grp * GV + vi];
            if (v >= V) continue;
            for (int c = 0; c < 3; ++c) {
                for (int k = 0; k < npf; ++k)
                    b[PNDF_LBS_BLOB_P + c * C_STRIDE + k * GV + vi] = posedirs[(size_t)k * V * 3 + (size_t)v * 3 + c];
                b[PNDF_LBS_BLOB_VS + c * GV + vi] = vsh[(size_t)v * 3 + c];
            }
            for (int j = 0; j < NJ; ++j) b[PNDF_LBS_BLOB_W + j * GV + vi] = lbs_weights[(size_t)v * NJ + j];
        }
    }
    return PNDF_OK;
}

// pndf_lbs_pack_split_host: the split-precision model (what pndf_lbs_create uploads for PNDF_LBS_F16X3) from the fp32 one
// of lbs_pack.  scales_out (may be null): p_scale, w_scale.
static inline int lbs_pack_split_host(int32_t V, const float* blob, void* sblob, float* scales_out) {
    if (V < 1 || !blob || !sblob) return PNDF_ERR_BAD_ARG;
    const int NG = (V + GV - 1) / GV;
    PndfLbsScales sc;      // (p_scale and w_scale depend on the blob alone: no rest joints needed)
    const float no_joints[NJ * 3] = {};
    pndf_lbs_select_scales(sc, blob, NG, no_joints, no_joints, 0.f, 0.f);
    lbs_pack_split(blob, NG, sc.p_scale, sc.w_scale, (uint8_t*)sblob);
    if (scales_out) { scales_out[0] = sc.p_scale; scales_out[1] = sc.w_scale; }
    return PNDF_OK;
}

// the picked vertices' own rows of a packed model, [n_extra][PICK_FLOATS], for the joints-only forward: copies of what
// lbs_pack wrote for vertex v into group v / 16, slot v % 16 (vertices as lbs_pack accepted them)
static inline void lbs_picked_table(const float* blob, const int32_t* extra_joint_vertex, int n_extra, float* out) {
    for (int x = 0; x < n_extra; ++x) {
        const float* b = blob + (size_t)(extra_joint_vertex[x] / GV) * BLOB;
        const int vi = extra_joint_vertex[x] % GV;
        float* P = out + (size_t)x * PICK_FLOATS;
        for (int c = 0; c < 3; ++c) P[c] = b[PNDF_LBS_BLOB_VS + c * GV + vi];
        for (int j = 0; j < NJ; ++j) P[3 + j] = b[PNDF_LBS_BLOB_W + j * GV + vi];
        for (int k = 0; k < 9 * (NJ - 1); ++k)
            for (int c = 0; c < 3; ++c) P[3 + NJ + 3 * k + c] = b[PNDF_LBS_BLOB_P + c * C_STRIDE + k * GV + vi];
    }
}

}  // namespace pndf_lbs
