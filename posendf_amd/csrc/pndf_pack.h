// Host-side packing helpers shared by the C-ABI translation units (pndf_capi.hip: the amass.yaml streams; pndf_generic.hip:
// runtime-planned networks): logical matrix views and the lane-linear 16 x 16 tile both kernel families read.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pndf_layout.h"

namespace pndf_pack {
using namespace pndf;
#define PNDF_PACK_LOCAL __attribute__((visibility("hidden")))      // (not an export of the library)

// Behind a step's stream sits a replica of its first slots, so that the ring's fetch offset never wraps inside a step: as many
// slots as the ring fetches ahead (pndf_device.h: RING_SLOTS - 1; 5 covers the six-buffer experiment arm as well).
constexpr int STREAM_PAD_SLOTS = 5;
static_assert(STREAM_PAD_SLOTS >= PNDF_RING_SLOTS - 1, "the replica covers the ring's prefetch distance");

struct Mat {          // logical matrix view M[r][c] of dfnet.lin{l}.weight, optionally transposed, zero padded
    const float* w;   // (out, in) row-major
    int out, in;
    bool transposed;
    float at(int r, int c) const {
        const int o = transposed ? c : r, i = transposed ? r : c;
        return (o < out && i < in) ? w[(size_t)o * in + i] : 0.f;
    }
};

// tile(M, nt, kt)[lane*4 + s] = M[16 nt + (lane & 15)][16 kt + 4 (lane >> 4) + s]   (pndf_layout.h)
inline void emit_tile(const Mat& m, int nt, int kt, float* dst) {
    for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s) dst[lane * 4 + s] = m.at(16 * nt + (lane & 15), 16 * kt + 4 * (lane >> 4) + s);
}

// Exact power-of-two scaling of a layer's weights for the split-precision streams (pndf_kernel_split.hip, "operand scaling"): the
// weights travel as s W with s = the power of two that brings the layer's largest |weight| into [2^12, 2^13) -- the hi halves cannot
// overflow and the lo halves of all weights down to 2^-14 of the largest stay in fp16's normal range.  False: the layer has no
// finite non-zero weight and cannot be scaled.
PNDF_PACK_LOCAL inline bool layer_scale(const float* w, int64_t n, float* scale) {
    float mx = 0.f;
    bool nan = false;
    for (int64_t i = 0; i < n; ++i) {
        const float a = fabsf(w[i]);
        nan |= (a != a);
        if (a > mx) mx = a;
    }
    if (nan || !(mx > 0x1p-100f && mx < 0x1p100f)) return false;
    int e;
    (void)frexpf(mx, &e);                  // mx = f * 2^e, f in [0.5, 1)
    *scale = ldexpf(1.0f, 13 - e);         // s * mx in [2^12, 2^13)
    return true;
}

// fp32 -> bfloat16 bits, round to nearest even (the packers' inputs are finite: a layer that is not has no layer_scale)
PNDF_PACK_LOCAL inline uint16_t bf16_bits(float w) {
    const uint32_t u = __builtin_bit_cast(uint32_t, w);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// split-precision block (pndf_layout.h "split-precision stream"): hi tile then lo tile of (16 rows x 32 k), 8 halfs per lane each,
//   block(M, nt, kb)[lane * 8 + jj] = scale * M[16 nt + (lane & 15)][16 (2 kb + (jj >> 2)) + 4 (lane >> 4) + (jj & 3)]
// hi = the value rounded to nearest even, lo = the remainder rounded to nearest; returns whether any lo half is non-zero.
// `bf16` (precision bf16, the one-term comparison kernel): the hi tile holds bfloat16 bits, the lo tile zeros.
PNDF_PACK_LOCAL inline bool emit_pair_f16(const Mat& m, int nt, int kb, float scale, float* dst, bool bf16 = false) {
    _Float16* hi = (_Float16*)dst;
    _Float16* lo = (_Float16*)(dst + TILE_FLOATS);
    bool any_lo = false;
    for (int lane = 0; lane < 64; ++lane)
        for (int jj = 0; jj < 8; ++jj) {
            const float w = scale * m.at(16 * nt + (lane & 15), 16 * (2 * kb + (jj >> 2)) + 4 * (lane >> 4) + (jj & 3));
            _Float16& h = hi[lane * 8 + jj];
            _Float16& l = lo[lane * 8 + jj];
            if (bf16) {
                h = __builtin_bit_cast(_Float16, bf16_bits(w));
                l = (_Float16)0;
                continue;
            }
            h = (_Float16)w;
            l = (_Float16)(w - (float)h);
#ifdef PNDF_EXP_LO_BITS                     // (energy experiment, profiles/r05/energy_breakdown.txt: the lo half keeps this many
            {                               // explicit mantissa bits -- does the matrix pipe pay for operand bits that toggle?)
                uint16_t u = __builtin_bit_cast(uint16_t, l);
                const int drop = 10 - PNDF_EXP_LO_BITS;
                u = (uint16_t)((u + (1u << (drop - 1))) & ~((1u << drop) - 1));
                l = __builtin_bit_cast(_Float16, u);
            }
#endif
            any_lo |= (l != (_Float16)0);
        }
    return any_lo;
}

// 16x16 logical matrices of one encoder joint (zero padded), see pndf_layout.h "encoder on the MFMA pipe"
struct EncMat {
    const float* w1;   // [10][in]
    const float* w2;   // [6][10]
    int in;
    int kind;          // 0: W1 (rows = hidden, k = input)   1: W2 (rows 4..9 = feature, k = hidden)
                       // 2: W2^T (rows = hidden, k = feature row 4..9)   3: W1^T (rows = input, k = hidden)
    float at(int r, int c) const {
        switch (kind) {
            case 0: return (r < HID && c < in) ? w1[r * in + c] : 0.f;
            case 1: return (r >= ENC_FEAT_ROW && r < ENC_FEAT_ROW + FEAT && c < HID) ? w2[(r - ENC_FEAT_ROW) * HID + c] : 0.f;
            case 2: return (r < HID && c >= ENC_FEAT_ROW && c < ENC_FEAT_ROW + FEAT) ? w2[(c - ENC_FEAT_ROW) * HID + r] : 0.f;
            default: return (r < in && c < HID) ? w1[c * in + r] : 0.f;
        }
    }
};
inline void emit_enc_tile(const EncMat& m, float* dst) {
    for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s) dst[lane * 4 + s] = m.at(lane & 15, 4 * (lane >> 4) + s);
}

// the encoder's two stream sections: forward = joint order, W1 then W2; backward = reverse joint order, W2^T then W1^T.
// `tensors`: the 84 encoder tensors in state-dict order; each destination holds ENC_TILES (42) tiles.
inline void emit_encoder_sections(const float* const* tensors, float* fwd, float* bwd) {
    for (int j = 0; j < NJ; ++j)
        for (int kind = 0; kind < 2; ++kind, fwd += TILE_FLOATS)
            emit_enc_tile(EncMat{tensors[4 * j], tensors[4 * j + 2], enc_in(j), kind}, fwd);
    for (int j = NJ - 1; j >= 0; --j)
        for (int kind = 2; kind < 4; ++kind, bwd += TILE_FLOATS)
            emit_enc_tile(EncMat{tensors[4 * j], tensors[4 * j + 2], enc_in(j), kind}, bwd);
}

// the encoder's rows of the bias block: per joint b1 padded to 16, b2 on rows 4..9 of 16
PNDF_PACK_LOCAL inline void emit_encoder_biases(const float* const* tensors, float* bias) {
    for (int j = 0; j < NJ; ++j) {
        memcpy(bias + ENCB_OFF + 32 * j, tensors[4 * j + 1], sizeof(float) * HID);
        memcpy(bias + ENCB_OFF + 32 * j + 16 + ENC_FEAT_ROW, tensors[4 * j + 3], sizeof(float) * FEAT);
    }
}

#undef PNDF_PACK_LOCAL
}  // namespace pndf_pack
