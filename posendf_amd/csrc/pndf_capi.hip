// C ABI of the Pose-NDF engine (include/posendf_amd.h): handle management, weight packing, launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/posendf_amd.h"
#include "pndf_layout.h"
#include "pndf_args.h"
#include "pndf_host.h"
#include "pndf_net_plan.h"
#include "pndf_pack.h"
#include "pndf_generic.h"
#include "pndf_project_opts.h"
#include "pndf_complete.h"
#include "pndf_interp.h"

using namespace pndf;

extern "C" __global__ void pndf_fused_relu_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_softplus_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_split_relu_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_split_softplus_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_split2_relu_kernel(PndfKernelArgs args);        // pndf_kernel_split_x2.hip
extern "C" __global__ void pndf_fused_split2_softplus_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_half_relu_kernel(PndfKernelArgs args);
extern "C" __global__ void pndf_fused_bf16_relu_kernel(PndfKernelArgs args);     // pndf_kernel_bf16.hip
extern "C" long long pndf_kernel_softplus_scratch_floats_per_wg();
extern "C" int pndf_kernel_lds_bytes();


// The limits and the SMPL table are written down where each reader needs them -- pndf_layout.h for the fused kernels, pndf_args.h for the
// runtime-planned kernels' arguments, pndf_net_plan.h for what the library accepts; this translation unit sees all three.
static_assert(MAXLIN == PNDF_NET_MAX_LIN && PNDF_GEN_MAXLIN == PNDF_NET_MAX_LIN && MAX_WIDTH == PNDF_NET_MAX_WIDTH, "one depth and one width limit");
static_assert(NJ == PNDF_SMPL_JOINTS && FEAT == PNDF_SKEL_FEAT && HID == PNDF_SKEL_HID && NQ == PNDF_SKEL_BONE * NJ && NFEAT == DIMS[0] &&
                  DIMS[0] == PNDF_SKEL_FEAT * NJ && NOENC_IN == PNDF_SKEL_BONE * NJ && NJ <= PNDF_SKEL_MAX_JOINTS,
              "one bone: 4 | 10 -> 10 -> 6, 21 of them");
constexpr bool smpl_tables_agree() {
    for (int j = 0; j < NJ; ++j)
        if (PARENT[j] != PNDF_SMPL_PARENT[j]) return false;
    return true;
}
static_assert(smpl_tables_agree(), "pndf_layout.h's PARENT is pndf_skeleton_is_smpl's table");

struct pndf_engine {
    LayerNet net;               // the network and the device (pndf_net_plan.h): SMPL's 21 joints, dims[0] 126 | 84
    int precision = PNDF_PREC_FP32;
    bool have_weights = false;
    // f16x3 only: every lo tile of the packed trunk is zero (weights exactly representable in fp16 at their layer scale),
    // so the lo hi term vanishes identically and the two-term kernels give bit-identical results with 2/3 of the MFMAs
    bool lo_all_zero = false;
    char* d_stream = nullptr;   // STEP_TILES KiB + a replica of the first STREAM_PAD_SLOTS slots (the ring never wraps)
    float* d_bias = nullptr;
    // softplus: fp32 derivative scratch, one block per RESIDENT workgroup (= per CU: the kernels take a whole CU each
    // and walk the 64-pose blocks with a grid-stride loop), allocated once in pndf_create.  Launches of one handle share
    // it, so launches on different streams are ordered with an event (sp_order, pndf_host.h).
    float* d_scratch = nullptr;
    int resident_wgs = 0;
    PndfScratchOrder sp_order;
    // any DFNet that is not shaped like configs/amass.yaml (another depth, wider layers): the runtime-planned path, pndf_generic.hip
    PndfGeneric* generic = nullptr;
    std::string err;
};

using pndf_pack::STREAM_PAD_SLOTS;

// The fused kernels, and the one a handle launches: by precision, activation family and (f16x3) whether every lo tile is zero
typedef void (*fused_kernel_t)(PndfKernelArgs);
struct FusedKernel {
    fused_kernel_t fn;
    const char* name;
};
#define PNDF_FUSED(k) {k, #k}
static const FusedKernel FUSED_KERNELS[8] = {
    PNDF_FUSED(pndf_fused_relu_kernel),       PNDF_FUSED(pndf_fused_softplus_kernel),       PNDF_FUSED(pndf_fused_split_relu_kernel),
    PNDF_FUSED(pndf_fused_split_softplus_kernel), PNDF_FUSED(pndf_fused_split2_relu_kernel), PNDF_FUSED(pndf_fused_split2_softplus_kernel),
    PNDF_FUSED(pndf_fused_half_relu_kernel),  PNDF_FUSED(pndf_fused_bf16_relu_kernel)};
#undef PNDF_FUSED
static const FusedKernel& fused_kernel(int precision, bool softplus, bool lo_all_zero) {
    switch (precision) {
        case PNDF_PREC_F16X3: return FUSED_KERNELS[(lo_all_zero ? 4 : 2) + softplus];
        case PNDF_PREC_F16: return FUSED_KERNELS[6];
        case PNDF_PREC_BF16: return FUSED_KERNELS[7];
        default: return FUSED_KERNELS[softplus];
    }
}

// The lab is quarantined from the product (pndf_experiment.h): every translation unit exports one word with a bit per tuning /
// ablation macro that differs from its product default; a product library reports 0.
PNDF_EXPORT_EXPERIMENT_WORD(capi)
extern "C" {
extern const unsigned pndf_experiment_word_fp32, pndf_experiment_word_split, pndf_experiment_word_split_x2, pndf_experiment_word_lbs,
    pndf_experiment_word_generic, pndf_experiment_word_bf16;
}
extern "C" unsigned pndf_experiment_word(void) {
    return pndf_experiment_word_capi | pndf_experiment_word_fp32 | pndf_experiment_word_split | pndf_experiment_word_split_x2 |
           pndf_experiment_word_lbs | pndf_experiment_word_generic | pndf_experiment_word_bf16;
}
extern "C" const char* pndf_version(void) {
    static const std::string v = [] {
        char w[16];
        snprintf(w, sizeof w, "0x%08x", pndf_experiment_word());
        return std::string("posendf_amd 0.4 (gfx950; fp32 MFMA 16x16x4 and split-fp16 MFMA 16x16x32; relu, lrelu, softplus; experiments=") + w + ")";
    }();
    return v.c_str();
}

extern "C" const char* pndf_last_error(pndf_handle h) { return pndf_last_error_of(h); }

extern "C" void pndf_default_config(pndf_config* cfg, int32_t act, float beta) {
    memset(cfg, 0, sizeof(*cfg));
    cfg->act = act;
    cfg->beta = beta;
    cfg->num_joints = NJ;
    cfg->n_dims = NLIN + 1;
    for (int i = 0; i <= NLIN; ++i) cfg->dims[i] = DIMS[i];
    for (int i = 0; i < NJ; ++i) cfg->parent[i] = PARENT[i];
    cfg->precision = PNDF_PREC_FP32;
    cfg->enc_act = -1;      // the same activation as the trunk (every config of the reference)
    cfg->enc_beta = 0.f;
}

static int check_config(pndf_engine* h, const pndf_config* cfg) {
    if (!cfg) return pndf_fail(h, PNDF_ERR_BAD_ARG, "cfg is null");
    // What the library accepts of a DFNet and its activations is pndf_net_plan.h's; the engine's own rules are the SMPL table, an input
    // of 126 | 84, the precisions and the Softplus betas.  Which kernels run an accepted network is pndf_generic_needed's decision.
    if (!pndf_skeleton_is_smpl(cfg))
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "num_joints / parent: the persistent engine runs the 21-joint table of get_parent_mapping('smpl') only; pndf_skel_create (posendf_amd_skeleton.h) takes any joint tree");
    if (const char* why = pndf_dfnet_refusal(cfg)) return pndf_fail(h, PNDF_ERR_UNSUPPORTED, why);
    if (cfg->dims[0] != DIMS[0] && cfg->dims[0] != NOENC_IN)
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "DFNet in_dim (dims[0]) must be 126 (StrEnc.use=True) or 84 (False)");
    if (cfg->act == PNDF_ACT_SOFTPLUS && !(cfg->beta > 0.f))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "softplus beta must be positive");
    if (cfg->enc_act == PNDF_ACT_SOFTPLUS && !(cfg->enc_beta > 0.f) && !(cfg->beta > 0.f))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "softplus beta of the encoder must be positive");
    if (cfg->precision != PNDF_PREC_FP32 && cfg->precision != PNDF_PREC_F16X3 && cfg->precision != PNDF_PREC_F16 &&
        cfg->precision != PNDF_PREC_BF16)
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "unknown precision (fp32, f16x3, f16 and bf16 are implemented)");
    if ((cfg->precision == PNDF_PREC_F16 || cfg->precision == PNDF_PREC_BF16) && cfg->act == PNDF_ACT_SOFTPLUS)
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "the plain-f16 / plain-bf16 comparison kernels implement relu / lrelu only");
    return PNDF_OK;
}

extern "C" int pndf_create(pndf_handle* out, const pndf_config* cfg, int device) {
    if (!out) return pndf_fail<pndf_engine>(nullptr, PNDF_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    int rc = check_config(nullptr, cfg);
    if (rc) return rc;
    const PndfDeviceCheck dev = pndf_check_gfx950(device, "the engine", true);
    if (dev.code != PNDF_OK) return pndf_fail<pndf_engine>(nullptr, dev.code, dev.text);
    const hipDeviceProp_t& prop = dev.prop;
    DeviceGuard guard(device);
    if (!guard.ok) return pndf_fail<pndf_engine>(nullptr, PNDF_ERR_HIP, "hipSetDevice failed");
    pndf_engine* h = new pndf_engine();
    layer_net_init(h->net, cfg, device);
    h->precision = cfg->precision;
    if (prop.multiProcessorCount <= 0) {
        delete h;
        return pndf_fail<pndf_engine>(nullptr, PNDF_ERR_HIP, "the device reports no compute units (multiProcessorCount <= 0)");
    }
    h->resident_wgs = prop.multiProcessorCount;
    if (pndf_generic_needed(*cfg)) {
        if (cfg->precision == PNDF_PREC_BF16) {
            delete h;
            return pndf_fail<pndf_engine>(nullptr, PNDF_ERR_UNSUPPORTED, "the plain-bf16 comparison kernel exists for amass.yaml-shaped networks only "
                                                       "(the runtime-planned kernels run fp32 or split-precision fp16)");
        }
        std::string why;
        rc = pndf_generic_create(&h->generic, h->net, h->precision, h->resident_wgs, why);
        if (rc != PNDF_OK) {
            delete h;
            return pndf_fail<pndf_engine>(nullptr, rc, why);
        }
        *out = h;
        return PNDF_OK;
    }
    hipError_t e = hipMalloc((void**)&h->d_stream, (size_t)(STEP_TILES + STREAM_PAD_SLOTS * SLOT_TILES) * TILE_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_bias, BIAS_FLOATS * sizeof(float));
    if (e == hipSuccess && cfg->act == PNDF_ACT_SOFTPLUS) {
        e = hipMalloc((void**)&h->d_scratch, (size_t)h->resident_wgs * pndf_kernel_softplus_scratch_floats_per_wg() * sizeof(float));
        if (e == hipSuccess) e = h->sp_order.create();
    }
    for (const FusedKernel& k : FUSED_KERNELS)
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, pndf_kernel_lds_bytes());
    if (e != hipSuccess) {
        std::string m = std::string("pndf_create: ") + hipGetErrorString(e);
        pndf_destroy(h);
        return pndf_fail<pndf_engine>(nullptr, PNDF_ERR_HIP, m);
    }
    *out = h;
    return PNDF_OK;
}

extern "C" int pndf_destroy(pndf_handle h) {
    if (!h) return PNDF_OK;
    DeviceGuard guard(h->net.device);
    pndf_generic_destroy(h->generic);
    h->sp_order.destroy();
    if (h->d_stream) (void)hipFree(h->d_stream);
    if (h->d_bias) (void)hipFree(h->d_bias);
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    delete h;
    return PNDF_OK;
}

// ------------------------------------------------------------------------------------------ packing
// (Mat / emit_tile / emit_pair_f16 / the encoder's sections and biases / layer_scale: pndf_pack.h, shared with pndf_generic.hip)
using pndf_pack::Mat;
using pndf_pack::emit_tile;

extern "C" void pndf_packed_sizes(int64_t* stream_floats, int64_t* bias_floats) {
    if (stream_floats) *stream_floats = (int64_t)STEP_TILES * TILE_FLOATS;
    if (bias_floats) *bias_floats = BIAS_FLOATS;
}

// The stateless packers have no handle, so the table brings its own plan: 98 tensors come with the structure encoder (in_dim 126), 14
// without it (84 = 21 x 4, model.StrEnc.use = False: DFNet sees the normalised quaternions, reference model/posendf.py:40-42,73-74),
// and the bias lengths are the layer widths -- at most configs/amass.yaml's, narrower layers travel zero padded.  Against that plan
// the table is checked like any other.  Does it fit?
static bool table_plan(const float* const* tensors, const int64_t* numel, int n, LayerNet& net) {
    if (!tensors || !numel || (n != 4 * NJ + 2 * NLIN && n != 2 * NLIN)) return false;
    pndf_config cfg;
    pndf_default_config(&cfg, PNDF_ACT_RELU, 0.f);
    cfg.dims[0] = n == 2 * NLIN ? NOENC_IN : DIMS[0];
    for (int l = 0; l < NLIN; ++l) {
        const int64_t out = numel[n - 2 * (NLIN - l) + 1];
        if (out < 1 || out > DIMS[l + 1] || (l == NLIN - 1 && out != 1)) return false;
        cfg.dims[l + 1] = (int)out;
    }
    layer_net_init(net, &cfg, -1);
    return !pndf_table_fault(net, tensors, numel, n);
}

// a table that fits `net` (SMPL, amass.yaml's depth, no layer wider than amass.yaml's) -> the fp32 stream and the bias block
static int pack_fp32(const float* const* tensors, const LayerNet& nd, float* stream, float* bias) {
    // ---- bias block: b0..b5 | w6 | b6 | per joint: b1 padded to 16, b2 on rows 4..9 of 16
    memset(bias, 0, BIAS_FLOATS * sizeof(float));
    for (int l = 0; l < 8; ++l) bias[SCALE_OFF + l] = 1.0f;
    const bool enc = nd.encoder;      // without the encoder its tiles / biases stay zero (skipped on chip)
    const float* const* lin = tensors + (enc ? 4 * NJ : 0);
    for (int l = 0; l < NLIN - 1; ++l) memcpy(bias + BIAS_OFF[l], lin[2 * l + 1], sizeof(float) * nd.out(l));   // narrower layers: zero padded
    memcpy(bias + W6_OFF, lin[2 * (NLIN - 1)], sizeof(float) * nd.in(NLIN - 1));
    bias[BIAS_OFF[NLIN - 1]] = lin[2 * (NLIN - 1) + 1][0];
    if (enc) pndf_pack::emit_encoder_biases(tensors, bias);
    // ---- stream: encoder forward tiles | trunk phases | encoder backward tiles, in consumption order
    memset(stream, 0, (size_t)STEP_TILES * TILE_FLOATS * sizeof(float));
    float* dst = stream + (size_t)ENC_TILES_PADDED * TILE_FLOATS;
    for (int ph = 0; ph < 6; ++ph) {
        const Phase& P = PHASES[ph];
        const Mat A{lin[2 * P.a_lin], nd.out(P.a_lin), nd.in(P.a_lin), P.transposed};
        const Mat B{lin[2 * P.b_lin], nd.out(P.b_lin), nd.in(P.b_lin), P.transposed};
        for (int c = 0; c < P.NC; ++c) {
            for (int kt = 0; kt < P.KA; ++kt)                       // part A: (kt, ci)
                for (int ci = 0; ci < P.CT; ++ci, dst += TILE_FLOATS) emit_tile(A, c * P.CT + ci, kt, dst);
            for (int nbp = 0; nbp < P.NB / 2; ++nbp)                // part B: (nbp, ci, h)
                for (int ci = 0; ci < P.CT; ++ci)
                    for (int hh = 0; hh < 2; ++hh, dst += TILE_FLOATS) emit_tile(B, 2 * nbp + hh, c * P.CT + ci, dst);
        }
    }
    if (dst - stream != (ptrdiff_t)(ENC_TILES_PADDED + TRUNK_FWD_TILES + TRUNK_BWD_TILES) * TILE_FLOATS) return PNDF_ERR_BAD_SHAPE;
    if (enc) pndf_pack::emit_encoder_sections(tensors, stream, dst);
    return PNDF_OK;
}
extern "C" int pndf_pack_host(const float* const* tensors, const int64_t* numel, int n_tensors, float* stream, float* bias) {
    LayerNet nd;
    if (!table_plan(tensors, numel, n_tensors, nd) || !stream || !bias) return PNDF_ERR_BAD_SHAPE;
    return pack_fp32(tensors, nd, stream, bias);
}

// ---- split-precision stream
// Exact power-of-two scaling (pndf_pack::layer_scale): the weights of layer l travel as s_l W; 1 / s_l goes to the bias block
// (SCALE_OFF + l).  Biases stay unscaled: activations and gradients are scaled PER POSE on the chip, and the packer only
// supplies the norms (NORM_OFF) from which the kernel derives guaranteed bounds for the layers it cannot measure.

static int pack_split(const float* const* tensors, const LayerNet& nd, float* stream, float* bias, bool* lo_all_zero, bool bf16 = false) {
    // biases and encoder tiles are identical to the fp32 stream (the encoder stays on fp32 MFMA)
    int rc = pack_fp32(tensors, nd, stream, bias);
    if (rc != PNDF_OK) return rc;
    const float* const* lin = tensors + (nd.encoder ? 4 * NJ : 0);
    // per-layer weight scale; a layer without a finite non-zero weight cannot be scaled: refused (-> fp32 kernel)
    float wscale[6];
    for (int l = 0; l < 6; ++l) {
        if (!pndf_pack::layer_scale(lin[2 * l], (int64_t)nd.out(l) * nd.in(l), &wscale[l])) return PNDF_ERR_UNSUPPORTED;
        bias[SCALE_OFF + l] = 1.0f / wscale[l];
    }
    // norms for the a-priori bounds of the chunked layers, rounded UP (they must stay upper bounds in fp32)
    auto up = [](double v) { return std::nextafter((float)v, INFINITY); };
    for (int k = 0; k < 3; ++k) {
        const int lf = 2 * k, lb = 5 - 2 * k;           // forward chunk layers 0, 2, 4; backward chunk layers 5, 3, 1
        const int inf = nd.in(lf), outf = nd.out(lf);
        double rowmax = 0.0, bmax = 0.0;
        for (int o = 0; o < outf; ++o) {
            double sum = 0.0;
            for (int i = 0; i < inf; ++i) sum += std::fabs((double)lin[2 * lf][(size_t)o * inf + i]);
            rowmax = std::max(rowmax, sum);
            bmax = std::max(bmax, std::fabs((double)lin[2 * lf + 1][o]));
        }
        const int inb = nd.in(lb), outb = nd.out(lb);
        double colmax = 0.0;
        for (int i = 0; i < inb; ++i) {
            double sum = 0.0;
            for (int o = 0; o < outb; ++o) sum += std::fabs((double)lin[2 * lb][(size_t)o * inb + i]);
            colmax = std::max(colmax, sum);
        }
        bias[NORM_OFF + k] = up(rowmax);
        bias[NORM_OFF + 3 + k] = up(bmax);
        bias[NORM_OFF + 6 + k] = up(colmax);
    }
    float* dst = stream + (size_t)ENC_TILES_PADDED * TILE_FLOATS;
    bool any_lo = false;
    for (int ph = 0; ph < 6; ++ph) {
        Phase P = PHASES[ph];
        if (PNDF_BIG_CT != 2 && P.NC == 32) {      // (experiment: the two big phases in chunks of PNDF_BIG_CT tiles, pndf_layout.h)
            P.NC = P.NC * P.CT / PNDF_BIG_CT;
            P.CT = PNDF_BIG_CT;
        }
        const Mat A{lin[2 * P.a_lin], nd.out(P.a_lin), nd.in(P.a_lin), P.transposed};
        const Mat B{lin[2 * P.b_lin], nd.out(P.b_lin), nd.in(P.b_lin), P.transposed};
        auto partA = [&](int c) {
            for (int kb = 0; kb < P.KA / 2; ++kb)
                for (int ci = 0; ci < P.CT; ++ci, dst += 2 * TILE_FLOATS) any_lo |= pndf_pack::emit_pair_f16(A, c * P.CT + ci, kb, wscale[P.a_lin], dst, bf16);
        };
        auto partB = [&](int c) {
            for (int nb = 0; nb < P.NB; ++nb)
                for (int b = 0; b < P.CT / 2; ++b, dst += 2 * TILE_FLOATS) any_lo |= pndf_pack::emit_pair_f16(B, nb, (c * P.CT) / 2 + b, wscale[P.b_lin], dst, bf16);
        };
        partA(0);
        for (int c = 0; c < P.NC; ++c) {
            if (c + 1 < P.NC) partA(c + 1);
            partB(c);
        }
    }
    if (dst - stream != (ptrdiff_t)(ENC_TILES_PADDED + TRUNK_FWD_TILES + TRUNK_BWD_TILES) * TILE_FLOATS) return PNDF_ERR_BAD_SHAPE;
    if (lo_all_zero) *lo_all_zero = !any_lo;
    return PNDF_OK;
}
extern "C" int pndf_pack_host_split(const float* const* tensors, const int64_t* numel, int n_tensors, float* stream,
                                    float* bias) {
    LayerNet nd;
    if (!table_plan(tensors, numel, n_tensors, nd) || !stream || !bias) return PNDF_ERR_BAD_SHAPE;
    return pack_split(tensors, nd, stream, bias, nullptr);
}

extern "C" int pndf_load_weights(pndf_handle h, const float* const* tensors, const int64_t* numel, int n_tensors) {
    if (!h) return PNDF_ERR_BAD_ARG;
    // One order for both kernel families: validate (a refused table leaves the previous weights serving), stage on the host, clear
    // the flag, synchronise, copy, commit.
    const LayerNet& nd = h->net;
    if (const PndfTableFault f = pndf_table_fault(nd, tensors, numel, n_tensors))
        return pndf_fail(h, PNDF_ERR_BAD_SHAPE, "the weight table does not fit the configured network (the encoder's 84 tensors for in_dim 126, then weight and bias of every dfnet.lin): " + f.text());
    DeviceGuard guard(nd.device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    if (h->generic) {      // stages under a plan of its own and commits it after its copies
        h->have_weights = false;
        std::string why;
        const int grc = pndf_generic_load(h->generic, tensors, why);
        if (grc != PNDF_OK) return pndf_fail(h, grc, why);
        h->have_weights = true;
        return PNDF_OK;
    }
    std::vector<float> stream((size_t)STEP_TILES * TILE_FLOATS), bias(BIAS_FLOATS);
    bool lo_zero = false;
    const int prc = (h->precision != PNDF_PREC_FP32) ? pack_split(tensors, nd, stream.data(), bias.data(), &lo_zero, h->precision == PNDF_PREC_BF16)
                                                     : pack_fp32(tensors, nd, stream.data(), bias.data());
    if (prc == PNDF_ERR_UNSUPPORTED)
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "a trunk layer has no finite non-zero weight: outside the operating "
                                             "range of the fp16 hi/lo split -- use precision fp32 for this network");
    if (prc != PNDF_OK)
        return pndf_fail(h, PNDF_ERR_BAD_SHAPE, "internal: packed stream length mismatch");
    if (nd.act == PNDF_ACT_SOFTPLUS) {
        // zero-padded units of a narrower network: softplus(0) = ln 2 / beta with derivative 1/2 is harmless for the
        // result (zero outgoing weights) but would enter the per-pose operand bounds the split kernels measure (largest
        // activation, largest derivative of a layer).  A bias of -1e6 makes both exactly zero; relu-family units are
        // zero at 0 anyway.
        for (int l = 0; l < NLIN - 1; ++l)
            for (int j = nd.out(l); j < DIMS[l + 1]; ++j) bias[BIAS_OFF[l] + j] = -1.0e6f;
    }
    h->have_weights = false;              // from here on a failure leaves no half-loaded engine behind
    HIP_TRY(h, hipDeviceSynchronize());   // no launch may still be reading the old weights
    HIP_TRY(h, hipMemcpy(h->d_stream, stream.data(), stream.size() * sizeof(float), hipMemcpyHostToDevice));
    // replica of the first slots behind the stream: the ring's fetch offset never wraps inside a step
    HIP_TRY(h, hipMemcpy(h->d_stream + (size_t)STEP_TILES * TILE_BYTES, stream.data(),
                         (size_t)STREAM_PAD_SLOTS * SLOT_TILES * TILE_BYTES, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_bias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
    // PNDF_THREE_TERMS=1 keeps the three-term kernels (same-box A/B runs and the bit-identity test)
    const char* keep3 = getenv("PNDF_THREE_TERMS");
    h->lo_all_zero = lo_zero && h->precision == PNDF_PREC_F16X3 && !(keep3 && keep3[0] == '1');
    h->have_weights = true;
    return PNDF_OK;
}

// name of the kernel the compute calls of this handle launch (after pndf_load_weights), for logs, benches and tests
extern "C" const char* pndf_kernel_name(pndf_handle h) {
    if (!h) return "";
    if (h->generic) return pndf_generic_kernel_name(h->generic);
    return fused_kernel(h->precision, h->net.act == PNDF_ACT_SOFTPLUS, h->lo_all_zero).name;
}

// ------------------------------------------------------------------------------------------ launches
// `instrumented`: a kernel of the DEBUG library (libposendf_amd_debug.so: the s_memtime / stage-dump builds of the fused kernels) to
// launch instead of the handle's own, with the same arguments, grid and LDS -- pndf_internal_launch below; nullptr on every
// product path.  The debug library decides which of its kernels matches the handle (pndf_internal_describe).
static int launch(pndf_engine* h, int mode, const float* q, const float* gout, float* qo, float* d, int64_t B,
                  int steps, float* dbg, void* stream, const void* instrumented = nullptr, const pndf_project_options* popt = nullptr) {
    const bool timing = instrumented != nullptr;
    if (!h) return PNDF_ERR_BAD_ARG;
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_load_weights has not been called");
    if (B < 0 || steps < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative batch or step count");
    if (B == 0) return PNDF_OK;
    if (!q || (mode != MODE_FORWARD && !qo) || (mode == MODE_FORWARD && !d))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / output pointer");
    if (((uintptr_t)q | (uintptr_t)qo) & 15) return pndf_fail(h, PNDF_ERR_BAD_ARG, "pose buffers must be 16-byte aligned");
    if (((uintptr_t)d | (uintptr_t)gout) & 3) return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned distance buffer");
    const bool softplus = h->net.act == PNDF_ACT_SOFTPLUS;
    if (h->generic && (dbg || timing))
        return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "stage dumps and region timing exist for the amass.yaml-shaped kernels only");
    DeviceGuard guard(h->net.device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    if (!h->generic) {
        if (dbg && !timing) return pndf_fail(h, PNDF_ERR_BAD_ARG, "a dump buffer needs an instrumented kernel (libposendf_amd_debug.so)");
        if (timing && softplus && B > (int64_t)WG_POSES * h->resident_wgs)
            return pndf_fail(h, PNDF_ERR_UNSUPPORTED, "instrumented softplus kernel: at most one 64-pose block per compute unit");
    }
    if (mode == MODE_PROJECT && steps == 0) {
        // zero iterations: the loop body never runs (sample_poses.py:70); poses pass through
        if (qo != q) HIP_TRY(h, hipMemcpyAsync(qo, q, (size_t)B * NQ * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        if (d) HIP_TRY(h, hipMemsetAsync(d, 0, (size_t)B * sizeof(float), (hipStream_t)stream));
        return PNDF_OK;
    }
    if (h->generic) {
        std::string why;
        const int grc = pndf_generic_launch(h->generic, mode, q, gout, qo, d, B, steps, stream, why, popt);
        return grc == PNDF_OK ? PNDF_OK : pndf_fail(h, grc, why);
    }
    PndfKernelArgs a;
    a.q_in = q; a.q_out = qo; a.d_out = d; a.grad_out = gout;
    a.stream = h->d_stream; a.bias = h->d_bias; a.dbg = dbg;
    a.B = B; a.steps = steps;
    pndf_fill_step_options(a, mode, popt);
    a.slope = (h->net.act == PNDF_ACT_LRELU) ? 0.01f : 0.0f;   // nn.LeakyReLU() default slope, net_modules.py:31
    a.beta = h->net.beta;
    a.scratch = softplus ? h->d_scratch : nullptr;
    a.noenc = h->net.encoder ? 0 : 1;
    // relu family: one workgroup per 64-pose block.  Softplus: a persistent grid, at most one workgroup per CU (a workgroup takes
    // a whole CU), each walking its blocks; the derivative scratch is indexed by workgroup and was allocated in pndf_create --
    // nothing is allocated, freed or synchronised here.  The scratch is shared by all launches of the handle: sp_order.
    // (Instrumented softplus: one workgroup per block like the relu timing kernel, hence B <= 64 * resident_wgs above.)
    const int64_t nblocks = (B + WG_POSES - 1) / WG_POSES;
    const dim3 grid((unsigned)(softplus && nblocks > h->resident_wgs ? h->resident_wgs : nblocks)), block(WG_THREADS);
    if (softplus) HIP_TRY(h, h->sp_order.wait(stream));
    if (timing) {
        void* kargs[] = {&a};
        HIP_TRY(h, hipLaunchKernel(instrumented, grid, block, kargs, pndf_kernel_lds_bytes(), (hipStream_t)stream));
    } else {
        hipLaunchKernelGGL(fused_kernel(h->precision, softplus, h->lo_all_zero).fn, grid, block, pndf_kernel_lds_bytes(), (hipStream_t)stream, a);
    }
    HIP_TRY(h, hipGetLastError());
    if (softplus) HIP_TRY(h, h->sp_order.record(stream));
    return PNDF_OK;
}

extern "C" int pndf_forward(pndf_handle h, const float* q, float* d, int64_t B, void* stream) {
    PndfRange range("pndf_forward");
    return launch(h, MODE_FORWARD, q, nullptr, nullptr, d, B, 1, nullptr, stream);
}

extern "C" int pndf_forward_grad(pndf_handle h, const float* q, const float* grad_out, float* d, float* dq,
                                 int64_t B, void* stream) {
    PndfRange range("pndf_forward_grad");
    return launch(h, MODE_FORWARD_GRAD, q, grad_out, dq, d, B, 1, nullptr, stream);
}

extern "C" int pndf_project(pndf_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                            void* stream) {
    PndfRange range("pndf_project");
    return launch(h, MODE_PROJECT, q_in, nullptr, q_out, d_last, B, steps, nullptr, stream);
}

extern "C" void pndf_default_project_options(pndf_project_options* opt) {
    if (!opt) return;
    pndf_project_options def;
    (void)pndf_check_project_options(nullptr, def);
    *opt = def;
}

extern "C" int pndf_project_ex(pndf_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                               const pndf_project_options* opt, void* stream) {
    PndfRange range("pndf_project_ex");
    if (!h) return PNDF_ERR_BAD_ARG;
    pndf_project_options o;
    if (const char* why = pndf_check_project_options(opt, o)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    return launch(h, MODE_PROJECT, q_in, nullptr, q_out, d_last, B, steps, nullptr, stream, nullptr, &o);
}

// Pose completion (include/posendf_amd_completion.h; DESIGN.md section 2 "Pose completion"): the projection loop with the observed
// joints held, as `steps` times { pndf_forward_grad ; the step kernel of pndf_complete.hip } on the caller's stream.  Everything is
// validated before the first enqueue; pndf_forward_grad orders the softplus scratch across streams as for any other caller.  The
// last iteration writes its distances straight to d_last when the caller wants them.
extern "C" int pndf_complete(pndf_handle h, const float* q_in, const uint32_t* observed, float* q_out, float* d_last, int64_t B,
                             int steps, const pndf_project_options* opt, void* workspace, void* stream) {
    PndfRange range("pndf_complete");
    if (!h) return PNDF_ERR_BAD_ARG;
    pndf_project_options o;
    if (const char* why = pndf_check_project_options(opt, o)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_load_weights has not been called");
    if (B < 0 || steps < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative batch or step count");
    if (B > PNDF_COMPLETE_MAX_B) return pndf_fail(h, PNDF_ERR_BAD_ARG, "batch too large for the step kernel's grid");
    if (B == 0) return PNDF_OK;
    if (!q_in || !q_out) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / output pointer");
    if (!workspace) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null workspace (pndf_complete_workspace_floats(B) floats of device memory)");
    if (const char* why = pndf_check_step_alignment({q_in, q_out, workspace}, d_last, observed)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    DeviceGuard guard(h->net.device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    if (q_out != q_in) HIP_TRY(h, hipMemcpyAsync(q_out, q_in, (size_t)B * NQ * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (steps == 0) {      // as pndf_project_ex: the poses pass through
        if (d_last) HIP_TRY(h, hipMemsetAsync(d_last, 0, (size_t)B * sizeof(float), (hipStream_t)stream));
        return PNDF_OK;
    }
    float* d_ws = (float*)workspace;
    float* dq = d_ws + pndf_complete_d_floats(B);
    for (int s = 0; s < steps; ++s) {
        float* d = (s == steps - 1 && d_last) ? d_last : d_ws;
        if (const int rc = pndf_forward_grad(h, q_out, nullptr, d, dq, B, stream)) return rc;
        pndf_complete_step_enqueue(q_out, d, dq, observed, B, o, stream);
        if (const int rc = pndf_check_launch(h, "pndf_complete_step_kernel")) return rc;
    }
    return PNDF_OK;
}

// Pose interpolation (include/posendf_amd_interpolation.h; DESIGN.md section 2 "Pose interpolation"): the fill, then `steps` times
// { pndf_forward_grad ; the band kernel of pndf_interp.hip } on the caller's stream.  The band step is out of place, so the track
// alternates between track_out and the pose buffer of the workspace; the fill goes to the one that makes the last step write
// track_out.  Everything is validated before the first enqueue.
extern "C" int pndf_interpolate(pndf_handle h, const float* a, const float* b, const uint32_t* observed, float* track_out, float* d_last,
                                int64_t P, int32_t T, int32_t mode, int steps, float lambda, const pndf_project_options* opt,
                                void* workspace, void* stream) {
    PndfRange range("pndf_interpolate");
    if (!h) return PNDF_ERR_BAD_ARG;
    pndf_project_options o;
    if (const char* why = pndf_check_project_options(opt, o)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_interp_check_mode(mode)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_interp_check_lambda(lambda)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_load_weights has not been called");
    if (steps < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count");
    if (const char* why = pndf_interp_check_shape(P, T)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (P == 0) return PNDF_OK;
    if (!a || !b || !track_out) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / output pointer");
    if (!workspace)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "null workspace (pndf_interpolate_workspace_floats(P, T) floats of device memory)");
    if (const char* why = pndf_check_step_alignment({a, b, track_out, workspace}, d_last, observed)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    DeviceGuard guard(h->net.device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    const int64_t B = P * T;
    float* d_ws = (float*)workspace;
    float* dq = d_ws + pndf_complete_d_floats(B);
    float* other = dq + B * NQ;
    float* cur = (steps & 1) ? other : track_out;      // `steps` swaps later the track is in track_out
    float* nxt = (steps & 1) ? track_out : other;
    pndf_interp_fill_enqueue(a, b, cur, P, T, mode, stream);
    if (const int rc = pndf_check_launch(h, "pndf_interp_fill_kernel")) return rc;
    if (steps == 0) {      // as pndf_project_ex: nothing to report
        if (d_last) HIP_TRY(h, hipMemsetAsync(d_last, 0, (size_t)B * sizeof(float), (hipStream_t)stream));
        return PNDF_OK;
    }
    for (int s = 0; s < steps; ++s) {
        float* d = (s == steps - 1 && d_last) ? d_last : d_ws;
        if (const int rc = pndf_forward_grad(h, cur, nullptr, d, dq, B, stream)) return rc;
        pndf_interp_band_enqueue(cur, nxt, d, dq, observed, P, T, lambda, o, stream);
        if (const int rc = pndf_check_launch(h, "pndf_interp_band_kernel")) return rc;
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    return PNDF_OK;
}

// ---- hooks for the debug library (libposendf_amd_debug.so; include/posendf_amd_debug.h).  Not declared in any installed header and
// not part of the boundary: the instrumented builds of the fused kernels, the stage-dump kernel and the memory probes live in a
// library of their own, which reaches the engine through these three entry points -- bound at run time by
// posendf_amd.engine (function addresses handed to pndf_debug_bind), so that a variant product library (PNDF_LIBRARY) is
// instrumented by its own debug library and never by the default one.
extern "C" int pndf_internal_launch(pndf_handle h, int mode, const float* q, const float* gout, float* qo, float* d, int64_t B, int steps,
                                    float* dbg, void* stream, const void* kernel) {
    if (!kernel) return pndf_fail(h, PNDF_ERR_BAD_ARG, "pndf_internal_launch: no kernel");
    return launch(h, mode, q, gout, qo, d, B, steps, dbg, stream, kernel);
}
// what[0..6] = precision, act, lo_all_zero, noenc, runtime-planned, resident workgroups, LDS bytes of a fused kernel
extern "C" int pndf_internal_describe(pndf_handle h, int* what, int n) {
    if (!h || !what || n < 7) return PNDF_ERR_BAD_ARG;
    what[0] = h->precision;
    what[1] = h->net.act;
    what[2] = h->lo_all_zero ? 1 : 0;
    what[3] = h->net.encoder ? 0 : 1;
    what[4] = h->generic ? 1 : 0;
    what[5] = h->resident_wgs;
    what[6] = pndf_kernel_lds_bytes();
    return PNDF_OK;
}
extern "C" int pndf_internal_fail(pndf_handle h, int code, const char* msg) { return pndf_fail(h, code, msg ? msg : ""); }
