// The network as the host describes it, once for every handle that holds one -- the units assembled layer by layer
// (csrc/pndf_train.hip, csrc/pndf_second_order.hip, csrc/pndf_skeleton.hip), the persistent engine (csrc/pndf_capi.hip and its
// runtime-planned side, csrc/pndf_generic.hip) and the host twins of csrc/pndf_cpu.cpp: what the library accepts of pndf_config's
// num_joints / parent / dims / act / enc_act, how the encoder's activation and beta default to the trunk's, LayerNet, the plan a
// handle keeps -- the joint count and the parent table as run-time values, where bone j's tensors sit in the packed encoder, the
// size of every tensor in state-dict order --, and pndf_table_fault, whether a weight table fits that plan.  The units that stay
// 21-joint add that on top (layer_network_refusal of pndf_bone.h, pndf_skeleton_is_smpl); the fused kernels have the compile-time
// layout of pndf_layout.h, which csrc/pndf_capi.hip holds to the limits below with static_asserts.
// Plain C++: pndf_cpu.cpp is compiled without a device pass.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/posendf_amd.h"

constexpr int PNDF_SKEL_MAX_JOINTS = 32;      // pndf_config.parent[32]
constexpr int PNDF_SKEL_BONE = 4, PNDF_SKEL_FEAT = 6, PNDF_SKEL_HID = 10;
constexpr int PNDF_NET_MAX_LIN = 8;           // 1 .. 7 hidden layers -> 2 .. 8 linear layers
constexpr int PNDF_NET_MAX_WIDTH = 1024;

// Null, or why the skeleton of `cfg` is PNDF_ERR_UNSUPPORTED; the text names the field.  Any number of roots (-1), every
// parent before its child.
inline const char* pndf_skeleton_refusal(const pndf_config* cfg) {
    const int nj = cfg->num_joints;
    if (nj < 1 || nj > PNDF_SKEL_MAX_JOINTS) return "num_joints must be 1 .. 32";
    for (int j = 0; j < nj; ++j)
        if (cfg->parent[j] < -1 || cfg->parent[j] >= j) return "parent[j] must be -1 (a root) or an earlier joint 0 .. j - 1";
    if (cfg->dims[0] != PNDF_SKEL_FEAT * nj && cfg->dims[0] != PNDF_SKEL_BONE * nj)
        return "dims[0] must be 6 * num_joints (with the structure encoder) or 4 * num_joints (without it)";
    return nullptr;
}

// is this the table of get_parent_mapping('smpl')?  (the units that stay 21-joint ask)
constexpr int PNDF_SMPL_JOINTS = 21;
constexpr int PNDF_SMPL_PARENT[PNDF_SMPL_JOINTS] = {-1, -1, -1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19};
inline bool pndf_skeleton_is_smpl(const pndf_config* cfg) {
    if (cfg->num_joints != PNDF_SMPL_JOINTS) return false;
    for (int j = 0; j < PNDF_SMPL_JOINTS; ++j)
        if (cfg->parent[j] != PNDF_SMPL_PARENT[j]) return false;
    return true;
}

// bone j: 4 | 10 -> 10 -> 6; its four tensors in state-dict order are weight [10][fin], bias [10], weight [6][10], bias [6]
inline int pndf_skeleton_fin(const pndf_config* cfg, int j) { return cfg->parent[j] < 0 ? PNDF_SKEL_BONE : PNDF_SKEL_BONE + PNDF_SKEL_FEAT; }
inline void pndf_skeleton_bone_sizes(int fin, int sizes[4]) {
    sizes[0] = PNDF_SKEL_HID * fin;
    sizes[1] = PNDF_SKEL_HID;
    sizes[2] = PNDF_SKEL_FEAT * PNDF_SKEL_HID;
    sizes[3] = PNDF_SKEL_FEAT;
}

// Null, or why the DFNet and the activations of `cfg` are PNDF_ERR_UNSUPPORTED: one to seven hidden layers up to 1024 wide, one
// output, relu / lrelu / softplus in the trunk and in the encoder (-1: the trunk's).  The text names the field.  Softplus betas
// are each unit's own check.
inline const char* pndf_dfnet_refusal(const pndf_config* cfg) {
    if (cfg->n_dims < 3 || cfg->n_dims > PNDF_NET_MAX_LIN + 1) return "DFNet depth: n_dims must be 3 .. 9 (1 .. 7 hidden layers + the output layer)";
    if (cfg->dims[cfg->n_dims - 1] != 1) return "dims: in_dim, the hidden widths, then 1 -- the DFNet must end in one output";
    for (int i = 1; i < cfg->n_dims - 1; ++i)
        if (cfg->dims[i] < 1 || cfg->dims[i] > PNDF_NET_MAX_WIDTH) return "dims: hidden widths 1 .. 1024";
    if (cfg->act < PNDF_ACT_RELU || cfg->act > PNDF_ACT_SOFTPLUS) return "act: unknown activation (relu, lrelu or softplus)";
    if (cfg->enc_act < -1 || cfg->enc_act > PNDF_ACT_SOFTPLUS) return "enc_act: unknown encoder activation (relu, lrelu, softplus or -1, the trunk's)";
    return nullptr;
}

// model.StrEnc.act / beta are read on their own (net_modules.py:128); -1 / <= 0: the trunk's
inline int pndf_enc_act(const pndf_config& cfg) { return cfg.enc_act >= 0 ? cfg.enc_act : cfg.act; }
inline float pndf_enc_beta(const pndf_config& cfg) { return cfg.enc_beta > 0.f ? cfg.enc_beta : cfg.beta; }

// what a unit's handle knows about the network (a `cfg` that pndf_skeleton_refusal and pndf_dfnet_refusal passed)
struct LayerNet {
    int device = 0;
    int nj = 0;                   // joints
    bool encoder = true;          // dims[0] = 6 nj; without it the trunk reads the 4 nj normalised components
    int L = 0;                    // linear layers of the trunk
    int dims[PNDF_NET_MAX_LIN + 1] = {};
    int in(int l) const { return dims[l]; }          // dfnet.lin{l}: weight [out][in], bias [out]
    int out(int l) const { return dims[l + 1]; }
    int act = 0, enc_act = 0;
    float beta = 100.f, enc_beta = 100.f;
    int parent[PNDF_SKEL_MAX_JOINTS] = {};
    int enc_off[PNDF_SKEL_MAX_JOINTS] = {};                  // offset of bone j in the packed encoder
    int enc_tensor_off[4 * PNDF_SKEL_MAX_JOINTS + 1] = {};   // of its 4 nj tensors, and their end
    int enc_params = 0, maxw = 0;
    std::vector<int64_t> numel;   // of every tensor in state-dict order: the encoder's 4 nj (with it), then W and b of every layer
};

inline void layer_net_init(LayerNet& n, const pndf_config* cfg, int device) {
    n.device = device;
    n.nj = cfg->num_joints;
    n.encoder = cfg->dims[0] == PNDF_SKEL_FEAT * n.nj;
    n.L = cfg->n_dims - 1;
    for (int t = 0; t <= n.L; ++t) {
        n.dims[t] = cfg->dims[t];
        if (cfg->dims[t] > n.maxw) n.maxw = cfg->dims[t];
    }
    n.act = cfg->act;
    n.beta = cfg->beta;
    n.enc_act = pndf_enc_act(*cfg);
    n.enc_beta = pndf_enc_beta(*cfg);
    int o = 0, k = 0;
    for (int j = 0; j < n.nj; ++j) {
        n.parent[j] = cfg->parent[j];
        n.enc_off[j] = o;
        if (!n.encoder) continue;
        int sizes[4];
        pndf_skeleton_bone_sizes(pndf_skeleton_fin(cfg, j), sizes);
        for (int s = 0; s < 4; ++s) {
            n.enc_tensor_off[k++] = o;
            n.numel.push_back(sizes[s]);
            o += sizes[s];
        }
    }
    n.enc_tensor_off[k] = o;
    n.enc_params = o;
    for (int t = 0; t < n.L; ++t) {
        n.numel.push_back((int64_t)n.dims[t + 1] * n.dims[t]);
        n.numel.push_back(n.dims[t + 1]);
    }
}

// Does a weight table -- `n_tensors` host tensors in state-dict order, tensor i of numel[i] floats -- fit the network?  The first
// thing that is wrong, in the order below and then by tensor index, or FITS.  Every loader asks here and maps the answer to its
// family's status code; a caller that has no sizes of its own (training, the second order) passes the plan's, and can only hear
// NULL_TABLE or NULL_TENSOR.
struct PndfTableFault {
    enum Kind { FITS = 0, NULL_TABLE, COUNT, NULL_TENSOR, SIZE } kind = FITS;
    int index = -1;                 // NULL_TENSOR, SIZE: the tensor
    int64_t have = 0, want = 0;     // COUNT: tensors; SIZE: elements
    explicit operator bool() const { return kind != FITS; }
    std::string text() const {
        switch (kind) {
            case NULL_TABLE: return "tensors / numel is null";
            case COUNT: return "tensor count: " + std::to_string(have) + ", expected " + std::to_string(want) + " in state-dict order";
            case NULL_TENSOR: return "null tensor " + std::to_string(index);
            case SIZE: return "tensor " + std::to_string(index) + " has " + std::to_string(have) + " elements, expected " + std::to_string(want);
            default: return "";
        }
    }
};
inline PndfTableFault pndf_table_fault(const LayerNet& n, const float* const* tensors, const int64_t* numel, int n_tensors) {
    if (!tensors || !numel) return {PndfTableFault::NULL_TABLE};
    if (n_tensors != (int)n.numel.size()) return {PndfTableFault::COUNT, -1, n_tensors, (int64_t)n.numel.size()};
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i]) return {PndfTableFault::NULL_TENSOR, i};
        if (numel[i] != n.numel[i]) return {PndfTableFault::SIZE, i, numel[i], n.numel[i]};
    }
    return {};
}
// a table that comes without sizes: 4 J + 2 L pointers, each taken to be of the plan's size
inline PndfTableFault pndf_table_fault(const LayerNet& n, const float* const* tensors) {
    return pndf_table_fault(n, tensors, n.numel.data(), (int)n.numel.size());
}
