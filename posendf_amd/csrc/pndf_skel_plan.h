// The skeleton of a network as a run-time value: what the first-order units that take any joint tree (csrc/pndf_skeleton.hip on
// the device, the first-order host twins of csrc/pndf_cpu.cpp) accept of pndf_config's num_joints / parent / dims[0], and where
// bone j's tensors sit in the packed encoder.  The fixed-NJ counterparts are LayerNet of pndf_bone.h (training, second order)
// and pndf_layout.h (the fused kernels).  Plain C++: pndf_cpu.cpp is compiled without a device pass.
#pragma once
#include "../../include/posendf_amd.h"

constexpr int PNDF_SKEL_MAX_JOINTS = 32;      // pndf_config.parent[32]
constexpr int PNDF_SKEL_BONE = 4, PNDF_SKEL_FEAT = 6, PNDF_SKEL_HID = 10;

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
inline bool pndf_skeleton_is_smpl(const pndf_config* cfg) {
    constexpr int SMPL[21] = {-1, -1, -1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19};
    if (cfg->num_joints != 21) return false;
    for (int j = 0; j < 21; ++j)
        if (cfg->parent[j] != SMPL[j]) return false;
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
