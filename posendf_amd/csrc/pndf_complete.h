// Pose completion (include/posendf_amd_completion.h): what pndf_complete (pndf_capi.hip, where the engine handle lives) shares with
// the step kernel's translation unit (pndf_complete.hip) -- and, both being one lane per joint quaternion around pndf_step.h, what
// that unit shares with the interpolation kernels' (pndf_interp.hip): the launch shape, the alignment refusals, the status slot.
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "../../include/posendf_amd_completion.h"
#include "pndf_error.h"
#include "pndf_layout.h"

// one lane per joint quaternion, pndf::NJ = 21 of them per pose
constexpr int PNDF_STEP_THREADS = 256;
inline unsigned pndf_step_blocks(long long quats) { return (unsigned)((quats + PNDF_STEP_THREADS - 1) / PNDF_STEP_THREADS); }
// largest B whose B * 21 joint quaternions fit the step kernel's one-dimensional grid
constexpr int64_t PNDF_COMPLETE_MAX_B = ((int64_t)0x7fffffff * PNDF_STEP_THREADS) / pndf::NJ;

// the stateless helpers have no handle: pndf_check_launch leaves its text here and the code is returned
struct PndfStepStatus {
    std::string err;
};

// Why the buffers of a step are refused, or nullptr: the kernels move one 16-byte vector per joint quaternion of every pose-sized
// buffer (`vec16`: the poses, dq, the workspace); the distances and the mask -- either may be null -- are read by the word.
inline const char* pndf_check_step_alignment(std::initializer_list<const void*> vec16, const void* d, const void* mask) {
    uintptr_t bits = 0;
    for (const void* p : vec16) bits |= (uintptr_t)p;
    if (bits & 15) return "pose buffers and the workspace must be 16-byte aligned";
    if (((uintptr_t)d | (uintptr_t)mask) & 3) return "misaligned distance or mask buffer";
    return nullptr;
}

// the workspace of pndf_complete: d [B] padded to a multiple of four floats, then dq [B,21,4] -- both on a 16-byte boundary
inline int64_t pndf_complete_d_floats(int64_t B) { return (B + 3) & ~(int64_t)3; }

// Enqueues the step kernel on `stream` and nothing else: no validation (the callers have done it: `o` comes from
// pndf_check_project_options, the pointers are non-null and aligned, B > 0), no device selection, no error check -- the caller
// follows it with pndf_check_launch.
PNDF_LOCAL void pndf_complete_step_enqueue(float* q, const float* d, const float* dq, const uint32_t* observed, int64_t B,
                                           const pndf_project_options& o, void* stream);
