// Pose completion (include/posendf_amd_completion.h): what pndf_complete (pndf_capi.hip, where the engine handle lives) shares with
// the step kernel's translation unit (pndf_complete.hip).
#pragma once
#include <stdint.h>

#include "../../include/posendf_amd_completion.h"
#include "pndf_error.h"

// the workspace of pndf_complete: d [B] padded to a multiple of four floats, then dq [B,21,4] -- both on a 16-byte boundary
inline int64_t pndf_complete_d_floats(int64_t B) { return (B + 3) & ~(int64_t)3; }

// Enqueues the step kernel on `stream` and nothing else: no validation (the callers have done it: `o` comes from
// pndf_check_project_options, the pointers are non-null and aligned, B > 0), no device selection, no error check -- the caller
// follows it with pndf_check_launch.
PNDF_LOCAL void pndf_complete_step_enqueue(float* q, const float* d, const float* dq, const uint32_t* observed, int64_t B,
                                           const pndf_project_options& o, void* stream);

// largest B whose B * 21 joint quaternions fit the step kernel's one-dimensional grid
constexpr int64_t PNDF_COMPLETE_MAX_B = ((int64_t)0x7fffffff * 256) / 21;
