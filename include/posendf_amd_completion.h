/* posendf_amd_completion.h -- pose completion: the projection loop of posendf_amd.h with some joints held.
 *
 * Companion of posendf_amd.h (same library, same handles).  Some of a pose's 21 joint rotations are observed and stay as they
 * are, bit for bit; the others descend the distance field as in pndf_project_ex.  The loop runs on the device as `steps` times
 * { pndf_forward_grad ; pndf_complete_step }: two launches per step on the caller's stream and no host work between them.  With
 * no joint held the result equals pndf_project_ex bit for bit, at every precision (DESIGN.md section 2 "Pose completion").
 *
 * Conventions: those of posendf_amd.h -- contiguous fp32, poses [B, 21, 4], distances [B]; device pointers to poses, gradients
 * and the workspace 16-byte aligned, `d` and `observed` 4-byte aligned; work is enqueued on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream) and the call returns without synchronising, allocating or freeing anything; every entry point
 * runs on the device of its handle (pndf_complete_step: of its buffers) and restores the caller's current device; return value 0
 * on success, a negative pndf_status otherwise.
 *
 * The mask: `observed` is one uint32 per pose, bit j set = joint j is held (bits 21 .. 31 are ignored); observed == NULL = no
 * joint is held.  A held joint is never read for the update nor written: whatever bits it holds (a NaN, a zero quaternion) stay.
 * It still enters the distance and the gradient of the other joints, like every joint of the pose.
 */
#ifndef POSENDF_AMD_COMPLETION_H
#define POSENDF_AMD_COMPLETION_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step on q [B,21,4] in place, from d [B] = dist_pred(q) and dq [B,21,4] = d d / d q (the outputs of pndf_forward_grad): the
 * step of pndf_project_ex (posendf_amd.h "Options of one projection step") on every joint that is not held.  Stateless helper:
 * status codes only, DEVICE pointers.  opt as pndf_project_ex (NULL = the defaults), same validation.  PNDF_ERR_BAD_ARG with
 * nothing launched for a refused option struct, a null or misaligned q / d / dq, a misaligned `observed`, a negative B; B == 0 is
 * a no-op. */
int pndf_complete_step(float* q, const float* d, const float* dq, const uint32_t* observed, int64_t B,
                       const pndf_project_options* opt, void* stream);

/* Floats of the workspace of pndf_complete for B poses: d and dq of one step, each on a 16-byte boundary.  Negative B:
 * PNDF_ERR_BAD_ARG. */
int64_t pndf_complete_workspace_floats(int64_t B);

/* q_out <- q_in (q_out may alias q_in), then `steps` times { pndf_forward_grad(h, q_out, NULL, d, dq) ; pndf_complete_step }.
 * d_last[b] (may be NULL) is dist_pred of the last iteration, evaluated before its update, as in pndf_project_ex; steps == 0
 * passes the poses through and zeroes d_last, as pndf_project_ex does.  `workspace`: pndf_complete_workspace_floats(B) floats of
 * device memory, owned by the caller, free to reuse once the stream has run the call.  2 * steps launches, none of them waits for
 * the host.  PNDF_ERR_BAD_ARG (text in pndf_last_error; nothing is launched or written) for a refused option struct, a null or
 * misaligned pointer, a null workspace when B > 0, a negative B or steps; B == 0 is a no-op. */
int pndf_complete(pndf_handle h, const float* q_in, const uint32_t* observed, float* q_out, float* d_last, int64_t B,
                  int steps, const pndf_project_options* opt, void* workspace, void* stream);

/* Host twin of pndf_complete (HOST pointers, no workspace, no stream; text in pndf_cpu_last_error): the same loop around the
 * host twin's forward + gradient.  With no joint held it equals pndf_project_ex_cpu bit for bit. */
int pndf_complete_cpu(pndf_cpu_handle h, const float* q_in, const uint32_t* observed, float* q_out, float* d_last,
                      int64_t B, int steps, const pndf_project_options* opt);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_COMPLETION_H */
