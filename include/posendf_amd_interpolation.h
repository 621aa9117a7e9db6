/* posendf_amd_interpolation.h -- pose interpolation: in-betweens of two key poses, relaxed onto the pose manifold as a track.
 *
 * Companion of posendf_amd.h (same library, same handles).  A call takes P pairs of poses (a, b) and a frame count T >= 2 and
 * returns the track [P, T, 21, 4]: frame 0 is a, frame T-1 is b (negated per joint where that is the shorter way round), the
 * frames between them are a quaternion interpolation that then descends the distance field as in pndf_complete while a
 * neighbour-coupling term of weight `lambda` keeps the frames of one track evenly spaced.  The loop runs on the device as one
 * fill and then `steps` times { pndf_forward_grad ; pndf_interp_band_step }: two launches per step on the caller's stream and no
 * host work between them.  With lambda == 0 it equals pndf_complete on the filled track with the two end frames observed, bit
 * for bit, at every precision (DESIGN.md section 2 "Pose interpolation").
 *
 * Conventions: those of posendf_amd.h and posendf_amd_completion.h -- contiguous fp32, poses [.., 21, 4], distances one per
 * pose; device pointers to poses, gradients and the workspace 16-byte aligned, `d`, `d_last` and `observed` 4-byte aligned; work
 * is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and the call returns without synchronising,
 * allocating or freeing anything; every entry point runs on the device of its handle (the stateless ones: of their buffers) and
 * restores the caller's current device; return value 0 on success, a negative pndf_status otherwise.
 *
 * The fill, per joint quaternion: c = <a, b>; b' = c < 0 ? -b : b (a NaN c does not flip).  Frame 0 is the bits of a, frame T-1
 * the bits of b'.  Frame k between them has t = (float)k / (float)(T-1) and
 *   PNDF_INTERP_NLERP  u = (1-t) a + t b'
 *   PNDF_INTERP_SLERP  theta = 2 atan2f(|a - b'|, |a + b'|), sn = sinf(theta); u = wa a + wb b' with wa = sinf((1-t) theta) / sn,
 *                      wb = sinf(t theta) / sn where sn > 0, and wa = 1-t, wb = t otherwise
 * followed by u / max(|u|, 1e-12), the unit renormalisation of a projection step.
 *
 * The band step, out of place (q_in is only read; one step is a Jacobi update and the same inputs give the same bits): the end
 * frames of every pair and the joints held by `observed` are copied; any other joint quaternion Q of frame k takes
 *   u = Q - step_size (d G)                                   the step of pndf_complete_step
 *   u = u + lambda (0.5 (N- + N+) - Q)     if lambda > 0      N-, N+: the joint in frames k-1, k+1 of the SAME pair, each negated
 *                                                             where <Q, N> < 0
 * and then the renormalisation, unit_flip and stop tolerance of pndf_complete_step.  With lambda == 0 no neighbour is read.
 *
 * The mask: `observed` is one uint32 per pose of the track ([P * T], frame-major within a pair), bit j set = joint j is held
 * (bits 21 .. 31 are ignored); observed == NULL = no joint is held beyond the end frames.
 */
#ifndef POSENDF_AMD_INTERPOLATION_H
#define POSENDF_AMD_INTERPOLATION_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum pndf_interp_mode { PNDF_INTERP_SLERP = 0, PNDF_INTERP_NLERP = 1 };

/* track [P,T,21,4] <- the fill of a, b [P,21,4] (see above).  Stateless helper: status codes only, DEVICE pointers.
 * PNDF_ERR_BAD_ARG with nothing launched for a null or misaligned pointer, T < 2, a negative P, P * T beyond the grid of the
 * kernel, a mode that is not a pndf_interp_mode; P == 0 is a no-op. */
int pndf_interp_fill(const float* a, const float* b, float* track, int64_t P, int32_t T, int32_t mode, void* stream);

/* q_out [P,T,21,4] <- one band step of q_in from d [P*T] = dist_pred(q_in) and dq [P,T,21,4] = d d / d q_in (the outputs of
 * pndf_forward_grad).  Stateless helper: status codes only, DEVICE pointers.  opt as pndf_project_ex (NULL = the defaults), same
 * validation.  PNDF_ERR_BAD_ARG with nothing launched for a refused option struct, a lambda outside [0, 1] (a NaN included), a
 * null or misaligned q_in / q_out / d / dq, a misaligned `observed`, q_out == q_in, T < 2, a negative P, P * T beyond the grid of
 * the kernel; P == 0 is a no-op. */
int pndf_interp_band_step(const float* q_in, float* q_out, const float* d, const float* dq, const uint32_t* observed, int64_t P,
                          int32_t T, float lambda, const pndf_project_options* opt, void* stream);

/* Floats of the workspace of pndf_interpolate for P pairs of T frames: d, dq and the second pose buffer of the out-of-place
 * step, each on a 16-byte boundary.  Negative P, T < 2 or P * T beyond the grid of the kernels: PNDF_ERR_BAD_ARG. */
int64_t pndf_interpolate_workspace_floats(int64_t P, int32_t T);

/* track_out <- the fill of a, b, then `steps` times { pndf_forward_grad ; pndf_interp_band_step } between track_out and the pose
 * buffer of the workspace; the fill goes to whichever of the two makes the last step write track_out, so nothing is copied
 * afterwards.  a and b are only read.  d_last [P*T] (may be NULL) is dist_pred of the last iteration, evaluated before its
 * update, as in pndf_project_ex; steps == 0 returns the fill and zeroes d_last.  `workspace`:
 * pndf_interpolate_workspace_floats(P, T) floats of device memory, owned by the caller, free to reuse once the stream has run
 * the call.  1 + 2 * steps launches, none of them waits for the host.  PNDF_ERR_BAD_ARG (text in pndf_last_error; nothing is
 * launched or written) for a refused option struct, a bad mode or lambda, a null or misaligned pointer, a null workspace when
 * P > 0, T < 2, a negative P or steps, P * T beyond the bound of pndf_complete; P == 0 is a no-op. */
int pndf_interpolate(pndf_handle h, const float* a, const float* b, const uint32_t* observed, float* track_out, float* d_last,
                     int64_t P, int32_t T, int32_t mode, int steps, float lambda, const pndf_project_options* opt, void* workspace,
                     void* stream);

/* Host twin of pndf_interpolate (HOST pointers, no workspace, no stream; text in pndf_cpu_last_error): the same fill and the same
 * loop around the host twin's forward + gradient.  With lambda == 0 it equals pndf_complete_cpu on the filled track with the end
 * frames observed, bit for bit. */
int pndf_interpolate_cpu(pndf_cpu_handle h, const float* a, const float* b, const uint32_t* observed, float* track_out,
                         float* d_last, int64_t P, int32_t T, int32_t mode, int steps, float lambda,
                         const pndf_project_options* opt);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_INTERPOLATION_H */
