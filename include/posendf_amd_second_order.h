/* posendf_amd_second_order.h -- the second order of the distance: Hessian-vector products with respect to the pose.
 *
 * Companion of posendf_amd.h (same library).  For a pose q [21,4], a direction v [21,4] and two per-pose scalars w_d, w_t let
 *     S(q, v) = w_d d(q) + w_t <v, grad_q d(q)>.
 * One call gives d, g = grad_q d, t = <v, grad_q d> and out = grad_q S = w_d g + w_t H v with H the Hessian of d in q;
 * grad_v S = w_t g needs no call.  This is the double backward of the reference's `gradient()` (model/posendf.py:18-27, which asks
 * for create_graph=True) with respect to the pose: the weights of the network are constants, as on the train=False path, and no
 * gradient with respect to them comes out of here.  DESIGN.md section 2s.
 *
 * The networks: those of pndf_train_create -- the structure encoder and a DFNet of one to seven hidden layers up to 1024 wide,
 * any pair of StrEnc.act / DFNet.act.  Arithmetic: exact fp32 MFMA, layer by layer over chunks of poses whose size depends on B
 * alone; no float atomics: the same inputs give the same bits.
 *
 * A pose with a component column (the 21 joints' values of one quaternion component) of norm <= 1e-12 sits on the clamp of
 * F.normalize: there the normalisation is linear, the call returns the finite value of that branch (J = I / eps, no curvature
 * term), and the reference's own double backward returns NaN.
 *
 * Conventions: those of posendf_amd.h -- contiguous fp32, poses and directions [B, 21, 4], per-pose scalars [B]; DEVICE pointers,
 * 4-byte aligned, the workspace 16-byte aligned; work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and the call returns without synchronising, allocating or freeing anything; every entry point runs on the device of
 * its handle and restores the caller's current device; return value 0 on success, a negative pndf_status otherwise, its text in
 * pndf_so_last_error (of the calling thread's slot when there is no handle).
 */
#ifndef POSENDF_AMD_SECOND_ORDER_H
#define POSENDF_AMD_SECOND_ORDER_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pndf_so_plan* pndf_so_handle;

/* A plan for the network of `cfg` on `device` (a gfx950 device: PNDF_ERR_NO_DEVICE otherwise).  PNDF_ERR_UNSUPPORTED for a
 * network without the structure encoder (dims[0] != 126), an unknown activation, a depth or a width outside the range above. */
int pndf_so_create(pndf_so_handle* out, const pndf_config* cfg, int device);
int pndf_so_destroy(pndf_so_handle h);
const char* pndf_so_last_error(pndf_so_handle h);

/* Floats of the workspace of pndf_second_order for B poses (bounded: the batch is processed in chunks); 0 for B == 0;
 * PNDF_ERR_BAD_ARG for a null handle or a negative B. */
int64_t pndf_so_workspace_floats(pndf_so_handle h, int64_t B);

/* `weights`: a HOST table of device pointers to the live parameters in state-dict order (84 encoder tensors, then weight and bias
 * of every dfnet.lin), read at the time the stream runs the call.  w_d == NULL means 0, w_t == NULL means 1.  Each of d [B],
 * g [B,21,4], t [B], out [B,21,4] may be NULL and is then not written; the ones that are written hold the same bits whichever of
 * the others are asked for.  `workspace`: at least pndf_so_workspace_floats(h, B) floats of device memory (`workspace_floats`
 * says how many there are), owned by the caller, free to reuse once the stream has run the call.  B == 0 succeeds without a
 * launch.  PNDF_ERR_BAD_ARG with nothing launched for a null or misaligned pointer, a negative B, a workspace that is too small,
 * or `out` / `g` overlapping q, v or each other. */
int pndf_second_order(pndf_so_handle h, const float* const* weights, const float* q, const float* v, const float* w_d,
                      const float* w_t, float* d, float* g, float* t, float* out, int64_t B, void* workspace,
                      int64_t workspace_floats, void* stream);

/* Host twin (HOST pointers, the weights of pndf_cpu_load_weights, no workspace, no stream; text in pndf_cpu_last_error): the same
 * per-pose dual-number arithmetic in plain C++.  PNDF_ERR_UNSUPPORTED for an engine without the structure encoder. */
int pndf_second_order_cpu(pndf_cpu_handle h, const float* q, const float* v, const float* w_d, const float* w_t, float* d,
                          float* g, float* t, float* out, int64_t B);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_SECOND_ORDER_H */
