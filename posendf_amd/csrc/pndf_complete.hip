// Pose completion (include/posendf_amd_completion.h): the projection step applied to the joints that are NOT observed.
//
// pndf_complete runs the projection loop on the device as `steps` times { pndf_forward_grad ; this kernel }: the fused kernels
// behind pndf_forward_grad stay as they are, and the mask lives in this one small element-wise kernel.
//   pndf_complete_step_kernel   one lane per joint quaternion: lane i holds joint j = i - 21 b of pose b = i / 21 (64-bit index
//                               arithmetic, bounded by B * 21).  One 16-byte load of q and of dq, d[b] and observed[b]; a held
//                               joint (bit j of observed[b]) is neither updated nor stored; any other joint takes pndf_step.h's
//                               pndf_step_quat -- the one statement of the step, which the fused kernels call too -- and is
//                               stored with one 16-byte store.
// The step options are plain kernel arguments.  No LDS, no atomics, no communication between lanes: the same inputs give the same
// bits, and with no joint held a step equals the one inside pndf_project_ex bit for bit (tests/test_completion_gpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/posendf_amd_completion.h"
#include "pndf_complete.h"
#include "pndf_host.h"
#include "pndf_project_opts.h"
#include "pndf_step.h"

using pndf::NJ;

extern "C" __global__ void __launch_bounds__(256) pndf_complete_step_kernel(float4* __restrict__ q, const float* __restrict__ d,
                                                                            const float4* __restrict__ dq,
                                                                            const uint32_t* __restrict__ observed, long long quats,
                                                                            float alpha, float tol, int renorm) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quats) return;
    const long long b = i / NJ;
    const int j = (int)(i - b * NJ);
    if (observed && ((observed[b] >> j) & 1u)) return;      // held: the joint's bits stay as they are
    const float dist = d[b];
    const float4 Q = q[i];
    float qv[4], gv[4], u[4];
    pndf_quat_unpack(Q, qv);
    pndf_quat_unpack(dq[i], gv);
    const bool rest = pndf_step_quat(qv, gv, dist, alpha, tol, renorm, u);
    q[i] = rest ? Q : make_float4(u[0], u[1], u[2], u[3]);
}

void pndf_complete_step_enqueue(float* q, const float* d, const float* dq, const uint32_t* observed, int64_t B,
                                const pndf_project_options& o, void* stream) {
    const long long quats = (long long)B * NJ;
    // (the default options give the plain step of pndf_project: a step size of 1 makes its product exact)
    hipLaunchKernelGGL(pndf_complete_step_kernel, dim3(pndf_step_blocks(quats)), dim3(PNDF_STEP_THREADS), 0, (hipStream_t)stream,
                       (float4*)q, d, (const float4*)dq, observed, quats, o.step_size, o.tol, (int)o.renorm);
}

// ------------------------------------------------------------------ C ABI (include/posendf_amd_completion.h)
extern "C" int pndf_complete_step(float* q, const float* d, const float* dq, const uint32_t* observed, int64_t B,
                                  const pndf_project_options* opt, void* stream) {
    PndfRange range("pndf_complete_step");
    pndf_project_options o;
    if (pndf_check_project_options(opt, o)) return PNDF_ERR_BAD_ARG;
    if (B < 0 || B > PNDF_COMPLETE_MAX_B) return PNDF_ERR_BAD_ARG;
    if (B == 0) return PNDF_OK;
    if (!q || !d || !dq || pndf_check_step_alignment({q, dq}, d, observed)) return PNDF_ERR_BAD_ARG;
    DeviceGuard guard(pndf_pointer_device(q));
    if (!guard.ok) return PNDF_ERR_HIP;
    pndf_complete_step_enqueue(q, d, dq, observed, B, o, stream);
    PndfStepStatus status;
    return pndf_check_launch(&status, "pndf_complete_step");
}

extern "C" int64_t pndf_complete_workspace_floats(int64_t B) {
    if (B < 0 || B > PNDF_COMPLETE_MAX_B) return PNDF_ERR_BAD_ARG;
    return pndf_complete_d_floats(B) + B * (int64_t)(NJ * 4);
}
