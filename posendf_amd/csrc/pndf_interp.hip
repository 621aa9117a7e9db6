// Pose interpolation (include/posendf_amd_interpolation.h): the fill of a track from its two key poses and the band step that relaxes
// it onto the pose manifold.
//
// pndf_interpolate runs on the device as one fill and then `steps` times { pndf_forward_grad ; the band kernel }: the fused kernels
// behind pndf_forward_grad stay as they are, and everything the track adds lives in two small element-wise kernels.  Both have
// one lane per joint quaternion of the track [P, T, 21, 4]: lane i holds joint j = i - 21 f of pose f = i / 21, which is frame
// k = f - T p of pair p = f / T (64-bit index arithmetic, bounded by P * T * 21).
//   pndf_interp_fill_kernel   one 16-byte load of a and of b of the lane's pair and joint, one 16-byte store.  Frame 0 stores the
//                             bits of a, frame T-1 the bits of b aligned to a, the frames between them pndf_interp_fill_quat.
//   pndf_interp_band_kernel   out of place, q_in -> q_out.  A held lane (an end frame of its pair, or bit j of observed[f]) copies
//                             its quaternion: one 16-byte load (and the mask word), one 16-byte store.  A free lane loads q_in and
//                             dq of its own quaternion, d[f] and -- only when lambda > 0 -- the same joint of frames k-1 and k+1
//                             of ITS pair (k is interior, so both exist and neither belongs to another pair): four 16-byte loads,
//                             the 4-byte d[f] and the mask word, then pndf_interp_band_quat and one 16-byte store.
// The arithmetic is shared with the host twin, every operation rounded to fp32 on its own (contraction off): the fill and the coupling
// are pndf_interp.h's, the projection step around the coupling is pndf_step.h's, which the fused kernels call too.  The
// options are plain kernel arguments.  No LDS, no atomics, no communication between lanes; q_out never aliases q_in, so one step
// is a Jacobi update and the same inputs give the same bits (tests/test_interpolation_gpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/posendf_amd_interpolation.h"
#include "pndf_host.h"
#include "pndf_interp.h"
#include "pndf_project_opts.h"

using pndf::NJ;

extern "C" __global__ void __launch_bounds__(256) pndf_interp_fill_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                                                                          float4* __restrict__ track, long long quats, int T, int mode) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quats) return;
    const long long f = i / NJ;
    const int j = (int)(i - f * NJ);
    const long long p = f / T;
    const int k = (int)(f - p * T);
    const float4 A = a[p * NJ + j], B = b[p * NJ + j];
    if (k == 0) {
        track[i] = A;
        return;
    }
    float av[4], bv[4], bp[4], u[4];
    pndf_quat_unpack(A, av);
    pndf_quat_unpack(B, bv);
    pndf_quat_align(av, bv, bp);
    if (k < T - 1) {
        const float t = (float)k / (float)(T - 1);
        pndf_interp_fill_quat(av, bp, t, mode, u);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) u[c] = bp[c];
    }
    track[i] = make_float4(u[0], u[1], u[2], u[3]);
}

extern "C" __global__ void __launch_bounds__(256) pndf_interp_band_kernel(const float4* __restrict__ q_in, float4* __restrict__ q_out,
                                                                          const float* __restrict__ d, const float4* __restrict__ dq,
                                                                          const uint32_t* __restrict__ observed, long long quats, int T,
                                                                          float lambda, float alpha, float tol, int renorm) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quats) return;
    const long long f = i / NJ;
    const int j = (int)(i - f * NJ);
    const int k = (int)(f % T);
    const float4 Q = q_in[i];
    if (k == 0 || k == T - 1 || (observed && ((observed[f] >> j) & 1u))) {      // held: the quaternion's bits, nothing else is read
        q_out[i] = Q;
        return;
    }
    const float dist = d[f];
    const float4 G = dq[i];
    float qv[4], gv[4], nm[4] = {0.f, 0.f, 0.f, 0.f}, np[4] = {0.f, 0.f, 0.f, 0.f}, u[4];
    pndf_quat_unpack(Q, qv);
    pndf_quat_unpack(G, gv);
    if (lambda > 0.f) {      // 0 < k < T-1: i - 21 and i + 21 are the same joint in frames k-1 and k+1 of the same pair
        pndf_quat_unpack(q_in[i - NJ], nm);
        pndf_quat_unpack(q_in[i + NJ], np);
    }
    const bool rest = pndf_interp_band_quat(qv, gv, dist, nm, np, lambda, alpha, tol, renorm, u);
    q_out[i] = rest ? Q : make_float4(u[0], u[1], u[2], u[3]);
}

void pndf_interp_fill_enqueue(const float* a, const float* b, float* track, int64_t P, int32_t T, int32_t mode, void* stream) {
    const long long quats = (long long)P * T * NJ;
    hipLaunchKernelGGL(pndf_interp_fill_kernel, dim3(pndf_step_blocks(quats)), dim3(PNDF_STEP_THREADS), 0, (hipStream_t)stream, (const float4*)a,
                       (const float4*)b, (float4*)track, quats, (int)T, (int)mode);
}

void pndf_interp_band_enqueue(const float* q_in, float* q_out, const float* d, const float* dq, const uint32_t* observed, int64_t P,
                              int32_t T, float lambda, const pndf_project_options& o, void* stream) {
    const long long quats = (long long)P * T * NJ;
    hipLaunchKernelGGL(pndf_interp_band_kernel, dim3(pndf_step_blocks(quats)), dim3(PNDF_STEP_THREADS), 0, (hipStream_t)stream, (const float4*)q_in,
                       (float4*)q_out, d, (const float4*)dq, observed, quats, (int)T, lambda, o.step_size, o.tol, (int)o.renorm);
}

// ------------------------------------------------------------------ C ABI (include/posendf_amd_interpolation.h)
extern "C" int pndf_interp_fill(const float* a, const float* b, float* track, int64_t P, int32_t T, int32_t mode, void* stream) {
    PndfRange range("pndf_interp_fill");
    if (pndf_interp_check_shape(P, T) || pndf_interp_check_mode(mode)) return PNDF_ERR_BAD_ARG;
    if (P == 0) return PNDF_OK;
    if (!a || !b || !track || pndf_check_step_alignment({a, b, track}, nullptr, nullptr)) return PNDF_ERR_BAD_ARG;
    DeviceGuard guard(pndf_pointer_device(track));
    if (!guard.ok) return PNDF_ERR_HIP;
    pndf_interp_fill_enqueue(a, b, track, P, T, mode, stream);
    PndfStepStatus status;
    return pndf_check_launch(&status, "pndf_interp_fill");
}

extern "C" int pndf_interp_band_step(const float* q_in, float* q_out, const float* d, const float* dq, const uint32_t* observed,
                                     int64_t P, int32_t T, float lambda, const pndf_project_options* opt, void* stream) {
    PndfRange range("pndf_interp_band_step");
    pndf_project_options o;
    if (pndf_check_project_options(opt, o)) return PNDF_ERR_BAD_ARG;
    if (pndf_interp_check_shape(P, T) || pndf_interp_check_lambda(lambda)) return PNDF_ERR_BAD_ARG;
    if (P == 0) return PNDF_OK;
    if (!q_in || !q_out || !d || !dq || q_out == q_in) return PNDF_ERR_BAD_ARG;
    if (pndf_check_step_alignment({q_in, q_out, dq}, d, observed)) return PNDF_ERR_BAD_ARG;
    DeviceGuard guard(pndf_pointer_device(q_out));
    if (!guard.ok) return PNDF_ERR_HIP;
    pndf_interp_band_enqueue(q_in, q_out, d, dq, observed, P, T, lambda, o, stream);
    PndfStepStatus status;
    return pndf_check_launch(&status, "pndf_interp_band_step");
}

extern "C" int64_t pndf_interpolate_workspace_floats(int64_t P, int32_t T) {
    if (pndf_interp_check_shape(P, T)) return PNDF_ERR_BAD_ARG;
    return pndf_interp_workspace_floats(P * T);
}
