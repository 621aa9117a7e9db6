// The 2D keypoint term of image fitting (reference experiments/image_fitting.py:67-92, camera experiments/exp_utils.py:119-143;
// robustifier and confidence weighting as in SMPLify-X, which that script copies) with its gradient, and the camera forward
// alone.  With pndf_forward_grad, pndf_lbs_forward(verts = NULL), pndf_lbs_backward(g_joints), pndf_denoise_update_w(g_body)
// and pndf_adam_step a whole fitting step is six launches with no host work in between.
//   global orientation   SMPL's global_orient is a rotation about the rest root joint J0 = joints[n, 0]:
//                            lbs(theta, global_orient = r) = R(r) (x - J0) + J0        (x computed at global_orient = 0)
//                        so it is applied HERE, to the joints, and csrc/pndf_lbs.hip is untouched.  J0 is a constant of the
//                        pose: no gradient flows into row 0 through its role as pivot.
//   camera               p = Rc (R(r) (x - J0) + J0) + t;  u = fx p_x / p_z + cx,  v = fy p_y / p_z + cy
//   data term            E_n = sum_j (w_j c_nj)^2 [rho(kx - u) + rho(ky - v)],  rho(e) = e^2  or  rho^2 e^2 / (e^2 + rho^2)
//   depth term           D_n = (t_z - depth_target)^2
// A joint with w_j c_nj == 0 is SKIPPED: its keypoint is not read into the arithmetic (a missing detection stored as NaN
// contributes exactly 0 to every output).  p_z <= 0 propagates inf / NaN as the PyTorch expression does.
// One wavefront per frame, one lane per joint (a lane loop when J > 64), four frames per 256-thread workgroup.  The per-frame
// sums (9 entries of dL/dR, 3 of g_transl, E_n) are reduced across the wave by an xor butterfly in a fixed order: no LDS, no
// atomics, the same inputs give the same bits.  Plain fp32, sinf / cosf.  HBM-bound: about 36 J + 60 bytes per frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/posendf_amd.h"
#include "pndf_host.h"

namespace {

constexpr int WAVE = 64, FRAMES_PER_WG = 4, WG = WAVE * FRAMES_PER_WG;

struct KeypointArgs {
    const float* joints;
    const float* orient;
    const float* transl;
    const float* keypoints;
    const float* joint_weight;
    float* terms;
    float* g_joints;
    float* g_orient;
    float* g_transl;
    float* posed;
    float* uv;
    long long N;
    int J;
    int use_conf;
    float fx, fy, cx, cy;
    float Rc[9];
    float data_coef, rho, depth_coef, depth_target;
};

// smplx batch_rodrigues (oracle/lbs_np.batch_rodrigues): angle = |r + 1e-8|, axis = r / angle, R = I + sin K + (1 - cos) K K
struct Rodrigues {
    float a[3], n[3], th, s, c;
    float K[9], KK[9], R[9];
};

__host__ __device__ __forceinline__ void mat3_mul(const float (&A)[9], const float (&B)[9], float (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * i + k] = A[3 * i] * B[k] + A[3 * i + 1] * B[3 + k] + A[3 * i + 2] * B[6 + k];
}

__host__ __device__ __forceinline__ void rodrigues(const float* __restrict__ r, Rodrigues& o) {
    const float rx = r[0], ry = r[1], rz = r[2];
    o.a[0] = rx + 1e-8f; o.a[1] = ry + 1e-8f; o.a[2] = rz + 1e-8f;
    o.th = sqrtf(o.a[0] * o.a[0] + o.a[1] * o.a[1] + o.a[2] * o.a[2]);
    o.n[0] = rx / o.th; o.n[1] = ry / o.th; o.n[2] = rz / o.th;
    o.s = sinf(o.th);
    o.c = cosf(o.th);
    o.K[0] = 0.f;      o.K[1] = -o.n[2]; o.K[2] = o.n[1];
    o.K[3] = o.n[2];   o.K[4] = 0.f;     o.K[5] = -o.n[0];
    o.K[6] = -o.n[1];  o.K[7] = o.n[0];  o.K[8] = 0.f;
    mat3_mul(o.K, o.K, o.KK);
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = ((i & 3) == 0 ? 1.0f : 0.0f) + o.s * o.K[i] + (1.0f - o.c) * o.KK[i];
}

// oracle/lbs_np._rodrigues_vjp: d <gR, R(r)> / d r
__host__ __device__ __forceinline__ void rodrigues_vjp(const Rodrigues& o, const float* __restrict__ r, const float (&gR)[9], float (&g)[3]) {
    float g_th = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) g_th += gR[i] * (o.c * o.K[i] + o.s * o.KK[i]);
    float KT[9], A[9], B[9], gK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) KT[3 * i + k] = o.K[3 * k + i];
    mat3_mul(gR, KT, A);
    mat3_mul(KT, gR, B);
#pragma unroll
    for (int i = 0; i < 9; ++i) gK[i] = o.s * gR[i] + (1.0f - o.c) * (A[i] + B[i]);
    const float gn[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    g_th -= (gn[0] * r[0] + gn[1] * r[1] + gn[2] * r[2]) / (o.th * o.th);      // n = r / th
#pragma unroll
    for (int e = 0; e < 3; ++e) g[e] = gn[e] / o.th + g_th * o.a[e] / o.th;
}

// every lane ends with the sum over the wave, added in the same order on every call
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}

// camera-space point of one joint: y = x - J0 (kept for dL/dR), p = Rc (R y + J0) + t
__host__ __device__ __forceinline__ void pose_point(const KeypointArgs& a, const float (&R)[9], const float (&J0)[3], const float (&t)[3],
                                                    const float* __restrict__ x, float (&y)[3], float (&p)[3]) {
    float w[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) y[e] = x[e] - J0[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) w[e] = R[3 * e] * y[0] + R[3 * e + 1] * y[1] + R[3 * e + 2] * y[2] + J0[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) p[e] = a.Rc[3 * e] * w[0] + a.Rc[3 * e + 1] * w[1] + a.Rc[3 * e + 2] * w[2] + t[e];
}

// One selected joint: adds its share to E, to d L / d R (gR += Rc^T g_p y^T) and to d L / d t, returns d L / d x = R^T Rc^T g_p
__host__ __device__ __forceinline__ void joint_term(const KeypointArgs& a, const float (&R)[9], const float (&J0)[3], const float (&t)[3],
                                                    const float* __restrict__ x, const float* __restrict__ kp, float wc, float (&gR)[9],
                                                    float (&gt)[3], float& E, float (&gx)[3]) {
    float y[3], p[3];
    pose_point(a, R, J0, t, x, y, p);
    const float iz = 1.0f / p[2];
    const float sx = a.fx * p[0] * iz, sy = a.fy * p[1] * iz;
    const float ex = kp[0] - (sx + a.cx), ey = kp[1] - (sy + a.cy);
    const float w2 = wc * wc, rho2 = a.rho * a.rho;
    float px, py, dx, dy;                                   // rho(e) and d rho / d e
    if (a.rho == 0.0f) {
        px = ex * ex; py = ey * ey;
        dx = 2.0f * ex; dy = 2.0f * ey;
    } else {
        const float qx = 1.0f / (ex * ex + rho2), qy = 1.0f / (ey * ey + rho2);
        px = rho2 * ex * ex * qx; py = rho2 * ey * ey * qy;
        dx = 2.0f * ex * (rho2 * qx) * (rho2 * qx); dy = 2.0f * ey * (rho2 * qy) * (rho2 * qy);
    }
    E += w2 * (px + py);
    const float gu = -a.data_coef * w2 * dx, gv = -a.data_coef * w2 * dy;      // d L / d (u, v)
    const float gp[3] = {gu * a.fx * iz, gv * a.fy * iz, -(gu * sx + gv * sy) * iz};
    float gw[3];                                            // Rc^T g_p
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        gt[e] += gp[e];
        gw[e] = a.Rc[e] * gp[0] + a.Rc[3 + e] * gp[1] + a.Rc[6 + e] * gp[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) gR[3 * i + k] += gw[i] * y[k];
#pragma unroll
    for (int e = 0; e < 3; ++e) gx[e] = R[e] * gw[0] + R[3 + e] * gw[1] + R[6 + e] * gw[2];
}

}  // namespace

extern "C" __global__ void __launch_bounds__(WG) pndf_keypoint_terms_grad_kernel(KeypointArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long n = (long long)blockIdx.x * FRAMES_PER_WG + (threadIdx.x >> 6);
    if (n >= a.N) return;                                   // whole waves: nothing below crosses a wave
    const float* r = a.orient + n * 3;
    const float t[3] = {a.transl[n * 3], a.transl[n * 3 + 1], a.transl[n * 3 + 2]};
    const float* jn = a.joints + n * a.J * 3;
    const float J0[3] = {jn[0], jn[1], jn[2]};
    Rodrigues ro;
    rodrigues(r, ro);

    float gR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gt[3] = {0.f, 0.f, 0.f}, E = 0.f;
    for (int j = lane; j < a.J; j += WAVE) {
        const float* kp = a.keypoints + (n * a.J + j) * 3;
        const float wc = (a.joint_weight ? a.joint_weight[j] : 1.0f) * (a.use_conf ? kp[2] : 1.0f);
        float gx[3] = {0.f, 0.f, 0.f};
        if (wc != 0.0f) joint_term(a, ro.R, J0, t, jn + 3 * j, kp, wc, gR, gt, E, gx);
        if (a.g_joints) {
            float* gj = a.g_joints + (n * a.J + j) * 3;
            gj[0] = gx[0]; gj[1] = gx[1]; gj[2] = gx[2];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) gR[i] = wave_sum(gR[i]);
#pragma unroll
    for (int e = 0; e < 3; ++e) gt[e] = wave_sum(gt[e]);
    E = wave_sum(E);
    if (lane != 0) return;
    const float dz = t[2] - a.depth_target;
    if (a.terms) {
        a.terms[n * 2] = E;
        a.terms[n * 2 + 1] = dz * dz;
    }
    if (a.g_transl) {
        a.g_transl[n * 3] = gt[0];
        a.g_transl[n * 3 + 1] = gt[1];
        a.g_transl[n * 3 + 2] = gt[2] + a.depth_coef * 2.0f * dz;
    }
    if (a.g_orient) {
        float go[3];
        rodrigues_vjp(ro, r, gR, go);
        a.g_orient[n * 3] = go[0]; a.g_orient[n * 3 + 1] = go[1]; a.g_orient[n * 3 + 2] = go[2];
    }
}

extern "C" __global__ void __launch_bounds__(WG) pndf_keypoint_project_kernel(KeypointArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long n = (long long)blockIdx.x * FRAMES_PER_WG + (threadIdx.x >> 6);
    if (n >= a.N) return;
    const float t[3] = {a.transl[n * 3], a.transl[n * 3 + 1], a.transl[n * 3 + 2]};
    const float* jn = a.joints + n * a.J * 3;
    const float J0[3] = {jn[0], jn[1], jn[2]};
    Rodrigues ro;
    rodrigues(a.orient + n * 3, ro);
    for (int j = lane; j < a.J; j += WAVE) {
        float y[3], p[3];
        pose_point(a, ro.R, J0, t, jn + 3 * j, y, p);
        if (a.posed) {
            float* o = a.posed + (n * a.J + j) * 3;
            o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        }
        if (a.uv) {
            const float iz = 1.0f / p[2];
            float* o = a.uv + (n * a.J + j) * 2;
            o[0] = a.fx * p[0] * iz + a.cx;
            o[1] = a.fy * p[1] * iz + a.cy;
        }
    }
}

// ------------------------------------------------------------------ C ABI (include/posendf_amd.h)
static int keypoint_launch(bool grad, KeypointArgs& a, const pndf_camera* cam, void* stream) {
    const long long blocks = (a.N + FRAMES_PER_WG - 1) / FRAMES_PER_WG;
    if (blocks > 0x7fffffffll) return PNDF_ERR_BAD_ARG;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    for (int i = 0; i < 9; ++i) a.Rc[i] = cam->R[i];
    DeviceGuard guard(pndf_pointer_device(a.joints));
    if (!guard.ok) return PNDF_ERR_HIP;
    if (grad) hipLaunchKernelGGL(pndf_keypoint_terms_grad_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(pndf_keypoint_project_kernel, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PNDF_OK : PNDF_ERR_HIP;
}

extern "C" int pndf_keypoint_terms_grad(const float* joints, const float* orient, const float* transl, const float* keypoints,
                                        const float* joint_weight, int64_t N, int32_t J, const pndf_camera* cam,
                                        const pndf_keypoint_opts* opt, float* terms, float* g_joints, float* g_orient,
                                        float* g_transl, void* stream) {
    PndfRange range("pndf_keypoint_terms_grad");
    if (N < 0 || J < 1 || !cam || !opt || !(opt->rho >= 0.0f)) return PNDF_ERR_BAD_ARG;
    if (N == 0) return PNDF_OK;
    if (!joints || !orient || !transl || !keypoints) return PNDF_ERR_BAD_ARG;
    KeypointArgs a = {};
    a.joints = joints; a.orient = orient; a.transl = transl; a.keypoints = keypoints; a.joint_weight = joint_weight;
    a.terms = terms; a.g_joints = g_joints; a.g_orient = g_orient; a.g_transl = g_transl;
    a.N = (long long)N; a.J = J; a.use_conf = opt->use_conf ? 1 : 0;
    a.data_coef = opt->data_coef; a.rho = opt->rho; a.depth_coef = opt->depth_coef; a.depth_target = opt->depth_target;
    return keypoint_launch(true, a, cam, stream);
}

extern "C" int pndf_keypoint_project(const float* joints, const float* orient, const float* transl, int64_t N, int32_t J,
                                     const pndf_camera* cam, float* posed, float* uv, void* stream) {
    PndfRange range("pndf_keypoint_project");
    if (N < 0 || J < 1 || !cam) return PNDF_ERR_BAD_ARG;
    if (N == 0) return PNDF_OK;
    if (!joints || !orient || !transl) return PNDF_ERR_BAD_ARG;
    KeypointArgs a = {};
    a.joints = joints; a.orient = orient; a.transl = transl; a.posed = posed; a.uv = uv;
    a.N = (long long)N; a.J = J;
    return keypoint_launch(false, a, cam, stream);
}
