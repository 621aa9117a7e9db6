// The projection step of ONE joint quaternion (DESIGN.md section 1 "The projection step"), written once for the device and the host:
// the fused kernels (pndf_device.h project_step), the completion kernel (pndf_complete.hip), the interpolation kernels
// (pndf_interp.h) and the host twins (pndf_cpu.cpp, compiled without a device pass) all call these functions, which is why they
// agree bit for bit.  Every operation is rounded to fp32 on its own, in the order written (contraction off in every body):
//   descend   u = Q - alpha * (dist * G)              three roundings; alpha = 1 makes alpha * p exact
//   finish    renorm 1, 2: u / clamp_min(sqrt(((u0 u0 + u1 u1) + u2 u2) + u3 u3), 1e-12)   0 stays 0, a NaN norm stays NaN
//             renorm 2: -u when u0 < 0                (the sign rule of posendf_amd.trainer.quat_flip)
//             returns the rest flag tol > 0 && dist < tol (false for a NaN dist): the caller then keeps Q as it came
// The two halves are separate so that the band step can put its coupling term between them.  The header needs no HIP runtime
// header before it.
#pragma once
#include <math.h>

#ifdef __HIP__
#define PNDF_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline)) inline
#else
#define PNDF_HD inline
#endif

// ((x0 y0 + x1 y1) + x2 y2) + x3 y3: the sum order of every norm and dot product of the step
PNDF_HD float pndf_quat_dot(const float* x, const float* y) {
#pragma clang fp contract(off)
    return ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3];
}

// out = <q, n> < 0 ? -n : n (a NaN dot product does not flip; the negation is exact)
PNDF_HD void pndf_quat_align(const float* q, const float* n, float* out) {
    const bool flip = pndf_quat_dot(q, n) < 0.f;
    for (int c = 0; c < 4; ++c) out[c] = flip ? -n[c] : n[c];
}

// u / max(|u|, 1e-12), the comparison written so that a NaN norm stays NaN
PNDF_HD void pndf_quat_unit(float* u) {
#pragma clang fp contract(off)
    const float ss = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3];
    const float n = sqrtf(ss);
    const float den = (n < 1e-12f) ? 1e-12f : n;
    for (int c = 0; c < 4; ++c) u[c] = u[c] / den;
}

PNDF_HD void pndf_step_descend(const float* Q, const float* G, float dist, float alpha, float* u) {
#pragma clang fp contract(off)
    for (int c = 0; c < 4; ++c) {
        const float p = dist * G[c];
        const float s = alpha * p;
        u[c] = Q[c] - s;
    }
}

PNDF_HD bool pndf_step_finish(float dist, float tol, int renorm, float* u) {
#pragma clang fp contract(off)
    if (renorm) {
        pndf_quat_unit(u);
        const bool flip = renorm == 2 && u[0] < 0.f;
        for (int c = 0; c < 4; ++c) u[c] = flip ? -u[c] : u[c];
    }
    return tol > 0.f && dist < tol;
}

PNDF_HD bool pndf_step_quat(const float* Q, const float* G, float dist, float alpha, float tol, int renorm, float* u) {
    pndf_step_descend(Q, G, dist, alpha, u);
    return pndf_step_finish(dist, tol, renorm, u);
}

// the components of a 16-byte vector (float4) a kernel loaded
template <class V4>
PNDF_HD void pndf_quat_unpack(const V4& v, float* x) {
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
