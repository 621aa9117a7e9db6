// Pose interpolation (include/posendf_amd_interpolation.h): what the kernels' translation unit (pndf_interp.hip), pndf_interpolate
// (pndf_capi.hip, where the engine handle lives) and the host twin (pndf_cpu.cpp, compiled without a device pass) share -- the
// arithmetic of one joint quaternion of the fill and of the band step's coupling, stated ONCE for the device and the host around the
// projection step of pndf_step.h, the argument checks, the workspace layout and the two enqueue functions.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/posendf_amd_interpolation.h"
#include "pndf_complete.h"
#include "pndf_error.h"
#include "pndf_step.h"

// An interior frame of the fill: `bp` is b aligned to a, t = (float)k / (float)(T-1).
PNDF_HD void pndf_interp_fill_quat(const float* a, const float* bp, float t, int mode, float* u) {
#pragma clang fp contract(off)
    float wa = 1.0f - t, wb = t;
    if (mode == PNDF_INTERP_SLERP) {
        float dm[4], dp[4];
        for (int c = 0; c < 4; ++c) {
            dm[c] = a[c] - bp[c];
            dp[c] = a[c] + bp[c];
        }
        const float s = sqrtf(pndf_quat_dot(dm, dm));
        const float p = sqrtf(pndf_quat_dot(dp, dp));
        const float theta = 2.0f * atan2f(s, p);
        const float sn = sinf(theta);
        if (sn > 0.f) {      // false for theta == 0 (a == b') and for a NaN: the linear weights
            const float ta = wa * theta, tb = t * theta;
            wa = sinf(ta) / sn;
            wb = sinf(tb) / sn;
        }
    }
    for (int c = 0; c < 4; ++c) {
        const float xa = wa * a[c];
        const float xb = wb * bp[c];
        u[c] = xa + xb;
    }
    pndf_quat_unit(u);
}

// A free joint quaternion of the band step.  nm / np: the joint in the two neighbour frames, read only when lambda > 0.
// Returns true when the pose rests (tol > 0 && dist < tol): the caller keeps Q.
PNDF_HD bool pndf_interp_band_quat(const float* Q, const float* G, float dist, const float* nm, const float* np, float lambda, float alpha,
                                   float tol, int renorm, float* u) {
#pragma clang fp contract(off)
    pndf_step_descend(Q, G, dist, alpha, u);
    if (lambda > 0.f) {
        float am[4], ap[4];
        pndf_quat_align(Q, nm, am);
        pndf_quat_align(Q, np, ap);
        for (int c = 0; c < 4; ++c) {
            const float sum = am[c] + ap[c];
            const float h = 0.5f * sum;
            const float m = h - Q[c];
            const float lm = lambda * m;
            u[c] = u[c] + lm;
        }
    }
    return pndf_step_finish(dist, tol, renorm, u);
}

// A free joint quaternion of the denoising step (pndf_project_options4; DESIGN.md section 2j "Motion denoising"): the band step with
// end frames that may be free and a data term towards the observation.  `nbr`: which neighbour frames the joint has, bit 0 = nm, bit
// 1 = np -- 3 an interior frame (exactly pndf_interp_band_quat's coupling), 1 or 2 a free end frame with its one neighbour, 0 none (no
// tracks); a neighbour is read only when its bit is set and lambda > 0.  w = mu * conf, rounded once by the caller; `A`, the joint of
// the observation, is read only when w > 0 (false for a zero, negative or NaN weight).  Returns the rest flag of pndf_step_finish.
// pndf_fit_quat is that step with one more term in front of the finish, the keypoint term of a pndf_project_options5 (pndf_fk.h): with
// gk, the gradient d E / d Q of the joint, not null, u <- u - nu * gk.
PNDF_HD bool pndf_fit_quat(const float* Q, const float* G, float dist, const float* nm, const float* np, int nbr, float lambda, const float* A,
                           float w, const float* gk, float nu, float alpha, float tol, int renorm, float* u) {
#pragma clang fp contract(off)
    pndf_step_descend(Q, G, dist, alpha, u);
    if (lambda > 0.f && nbr == 3) {
        float am[4], ap[4];
        pndf_quat_align(Q, nm, am);
        pndf_quat_align(Q, np, ap);
        for (int c = 0; c < 4; ++c) {
            const float sum = am[c] + ap[c];
            const float h = 0.5f * sum;
            const float m = h - Q[c];
            const float lm = lambda * m;
            u[c] = u[c] + lm;
        }
    } else if (lambda > 0.f && nbr != 0) {
        float n[4], an[4];
        for (int c = 0; c < 4; ++c) n[c] = nbr == 1 ? nm[c] : np[c];
        pndf_quat_align(Q, n, an);
        for (int c = 0; c < 4; ++c) {
            const float m = an[c] - Q[c];
            const float h = 0.5f * m;
            const float lm = lambda * h;
            u[c] = u[c] + lm;
        }
    }
    if (w > 0.f) {
        float aa[4];
        pndf_quat_align(Q, A, aa);
        for (int c = 0; c < 4; ++c) {
            const float m = aa[c] - Q[c];
            const float wm = w * m;
            u[c] = u[c] + wm;
        }
    }
    if (gk)
        for (int c = 0; c < 4; ++c) {
            const float s = nu * gk[c];
            u[c] = u[c] - s;
        }
    return pndf_step_finish(dist, tol, renorm, u);
}

PNDF_HD bool pndf_denoise_quat(const float* Q, const float* G, float dist, const float* nm, const float* np, int nbr, float lambda,
                               const float* A, float w, float alpha, float tol, int renorm, float* u) {
    return pndf_fit_quat(Q, G, dist, nm, np, nbr, lambda, A, w, nullptr, 0.f, alpha, tol, renorm, u);
}

// P pairs of T frames are P * T poses for the engine and the kernels: the reason a shape is refused, or nullptr
inline const char* pndf_interp_check_shape(int64_t P, int32_t T) {
    if (T < 2) return "an interpolation has at least two frames (T >= 2)";
    if (P < 0) return "negative pair count";
    if (P > PNDF_COMPLETE_MAX_B / T) return "P * T too large for the step kernel's grid";
    return nullptr;
}
inline const char* pndf_interp_check_mode(int32_t mode) {
    return (mode == PNDF_INTERP_SLERP || mode == PNDF_INTERP_NLERP) ? nullptr : "mode is not a pndf_interp_mode";
}
inline const char* pndf_interp_check_lambda(float lambda) {
    return (lambda >= 0.f && lambda <= 1.f) ? nullptr : "lambda must lie in [0, 1] (and not be NaN)";
}

// the workspace of pndf_interpolate: d [B] padded to a multiple of four floats, dq [B,21,4], the second pose buffer [B,21,4]
inline int64_t pndf_interp_workspace_floats(int64_t B) { return pndf_complete_d_floats(B) + 2 * B * (int64_t)pndf::NQ; }

// Enqueue the kernels on `stream` and nothing else: no validation (the callers have done it), no device selection, no error check
// -- the caller follows them with pndf_check_launch.
PNDF_LOCAL void pndf_interp_fill_enqueue(const float* a, const float* b, float* track, int64_t P, int32_t T, int32_t mode, void* stream);
PNDF_LOCAL void pndf_interp_band_enqueue(const float* q_in, float* q_out, const float* d, const float* dq, const uint32_t* observed,
                                         int64_t P, int32_t T, float lambda, const pndf_project_options& o, void* stream);
