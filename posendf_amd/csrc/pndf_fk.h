// Forward kinematics of a joint tree and the keypoint data term of a pndf_project_options5 (include/posendf_amd.h; DESIGN.md section 2j
// "Keypoint fitting"), written ONCE for the device and the host in the manner of pndf_step.h / pndf_interp.h: the last kernel of the
// skeleton unit (pndf_skeleton.hip, pndf_skel_enc_rev_fit_kernel) and the host twin (pndf_cpu.cpp, compiled without a device pass) call
// these functions, which is why they agree bit for bit.  Every operation is rounded to fp32 on its own, in the order written
// (contraction off in every body); a three-term sum runs as (a0 b0 + a1 b1) + a2 b2.
//
// For one pose Q [J][4] (real part first) on a parent table, rest offsets t [J][3] and K keypoints (joint a(k), local offset o_k):
//   r_j = Q_j / max(|Q_j|, 1e-12)    |.| in pndf_quat_dot's sum order;  R_j = pndf_fk_rot(r_j), the rotation matrix of a unit quaternion
//   root:  G_j = R_j          p_j = t_j
//   else:  G_j = G_pi(j) R_j  p_j = p_pi(j) + G_pi(j) t_j
//   P_k = p_a(k) + G_a(k) o_k        E = 1/2 sum_k w_k |P_k - Y_k|^2, the keypoints in index order; a keypoint whose w_k > 0 is false
//                                    (zero, negative, NaN) takes no part and its target is not read
// and the reverse, joints J-1 .. 0 (children before parents, so a parent takes its children in descending index after its keypoints):
//   ap_j = sum_{a(k)=j} w_k (P_k - Y_k) + sum_children ap_c
//   M_j  = sum_{a(k)=j} w_k (P_k - Y_k) o_k^T + sum_children (ap_c t_c^T + M_c R_c^T)
//   the adjoint of R_j is G_pi(j)^T M_j (M_j for a root); d E / d Q_j goes through R(r) and through r = Q / |Q|:
//   (g_r - r (r . g_r)) / |Q|, and g_r / 1e-12 where the norm is clamped (there the map is linear)
//
// Storage: 24 rows per joint in `W`, row i of a pose at W[i * ld] -- on the device the workspace rows [row][ld] with the pose index
// contiguous (W = base + the lane's column: a lane reads and writes its own column, coalesced; a per-thread array of global
// transforms indexed by a run-time parent would live in scratch memory), on the host a local array with ld = 1.  A child's adjoints
// are added to its parent's rows in place.  Rows: G_j 9 j .., p_j 9 J + 3 j .., M_j 12 J + 9 j .., ap_j 21 J + 3 j ..; once joint j
// is reversed the first four rows of M_j hold d E / d Q_j (pndf_fk_grad_row).  The step that takes nu * d E / d Q_j is pndf_fit_quat of
// pndf_interp.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pndf_step.h"

constexpr int PNDF_FK_MAX_KEYPOINTS = 64;
constexpr int PNDF_FK_ROWS = 24;      // workspace rows per joint

PNDF_HD int pndf_fk_G(int nj, int j) { (void)nj; return 9 * j; }
PNDF_HD int pndf_fk_p(int nj, int j) { return 9 * nj + 3 * j; }
PNDF_HD int pndf_fk_M(int nj, int j) { return 12 * nj + 9 * j; }
PNDF_HD int pndf_fk_ap(int nj, int j) { return 21 * nj + 3 * j; }
PNDF_HD int pndf_fk_grad_row(int nj, int j) { return 12 * nj + 9 * j; }      // rows +0 .. +3: d E / d Q_j

// (a0 b0 + a1 b1) + a2 b2
PNDF_HD float pndf_fk_dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
#pragma clang fp contract(off)
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// r = Q / max(|Q|, 1e-12); returns |Q| as it was computed (a NaN norm stays NaN)
PNDF_HD float pndf_fk_unit(const float* Q, float* r) {
#pragma clang fp contract(off)
    const float n = sqrtf(pndf_quat_dot(Q, Q));
    const float den = (n < 1e-12f) ? 1e-12f : n;
    for (int c = 0; c < 4; ++c) r[c] = Q[c] / den;
    return n;
}

// the rotation matrix of the unit quaternion r = (w, x, y, z), row-major
PNDF_HD void pndf_fk_rot(const float* r, float* R) {
#pragma clang fp contract(off)
    const float w = r[0], x = r[1], y = r[2], z = r[3];
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, xz = x * z, yz = y * z;
    const float wx = w * x, wy = w * y, wz = w * z;
    const float s0 = yy + zz, s1 = xx + zz, s2 = xx + yy;
    R[0] = 1.0f - 2.0f * s0;
    R[4] = 1.0f - 2.0f * s1;
    R[8] = 1.0f - 2.0f * s2;
    const float a01 = xy - wz, a10 = xy + wz, a02 = xz + wy, a20 = xz - wy, a12 = yz - wx, a21 = yz + wx;
    R[1] = 2.0f * a01;
    R[3] = 2.0f * a10;
    R[2] = 2.0f * a02;
    R[6] = 2.0f * a20;
    R[5] = 2.0f * a12;
    R[7] = 2.0f * a21;
}

// The reverse of pndf_fk_rot and of pndf_fk_unit: A = the adjoint of R [9], r and n = pndf_fk_unit's -> g = d E / d Q [4]
PNDF_HD void pndf_fk_quat_adj(const float* A, const float* r, float n, float* g) {
#pragma clang fp contract(off)
    const float w = r[0], x = r[1], y = r[2], z = r[3];
    const float d0 = A[7] - A[5], d1 = A[2] - A[6], d2 = A[3] - A[1];
    const float s01 = A[1] + A[3], s02 = A[2] + A[6], s12 = A[5] + A[7];
    const float t0 = A[4] + A[8], t1 = A[0] + A[8], t2 = A[0] + A[4];
    float gr[4];
    gr[0] = 2.0f * pndf_fk_dot3(x, d0, y, d1, z, d2);
    const float cx = x * t0, cy = y * t1, cz = z * t2;
    const float ex = pndf_fk_dot3(w, d0, y, s01, z, s02) - 2.0f * cx;
    const float ey = pndf_fk_dot3(w, d1, x, s01, z, s12) - 2.0f * cy;
    const float ez = pndf_fk_dot3(w, d2, x, s02, y, s12) - 2.0f * cz;
    gr[1] = 2.0f * ex;
    gr[2] = 2.0f * ey;
    gr[3] = 2.0f * ez;
    if (n < 1e-12f) {      // the clamped norm: r = Q / 1e-12 is linear
        for (int c = 0; c < 4; ++c) g[c] = gr[c] / 1e-12f;
    } else {
        const float dot = pndf_quat_dot(r, gr);
        for (int c = 0; c < 4; ++c) {
            const float rd = r[c] * dot;
            const float t = gr[c] - rd;
            g[c] = t / n;
        }
    }
}

// Forward of joint j (its parent's rows are written already): G_j and p_j stored, M_j and ap_j cleared
PNDF_HD void pndf_fk_joint(const float* Q, int parent, const float* t, float* W, int64_t ld, int nj, int j) {
#pragma clang fp contract(off)
    float r[4], R[9];
    (void)pndf_fk_unit(Q, r);
    pndf_fk_rot(r, R);
    float* Gj = W + (int64_t)pndf_fk_G(nj, j) * ld;
    float* pj = W + (int64_t)pndf_fk_p(nj, j) * ld;
    float* Mj = W + (int64_t)pndf_fk_M(nj, j) * ld;
    float* aj = W + (int64_t)pndf_fk_ap(nj, j) * ld;
    if (parent < 0) {
        for (int i = 0; i < 9; ++i) Gj[i * ld] = R[i];
        for (int a = 0; a < 3; ++a) pj[a * ld] = t[a];
    } else {
        const float* Gp = W + (int64_t)pndf_fk_G(nj, parent) * ld;
        const float* pp = W + (int64_t)pndf_fk_p(nj, parent) * ld;
        for (int a = 0; a < 3; ++a) {
            const float g0 = Gp[(3 * a) * ld], g1 = Gp[(3 * a + 1) * ld], g2 = Gp[(3 * a + 2) * ld];
            for (int b = 0; b < 3; ++b) Gj[(3 * a + b) * ld] = pndf_fk_dot3(g0, R[b], g1, R[3 + b], g2, R[6 + b]);
            const float v = pndf_fk_dot3(g0, t[0], g1, t[1], g2, t[2]);
            pj[a * ld] = pp[a * ld] + v;
        }
    }
    for (int i = 0; i < 9; ++i) Mj[i * ld] = 0.f;
    for (int a = 0; a < 3; ++a) aj[a * ld] = 0.f;
}

// Keypoint on joint `a` at offset o with target Y and weight w > 0: its residual added to ap_a and M_a; returns acc + w |P - Y|^2
PNDF_HD float pndf_fk_keypoint(int a, const float* o, const float* Y, float w, float acc, float* W, int64_t ld, int nj) {
#pragma clang fp contract(off)
    const float* Ga = W + (int64_t)pndf_fk_G(nj, a) * ld;
    const float* pa = W + (int64_t)pndf_fk_p(nj, a) * ld;
    float* Ma = W + (int64_t)pndf_fk_M(nj, a) * ld;
    float* aa = W + (int64_t)pndf_fk_ap(nj, a) * ld;
    float res[3];
    for (int x = 0; x < 3; ++x) {
        const float v = pndf_fk_dot3(Ga[(3 * x) * ld], o[0], Ga[(3 * x + 1) * ld], o[1], Ga[(3 * x + 2) * ld], o[2]);
        const float P = pa[x * ld] + v;
        res[x] = P - Y[x];
    }
    const float ss = pndf_fk_dot3(res[0], res[0], res[1], res[1], res[2], res[2]);
    const float e = w * ss;
    for (int x = 0; x < 3; ++x) {
        const float wr = w * res[x];
        aa[x * ld] = aa[x * ld] + wr;
        for (int y = 0; y < 3; ++y) {
            const float m = wr * o[y];
            Ma[(3 * x + y) * ld] = Ma[(3 * x + y) * ld] + m;
        }
    }
    return acc + e;
}

// Reverse of joint j (its children are reversed already): ap_j and M_j are added to the parent's, d E / d Q_j is stored
PNDF_HD void pndf_fk_joint_rev(const float* Q, int parent, const float* t, float* W, int64_t ld, int nj, int j) {
#pragma clang fp contract(off)
    float r[4], R[9], M[9], A[9], g[4];
    const float n = pndf_fk_unit(Q, r);
    pndf_fk_rot(r, R);
    float* Mj = W + (int64_t)pndf_fk_M(nj, j) * ld;
    for (int i = 0; i < 9; ++i) M[i] = Mj[i * ld];
    if (parent < 0) {
        for (int i = 0; i < 9; ++i) A[i] = M[i];
    } else {
        const float* Gp = W + (int64_t)pndf_fk_G(nj, parent) * ld;
        const float* aj = W + (int64_t)pndf_fk_ap(nj, j) * ld;
        float* Mp = W + (int64_t)pndf_fk_M(nj, parent) * ld;
        float* ap = W + (int64_t)pndf_fk_ap(nj, parent) * ld;
        for (int a = 0; a < 3; ++a) {      // A = G_pi^T M
            const float g0 = Gp[a * ld], g1 = Gp[(3 + a) * ld], g2 = Gp[(6 + a) * ld];
            for (int b = 0; b < 3; ++b) A[3 * a + b] = pndf_fk_dot3(g0, M[b], g1, M[3 + b], g2, M[6 + b]);
        }
        for (int a = 0; a < 3; ++a) {
            const float av = aj[a * ld];
            ap[a * ld] = ap[a * ld] + av;
            for (int b = 0; b < 3; ++b) {      // ap t^T + M R^T
                const float at = av * t[b];
                const float mr = pndf_fk_dot3(M[3 * a], R[3 * b], M[3 * a + 1], R[3 * b + 1], M[3 * a + 2], R[3 * b + 2]);
                const float add = at + mr;
                Mp[(3 * a + b) * ld] = Mp[(3 * a + b) * ld] + add;
            }
        }
    }
    pndf_fk_quat_adj(A, r, n, g);
    float* gj = W + (int64_t)pndf_fk_grad_row(nj, j) * ld;
    for (int c = 0; c < 4; ++c) gj[c * ld] = g[c];
}

// The whole term of one pose: q [nj][4] the iterate, rest [nj][3], kp_joint [K], kp_offset [K][3], Y [K][3], conf [K] or null (ones).
// Leaves d E / d Q_j in the rows pndf_fk_grad_row(nj, j) and returns E.
PNDF_HD float pndf_fk_energy_grad(const float* q, int nj, const int* parent, const float* rest, int K, const int32_t* kp_joint,
                                  const float* kp_offset, const float* Y, const float* conf, float* W, int64_t ld) {
#pragma clang fp contract(off)
    for (int j = 0; j < nj; ++j) pndf_fk_joint(q + 4 * j, parent[j], rest + 3 * j, W, ld, nj, j);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float w = conf ? conf[k] : 1.0f;
        if (w > 0.f) acc = pndf_fk_keypoint(kp_joint[k], kp_offset + 3 * k, Y + 3 * k, w, acc, W, ld, nj);
    }
    for (int j = nj - 1; j >= 0; --j) pndf_fk_joint_rev(q + 4 * j, parent[j], rest + 3 * j, W, ld, nj, j);
    return 0.5f * acc;
}
