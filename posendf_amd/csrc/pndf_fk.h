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
// pndf_interp.h.  The camera term of a pndf_project_options6 -- a root per pose, a pinhole residual -- is a second entry further down.
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

// ---- The camera term of a pndf_project_options6 (DESIGN.md section 2j "Image fitting"): the same tree, with a placement of it in the
// target's frame (the "root" of a pose: c [4] a raw quaternion, real part first, s [3] a translation) and, with PNDF_KP_IMAGE, a pinhole
// camera in front of the residual.  Stated once beside the 3D term, whose functions above stay as they are (their bits are pinned):
//   c^ = pndf_fk_unit(c), R_c = pndf_fk_rot(c^);  C_k = R_c P_k + s, rows as pndf_fk_dot3;  without a root C_k = P_k, no arithmetic
//   3D:     e = C - Y,  E = 1/2 sum_k w_k |e|^2,  a_k = w_k e
//   image:  a keypoint for which C_z > 0 is false takes no part;  n = (C_x / C_z, C_y / C_z),  y' = ((Y_u - cx) / fx, (Y_v - cy) / fy),
//           e = n - y',  E = 1/2 sum_k w_k [rho(e_u) + rho(e_v)],  a_k = w_k (psi_u / C_z, psi_v / C_z, -(psi_u n_u + psi_v n_v) / C_z)
//           rho(e) = e^2 and psi(e) = e for rho == 0, else with r2 = rho rho, d = e e + r2:  (r2 (e e)) / d  and  (e (r2 r2)) / (d d)
//   d E / d P_k = R_c^T a_k goes into ap and M as w_k (P_k - Y_k) does above;  d E / d s = sum_k a_k;  the adjoint of R_c is
//   sum_k a_k P_k^T and d E / d c = pndf_fk_quat_adj of it.  The root's adjoints are 3 + 9 accumulators with fixed indices: registers.
struct PndfFkCamera {
    float fx, fy, cx, cy;      // read only with `image`
    float rho;                 // the robustifier of the image residual; 0 = squared error
    int image;                 // PNDF_KP_IMAGE: targets are [K][2] pixels
};

// rho(e) and psi(e) = 1/2 rho'(e)
PNDF_HD float pndf_fk_robust(float e, float rho, float* psi) {
#pragma clang fp contract(off)
    const float ee = e * e;
    if (rho == 0.f) {
        *psi = e;
        return ee;
    }
    const float r2 = rho * rho;
    const float d = ee + r2;
    const float num = r2 * ee;
    const float r4 = r2 * r2;
    const float en = e * r4;
    const float dd = d * d;
    *psi = en / dd;
    return num / d;
}

// Keypoint on joint `a` at offset o with weight w > 0 under the camera: Y its target ([3], or [2] pixels), Rc / s the root (read only when
// has_root: a flag and not a null pointer, so that on the device the arrays stay registers).
// Its adjoint goes to ap_a and M_a and to the root's accumulators as [3] and AR [9]; returns acc + its energy (twice E's share).
PNDF_HD float pndf_fk_camera_keypoint(int a, const float* o, const float* Y, float w, float acc, const PndfFkCamera& cam, bool has_root,
                                      const float* Rc, const float* s, float* as, float* AR, float* W, int64_t ld, int nj) {
#pragma clang fp contract(off)
    const float* Ga = W + (int64_t)pndf_fk_G(nj, a) * ld;
    const float* pa = W + (int64_t)pndf_fk_p(nj, a) * ld;
    float* Ma = W + (int64_t)pndf_fk_M(nj, a) * ld;
    float* aa = W + (int64_t)pndf_fk_ap(nj, a) * ld;
    float P[3], C[3], adj[3];
    for (int x = 0; x < 3; ++x) {
        const float v = pndf_fk_dot3(Ga[(3 * x) * ld], o[0], Ga[(3 * x + 1) * ld], o[1], Ga[(3 * x + 2) * ld], o[2]);
        P[x] = pa[x * ld] + v;
    }
    if (has_root) {
        for (int x = 0; x < 3; ++x) {
            const float v = pndf_fk_dot3(Rc[3 * x], P[0], Rc[3 * x + 1], P[1], Rc[3 * x + 2], P[2]);
            C[x] = v + s[x];
        }
    } else {
        for (int x = 0; x < 3; ++x) C[x] = P[x];
    }
    float e;
    if (cam.image) {
        if (!(C[2] > 0.f)) return acc;      // behind the camera, in its plane, or NaN: no energy, no gradient
        const float nu = C[0] / C[2], nv = C[1] / C[2];
        const float du = Y[0] - cam.cx, dv = Y[1] - cam.cy;
        const float yu = du / cam.fx, yv = dv / cam.fy;
        const float eu = nu - yu, ev = nv - yv;
        float pu, pv;
        const float ru = pndf_fk_robust(eu, cam.rho, &pu);
        const float rv = pndf_fk_robust(ev, cam.rho, &pv);
        const float rs = ru + rv;
        e = w * rs;
        const float tu = pu / C[2], tv = pv / C[2];
        const float un = pu * nu, vn = pv * nv;
        const float sn = un + vn;
        const float tz = -(sn / C[2]);
        adj[0] = w * tu;
        adj[1] = w * tv;
        adj[2] = w * tz;
    } else {
        float res[3];
        for (int x = 0; x < 3; ++x) res[x] = C[x] - Y[x];
        const float ss = pndf_fk_dot3(res[0], res[0], res[1], res[1], res[2], res[2]);
        e = w * ss;
        for (int x = 0; x < 3; ++x) adj[x] = w * res[x];
    }
    if (has_root)
        for (int x = 0; x < 3; ++x) {
            as[x] = as[x] + adj[x];
            for (int y = 0; y < 3; ++y) {
                const float m = adj[x] * P[y];
                AR[3 * x + y] = AR[3 * x + y] + m;
            }
        }
    for (int x = 0; x < 3; ++x) {
        const float wr = has_root ? pndf_fk_dot3(Rc[x], adj[0], Rc[3 + x], adj[1], Rc[6 + x], adj[2]) : adj[x];      // R_c^T a
        aa[x * ld] = aa[x * ld] + wr;
        for (int y = 0; y < 3; ++y) {
            const float m = wr * o[y];
            Ma[(3 * x + y) * ld] = Ma[(3 * x + y) * ld] + m;
        }
    }
    return acc + e;
}

// The whole term of one pose under the camera: pndf_fk_energy_grad's arguments, Y [K][3] or [K][2], and root [7] = (c, s), read only when
// has_root (else groot is not written).  Leaves d E / d Q_j in the rows pndf_fk_grad_row(nj, j), d E / d c in groot [0..3] and d E / d s in groot [4..6],
// and returns E.  Without a root and without cam.image it computes pndf_fk_energy_grad's bits.
PNDF_HD float pndf_fk_camera_energy_grad(const float* q, int nj, const int* parent, const float* rest, int K, const int32_t* kp_joint,
                                         const float* kp_offset, const float* Y, const float* conf, bool has_root,
                                         const float* root, const PndfFkCamera& cam, float* groot, float* W, int64_t ld) {
#pragma clang fp contract(off)
    for (int j = 0; j < nj; ++j) pndf_fk_joint(q + 4 * j, parent[j], rest + 3 * j, W, ld, nj, j);
    float ch[4] = {0.f, 0.f, 0.f, 0.f}, Rc[9], s[3] = {0.f, 0.f, 0.f}, n = 0.f;
    float as[3] = {0.f, 0.f, 0.f}, AR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 9; ++i) Rc[i] = 0.f;
    if (has_root) {
        float c[4];
        for (int i = 0; i < 4; ++i) c[i] = root[i];
        for (int x = 0; x < 3; ++x) s[x] = root[4 + x];
        n = pndf_fk_unit(c, ch);
        pndf_fk_rot(ch, Rc);
    }
    const int dims = cam.image ? 2 : 3;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float w = conf ? conf[k] : 1.0f;
        if (w > 0.f)
            acc = pndf_fk_camera_keypoint(kp_joint[k], kp_offset + 3 * k, Y + dims * k, w, acc, cam, has_root, Rc, s, as, AR, W, ld, nj);
    }
    for (int j = nj - 1; j >= 0; --j) pndf_fk_joint_rev(q + 4 * j, parent[j], rest + 3 * j, W, ld, nj, j);
    if (has_root) {
        pndf_fk_quat_adj(AR, ch, n, groot);
        for (int x = 0; x < 3; ++x) groot[4 + x] = as[x];
    }
    return 0.5f * acc;
}

// The root's own step: root [7] at the step's input, groot of pndf_fk_camera_energy_grad -> out [7].  A pose that rests under tol keeps
// its root; s <- s - nu_trans * dE/ds when nu_trans > 0, c <- pndf_fk_unit(c - nu_rot * dE/dc) when nu_rot > 0; a part whose weight is
// zero keeps its bits.
PNDF_HD void pndf_fk_root_step(const float* root, const float* groot, float nu_rot, float nu_trans, float dist, float tol, float* out) {
#pragma clang fp contract(off)
    for (int i = 0; i < 7; ++i) out[i] = root[i];
    if (tol > 0.f && dist < tol) return;
    if (nu_rot > 0.f) {
        float u[4];
        for (int i = 0; i < 4; ++i) {
            const float t = nu_rot * groot[i];
            u[i] = root[i] - t;
        }
        (void)pndf_fk_unit(u, out);
    }
    if (nu_trans > 0.f)
        for (int x = 0; x < 3; ++x) {
            const float t = nu_trans * groot[4 + x];
            out[4 + x] = root[4 + x] - t;
        }
}

// The root's step of a pndf_project_options9 (DESIGN.md section 2j "Root trajectory"): pndf_fk_root_step above -- which stays as it is, its
// bits are pinned -- with the root coupled to the roots of the neighbour frames of its track and drawn towards an anchor.  root [7] at the
// step's input, groot as above -> out [7], which must not be `root` or a neighbour's row: the step is Jacobi, every frame reads its
// neighbours as the step before left them.  nm / np: the root rows of frames k - 1 / k + 1, read only where `nbr` has bit 0 / bit 1 and
// the part's lambda and nu are positive; A: the anchor's row, a part of it read only when that part's mu and nu are positive.  nbr 3: an
// interior frame, 1 or 2: an end frame with its one neighbour, 0: none.  The coupling and the data term MIRROR pndf_fit_quat of
// pndf_interp.h under PNDF_TRACK_FREE_ENDS, operation for operation: that function's coupling sits between a descent along dist * G and
// a renorm mode, neither of which the root has, so it does not separate.  The translation takes the same three parts per component
// without alignment or normalisation.  A pose that rests under tol keeps its root; a part whose nu is zero keeps its bits.
PNDF_HD void pndf_fk_root_smooth_step(const float* root, const float* groot, float nu_rot, float nu_trans, float dist, float tol,
                                      const float* nm, const float* np, int nbr, float lambda_rot, float lambda_trans, const float* A,
                                      float mu_rot, float mu_trans, float* out) {
#pragma clang fp contract(off)
    for (int i = 0; i < 7; ++i) out[i] = root[i];
    if (tol > 0.f && dist < tol) return;
    if (nu_rot > 0.f) {
        float u[4];
        for (int i = 0; i < 4; ++i) {
            const float t = nu_rot * groot[i];
            u[i] = root[i] - t;
        }
        if (lambda_rot > 0.f && nbr == 3) {
            float m_[4], p_[4], am[4], ap[4];
            for (int i = 0; i < 4; ++i) {
                m_[i] = nm[i];
                p_[i] = np[i];
            }
            pndf_quat_align(root, m_, am);
            pndf_quat_align(root, p_, ap);
            for (int i = 0; i < 4; ++i) {
                const float sum = am[i] + ap[i];
                const float h = 0.5f * sum;
                const float m = h - root[i];
                const float lm = lambda_rot * m;
                u[i] = u[i] + lm;
            }
        } else if (lambda_rot > 0.f && nbr != 0) {
            float n[4], an[4];
            for (int i = 0; i < 4; ++i) n[i] = nbr == 1 ? nm[i] : np[i];
            pndf_quat_align(root, n, an);
            for (int i = 0; i < 4; ++i) {
                const float m = an[i] - root[i];
                const float h = 0.5f * m;
                const float lm = lambda_rot * h;
                u[i] = u[i] + lm;
            }
        }
        if (mu_rot > 0.f) {
            float a[4], aa[4];
            for (int i = 0; i < 4; ++i) a[i] = A[i];
            pndf_quat_align(root, a, aa);
            for (int i = 0; i < 4; ++i) {
                const float m = aa[i] - root[i];
                const float wm = mu_rot * m;
                u[i] = u[i] + wm;
            }
        }
        (void)pndf_fk_unit(u, out);
    }
    if (nu_trans > 0.f)
        for (int x = 4; x < 7; ++x) {
            const float t = nu_trans * groot[x];
            float u = root[x] - t;
            if (lambda_trans > 0.f && nbr == 3) {
                const float sum = nm[x] + np[x];
                const float h = 0.5f * sum;
                const float m = h - root[x];
                const float lm = lambda_trans * m;
                u = u + lm;
            } else if (lambda_trans > 0.f && nbr != 0) {
                const float n = nbr == 1 ? nm[x] : np[x];
                const float m = n - root[x];
                const float h = 0.5f * m;
                const float lm = lambda_trans * h;
                u = u + lm;
            }
            if (mu_trans > 0.f) {
                const float m = A[x] - root[x];
                const float wm = mu_trans * m;
                u = u + wm;
            }
            out[x] = u;
        }
}

// ---- Bone lengths of a pndf_project_options7 (DESIGN.md section 2j "Bone lengths"): the camera term above on a tree whose rest offsets and
// keypoint offsets are scaled, t'_j = sigma_j t_j and o'_k = sigma_{J+k} o_k per component, and the gradient of E with respect to the
// S = J + K scales.  Stated once beside the other terms, whose functions above stay as they are (their bits are pinned); with every scale
// 1.0f the products are exact and the term computes pndf_fk_camera_energy_grad's bits.
//   joint j:     h_j = <ap_j, v_j> with ap_j complete (its own keypoints and all its children: joint j is about to be reversed) and
//                v_j = G_pi(j) t_j, three pndf_fk_dot3 rows on the unscaled t_j; v_j = t_j for a root; the product a pndf_fk_dot3
//   keypoint k:  h_{J+k} = <dE/dP_k, G_a(k) o_k>, dE/dP_k what goes into ap; a skipped keypoint gives exactly 0
// h is left in the S rows pndf_fk_len_row(nj, i) of W, behind the 24 J rows of the tree.  The scales are read through a pointer with a
// run-time index (on the device: the group's row in global memory, not a per-thread array); t' and o' are three values at a time.
PNDF_HD int pndf_fk_len_row(int nj, int i) { return PNDF_FK_ROWS * nj + i; }
constexpr int PNDF_FK_LEN_BLOCK = 64;      // frames per partial sum of pndf_fk_len_group_sum

// pndf_fk_camera_keypoint on the scaled offset sg * o; *h = <R_c^T a, G_a o> (0 when the keypoint is skipped behind the camera)
PNDF_HD float pndf_fk_len_keypoint(int a, const float* o, float sg, const float* Y, float w, float acc, const PndfFkCamera& cam, bool has_root,
                                   const float* Rc, const float* s, float* as, float* AR, float* W, int64_t ld, int nj, float* h) {
#pragma clang fp contract(off)
    const float* Ga = W + (int64_t)pndf_fk_G(nj, a) * ld;
    const float* pa = W + (int64_t)pndf_fk_p(nj, a) * ld;
    float* Ma = W + (int64_t)pndf_fk_M(nj, a) * ld;
    float* aa = W + (int64_t)pndf_fk_ap(nj, a) * ld;
    float os[3], P[3], C[3], adj[3], vu[3];
    *h = 0.f;
    for (int x = 0; x < 3; ++x) os[x] = sg * o[x];
    for (int x = 0; x < 3; ++x) {
        const float v = pndf_fk_dot3(Ga[(3 * x) * ld], os[0], Ga[(3 * x + 1) * ld], os[1], Ga[(3 * x + 2) * ld], os[2]);
        P[x] = pa[x * ld] + v;
        vu[x] = pndf_fk_dot3(Ga[(3 * x) * ld], o[0], Ga[(3 * x + 1) * ld], o[1], Ga[(3 * x + 2) * ld], o[2]);
    }
    if (has_root) {
        for (int x = 0; x < 3; ++x) {
            const float v = pndf_fk_dot3(Rc[3 * x], P[0], Rc[3 * x + 1], P[1], Rc[3 * x + 2], P[2]);
            C[x] = v + s[x];
        }
    } else {
        for (int x = 0; x < 3; ++x) C[x] = P[x];
    }
    float e;
    if (cam.image) {
        if (!(C[2] > 0.f)) return acc;      // behind the camera, in its plane, or NaN: no energy, no gradient
        const float nu = C[0] / C[2], nv = C[1] / C[2];
        const float du = Y[0] - cam.cx, dv = Y[1] - cam.cy;
        const float yu = du / cam.fx, yv = dv / cam.fy;
        const float eu = nu - yu, ev = nv - yv;
        float pu, pv;
        const float ru = pndf_fk_robust(eu, cam.rho, &pu);
        const float rv = pndf_fk_robust(ev, cam.rho, &pv);
        const float rs = ru + rv;
        e = w * rs;
        const float tu = pu / C[2], tv = pv / C[2];
        const float un = pu * nu, vn = pv * nv;
        const float sn = un + vn;
        const float tz = -(sn / C[2]);
        adj[0] = w * tu;
        adj[1] = w * tv;
        adj[2] = w * tz;
    } else {
        float res[3];
        for (int x = 0; x < 3; ++x) res[x] = C[x] - Y[x];
        const float ss = pndf_fk_dot3(res[0], res[0], res[1], res[1], res[2], res[2]);
        e = w * ss;
        for (int x = 0; x < 3; ++x) adj[x] = w * res[x];
    }
    if (has_root)
        for (int x = 0; x < 3; ++x) {
            as[x] = as[x] + adj[x];
            for (int y = 0; y < 3; ++y) {
                const float m = adj[x] * P[y];
                AR[3 * x + y] = AR[3 * x + y] + m;
            }
        }
    float wr[3];
    for (int x = 0; x < 3; ++x) {
        wr[x] = has_root ? pndf_fk_dot3(Rc[x], adj[0], Rc[3 + x], adj[1], Rc[6 + x], adj[2]) : adj[x];      // R_c^T a
        aa[x * ld] = aa[x * ld] + wr[x];
        for (int y = 0; y < 3; ++y) {
            const float m = wr[x] * os[y];
            Ma[(3 * x + y) * ld] = Ma[(3 * x + y) * ld] + m;
        }
    }
    *h = pndf_fk_dot3(wr[0], vu[0], wr[1], vu[1], wr[2], vu[2]);
    return acc + e;
}

// The whole term of one pose on the scaled tree: pndf_fk_camera_energy_grad's arguments and sigma [nj + K], the scales of the pose's
// group at the step's input.  Leaves d E / d Q_j in the rows pndf_fk_grad_row(nj, j), d E / d sigma_i in the rows pndf_fk_len_row(nj, i),
// d E / d (c, s) in groot, and returns E.
PNDF_HD float pndf_fk_len_energy_grad(const float* q, int nj, const int* parent, const float* rest, int K, const int32_t* kp_joint,
                                      const float* kp_offset, const float* Y, const float* conf, bool has_root, const float* root,
                                      const PndfFkCamera& cam, const float* sigma, float* groot, float* W, int64_t ld) {
#pragma clang fp contract(off)
    for (int j = 0; j < nj; ++j) {
        const float sg = sigma[j];
        float ts[3];
        for (int x = 0; x < 3; ++x) ts[x] = sg * rest[3 * j + x];
        pndf_fk_joint(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    float ch[4] = {0.f, 0.f, 0.f, 0.f}, Rc[9], s[3] = {0.f, 0.f, 0.f}, n = 0.f;
    float as[3] = {0.f, 0.f, 0.f}, AR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 9; ++i) Rc[i] = 0.f;
    if (has_root) {
        float c[4];
        for (int i = 0; i < 4; ++i) c[i] = root[i];
        for (int x = 0; x < 3; ++x) s[x] = root[4 + x];
        n = pndf_fk_unit(c, ch);
        pndf_fk_rot(ch, Rc);
    }
    const int dims = cam.image ? 2 : 3;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float w = conf ? conf[k] : 1.0f;
        float h = 0.f;
        if (w > 0.f)
            acc = pndf_fk_len_keypoint(kp_joint[k], kp_offset + 3 * k, sigma[nj + k], Y + dims * k, w, acc, cam, has_root, Rc, s, as, AR, W, ld,
                                       nj, &h);
        W[(int64_t)pndf_fk_len_row(nj, nj + k) * ld] = h;
    }
    for (int j = nj - 1; j >= 0; --j) {
        const float* t = rest + 3 * j;
        const float* aj = W + (int64_t)pndf_fk_ap(nj, j) * ld;
        const float sg = sigma[j];
        float ts[3], v[3];
        for (int x = 0; x < 3; ++x) ts[x] = sg * t[x];
        if (parent[j] < 0) {
            for (int x = 0; x < 3; ++x) v[x] = t[x];
        } else {
            const float* Gp = W + (int64_t)pndf_fk_G(nj, parent[j]) * ld;
            for (int x = 0; x < 3; ++x) v[x] = pndf_fk_dot3(Gp[(3 * x) * ld], t[0], Gp[(3 * x + 1) * ld], t[1], Gp[(3 * x + 2) * ld], t[2]);
        }
        W[(int64_t)pndf_fk_len_row(nj, j) * ld] = pndf_fk_dot3(aj[0], v[0], aj[ld], v[1], aj[2 * ld], v[2]);
        pndf_fk_joint_rev(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    if (has_root) {
        pndf_fk_quat_adj(AR, ch, n, groot);
        for (int x = 0; x < 3; ++x) groot[4 + x] = as[x];
    }
    return 0.5f * acc;
}

// The sum of a group: h of frame f at h[f * stride], n >= 1 frames.  The partial of every block of PNDF_FK_LEN_BLOCK consecutive frames is
// accumulated in frame order from 0.0f (the last block may be shorter); the partials are added in block order from 0.0f.
PNDF_HD float pndf_fk_len_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
PNDF_HD float pndf_fk_len_block_sum(const float* h, int64_t stride, int64_t f0, int64_t f1) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int64_t f = f0; f < f1; ++f) acc = acc + h[f * stride];
    return acc;
}
PNDF_HD float pndf_fk_len_group_sum(const float* h, int64_t stride, int64_t n) {
#pragma clang fp contract(off)
    float total = 0.f;
    for (int64_t f0 = 0; f0 < n; f0 += PNDF_FK_LEN_BLOCK) {
        const int64_t f1 = f0 + PNDF_FK_LEN_BLOCK < n ? f0 + PNDF_FK_LEN_BLOCK : n;
        total = pndf_fk_len_add(total, pndf_fk_len_block_sum(h, stride, f0, f1));
    }
    return total;
}

// The step of one scale: sigma at the step's input, H the group's sum over its n frames, w = nu_len * rate (formed by the caller, rounded
// once), `rests`: tol > 0 and every frame of the group rests.  Returns the new scale; where it returns sigma the scale keeps its bits.
PNDF_HD float pndf_fk_len_step(float sigma, float H, int64_t n, float w, float kappa, float len_min, float len_max, bool rests) {
#pragma clang fp contract(off)
    if (!(w > 0.f) || rests) return sigma;
    const float m = H / (float)n;
    const float d1 = sigma - 1.0f;
    const float pr = kappa * d1;
    const float gsum = m + pr;
    const float t = w * gsum;
    const float v = sigma - t;
    if (len_min == 0.f && len_max == 0.f) return v;
    return v < len_min ? len_min : (v > len_max ? len_max : v);
}

// ---- Several cameras of a pndf_project_options8 (DESIGN.md section 2j "Several cameras"): the image term above seen by V calibrated
// views of the same frame.  Stated once beside the other terms, whose functions above stay as they are (their bits are pinned).  The
// root places the tree in a WORLD frame, W_k = R_c P_k + s (without a root W_k = P_k, no arithmetic: what pndf_fk_len_keypoint computes
// as C); view v is a row of 16 floats, fx fy cx cy, R_v [9] row-major (world -> camera), t_v [3], and C_vk = R_v W_k + t_v, rows as
// pndf_fk_dot3, then the add.  Keypoints in the outer loop, views 0 .. V-1 in the inner one:
//   a view takes no part for a keypoint when w_vk > 0 is false (w_vk = conf [v][k], or 1) or when C_z > 0 is false; its target
//   Y [v][k][2] is then not read.  A view that takes part gives e, rho, psi and a_vk as pndf_fk_camera_keypoint does with its own
//   intrinsics; its energy share is added to the accumulator in view order, and aW_k = sum_v R_v^T a_vk is accumulated in view order
//   from 0.0f.  After the views aW_k takes the place of a_k: in as and AR (with P_k), as R_c^T aW_k in ap and M, and in h_{J+k} -- only
//   when at least one view took part; otherwise the keypoint adds nothing anywhere (h_{J+k} = 0).
// The view table is uniform over the poses (on the device: values of the kernel's argument struct, read with scalar loads; the view
// loop has a uniform trip count and nothing per lane is indexed by the view).  sigma may be null: every scale 1.0f, no product.
constexpr int PNDF_FK_VIEW_FLOATS = 16;      // (at most PNDF_FK_MAX_VIEWS rows: include/posendf_amd.h)

PNDF_HD float pndf_fk_views_keypoint(int a, const float* o, bool scaled, float sg, int k, int K, const float* Y, const float* conf, float acc,
                                     float rho, int V, const float* views, bool has_root, const float* Rc, const float* s, float* as,
                                     float* AR, float* W, int64_t ld, int nj, float* h) {
#pragma clang fp contract(off)
    const float* Ga = W + (int64_t)pndf_fk_G(nj, a) * ld;
    const float* pa = W + (int64_t)pndf_fk_p(nj, a) * ld;
    float* Ma = W + (int64_t)pndf_fk_M(nj, a) * ld;
    float* aa = W + (int64_t)pndf_fk_ap(nj, a) * ld;
    float os[3], P[3], Wd[3], vu[3];
    *h = 0.f;
    for (int x = 0; x < 3; ++x) os[x] = scaled ? sg * o[x] : o[x];
    for (int x = 0; x < 3; ++x) {
        const float v = pndf_fk_dot3(Ga[(3 * x) * ld], os[0], Ga[(3 * x + 1) * ld], os[1], Ga[(3 * x + 2) * ld], os[2]);
        P[x] = pa[x * ld] + v;
        vu[x] = pndf_fk_dot3(Ga[(3 * x) * ld], o[0], Ga[(3 * x + 1) * ld], o[1], Ga[(3 * x + 2) * ld], o[2]);
    }
    if (has_root) {
        for (int x = 0; x < 3; ++x) {
            const float v = pndf_fk_dot3(Rc[3 * x], P[0], Rc[3 * x + 1], P[1], Rc[3 * x + 2], P[2]);
            Wd[x] = v + s[x];
        }
    } else {
        for (int x = 0; x < 3; ++x) Wd[x] = P[x];
    }
    float aW[3] = {0.f, 0.f, 0.f};
    bool seen = false;
    for (int v = 0; v < V; ++v) {
        const float* vw = views + PNDF_FK_VIEW_FLOATS * v;
        const float w = conf ? conf[v * K + k] : 1.0f;
        if (!(w > 0.f)) continue;
        float C[3];
        for (int x = 0; x < 3; ++x) {
            const float d = pndf_fk_dot3(vw[4 + 3 * x], Wd[0], vw[5 + 3 * x], Wd[1], vw[6 + 3 * x], Wd[2]);
            C[x] = d + vw[13 + x];
        }
        if (!(C[2] > 0.f)) continue;      // behind this camera, in its plane, or NaN: no energy, no gradient from this view
        const float* y = Y + 2 * (v * K + k);
        const float nu = C[0] / C[2], nv = C[1] / C[2];
        const float du = y[0] - vw[2], dv = y[1] - vw[3];
        const float yu = du / vw[0], yv = dv / vw[1];
        const float eu = nu - yu, ev = nv - yv;
        float pu, pv;
        const float ru = pndf_fk_robust(eu, rho, &pu);
        const float rv = pndf_fk_robust(ev, rho, &pv);
        const float rs = ru + rv;
        const float e = w * rs;
        acc = acc + e;
        const float tu = pu / C[2], tv = pv / C[2];
        const float un = pu * nu, vn = pv * nv;
        const float sn = un + vn;
        const float tz = -(sn / C[2]);
        const float a0 = w * tu, a1 = w * tv, a2 = w * tz;
        for (int x = 0; x < 3; ++x) {      // R_v^T a
            const float d = pndf_fk_dot3(vw[4 + x], a0, vw[7 + x], a1, vw[10 + x], a2);
            aW[x] = aW[x] + d;
        }
        seen = true;
    }
    if (!seen) return acc;
    if (has_root)
        for (int x = 0; x < 3; ++x) {
            as[x] = as[x] + aW[x];
            for (int y = 0; y < 3; ++y) {
                const float m = aW[x] * P[y];
                AR[3 * x + y] = AR[3 * x + y] + m;
            }
        }
    float wr[3];
    for (int x = 0; x < 3; ++x) {
        wr[x] = has_root ? pndf_fk_dot3(Rc[x], aW[0], Rc[3 + x], aW[1], Rc[6 + x], aW[2]) : aW[x];      // R_c^T aW
        aa[x * ld] = aa[x * ld] + wr[x];
        for (int y = 0; y < 3; ++y) {
            const float m = wr[x] * os[y];
            Ma[(3 * x + y) * ld] = Ma[(3 * x + y) * ld] + m;
        }
    }
    *h = pndf_fk_dot3(wr[0], vu[0], wr[1], vu[1], wr[2], vu[2]);
    return acc;
}

// The whole term of one pose under V views: pndf_fk_len_energy_grad's arguments with Y [V][K][2] pixels, conf [V][K] or null (ones),
// views [V][16] and sigma [nj + K] or null (all ones).  Leaves d E / d Q_j in the rows pndf_fk_grad_row(nj, j), d E / d sigma_i in the rows
// pndf_fk_len_row(nj, i) (only with sigma: without scales those rows are neither computed for the joints nor written), d E / d (c, s) in
// groot, and returns E.
PNDF_HD float pndf_fk_views_energy_grad(const float* q, int nj, const int* parent, const float* rest, int K, const int32_t* kp_joint,
                                        const float* kp_offset, const float* Y, const float* conf, bool has_root, const float* root,
                                        float rho, int V, const float* views, const float* sigma, float* groot, float* W, int64_t ld) {
#pragma clang fp contract(off)
    const bool scaled = sigma != nullptr;
    for (int j = 0; j < nj; ++j) {
        float ts[3];
        for (int x = 0; x < 3; ++x) ts[x] = scaled ? sigma[j] * rest[3 * j + x] : rest[3 * j + x];
        pndf_fk_joint(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    float ch[4] = {0.f, 0.f, 0.f, 0.f}, Rc[9], s[3] = {0.f, 0.f, 0.f}, n = 0.f;
    float as[3] = {0.f, 0.f, 0.f}, AR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 9; ++i) Rc[i] = 0.f;
    if (has_root) {
        float c[4];
        for (int i = 0; i < 4; ++i) c[i] = root[i];
        for (int x = 0; x < 3; ++x) s[x] = root[4 + x];
        n = pndf_fk_unit(c, ch);
        pndf_fk_rot(ch, Rc);
    }
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        float h = 0.f;
        acc = pndf_fk_views_keypoint(kp_joint[k], kp_offset + 3 * k, scaled, scaled ? sigma[nj + k] : 1.0f, k, K, Y, conf, acc, rho, V, views,
                                     has_root, Rc, s, as, AR, W, ld, nj, &h);
        if (scaled) W[(int64_t)pndf_fk_len_row(nj, nj + k) * ld] = h;      // (without scales nobody reads the rows of h: they are not written)
    }
    for (int j = nj - 1; j >= 0; --j) {
        const float* t = rest + 3 * j;
        const float* aj = W + (int64_t)pndf_fk_ap(nj, j) * ld;
        float ts[3], v[3] = {0.f, 0.f, 0.f};
        for (int x = 0; x < 3; ++x) ts[x] = scaled ? sigma[j] * t[x] : t[x];
        if (scaled) {
            if (parent[j] < 0) {
                for (int x = 0; x < 3; ++x) v[x] = t[x];
            } else {
                const float* Gp = W + (int64_t)pndf_fk_G(nj, parent[j]) * ld;
                for (int x = 0; x < 3; ++x) v[x] = pndf_fk_dot3(Gp[(3 * x) * ld], t[0], Gp[(3 * x + 1) * ld], t[1], Gp[(3 * x + 2) * ld], t[2]);
            }
            W[(int64_t)pndf_fk_len_row(nj, j) * ld] = pndf_fk_dot3(aj[0], v[0], aj[ld], v[1], aj[2 * ld], v[2]);
        }
        pndf_fk_joint_rev(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    if (has_root) {
        pndf_fk_quat_adj(AR, ch, n, groot);
        for (int x = 0; x < 3; ++x) groot[4 + x] = as[x];
    }
    return 0.5f * acc;
}

// ---- Moving cameras of a pndf_project_options10 (DESIGN.md section 2j "Moving cameras"): the several-camera term above with a view table
// per pose.  Stated once beside the other terms, whose functions above stay as they are (their bits are pinned).  `views` is the POSE's
// own block [V][16], 16-byte aligned, in memory the lane reads itself (on the device: global memory, every lane another block; nothing
// here is wave-uniform).  Everything is pndf_fk_views_keypoint / pndf_fk_views_energy_grad, operation for operation and in their order --
// keypoints in the outer loop, views 0 .. V-1 in the inner one, the energy in that order, aW_k in view order from 0.0f -- with one rule in
// front of a view, which is the table's validation (the host cannot look at values in device memory):
//   a view takes no part for the pose when fx > 0 && fy > 0 is false for its row (zero, negative, NaN).  The test comes before the
//   confidence is read: neither conf [v][*] nor Y [v][*] is read for that view, and the rest of its row may hold anything.
// So no division by a focal length that is not positive happens.  In a row whose focal lengths are positive, finite cx, cy, R and t are
// the CALLER's responsibility, as finite targets are.  With every block equal to one table whose focal lengths are positive the result
// is that of the functions above with that table, bit for bit.
// A row is fetched as four 16-byte quads per (keypoint, view): the block is not held across the keypoint loop (V = 8 would be 128
// registers), so a pose reads its block K times per step, from the caches after the first.
struct alignas(16) PndfFkQuad {
    float v[4];
};

PNDF_HD void pndf_fk_cams_row(const float* row, float* vw) {
    const PndfFkQuad* p = reinterpret_cast<const PndfFkQuad*>(row);
    const PndfFkQuad a = p[0], b = p[1], c = p[2], d = p[3];
    for (int i = 0; i < 4; ++i) {
        vw[i] = a.v[i];
        vw[4 + i] = b.v[i];
        vw[8 + i] = c.v[i];
        vw[12 + i] = d.v[i];
    }
}

PNDF_HD float pndf_fk_cams_keypoint(int a, const float* o, bool scaled, float sg, int k, int K, const float* Y, const float* conf, float acc,
                                    float rho, int V, const float* views, bool has_root, const float* Rc, const float* s, float* as,
                                    float* AR, float* W, int64_t ld, int nj, float* h) {
#pragma clang fp contract(off)
    const float* Ga = W + (int64_t)pndf_fk_G(nj, a) * ld;
    const float* pa = W + (int64_t)pndf_fk_p(nj, a) * ld;
    float* Ma = W + (int64_t)pndf_fk_M(nj, a) * ld;
    float* aa = W + (int64_t)pndf_fk_ap(nj, a) * ld;
    float os[3], P[3], Wd[3], vu[3];
    *h = 0.f;
    for (int x = 0; x < 3; ++x) os[x] = scaled ? sg * o[x] : o[x];
    for (int x = 0; x < 3; ++x) {
        const float v = pndf_fk_dot3(Ga[(3 * x) * ld], os[0], Ga[(3 * x + 1) * ld], os[1], Ga[(3 * x + 2) * ld], os[2]);
        P[x] = pa[x * ld] + v;
        vu[x] = pndf_fk_dot3(Ga[(3 * x) * ld], o[0], Ga[(3 * x + 1) * ld], o[1], Ga[(3 * x + 2) * ld], o[2]);
    }
    if (has_root) {
        for (int x = 0; x < 3; ++x) {
            const float v = pndf_fk_dot3(Rc[3 * x], P[0], Rc[3 * x + 1], P[1], Rc[3 * x + 2], P[2]);
            Wd[x] = v + s[x];
        }
    } else {
        for (int x = 0; x < 3; ++x) Wd[x] = P[x];
    }
    float aW[3] = {0.f, 0.f, 0.f};
    bool seen = false;
    for (int v = 0; v < V; ++v) {
        float vw[PNDF_FK_VIEW_FLOATS];
        pndf_fk_cams_row(views + PNDF_FK_VIEW_FLOATS * v, vw);
        if (!(vw[0] > 0.f && vw[1] > 0.f)) continue;      // no calibration for this camera and pose: nothing of the view is read
        const float w = conf ? conf[v * K + k] : 1.0f;
        if (!(w > 0.f)) continue;
        float C[3];
        for (int x = 0; x < 3; ++x) {
            const float d = pndf_fk_dot3(vw[4 + 3 * x], Wd[0], vw[5 + 3 * x], Wd[1], vw[6 + 3 * x], Wd[2]);
            C[x] = d + vw[13 + x];
        }
        if (!(C[2] > 0.f)) continue;      // behind this camera, in its plane, or NaN: no energy, no gradient from this view
        const float* y = Y + 2 * (v * K + k);
        const float nu = C[0] / C[2], nv = C[1] / C[2];
        const float du = y[0] - vw[2], dv = y[1] - vw[3];
        const float yu = du / vw[0], yv = dv / vw[1];
        const float eu = nu - yu, ev = nv - yv;
        float pu, pv;
        const float ru = pndf_fk_robust(eu, rho, &pu);
        const float rv = pndf_fk_robust(ev, rho, &pv);
        const float rs = ru + rv;
        const float e = w * rs;
        acc = acc + e;
        const float tu = pu / C[2], tv = pv / C[2];
        const float un = pu * nu, vn = pv * nv;
        const float sn = un + vn;
        const float tz = -(sn / C[2]);
        const float a0 = w * tu, a1 = w * tv, a2 = w * tz;
        for (int x = 0; x < 3; ++x) {      // R_v^T a
            const float d = pndf_fk_dot3(vw[4 + x], a0, vw[7 + x], a1, vw[10 + x], a2);
            aW[x] = aW[x] + d;
        }
        seen = true;
    }
    if (!seen) return acc;
    if (has_root)
        for (int x = 0; x < 3; ++x) {
            as[x] = as[x] + aW[x];
            for (int y = 0; y < 3; ++y) {
                const float m = aW[x] * P[y];
                AR[3 * x + y] = AR[3 * x + y] + m;
            }
        }
    float wr[3];
    for (int x = 0; x < 3; ++x) {
        wr[x] = has_root ? pndf_fk_dot3(Rc[x], aW[0], Rc[3 + x], aW[1], Rc[6 + x], aW[2]) : aW[x];      // R_c^T aW
        aa[x * ld] = aa[x * ld] + wr[x];
        for (int y = 0; y < 3; ++y) {
            const float m = wr[x] * os[y];
            Ma[(3 * x + y) * ld] = Ma[(3 * x + y) * ld] + m;
        }
    }
    *h = pndf_fk_dot3(wr[0], vu[0], wr[1], vu[1], wr[2], vu[2]);
    return acc;
}

// The whole term of one pose under the V views of its own block: pndf_fk_views_energy_grad's arguments and results, `views` [V][16] being
// the pose's block.
PNDF_HD float pndf_fk_cams_energy_grad(const float* q, int nj, const int* parent, const float* rest, int K, const int32_t* kp_joint,
                                       const float* kp_offset, const float* Y, const float* conf, bool has_root, const float* root,
                                       float rho, int V, const float* views, const float* sigma, float* groot, float* W, int64_t ld) {
#pragma clang fp contract(off)
    const bool scaled = sigma != nullptr;
    for (int j = 0; j < nj; ++j) {
        float ts[3];
        for (int x = 0; x < 3; ++x) ts[x] = scaled ? sigma[j] * rest[3 * j + x] : rest[3 * j + x];
        pndf_fk_joint(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    float ch[4] = {0.f, 0.f, 0.f, 0.f}, Rc[9], s[3] = {0.f, 0.f, 0.f}, n = 0.f;
    float as[3] = {0.f, 0.f, 0.f}, AR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 9; ++i) Rc[i] = 0.f;
    if (has_root) {
        float c[4];
        for (int i = 0; i < 4; ++i) c[i] = root[i];
        for (int x = 0; x < 3; ++x) s[x] = root[4 + x];
        n = pndf_fk_unit(c, ch);
        pndf_fk_rot(ch, Rc);
    }
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        float h = 0.f;
        acc = pndf_fk_cams_keypoint(kp_joint[k], kp_offset + 3 * k, scaled, scaled ? sigma[nj + k] : 1.0f, k, K, Y, conf, acc, rho, V, views,
                                    has_root, Rc, s, as, AR, W, ld, nj, &h);
        if (scaled) W[(int64_t)pndf_fk_len_row(nj, nj + k) * ld] = h;      // (without scales nobody reads the rows of h: they are not written)
    }
    for (int j = nj - 1; j >= 0; --j) {
        const float* t = rest + 3 * j;
        const float* aj = W + (int64_t)pndf_fk_ap(nj, j) * ld;
        float ts[3], v[3] = {0.f, 0.f, 0.f};
        for (int x = 0; x < 3; ++x) ts[x] = scaled ? sigma[j] * t[x] : t[x];
        if (scaled) {
            if (parent[j] < 0) {
                for (int x = 0; x < 3; ++x) v[x] = t[x];
            } else {
                const float* Gp = W + (int64_t)pndf_fk_G(nj, parent[j]) * ld;
                for (int x = 0; x < 3; ++x) v[x] = pndf_fk_dot3(Gp[(3 * x) * ld], t[0], Gp[(3 * x + 1) * ld], t[1], Gp[(3 * x + 2) * ld], t[2]);
            }
            W[(int64_t)pndf_fk_len_row(nj, j) * ld] = pndf_fk_dot3(aj[0], v[0], aj[ld], v[1], aj[2 * ld], v[2]);
        }
        pndf_fk_joint_rev(q + 4 * j, parent[j], ts, W, ld, nj, j);
    }
    if (has_root) {
        pndf_fk_quat_adj(AR, ch, n, groot);
        for (int x = 0; x < 3; ++x) groot[4 + x] = as[x];
    }
    return 0.5f * acc;
}
