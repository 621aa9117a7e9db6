// Distance, gradient and projection for any joint tree on gfx950 (include/posendf_amd_skeleton.h): the
// first-order path of model/posendf.py:62-76 / experiments/sample_poses.py:67-74 with the skeleton as a run-time value -- up to 32
// joints, every parent before its child, any number of roots.  The fused and runtime-planned persistent kernels keep the 21-joint
// table (their MFMA encoder indexes registers by a compile-time parent); this unit is assembled layer by layer from shared pieces:
//   pndf_net_plan.h   what is accepted of a skeleton and of a DFNet, and the plan (LayerNet) the handle derives from
//   pndf_gemm.h       the 128 x 128 exact-fp32 MFMA GEMM and its epilogues; on the host trunk_forward / trunk_reverse
//   pndf_bone.h       one bone MLP (bone_load / bone_fwd / bone_dual_rev without the primal chain / bone_input_adj), pose_col_norms, norm_x
//   pndf_step.h       the projection step of one joint quaternion
// Here: the two encoder kernels with the joint count and the parent table as kernel arguments, the weights' device copy, the calls.
//
// Over a chunk of SK_CHUNK poses, every activation matrix [features][columns] (the pose index contiguous) in the caller's workspace:
//   pndf_skel_enc_fwd_kernel   lanes own poses: x = normalize(q, dim=1), the bones in index order (a uniform branch on the
//                              parent selects the 4- or 10-input bone), features and sigma' of both bone layers stored
//   trunk forward              L NN GEMMs, epilogue bias + sigma, sigma' kept
//   trunk reverse              L TN GEMMs, epilogue * sigma'
//   pndf_skel_enc_rev_kernel   lanes own poses: joints nj-1 .. 0 (children before parents), rows 4..9 of a bone's input adjoint
//                              added to the parent's feature adjoint, the reverse of the normalisation, grad_out; in project mode
//                              the step of pndf_step.h in the same kernel, and with the joint mask of a pndf_project_options2 (pose
//                              completion: one word per pose) a held joint stores the bits it read instead; with the tracks of a
//                              pndf_project_options3 (pose interpolation: lane c is frame c % T of its track) its second
//                              instantiation pndf_skel_enc_rev_track_kernel: the end frames are held and a free joint of an
//                              interior frame takes the neighbour coupling of pndf_interp.h between the descent and the
//                              renormalisation, out of place; with the observation or the free end frames of a
//                              pndf_project_options4 (motion denoising) its third instantiation pndf_skel_enc_rev_denoise_kernel:
//                              pndf_denoise_quat of pndf_interp.h, with tracks (out of place) or without (in place allowed); with the
//                              3D keypoints of a pndf_project_options5 (keypoint fitting) its fourth instantiation
//                              pndf_skel_enc_rev_fit_kernel: in front of the steps of the joints the forward kinematics of the
//                              lane's pose, the keypoint residuals and the reverse of pndf_fk.h in workspace rows [24 J][ld], then
//                              pndf_fit_quat -- the denoising step with nu * dE/dQ_j in front of its finish; with the camera or the
//                              root of a pndf_project_options6 (image fitting) its fifth instantiation
//                              pndf_skel_enc_rev_image_kernel: pndf_fk.h's camera term in place of the 3D term and the root's own step;
//                              with the bone lengths of a pndf_project_options7 its sixth instantiation pndf_skel_enc_rev_len_kernel:
//                              the camera term on the tree scaled by the row of the lane's group, d E / d sigma of the frame left in
//                              S workspace rows; with the views of a pndf_project_options8 its seventh instantiation
//                              pndf_skel_enc_rev_views_kernel: the same, with the pixels of V cameras in front of the root's frame;
//                              with the root trajectory of a pndf_project_options9 its eighth instantiation
//                              pndf_skel_enc_rev_root_kernel: any of those three terms, and the root stepped out of place, coupled to
//                              the roots of the neighbour frames and drawn towards an anchor; with the moving cameras of a
//                              pndf_project_options10 its ninth instantiation pndf_skel_enc_rev_cams_kernel: the several-camera term
//                              on the lane's own block of a view table in device memory, the root stepped in place or out of place
//   pndf_skel_len_step_kernel  once per chunk and step behind that kernel (only when nu_len > 0): the sum of those rows over the frames
//                              of every group in pndf_fk.h's order and the step of the scales in place
//   pndf_skel_fill_kernel      the fill of a track from its two end frames, once per chunk in front of the steps
// 2 + 2 L launches per evaluation.  No float atomics, no communication between workgroups, every column of a GEMM summed in the
// same order wherever it sits: the same inputs give the same bits and a pose's result does not depend on its batch.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/posendf_amd_skeleton.h"
#include "pndf_experiment.h"
#include "pndf_bone.h"
#include "pndf_fk.h"
#include "pndf_host.h"
#include "pndf_interp.h"
#include "pndf_project_opts.h"
#include "pndf_step.h"

PNDF_EXPORT_EXPERIMENT_WORD(skeleton)

namespace {

// Poses per pass over the layers: a constant, so the chunk seams depend on B only (the value of the second order's SO_CHUNK,
// whose sweep found two workgroups per compute unit on every layer worth more than a chunk inside the last-level cache).
constexpr int64_t SK_CHUNK = 16384;

enum { SK_FORWARD = 0, SK_GRAD = 1, SK_PROJECT = 2 };

struct SkArgs {
    const float* wenc;        // packed encoder weights
    const float* q;           // the chunk's poses [n][4 nj]
    const float* grad_out;    // [n] or null (ones)                            (SK_GRAD)
    float* d_out;             // [n] or null
    float* out;               // dq (SK_GRAD) or the stepped poses (SK_PROJECT) [n][4 nj]
    float* X;                 // normalised poses [4 nj][ld]; without the encoder this is the trunk's input
    float* act0;              // encoder output [6 nj][ld]
    float* S1;                // sigma' of the bones' hidden layers [10 nj][ld]
    float* S2;                // sigma' of the bones' output layers [6 nj][ld]
    float* U0;                // adjoint of the trunk's input, accumulated in place [6 nj][ld] (without the encoder: g_x [4 nj][ld])
    float* Gx;                // g_x = d d / d x [4 nj][ld]
    const float* dist;        // the trunk's output row [ld]
    const uint32_t* observed; // the chunk's mask words [n], bit j = joint j is held, or null (no joint is held)   (SK_PROJECT)
    int64_t n, ld;
    int nj, encoder, mode;
    int act;                  // act / beta: the encoder's
    float beta;
    float step_size, tol;     // SK_PROJECT
    int renorm;
    int frames;               // T of a pndf_project_options3: the chunk is n / T whole tracks, lane c is frame c % T; 0 = no tracks  (SK_PROJECT)
    float lambda;             // the neighbour coupling of an interior frame
    int parent[MAXJ];
    int off[MAXJ];
};

// SkArgs with the observation of a pndf_project_options4 (SK_PROJECT), which the host side carries and pndf_skel_enc_rev_denoise_kernel
// alone takes: every other kernel takes the SkArgs part as it was, so its hidden kernel arguments -- which follow the struct -- keep
// their offsets and its code stays what it was to the byte.
struct SkDenoiseArgs : SkArgs {
    const float* anchor;      // the chunk's observation [n][4 nj], or null (no data term)
    const float* conf;        // the chunk's confidences [n][nj], or null (ones)
    float mu;                 // the weight of the data term
    uint32_t flags;           // PNDF_TRACK_FREE_ENDS: the end frames of a track are not held
};

// SkDenoiseArgs with the keypoints of a pndf_project_options5 (SK_PROJECT), which pndf_skel_enc_rev_fit_kernel alone takes, derived for the
// same reason.  The small tables are values of the argument struct: wave-uniform, read with scalar loads, validated on the host.
struct SkFitArgs : SkDenoiseArgs {
    const float* kp_target;   // the chunk's targets [n][K][3], or null (no keypoint term)
    const float* kp_conf;     // the chunk's confidences [n][K], or null (ones)
    float* kp_energy;         // [n] or null: E at the step's input iterate
    float* fk;                // the rows [24 nj][ld] of pndf_fk.h
    int K;                    // keypoints, 1 .. 64
    float nu;                 // the weight of the keypoint term
    int kpj[PNDF_FK_MAX_KEYPOINTS];            // the joint of keypoint k
    float kpo[3 * PNDF_FK_MAX_KEYPOINTS];      // its local offset
    float rest[3 * MAXJ];                      // the rest offsets of the joints
};

// SkFitArgs with the camera and the root of a pndf_project_options6 (SK_PROJECT), which pndf_skel_enc_rev_image_kernel alone takes, derived
// for the same reason.  The intrinsics and the flag are values of the argument struct: wave-uniform scalar loads.
struct SkImageArgs : SkFitArgs {
    float* root;              // the chunk's roots [n][7] (c, s), or null (identity)
    PndfFkCamera cam;         // fx, fy, cx, cy, rho, image
    float nu_rot, nu_trans;   // the weights of the root's own step; both 0: the root is not written
};

// SkImageArgs with the bone lengths of a pndf_project_options7 (SK_PROJECT), which pndf_skel_enc_rev_len_kernel alone takes, derived for the
// same reason.
struct SkLenArgs : SkImageArgs {
    const float* bone_scale;  // the rows [groups of the chunk][S] of the scales, or null (no lengths)
    int S;                    // nj + K
    int group;                // frames per group: lane c reads row c / group
};

// SkLenArgs with the views of a pndf_project_options8 (SK_PROJECT), which pndf_skel_enc_rev_views_kernel alone takes, derived for the same
// reason.  The table is a value of the argument struct: wave-uniform, read with scalar loads in a loop of uniform trip count.
struct SkViewsArgs : SkLenArgs {
    int V;                                                     // views, 1 .. PNDF_FK_MAX_VIEWS; 0: none
    float views[PNDF_FK_MAX_VIEWS * PNDF_FK_VIEW_FLOATS];      // row v: fx, fy, cx, cy, R_v [9] row-major, t_v [3]
};
static_assert(sizeof(SkViewsArgs) <= 4096, "a kernel's arguments are at most 4,096 bytes");

// SkViewsArgs with the root trajectory of a pndf_project_options9 (SK_PROJECT), which pndf_skel_enc_rev_root_kernel alone takes, derived
// for the same reason.  With it `root` is the buffer the step READS (the lane's row and its neighbours') and `root_out` the one it writes.
struct SkRootArgs : SkViewsArgs {
    float* root_out;                 // [n][7]: the other root buffer of the Jacobi step; null: no trajectory term
    const float* root_anchor;        // the chunk's anchor [n][7], or null (no data term)
    float lambda_rot, lambda_trans;  // the neighbour coupling of the root's rotation / translation
    float mu_rot, mu_trans;          // the weights of the data term towards root_anchor
};
static_assert(sizeof(SkRootArgs) <= 4096, "a kernel's arguments are at most 4,096 bytes");

// SkRootArgs with the moving cameras of a pndf_project_options10 (SK_PROJECT), which pndf_skel_enc_rev_cams_kernel alone takes, derived
// for the same reason.  The table is device memory: every lane fetches the rows of its own block with vector loads.
struct SkCamsArgs : SkRootArgs {
    const float* pose_views;         // the chunk's blocks [n][V][16], or with views_per_frame the call's [frames][V][16]; 16-byte aligned
    int views_per_frame;             // != 0: lane c reads block c % frames; 0: block c
};
static_assert(sizeof(SkCamsArgs) <= 4096, "a kernel's arguments are at most 4,096 bytes");

// What pndf_skel_len_step_kernel takes: the rows h [S][ld] the reverse left, the chunk's distance row and the scales to step in place
struct SkLenStepArgs {
    float* bone_scale;        // [G][S]
    const float* h;           // row i of frame c at h[i * ld + c]
    const float* dist;        // [ld]
    int64_t ld;
    int G, S, n;              // groups of the chunk, scales per group, frames per group
    float nu_len, kappa, len_min, len_max, tol;
    float rate[PNDF_MAX_SCALES];
};

// bone j forward on column c: the parent's features are read back from act0 (a per-thread feature array indexed by a run-time
// parent would live in scratch memory)
template <int FIN>
__device__ __forceinline__ void skel_fwd_bone(const SkArgs& e, int j, int64_t c) {
    float in[FIN];
    BoneDual b;
    bone_load<FIN>(e.X, e.ld, e.act0, e.ld, e.parent, j, c, in);
    bone_fwd<FIN>(e, e.wenc + e.off[j], in, b);
#pragma unroll
    for (int i = 0; i < HID; ++i) e.S1[(int64_t)(j * HID + i) * e.ld + c] = b.d1h[i];
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        e.act0[(int64_t)(j * FEAT + i) * e.ld + c] = b.ao[i];
        e.S2[(int64_t)(j * FEAT + i) * e.ld + c] = b.d1o[i];
    }
}

// bone j reverse on column c: U0 rows of j -> Gx rows of j, and (FIN = 10) added to the U0 rows of the parent
template <int FIN>
__device__ __forceinline__ void skel_rev_bone(const SkArgs& e, int j, int64_t c) {
    const float* w = e.wenc + e.off[j];
    float adb[FEAT];
    BoneDual b;
    BoneAdj r;
#pragma unroll
    for (int i = 0; i < HID; ++i) {
        b.d1h[i] = e.S1[(int64_t)(j * HID + i) * e.ld + c];
        b.hz[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < FEAT; ++i) {
        b.d1o[i] = e.S2[(int64_t)(j * FEAT + i) * e.ld + c];
        b.oz[i] = 0.f;
        adb[i] = e.U0[(int64_t)(j * FEAT + i) * e.ld + c];
    }
    bone_dual_rev<FIN, false>(w, b, nullptr, adb, r);
#pragma unroll
    for (int m = 0; m < FIN; ++m) {
        float s, sd;
        bone_input_adj<FIN, false>(w, r, m, s, sd);
        if (m < BONE) e.Gx[(int64_t)(j * BONE + m) * e.ld + c] = sd;
        else e.U0[(int64_t)(e.parent[j] * FEAT + (m - BONE)) * e.ld + c] += sd;
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pndf_skel_gemm_nn_kernel(GemmArgs g) { gemm_body<1, 0>(g); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_gemm_tn_kernel(GemmArgs g) { gemm_body<0, 0>(g); }

// x = normalize(q, dim=1) (over the joint axis, per quaternion component) and the encoder
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_fwd_kernel(SkArgs e) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.n) return;
    const float* q = e.q + c * (e.nj * BONE);
    float nrm[BONE];
    pose_col_norms(q, e.nj, nrm);
    for (int j = 0; j < e.nj; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) e.X[(int64_t)(j * BONE + k) * e.ld + c] = norm_x(q[j * BONE + k], nrm[k]);
    if (!e.encoder) return;
    for (int j = 0; j < e.nj; ++j) {
        if (e.parent[j] < 0) skel_fwd_bone<BONE>(e, j, c);
        else skel_fwd_bone<BONE + FEAT>(e, j, c);
    }
}

// The reverse of the encoder and of the normalisation: per component column k with s = |q_k| and x = q_k / s,
// d d / d q = (g_x - x (x . g_x)) / s; where the norm is clamped the normalisation is linear, g_x / eps.  Then grad_out, or the step.
// KIND: SK_REV_TRACKS is the instantiation of a projection with tracks (e.frames >= 2); SK_REV_PLAIN runs every other call that brings no
// observation and no free ends, with no branch on the tracks and no neighbour registers (as a branch in one kernel the tracks cost the
// call without them up to 0.2 %).  SK_REV_DENOISE is the instantiation of a pndf_project_options4 with an anchor and / or
// free end frames, with tracks (e.frames >= 2) or without (e.frames == 0): pndf_denoise_quat of pndf_interp.h in place of the step.
// SK_REV_FIT is the instantiation of a pndf_project_options5 with a keypoint term: everything SK_REV_DENOISE does, and pndf_fk.h's
// energy and gradient of the lane's pose at the step's input iterate -- all of it before the first store to `out`, which may be `q`.
// SK_REV_IMAGE is the instantiation of a pndf_project_options6 with a root or PNDF_KP_IMAGE: SK_REV_FIT with pndf_fk.h's camera term in
// place of the 3D term, and the root's own step -- a lane reads its root row before the term and writes it after the joints.
// SK_REV_LEN is the instantiation of a pndf_project_options7 with scales: SK_REV_IMAGE with pndf_fk.h's scaled term, which reads the row
// of the lane's group and leaves d E / d sigma of the lane's frame in the rows behind the tree's; the scales step in their own kernel.
// SK_REV_VIEWS is the instantiation of a pndf_project_options8 with views: SK_REV_LEN with pndf_fk.h's several-camera term (targets
// [V][K][2] and confidences [V][K] per lane); the group's row of scales may be missing (all ones).
// SK_REV_ROOT is the instantiation of a pndf_project_options9 with a positive lambda or mu of the root: the term of SK_REV_IMAGE, SK_REV_LEN
// or SK_REV_VIEWS -- a wave-uniform choice from V and bone_scale, as sk_run_chunk chooses among those kernels -- and pndf_fk.h's
// pndf_fk_root_smooth_step from `root` to `root_out` in place of the root's step; the neighbours' and the anchor's rows are loaded inside
// that step, behind the energy and its reverse.
// SK_REV_CAMS is the instantiation of a pndf_project_options10 with a view table per pose: pndf_fk.h's pndf_fk_cams_energy_grad on the
// lane's own block (block c, or c % frames: a chunk holds whole tracks), with the scales or without, and both forms of the root's step by
// a wave-uniform branch on root_out -- pndf_fk_root_step in place as SK_REV_VIEWS, pndf_fk_root_smooth_step out of place as SK_REV_ROOT.
enum { SK_REV_PLAIN = 0, SK_REV_TRACKS = 1, SK_REV_DENOISE = 2, SK_REV_FIT = 3, SK_REV_IMAGE = 4, SK_REV_LEN = 5, SK_REV_VIEWS = 6, SK_REV_ROOT = 7,
       SK_REV_CAMS = 8 };
template <int KIND, class Args>
__device__ __forceinline__ void skel_enc_rev(const Args& e) {
    constexpr bool TRACKS = KIND == SK_REV_TRACKS;
    constexpr bool LEN = KIND == SK_REV_LEN;
    constexpr bool VIEWS = KIND == SK_REV_VIEWS;
    constexpr bool ROOT = KIND == SK_REV_ROOT;
    constexpr bool CAMS = KIND == SK_REV_CAMS;
    constexpr bool IMAGE = KIND == SK_REV_IMAGE || LEN || VIEWS || ROOT || CAMS;
    constexpr bool FIT = KIND == SK_REV_FIT || IMAGE;
    constexpr bool DENOISE = KIND == SK_REV_DENOISE || FIT;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= e.n) return;
    if (e.encoder)
        for (int j = e.nj - 1; j >= 0; --j) {
            if (e.parent[j] < 0) skel_rev_bone<BONE>(e, j, c);
            else skel_rev_bone<BONE + FEAT>(e, j, c);
        }
    const int nq = e.nj * BONE;
    const float* q = e.q + c * nq;
    float* out = e.out + c * nq;
    float s[BONE], b[BONE] = {0.f, 0.f, 0.f, 0.f};
    pose_col_norms(q, e.nj, s);      // before the first store: in project mode `out` may be `q`
    for (int j = 0; j < e.nj; ++j)
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const int64_t at = (int64_t)(j * BONE + k) * e.ld + c;
            b[k] = fmaf(e.X[at], e.Gx[at], b[k]);
        }
    const float dist = e.dist[c];
    const float go = (e.mode == SK_GRAD && e.grad_out) ? e.grad_out[c] : 1.f;
    uint32_t held = (e.mode == SK_PROJECT && e.observed) ? e.observed[c] : 0u;
    float lambda = 0.f;      // > 0: an interior frame of a track, whose neighbours c - 1 and c + 1 are frames of the same track and chunk
    if (TRACKS) {            // (SK_PROJECT, e.frames >= 2)
        const int k = (int)(c % e.frames);
        if (k == 0 || k == e.frames - 1) held = ~0u;
        else lambda = e.lambda;
    }
    int nbr = 0;             // DENOISE: bit 0 = frame c - 1, bit 1 = frame c + 1 is a frame of the same track (and chunk)
    if constexpr (DENOISE) {
        if (e.frames) {
            const int k = (int)(c % e.frames);
            nbr = (k > 0 ? 1 : 0) | (k < e.frames - 1 ? 2 : 0);
            if (nbr != 3 && !(e.flags & PNDF_TRACK_FREE_ENDS)) held = ~0u;
            lambda = e.lambda;
        }
    }
    float energy = 0.f;      // FIT: E of the pose; d E / d Q_j is left in the rows pndf_fk_grad_row of e.fk
    float root[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, groot[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // IMAGE: the lane's root at the step's input and d E / d (c, s)
    if constexpr (IMAGE) {
        if (e.root)
#pragma unroll
            for (int i = 0; i < 7; ++i) root[i] = e.root[c * 7 + i];
        if constexpr (CAMS) {
            const int64_t blk = e.views_per_frame ? c % e.frames : c;
            energy = pndf_fk_cams_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.V * e.K * 2),
                                              e.kp_conf ? e.kp_conf + c * (e.V * e.K) : nullptr, e.root != nullptr, root, e.cam.rho, e.V,
                                              e.pose_views + blk * (e.V * PNDF_FK_VIEW_FLOATS),
                                              e.bone_scale ? e.bone_scale + (c / e.group) * e.S : nullptr, groot, e.fk + c, e.ld);
        } else if constexpr (ROOT) {
            if (e.V > 0)
                energy = pndf_fk_views_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.V * e.K * 2),
                                                   e.kp_conf ? e.kp_conf + c * (e.V * e.K) : nullptr, e.root != nullptr, root, e.cam.rho, e.V,
                                                   e.views, e.bone_scale ? e.bone_scale + (c / e.group) * e.S : nullptr, groot, e.fk + c, e.ld);
            else if (e.bone_scale)
                energy = pndf_fk_len_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.K * (e.cam.image ? 2 : 3)),
                                                 e.kp_conf ? e.kp_conf + c * e.K : nullptr, e.root != nullptr, root, e.cam,
                                                 e.bone_scale + (c / e.group) * e.S, groot, e.fk + c, e.ld);
            else
                energy = pndf_fk_camera_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.K * (e.cam.image ? 2 : 3)),
                                                    e.kp_conf ? e.kp_conf + c * e.K : nullptr, e.root != nullptr, root, e.cam, groot, e.fk + c, e.ld);
        } else if constexpr (VIEWS)
            energy = pndf_fk_views_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.V * e.K * 2),
                                               e.kp_conf ? e.kp_conf + c * (e.V * e.K) : nullptr, e.root != nullptr, root, e.cam.rho, e.V,
                                               e.views, e.bone_scale ? e.bone_scale + (c / e.group) * e.S : nullptr, groot, e.fk + c, e.ld);
        else if constexpr (LEN)
            energy = pndf_fk_len_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.K * (e.cam.image ? 2 : 3)),
                                             e.kp_conf ? e.kp_conf + c * e.K : nullptr, e.root != nullptr, root, e.cam,
                                             e.bone_scale + (c / e.group) * e.S, groot, e.fk + c, e.ld);
        else
        energy = pndf_fk_camera_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.K * (e.cam.image ? 2 : 3)),
                                            e.kp_conf ? e.kp_conf + c * e.K : nullptr, e.root != nullptr, root, e.cam, groot, e.fk + c, e.ld);
    } else if constexpr (FIT)
        energy = pndf_fk_energy_grad(q, e.nj, e.parent, e.rest, e.K, e.kpj, e.kpo, e.kp_target + c * (e.K * 3),
                                     e.kp_conf ? e.kp_conf + c * e.K : nullptr, e.fk + c, e.ld);
    for (int j = 0; j < e.nj; ++j) {
        float g[BONE];
#pragma unroll
        for (int k = 0; k < BONE; ++k) {
            const int64_t at = (int64_t)(j * BONE + k) * e.ld + c;
            const float x = e.X[at], gx = e.Gx[at];
            g[k] = s[k] > NORM_EPS ? (gx - x * b[k]) / s[k] : gx / NORM_EPS;
        }
        if (e.mode == SK_PROJECT) {
            float Q[BONE], u[BONE];
#pragma unroll
            for (int k = 0; k < BONE; ++k) Q[k] = q[j * BONE + k];
            bool rest;
            if (TRACKS) {
                float nm[BONE] = {0.f, 0.f, 0.f, 0.f}, np[BONE] = {0.f, 0.f, 0.f, 0.f};
                if (lambda > 0.f)
#pragma unroll
                    for (int k = 0; k < BONE; ++k) {
                        nm[k] = q[j * BONE + k - nq];
                        np[k] = q[j * BONE + k + nq];
                    }
                rest = pndf_interp_band_quat(Q, g, dist, nm, np, lambda, e.step_size, e.tol, e.renorm, u);      // lambda 0: pndf_step_quat
            } else if constexpr (DENOISE) {
                float nm[BONE] = {0.f, 0.f, 0.f, 0.f}, np[BONE] = {0.f, 0.f, 0.f, 0.f}, A[BONE] = {0.f, 0.f, 0.f, 0.f};
                if (lambda > 0.f && (nbr & 1))
#pragma unroll
                    for (int k = 0; k < BONE; ++k) nm[k] = q[j * BONE + k - nq];
                if (lambda > 0.f && (nbr & 2))
#pragma unroll
                    for (int k = 0; k < BONE; ++k) np[k] = q[j * BONE + k + nq];
                float w = 0.f;      // the weight of the data term: mu * conf, rounded once; the anchor is read only when it is positive
                if (e.anchor) w = e.conf ? e.mu * e.conf[c * e.nj + j] : e.mu;
                if (w > 0.f)
#pragma unroll
                    for (int k = 0; k < BONE; ++k) A[k] = e.anchor[c * nq + j * BONE + k];
                if constexpr (FIT) {
                    float gk[BONE];
#pragma unroll
                    for (int k = 0; k < BONE; ++k) gk[k] = e.fk[(int64_t)(pndf_fk_grad_row(e.nj, j) + k) * e.ld + c];
                    rest = pndf_fit_quat(Q, g, dist, nm, np, nbr, lambda, A, w, gk, e.nu, e.step_size, e.tol, e.renorm, u);
                } else {
                    rest = pndf_denoise_quat(Q, g, dist, nm, np, nbr, lambda, A, w, e.step_size, e.tol, e.renorm, u);
                }
            } else {
                rest = pndf_step_quat(Q, g, dist, e.step_size, e.tol, e.renorm, u);
            }
#pragma unroll
            for (int k = 0; k < BONE; ++k) {      // a held joint keeps the bits it came with: an integer select, no arithmetic on them
                const uint32_t kept = __float_as_uint(Q[k]), stepped = __float_as_uint(rest ? Q[k] : u[k]);
                out[j * BONE + k] = __uint_as_float(((held >> j) & 1u) ? kept : stepped);
            }
        } else {
#pragma unroll
            for (int k = 0; k < BONE; ++k) out[j * BONE + k] = g[k] * go;
        }
    }
    if (e.d_out) e.d_out[c] = dist;
    if constexpr (FIT)
        if (e.kp_energy) e.kp_energy[c] = energy;
    if constexpr (CAMS) {
        if (e.root_out) {      // (wave-uniform; set only with a root, a positive root weight and a positive lambda or mu)
            const int k = e.frames ? (int)(c % e.frames) : 0;
            const int rn = e.frames ? ((k > 0 ? 1 : 0) | (k < e.frames - 1 ? 2 : 0)) : 0;
            const float* row = e.root + c * 7;
            float stepped[7];
            pndf_fk_root_smooth_step(root, groot, e.nu_rot, e.nu_trans, dist, e.tol, row - 7, row + 7, rn, e.lambda_rot, e.lambda_trans,
                                     e.root_anchor + c * 7, e.mu_rot, e.mu_trans, stepped);
#pragma unroll
            for (int i = 0; i < 7; ++i) e.root_out[c * 7 + i] = stepped[i];
        } else if (e.root && (e.nu_rot > 0.f || e.nu_trans > 0.f)) {
            float stepped[7];
            pndf_fk_root_step(root, groot, e.nu_rot, e.nu_trans, dist, e.tol, stepped);
#pragma unroll
            for (int i = 0; i < 7; ++i) e.root[c * 7 + i] = stepped[i];
        }
    } else if constexpr (ROOT) {      // (the host launches this kernel only with a root, a positive root weight and a positive lambda or mu)
        const int k = e.frames ? (int)(c % e.frames) : 0;
        const int rn = e.frames ? ((k > 0 ? 1 : 0) | (k < e.frames - 1 ? 2 : 0)) : 0;
        const float* row = e.root + c * 7;
        float stepped[7];
        pndf_fk_root_smooth_step(root, groot, e.nu_rot, e.nu_trans, dist, e.tol, row - 7, row + 7, rn, e.lambda_rot, e.lambda_trans,
                                 e.root_anchor + c * 7, e.mu_rot, e.mu_trans, stepped);
#pragma unroll
        for (int i = 0; i < 7; ++i) e.root_out[c * 7 + i] = stepped[i];
    } else if constexpr (IMAGE)
        if (e.root && (e.nu_rot > 0.f || e.nu_trans > 0.f)) {
            float stepped[7];
            pndf_fk_root_step(root, groot, e.nu_rot, e.nu_trans, dist, e.tol, stepped);
#pragma unroll
            for (int i = 0; i < 7; ++i) e.root[c * 7 + i] = stepped[i];
        }
}

extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_kernel(SkArgs e) { skel_enc_rev<SK_REV_PLAIN>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_track_kernel(SkArgs e) { skel_enc_rev<SK_REV_TRACKS>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_denoise_kernel(SkDenoiseArgs e) { skel_enc_rev<SK_REV_DENOISE>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_fit_kernel(SkFitArgs e) { skel_enc_rev<SK_REV_FIT>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_image_kernel(SkImageArgs e) { skel_enc_rev<SK_REV_IMAGE>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_len_kernel(SkLenArgs e) { skel_enc_rev<SK_REV_LEN>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_views_kernel(SkViewsArgs e) { skel_enc_rev<SK_REV_VIEWS>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_root_kernel(SkRootArgs e) { skel_enc_rev<SK_REV_ROOT>(e); }
extern "C" __global__ void __launch_bounds__(256) pndf_skel_enc_rev_cams_kernel(SkCamsArgs e) { skel_enc_rev<SK_REV_CAMS>(e); }

// The step of the scales of a chunk (pndf_fk.h: pndf_fk_len_group_sum's order, pndf_fk_len_step).  Frames per group n <= 64: lanes own
// (group, scale) pairs and sum their frames in order.  n > 64: one workgroup per (group, scale), lane b sums block b of 64 frames, lane 0
// adds the partials in block order (a chunk has at most 16,384 frames, so at most 256 blocks); whether every frame rests goes the same way.
extern "C" __global__ void __launch_bounds__(256) pndf_skel_len_step_kernel(SkLenStepArgs a) {
    __shared__ float part[256];
    __shared__ int moving[256];
    if (a.n <= PNDF_FK_LEN_BLOCK) {
        const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= (int64_t)a.G * a.S) return;
        const int g = (int)(t / a.S), i = (int)(t - (int64_t)g * a.S);
        const float w = a.nu_len * a.rate[i];
        if (!(w > 0.f)) return;
        const int64_t f0 = (int64_t)g * a.n;
        bool rests = a.tol > 0.f;
        if (rests)
            for (int f = 0; f < a.n; ++f) rests = rests && (a.dist[f0 + f] < a.tol);
        if (rests) return;
        const float H = pndf_fk_len_group_sum(a.h + (int64_t)i * a.ld + f0, 1, a.n);
        float* sg = a.bone_scale + (int64_t)g * a.S + i;
        *sg = pndf_fk_len_step(*sg, H, a.n, w, a.kappa, a.len_min, a.len_max, false);
        return;
    }
    const int g = (int)(blockIdx.x / a.S), i = (int)(blockIdx.x - (unsigned)g * a.S);      // uniform over the workgroup
    const float w = a.nu_len * a.rate[i];
    if (!(w > 0.f)) return;
    const int nb = (a.n + PNDF_FK_LEN_BLOCK - 1) / PNDF_FK_LEN_BLOCK;
    const int b = threadIdx.x;
    const int64_t f0 = (int64_t)g * a.n;
    float p = 0.f;
    int mv = 0;
    if (b < nb) {
        const int64_t b0 = (int64_t)b * PNDF_FK_LEN_BLOCK, b1 = b0 + PNDF_FK_LEN_BLOCK < a.n ? b0 + PNDF_FK_LEN_BLOCK : a.n;
        p = pndf_fk_len_block_sum(a.h + (int64_t)i * a.ld + f0, 1, b0, b1);
        for (int64_t f = b0; f < b1; ++f) mv |= (a.dist[f0 + f] < a.tol) ? 0 : 1;
    }
    part[b] = p;
    moving[b] = mv;
    __syncthreads();
    if (b != 0) return;
    int any = 0;
    float H = 0.f;
    for (int k = 0; k < nb; ++k) {
        any |= moving[k];
        H = pndf_fk_len_add(H, part[k]);
    }
    float* sg = a.bone_scale + (int64_t)g * a.S + i;
    *sg = pndf_fk_len_step(*sg, H, a.n, w, a.kappa, a.len_min, a.len_max, a.tol > 0.f && !any);
}

// The fill of a chunk of whole tracks (pndf_project_options3, PNDF_TRACK_SLERP / _NLERP): one lane per joint quaternion.  Of every track
// only frames 0 (a) and T-1 (b) of `src` are read; frame 0 of `dst` takes the bits of a, frame T-1 b aligned to a, the frames between
// them pndf_interp_fill_quat -- the statements of pndf_interp_fill_kernel for a run-time joint count.  dst does not overlap src.
extern "C" __global__ void __launch_bounds__(256) pndf_skel_fill_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t quats,
                                                                        int nj, int T, int mode) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quats) return;
    const int64_t f = i / nj;
    const int j = (int)(i - f * nj);
    const int k = (int)(f % T);
    const float* a = src + ((f - k) * nj + j) * BONE;
    const float* b = a + (int64_t)(T - 1) * nj * BONE;
    float av[BONE], bv[BONE], u[BONE];
#pragma unroll
    for (int c = 0; c < BONE; ++c) av[c] = a[c];
    if (k > 0) {
#pragma unroll
        for (int c = 0; c < BONE; ++c) bv[c] = b[c];
        float bp[BONE];
        pndf_quat_align(av, bv, bp);
        if (k < T - 1) pndf_interp_fill_quat(av, bp, (float)k / (float)(T - 1), mode, u);
        else
#pragma unroll
            for (int c = 0; c < BONE; ++c) u[c] = bp[c];
    } else {
#pragma unroll
        for (int c = 0; c < BONE; ++c) u[c] = av[c];
    }
#pragma unroll
    for (int c = 0; c < BONE; ++c) dst[i * BONE + c] = u[c];
}

// the forward alone ends here: the trunk's output row -> d
extern "C" __global__ void __launch_bounds__(256) pndf_skel_copy_kernel(const float* src, float* dst, int64_t n) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) dst[c] = src[c];
}

// ------------------------------------------------------------------------------------------------------------ host side
struct pndf_skel_plan : LayerNet {
    bool have_weights = false;
    int64_t w_off[MAX_LIN] = {}, b_off[MAX_LIN] = {}, blob_floats = 0;      // the device copy: the packed encoder, then W and b of every layer
    float* d_blob = nullptr;
    std::string err;
};

namespace {

const GemmKernels SK_GEMM = {pndf_skel_gemm_nn_kernel, pndf_skel_gemm_tn_kernel, nullptr};

// workspace layout in floats (every region 256-byte aligned); nc: the columns of a chunk
struct SkLayout {
    int64_t nc;
    int64_t X, act0, S1, S2, U0, Gx, dist, D1[MAX_LIN], P[2];
    int64_t Q2;      // the second pose buffer [nc][4 J] of the out-of-place steps of a pndf_project_options3
    int64_t FK;      // the rows [24 J][nc] of the forward kinematics and its adjoints of a pndf_project_options5 (pndf_fk.h), and behind
                     // them the rows [96][nc] of d E / d sigma of a pndf_project_options7
    int64_t ROOT;    // the second root buffer [nc][7] of the Jacobi steps of a pndf_project_options9
    int64_t total;
};

SkLayout sk_layout(const pndf_skel_plan* h, int64_t B) {
    SkLayout l{};
    l.nc = B < SK_CHUNK ? B : SK_CHUNK;
    Carver c;
    const int64_t nq = (int64_t)h->nj * BONE, nf = (int64_t)h->nj * FEAT;
    l.X = c.take(nq * l.nc);
    if (h->encoder) {
        l.act0 = c.take(nf * l.nc);
        l.S1 = c.take((int64_t)h->nj * HID * l.nc);
        l.S2 = c.take(nf * l.nc);
        l.U0 = c.take(nf * l.nc);
        l.Gx = c.take(nq * l.nc);
    } else {      // the trunk reads x and its reverse ends in g_x
        l.act0 = l.X;
        l.S1 = l.S2 = -1;
        l.U0 = l.Gx = c.take(nq * l.nc);
    }
    l.dist = c.take(l.nc);
    for (int t = 0; t < h->L; ++t) l.D1[t] = c.take((int64_t)h->dims[t + 1] * l.nc);
    l.P[0] = c.take((int64_t)h->maxw * l.nc);
    l.P[1] = c.take((int64_t)h->maxw * l.nc);
    l.Q2 = c.take(nq * l.nc);
    l.FK = c.take(((int64_t)PNDF_FK_ROWS * h->nj + PNDF_MAX_SCALES) * l.nc);      // the tree's rows, then pndf_fk_len_row's
    l.ROOT = c.take(7 * l.nc);
    l.total = c.o;
    return l;
}

// One evaluation of a chunk of n poses at `q`: the 2 + 2 L launches (the forward alone: 1 + L and the copy of the output row)
void sk_run_chunk(const pndf_skel_plan* h, const SkLayout& l, float* ws, const SkCamsArgs& e, hipStream_t st) {
    const int n = (int)e.n;
    TrunkWeights w{};
    TrunkBuffers b{};
    for (int t = 0; t < h->L; ++t) { w.W[t] = h->d_blob + h->w_off[t]; w.b[t] = h->d_blob + h->b_off[t]; b.D1[t] = ws + l.D1[t]; }
    b.in = ws + l.act0; b.P[0] = ws + l.P[0]; b.P[1] = ws + l.P[1]; b.out = ws + l.dist; b.din = ws + l.U0;
    b.ld = l.nc; b.n = n;
    const SkArgs& plain = e;      // what every kernel but the denoising and the fitting one takes
    const SkDenoiseArgs& denoise = e;
    const SkFitArgs& fit = e;
    const SkImageArgs& image = e;
    const SkLenArgs& lengths = e;
    const SkViewsArgs& views = e;
    const SkRootArgs& rooted = e;
    hipLaunchKernelGGL(pndf_skel_enc_fwd_kernel, dim3(blocks(n)), dim3(256), 0, st, plain);
    trunk_forward(SK_GEMM, *h, w, b, st);
    if (e.mode == SK_FORWARD) {
        hipLaunchKernelGGL(pndf_skel_copy_kernel, dim3(blocks(n)), dim3(256), 0, st, ws + l.dist, e.d_out, (int64_t)n);
        return;
    }
    trunk_reverse(SK_GEMM, *h, w, b, st);      // grad_out scales the result in the encoder's reverse
    if (e.mode == SK_PROJECT && e.kp_target && e.pose_views) hipLaunchKernelGGL(pndf_skel_enc_rev_cams_kernel, dim3(blocks(n)), dim3(256), 0, st, e);
    else if (e.mode == SK_PROJECT && e.kp_target && e.root_out) hipLaunchKernelGGL(pndf_skel_enc_rev_root_kernel, dim3(blocks(n)), dim3(256), 0, st, rooted);
    else if (e.mode == SK_PROJECT && e.kp_target && e.V > 0) hipLaunchKernelGGL(pndf_skel_enc_rev_views_kernel, dim3(blocks(n)), dim3(256), 0, st, views);
    else if (e.mode == SK_PROJECT && e.kp_target && e.bone_scale) hipLaunchKernelGGL(pndf_skel_enc_rev_len_kernel, dim3(blocks(n)), dim3(256), 0, st, lengths);
    else if (e.mode == SK_PROJECT && e.kp_target && (e.root || e.cam.image)) hipLaunchKernelGGL(pndf_skel_enc_rev_image_kernel, dim3(blocks(n)), dim3(256), 0, st, image);
    else if (e.mode == SK_PROJECT && e.kp_target) hipLaunchKernelGGL(pndf_skel_enc_rev_fit_kernel, dim3(blocks(n)), dim3(256), 0, st, fit);
    else if (e.mode == SK_PROJECT && (e.anchor || e.flags)) hipLaunchKernelGGL(pndf_skel_enc_rev_denoise_kernel, dim3(blocks(n)), dim3(256), 0, st, denoise);
    else if (e.mode == SK_PROJECT && e.frames) hipLaunchKernelGGL(pndf_skel_enc_rev_track_kernel, dim3(blocks(n)), dim3(256), 0, st, plain);
    else hipLaunchKernelGGL(pndf_skel_enc_rev_kernel, dim3(blocks(n)), dim3(256), 0, st, plain);
}

SkCamsArgs sk_args(const pndf_skel_plan* h, const SkLayout& l, float* ws, int mode) {
    SkCamsArgs e;
    memset(&e, 0, sizeof(e));
    e.wenc = h->d_blob;
    e.X = ws + l.X; e.act0 = ws + l.act0; e.U0 = ws + l.U0; e.Gx = ws + l.Gx; e.dist = ws + l.dist; e.fk = ws + l.FK;
    if (h->encoder) { e.S1 = ws + l.S1; e.S2 = ws + l.S2; }
    e.ld = l.nc;
    e.nj = h->nj; e.encoder = h->encoder ? 1 : 0; e.mode = mode;
    e.act = h->enc_act; e.beta = h->enc_beta;
    e.step_size = 1.f;
    for (int j = 0; j < h->nj; ++j) { e.parent[j] = h->parent[j]; e.off[j] = h->enc_off[j]; }
    return e;
}

// what the three compute calls check alike, and the layout for B > 0 poses (PNDF_OK with B == 0: nothing to do)
int sk_check(pndf_skel_plan* h, int64_t B, const void* workspace, int64_t workspace_bytes, SkLayout& l) {
    if (B < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative batch");
    if (!h->have_weights) return pndf_fail(h, PNDF_ERR_NO_WEIGHTS, "pndf_skel_load_weights has not been called");
    if (B == 0) return PNDF_OK;
    l = sk_layout(h, B);
    return pndf_check_workspace(h, workspace, workspace_bytes, l.total * (int64_t)sizeof(float), "bytes", "pndf_skel_workspace_bytes");
}

}  // namespace

extern "C" const char* pndf_skel_last_error(pndf_skel_handle h) { return pndf_last_error_of(h); }

extern "C" int pndf_skel_create(pndf_skel_handle* out, const pndf_config* cfg, int device) {
    auto refuse = [](int code, const std::string& why) { return pndf_fail<pndf_skel_plan>(nullptr, code, why); };
    if (!out || !cfg) return refuse(PNDF_ERR_BAD_ARG, "out / cfg is null");
    *out = nullptr;
    if (const char* why = pndf_skeleton_refusal(cfg)) return refuse(PNDF_ERR_UNSUPPORTED, why);
    if (const char* why = pndf_dfnet_refusal(cfg)) return refuse(PNDF_ERR_UNSUPPORTED, why);
    if (cfg->precision != PNDF_PREC_FP32) return refuse(PNDF_ERR_UNSUPPORTED, "precision: this unit runs exact fp32 (PNDF_PREC_FP32) only");
    if (cfg->act == PNDF_ACT_SOFTPLUS && !(cfg->beta > 0.f)) return refuse(PNDF_ERR_UNSUPPORTED, "beta: Softplus beta must be positive");
    if (pndf_enc_act(*cfg) == PNDF_ACT_SOFTPLUS && !(pndf_enc_beta(*cfg) > 0.f))
        return refuse(PNDF_ERR_UNSUPPORTED, "enc_beta: Softplus beta of the encoder must be positive");
    const PndfDeviceCheck dev = pndf_check_gfx950(device, "the skeleton unit");
    if (dev.code != PNDF_OK) return refuse(dev.code, dev.text);
    pndf_skel_plan* h = new pndf_skel_plan();
    layer_net_init(*h, cfg, device);
    Carver blob;
    blob.take(h->enc_params);
    for (int t = 0; t < h->L; ++t) {
        h->w_off[t] = blob.take((int64_t)h->dims[t + 1] * h->dims[t]);
        h->b_off[t] = blob.take(h->dims[t + 1]);
    }
    h->blob_floats = blob.o;
    DeviceGuard guard(device);
    const hipError_t e = guard.ok ? hipMalloc((void**)&h->d_blob, (size_t)h->blob_floats * sizeof(float)) : hipErrorInvalidDevice;
    if (e != hipSuccess) {
        delete h;
        (void)hipGetLastError();
        return refuse(PNDF_ERR_HIP, std::string("hipMalloc of the weights: ") + hipGetErrorString(e));
    }
    *out = h;
    return PNDF_OK;
}

extern "C" int pndf_skel_destroy(pndf_skel_handle h) {
    if (!h) return PNDF_OK;
    if (h->d_blob) {
        DeviceGuard guard(h->device);
        (void)hipFree(h->d_blob);
    }
    delete h;
    return PNDF_OK;
}

extern "C" int pndf_skel_load_weights(pndf_skel_handle h, const float* const* tensors, const int64_t* numel, int n_tensors) {
    if (!h) return PNDF_ERR_BAD_ARG;
    if (const PndfTableFault f = pndf_table_fault(*h, tensors, numel, n_tensors)) {      // a null pointer is an argument's fault here
        const bool null = f.kind == PndfTableFault::NULL_TABLE || f.kind == PndfTableFault::NULL_TENSOR;
        return pndf_fail(h, null ? PNDF_ERR_BAD_ARG : PNDF_ERR_BAD_SHAPE, f.text());
    }
    std::vector<float> blob((size_t)h->blob_floats, 0.f);
    int i = 0;
    int64_t o = 0;
    for (; i < (h->encoder ? 4 * h->nj : 0); ++i) {      // the packed encoder: the tensors one after the other
        memcpy(blob.data() + o, tensors[i], sizeof(float) * (size_t)numel[i]);
        o += numel[i];
    }
    for (int t = 0; t < h->L; ++t, i += 2) {
        memcpy(blob.data() + h->w_off[t], tensors[i], sizeof(float) * (size_t)numel[i]);
        memcpy(blob.data() + h->b_off[t], tensors[i + 1], sizeof(float) * (size_t)numel[i + 1]);
    }
    h->have_weights = false;      // from here on a failure leaves no half-loaded plan behind
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    HIP_TRY(h, hipDeviceSynchronize());      // launches that still read the previous weights
    HIP_TRY(h, hipMemcpy(h->d_blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    h->have_weights = true;
    return PNDF_OK;
}

extern "C" int64_t pndf_skel_workspace_bytes(pndf_skel_handle h, int64_t B) {
    if (!h || B < 0) return PNDF_ERR_BAD_ARG;
    return B == 0 ? 0 : sk_layout(h, B).total * (int64_t)sizeof(float);
}

extern "C" int pndf_skel_forward(pndf_skel_handle h, const float* q, float* d, int64_t B, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    SkLayout l;
    if (B > 0 && (!q || !d)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / distance pointer");
    if (((uintptr_t)q | (uintptr_t)d) & 3) return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose or distance buffer");
    if (const int rc = sk_check(h, B, workspace, workspace_bytes, l); rc != PNDF_OK || B == 0) return rc;
    PndfRange range("pndf_skel_forward");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    float* ws = (float*)workspace;
    SkCamsArgs e = sk_args(h, l, ws, SK_FORWARD);
    for (int64_t c0 = 0; c0 < B; c0 += l.nc) {
        e.n = B - c0 < l.nc ? B - c0 : l.nc;
        e.q = q + c0 * h->nj * BONE;
        e.d_out = d + c0;
        sk_run_chunk(h, l, ws, e, (hipStream_t)stream);
    }
    return pndf_check_launch(h, "pndf_skel_forward");
}

extern "C" int pndf_skel_forward_grad(pndf_skel_handle h, const float* q, const float* grad_out, float* d, float* dq, int64_t B,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    SkLayout l;
    if (B > 0 && (!q || !dq)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose / gradient pointer");
    if (((uintptr_t)q | (uintptr_t)grad_out | (uintptr_t)d | (uintptr_t)dq) & 3)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose, grad_out, distance or gradient buffer");
    if (B > 0 && overlaps(q, dq, B * h->nj * BONE)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "dq must not overlap q");
    if (const int rc = sk_check(h, B, workspace, workspace_bytes, l); rc != PNDF_OK || B == 0) return rc;
    PndfRange range("pndf_skel_forward_grad");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    float* ws = (float*)workspace;
    SkCamsArgs e = sk_args(h, l, ws, SK_GRAD);
    for (int64_t c0 = 0; c0 < B; c0 += l.nc) {
        e.n = B - c0 < l.nc ? B - c0 : l.nc;
        e.q = q + c0 * h->nj * BONE;
        e.grad_out = grad_out ? grad_out + c0 : nullptr;
        e.d_out = d ? d + c0 : nullptr;
        e.out = dq + c0 * h->nj * BONE;
        sk_run_chunk(h, l, ws, e, (hipStream_t)stream);
    }
    return pndf_check_launch(h, "pndf_skel_forward_grad");
}

extern "C" int pndf_skel_project(pndf_skel_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                                 const pndf_project_options* opt, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!h) return PNDF_ERR_BAD_ARG;
    pndf_project_options o;
    const uint32_t* observed;      // a pndf_project_options2 brings the joint mask: one word per pose, device memory
    PndfTracks tracks;             // a pndf_project_options3 the tracks besides: B / frames of them
    PndfData data;                 // a pndf_project_options4 the observation besides (motion denoising): device memory, as the poses
    PndfKeypoints kp;              // a pndf_project_options5 the 3D keypoints besides (keypoint fitting): the arrays per pose in device memory, the small tables in host memory
    PndfCameraTerm cam;            // a pndf_project_options6 the camera and the root besides (image fitting): the roots per pose in device memory
    PndfLengths len;               // a pndf_project_options7 the bone lengths besides: the scales per group in device memory, the rates in host memory
    PndfViews vw;                  // a pndf_project_options8 the views besides: the table in host memory, targets [B,V,K,2] and confidences [B,V,K] in device memory
    PndfRootSmooth rs;             // a pndf_project_options9 the root's trajectory besides: the anchor [B,7] in device memory
    PndfPoseViews pv;              // a pndf_project_options10 the moving cameras besides: a table [B,V,16] or [frames,V,16] in device memory
    if (const char* why = pndf_check_project_options10(opt, B, h->nj, o, observed, tracks, data, kp, cam, len, vw, rs, pv)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (steps < 0) return pndf_fail(h, PNDF_ERR_BAD_ARG, "negative step count");
    SkLayout l;
    if (B > 0 && (!q_in || !q_out)) return pndf_fail(h, PNDF_ERR_BAD_ARG, "null pose pointer");
    if (((uintptr_t)q_in | (uintptr_t)q_out | (uintptr_t)d_last) & 3) return pndf_fail(h, PNDF_ERR_BAD_ARG, "misaligned pose or distance buffer");
    if (B > 0 && q_in != q_out && overlaps(q_in, q_out, B * h->nj * BONE))
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "q_out may be q_in itself, but must not overlap it otherwise");
    if (B > 0 && tracks.frames && q_in == q_out)
        return pndf_fail(h, PNDF_ERR_BAD_ARG, "q_out must not overlap q_in when pndf_project_options3.frames > 0: a step reads the neighbour "
                                              "frames of its input");
    if (const char* why = pndf_check_observation_apart(data, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_keypoints_apart(kp, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_root_apart(cam, data, kp, q_in, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_lengths_apart(len, cam, data, kp, q_in, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_root_anchor_apart(rs, cam, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const char* why = pndf_check_pose_views_apart(pv, cam, len, q_out, B, h->nj)) return pndf_fail(h, PNDF_ERR_BAD_ARG, why);
    if (const int rc = sk_check(h, B, workspace, workspace_bytes, l); rc != PNDF_OK || B == 0) return rc;
    PndfRange range("pndf_skel_project");
    DeviceGuard guard(h->device);
    if (!guard.ok) return pndf_fail(h, PNDF_ERR_HIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nq = (int64_t)h->nj * BONE;
    const bool filled = tracks.fill != PNDF_TRACK_GIVEN;
    if (steps == 0 && !filled) {
        if (q_in != q_out) HIP_TRY(h, hipMemcpyAsync(q_out, q_in, sizeof(float) * (size_t)(B * nq), hipMemcpyDeviceToDevice, st));
        if (d_last) HIP_TRY(h, hipMemsetAsync(d_last, 0, sizeof(float) * (size_t)B, st));
        if (kp.energy) HIP_TRY(h, hipMemsetAsync(kp.energy, 0, sizeof(float) * (size_t)B, st));
        return PNDF_OK;
    }
    float* ws = (float*)workspace;
    SkCamsArgs e = sk_args(h, l, ws, SK_PROJECT);
    e.step_size = o.step_size; e.tol = o.tol; e.renorm = (int)o.renorm;
    e.frames = tracks.frames; e.lambda = tracks.lambda;
    e.mu = data.mu; e.flags = data.free_ends ? (uint32_t)PNDF_TRACK_FREE_ENDS : 0u;
    if (kp.any()) {
        e.K = kp.K; e.nu = kp.nu;
        pndf_fill_keypoint_tables(e, kp, h->nj);
        e.cam.fx = cam.fx; e.cam.fy = cam.fy; e.cam.cx = cam.cx; e.cam.cy = cam.cy; e.cam.rho = cam.rho; e.cam.image = cam.image ? 1 : 0;
        e.nu_rot = cam.nu_rot; e.nu_trans = cam.nu_trans;
    }
    if (vw.any()) {
        e.V = vw.V;
        for (int i = 0; i < PNDF_FK_MAX_VIEWS * PNDF_FK_VIEW_FLOATS; ++i) e.views[i] = vw.table[i];
    }
    if (pv.any()) {
        e.V = pv.V;
        e.views_per_frame = pv.frames ? 1 : 0;
    }
    if (rs.any()) { e.lambda_rot = rs.lambda_rot; e.lambda_trans = rs.lambda_trans; e.mu_rot = rs.mu_rot; e.mu_trans = rs.mu_trans; }
    SkLenStepArgs ls;
    memset(&ls, 0, sizeof(ls));
    if (len.any()) {
        e.S = len.S; e.group = len.group;
        ls.h = ws + l.FK + (int64_t)pndf_fk_len_row(h->nj, 0) * l.nc; ls.dist = ws + l.dist; ls.ld = l.nc;
        ls.S = len.S; ls.n = len.group;
        ls.nu_len = len.nu_len; ls.kappa = len.kappa; ls.len_min = len.len_min; ls.len_max = len.len_max; ls.tol = o.tol;
        for (int i = 0; i < PNDF_MAX_SCALES; ++i) ls.rate[i] = len.rate[i];
    }
    // with tracks a chunk holds whole tracks, so no track straddles a seam and lane c of a chunk is frame c % T
    const int64_t nc = tracks.frames ? (l.nc / tracks.frames) * tracks.frames : l.nc;
    if (steps == 0 && d_last) HIP_TRY(h, hipMemsetAsync(d_last, 0, sizeof(float) * (size_t)B, st));
    if ((steps == 0 || !kp.any()) && kp.energy) HIP_TRY(h, hipMemsetAsync(kp.energy, 0, sizeof(float) * (size_t)B, st));
    for (int64_t c0 = 0; c0 < B; c0 += nc) {
        e.n = B - c0 < nc ? B - c0 : nc;
        e.observed = observed ? observed + c0 : nullptr;
        e.anchor = data.anchor ? data.anchor + c0 * nq : nullptr;
        e.conf = data.conf ? data.conf + c0 * h->nj : nullptr;
        e.kp_target = kp.target ? kp.target + c0 * kp.views * kp.K * kp.dims : nullptr;
        e.root = cam.root ? cam.root + c0 * 7 : nullptr;
        e.bone_scale = len.any() ? len.scale + (c0 / len.group) * len.S : nullptr;      // a chunk is whole groups: with tracks it is whole tracks
        e.kp_conf = kp.conf ? kp.conf + c0 * kp.views * kp.K : nullptr;
        // Without tracks the iterate is in q_out from the second step on: a lane reads its pose before it writes it.  With tracks a
        // step is out of place: the steps alternate between the chunk of q_out and the second pose buffer, the last one writes
        // q_out; step 0 reads q_in, or the buffer the fill wrote.
        float* buf[2] = {q_out + c0 * nq, tracks.frames ? ws + l.Q2 : q_out + c0 * nq};
        const float* cur = q_in + c0 * nq;
        // With the trajectory of a pndf_project_options9 the root's step is out of place too: step s reads rbuf[s & 1] and writes the other
        // buffer, step 0 reads the caller's rows; after an odd step count the result is copied back into them.
        float* rbuf[2] = {cam.root ? cam.root + c0 * 7 : nullptr, ws + l.ROOT};
        e.root_anchor = rs.anchor ? rs.anchor + c0 * 7 : nullptr;
        // A table per pose goes with the chunk; a table per frame does not: a chunk holds whole tracks, so c0 is a multiple of frames.
        if (pv.any()) e.pose_views = pv.frames ? pv.table : pv.table + c0 * ((int64_t)pv.V * PNDF_FK_VIEW_FLOATS);
        if (filled) {
            float* dst = buf[steps & 1];      // what step 0 does not write; q_out itself when there is no step
            hipLaunchKernelGGL(pndf_skel_fill_kernel, dim3(blocks(e.n * h->nj)), dim3(256), 0, st, cur, dst, e.n * (int64_t)h->nj, h->nj,
                               tracks.frames, tracks.fill == PNDF_TRACK_SLERP ? PNDF_INTERP_SLERP : PNDF_INTERP_NLERP);
            cur = dst;
        }
        for (int s = 0; s < steps; ++s) {
            e.q = cur;
            e.out = buf[(steps - 1 - s) & 1];
            e.d_out = (d_last && s == steps - 1) ? d_last + c0 : nullptr;
            e.kp_energy = (kp.any() && kp.energy && s == steps - 1) ? kp.energy + c0 : nullptr;
            if (rs.any()) {
                e.root = rbuf[s & 1];
                e.root_out = rbuf[(s + 1) & 1];
            }
            sk_run_chunk(h, l, ws, e, st);
            if (len.moves()) {      // behind the reverse on the same stream: the frames of this step have read the scales
                ls.bone_scale = len.scale + (c0 / len.group) * len.S;
                ls.G = (int)(e.n / len.group);
                const int64_t lanes = (int64_t)ls.G * ls.S;
                const unsigned grid = ls.n <= PNDF_FK_LEN_BLOCK ? (unsigned)blocks(lanes) : (unsigned)lanes;
                hipLaunchKernelGGL(pndf_skel_len_step_kernel, dim3(grid), dim3(256), 0, st, ls);
            }
            cur = e.out;
        }
        if (rs.any() && (steps & 1))
            hipLaunchKernelGGL(pndf_skel_copy_kernel, dim3(blocks(e.n * 7)), dim3(256), 0, st, rbuf[1], rbuf[0], e.n * (int64_t)7);
    }
    return pndf_check_launch(h, "pndf_skel_project");
}
