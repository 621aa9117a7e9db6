/* posendf_amd_skeleton_data.h -- training data for any joint tree: the exact k-NN index and the online sampler for poses of J joints.
 *
 * Companion of posendf_amd.h (same library).  posendf_amd_skeleton_train.h trains a joint tree of 1 .. 32 joints; these three
 * calls make its data: the index that labels noisy poses with their exact distance to a pose manifold [N,J,4], and the sampler
 * that draws those noisy poses from it.  pndf_knn_create, pndf_online_sample and pndf_online_sample_cpu are these with
 * num_joints = 21, with the same refusals, texts and codes.  DESIGN.md section 2u.
 *
 * Conventions: those of the pndf_knn_* block of posendf_amd.h and of posendf_amd_online.h, with [.., J, 4] in place of
 * [.., 21, 4].  num_joints outside 1 .. 32 is PNDF_ERR_BAD_ARG, decided before any pointer is looked at (the rule of
 * pndf_skel_train_batch).
 *
 * Still 21-joint: pndf_quat_topk (dist_utils.geo / euc) and the second order (completion, interpolation, motion denoising and 3D / 2D keypoint
 * fitting for J joints: pndf_skel_project with a pndf_project_options2 / 3 / 4 / 5 / 6 / 7 / 8 / 9 / 10, posendf_amd_skeleton.h).
 */
#ifndef POSENDF_AMD_SKELETON_DATA_H
#define POSENDF_AMD_SKELETON_DATA_H

#include "posendf_amd.h"
#include "posendf_amd_online.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pndf_knn_create for poses of num_joints joints.  The handle is a pndf_knn_handle: pndf_knn_search / _workspace_bytes / _size /
 * _destroy / _last_error of posendf_amd.h serve it unchanged, with q [Q,J,4].  `weights`: num_joints HOST floats (finite, > 0) or
 * NULL = 1 / num_joints each.  Distances: sum_j w_j (1 - |<q_j, p_j>|) (geo) or sum_j w_j ||q_j - p_j|| (euc), joints summed in
 * the order 0 .. J-1; the results do not depend on how a search is planned. */
int pndf_skel_knn_create(pndf_knn_handle* out, const float* poses /* device [N,J,4] */, int64_t N, int32_t num_joints,
                         int32_t metric, const float* weights /* J host floats or NULL = 1/J */, void* stream);

/* pndf_online_sample for poses of num_joints joints: q [count,J,4] <- poses first .. first + count - 1 of the pool over man_db
 * [N,J,4].  Pose i draws block 0 (source row, sigma group) and block 1 + j for joint j, as posendf_amd_online.h states them; the
 * bound on `count` is that of a grid of 2^31 - 1 blocks of 256 joint quaternions, (2^31 - 1) * 256 / num_joints. */
int pndf_skel_online_sample(const float* man_db, int64_t N, int32_t num_joints, int64_t first, int64_t count,
                            const pndf_online_opts* opt, float* q, int64_t* src /* may be NULL */, int32_t* group /* may be NULL */,
                            void* stream);

/* Host twin (HOST pointers, no stream): the same expression, the same bits. */
int pndf_skel_online_sample_cpu(const float* man_db, int64_t N, int32_t num_joints, int64_t first, int64_t count,
                                const pndf_online_opts* opt, float* q, int64_t* src, int32_t* group);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_SKELETON_DATA_H */
