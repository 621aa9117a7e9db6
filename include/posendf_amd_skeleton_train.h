/* posendf_amd_skeleton_train.h -- the training objective, its weight gradients and the batch sampler for any joint tree.
 *
 * Companion of posendf_amd.h (same library).  pndf_train_create plans the 21-joint table of get_parent_mapping('smpl');
 * nobody publishes weights for a hand, a body with a jaw or an animal rig, so a user of posendf_amd_skeleton.h trains first.  The
 * reference cannot (model/posendf.py:64,80 reshape to (-1, 21, 4)): this is its train=True branch with J in place of 21, on the
 * kernels of csrc/pndf_train.hip, which take the joint count, the parent table and every bone's offset at run time.  DESIGN.md
 * section 2t.
 *
 * Conventions, arithmetic and determinism: those of the pndf_train_* block of posendf_amd.h (exact fp32 MFMA, fixed K splits, no
 * float atomics, the same inputs give the same bits).  On the SMPL table pndf_skel_train_create builds the plan pndf_train_create
 * builds, and the compute calls return the same bits.
 *
 * Still 21-joint: the second order (posendf_amd_second_order.h).  Completion, interpolation, motion denoising, 3D keypoint fitting and
 * fitting to 2D keypoints with a free root for J joints are pndf_skel_project with a pndf_project_options2 / 3 / 4 / 5 / 6 / 7 / 8 / 9 / 10
 * (posendf_amd_skeleton.h).  The k-NN index and the online
 * sampler for J joints, which make this trainer's data: posendf_amd_skeleton_data.h.
 */
#ifndef POSENDF_AMD_SKELETON_TRAIN_H
#define POSENDF_AMD_SKELETON_TRAIN_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A training plan for ANY joint tree: what pndf_skel_create accepts with the structure encoder (num_joints 1 .. 32, parent[j] in
 * -1 .. j-1, dims[0] = 6 * num_joints, 1 .. 7 hidden layers up to 1024 wide, any activation pair).  The handle is a
 * pndf_train_handle: pndf_train_workspace_floats / _forward / _backward / _destroy / _last_error of posendf_amd.h serve it, with
 * q [B,J,4], q_man [Bm,J,4], 4 J encoder tensors in front of the trunk's in `weights` / `grads`, eikonal = mean over b and the J
 * joints.  Anything else is PNDF_ERR_UNSUPPORTED (an encoder-less config, dims[0] = 4 * num_joints, with the text of
 * pndf_train_create), decided before a device is looked for; the text of a failed create is in pndf_train_last_error(NULL). */
int pndf_skel_train_create(pndf_train_handle* out, const pndf_config* cfg, int device);

/* pndf_train_batch for poses of num_joints joints (pose_db [N,J,4], man_db [M,J,4], q / q_man [items*num_pts,J,4]);
 * num_joints outside 1 .. 32: PNDF_ERR_BAD_ARG.  pndf_train_batch is this with 21. */
int pndf_skel_train_batch(const float* pose_db, const float* dist_db, const float* man_db, const int64_t* file_off,
                          const int64_t* man_off, const int32_t* item_file, const int32_t* item_man_file, const uint32_t* words,
                          int32_t F, int32_t Fm, int32_t k, int32_t items, int32_t num_pts, int32_t flip, int32_t num_joints,
                          float* q, float* dist_gt, float* q_man, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_SKELETON_TRAIN_H */
