/* posendf_amd_skeleton.h -- distance, gradient and projection for any joint tree.
 *
 * Companion of posendf_amd.h (same library).  The model has nothing SMPL-specific in it: a chain of bone MLPs along a parent
 * table in front of an MLP (model/network/net_modules.py:140-170, :46-72).  pndf_create runs the 21-joint table of
 * get_parent_mapping('smpl') on persistent kernels; this unit runs ANY table -- a hand, a body with a jaw, an animal rig -- layer
 * by layer: two encoder kernels around exact-fp32 MFMA GEMMs, 2 + 2 L launches per evaluation for L linear layers.  DESIGN.md
 * section 2j.
 *
 * The networks: pndf_config as pndf_create reads it, with
 *   num_joints J  1 .. 32;   parent[j] in -1 .. j-1, -1 = a root, any number of roots;
 *   dims[0] = 6 J (structure encoder) or 4 J (model.StrEnc.use = False);  1 .. 7 hidden layers of width 1 .. 1024;  dims[last] = 1;
 *   act / enc_act relu, lrelu or softplus (enc_act -1, enc_beta <= 0: the trunk's);  precision PNDF_PREC_FP32 only.
 * Anything else is PNDF_ERR_UNSUPPORTED with a text that names the field, decided before a device is looked for.
 *
 * Arithmetic: the reference's, for a pose [J,4]: x = F.normalize(pose, dim=1) (over the JOINT axis, per quaternion component), the
 * bones in index order on cat(x_j, feature of the parent), the trunk on the concatenated features; the gradient is the analytic
 * reverse.  Exact fp32 MFMA, fp32 accumulate; no float atomics, poses are processed in chunks whose seams depend on B alone: the
 * same inputs give the same bits, and a pose's result does not depend on the other poses of the batch.
 *
 * Conventions: those of posendf_amd.h -- contiguous fp32, poses [B, J, 4], distances [B]; DEVICE pointers, 4-byte aligned, the
 * workspace 16-byte aligned; work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and the call
 * returns without synchronising, allocating or freeing anything (pndf_skel_create and pndf_skel_load_weights allocate /
 * synchronise); every entry point runs on the device of its handle and restores the caller's current device; 0 on success, a
 * negative pndf_status otherwise, its text in pndf_skel_last_error (of the calling thread's slot when there is no handle).
 * B == 0 succeeds without a launch.  PNDF_ERR_BAD_ARG with nothing launched or written for a null handle, a negative B or step
 * count, a null or misaligned pointer that is not optional, a workspace that is too small; PNDF_ERR_NO_WEIGHTS before
 * pndf_skel_load_weights.
 *
 * The host twins pndf_cpu_create / pndf_cpu_load_weights / pndf_forward_cpu / pndf_forward_grad_cpu / pndf_project_cpu /
 * pndf_project_ex_cpu (posendf_amd.h) accept the same skeletons.
 *
 * Pose completion -- some joints observed and held, the others pulled onto the manifold -- is pndf_skel_project (the host twin:
 * pndf_project_ex_cpu) with a pndf_project_options2 (posendf_amd.h) in place of the options: one mask word per pose, the select
 * inside the step of the gradient's last kernel, no launch more than an unmasked projection.
 *
 * Pose interpolation -- tracks of T frames between two key poses, relaxed onto the manifold with their end frames held and a coupling
 * between neighbouring frames -- is the same two entry points with a pndf_project_options3 (posendf_amd.h) in place of the options:
 * the B poses are B / T tracks, one small kernel fills a chunk of tracks from their end frames, and the coupling sits in the step of the
 * gradient's last kernel (its second instantiation), so a step costs no launch more than a projection step.
 *
 * Motion denoising -- a noisy clip pulled onto the manifold by the descent (the pose prior), the coupling between neighbouring frames
 * (the temporal term) and a data term towards the observation, the end frames free -- is the same two entry points with a
 * pndf_project_options4 (posendf_amd.h): anchor [B,J,4] and conf [B,J] in device memory beside the poses, mu and PNDF_TRACK_FREE_ENDS; the
 * terms sit in the step of the gradient's last kernel (its third instantiation), so a denoising step costs no launch more either.
 *
 * Keypoint fitting -- inverse kinematics under the learned prior: 3D detections of K keypoints attached to the joints, the joint tree
 * with its rest offsets as the body model -- is the same two entry points with a pndf_project_options5 (posendf_amd.h): kp_target [B,K,3],
 * kp_conf [B,K] and kp_energy [B] in device memory, the small tables rest [J,3], kp_joint [K] and kp_offset [K,3] in host memory (validated
 * without a synchronisation, handed to the kernel as arguments).  The forward kinematics, its reverse and the term nu * dE/dQ sit in the
 * step of the gradient's last kernel (its fourth instantiation), so a fitting step costs no launch more; the 72-byte struct's mask, tracks
 * and observation come along unchanged.
 *
 * Image fitting -- the same inverse kinematics on what a tracker of another joint tree delivers: 2D detections, and a placement of the tree
 * in the camera that nobody knows in advance -- is the same two entry points with a pndf_project_options6 (posendf_amd.h): root [B,7] in
 * device memory (a quaternion and a translation per pose, C_k = R(c) P_k + s, read and -- with nu_rot or nu_trans positive -- written by
 * every step), the pinhole intrinsics, rho and PNDF_KP_IMAGE (kp_target is [B,K,2] pixels; the residual in normalised image coordinates,
 * a keypoint not in front of the camera skipped).  The camera, both residual kinds, the adjoint into the tree, the root's adjoints and
 * the root's step sit in the step of the gradient's last kernel (its fifth instantiation), so an image step costs no launch more and the
 * workspace is what it was; the 128-byte struct's keypoints, mask, tracks and observation come along unchanged.
 *
 * Bone lengths -- the segment lengths of the subject as unknowns of the same fit, one set per track -- are the same two entry points with a
 * pndf_project_options7 (posendf_amd.h): bone_scale [G,S] in device memory (S = J + K scales of the rest offsets and of the keypoints'
 * local offsets; one row per track of base3.frames frames, or per pose), read and -- with nu_len positive -- written by every step.  The
 * scaled tree and the per-frame gradient of the scales sit in the gradient's last kernel (its sixth instantiation,
 * pndf_skel_enc_rev_len_kernel), which leaves them in S workspace rows; pndf_skel_len_step_kernel then sums them over the frames of every
 * group in a fixed order and steps the scales: one launch more per step and chunk than an image step, and only when nu_len > 0.
 *
 * Several cameras -- pixels of the same frame in V calibrated views -- are the same two entry points with a pndf_project_options8
 * (posendf_amd.h): views [V,16] in HOST memory (intrinsics, world -> camera rotation and translation per view), kp_target [B,V,K,2] and
 * kp_conf [B,V,K] in device memory; the root places the tree in the world frame.  The view loop sits in the gradient's last kernel (its
 * seventh instantiation, pndf_skel_enc_rev_views_kernel), which takes the view table by value; no launch more than a length-fitting
 * step, and the workspace is what it was.
 *
 * The root's trajectory -- the root of every frame of a track coupled to its neighbour frames' roots and drawn towards an observed
 * trajectory -- is the same two entry points with a pndf_project_options9 (posendf_amd.h): root_anchor [B,7] in device memory, lambda_rot,
 * lambda_trans, mu_rot, mu_trans.  The root's step is then Jacobi and out of place: it alternates between the caller's root and [chunk][7]
 * floats of the workspace, which pndf_skel_workspace_bytes includes for every caller, and after an odd step count one small copy per chunk
 * brings the result back into root.  The gradient's last kernel is then its eighth instantiation, pndf_skel_enc_rev_root_kernel, launched
 * only when a lambda or mu is positive; no step gains a launch.
 *
 * Moving cameras -- a view table per pose, or per frame of a track, in place of the one table of a pndf_project_options8 -- are the same
 * two entry points with a pndf_project_options10 (posendf_amd.h): pose_views [B,V,16] or [frames,V,16] in DEVICE memory, 16-byte aligned,
 * read by every step.  The gradient's last kernel is then its ninth instantiation, pndf_skel_enc_rev_cams_kernel, which steps the root in
 * place or, with a root trajectory, out of place; a row whose fx or fy is not positive switches its view off for that pose.  No step
 * gains a launch, and the workspace is what it was.
 *
 * Still 21-joint: the second order (posendf_amd_second_order.h) only -- pndf_so_create refuses another joint count and
 * pndf_second_order_cpu a handle of another tree, and that is pinned.  2D keypoints with a camera run for any joint tree through
 * pndf_skel_project (above); pndf_keypoint_terms_grad and pndf_lbs_* are the SMPL body model's (vertices, shape, lens of ImageFit).
 * pndf_complete, pndf_interpolate and their host twins keep the SMPL table.
 */
#ifndef POSENDF_AMD_SKELETON_H
#define POSENDF_AMD_SKELETON_H

#include "posendf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pndf_skel_plan* pndf_skel_handle;

/* A plan for the network of `cfg` on `device` (a gfx950 device: PNDF_ERR_NO_DEVICE otherwise). */
int pndf_skel_create(pndf_skel_handle* out, const pndf_config* cfg, int device);
int pndf_skel_destroy(pndf_skel_handle h);

/* load_state_dict.  `tensors` are HOST pointers in state-dict order: with the encoder, for j in 0 .. J-1 enc.net.j.net.0.weight
 * [10, 4 | 10], .bias [10], enc.net.j.net.2.weight [6, 10], .bias [6] (4 J tensors; a root's first layer is 4 wide); then weight
 * [out, in] and bias [out] of every dfnet.lin.  `numel[i]` is checked against the architecture (PNDF_ERR_BAD_SHAPE).  The call
 * uploads a copy and synchronises. */
int pndf_skel_load_weights(pndf_skel_handle h, const float* const* tensors, const int64_t* numel, int n_tensors);

/* Bytes of the workspace of the three compute calls for B poses: a function of the plan and B only -- not of the options of a call --,
 * bounded (the batch is processed in chunks of at most 16,384 poses); 0 for B == 0; PNDF_ERR_BAD_ARG for a null handle or a negative B.
 * It includes, for every caller, one pose buffer [chunk][4 J] for the out-of-place steps of a projection with tracks (at most
 * 16,384 x 128 x 4 B = 8 MB) and the rows [24 J][chunk] of the forward kinematics and its adjoints of a pndf_project_options5 (at most
 * 16,384 x 768 x 4 B = 48 MB), followed by the 96 rows [96][chunk] of the per-frame gradient of the scales of a pndf_project_options7 (at
 * most 16,384 x 96 x 4 B = 6 MB). */
int64_t pndf_skel_workspace_bytes(pndf_skel_handle h, int64_t B);

/* forward(pose, train=False)['dist_pred']: q [B,J,4] -> d [B]. */
int pndf_skel_forward(pndf_skel_handle h, const float* q, float* d, int64_t B, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* forward + torch.autograd.grad(d, q, grad_out): dq[b] = grad_out[b] * d d_b / d q_b; grad_out == NULL means ones; d may be
 * NULL and is then not written.  dq must not overlap q. */
int pndf_skel_forward_grad(pndf_skel_handle h, const float* q, const float* grad_out, float* d, float* dq, int64_t B,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* `steps` projection steps with the options of pndf_project_ex (opt == NULL: the plain step q <- q - d * grad d); the step runs
 * inside the gradient's last kernel.  q_out may be q_in itself (no other overlap).  d_last (may be NULL) is dist_pred of the last
 * iteration, evaluated before its update; with steps == 0 q_out is a copy of q_in and d_last is zero.  `opt` may point to a
 * pndf_project_options2 (posendf_amd.h; observed: DEVICE memory, one word per pose, read by the kernels of this call): the joints
 * of its mask are held, bit for bit, and the call is otherwise the same -- with no mask or all words zero the same bits.  Or to a
 * pndf_project_options3: with frames = T >= 2 the poses are B / T tracks of T consecutive frames (B % T == 0, T <= 16,384), filled
 * from their end frames or given, the end frames held, the interior frames coupled to their neighbours with weight lambda; the batch is
 * then processed in chunks of whole tracks, every step is out of place and q_out must not overlap q_in.  Or to a
 * pndf_project_options4: besides, `anchor` [B,J,4] and `conf` [B,J] (DEVICE memory, read by the kernels of this call; neither may overlap
 * q_out, both may be q_in) add the data term of weight mu * conf to every free joint, and PNDF_TRACK_FREE_ENDS frees the end frames of
 * every track; without tracks such a call may still run in place.  Or to a pndf_project_options5: besides, kp_target [B,K,3], kp_conf [B,K]
 * and kp_energy [B] (DEVICE memory; none may overlap q_out) and the HOST tables rest, kp_joint and kp_offset (read during the call) add the
 * keypoint term of weight nu to every free joint; kp_energy is E of the last iteration, evaluated before its update, as d_last is.  Or to
 * a pndf_project_options6 (root [B,7]: DEVICE memory) or a pndf_project_options7 (bone_scale [G,S]: DEVICE memory, len_rate [S]: HOST
 * memory, read during the call) or a pndf_project_options8 (views [V,16]: HOST memory, read during the call; kp_target [B,V,K,2] and
 * kp_conf [B,V,K]: DEVICE memory) or a pndf_project_options9 (root_anchor [B,7]: DEVICE memory) or a pndf_project_options10 (pose_views
 * [B,V,16] or [frames,V,16]: DEVICE memory): ten sizes in all, every other one is refused. */
int pndf_skel_project(pndf_skel_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                      const pndf_project_options* opt, void* workspace, int64_t workspace_bytes, void* stream);

const char* pndf_skel_last_error(pndf_skel_handle h);   /* h may be NULL: last error of a failed pndf_skel_create */

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_SKELETON_H */
