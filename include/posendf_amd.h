/* posendf_amd.h -- C ABI of the MI355X-native Pose-NDF distance / projection engine.
 *
 * The reference (garvita-tiwari/PoseNDF) has no FFI layer: its seam is the Python class
 * PoseNDF(nn.Module) (reference model/posendf.py:30-101) as called from
 * experiments/sample_poses.py:71-74 and experiments/motion_denoise.py:82.  These entry points are what a
 * binding for that seam needs (INTEGRATION.md shows the ctypes stub); each cites the reference lines it
 * replaces.  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - all tensors are contiguous fp32; poses are [B, 21, 4] = [B, 84] row-major (model/posendf.py:64),
 *     distances are [B] (the reference's [B, 1]); device pointers must be 16-byte aligned;
 *   - every compute call enqueues work on the caller's HIP stream (`stream` is a hipStream_t passed as void*;
 *     NULL = the default stream) and returns without synchronising, allocating or freeing anything (safe under
 *     stream capture); pndf_create and pndf_load_weights allocate / synchronise;
 *   - every entry point runs on the device of its handle (stateless helpers: of their buffers) and restores the
 *     caller's current device before it returns;
 *   - the caller owns every buffer; the engine owns its packed copy of the weights and, for softplus, one derivative
 *     scratch (843 KB per compute unit, allocated by pndf_create).  Softplus launches of one handle share that scratch:
 *     a launch on another stream than the previous one first waits (on the device) for the previous one's completion.
 *     Launches recorded during stream capture are not tracked that way: replays of a captured softplus launch must be
 *     ordered by the caller against other launches of the same handle (use one handle per concurrently replayed graph);
 *   - return value: 0 on success, a negative pndf_status otherwise; pndf_last_error() has the text;
 *   - a handle belongs to one device and must not be used from two threads at once.
 */
#ifndef POSENDF_AMD_H
#define POSENDF_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pndf_engine* pndf_handle;

typedef enum {
    PNDF_OK = 0,
    PNDF_ERR_BAD_ARG = -1,        /* null / misaligned pointer, negative size */
    PNDF_ERR_BAD_SHAPE = -2,      /* weight tensor count or shape does not match the architecture */
    PNDF_ERR_HIP = -3,            /* a HIP runtime call failed (text in pndf_last_error) */
    PNDF_ERR_UNSUPPORTED = -4,    /* activation / architecture the kernels do not implement */
    PNDF_ERR_NO_WEIGHTS = -5,     /* compute call before pndf_load_weights */
    PNDF_ERR_NO_DEVICE = -6,      /* no gfx950 device visible */
    PNDF_ERR_HOST = -7            /* host twins only: a worker thread or an allocation failed (text in pndf_cpu_last_error) */
} pndf_status;

typedef enum { PNDF_ACT_RELU = 0, PNDF_ACT_LRELU = 1, PNDF_ACT_SOFTPLUS = 2 } pndf_act;

/* Mirrors the keys PoseNDF.__init__ actually reads (reference model/posendf.py:35-55,
 * model/network/net_modules.py:14-41,116-128; configs/amass.yaml:22-43). */
typedef struct {
    int32_t act;            /* pndf_act: model.DFNet.act (and model.StrEnc.act unless enc_act says otherwise) */
    float beta;             /* Softplus beta (amass.yaml:32,43); ignored for relu / lrelu */
    int32_t num_joints;     /* 21 */
    int32_t n_dims;         /* 8: in_dim, dims..., 1 */
    int32_t dims[16];       /* 126,256,512,1024,512,256,64,1 (amass.yaml:26,30); dims[0] = 84 selects the
                               encoder-less model (model.StrEnc.use = False, model/posendf.py:40-42,73-74).  `dims` is the
                               reference's free list (net_modules.py:14-28): six hidden widths within amass.yaml's run on the
                               fused kernels (narrower ones zero padded; softplus with a hidden width <= 8 under split precision: as the
                               next case); any other n_dims 3 .. 9 with hidden widths 1 .. 1024
                               runs on the runtime-planned kernels (exact fp32, or split-precision
                               fp16 MFMAs for PNDF_PREC_F16X3 / _F16); beyond that PNDF_ERR_UNSUPPORTED */
    int32_t parent[32];     /* net_utils.py:46 */
    int32_t precision;      /* pndf_precision: arithmetic of the trunk (engine knob, no reference counterpart) */
    int32_t enc_act;        /* model.StrEnc.act when it differs from model.DFNet.act (net_modules.py:128 reads its own key);
                               -1 (pndf_default_config) = the same as `act`.  A mixed pair runs on the runtime-planned kernels */
    float enc_beta;         /* model.StrEnc.beta for a softplus encoder; <= 0 = the same as `beta` */
} pndf_config;

/* PNDF_PREC_FP32 : exact fp32 MFMA (v_mfma_f32_16x16x4_f32), bit-comparable to an fmaf chain.
 * PNDF_PREC_F16X3: every fp32 operand split into fp16 hi + lo, three v_mfma_f32_16x16x32_f16 per product block,
 *                  fp32 accumulate: ~2^-22 relative product error (fp32-class), ~3x the throughput.
 *                  All scaling is by exact powers of two: weights per layer (any magnitude packs; pndf_load_weights
 *                  refuses -- PNDF_ERR_UNSUPPORTED -- only a trunk layer without a finite non-zero weight), activations
 *                  and gradients PER POSE from bounds measured on the chip or derived from the layers' norms, so that
 *                  no operand can overflow fp16 for any finite weights and poses and none is flushed for poses whose
 *                  gradients are tiny (small-gain networks).
 *                  When every trunk weight is exactly representable in fp16 at its layer scale (e.g. a checkpoint saved
 *                  in half precision), all lo halves of the weights are zero and the lo*hi term vanishes identically:
 *                  pndf_load_weights then selects the two-term kernels (2 MFMAs per block, no lo-tile reads) -- the same
 *                  results bit for bit, ~1.2x the throughput.  The environment variable PNDF_THREE_TERMS=1 keeps the
 *                  three-term kernels (A/B runs); pndf_kernel_name() tells which one a handle launches.
 * PNDF_PREC_F16  : plain fp16 operands (round to nearest), ONE MFMA per product block, fp32 accumulate.  A measured
 *                  comparison point (BASELINE.json configs[2] "fp32 vs bf16"): ~1e-3 relative, NOT within the 1e-4
 *                  parity bar of the two modes above; never selected implicitly; relu / lrelu only.
 * PNDF_PREC_BF16 : plain bfloat16 operands (round to nearest even), ONE v_mfma_f32_16x16x32_bf16 per product block, fp32
 *                  accumulate: the literal second half of BASELINE.json configs[2] "fp32 vs bf16".  Same schedule and rate
 *                  as PNDF_PREC_F16 with three fewer significant bits (~1e-2 relative): a measured comparison point only;
 *                  never selected implicitly; relu / lrelu only; amass.yaml-shaped networks only. */
typedef enum { PNDF_PREC_FP32 = 0, PNDF_PREC_F16X3 = 1, PNDF_PREC_F16 = 2, PNDF_PREC_BF16 = 3 } pndf_precision;

/* Fills cfg with the configs/amass.yaml architecture and the SMPL parent table. */
void pndf_default_config(pndf_config* cfg, int32_t act, float beta);

/* PoseNDF(opt) + .to(device) (model/posendf.py:32-55; sample_poses.py:88,93). */
int pndf_create(pndf_handle* out, const pndf_config* cfg, int device);
int pndf_destroy(pndf_handle h);

/* load_state_dict (sample_poses.py:90-91).  `tensors` are HOST pointers in state-dict order:
 * for i in 0..20: enc.net.i.net.0.weight [10,in], .bias [10], enc.net.i.net.2.weight [6,10], .bias [6];
 * then for l in 0..6: dfnet.lin{l}.weight [out,in] row-major, .bias [out]   (98 tensors; the 14 dfnet tensors
 * only when dims[0] == 84).
 * `numel[i]` is checked against the architecture.  Weights are re-packed into MFMA tile order and
 * uploaded; the call synchronises. */
int pndf_load_weights(pndf_handle h, const float* const* tensors, const int64_t* numel, int n_tensors);

/* PoseNDF.forward(pose, train=False)['dist_pred'] (model/posendf.py:62-76,100-101). */
int pndf_forward(pndf_handle h, const float* q, float* d, int64_t B, void* stream);

/* forward + torch.autograd.grad(d, q, grad_outputs) (model/posendf.py:18-27; sample_poses.py:71-73;
 * motion_denoise.py:82-83,97-98).  dq[b] = grad_out[b] * d d_b / d q_b; grad_out == NULL means ones. */
int pndf_forward_grad(pndf_handle h, const float* q, const float* grad_out, float* d, float* dq,
                      int64_t B, void* stream);

/* The projection loop of experiments/sample_poses.py:67-74: `steps` times q <- q - d(q) * grad d(q), in one
 * persistent launch.  q_out may alias q_in.  d_last[b] (may be NULL) is dist_pred of the last iteration. */
int pndf_project(pndf_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                 void* stream);

/* Options of one projection step (pndf_project_ex; DESIGN.md section 1 "The projection step").  Per pose and step, every operation
 * rounded to fp32 on its own (no fused multiply-add), d = dist_pred(q) and g = d d / d q as in pndf_project:
 *   tol > 0 and d < tol : the pose is left unchanged, bit for bit (a NaN d compares false and is not frozen).  The rule is
 *                         stateless: an unchanged pose has the same d at the next step and stays frozen.  It stops the motion,
 *                         not the work: the launch still runs every step for every pose;
 *   otherwise             u = q - step_size * (d * g);   step_size = 1 is the step of pndf_project, bit for bit;
 *   PNDF_RENORM_UNIT    : per joint, u <- u / clamp_min(sqrt(((u0 u0 + u1 u1) + u2 u2) + u3 u3), 1e-12) (the clamp of F.normalize: a
 *                         zero quaternion stays zero);
 *   PNDF_RENORM_UNIT_FLIP: the same, then u <- -u where u0 < 0 (the convention of the training data, model/load_data.py:12-16).
 * The input of the first step is used as given: only the results of updates are normalised. */
enum { PNDF_RENORM_NONE = 0, PNDF_RENORM_UNIT = 1, PNDF_RENORM_UNIT_FLIP = 2 };
typedef struct {
    uint32_t struct_size;   /* sizeof(pndf_project_options): a struct of another size (a zero-initialised one) is refused */
    float step_size;        /* alpha, finite and > 0; default 1 */
    int32_t renorm;         /* PNDF_RENORM_*; default PNDF_RENORM_NONE */
    float tol;              /* >= 0; default 0 = no pose is ever frozen */
} pndf_project_options;
void pndf_default_project_options(pndf_project_options* opt);

/* The options with a joint mask: pose completion inside the projection step, for any joint tree (J = 1 .. 32 joints).  A joint whose
 * bit is set in its pose's word is HELD: it keeps the bits it came with in q_out, whatever they are (a NaN, a zero quaternion),
 * and still enters the distance and the gradient of the other joints; the other joints take the step above.  Bits J .. 31 of a
 * word are ignored; `tol` rests a whole pose as before, d_last keeps its meaning, q_out == q_in stays allowed.  With observed ==
 * NULL or all words zero the call is the one with the 16-byte struct, bit for bit.  Fill it with
 *   pndf_project_options2 o;  pndf_default_project_options(&o.base);  o.base.struct_size = sizeof o;  o.observed = mask;  o.reserved = 0;
 * and pass (const pndf_project_options*)&o.  Exactly two entry points take it: pndf_skel_project of posendf_amd_skeleton.h (any
 * handle) and pndf_project_ex_cpu below (any handle: the 21-joint table and the encoder-less model too).  Every other function
 * with a pndf_project_options parameter keeps refusing a struct_size other than sizeof(pndf_project_options).  PNDF_ERR_BAD_ARG with
 * a text that names the field, before anything is launched or written: a struct_size that is neither of the two sizes, reserved
 * != 0, a misaligned observed, and what is refused in `base`. */
typedef struct {
    pndf_project_options base;   /* base.struct_size = sizeof(pndf_project_options2); the rest as pndf_project_options */
    const uint32_t* observed;    /* one word per pose, bit j set = joint j is held; NULL = no joint is held.
                                    DEVICE memory for the device entry point, HOST memory for the host twin; 4-byte aligned */
    uint64_t reserved;           /* must be 0 */
} pndf_project_options2;         /* 32 bytes */

/* The options with tracks: pose interpolation inside the projection step, for any joint tree.  With frames = T >= 2 the B poses are
 * B / T tracks of T consecutive frames (include/posendf_amd_interpolation.h states the semantics for the 21 joints; here J joints):
 *   fill PNDF_TRACK_GIVEN : q_in is the track; frames 0 and T-1 of every track are copied bit for bit;
 *   fill PNDF_TRACK_SLERP / _NLERP: only frames 0 (a) and T-1 (b) of every track are read from q_in; frame T-1 of the result is b with
 *                           every joint quaternion negated where <a, b> < 0, the frames between them the interpolation of each joint;
 *   step                  : the end frames and the joints of `observed` keep their bits (the integer select of the mask); every other
 *                           joint quaternion descends as above, then takes lambda (0.5 (N- + N+) - Q) with N-, N+ the joint in the two
 *                           neighbour frames of the step's INPUT iterate, each negated where its dot product with Q is negative, then
 *                           renorm / flip / tol as above.  A step is out of place (a Jacobi update): q_out must not overlap q_in.
 * steps == 0 returns the fill (or the copy) and zeroes d_last; d_last keeps its meaning.  With frames == 0 (then lambda must be 0 and
 * fill PNDF_TRACK_GIVEN) the call is the one with the 32-byte struct, bit for bit; with lambda == 0 and PNDF_TRACK_GIVEN it is that call
 * with all ones in the words of the end frames, bit for bit.  Fill it with
 *   pndf_project_options3 o;  pndf_default_project_options(&o.base2.base);  o.base2.base.struct_size = sizeof o;  o.base2.observed = mask;
 *   o.base2.reserved = 0;  o.frames = T;  o.lambda = 0.5f;  o.fill = PNDF_TRACK_SLERP;  o.reserved2 = 0;
 * and pass (const pndf_project_options*)&o.  Exactly two entry points take it, the two that take a pndf_project_options2:
 * pndf_skel_project of posendf_amd_skeleton.h and pndf_project_ex_cpu below (any handle: the 21-joint table and the encoder-less
 * model too); every other function with a pndf_project_options parameter keeps refusing a struct_size other than sizeof(pndf_project_options).
 * PNDF_ERR_BAD_ARG with a text that names the field, before anything is launched or written: a struct_size that is none of the
 * three sizes, reserved2 != 0, frames of 1, negative or above 16,384, B % frames != 0, a lambda outside [0, 1] or NaN, an unknown
 * fill, frames == 0 with a non-zero lambda or another fill than PNDF_TRACK_GIVEN, frames > 0 with q_out overlapping q_in, and what is
 * refused in `base2`. */
enum { PNDF_TRACK_GIVEN = 0, PNDF_TRACK_SLERP = 1, PNDF_TRACK_NLERP = 2 };
typedef struct {
    pndf_project_options2 base2; /* base2.base.struct_size = sizeof(pndf_project_options3); mask and reserved as before */
    int32_t frames;              /* T: 0 = no tracks; else 2 .. 16384 and B % T == 0 */
    float   lambda;              /* neighbour coupling, in [0, 1] */
    int32_t fill;                /* PNDF_TRACK_* */
    int32_t reserved2;           /* must be 0 */
} pndf_project_options3;         /* 48 bytes */

/* The options with an observation: motion denoising inside the projection step, for any joint tree -- a pose prior (the descent), a
 * temporal term (the tracks' coupling) and a data term that ties the result to the noisy observation, all in quaternion space.  Per
 * free joint quaternion Q of a pose, every operation rounded on its own, between the descent and renorm / flip / tol:
 *   coupling : an interior frame of a track as in pndf_project_options3.  With PNDF_TRACK_FREE_ENDS the two end frames of a track are
 *              no longer held: they descend like every frame, and with lambda > 0 take lambda (0.5 (N - Q)) with N the joint in their
 *              one neighbour frame, negated where <Q, N> < 0 (the gradient of sum_k |q_k - q_k+1|^2, which for an interior frame is
 *              lambda (mean - Q)); the joints of `observed` stay held in every frame.  Without the flag the end frames are held;
 *   data term: w = mu * conf[pose][j] (w = mu when conf is NULL); when w > 0, u <- u + w (A - Q) with A the joint of `anchor`, negated
 *              where <Q, A> < 0.  When w > 0 is false -- a zero, negative or NaN confidence -- the joint takes no data term and its
 *              anchor is NOT READ: a missing detection may hold anything, a NaN included.
 * anchor [B,J,4] and conf [B,J] are laid out as the poses are (DEVICE memory for the device entry point, HOST memory for the host twin);
 * they may be q_in itself or overlap it, and must not overlap q_out.  Without tracks (frames == 0) the call may still run in place.
 * With anchor == NULL and flags == 0 the call is the one with the 48-byte struct, bit for bit; with mu == 0 it is that call too and
 * the anchors are never read.  Fill it with
 *   pndf_project_options4 o;  pndf_default_project_options(&o.base3.base2.base);  o.base3.base2.base.struct_size = sizeof o;
 *   o.base3.base2.observed = NULL;  o.base3.base2.reserved = 0;  o.base3.frames = T;  o.base3.lambda = 0.5f;
 *   o.base3.fill = PNDF_TRACK_GIVEN;  o.base3.reserved2 = 0;  o.anchor = noisy;  o.conf = NULL;  o.mu = 0.25f;  o.flags = PNDF_TRACK_FREE_ENDS;
 * and pass (const pndf_project_options*)&o.  Exactly the two entry points that take a pndf_project_options3 take it: pndf_skel_project
 * and pndf_project_ex_cpu; every other function with a pndf_project_options parameter keeps refusing a struct_size other than
 * sizeof(pndf_project_options).  PNDF_ERR_BAD_ARG with a text that names the field, before anything is launched or written: a
 * struct_size that is none of the four sizes, a mu outside [0, 1] or NaN, an unknown bit in flags, anchor == NULL with mu != 0 or
 * conf != NULL, a misaligned anchor or conf, PNDF_TRACK_FREE_ENDS with frames == 0 or with a fill other than PNDF_TRACK_GIVEN, anchor
 * or conf overlapping q_out, and what is refused in `base3`. */
enum { PNDF_TRACK_FREE_ENDS = 1 };
typedef struct {
    pndf_project_options3 base3;  /* base3.base2.base.struct_size = sizeof(pndf_project_options4); mask and tracks as before */
    const float* anchor;          /* [B,J,4] the observation, or NULL (no data term); 4-byte aligned */
    const float* conf;            /* [B,J] per-joint confidence, or NULL (ones); 4-byte aligned */
    float mu;                     /* weight of the data term, in [0, 1] */
    uint32_t flags;               /* 0 or PNDF_TRACK_FREE_ENDS */
} pndf_project_options4;          /* 72 bytes */

/* The options with 3D keypoints: inverse kinematics under the learned prior inside the projection step, for any joint tree.  The joint
 * tree with its rest offsets is the body model: rest[j] is joint j relative to its parent in the rest pose (the position of a root), and
 * keypoint k is rigidly attached to joint kp_joint[k] at the local offset kp_offset[k] (zero: the joint itself; an end effector is a
 * keypoint with an offset on a leaf).  For one pose Q [J,4], real part first:
 *   r_j = Q_j / max(|Q_j|, 1e-12), R_j its rotation matrix;  root: G_j = R_j, p_j = t_j;  else: G_j = G_parent R_j, p_j = p_parent + G_parent t_j
 *   P_k = p_a(k) + G_a(k) o_k        E(Q) = 1/2 sum_k w_k |P_k - Y_k|^2        w_k = kp_conf[pose][k] (1 when kp_conf is NULL)
 * A keypoint whose w_k > 0 is false -- zero, negative or NaN -- takes no part and its target is NOT READ (the rule of anchor / conf).
 * The step of a free joint quaternion is that of pndf_project_options4 with one more term, taken at the step's input iterate: the
 * descent, the neighbour coupling, the data term w (A - Q), then u <- u - nu * dE/dQ_j, then renorm / flip / tol.  dE/dQ_j is the exact
 * gradient with respect to the raw quaternion, through R(r) and through r = Q / |Q| (linear where the norm is clamped).  Held joints keep
 * their bits and still rotate their subtree; a pose that rests under tol stays as it is; a joint without a keypoint in its subtree takes a
 * gradient of exactly zero.  Targets are in the roots' frame.
 * kp_target [B,K,3], kp_conf [B,K] and kp_energy [B] are DEVICE memory for pndf_skel_project and HOST memory for pndf_project_ex_cpu; rest,
 * kp_joint and kp_offset are HOST memory in both and are read during the call.  With kp_target == NULL or nu == 0 the call is the one
 * with the 72-byte struct, bit for bit, no keypoint array is read, and kp_energy (when given) is zeroed.  Fill it with
 *   pndf_project_options5 o;  memset(&o, 0, sizeof o);  pndf_default_project_options(&o.base4.base3.base2.base);
 *   o.base4.base3.base2.base.struct_size = sizeof o;  o.kp_target = detections;  o.rest = offsets;  o.n_keypoints = J;  o.nu = 0.02f;
 * and pass (const pndf_project_options*)&o.  Exactly the two entry points that take a pndf_project_options4 take it.  PNDF_ERR_BAD_ARG
 * with a text that names the field, before anything is launched or written: a struct_size that is none of the five sizes, a nu that is
 * negative or not finite, with kp_target != NULL an n_keypoints outside 1 .. 64, rest == NULL, kp_joint == NULL with n_keypoints != J, a
 * kp_joint entry outside 0 .. J-1, a rest or kp_offset value that is not finite; a misaligned pointer; kp_target, kp_conf or kp_energy
 * overlapping q_out; and what is refused in `base4`. */
typedef struct {
    pndf_project_options4 base4;   /* base4.base3.base2.base.struct_size = sizeof(pndf_project_options5); mask, tracks, observation as before */
    const float*   kp_target;      /* [B,K,3] or NULL (no keypoint term); DEVICE (pndf_skel_project) / HOST (pndf_project_ex_cpu) */
    const float*   kp_conf;        /* [B,K] or NULL (ones); the same memory space */
    float*         kp_energy;      /* [B] or NULL: E of the last iteration, evaluated before its update (as d_last); 0 when steps == 0 */
    const float*   rest;           /* [J,3]; HOST memory in both entry points, read during the call */
    const int32_t* kp_joint;       /* [K] in 0 .. J-1, HOST memory; NULL: K must equal J and keypoint k is joint k */
    const float*   kp_offset;      /* [K,3], HOST memory; NULL: zeros */
    int32_t        n_keypoints;    /* K, 1 .. 64 */
    float          nu;             /* weight of the keypoint term, finite and >= 0 */
} pndf_project_options5;           /* 128 bytes */

/* The options with a camera: the keypoint term of pndf_project_options5 on 2D detections, and a placement of the joint tree in the
 * target's frame (the "root": a rotation and a translation per pose) that the step may move.  For one pose, at the step's input iterate,
 * every operation rounded to fp32 on its own in the order written:
 *   c^ = c / max(|c|, 1e-12), R_c its rotation matrix;  C_k = R_c P_k + s  (P_k as above, in the roots' frame); root == NULL: C_k = P_k
 *   kp_flags == 0:     kp_target [B,K,3],  e_k = C_k - Y_k,  E = 1/2 sum_k w_k |e_k|^2,  a_k = dE/dC_k = w_k e_k
 *   PNDF_KP_IMAGE:     kp_target [B,K,2] in pixels.  A keypoint for which C_kz > 0 is false (behind the camera, in its plane, NaN) takes
 *                      no part in that step, as one whose w_k > 0 is false.  Otherwise n = (C_x / C_z, C_y / C_z),
 *                      y' = ((Y_u - cx) / fx, (Y_v - cy) / fy), e = n - y' (normalised image coordinates: E does not depend on the
 *                      resolution), E = 1/2 sum_k w_k [rho(e_u) + rho(e_v)] with rho(e) = e^2 for rho == 0, else
 *                      rho^2 e^2 / (e^2 + rho^2); with psi(e) = e for rho == 0, else e rho^4 / (e^2 + rho^2)^2:
 *                      a_k = w_k (psi_u / C_z, psi_v / C_z, -(psi_u n_u + psi_v n_v) / C_z)
 *   into the tree:     dE/dP_k = R_c^T a_k takes the place of w_k (P_k - Y_k); the joints then step as with the 128-byte struct
 *   into the root:     dE/ds = sum_k a_k;  the adjoint of R_c is sum_k a_k P_k^T, and dE/dc goes through R(c^) and c^ = c / |c| as a
 *                      joint's does.  Unless the pose rests under tol: s <- s - nu_trans * dE/ds, and when nu_rot > 0
 *                      c <- unit(c - nu_rot * dE/dc); with nu_rot == 0 c keeps its bits.  The root is not a joint: neither the joint
 *                      mask nor the held end frames of tracks hold it.
 * root [B,7] (c real part first, then s) is DEVICE memory for pndf_skel_project and HOST memory for pndf_project_ex_cpu; it is READ by
 * every step and WRITTEN by every step when a root weight is positive.  With root == NULL, kp_flags == 0 and both root weights 0 the
 * call is the one with the 128-byte struct, bit for bit; with kp_target == NULL or nu == 0, and both root weights 0, it is the one with
 * the 72-byte struct and root is neither read nor written.  (Without a keypoint term there is no energy for the root to descend, so it is
 * left as it is whatever its weights; to move the root alone, hold every joint with the mask.)  Fill it as a pndf_project_options5 with
 *   o.base5.base4.base3.base2.base.struct_size = sizeof o;  o.root = placement;  o.fx = o.fy = 500.f;  o.cx = 320.f;  o.cy = 240.f;
 *   o.nu_rot = 0.02f;  o.nu_trans = 0.02f;  o.kp_flags = PNDF_KP_IMAGE;
 * Exactly the two entry points that take a pndf_project_options5 take it.  PNDF_ERR_BAD_ARG with a text that names the field, before
 * anything is launched or written: a struct_size that is none of the ten sizes, an unknown bit in kp_flags, a rho, nu_rot or nu_trans
 * that is negative or not finite, rho != 0 without PNDF_KP_IMAGE, with PNDF_KP_IMAGE an fx or fy that is not finite or <= 0 or a cx or
 * cy that is not finite, root == NULL with a positive root weight, a misaligned root, root overlapping q_out, with a positive root
 * weight root overlapping q_in, anchor, conf, kp_target, kp_conf or kp_energy; and what is refused in `base5`. */
enum { PNDF_KP_IMAGE = 1 };
typedef struct {
    pndf_project_options5 base5;  /* base5.base4.base3.base2.base.struct_size = sizeof(pndf_project_options6) */
    float*   root;                /* [B,7] (c: quaternion, real part first; s: translation), or NULL = identity; DEVICE / HOST as the poses */
    float    fx, fy, cx, cy;      /* pinhole intrinsics; read only with PNDF_KP_IMAGE */
    float    rho;                 /* robustifier of the image residual, >= 0, 0 = squared error */
    float    nu_rot, nu_trans;    /* weights of the root's own step, finite and >= 0; 0 = that part of the root is held */
    uint32_t kp_flags;            /* 0 or PNDF_KP_IMAGE */
} pndf_project_options6;          /* 168 bytes */

/* The options with bone lengths: the fit of pndf_project_options6 on a joint tree whose segment lengths are unknowns too, one set per
 * track.  S = J + K scales: sigma_j (j < J) scales joint j's rest offset, t'_j = sigma_j t_j per component, sigma_{J+k} keypoint k's local
 * offset, o'_k = sigma_{J+k} o_k; forward kinematics, keypoints, camera and root are those of the 168-byte struct on t' and o'.  With
 * base3.frames = T >= 2 and without PNDF_LEN_PER_POSE there are G = B / T groups: track g owns row g of bone_scale and all its frames read
 * it; otherwise G = B, one row per pose (PNDF_LEN_PER_POSE with frames == 0 is accepted and says what holds there anyway).  For one step,
 * every operation rounded to fp32 on its own in the order written:
 *   per frame  h_j = <ap_j, v_j> for a joint (ap_j the complete adjoint of p_j: its own keypoints and all its children; v_j = G_pi(j) t_j
 *              on the unscaled t_j, t_j itself for a root), h_{J+k} = <dE/dP_k, G_a(k) o_k> for a keypoint (exactly 0 for one that is
 *              skipped); the term ap_c t_c^T of a parent's M uses the scaled t'_c.  Held end frames and masked joints contribute: like
 *              the root, the scales are not joints.
 *   per group  H_i = the sum of h_i over the group's n frames: the partial of every block of 64 consecutive frames accumulated in frame
 *              order from 0.0f (the last block may be shorter), the partials then added in block order from 0.0f
 *   the step   w_i = nu_len * len_rate_i; if w_i > 0 is false the scale keeps its bits; if tol > 0 and every frame of the group rests
 *              (d < tol) the group keeps its bits; else m = H_i / (float)n, pr = kappa * (sigma_i - 1.0f), gsum = m + pr,
 *              v = sigma_i - w_i * gsum, and with a clamp sigma_i <- v < len_min ? len_min : (v > len_max ? len_max : v) (a NaN stays).
 * The update is Jacobi: every frame of a step reads the scales as the step before left them; kp_energy is E at the step's input scales.
 * bone_scale [G,S] is DEVICE memory for pndf_skel_project and HOST memory for pndf_project_ex_cpu, READ by every step and WRITTEN by every
 * step when nu_len > 0.  With bone_scale == NULL (then nu_len must be 0), or with every scale 1.0f and nu_len == 0, the call is the one with
 * the 168-byte struct bit for bit and bone_scale is not written; with kp_target == NULL or nu == 0 it is the one with the 72-byte struct
 * and bone_scale is neither read nor written; steps == 0 leaves it untouched.  Exactly the two entry points that take a
 * pndf_project_options6 take it.  PNDF_ERR_BAD_ARG with a text that names the field, before anything is launched or written: a
 * struct_size that is none of the ten sizes, reserved3 != 0, an unknown bit in len_flags, a nu_len or kappa that is negative or not
 * finite, a clamp that is not 0 < len_min <= len_max finite (both 0: none), a len_rate entry that is negative or not finite, bone_scale
 * == NULL with nu_len > 0, a misaligned bone_scale or len_rate, bone_scale overlapping q_out, q_in, root, anchor, conf, kp_target, kp_conf
 * or kp_energy; and what is refused in `base6`. */
enum { PNDF_LEN_PER_POSE = 1 };
typedef struct {
    pndf_project_options6 base6;   /* base6.base5.base4.base3.base2.base.struct_size = sizeof(pndf_project_options7) */
    float*       bone_scale;       /* [G,S], S = J + K; DEVICE (pndf_skel_project) / HOST (pndf_project_ex_cpu); NULL: all ones, no fitting */
    const float* len_rate;         /* [S], HOST memory, finite and >= 0; NULL: ones.  0 = that scale keeps its bits */
    float        nu_len;           /* weight of the scales' own step, finite and >= 0 */
    float        kappa;            /* weight of the prior 1/2 kappa (sigma - 1)^2, finite and >= 0 */
    float        len_min, len_max; /* both 0: no clamp; else 0 < len_min <= len_max, finite */
    uint32_t     len_flags;        /* 0 or PNDF_LEN_PER_POSE */
    uint32_t     reserved3;        /* 0 */
} pndf_project_options7;           /* 208 bytes */

/* The options with several cameras: the fit of pndf_project_options7 to pixels seen by V calibrated views of the same frame.  The root
 * (c, s) places the tree in a WORLD frame, W_k = R_c P_k + s (root == NULL: W_k = P_k); view v is a row of 16 floats of `views`:
 * fx, fy, cx, cy, then R_v [9] row-major (world -> camera), then t_v [3].  R_v need not be orthonormal: the gradient is exact for any
 * matrix.  For one step, every operation rounded to fp32 on its own in the order written, keypoints in the outer loop and views
 * 0 .. V-1 in the inner one:
 *   C_vk = R_v W_k + t_v, every row (a0 b0 + a1 b1) + a2 b2, then the add.  View v takes no part for keypoint k when w_vk > 0 is false
 *   (w_vk = kp_conf[b][v][k], or 1 when kp_conf == NULL) or when C_z > 0 is false; its target is then NOT READ and may hold anything.
 *   A view that takes part: n, y', e, rho, psi and a_vk as PNDF_KP_IMAGE of the 168-byte struct states them, with view v's intrinsics;
 *   its share w_vk [rho(e_u) + rho(e_v)] is added to the energy in that order, and aW_k = sum_v R_v^T a_vk is accumulated in view order
 *   from 0.0f.  After the views aW_k takes the place of a_k in dE/ds, in the adjoint of R_c (with P_k), as R_c^T aW_k in the tree and in
 *   h_{J+k} of the scales -- only when at least one view took part; otherwise the keypoint adds nothing anywhere.
 * Joints, root, scales, masks, tracks, anchor and tol are those of the 208-byte struct.  With n_views = V > 0: kp_target is [B,V,K,2] in
 * pixels, kp_conf [B,V,K]; kp_energy, root and bone_scale keep their shapes; kp_flags must have PNDF_KP_IMAGE; the intrinsics of `base6`
 * are not read.  `views` is HOST memory in both entry points, read during the call.  With views == NULL and n_views == 0 the call is the
 * one with the 208-byte struct bit for bit; with kp_target's term absent (nu == 0) it is the one with the 72-byte struct and neither the
 * targets nor the confidences are read.  Exactly the two entry points that take a pndf_project_options7 take it.  PNDF_ERR_BAD_ARG with a
 * text that names the field, before anything is launched or written: a struct_size that is none of the ten sizes, reserved4 != 0,
 * n_views outside 0 .. PNDF_FK_MAX_VIEWS, exactly one of views == NULL and n_views == 0, n_views > 0 without PNDF_KP_IMAGE or without
 * kp_target, a view whose fx or fy is not finite or <= 0, any other view entry that is not finite, a misaligned views; and what is
 * refused in `base7` (the overlap checks of kp_target and kp_conf with their extents [B,V,K,2] and [B,V,K]). */
enum { PNDF_FK_MAX_VIEWS = 8 };
typedef struct {
    pndf_project_options7 base7;   /* base7.base6.base5.base4.base3.base2.base.struct_size = sizeof(pndf_project_options8) */
    const float* views;            /* [V,16] HOST memory in both entry points: fx, fy, cx, cy, R_v[9] row-major, t_v[3]; NULL: no views */
    int32_t      n_views;          /* V, 0 or 1 .. PNDF_FK_MAX_VIEWS */
    uint32_t     reserved4;        /* 0 */
} pndf_project_options8;           /* 224 bytes */

/* The options with a root trajectory: the fit of pndf_project_options8 with the root (c, s) of every frame coupled to the roots of its
 * neighbour frames in the track and, optionally, drawn towards an observed or earlier trajectory `root_anchor` [B,7].  For one pose the
 * joints, scales, energy, views, mask, tracks and tol are those of the 224-byte struct; only the root's own step changes
 * (pndf_fk_root_smooth_step of csrc/pndf_fk.h).  Every operation rounded to fp32 on its own in the order written; c, s: the root at the
 * step's input, g_c, g_s: d E / d (c, s), frame k = pose % frames.  A pose that rests under tol keeps its root bits.
 *   rotation, when nu_rot > 0:   u = c - nu_rot g_c
 *     lambda_rot > 0:  N-, N+ the root rotations of frames k-1 and k+1 of the same track at the step's INPUT (the step is Jacobi), each
 *                      negated where its dot product with c is negative; an interior frame  u <- u + lambda_rot ((0.5 (N- + N+)) - c),
 *                      an end frame with its one neighbour N  u <- u + lambda_rot (0.5 (N - c))
 *     mu_rot > 0:      A the anchor's rotation, aligned to c the same way;  u <- u + mu_rot (A - c)
 *     c <- u / max(|u|, 1e-12)
 *   translation, when nu_trans > 0: the same three parts on the three components of s with lambda_trans and mu_trans, without alignment
 *     and without normalisation.
 * A part whose nu is 0 keeps its bits and reads neither neighbours nor anchor; the anchor of a part is not read when its mu is 0.  The
 * root is not a joint: the end frames take the one-neighbour term whether or not PNDF_TRACK_FREE_ENDS is set, and the mask does not hold
 * the root.  With lambda_rot = lambda_trans = 0 and root_anchor == NULL the call is the one with the 224-byte struct bit for bit; with
 * kp_target == NULL or nu == 0 it is the one with the 72-byte struct and neither root nor root_anchor is read or written; steps == 0
 * leaves root untouched.  After the call the result is in `root`, whatever the parity of steps.  Exactly the two entry points that take a
 * pndf_project_options8 take it.  PNDF_ERR_BAD_ARG with a text that names the field, before anything is launched or written: a
 * struct_size that is none of the ten sizes, reserved5 != 0, a lambda or mu outside [0, 1] or NaN, a positive lambda with frames == 0, a
 * positive lambda_rot or mu_rot with nu_rot == 0 (likewise the translation), a positive lambda or mu with root == NULL, a positive mu with
 * root_anchor == NULL, root_anchor != NULL with both mu 0, a misaligned root_anchor, root_anchor overlapping root or q_out; and what is
 * refused in `base8`. */
typedef struct {
    pndf_project_options8 base8;   /* base8.base7.base6.base5.base4.base3.base2.base.struct_size = sizeof(pndf_project_options9) */
    const float* root_anchor;      /* [B,7] an observed / earlier root trajectory, or NULL; DEVICE (pndf_skel_project) / HOST (pndf_project_ex_cpu) */
    float lambda_rot, lambda_trans;/* neighbour coupling of the root's rotation / translation, each in [0, 1] */
    float mu_rot, mu_trans;        /* weight of the root's data term towards root_anchor, each in [0, 1] */
    uint64_t reserved5;            /* must be 0 */
} pndf_project_options9;           /* 256 bytes */

/* The options with moving cameras: the fit of pndf_project_options9 with a view table per pose, or per frame of a track, in place of the
 * one table of pndf_project_options8.  `pose_views` is [B,V,16] (view_flags == 0: pose b reads block b) or [T,V,16] with T = frames
 * (PNDF_VIEWS_PER_FRAME: pose b reads block b % T, one camera path shared by every track of the call); a row is fx, fy, cx, cy, R_v [9]
 * row-major (world -> camera), t_v [3], as in the 224-byte struct.  The table is DEVICE memory for pndf_skel_project and HOST memory for
 * pndf_project_ex_cpu, read by every step, and 16-byte aligned.  The term is the several-camera term of the 224-byte struct, operation
 * for operation and in its order (pndf_fk_cams_energy_grad of csrc/pndf_fk.h), with the pose's own block, and with one rule more, which
 * is the table's validation -- the library cannot look at values in device memory:
 *   view v takes no part for a pose when fx > 0 && fy > 0 is false for that pose's row v.  This comes before anything else of the view:
 *   neither kp_conf [b][v][*] nor kp_target [b][v][*] is read, and the rest of the row may hold anything.  A row of zeros or NaNs says
 *   "no calibration for this camera in this frame".  No division by a focal length that is not positive happens.
 * In a row whose fx and fy are positive, finite cx, cy, R_v and t_v are the CALLER's responsibility, as finite targets are.  A pose whose
 * every view is skipped has energy 0 and takes the step of the prior alone.  With n_pose_views = V > 0: kp_target is [B,V,K,2], kp_conf
 * [B,V,K], kp_flags must have PNDF_KP_IMAGE, base9.base8.views must be NULL; root, root_anchor, the lambdas and mus, bone_scale, masks
 * and tracks are those of the 256-byte struct.  With pose_views == NULL, n_pose_views == 0 and view_flags == 0 the call is the one with
 * the 256-byte struct bit for bit; without a keypoint term (kp_target == NULL or nu == 0) nothing of the table is read and the call is
 * the one with the 72-byte struct.  Exactly the two entry points that take a pndf_project_options9 take it.  PNDF_ERR_BAD_ARG with a text
 * that names the field, before anything is launched or written: a struct_size that is none of the ten sizes, reserved6 != 0, an unknown
 * bit in view_flags, n_pose_views outside 0 .. PNDF_FK_MAX_VIEWS, exactly one of pose_views == NULL and n_pose_views == 0, view_flags
 * != 0 without a table, PNDF_VIEWS_PER_FRAME with frames == 0, a pose_views that is not 16-byte aligned, pose_views together with
 * base9.base8.views or n_views, n_pose_views > 0 without PNDF_KP_IMAGE or without kp_target, pose_views overlapping q_out, root (when a
 * root weight is positive) or bone_scale (when nu_len > 0); and what is refused in `base9`. */
enum { PNDF_VIEWS_PER_FRAME = 1 };     /* view_flags: pose_views is [frames,V,16], pose b reads block b % frames */
typedef struct {
    pndf_project_options9 base9;   /* base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = sizeof(pndf_project_options10) */
    const float* pose_views;       /* [B,V,16] or [frames,V,16], 16-byte aligned, or NULL; DEVICE (pndf_skel_project) / HOST (pndf_project_ex_cpu) */
    int32_t      n_pose_views;     /* V, 0 or 1 .. PNDF_FK_MAX_VIEWS */
    uint32_t     view_flags;       /* 0 or PNDF_VIEWS_PER_FRAME */
    uint64_t     reserved6;        /* must be 0 */
} pndf_project_options10;          /* 280 bytes */

/* pndf_project with step options.  opt == NULL means the defaults, and with the defaults the call is pndf_project bit for
 * bit.  PNDF_ERR_BAD_ARG (text in pndf_last_error; nothing is launched or written) for a struct_size other than
 * sizeof(pndf_project_options), a step_size that is not finite or <= 0, a tol that is NaN or < 0, an unknown renorm mode.
 * d_last[b] stays dist_pred of the last iteration, evaluated before its update.  Every kernel behind pndf_project honours the
 * options (all precisions, the encoder-less model, the runtime-planned networks). */
int pndf_project_ex(pndf_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                    const pndf_project_options* opt, void* stream);

/* ---- host twins (SURVEY.md 8b `pndf_*_cpu`): the same three operations on HOST pointers, for a caller whose
 * `train.device` is "cpu" (model/posendf.py:35,64 runs wherever the config says).  A separate handle type with no device
 * behind it: plain C++ on the host cores, fp32, PyTorch's activation conventions; blocks of 32 poses are dealt to threads
 * (PNDF_CPU_THREADS, default: all hardware threads).  Same configurations as pndf_create (all three activations, the
 * encoder-less model, narrower hidden layers; `precision` is ignored) and, for the six first-order calls below, any joint tree
 * that pndf_skel_create takes (posendf_amd_skeleton.h: 1 .. 32 joints, parent[j] in -1 .. j-1, dims[0] = 6 J or 4 J, poses
 * [B, J, 4]); same status codes; no stream argument: the calls
 * return when the result is in memory.  Never used as a fallback: the device entry points above fail when there is no
 * gfx950 device. */
typedef struct pndf_cpu_engine* pndf_cpu_handle;
int pndf_cpu_create(pndf_cpu_handle* out, const pndf_config* cfg);
int pndf_cpu_destroy(pndf_cpu_handle h);
int pndf_cpu_load_weights(pndf_cpu_handle h, const float* const* tensors, const int64_t* numel, int n_tensors);   /* as pndf_load_weights */
int pndf_forward_cpu(pndf_cpu_handle h, const float* q, float* d, int64_t B);                                       /* posendf.py:62-76 */
int pndf_forward_grad_cpu(pndf_cpu_handle h, const float* q, const float* grad_out, float* d, float* dq, int64_t B); /* posendf.py:18-27 */
int pndf_project_cpu(pndf_cpu_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps);      /* sample_poses.py:67-74 */
int pndf_project_ex_cpu(pndf_cpu_handle h, const float* q_in, float* q_out, float* d_last, int64_t B, int steps,
                        const pndf_project_options* opt);      /* pndf_project_ex: same semantics, same validation; also takes a
                                                                  pndf_project_options2, a pndf_project_options3, a
                                                                  pndf_project_options4, a pndf_project_options5, a
                                                                  pndf_project_options6, a pndf_project_options7, a
                                                                  pndf_project_options8, a pndf_project_options9 or a
                                                                  pndf_project_options10, `observed` / `anchor` / `conf` /
                                                                  `kp_*` / `root` / `bone_scale` / `root_anchor` /
                                                                  `pose_views` in HOST memory */
const char* pndf_cpu_last_error(pndf_cpu_handle h);   /* h may be NULL: last error of a failed pndf_cpu_create */

/* Host-only weight packer (what pndf_load_weights uploads); needs no device.  Output sizes in floats come
 * from pndf_packed_sizes.  Used by the CPU tests that check the MFMA tile order against a lane-level model. */
void pndf_packed_sizes(int64_t* stream_floats, int64_t* bias_floats);
int pndf_pack_host(const float* const* tensors, const int64_t* numel, int n_tensors, float* stream,
                   float* bias);
/* same for the split-precision stream (same size in bytes; trunk tiles hold fp16 pairs) */
int pndf_pack_host_split(const float* const* tensors, const int64_t* numel, int n_tensors, float* stream,
                         float* bias);

/* ---- motion-denoise optimiser step around the engine (experiments/motion_denoise.py:29-45,70-99).
 * Stateless helpers (no handle; status codes as above, no error text).  One Adam step =
 *   pndf_forward_grad(h, q, NULL, d, dq, S*T, stream);  pndf_denoise_update(...)   -- q for the first step from
 * pndf_aa2quat.  Terms: pose prior 1e7 c_s^2 / (1+it), c_s = mean_t d (:81-83,33) and the pose-space surrogates of the
 * SMPL temporal / data terms (:31-32,88-94; the body model itself is out of scope).  Adam(lr, 0.9, 0.999, 1e-8) (:70): the
 * arithmetic of pndf_adam_step with weight decay 0 -- `float lr` is widened and the step's scalars are formed in double. */
/* theta [N,69] axis-angle (SMPL body pose) -> q [N,21,4] real-part-first quaternions of the first 21 joints
 * (pytorch3d.transforms.axis_angle_to_quaternion, :81). */
int pndf_aa2quat(const float* theta, float* q, int64_t N, void* stream);
/* theta_in/theta_out/theta0/m/v: [S,T,69]; d: [S*T]; dq, q_next: [S*T,21,4].  theta_in != theta_out (frames read their
 * neighbours; swap the buffers every step).  `it` = outer iteration (weights), `adam_step` = 1, 2, ... */
int pndf_denoise_update(const float* theta_in, float* theta_out, const float* theta0, const float* d, const float* dq,
                        float* m, float* v, float* q_next, int32_t S, int32_t T, int32_t it, int32_t adam_step, float lr,
                        void* stream);

/* The same step with EXPLICIT loss weights of the current outer iteration -- for callers whose schedule differs from
 * motion_denoise.py's, e.g. the copy of the loop in experiments/partial_observation.py:29-35 (temp 1e2 (1+it), data 1e1/(1+it),
 * pose prior 1e2 c/(1+it): LINEAR in c).  Objective: prior_coef * c^prior_power + temp_coef * temp + data_coef * data with
 * c = mean_t d; prior_power 1 or 2; data_coef 0 switches the data term off (the reference does for it == 0).  g_body NULL:
 * pose-space surrogates; otherwise the body-model gradient of pndf_lbs_terms_grad_w, evaluated with the same temp / data weights. */
typedef struct {
    float prior_coef;
    int32_t prior_power;
    float temp_coef;
    float data_coef;
} pndf_denoise_weights;
int pndf_denoise_update_w(const float* theta_in, float* theta_out, const float* theta0, const float* d, const float* dq,
                          const float* g_body, float* m, float* v, float* q_next, int32_t S, int32_t T,
                          const pndf_denoise_weights* w, int32_t adam_step, float lr, void* stream);

/* The same Adam step with the gradient of the BODY-MODEL terms (SMPL vertex temporal term + joint data term,
 * motion_denoise.py:86-94) in place of the pose-space surrogates: g_body [S,T,69] = d(weighted temp + data terms)/d theta as
 * produced by pndf_lbs_terms_grad below.  All 23 joints of the body pose are updated (the surrogates leave the two hand
 * joints alone; the body model moves vertices with them). */
int pndf_denoise_update_body(const float* theta_in, float* theta_out, const float* theta0, const float* d, const float* dq,
                             const float* g_body, float* m, float* v, float* q_next, int32_t S, int32_t T, int32_t it,
                             int32_t adam_step, float lr, void* stream);

/* ---- SMPL-shaped body model: linear-blend skinning and the body-model terms of the motion-denoise objective
 * (SURVEY 8f-3).  Replaces experiments/body_model.py:27-40 (smplx.SMPL called with betas, body_pose, global_orient = None)
 * and experiments/motion_denoise.py:86-94 (vertex temporal term, joint data term) with their reverse pass.  smplx and the
 * SMPL model files are third-party and absent from the reference: the published lbs() algorithm is restated, parity
 * unpinned.  The model is supplied by the caller as plain arrays (HOST pointers, fp32, the shapes of the SMPL model file):
 *   v_template [V,3]; shapedirs [V,3,NB] and betas [NB] (fixed during the optimisation, motion_denoise.py:27,67; NB may be 0);
 *   posedirs [207, 3V] (row k = entry k of the pose feature (R_1..R_23 - I), as smplx stores it); J_regressor [24,V];
 *   parents [24] (parents[0] = -1, every parent before its children); lbs_weights [V,24];
 *   extra_joint_vertex [n_extra <= 32]: joints picked from vertices (smplx VertexJointSelector; SMPL: 21 -> 45 joints).
 * Compute calls take DEVICE pointers, enqueue on `stream`, allocate nothing: scratch comes from the caller
 * (`workspace`: pndf_lbs_workspace_floats(h, S, T) floats, 16-byte aligned, for S sequences of T frames; the flat calls
 * with N frames use S = 1, T = N). */
typedef struct pndf_lbs_model* pndf_lbs_handle;
int pndf_lbs_create(pndf_lbs_handle* out, int32_t V, int32_t NB, const float* v_template, const float* shapedirs,
                    const float* betas, const float* posedirs, const float* J_regressor, const int32_t* parents,
                    const float* lbs_weights, const int32_t* extra_joint_vertex, int32_t n_extra, int device);
int pndf_lbs_destroy(pndf_lbs_handle h);
/* Arithmetic of the forward and fused-terms passes.  PNDF_LBS_F16X3 (default): the vertex-side contractions on fp16 MFMAs
 * with every fp32 operand split into fp16 hi + lo (three products per block, fp32 accumulate) -- the arithmetic of the
 * distance engine's f16x3 kernels, fp32-class accuracy; PNDF_LBS_FP32: the same on fp32 MFMAs (exact fp32 products).  The
 * general reverse pass (pndf_lbs_backward) always runs on fp32.  Returns 0 or a negative pndf_status. */
enum { PNDF_LBS_FP32 = 0, PNDF_LBS_F16X3 = 1 };
int pndf_lbs_set_precision(pndf_lbs_handle h, int32_t precision);
int32_t pndf_lbs_precision(pndf_lbs_handle h);         /* -1 for a NULL handle */
int32_t pndf_lbs_num_joints(pndf_lbs_handle h);        /* 24 + n_extra */
int32_t pndf_lbs_num_vertices(pndf_lbs_handle h);
int64_t pndf_lbs_workspace_floats(pndf_lbs_handle h, int32_t S, int32_t T);
/* BodyModel.forward(pose_body = theta, betas) (body_model.py:33-52): theta [N,69] -> verts [N,V,3] (may be NULL),
 * joints [N, 24 + n_extra, 3] (may be NULL; `Jtr` of the reference). */
int pndf_lbs_forward(pndf_lbs_handle h, const float* theta, int64_t N, float* verts, float* joints, void* workspace,
                     void* stream);
/* d / d theta of  10 (1 + it) mean_{t,v} |V[t,v] - V[t+1,v]|  +  [it > 0] 100 / (1 + it) mean_{t,j} |Jtr[t,j] - joints0[t,j]|
 * (motion_denoise.py:31-32,88-89,92-94) per sequence: theta, g_theta [S,T,69]; joints0 [S,T,24 + n_extra,3] (may be NULL
 * when it == 0).  One fused pass: vertices never reach HBM.  Like the reference there is no epsilon under the roots
 * (identical consecutive vertices give NaN). */
int pndf_lbs_terms_grad(pndf_lbs_handle h, const float* theta, const float* joints0, int32_t S, int32_t T, int32_t it,
                        float* g_theta, void* workspace, void* stream);
/* The same with explicit weights: d / d theta of temp_coef * temp + data_coef * data (data_coef == 0: no data term). */
int pndf_lbs_terms_grad_w(pndf_lbs_handle h, const float* theta, const float* joints0, int32_t S, int32_t T, float temp_coef,
                          float data_coef, float* g_theta, void* workspace, void* stream);
/* General reverse pass: g_theta [N,69] = d (<g_verts, verts> + <g_joints, joints>) / d theta (either may be NULL). */
int pndf_lbs_backward(pndf_lbs_handle h, const float* theta, const float* g_verts, const float* g_joints, int64_t N,
                      float* g_theta, void* workspace, void* stream);
/* Host-only model packer (what pndf_lbs_create uploads; needs no device): `blob` takes pndf_lbs_packed_floats(V) floats in
 * MFMA tile order, J_out / rel_out (72 floats each, may be NULL) the rest joints and their parent-relative offsets. */
int64_t pndf_lbs_packed_floats(int32_t V);
int pndf_lbs_pack_host(int32_t V, int32_t NB, const float* v_template, const float* shapedirs, const float* betas,
                       const float* posedirs, const float* J_regressor, const int32_t* parents, const float* lbs_weights,
                       const int32_t* extra_joint_vertex, int32_t n_extra, float* blob, float* J_out, float* rel_out);
/* The model for PNDF_LBS_F16X3 from the packed fp32 one (host only): sblob takes pndf_lbs_packed_split_bytes(V) bytes -- per
 * 16 vertices, planes of fp16 hi / lo halves [row][16 v] of posedirs x p_scale and weights x w_scale (powers of two, returned in
 * scales_out[0..1], may be NULL), laid out in bank-conflict-free tiles (csrc/pndf_lbs_split.h). */
int64_t pndf_lbs_packed_split_bytes(int32_t V);
int pndf_lbs_pack_split_host(int32_t V, const float* blob, void* sblob, float* scales_out);
const char* pndf_lbs_last_error(pndf_lbs_handle h);    /* h may be NULL: last error of a failed pndf_lbs_create */

/* ---- the training objective (model/posendf.py:62-99, train=True; what model/train_posendf.py:87-96 runs every step) and its
 * weight gradients.  q [B,21,4] noisy poses, dist_gt [B] their labels, q_man [Bm,21,4] manifold poses:
 *   dist = mean_b |d(normalize(q, dim=1)) - dist_gt|  (loss_type 0 = L1Loss; 1 = MSELoss),  man = mean_b |d(q_man)|  (no
 *   normalisation, as in the reference),  eikonal = mean_{b,j} (|d d / d q[b,j,:]|_2 - 1)^2.
 * The handle carries the plan: the architecture of the config, i.e. every network that pndf_create accepts with the structure
 * encoder (an encoder-less config is PNDF_ERR_UNSUPPORTED: the reference cannot train one either); exact fp32 MFMA, `precision`
 * is ignored.  A handle of posendf_amd_skeleton_train.h's pndf_skel_train_create plans any joint tree of J = 1 .. 32 joints: for it
 * read [B,J,4] / [Bm,J,4] for the poses, 4 J encoder tensors in front of the trunk's, and the eikonal mean over b and the J joints.
 * Compute calls take DEVICE pointers, enqueue on `stream` and allocate nothing: all scratch is `workspace`
 * (pndf_train_workspace_floats(h, B, Bm, eikonal) floats, 16-byte aligned), which carries the forward's state to the backward.
 * Weights are read in place: `weights` is a HOST array of DEVICE pointers in state-dict order (the tensors of pndf_load_weights,
 * row-major [out,in] as torch stores them).  Deterministic: the same inputs give the same bits (fixed K splits, no atomics). */
typedef struct pndf_train_plan* pndf_train_handle;
int pndf_train_create(pndf_train_handle* out, const pndf_config* cfg, int device);    /* PNDF_ERR_NO_DEVICE without gfx950 */
int pndf_train_destroy(pndf_train_handle h);
int64_t pndf_train_workspace_floats(pndf_train_handle h, int64_t B, int64_t Bm, int32_t eikonal);
/* The forward half: both batches, the losses and, with eikonal != 0, the input gradient and the tangent pass the eikonal term's
 * double backward needs.  losses: device [3] = dist, man, eikonal (0 when eikonal == 0). */
int pndf_train_forward(pndf_train_handle h, const float* const* weights, const float* q, const float* dist_gt, const float* q_man,
                       int64_t B, int64_t Bm, int32_t loss_type, int32_t eikonal, float* losses, void* workspace, void* stream);
/* The backward half, once per forward, on the workspace that forward filled: upstream = device [3] d(total) / d(dist, man,
 * eikonal), read on the device (no synchronisation); grads: HOST array of DEVICE pointers in the order of `weights`, written
 * (not added).  With eikonal == 0 only `dist` has a gradient, as in the reference's (loss, {'dist': loss}) branch. */
int pndf_train_backward(pndf_train_handle h, const float* const* weights, const float* upstream, float* const* grads,
                        void* workspace, void* stream);
const char* pndf_train_last_error(pndf_train_handle h);  /* h may be NULL: last error of a failed pndf_train_create */

/* ---- the rest of a training step (model/train_posendf.py:92-99, model/load_data.py:43-71): with the two calls above,
 *   pndf_train_batch;  pndf_train_forward;  pndf_train_backward;  pndf_adam_step
 * is one step with no host work between the launches.  Stateless helpers (no handle; status codes as above, no error text):
 * DEVICE pointers, work enqueued on `stream`, nothing allocated, no synchronisation; plain loads and stores, no atomics: the
 * same inputs give the same bits. */
/* torch.optim.Adam(lr, betas, eps, weight_decay, amsgrad=False, maximize=False).step() (train_posendf.py:30,99) over ONE flat
 * fp32 buffer: p, g, m (exp_avg), v (exp_avg_sq) hold every tensor of the model at the same offsets (state-dict order, every
 * tensor on a 16-byte boundary); the pad elements between tensors are zero in all four buffers and stay zero, so no tensor
 * table is needed.  n: floats, any count (the tail is not read past).  Coupled L2 weight decay: g + weight_decay * p enters both
 * moments.  `step` = 1, 2, ...: the bias corrections 1 - beta^step are computed on the host in double, as torch does; eps is
 * added after the division by sqrt(1 - beta2^step).  The hyper-parameters are doubles (torch holds Python floats) and are
 * rounded to fp32 once, where torch rounds them.  step < 1, n < 0, a beta outside [0, 1), a null or misaligned pointer:
 * PNDF_ERR_BAD_ARG; n == 0: no-op. */
int pndf_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2,
                   double eps, double weight_decay, void* stream);
/* PoseData.__getitem__ (load_data.py:43-71) for every item of one batch, from a data set that is resident on the device:
 *   pose_db [N,21,4] noisy poses and dist_db [N,k] their labels, the rows of F data files one after the other, file f =
 *   rows file_off[f] .. file_off[f+1]-1 (file_off: F+1 int64, 8-byte aligned); man_db [M,21,4] manifold poses, Fm files,
 *   man_off likewise; item_file / item_man_file [items] int32: the data file and the manifold file of every item;
 *   words [items,2,num_pts] uint32: raw random words.
 * Pose i of item t is row file_off[f] + ((uint64)words[t,0,i] * len_f >> 32) of its data file f (len_f rows), its manifold pose
 * the same with words[t,1,i] in its manifold file: uniform up to a bias below len / 2^32 per row (a file has fewer than 2^32
 * rows).  Outputs in the layout pndf_train_forward takes: q [items*num_pts,21,4], dist_gt [items*num_pts] = the mean of the
 * row's k labels (fp32, summed in index order, then divided by k: load_data.py:53), q_man [items*num_pts,21,4].  flip != 0
 * negates every joint quaternion whose real part is < 0 (quat_flip, load_data.py:12-16), of the noisy poses and of the manifold
 * poses themselves (load_data.py:63 flips the noisy poses into the manifold batch instead; that is not reproduced).
 * pose_db, man_db, q, dist_gt, q_man 16-byte aligned.  The offsets live on the device and are not read back: an item that
 * names a file outside 0 .. F-1 (Fm-1) or an empty file gets NaN poses and a NaN label and nothing is read out of bounds;
 * callers refuse empty files when they load the data set.  posendf_amd_skeleton_train.h's pndf_skel_train_batch is this call for
 * poses [.,J,4] of any joint count.  F, Fm, k < 1, a negative count, a null or misaligned pointer:
 * PNDF_ERR_BAD_ARG; items == 0 or num_pts == 0: no-op. */
int pndf_train_batch(const float* pose_db, const float* dist_db, const float* man_db, const int64_t* file_off,
                     const int64_t* man_off, const int32_t* item_file, const int32_t* item_man_file, const uint32_t* words,
                     int32_t F, int32_t Fm, int32_t k, int32_t items, int32_t num_pts, int32_t flip, float* q, float* dist_gt,
                     float* q_man, void* stream);

/* ---- fitting poses to 2D keypoints through a perspective camera (experiments/image_fitting.py:67-92, camera
 * experiments/exp_utils.py:119-143; robustifier and confidence weighting of SMPLify-X, which that script copies).  Stateless
 * helpers as the two above: no handle, DEVICE pointers, enqueued on `stream`, nothing allocated, no synchronisation, no atomics,
 * the same inputs give the same bits; status codes only.
 * SMPL's global orientation r is a rotation about the rest root joint J0 = joints[n,0] and is applied here, to joints computed
 * at zero global orientation (J0 is a constant of the pose: no gradient flows into row 0 through its role as pivot):
 *   p = Rc (R(r) (x - J0) + J0) + t,   u = fx p_x / p_z + cx,   v = fy p_y / p_z + cy       (p_z <= 0: inf / NaN propagate)
 *   E_n = sum_j (w_j c_nj)^2 [rho(kx_nj - u_nj) + rho(ky_nj - v_nj)],   D_n = (t_z - depth_target)^2
 * rho(e) = e^2 for rho == 0, else rho^2 e^2 / (e^2 + rho^2) per component; c_nj = the keypoint's confidence, 1 when
 * use_conf == 0.  A joint with w_j c_nj == 0 is SKIPPED: exactly 0 in every output whatever its keypoint holds (NaN, inf).
 * R(r): smplx batch_rodrigues including its 1e-8, the convention of the pndf_lbs_* calls. */
typedef struct pndf_camera { float fx, fy, cx, cy; float R[9]; } pndf_camera;             /* R = Rc, row-major */
typedef struct pndf_keypoint_opts { float data_coef, rho, depth_coef, depth_target; int32_t use_conf, reserved; } pndf_keypoint_opts;
/* joints [N,J,3] at zero global orientation (pndf_lbs_forward), orient / transl [N,3], keypoints [N,J,3] = (x, y, conf),
 * joint_weight [J] (NULL = ones).  Outputs, each may be NULL: terms [N,2] = (E_n, D_n) unweighted; g_joints [N,J,3] (rows of
 * skipped joints are written as zeros), g_orient [N,3], g_transl [N,3] = d(data_coef sum_n E_n + depth_coef sum_n D_n)/d(.).
 * `cam` and `opt` are HOST structs, read before the call returns.  N == 0: no-op; N < 0, J < 1, a null required pointer, a null
 * cam / opt or rho < 0: PNDF_ERR_BAD_ARG. */
int pndf_keypoint_terms_grad(const float* joints, const float* orient, const float* transl, const float* keypoints,
                             const float* joint_weight, int64_t N, int32_t J, const pndf_camera* cam,
                             const pndf_keypoint_opts* opt, float* terms, float* g_joints, float* g_orient, float* g_transl,
                             void* stream);
/* the forward alone: posed [N,J,3] camera-space points p and/or uv [N,J,2] (either may be NULL) */
int pndf_keypoint_project(const float* joints, const float* orient, const float* transl, int64_t N, int32_t J,
                          const pndf_camera* cam, float* posed, float* uv, void* stream);

/* ---- quaternion pose distance + k nearest candidates (data/dist_utils.py:9-50, classes euc / geo; caller
 * data/prepare_traindata.py:159).  noise [B,21,4], valid [B,K,21,4] (device, 16-byte aligned);
 * metric 0 = geo: sum_j w_j (1 - |<q_valid_j, q_noise_j>|), 1 = euc: sum_j w_j ||q_noise_j - q_valid_j||;
 * weights = 21 HOST floats (the reference's normalised joint ranks) or NULL for the unweighted mean;
 * vals [B,k] ascending, idx [B,k] int64, ties towards the lower index; k <= min(K, 16), K <= ~1850. */
int pndf_quat_topk(const float* noise, const float* valid, int64_t B, int32_t K, int32_t metric, const float* weights,
                   int32_t k, float* vals, long long* idx, void* stream);

/* ---- exact k-nearest-pose search over a pose database (the search of data/prepare_traindata.py:152-159 with the whole
 * database as every query's candidate list: no joint-space prefilter).  Metrics and semantics of pndf_quat_topk:
 * metric 0 = geo, 1 = euc; weights = 21 HOST floats (> 0) or NULL for the unweighted mean; vals [Q,k] ascending, idx [Q,k]
 * int64, ties towards the lower database index, a NaN distance is never selected (missing slots: NaN / -1);
 * 1 <= k <= min(16, N), N < 2^31.
 * pndf_knn_create packs a copy of `poses` (device [N,21,4], 16-byte aligned) into the layout the search kernels stream and
 * synchronises `stream`: the caller may free or overwrite `poses` when it returns (FAISS `add` semantics).  Without a gfx950
 * device it returns PNDF_ERR_NO_DEVICE.  The index lives on the device of `poses`.
 * pndf_knn_search: q device [Q,21,4] (16-byte aligned), `workspace` pndf_knn_workspace_bytes(h, Q, k) bytes (16-byte aligned;
 * may be NULL when that is 0).  Allocates nothing, does not synchronise; Q = 0 is a no-op.  The plan (query blocks x
 * database splits) depends on (Q, N, k) only, and the results do not depend on it: the same bits for any chunking of the
 * queries.
 * An index over poses of another joint count J (q then [Q,J,4]): pndf_skel_knn_create of posendf_amd_skeleton_data.h. */
typedef struct pndf_knn_index* pndf_knn_handle;
int pndf_knn_create(pndf_knn_handle* out, const float* poses, int64_t N, int32_t metric, const float* weights, void* stream);
int pndf_knn_destroy(pndf_knn_handle h);
int64_t pndf_knn_size(pndf_knn_handle h);                                        /* N; -1 for a NULL handle */
int64_t pndf_knn_workspace_bytes(pndf_knn_handle h, int64_t Q, int32_t k);       /* negative pndf_status on bad arguments */
int pndf_knn_search(pndf_knn_handle h, const float* q, int64_t Q, int32_t k, float* vals, long long* idx, void* workspace,
                    void* stream);
const char* pndf_knn_last_error(pndf_knn_handle h);   /* h may be NULL: last error of a call without a handle */

const char* pndf_last_error(pndf_handle h);   /* h may be NULL: last error of a failed pndf_create */
const char* pndf_version(void);
/* 0 in every product build: one bit per compile-time tuning / ablation macro that differed from its product default when the
 * library was built (posendf_amd/csrc/pndf_experiment.h); pndf_version() prints it as `experiments=0x........`.  A library that
 * reports anything else is a lab build (tools/build_variants.py) and may compute wrong results on purpose. */
unsigned pndf_experiment_word(void);
/* Name of the device kernel the compute calls of this handle launch (valid after pndf_load_weights): for logs, profiles
 * and tests; "" for a NULL handle. */
const char* pndf_kernel_name(pndf_handle h);

#ifdef __cplusplus
}
#endif
#endif /* POSENDF_AMD_H */
