"""The C ABI of libposendf_amd.so and libposendf_amd_debug.so as ctypes sees it: the structures, the codes, one signature table
per header of include/ (`HEADERS`) and the loader that binds them.  posendf_amd/engine.py holds the wrappers that call through it;
__graft_entry__.build() and tests/test_cabi.py hold `HEADERS` against the headers and the two binaries.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint, c_void_p

# PyTorch is the plumbing for device memory and streams, so the library must share PyTorch's HIP runtime: torch is imported
# FIRST, here, so that its bundled libamdhip64 is the one already mapped when the loader resolves the library's dependency (the
# other order puts two HIP runtimes in the process and pndf_create then sees no device).  Without torch installed the system
# runtime is used.
try:
    import torch
except ImportError:
    torch = None

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libposendf_amd.so")

ACT_CODES = {"relu": 0, "lrelu": 1, "softplus": 2}
PRECISION_CODES = {"fp32": 0, "f16x3": 1, "f16": 2, "bf16": 3}
RENORM_CODES = {"none": 0, "unit": 1, "unit_flip": 2}      # PNDF_RENORM_*
INTERP_MODES = {"slerp": 0, "nlerp": 1}                    # PNDF_INTERP_*
TRACK_FILLS = {"given": 0, "slerp": 1, "nlerp": 2}         # PNDF_TRACK_*
KP_IMAGE = 1                                               # PNDF_KP_IMAGE (pndf_project_options6.kp_flags)
LEN_PER_POSE = 1                                           # PNDF_LEN_PER_POSE (pndf_project_options7.len_flags)
TRACK_FREE_ENDS = 1                                        # PNDF_TRACK_FREE_ENDS (pndf_project_options4.flags)
NOISE_CODES = {"uniform": 0, "symmetric": 1}               # PNDF_ONLINE_*
METRIC_CODES = {"geo": 0, "euc": 1}


class PndfConfig(ctypes.Structure):
    _fields_ = [("act", c_int32), ("beta", c_float), ("num_joints", c_int32), ("n_dims", c_int32),
                ("dims", c_int32 * 16), ("parent", c_int32 * 32), ("precision", c_int32), ("enc_act", c_int32), ("enc_beta", c_float)]


class ProjectOptions(ctypes.Structure):
    """pndf_project_options: step size, renormalisation and stop tolerance of pndf_project_ex"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("step_size", c_float), ("renorm", c_int32), ("tol", c_float)]


class ProjectOptions2(ctypes.Structure):
    """pndf_project_options2: the options (`base`, with struct_size = 32) and a joint mask, one uint32 per pose, bit j = joint j is
    held; taken by pndf_skel_project (device memory) and pndf_project_ex_cpu (host memory) through the options pointer"""
    _fields_ = [("base", ProjectOptions), ("observed", c_void_p), ("reserved", ctypes.c_uint64)]


class ProjectOptions3(ctypes.Structure):
    """pndf_project_options3: the options with a mask (`base2`, with base2.base.struct_size = 48) and tracks -- the poses are B / frames
    tracks of `frames` consecutive frames, the end frames held, `lambda_` the neighbour coupling of the interior ones, `fill` a
    PNDF_TRACK_* code; taken by the two entry points that take a ProjectOptions2"""
    _fields_ = [("base2", ProjectOptions2), ("frames", c_int32), ("lambda_", c_float), ("fill", c_int32), ("reserved2", c_int32)]


class ProjectOptions4(ctypes.Structure):
    """pndf_project_options4: the options with a mask and tracks (`base3`, with base3.base2.base.struct_size = 72) and an observation --
    `anchor` [B,J,4] the noisy poses the data term pulls towards (None: no data term), `conf` [B,J] per-joint confidences (None: ones),
    `mu` the data term's weight, `flags` 0 or TRACK_FREE_ENDS; taken by the two entry points that take a ProjectOptions3"""
    _fields_ = [("base3", ProjectOptions3), ("anchor", c_void_p), ("conf", c_void_p), ("mu", c_float), ("flags", ctypes.c_uint32)]


class ProjectOptions5(ctypes.Structure):
    """pndf_project_options5: the options with a mask, tracks and an observation (`base4`, with base4.base3.base2.base.struct_size = 128)
    and 3D keypoints -- `kp_target` [B,K,3] the detections (None: no keypoint term), `kp_conf` [B,K] (None: ones), `kp_energy` [B] out (or
    None), in the memory space of the poses; `rest` [J,3], `kp_joint` [K] (None: keypoint k is joint k) and `kp_offset` [K,3] (None: zeros)
    in HOST memory; `n_keypoints` K, `nu` the term's weight; taken by the two entry points that take a ProjectOptions4"""
    _fields_ = [("base4", ProjectOptions4), ("kp_target", c_void_p), ("kp_conf", c_void_p), ("kp_energy", c_void_p), ("rest", c_void_p),
                ("kp_joint", c_void_p), ("kp_offset", c_void_p), ("n_keypoints", c_int32), ("nu", c_float)]


class ProjectOptions6(ctypes.Structure):
    """pndf_project_options6: the options with a mask, tracks, an observation and keypoints (`base5`, with
    base5.base4.base3.base2.base.struct_size = 168) and a camera -- `root` [B,7] (quaternion, real part first, then translation; None:
    identity) in the memory space of the poses, read and (with a positive root weight) written by every step; `fx`, `fy`, `cx`, `cy` the
    pinhole intrinsics and `rho` the robustifier of the image residual; `nu_rot`, `nu_trans` the weights of the root's own step;
    `kp_flags` 0 or KP_IMAGE (kp_target is [B,K,2] pixels); taken by the two entry points that take a ProjectOptions5"""
    _fields_ = [("base5", ProjectOptions5), ("root", c_void_p), ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float),
                ("rho", c_float), ("nu_rot", c_float), ("nu_trans", c_float), ("kp_flags", ctypes.c_uint32)]


class ProjectOptions7(ctypes.Structure):
    """pndf_project_options7: the options with a mask, tracks, an observation, keypoints and a camera (`base6`, with
    base6.base5.base4.base3.base2.base.struct_size = 208) and bone lengths -- `bone_scale` [G,S] (S = J + K scales of the rest offsets and
    of the keypoints' offsets; one row per track, or per pose with LEN_PER_POSE or without tracks; None: all ones) in the memory space of
    the poses, read and (with nu_len > 0) written by every step; `len_rate` [S] in HOST memory (None: ones; 0 holds that scale);
    `nu_len` the weight of the scales' step, `kappa` of the prior 1/2 kappa (sigma - 1)^2; `len_min`, `len_max` a clamp (both 0: none);
    `len_flags` 0 or LEN_PER_POSE; taken by the two entry points that take a ProjectOptions6"""
    _fields_ = [("base6", ProjectOptions6), ("bone_scale", c_void_p), ("len_rate", c_void_p), ("nu_len", c_float), ("kappa", c_float),
                ("len_min", c_float), ("len_max", c_float), ("len_flags", ctypes.c_uint32), ("reserved3", ctypes.c_uint32)]


MAX_VIEWS = 8                                              # PNDF_FK_MAX_VIEWS (pndf_project_options8.n_views)


class ProjectOptions8(ctypes.Structure):
    """pndf_project_options8: the options with a mask, tracks, an observation, keypoints, a camera and bone lengths (`base7`, with
    base7.base6.base5.base4.base3.base2.base.struct_size = 224) and several cameras -- `views` [V,16] in HOST memory (per view fx, fy, cx,
    cy, the world -> camera rotation R_v [9] row-major and translation t_v [3]; None: no views), `n_views` V in 0 .. MAX_VIEWS.  With views
    kp_target is [B,V,K,2] pixels and kp_conf [B,V,K], the root places the tree in the world frame and kp_flags must have KP_IMAGE;
    taken by the two entry points that take a ProjectOptions7"""
    _fields_ = [("base7", ProjectOptions7), ("views", c_void_p), ("n_views", c_int32), ("reserved4", ctypes.c_uint32)]


class ProjectOptions9(ctypes.Structure):
    """pndf_project_options9: the options with a mask, tracks, an observation, keypoints, a camera, bone lengths and several cameras
    (`base8`, with base8.base7.base6.base5.base4.base3.base2.base.struct_size = 256) and the root's trajectory -- `root_anchor` [B,7] an
    observed or earlier trajectory of the roots (device memory for the skeleton unit, host memory for the twin; None: none),
    `lambda_rot` / `lambda_trans` the coupling of a frame's root rotation / translation to its neighbour frames' in the track, `mu_rot` /
    `mu_trans` the weights of the data term towards root_anchor, each in [0, 1]; taken by the two entry points that take a ProjectOptions8"""
    _fields_ = [("base8", ProjectOptions8), ("root_anchor", c_void_p), ("lambda_rot", c_float), ("lambda_trans", c_float),
                ("mu_rot", c_float), ("mu_trans", c_float), ("reserved5", ctypes.c_uint64)]


VIEWS_PER_FRAME = 1                                        # PNDF_VIEWS_PER_FRAME (pndf_project_options10.view_flags)


class ProjectOptions10(ctypes.Structure):
    """pndf_project_options10: the options with a mask, tracks, an observation, keypoints, a camera, bone lengths, several cameras and a
    root trajectory (`base9`, with base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = 280) and moving cameras --
    `pose_views` a view table [B,V,16] with one block per pose, or with VIEWS_PER_FRAME in `view_flags` [frames,V,16] with one block per
    frame of a track (device memory for the skeleton unit, host memory for the twin, 16-byte aligned; None: none), `n_pose_views` V in
    0 .. MAX_VIEWS.  A row whose fx or fy is not positive switches its view off for that pose.  With pose_views base9.base8.views is None;
    taken by the two entry points that take a ProjectOptions9"""
    _fields_ = [("base9", ProjectOptions9), ("pose_views", c_void_p), ("n_pose_views", c_int32), ("view_flags", ctypes.c_uint32),
                ("reserved6", ctypes.c_uint64)]


class DenoiseWeights(ctypes.Structure):
    """pndf_denoise_weights: the loss weights of one outer iteration, evaluated"""
    _fields_ = [("prior_coef", c_float), ("prior_power", c_int32), ("temp_coef", c_float), ("data_coef", c_float)]


class Camera(ctypes.Structure):
    """pndf_camera: focal lengths, centre and the fixed rotation Rc (row-major) of the perspective camera"""
    _fields_ = [("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float), ("R", c_float * 9)]


class KeypointOpts(ctypes.Structure):
    """pndf_keypoint_opts: the weights of the keypoint and depth terms, the robustifier's rho, confidence weighting on / off"""
    _fields_ = [("data_coef", c_float), ("rho", c_float), ("depth_coef", c_float), ("depth_target", c_float),
                ("use_conf", c_int32), ("reserved", c_int32)]


class OnlineOpts(ctypes.Structure):
    """pndf_online_opts: the stream (seed, draw), the noise mode and the sigma groups of the online sampler"""
    _fields_ = [("seed", ctypes.c_uint64), ("draw", ctypes.c_uint32), ("noise", c_int32), ("n_sigma", c_int32),
                ("sigma", c_float * 16), ("cum", ctypes.c_uint32 * 16)]


class PndfError(RuntimeError):
    pass


_H = c_void_p                          # every handle type, and every `void* stream`
_P = c_void_p                          # any other address: tensor data (an int from data_ptr(), or None), a callback, an out value
_TENSORS = [POINTER(c_void_p), POINTER(c_int64), c_int]      # tensors, numel, n_tensors (host pointers in state-dict order)
_OPT2 = c_void_p                       # `const pndf_project_options*` where it may point to a ProjectOptions, a ProjectOptions2 .. a ProjectOptions10 (byref of any)
# ---- the header set, stated once: header of include/ -> {name: (restype, argtypes)} in the header's order; the headers in the order
# they were added.  A new header is a file in include/, a table here and its declaration count in tests/test_cabi.py.
DEBUG_HEADER = "posendf_amd_debug.h"      # the one header that lives in libposendf_amd_debug.so; every other one in the product library
HEADERS = {
    "posendf_amd.h": {
        "pndf_default_config": (None, [POINTER(PndfConfig), c_int32, c_float]),
        "pndf_create": (c_int, [POINTER(_H), POINTER(PndfConfig), c_int]),
        "pndf_destroy": (c_int, [_H]),
        "pndf_load_weights": (c_int, [_H] + _TENSORS),
        "pndf_forward": (c_int, [_H, _P, _P, c_int64, _H]),
        "pndf_forward_grad": (c_int, [_H, _P, _P, _P, _P, c_int64, _H]),
        "pndf_project": (c_int, [_H, _P, _P, _P, c_int64, c_int, _H]),
        "pndf_default_project_options": (None, [POINTER(ProjectOptions)]),
        "pndf_project_ex": (c_int, [_H, _P, _P, _P, c_int64, c_int, POINTER(ProjectOptions), _H]),
        # ---- host twins
        "pndf_cpu_create": (c_int, [POINTER(_H), POINTER(PndfConfig)]),
        "pndf_cpu_destroy": (c_int, [_H]),
        "pndf_cpu_load_weights": (c_int, [_H] + _TENSORS),
        "pndf_forward_cpu": (c_int, [_H, _P, _P, c_int64]),
        "pndf_forward_grad_cpu": (c_int, [_H, _P, _P, _P, _P, c_int64]),
        "pndf_project_cpu": (c_int, [_H, _P, _P, _P, c_int64, c_int]),
        "pndf_project_ex_cpu": (c_int, [_H, _P, _P, _P, c_int64, c_int, _OPT2]),
        "pndf_cpu_last_error": (c_char_p, [_H]),
        # host-only weight packer
        "pndf_packed_sizes": (None, [POINTER(c_int64)] * 2),
        "pndf_pack_host": (c_int, _TENSORS + [_P, _P]),
        "pndf_pack_host_split": (c_int, _TENSORS + [_P, _P]),
        # ---- motion-denoise optimiser step
        "pndf_aa2quat": (c_int, [_P, _P, c_int64, _H]),
        "pndf_denoise_update": (c_int, [_P] * 8 + [c_int32] * 4 + [c_float, _H]),
        "pndf_denoise_update_w": (c_int, [_P] * 9 + [c_int32, c_int32, POINTER(DenoiseWeights), c_int32, c_float, _H]),
        "pndf_denoise_update_body": (c_int, [_P] * 9 + [c_int32] * 4 + [c_float, _H]),
        # ---- SMPL-shaped body model
        "pndf_lbs_create": (c_int, [POINTER(_H), c_int32, c_int32] + [_P] * 8 + [c_int32, c_int]),
        "pndf_lbs_destroy": (c_int, [_H]),
        "pndf_lbs_set_precision": (c_int, [_H, c_int32]),
        "pndf_lbs_precision": (c_int32, [_H]),
        "pndf_lbs_num_joints": (c_int32, [_H]),
        "pndf_lbs_num_vertices": (c_int32, [_H]),
        "pndf_lbs_workspace_floats": (c_int64, [_H, c_int32, c_int32]),
        "pndf_lbs_forward": (c_int, [_H, _P, c_int64, _P, _P, _P, _H]),
        "pndf_lbs_terms_grad": (c_int, [_H, _P, _P, c_int32, c_int32, c_int32, _P, _P, _H]),
        "pndf_lbs_terms_grad_w": (c_int, [_H, _P, _P, c_int32, c_int32, c_float, c_float, _P, _P, _H]),
        "pndf_lbs_backward": (c_int, [_H, _P, _P, _P, c_int64, _P, _P, _H]),
        "pndf_lbs_packed_floats": (c_int64, [c_int32]),
        "pndf_lbs_pack_host": (c_int, [c_int32, c_int32] + [_P] * 8 + [c_int32, _P, _P, _P]),
        "pndf_lbs_packed_split_bytes": (c_int64, [c_int32]),
        "pndf_lbs_pack_split_host": (c_int, [c_int32, _P, _P, _P]),
        "pndf_lbs_last_error": (c_char_p, [_H]),
        # ---- the training objective
        "pndf_train_create": (c_int, [POINTER(_H), POINTER(PndfConfig), c_int]),
        "pndf_train_destroy": (c_int, [_H]),
        "pndf_train_workspace_floats": (c_int64, [_H, c_int64, c_int64, c_int32]),
        "pndf_train_forward": (c_int, [_H, _P, _P, _P, _P, c_int64, c_int64, c_int32, c_int32, _P, _P, _H]),
        "pndf_train_backward": (c_int, [_H, _P, _P, _P, _P, _H]),
        "pndf_train_last_error": (c_char_p, [_H]),
        # ---- the rest of a training step
        "pndf_adam_step": (c_int, [_P] * 4 + [c_int64, c_int32] + [c_double] * 5 + [_H]),
        "pndf_train_batch": (c_int, [_P] * 8 + [c_int32] * 6 + [_P] * 3 + [_H]),
        # ---- fitting poses to 2D keypoints
        "pndf_keypoint_terms_grad": (c_int, [_P] * 5 + [c_int64, c_int32, POINTER(Camera), POINTER(KeypointOpts)] + [_P] * 4 + [_H]),
        "pndf_keypoint_project": (c_int, [_P] * 3 + [c_int64, c_int32, POINTER(Camera), _P, _P, _H]),
        # ---- quaternion pose distance + k nearest candidates
        "pndf_quat_topk": (c_int, [_P, _P, c_int64, c_int32, c_int32, _P, c_int32, _P, _P, _H]),
        # ---- exact k-nearest-pose search
        "pndf_knn_create": (c_int, [POINTER(_H), _P, c_int64, c_int32, _P, _H]),
        "pndf_knn_destroy": (c_int, [_H]),
        "pndf_knn_size": (c_int64, [_H]),
        "pndf_knn_workspace_bytes": (c_int64, [_H, c_int64, c_int32]),
        "pndf_knn_search": (c_int, [_H, _P, c_int64, c_int32, _P, _P, _P, _H]),
        "pndf_knn_last_error": (c_char_p, [_H]),

        "pndf_last_error": (c_char_p, [_H]),
        "pndf_version": (c_char_p, []),
        "pndf_experiment_word": (c_uint, []),
        "pndf_kernel_name": (c_char_p, [_H]),
    },
    DEBUG_HEADER: {      # bring-up / profiling / measurement aids, NOT the drop-in boundary
        "pndf_debug_bind": (c_int, [_P, _P, _P]),
        "pndf_debug_experiment_word": (c_uint, []),
        "pndf_debug_forward_grad": (c_int, [_H, _P, _P, _P, c_int64, _P, _H]),
        "pndf_debug_floats": (c_int64, []),
        "pndf_debug_project_timing": (c_int, [_H, _P, _P, c_int64, c_int, _P, _H]),
        "pndf_debug_timing_regions": (c_int, []),
        "pndf_debug_timing_layout": (c_int, [c_int]),
        "pndf_debug_mem_probe": (c_int, [c_int, _P, c_int]),
        "pndf_debug_ring_stream": (c_int, [c_int, c_int, _P]),
        "pndf_debug_lbs_scales": (c_int, [c_int32, _P, _P, _P, c_float, c_float, _P]),
    },
    "posendf_amd_completion.h": {      # pose completion
        "pndf_complete_step": (c_int, [_P, _P, _P, _P, c_int64, POINTER(ProjectOptions), _H]),
        "pndf_complete_workspace_floats": (c_int64, [c_int64]),
        "pndf_complete": (c_int, [_H, _P, _P, _P, _P, c_int64, c_int, POINTER(ProjectOptions), _P, _H]),
        "pndf_complete_cpu": (c_int, [_H, _P, _P, _P, _P, c_int64, c_int, POINTER(ProjectOptions)]),
    },
    "posendf_amd_interpolation.h": {      # pose interpolation
        "pndf_interp_fill": (c_int, [_P, _P, _P, c_int64, c_int32, c_int32, _H]),
        "pndf_interp_band_step": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int32, c_float, POINTER(ProjectOptions), _H]),
        "pndf_interpolate_workspace_floats": (c_int64, [c_int64, c_int32]),
        "pndf_interpolate": (c_int, [_H, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int, c_float, POINTER(ProjectOptions), _P, _H]),
        "pndf_interpolate_cpu": (c_int, [_H, _P, _P, _P, _P, _P, c_int64, c_int32, c_int32, c_int, c_float, POINTER(ProjectOptions)]),
    },
    "posendf_amd_second_order.h": {      # Hessian-vector products of the distance
        "pndf_so_create": (c_int, [POINTER(_H), POINTER(PndfConfig), c_int]),
        "pndf_so_destroy": (c_int, [_H]),
        "pndf_so_last_error": (c_char_p, [_H]),
        "pndf_so_workspace_floats": (c_int64, [_H, c_int64]),
        "pndf_second_order": (c_int, [_H] + [_P] * 9 + [c_int64, _P, c_int64, _H]),
        "pndf_second_order_cpu": (c_int, [_H] + [_P] * 8 + [c_int64]),
    },
    "posendf_amd_online.h": {      # the sampler of online training data
        "pndf_online_default_opts": (c_int, [POINTER(OnlineOpts)]),
        "pndf_online_shares": (c_int, [POINTER(OnlineOpts), POINTER(c_float)]),
        "pndf_online_sample": (c_int, [_P, c_int64, c_int64, c_int64, POINTER(OnlineOpts), _P, _P, _P, _H]),
        "pndf_online_sample_cpu": (c_int, [_P, c_int64, c_int64, c_int64, POINTER(OnlineOpts), _P, _P, _P]),
    },
    "posendf_amd_skeleton.h": {      # distance, gradient and projection for any joint tree
        "pndf_skel_create": (c_int, [POINTER(_H), POINTER(PndfConfig), c_int]),
        "pndf_skel_destroy": (c_int, [_H]),
        "pndf_skel_load_weights": (c_int, [_H] + _TENSORS),
        "pndf_skel_workspace_bytes": (c_int64, [_H, c_int64]),
        "pndf_skel_forward": (c_int, [_H, _P, _P, c_int64, _P, c_int64, _H]),
        "pndf_skel_forward_grad": (c_int, [_H, _P, _P, _P, _P, c_int64, _P, c_int64, _H]),
        "pndf_skel_project": (c_int, [_H, _P, _P, _P, c_int64, c_int, _OPT2, _P, c_int64, _H]),
        "pndf_skel_last_error": (c_char_p, [_H]),
    },
    "posendf_amd_skeleton_train.h": {      # training any joint tree
        "pndf_skel_train_create": (c_int, [POINTER(_H), POINTER(PndfConfig), c_int]),
        "pndf_skel_train_batch": (c_int, [_P] * 8 + [c_int32] * 7 + [_P] * 3 + [_H]),
    },
    "posendf_amd_skeleton_data.h": {      # the k-NN index and the online sampler for any J
        "pndf_skel_knn_create": (c_int, [POINTER(_H), _P, c_int64, c_int32, c_int32, _P, _H]),
        "pndf_skel_online_sample": (c_int, [_P, c_int64, c_int32, c_int64, c_int64, POINTER(OnlineOpts), _P, _P, _P, _H]),
        "pndf_skel_online_sample_cpu": (c_int, [_P, c_int64, c_int32, c_int64, c_int64, POINTER(OnlineOpts), _P, _P, _P]),
    },
}


def exports(header) -> tuple:
    """the names `header` declares, in its order"""
    return tuple(HEADERS[header])


EXPORTS, DEBUG_EXPORTS = exports("posendf_amd.h"), exports(DEBUG_HEADER)
PRODUCT_EXPORTS = tuple(name for header in HEADERS if header != DEBUG_HEADER for name in HEADERS[header])
# per-translation-unit experiment words (csrc/pndf_experiment.h): data symbols, all zero in a product build
EXPERIMENT_WORDS = ("pndf_experiment_word_capi", "pndf_experiment_word_fp32", "pndf_experiment_word_split", "pndf_experiment_word_split_x2",
                    "pndf_experiment_word_bf16", "pndf_experiment_word_lbs", "pndf_experiment_word_generic", "pndf_experiment_word_train",
                    "pndf_experiment_word_optim", "pndf_experiment_word_second_order", "pndf_experiment_word_skeleton")
DEBUG_EXPERIMENT_WORDS = ("pndf_experiment_word_debug", "pndf_experiment_word_fp32_timing", "pndf_experiment_word_split_timing",
                          "pndf_experiment_word_fp32_dbg", "pndf_experiment_word_probe")


def _bind(lib, signatures):
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def debug_library_path(product_path: str) -> str:
    """libposendf_amd.so -> libposendf_amd_debug.so (variant builds: lib_<name>.so -> lib_<name>_debug.so, next to it)"""
    base, ext = os.path.splitext(product_path)
    return base + "_debug" + ext


class _PndfLibrary(ctypes.CDLL):
    """The PRODUCT library.  It exports no `pndf_debug_*` symbol (include/posendf_amd_debug.h lives in libposendf_amd_debug.so);
    asking this object for one loads the debug library that was built next to it -- on first use only, so a process that never
    profiles maps the product library alone --, binds it to this library's `pndf_internal_*` hooks and answers from there."""

    def __getattr__(self, name):
        if name.startswith("pndf_debug_"):
            fn = getattr(self._debug(), name)
            setattr(self, name, fn)
            return fn
        return super().__getattr__(name)

    def _debug(self):
        dbg = self.__dict__.get("_pndf_debug_lib")
        if dbg is None:
            path = debug_library_path(self._name)
            if not os.path.exists(path):
                raise PndfError(f"{path} not found (the debug library is built with the product one: __graft_entry__.build())")
            dbg = _bind(ctypes.CDLL(path), HEADERS[DEBUG_HEADER])
            hooks = [ctypes.cast(ctypes.CDLL.__getattr__(self, n), c_void_p) for n in
                     ("pndf_internal_launch", "pndf_internal_describe", "pndf_internal_fail")]
            if dbg.pndf_debug_bind(*hooks) != 0:
                raise PndfError("pndf_debug_bind failed")
            self.__dict__["_pndf_debug_lib"] = dbg
        return dbg


def load_library(path: str | None = None) -> ctypes.CDLL:
    path = path or os.environ.get("PNDF_LIBRARY") or _LIB_PATH      # PNDF_LIBRARY: A/B runs of two builds on one box
    if not os.path.exists(path):
        raise PndfError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). The engine has no fallback path.")
    lib = _PndfLibrary(path)
    for header, table in HEADERS.items():
        if header != DEBUG_HEADER:      # (the debug table: bound by _PndfLibrary._debug(), on first use)
            _bind(lib, table)
    return lib


def experiment_word(lib=None) -> int:
    """OR of the library's per-translation-unit experiment words, read from the data symbols themselves (not through
    pndf_experiment_word(), which a lab build could have touched): 0 for a product build."""
    lib = lib or load_library()
    w = 0
    for name in EXPERIMENT_WORDS:
        w |= int(ctypes.c_uint.in_dll(lib, name).value)
    dbg = lib._debug() if isinstance(lib, _PndfLibrary) else None      # (the debug library next to it: the same rule)
    for name in (DEBUG_EXPERIMENT_WORDS if dbg is not None else ()):
        w |= int(ctypes.c_uint.in_dll(dbg, name).value)
    return w
