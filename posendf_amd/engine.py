"""ctypes binding of libposendf_amd.so (include/posendf_amd.h).

This module is deliberately thin: tensors are passed as raw device pointers (`tensor.data_ptr()`),
the current HIP stream as an integer handle.  There is NO CPU fallback: if the library is missing the
import of `Engine` fails loudly, and if no gfx950 device is visible `Engine(...)` raises.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int64, c_void_p

import numpy as np

# The boundary itself -- structures, codes, one signature table per header (abi.HEADERS), the loader -- is posendf_amd/abi.py; its
# public names stay importable from here.  `torch` comes from there too: abi imports it before the library is loaded (None without it).
from .abi import (ACT_CODES, DEBUG_EXPERIMENT_WORDS, DEBUG_EXPORTS, EXPERIMENT_WORDS, EXPORTS, INTERP_MODES, METRIC_CODES,  # noqa: F401
                  NOISE_CODES, PRECISION_CODES, RENORM_CODES, Camera, DenoiseWeights, KeypointOpts, OnlineOpts, PndfConfig, PndfError,
                  ProjectOptions, ProjectOptions2, ProjectOptions3, ProjectOptions4, ProjectOptions5, ProjectOptions6, ProjectOptions7, ProjectOptions8, ProjectOptions9, ProjectOptions10, KP_IMAGE, LEN_PER_POSE, MAX_VIEWS, TRACK_FILLS, TRACK_FREE_ENDS, VIEWS_PER_FRAME, debug_library_path, experiment_word, load_library, torch)


def stream_handle(device) -> int:
    """The caller's current HIP stream on `device` (a torch.device) as the integer the C ABI's `void* stream` takes; 0 for a host
    device: the host twins take none, and a caller that launches a kernel refuses a host device itself (`_device_only`)."""
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0


def device_index(device) -> int:
    """the index of a cuda torch.device, the current device's for a bare "cuda": the key of every per-device cache"""
    return device.index if device.index is not None else torch.cuda.current_device()


class StreamWorkspaces:
    """A unit's workspace tensors, one per (device index, stream) and grown on demand: calls on one stream run in order, so they
    may share one.  `dtype` is the unit the entry point counts the workspace in (float32, or uint8 for bytes)."""

    def __init__(self, dtype):
        self.dtype = dtype
        self._tensors = {}

    def get(self, device, n):
        """a tensor of at least `n` elements on `device` (a cuda torch.device) for the caller's current stream"""
        key = (device_index(device), stream_handle(device))
        ws = self._tensors.get(key)
        if ws is None or ws.numel() < n:
            ws = self._tensors[key] = torch.empty(n, device=device, dtype=self.dtype)
        return ws


def _device_only(device, what):
    """the refusal of the entry points that have no host twin: their pointers must be device memory"""
    if device.type != "cuda":
        raise PndfError(f"{what} runs on the HIP kernel only: tensors on {device}")


def state_dict_order(encoder: bool = True, n_lin: int = 7, parents=None):
    """Keys in the order pndf_load_weights expects (== reference state_dict order): the 84 encoder tensors (with the
    structure encoder; without it -- model.StrEnc.use = False, in_dim 84 -- none), then weight and bias of every
    dfnet.lin{l}: 98 / 14 tensors for configs/amass.yaml's seven linear layers.  `parents`: another skeleton's parent table
    (four encoder tensors per joint); None = the SMPL table."""
    from .synth import BONE_DIM, FEAT, PARENT, state_dict_shapes
    parents = PARENT if parents is None else tuple(parents)
    first = len(parents) * (FEAT if encoder else BONE_DIM)
    return list(state_dict_shapes((first,) + (1,) * n_lin, parents=parents).keys())


def _tensor_table(sd_np, parents=None):
    n_lin = sum(1 for k in sd_np if k.startswith("dfnet.lin") and k.endswith(".weight"))
    keys = state_dict_order(encoder=any(k.startswith("enc.") for k in sd_np), n_lin=n_lin, parents=parents)
    arrs = [np.ascontiguousarray(np.asarray(sd_np[k], dtype=np.float32)) for k in keys]
    ptrs = (c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    numel = (c_int64 * len(arrs))(*[a.size for a in arrs])
    return arrs, ptrs, numel


def pack_host(sd_np, lib=None, split=False):
    """Host-only packing (no device): returns (stream[STEP_TILES*256], bias) float32 arrays; split=True gives
    the split-precision stream (trunk tiles = fp16 hi/lo pairs, view them with .view(np.float16))."""
    lib = lib or load_library()
    n = [c_int64(), c_int64()]
    lib.pndf_packed_sizes(*[ctypes.byref(x) for x in n])
    stream = np.empty(n[0].value, np.float32)
    bias = np.empty(n[1].value, np.float32)
    arrs, ptrs, numel = _tensor_table(sd_np)
    fn = lib.pndf_pack_host_split if split else lib.pndf_pack_host
    rc = fn(ptrs, numel, len(arrs), stream.ctypes.data, bias.ctypes.data)
    if rc != 0:
        raise PndfError(f"pndf_pack_host failed ({rc})")
    return stream, bias


def project_options(lib, step_size=1.0, renorm="none", tol=0.0):
    """pndf_project_options for the step options of `project` (include/posendf_amd.h), or None when all three are the defaults
    (the caller then uses the plain entry point).  `renorm`: "none" / None, "unit", "unit_flip".  The values are checked by the
    library (PNDF_ERR_BAD_ARG), only the mode's name here."""
    renorm = "none" if renorm is None else renorm
    if renorm not in RENORM_CODES:
        raise PndfError(f"unknown renormalisation {renorm!r} (None, 'unit', 'unit_flip')")
    if float(step_size) == 1.0 and renorm == "none" and float(tol) == 0.0:
        return None
    opt = ProjectOptions()
    lib.pndf_default_project_options(ctypes.byref(opt))
    opt.step_size, opt.renorm, opt.tol = float(step_size), RENORM_CODES[renorm], float(tol)
    return opt


def _opt_ref(lib, step_size, renorm, tol):
    """the `const pndf_project_options*` argument of the entry points that take null for the defaults"""
    opt = project_options(lib, step_size, renorm, tol)
    return None if opt is None else ctypes.byref(opt)


def project_options2(lib, observed_ptr, step_size=1.0, renorm="none", tol=0.0):
    """pndf_project_options2 (include/posendf_amd.h): the step options and the joint mask at `observed_ptr` -- one uint32 per pose, bit j
    = joint j is held; device memory for pndf_skel_project, host memory for pndf_project_ex_cpu"""
    opt = ProjectOptions2()
    lib.pndf_default_project_options(ctypes.byref(opt.base))
    base = project_options(lib, step_size, renorm, tol)
    if base is not None:
        opt.base = base
    opt.base.struct_size = ctypes.sizeof(opt)
    opt.observed, opt.reserved = observed_ptr, 0
    return opt


def project_options3(lib, observed_ptr, frames, smooth=0.0, fill=None, step_size=1.0, renorm="none", tol=0.0):
    """pndf_project_options3 (include/posendf_amd.h): the options, the mask and the tracks -- the poses are tracks of `frames` frames with the
    end frames held, `smooth` the neighbour coupling lambda, `fill` "given" / None (the poses are the track), "slerp" or "nlerp" (the
    frames between the end frames are interpolated).  The values are checked by the library, only the fill's name here."""
    fill = "given" if fill is None else fill
    if fill not in TRACK_FILLS:
        raise PndfError(f"unknown track fill {fill!r} (None / 'given', 'slerp', 'nlerp')")
    opt = ProjectOptions3()
    opt.base2 = project_options2(lib, observed_ptr, step_size, renorm, tol)
    opt.base2.base.struct_size = ctypes.sizeof(opt)
    opt.frames, opt.lambda_, opt.fill, opt.reserved2 = int(frames), float(smooth), TRACK_FILLS[fill], 0
    return opt


def project_options4(lib, observed_ptr, frames, smooth=0.0, fill=None, anchor_ptr=None, conf_ptr=None, data=0.0, free_ends=False,
                     step_size=1.0, renorm="none", tol=0.0):
    """pndf_project_options4 (include/posendf_amd.h): the options, the mask, the tracks and the observation of motion denoising --
    `anchor_ptr` [B,J,4] the noisy poses (None: no data term), `conf_ptr` [B,J] per-joint confidences (None: ones), `data` the data term's
    weight mu, `free_ends`: the end frames of a track are not held.  The values are checked by the library."""
    opt = ProjectOptions4()
    opt.base3 = project_options3(lib, observed_ptr, frames, smooth, fill, step_size, renorm, tol)
    opt.base3.base2.base.struct_size = ctypes.sizeof(opt)
    opt.anchor, opt.conf, opt.mu, opt.flags = anchor_ptr, conf_ptr, float(data), TRACK_FREE_ENDS if free_ends else 0
    return opt


def project_options5(lib, observed_ptr, frames, smooth=0.0, fill=None, anchor_ptr=None, conf_ptr=None, data=0.0, free_ends=False,
                     kp_target_ptr=None, kp_conf_ptr=None, kp_energy_ptr=None, rest_ptr=None, kp_joint_ptr=None, kp_offset_ptr=None,
                     n_keypoints=0, kp_weight=0.0, step_size=1.0, renorm="none", tol=0.0):
    """pndf_project_options5 (include/posendf_amd.h): the options, the mask, the tracks, the observation and the 3D keypoints of a fit --
    `kp_target_ptr` [B,K,3] (None: no keypoint term), `kp_conf_ptr` [B,K] (None: ones) and `kp_energy_ptr` [B] (out, or None) in the memory
    space of the poses; `rest_ptr` [J,3], `kp_joint_ptr` [K] int32 (None: keypoint k is joint k) and `kp_offset_ptr` [K,3] (None: zeros) in
    HOST memory; `n_keypoints` K and `kp_weight` the term's weight nu.  The values are checked by the library."""
    opt = ProjectOptions5()
    opt.base4 = project_options4(lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, step_size, renorm, tol)
    opt.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    opt.kp_target, opt.kp_conf, opt.kp_energy = kp_target_ptr, kp_conf_ptr, kp_energy_ptr
    opt.rest, opt.kp_joint, opt.kp_offset = rest_ptr, kp_joint_ptr, kp_offset_ptr
    opt.n_keypoints, opt.nu = int(n_keypoints), float(kp_weight)
    return opt


def project_options6(lib, *args, root_ptr=None, root_weights=(0.0, 0.0), camera=None, rho=0.0, image=None, **kw):
    """pndf_project_options6 (include/posendf_amd.h): `project_options5`'s arguments, and the camera and the root of a fit to 2D keypoints --
    `root_ptr` [B,7] (quaternion, real part first, then translation; None: identity) in the memory space of the poses, read and, with a
    positive weight, written by every step; `root_weights` (nu_rot, nu_trans); `camera` (fx, fy, cx, cy); `rho` the robustifier; `image`:
    whether kp_target is [B,K,2] pixels (PNDF_KP_IMAGE; None: whenever a camera is given).  The values are checked by the library."""
    opt = ProjectOptions6()
    opt.base5 = project_options5(lib, *args, **kw)
    opt.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    opt.root = root_ptr
    if camera is not None:
        opt.fx, opt.fy, opt.cx, opt.cy = (float(v) for v in camera)
    opt.rho = float(rho)
    opt.nu_rot, opt.nu_trans = (float(v) for v in root_weights)
    opt.kp_flags = KP_IMAGE if (camera is not None if image is None else image) else 0
    return opt


def project_options7(lib, *args, bone_scale_ptr=None, len_rate=None, len_weight=0.0, len_prior=0.0, len_range=None, per_pose_lengths=False, **kw):
    """pndf_project_options7 (include/posendf_amd.h): `project_options6`'s arguments, and the bone lengths of a fit -- `bone_scale_ptr` [G,S]
    (S = J + K; one row per track, or per pose with `per_pose_lengths` or without tracks; None: all ones) in the memory space of the poses,
    read and, with a positive `len_weight` (nu_len), written by every step; `len_rate`: S floats (a sequence; None: ones; 0 holds that
    scale), kept alive on the returned struct; `len_prior` kappa; `len_range` (len_min, len_max) or None.  The values are checked by the
    library."""
    opt = ProjectOptions7()
    opt.base6 = project_options6(lib, *args, **kw)
    opt.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    opt.bone_scale = bone_scale_ptr
    if len_rate is not None:
        rates = [float(v) for v in len_rate]
        opt._rates = (ctypes.c_float * max(len(rates), 1))(*rates)      # host memory that lives as long as the struct
        opt.len_rate = ctypes.cast(opt._rates, ctypes.c_void_p).value
    opt.nu_len, opt.kappa = float(len_weight), float(len_prior)
    if len_range is not None:
        opt.len_min, opt.len_max = (float(v) for v in len_range)
    opt.len_flags = LEN_PER_POSE if per_pose_lengths else 0
    return opt


def view_table(views):
    """The [V,16] float32 table of a pndf_project_options8 (per view fx, fy, cx, cy, R row-major, t) as a C-contiguous numpy array, from
    such an array (or tensor) or from a sequence of (K [3,3] or (fx, fy, cx, cy), R [3,3], t [3]).  The values are checked by the library."""
    if torch is not None and isinstance(views, torch.Tensor):
        views = views.detach().cpu().numpy()
    if isinstance(views, np.ndarray) and views.ndim == 2:
        if views.shape[1] != 16:
            raise PndfError(f"views is [V,16], not {list(views.shape)}")
        return np.ascontiguousarray(views, dtype=np.float32)
    rows = []
    for view in views:
        if len(view) != 3:
            raise PndfError("a view is (K [3,3] or (fx, fy, cx, cy), R [3,3], t [3])")
        K, R, t = (np.asarray(v.detach().cpu() if torch is not None and isinstance(v, torch.Tensor) else v, dtype=np.float64) for v in view)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        if K.shape != (4,) or R.shape != (3, 3) or t.shape != (3,):
            raise PndfError(f"a view is (K [3,3] or (fx, fy, cx, cy), R [3,3], t [3]), not {K.shape}, {R.shape}, {t.shape}")
        rows.append(np.concatenate([K, R.reshape(9), t]))
    return np.ascontiguousarray(np.stack(rows) if rows else np.zeros((0, 16)), dtype=np.float32)


def project_options8(lib, *args, views=None, **kw):
    """pndf_project_options8 (include/posendf_amd.h): `project_options7`'s arguments, and the cameras of a fit to pixels seen by several
    views -- `views`: what `view_table` takes (HOST memory, kept alive on the returned struct; None: no views).  With views kp_target_ptr is
    [B,V,K,2], kp_conf_ptr [B,V,K], and the image flag is set (the `camera` of project_options6 is not read).  The values are checked by
    the library."""
    opt = ProjectOptions8()
    if views is not None and kw.get("image") is None:
        kw = dict(kw, image=True)
    opt._base7 = project_options7(lib, *args, **kw)      # (kept: it owns the rates that the copy below points to)
    opt.base7 = opt._base7
    opt.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    if views is not None:
        opt._views = view_table(views)      # host memory that lives as long as the struct
        opt.views = opt._views.ctypes.data if opt._views.size else None
        opt.n_views = int(opt._views.shape[0])
    return opt


def project_options9(lib, *args, root_smooth=None, root_anchor_ptr=None, root_data=None, **kw):
    """pndf_project_options9 (include/posendf_amd.h): `project_options8`'s arguments, and the root's trajectory over the frames of a track --
    `root_smooth` = (lambda_rot, lambda_trans): the coupling of a frame's root to its neighbour frames'; `root_anchor_ptr`: an observed or
    earlier trajectory [B,7] (device memory for the skeleton unit, host memory for the twin); `root_data` = (mu_rot, mu_trans): the weights
    of the data term towards it.  The values are checked by the library."""
    opt = ProjectOptions9()
    opt._base8 = project_options8(lib, *args, **kw)      # (kept: it owns the view table that the copy below points to)
    opt.base8 = opt._base8
    opt.base8.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    opt.root_anchor = root_anchor_ptr
    opt.lambda_rot, opt.lambda_trans = (float(v) for v in (root_smooth or (0.0, 0.0)))
    opt.mu_rot, opt.mu_trans = (float(v) for v in (root_data or (0.0, 0.0)))
    return opt


def project_options10(lib, *args, pose_views=None, views_per_frame=False, **kw):
    """pndf_project_options10 (include/posendf_amd.h): `project_options9`'s arguments, and moving cameras -- `pose_views`: a contiguous
    float32 view table [B,V,16] with one block per pose, or with `views_per_frame` [frames,V,16] with one block per frame of a track, as
    a tensor in device memory for the skeleton unit or a tensor / numpy array in host memory for the twin; 16-byte aligned.  The returned
    struct keeps the table alive.  With it kp_target_ptr is [B,V,K,2], kp_conf_ptr [B,V,K], the image flag is set and `views` stays None.
    The shape is checked here, the rest by the library -- which cannot see the values of a table in device memory: a row whose fx or fy
    is not positive switches its view off for that pose."""
    opt = ProjectOptions10()
    if pose_views is not None and kw.get("image") is None:
        kw = dict(kw, image=True)
    opt._base9 = project_options9(lib, *args, **kw)      # (kept: it owns what the copy below points to)
    opt.base9 = opt._base9
    opt.base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = ctypes.sizeof(opt)
    if pose_views is not None:
        table = pose_views
        is_tensor = torch is not None and isinstance(table, torch.Tensor)
        if not is_tensor:
            table = np.ascontiguousarray(table, dtype=np.float32)
        elif table.dtype != torch.float32 or not table.is_contiguous():
            raise PndfError(f"pose_views is a contiguous float32 tensor, not {table.dtype} with strides {tuple(table.stride())}")
        if table.ndim != 3 or table.shape[2] != 16:
            raise PndfError(f"pose_views is [B,V,16] or [frames,V,16], not {list(table.shape)}")
        opt._pose_views = table      # the table lives as long as the struct
        filled = table.numel() if is_tensor else table.size
        opt.pose_views = (table.data_ptr() if is_tensor else table.ctypes.data) if filled else None
        opt.n_pose_views = int(table.shape[1]) if filled else 0
        opt.view_flags = VIEWS_PER_FRAME if views_per_frame and filled else 0
    return opt


_ROOT_TRACK_KEYS = ("root_smooth", "root_anchor_ptr", "root_data")


def _root_tracked(kw):
    """(the root-trajectory keywords of a `project` call, the rest): only when one of them says something is the 256-byte struct built"""
    mine = {k: kw[k] for k in _ROOT_TRACK_KEYS if k in kw}
    rest = {k: v for k, v in kw.items() if k not in _ROOT_TRACK_KEYS}
    named = (mine.get("root_anchor_ptr") is not None or any(float(v) != 0.0 for v in (mine.get("root_smooth") or ()))
             or any(float(v) != 0.0 for v in (mine.get("root_data") or ())))
    return (mine if named else None), rest


_LENGTH_KEYS = ("bone_scale_ptr", "len_rate", "len_weight", "len_prior", "len_range", "per_pose_lengths")


def _lengthed(kw):
    """(the bone-length keywords of a `project` call, the rest): only when one of them is given is the 208-byte struct built"""
    mine = {k: kw[k] for k in _LENGTH_KEYS if k in kw}
    rest = {k: v for k, v in kw.items() if k not in _LENGTH_KEYS}
    named = (mine.get("bone_scale_ptr") is not None or mine.get("len_rate") is not None or mine.get("len_range") is not None
             or bool(mine.get("per_pose_lengths")) or float(mine.get("len_weight") or 0.0) != 0.0 or float(mine.get("len_prior") or 0.0) != 0.0)
    return (mine if named else None), rest


_IMAGE_KEYS = ("root_ptr", "root_weights", "camera", "rho", "image")


def _imaged(kw):
    """(the camera / root keywords of a `project` call, the rest): only when one of them says something is the 168-byte struct built"""
    mine = {k: kw[k] for k in _IMAGE_KEYS if k in kw}
    rest = {k: v for k, v in kw.items() if k not in _IMAGE_KEYS}
    named = (mine.get("root_ptr") is not None or mine.get("camera") is not None or bool(mine.get("image")) or float(mine.get("rho") or 0.0) != 0.0
             or any(float(v) != 0.0 for v in (mine.get("root_weights") or ())))
    return (mine if named else None), rest


_KEYPOINT_KEYS = ("kp_target_ptr", "kp_conf_ptr", "kp_energy_ptr", "rest_ptr", "kp_joint_ptr", "kp_offset_ptr", "n_keypoints", "kp_weight")


def _keypointed(kw) -> bool:
    """whether a `project` call names keypoints at all: only then is the 128-byte struct built"""
    unknown = sorted(set(kw) - set(_KEYPOINT_KEYS))
    if unknown:
        raise TypeError(f"project() got unexpected keyword arguments {unknown}")
    return any(kw.get(k) is not None for k in _KEYPOINT_KEYS[:6]) or bool(kw.get("n_keypoints")) or float(kw.get("kp_weight") or 0.0) != 0.0


def _anchored(anchor_ptr, conf_ptr, data, free_ends) -> bool:
    """whether a `project` call names an observation or free end frames at all: only then is the 72-byte struct built"""
    return anchor_ptr is not None or conf_ptr is not None or float(data) != 0.0 or bool(free_ends)


def _tracked(frames, smooth, fill) -> bool:
    """whether a `project` call names tracks at all: only then is the 48-byte struct built"""
    return bool(frames) or float(smooth) != 0.0 or fill not in (None, "given")


def interp_mode(mode) -> int:
    """PNDF_INTERP_* of a fill mode's name"""
    if mode not in INTERP_MODES:
        raise PndfError(f"unknown interpolation mode {mode!r} ('slerp', 'nlerp')")
    return INTERP_MODES[mode]


def _set_encoder_act(cfg, act, beta, enc_act, enc_beta):
    """model.StrEnc.act / beta when they differ from model.DFNet's (reference net_modules.py:128 reads its own keys; every config
    of the reference sets them equal): a mixed pair runs on the runtime-planned kernels."""
    if enc_act is not None and enc_act not in ACT_CODES:
        raise PndfError(f"unknown encoder activation {enc_act!r}")
    if enc_act is not None and (enc_act != act or (enc_act == "softplus" and enc_beta is not None and float(enc_beta) != float(beta))):
        cfg.enc_act = ACT_CODES[enc_act]
        cfg.enc_beta = float(enc_beta if enc_beta is not None else beta)


def _network_config(lib, act, beta, *, precision=None, encoder=True, hidden=None, enc_act=None, enc_beta=None, parents=None) -> PndfConfig:
    """The pndf_config of a network: configs/amass.yaml's architecture (pndf_default_config) with the activation pair, the trunk's
    arithmetic, the encoder-less input and model.DFNet.dims of the caller.  `parents`: the parent table of another skeleton (1 .. 32
    joints, -1 = a root; pndf_skel_create and the first-order host twins take it, the values are checked by the library); None = SMPL."""
    if act not in ACT_CODES:
        raise PndfError(f"unknown activation {act!r}")
    if precision is not None and precision not in PRECISION_CODES:
        raise PndfError(f"unknown precision {precision!r} (fp32, f16x3, f16, bf16)")
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), ACT_CODES[act], float(beta))
    if precision is not None:
        cfg.precision = PRECISION_CODES[precision]
    _set_encoder_act(cfg, act, beta, enc_act, enc_beta)
    if parents is not None:
        parents = [int(p) for p in parents]
        if len(parents) > len(cfg.parent):
            raise PndfError(f"a skeleton of {len(parents)} joints: pndf_config.parent holds {len(cfg.parent)}")
        cfg.num_joints = len(parents)
        for j in range(len(cfg.parent)):
            cfg.parent[j] = parents[j] if j < len(parents) else 0
        cfg.dims[0] = 6 * len(parents)
    if not encoder:
        cfg.dims[0] = 4 * cfg.num_joints      # model.StrEnc.use = False: DFNet on the J x 4 normalised quaternions (84 for SMPL)
    if hidden is not None:
        # model.DFNet.dims (reference net_modules.py:14-28: a free list).  Six hidden widths within configs/amass.yaml's run on
        # the fused kernels (narrower ones zero padded); any other list of 1 .. 7 widths up to 1024 on the runtime-planned
        # kernels (csrc/pndf_generic.hip: exact fp32, or split-precision fp16 MFMAs for f16x3 / f16); pndf_create refuses the rest
        hidden = [int(w) for w in hidden]
        if not 1 <= len(hidden) <= 7:
            raise PndfError(f"DFNet with {len(hidden)} hidden layers: 1 .. 7 are implemented")
        cfg.n_dims = len(hidden) + 2
        for i in range(1, len(cfg.dims)):
            cfg.dims[i] = 0
        for i, w in enumerate(hidden):
            cfg.dims[i + 1] = w
        cfg.dims[len(hidden) + 1] = 1
    return cfg


class _Handle:
    """The life cycle of one C-ABI handle.  A subclass names its handle type's destroy and last-error functions and sets `lib`
    before it calls `_create`; compute methods call the bound function themselves and pass its status to `_check`."""
    _destroy = _last_error = None
    handle = None

    def _create(self, fn, *args):
        """self.handle = the handle that `fn(&handle, *args)` makes"""
        self.handle = c_void_p()
        rc = getattr(self.lib, fn)(ctypes.byref(self.handle), *args)
        if rc != 0:
            msg = getattr(self.lib, self._last_error)(None).decode()
            self.handle = None
            raise PndfError(f"{fn} failed ({rc}): {msg}")

    def _check(self, rc, what):
        if rc != 0:
            raise PndfError(f"{what} failed ({rc}): {getattr(self.lib, self._last_error)(self.handle).decode()}")

    def close(self):
        if self.handle:
            getattr(self.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One engine per device.  All compute methods take raw device pointers and a stream handle."""
    _destroy, _last_error = "pndf_destroy", "pndf_last_error"

    def __init__(self, act: str = "lrelu", beta: float = 100.0, device: int = 0, lib=None, precision: str = "fp32",
                 encoder: bool = True, hidden=None, enc_act: str | None = None, enc_beta: float | None = None):
        self.lib = lib or load_library()
        cfg = _network_config(self.lib, act, beta, precision=precision, encoder=encoder, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta)
        self.precision = precision
        self._create("pndf_create", ctypes.byref(cfg), int(device))
        self.device = device
        self.act = act

    def load_weights(self, sd_np):
        arrs, ptrs, numel = _tensor_table(sd_np)
        self._check(self.lib.pndf_load_weights(self.handle, ptrs, numel, len(arrs)), "pndf_load_weights")

    def kernel_name(self) -> str:
        """the device kernel this engine's compute calls launch (after load_weights)"""
        return self.lib.pndf_kernel_name(self.handle).decode()

    def forward(self, q_ptr, d_ptr, B, stream=0):
        self._check(self.lib.pndf_forward(self.handle, q_ptr, d_ptr, B, stream), "pndf_forward")

    def forward_grad(self, q_ptr, gout_ptr, d_ptr, dq_ptr, B, stream=0):
        self._check(self.lib.pndf_forward_grad(self.handle, q_ptr, gout_ptr, d_ptr, dq_ptr, B, stream),
                    "pndf_forward_grad")

    def project(self, q_in_ptr, q_out_ptr, d_ptr, B, steps, stream=0, *, step_size=1.0, renorm="none", tol=0.0):
        """pndf_project; with a step option that differs from its default, pndf_project_ex (include/posendf_amd.h)"""
        opt = project_options(self.lib, step_size, renorm, tol)
        if opt is None:
            self._check(self.lib.pndf_project(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), stream),
                        "pndf_project")
        else:
            self._check(self.lib.pndf_project_ex(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt), stream),
                        "pndf_project_ex")

    def complete_workspace_floats(self, B) -> int:
        n = int(self.lib.pndf_complete_workspace_floats(int(B)))
        if n < 0:
            raise PndfError(f"pndf_complete_workspace_floats failed ({n}): B = {B}")
        return n

    def complete(self, q_in_ptr, observed_ptr, q_out_ptr, d_ptr, B, steps, ws_ptr, stream=0, *, step_size=1.0, renorm="none", tol=0.0):
        """pndf_complete (include/posendf_amd_completion.h): the projection loop with the joints of `observed_ptr` (one uint32 per
        pose, bit j = joint j; None = no joint) held; `ws_ptr`: complete_workspace_floats(B) floats of device memory"""
        self._check(self.lib.pndf_complete(self.handle, q_in_ptr, observed_ptr, q_out_ptr, d_ptr, B, int(steps),
                                           _opt_ref(self.lib, step_size, renorm, tol), ws_ptr, stream), "pndf_complete")

    def complete_step(self, q_ptr, d_ptr, dq_ptr, observed_ptr, B, stream=0, *, step_size=1.0, renorm="none", tol=0.0):
        """pndf_complete_step: one masked step on q in place from the d and dq of a forward_grad (a stateless helper: no text)"""
        rc = self.lib.pndf_complete_step(q_ptr, d_ptr, dq_ptr, observed_ptr, B, _opt_ref(self.lib, step_size, renorm, tol), stream)
        if rc != 0:
            raise PndfError(f"pndf_complete_step failed ({rc}): B = {B}; q and dq must be non-null and 16-byte aligned, d non-null, "
                            "the options those of pndf_project_ex")

    def interpolate_workspace(self, P, T) -> int:
        n = int(self.lib.pndf_interpolate_workspace_floats(int(P), int(T)))
        if n < 0:
            raise PndfError(f"pndf_interpolate_workspace_floats failed ({n}): P = {P}, T = {T}")
        return n

    def interpolate(self, a_ptr, b_ptr, observed_ptr, track_ptr, d_ptr, P, T, steps, ws_ptr, stream=0, *, mode="slerp", smooth=0.0,
                    step_size=1.0, renorm="none", tol=0.0):
        """pndf_interpolate (include/posendf_amd_interpolation.h): the track [P,T,21,4] between the pairs a, b [P,21,4] -- the fill
        in `mode`, then `steps` band steps with the neighbour coupling `smooth` (lambda); `observed_ptr`: one uint32 per pose of the
        track or None; `ws_ptr`: interpolate_workspace(P, T) floats of device memory"""
        opt = _opt_ref(self.lib, step_size, renorm, tol)      # (refuses an unknown `renorm` before an unknown `mode`)
        self._check(self.lib.pndf_interpolate(self.handle, a_ptr, b_ptr, observed_ptr, track_ptr, d_ptr, int(P), int(T), interp_mode(mode),
                                              int(steps), float(smooth), opt, ws_ptr, stream),
                    "pndf_interpolate")

    def interp_fill(self, a_ptr, b_ptr, track_ptr, P, T, stream=0, *, mode="slerp"):
        """pndf_interp_fill: the filled track alone (a stateless helper: no text)"""
        rc = self.lib.pndf_interp_fill(a_ptr, b_ptr, track_ptr, int(P), int(T), interp_mode(mode), stream)
        if rc != 0:
            raise PndfError(f"pndf_interp_fill failed ({rc}): P = {P}, T = {T}; a, b and the track must be non-null and 16-byte aligned, T >= 2")

    def interp_band_step(self, q_in_ptr, q_out_ptr, d_ptr, dq_ptr, observed_ptr, P, T, stream=0, *, smooth=0.0, step_size=1.0, renorm="none",
                         tol=0.0):
        """pndf_interp_band_step: one out-of-place band step from the d and dq of a forward_grad (a stateless helper: no text)"""
        rc = self.lib.pndf_interp_band_step(q_in_ptr, q_out_ptr, d_ptr, dq_ptr, observed_ptr, int(P), int(T), float(smooth),
                                            _opt_ref(self.lib, step_size, renorm, tol), stream)
        if rc != 0:
            raise PndfError(f"pndf_interp_band_step failed ({rc}): P = {P}, T = {T}, lambda = {smooth}; q_in, q_out and dq must be non-null, "
                            "distinct and 16-byte aligned, d non-null, lambda in [0, 1], the options those of pndf_project_ex")

    def debug_forward_grad(self, q_ptr, d_ptr, dq_ptr, B, dump_ptr, stream=0):
        self._check(self.lib.pndf_debug_forward_grad(self.handle, q_ptr, d_ptr, dq_ptr, B, dump_ptr, stream),
                    "pndf_debug_forward_grad")

    def debug_floats(self):
        return int(self.lib.pndf_debug_floats())

    REGION_NAMES = ("enc fwd + x0", "P1 lin0,lin1", "act x2", "P2 lin2,lin3", "act x4", "P3 lin4,lin5", "act x6+lin6+g6",
                    "P4 lin5T,lin4T +dact", "P5 lin3T,lin2T +dact", "P6 lin1T,lin0T", "enc bwd", "norm bwd+update+sync")

    def project_timing(self, q, steps=3, out=None):
        """pndf_debug_project_timing on a CUDA tensor of poses: the instrumented kernel's per-region shader cycles of one
        step (mean over waves), the effective shader clock, and the weight ring's sampled events -- how long a wave sits in
        the ring's counted wait (the slot's DMA had not landed) and in its barrier, per slot."""
        _device_only(q.device, "pndf_debug_project_timing")
        B = int(q.shape[0])
        R = int(self.lib.pndf_debug_timing_regions())
        nreg, ngrp, nring, period, slots = (int(self.lib.pndf_debug_timing_layout(i)) for i in range(5))
        cyc = torch.zeros((-(-B // 64)) * 4 * R, dtype=torch.int64, device=q.device)
        out = torch.empty_like(q) if out is None else out
        st = stream_handle(q.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._check(self.lib.pndf_debug_project_timing(self.handle, q.data_ptr(), out.data_ptr(), B, int(steps), cyc.data_ptr(), st),
                    "pndf_debug_project_timing")
        e1.record()
        torch.cuda.synchronize(q.device)
        ms = e0.elapsed_time(e1)
        rows = cyc.cpu().numpy().reshape(-1, R).astype(np.float64)
        reg = rows[:, :nreg].copy()
        reg[:, 3] += rows[:, nreg:nreg + ngrp].sum(1)       # per-group stamps (if built in) take their time out of region 3
        per_step = reg.mean(0) / steps
        ring = rows[:, nreg + ngrp:nreg + ngrp + nring]
        n = max(ring[:, 2].sum(), 1.0)
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        rounds = -(-(-(-B // 64)) // cus)
        total = float(per_step.sum())
        return {"steps": int(steps), "launch_ms": ms, "workgroup_rounds": rounds,
                "cycles_per_wave_step": total,
                "effective_sclk_ghz": reg.sum(1).mean() * rounds / (ms * 1e-3) / 1e9,
                "regions": {name: float(c) for name, c in zip(self.REGION_NAMES, per_step)},
                "ring": {"look_ahead_slots": slots - 1, "sampled_every": period, "sampled_slots_per_wave": float(ring[:, 2].mean()),
                         "wait_cycles_per_slot": float(ring[:, 0].sum() / n), "barrier_cycles_per_slot": float(ring[:, 1].sum() / n),
                         "stamp_floor_cycles": float(ring[:, 3].mean()),
                         "wait_cycles_per_slot_p99_wave": float(np.percentile(ring[:, 0] / np.maximum(ring[:, 2], 1), 99))},
                "spread_over_waves": [float(reg.sum(1).min() / steps), float(reg.sum(1).max() / steps)]}


class TrainEngine(_Handle):
    """`pndf_train_*` (csrc/pndf_train.hip): the training objective of model/posendf.py:62-99 and its weight gradients on one
    device.  Exact fp32 MFMA; the structure encoder is required (the reference cannot train without it).  `parents`: the parent
    table of another skeleton (1 .. 32 joints), planned by pndf_skel_train_create of include/posendf_amd_skeleton_train.h; None =
    the SMPL table through pndf_train_create.  All compute methods take raw device pointers (the weights and gradients as lists
    of them, state-dict order; poses [B, num_joints, 4]) and a stream handle."""
    _destroy, _last_error = "pndf_train_destroy", "pndf_train_last_error"

    def __init__(self, act: str = "lrelu", beta: float = 100.0, device: int = 0, lib=None, encoder: bool = True, hidden=None,
                 enc_act: str | None = None, enc_beta: float | None = None, parents=None):
        self.lib = lib or load_library()
        cfg = _network_config(self.lib, act, beta, encoder=encoder, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta, parents=parents)
        self.parents = None if parents is None else tuple(int(p) for p in parents)
        self.num_joints = int(cfg.num_joints)
        self.n_tensors = len(state_dict_order(encoder, cfg.n_dims - 1, parents=self.parents))
        self._create("pndf_train_create" if parents is None else "pndf_skel_train_create", ctypes.byref(cfg), int(device))
        self.device = device
        self.act = act

    def _table(self, ptrs):
        if isinstance(ptrs, ctypes.Array):      # a table the caller built once (posendf_amd.trainer: one per trainer, not per step)
            return ptrs
        if len(ptrs) != self.n_tensors:
            raise PndfError(f"{len(ptrs)} tensors given, the network has {self.n_tensors}")
        return (c_void_p * len(ptrs))(*ptrs)

    def workspace_floats(self, B, Bm, eikonal) -> int:
        n = int(self.lib.pndf_train_workspace_floats(self.handle, int(B), int(Bm), int(bool(eikonal))))
        if n < 0:
            raise PndfError(f"pndf_train_workspace_floats failed ({n})")
        return n

    def forward(self, weight_ptrs, q_ptr, gt_ptr, qm_ptr, B, Bm, loss_type, eikonal, losses_ptr, ws_ptr, stream=0):
        self._check(self.lib.pndf_train_forward(self.handle, self._table(weight_ptrs), q_ptr, gt_ptr, qm_ptr, int(B), int(Bm),
                                                int(loss_type), int(bool(eikonal)), losses_ptr, ws_ptr, stream),
                    "pndf_train_forward")

    def backward(self, weight_ptrs, upstream_ptr, grad_ptrs, ws_ptr, stream=0):
        self._check(self.lib.pndf_train_backward(self.handle, self._table(weight_ptrs), upstream_ptr, self._table(grad_ptrs), ws_ptr,
                                                 stream), "pndf_train_backward")


class SecondOrderEngine(_Handle):
    """`pndf_so_*` / `pndf_second_order` (csrc/pndf_second_order.hip): d, grad_q d, <v, grad_q d> and w_d grad_q d + w_t H v on one
    device, the weights read in place.  Exact fp32 MFMA; the structure encoder is required.  Raw device pointers (the weights as
    a list of them, state-dict order) and a stream handle."""
    _destroy, _last_error = "pndf_so_destroy", "pndf_so_last_error"

    def __init__(self, act: str = "lrelu", beta: float = 100.0, device: int = 0, lib=None, encoder: bool = True, hidden=None,
                 enc_act: str | None = None, enc_beta: float | None = None):
        self.lib = lib or load_library()
        cfg = _network_config(self.lib, act, beta, encoder=encoder, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta)
        self.n_tensors = len(state_dict_order(encoder, cfg.n_dims - 1))
        self._create("pndf_so_create", ctypes.byref(cfg), int(device))
        self.device = device
        self.act = act

    def workspace_floats(self, B) -> int:
        n = int(self.lib.pndf_so_workspace_floats(self.handle, int(B)))
        if n < 0:
            raise PndfError(f"pndf_so_workspace_floats failed ({n}): B = {B}")
        return n

    def second_order(self, weight_ptrs, q_ptr, v_ptr, wd_ptr, wt_ptr, d_ptr, g_ptr, t_ptr, out_ptr, B, ws_ptr, ws_floats, stream=0):
        """every output pointer, wd_ptr (0) and wt_ptr (1) may be None"""
        if not isinstance(weight_ptrs, ctypes.Array):
            if len(weight_ptrs) != self.n_tensors:
                raise PndfError(f"{len(weight_ptrs)} tensors given, the network has {self.n_tensors}")
            weight_ptrs = (c_void_p * len(weight_ptrs))(*weight_ptrs)
        self._check(self.lib.pndf_second_order(self.handle, weight_ptrs, q_ptr, v_ptr, wd_ptr, wt_ptr, d_ptr, g_ptr, t_ptr, out_ptr, int(B),
                                               ws_ptr, int(ws_floats), stream), "pndf_second_order")


class SkeletonEngine(_Handle):
    """`pndf_skel_*` (csrc/pndf_skeleton.hip): distance, gradient and projection for the joint tree `parents` (1 .. 32 joints, -1 = a
    root, every parent before its child; None = SMPL) on one device, layer by layer in exact fp32.  Raw device pointers, a workspace
    of `workspace_bytes(B)` bytes from the caller and a stream handle."""
    _destroy, _last_error = "pndf_skel_destroy", "pndf_skel_last_error"

    def __init__(self, parents=None, act: str = "lrelu", beta: float = 100.0, device: int = 0, lib=None, encoder: bool = True, hidden=None,
                 enc_act: str | None = None, enc_beta: float | None = None):
        self.lib = lib or load_library()
        cfg = _network_config(self.lib, act, beta, encoder=encoder, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta, parents=parents)
        self.parents = None if parents is None else tuple(int(p) for p in parents)
        self.num_joints = int(cfg.num_joints)
        self.precision = "fp32"
        self._create("pndf_skel_create", ctypes.byref(cfg), int(device))
        self.device = device
        self.act = act

    def load_weights(self, sd_np):
        arrs, ptrs, numel = _tensor_table(sd_np, self.parents)
        self._check(self.lib.pndf_skel_load_weights(self.handle, ptrs, numel, len(arrs)), "pndf_skel_load_weights")

    def kernel_name(self) -> str:
        return "pndf_skel_enc_fwd_kernel"

    def workspace_bytes(self, B) -> int:
        n = int(self.lib.pndf_skel_workspace_bytes(self.handle, int(B)))
        if n < 0:
            raise PndfError(f"pndf_skel_workspace_bytes failed ({n}): B = {B}")
        return n

    def forward(self, q_ptr, d_ptr, B, ws_ptr, ws_bytes, stream=0):
        self._check(self.lib.pndf_skel_forward(self.handle, q_ptr, d_ptr, int(B), ws_ptr, int(ws_bytes), stream), "pndf_skel_forward")

    def forward_grad(self, q_ptr, gout_ptr, d_ptr, dq_ptr, B, ws_ptr, ws_bytes, stream=0):
        """gout_ptr None = ones; d_ptr may be None"""
        self._check(self.lib.pndf_skel_forward_grad(self.handle, q_ptr, gout_ptr, d_ptr, dq_ptr, int(B), ws_ptr, int(ws_bytes), stream),
                    "pndf_skel_forward_grad")

    def project(self, q_in_ptr, q_out_ptr, d_ptr, B, steps, ws_ptr, ws_bytes, stream=0, *, step_size=1.0, renorm="none", tol=0.0,
                observed_ptr=None, frames=0, smooth=0.0, fill=None, anchor_ptr=None, conf_ptr=None, data=0.0, free_ends=False, **keypoints):
        """pndf_skel_project; `observed_ptr`: one uint32 per pose in device memory, bit j = joint j is held (pose completion, through a
        pndf_project_options2); None: no joint is held and the call is the one without a mask.  `frames` = T >= 2: the poses are B / T
        tracks (pose interpolation, through a pndf_project_options3: `project_options3`), q_out apart from q_in.  `anchor_ptr` [B,J,4] /
        `conf_ptr` [B,J] in device memory, `data` and `free_ends`: the observation of motion denoising (through a
        pndf_project_options4: `project_options4`), apart from q_out.  `**keypoints`: kp_target_ptr [B,K,3] / kp_conf_ptr [B,K] / kp_energy_ptr
        [B] in device memory, rest_ptr / kp_joint_ptr / kp_offset_ptr in HOST memory, n_keypoints, kp_weight: the 3D keypoints of a fit
        (through a pndf_project_options5: `project_options5`); root_ptr [B,7] in device memory, root_weights, camera, rho, image: the root and
        the camera of a fit to 2D keypoints (through a pndf_project_options6: `project_options6`); bone_scale_ptr [G,S] in device memory,
        len_rate, len_weight, len_prior, len_range, per_pose_lengths: the bone lengths of a fit (through a pndf_project_options7:
        `project_options7`); views: the cameras of a fit to pixels seen by several views, kp_target_ptr then [B,V,K,2] and kp_conf_ptr
        [B,V,K] (through a pndf_project_options8: `project_options8`, built only when views are given); root_smooth, root_anchor_ptr
        [B,7] in device memory, root_data: the root's trajectory over the frames of a track (through a pndf_project_options9:
        `project_options9`, built only when one of them says something); pose_views [B,V,16] or, with views_per_frame, [frames,V,16]: a
        tensor in device memory, the cameras of a fit to pixels seen by moving views (through a pndf_project_options10:
        `project_options10`, built only when pose_views is given)"""
        views = keypoints.pop("views", None)
        pose_views, views_per_frame = keypoints.pop("pose_views", None), keypoints.pop("views_per_frame", False)
        rooted, keypoints = _root_tracked(keypoints)
        lengthed, keypoints = _lengthed(keypoints)
        imaged, keypoints = _imaged(keypoints)
        named = _keypointed(keypoints)      # (refuses an unknown keyword)
        if pose_views is not None:
            opt10 = project_options10(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                      step_size=step_size, renorm=renorm, tol=tol, pose_views=pose_views, views_per_frame=views_per_frame,
                                      **keypoints, **(imaged or {}), **(lengthed or {}), **(rooted or {}))
            opt = ctypes.byref(opt10)
        elif rooted is not None:
            opt9 = project_options9(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **(lengthed or {}), **rooted)
            opt = ctypes.byref(opt9)
        elif views is not None:
            opt8 = project_options8(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **(lengthed or {}))
            opt = ctypes.byref(opt8)
        elif lengthed is not None:
            opt7 = project_options7(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **lengthed)
            opt = ctypes.byref(opt7)
        elif imaged is not None:
            opt = ctypes.byref(project_options6(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                                step_size=step_size, renorm=renorm, tol=tol, **keypoints, **imaged))
        elif named:
            opt = ctypes.byref(project_options5(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                                step_size=step_size, renorm=renorm, tol=tol, **keypoints))
        elif _anchored(anchor_ptr, conf_ptr, data, free_ends):
            opt = ctypes.byref(project_options4(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, step_size, renorm, tol))
        elif _tracked(frames, smooth, fill):
            opt = ctypes.byref(project_options3(self.lib, observed_ptr, frames, smooth, fill, step_size, renorm, tol))
        elif observed_ptr is None:
            opt = _opt_ref(self.lib, step_size, renorm, tol)
        else:
            opt = ctypes.byref(project_options2(self.lib, observed_ptr, step_size, renorm, tol))
        self._check(self.lib.pndf_skel_project(self.handle, q_in_ptr, q_out_ptr, d_ptr, int(B), int(steps), opt, ws_ptr, int(ws_bytes), stream),
                    "pndf_skel_project")


def adam_step(p_ptr, g_ptr, m_ptr, v_ptr, n, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, stream=0, lib=None):
    """`pndf_adam_step` (csrc/pndf_optim.hip): one torch.optim.Adam step over flat fp32 device buffers of n floats"""
    rc = (lib or load_library()).pndf_adam_step(p_ptr, g_ptr, m_ptr, v_ptr, int(n), int(step), float(lr), float(beta1), float(beta2),
                                                float(eps), float(weight_decay), stream)
    if rc != 0:
        raise PndfError(f"pndf_adam_step failed ({rc}): n = {n}, step = {step}; the four buffers must be non-null and 16-byte aligned")


def train_batch(pose_db_ptr, dist_db_ptr, man_db_ptr, file_off_ptr, man_off_ptr, item_file_ptr, item_man_file_ptr, words_ptr, F, Fm, k,
                items, num_pts, flip, q_ptr, gt_ptr, qm_ptr, stream=0, lib=None):
    """`pndf_train_batch` (csrc/pndf_optim.hip): one training batch gathered from a device-resident data set"""
    rc = (lib or load_library()).pndf_train_batch(pose_db_ptr, dist_db_ptr, man_db_ptr, file_off_ptr, man_off_ptr, item_file_ptr,
                                                  item_man_file_ptr, words_ptr, int(F), int(Fm), int(k), int(items), int(num_pts),
                                                  int(bool(flip)), q_ptr, gt_ptr, qm_ptr, stream)
    if rc != 0:
        raise PndfError(f"pndf_train_batch failed ({rc}): F = {F}, Fm = {Fm}, k = {k}, items = {items}, num_pts = {num_pts}")


def skel_train_batch(pose_db_ptr, dist_db_ptr, man_db_ptr, file_off_ptr, man_off_ptr, item_file_ptr, item_man_file_ptr, words_ptr, F, Fm, k,
                     items, num_pts, flip, num_joints, q_ptr, gt_ptr, qm_ptr, stream=0, lib=None):
    """`pndf_skel_train_batch` (csrc/pndf_optim.hip): `train_batch` for poses of `num_joints` joints"""
    rc = (lib or load_library()).pndf_skel_train_batch(pose_db_ptr, dist_db_ptr, man_db_ptr, file_off_ptr, man_off_ptr, item_file_ptr,
                                                       item_man_file_ptr, words_ptr, int(F), int(Fm), int(k), int(items), int(num_pts),
                                                       int(bool(flip)), int(num_joints), q_ptr, gt_ptr, qm_ptr, stream)
    if rc != 0:
        raise PndfError(f"pndf_skel_train_batch failed ({rc}): F = {F}, Fm = {Fm}, k = {k}, items = {items}, num_pts = {num_pts}, "
                        f"num_joints = {num_joints}")


def online_opts(sigmas, shares, noise="uniform", seed=0, draw=0, lib=None) -> OnlineOpts:
    """pndf_online_opts of one pool: `sigmas` and `shares` of equal length 1 .. 16, thresholds by pndf_online_shares"""
    lib = lib or load_library()
    if noise not in NOISE_CODES:
        raise PndfError(f"unknown noise {noise!r} ('uniform', 'symmetric')")
    sigmas, shares = [float(s) for s in sigmas], [float(s) for s in shares]
    if len(sigmas) != len(shares) or not 1 <= len(sigmas) <= 16:
        raise PndfError(f"{len(sigmas)} sigmas and {len(shares)} shares: 1 .. 16 of each, one share per sigma")
    opt = OnlineOpts()
    opt.seed, opt.draw, opt.noise, opt.n_sigma = int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff, NOISE_CODES[noise], len(sigmas)
    for g, s in enumerate(sigmas):
        opt.sigma[g] = s
    rc = lib.pndf_online_shares(ctypes.byref(opt), (c_float * len(shares))(*shares))
    if rc != 0:
        raise PndfError(f"pndf_online_shares failed ({rc}): {lib.pndf_cpu_last_error(None).decode()}")
    return opt


def online_sample(man_ptr, N, first, count, opt, q_ptr, src_ptr=None, group_ptr=None, stream=0, lib=None, num_joints=21):
    """`pndf_online_sample` (csrc/pndf_online.hip): poses first .. first + count - 1 of the pool of `opt` over the device manifold;
    another `num_joints` than 21: `pndf_skel_online_sample`"""
    lib = lib or load_library()
    if int(num_joints) == 21:
        fn, rc = "pndf_online_sample", lib.pndf_online_sample(man_ptr, int(N), int(first), int(count), ctypes.byref(opt), q_ptr, src_ptr, group_ptr, stream)
    else:
        fn, rc = "pndf_skel_online_sample", lib.pndf_skel_online_sample(man_ptr, int(N), int(num_joints), int(first), int(count), ctypes.byref(opt),
                                                                        q_ptr, src_ptr, group_ptr, stream)
    if rc != 0:
        raise PndfError(f"{fn} failed ({rc}): {lib.pndf_last_error(None).decode()}")


def online_sample_cpu(man_ptr, N, first, count, opt, q_ptr, src_ptr=None, group_ptr=None, lib=None, num_joints=21):
    """`pndf_online_sample_cpu` (csrc/pndf_cpu.cpp): the host twin of online_sample, HOST pointers"""
    lib = lib or load_library()
    if int(num_joints) == 21:
        fn, rc = "pndf_online_sample_cpu", lib.pndf_online_sample_cpu(man_ptr, int(N), int(first), int(count), ctypes.byref(opt), q_ptr, src_ptr, group_ptr)
    else:
        fn, rc = "pndf_skel_online_sample_cpu", lib.pndf_skel_online_sample_cpu(man_ptr, int(N), int(num_joints), int(first), int(count),
                                                                                ctypes.byref(opt), q_ptr, src_ptr, group_ptr)
    if rc != 0:
        raise PndfError(f"{fn} failed ({rc}): {lib.pndf_cpu_last_error(None).decode()}")


def aa2quat(theta_ptr, q_ptr, N, stream=0, lib=None):
    """`pndf_aa2quat` (csrc/pndf_denoise.hip): device theta [N,69] axis-angle -> q [N,21,4] quaternions of the first 21 joints"""
    rc = (lib or load_library()).pndf_aa2quat(theta_ptr, q_ptr, int(N), stream)
    if rc != 0:
        raise PndfError(f"pndf_aa2quat failed ({rc}): N = {N}")


def denoise_update_w(theta_in_ptr, theta_out_ptr, theta0_ptr, d_ptr, dq_ptr, g_body_ptr, m_ptr, v_ptr, q_next_ptr, S, T, weights, step, lr,
                     stream=0, lib=None):
    """`pndf_denoise_update_w` (csrc/pndf_denoise.hip): one Adam step of the motion-denoise objective with the explicit loss
    weights `weights` (a DenoiseWeights); g_body_ptr None selects the pose-space surrogates"""
    rc = (lib or load_library()).pndf_denoise_update_w(theta_in_ptr, theta_out_ptr, theta0_ptr, d_ptr, dq_ptr, g_body_ptr, m_ptr, v_ptr,
                                                       q_next_ptr, int(S), int(T), ctypes.byref(weights), int(step), float(lr), stream)
    if rc != 0:
        raise PndfError(f"pndf_denoise_update_w failed ({rc}): S = {S}, T = {T}, step = {step}, prior_power = {weights.prior_power}")


def keypoint_terms_grad(joints_ptr, orient_ptr, transl_ptr, keypoints_ptr, joint_weight_ptr, N, J, cam, opt, terms_ptr, g_joints_ptr,
                        g_orient_ptr, g_transl_ptr, stream=0, lib=None):
    """`pndf_keypoint_terms_grad` (csrc/pndf_keypoints.hip): the keypoint and depth terms of N frames of J joints and their
    gradients; `cam` a Camera, `opt` a KeypointOpts; every output pointer may be None"""
    rc = (lib or load_library()).pndf_keypoint_terms_grad(joints_ptr, orient_ptr, transl_ptr, keypoints_ptr, joint_weight_ptr, int(N), int(J),
                                                          ctypes.byref(cam), ctypes.byref(opt), terms_ptr, g_joints_ptr, g_orient_ptr,
                                                          g_transl_ptr, stream)
    if rc != 0:
        raise PndfError(f"pndf_keypoint_terms_grad failed ({rc}): N = {N}, J = {J}, rho = {opt.rho}")


def keypoint_project(joints_ptr, orient_ptr, transl_ptr, N, J, cam, posed_ptr, uv_ptr, stream=0, lib=None):
    """`pndf_keypoint_project` (csrc/pndf_keypoints.hip): camera-space points [N,J,3] and / or image points [N,J,2]"""
    rc = (lib or load_library()).pndf_keypoint_project(joints_ptr, orient_ptr, transl_ptr, int(N), int(J), ctypes.byref(cam), posed_ptr,
                                                       uv_ptr, stream)
    if rc != 0:
        raise PndfError(f"pndf_keypoint_project failed ({rc}): N = {N}, J = {J}")


def quat_topk(noise_ptr, valid_ptr, B, K, metric, weights, k, vals_ptr, idx_ptr, stream=0, lib=None):
    """`pndf_quat_topk` (csrc/pndf_quatdist.hip): the k nearest of every pose's K candidates; `weights` 21 host floats or None"""
    rc = (lib or load_library()).pndf_quat_topk(noise_ptr, valid_ptr, int(B), int(K), int(metric), weights, int(k), vals_ptr, idx_ptr, stream)
    if rc != 0:
        raise PndfError(f"pndf_quat_topk failed ({rc}): B={B} K={K} k={k} (k <= min(K, 16), K <= ~1850)")


class KnnIndex(_Handle):
    """`pndf_knn_*` (csrc/pndf_knn.hip): an exact k-nearest-pose index on one device.  The constructor packs a copy of the
    poses at `poses_ptr` (device [N,J,4], J = `num_joints`; another J than 21: `pndf_skel_knn_create`); `search` takes raw device
    pointers and a stream handle."""
    _destroy, _last_error = "pndf_knn_destroy", "pndf_knn_last_error"

    def __init__(self, poses_ptr, N, metric: str = "geo", weights=None, stream=0, lib=None, num_joints=21):
        self.lib = lib or load_library()
        if metric not in METRIC_CODES:
            raise PndfError(f"unknown metric {metric!r} (geo, euc)")
        J = int(num_joints)
        if not 1 <= J <= 32:
            raise PndfError(f"num_joints = {J}: the index takes 1 .. 32 joints")
        w = None
        if weights is not None:
            w = (c_float * J)(*[float(x) for x in np.asarray(weights, dtype=np.float32).reshape(J)])
        if J == 21:
            self._create("pndf_knn_create", poses_ptr, int(N), METRIC_CODES[metric], w, stream)
        else:
            self._create("pndf_skel_knn_create", poses_ptr, int(N), J, METRIC_CODES[metric], w, stream)
        self.metric, self.num_joints = metric, J

    def size(self) -> int:
        return int(self.lib.pndf_knn_size(self.handle))

    def workspace_bytes(self, Q, k) -> int:
        n = int(self.lib.pndf_knn_workspace_bytes(self.handle, int(Q), int(k)))
        if n < 0:
            raise PndfError(f"pndf_knn_workspace_bytes failed ({n}): Q = {Q}, k = {k}, N = {self.size()}")
        return n

    def search(self, q_ptr, Q, k, vals_ptr, idx_ptr, ws_ptr, stream=0):
        self._check(self.lib.pndf_knn_search(self.handle, q_ptr, int(Q), int(k), vals_ptr, idx_ptr, ws_ptr, stream),
                    "pndf_knn_search")


class CpuEngine(_Handle):
    """The host twins `pndf_*_cpu` behind the interface of `Engine` (raw HOST pointers; `stream` is accepted and ignored):
    what `PoseNDF` runs on when its config says `train.device: cpu`, as the reference's class does (model/posendf.py:35,64).
    Plain C++ on the host cores -- not the oracle, and never a fallback of the device engine."""
    _destroy, _last_error = "pndf_cpu_destroy", "pndf_cpu_last_error"

    def __init__(self, act: str = "lrelu", beta: float = 100.0, lib=None, encoder: bool = True, hidden=None,
                 enc_act: str | None = None, enc_beta: float | None = None, parents=None):
        self.lib = lib or load_library()
        cfg = _network_config(self.lib, act, beta, encoder=encoder, hidden=hidden, enc_act=enc_act, enc_beta=enc_beta, parents=parents)
        self.precision = "fp32"
        self.parents = None if parents is None else tuple(int(p) for p in parents)      # another skeleton: the first-order calls only
        self._create("pndf_cpu_create", ctypes.byref(cfg))
        self.device = "cpu"
        self.act = act

    def load_weights(self, sd_np):
        arrs, ptrs, numel = _tensor_table(sd_np, self.parents)
        self._check(self.lib.pndf_cpu_load_weights(self.handle, ptrs, numel, len(arrs)), "pndf_cpu_load_weights")

    def kernel_name(self) -> str:
        return "pndf_cpu (host twin)"

    def forward(self, q_ptr, d_ptr, B, stream=0):
        self._check(self.lib.pndf_forward_cpu(self.handle, q_ptr, d_ptr, B), "pndf_forward_cpu")

    def forward_grad(self, q_ptr, gout_ptr, d_ptr, dq_ptr, B, stream=0):
        self._check(self.lib.pndf_forward_grad_cpu(self.handle, q_ptr, gout_ptr, d_ptr, dq_ptr, B), "pndf_forward_grad_cpu")

    def project(self, q_in_ptr, q_out_ptr, d_ptr, B, steps, stream=0, *, step_size=1.0, renorm="none", tol=0.0, observed_ptr=None,
                frames=0, smooth=0.0, fill=None, anchor_ptr=None, conf_ptr=None, data=0.0, free_ends=False, **keypoints):
        """`observed_ptr`: one uint32 per pose in host memory, bit j = joint j is held (pndf_project_ex_cpu with a pndf_project_options2:
        any joint tree); None: the call without a mask.  `frames` = T >= 2: the poses are B / T tracks (pndf_project_ex_cpu with a
        pndf_project_options3: `project_options3`).  `anchor_ptr` [B,J,4] / `conf_ptr` [B,J] in host memory, `data` and `free_ends`: the
        observation of motion denoising (pndf_project_ex_cpu with a pndf_project_options4: `project_options4`).  `**keypoints`: as
        SkeletonEngine.project, every pointer in host memory (pndf_project_ex_cpu with a pndf_project_options5: `project_options5`, or with
        root_ptr / root_weights / camera / rho / image a pndf_project_options6: `project_options6`, or with bone_scale_ptr / len_rate /
        len_weight / len_prior / len_range / per_pose_lengths a pndf_project_options7: `project_options7`, or with views a
        pndf_project_options8: `project_options8`, or with root_smooth / root_anchor_ptr / root_data a pndf_project_options9:
        `project_options9`, or with pose_views / views_per_frame a pndf_project_options10: `project_options10`)"""
        views = keypoints.pop("views", None)
        pose_views, views_per_frame = keypoints.pop("pose_views", None), keypoints.pop("views_per_frame", False)
        rooted, keypoints = _root_tracked(keypoints)
        lengthed, keypoints = _lengthed(keypoints)
        imaged, keypoints = _imaged(keypoints)
        named = _keypointed(keypoints)      # (refuses an unknown keyword)
        if pose_views is not None:
            opt10 = project_options10(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                      step_size=step_size, renorm=renorm, tol=tol, pose_views=pose_views, views_per_frame=views_per_frame,
                                      **keypoints, **(imaged or {}), **(lengthed or {}), **(rooted or {}))
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt10)),
                        "pndf_project_ex_cpu")
            return
        if rooted is not None:
            opt9 = project_options9(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **(lengthed or {}), **rooted)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt9)),
                        "pndf_project_ex_cpu")
            return
        if views is not None:
            opt8 = project_options8(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, views=views,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **(lengthed or {}))
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt8)),
                        "pndf_project_ex_cpu")
            return
        if lengthed is not None:
            opt7 = project_options7(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **(imaged or {}), **lengthed)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt7)),
                        "pndf_project_ex_cpu")
            return
        if imaged is not None:
            opt6 = project_options6(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints, **imaged)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt6)),
                        "pndf_project_ex_cpu")
            return
        if named:
            opt5 = project_options5(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends,
                                    step_size=step_size, renorm=renorm, tol=tol, **keypoints)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt5)),
                        "pndf_project_ex_cpu")
            return
        if _anchored(anchor_ptr, conf_ptr, data, free_ends):
            opt4 = project_options4(self.lib, observed_ptr, frames, smooth, fill, anchor_ptr, conf_ptr, data, free_ends, step_size, renorm, tol)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt4)),
                        "pndf_project_ex_cpu")
            return
        if _tracked(frames, smooth, fill):
            opt3 = project_options3(self.lib, observed_ptr, frames, smooth, fill, step_size, renorm, tol)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt3)),
                        "pndf_project_ex_cpu")
            return
        if observed_ptr is not None:
            opt2 = project_options2(self.lib, observed_ptr, step_size, renorm, tol)
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt2)),
                        "pndf_project_ex_cpu")
            return
        opt = project_options(self.lib, step_size, renorm, tol)
        if opt is None:
            self._check(self.lib.pndf_project_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps)), "pndf_project_cpu")
        else:
            self._check(self.lib.pndf_project_ex_cpu(self.handle, q_in_ptr, q_out_ptr, d_ptr, B, int(steps), ctypes.byref(opt)),
                        "pndf_project_ex_cpu")

    def complete_workspace_floats(self, B) -> int:
        return 0      # the host twin needs none

    def complete(self, q_in_ptr, observed_ptr, q_out_ptr, d_ptr, B, steps, ws_ptr=None, stream=0, *, step_size=1.0, renorm="none", tol=0.0):
        self._check(self.lib.pndf_complete_cpu(self.handle, q_in_ptr, observed_ptr, q_out_ptr, d_ptr, B, int(steps),
                                               _opt_ref(self.lib, step_size, renorm, tol)), "pndf_complete_cpu")

    def interpolate_workspace(self, P, T) -> int:
        return 0      # the host twin needs none

    def interpolate(self, a_ptr, b_ptr, observed_ptr, track_ptr, d_ptr, P, T, steps, ws_ptr=None, stream=0, *, mode="slerp", smooth=0.0,
                    step_size=1.0, renorm="none", tol=0.0):
        opt = _opt_ref(self.lib, step_size, renorm, tol)
        self._check(self.lib.pndf_interpolate_cpu(self.handle, a_ptr, b_ptr, observed_ptr, track_ptr, d_ptr, int(P), int(T), interp_mode(mode),
                                                  int(steps), float(smooth), opt), "pndf_interpolate_cpu")

    def second_order(self, q_ptr, v_ptr, wd_ptr, wt_ptr, d_ptr, g_ptr, t_ptr, out_ptr, B):
        """pndf_second_order_cpu (include/posendf_amd_second_order.h) with the weights of load_weights; outputs, wd_ptr (0) and wt_ptr
        (1) may be None"""
        self._check(self.lib.pndf_second_order_cpu(self.handle, q_ptr, v_ptr, wd_ptr, wt_ptr, d_ptr, g_ptr, t_ptr, out_ptr, int(B)),
                    "pndf_second_order_cpu")
