"""`BodyModel` -- the SMPL body model behind the interface of the reference's wrapper (reference
experiments/body_model.py:11-53: `BodyModel(bm_path, num_betas, batch_size, model_type='smpl')`, `forward(root_orient=None,
pose_body=None, betas=None)` returning an object with `.vertices`, `.Jtr`, `.faces`, `.body_pose`, `.betas`), running on
the HIP linear-blend-skinning kernels of posendf_amd/csrc/pndf_lbs.hip through the C ABI (include/posendf_amd.h,
`pndf_lbs_*`).

The reference builds `smplx.SMPL(bm_path)` from the licensed SMPL model file.  Neither smplx nor the file is reachable
here, so the model PARAMETERS are supplied by the caller as arrays with the shapes of the SMPL file (the constructor
takes the dict, `from_arrays` keyword arguments, `from_npz` a converted model file); the algorithm is smplx's published lbs() restated -- parity unpinned.

`precision` selects the arithmetic of the forward and fused-terms passes: "f16x3" (default; fp16 MFMAs on operands split
into hi + lo halves, fp32 accumulate: the distance engine's split arithmetic, fp32-class accuracy) or "fp32" (fp32 MFMAs);
the general reverse pass behind autograd always runs on fp32.  "f16x3" scales its operands by powers of two chosen from
a-priori bounds of the model and the term weights (csrc/pndf_lbs_scales.h); they are tested for SMPL-like models whose
length unit is anything from kilometres to millimetres (template x 1e-3 .. 1e3, tests/test_lbs_range*.py).  Rotation and
translation entries of the joint transforms share one scale, so a model far outside that range (extent below ~1e-2 or above
~1e4 length units) should use "fp32".

`forward` is differentiable with respect to `pose_body` (first order, through `pndf_lbs_backward`); the betas and the global
orientation are constants, as in the reference's optimisation (motion_denoise.py:27,67; root_orient=None).  There is no CPU
or eager fallback: without the library or a gfx950 device the constructor raises.

The C ABI takes its scratch from the caller; this class keeps ONE workspace per device and re-uses it for every call, so
calls of one instance must be ordered on the device (one stream, or events) -- use one `BodyModel` per concurrently used
stream, as with the softplus engine.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .engine import PndfError, _Handle, load_library, stream_handle

_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


class _Lbs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose_body, owner):
        th = pose_body.detach().reshape(-1, 69)
        if th.dtype != torch.float32 or not th.is_contiguous():
            th = th.float().contiguous()
        N = th.shape[0]
        verts = torch.empty(N, owner.num_vertices, 3, device=th.device, dtype=torch.float32)
        joints = torch.empty(N, owner.num_joints, 3, device=th.device, dtype=torch.float32)
        owner._call("pndf_lbs_forward", th.data_ptr(), N, verts.data_ptr(), joints.data_ptr(), owner._workspace(1, N, th.device),
                    owner._stream(th.device))
        ctx.owner = owner
        ctx.save_for_backward(th)
        ctx.in_shape, ctx.in_dtype = pose_body.shape, pose_body.dtype
        return verts, joints

    @staticmethod
    @once_differentiable
    def backward(ctx, g_verts, g_joints):
        (th,) = ctx.saved_tensors
        owner, N = ctx.owner, th.shape[0]
        gv = None if g_verts is None else g_verts.float().contiguous()
        gj = None if g_joints is None else g_joints.float().contiguous()
        g = torch.empty_like(th)
        owner._call("pndf_lbs_backward", th.data_ptr(), None if gv is None else gv.data_ptr(),
                    None if gj is None else gj.data_ptr(), N, g.data_ptr(), owner._workspace(1, N, th.device),
                    owner._stream(th.device))
        return g.reshape(ctx.in_shape).to(ctx.in_dtype), None


class BodyModel(_Handle, torch.nn.Module):
    _destroy, _last_error = "pndf_lbs_destroy", "pndf_lbs_last_error"
    PRECISIONS = {"fp32": 0, "f16x3": 1}      # PNDF_LBS_FP32 / PNDF_LBS_F16X3 (include/posendf_amd.h)

    def __init__(self, params, num_betas=10, batch_size=1, model_type="smpl", device="cuda:0", betas=None,
                 extra_joint_vertex=None, faces=None, precision="f16x3"):
        super().__init__()
        if model_type != "smpl":
            raise PndfError("only model_type='smpl' (24 joints, 23 x 9 pose feature) is implemented")
        self.model_type = model_type
        self.num_joints_smpl = 23                                    # SMPL.NUM_JOINTS (body_model.py:30)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PndfError("BodyModel runs on the HIP kernels only; no CPU path exists")
        self.device = torch.device("cuda", self.device.index or 0)      # indexed: compared with tensor.device below
        missing = [k for k in _KEYS if k not in params]
        if missing:
            raise PndfError(f"body-model parameters lack {missing}")
        if precision not in self.PRECISIONS:      # (before anything is created: nothing to leak on a bad value)
            raise PndfError(f"precision must be one of {sorted(self.PRECISIONS)}")
        vt = _f32(params["v_template"])
        V = vt.shape[0]
        sd = _f32(params["shapedirs"])[:, :, :num_betas]
        nb = sd.shape[2]
        if betas is None:                         # the model file's own betas, as the oracle's rest_shape() uses them
            betas = params.get("betas")
        b = np.zeros(nb, np.float32)
        if betas is not None:
            given = _f32(betas).reshape(-1)[:nb]  # shorter than nb: the remaining shape coefficients are zero
            b[:len(given)] = given
        pd = _f32(params["posedirs"])
        if pd.shape != (207, V * 3):
            raise PndfError(f"posedirs must be [207, {V * 3}] (smplx layout), got {pd.shape}")
        jr, w = _f32(params["J_regressor"]), _f32(params["lbs_weights"])
        par = np.array(params["parents"], dtype=np.int32)      # a copy: the caller's table keeps its root entry
        par[0] = -1
        if extra_joint_vertex is None:      # smplx's SMPL always appends its 21 vertex-picked joints (45 in all)
            from .synth import SMPL_EXTRA_JOINT_VERTICES, SMPL_V
            extra_joint_vertex = params.get("extra_joint_vertex", SMPL_EXTRA_JOINT_VERTICES if V == SMPL_V else ())
        ex = np.ascontiguousarray(np.asarray(extra_joint_vertex, dtype=np.int32))
        if jr.shape != (24, V) or w.shape != (V, 24) or par.shape != (24,):
            raise PndfError("J_regressor [24,V], lbs_weights [V,24], parents [24] expected")
        self.lib = load_library()
        sd_c = np.ascontiguousarray(sd)
        self._create("pndf_lbs_create", V, nb, vt.ctypes.data, sd_c.ctypes.data, b.ctypes.data, pd.ctypes.data, jr.ctypes.data,
                     par.ctypes.data, w.ctypes.data, ex.ctypes.data, len(ex), self.device.index or 0)
        self._call("pndf_lbs_set_precision", self.PRECISIONS[precision])
        self.precision = precision
        self.num_vertices = V
        self.num_joints = 24 + len(ex)
        self.faces_tensor = None if faces is None else torch.as_tensor(np.asarray(faces, dtype=np.int64), device=self.device)
        self.register_buffer("betas", torch.from_numpy(b.copy()).to(self.device))
        self._ws = {}
        self._betas_ok = None

    @classmethod
    def from_npz(cls, path, **kw):
        """A converted SMPL model file: an .npz holding v_template, shapedirs, posedirs [207, 3V], J_regressor (dense),
        parents (kintree_table[0]), lbs_weights (`weights` of the SMPL pickle) and optionally f (faces)."""
        z = dict(np.load(path))
        if "weights" in z and "lbs_weights" not in z:
            z["lbs_weights"] = z["weights"]
        kw.setdefault("faces", z.get("f"))
        return cls(z, **kw)

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, **kw):
        """The six arrays of an SMPL model file by name (shapes as in smplx: [V,3], [V,3,NB], [207,3V], [24,V], [24], [V,24])."""
        return cls(dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor,
                        parents=parents, lbs_weights=lbs_weights), **kw)

    # ---- plumbing -------------------------------------------------------------------------------
    _stream = staticmethod(stream_handle)

    def _workspace(self, S, T, device):
        """scratch of the C ABI calls (caller-owned there): one cached buffer per shape class, grown on demand"""
        need = max(int(self.lib.pndf_lbs_workspace_floats(self.handle, S, T)),
                   int(self.lib.pndf_lbs_workspace_floats(self.handle, 1, S * T)))
        buf = self._ws.get(device)
        if buf is None or buf.numel() < need:
            buf = self._ws[device] = torch.empty(need, device=device, dtype=torch.float32)
        return buf.data_ptr()

    def _device_f32(self, t, what, coerce=True):
        """The C ABI takes raw pointers: float32, contiguous, on this model's device.  Inputs are coerced (a copy when
        needed); an output buffer must already be right, a copy would swallow the result."""
        ok = t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device
        if ok:
            return t
        if not coerce:
            raise PndfError(f"{what} must be a contiguous float32 tensor on {self.device}, got {t.dtype} "
                            f"{'contiguous' if t.is_contiguous() else 'strided'} on {t.device}")
        return t.detach().to(self.device, torch.float32).contiguous()

    def _call(self, name, *args):
        self._check(getattr(self.lib, name)(self.handle, *args), name)

    # ---- reference API (body_model.py:33-52) -----------------------------------------------------
    def forward(self, root_orient=None, pose_body=None, betas=None, return_dict=False, **kwargs):
        if root_orient is not None:
            raise PndfError("root_orient is SMPL's zero global_orient parameter here (the reference passes None)")
        if betas is not None and self.betas.numel() > 0:
            # the reference passes the same (zero) betas tensor every step (motion_denoise.py:27,86): compared once per
            # tensor version, not once per call -- the comparison is a host sync
            # (the tensor OBJECT is part of the key, held weakly: the caching allocator hands a freed tensor's address to the
            # next tensor of the same size, whose version counter also starts at 0)
            seen = self._betas_ok
            if not (seen is not None and seen[0]() is betas and seen[1] == betas._version):
                if torch.count_nonzero(betas.detach().to(self.betas.device).reshape(-1, self.betas.numel()) - self.betas):
                    raise PndfError("betas are fixed at construction (motion_denoise.py:27,67: zeros, requires_grad False)")
                import weakref
                self._betas_ok = (weakref.ref(betas), betas._version)
        pose_body = pose_body.to(self.device)
        verts, joints = _Lbs.apply(pose_body, self)
        # smplx hands back the caller's own tensor: the reference feeds `smpl_init.body_pose` into the next step (:86), and a
        # fresh view per step would chain one ViewBackward node per step onto the leaf
        body_pose = pose_body if (pose_body.dim() == 2 and pose_body.shape[1] == 69) else pose_body.reshape(-1, 69)
        out = {"vertices": verts, "faces": self.faces_tensor, "betas": self.betas, "Jtr": joints,
               "body_pose": body_pose, "full_pose": None}
        return out if return_dict else SimpleNamespace(**out)

    # ---- fused objective terms (motion_denoise.py:86-94 with their reverse pass, one launch sequence) -------------------
    @torch.no_grad()
    def joints_of(self, theta):
        """Jtr of the given poses [.., 69] -> [N, num_joints, 3] (no vertices written)."""
        th = theta.to(self.device, torch.float32).reshape(-1, 69).contiguous()
        joints = torch.empty(th.shape[0], self.num_joints, 3, device=self.device, dtype=torch.float32)
        self._call("pndf_lbs_forward", th.data_ptr(), th.shape[0], None, joints.data_ptr(), self._workspace(1, th.shape[0], th.device),
                   self._stream(th.device))
        return joints

    @torch.no_grad()
    def terms_grad(self, theta, joints0, it, out=None, coefs=None):
        """theta [S,T,69], joints0 [S*T, num_joints, 3] -> d (10 (1+it) temp + [it>0] 100/(1+it) data) / d theta [S,T,69];
        `coefs` = (temp_coef, data_coef) replaces the motion_denoise.py schedule (data_coef 0: no data term)."""
        if theta.dim() != 3 or theta.shape[-1] != 69:
            raise PndfError(f"theta must be [S, T, 69], got {tuple(theta.shape)}")
        S, T = theta.shape[:2]
        theta = self._device_f32(theta, "theta")
        g = torch.empty_like(theta) if out is None else self._device_f32(out, "out", coerce=False)
        if g.shape != theta.shape:
            raise PndfError(f"out must have theta's shape {tuple(theta.shape)}, got {tuple(g.shape)}")
        if joints0 is not None:
            joints0 = self._device_f32(joints0, "joints0")
            if joints0.numel() != S * T * self.num_joints * 3:
                raise PndfError(f"joints0 must hold S*T*{self.num_joints}*3 = {S * T * self.num_joints * 3} floats, got {joints0.numel()}")
        j0 = None if joints0 is None else joints0.data_ptr()
        if coefs is None:
            self._call("pndf_lbs_terms_grad", theta.data_ptr(), j0, S, T, int(it), g.data_ptr(),
                       self._workspace(S, T, theta.device), self._stream(theta.device))
        else:
            self._call("pndf_lbs_terms_grad_w", theta.data_ptr(), j0, S, T, float(coefs[0]), float(coefs[1]), g.data_ptr(),
                       self._workspace(S, T, theta.device), self._stream(theta.device))
        return g
