"""`PoseModel` -- what `PoseNDF` (posendf_amd.facade) and `SkeletonPoseNDF` (posendf_amd.skeleton) share: the reference's model class
(model/posendf.py:30-101) for a joint tree `parents`, with train=False on a HIP engine.

Same parameter tree and state-dict keys as the reference (`enc.net.{j}.net.{0,2}`, `dfnet.lin{l}`).  With train=False the distance and
its input gradient come from ONE launch of the subclass's engine through the C ABI; `project()` runs the whole projection loop of
experiments/sample_poses.py:67-74 in one call.  There is no fallback on that path: a pose on a `cuda` device runs on the HIP engine or
raises (no built library, no gfx950 device).  A model whose config says `train.device: cpu` -- the reference's class works there too,
posendf.py:35,64 -- runs on the library's host twins (`pndf_*_cpu`, plain C++ on the host cores), selected by the
pose's device alone, never by a failure of the device path.

`forward(train=True)` runs on the stock PyTorch modules unless `opt['engine']['train'] = 'hip'`: then a cuda model's training
objective and every weight gradient come from csrc/pndf_train.hip (posendf_amd.train.TrainObjective) for the model's joint tree,
again with no fallback.

A subclass fills in `_new_engine` (which engine a cuda device gets), `_engine_args` (the trailing arguments of that engine's compute
calls) and, where it has one, `_engine_after_refusal` (another engine for weights the first one refused).
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .engine import CpuEngine, PndfError, TrainEngine, device_index, state_dict_order
from .modules import DFNet, StructureEncoder


def gradient(inputs, outputs):
    """reference model/posendf.py:18-27: d(sum outputs)/d inputs with create_graph/retain_graph."""
    ones = torch.ones_like(outputs, requires_grad=False, device=outputs.device)
    return torch.autograd.grad(outputs=outputs, inputs=inputs, grad_outputs=ones, create_graph=True,
                               retain_graph=True, only_inputs=True)[0]


def cached(cache, key, make):
    """cache[key], made on first use: the get-or-create of every per-device cache of the model layer"""
    value = cache.get(key)
    if value is None:
        value = cache[key] = make()
    return value


def pack_observed(observed, B, device, num_joints=21):
    """bool [J] or [B,J] (True = the joint is observed and held) -> one word per pose, bit j = joint j, as an int32 tensor [B] on
    `device`: the bits of the uint32 of include/posendf_amd_completion.h and of pndf_project_options2.  J = `num_joints` is 1 .. 32; with
    32 joints joint 31 is the sign bit of the int32 (torch has no arithmetic on uint32): the word is put together in int64 and
    brought into the int32 range before the cast, so the 32 bits are exact."""
    obs = torch.as_tensor(observed, device=device)
    if obs.dtype != torch.bool:
        raise PndfError(f"observed must be a bool tensor, not {obs.dtype}")
    J = int(num_joints)
    if not 1 <= J <= 32:
        raise PndfError(f"a mask of {J} joints: one word holds 1 .. 32")
    if obs.shape == (J,):
        obs = obs.expand(B, J)
    if obs.shape != (B, J):
        raise PndfError(f"observed must have shape [{J}] or [{B}, {J}], not {list(obs.shape)}")
    bits = torch.ones(J, dtype=torch.int64, device=device) << torch.arange(J, device=device)
    word = (obs.to(torch.int64) * bits).sum(dim=1)
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)
    return word.to(torch.int32).contiguous()


class _Distance(torch.autograd.Function):
    """dist_pred = f(pose) with first-order autograd: backward(g) = g * d dist / d pose.
    Both come from ONE engine call; double backward is not provided (train=True path has it)."""

    @staticmethod
    def forward(ctx, pose, owner):
        d, dq = owner._launch(pose, ctx.needs_input_grad[0])
        if dq is not None:
            ctx.save_for_backward(dq)
        ctx.pose_dtype = pose.dtype
        return d

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (dq,) = ctx.saved_tensors
        return (grad_out.reshape(-1, 1, 1).to(dq.dtype) * dq).to(ctx.pose_dtype), None


class PoseModel(nn.Module):
    _hip_path = "engine"        # what the refusal of `_engine_for` calls the device path

    def __init__(self, opt, parents, strenc=None, dfnet=None):
        """`strenc` / `dfnet`: the encoder's and DFNet's config where they are not opt's own model.StrEnc / model.DFNet"""
        super().__init__()
        strenc = opt["model"]["StrEnc"] if strenc is None else strenc
        dfnet = opt["model"]["DFNet"] if dfnet is None else dfnet
        self.device = opt["train"]["device"]                       # posendf.py:35
        self.parents = tuple(parents)
        self.num_joints = len(self.parents)
        self.enc = StructureEncoder(strenc).to(self.device) if strenc["use"] else None      # posendf.py:41-42
        self.dfnet = DFNet(dfnet).to(self.device)                  # posendf.py:44
        self.loss = opt["train"]["loss_type"]
        if self.loss == "l1":
            self.loss_l1 = nn.L1Loss()
        elif self.loss == "l2":
            self.loss_l1 = nn.MSELoss()
        self._act = dfnet["act"]
        self._beta = float(dfnet.get("beta", 100.0))
        # model.StrEnc.act / beta are read on their own (net_modules.py:128, :116-128); every config of the reference sets them equal
        # to DFNet's.  A mixed pair runs on the runtime-planned kernels (csrc/pndf_generic.hip).
        self._enc_act = strenc["act"] if self.enc is not None else None
        self._enc_beta = float(strenc.get("beta", self._beta)) if self.enc is not None else None
        self._hidden = list(dfnet["dims"])       # net_modules.py:14-28; narrower than amass.yaml: zero padded
        # the network as every engine's constructor takes it (a subclass whose engines take the parent table adds `parents`)
        self._net_kw = dict(act=self._act, beta=self._beta, encoder=self.enc is not None, hidden=self._hidden, enc_act=self._enc_act,
                            enc_beta=self._enc_beta)
        self._engines = {}          # device index or "cpu" -> [engine, weight fingerprint]
        # engine knob (no reference counterpart): where forward(train=True) runs for a cuda model -- "torch" (default: the stock
        # modules below) or "hip" (the objective and every weight gradient on csrc/pndf_train.hip, posendf_amd.train; no fallback:
        # PndfError without the library or a gfx950 device).  A model whose train.device is cpu keeps the stock path either way.
        self._train_backend = (opt.get("engine") or {}).get("train", "torch")
        if self._train_backend not in ("torch", "hip"):
            raise ValueError(f"opt['engine']['train'] must be 'torch' or 'hip', not {self._train_backend!r}")
        if self._train_backend == "hip" and self.enc is None:
            raise PndfError("opt['engine']['train'] = 'hip' needs the structure encoder (model.StrEnc.use: True): the reference's "
                            "train=True branch cannot run without it either")
        self._train_engines = {}    # device index -> TrainEngine
        self._param_list = None     # the cached walk of the module tree, see _fingerprint

    # ---- nn.Module conveniences the reference callers rely on -----------------------------------
    def train(self, mode=True):     # the reference override returns None (posendf.py:58-59); returning
        super().train(mode)         # self keeps statement-style callers working and fixes chaining
        return self

    # ---- engine plumbing -----------------------------------------------------------------------
    def _fingerprint(self):
        """(storage, version) of every parameter.  Walking the module tree costs 0.15 ms per call, so the walk is cached as
        (owner module, name, Parameter) triples plus the (parent, name, child) links of the tree -- and VALIDATED by identity
        on every call (~140 dict lookups): a Parameter or submodule replaced by attribute assignment
        (`net.dfnet.lin0.weight = nn.Parameter(...)`, `net.dfnet = DFNet(...)`) rebuilds the cache and so re-packs."""
        c = self._param_list
        if c is not None:
            links, leaves = c
            if not (all(par._modules.get(n) is ch for par, n, ch in links)
                    and all(m._parameters.get(n) is p for m, n, p in leaves)):
                c = None
        if c is None:
            links = [(par, n, ch) for par in self.modules() for n, ch in par._modules.items()]
            leaves = [(m, n, p) for m in self.modules() for n, p in m._parameters.items() if p is not None]
            if len(leaves) != len(list(self.parameters())):      # shared / parametrised tensors: no cache, full walk
                return tuple((p.data_ptr(), p._version) for p in self.parameters())
            c = self._param_list = (links, leaves)
        return tuple((p.data_ptr(), p._version) for _, _, p in c[1])

    def _apply(self, fn, *args, **kwargs):          # .to() / .float() / .cuda(): parameters may be replaced
        self._param_list = None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):     # assign=True replaces the Parameter objects
        self._param_list = None
        return super().load_state_dict(*args, **kwargs)

    def _new_engine(self, idx):
        """the HIP engine of cuda device `idx`, without weights"""
        raise NotImplementedError

    def _engine_args(self, eng, device, B):
        """what a compute call of `_new_engine`'s engine takes after the batch size, for B poses on the cuda `device`"""
        raise NotImplementedError

    def _engine_after_refusal(self, eng, err):
        """the engine to load the weights into after `eng.load_weights` raised `err`; None: the error stands"""
        return None

    def _engine_for(self, device):
        if device.type not in ("cuda", "cpu"):
            raise PndfError(f"{type(self).__name__} inference runs on the HIP {self._hip_path} (cuda) or the host twins (cpu), not on {device}")
        host = device.type == "cpu"
        idx = "cpu" if host else device_index(device)
        entry = cached(self._engines, idx, lambda: [CpuEngine(**self._net_kw) if host else self._new_engine(idx), None])
        fp = self._fingerprint()
        if entry[1] != fp:          # first use, load_state_dict, an optimiser step, a replaced Parameter, .to(): re-pack the weights
            sd = self.state_dict()
            keys = state_dict_order(self.enc is not None, len(self._hidden) + 1, parents=self.parents)
            weights = {k: sd[k].detach().float().cpu().numpy() for k in keys}
            try:
                entry[0].load_weights(weights)
            except PndfError as e:
                other = self._engine_after_refusal(entry[0], e)
                if other is None:
                    raise
                entry[0] = other
                other.load_weights(weights)
            entry[1] = fp
        return entry[0]

    def _launch(self, pose, want_grad):
        """dist_pred [B,1] and, when asked for, d dist / d pose [B,J,4] (else None) from ONE engine call.  A cuda engine is not called
        for an empty batch; the host twin is."""
        q = pose.detach()
        if q.dtype != torch.float32 or not q.is_contiguous():
            q = q.float().contiguous()
        B = q.shape[0]
        d = torch.empty(B, device=q.device, dtype=torch.float32)
        dq = torch.empty_like(q) if want_grad else None
        eng = self._engine_for(q.device)
        host = q.device.type == "cpu"
        if B or host:
            tail = () if host else self._engine_args(eng, q.device, B)
            if want_grad:
                eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, *tail)
            else:
                eng.forward(q.data_ptr(), d.data_ptr(), B, *tail)
        return d.view(B, 1), dq

    # ---- reference API -------------------------------------------------------------------------
    def _forward_train(self, pose, dist_gt, man_poses, eikonal):
        """forward(train=True) for `pose` [B,J,4] on the model's device: the HIP objective for a cuda pose of a model whose
        opt['engine']['train'] is 'hip', the stock modules otherwise"""
        if self._train_backend == "hip" and pose.device.type == "cuda":
            return self._forward_train_hip(pose, dist_gt, man_poses, eikonal)
        return self._objective(pose, dist_gt, man_poses, eikonal)

    def _forward_train_hip(self, pose, dist_gt, man_poses, eikonal):
        """posendf.py:65-99 on the HIP engine: the same (loss, loss_dict), `loss` and loss_dict['dist'] the same tensor."""
        from .train import LOSS_CODES, TrainObjective
        idx = device_index(pose.device)
        eng = cached(self._train_engines, idx, lambda: TrainEngine(device=idx, **self._net_kw))
        named = dict(self.named_parameters())
        params = [named[k] for k in state_dict_order(True, len(self._hidden) + 1, parents=self.parents)]
        man = man_poses.to(device=self.device).reshape(-1, self.num_joints, 4)
        eik = eikonal > 0.0
        loss, loss_man, loss_eik = TrainObjective.apply(eng, pose, dist_gt.to(device=self.device).reshape(-1), man,
                                                        LOSS_CODES[self.loss], eik, *params)
        if eik:
            return loss, {"dist": loss, "man_loss": loss_man, "eikonal": loss_eik}
        return loss, {"dist": loss}

    def _objective(self, pose, dist_gt, man_poses, eikonal):
        """the training objective of model/posendf.py:65-99 on the stock PyTorch modules"""
        pose.requires_grad = True
        dist_gt = dist_gt.to(device=self.device).reshape(-1)
        x = torch.nn.functional.normalize(pose, dim=1)             # joint-axis normalisation, posendf.py:71
        dist_pred = self.dfnet(self.enc(x) if self.enc is not None else x)
        man = man_poses.to(device=self.device).reshape(-1, self.num_joints, 4)
        dist_man = self.dfnet(self.enc(man) if self.enc is not None else man)
        loss = self.loss_l1(dist_pred[:, 0], dist_gt)
        if eikonal > 0.0:
            eik = ((gradient(pose, dist_pred).norm(2, dim=-1) - 1) ** 2).mean()
            return loss, {"dist": loss, "man_loss": dist_man.abs().mean(), "eikonal": eik}
        return loss, {"dist": loss}

    @torch.no_grad()
    def project(self, noisy_poses, steps=100, return_dist=True, *, step_size=1.0, renormalize=None, tol=0.0):
        """experiments/sample_poses.py:67-74 as ONE engine call: `steps` times
        q <- q - dist_pred(q) * d dist_pred / d q.  Returns (poses [B,J,4], dist [B,1] of the last
        iteration).

        Step options (keyword only; the defaults are the reference's bare loop, bit for bit): `step_size` alpha scales the step,
        q <- q - alpha (d grad); `renormalize` = "unit" divides every joint quaternion of an updated pose by its norm (clamped at
        1e-12 like F.normalize), "unit_flip" also negates those with a negative real part; `tol` > 0 leaves a pose with
        dist_pred < tol unchanged.  The input is used as given; `dist` stays the distance evaluated before the last update."""
        q = noisy_poses.to(device=self.device).reshape(-1, self.num_joints, 4).float().contiguous()
        B = q.shape[0]
        out = torch.empty_like(q)
        d = torch.empty(B, device=q.device, dtype=torch.float32)
        eng = self._engine_for(q.device)
        host = q.device.type == "cpu"
        if B or host:       # as `_launch`
            eng.project(q.data_ptr(), out.data_ptr(), d.data_ptr(), B, int(steps), *(() if host else self._engine_args(eng, q.device, B)),
                        step_size=step_size, renorm=renormalize, tol=tol)
        return (out, d.view(-1, 1)) if return_dist else out
