"""The model layer, `PoseNDF` (posendf_amd.facade) and `SkeletonPoseNDF` (posendf_amd.skeleton), characterised from outside: what
either class returns is held, bit for bit, to a direct call of the engine it drives (`CpuEngine` on the host; `Engine` /
`SkeletonEngine` on an MI355X) and, for train=True, to the stock-PyTorch statement of model/posendf.py:65-99 on the model's own
modules; the defaults and refusal texts in which the two classes differ; the weight re-upload after an in-place change, a replaced
Parameter and load_state_dict; the first-order contract.  On the SMPL table the two classes are compared with each other.

Synthetic weights behind hidden widths (64, 48) as tests/skeleton_oracle.py; lrelu and softplus; the joint trees (-1,), the 15-joint
hand and SMPL; B = 0, 1, 5 on the host, B = 0, 1, 65 (one full 64-pose block and a one-pose tail) on two streams on the GPU."""
import functools
import inspect

import numpy as np
import pytest
import torch

import skeleton_oracle as sko
from posendf_amd import synth

ACTS = ("lrelu", "softplus")
TREES = {"one": sko.ONE, "hand": sko.HAND, "smpl": tuple(synth.PARENT)}
MODELS = [("PoseNDF", "smpl")] + [("SkeletonPoseNDF", t) for t in TREES]
MODEL_IDS = [f"{c}-{t}" for c, t in MODELS]
STEPS = 3


# ------------------------------------------------------------------------------------------ the models and their engines
def config(cls, tree, act, device):
    from posendf_amd import amass_config, skeleton_config
    if cls == "SkeletonPoseNDF":
        return skeleton_config(list(TREES[tree]), act, device, hidden=sko.HIDDEN)
    assert tree == "smpl"
    cfg = amass_config(act, device)
    cfg["model"]["DFNet"]["dims"] = list(sko.HIDDEN)
    return cfg


def tensors(sd):
    return {k: torch.from_numpy(v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def network(tree, act, k=0):
    """the k-th synthetic network of a tree, counting seeds from 7 on, whose five test poses all lie off the output clip (d == 0; for
    Softplus d <= ln 2 / 100) in the fp64 oracle and do not all have one distance: a pinned value has to be able to differ"""
    parents, q, live = TREES[tree], poses(tree, 5), -1
    for seed in range(7, 71):
        sd = sko.network(parents, seed)
        d = sko.forward(q, sd, act, parents, np.float64).reshape(-1)
        live += sko.clipped(d, act) == 0 and len(set(d.tolist())) > 1
        if live == k:
            return sd
    raise AssertionError(f"no {k + 1} live networks for {tree} {act}")


def build(cls, tree, act, device="cpu", k=0, **engine):
    import posendf_amd
    cfg = config(cls, tree, act, device)
    if engine:
        cfg["engine"] = engine
    net = getattr(posendf_amd, cls)(cfg)
    net.load_state_dict(tensors(network(tree, act, k)))
    return net.eval()


@functools.lru_cache(maxsize=None)
def model(cls, tree, act, device="cpu"):
    """a model that no test changes"""
    return build(cls, tree, act, device)


def poses(tree, B, seed=21):
    J = len(TREES[tree])
    return synth.make_poses(B, seed=seed, signed=J == 1, num_joints=J)


def weights(B):
    i = np.arange(B)
    return ((-1.0) ** i * 2.0 ** (i % 5 - 2)).astype(np.float32)


def host_engine(cls, tree, act, k=0, sd=None):
    """the host twin as the class constructs it: the SMPL default for `PoseNDF`, the parent table for `SkeletonPoseNDF`"""
    from posendf_amd.engine import CpuEngine
    beta = float(config(cls, tree, act, "cpu")["model"]["DFNet"]["beta"])
    eng = CpuEngine(act, beta, hidden=sko.HIDDEN, parents=TREES[tree] if cls == "SkeletonPoseNDF" else None)
    eng.load_weights(network(tree, act, k) if sd is None else sd)
    return eng


def host_forward_grad(eng, q):
    d, dq = np.full(len(q), 7.0, np.float32), np.full(q.shape, 7.0, np.float32)
    eng.forward_grad(q.ctypes.data, None, d.ctypes.data, dq.ctypes.data, len(q))
    d0 = np.full(len(q), 7.0, np.float32)
    eng.forward(q.ctypes.data, d0.ctypes.data, len(q))
    return d, dq, d0


def host_project(eng, q, **opts):
    out, d = np.full(q.shape, 7.0, np.float32), np.full(len(q), 7.0, np.float32)
    eng.project(q.ctypes.data, out.ctypes.data, d.ctypes.data, len(q), STEPS, renorm=opts.get("renormalize"))
    return out, d


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def model_forward_grad(net, q, go):
    """(dist_pred with autograd, the pose gradient under the upstream `go`, dist_pred without autograd) as numpy"""
    x = q.clone().requires_grad_(True)
    out = net(x, train=False)
    assert list(out) == ["dist_pred"]
    d = out["dist_pred"]
    assert d.shape == (len(q), 1) and d.dtype == torch.float32 and d.requires_grad
    (g,) = torch.autograd.grad(d, x, go.reshape(-1, 1))
    assert g.shape == q.shape and g.dtype == q.dtype
    d0 = net(q, train=False)["dist_pred"]
    assert not d0.requires_grad
    return d.detach().cpu().numpy(), g.cpu().numpy(), d0.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. train=False and project on the host
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_distance_and_gradient_are_the_host_twins(cls, tree, act):
    net, eng = model(cls, tree, act), host_engine(cls, tree, act)
    for B in (0, 1, 5):
        q, go = poses(tree, B), weights(B)
        d_ref, dq_ref, d0_ref = host_forward_grad(eng, q)
        d, g, d0 = model_forward_grad(net, torch.from_numpy(q), torch.from_numpy(go))
        assert same(d, d_ref.reshape(B, 1)) and same(d0, d0_ref.reshape(B, 1)) and same(g, go.reshape(B, 1, 1) * dq_ref)
        # any leading shape, any float dtype: the gradient comes back in the pose's
        x = torch.from_numpy(q).double().reshape(B, q.shape[1] * 4).requires_grad_(True)
        d64 = net(x, train=False)["dist_pred"]
        (g64,) = torch.autograd.grad(d64.sum(), x)
        assert same(d64.detach().numpy(), d_ref.reshape(B, 1)) and same(g64.numpy(), dq_ref.astype(np.float64).reshape(x.shape))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_project_is_the_host_twin(cls, tree, act):
    net, eng = model(cls, tree, act), host_engine(cls, tree, act)
    for B in (0, 1, 5):
        q = poses(tree, B)
        for opts in ({}, {"renormalize": "unit"}):
            out_ref, d_ref = host_project(eng, q, **opts)
            x = torch.from_numpy(q.copy())
            out, d = net.project(x, steps=STEPS, **opts)
            assert same(out.numpy(), out_ref) and same(d.numpy(), d_ref.reshape(B, 1)) and same(x.numpy(), q)
            assert not out.requires_grad and not d.requires_grad
            only = net.project(x.reshape(B, q.shape[1] * 4), steps=STEPS, return_dist=False, **opts)
            assert torch.is_tensor(only) and same(only.numpy(), out_ref)
        zero, dz = net.project(torch.from_numpy(q), steps=0)      # no step: the poses pass through, the distance is reported as 0
        assert same(zero.numpy(), q) and same(dz.numpy(), np.zeros((B, 1), np.float32))


@pytest.mark.parametrize("act", ACTS)
def test_the_two_classes_agree_on_the_smpl_table(act):
    """on the SMPL table the first-order host twins behind the two classes are the same arithmetic, bit for bit"""
    a, b = model("PoseNDF", "smpl", act), model("SkeletonPoseNDF", "smpl", act)
    assert list(a.state_dict()) == list(b.state_dict()) == list(synth.state_dict_shapes(synth.skeleton_dims(synth.PARENT, sko.HIDDEN)))
    for B in (0, 1, 5):
        q, go = torch.from_numpy(poses("smpl", B)), torch.from_numpy(weights(B))
        for x, y in zip(model_forward_grad(a, q, go), model_forward_grad(b, q, go)):
            assert same(x, y)
        for opts in ({}, {"renormalize": "unit"}):
            for x, y in zip(a.project(q, steps=STEPS, **opts), b.project(q, steps=STEPS, **opts)):
                assert same(x.numpy(), y.numpy())


# ------------------------------------------------------------------------------------------ 2. train=True
def objective(net, pose, dist_gt, man_poses, eikonal):
    """model/posendf.py:65-99 on the model's own modules"""
    J = net.enc.num_joints
    pose = pose.reshape(-1, J, 4).clone().requires_grad_(True)
    dist_pred = net.dfnet(net.enc(torch.nn.functional.normalize(pose, dim=1)))
    dist_man = net.dfnet(net.enc(man_poses.reshape(-1, J, 4)))
    loss = net.loss_l1(dist_pred[:, 0], dist_gt.reshape(-1))
    if not eikonal > 0.0:
        return loss, {"dist": loss}
    (grad,) = torch.autograd.grad(dist_pred, pose, torch.ones_like(dist_pred), create_graph=True, retain_graph=True)
    return loss, {"dist": loss, "man_loss": dist_man.abs().mean(), "eikonal": ((grad.norm(2, dim=-1) - 1) ** 2).mean()}


def weight_grads(net, total):
    net.zero_grad()
    total.backward()
    return [p.grad.clone() for p in net.parameters()]


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_training_objective_is_the_stock_statement(cls, tree, act, loss_type):
    """B = 1, 5: the objective of an empty batch is the mean of no term, NaN, which pins nothing"""
    import posendf_amd
    cfg = config(cls, tree, act, "cpu")
    cfg["train"]["loss_type"] = loss_type
    net = getattr(posendf_amd, cls)(cfg)
    net.load_state_dict(tensors(network(tree, act)))
    assert type(net.loss_l1) is (torch.nn.MSELoss if loss_type == "l2" else torch.nn.L1Loss)
    assert net.train() is net and net.training and net.train(False) is net and not net.training
    for B in (1, 5):
        q, man = torch.from_numpy(poses(tree, B)), torch.from_numpy(poses(tree, 3, seed=5))
        gt = torch.linspace(0.0, 0.5, B)
        for eikonal in (0.0, 0.1):
            loss, terms = net(q.reshape(B, q.shape[1] * 4), dist_gt=gt.reshape(B, 1), man_poses=man, train=True, eikonal=eikonal)
            ref, ref_terms = objective(net, q, gt, man, eikonal)
            assert list(terms) == list(ref_terms) == (["dist", "man_loss", "eikonal"] if eikonal > 0.0 else ["dist"])
            assert terms["dist"] is loss and loss.shape == ()
            assert all(torch.equal(terms[k], ref_terms[k]) for k in terms)
            got, want = weight_grads(net, sum(terms.values())), weight_grads(net, sum(ref_terms.values()))
            assert len(got) == len(list(net.parameters())) and all(torch.equal(x, y) for x, y in zip(got, want))


# ------------------------------------------------------------------------------------------ 3. where the two classes differ
def test_forward_defaults():
    from posendf_amd import PoseNDF, SkeletonPoseNDF
    for cls, train in ((PoseNDF, True), (SkeletonPoseNDF, False)):
        par = inspect.signature(cls.forward).parameters
        assert list(par) == ["self", "pose", "dist_gt", "man_poses", "train", "eikonal"]
        assert [par[k].default for k in ("dist_gt", "man_poses", "train", "eikonal")] == [None, None, train, 0.0]
        par = inspect.signature(cls.project).parameters
        assert [(k, par[k].default) for k in list(par)[2:]] == [("steps", 100), ("return_dist", True), ("step_size", 1.0),
                                                                 ("renormalize", None), ("tol", 0.0)]
    q = torch.from_numpy(poses("smpl", 2))
    assert list(model("SkeletonPoseNDF", "smpl", "lrelu")(q)) == ["dist_pred"]
    with pytest.raises(AttributeError):      # train=True without dist_gt
        model("PoseNDF", "smpl", "lrelu")(q)


def test_config_keys_and_loss_types():
    from posendf_amd import PoseNDF, SkeletonPoseNDF
    cfg = config("PoseNDF", "smpl", "lrelu", "cpu")
    assert PoseNDF(cfg).batch_size == cfg["train"]["batch_size"]
    del cfg["train"]["batch_size"]
    with pytest.raises(KeyError, match="batch_size"):
        PoseNDF(cfg)
    net = SkeletonPoseNDF(cfg)      # train.batch_size is not read
    assert net.parents == tuple(synth.PARENT) and net.num_joints == 21
    cfg = config("PoseNDF", "smpl", "lrelu", "cpu")
    cfg["train"]["loss_type"] = "huber"      # neither l1 nor l2
    cfg["train"]["batch_size"] = 4
    assert not hasattr(PoseNDF(cfg), "loss_l1") and type(SkeletonPoseNDF(cfg).loss_l1) is torch.nn.L1Loss


def test_refusal_texts():
    from posendf_amd import SkeletonPoseNDF, skeleton_config
    from posendf_amd.engine import PndfError
    meta = torch.device("meta")
    with pytest.raises(PndfError) as e:
        model("PoseNDF", "smpl", "lrelu")._engine_for(meta)
    assert str(e.value) == "PoseNDF inference runs on the HIP engine (cuda) or the host twins (cpu), not on meta"
    with pytest.raises(PndfError) as e:
        model("SkeletonPoseNDF", "hand", "lrelu")._engine_for(meta)
    assert str(e.value) == "SkeletonPoseNDF inference runs on the HIP unit (cuda) or the host twins (cpu), not on meta"
    cfg = skeleton_config("hand", "lrelu", "cpu")
    cfg["model"]["DFNet"]["in_dim"] = 126
    with pytest.raises(PndfError) as e:
        SkeletonPoseNDF(cfg)
    assert str(e.value) == "model.DFNet.in_dim is 126; a skeleton of 15 joints with the structure encoder feeds it 90"
    cfg = skeleton_config("hand", "lrelu", "cpu", encoder=False)
    cfg["model"]["DFNet"]["in_dim"] = 90
    with pytest.raises(PndfError) as e:
        SkeletonPoseNDF(cfg)
    assert str(e.value) == "model.DFNet.in_dim is 90; a skeleton of 15 joints without the structure encoder feeds it 60"
    del cfg["model"]["DFNet"]["in_dim"]      # an absent in_dim is filled in
    assert SkeletonPoseNDF(cfg).dfnet.lin0.in_features == 60
    for table in ([-1] + list(range(32)), []):
        cfg = skeleton_config("hand", "lrelu", "cpu")
        cfg["model"]["StrEnc"]["parent_mapping"] = table
        with pytest.raises(PndfError) as e:
            SkeletonPoseNDF(cfg)
        assert str(e.value) == f"a skeleton of {len(table)} joints: 1 .. 32 are implemented"
    cfg["model"]["StrEnc"]["parent_mapping"] = "octopus"
    with pytest.raises(PndfError) as e:
        SkeletonPoseNDF(cfg)
    assert str(e.value) == "unknown skeleton 'octopus' (smpl, hand, or a parent table as a list)"


# ------------------------------------------------------------------------------------------ 4. re-upload, first order only
@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_changed_weights_are_uploaded_again(cls, tree):
    net = build(cls, tree, "lrelu")
    q = poses(tree, 5)
    x = torch.from_numpy(q)
    last = f"lin{len(sko.HIDDEN)}"

    def check(eng, before):
        d = net(x, train=False)["dist_pred"].numpy()
        assert same(d, host_forward_grad(eng, q)[2].reshape(-1, 1)) and not same(d, before)
        out, dl = net.project(x, steps=STEPS)
        ref = host_project(eng, q)
        assert same(out.numpy(), ref[0]) and same(dl.numpy(), ref[1].reshape(-1, 1))
        return d

    d = net(x, train=False)["dist_pred"].numpy()
    assert same(d, host_forward_grad(host_engine(cls, tree, "lrelu"), q)[2].reshape(-1, 1))
    eng = net._engine_for(torch.device("cpu"))
    sd = {k: v.copy() for k, v in network(tree, "lrelu").items()}
    with torch.no_grad():      # an in-place change, as an optimiser step makes it
        getattr(net.dfnet, last).bias.add_(0.25)
    sd[f"dfnet.{last}.bias"] = sd[f"dfnet.{last}.bias"] + np.float32(0.25)
    d = check(host_engine(cls, tree, "lrelu", sd=sd), d)
    sd["dfnet.lin0.bias"] = sd["dfnet.lin0.bias"] + np.float32(0.125)      # a Parameter replaced by attribute assignment
    net.dfnet.lin0.bias = torch.nn.Parameter(torch.from_numpy(sd["dfnet.lin0.bias"].copy()))
    d = check(host_engine(cls, tree, "lrelu", sd=sd), d)
    net.load_state_dict(tensors(network(tree, "lrelu", 1)))
    d = check(host_engine(cls, tree, "lrelu", 1), d)
    net.load_state_dict(tensors(network(tree, "lrelu", 2)), assign=True)
    d = check(host_engine(cls, tree, "lrelu", 2), d)
    sd = dict(network(tree, "lrelu", 2), **{k: v for k, v in network(tree, "lrelu", 3).items() if k.startswith("dfnet.")})
    dfnet = type(net.dfnet)(dict(config(cls, tree, "lrelu", "cpu")["model"]["DFNet"], in_dim=net.dfnet.lin0.in_features))
    dfnet.load_state_dict({k[len("dfnet."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("dfnet.")})
    net.dfnet = dfnet      # a submodule replaced
    check(host_engine(cls, tree, "lrelu", sd=sd), d)
    assert net._engine_for(torch.device("cpu")) is eng      # one engine all along: the weights were loaded into it again


@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_a_double_backward_raises(cls, tree):
    x = torch.from_numpy(poses(tree, 5)).requires_grad_(True)
    (g,) = torch.autograd.grad(model(cls, tree, "softplus")(x, train=False)["dist_pred"].sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ------------------------------------------------------------------------------------------ 5. on the GPU
@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    return torch.device("cuda:0")


class Direct:
    """the engine a class drives on cuda:0, called directly: `Engine` in the arithmetic `precision`, or `SkeletonEngine`"""

    def __init__(self, cls, tree, act, precision="f16x3"):
        from posendf_amd.engine import Engine, SkeletonEngine
        beta = float(config(cls, tree, act, "cuda:0")["model"]["DFNet"]["beta"])
        self.skel = cls == "SkeletonPoseNDF"
        self.eng = (SkeletonEngine(TREES[tree], act, beta, hidden=sko.HIDDEN) if self.skel else
                    Engine(act, beta, 0, precision=precision, hidden=sko.HIDDEN))
        self.eng.load_weights(network(tree, act))

    def tail(self, q):
        st = torch.cuda.current_stream(q.device).cuda_stream
        if not self.skel:
            return (st,)
        n = self.eng.workspace_bytes(len(q))
        self.ws = torch.empty(max(n, 16), dtype=torch.uint8, device=q.device)
        return self.ws.data_ptr(), self.ws.numel(), st

    def run(self, q, go):
        """what model_forward_grad and project (plain, unit quaternions) return, from direct calls"""
        B = len(q)
        d, d0, dq = torch.full((B,), 7.0, device=q.device), torch.full((B,), 7.0, device=q.device), torch.full_like(q, 7.0)
        self.eng.forward_grad(q.data_ptr(), None, d.data_ptr(), dq.data_ptr(), B, *self.tail(q))
        self.eng.forward(q.data_ptr(), d0.data_ptr(), B, *self.tail(q))
        res = [d.view(B, 1), go.reshape(B, 1, 1) * dq, d0.view(B, 1)]
        for renorm in (None, "unit"):
            out, dl = torch.full_like(q, 7.0), torch.full((B,), 7.0, device=q.device)
            self.eng.project(q.data_ptr(), out.data_ptr(), dl.data_ptr(), B, STEPS, *self.tail(q), renorm=renorm)
            res += [out, dl.view(B, 1)]
        return [x.cpu().numpy() for x in res]


def model_run(net, q, go):
    res = list(model_forward_grad(net, q, go))
    for renorm in (None, "unit"):
        res += [x.cpu().numpy() for x in net.project(q, steps=STEPS, renormalize=renorm)]
    return res


def on_two_streams(cuda, fn):
    """fn() on the default stream, on a second one, and on the default one again"""
    side = torch.cuda.Stream(cuda)
    res = [fn()]
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        res.append(fn())
    side.synchronize()
    res.append(fn())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cls,tree", MODELS, ids=MODEL_IDS)
def test_gpu_model_is_its_engine(cuda, cls, tree, act):
    net, direct = model(cls, tree, act, "cuda:0"), Direct(cls, tree, act)
    assert net._engine_for(cuda).precision == ("fp32" if cls == "SkeletonPoseNDF" else "f16x3")
    for B in (0, 1, 65):
        q, go = torch.from_numpy(poses(tree, B)).to(cuda), torch.from_numpy(weights(B)).to(cuda)
        want = direct.run(q, go) if B else [np.zeros(s, np.float32) for s in ((0, 1), q.shape, (0, 1), q.shape, (0, 1), q.shape, (0, 1))]
        for got in on_two_streams(cuda, lambda: model_run(net, q, go)):
            assert len(got) == len(want) and all(same(x, y) for x, y in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("act", ACTS)
def test_gpu_the_two_classes_on_the_smpl_table(cuda, act):
    """`PoseNDF` in exact fp32 (the runtime-planned kernels for these widths) and `SkeletonPoseNDF` (the layer-by-layer unit) are two
    fp32 evaluations of one network: each is held to the fp32 noise envelope around the fp64 oracle (tests/skeleton_oracle.py: gate),
    and each class to its own engine bit for bit"""
    a, b = build("PoseNDF", "smpl", act, "cuda:0", precision="fp32"), model("SkeletonPoseNDF", "smpl", act, "cuda:0")
    da, db = Direct("PoseNDF", "smpl", act, "fp32"), Direct("SkeletonPoseNDF", "smpl", act)
    parents, sd = TREES["smpl"], network("smpl", act)
    for B in (0, 1, 65):
        q = poses("smpl", B)
        x, go = torch.from_numpy(q).to(cuda), torch.ones(B, device=cuda)
        for net, direct in ((a, da), (b, db)):
            want = direct.run(x, go) if B else None
            for got in on_two_streams(cuda, lambda: model_run(net, x, go)):
                assert got[0].shape == (B, 1) and got[1].shape == q.shape and got[3].shape == q.shape and got[4].shape == (B, 1)
                if B:
                    assert all(same(u, v) for u, v in zip(got, want))
                    sko.gate(got[0], got[1], q, sd, act, parents, f"{type(net).__name__} {act} B={B}")
