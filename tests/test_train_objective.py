"""CPU checks of the training objective's HIP path (csrc/pndf_train.hip, posendf_amd/train.py): the new C-ABI entry points exist,
refuse to run without a gfx950 device and refuse an encoder-less network; the facade's opt-in key defaults to the stock path;
and the fp64 oracle of the objective -- torch autograd in float64 of this repository's own module tree, the facade's stock
train=True code -- reproduces every tests/golden/train_*.npz fixture, which the real reference produced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import train_fixtures as tf

NAMES = ("pndf_train_create", "pndf_train_destroy", "pndf_train_workspace_floats", "pndf_train_forward", "pndf_train_backward",
         "pndf_train_last_error")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def _cfg(lib, encoder=True):
    from posendf_amd.engine import ACT_CODES, PndfConfig
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), ACT_CODES["lrelu"], 100.0)
    if not encoder:
        cfg.dims[0] = 84
    return cfg


def test_train_entry_points_are_exported(lib):
    from posendf_amd import engine
    for name in NAMES:
        assert name in engine.EXPORTS and hasattr(lib, name), name
    assert "pndf_experiment_word_train" in engine.EXPERIMENT_WORDS
    assert ctypes.c_uint.in_dll(lib, "pndf_experiment_word_train").value == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is visible")
def test_create_without_a_gfx950_device_fails(lib):
    from posendf_amd.engine import PndfError, TrainEngine
    h = ctypes.c_void_p()
    assert lib.pndf_train_create(ctypes.byref(h), ctypes.byref(_cfg(lib)), 0) == -6      # PNDF_ERR_NO_DEVICE
    assert not h.value and b"no CPU fallback" in lib.pndf_train_last_error(None)
    with pytest.raises(PndfError, match="pndf_train_create"):
        TrainEngine("lrelu")


def test_create_refuses_an_encoderless_network(lib):
    h = ctypes.c_void_p()
    assert lib.pndf_train_create(ctypes.byref(h), ctypes.byref(_cfg(lib, encoder=False)), 0) == -4      # PNDF_ERR_UNSUPPORTED
    assert not h.value and b"structure encoder" in lib.pndf_train_last_error(None)


def test_facade_hip_path_refuses_an_encoderless_config():
    from posendf_amd import PoseNDF
    from posendf_amd.engine import PndfError
    cfg = tf.config("lrelu", [256, 512, 1024, 512, 256, 64], "l1", "cpu", train_backend="hip")
    cfg["model"]["StrEnc"]["use"] = False
    cfg["model"]["DFNet"]["in_dim"] = 84
    with pytest.raises(PndfError, match="structure encoder"):
        PoseNDF(cfg)


def test_train_key_defaults_to_torch():
    from posendf_amd import PoseNDF, amass_config
    assert PoseNDF(amass_config("lrelu", "cpu"))._train_backend == "torch"
    cfg = amass_config("lrelu", "cpu")
    cfg["engine"] = {"train": "cuda"}
    with pytest.raises(ValueError, match="'torch' or 'hip'"):
        PoseNDF(cfg)


def test_hip_key_on_a_cpu_model_keeps_the_stock_path():
    from posendf_amd import PoseNDF
    sd, hidden = tf.case_weights("trained_lrelu")
    q, gt, qm = (torch.from_numpy(a[:40]) for a in tf.case_inputs())
    out = []
    for backend in ("torch", "hip"):
        net = PoseNDF(tf.config("lrelu", hidden, "l1", "cpu", train_backend=backend))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        losses, grads, ld = tf.run_objective(net, q.clone(), gt, qm, 1.0)
        assert type(ld["dist"].grad_fn).__name__ != "TrainObjectiveBackward"
        out.append((losses, grads))
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(out[0][1][k], out[1][1][k]) for k in out[0][1])


@pytest.mark.parametrize("name", list(tf.CASES))
def test_fp64_oracle_reproduces_the_fixture(name):
    z = dict(np.load(tf.fixture_path(name)))
    act, weights, loss, eikonal = tf.CASES[name]
    assert str(z["act"]) == act and str(z["weights"]) == weights and str(z["loss_type"]) == loss and float(z["eikonal"]) == eikonal
    trunk, beta, enc_act, enc_beta = tf.sides(act)      # what the reference's config held: model.DFNet.act / beta, model.StrEnc.act / beta
    assert (str(z["dfnet_act"]), float(z["dfnet_beta"]), str(z["strenc_act"]), float(z["strenc_beta"])) == (trunk, beta, enc_act, enc_beta)
    assert os.path.getsize(tf.fixture_path(name)) < 700 * 1024
    q, gt, qm = tf.case_inputs()
    assert np.array_equal(z["q"], q) and np.array_equal(z["dist_gt"], gt) and np.array_equal(z["q_man"], qm)
    losses, grads = tf.oracle64(act, weights, loss, eikonal, q, gt, qm)
    ref = z["losses_f64"]
    for i, k in enumerate(tf.LOSS_KEYS):
        if k in losses:
            assert abs(losses[k] - ref[i]) <= 1e-12 * max(abs(ref[i]), 1.0), (k, losses[k], ref[i])
        else:
            assert np.isnan(ref[i])
    hidden = [int(w) for w in z["hidden"]]
    for k, g in grads.items():
        for part, v in tf.digest(k, g, hidden).items():
            want = z[f"g_f64::{k}" + (f"::{part}" if part else "")]
            err = np.linalg.norm(np.asarray(v, np.float64) - want) / max(np.linalg.norm(want), 1e-300)
            assert err <= 1e-10, (name, k, part, err)


@pytest.mark.skipif(not os.path.isdir(os.environ.get("POSENDF_REFERENCE", "/root/reference")), reason="the reference is not here")
def test_regenerating_a_fixture_is_bit_equal():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_train", os.path.join(tf.GOLDEN, "make_golden_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in tf.CASES:
        fresh = mod.make(name)
        z = np.load(tf.fixture_path(name))
        assert set(fresh) == set(z.files), name
        for k in z.files:
            if k != "torch_version":
                assert np.array_equal(np.asarray(fresh[k]), z[k], equal_nan=z[k].dtype.kind == "f"), (name, k)
