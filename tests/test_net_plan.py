"""What the five creates that share csrc/pndf_net_plan.h refuse of a pndf_config (DESIGN.md sections 2s and 2j): pndf_train_create,
pndf_so_create, pndf_skel_create, pndf_cpu_create and pndf_create against one table of configurations with a single fault each.  The
status codes are literals, recorded from the library before each create's own checks were merged into pndf_skeleton_refusal /
pndf_dfnet_refusal; a refusal leaves a text in the family's slot.  Runs without a GPU: a configuration is refused before the device is looked for, and a
configuration a device unit accepts ends in PNDF_ERR_NO_DEVICE there."""
import ctypes

import pytest
import torch

OK, BAD_ARG, UNSUPPORTED, NO_DEVICE = 0, -1, -4, -6
ACCEPT = "accepted"      # the configuration passes: the device decides (a device unit), PNDF_OK (the host twin)

CREATES = ("pndf_train_create", "pndf_so_create", "pndf_skel_create", "pndf_cpu_create", "pndf_create")


def _set(field, value):
    return lambda c: setattr(c, field, value)


def _item(field, i, value):
    return lambda c: getattr(c, field).__setitem__(i, value)


def _ten_dims(c):
    c.n_dims = 10
    for i in range(1, 9):
        c.dims[i] = 8
    c.dims[9] = 1


def _twenty_joints(c):
    c.num_joints = 20
    c.dims[0] = 120


def _softplus_beta_0(c):
    c.act = 2
    c.beta = 0.0


def _softplus_at(precision):
    def fault(c):
        c.act = 2
        c.precision = precision
    return fault


def _softplus_encoder(beta):
    """the trunk stays lrelu; the encoder's Softplus has no beta of its own and falls back to the trunk's"""
    def fault(c):
        c.enc_act = 2
        c.enc_beta = 0.0
        c.beta = beta
    return fault


# fault on configs/amass.yaml's lrelu network (21 joints, the encoder, eight linear layers) -> train, so, skel, cpu, the engine
TABLE = (
    ("n_dims 2", _set("n_dims", 2), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("n_dims 10", _ten_dims, (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("hidden width 0", _item("dims", 2, 0), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("hidden width 1025", _item("dims", 2, 1025), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("last dim 2", _item("dims", 7, 2), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("act -1", _set("act", -1), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("act 3", _set("act", 3), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("enc_act 3", _set("enc_act", 3), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("num_joints 0", _set("num_joints", 0), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("num_joints 33", _set("num_joints", 33), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("parent[4] = 4", _item("parent", 4, 4), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("parent[2] = -2", _item("parent", 2, -2), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("dims[0] = 100", _item("dims", 0, 100), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
    ("no encoder", _item("dims", 0, 84), (UNSUPPORTED, UNSUPPORTED, ACCEPT, ACCEPT, ACCEPT)),
    ("20 joints", _twenty_joints, (UNSUPPORTED, UNSUPPORTED, ACCEPT, ACCEPT, UNSUPPORTED)),
    ("softplus, beta 0", _softplus_beta_0, (ACCEPT, ACCEPT, UNSUPPORTED, BAD_ARG, BAD_ARG)),
    # precisions and the encoder's own activation: each unit's own rules on top of the shared ones
    ("precision 7", _set("precision", 7), (ACCEPT, ACCEPT, UNSUPPORTED, ACCEPT, UNSUPPORTED)),
    ("precision f16x3", _set("precision", 1), (ACCEPT, ACCEPT, UNSUPPORTED, ACCEPT, ACCEPT)),
    ("softplus + precision f16", _softplus_at(2), (ACCEPT, ACCEPT, UNSUPPORTED, ACCEPT, UNSUPPORTED)),
    ("softplus + precision bf16", _softplus_at(3), (ACCEPT, ACCEPT, UNSUPPORTED, ACCEPT, UNSUPPORTED)),
    ("enc_act softplus, enc_beta 0, beta 0", _softplus_encoder(0.0), (ACCEPT, ACCEPT, UNSUPPORTED, BAD_ARG, BAD_ARG)),
    ("enc_act softplus, enc_beta 0, beta 100", _softplus_encoder(100.0), (ACCEPT, ACCEPT, ACCEPT, ACCEPT, ACCEPT)),
    ("enc_act -2", _set("enc_act", -2), (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)),
)


def run_create(lib, name, cfg):
    """(status, the text of the family's slot) of one create; a handle it made is destroyed again"""
    h = ctypes.c_void_p()
    family = name[:-len("_create")]
    args = (ctypes.byref(h), ctypes.byref(cfg)) + (() if name == "pndf_cpu_create" else (0,))
    rc = getattr(lib, name)(*args)
    text = getattr(lib, family + "_last_error")(None)
    if rc == OK:
        assert h.value and getattr(lib, family + "_destroy")(h) == OK
    else:
        assert not h.value
    return rc, text


def base_config(lib):
    from posendf_amd import engine
    return engine._network_config(lib, "lrelu", 100.0)


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_single_fault_configurations(row):
    from posendf_amd import engine
    lib = engine.load_library()
    _, fault, want = row
    for name, code in zip(CREATES, want):
        cfg = base_config(lib)
        fault(cfg)
        rc, text = run_create(lib, name, cfg)
        if code == ACCEPT:
            code = OK if name == "pndf_cpu_create" or torch.cuda.is_available() else NO_DEVICE
        assert rc == code, (name, row[0], rc, text)
        if rc != OK:
            assert text, (name, row[0])


def test_the_unfaulted_configuration_passes():
    from posendf_amd import engine
    lib = engine.load_library()
    for name in CREATES:
        rc, text = run_create(lib, name, base_config(lib))
        assert rc == (OK if name == "pndf_cpu_create" or torch.cuda.is_available() else NO_DEVICE), (name, rc, text)
