"""What the loaders without a device answer to a weight table that does not fit (csrc/pndf_net_plan.h: pndf_table_fault; DESIGN.md
section 2j): pndf_cpu_load_weights and the stateless packers pndf_pack_host / pndf_pack_host_split against the faulty tables of
tests/weight_table_faults.py.  The status codes are literals, recorded from the library before the loaders shared one check.  The
device loaders: tests/test_weight_table_gpu.py."""
import ctypes

import numpy as np
import pytest

import weight_table_faults as wtf
from posendf_amd import synth

OK, BAD_ARG, BAD_SHAPE, NO_WEIGHTS = 0, -1, -2, -5


@pytest.fixture(scope="module")
def lib():
    from posendf_amd import engine
    return engine.load_library()


# (hidden widths | None = configs/amass.yaml's, structure encoder)
NETWORKS = [(None, True), (None, False), ([16, 16], True)]


@pytest.mark.parametrize("hidden,encoder", NETWORKS, ids=["amass", "amass-noenc", "16-16"])
def test_the_host_twin_refuses_a_table_that_does_not_fit(lib, hidden, encoder):
    from posendf_amd.engine import CpuEngine
    widths = synth.DFNET_DIMS[1:-1] if hidden is None else tuple(hidden)
    sd = synth.make_weights(0, 2.0, 0.1, dims=((126 if encoder else 84),) + tuple(widths) + (1,))
    eng = CpuEngine("lrelu", hidden=hidden, encoder=encoder, lib=lib)
    q = synth.make_poses(65, seed=3).reshape(65, 84)
    d = np.zeros(65, np.float32)

    def forward():
        return lib.pndf_forward_cpu(eng.handle, q.ctypes.data, d.ctypes.data, 65)

    eng.load_weights(sd)
    assert forward() == OK
    first = d.copy()
    seen = []
    for fault, keep, tensors, numel, n in wtf.faulty_tables(sd):
        seen.append(fault)
        rc = lib.pndf_cpu_load_weights(eng.handle, tensors, numel, n)
        assert rc == (BAD_ARG if fault in wtf.NULL_TABLE else BAD_SHAPE), (fault, rc)
        if fault not in wtf.NULL_TABLE:
            assert lib.pndf_cpu_last_error(eng.handle), fault
        if fault in ("one tensor null", "encoder tensor of the wrong size", "trunk weight of the wrong size", "trunk bias of the wrong size"):
            # a table of the right length that does not fit leaves the handle without weights ...
            assert forward() == NO_WEIGHTS, fault
            assert lib.pndf_cpu_last_error(eng.handle) == b"pndf_cpu_load_weights has not been called"
            eng.load_weights(sd)      # ... and after a good one it computes again, the same bytes
            d[:] = 7.0
            assert forward() == OK and np.array_equal(d, first), fault
    assert seen == [f for f in wtf.FAULTS if encoder or f not in ("encoder tensor of the wrong size", "dfnet-only table")]
    assert lib.pndf_cpu_load_weights(None, None, None, 0) == BAD_ARG


@pytest.mark.parametrize("packer", ["pndf_pack_host", "pndf_pack_host_split"])
@pytest.mark.parametrize("encoder", [True, False], ids=["98 tensors", "14 tensors"])
def test_the_packers_refuse_a_table_that_does_not_fit(lib, packer, encoder):
    n = [ctypes.c_int64(), ctypes.c_int64()]
    lib.pndf_packed_sizes(*[ctypes.byref(x) for x in n])
    stream, bias = np.empty(n[0].value, np.float32), np.empty(n[1].value, np.float32)
    pack = getattr(lib, packer)
    sd = synth.make_weights(0, 2.0, 0.1, dims=synth.DFNET_DIMS if encoder else synth.DFNET_DIMS_NOENC)
    keep, tensors, numel, count = wtf.good_table(sd)
    assert pack(tensors, numel, count, stream.ctypes.data, bias.ctypes.data) == OK
    assert pack(tensors, numel, count, None, bias.ctypes.data) == BAD_SHAPE and pack(tensors, numel, count, stream.ctypes.data, None) == BAD_SHAPE
    for fault, keep, tensors, numel, count in wtf.faulty_tables(sd):
        # (the packers have no handle and take 14 tensors for a network without the encoder: dfnet.lin0.weight is then 126 wide, not 84)
        assert pack(tensors, numel, count, stream.ctypes.data, bias.ctypes.data) == BAD_SHAPE, fault
    # the widths are the table's own, up to configs/amass.yaml's: a narrower network packs, a wider one does not
    dims = list(synth.DFNET_DIMS if encoder else synth.DFNET_DIMS_NOENC)
    dims[2] = 384
    keep, tensors, numel, count = wtf.good_table(synth.make_weights(1, 2.0, 0.1, dims=tuple(dims)))
    assert pack(tensors, numel, count, stream.ctypes.data, bias.ctypes.data) == OK
    dims[2] = 640
    keep, tensors, numel, count = wtf.good_table(synth.make_weights(1, 2.0, 0.1, dims=tuple(dims)))
    assert pack(tensors, numel, count, stream.ctypes.data, bias.ctypes.data) == BAD_SHAPE
