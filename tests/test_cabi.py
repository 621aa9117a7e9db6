"""CPU-side checks of the C ABI: the library loads, exports every symbol include/posendf_amd.h declares,
validates arguments, and refuses to run without a gfx950 device (no CPU fallback).  No compute calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import cabi_headers as ch
from conftest import REPO

# the headers of include/ in the order of posendf_amd/abi.py: HEADERS, each with the number of entry points it declares
HEADER_COUNTS = {"posendf_amd.h": 61, "posendf_amd_debug.h": 10, "posendf_amd_completion.h": 4, "posendf_amd_interpolation.h": 5,
                 "posendf_amd_second_order.h": 6, "posendf_amd_online.h": 4, "posendf_amd_skeleton.h": 8, "posendf_amd_skeleton_train.h": 2,
                 "posendf_amd_skeleton_data.h": 3}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from posendf_amd import engine
    return engine.load_library()


def _declared(header):
    return ch.called(ch.header_text(header))


def test_exports_match_header(lib):
    declared = _declared("posendf_amd.h")
    assert declared, "no declarations found"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    from posendf_amd import engine
    assert set(engine.EXPORTS) == declared


def test_debug_entry_points_live_in_their_own_header(lib):
    """the drop-in boundary carries no bring-up / profiling entry point -- those are declared in
    include/posendf_amd_debug.h, which a maintainer binding the library never includes."""
    from posendf_amd import engine
    public = open(os.path.join(REPO, "include", "posendf_amd.h")).read()
    assert "debug" not in public.lower()
    dbg = _declared("posendf_amd_debug.h")
    assert dbg == set(engine.DEBUG_EXPORTS) and all(n.startswith("pndf_debug_") for n in dbg)
    assert not (dbg & set(engine.EXPORTS))
    for name in dbg:
        assert hasattr(lib, name), f"{name} declared in the debug header but not exported"      # (answered by the debug library, lazily)
    # ... and the PRODUCT library carries none of it: no pndf_debug_* symbol, no instrumented / stage-dump kernel, no probe
    import __graft_entry__ as ge
    names = ch.exported_symbols(ge.LIB)
    assert "pndf_project" in names and "pndf_fused_split_relu_kernel" in names
    leaked = sorted(n for n in names if "debug" in n or "timing" in n or n.endswith("_dbg") or "probe" in n)
    assert not leaked, leaked
    assert dbg <= ch.exported_symbols(engine.debug_library_path(ge.LIB))


def test_product_library_carries_no_experiment(lib, tmp_path):
    """The lab is quarantined from the product (csrc/pndf_experiment.h): every translation unit of the library exports one
    word with a bit per tuning / ablation macro that differed from its product default at build time; all of them are 0 in
    the library the package loads, pndf_version() says so, and an experiment macro without the umbrella does not compile."""
    import subprocess
    from posendf_amd import engine
    for name in engine.EXPERIMENT_WORDS:
        assert ctypes.c_uint.in_dll(lib, name).value == 0, name
    for name in engine.DEBUG_EXPERIMENT_WORDS:      # the debug library built next to it: the same rule
        assert ctypes.c_uint.in_dll(lib._debug(), name).value == 0, name
    assert engine.experiment_word(lib) == 0 and lib.pndf_experiment_word() == 0 and lib.pndf_debug_experiment_word() == 0
    assert b"experiments=0x00000000" in lib.pndf_version()
    hdr = os.path.join(REPO, "posendf_amd", "csrc", "pndf_experiment.h")
    cc = ["gcc", "-x", "c", "-fsyntax-only", hdr]
    assert subprocess.run(cc, capture_output=True).returncode == 0
    for macro in ("PNDF_ABLATE=2", "PNDF_SP_DIAG=4", "PNDF_RING_ALIAS_F", "PNDF_NT_MODE=1", "PNDF_RING_SLOTS=4", "PNDF_DMA_EARLY=0",
                  "PNDF_LBS_DIAG=1", "PNDF_EXP_LO_BITS=4", "PNDF_RING_PIECES=2", "PNDF_RING_STAMPS=1"):
        bad = subprocess.run(cc + ["-D" + macro], capture_output=True, text=True)
        assert bad.returncode != 0 and "PNDF_EXPERIMENT" in bad.stderr, macro
        assert subprocess.run(cc + ["-D" + macro, "-DPNDF_EXPERIMENT=1"], capture_output=True).returncode == 0, macro
    # the word itself: a probe translation unit built with an arm set reports the arm's bit and the umbrella's
    src = tmp_path / "word.c"
    src.write_text('#include "pndf_experiment.h"\n#include <stdio.h>\nint main(void) { printf("%08x\\n", PNDF_EXPERIMENT_WORD); return 0; }\n')
    exe = tmp_path / "word"
    inc = ["-I", os.path.dirname(hdr)]
    for flags, want in (([], "00000000"), (["-DPNDF_EXPERIMENT=1", "-DPNDF_ABLATE=1024"], "80000001"),
                        (["-DPNDF_EXPERIMENT=1", "-DPNDF_SP_DIAG=32", "-DPNDF_DMA_EARLY=0"], "80000202"),
                        (["-DPNDF_TU_RING_PIECES=2", "-DPNDF_TU_RING_STAMPS=1"], "00000000")):      # a wrapper unit's structural values
        subprocess.run(["gcc", *inc, *flags, str(src), "-o", str(exe)], check=True)
        assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == want, flags
    # and the build entry refuses flags for the product path
    import __graft_entry__ as ge
    with pytest.raises(ValueError, match="product library takes no compile flags"):
        ge.build_library(ge.LIB, flags=["-DPNDF_ABLATE=2"])


def test_default_config(lib):
    from posendf_amd.engine import PndfConfig
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), 1, 100.0)
    assert cfg.num_joints == 21 and cfg.n_dims == 8
    assert list(cfg.dims[:8]) == [126, 256, 512, 1024, 512, 256, 64, 1]
    assert list(cfg.parent[:21]) == [-1, -1, -1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19]


def test_create_rejects_unsupported(lib):
    from posendf_amd.engine import PndfConfig
    h = ctypes.c_void_p()
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), 7, 100.0)            # unknown activation code
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4
    assert b"activation" in lib.pndf_last_error(None)
    lib.pndf_default_config(ctypes.byref(cfg), 2, -1.0)             # softplus needs beta > 0
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -1
    lib.pndf_default_config(ctypes.byref(cfg), 2, 100.0)
    cfg.precision = 2                                               # the plain-f16 comparison kernel is relu-family only
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4
    lib.pndf_default_config(ctypes.byref(cfg), 1, 100.0)
    cfg.precision = 9                                               # unknown precision code
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4
    lib.pndf_default_config(ctypes.byref(cfg), 1, 100.0)
    assert cfg.precision == 0
    cfg.dims[2] = 2048                                              # wider than 1024: refused
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4
    cfg.dims[2] = 512
    cfg.n_dims = 10                                                 # deeper than n_dims 9: refused
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4
    cfg.n_dims = 8
    # (wider than amass.yaml up to 1024, and other depths, run on the runtime-planned kernels: tests/test_depth.py)
    cfg.dims[2] = 640
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) in (0, -6)
    if h.value:
        lib.pndf_destroy(h)
        h = ctypes.c_void_p()
    cfg.dims[2] = 512
    cfg.dims[2] = 384                                               # narrower: accepted (runs zero padded) -- the
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) in (0, -6)    # next hurdle is the device
    if h.value:
        lib.pndf_destroy(h)
        h = ctypes.c_void_p()
    cfg.dims[2] = 512
    cfg.parent[3] = 0
    assert lib.pndf_create(ctypes.byref(h), ctypes.byref(cfg), 0) == -4


def test_no_device_is_a_loud_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from posendf_amd.engine import Engine, PndfError
    with pytest.raises(PndfError, match="no HIP device|no CPU fallback"):
        Engine("lrelu")


def test_pack_host_rejects_bad_tables(lib):
    from posendf_amd import engine, synth
    sd = synth.make_weights(1)
    stream, bias = engine.pack_host(sd, lib)
    assert np.isfinite(stream).all()
    bad = dict(sd)
    bad["dfnet.lin3.weight"] = bad["dfnet.lin3.weight"][:, :-1]
    with pytest.raises(engine.PndfError):
        engine.pack_host(bad, lib)


def test_split_packer_scales_each_layer_and_refuses_the_unscalable(lib):
    """The fp16 hi/lo split carries s_l W with a per-layer power of two s_l (largest |weight| -> [2^12, 2^13)), so any
    weight magnitude packs; a layer without a finite non-zero weight cannot be scaled and is refused, not degraded."""
    from posendf_amd import engine, synth
    from lane_model import SCALE_OFF
    sd = synth.make_weights(1)
    _, bias = engine.pack_host(sd, lib, split=True)
    for scale_by in (1e-6, 1e7):                                 # far outside any fixed scaling window
        odd = dict(sd)
        odd["dfnet.lin2.weight"] = sd["dfnet.lin2.weight"] * np.float32(scale_by)
        stream, b2 = engine.pack_host(odd, lib, split=True)
        trunk = stream.reshape(-1, 256)[48:48 + 10624].view(np.float16).astype(np.float32)     # between the encoder sections
        assert np.isfinite(trunk).all() and np.abs(trunk).max() <= 2.0 ** 13            # hi = rne(scaled weight) may round up to 2^13
        inv = b2[SCALE_OFF:SCALE_OFF + 6]
        assert (np.log2(inv) == np.round(np.log2(inv))).all()
        mx = np.abs(odd["dfnet.lin2.weight"]).max() / inv[2]
        assert 2.0 ** 12 <= mx < 2.0 ** 13
        assert (inv[[0, 1, 3, 4, 5]] == bias[SCALE_OFF:SCALE_OFF + 6][[0, 1, 3, 4, 5]]).all()
    zero = dict(sd)
    zero["dfnet.lin4.weight"] = np.zeros_like(sd["dfnet.lin4.weight"])
    engine.pack_host(zero, lib)                                  # fine for the exact fp32 stream
    with pytest.raises(engine.PndfError):
        engine.pack_host(zero, lib, split=True)
    nan = dict(sd)
    w = sd["dfnet.lin0.weight"].copy()
    w[3, 5] = np.nan
    nan["dfnet.lin0.weight"] = w
    with pytest.raises(engine.PndfError):
        engine.pack_host(nan, lib, split=True)


def test_facade_surface_cpu():
    """Reference-compatible surface without touching the engine: state-dict keys, train=True objective
    (pinned against the reference in tests/golden); train=False of a `train.device: cpu` model runs on the library's host
    twins (tests/test_cpu_twin.py holds them to the golden vectors), any other device type is refused."""
    import torch
    from conftest import golden_weights, load_golden
    from posendf_amd import PoseNDF, amass_config, synth
    from posendf_amd.engine import PndfError
    net = PoseNDF(amass_config("lrelu", "cpu"))
    assert list(net.state_dict().keys()) == list(synth.state_dict_shapes().keys())
    assert sum(p.numel() for p in net.parameters()) == 1365565
    net.load_state_dict({k: torch.from_numpy(v) for k, v in golden_weights("live").items()})
    assert net.eval() is net
    g = load_golden("lrelu", "live")
    loss, ld = net(torch.from_numpy(g["train_q"]).clone(), torch.from_numpy(g["train_dist"]),
                   torch.from_numpy(g["train_man"]), train=True, eikonal=1.0)
    assert abs(loss.item() - g["train_loss"]) < 1e-6
    assert abs(ld["man_loss"].item() - g["train_man_loss"]) < 1e-6
    assert abs(ld["eikonal"].item() - g["train_eikonal"]) < 1e-5
    loss.backward()                                                 # weight gradients flow (train_posendf.py:98)
    assert net.dfnet.lin0.weight.grad is not None
    d = net(torch.from_numpy(g["q"]), train=False)["dist_pred"]
    assert d.shape == (len(g["q"]), 1) and d.device.type == "cpu"
    assert net._engine_for(torch.device("cpu")).kernel_name() == "pndf_cpu (host twin)"
    with pytest.raises(PndfError):
        net._engine_for(torch.device("meta"))


def test_reference_checkpoint_interchange(tmp_path):
    """the reference's on-disk checkpoint (model/train_posendf.py:147-156: a dict with
    'epoch' / 'model_state_dict' / 'optimizer_state_dict', legacy non-zip serialisation) loads unchanged, the way
    experiments/sample_poses.py:90-91 does it, and round-trips."""
    import torch
    from conftest import golden_weights
    from posendf_amd import PoseNDF, amass_config
    src = PoseNDF(amass_config("lrelu", "cpu"))
    src.load_state_dict({k: torch.from_numpy(v) for k, v in golden_weights("mixed").items()})
    opt = torch.optim.Adam(src.parameters(), lr=1e-5, weight_decay=1e-4)          # train_posendf.py:30
    path = tmp_path / "checkpoint_epoch_best.tar"
    torch.save({"epoch": 7, "model_state_dict": src.state_dict(), "optimizer_state_dict": opt.state_dict()}, path,
               _use_new_zipfile_serialization=False)
    ckpt = torch.load(path, map_location="cpu")["model_state_dict"]                # sample_poses.py:90
    dst = PoseNDF(amass_config("lrelu", "cpu"))
    dst.load_state_dict(ckpt)                                                      # sample_poses.py:91
    dst.eval()
    for (ka, a), (kb, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    # the packed engine weights are a pure function of the state dict
    from posendf_amd import engine
    s1, b1 = engine.pack_host({k: v.numpy() for k, v in src.state_dict().items()})
    s2, b2 = engine.pack_host({k: v.numpy() for k, v in dst.state_dict().items()})
    assert np.array_equal(s1, s2) and np.array_equal(b1, b2)


@pytest.mark.parametrize("header", list(HEADER_COUNTS))
def test_header_is_plain_c(tmp_path, header):
    """The drop-in boundary is a C ABI: every header of include/, included alone, must compile as C99 (no C++-isms, no torch / HIP
    types in the signatures) and a C translation unit must be able to name every entry point: its own and, through it, posendf_amd.h's."""
    import shutil
    from posendf_amd import abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    refs = "\n".join(f"    (void)&{name};" for name in dict.fromkeys(abi.exports(header) + abi.EXPORTS))
    ok, diagnostics = ch.compiles_as_c99(tmp_path, f'#include "{header}"\nint main(void) {{\n{refs}\n'
                                         "    return sizeof(pndf_config) > 0 && sizeof(pndf_project_options) > 0 ? 0 : 1;\n}\n")
    assert ok, diagnostics


def test_weight_fingerprint_sees_replaced_parameters_and_modules():
    """The facade re-packs the engine's weights when the fingerprint changes.  Its cached walk of the module tree is validated
    by identity on every call: in-place updates, a Parameter replaced by attribute assignment, a swapped submodule and
    load_state_dict(assign=True) all change it (the cache used to go stale on the middle two)."""
    import torch
    import torch.nn as nn
    from posendf_amd import PoseNDF, amass_config
    net = PoseNDF(amass_config("lrelu", "cpu"))
    f = [net._fingerprint()]
    assert net._fingerprint() == f[0]
    with torch.no_grad():
        net.dfnet.lin6.bias.add_(1.0)
    f.append(net._fingerprint())
    net.dfnet.lin0.weight = nn.Parameter(net.dfnet.lin0.weight.detach().clone())
    f.append(net._fingerprint())
    old = net.dfnet.lin3
    net.dfnet.lin3 = nn.Linear(old.in_features, old.out_features)
    f.append(net._fingerprint())
    net.enc.net[4].net[0].bias = nn.Parameter(torch.zeros(10))
    f.append(net._fingerprint())
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()}, assign=True)
    f.append(net._fingerprint())
    assert len(set(f)) == len(f)
    assert len(f[-1]) == 98


# ---- the header registry (posendf_amd/abi.py: HEADERS), the handle base, stream helper and stateless wrappers (posendf_amd/engine.py) ----

def test_header_registry():
    """abi.HEADERS is the header set: the files of include/, in the order they were added, no name in two tables; the export
    tuples are read from it."""
    from posendf_amd import abi, engine
    assert list(abi.HEADERS) == list(HEADER_COUNTS)
    assert set(abi.HEADERS) == {name for name in os.listdir(os.path.join(REPO, "include")) if name.endswith(".h")}
    tables = list(abi.HEADERS.items())
    for i, (header, table) in enumerate(tables):
        for other, other_table in tables[i + 1:]:
            assert not set(table) & set(other_table), (header, other, sorted(set(table) & set(other_table)))
    assert abi.DEBUG_HEADER in abi.HEADERS
    assert abi.PRODUCT_EXPORTS == sum((abi.exports(h) for h in abi.HEADERS if h != abi.DEBUG_HEADER), ())
    assert engine.EXPORTS == abi.EXPORTS == abi.exports("posendf_amd.h") and engine.DEBUG_EXPORTS == abi.DEBUG_EXPORTS == abi.exports(abi.DEBUG_HEADER)


@pytest.mark.parametrize("header,count", list(HEADER_COUNTS.items()))
def test_signature_table_matches_header(lib, header, count):
    """Every declaration of the header has an entry of the same parameter count and return kind in the table the binding is
    made from, in the header's order, no entry leaves its restype to ctypes' default, the loaded library is bound from the table and
    the binary the header belongs to defines every name."""
    import __graft_entry__ as ge
    from posendf_amd import abi
    protos, sigs = ch.prototypes(header), abi.HEADERS[header]
    assert len(protos) == count and set(protos) == ch.called(ch.header_text(header, comments=False)), "the declaration pattern missed one"
    if header in ("posendf_amd.h", abi.DEBUG_HEADER):      # (the companion headers' comments name other headers' functions)
        assert set(protos) == _declared(header), "the declaration pattern missed one"
    assert list(sigs) == list(protos) and tuple(sigs) == abi.exports(header)
    kinds = {"void": (None,), "const char *": (ctypes.c_char_p,), "int64_t": (ctypes.c_int64,), "int": (ctypes.c_int, ctypes.c_int32),
             "int32_t": (ctypes.c_int, ctypes.c_int32), "unsigned": (ctypes.c_uint,)}
    assert ctypes.sizeof(ctypes.c_int) == 4
    debug = header == abi.DEBUG_HEADER
    bound = lib._debug() if debug else lib
    defined = ch.exported_symbols(abi.debug_library_path(ge.LIB) if debug else ge.LIB)
    for name, (ret, n_params) in protos.items():
        entry = sigs[name]
        assert isinstance(entry, tuple) and len(entry) == 2, f"{name}: the entry must be (restype, argtypes)"
        restype, argtypes = entry
        assert len(argtypes) == n_params, f"{name}: {n_params} parameters declared, {len(argtypes)} bound"
        assert ret in kinds and restype in kinds[ret], f"{name}: returns {ret}, bound as {restype}"
        fn = getattr(bound, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), f"{name}: the loaded library is not bound from the table"
        assert name in defined, f"{name}: not a defined dynamic symbol of its library"


def test_experiment_words_cover_every_translation_unit(lib):
    """The gate of build() reads EXPERIMENT_WORDS / DEBUG_EXPERIMENT_WORDS: they are exactly the pndf_experiment_word_* data symbols the
    two libraries export, so a new translation unit cannot stay outside the gate."""
    import subprocess
    import __graft_entry__ as ge
    from posendf_amd import engine

    def words(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines() if ln.strip()]
        return [r[-1] for r in rows if r[-1].startswith("pndf_experiment_word_") and r[-2] in "BbDdRrSsGg"]
    product, debug = words(ge.LIB), words(engine.debug_library_path(ge.LIB))
    assert len(set(product)) == len(product) and len(set(debug)) == len(debug)
    assert set(product) == set(engine.EXPERIMENT_WORDS) and len(engine.EXPERIMENT_WORDS) == len(product)
    assert set(debug) == set(engine.DEBUG_EXPERIMENT_WORDS) and len(engine.DEBUG_EXPERIMENT_WORDS) == len(debug)
    assert "pndf_experiment_word_bf16" in engine.EXPERIMENT_WORDS


def _refused_handles():
    from posendf_amd import engine
    return {"CpuEngine": (engine.CpuEngine, dict(hidden=[2048]), "pndf_cpu_create", False),      # wider than 1024: refused on any machine
            "Engine": (engine.Engine, {}, "pndf_create", True),
            "TrainEngine": (engine.TrainEngine, {}, "pndf_train_create", True),
            "KnnIndex": (engine.KnnIndex, dict(poses_ptr=None, N=0), "pndf_knn_create", False)}  # N < 1: refused before the device is looked for


@pytest.mark.parametrize("which", ["CpuEngine", "Engine", "TrainEngine", "KnnIndex"])
def test_handle_life_cycle_after_a_failed_create(lib, which):
    import torch
    from posendf_amd.engine import PndfError
    cls, kwargs, create, needs_no_device = _refused_handles()[which]
    if needs_no_device and torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    obj = cls.__new__(cls)
    with pytest.raises(PndfError, match=rf"{create} failed \(-\d\): \S") as e:
        obj.__init__(lib=lib, **kwargs)
    if needs_no_device:
        assert re.search("no HIP device|no CPU fallback|gfx950", str(e.value))
    assert obj.handle is None
    obj.close()
    obj.close()
    obj.__del__()
    assert obj.handle is None


def test_handle_close_is_idempotent(lib):
    from posendf_amd.engine import CpuEngine
    eng = CpuEngine("relu", lib=lib)
    assert eng.handle
    eng.close()
    assert eng.handle is None
    eng.close()
    eng.__del__()
    assert eng.handle is None


def test_stream_handle_and_checked_wrappers(lib):
    """stream_handle is 0 on the host; a stateless wrapper raises PndfError naming the entry point that refused.  The refusals used
    here come from the argument checks at the top of the entry points: nothing is launched and no device is looked for."""
    import torch
    from posendf_amd import engine
    assert engine.stream_handle(torch.device("cpu")) == 0
    from posendf_amd.body_model import BodyModel
    assert BodyModel._stream(torch.device("cpu")) == 0          # the same function under the name tests/test_image_fitting_gpu.py calls
    w = engine.DenoiseWeights(1.0, 2, 1.0, 0.0)
    nine = (None,) * 9
    # S = 0 with Adam step 0: pndf_denoise_update_w checks the step before it treats S == 0 as the header's no-op
    with pytest.raises(engine.PndfError, match=r"pndf_denoise_update_w failed \(-1\)") as e:
        engine.denoise_update_w(*nine, 0, 3, w, 0, 0.02, 0, lib)
    assert type(e.value) is engine.PndfError and isinstance(e.value, RuntimeError)
    engine.denoise_update_w(*nine, 0, 3, w, 1, 0.02, 0, lib)          # S = 0 alone: a no-op, not an error
    with pytest.raises(engine.PndfError, match=r"pndf_denoise_update_w failed \(-1\)"):
        engine.denoise_update_w(*nine, 0, 3, engine.DenoiseWeights(1.0, 3, 1.0, 0.0), 1, 0.02, 0, lib)      # prior_power 1 or 2
    with pytest.raises(engine.PndfError, match="pndf_aa2quat failed"):
        engine.aa2quat(None, None, -1, 0, lib)
    with pytest.raises(engine.PndfError, match="pndf_keypoint_project failed"):
        engine.keypoint_project(None, None, None, -1, 1, engine.Camera(), None, None, 0, lib)
    with pytest.raises(engine.PndfError, match="pndf_keypoint_terms_grad failed"):
        engine.keypoint_terms_grad(None, None, None, None, None, -1, 1, engine.Camera(), engine.KeypointOpts(), None, None, None, None, 0, lib)
    with pytest.raises(engine.PndfError, match=r"pndf_quat_topk failed .*k <= min\(K, 16\)"):
        engine.quat_topk(None, None, 1, 4, 0, None, 17, None, None, 0, lib)


def test_kernel_only_entry_points_refuse_host_tensors(lib, monkeypatch):
    """pndf_quat_topk, pndf_keypoint_project and pndf_debug_project_timing have no host twin and check their pointers for null
    and alignment only: their drivers refuse a host device themselves, before the library is reached."""
    import torch
    from posendf_amd import dist_utils, engine, image_fitting

    def reached(*a, **k):
        raise AssertionError("the library was reached with host pointers")
    monkeypatch.setattr(dist_utils, "quat_topk", reached)
    monkeypatch.setattr(image_fitting, "keypoint_project", reached)
    q = torch.zeros(1, 21, 4)
    q[..., 0] = 1
    for cls in (dist_utils.geo, dist_utils.euc):
        with pytest.raises(engine.PndfError, match="pndf_quat_topk runs on the HIP kernel only"):
            cls(1, "cpu").dist_calc(q, q[:, None].repeat(1, 4, 1, 1), 4, 2)
    with pytest.raises(engine.PndfError, match="pndf_keypoint_project runs on the HIP kernel only"):
        image_fitting.project(torch.zeros(1, 24, 3), torch.zeros(1, 3), torch.zeros(1, 3), image_fitting.PerspectiveCamera())
    eng = engine.Engine.__new__(engine.Engine)      # no device needed: the refusal comes before the handle is used
    eng.lib = lib
    monkeypatch.setattr(lib, "pndf_debug_timing_regions", reached, raising=False)
    with pytest.raises(engine.PndfError, match="pndf_debug_project_timing runs on the HIP kernel only"):
        eng.project_timing(q.reshape(1, 84))


# ---- the error channel (csrc/pndf_error.h): one slot per handle family and thread for refusals without a handle, the handle's own
# text otherwise.  Codes and texts below are the ones the library gave before the five copies of the channel became one.
_LAST_ERROR = {"engine": "pndf_last_error", "train": "pndf_train_last_error", "knn": "pndf_knn_last_error",
               "lbs": "pndf_lbs_last_error", "cpu": "pndf_cpu_last_error"}


def _refused_creates(lib):
    """family -> [(call, code, text)]: creates refused by an argument check, before any device is looked for"""
    from posendf_amd.engine import PndfConfig
    h = ctypes.c_void_p()
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), 1, 100.0)
    shallow = PndfConfig()
    lib.pndf_default_config(ctypes.byref(shallow), 1, 100.0)
    shallow.n_dims = 2
    noenc = PndfConfig()
    lib.pndf_default_config(ctypes.byref(noenc), 1, 100.0)
    noenc.dims[0] = 84
    keep = (h, cfg, shallow, noenc)      # (the closures below hold the ctypes objects alive)
    return {
        "engine": [(lambda: lib.pndf_create(None, ctypes.byref(cfg), 0), -1, b"out is null", keep),
                   (lambda: lib.pndf_create(ctypes.byref(h), ctypes.byref(shallow), 0), -4,
                    b"DFNet depth: n_dims must be 3 .. 9 (1 .. 7 hidden layers + the output layer)", keep)],
        "train": [(lambda: lib.pndf_train_create(ctypes.byref(h), ctypes.byref(noenc), 0), -4,
                   b"training needs the structure encoder (model.StrEnc.use: True, dims[0] = 126): the reference's train=True "
                   b"branch cannot run without it either (man_pose_in is unbound)", keep)],
        "knn": [(lambda: lib.pndf_knn_create(ctypes.byref(h), None, 1, 2, None, None), -4, b"metric: 0 = geo or 1 = euc", keep)],
        "lbs": [(lambda: lib.pndf_lbs_create(ctypes.byref(h), 0, 0, *([None] * 8), 0, 0), -1, b"V < 1", keep)],
        "cpu": [(lambda: lib.pndf_cpu_create(ctypes.byref(h), None), -1, b"null argument", keep)],
    }


def _null_slots(lib):
    return {fam: getattr(lib, fn)(None) for fam, fn in _LAST_ERROR.items()}


def test_refused_creates_keep_their_codes_texts_and_slots(lib):
    """Every family's refusal gives the pinned code and text in its OWN null-handle slot and leaves the other four slots as
    they were (a failed pndf_knn_create does not change what pndf_last_error(NULL) returns)."""
    cases = _refused_creates(lib)
    assert set(cases) == set(_LAST_ERROR)
    for fam in cases:      # give every slot a text of its own first, so "unchanged" means something
        for call, _, _, _ in cases[fam]:
            call()
    for fam, calls in cases.items():
        for call, code, text, _ in calls:
            before = _null_slots(lib)
            assert call() == code, fam
            after = _null_slots(lib)
            assert after[fam] == text, (fam, after[fam])
            for other in _LAST_ERROR:
                if other != fam:
                    assert after[other] == before[other], (fam, other)


def test_null_handle_slots_are_per_thread(lib):
    import threading
    cases = _refused_creates(lib)
    for fam, calls in cases.items():
        calls[0][0]()
        mine = _null_slots(lib)
        seen = {}

        def other_thread():
            seen["before"] = _null_slots(lib)[fam]
            seen["code"] = calls[-1][0]()
            seen["after"] = _null_slots(lib)[fam]
        # (engine: the other thread's refusal has another text than this thread's, so a shared slot would show)
        t = threading.Thread(target=other_thread)
        t.start()
        t.join()
        assert seen["before"] == b"", (fam, seen)      # a fresh thread starts with empty slots
        assert seen["code"] < 0 and seen["after"] != b""
        assert _null_slots(lib) == mine, fam


def test_handle_errors_stay_on_the_handle(lib):
    """A compute call on a pndf_cpu handle before pndf_cpu_load_weights: the text is the handle's, the null slot is untouched."""
    from posendf_amd.engine import PndfConfig
    lib.pndf_cpu_create(ctypes.byref(ctypes.c_void_p()), None)
    null_before = lib.pndf_cpu_last_error(None)
    assert null_before == b"null argument"
    cfg = PndfConfig()
    lib.pndf_default_config(ctypes.byref(cfg), 1, 100.0)
    h = ctypes.c_void_p()
    assert lib.pndf_cpu_create(ctypes.byref(h), ctypes.byref(cfg)) == 0 and h.value
    try:
        assert lib.pndf_cpu_last_error(h) == b""
        q = np.zeros((1, 84), np.float32)
        d = np.zeros(1, np.float32)
        assert lib.pndf_forward_cpu(h, q.ctypes.data, d.ctypes.data, 1) == -5      # PNDF_ERR_NO_WEIGHTS
        assert lib.pndf_cpu_last_error(h) == b"pndf_cpu_load_weights has not been called"
        assert lib.pndf_cpu_last_error(None) == null_before
    finally:
        lib.pndf_cpu_destroy(h)


def test_stateless_calls_return_the_named_codes(lib):
    """pndf_quat_topk with k > K is PNDF_ERR_BAD_ARG (-1) and pndf_aa2quat with N = 0 is PNDF_OK (0): both return before any
    device is looked for.  (test_stream_handle_and_checked_wrappers reaches the drivers' own checks, not these.)"""
    assert lib.pndf_quat_topk(None, None, 1, 4, 0, None, 5, None, None, None) == -1
    assert lib.pndf_aa2quat(None, None, 0, None) == 0
