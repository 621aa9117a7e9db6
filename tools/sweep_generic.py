#!/usr/bin/env python3
"""Randomised architectures through the runtime-planned kernels (csrc/pndf_generic.hip), both forms (precision fp32 / f16x3), against the
numpy oracle with the gates of tests/test_depth.py's extremes test: depth 1 .. 7, widths 1 .. 1024 (biased towards tile / group / pass
edges), the three activations, with and without the encoder, and the weight regime ((gain, output bias) of tests/depth_range.py REGIMES,
drawn per network from a stream of its own: the architectures of a seed are those of earlier sweeps).
usage: python tools/sweep_generic.py [n_networks] [seed] [rescale pattern]
`rescale pattern`: a name of depth_range.DECIMAL or depth_range.POW2 ("zigzag", "tiny", "uniform+24", ...): the hidden layers of every
relu-family network are rescaled by it (the same function, other magnitudes; Softplus networks run as drawn).
Prints one line per network and a summary; exit code 1 on any failure."""
import os
import sys
import traceback

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import depth_range as dr  # noqa: E402
import test_depth as td  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2026
pattern = sys.argv[3] if len(sys.argv) > 3 else None
if pattern is not None and pattern not in dr.DECIMAL and pattern not in dr.POW2:
    sys.exit(f"rescale pattern {pattern!r}: one of {list(dr.DECIMAL) + list(dr.POW2)}")
rng = np.random.default_rng(seed)
rng_w = np.random.default_rng([seed, 1])
EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 767, 768, 896, 1000, 1023, 1024]
fails = 0
for i in range(n):
    depth = int(rng.integers(1, 8))
    hidden = [int(rng.choice(EDGES)) if rng.random() < 0.6 else int(rng.integers(1, 1025)) for _ in range(depth)]
    if depth == 6 and all(w <= a for w, a in zip(hidden, (256, 512, 1024, 512, 256, 64))):
        hidden[2] = 1024 + 0 * hidden[2] if hidden[0] > 256 else hidden[2]
        hidden[0] = 257                     # (six hidden widths within amass.yaml's run on the FUSED kernels: not this sweep's subject)
    act = str(rng.choice(["lrelu", "relu", "softplus"]))
    enc = bool(rng.random() < 0.7)
    gain, bias = dr.REGIMES[int(rng_w.integers(len(dr.REGIMES)))]
    what = f"[{i}] {hidden} {act} enc={enc} gain {gain} bias {bias}"
    try:
        sd = td.live_weights((126 if enc else 84, *hidden, 1), act, gain, bias)
    except AssertionError:
        print(f"{what}: no live weight set (dead network), skipped", flush=True)
        continue
    if pattern is not None and act != "softplus":
        what += f" {pattern}"
        sd = dr.rescaled(sd, dr.decimal_pattern(pattern, depth) if pattern in dr.DECIMAL else dr.pow2_pattern(pattern, depth))
    for precision in ("fp32", "f16x3"):
        try:
            kernel = td._check_against_oracle(hidden, act, enc, precision, sd)
            assert kernel == td.generic_kernel(act, enc, precision), kernel
            print(f"{what} {precision}: ok", flush=True)
        except Exception as exc:      # noqa: BLE001
            fails += 1
            print(f"{what} {precision}: FAIL {type(exc).__name__}: {str(exc)[:300]}", flush=True)
            traceback.print_exc(limit=2)
print(f"sweep_generic: {fails} failure(s)")
sys.exit(1 if fails else 0)
