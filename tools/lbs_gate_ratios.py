#!/usr/bin/env python3
"""profiles/lbs_gates/ratios.json from the printed lines of the marginal gates (tests/lbs_gates.py):

  python -m pytest tests/test_lbs_range_gpu.py tests/test_lbs_gpu.py -m gpu -s > gpu.log        (one MI355X)
  python -m pytest tests/test_lbs_range.py -s -k "sharp or sound" > cpu.log                      (no GPU)
  python tools/lbs_gate_ratios.py gpu.log cpu.log > profiles/lbs_gates/ratios.json

`[lbs_gate <what>] <kind> <ratio> ...` lines become {entry_point, arithmetic, case, kind, ratio}; `[lbs_gate mutant, halves
<rule>] <contraction> without <product>: <result> <ratio> ...` lines become the sharpness table."""
import json
import re
import sys

ENTRY = (("joints_of", "joints_of"), ("verts + joints", None), ("verts", "forward vertices"), ("Jtr", "forward Jtr"))


def gate_row(what, kind, ratio):
    arithmetic = next((p for p in ("f16x3", "fp32") if f" {p} " in f" {what} "), None)
    case = " ".join(w for w in what.split() if w != arithmetic)
    if what.startswith("ninth draw") or what.startswith("split oracle"):
        entry, arithmetic = "reference arithmetic (CPU)", arithmetic or "f16x3"
    elif "general reverse" in what:
        entry = "general reverse (autograd)"
    elif "grad" in what:
        entry = "terms_grad"
    else:
        entry = next(name for tail, name in ENTRY if name and what.endswith(tail))
    return {"entry_point": entry, "arithmetic": arithmetic, "case": case, "kind": kind, "ratio": ratio}


def main(paths):
    gates, mutants = [], []
    for path in paths:
        for line in open(path, errors="replace"):
            for m in re.finditer(r"\[lbs_gate mutant, halves ([a-z ]+)\] (.+?) without (lo hi|hi lo): (.*)", line):
                figures = {k.strip(): float(v) for k, v in re.findall(r"([a-z][a-z ]*?) ([0-9.e+-]+|inf|nan)(?:  |$)", m.group(4).strip())}
                mutants.append({"halves": m.group(1), "contraction": m.group(2).strip(), "without": m.group(3), **figures})
            for m in re.finditer(r"\[lbs_gate (?!mutant)(.+?)\] (.+?)  \(error / bound", line):
                for kind, v in re.findall(r"(\w+) ([0-9.e+-]+|inf|nan)", m.group(2)):
                    gates.append(gate_row(m.group(1), kind, float(v)))
    worst = {}
    for g in gates:
        key = f"{g['entry_point']} | {g['arithmetic']} | {g['kind']}"
        worst[key] = max(worst.get(key, 0.0), g["ratio"])
    json.dump({"what": "worst error / bound of the marginal gates of tests/lbs_gates.py (1 = at the gate): bound = 8 x the reference "
                       "arithmetic's own error over eight perturbed draws + 2^-22 x the marginal's largest fp64 entry",
               "worst_per_entry_point_arithmetic_kind": dict(sorted(worst.items())), "gates": gates, "cpu_sharpness_mutants": mutants},
              sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main(sys.argv[1:])
