#!/usr/bin/env python3
"""One line per device kernel of a library: sha256 of its disassembly (mnemonics, operands and encodings; load addresses removed), read
from the embedded gfx950 code objects the way tools/isa_table.py reads them (no GPU needed).  Two builds whose lines are equal run the
same device code.
usage: python tools/isa_hashes.py library.so [library.so ...] > profiles/<change>/isa_hashes_<build>.txt"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    """{kernel name: (instructions, sha256)} of every kernel descriptor's function in `lib`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], check=True, capture_output=True, cwd=tmp)
        for name in sorted(os.listdir(tmp)):
            if "amdgcn" not in name:
                continue
            co = os.path.join(tmp, name)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            names = set(re.findall(r"\.name:\s+(\S+)", notes))
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <([\w.$]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M):
                if m.group(1) in names:
                    body = re.sub(r"// [0-9A-Fa-f]+:", "//", m.group(2))      # the instruction's own address
                    out[m.group(1)] = (body.count("\n"), hashlib.sha256(body.encode()).hexdigest())
    return out


def main():
    for lib in sys.argv[1:]:
        print(f"# {os.path.basename(lib)}")
        for name, (n, digest) in sorted(kernels(lib).items()):
            print(f"{name:52s} {n:7d} {digest}")


if __name__ == "__main__":
    main()
