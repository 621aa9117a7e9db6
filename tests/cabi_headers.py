"""What tests/test_cabi.py reads out of the headers of include/ and out of the two libraries (a helper, not a test module)."""
import os
import re
import subprocess

from conftest import REPO

_DECLARATION = re.compile(r"((?:const\s+)?\b[A-Za-z_][A-Za-z0-9_]*(?:\s*\*)?)\s*\b(pndf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def header_text(header, comments=True):
    """the header's text; comments=False: comments and preprocessor lines stripped"""
    text = open(os.path.join(REPO, "include", header)).read()
    if comments:
        return text
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return "\n".join(ln for ln in re.sub(r"//[^\n]*", " ", text).splitlines() if not ln.lstrip().startswith("#"))


def prototypes(header):
    """{name: (return type, parameter count)} of every `pndf_*(...);` declaration, comments stripped"""
    protos = {}
    for ret, name, params in _DECLARATION.findall(header_text(header, comments=False)):
        assert name not in protos, f"{name} declared twice"
        params = params.strip()
        protos[name] = (" ".join(ret.replace("*", " * ").split()), 0 if params in ("", "void") else params.count(",") + 1)
    return protos


def called(text):
    """every name that stands in front of a `(` in `text`, declared or merely mentioned"""
    return set(re.findall(r"\b(pndf_[a-z0-9_]+)\s*\(", text))


def exported_symbols(path):
    """the defined dynamic symbols of a shared library (`nm -D --defined-only`)"""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def compiles_as_c99(tmp_path, source):
    """gcc's verdict on `source` as strict C99 with include/ on the path: (ok, diagnostics)"""
    src = tmp_path / "use_header.c"
    src.write_text(source)
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    return r.returncode == 0, r.stderr
