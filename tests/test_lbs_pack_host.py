"""The body model's host-only layer (posendf_amd/csrc/pndf_lbs_pack.h: packers, picked-joint table, fp16 conversion) as a
stand-alone host program: tests/host/lbs_pack_check.cpp includes that header alone -- no HIP, no library -- and checks it on
three synthetic models.  No GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lbs_pack_host_check_program(tmp_path):
    """Compiled as plain C++17 by the compiler that builds the library's host-only translation unit (hipcc -x c++, no device
    pass: it is the one compiler every build of this tree has, and unlike older g++ it knows `_Float16`, which the program holds
    f32_to_f16 against), without sanitizer flags; the program exits 0 after one line that names what it checked."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "lbs_pack_check"
    cc = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "posendf_amd", "csrc"),
                         os.path.join(REPO, "tests", "host", "lbs_pack_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("lbs_pack_check: ok") and "FAIL" not in run.stdout
