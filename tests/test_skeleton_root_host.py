"""The host twin's root-trajectory path (pndf_project_ex_cpu with a pndf_project_options9) as a stand-alone host program:
tests/host/skeleton_root_check.cpp is built with csrc/pndf_cpu.cpp in one command -- no HIP, no library -- and runs a 15-joint hand with 20
keypoints seen by one camera, three tracks of five frames with the roots coupled along the track and drawn towards an anchor: the reduction
to the 224-byte call, chained one-step calls against two and three steps (both parities of the root buffer), the translation against a
hand-written step, equal roots, a held rotation and two refusals.  The same command with -fsanitize=address,undefined is the sanitizer run of
the twin (profiles/skeleton_root/host_check_san.txt); here it is built without one.  No GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skeleton_root_check_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "skeleton_root_check"
    cc = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", os.path.join(REPO, "tests", "host", "skeleton_root_check.cpp"),
                         os.path.join(REPO, "posendf_amd", "csrc", "pndf_cpu.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("skeleton_root_check: ok") and "FAIL" not in run.stdout
