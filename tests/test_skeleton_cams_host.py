"""The host twin's moving-camera path (pndf_project_ex_cpu with a pndf_project_options10) as a stand-alone host program:
tests/host/skeleton_cams_check.cpp is built with csrc/pndf_cpu.cpp in one command -- no HIP, no library -- and runs a 15-joint hand with 20
keypoints seen by two cameras, three tracks of five frames: the reduction to the static call per pose and per frame, the table per frame
against the path repeated per track, chained one-step calls against two and three steps in both layouts, skipped views and two refusals.
The same command with -fsanitize=address,undefined is the sanitizer run of the twin (profiles/skeleton_cams/host_check_san.txt); here it is
built without one.  No GPU.  Fails on the parent commit, whose header has no pndf_project_options10."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skeleton_cams_check_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "skeleton_cams_check"
    cc = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", os.path.join(REPO, "tests", "host", "skeleton_cams_check.cpp"),
                         os.path.join(REPO, "posendf_amd", "csrc", "pndf_cpu.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("skeleton_cams_check: ok") and "FAIL" not in run.stdout
