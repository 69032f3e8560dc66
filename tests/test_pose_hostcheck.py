"""The host side of the pose unit under AddressSanitizer and UBSan, on the CPU: csrc/radegs_pose_check.cpp (a program with its own main)
is built together with csrc/radegs_pose.hip, host code instrumented, and run.  It calls radegs_pose_gradient / radegs_pose_step with every
argument they refuse -- the refusals come before the first HIP call, so no GPU is needed or touched -- and rg_pose.h's row term, retraction
and camera elements on heap arrays of exactly the documented sizes."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_host_code_is_clean_under_the_sanitizers(tmp_path):
    spec = importlib.util.spec_from_file_location("radegs_build_for_pose_check", os.path.join(ROOT, "rade-gs_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    hipcc = os.environ.get("HIPCC", "hipcc")
    if not shutil.which(hipcc):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path / "radegs_pose_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
    cmd = [hipcc] + build.FLAGS + ["-O1", "-g"] + san + [os.path.join(build.CSRC, "radegs_pose.hip"), os.path.join(build.CSRC, "radegs_pose_check.cpp"),
                                                        "-fsanitize=address,undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the HIP runtime's own start-up allocations are not this project's: leak detection off, everything else on
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "radegs_pose_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
