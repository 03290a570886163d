"""CPU: the owning types of the host code (csrc/common.hpp, bodies in csrc/device_owned.cpp: DeviceBuffer, Event, Stream,
Pinned) under AddressSanitizer + UndefinedBehaviorSanitizer, over stand-ins of the HIP calls that count live objects: growth
frees the old block once, a move leaves one owner, release() twice is harmless, a borrower never frees or grows its lender's
resource, a failed allocation leaves an empty buffer and a status, nothing is copyable, nothing is alive at exit."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_owning_types_are_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers (type definitions only)")
    exe = str(tmp_path / "device_owned_san")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                            "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "helpers", "device_owned_san_main.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    assert "failures 0" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
