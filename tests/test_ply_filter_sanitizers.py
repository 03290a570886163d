"""CPU: lcgs_ply_filter_rows (csrc/host/ply.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program:
records of 1, 7 and 248 bytes, 0 / 1 / 4096 / 9001 rows (the copy works in blocks of 4096), keep-all / none / every other row --
the output is the header with the new count followed by the kept records, byte for byte -- and every refusal (ascii, a wrong row
count, a truncated payload or header, an element after `vertex`, missing files, NULL arguments) returns its status and leaves no
output file; nothing reads or writes out of bounds, nothing leaks."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_ply_filter_rows_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the HIP headers (type definitions only)")
    exe = str(tmp_path / "ply_filter_san")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "helpers", "ply_filter_san_main.cpp"),
                            "-o", exe, "-lpthread"], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-2000:]
    work = tmp_path / "files"
    work.mkdir()
    run = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "failures 0" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
