"""CPU: which Linear kernel a launcher starts (csrc/vs_linear_pick.h) - the kernel family, the template tuple
and the launch geometry as a pure function of the epilogue, the shape, the mode word, the weight copy and VS_SKINNY_ROWS.
tests/cabi/linear_pick_demo.cpp includes that header alone and is built with the host C++17 compiler under AddressSanitizer and
UBSan: a table of named cases gives the expected pick at every deciding shape and reaches every family and template tuple, every
refusal is refused, and over a grid the pick is total, names only instantiations that exist - and each of them - and its grids
cover the output."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_linear_pick_as_plain_cxx17_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "linear_pick_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "cabi", "linear_pick_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout == "OK\n", (run.stdout, run.stderr[-2000:])
