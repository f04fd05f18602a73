"""CPU: the layout of the packed-parameter handle (csrc/vs_weights_layout.h) - where every parameter
tensor and every kernel-layout image lies in the handle's two device allocations, as a pure function of the model's shape and of
the three image sizes only the kernels know.  tests/cabi/weights_layout_demo.cpp includes that header alone and is built with the
host C++17 compiler under AddressSanitizer and UBSan.  Its oracle is the code the header replaced, restated as straight-line code:
the two `take` sequences and the optimizer's 16-way switch.  Over d_model x layers x in_features x classes x with / without a
positional table every offset of both blobs and both totals are equal, the tensor table equals the switch entry by entry, the matrix
table has the five [N, K] shapes, and every range lies inside its blob and overlaps no other."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_weights_layout_as_plain_cxx17_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "weights_layout_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "cabi", "weights_layout_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout == "OK\n", (run.stdout, run.stderr[-2000:])
