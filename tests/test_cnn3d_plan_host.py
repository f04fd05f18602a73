"""CPU: the R3D-18 plan (csrc/vs_cnn3d_plan.h).  tests/cabi/cnn3d_plan_demo.cpp includes that header alone and
is built with the host C++17 compiler under AddressSanitizer and UBSan as a stand-alone program.  For (1,1,1,1), (1,5,17,15),
(2,9,23,31) and (1,16,112,112) and both input kinds it walks every record's gather and store addresses over the whole padded tile
grid with the functions the kernel calls; the per-record output sizes it prints are compared here with torch's own conv3d."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

SHAPES = ((1, 1, 1, 1), (1, 5, 17, 15), (2, 9, 23, 31), (1, 16, 112, 112))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("cnn3d_plan") / "cnn3d_plan_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cabi", "cnn3d_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def _torch_sizes(t, h, w):
    """[(cout, to, ho, wo)] of the 20 convs in execution order, by torch's own conv3d on a one-channel tensor"""
    def conv(x, k, s, p):
        return F.conv3d(x, torch.zeros((1, 1) + k), None, s, p)

    out = []
    x = conv(torch.zeros(1, 1, t, h, w), (3, 7, 7), (1, 2, 2), (1, 3, 3))
    out.append((64,) + tuple(x.shape[2:]))
    for layer, planes in enumerate((64, 128, 256, 512)):
        for block in range(2):
            s = 2 if layer > 0 and block == 0 else 1
            y = conv(x, (3, 3, 3), s, 1)
            out.append((planes,) + tuple(y.shape[2:]))
            if s == 2:
                d = conv(x, (1, 1, 1), 2, 0)
                assert d.shape == y.shape
                out.append((planes,) + tuple(d.shape[2:]))
            x = conv(y, (3, 3, 3), 1, 1)
            out.append((planes,) + tuple(x.shape[2:]))
    return out


def test_cnn3d_plan_addresses_and_sizes_under_sanitizers(demo):
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([demo] + args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.endswith("OK\n"), (run.stdout[-500:], run.stderr[-2000:])
    got, cur = {}, None
    for line in run.stdout.split("\n"):
        f = line.split()
        if f and f[0] == "shape":
            cur = got.setdefault(tuple(int(v) for v in f[1:]), [])
        elif f and f[0] == "conv":
            cur.append(tuple(int(v) for v in f[1:]))
    assert len(got) == len(SHAPES) * 2                              # both input kinds
    for (n, t, h, w, kind), convs in got.items():
        assert convs == _torch_sizes(t, h, w), ((n, t, h, w, kind), convs)


def test_cnn3d_plan_header_has_no_hip_include():
    text = open(os.path.join(ROOT, "video-summarization_amd", "csrc", "vs_cnn3d_plan.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
