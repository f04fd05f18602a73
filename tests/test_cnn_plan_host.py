"""CPU: the GoogLeNet front end's plan (csrc/vs_cnn_plan.h).  tests/cabi/cnn_plan_demo.cpp includes that header
alone and is built with the host C++17 compiler under AddressSanitizer and UBSan as a stand-alone program.  For 17x15, 33x47, 64x80,
224x224 and 224x398 with N = 1, 3 and 5 it walks every layer's gather and store addresses with the functions the kernel calls and
asserts that they are inside their buffers and that no live buffer is overwritten; the per-layer output sizes it prints are compared
here with a table made by torch's own layers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
import googlenet_ref

SHAPES = ((17, 15), (33, 47), (64, 80), (224, 224), (224, 398))
BATCHES = (1, 3, 5)


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("cnn_plan") / "cnn_plan_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cabi", "cnn_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def test_cnn_plan_addresses_and_sizes_under_sanitizers(demo):
    args = [str(v) for n in BATCHES for h, w in SHAPES for v in (n, h, w)]
    run = subprocess.run([demo] + args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.endswith("OK\n"), (run.stdout[-500:], run.stderr[-2000:])
    got, cur = {}, None
    for line in run.stdout.split("\n"):
        f = line.split()
        if f and f[0] == "shape":
            cur = got.setdefault(tuple(int(v) for v in f[1:]), [])
        elif f and f[0] == "layer":
            cur.append(tuple(int(v) for v in f[1:]))
    assert len(got) == len(BATCHES) * len(SHAPES) * 2               # both input kinds
    for (n, h, w, kind), layers in got.items():
        want = [(c, hh, ww) for _, c, hh, ww in googlenet_ref.layer_sizes(h, w)] + [(1024, 1, 1)]
        assert layers == want, ((n, h, w, kind), layers, want)


def test_cnn_plan_header_has_no_hip_include():
    text = open(os.path.join(ROOT, "video-summarization_amd", "csrc", "vs_cnn_plan.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
