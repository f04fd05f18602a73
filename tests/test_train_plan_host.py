"""CPU: the training path's plan (csrc/vs_train_plan.h) - the form of a call's activation record and the mode
word of every launch that reads or writes it, as a pure function of the model's shape, the call, the dropout config and the
switches.  tests/cabi/train_plan_demo.cpp includes that header alone and is built with the host C++17 compiler under
AddressSanitizer and UBSan: a table of named cases gives the expected plan and reaches every attention kernel and every mode-word
value, each switch flips exactly the fields DESIGN.md section 10 names, over a grid of shapes, flags, switches, call forms and
directions the plan's invariants hold, every form word a backward can be handed is accepted or refused by the documented rule, and
every argument refusal has its text and its place in the order."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_train_plan_as_plain_cxx17_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path / "train_plan_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            "-I" + os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "cabi", "train_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout == "OK\n", (run.stdout, run.stderr[-2000:])
