"""GPU: a training loop through the C ABI from a plain C program (tests/cabi/optim_demo.c) - forward, loss, backward and
vs_adam_step(params = NULL) on the handle's own copy of the parameters; no Python or torch in the process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_c_training_loop_through_the_c_abi(vsa, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    pkg = os.path.join(ROOT, "video-summarization_amd")
    exe = str(tmp_path / "optim_demo")
    build = subprocess.run([gcc, "-std=gnu99", "-O2", os.path.join(ROOT, "tests", "cabi", "optim_demo.c"),
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                            "-L" + pkg, "-lvsscore", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                            "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lm", "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    runs = []
    for _ in range(2):
        run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith("OK"), (run.stdout, run.stderr[-2000:])
        runs.append(run.stdout)
    assert runs[0] == runs[1]                                       # identical bits, run to run
    words = runs[0].split("\n")[1:]
    losses = np.array([int(w_, 16) for w_ in words if w_], dtype=np.uint32).view(np.float32)
    print(runs[0].split("\n")[0], losses)
    assert len(losses) == 26 and np.all(np.isfinite(losses))
    assert losses[24] < losses[0]                                   # strictly lower after the 24 steps than at the start
    assert losses[25] == losses[24]                                 # the step with found_inf raised changed nothing
