"""GPU: one clipped optimizer step through the C ABI from a plain C program (tests/cabi/clip_demo.c) - vs_grad_norm, then
vs_adam_step with out + 2 as its grad_scale - against the Python path (Adam(max_grad_norm=...)) on the same numbers.
Both run the same kernels on the same inputs in the same tensor order, so the comparison is bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from adam_ref import ulp32
from conftest import ROOT

pytestmark = pytest.mark.gpu
D, L, DIN, PROBE = 128, 1, 1024, 54321


def _hval(tensor, n):
    """clip_demo.c: hval(tensor, i) for i < n"""
    with np.errstate(over="ignore"):
        h = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32((tensor * 40503 + 12345) & 0xFFFFFFFF)
        h ^= h >> np.uint32(15)
        h *= np.uint32(2246822519)
        h ^= h >> np.uint32(13)
        h *= np.uint32(3266489917)
        h ^= h >> np.uint32(16)
    return (h >> np.uint32(8)).astype(np.float32) / np.float32(8388608.0) - np.float32(1.0)


def test_plain_c_clipped_step_equals_the_python_path(vsa, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    pkg = os.path.join(ROOT, "video-summarization_amd")
    exe = str(tmp_path / "clip_demo")
    build = subprocess.run([gcc, "-std=gnu99", "-O2", os.path.join(ROOT, "tests", "cabi", "clip_demo.c"),
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                            "-L" + pkg, "-lvsscore", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                            "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-lm", "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK"), (run.stdout, run.stderr[-2000:])
    words = [w_ for w_ in run.stdout.split("\n")[1:] if w_]
    c_norm, c_coef, c_div, c_probe, c_coef1, c_div1, c_g0 = np.array([int(w_, 16) for w_ in words], dtype=np.uint32).view(np.float32)
    print(run.stdout.split("\n")[0])

    dev = torch.device("cuda:0")
    model = vsa.SimNet(num_heads=2, d_model=D, num_layers=L, sparsity=0.0, dropout=0.0, use_pos=False).to(dev)
    params = [t for t in model._tensors() if isinstance(t, torch.nn.Parameter)]        # vs_model_params order
    assert len(params) == 4 + 16 * L
    g64 = []
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(torch.from_numpy(_hval(i, p.numel()) * np.float32(0.125)).view(p.shape))
            g = _hval(100 + i, p.numel()) * np.float32(16.0)
            p.grad = torch.from_numpy(g).view(p.shape).to(dev)
            g64.append(g.astype(np.float64))
    opt = vsa.Adam(params, lr=1e-3, weight_decay=1e-5, max_grad_norm=1.0)
    opt.grad_scale = torch.full((), 1024.0, device=dev)          # what torch.amp.GradScaler.step sets for the call
    opt.step()
    del opt.grad_scale
    norm = opt.last_grad_norm.cpu().numpy()
    assert norm.tobytes() == np.float32(c_norm).tobytes(), (float(norm), float(c_norm))
    probe = params[0].detach().view(-1)[PROBE].cpu().numpy()
    assert probe.tobytes() == np.float32(c_probe).tobytes(), (float(probe), float(c_probe))
    # and the C numbers are the right ones: the float64 norm to one fp32 spacing, torch's coefficient, the untouched scale
    norm64 = np.sqrt(sum(float(np.dot(g, g)) for g in g64)) / 1024.0
    coef64, div64 = 1.0 / (norm64 + 1e-6), 1024.0 * (norm64 + 1e-6)
    assert abs(float(c_norm) - norm64) <= ulp32(norm64)
    assert abs(float(c_coef) - coef64) <= ulp32(coef64) and abs(float(c_div) - div64) <= ulp32(div64)
    assert c_coef1 == 1.0 and c_div1 == 1024.0
    assert c_g0 == _hval(100, 1)[0] * np.float32(16.0)
