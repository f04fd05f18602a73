"""CPU (no GPU): the surface of the native Adam step (include/vs_optim.h, video-summarization_amd/optim.py) and the
float64 yardstick the GPU tests measure against (tests/adam_ref.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from adam_ref import adam_ref64, distances, ulp32
from conftest import ROOT


def test_optim_header_symbols_are_declared_listed_and_exported(vsa):
    vsa._lib.build()
    lib = vsa._lib.load()
    hdr = open(os.path.join(ROOT, "include", "vs_optim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vs_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(vsa._lib.OPTIM_EXPORTS), declared ^ set(vsa._lib.OPTIM_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert "vs_optim.hip" in vsa._lib.SOURCES
    assert int(re.search(r"#define VS_ADAM_MAX_TENSORS (\d+)", hdr).group(1)) == vsa._lib.VS_ADAM_MAX_TENSORS


def test_optim_header_is_plain_c99_and_the_c_client_compiles():
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    inc = os.path.join(ROOT, "include")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "vs_optim.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([gcc, "-std=gnu99", "-fsyntax-only", "-I" + inc, "-I" + os.path.join(rocm, "include"),
                        "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "cabi", "optim_demo.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_optim_argument_checks_need_no_gpu(vsa):
    lib, L = vsa._lib.load(), vsa._lib
    cfg = L.AdamCfg(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
    word = C.c_uint32(0)
    tab = (L.AdamTensor * 1)()
    assert lib.vs_adam_step_tensors(tab, -1, C.byref(cfg), None, None, C.byref(word), None) == L.VS_ERR_INVALID
    assert b"n_tensors" in lib.vs_last_error()
    assert lib.vs_adam_step_tensors(None, 2, C.byref(cfg), None, None, C.byref(word), None) == L.VS_ERR_INVALID
    assert b"table" in lib.vs_last_error()
    assert lib.vs_adam_step_tensors(tab, 1, None, None, None, C.byref(word), None) == L.VS_ERR_INVALID
    assert b"cfg" in lib.vs_last_error()
    assert lib.vs_adam_step_tensors(tab, 1, C.byref(cfg), None, None, None, None) == L.VS_ERR_INVALID
    assert b"sync_word" in lib.vs_last_error()
    tab[0].n = 8                                            # elements but no pointers
    assert lib.vs_adam_step_tensors(tab, 1, C.byref(cfg), None, None, C.byref(word), None) == L.VS_ERR_INVALID
    assert b"NULL" in lib.vs_last_error()
    for bad, word_ in ((L.AdamCfg(-1.0, 0.9, 0.999, 1e-8, 0.0, 0, 0), b"lr"), (L.AdamCfg(1e-3, 1.0, 0.999, 1e-8, 0.0, 0, 0), b"beta1"),
                       (L.AdamCfg(1e-3, 0.9, -0.1, 1e-8, 0.0, 0, 0), b"beta2"), (L.AdamCfg(1e-3, 0.9, 0.999, -1.0, 0.0, 0, 0), b"eps"),
                       (L.AdamCfg(1e-3, 0.9, 0.999, 1e-8, -0.5, 0, 0), b"weight_decay"), (L.AdamCfg(1e-3, 0.9, 0.999, 1e-8, 0.0, 7, 0), b"decoupled")):
        tab[0].n = 0
        assert lib.vs_adam_step_tensors(tab, 1, C.byref(bad), None, None, C.byref(word), None) == L.VS_ERR_INVALID
        assert word_ in lib.vs_last_error()
    assert lib.vs_adam_state_bytes(None) == 0
    assert lib.vs_adam_state_init(None, None, None) == L.VS_ERR_INVALID
    off, cnt = C.c_size_t(), C.c_size_t()
    assert lib.vs_adam_state_field(None, 0, 0, C.byref(off), C.byref(cnt)) == L.VS_ERR_INVALID
    assert lib.vs_adam_step(None, None, None, None, C.byref(cfg), None, None, None) == L.VS_ERR_INVALID
    assert b"NULL" in lib.vs_last_error()
    # an empty table is a valid no-op and launches nothing
    assert lib.vs_adam_step_tensors(None, 0, C.byref(cfg), None, None, C.byref(word), None) == L.VS_OK


def test_constructor_contract(vsa):
    w = torch.nn.Parameter(torch.zeros(5, 3))
    for cls in (vsa.Adam, vsa.AdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls([w], amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls([w], maximize=True)
    with pytest.raises(ValueError, match="learning rate"):
        vsa.Adam([w], lr=-1.0)
    with pytest.raises(ValueError, match="beta"):
        vsa.Adam([w], betas=(0.9, 1.0))
    opt = vsa.Adam([w], lr=1e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["decoupled_weight_decay"]) == (1e-4, (0.8, 0.99), 1e-6, 0.01, False)
    assert vsa.AdamW([w]).param_groups[0]["decoupled_weight_decay"] is True and vsa.AdamW([w]).param_groups[0]["weight_decay"] == 1e-2
    assert issubclass(vsa.Adam, torch.optim.Optimizer) and vsa.optim.Adam is vsa.Adam
    # what makes an unmodified GradScaler.step take its non-synchronising branch
    import inspect
    assert getattr(opt, "_step_supports_amp_scaling", False) is True
    assert "grad_scaler" not in inspect.signature(opt.step).parameters


def test_cpu_parameters_are_refused_at_step_without_fallback(vsa):
    w = torch.nn.Parameter(torch.ones(4))
    opt = vsa.Adam([w], lr=0.1)
    w.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="HIP"):
        opt.step()
    assert torch.equal(w.detach(), torch.ones(4)) and len(opt.state) == 0        # nothing was computed anywhere


def test_state_dict_key_set_is_torch_adams(vsa):
    model = vsa.SimNet(num_heads=4, d_model=256, num_layers=1)
    groups = lambda: [{"params": list(model.final_layer.parameters()), "lr": 1e-3},       # noqa: E731
                      {"params": [p for n, p in model.named_parameters() if not n.startswith("final_layer")]}]
    ours, theirs = vsa.Adam(groups(), lr=1e-5, weight_decay=1e-5).state_dict(), torch.optim.Adam(groups(), lr=1e-5, weight_decay=1e-5).state_dict()
    assert set(ours) == set(theirs) and ours["state"] == theirs["state"] == {}
    assert len(ours["param_groups"]) == len(theirs["param_groups"]) == 2
    for a, b in zip(ours["param_groups"], theirs["param_groups"]):
        assert set(a) == set(b) and a["params"] == b["params"]
        assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay"))
    # a torch.optim.Adam checkpoint (CPU tensors, int-like step) loads; its tensors are re-homed by the first step
    t = torch.optim.Adam(groups(), lr=1e-5)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    t.step()
    o = vsa.Adam(groups(), lr=1e-5)
    o.load_state_dict(t.state_dict())
    assert set(o.state_dict()["state"]) == set(t.state_dict()["state"])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in o.state_dict()["state"].values())


# ---- the yardstick is itself tested -------------------------------------------------------------------------------
# Bounds, from the formats (not from any kernel): an fp32 step rounds m twice (the product and the sum of the lerp) and v
# three times (v * beta2, g * g scaled, their sum), each by at most half an ulp of a value no larger than the tensor's
# largest entry: <= 2^-24 of it per rounding.  Carried errors shrink by beta every step, so the sum over steps is at most
# roundings * 2^-24 * min(steps, 1 / (1 - beta)).  p: one storage rounding of p per step (half an ulp of |p|) plus the
# update's own error, lr-sized and far below it; the bound is one ulp of the largest |p| per step.
def _m_bound(steps, beta1):
    return 2 * 2.0 ** -24 * min(steps, 1.0 / (1.0 - beta1))


def _v_bound(steps, beta2):
    return 3 * 2.0 ** -24 * min(steps, 1.0 / (1.0 - beta2))


@pytest.mark.parametrize("impl", ["single", "foreach", "fused"])
@pytest.mark.parametrize("steps,lr,wd", [(10, 1e-3, 0.0), (50, 1e-5, 1e-5), (25, 1e-4, 1e-2)])
def test_float64_restatement_against_torch_adam_on_the_cpu(impl, steps, lr, wd):
    gen = torch.Generator().manual_seed(1000 + steps)
    n = 262147
    p0 = torch.randn(n, generator=gen) * 0.05
    scale = 10.0 ** (torch.rand(n, generator=gen) * 3 - 3)                         # gradients over three decades
    grads = [torch.randn(n, generator=gen) * scale for _ in range(steps)]
    for g in grads:
        g[::1001] = 0.0                                                            # a few exact zeros
    p = torch.nn.Parameter(p0.clone())
    kw = dict(foreach=False) if impl == "single" else dict(foreach=True) if impl == "foreach" else dict(fused=True)
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd, **kw)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    ref = adam_ref64(p0, grads, lr, weight_decay=wd)
    st = opt.state[p]
    dp, dm, dv = distances(p, st["exp_avg"], st["exp_avg_sq"], ref)
    print("torch CPU Adam (%s) vs float64: |dp| %.3e (%.2f ulp of max|p|), exp_avg %.3e, exp_avg_sq %.3e"
          % (impl, dp, dp / ulp32(p0.abs().max().item()), dm, dv))
    assert float(st["step"]) == ref[3] == steps
    assert dm <= _m_bound(steps, 0.9) and dv <= _v_bound(steps, 0.999), (dm, dv)
    assert dp <= steps * ulp32(ref[0].abs().max().item()), dp


def test_float64_restatement_adamw_and_continuation():
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(4099, generator=gen)
    grads = [torch.randn(4099, generator=gen) for _ in range(12)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.05)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    ref = adam_ref64(p0, grads, 1e-3, weight_decay=0.05, decoupled=True)
    dp, dm, dv = distances(p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ref)
    assert dm <= _m_bound(12, 0.9) and dv <= _v_bound(12, 0.999) and dp <= 12 * ulp32(ref[0].abs().max().item())
    # continuing from a state equals running through; a grad_scale divides the gradient
    half = adam_ref64(p0, grads[:5], 1e-3, weight_decay=0.05, decoupled=True)
    rest = adam_ref64(half[0], grads[5:], 1e-3, weight_decay=0.05, decoupled=True, state=half[1:])
    assert rest[3] == 12 and (rest[0] - ref[0]).abs().max().item() < 1e-15
    scaled = adam_ref64(p0, [g * 1024.0 for g in grads], 1e-3, weight_decay=0.05, decoupled=True, grad_scale=1024.0)
    assert (scaled[0] - ref[0]).abs().max().item() == 0.0
