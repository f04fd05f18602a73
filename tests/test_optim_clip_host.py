"""CPU (no GPU): the surface of gradient-norm clipping (include/vs_optim.h: vs_grad_norm*, vs_grad_scale_tensors;
video-summarization_amd/optim.py: Adam(max_grad_norm=...), clip_grad_norm_, grad_norm).  Every C call below must be
refused BEFORE any device access: the pointers are fake."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

FAKE = 0x7F0000001000          # never dereferenced: every case is refused by the argument checks


def _table(L, sizes, ptr=FAKE):
    tab = (L.GradTensor * len(sizes))()
    for e, n in zip(tab, sizes):
        e.g, e.n = ptr, n
    return tab


def test_workspace_bytes_of_a_table(vsa):
    lib, L = vsa._lib.load(), vsa._lib
    tab = _table(L, [1, 4096, 4097, 100000])
    need = lib.vs_grad_norm_workspace_bytes(tab, 4)
    chunks = 1 + 1 + 2 + 25
    assert need > 0 and need % 256 == 0 and need >= 8 * chunks
    assert lib.vs_grad_norm_workspace_bytes(tab, 1) == 256                   # one double, rounded up
    big = _table(L, [3000 * 4096])
    assert lib.vs_grad_norm_workspace_bytes(big, 1) == 3000 * 8 + (-(3000 * 8)) % 256
    # skipped entries (NULL pointer or no elements) need nothing, and an empty table is valid: still non-zero
    skip = _table(L, [0, 77])
    skip[1].g = None
    assert lib.vs_grad_norm_workspace_bytes(skip, 2) == 256
    assert lib.vs_grad_norm_workspace_bytes(tab, 0) == 256
    # invalid input: 0
    assert lib.vs_grad_norm_workspace_bytes(None, 4) == 0
    assert lib.vs_grad_norm_workspace_bytes(tab, -1) == 0
    assert lib.vs_grad_norm_workspace_bytes(_table(L, [5, 2 ** 32]), 2) == 0


def test_norm_argument_checks_need_no_gpu(vsa):
    lib, L = vsa._lib.load(), vsa._lib
    tab = _table(L, [5, 4097])
    need = lib.vs_grad_norm_workspace_bytes(tab, 2)

    def norm(table=tab, n=2, kind=L.VS_GRAD_NORM_L2, max_norm=1.0, out=FAKE, ws=FAKE + 4096, nbytes=need):
        return lib.vs_grad_norm_tensors(table, n, kind, max_norm, None, out, ws, nbytes, None)

    for kw, word in ((dict(table=None), b"table"), (dict(out=None), b"out"), (dict(ws=None), b"workspace"), (dict(n=-1), b"n_tensors"),
                     (dict(max_norm=float("nan")), b"max_norm"), (dict(max_norm=0.0), b"max_norm"), (dict(max_norm=-1.0), b"max_norm"),
                     (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"), (dict(ws=FAKE + 4096 + 4), b"aligned"),
                     (dict(table=_table(L, [5, 2 ** 32])), b"2^32")):
        assert norm(**kw) == L.VS_ERR_INVALID, kw
        assert word in lib.vs_last_error(), (kw, lib.vs_last_error())
    assert norm(nbytes=need - 1) == L.VS_ERR_WORKSPACE
    assert b"workspace" in lib.vs_last_error()
    assert norm(nbytes=0) == L.VS_ERR_WORKSPACE
    # the handle form and the in-place scale
    grads = L.ModelGrads()
    assert lib.vs_grad_norm(None, C.byref(grads), 0, 1.0, None, FAKE, FAKE + 4096, need, None) == L.VS_ERR_INVALID
    assert b"NULL" in lib.vs_last_error()
    assert lib.vs_grad_norm(FAKE, None, 0, 1.0, None, FAKE, FAKE + 4096, need, None) == L.VS_ERR_INVALID
    assert lib.vs_grad_scale_tensors(None, 2, FAKE, None) == L.VS_ERR_INVALID
    assert b"table" in lib.vs_last_error()
    assert lib.vs_grad_scale_tensors(tab, 2, None, None) == L.VS_ERR_INVALID
    assert b"coef" in lib.vs_last_error()
    assert lib.vs_grad_scale_tensors(tab, -3, FAKE, None) == L.VS_ERR_INVALID
    assert lib.vs_grad_scale_tensors(_table(L, [2 ** 32]), 1, FAKE, None) == L.VS_ERR_INVALID
    assert b"2^32" in lib.vs_last_error()


def test_the_c_client_compiles():
    gcc = shutil.which("gcc")
    assert gcc, "gcc not found"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([gcc, "-std=gnu99", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "cabi", "clip_demo.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_constructor_contract_of_clipping(vsa):
    w = torch.nn.Parameter(torch.zeros(5, 3))
    for cls in (vsa.Adam, vsa.AdamW):
        opt = cls([w])
        assert opt.max_grad_norm is None and opt.grad_norm_type == 2.0 and opt.last_grad_norm is None
        opt = cls([w], max_grad_norm=1.5, grad_norm_type=float("inf"))
        assert opt.max_grad_norm == 1.5 and opt.grad_norm_type == float("inf")
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="max_norm"):
                cls([w], max_grad_norm=bad)
        for bad in (1.0, 3, 0.0, "2", None):
            with pytest.raises(ValueError, match="norm_type"):
                cls([w], max_grad_norm=1.0, grad_norm_type=bad)
        with pytest.raises(ValueError, match="norm_type"):
            cls([w], grad_norm_type=1.0)                         # refused even while clipping is off
        with pytest.raises(TypeError):
            cls([w], 1e-3, (0.9, 0.999), 1e-8, 0, False, 1.0)   # keyword only
    assert vsa.Adam([w], max_grad_norm=float("inf")).max_grad_norm == float("inf")       # measure only
    assert vsa.clip_grad_norm_ is vsa.optim.clip_grad_norm_ and vsa.grad_norm is vsa.optim.grad_norm


def test_clipping_is_not_in_the_state_dict_and_it_loads_into_torch_adam(vsa):
    ps = [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))]
    opt = vsa.Adam(ps, lr=1e-4, weight_decay=1e-5, max_grad_norm=1.0)
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd["param_groups"][0] and "grad_norm_type" not in sd["param_groups"][0]
    assert "max_grad_norm" not in opt.defaults and "grad_norm_type" not in opt.defaults
    theirs = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1.0)
    assert set(sd["param_groups"][0]) == set(theirs.state_dict()["param_groups"][0])
    theirs.load_state_dict(sd)
    assert theirs.param_groups[0]["lr"] == 1e-4 and theirs.param_groups[0]["weight_decay"] == 1e-5
    assert "max_grad_norm" not in theirs.param_groups[0]
    # and back: loading leaves the clipping attributes of the receiving optimizer alone
    opt.load_state_dict(theirs.state_dict())
    assert opt.max_grad_norm == 1.0 and opt.grad_norm_type == 2.0
    opt.max_grad_norm = 0.5                                      # may be rewritten between steps
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]


def test_cpu_parameters_are_refused_by_a_clipping_step(vsa):
    w = torch.nn.Parameter(torch.ones(4))
    opt = vsa.Adam([w], lr=0.1, max_grad_norm=1.0)
    w.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="HIP"):
        opt.step()
    assert torch.equal(w.detach(), torch.ones(4)) and torch.equal(w.grad, torch.ones(4)) and len(opt.state) == 0
    opt.max_grad_norm = -2.0                                     # a bad rewrite is caught by the step, before anything runs
    with pytest.raises(ValueError, match="max_norm"):
        opt.step()


def test_free_functions_refuse_what_they_cannot_do(vsa):
    w = torch.nn.Parameter(torch.ones(4, 4))
    w.grad = torch.full((4, 4), 2.0)
    for fn in (lambda p: vsa.clip_grad_norm_(p, 1.0), vsa.grad_norm):
        with pytest.raises(RuntimeError, match="HIP"):
            fn([w])
        with pytest.raises(RuntimeError, match="HIP"):
            fn(w)                                                # a single tensor, as torch accepts
    assert torch.equal(w.grad, torch.full((4, 4), 2.0))         # nothing was scaled anywhere
    with pytest.raises(ValueError, match="error_if_nonfinite"):
        vsa.clip_grad_norm_([w], 1.0, error_if_nonfinite=True)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            vsa.clip_grad_norm_([w], bad)
    for bad in (1.0, 0.5, "inf"):
        with pytest.raises(ValueError, match="norm_type"):
            vsa.clip_grad_norm_([w], 1.0, norm_type=bad)
        with pytest.raises(ValueError, match="norm_type"):
            vsa.grad_norm([w], norm_type=bad)
    # no gradients at all: torch's answer, a zero
    assert float(vsa.clip_grad_norm_([torch.nn.Parameter(torch.ones(3))], 1.0)) == 0.0
    assert float(vsa.grad_norm([])) == 0.0
