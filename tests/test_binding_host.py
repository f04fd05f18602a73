"""CPU (no GPU): the Python layer's one calling convention - the binding table against the headers, the marshalling
helpers of ``_call.py``, the decoded format word and the one packed-scoring rule."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

from conftest import ROOT


def _prototypes():
    """{header name: {symbol: (return kind, argument count)}} of include/*.h"""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = open(path).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
        text = text.replace('extern "C" {', "")
        while re.search(r"\{[^{}]*\}", text):                   # struct / enum bodies
            text = re.sub(r"\{[^{}]*\}", "", text)
        protos = {}
        for stmt in text.split(";"):
            m = re.match(r"^(.*?)\b(vs_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt.strip(), flags=re.S)
            if not m or "typedef" in m.group(1):
                continue
            ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
            assert "(" not in args, (name, args)                 # no function-pointer arguments: a comma is an argument
            if "*" in ret:
                kind = "pointer"
            else:
                kind = {"int": "int", "size_t": "size_t", "uint32_t": "uint32", "float": "float", "void": "void"}[ret]
            protos[name] = (kind, 0 if args in ("", "void") else args.count(",") + 1)
        out[os.path.basename(path)] = protos
    return out


class _Recorder:
    """Stands in for the loaded library: every attribute is a function object that records ``restype`` / ``argtypes``."""

    class _Fn:
        def __init__(self, abi):
            self._abi = abi

        def __call__(self, *args):
            return self._abi

    def __init__(self, abi):
        self._abi, self.fns = abi, {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.fns.setdefault(name, _Recorder._Fn(self._abi))


_KIND = {C.c_int: "int", C.c_size_t: "size_t", C.c_uint32: "uint32", C.c_float: "float", C.c_char_p: "pointer", C.c_void_p: "pointer",
         None: "void"}


def test_binding_table_matches_the_prototypes_of_every_header(vsa):
    """Every declared symbol is bound and every bound symbol declared, header by header, with the same argument count
    and the same kind of return value.  (A wrong ``argtypes`` does not fail at run time: it truncates a pointer.)"""
    L = vsa._lib
    declared = _prototypes()
    assert set(declared) == set(L._BINDINGS), set(declared) ^ set(L._BINDINGS)
    lib = _Recorder(L.ABI_VERSION)
    L._bind(lib)                                                 # what load() does to the real library
    n = 0
    for header, protos in declared.items():
        assert set(protos) == set(L._BINDINGS[header]), (header, set(protos) ^ set(L._BINDINGS[header]))
        for name, (kind, nargs) in protos.items():
            fn = lib.fns[name]
            assert _KIND[fn.restype] == kind, (name, fn.restype, kind)
            assert len(fn.argtypes) == nargs, (name, len(fn.argtypes), nargs)
            n += 1
    assert n == 114 and len(lib.fns) == n
    assert lib.fns["vs_abi_version"].argtypes == [] and lib.fns["vs_last_error"].argtypes == []
    # the per-header export tuples are the table's keys
    assert L.EXPORTS == tuple(L._BINDINGS["vs_scorer.h"]) and L.TRAIN_EXPORTS == tuple(L._BINDINGS["vs_train.h"])
    assert sum(len(t) for t in (L.EXPORTS, L.EVAL_EXPORTS, L.EVAL_DEVICE_EXPORTS, L.SUMMARY_EXPORTS, L.BATCH_EXPORTS, L.TRAIN_EXPORTS,
                                L.SEGMENT_EXPORTS, L.OPTIM_EXPORTS, L.INSPECT_EXPORTS)) == n


def test_bind_refuses_a_missing_symbol_and_a_stale_abi(vsa):
    L = vsa._lib

    class Partial(_Recorder):
        def __getattr__(self, name):
            if name == "vs_summarize":
                raise AttributeError(name)
            return _Recorder.__getattr__(self, name)

    with pytest.raises(RuntimeError, match=r"lacks symbol vs_summarize \(stale build\?\)"):
        L._bind(Partial(L.ABI_VERSION))
    with pytest.raises(RuntimeError, match=r"ABI %d != binding ABI %d" % (L.ABI_VERSION - 1, L.ABI_VERSION)):
        L._bind(_Recorder(L.ABI_VERSION - 1))


def test_mask_u8(vsa):
    mask_u8 = vsa._call.mask_u8
    assert mask_u8(None) is None
    truth = torch.tensor([[True, False, True, True], [False, False, True, False]])
    for m in (truth, truth.to(torch.uint8), truth.float() * 3.0, truth.to(torch.int64)):
        out = mask_u8(m)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == m.shape
        assert torch.equal(out != 0, truth)
    assert mask_u8(truth).data_ptr() == truth.data_ptr()                      # a bool mask is viewed, not copied
    wide = torch.zeros(2, 8, dtype=torch.bool)
    wide[:, ::2] = truth
    part = wide[:, ::2]                                                        # a non-contiguous slice
    assert not part.is_contiguous()
    out = mask_u8(part)
    assert out.dtype == torch.uint8 and out.is_contiguous() and torch.equal(out != 0, truth)


def test_host_lengths_and_scratch(vsa):
    call = vsa._call
    lengths, host = call.host_lengths((3, torch.tensor(65), 130.0))
    assert lengths == [3, 65, 130] and all(type(t) is int for t in lengths)
    assert isinstance(host, C.Array) and host._type_ is C.c_int32 and list(host) == lengths
    lengths, host = call.host_lengths([])
    assert lengths == [] and len(host) == 0
    ws = call.scratch(1000, "cpu")
    assert ws.dtype == torch.uint8 and ws.shape == (1000,) and ws.device.type == "cpu"
    assert call.scratch(0, "cpu").numel() == 0
    assert call.scratch(0, "cpu", floor=256).numel() == 256 and call.scratch(300, "cpu", floor=256).numel() == 300
    assert call.ptr(None) is None and call.ptr(ws) == ws.data_ptr()


def test_train_form_decodes_the_bits_of_the_header(vsa):
    """include/vs_train.h (vs_train_last_format): bit 0 16-bit Linear / dgrad / wgrad products, bit 1 16-bit attention
    products, bits 2..4 which tensors of the record are 16-bit planes (q/k/v; MLP hidden; written by the A-stationary
    GEMM), bit 5 the 16-bit type is fp16; bit 31 only says that the word is valid."""
    fields = ("lp", "lpa", "qkv16", "h16", "rows16", "f16")
    assert vsa._lib.TrainForm._fields == fields
    for word in range(64):
        for valid in (0, 0x80000000):
            form = vsa._lib.train_form(word | valid)
            for bit, name in enumerate(fields):
                assert getattr(form, name) is bool(word & (1 << bit)), (word, name)
            assert form.dtype(form.lp or form.lpa) == (("fp16" if word & 32 else "bf16") if word & 3 else "fp32")
            assert form.dtype(form.lpa) == (("fp16" if word & 32 else "bf16") if word & 2 else "fp32")


def test_packed_scorer_rule(vsa):
    """Packed scoring: the model has ``score_packed`` and its head dim - the library's, for an embedded model - is 32, 64
    or 128.  The models are constructed and never run."""
    packed_scorer = vsa.corpus.packed_scorer
    assert callable(packed_scorer(vsa.SimNet(num_heads=2, d_model=256, num_layers=1, use_pos=False)))       # head dim 128
    assert packed_scorer(vsa.SimNet(num_heads=1, d_model=256, num_layers=1, use_pos=False)) is None         # head dim 256
    embedded = vsa.SimNet(num_heads=5, d_model=100, num_layers=1, use_pos=False)                            # head dim 20, embedded
    assert embedded._plan == (320, 64) and embedded._lib_dh == 64          # the library's head dim is read, not d_model // num_heads = 20
    assert callable(packed_scorer(embedded))

    class Plain:
        d_model, num_heads = 256, 4

    assert packed_scorer(Plain()) is None                                                    # no score_packed

    class Foreign(Plain):                                                                    # no _lib_dh: d_model // num_heads
        def score_packed(self, x, lengths):
            return ("scored", x, lengths)

    fn = packed_scorer(Foreign())
    assert fn("x", [1, 2]) == ("scored", "x", [1, 2])
    Foreign.num_heads = 1
    assert packed_scorer(Foreign()) is None
