"""CPU: the opt-in 16-bit attention of packed ragged training (VS_TRAIN_FLAG_PACKED_LP_ATTENTION) as far as it needs no GPU -
the new symbols and the flag, the argument checks of the two per-kernel entry points (VS_ERR_INVALID / VS_ERR_WORKSPACE with a
message, before any device access), the scratch size, and SimNet.set_train_dtype(..., packed_attention=True)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

LENGTHS = [129, 1, 64, 257, 33, 128, 63, 2, 65, 31, 127, 32]


@pytest.fixture(scope="module")
def L(vsa):
    vsa._lib.build()
    return vsa._lib


def _i32(values):
    return (C.c_int32 * len(values))(*values)


def _host_block(nbytes):
    """a 256-byte aligned address inside a host buffer the test keeps alive: the checks must return before reading it"""
    buf = C.create_string_buffer(nbytes + 256)
    return buf, (C.addressof(buf) + 255) // 256 * 256


def test_symbols_and_flag_exist(L):
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "vs_train.h")).read()
    assert re.search(r"#define\s+VS_TRAIN_FLAG_PACKED_LP_ATTENTION\s+8u", hdr)
    assert L.VS_TRAIN_FLAG_PACKED_LP_ATTENTION == 8
    for name in ("vs_train_attention_packed_lp_scratch_bytes", "vs_train_attention_forward_packed_lp",
                 "vs_train_attention_backward_packed_lp"):
        assert name in L.TRAIN_EXPORTS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, hdr), name


def _plan_floats(B, nwork):
    return (2 * (B + 1) + 2 * nwork + 63) // 64 * 64


@pytest.mark.parametrize("lengths,H", [(LENGTHS, 2), ([129], 4), ([1], 1), ([32, 33], 8)])
def test_scratch_bytes_hold_plan_delta_and_both_keep_word_copies(L, lengths, H):
    lib = L.load()
    words = sum(t * ((t + 31) // 32) for t in lengths)
    nwork = sum((t + 127) // 128 for t in lengths)
    r = lambda n: (n + 63) // 64 * 64      # noqa: E731  256-byte granules, in floats
    want = 4 * (_plan_floats(len(lengths), nwork) + r(H * sum(lengths)) + r(2 * H * words))
    got = lib.vs_train_attention_packed_lp_scratch_bytes(_i32(lengths), len(lengths), H)
    assert got == want and got % 256 == 0
    # ... the exact entry points' scratch (plan + delta) plus the keep words
    assert got == lib.vs_train_attention_packed_scratch_bytes(_i32(lengths), len(lengths), H) + 4 * r(2 * H * words)


def test_scratch_bytes_are_zero_on_invalid_input(L):
    lib = L.load()
    assert lib.vs_train_attention_packed_lp_scratch_bytes(_i32([10, 0]), 2, 2) == 0
    assert lib.vs_train_attention_packed_lp_scratch_bytes(_i32([10]), 1, 0) == 0
    assert lib.vs_train_attention_packed_lp_scratch_bytes(_i32([10]), 0, 2) == 0
    assert lib.vs_train_attention_packed_lp_scratch_bytes(None, 1, 2) == 0


def _call(L, which, lengths=(129, 33), H=2, dh=64, p=0.3, null=None, scratch_bytes=None, short=False):
    """one entry point on host addresses (never dereferenced when a check fires); null: index of the pointer set to NULL"""
    lib = L.load()
    lengths = list(lengths)
    B = len(lengths)
    need = max(lib.vs_train_attention_packed_lp_scratch_bytes(_i32([max(t, 1) for t in lengths]), B, max(H, 1)), 256)
    keep, addr = _host_block(need)
    ptrs = [addr] * (5 if which == "forward" else 7)
    host, dev, scratch = _i32(lengths), addr, addr
    if null is not None:
        if null < len(ptrs):
            ptrs[null] = None
        elif null == len(ptrs):
            host = None
        elif null == len(ptrs) + 1:
            dev = None
        else:
            scratch = None
    nbytes = need if scratch_bytes is None else scratch_bytes
    fn = lib.vs_train_attention_forward_packed_lp if which == "forward" else lib.vs_train_attention_backward_packed_lp
    rc = fn(*ptrs, host, dev, B, H, dh, 0.0625, 1, 7, p, 0, scratch, nbytes - (64 if short else 0), None)
    del keep
    return rc, lib.vs_last_error()


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_entry_points_reject_bad_arguments_before_touching_a_device(L, which):
    rc, msg = _call(L, which, dh=256)
    assert rc == L.VS_ERR_INVALID and b"head dim 256" in msg, msg
    rc, msg = _call(L, which, dh=48)
    assert rc == L.VS_ERR_INVALID and b"head dim 48" in msg, msg
    rc, msg = _call(L, which, H=0)
    assert rc == L.VS_ERR_INVALID and b"H=0" in msg, msg
    rc, msg = _call(L, which, lengths=(129, 0))
    assert rc == L.VS_ERR_INVALID and b"lengths[1]=0" in msg, msg
    rc, msg = _call(L, which, p=1.0)
    assert rc == L.VS_ERR_INVALID and b"dropout" in msg, msg
    n = 5 if which == "forward" else 7
    for null in range(n + 3):          # q, k, v, out, (d_out, lse2,) ..., then lengths, lengths_dev, scratch
        rc, msg = _call(L, which, null=null)
        assert rc == L.VS_ERR_INVALID and b"NULL" in msg, (null, msg)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_entry_points_reject_a_short_scratch(L, which):
    rc, msg = _call(L, which, short=True)
    assert rc == L.VS_ERR_WORKSPACE and b"scratch" in msg, msg
    # the exact entry points' size (no keep words) is too small for these
    small = L.load().vs_train_attention_packed_scratch_bytes(_i32([129, 33]), 2, 2)
    rc, msg = _call(L, which, scratch_bytes=small)
    assert rc == L.VS_ERR_WORKSPACE and b"scratch" in msg, msg


def test_set_train_dtype_keyword(vsa):
    m = vsa.SimNet(num_heads=4, d_model=256, num_layers=1)
    assert m.set_train_dtype("bf16", packed_attention=True) is m
    flags = m._train_flags(packed=True)
    assert flags == (vsa._lib.VS_TRAIN_FLAG_BF16_LINEAR | vsa._lib.VS_TRAIN_FLAG_BF16_ATTENTION | vsa._lib.VS_TRAIN_FLAG_PACKED_LP_ATTENTION)
    assert m._train_flags() == flags & ~vsa._lib.VS_TRAIN_FLAG_PACKED_LP_ATTENTION        # padded calls never carry the bit
    assert m.set_train_dtype("fp16", packed_attention=True)._train_flags(packed=True) == flags | vsa._lib.VS_TRAIN_FLAG_FP16
    assert m.set_train_dtype("bf16")._train_flags(packed=True) == flags & ~vsa._lib.VS_TRAIN_FLAG_PACKED_LP_ATTENTION     # the default: as before
    assert m.set_train_dtype("fp32", packed_attention=True)._train_flags(packed=True) == 0      # no effect with fp32
    assert m.last_packed_attention_dtype == "fp32"
    with pytest.raises(AttributeError):
        m.last_packed_attention_dtype = "bf16"
    with pytest.raises(ValueError, match="train dtype must be"):
        m.set_train_dtype("int8")
    with pytest.raises(ValueError, match="train dtype must be"):
        m.set_train_dtype("int8", packed_attention=True)


def test_set_train_dtype_keyword_needs_a_16_bit_head_dim(vsa):
    m = vsa.SimNet(num_heads=1, d_model=256, num_layers=1)          # head dim 256: exact attention only
    with pytest.raises(ValueError, match="attention needs head_dim in"):
        m.set_train_dtype("bf16", packed_attention=True)
    assert m._train_flags(packed=True) == 0                          # ... and the failed call changed nothing
    m.set_train_dtype("bf16")                                        # without the keyword: as before
    m.set_train_dtype("fp32", packed_attention=True)                 # fp32: the keyword has no effect, so nothing to reject
