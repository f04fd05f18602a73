"""CPU (no GPU): the GoogLeNet pool5 front end's host side - the key and shape table against the architecture, the reference's
``model.<i>`` names, the checkpoint head strip, the C ABI's argument checks and binding table, the header as C99, no CPU path."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
import googlenet_ref

# the architecture table: block -> (in, c1, c3r, c3, c5r, c5, pp, out)
ARCH = {"inception3a": (192, 64, 96, 128, 16, 32, 32, 256), "inception3b": (256, 128, 128, 192, 32, 96, 64, 480),
        "inception4a": (480, 192, 96, 208, 16, 48, 64, 512), "inception4b": (512, 160, 112, 224, 24, 64, 64, 512),
        "inception4c": (512, 128, 128, 256, 24, 64, 64, 512), "inception4d": (512, 112, 144, 288, 32, 64, 64, 528),
        "inception4e": (528, 256, 160, 320, 32, 128, 128, 832), "inception5a": (832, 256, 160, 320, 32, 128, 128, 832),
        "inception5b": (832, 384, 192, 384, 48, 128, 128, 1024)}
HEADER = os.path.join(ROOT, "include", "features", "vs_features.h")


def _expected_shapes():
    out = {}

    def basic(prefix, cin, cout, k):
        out[prefix + ".conv.weight"] = (cout, cin, k, k)
        for f in ("weight", "bias", "running_mean", "running_var"):
            out[prefix + ".bn." + f] = (cout,)
        out[prefix + ".bn.num_batches_tracked"] = ()

    basic("conv1", 3, 64, 7)
    basic("conv2", 64, 64, 1)
    basic("conv3", 64, 192, 3)
    prev = 192
    for name, (cin, c1, c3r, c3, c5r, c5, pp, cout) in ARCH.items():
        assert cin == prev and c1 + c3 + c5 + pp == cout            # the table is consistent with itself
        prev = cout
        basic(name + ".branch1", cin, c1, 1)
        basic(name + ".branch2.0", cin, c3r, 1)
        basic(name + ".branch2.1", c3r, c3, 3)
        basic(name + ".branch3.0", cin, c5r, 1)
        basic(name + ".branch3.1", c5r, c5, 3)
        basic(name + ".branch4.1", cin, pp, 1)
    return out


def test_key_and_shape_table_is_the_architecture(vsa):
    f = vsa.features
    want = _expected_shapes()
    assert dict(f.state_dict_shapes()) == want and len(want) == 57 * 6
    model = f.GoogLeNetFeatures()
    sd = model.state_dict()
    assert list(sd) == list(f.state_dict_shapes())
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(f.conv_table()) == vsa._lib.VS_CNN_NUM_CONVS == 57
    for prefix, cout, cin, k, stride, pad in f.conv_table():
        m = model.get_submodule(prefix)
        assert m.conv.stride == (stride, stride) and m.conv.padding == (pad, pad) and m.conv.bias is None and m.bn.eps == 0.001
    seeded = f.make_state_dict(5)
    assert {k: tuple(v.shape) for k, v in seeded.items()} == want
    assert all(torch.equal(a, b) for a, b in zip(seeded.values(), f.make_state_dict(5).values()))
    for k, v in seeded.items():
        if k.endswith("bn.weight") or k.endswith("running_var"):
            assert 0.5 <= v.min() and v.max() <= 1.5
    model.load_state_dict(seeded, strict=True)
    # the float64 restatement runs on these keys (17 x 15: the smallest shape of the suite)
    out = googlenet_ref.forward(googlenet_ref.cast(seeded, torch.float64), torch.zeros(1, 3, 17, 15, dtype=torch.float64))
    assert out.shape == (1, 1024) and torch.isfinite(out).all()


def test_sequential_names_round_trip_and_load(vsa):
    f = vsa.features
    sd = f.make_state_dict(2)
    seq = f.to_sequential_names(sd)
    assert "model.0.conv.weight" in seq and "model.5.branch4.1.bn.running_var" in seq and "model.15.branch1.conv.weight" in seq
    assert "model.8.branch2.0.conv.weight" in seq and seq["model.8.branch2.0.conv.weight"].shape == (96, 480, 1, 1)      # inception4a
    assert not any(k.startswith(("model.1.", "model.4.", "model.7.", "model.13.", "model.16.")) for k in seq)               # the pools
    back = f.from_sequential_names(seq)
    assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
    a, b = f.GoogLeNetFeatures(), f.GoogLeNetFeatures()
    a.load_state_dict(sd, strict=True)
    b.load_state_dict(seq, strict=True)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert f.SEQUENTIAL_NAMES[5] == "inception3a" and f.SEQUENTIAL_NAMES[13] == "maxpool4" and len(f.SEQUENTIAL_NAMES) == 17


def test_strip_torchvision_head(vsa):
    f = vsa.features
    sd = f.make_state_dict(3)
    full = dict(sd)
    full.update({"fc.weight": torch.zeros(1000, 1024), "fc.bias": torch.zeros(1000), "aux1.conv.conv.weight": torch.zeros(128, 512, 1, 1),
                 "aux2.fc2.bias": torch.zeros(1000)})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        f.GoogLeNetFeatures().load_state_dict(full, strict=True)
    stripped = f.strip_torchvision_head(full)
    assert list(stripped) == list(sd)
    f.GoogLeNetFeatures().load_state_dict(stripped, strict=True)


def test_c_abi_argument_checks_need_no_gpu(vsa):
    L = vsa._lib
    lib = L.load()
    INV = L.VS_ERR_INVALID
    assert lib.vs_cnn_min_side() == 15
    assert lib.vs_cnn_workspace_bytes(1, 15, 17) > 0 and lib.vs_cnn_workspace_bytes(2, 17, 15) > 0      # torch accepts them
    for n, h, w in ((0, 224, 224), (-1, 224, 224), (1, 14, 224), (1, 224, 14), (1, 0, 0)):
        assert lib.vs_cnn_workspace_bytes(n, h, w) == 0
        assert b"cnn" in lib.vs_last_error()
    one = lib.vs_cnn_workspace_bytes(1, 224, 224)
    assert lib.vs_cnn_workspace_bytes(64, 224, 224) <= 64 * one + 64 * 256 and lib.vs_cnn_workspace_bytes(64, 224, 224) > 32 * one
    handle = C.c_void_p()
    assert lib.vs_cnn_pack(None, None, C.byref(handle)) == INV
    P = L.CnnParams()
    assert lib.vs_cnn_pack(C.byref(P), None, None) == INV
    assert lib.vs_cnn_pack(C.byref(P), None, C.byref(handle)) == INV and b"NULL tensor" in lib.vs_last_error()      # no tensor set
    lib.vs_cnn_free(None)
    fake = 4096                                                     # non-NULL stand-ins: every check below fails before any is read
    assert lib.vs_cnn_forward(None, fake, 0, 1, 224, 224, fake, fake, 1 << 30, None) == INV
    assert lib.vs_cnn_forward(fake, None, 0, 1, 224, 224, fake, fake, 1 << 30, None) == INV
    assert lib.vs_cnn_forward(fake, fake, 0, 1, 224, 224, None, fake, 1 << 30, None) == INV
    assert lib.vs_cnn_forward(fake, fake, 0, 1, 224, 224, fake, None, 1 << 30, None) == INV
    assert lib.vs_cnn_forward(fake, fake, 2, 1, 224, 224, fake, fake, 1 << 30, None) == INV and b"input_kind" in lib.vs_last_error()
    assert lib.vs_cnn_forward(fake, fake, 0, 0, 224, 224, fake, fake, 1 << 30, None) == INV
    assert lib.vs_cnn_forward(fake, fake, 1, 1, 14, 224, fake, fake, 1 << 30, None) == INV and b"smallest" in lib.vs_last_error()
    assert lib.vs_cnn_forward(fake, fake, 0, 1, 224, 224, fake, fake, one - 1, None) == INV and b"workspace" in lib.vs_last_error()
    assert lib.vs_cnn_forward(fake, fake, 0, 1, 224, 224, fake, fake + 16, one, None) == INV and b"aligned" in lib.vs_last_error()
    assert lib.vs_cnn_packed_floats(64, 3, 7) == 64 * 160 + 64 and lib.vs_cnn_packed_floats(24, 512, 1) == 64 * 512 + 64
    assert lib.vs_cnn_packed_floats(0, 3, 7) == 0
    assert lib.vs_cnn_conv(None, 2, 1, 8, 8, 4, fake, 4, 1, 1, 0, fake, 0, 4, None) == INV
    assert lib.vs_cnn_conv(fake, 1, 1, 8, 8, 4, fake, 4, 1, 1, 0, fake, 0, 4, None) == INV and b"3 channels" in lib.vs_last_error()
    assert lib.vs_cnn_conv(fake, 2, 1, 8, 8, 4, fake, 4, 1, 1, 0, fake, 2, 4, None) == INV and b"outside a row" in lib.vs_last_error()
    assert lib.vs_cnn_conv(fake, 2, 1, 2, 2, 4, fake, 4, 7, 1, 0, fake, 0, 4, None) == INV and b"no output" in lib.vs_last_error()
    assert lib.vs_cnn_maxpool(None, 1, 8, 8, 4, 3, 2, 0, 1, fake, None) == INV
    assert lib.vs_cnn_maxpool(fake, 1, 8, 8, 6, 3, 2, 0, 1, fake, None) == INV                      # channels not a multiple of 4
    assert lib.vs_cnn_maxpool(fake, 1, 8, 8, 4, 3, 2, 2, 1, fake, None) == INV                      # pad above k / 2
    assert lib.vs_cnn_maxpool(fake, 1, 1, 8, 4, 3, 2, 0, 1, fake, None) == INV                      # no output row


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    text = text.replace('extern "C" {', "")
    while re.search(r"\{[^{}]*\}", text):
        text = re.sub(r"\{[^{}]*\}", "", text)
    out = {}
    for stmt in text.split(";"):
        m = re.match(r"^(.*?)\b(vs_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt.strip(), flags=re.S)
        if not m or "typedef" in m.group(1):
            continue
        ret, args = " ".join(m.group(1).split()), m.group(3).strip()
        out[m.group(2)] = (ret, 0 if args in ("", "void") else args.count(",") + 1)
    return out


def test_binding_table_matches_the_header_and_the_library_exports_it(vsa):
    L = vsa._lib
    protos = _prototypes(open(HEADER).read())
    assert set(protos) == set(L._FEATURES_BINDINGS) == set(L.FEATURES_EXPORTS)
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "int32_t": C.c_int32, "void": None}
    for name, (ret, nargs) in protos.items():
        restype, argtypes = L._FEATURES_BINDINGS[name]
        assert kinds[ret] is restype and len(argtypes) == nargs, name
    lib = L.load()
    for name in protos:
        assert hasattr(lib, name), name
    for src in ("vs_cnn.hip", "vs_cnn.cpp"):
        assert src in L.SOURCES
    # the constants of the header
    text = open(HEADER).read()
    for name in ("VS_CNN_INPUT_F32_NCHW", "VS_CNN_INPUT_U8_NHWC", "VS_CNN_INPUT_F32_NHWC", "VS_CNN_NUM_CONVS", "VS_CNN_FEATURES"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(L, name)
    assert C.sizeof(L.CnnParams) == 57 * 5 * C.sizeof(C.c_void_p)

    class Partial:                      # a stale library: no quiet fall-back, load() refuses it
        def __getattr__(self, name):
            if name == "vs_cnn_forward":
                raise AttributeError(name)
            return lambda *a: 0

    with pytest.raises(RuntimeError, match=r"lacks symbol vs_cnn_forward \(stale build\?\)"):
        L._bind_features(Partial())


def test_header_is_plain_c99():
    gcc = shutil.which("gcc")
    assert gcc
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_a_cpu_tensor_raises(vsa):
    model = vsa.GoogLeNetFeatures()
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.extract(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="model= or weights="):
        vsa.get_google_net_features(torch.zeros(1, 32, 32, 3, dtype=torch.uint8).numpy())
    assert model.train().training and "running statistics" in vsa.features.__doc__
