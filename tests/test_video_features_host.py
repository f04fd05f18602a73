"""CPU (no GPU): the R3D-18 video-level feature's host side - the key and shape table against the architecture, the reference's
``model.<i>`` names, the checkpoint head strip, the C ABI's argument checks and binding table, the header as C99, no CPU path, and
the float64 restatement at the smallest shapes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
import r3d_ref

HEADER = os.path.join(ROOT, "include", "features", "vs_video_features.h")

# the architecture, written out: (prefix, cin, cout, kernel (t, h, w), stride, padding) of the 20 convs in state_dict order
ARCH = [("stem", 3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3))]
for _layer, (_cin, _planes, _stride) in enumerate(((64, 64, 1), (64, 128, 2), (128, 256, 2), (256, 512, 2)), 1):
    ARCH.append(("layer%d.0.conv1" % _layer, _cin, _planes, (3, 3, 3), (_stride,) * 3, (1, 1, 1)))
    ARCH.append(("layer%d.0.conv2" % _layer, _planes, _planes, (3, 3, 3), (1, 1, 1), (1, 1, 1)))
    if _stride == 2:
        ARCH.append(("layer%d.0.downsample" % _layer, _cin, _planes, (1, 1, 1), (2, 2, 2), (0, 0, 0)))
    ARCH.append(("layer%d.1.conv1" % _layer, _planes, _planes, (3, 3, 3), (1, 1, 1), (1, 1, 1)))
    ARCH.append(("layer%d.1.conv2" % _layer, _planes, _planes, (3, 3, 3), (1, 1, 1), (1, 1, 1)))


def _expected_shapes():
    out = {}
    for prefix, cin, cout, k, _, _ in ARCH:
        out[prefix + ".0.weight"] = (cout, cin) + k
        for f in ("weight", "bias", "running_mean", "running_var"):
            out[prefix + ".1." + f] = (cout,)
        out[prefix + ".1.num_batches_tracked"] = ()
    return out


def test_key_and_shape_table_is_the_architecture(vsa):
    f = vsa.video_features
    want = _expected_shapes()
    assert len(ARCH) == 20 and len(want) == 20 * 6
    assert dict(f.state_dict_shapes()) == want and list(f.state_dict_shapes()) == list(want)
    model = f.R3D18Features()
    sd = model.state_dict()
    assert list(sd) == list(want)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    table = f.conv_table()
    assert len(table) == vsa._lib.VS_R3D_NUM_CONVS == 20 and {row[0] for row in table} == {row[0] for row in ARCH}
    arch = {row[0]: row for row in ARCH}
    for prefix, cout, cin, (kt, ks), (st, ss), (pt, ps) in table:
        _, acin, acout, k, stride, pad = arch[prefix]
        assert (cin, cout, (kt, ks, ks), (st, ss, ss), (pt, ps, ps)) == (acin, acout, k, stride, pad), prefix
        m = model.get_submodule(prefix)
        assert m[0].kernel_size == k and m[0].stride == stride and m[0].padding == pad and m[0].bias is None and m[1].eps == 1e-5
    # execution order: a block's downsample runs before its conv2, which adds it
    names = [row[0] for row in table]
    assert names[0] == "stem" and names.index("layer2.0.downsample") == names.index("layer2.0.conv2") - 1
    seeded = f.make_state_dict(5)
    assert {k: tuple(v.shape) for k, v in seeded.items()} == want
    assert all(torch.equal(a, b) for a, b in zip(seeded.values(), f.make_state_dict(5).values()))
    for k, v in seeded.items():
        if k.endswith(".1.weight") or k.endswith("running_var"):
            assert 0.5 <= v.min() and v.max() <= 1.5
    model.load_state_dict(seeded, strict=True)


@pytest.mark.parametrize("shape", ((1, 3, 1, 1, 1), (1, 3, 5, 17, 15)), ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_accepts_every_size_from_one(vsa, shape):
    """the padding keeps every layer's output at least 1, so the plan states no smallest side"""
    sd = r3d_ref.cast(vsa.video_features.make_state_dict(5), torch.float64)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = r3d_ref.forward(sd, x)
    assert out.shape == (1, 512) and torch.isfinite(out).all() and out.abs().max() > 0
    assert vsa._lib.load().vs_r3d_workspace_bytes(shape[0], *shape[2:]) > 0


def test_sequential_names_round_trip_and_load(vsa):
    f = vsa.video_features
    sd = f.make_state_dict(2)
    seq = f.to_sequential_names(sd)
    assert "model.0.0.weight" in seq and "model.0.1.running_var" in seq and "model.4.1.conv2.1.bias" in seq
    assert seq["model.2.0.downsample.0.weight"].shape == (128, 64, 1, 1, 1) and not any(k.startswith("model.5.") for k in seq)
    back = f.from_sequential_names(seq)
    assert list(back) == list(sd) and all(back[k] is sd[k] for k in sd)
    a, b = f.R3D18Features(), f.R3D18Features()
    a.load_state_dict(sd, strict=True)
    b.load_state_dict(seq, strict=True)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert f.SEQUENTIAL_NAMES == ("stem", "layer1", "layer2", "layer3", "layer4", "avgpool")


def test_strip_torchvision_head(vsa):
    f = vsa.video_features
    sd = f.make_state_dict(3)
    full = dict(sd)
    full.update({"fc.weight": torch.zeros(400, 512), "fc.bias": torch.zeros(400)})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        f.R3D18Features().load_state_dict(full, strict=True)
    stripped = f.strip_torchvision_head(full)
    assert list(stripped) == list(sd)
    f.R3D18Features().load_state_dict(stripped, strict=True)


def test_c_abi_argument_checks_need_no_gpu(vsa):
    L = vsa._lib
    lib = L.load()
    INV = L.VS_ERR_INVALID
    assert lib.vs_r3d_workspace_bytes(1, 1, 1, 1) > 0 and lib.vs_r3d_workspace_bytes(2, 9, 23, 31) > 0
    for n, t, h, w in ((0, 16, 112, 112), (-1, 16, 112, 112), (1, 0, 112, 112), (1, 16, 0, 112), (1, 16, 112, 0), (1 << 10, 1 << 10, 64, 64)):
        assert lib.vs_r3d_workspace_bytes(n, t, h, w) == 0
        assert b"r3d" in lib.vs_last_error()
        assert lib.vs_r3d_flops(n, t, h, w) == 0.0
    one = lib.vs_r3d_workspace_bytes(1, 16, 112, 112)
    # the stem's output [16, 56, 56, 64] three times (ping, pong, conv1's) and layer2.0's downsample, a quarter of it
    assert one == 4 * (3 * 16 * 56 * 56 * 64 + 8 * 28 * 28 * 128)
    assert lib.vs_r3d_workspace_bytes(3, 16, 112, 112) == 3 * one
    # the 16 x 112 x 112 clip: 40.7 G multiply-adds (the figure usually quoted for r3d_18), two operations each
    assert 2 * 40.6e9 < lib.vs_r3d_flops(1, 16, 112, 112) < 2 * 40.8e9
    ms = (C.c_float * 6)()
    assert lib.vs_r3d_normalisation(None) == INV and lib.vs_r3d_normalisation(ms) == 0
    assert list(ms) == [torch.tensor(v, dtype=torch.float32).item() for v in r3d_ref.MEAN + r3d_ref.STD]
    handle = C.c_void_p()
    assert lib.vs_r3d_pack(None, None, C.byref(handle)) == INV
    P = L.R3dParams()
    assert lib.vs_r3d_pack(C.byref(P), None, None) == INV
    assert lib.vs_r3d_pack(C.byref(P), None, C.byref(handle)) == INV and b"NULL tensor" in lib.vs_last_error()
    lib.vs_r3d_free(None)
    fake = 4096                                                     # non-NULL stand-ins: every check below fails before any is read
    assert lib.vs_r3d_forward(None, fake, 0, 1, 16, 112, 112, fake, fake, 1 << 30, None) == INV
    assert lib.vs_r3d_forward(fake, None, 0, 1, 16, 112, 112, fake, fake, 1 << 30, None) == INV
    assert lib.vs_r3d_forward(fake, fake, 0, 1, 16, 112, 112, None, fake, 1 << 30, None) == INV
    assert lib.vs_r3d_forward(fake, fake, 0, 1, 16, 112, 112, fake, None, 1 << 30, None) == INV
    assert lib.vs_r3d_forward(fake, fake, 2, 1, 16, 112, 112, fake, fake, 1 << 30, None) == INV and b"input_kind" in lib.vs_last_error()
    assert lib.vs_r3d_forward(fake, fake, 0, 0, 16, 112, 112, fake, fake, 1 << 30, None) == INV
    assert lib.vs_r3d_forward(fake, fake, 1, 1, 0, 112, 112, fake, fake, 1 << 30, None) == INV and b"below 1" in lib.vs_last_error()
    assert lib.vs_r3d_forward(fake, fake, 0, 1, 16, 112, 112, fake, fake, one - 1, None) == INV and b"workspace" in lib.vs_last_error()
    assert lib.vs_r3d_forward(fake, fake, 0, 1, 16, 112, 112, fake, fake + 16, one, None) == INV and b"aligned" in lib.vs_last_error()
    assert lib.vs_cnn3d_packed_floats(64, 3, 3, 7) == 64 * 448 + 64 and lib.vs_cnn3d_packed_floats(128, 64, 1, 1) == 128 * 64 + 128
    assert lib.vs_cnn3d_packed_floats(512, 512, 3, 3) == 512 * 13824 + 512
    assert lib.vs_cnn3d_packed_floats(0, 3, 3, 7) == 0 and lib.vs_cnn3d_packed_floats(64, 3, 16, 7) == 0
    Q = L.Cnn3dConvParams()
    assert lib.vs_cnn3d_pack_conv(None, 64, 3, 3, 7, fake, None) == INV
    assert lib.vs_cnn3d_pack_conv(C.byref(Q), 64, 3, 3, 7, fake, None) == INV and b"NULL" in lib.vs_last_error()
    #                     input kind n  t  h  w cin packed cout kt ks st ss pt ps residual relu out stream
    assert lib.vs_cnn3d_conv(None, 2, 1, 4, 8, 8, 4, fake, 4, 1, 1, 1, 1, 0, 0, None, 0, fake, None) == INV
    assert lib.vs_cnn3d_conv(fake, 2, 1, 4, 8, 8, 4, None, 4, 1, 1, 1, 1, 0, 0, None, 0, fake, None) == INV
    assert lib.vs_cnn3d_conv(fake, 2, 1, 4, 8, 8, 4, fake, 4, 1, 1, 1, 1, 0, 0, None, 0, None, None) == INV
    assert lib.vs_cnn3d_conv(fake, 3, 1, 4, 8, 8, 4, fake, 4, 1, 1, 1, 1, 0, 0, None, 0, fake, None) == INV and b"input_kind" in lib.vs_last_error()
    assert lib.vs_cnn3d_conv(fake, 1, 1, 4, 8, 8, 4, fake, 4, 1, 1, 1, 1, 0, 0, None, 0, fake, None) == INV and b"3 channels" in lib.vs_last_error()
    assert lib.vs_cnn3d_conv(fake, 2, 1, 4, 8, 8, 4, fake, 4, 3, 3, 0, 1, 1, 1, None, 0, fake, None) == INV and b"stride" in lib.vs_last_error()
    assert lib.vs_cnn3d_conv(fake, 2, 1, 4, 8, 8, 4, fake, 4, 3, 3, 1, 1, 3, 1, None, 0, fake, None) == INV and b"pad" in lib.vs_last_error()
    assert lib.vs_cnn3d_conv(fake, 2, 1, 2, 8, 8, 4, fake, 4, 3, 3, 1, 1, 0, 1, None, 0, fake, None) == INV and b"no output" in lib.vs_last_error()
    assert lib.vs_cnn3d_conv(fake, 2, 1, 4, 2, 8, 4, fake, 4, 1, 7, 1, 1, 0, 0, None, 0, fake, None) == INV and b"no output" in lib.vs_last_error()


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
    assert set(protos) == set(L._VIDEO_FEATURES_BINDINGS) == set(L.VIDEO_FEATURES_EXPORTS)
    for name in ("vs_r3d_pack", "vs_r3d_free", "vs_r3d_workspace_bytes", "vs_r3d_forward", "vs_cnn3d_packed_floats", "vs_cnn3d_pack_conv",
                 "vs_cnn3d_conv"):
        assert name in protos
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "int32_t": C.c_int32, "double": C.c_double, "void": None}
    for name, (ret, nargs) in protos.items():
        restype, argtypes = L._VIDEO_FEATURES_BINDINGS[name]
        assert kinds[ret] is restype and len(argtypes) == nargs, name
    lib = L.load()
    for name in protos:
        assert hasattr(lib, name), name
    for src in ("vs_cnn3d.hip", "vs_cnn3d.cpp"):
        assert src in L.SOURCES
    assert not set(L._VIDEO_FEATURES_BINDINGS) & set(L._FEATURES_BINDINGS) and L.ABI_VERSION == 3
    text = open(HEADER).read()
    for name in ("VS_CNN3D_INPUT_F32_NCDHW", "VS_CNN3D_INPUT_U8_NDHWC", "VS_CNN3D_INPUT_F32_NDHWC", "VS_R3D_NUM_CONVS", "VS_R3D_FEATURES"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(L, name)
    assert C.sizeof(L.R3dParams) == 20 * 5 * C.sizeof(C.c_void_p)
    # the two decisions carried over from the GoogLeNet front end are stated where the ABI is read
    assert "RUNNING statistics" in text and "No pretrained weights" in text

    class Partial:                      # a stale library: no quiet fall-back, load() refuses it
        def __getattr__(self, name):
            if name == "vs_r3d_forward":
                raise AttributeError(name)
            return lambda *a: 0

    with pytest.raises(RuntimeError, match=r"lacks symbol vs_r3d_forward \(stale build\?\)"):
        L._bind_video_features(Partial())


def test_header_is_plain_c99():
    gcc = shutil.which("gcc")
    assert gcc
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_a_cpu_tensor_raises(vsa):
    model = vsa.R3D18Features()
    with pytest.raises(RuntimeError, match="no CPU path"):
        model(torch.zeros(1, 3, 4, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.extract(torch.zeros(4, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="model= or weights="):
        vsa.get_video_feature(torch.zeros(4, 16, 16, 3, dtype=torch.uint8).numpy())
    doc = vsa.video_features.__doc__
    assert model.train().training and "running statistics" in doc and "never fetched" in doc
