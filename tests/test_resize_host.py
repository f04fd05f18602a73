"""CPU (no GPU): the frame resize's host side.  tests/resize_ref.py against PIL bit for bit;
csrc/vs_resize_plan.h, alone in tests/cabi/resize_plan_demo.cpp under AddressSanitizer and UBSan, against resize_ref (the
coefficient tables) and against itself (every load, LDS and store address of every tile in bounds, every output byte written
exactly once); the C ABI's argument checks, its binding table and the output-size rule."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import resize_ref

HEADER = os.path.join(ROOT, "include", "features", "vs_resize.h")
PLAN_HEADER = os.path.join(ROOT, "video-summarization_amd", "csrc", "vs_resize_plan.h")
# (n, h, w, oh, ow) of tests/test_hip_resize.py
GPU_GEOMETRIES = ((3, 17, 15, 40, 33), (1, 64, 80, 15, 19), (2, 33, 47, 33, 20), (2, 33, 47, 20, 47), (1, 300, 40, 15, 40),
                  (2, 360, 640, 224, 398))
EXTRA_GEOMETRIES = ((1, 1080, 1920, 224, 398), (1, 224, 300, 224, 224), (1, 5, 3, 1, 1), (1, 2, 2, 9, 9))
# (n, h, w, oh, ow) of tests/test_hip_resize_tiles.py: the tiles narrower or shorter than the default one, and its edges
TILE_GEOMETRIES = tuple(c[0] + c[1] for c in resize_ref.TILE_CASES.values())
NEW_TILE_GEOMETRIES = tuple(g for g in TILE_GEOMETRIES if g not in GPU_GEOMETRIES + EXTRA_GEOMETRIES)
AXES = ((360, 224), (640, 398), (1080, 224), (1920, 398), (2160, 224), (60, 224), (300, 15))
GRID = 40


@pytest.mark.parametrize("geometry", GPU_GEOMETRIES + EXTRA_GEOMETRIES + NEW_TILE_GEOMETRIES,
                         ids=lambda g: "%dx%d-%dx%d" % g[1:])
def test_resize_ref_is_pil_bit_for_bit(geometry):
    Image = pytest.importorskip("PIL.Image")
    _, h, w, oh, ow = geometry
    for kind in ("random", "ramp", "checker", "blocks"):
        x = resize_ref.blocks(1, h, w, oh, ow, seed=11) if kind == "blocks" else resize_ref.content(kind, 1, h, w, seed=11)
        want = np.asarray(Image.fromarray(x[0]).resize((ow, oh), Image.BILINEAR))
        got = resize_ref.resize(x, (oh, ow))[0]
        assert got.shape == want.shape and np.array_equal(got, want), (geometry, kind)


def test_golden_file_is_what_resize_ref_computes():
    z = np.load(os.path.join(GOLDEN, "resize_golden.npz"))
    names = sorted(k[:-5] for k in z.files if k.endswith(".spec"))
    assert len(names) == 8
    for name in names:
        n, h, w, oh, ow, seed = (int(v) for v in z[name + ".spec"])
        x = z[name + ".in"] if name + ".in" in z.files else resize_ref.content("ramp", n, h, w, seed)
        assert x.shape == (n, h, w, 3) and np.array_equal(resize_ref.resize(x, (oh, ow)), z[name + ".out"]), name
    assert os.path.getsize(os.path.join(GOLDEN, "resize_golden.npz")) < 1 << 20


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("resize_plan") / "resize_plan_demo")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "video-summarization_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cabi", "resize_plan_demo.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def test_tables_equal_resize_ref(demo):
    args = [str(v) for pair in AXES for v in pair]
    run = subprocess.run([demo, "tables", "grid", str(GRID)] + args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.endswith("OK\n"), (run.stdout[-500:], run.stderr[-2000:])
    lines = run.stdout.split("\n")
    at, seen = 0, []
    while lines[at].startswith("axis"):
        n_in, n_out, ksize = (int(v) for v in lines[at].split()[1:])
        rows = np.array([[int(v) for v in line.split()] for line in lines[at + 1:at + 1 + n_out]], dtype=np.int64)
        at += 1 + n_out
        want_ksize, bounds, coef = resize_ref.axis_table(n_in, n_out)
        assert ksize == want_ksize and rows.shape == (n_out, 2 + ksize), (n_in, n_out)
        assert np.array_equal(rows[:, :2], bounds) and np.array_equal(rows[:, 2:], coef), (n_in, n_out)
        # what the kernel relies on: windows inside the image, never empty, not moving backwards, sums that fit int32
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= n_in).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all()
        assert (coef >= 0).all() and ((1 << 21) + 255 * coef.sum(axis=1) < 1 << 31).all()
        seen.append((n_in, n_out))
    assert lines[at] == "OK"
    assert seen == [(i, o) for i in range(1, GRID + 1) for o in range(1, GRID + 1)] + list(AXES)


def test_every_tile_address_is_in_bounds_and_every_output_byte_written_once(demo):
    # 4K, the smaller tiles in each axis, input rows staged in several chunks at changing address phases
    extra = ((1, 2160, 3840, 224, 398), (1, 7, 2000, 7, 3), (1, 3000, 5, 2, 5), (2, 120, 1500, 16, 40), (2, 120, 1501, 16, 40))
    args = [str(v) for g in GPU_GEOMETRIES + EXTRA_GEOMETRIES + extra + NEW_TILE_GEOMETRIES for v in g]
    run = subprocess.run([demo, "walk"] + args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.endswith("OK\n"), (run.stdout[-500:], run.stderr[-2000:])
    geoms = {}
    for line in run.stdout.split("\n"):
        f = line.split()
        if f and f[0] == "geom":
            geoms[tuple(int(v) for v in f[1:6])] = (int(f[7]), int(f[9]), int(f[10]))          # path, tile_oh, tile_ow
    assert len(geoms) == len(GPU_GEOMETRIES + EXTRA_GEOMETRIES + extra + NEW_TILE_GEOMETRIES)
    assert geoms[(2, 360, 640, 224, 398)] == (0, 32, 64) and geoms[(1, 1080, 1920, 224, 398)] == (0, 32, 64)
    path, tile_oh, tile_ow = geoms[(1, 300, 40, 15, 40)]            # ksize 41, 20 input rows per output row: the smaller tile
    assert path == 1 and tile_oh < 32 and tile_ow == 64
    assert geoms[(1, 2160, 3840, 224, 398)][0] == 1 and geoms[(1, 3000, 5, 2, 5)][0] == 1 and geoms[(1, 3000, 5, 2, 5)][2] < 64
    # every tile the GPU cases name is the tile walked here: widths 16, 4 and 1, heights 8, 4, 2 and 1 among them
    for (shape, size, path, tile) in resize_ref.TILE_CASES.values():
        assert geoms[shape + size] == (path,) + tile, (shape, size)
    assert geoms[(1, 2, 20000, 2, 33)][2] == 4 and geoms[(1, 2, 65536, 2, 130)][2] == 4 and geoms[(1, 2, 65536, 2, 40)][2] == 1
    assert {g[2] for g in geoms.values()} >= {64, 16, 4, 1} and {g[1] for g in geoms.values()} >= {32, 8, 4, 2, 1}


def test_plan_header_has_no_hip_include():
    text = open(PLAN_HEADER).read()
    assert "#include <hip" not in text and "hip_runtime" not in text


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


def test_sources_binding_table_and_abi_version(vsa):
    L = vsa._lib
    for src in ("vs_resize.hip", "vs_resize.cpp"):
        assert src in L.SOURCES
    assert L.EXTRA_FLAGS["vs_resize.cpp"] == ("-ffp-contract=off",)
    assert L.ABI_VERSION == 3 and L.load().vs_abi_version() == 3
    protos = _prototypes(open(HEADER).read())
    assert set(protos) == set(L._RESIZE_BINDINGS) == set(L.RESIZE_EXPORTS)
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "void": None}
    for name, (ret, nargs) in protos.items():
        restype, argtypes = L._RESIZE_BINDINGS[name]
        assert kinds[ret] is restype and len(argtypes) == nargs, name
    lib = L.load()
    for name in protos:
        assert hasattr(lib, name), name
    text = open(HEADER).read()
    for name in ("VS_RESIZE_SWAP_RB", "VS_RESIZE_PATH_FUSED", "VS_RESIZE_PATH_SMALL_TILE"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(L, name)

    class Partial:                      # a stale library: no quiet fall-back, load() refuses it
        def __getattr__(self, name):
            if name == "vs_resize_run":
                raise AttributeError(name)
            return lambda *a: 0

    with pytest.raises(RuntimeError, match=r"lacks symbol vs_resize_run \(stale build\?\)"):
        L._bind_resize(Partial())


def test_header_is_plain_c99():
    gcc = shutil.which("gcc")
    assert gcc
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_c_abi_argument_checks_need_no_gpu(vsa):
    L = vsa._lib
    lib = L.load()
    INV = L.VS_ERR_INVALID
    oh, ow, handle = C.c_int32(), C.c_int32(), C.c_void_p()
    fake = 4096                                                     # non-NULL stand-ins: every check below fails before any is read
    assert lib.vs_resize_output_size(360, 640, 224, None, C.byref(ow)) == INV and b"NULL" in lib.vs_last_error()
    assert lib.vs_resize_output_size(360, 640, 224, C.byref(oh), None) == INV
    for h, w, size in ((0, 640, 224), (360, 0, 224), (360, 640, 0), (-1, 640, 224), (1, 65536, 224)):
        assert lib.vs_resize_output_size(h, w, size, C.byref(oh), C.byref(ow)) == INV and b"resize_output_size" in lib.vs_last_error()
    assert lib.vs_resize_plan_create(360, 640, 224, 398, None, None) == INV and b"out is NULL" in lib.vs_last_error()
    for h, w, a, b in ((0, 640, 224, 398), (360, 0, 224, 398), (360, 640, 0, 398), (360, 640, 224, -3)):
        assert lib.vs_resize_plan_create(h, w, a, b, None, C.byref(handle)) == INV and b"below 1" in lib.vs_last_error()
        assert handle.value is None
    assert lib.vs_resize_plan_create(65537, 640, 224, 398, None, C.byref(handle)) == INV and b"above 65536" in lib.vs_last_error()
    assert lib.vs_resize_plan_create(60000, 8, 1, 8, None, C.byref(handle)) == INV and b"too large" in lib.vs_last_error()
    lib.vs_resize_plan_free(None)
    p, th, tw = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.vs_resize_plan_describe(None, C.byref(p), C.byref(th), C.byref(tw)) == INV
    assert lib.vs_resize_plan_describe(fake, None, C.byref(th), C.byref(tw)) == INV and b"NULL" in lib.vs_last_error()
    assert lib.vs_resize_workspace_bytes(None, 1) == 0 and b"resize_workspace_bytes" in lib.vs_last_error()
    assert lib.vs_resize_workspace_bytes(fake, 0) == 0 and b"below 1" in lib.vs_last_error()
    assert lib.vs_resize_run(None, fake, 1, 0, fake, None, 0, None) == INV and b"NULL" in lib.vs_last_error()
    assert lib.vs_resize_run(fake, None, 1, 0, fake, None, 0, None) == INV
    assert lib.vs_resize_run(fake, fake, 1, 0, None, None, 0, None) == INV
    assert lib.vs_resize_run(fake, fake, 0, 0, fake, None, 0, None) == INV and b"n=0" in lib.vs_last_error()
    assert lib.vs_resize_run(fake, fake, -2, 0, fake, None, 0, None) == INV
    assert lib.vs_resize_run(fake, fake, 1, 2, fake, None, 0, None) == INV and b"unknown flags" in lib.vs_last_error()
    assert lib.vs_resize_run(fake, fake, 1, 0x80000001, fake, None, 0, None) == INV and b"unknown flags" in lib.vs_last_error()
    # a short workspace: both paths keep the intermediate in LDS, so every plan needs 0 bytes today and no size is short; the
    # check stands in vs_resize_run for a path that needs one


def test_resize_output_size_is_the_rule_inside_resize_frames(vsa):
    def rule(h, w, size):           # features.resize_frames, lines of its int branch
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long / short)
        ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
        return oh, ow

    for h in (1, 2, 15, 224, 360, 479, 480, 1080, 2160):
        for w in (1, 3, 15, 224, 398, 640, 853, 1920, 3840):
            for size in (1, 7, 224, 225, 256, 1000):
                if 1 <= int(size * max(h, w) / min(h, w)) <= 65536:
                    assert vsa.resize_output_size(h, w, size) == rule(h, w, size) == resize_ref.output_size(h, w, size), (h, w, size)
    assert vsa.resize_output_size(224, 224, 100) == (100, 100) and vsa.resize_output_size(300, 300, 300) == (300, 300)      # w == h
    assert vsa.resize_output_size(360, 640, (17, 19)) == (17, 19)
    with pytest.raises(RuntimeError, match="resize_output_size"):
        vsa.resize_output_size(1, 4000, 224)


def test_a_cpu_tensor_raises(vsa):
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        vsa.resize_frames_device(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vsa.GoogLeNetFeatures().extract(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), size=24)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        vsa.get_google_net_features(np.zeros((1, 32, 32, 3), dtype=np.uint8), model=vsa.GoogLeNetFeatures(), resize="gpu")
