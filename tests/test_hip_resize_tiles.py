"""GPU: every tile form resize_make_plan (csrc/vs_resize_plan.h) can choose, run by resize_bilinear_u8 and compared with
tests/resize_ref.py (which test_resize_host.py holds equal to PIL) with ``==`` on bytes.  test_hip_resize.py runs the default
32 x 64 tile and one 8 x 64 case; the tile's width sets lane_shift, lanes_y and which lanes run each pass, and its height how the
vertical pass walks the block, so each width in {64, 16, 4, 1} and each height in {32, 8, 4, 2, 1} runs here at least once.

Every case first asserts the tile the plan chose (a retune of the LDS budget cannot make a case vacuous unnoticed) and that the
expected output can tell one tile's pixels from another's: the inputs are resize_ref.blocks, whose large reductions keep most of
the byte range and differ between neighbouring output pixels (independent random bytes average to a few values near 127)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import resize_ref

pytestmark = pytest.mark.gpu

SMALL, FUSED = resize_ref.PATH_SMALL_TILE, resize_ref.PATH_FUSED
CASES = resize_ref.TILE_CASES         # name: ((n, h, w), (oh, ow), path, (tile_oh, tile_ow))
# one input pixel gives a constant output and one output pixel has no neighbour: no spread to ask of these two
ONE_PIXEL = ("one pixel in", "one pixel out")
ODD = ("w16 batch of 3 odd frames", "h2 w16 batch of 3 odd frames")


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vsa():
    return importlib.import_module("video-summarization_amd")


_REFS = {}


def _reference(name):
    """(blocks input, resize_ref's output) of a case: computed once, shared, never written; the output's spread is asserted here,
    before any test touches the GPU with it"""
    if name not in _REFS:
        (n, h, w), (oh, ow) = CASES[name][:2]
        x = resize_ref.blocks(n, h, w, oh, ow, seed=40 + list(CASES).index(name))
        want = resize_ref.resize(x, (oh, ow))
        span, share = resize_ref.spread(want)
        if name in ONE_PIXEL:
            assert len(set(want[0, 0, 0].tolist())) == 3, name          # the three channels differ: a swap shows
        else:
            assert span >= 128 and share >= 0.9, (name, span, share)
        x.setflags(write=False)
        want.setflags(write=False)
        _REFS[name] = (x, want)
    return _REFS[name]


def _assert_tile(vsa, name):
    (n, h, w), (oh, ow), path, tile = CASES[name]
    assert (SMALL, FUSED) == (vsa._lib.VS_RESIZE_PATH_SMALL_TILE, vsa._lib.VS_RESIZE_PATH_FUSED)
    assert vsa.features.resize_plan_path(_dev(), h, w, oh, ow) == (path, tile), name


def _resize(vsa, x, size, **kw):
    """numpy in, numpy out through the device"""
    got = vsa.resize_frames_device(torch.from_numpy(np.ascontiguousarray(x)).to(_dev()), size, **kw)
    assert got.dtype == torch.uint8 and got.is_cuda and got.is_contiguous()
    return got.cpu().numpy()


def _report(name, what):
    print("resize_tiles %-50s tile %2d x %2d  %s" % ((name,) + CASES[name][3] + (what,)))


def test_the_cases_cover_every_tile_width_and_height():
    tiles = [c[3] for c in CASES.values()]
    assert {t[1] for t in tiles} == {64, 16, 4, 1} and {t[0] for t in tiles} == {32, 8, 4, 2, 1}


@pytest.mark.parametrize("name", list(CASES))
def test_every_tile_form_equals_resize_ref_bit_for_bit(vsa, name):
    x, want = _reference(name)
    _assert_tile(vsa, name)
    got = _resize(vsa, x, CASES[name][1])
    assert got.shape == want.shape
    assert np.array_equal(got, want), "%s: %d of %d bytes differ" % (name, (got != want).sum(), want.size)
    _report(name, "%d bytes equal to resize_ref" % want.size)


@pytest.mark.parametrize("name", ODD)
def test_narrow_and_short_tiles_with_bgr_and_in_any_batch(vsa, name):
    """the R/B swap of the horizontal pass and the frame offsets, on a 16-column and a 2-row tile: the flipped frames with
    bgr=True give the plain result, and a frame gives the same bytes alone, in another order and in the batch of 3"""
    x, want = _reference(name)
    size = CASES[name][1]
    _assert_tile(vsa, name)
    assert x.shape[0] == 3 and x[0].size % 2 == 1
    assert np.array_equal(_resize(vsa, x[..., ::-1], size, bgr=True), want)
    swapped = _resize(vsa, x, size, bgr=True)
    assert np.array_equal(swapped, want[..., ::-1]) and (swapped != want).any()
    for i in range(3):
        assert np.array_equal(_resize(vsa, x[i:i + 1], size)[0], want[i]), i
    assert np.array_equal(_resize(vsa, x[[2, 0]], size), want[[2, 0]])
    assert (want[0] != want[1]).any() and (want[1] != want[2]).any()
    _report(name, "bgr and every batch form equal")


@pytest.mark.parametrize("out_shift", (1, 3))
@pytest.mark.parametrize("name", ODD)
def test_narrow_and_short_tiles_at_odd_addresses_write_no_byte_outside(vsa, name, out_shift):
    """through the C ABI, the output at address 1 and 3 modulo 4 inside canaries (the frames at 2 and 0): the narrow tiles' last
    dword of a row is a partial store, and no 2- or 4-byte store may be chosen for an address that is not a multiple of it"""
    L = vsa._lib
    lib = L.load()
    dev = _dev()
    x, want = _reference(name)
    (n, h, w), (oh, ow) = CASES[name][:2]
    _assert_tile(vsa, name)
    guard, in_shift = 64, 3 - out_shift
    src = torch.zeros(x.size + 8, dtype=torch.uint8, device=dev)
    src[in_shift:in_shift + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
    dst = torch.full((guard + want.size + guard + 8,), 0x5A, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 4 == 0 and dst.data_ptr() % 4 == 0 and guard % 4 == 0
    plan = C.c_void_p()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.vs_resize_plan_create(h, w, oh, ow, stream, C.byref(plan)))
    try:
        path, th, tw = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(lib.vs_resize_plan_describe(plan, C.byref(path), C.byref(th), C.byref(tw)))
        assert (path.value, (th.value, tw.value)) == CASES[name][2:]
        L.check(lib.vs_resize_run(plan, src.data_ptr() + in_shift, n, 0, dst.data_ptr() + guard + out_shift, None, 0, stream))
        torch.cuda.synchronize()
    finally:
        lib.vs_resize_plan_free(plan)
    got = dst.cpu().numpy()
    at = guard + out_shift
    assert np.array_equal(got[at:at + want.size].reshape(want.shape), want)
    assert (got[:at] == 0x5A).all() and (got[at + want.size:] == 0x5A).all()
    _report(name, "output at address %d mod 4: equal, canaries whole" % out_shift)
