"""PIL's antialiased bilinear resize of 8-bit images (``Image.resize((ow, oh), Image.BILINEAR)``), restated in numpy: the
coefficient tables in Python floats (IEEE doubles, one operation per rounding), everything after them in integers.  The
checker of the device resize (csrc/vs_resize_plan.h builds the same tables, csrc/vs_resize.hip runs the same passes)."""
import math

import numpy as np

PRECISION_BITS = 22


def output_size(h, w, size):
    """torchvision's rule: an int scales the shorter side (``w <= h`` counts as "w is shorter"), a pair is (oh, ow)"""
    if isinstance(size, int):
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long / short)
        ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
        return oh, ow
    oh, ow = size
    return int(oh), int(ow)


def axis_table(n_in, n_out):
    """(ksize, bounds [n_out, 2] = (xmin, n), coefficients [n_out, ksize]) of one axis"""
    scale = float(np.float32(n_in)) / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    coef = np.zeros((n_out, ksize), dtype=np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)          # int() truncates toward zero
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = []
        ww = 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        for x in range(n):
            if ww != 0.0:
                w[x] /= ww
            coef[xx, x] = int(-0.5 + w[x] * (1 << PRECISION_BITS)) if w[x] < 0 else int(0.5 + w[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return ksize, bounds, coef


def _pass(img, axis, n_out):
    """one pass along ``axis`` of an integer array; the result is rounded to uint8 range"""
    _, bounds, coef = axis_table(img.shape[axis], n_out)
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        k = coef[xx, :n].reshape((n,) + (1,) * (img.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (img[xmin:xmin + n] * k).sum(axis=0)
        assert acc.max() < 1 << 31 and acc.min() >= 0                   # int32 on the device
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(frames, size):
    """uint8 [..., H, W, C] -> uint8 [..., oh, ow, C]: horizontal pass, rounded to uint8, then the vertical pass; a pass whose
    sizes are equal is skipped"""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim >= 3
    h, w = frames.shape[-3:-1]
    oh, ow = output_size(h, w, size)
    out = frames
    if ow != w:
        out = _pass(out, out.ndim - 2, ow)
    if oh != h:
        out = _pass(out, out.ndim - 3, oh)
    return np.ascontiguousarray(out).astype(np.uint8)


# ---- shared inputs: every content the tests and the golden file use comes from here ----
def content(kind, n, h, w, seed=0):
    """uint8 [n, h, w, 3]: 'random' bytes, a 'ramp' (a stated formula, so large cases need not be stored), a 0/255 'checker'"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f, y, x, c = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "ramp":
        return ((7 * x + 13 * y + 5 * x * y // 3 + 31 * f + 85 * c + seed) % 256).astype(np.uint8)
    if kind == "checker":
        return (((x // 2 + y // 3 + f + c + seed) % 2) * 255).astype(np.uint8)
    raise ValueError(kind)


def blocks(n, h, w, oh, ow, seed=0):
    """uint8 [n, h, w, 3] for a large reduction to (oh, ow): random bytes that stay constant over runs of ``in // (2 * out)`` rows
    and columns (at least 1), about two runs per output pixel and axis.  Independent bytes average out under a 100x reduction
    (every output byte lands near 127, so a tile that read its neighbour's columns would still compare equal); these do not:
    neighbouring output pixels differ, over most of the byte range (``spread`` below says by how much)."""
    by, bx = max(1, h // (2 * oh)), max(1, w // (2 * ow))
    coarse = np.random.default_rng(seed).integers(0, 256, size=(n, -(-h // by), -(-w // bx), 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, by, axis=1), bx, axis=2)[:, :h, :w])


def spread(out):
    """(largest - smallest byte, share of horizontally and vertically adjacent pixels of uint8 [n, oh, ow, 3] that differ): what a
    test asserts of an expected output before it trusts ``==`` on it to tell one tile's pixels from another's.  An axis of one
    pixel has no pairs and does not count."""
    out = np.asarray(out)
    pairs = [(out[:, :, 1:] != out[:, :, :-1]).any(axis=-1), (out[:, 1:] != out[:, :-1]).any(axis=-1)]
    differ, total = sum(int(p.sum()) for p in pairs), sum(p.size for p in pairs)
    return int(out.max()) - int(out.min()), (differ / total if total else 1.0)


# ---- the geometries that leave the default tile, and the default tile's edges: name -> ((n, h, w), (oh, ow), path, (tile_oh,
# tile_ow)) as csrc/vs_resize_plan.h chooses today.  test_resize_host.py walks them on the host and holds them equal to PIL,
# test_hip_resize_tiles.py runs them on the device; both assert the tile, so a retune of the plan shows in both ----
PATH_FUSED, PATH_SMALL_TILE = 0, 1      # = VS_RESIZE_PATH_* of include/features/vs_resize.h
TILE_CASES = {
    "w16 four column tiles": ((2, 3, 6400), (3, 64), PATH_SMALL_TILE, (32, 16)),
    "w4 nine tiles, the last one column wide": ((1, 2, 20000), (2, 33), PATH_SMALL_TILE, (32, 4)),
    "w4 33 tiles": ((1, 2, 65536), (2, 130), PATH_SMALL_TILE, (32, 4)),
    "w1": ((1, 2, 65536), (2, 40), PATH_SMALL_TILE, (32, 1)),
    "w16 at the LDS limit": ((1, 2, 36000), (2, 100), PATH_SMALL_TILE, (32, 16)),
    # the narrow tiles with all 32 rows in use (the cases above have 2 or 3): 16, 64 and 256 rows of lanes walk 32 + 8 rows
    "w16 40 rows": ((1, 40, 6400), (40, 64), PATH_SMALL_TILE, (32, 16)),
    "w4 40 rows": ((1, 40, 20000), (40, 33), PATH_SMALL_TILE, (32, 4)),
    "w1 40 rows": ((1, 40, 65536), (40, 40), PATH_SMALL_TILE, (32, 1)),
    "h8": ((1, 300, 40), (15, 40), PATH_SMALL_TILE, (8, 64)),
    "h4 w16": ((1, 6400, 3), (64, 3), PATH_SMALL_TILE, (4, 16)),
    "h2 w16 2 x 3 tiles": ((1, 700, 40), (4, 40), PATH_SMALL_TILE, (2, 16)),
    "h2 w16 one column tile": ((1, 960, 5), (6, 5), PATH_SMALL_TILE, (2, 16)),
    "h2 w64": ((1, 400, 7), (10, 7), PATH_SMALL_TILE, (2, 64)),
    "h1 w64": ((1, 640, 5), (8, 5), PATH_SMALL_TILE, (1, 64)),
    # frames of an odd number of bytes (57609 and 86223): frames 1 and 2 start at odd addresses
    "w16 batch of 3 odd frames": ((3, 3, 6401), (3, 64), PATH_SMALL_TILE, (32, 16)),
    "h2 w16 batch of 3 odd frames": ((3, 701, 41), (4, 40), PATH_SMALL_TILE, (2, 16)),
    # the default tile's edges
    "one pixel in": ((1, 1, 1), (9, 9), PATH_FUSED, (32, 64)),
    "one pixel out": ((1, 5, 3), (1, 1), PATH_FUSED, (32, 64)),
    "65 columns: a second column tile of one column": ((1, 9, 200), (9, 65), PATH_FUSED, (32, 64)),
    "33 x 65: 2 x 2 tiles, the last of one pixel": ((1, 40, 20), (33, 65), PATH_FUSED, (32, 64)),
}
