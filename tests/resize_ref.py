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
