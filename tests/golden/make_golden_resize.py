"""Writes tests/golden/resize_golden.npz: inputs and PIL's own ``Image.resize((ow, oh), Image.BILINEAR)`` outputs for the
geometries of tests/test_hip_resize.py, so that the GPU tests need neither PIL nor anything outside the tree.  Run on a CPU:

    python tests/golden/make_golden_resize.py

The 360 x 640 input is not stored: it is ``resize_ref.content("ramp", 2, 360, 640)``, a stated formula."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_ref  # noqa: E402

# name: (n, h, w, oh, ow, content kind, seed, store the input)
CASES = {
    "up_17x15": (3, 17, 15, 40, 33, "random", 1, True),
    "down_64x80": (1, 64, 80, 15, 19, "random", 2, True),
    "h_only_33x47": (2, 33, 47, 33, 20, "random", 3, True),
    "v_only_33x47": (2, 33, 47, 20, 47, "random", 4, True),
    "tall_300x40": (1, 300, 40, 15, 40, "random", 5, True),
    "real_360x640": (2, 360, 640, 224, 398, "ramp", 0, False),
    "checker_17x15": (1, 17, 15, 40, 33, "checker", 0, True),
    "checker_64x80": (1, 64, 80, 15, 19, "checker", 1, True),
}


def pil_resize(frames, oh, ow):
    return np.stack([np.asarray(Image.fromarray(f).resize((ow, oh), Image.BILINEAR)) for f in frames])


def main():
    out = {}
    for name, (n, h, w, oh, ow, kind, seed, keep) in CASES.items():
        x = resize_ref.content(kind, n, h, w, seed)
        y = pil_resize(x, oh, ow)
        assert y.shape == (n, oh, ow, 3) and y.dtype == np.uint8
        assert np.array_equal(y, resize_ref.resize(x, (oh, ow))), name      # the restatement is PIL, bit for bit
        if keep:
            out[name + ".in"] = x
        out[name + ".out"] = y
        out[name + ".spec"] = np.array([n, h, w, oh, ow, seed], dtype=np.int64)
    path = os.path.join(HERE, "resize_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
