"""CPU reference of the box mean (MI355_FILTER_BOX / BOX_GRAY8) and of the mean adaptive threshold.

cv::blur(src, dst, Size(k, k), Point(-1, -1), BORDER_REPLICATE): clamp-to-edge padding (np.pad mode="edge"), the int sum
s of the k x k window from an integral image, and out = floor((2 s + d) / (2 d)) with d = k * k, the integer nearest to
s / d (d is odd: no tie).  adaptive_ref is cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) on top of it.  A plain numpy
helper, not a fixture module.  `rows` restricts the output to chosen rows (median_ref.sample_rows picks them), so 4K
frames can be checked in bounded memory.
"""
import math

import numpy as np

BINARY, BINARY_INV = 0, 1


def box_sums(img, k, rows=None):
    """The int window sums: img (h, w) or (h, w, c) uint8 -> int64 of the same shape (or len(rows) rows of it)."""
    img = np.asarray(img, np.uint8)
    assert k % 2 == 1 and k >= 1
    r = k // 2
    rows = np.arange(img.shape[0]) if rows is None else np.asarray(rows, np.int64)
    pad = np.pad(img, ((r, r), (r, r)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    # integral image, one axis at a time; int32 holds it: (h + 2r) * 255 and (w + 2r) * k * 255 stay far below 2^31
    down = np.zeros((pad.shape[0] + 1,) + pad.shape[1:], np.int32)
    np.cumsum(pad, axis=0, dtype=np.int32, out=down[1:])
    cols = down[rows + k] - down[rows]                               # (n, w + 2r, [c]): k rows summed
    along = np.zeros((cols.shape[0], cols.shape[1] + 1) + cols.shape[2:], np.int32)
    np.cumsum(cols, axis=1, dtype=np.int32, out=along[:, 1:])
    return (along[:, k:] - along[:, :-k]).astype(np.int64)


def box_ref(img, k, rows=None):
    """Box mean of one frame: img (h, w) or (h, w, c) uint8 -> uint8 of the same shape (or len(rows) rows of it)."""
    d = k * k
    return ((2 * box_sums(img, k, rows) + d) // (2 * d)).astype(np.uint8)


def idelta_of(type, delta):
    """cv::adaptiveThreshold's integer delta: ceil for BINARY, floor for BINARY_INV, clamped to [-256, 256]."""
    assert type in (BINARY, BINARY_INV)
    v = math.ceil(delta) if type == BINARY else math.floor(delta)
    return int(min(256, max(-256, v)))


def adaptive_ref(y, max_value, type, block, delta, rows=None, mean=None):
    """Mean adaptive threshold of one gray8 frame (h, w) -> uint8 (h, w) (or len(rows) rows of it).  `mean` may carry
    box_ref(y, block, rows) from an earlier call, so a sweep over types, deltas and values computes it once."""
    y = np.asarray(y, np.uint8)
    assert y.ndim == 2
    src = (y if rows is None else y[np.asarray(rows, np.int64)]).astype(np.int32)
    diff = src - (box_ref(y, block, rows) if mean is None else mean).astype(np.int32)
    idelta = idelta_of(type, delta)
    on = diff > -idelta if type == BINARY else diff <= -idelta
    return np.where(on, max_value, 0).astype(np.uint8)
