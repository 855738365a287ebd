"""CPU reference of the median filter (MI355_FILTER_MEDIAN / MEDIAN_GRAY8): cv::medianBlur semantics.

Clamp-to-edge padding (np.pad mode="edge" = BORDER_REPLICATE), a k x k sliding window, and the middle one of the k*k
values per channel (np.partition).  A plain numpy helper for the median tests, not a fixture module.  `rows` restricts
the output to chosen rows, so 4K frames can be checked on sampled bands plus the border rows in bounded memory.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def median_ref(img, k, rows=None, chunk=32):
    """Median of one frame: img (h, w) or (h, w, c) uint8 -> the same shape (or len(rows) rows of it)."""
    img = np.asarray(img, np.uint8)
    assert k % 2 == 1 and k >= 1
    r = k // 2
    h = img.shape[0]
    pad = np.pad(img, ((r, r), (r, r)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    rows = np.arange(h) if rows is None else np.asarray(rows, np.int64)
    out = np.empty((len(rows),) + img.shape[1:], np.uint8)
    mid = k * k // 2
    for i0 in range(0, len(rows), chunk):
        sel = rows[i0:i0 + chunk]
        # windows of the selected output rows only: (n, w, [c], k, k)
        band = np.stack([pad[y:y + k] for y in sel])
        win = sliding_window_view(band, (k, k), axis=(1, 2))[:, 0]
        flat = win.reshape(win.shape[:-2] + (k * k,))
        out[i0:i0 + len(sel)] = np.partition(flat, mid, axis=-1)[..., mid]
    return out


def sample_rows(h, k, bands=((0.25, 16), (0.6, 16))):
    """Every border row a window can clamp in (the first and last k rows) plus a few interior bands."""
    rows = set(range(min(h, k))) | set(range(max(0, h - k), h))
    for frac, n in bands:
        y0 = int(h * frac)
        rows |= set(range(y0, min(h, y0 + n)))
    return np.array(sorted(rows), np.int64)
