"""CPU reference of rectangular grey-level morphology (MI355_FILTER_ERODE ... CLOSE_GRAY8).

A k x k MORPH_RECT element anchored at the centre, clamp-to-edge padding (np.pad mode="edge" = BORDER_REPLICATE), and
the min (erode) or max (dilate) of the window per channel.  OPEN = dilate(erode(x)) and CLOSE = erode(dilate(x)): each
stage pads its own input, so the intermediate frame has its own clamp-to-edge border.  A plain numpy helper for the
morphology tests, not a fixture module.  `rows` restricts the output to chosen rows (median_ref.sample_rows picks
them), so 4K frames can be checked in bounded memory; OPEN / CLOSE then compute the intermediate on the rows they need.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

OPS = ("erode", "dilate", "open", "close")


def _minmax(img, k, fn, rows):
    r = k // 2
    pad = np.pad(img, ((r, r), (r, r)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    rows = np.arange(img.shape[0]) if rows is None else np.asarray(rows, np.int64)
    out = np.empty((len(rows),) + img.shape[1:], np.uint8)
    for i0 in range(0, len(rows), 32):
        sel = rows[i0:i0 + 32]
        band = np.stack([pad[y:y + k] for y in sel])                 # (n, k, w + 2r, [c])
        v = fn(band, axis=1)                                          # separable: rows first, then columns
        win = sliding_window_view(v, k, axis=1)                       # (n, w, [c], k)
        out[i0:i0 + len(sel)] = fn(win, axis=-1)
    return out


def erode_ref(img, k, rows=None):
    return _minmax(np.asarray(img, np.uint8), k, np.min, rows)


def dilate_ref(img, k, rows=None):
    return _minmax(np.asarray(img, np.uint8), k, np.max, rows)


def _two(img, k, first, second, rows):
    img = np.asarray(img, np.uint8)
    h = img.shape[0]
    if rows is None:
        return second(first(img, k), k)
    r = k // 2
    rows = np.asarray(rows, np.int64)
    need = np.unique(np.clip((rows[:, None] + np.arange(-r, r + 1)[None, :]).ravel(), 0, h - 1))
    mid = np.empty_like(img)
    mid[need] = first(img, k, rows=need)                              # only the rows the second stage reads
    return second(mid, k, rows=rows)


def open_ref(img, k, rows=None):
    return _two(img, k, erode_ref, dilate_ref, rows)


def close_ref(img, k, rows=None):
    return _two(img, k, dilate_ref, erode_ref, rows)


def morph_ref(op, img, k, rows=None):
    """op in OPS; img (h, w) or (h, w, c) uint8 -> the same shape (or len(rows) rows of it)."""
    assert k % 2 == 1 and k >= 1
    return {"erode": erode_ref, "dilate": dilate_ref, "open": open_ref, "close": close_ref}[op](img, k, rows=rows)
