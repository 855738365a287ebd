"""CPU reference of the distance transform calls (mi355_dist_*): include/mi355_imgfilter.h, "how far from the background".

A pixel whose byte is zero is a site.  Per pixel: the exact squared Euclidean distance to the nearest site (int32), its
square root np.sqrt(sq.astype(np.float32)) (float32), and y' * w + x' of the nearest site (int32): among equally near
sites the smallest column x', among those the smallest row y'.  A frame without a site holds NONE, +inf and -1.

dist_ref runs the two passes the header describes, in numpy: per column the signed row offset to the nearest site (a tie
goes to the site above), by cumulative maxima and minima; per row the minimum over all candidate columns of the composite
key (value, x'), in chunks of rows so that a 1030-wide row stays small in memory.  all_pairs is the independent check of
it: every site against every pixel, with the tie rule stated directly.
"""
import numpy as np

NONE = 2147483647
NO_SITE = 1 << 30       # the value of a column without a site in the row pass: above 2 * 16383^2, and with 16383^2 inside int64 keys
MAX_DIM = 16384


def column_offsets(mask):
    """(h, w) int64 dy = y' - y to the nearest site of the pixel's own column, a tie to the site above; and the (h, w) bool
    array of pixels whose column has no site at all"""
    m = np.asarray(mask)
    h, w = m.shape
    site = m == 0
    rows = np.arange(h, dtype=np.int64)[:, None]
    far = 4 * MAX_DIM
    above = np.maximum.accumulate(np.where(site, rows, -far), axis=0)              # the last site row at or above y
    below = np.minimum.accumulate(np.where(site, rows, far)[::-1], axis=0)[::-1]   # the first site row at or below y
    du, dd = rows - above, below - rows
    dy = np.where(du <= dd, -du, dd)
    return dy, ~site.any(axis=0)[None, :].repeat(h, axis=0)


def _one(mask, row_chunk):
    m = np.asarray(mask)
    h, w = m.shape
    dy, empty = column_offsets(m)
    f = np.where(empty, NO_SITE, dy * dy)                                          # (h, w) int64
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                         # [x, x']
    sq = np.empty((h, w), np.int64)
    arg = np.empty((h, w), np.int64)
    for y0 in range(0, h, row_chunk):
        fr = f[y0:y0 + row_chunk]                                                  # (r, w)
        key = (dx2[None, :, :] + fr[:, None, :]) * MAX_DIM + xs[None, None, :]     # (r, x, x'): value first, then x'
        best = key.min(axis=2)
        sq[y0:y0 + row_chunk] = best // MAX_DIM
        arg[y0:y0 + row_chunk] = best % MAX_DIM
    ys = np.arange(h, dtype=np.int64)[:, None]
    near = (ys + np.take_along_axis(dy, arg, axis=1)) * w + arg
    if not (m == 0).any():
        return (np.full((h, w), NONE, np.int32), np.full((h, w), np.inf, np.float32), np.full((h, w), -1, np.int32))
    sq32 = sq.astype(np.int32)
    return sq32, np.sqrt(sq32.astype(np.float32)), near.astype(np.int32)


def dist_ref(masks):
    """(sq int32, dist float32, nearest int32), each (n, h, w), of (h, w) / (n, h, w) masks"""
    ms = np.asarray(masks)
    ms = ms[None] if ms.ndim == 2 else ms
    n, h, w = ms.shape
    assert 1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM
    row_chunk = max(1, (1 << 22) // (w * w))                                       # at most 4 Mi keys at a time
    outs = [_one(m, row_chunk) for m in ms]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))


def all_pairs(mask):
    """The same three outputs of one (h, w) mask by a search over every (pixel, site) pair with the tie rule stated
    directly: the smallest squared distance, then the smallest x', then the smallest y'.  For small frames only."""
    m = np.asarray(mask)
    h, w = m.shape
    sy, sx = np.nonzero(m == 0)
    if sy.size == 0:
        return (np.full((h, w), NONE, np.int32), np.full((h, w), np.inf, np.float32), np.full((h, w), -1, np.int32))
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy[:, :, None] - sy[None, None, :]).astype(np.int64) ** 2 + (xx[:, :, None] - sx[None, None, :]).astype(np.int64) ** 2
    key = (d2 * MAX_DIM + sx[None, None, :]) * MAX_DIM + sy[None, None, :]
    k = key.argmin(axis=2)
    sq = np.take_along_axis(d2, k[:, :, None], axis=2)[:, :, 0].astype(np.int32)
    near = (sy[k] * w + sx[k]).astype(np.int32)
    return sq, np.sqrt(sq.astype(np.float32)), near


def unique_nearest(mask):
    """(h, w) bool: the pixel has exactly one nearest site (small frames only)"""
    m = np.asarray(mask)
    h, w = m.shape
    sy, sx = np.nonzero(m == 0)
    if sy.size == 0:
        return np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy[:, :, None] - sy[None, None, :]).astype(np.int64) ** 2 + (xx[:, :, None] - sx[None, None, :]).astype(np.int64) ** 2
    return (d2 == d2.min(axis=2, keepdims=True)).sum(axis=2) == 1
