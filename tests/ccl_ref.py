"""CPU reference of the labelling calls (mi355_ccl_*): include/mi355_imgfilter.h, "the blobs of a mask".

Pure Python and numpy.  A raster scan over the row runs of the mask with a union-find whose root is always the smallest
index: runs are numbered in raster order of their first pixel, so a component's root is the run that holds its first
pixel, and numbering the roots in index order is the contract's numbering by first pixel.  scipy.ndimage.label gives the
same labels and is taken when scipy imports (it is much faster on large frames); nothing here needs it, and
test_ccl_cpu.py holds the two against each other.
"""
import numpy as np

try:
    from scipy import ndimage as _ndimage
except Exception:  # pragma: no cover - scipy is optional
    _ndimage = None


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def label_pure(mask, connectivity=8):
    """(labels int32 (h, w), N) of one (h, w) mask: foreground = nonzero, numbered 1 .. N - 1 by first pixel."""
    assert connectivity in (4, 8)
    fg = np.ascontiguousarray(mask) != 0
    h, w = fg.shape
    reach = 1 if connectivity == 8 else 0
    # the runs of every row: starts and ends (exclusive) from the row's padded difference
    pad = np.zeros((h, w + 2), np.int8)
    pad[:, 1:-1] = fg
    d = np.diff(pad, axis=1)
    rows_s, starts = np.nonzero(d == 1)
    _, ends = np.nonzero(d == -1)
    nruns = len(starts)
    parent = list(range(nruns))
    first = np.searchsorted(rows_s, np.arange(h + 1))  # the runs of row y are first[y] .. first[y + 1] - 1
    starts_l, ends_l = starts.tolist(), ends.tolist()
    for y in range(1, h):
        i, i_end = int(first[y - 1]), int(first[y])
        j, j_end = i_end, int(first[y + 1])
        while i < i_end and j < j_end:
            # run i of the row above and run j of this row touch iff their column ranges, widened by `reach`, overlap
            if starts_l[i] < ends_l[j] + reach and starts_l[j] < ends_l[i] + reach:
                a, b = _find(parent, i), _find(parent, j)
                if a != b:
                    if a < b:
                        parent[b] = a
                    else:
                        parent[a] = b
            if ends_l[i] < ends_l[j]:
                i += 1
            else:
                j += 1
    number = [0] * nruns
    n = 1
    for r in range(nruns):
        root = _find(parent, r)
        if root == r:
            number[r] = n
            n += 1
        else:
            number[r] = number[root]  # root < r: already numbered
    labels = np.zeros((h, w), np.int32)
    if nruns:
        lengths = ends - starts
        flat = np.repeat(rows_s * w + starts - np.cumsum(lengths) + lengths, lengths) + np.arange(int(lengths.sum()))
        labels.ravel()[flat] = np.repeat(np.asarray(number, np.int32), lengths)
    return labels, n


def label_scipy(mask, connectivity=8):
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    labels, n = _ndimage.label(np.ascontiguousarray(mask) != 0, structure=structure, output=np.int32)
    return labels, int(n) + 1


def have_scipy():
    return _ndimage is not None


def label(mask, connectivity=8):
    return label_scipy(mask, connectivity) if _ndimage is not None else label_pure(mask, connectivity)


def stats_of(labels, n, stats_rows):
    """(stats (stats_rows, 5) int32 {left, top, width, height, area}, sums (stats_rows, 2) uint64 {sum x, sum y}) of one
    frame's labels; rows without a pixel are zeros, labels >= stats_rows have no row."""
    h, w = labels.shape
    stats = np.zeros((stats_rows, 5), np.int32)
    sums = np.zeros((stats_rows, 2), np.uint64)
    if stats_rows == 0:
        return stats, sums
    flat = labels.ravel().astype(np.int64)
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    area = np.bincount(flat, minlength=n)
    # every partial sum is an integer below 2^53: the float64 sums of bincount are exact
    sx = np.bincount(flat, weights=xs, minlength=n).astype(np.uint64)
    sy = np.bincount(flat, weights=ys, minlength=n).astype(np.uint64)
    lo_x = np.full(n, w, np.int64)
    lo_y = np.full(n, h, np.int64)
    hi_x = np.full(n, -1, np.int64)
    hi_y = np.full(n, -1, np.int64)
    np.minimum.at(lo_x, flat, xs)
    np.minimum.at(lo_y, flat, ys)
    np.maximum.at(hi_x, flat, xs)
    np.maximum.at(hi_y, flat, ys)
    k = min(n, stats_rows)
    full = np.stack([lo_x, lo_y, hi_x - lo_x + 1, hi_y - lo_y + 1, area], axis=1)[:k]
    full[area[:k] == 0] = 0
    stats[:k] = full
    sums[:k, 0] = sx[:k]
    sums[:k, 1] = sy[:k]
    return stats, sums


def ccl_ref(masks, connectivity=8, stats_rows=0, labeller=None):
    """(labels (n, h, w) int32, count (n,) int32, stats (n, stats_rows, 5) int32, sums (n, stats_rows, 2) uint64) of
    (h, w) or (n, h, w) masks, every frame on its own."""
    masks = np.ascontiguousarray(masks, np.uint8)
    if masks.ndim == 2:
        masks = masks[None]
    labeller = labeller or label
    nf, h, w = masks.shape
    labels = np.zeros((nf, h, w), np.int32)
    count = np.zeros(nf, np.int32)
    stats = np.zeros((nf, stats_rows, 5), np.int32)
    sums = np.zeros((nf, stats_rows, 2), np.uint64)
    for f in range(nf):
        labels[f], n = labeller(masks[f], connectivity)
        count[f] = n
        stats[f], sums[f] = stats_of(labels[f], n, stats_rows)
    return labels, count, stats, sums


def centroids_of(stats, sums):
    """sums / area as float64: what Context.ccl_gray8 returns (NaN for a row without a pixel)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums.astype(np.float64) / stats[..., 4:5].astype(np.float64)
