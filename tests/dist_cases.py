"""The shapes and contents of the distance transform tests (test_dist_cpu.py, test_gpu_dist.py).

The column launch of csrc/dist.hip cuts a frame into groups of COL_W columns and into whole chunks of CHUNK rows, at most
MAX_SEGS segments of chunks below each other: up to CHUNK * MAX_SEGS = 2048 rows a segment is one chunk, above that it is
several.  The row launch resolves a row in levels of a binary cut of its width (1030 lies just past a power of two) and
hands a query with more than LANE_RANGE candidates to the whole wave.  The shapes are the smallest at which that can go
wrong: one pixel, one row, one column, fewer pixels than a group, several groups and chunks with ragged edges, rows and
columns past 1024, and a height on either side of the 2048-row boundary.
"""
import numpy as np

COL_W, CHUNK, MAX_SEGS, LANE_RANGE = 64, 32, 64, 64   # test_dist_cpu.py reads them out of csrc/dist.hip
ONE_CHUNK_ROWS = CHUNK * MAX_SEGS                     # the tallest frame whose segments are single chunks

#         (w, h)
SHAPES = [(1, 1), (5, 3), (1, 300), (300, 1), (67, 48), (250, 130), (130, 250), (1030, 3), (3, 1030),
          (9, ONE_CHUNK_ROWS), (9, ONE_CHUNK_ROWS + 1)]
DENSITIES = (0.01, 0.5, 0.99)   # the share of pixels that are sites


def all_sites(h, w):
    return np.zeros((h, w), np.uint8)


def no_site(h, w):
    return np.full((h, w), 255, np.uint8)


def _single(y, x):
    def make(h, w):
        m = no_site(h, w)
        m[y(h), x(w)] = 0
        return m
    return make


def left_column(h, w):
    m = no_site(h, w)
    m[:, 0] = 0
    return m


def right_column(h, w):
    m = no_site(h, w)
    m[:, w - 1] = 0
    return m


def top_row(h, w):
    m = no_site(h, w)
    m[0] = 0
    return m


def bottom_row(h, w):
    m = no_site(h, w)
    m[h - 1] = 0
    return m


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) == 0).astype(np.uint8) * 255


def lattice(h, w, pitch=6):
    """sites on an even pitch: the pixels half way are equidistant from two sites, the cell centres from four"""
    m = no_site(h, w)
    m[1::pitch, 1::pitch] = 0
    return m


def two_columns(h, w):
    """two site columns an even distance apart (as far as the width allows): the column half way ties left and right"""
    m = no_site(h, w)
    a = min(2, w - 1)
    b = a + (w - 1 - a) // 2 * 2
    m[:, a] = 0
    m[:, b] = 0
    return m


def noise(h, w, density, seed=1):
    """site noise: a pixel is a site with probability `density`; the frames of the DENSITIES are consecutive draws"""
    rng = np.random.default_rng(seed)
    for d in DENSITIES:
        m = rng.random((h, w)) >= d
        if d == density:
            return m.astype(np.uint8) * 255
    raise ValueError("density %r is not one of DENSITIES" % (density,))


def blobs(h, w, seed=3):
    """an Otsu-like mask: a dozen filled ellipses (255) on a background of sites, some of them touching"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    for _ in range(12):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(1, max(h / 4, 2)), rng.uniform(1, max(w / 4, 2))
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 255
    return m


def other_values(h, w):
    """noise whose non-site bytes are 1, 2, 128 and 254: anything but zero is not a site"""
    rng = np.random.default_rng(7)
    v = np.array([1, 2, 128, 254], np.uint8)[rng.integers(0, 4, (h, w))]
    return np.where(rng.random((h, w)) < 0.8, v, 0).astype(np.uint8)


def seventh_columns(h, w):
    """sparse sites in every 7th column only: for most rows the neighbouring columns have no site at all"""
    rng = np.random.default_rng(11)
    m = no_site(h, w)
    sites = rng.random((h, w)) < 0.08
    sites[:, np.arange(w) % 7 != 3] = False
    sites[h // 2, min(3, w - 1)] = True      # at least one site, also in the narrowest frames
    m[sites] = 0
    return m


_first, _last, _mid = (lambda n: 0), (lambda n: n - 1), (lambda n: n // 2)
CONTENTS = [("all_sites", all_sites), ("no_site", no_site),
            ("site_top_left", _single(_first, _first)), ("site_top_right", _single(_first, _last)),
            ("site_bottom_left", _single(_last, _first)), ("site_bottom_right", _single(_last, _last)),
            ("site_middle", _single(_mid, _mid)),
            ("left_column", left_column), ("right_column", right_column), ("top_row", top_row), ("bottom_row", bottom_row),
            ("checkerboard", checkerboard), ("lattice", lattice), ("two_columns", two_columns)]
CONTENTS += [("noise_%g" % d, (lambda d: lambda h, w: noise(h, w, d))(d)) for d in DENSITIES]
CONTENTS += [("blobs", blobs), ("other_values", other_values), ("seventh_columns", seventh_columns)]


def frames_of(shape):
    """[(name, (h, w) uint8 mask)] of every content at shape = (w, h)"""
    w, h = shape
    return [(name, make(h, w)) for name, make in CONTENTS]


def border_sites(h, w):
    """only the frame's border is sites: sq = min(x, y, w - 1 - x, h - 1 - y)^2"""
    m = no_site(h, w)
    m[0] = m[h - 1] = 0
    m[:, 0] = m[:, w - 1] = 0
    return m


def border_sq(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(xx, yy), np.minimum(w - 1 - xx, h - 1 - yy)).astype(np.int64)
    return (d * d).astype(np.int32)


def corner_site_sq(h, w, y0, x0):
    """the squared distances of a frame whose only site is (x0, y0)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - y0).astype(np.int64) ** 2 + (xx - x0).astype(np.int64) ** 2).astype(np.int32)
