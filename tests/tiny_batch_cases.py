"""Cases of the tiny-batch tests (test_tiny_batch_cpu.py, test_gpu_tiny_batch.py): batches of thousands of frames that are
smaller than a lane's quad, a 16-byte vector, a strip, a tile or a band.

Every kernel cuts a batch into work items with the same few rules (tile_common.hpp tile_decode, slide_common.hpp
slide_item, blockIdx.x / tiles in hist.hip, item / ncg / nstrips in median.hip), and frames lie back to back: frame f of
a gray8 batch starts at byte f * w * h, whatever alignment that gives.  A kernel may vector-load across a frame's end; it
must not use what it read there and must not store there.  A stray store across a frame boundary is usually invisible in
a batch of two frames (the next row overwrites it, or the right bytes win the race); it shows when many frames, each
owned by another wave, are all compared byte for byte.  And a few thousand tiny frames are enough work items for every
production band plan (make_band_plan halves the band height below 2800 work items), which otherwise takes a launch of
gigabytes.

Holds the shapes, the batch builder, the launch plans restated term by term from the sources (as large_k_cases.py
restates the LDS carves), and COUNTS: the frame counts on either side of each launch-size rule.  COUNTS is a table of
literals on purpose: test_tiny_batch_cpu.py puts every pair through the restated plans, so moving a threshold (there or,
through SOURCE_LINES, in the sources) fails that test and asks for new counts instead of the GPU tests silently standing
on one side.  A plain numpy helper, not a fixture module.
"""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl-development-real-time-image-processing_amd", "csrc")

# ---- shapes (h, w) ---------------------------------------------------------------------------------------------------
RGBA_WHY = collections.OrderedDict([
    ((1, 1), "one pixel: below a quad and below every halo"),
    ((1, 2), "below a quad, one row"),
    ((2, 1), "below a quad, one column"),
    ((1, 3), "below a quad: the widest frame of the per-pixel store forms (w < 4)"),
    ((3, 1), "one column, as tall as the smallest window"),
    ((2, 4), "the pipeline's smallest sliding shape (w >= 4, h >= 2)"),
    ((3, 5), "ragged: 15 output bytes per frame, every residue mod 4 and mod 16"),
    ((5, 7), "ragged: 35 output bytes per frame"),
    ((13, 17), "ragged: 221 output bytes per frame, more rows than a halved band"),
    ((9, 8), "whole quads, part of one strip"),
    ((7, 12), "whole quads, part of one strip, fewer rows than the widest windows"),
    ((6, 252), "63 quads: two strips per row, frames of one band"),
    ((16, 64), "one RGBA tile exactly, w >= 64: the matrix-core rule's shape"),
    ((75, 75), "the thumbnail size of bench.py's side figures: ragged, several bands"),
])
RGBA_SHAPES = tuple(RGBA_WHY)
G8_WHY = collections.OrderedDict(RGBA_WHY)
G8_WHY.update([
    ((4, 4), "exactly 16 bytes"),
    ((1, 17), "one byte over one 16-byte vector"),
    ((1, 33), "one byte over two 16-byte vectors"),
    ((32, 129), "one byte over morph's gray8 tile width of 128"),
])
G8_SHAPES = tuple(G8_WHY)
ODD_SHAPES = ((3, 5), (5, 7), (13, 17))          # odd frame sizes: consecutive frames start at every residue mod 16
# the shapes that also run at n_lo on the GPU: smallest sliding, ragged, two strips, aligned one-tile, several bands
THRESHOLD_SHAPES = ((2, 4), (5, 7), (6, 252), (16, 64), (75, 75))
MATRIX_SHAPE = (16, 64)

SIGMA = {3: 0.8, 5: 1.5, 7: 2.0, 9: 2.5, 11: 3.0, 17: 6.0}

# ---- batch content ---------------------------------------------------------------------------------------------------
P = 11                       # distinct frames a batch cycles through: frame f = member f % 11
FIRST, LAST_LOW, LAST_HIGH = P, P + 1, P + 2     # rows of distinct(): the first frame's and the last frame's own content
NDISTINCT = P + 3            # 13 of them appear in any one batch (one of the two last frames)
LOW, HIGH, MID = (0, 127), (128, 255), (64, 191)
ALPHA_NOISE, ALPHA_255, ALPHA_77 = 0, 1, 2


def member_range(i):
    """Even members draw bytes from 0 .. 127, odd members from 128 .. 255: a byte taken from a neighbouring frame is then
    far from any correct value.  11 is odd, so two ranges cannot alternate round the cycle: member 10, which sits between
    member 9 (high) and member 0 (low), draws from 64 .. 191, the one range that is neither neighbour's."""
    if i == FIRST or i == LAST_LOW:
        return LOW                               # frame 1 is member 1: high
    if i == LAST_HIGH:
        return HIGH
    return MID if i == P - 1 else (LOW if i % 2 == 0 else HIGH)


def member_alpha(i):
    """RGBA members draw alpha as noise, constant 255 and constant 77 in turn: the general, opaque and constant-alpha
    Gaussian passes in one launch."""
    return i % 3


_distinct = {}


def distinct(h, w, bpp):
    """(NDISTINCT, h, w[, 4]) uint8, read-only: members 0 .. 10, the first frame, the last frame in either range."""
    key = (h, w, bpp)
    if key not in _distinct:
        rng = np.random.default_rng(h * 100003 + w * 101 + bpp)
        out = np.empty((NDISTINCT, h, w, 4) if bpp == 4 else (NDISTINCT, h, w), np.uint8)
        for i in range(NDISTINCT):
            lo, hi = member_range(i)
            out[i] = rng.integers(lo, hi + 1, out.shape[1:], dtype=np.uint8)
            if bpp == 4 and member_alpha(i) == ALPHA_255:
                out[i, ..., 3] = 255
            if bpp == 4 and member_alpha(i) == ALPHA_77:
                out[i, ..., 3] = 77
        out.setflags(write=False)
        _distinct[key] = out
    return _distinct[key]


def frame_index(n):
    """(n,) row of distinct() for every frame: f % 11, except the first and the last frame; the last frame takes the
    range its neighbour n - 2 does not have."""
    assert n >= 3
    idx = np.arange(n) % P
    idx[0] = FIRST
    idx[-1] = LAST_LOW if member_range(int(idx[-2])) != LOW else LAST_HIGH
    return idx


def batch(h, w, n, bpp):
    """(n, h, w[, 4]) frames of one batch."""
    return np.ascontiguousarray(distinct(h, w, bpp)[frame_index(n)])


def expand(per_distinct, n):
    """The expected batch from the reference of every distinct frame (any dtype, (NDISTINCT, ...))."""
    return np.ascontiguousarray(np.asarray(per_distinct)[frame_index(n)])


# ---- the launch plans, restated ---------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


SLIDE_LANES_OUT_MAX = 62     # slide_common.hpp:37 kSlideLanesOutMax
SLIDE_WAVES_PER_BLOCK = 4    # slide_common.hpp:38
SMALL_LAUNCH = 2800          # slide_common.hpp:101 (make_band_plan) and gauss_slide.hip:683 (k = 5's 15-row rule)
MFMA_MIN_K = 7               # gauss.hip:32 kMfmaAutoMinK
MFMA_MIN_W = 64              # gauss.hip:49
MFMA_MIN_PIXELS = 1 << 16    # gauss.hip:49
SOBEL_BIG_PIXELS = 1 << 28   # sobel_slide.hip:282: the aligned-strip kernel and 48-lane strips
PIPE8_PIXELS = 10 ** 9       # sobel_tile.hip:218: 8 pixels per lane
RESIZE_STRIP = 256           # resize.hip:26 kResizeStrip = kWave * kResizePx
RESIZE_BAND_MAX = 16         # resize.hip:28
RESIZE_MIN_WORK = 4096       # resize.hip:29
RGBA_TILE = (16, 64)         # tile_common.hpp:18-19 kRgbaTH x kRgbaTW

StripPlan = collections.namedtuple("StripPlan", "quads nstrips lanes_out")
BandPlan = collections.namedtuple("BandPlan", "rows_big rows_a nbands_a rows_b nbands_b y_split nwork_a nwork_b")
TileGrid = collections.namedtuple("TileGrid", "tiles_x tiles_y ntiles")
Launch = collections.namedtuple("Launch", "kernel rows nwork")


def make_strip_plan(w, lanes_pref=0):
    """slide_common.hpp:54 make_strip_plan (without the tuning override)."""
    quads = (w + 3) // 4
    nstrips = _ceil_div(quads, SLIDE_LANES_OUT_MAX)
    lanes_out = _ceil_div(quads, nstrips)
    if 0 < lanes_pref <= SLIDE_LANES_OUT_MAX and nstrips > 1:
        lanes_out, nstrips = lanes_pref, _ceil_div(quads, lanes_pref)
    return StripPlan(quads, nstrips, lanes_out)


def make_band_plan(h, nstrips, nframes, waves_per_simd, rows_min, rows_max, rows_tail, tail_frac, rows_small):
    """slide_common.hpp:80 make_band_plan (without the tuning overrides); rows_big is the height before balancing."""
    resident = 256.0 * 4.0 * waves_per_simd
    rows = float(h) * nstrips * nframes / (10.0 * resident)
    rows_big = int(rows_min if rows < rows_min else (rows_max if rows > rows_max else rows))
    while rows_small > 0 and rows_big // 2 >= rows_small and nstrips * _ceil_div(h, rows_big) * nframes < SMALL_LAUNCH:
        rows_big //= 2
    h_b = int(h * tail_frac)
    if h_b < rows_tail or h - h_b < rows_big or tail_frac <= 0.0 or rows_tail >= rows_big:
        h_b = 0
    h_a = h - h_b
    nbands_a = _ceil_div(h_a, rows_big)
    rows_a = _ceil_div(h_a, nbands_a)
    nbands_b = _ceil_div(h_b, rows_tail) if h_b > 0 else 0
    rows_b = _ceil_div(h_b, nbands_b) if h_b > 0 else 1
    na, nb = nstrips * nbands_a * nframes, nstrips * nbands_b * nframes
    assert na + nb <= 0x3FFFFFFF
    return BandPlan(rows_big, rows_a, nbands_a, rows_b, nbands_b, h_a, na, nb)


def tile_grid(w, h, nframes, tw, th):
    """tile_common.hpp:23 TileGrid."""
    tx, ty = _ceil_div(w, tw), _ceil_div(h, th)
    return TileGrid(tx, ty, tx * ty * nframes)


# family -> (waves per SIMD, rows_min, rows_max, rows_tail, tail_frac, rows_small): the make_band_plan call of
# gauss_slide.hip:685-688 (slide_plan; k = 5 is gauss5_plan below), gauss_wide.hip:213, gauss_exact.hip:160-162,
# sobel_slide.hip:298 and pipe_slide.hip:324-325 (4 pixels per lane)
BAND_ARGS = {
    ("gauss", 3): (5, 12, 12, 12, 0.0, 6),
    ("gauss", 7): (3, 96, 270, 40, 0.1, 4 * 3 + 4),
    ("gauss", 9): (3, 96, 270, 40, 0.1, 4 * 4 + 4),
    ("gauss", 11): (2, 128, 360, 48, 0.1, 4 * 5),
    ("gauss", 17): (2, 128, 360, 48, 0.1, 4 * 8),
    ("exact", 3): (5, 16, 16, 16, 0.0, 8),
    ("exact", 5): (3, 24, 24, 24, 0.0, 12),
    ("exact", 7): (2, 40, 40, 40, 0.0, 20),
    ("sobel", 0): (8, 16, 16, 16, 0.0, 8),
    ("pipe", 3): (8, 16, 16, 16, 0.0, 8),
    ("pipe", 5): (8, 24, 24, 24, 0.0, 12),
    ("pipe", 7): (8, 40, 40, 40, 0.0, 20),
}
# the band height a big batch gets, and what a launch below SMALL_LAUNCH work items is left with
PRODUCTION_ROWS = {("gauss", 3): 12, ("gauss", 5, "aligned"): 15, ("gauss", 5, "ragged"): 24, ("gauss", 7): 96,
                   ("gauss", 9): 96, ("gauss", 11): 128, ("gauss", 17): 128, ("exact", 3): 16, ("exact", 5): 24,
                   ("exact", 7): 40, ("sobel", 0): 16, ("pipe", 3): 16, ("pipe", 5): 24, ("pipe", 7): 40}
HALVED_ROWS = {("gauss", 3): 6, ("gauss", 5, "aligned"): 12, ("gauss", 5, "ragged"): 12, ("gauss", 7): 24,
               ("gauss", 9): 24, ("gauss", 11): 32, ("gauss", 17): 32, ("exact", 3): 8, ("exact", 5): 12,
               ("exact", 7): 20, ("sobel", 0): 8, ("pipe", 3): 8, ("pipe", 5): 12, ("pipe", 7): 20}
FAMILIES = tuple(sorted(set(BAND_ARGS) | {("gauss", 5)}))

# the lines of the sources the restatement above follows: if one of them changes, so must the restatement and COUNTS
SOURCE_LINES = [
    ("slide_common.hpp", "constexpr int kSlideLanesOutMax = 62;"),
    ("slide_common.hpp", "(size_t)nstrips * ((h + rows_big - 1) / rows_big) * nframes < 2800)"),
    ("slide_common.hpp", "while (rows_small > 0 && rows_big / 2 >= rows_small &&"),
    ("gauss_slide.hip", "const bool big = (size_t)sp->nstrips * ((h + 23) / 24) * nframes >= 2800;"),
    ("gauss_slide.hip", "const int rows = (big && !ragged) ? 15 : 24;"),
    ("gauss_slide.hip", "return make_band_plan(h, sp->nstrips, nframes, 4, rows, rows, rows, 0.0, 12, plan);"),
    ("gauss_slide.hip", "make_band_plan(h, sp->nstrips, nframes, 5, 12, 12, 12, 0.0, 6, plan)"),
    ("gauss_slide.hip", "make_band_plan(h, sp->nstrips, nframes, 3, 96, 270, 40, 0.1, 4 * R + 4, plan);"),
    ("gauss_wide.hip", "return make_band_plan(h, nstrips, nframes, 2, 128, 360, 48, 0.1, 4 * R, plan);"),
    ("gauss_exact.hip", "constexpr int kRows = (R == 1) ? 16 : (R == 2 ? 24 : 40);"),
    ("gauss_exact.hip", "make_band_plan(h, sp.nstrips, nframes, kWavesPerSimd, kRows, kRows, kRows, 0.0, kRows / 2, &plan)"),
    ("sobel_slide.hip", "if (!make_band_plan(h, sp.nstrips, nframes, 8, 16, 16, 16, 0.0, 8, &plan))"),
    ("sobel_slide.hip", "const bool big = (size_t)w * h * nframes >= ((size_t)1 << 28) || kStripMode == 2;"),
    ("pipe_slide.hip", "constexpr int kRows = (R == 1) ? 16 : (R == 2 ? 24 : 40);"),
    ("pipe_slide.hip", "planned = make_band_plan(h, nstrips, nframes, 8, kRows, kRows, kRows, 0.0, kRows / 2, &plan);"),
    ("pipe_slide.hip", "if (w < 4 || h < 2 || !exact_tables_ok(coef) || !aligned_to(d_in, 4))"),
    ("sobel_tile.hip", "bool want8 = coef.k == 5 && lanes8 >= 56 && (size_t)w * h * nframes >= 1000000000ull;"),
    ("gauss.hip", "constexpr int kMfmaAutoMinK = 7;"),
    ("gauss.hip", "coef.k >= kMfmaAutoMinK && w >= 64 && (size_t)w * h * nframes >= (1u << 16))"),
    ("resize.hip", "constexpr int kResizeBandMax = 16;"),
    ("resize.hip", "constexpr size_t kResizeMinWork = 4096;"),
    ("resize.hip", "while (a.band_rows > 1 && nwork(a.band_rows) < kResizeMinWork)"),
    ("tile_common.hpp", "constexpr int kRgbaTW = 64;"),
    ("tile_common.hpp", "constexpr int kRgbaTH = 16;"),
]


def gauss5_plan(h, w, n, ragged):
    """gauss_slide.hip:682-686: k = 5 takes 15-row bands from SMALL_LAUNCH 24-row work items on, aligned rows only."""
    sp = make_strip_plan(w)
    big = sp.nstrips * _ceil_div(h, 24) * n >= SMALL_LAUNCH
    rows = 15 if (big and not ragged) else 24
    return make_band_plan(h, sp.nstrips, n, 4, rows, rows, rows, 0.0, 12)


def launch_of(family, h, w, n):
    """Which kernel a call on 16-byte aligned buffers runs, its band height before balancing (None for a tiled kernel)
    and its work items.  family: ("gauss", k) = FAST under IMPL_VALU (gauss.hip:51-55 choose), ("exact", k) = EXACT under
    IMPL_AUTO (gauss.hip:39-42), ("sobel", 0) and ("pipe", k) under IMPL_AUTO (sobel_tile.hip:198, :224)."""
    name, k = family
    ragged = w % 4 != 0                                      # common.hpp:46 rows_ragged with aligned pointers
    tiles = tile_grid(w, h, n, RGBA_TILE[1], RGBA_TILE[0])
    if name == "gauss" and k == 5:
        p = gauss5_plan(h, w, n, ragged)
        return Launch("gauss_slide", p.rows_big, p.nwork_a + p.nwork_b)
    if name == "gauss" and k in (3, 7, 9):                   # gauss_slide.hip:745 gauss_slide_supported: any w, h
        p = make_band_plan(h, make_strip_plan(w).nstrips, n, *BAND_ARGS[family])
        return Launch("gauss_slide", p.rows_big, p.nwork_a + p.nwork_b)
    if name == "gauss":                                      # gauss_wide.hip:242 gauss_wide_supported: even widths
        if w % 2:
            return Launch("gauss_tile", None, tiles.ntiles)
        r = k // 2
        pairs, lanes_max = w // 2, 64 - 2 * ((r + 1) // 2)   # gauss_wide.hip:208-212 wide_plan
        p = make_band_plan(h, _ceil_div(pairs, lanes_max), n, *BAND_ARGS[family])
        return Launch("gauss_wide", p.rows_big, p.nwork_a + p.nwork_b)
    if name == "exact":                                      # gauss_exact.hip:184 gauss_exact_supported
        if ragged:
            return Launch("gauss_tile", None, tiles.ntiles)
        p = make_band_plan(h, make_strip_plan(w).nstrips, n, *BAND_ARGS[family])
        return Launch("gauss_exact", p.rows_big, p.nwork_a + p.nwork_b)
    if name == "sobel":
        assert w * h * n < SOBEL_BIG_PIXELS
        p = make_band_plan(h, make_strip_plan(w, 0).nstrips, n, *BAND_ARGS[family])
        return Launch("sobel_slide", p.rows_big, p.nwork_a + p.nwork_b)
    assert name == "pipe" and w * h * n < PIPE8_PIXELS
    if w < 4 or h < 2:                                       # pipe_slide.hip:353
        return Launch("pipeline_tile", None, tiles.ntiles)
    p = make_band_plan(h, make_strip_plan(w).nstrips, n, *BAND_ARGS[family])
    return Launch("pipe_slide", p.rows_big, p.nwork_a + p.nwork_b)


def rows_key(family, w):
    return family + (("ragged" if w % 4 else "aligned"),) if family == ("gauss", 5) else family


def auto_takes_matrix_cores(h, w, n, k):
    """gauss.hip:49 with aligned buffers and a generated table (gauss_mfma_reg.hip:341 gauss_mfma_reg_supported)."""
    return 3 <= k <= 17 and w % 4 == 0 and k >= MFMA_MIN_K and w >= MFMA_MIN_W and w * h * n >= MFMA_MIN_PIXELS


def resize_band_rows(dw, dh, n):
    """resize.hip:342-346: (rows per band, work items)."""
    nstrips = _ceil_div(dw, RESIZE_STRIP)
    rows = RESIZE_BAND_MAX
    while rows > 1 and nstrips * _ceil_div(dh, rows) * n < RESIZE_MIN_WORK:
        rows //= 2
    return rows, nstrips * _ceil_div(dh, rows) * n


# ---- frame counts ----------------------------------------------------------------------------------------------------
SLIDE_CAP = 16 << 20         # bytes of the largest input batch: 75 x 75 x 700 RGBA is 15.75 MB
TILE_CAP = 4 << 20           # kernels without a launch-size rule
TILE_COUNTS = (3001, 699, 301, 101)   # odd, no multiple of 8 or of 4 waves per block: the first that fits TILE_CAP


def tile_count(h, w, bpp):
    return next(n for n in TILE_COUNTS if h * w * bpp * n <= TILE_CAP)


# (n_lo, n_hi) per (family, shape): n_hi is the first count at which the launch has SMALL_LAUNCH work items of the
# production height, n_lo = n_hi - 1 the last that is halved.  (None, n): the rule is out of reach below SLIDE_CAP
# (gauss_slide k >= 7 at 75 x 75 needs 2800 frames = 63 MB, pipe_slide k = 7 1400 = 31.5 MB: they take the k = 5 count),
# or a tiled kernel serves the shape (tile_count).  Literals, so that a moved threshold cannot move them along.
COUNTS = {(_f, _s): (2799, 2800) for _f in FAMILIES for _s in RGBA_SHAPES}        # one strip, one band
for _f in FAMILIES:
    COUNTS[_f, (6, 252)] = (1399, 1400)                       # 63 quads: two strips, one band
COUNTS.update({
    (("gauss", 3), (13, 17)): (1399, 1400),                   # 2 bands of 12 rows
    (("gauss", 3), (16, 64)): (1399, 1400),
    (("gauss", 3), (75, 75)): (399, 400),                     # 7 bands of 12 rows
    (("gauss", 5), (75, 75)): (699, 700),                     # 4 bands of 24 rows: ragged, keeps them
    (("gauss", 7), (75, 75)): (None, 700),
    (("gauss", 9), (75, 75)): (None, 700),
    (("gauss", 11), (6, 252)): (933, 934),                    # 126 pixel pairs in strips of <= 58 lanes: three strips
    (("gauss", 17), (6, 252)): (933, 934),                    # ... of <= 56 lanes
    (("sobel", 0), (75, 75)): (559, 560),                     # 5 bands of 16 rows
    (("pipe", 3), (75, 75)): (559, 560),
    (("pipe", 5), (75, 75)): (699, 700),
    (("pipe", 7), (75, 75)): (None, 700),
})
for _s in RGBA_SHAPES:
    _t = (None, tile_count(_s[0], _s[1], 4))
    for _k in (3, 5, 7):
        if _s[1] % 4:                                         # EXACT: ragged widths go to the tiled kernel
            COUNTS[("exact", _k), _s] = _t
        if _s[1] < 4 or _s[0] < 2:                            # pipe_slide: w >= 4 and h >= 2
            COUNTS[("pipe", _k), _s] = _t
    for _k in (11, 17):
        if _s[1] % 2:                                         # gauss_wide: even widths only
            COUNTS[("gauss", _k), _s] = _t
MATRIX_COUNTS = (63, 64)     # 16 x 64 x 63 = 64512 pixels, x 64 = 65536 = MFMA_MIN_PIXELS


def counts(family, shape):
    return COUNTS[family, shape]


# ---- resize -----------------------------------------------------------------------------------------------------------
# (src w, src h, dst w, dst h): the pairs of test_resize_cpu.SMALL_PAIRS with at most 14 x 10 pixels on either side, and
# 5 x 7 -> 3 x 4 rows x columns, one pixel up, 4 x 4 -> 2 x 2 (LINEAR's switch to AREA), 6 x 8 -> 3 x 2 (AREA 4 x 2)
RESIZE_PAIRS = [(1, 1, 1, 1), (1, 1, 5, 3), (5, 3, 1, 1), (2, 2, 17, 3), (7, 5, 13, 9), (13, 9, 7, 5), (12, 8, 6, 4),
                (14, 10, 7, 5), (7, 5, 4, 3), (1, 1, 3, 3), (4, 4, 2, 2), (8, 6, 2, 3)]
RESIZE_COUNTS = (4095, 4096)  # every pair has one strip and, at 16 rows, one band


# ---- the comparison ----------------------------------------------------------------------------------------------------
def where(index, frame_bytes, row_bytes):
    """'frame f row y byte x' of a payload index."""
    f, r = divmod(int(index), frame_bytes)
    return "frame %d row %d byte %d (frame of %d bytes)" % (f, r // row_bytes, r % row_bytes, frame_bytes)
