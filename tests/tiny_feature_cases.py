"""Cases of the tiny-batch tests of the per-frame features (test_tiny_batch_features_cpu.py,
test_gpu_tiny_batch_features.py): CLAHE, the mean adaptive threshold, connected-component labelling, hysteresis, Canny
and the Hough transform on the batches of tiny_batch_cases.py, thousands of back-to-back frames each.

These kernels carry the most per-frame machinery of the code base: ccl.hip decodes a frame index from blockIdx.x in six
kernels and keeps one scratch count per 2048-pixel flat block of every frame, canny.hip cuts 16-byte chunks apart where
one straddles two frames, hough.hip keeps a counter, a point list and a candidate list per frame in one pooled buffer,
clahe.hip walks (frame, tile, band) and (frame, row group, chunk).  A pixel linked, counted or blended across a frame
boundary is invisible in a batch of three frames; here every frame's neighbours hold other content and every byte of
every frame is compared.

None of these kernels has a launch-size rule (no band plan, no threshold on the number of work items), so there is no
n_lo / n_hi pair as in tiny_batch_cases.COUNTS: a row runs at ONE count, the first of tb.TILE_COUNTS whose largest arena
(the input plus every output of one call, as tests/guarded.py lays them out) stays within ARENA_CAP.  That is a budget
condition, not a measurement: it keeps a call's copies in the milliseconds and a test in seconds.  It bites on the
int32 labels (4 B/px), the CLAHE tables (16 KB per frame at 8 x 8) and the Hough accumulators (19.6 KB per 5 x 7 frame at
theta = pi / 180, 45.9 KB per 13 x 17 frame).  ARENA_CAP is tb.SLIDE_CAP, the largest batch of test_gpu_tiny_batch.py:
at 64 MiB the GPU file took 26.9 s on the MI355X host against that file's 15.8 s, nearly all of it the host filling and
comparing arenas, so the counts were cut by the rule above (13.0 s against 15.9 s); no shape was.  A plain numpy helper, not a fixture module.
"""
import collections
import math

import numpy as np

import canny_cases as kc
import ccl_cases as cc
import guarded
import hough_cases as hc
import tiny_batch_cases as tb

ARENA_CAP = tb.SLIDE_CAP
OFF_WORST = (3, 4)           # the largest offsets the GPU file uses

# ---- shapes (h, w), beside tb.G8_SHAPES ---------------------------------------------------------------------------------
SEAM_SHAPE = (33, 65)        # one past ccl.hip's 64 x 32 tile each way: four tiles and their seams in every frame
NMS_SHAPE = (17, 257)        # one past canny.hip's 256 x 16 non-maximum-suppression tile each way
assert (SEAM_SHAPE[1], SEAM_SHAPE[0]) == (cc.TILE_W + 1, cc.TILE_H + 1)
assert (NMS_SHAPE[1], NMS_SHAPE[0]) == (kc.NMS_TW + 1, kc.NMS_TH + 1)
HOUGH_MAX = (13, 17)         # the accumulator of a 13 x 17 frame is 45.9 KB already

CLAHE_GRIDS = ((1, 1), (2, 2), (8, 8))       # (tiles_x, tiles_y)
CLAHE_CLIPS = (2.0, 40.0)
ADAPTIVE_PARAMS = [(255, 0, 3, 2.5), (200, 1, 3, 2.5), (255, 0, 17, -1.25), (200, 1, 17, -1.25)]  # max, type, block, delta
CCL_STATS_ROWS = (0, 4)
HYST_PARAMS = [(kc.LOW, kc.HIGH, 4), (kc.LOW, kc.HIGH, 8), (kc.LOW, 255, 8)]   # high = 255: no mark launch runs
CANNY_PARAMS = [(50, 150, 0), (37.5, 112.5, 1)]
HOUGH_COARSE = (1.0, hc.PI / 90, 0.0, hc.PI)
HOUGH_GEOMS = (hc.DEFAULT, HOUGH_COARSE)
# (threshold, max_lines): more peaks than lines, so the radix select runs; fewer, so the output is zero-filled
HOUGH_SELECT = ((0, 7), (2, 64))

Row = collections.namedtuple("Row", "shape params out_bytes n")   # out_bytes: the largest output of one call, per frame


def arena_bytes(nin, nout, off_in=OFF_WORST[0], off_out=OFF_WORST[1]):
    """guarded.run's `total` for an input of nin and a payload of nout bytes"""
    up = lambda x: (x + 255) // 256 * 256                      # noqa: E731
    out_region = up(guarded.GUARD + off_in + nin + guarded.GUARD)
    return up(out_region + guarded.GUARD + off_out + nout + guarded.GUARD + guarded.GUARD)


def count_of(h, w, out_bytes):
    """The first of tb.TILE_COUNTS at which a call with out_bytes of output per frame (alignment gaps: at most 8 more
    bytes per call) stays within ARENA_CAP."""
    return next(n for n in tb.TILE_COUNTS if arena_bytes(n * h * w, n * out_bytes + 8) <= ARENA_CAP)


def _rows(shapes, params, out_bytes, accepts):
    return [Row(s, p, out_bytes(s, p), count_of(s[0], s[1], out_bytes(s, p))) for s in shapes for p in params
            if accepts(s, p) == 0]


def ccl_out_bytes(shape, stats_rows):
    """labels, count, stats and sums of one frame"""
    return 4 * shape[0] * shape[1] + 4 + 20 * stats_rows + 16 * stats_rows


def hough_out_bytes(pkg, shape, geom, max_lines):
    """lines, votes, count and the caller's accumulator of one frame"""
    na, nr = pkg.hough_shape(shape[1], shape[0], *geom)
    return 8 * max_lines + 4 * max_lines + 4 + 4 * (na + 2) * (nr + 2)


def clahe_rows(pkg):
    """params = (tiles_x, tiles_y); the row serves both clip limits and both calls (the frames and the tables)"""
    return _rows(tb.G8_SHAPES, CLAHE_GRIDS, lambda s, g: max(s[0] * s[1], 256 * g[0] * g[1]),
                 lambda s, g: max(pkg.clahe_check(s[1], s[0], 1, c, g[0], g[1]) for c in CLAHE_CLIPS))


def adaptive_rows(pkg):
    return _rows(tb.G8_SHAPES, ADAPTIVE_PARAMS, lambda s, p: s[0] * s[1],
                 lambda s, p: pkg.adaptive_threshold_check(s[1], s[0], 1, *p))


def ccl_rows(pkg):
    """params = (connectivity, stats_rows)"""
    return _rows(tb.G8_SHAPES + (SEAM_SHAPE,), [(c, r) for c in cc.CONNECTIVITIES for r in CCL_STATS_ROWS],
                 lambda s, p: ccl_out_bytes(s, p[1]), lambda s, p: pkg.ccl_check(s[1], s[0], 1, *p))


def hyst_rows(pkg):
    return _rows(tb.G8_SHAPES + (SEAM_SHAPE,), HYST_PARAMS, lambda s, p: s[0] * s[1],
                 lambda s, p: pkg.hysteresis_check(s[1], s[0], 1, *p))


def canny_rows(pkg):
    return _rows(tb.G8_SHAPES + (NMS_SHAPE,), CANNY_PARAMS, lambda s, p: s[0] * s[1],
                 lambda s, p: pkg.canny_check(s[1], s[0], 1, *p))


def hough_shapes():
    return tuple(s for s in tb.G8_SHAPES if s[0] <= HOUGH_MAX[0] and s[1] <= HOUGH_MAX[1])


def hough_rows(pkg):
    """params = (rho, theta, min_theta, max_theta); the row is sized by its largest call, max_lines = 64 with the
    caller's accumulator"""
    ml = max(m for _, m in HOUGH_SELECT)
    return _rows(hough_shapes(), HOUGH_GEOMS, lambda s, g: hough_out_bytes(pkg, s, g, ml),
                 lambda s, g: max(pkg.hough_check(s[1], s[0], 1, g[0], g[1], t, m, g[2], g[3]) for t, m in HOUGH_SELECT))


ROWS = collections.OrderedDict([("clahe", clahe_rows), ("adaptive", adaptive_rows), ("ccl", ccl_rows),
                                ("hysteresis", hyst_rows), ("canny", canny_rows), ("hough", hough_rows)])
# The fewest (shape, parameter) rows a feature may have: every shape at every parameter set, but for CLAHE, whose check
# refuses a grid whose pad one reflection cannot serve: all 18 shapes take 1 x 1; 2 x 2 takes the 11 with more than
# one row and more than one column; 8 x 8 takes the 7 whose pad (both ways as soon as one way
# does not divide) stays below the frame's size.  A check that starts refusing shapes must not silently empty a test.
MIN_ROWS = {"clahe": 18 + 11 + 7, "adaptive": 18 * 4, "ccl": 19 * 4, "hysteresis": 19 * 3, "canny": 19 * 2, "hough": 13 * 2}


def shapes_of(rows):
    return list(collections.OrderedDict((r.shape, None) for r in rows))


# ---- mask content (labelling, Hough) --------------------------------------------------------------------------------------
FOREGROUND_VALUES = (1, 2, 128, 254)


def corners(h, w):
    """the flat indices of the four corners (they coincide in a 1 x 1 frame and in one-row and one-column frames)"""
    return sorted({0, w - 1, (h - 1) * w, h * w - 1})


_masks = {}


def mask_distinct(h, w):
    """(tb.NDISTINCT, h, w) uint8, read-only, the rows tb.frame_index picks from: member i is seeded site noise of
    density cc.DENSITIES[i % 4] with the four corners forced to foreground, so that the last row of any frame and the
    first row of the next hold foreground in the same column (a link, a vote or a count taken across the boundary
    changes the answer); the foreground bytes are 255 in even members and drawn from FOREGROUND_VALUES in odd ones."""
    if (h, w) not in _masks:
        rng = np.random.default_rng(h * 100003 + w * 101 + 17)
        out = np.empty((tb.NDISTINCT, h, w), np.uint8)
        for i in range(tb.NDISTINCT):
            on = rng.random((h, w)) < cc.DENSITIES[i % 4]
            on.ravel()[corners(h, w)] = True
            values = np.array(FOREGROUND_VALUES, np.uint8)[rng.integers(0, 4, (h, w))]
            out[i] = np.where(on, values if i % 2 else 255, 0)
        out.setflags(write=False)
        _masks[h, w] = out
    return _masks[h, w]


def mask_batch(h, w, n):
    return np.ascontiguousarray(mask_distinct(h, w)[tb.frame_index(n)])


# ---- response content (hysteresis) ------------------------------------------------------------------------------------------
def is_strong(i):
    """Odd members of the cycle hold strong pixels, even ones (member 10 included) none at all.  The first frame is
    weak; of the two last frames LAST_LOW is weak and LAST_HIGH strong, and tb.frame_index picks the one whose class
    the frame before it lacks (test_tiny_batch_features_cpu.py asserts that for every count in use)."""
    if i == tb.FIRST or i == tb.LAST_LOW:
        return False
    if i == tb.LAST_HIGH:
        return True
    return i % 2 == 1


_responses = {}


def response_distinct(h, w):
    """(tb.NDISTINCT, h, w) uint8, read-only: kc.FG on the mask of mask_distinct, kc.BG elsewhere.  A strong member has
    kc.STRONG in all four corners and on one more foreground pixel in 400; a weak member has no byte above kc.HIGH, so its
    reference output is all zero, and any 255 in it came across a frame boundary."""
    if (h, w) not in _responses:
        rng = np.random.default_rng(h * 100003 + w * 101 + 29)
        masks = mask_distinct(h, w)
        out = np.where(masks != 0, kc.FG, kc.BG).astype(np.uint8)
        for i in range(tb.NDISTINCT):
            if is_strong(i):
                flat = out[i].reshape(-1)
                flat[(masks[i].reshape(-1) != 0) & (rng.random(h * w) < 1.0 / 400.0)] = kc.STRONG
                flat[corners(h, w)] = kc.STRONG
        out.setflags(write=False)
        _responses[h, w] = out
    return _responses[h, w]


def response_batch(h, w, n):
    return np.ascontiguousarray(response_distinct(h, w)[tb.frame_index(n)])


def weak_frames(n):
    """(n,) bool: the frames whose hysteresis output must be all zero"""
    return np.array([not is_strong(int(i)) for i in tb.frame_index(n)])


def neighbour_pairs(counts):
    """the (member, member) pairs that are consecutive frames in a batch of any of `counts` frames"""
    pairs = set()
    for n in counts:
        idx = tb.frame_index(n).tolist()
        pairs |= set(zip(idx, idx[1:]))
    return sorted(pairs)


def stacked(a, b):
    """two frames as one (2h, w) raster: the model of a kernel that takes the next frame's rows for its own"""
    return np.concatenate([a, b], axis=0)


def starts_mod(n, frame_bytes, m=16):
    """the residues mod m at which the frames of a batch of n start"""
    return set(((np.arange(n, dtype=np.int64) * frame_bytes) % m).tolist())


assert math.gcd(15, 16) == math.gcd(35, 16) == math.gcd(221, 16) == 1          # tb.ODD_SHAPES, 1-byte outputs
