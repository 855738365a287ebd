"""The CLAHE case list: (w, h, tiles_x, tiles_y, clip), each run on the three contents below.

Together the cases reach every branch of tests/clahe_ref.py (tests/test_clahe_cpu.py asserts each one by name): batch > 0
and batch == 0, residual == 0, step == 1, step == 2 and step >= 3, a table product exactly on .5, a blended res exactly on
.5, both padding quirks (only the width, only the height fails to divide) and 1-pixel tiles.  A plain module shared by
the CPU and the GPU tests.
"""
import numpy as np

CASES = [
    (64, 48, 8, 8, 2.0),
    (64, 48, 8, 8, 40.0),
    (64, 48, 8, 8, 0.0),
    (67, 48, 8, 8, 2.0),     # only the width fails to divide: 8 whole rows are padded too
    (64, 50, 8, 8, 3.0),     # only the height fails to divide: 8 whole columns are padded too
    (61, 45, 4, 3, 4.0),
    (16, 16, 16, 16, 40.0),  # 1-pixel tiles
    (33, 17, 1, 1, 2.0),
    (100, 7, 5, 1, 1.5),
    (7, 100, 1, 5, 0.5),
    (250, 130, 8, 8, 4.0),
    (480, 270, 3, 2, 2.0),
    (1, 1, 1, 1, 1.0),
    (31, 17, 16, 16, 2.0),
]


def uniform_noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def low_contrast(h, w, seed):
    """noise in 100 .. 123: every tile's counts sit in 24 bins, far above any clip limit"""
    return np.random.default_rng(seed).integers(100, 124, (h, w), dtype=np.uint8)


def wrapped_gradient(h, w, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((3 * xx + 5 * yy + seed) & 0xFF).astype(np.uint8)


CONTENTS = [uniform_noise, low_contrast, wrapped_gradient]


def frames_of(case):
    """[(content name, (h, w) frame)] of one case; the seed depends on the case alone."""
    w, h = case[0], case[1]
    seed = 1000 * w + h + 7 * case[2] + case[3]
    return [(make.__name__, make(h, w, seed)) for make in CONTENTS]
