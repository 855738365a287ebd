"""Inputs and weight tables of the Gaussian table tests (test_gauss_tables_cpu.py, test_gpu_gauss_tables.py).

frames() builds one batch whose three frames share their RGB and differ in alpha, so that one launch covers the
4-channel pass (alpha noise), the opaque pass (alpha 255) and the constant-alpha pass (alpha 128) of the sliding-window
kernels.  The RGB holds what the kernels treat differently: noise (few flagged pixels), bright noise (sums that
saturate once a table's gain exceeds 1) and two flat 40 x 40 blocks, wider than a 17 x 17 window (constant windows: the
table path of the exact-by-exception stage; the 255-block is where a gain just above 1 first overflows a byte).
A plain numpy helper for those tests, not a fixture module.
"""
import numpy as np

# (h, w): aligned rows and 3 strips (131 * 512 >= 2^16: AUTO gives k >= 7 to the matrix cores); width % 4 == 2 (RAGGED
# sliding kernels, gauss_wide for k >= 11, frames 1 and 2 of the batch start unaligned); odd width (RAGGED; k >= 11 tiled).
# Each has several bands (odd ones walk upward) at every k.
SHAPES = ((131, 512), (97, 250), (53, 501))
BLOCK = 40

# part 1: generated tables
GRID_KS = (3, 5, 7, 9, 11, 17)
GRID_SIGMAS = (0.2, 0.35, 0.6, 1.0, 3.0, 10.0, 50.0)
EDGE_KS = (1, 31)
EDGE_SIGMAS = (0.35, 10.0)

# part 2: installed tables = base table * gain
BASES = ((3, 0.8), (5, 1.5), (7, 2.0), (9, 2.5), (11, 3.0), (17, 6.0))
GAINS = (0.5, 1.0035, 1.0038, 1.0039, 1.25, 2.0, 100.0)
ASYM_GAIN = 1.25
ASYM_FACTORS = {5: (0.05, 0.15, 0.4, 0.25, 0.15), 9: (0.02, 0.03, 0.05, 0.1, 0.3, 0.2, 0.15, 0.1, 0.05)}


def block_origin(h, w, which):
    """(y0, x0) of the 255-block (which = 255: in the noise half) or the 0-block (which = 0: in the bright half)."""
    if which == 255:
        return min(5, max(0, h - BLOCK)), min(10, max(0, w // 2 - BLOCK))
    return max(0, min(50, h - BLOCK - 5)), max(w // 2, w - BLOCK - 20)


def block_centre(h, w, which):
    y0, x0 = block_origin(h, w, which)
    return y0 + BLOCK // 2, x0 + BLOCK // 2


def frames(h, w, seed):
    """(3, h, w, 4) uint8: the same RGB three times; alpha noise / 255 / 128."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[:, w // 2:] = rng.integers(192, 256, (h, w - w // 2, 3), dtype=np.uint8)
    for which in (255, 0):
        y0, x0 = block_origin(h, w, which)
        rgb[y0:y0 + BLOCK, x0:x0 + BLOCK] = which   # slices clip to the frame
    out = np.empty((3, h, w, 4), np.uint8)
    out[..., :3] = rgb
    out[0, ..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    out[1, ..., 3] = 255
    out[2, ..., 3] = 128
    return out


def gray_plane(batch):
    """The single-channel test plane: frame 1's R channel."""
    return np.ascontiguousarray(batch[1, ..., 0])


def scaled(table, gain):
    return (table * np.float32(gain)).astype(np.float32)


def asym_table(k):
    """u (x) u with an asymmetric u (test_gpu_configs.py: test_asymmetric_separable_factor_keeps_its_orientation)."""
    u = np.array(ASYM_FACTORS[k], np.float32)
    return np.outer(u, u).astype(np.float32)
