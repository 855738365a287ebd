"""The shapes and contents of the labelling tests (test_ccl_cpu.py, test_gpu_ccl.py).

The kernels work on 64 x 32 tiles (TILE_W x TILE_H of csrc/ccl.hip) and on flat blocks of 2048 raster-consecutive
pixels (FLAT_PX); the shapes are the smallest at which that walk can go wrong: one pixel, one row, one column, fewer
pixels than a tile, several tiles each way with ragged edges, a whole number of tiles, and that plus one.
"""
import numpy as np

TILE_W, TILE_H, FLAT_PX = 64, 32, 2048

#         (w, h)
SHAPES = [(1, 1), (1, 300), (300, 1), (5, 3), (67, 48), (250, 130), (130, 250), (2 * TILE_W, 2 * TILE_H),
          (2 * TILE_W + 1, 2 * TILE_H + 1)]
CONNECTIVITIES = (4, 8)
DENSITIES = (0.3, 0.41, 0.59, 0.8)  # site percolation: below, at the 8-connected threshold, at the 4-connected, above
STATS_ROWS = 64                     # of the all-cases test: some noise frames have more labels, some fewer


def background(h, w):
    return np.zeros((h, w), np.uint8)


def foreground(h, w):
    return np.full((h, w), 255, np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) == 0).astype(np.uint8) * 255


def noise(h, w, density, seed=1):
    """site noise: the frames of the four DENSITIES are consecutive draws of one generator.  At seed 1 on 250 x 130 the
    reference counts N = 4137 at 0.3, 4-connected, and N = 38 at 0.59, 8-connected, with one component of 19095 pixels"""
    rng = np.random.default_rng(seed)
    for d in DENSITIES:
        m = rng.random((h, w)) < d
        if d == density:
            return m.astype(np.uint8) * 255
    raise ValueError("density %r is not one of DENSITIES" % (density,))


def diagonal(h, w):
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(h, w))
    m[k, k] = 255
    return m


def anti_diagonal(h, w):
    return diagonal(h, w)[:, ::-1].copy()


def serpentine(h, w):
    """a one-pixel line: every other row whole, joined at alternating ends"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 255
    for i, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if i % 2 == 0 else 0] = 255
    return m


def spiral(h, w):
    """a one-pixel rectangular spiral from the top-left corner inwards, one background pixel between its arms: ring r is
    the outline of the rectangle 2r pixels in from every edge, opened one pixel below its top-left corner, and a
    two-pixel bridge from the upper end of its left side leads into ring r + 1"""
    m = np.zeros((h, w), np.uint8)
    t, l, b, r = 0, 0, h - 1, w - 1
    while t <= b and l <= r:
        m[t, l:r + 1] = 255
        m[t:b + 1, r] = 255
        if b - t < 2 or r - l < 2:
            break
        m[b, l:r + 1] = 255
        m[t + 2:b + 1, l] = 255
        if b - t < 4 or r - l < 4:
            break
        m[t + 2, l:l + 2] = 255
        t, l, b, r = t + 2, l + 2, b - 2, r - 2
    return m


def comb(h, w):
    """teeth in every other column that join only in the last row: the first pixel is far from the joint"""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 255
    m[h - 1] = 255
    return m


def u_shape(h, w):
    """two arms in the first and the last column that join only in the last row"""
    m = np.zeros((h, w), np.uint8)
    m[:, 0] = 255
    m[:, w - 1] = 255
    m[h - 1] = 255
    return m


def corner_blobs(h, w):
    """two blobs that touch only diagonally, across the corner of four tiles where the frame has one; and two more
    across the anti-diagonal of the next tile corner to the right or below, if there is one"""
    m = np.zeros((h, w), np.uint8)
    cy, cx = (TILE_H, TILE_W) if h > TILE_H and w > TILE_W else (h // 2, w // 2)
    m[max(cy - 3, 0):cy, max(cx - 3, 0):cx] = 255
    m[cy:cy + 3, cx:cx + 3] = 255
    if w > 2 * TILE_W:
        cx2 = 2 * TILE_W
        m[max(cy - 3, 0):cy, cx2:cx2 + 3] = 200
        m[cy:cy + 3, cx2 - 3:cx2] = 200
    return m


def row_ends(h, w):
    """the first and the last pixel of every other row: row ends must not wrap into the next row"""
    m = np.zeros((h, w), np.uint8)
    m[0::2, 0] = 255
    m[0::2, w - 1] = 255
    m[1::2, w // 2] = 255
    return m


def last_row(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h - 1] = 255
    return m


def first_row(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0] = 255
    return m


def other_values(h, w):
    """noise whose foreground bytes are 1, 2, 128 and 254: anything but zero is foreground"""
    rng = np.random.default_rng(7)
    v = np.array([1, 2, 128, 254], np.uint8)[rng.integers(0, 4, (h, w))]
    return np.where(rng.random((h, w)) < 0.55, v, 0).astype(np.uint8)


CONTENTS = [("background", background), ("foreground", foreground), ("checkerboard", checkerboard)]
CONTENTS += [("noise_%g" % d, (lambda d: lambda h, w: noise(h, w, d))(d)) for d in DENSITIES]
CONTENTS += [("diagonal", diagonal), ("anti_diagonal", anti_diagonal), ("serpentine", serpentine), ("spiral", spiral),
             ("comb", comb), ("u_shape", u_shape), ("corner_blobs", corner_blobs), ("row_ends", row_ends),
             ("last_row", last_row), ("first_row", first_row), ("other_values", other_values)]


def frames_of(shape):
    """[(name, (h, w) uint8 mask)] of every content at shape = (w, h)"""
    w, h = shape
    return [(name, make(h, w)) for name, make in CONTENTS]


def grid_of_rectangles(h, w, period=64):
    """disjoint rectangles, one per period x period cell, whose size depends on the cell; with the closed-form labels:
    the rectangles of a cell row start in the same image row, so raster order of first pixels is cell order"""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = yy // period, xx // period
    ncx = (w + period - 1) // period
    rw = 5 + (cx * 7 + cy * 3) % 40      # widths 5 .. 44, heights 4 .. 33: never reaching the next cell
    rh = 4 + (cx * 5 + cy * 11) % 30
    inside = (xx % period >= 3) & (xx % period < 3 + rw) & (yy % period >= 2) & (yy % period < 2 + rh)
    mask = inside.astype(np.uint8) * 255
    labels = np.where(inside, cy * ncx + cx + 1, 0).astype(np.int32)
    return mask, labels
