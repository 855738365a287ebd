"""CPU reference of the resize calls (mi355_resize_*): cv::resize of 8-bit frames, NEAREST / LINEAR / AREA.

The arithmetic is the one include/mi355_imgfilter.h states, operation by operation, vectorised in numpy: fp64 where the
header says fp64, np.float32 where it says fp32 (numpy never fuses a multiply with an add; np.rint rounds half to
even), int64 for the integer part (every value fits an int32).  Frames are (h, w) or (h, w, c) uint8; every channel is
resized on its own.  `rows` restricts the output to chosen output rows, so 4K frames can be checked in bounded memory.
A plain numpy helper for the resize tests, not a fixture module.
"""
import numpy as np

NEAREST, LINEAR, AREA = 0, 1, 3
MAX_AREA_FACTOR = 16
F32 = np.float32


def scale_of(src, dst):
    """1.0 / ((double)dst / (double)src) — not src / dst: the two differ in the last bit for many size pairs."""
    return 1.0 / (float(dst) / float(src))


def area_factors(sw, sh, dw, dh):
    """(n, m) when AREA is offered for the size pair, else None."""
    if dw <= 0 or dh <= 0 or sw % dw or sh % dh:
        return None
    n, m = sw // dw, sh // dh
    return (n, m) if 1 <= n <= MAX_AREA_FACTOR and 1 <= m <= MAX_AREA_FACTOR else None


def accepts(interp, sw, sh, dw, dh):
    return interp in (NEAREST, LINEAR) or (interp == AREA and area_factors(sw, sh, dw, dh) is not None)


def linear_cols(sw, dw):
    """(sx, sx1, a0, a1) of every output column."""
    dx = np.arange(dw, dtype=np.float64)
    fx = ((dx + 0.5) * scale_of(sw, dw) - 0.5).astype(F32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(F32)
    lo, hi = sx < 0, sx >= sw - 1
    sx = np.where(lo, 0, np.where(hi, sw - 1, sx))
    fx = np.where(lo | hi, F32(0), fx).astype(F32)
    a0 = np.rint((F32(1) - fx) * F32(2048)).astype(np.int64)
    a1 = np.rint(fx * F32(2048)).astype(np.int64)
    return sx, np.minimum(sx + 1, sw - 1), a0, a1


def linear_rows(sh, dh, rows=None):
    """(r0, r1, b0, b1) of the output rows; fy is not clamped."""
    dy = (np.arange(dh) if rows is None else np.asarray(rows)).astype(np.float64)
    fy = ((dy + 0.5) * scale_of(sh, dh) - 0.5).astype(F32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(F32)).astype(F32)
    b0 = np.rint((F32(1) - fy) * F32(2048)).astype(np.int64)
    b1 = np.rint(fy * F32(2048)).astype(np.int64)
    return np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1), b0, b1


def _bc(v, img):
    """a per-row or per-column vector shaped to broadcast over (rows, cols[, c])"""
    return v.reshape(v.shape + (1,) * (img.ndim - 2))


def _nearest(img, dw, dh, rows):
    sh, sw = img.shape[:2]
    dx = np.arange(dw, dtype=np.float64)
    dy = (np.arange(dh) if rows is None else np.asarray(rows)).astype(np.float64)
    sx = np.minimum(np.floor(dx * scale_of(sw, dw)).astype(np.int64), sw - 1)
    sy = np.minimum(np.floor(dy * scale_of(sh, dh)).astype(np.int64), sh - 1)
    return img[sy][:, sx]


def _linear(img, dw, dh, rows):
    sh, sw = img.shape[:2]
    sx, sx1, a0, a1 = linear_cols(sw, dw)
    r0, r1, b0, b1 = linear_rows(sh, dh, rows)
    a0, a1 = _bc(a0, img)[None], _bc(a1, img)[None]

    def hrow(r):
        band = img[r].astype(np.int64)                                  # (n, sw[, c])
        return (band[:, sx] * a0 + band[:, sx1] * a1) >> 4

    b0, b1 = _bc(b0[:, None], img), _bc(b1[:, None], img)
    out = (((b0 * hrow(r0)) >> 16) + ((b1 * hrow(r1)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def area_byte(total, n, m):
    """One output byte per block sum (any integer array)."""
    total = np.asarray(total, np.int64)
    if n == 2 and m == 2:
        return ((total + 2) >> 2).astype(np.uint8)
    scale = F32(1) / F32(n * m)
    return np.clip(np.rint(total.astype(F32) * scale), 0, 255).astype(np.uint8)


def _area(img, dw, dh, rows):
    sh, sw = img.shape[:2]
    n, m = area_factors(sw, sh, dw, dh)
    dy = np.arange(dh) if rows is None else np.asarray(rows, np.int64)
    src_rows = (dy[:, None] * m + np.arange(m)[None, :]).ravel()
    band = img[src_rows].astype(np.int64).reshape((len(dy), m, dw, n) + img.shape[2:])
    return area_byte(band.sum(axis=(1, 3)), n, m)


def resize_ref(img, dw, dh, interp, rows=None):
    """img (h, w) or (h, w, c) uint8 -> (dh, dw[, c]) (or len(rows) rows of it)."""
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    assert accepts(interp, sw, sh, dw, dh), (interp, sw, sh, dw, dh)
    if interp == LINEAR and sw == 2 * dw and sh == 2 * dh:
        interp = AREA                                                   # OpenCV switches there
    return {NEAREST: _nearest, LINEAR: _linear, AREA: _area}[interp](img, dw, dh, rows)


def sample_rows(dh, step=97):
    """Output rows for the large frames: both ends, a run in the middle, and a stride across the rest."""
    rows = set(range(min(dh, 20))) | set(range(max(0, dh - 20), dh)) | set(range(0, dh, step))
    rows |= set(range(dh // 2, min(dh, dh // 2 + 20)))
    return np.array(sorted(rows))
