"""CPU reference of the warp calls (mi355_warp_affine_*): cv::warpAffine of 8-bit frames, NEAREST / LINEAR, constant and
replicated borders.

The arithmetic is the one include/mi355_imgfilter.h states, operation by operation, vectorised in numpy: float64 for
the matrix and the coordinates (numpy never fuses a multiply with an add; np.rint rounds half to even), int64 for
everything after the rounding, no shortcuts.  Frames are (h, w) or (h, w, c) uint8; every channel is warped on its own.
`rows` restricts the output to chosen output rows, so 4K frames can be checked in bounded memory.  A plain numpy helper
for the warp tests, not a fixture module.
"""
import numpy as np

NEAREST, LINEAR, AREA = 0, 1, 3
INVERSE_MAP = 16
CONSTANT, REPLICATE = 0, 1
MAX_SIZE = 32766
LIMIT = float(1 << 20)


def inverse_of(m, flags):
    """The six doubles that map an output pixel to its source position: m under INVERSE_MAP, else OpenCV's inversion."""
    m = [np.float64(v) for v in np.asarray(m, np.float64).ravel()]
    assert len(m) == 6
    if flags & INVERSE_MAP:
        return np.array(m, np.float64)
    with np.errstate(all="ignore"):                                     # a tiny determinant may overflow: not an error here
        D = m[0] * m[4] - m[1] * m[3]
        D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
        A11, A22 = m[4] * D, m[0] * D
        i0, i1, i3, i4 = A11, m[1] * (-D), m[3] * (-D), A22
        i2 = -i0 * m[2] - i1 * m[5]
        i5 = -i3 * m[2] - i4 * m[5]
    return np.array([i0, i1, i2, i3, i4, i5], np.float64)


def accepts(bpp, sw, sh, dw, dh, nframes, m, flags, border):
    """The code mi355_warp_affine_check returns for these values: 0, -1 (bad argument) or -4 (unsupported)."""
    if m is None or bpp not in (1, 4) or (flags & ~INVERSE_MAP) not in (NEAREST, LINEAR) or \
            border not in (CONSTANT, REPLICATE) or min(sw, sh, dw, dh, nframes) <= 0:
        return -1
    m = np.asarray(m, np.float64).ravel()
    if m.size != 6 or not np.all(np.isfinite(m)):
        return -1
    if max(sw, sh, dw, dh) > MAX_SIZE:
        return -4
    if float(sw) * sh * nframes > 6.0e10 or float(dw) * dh * nframes > 6.0e10:
        return -1
    with np.errstate(all="ignore"):
        i = inverse_of(m, flags)
        rx = abs(i[0]) * np.float64(dw - 1) + abs(i[1]) * np.float64(dh - 1) + abs(i[2])
        ry = abs(i[3]) * np.float64(dw - 1) + abs(i[4]) * np.float64(dh - 1) + abs(i[5])
    return 0 if rx < LIMIT and ry < LIMIT else -4


def fixed_coords(m, dw, dh, flags, rows=None):
    """(X, Y): int64 arrays (rows, dw) of X0(y) + adelta(x) and Y0(y) + bdelta(x), rd included."""
    i = inverse_of(m, flags)
    rd = 16 if (flags & ~INVERSE_MAP) == LINEAR else 512
    x = np.arange(dw, dtype=np.float64)
    y = (np.arange(dh) if rows is None else np.asarray(rows)).astype(np.float64)
    adelta = np.rint((i[0] * x) * 1024.0).astype(np.int64)
    bdelta = np.rint((i[3] * x) * 1024.0).astype(np.int64)
    X0 = np.rint((i[1] * y + i[2]) * 1024.0).astype(np.int64) + rd
    Y0 = np.rint((i[4] * y + i[5]) * 1024.0).astype(np.int64) + rd
    return X0[:, None] + adelta[None, :], Y0[:, None] + bdelta[None, :]


def border_pixel(value, img):
    """The border pixel of an (h, w[, c]) frame: the bytes of `value` in memory order."""
    b = np.array([(int(value) >> (8 * k)) & 0xFF for k in range(4)], np.uint8)
    return b[:img.shape[2]] if img.ndim == 3 else b[0]


def _tap(img, u, v, border, value):
    sh, sw = img.shape[:2]
    got = img[np.clip(v, 0, sh - 1), np.clip(u, 0, sw - 1)]
    if border == CONSTANT:
        outside = (u < 0) | (u >= sw) | (v < 0) | (v >= sh)
        got = got.copy()
        got[outside] = border_pixel(value, img)
    return got.astype(np.int64)


def warp_ref(img, m, dw, dh, flags, border, value, rows=None):
    """img (h, w) or (h, w, c) uint8 -> (dh, dw[, c]) (or len(rows) rows of it)."""
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    assert accepts(4 if img.ndim == 3 else 1, sw, sh, dw, dh, 1, m, flags, border) == 0
    X, Y = fixed_coords(m, dw, dh, flags, rows)
    if (flags & ~INVERSE_MAP) == NEAREST:
        return _tap(img, X >> 10, Y >> 10, border, value).astype(np.uint8)
    X, Y = X >> 5, Y >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    out = ((32 - fx) * (32 - fy) * _tap(img, sx, sy, border, value) +
           fx * (32 - fy) * _tap(img, sx + 1, sy, border, value) +
           (32 - fx) * fy * _tap(img, sx, sy + 1, border, value) +
           fx * fy * _tap(img, sx + 1, sy + 1, border, value) + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def taps_inside(m, sw, sh, dw, dh, flags, x0, x1, y0, y1):
    """Whether every tap of the output pixels [x0, x1) x [y0, y1) lies inside the sw x sh frame."""
    X, Y = fixed_coords(m, dw, dh, flags, rows=np.arange(y0, y1))
    sx, sy = X[:, x0:x1] >> 10, Y[:, x0:x1] >> 10
    reach = 1 if (flags & ~INVERSE_MAP) == LINEAR else 0
    return bool(sx.min() >= 0 and sx.max() + reach <= sw - 1 and sy.min() >= 0 and sy.max() + reach <= sh - 1)


def sample_rows(dh, step=97):
    """Output rows for the large frames: both ends, a run in the middle, and a stride across the rest."""
    rows = set(range(min(dh, 20))) | set(range(max(0, dh - 20), dh)) | set(range(0, dh, step))
    rows |= set(range(dh // 2, min(dh, dh // 2 + 20)))
    return np.array(sorted(rows))


def rotation(cx, cy, angle_deg, scale=1.0):
    """cv::getRotationMatrix2D in Python floats."""
    import math
    a = math.cos(angle_deg * math.pi / 180.0) * scale
    b = math.sin(angle_deg * math.pi / 180.0) * scale
    return [a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy]
