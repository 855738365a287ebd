"""CPU reference of the remap and perspective calls (mi355_remap_*, mi355_warp_perspective_*): cv::remap through one
per-pixel map and cv::warpPerspective of 8-bit frames, NEAREST / LINEAR, constant and replicated borders.

The arithmetic is the one include/mi355_imgfilter.h states, operation by operation, vectorised in numpy: float32 for
the FLOAT map rule, float64 for the homography (numpy never fuses a multiply with an add; np.rint rounds half to even;
the division is IEEE), int64 for everything after the rounding, the clamp to short included.  Sampling is warp_ref's.
Frames are (h, w) or (h, w, c) uint8.  `rows` restricts the output to chosen output rows, so 4K frames can be checked
in bounded memory.  A plain numpy helper for the remap tests, not a fixture module.
"""
import numpy as np

from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, MAX_SIZE, NEAREST, REPLICATE, _tap

FIXED, FLOAT = 0, 1
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def clamp16(v):
    return np.clip(v, -32768, 32767)


def _shapes_code(bpp, sw, sh, dw, dh, nframes, border):
    if bpp not in (1, 4) or border not in (CONSTANT, REPLICATE) or min(sw, sh, dw, dh, nframes) <= 0:
        return -1
    if max(sw, sh, dw, dh) > MAX_SIZE:
        return -4
    if float(sw) * sh * nframes > 6.0e10 or float(dw) * dh * nframes > 6.0e10:
        return -1
    return 0


def remap_accepts(bpp, sw, sh, dw, dh, nframes, map_kind, interp, border):
    """The code mi355_remap_check returns for these values: 0, -1 (bad argument) or -4 (unsupported)."""
    if map_kind not in (FIXED, FLOAT) or interp not in (NEAREST, LINEAR):
        return -1
    return _shapes_code(bpp, sw, sh, dw, dh, nframes, border)


def perspective_accepts(bpp, sw, sh, dw, dh, nframes, m, flags, border):
    """The code mi355_warp_perspective_check returns for these values."""
    if m is None or (flags & ~INVERSE_MAP) not in (NEAREST, LINEAR):
        return -1
    if bpp not in (1, 4) or border not in (CONSTANT, REPLICATE) or min(sw, sh, dw, dh, nframes) <= 0:
        return -1
    m = np.asarray(m, np.float64).ravel()
    if m.size != 9 or not np.all(np.isfinite(m)):
        return -1
    return _shapes_code(bpp, sw, sh, dw, dh, nframes, border)


def perspective_inverse(m, flags):
    """The nine doubles that map an output pixel to its source position: m under INVERSE_MAP, else the adjugate times
    1 / det, operation by operation."""
    m = [np.float64(v) for v in np.asarray(m, np.float64).ravel()]
    assert len(m) == 9
    if flags & INVERSE_MAP:
        return np.array(m, np.float64)
    with np.errstate(all="ignore"):
        det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
        d = np.float64(1.0) / det if det != 0 else np.float64(0.0)
        inv = [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
               (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
               (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]
    return np.array(inv, np.float64)


def _split(X, Y, interp):
    """(sx, sy, fx, fy) int64 from the rounded coordinates, the clamp to short included."""
    if interp == LINEAR:
        return clamp16(X >> 5), clamp16(Y >> 5), X & 31, Y & 31
    return clamp16(X), clamp16(Y), np.zeros_like(X), np.zeros_like(Y)


def _round_float(t):
    """(int)rint of float32 values: NaN and t <= -2^31 give INT_MIN, t >= 2^31 gives INT_MAX."""
    assert t.dtype == np.float32
    low = np.isnan(t) | (t <= np.float32(-2147483648.0))
    high = ~low & (t >= np.float32(2147483648.0))
    mid = np.where(low | high, np.float32(0), t)
    return np.where(low, INT_MIN, np.where(high, INT_MAX, np.rint(mid).astype(np.int64)))


def float_coords(map_x, map_y, interp, rows=None):
    """(sx, sy, fx, fy) of FLOAT maps (dh, dw) float32."""
    map_x, map_y = np.asarray(map_x), np.asarray(map_y)
    assert map_x.dtype == np.float32 and map_y.dtype == np.float32 and map_x.shape == map_y.shape
    if rows is not None:
        map_x, map_y = map_x[rows], map_y[rows]
    S = np.float32(32.0 if interp == LINEAR else 1.0)
    with np.errstate(all="ignore"):
        tx, ty = map_x * S, map_y * S
    assert tx.dtype == np.float32
    return _split(_round_float(tx), _round_float(ty), interp)


def fixed_coords_of_maps(map1, map2, interp, rows=None):
    """(sx, sy, fx, fy) of FIXED maps: map1 (dh, dw, 2) int16, map2 (dh, dw) uint16 (None with NEAREST)."""
    map1 = np.asarray(map1)
    assert map1.dtype == np.int16 and map1.shape[-1] == 2
    if rows is not None:
        map1 = map1[rows]
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    if interp == NEAREST:
        return sx, sy, np.zeros_like(sx), np.zeros_like(sx)
    map2 = np.asarray(map2)
    assert map2.dtype == np.uint16
    if rows is not None:
        map2 = map2[rows]
    a = map2.astype(np.int64) & 1023
    return sx, sy, a & 31, a >> 5


def convert_maps(map_x, map_y, interp=LINEAR):
    """cv::convertMaps: FLOAT maps -> (map1 int16 (dh, dw, 2), map2 uint16 (dh, dw)) through the FLOAT rule."""
    sx, sy, fx, fy = float_coords(map_x, map_y, interp)
    return np.stack([sx, sy], -1).astype(np.int16), (fy * 32 + fx).astype(np.uint16)


def perspective_coords(m, dw, dh, flags, rows=None):
    """(sx, sy, fx, fy) of a homography, int64 arrays (rows, dw)."""
    h = perspective_inverse(m, flags)
    interp = flags & ~INVERSE_MAP
    S = np.float64(32.0 if interp == LINEAR else 1.0)
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = (np.arange(dh) if rows is None else np.asarray(rows)).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        w = (h[6] * x) + (h[7] * y + h[8])
        s = np.where(w != 0, S / np.where(w != 0, w, 1.0), 0.0)
        tX = ((h[0] * x) + (h[1] * y + h[2])) * s
        tY = ((h[3] * x) + (h[4] * y + h[5])) * s

        def to_int(t):
            f = np.where(~(t < 2147483647.0), 2147483647.0, t)
            f = np.where(f < -2147483648.0, -2147483648.0, f)
            return np.rint(f).astype(np.int64)
        X, Y = to_int(tX), to_int(tY)
    return _split(X, Y, interp)


def perspective_w(m, dw, dh, flags):
    """The denominators w of a homography, (dh, dw) float64 (for the tests that place w == 0 and a sign change)."""
    h = perspective_inverse(m, flags)
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    return (h[6] * x) + (h[7] * y + h[8])


def sample(img, coords, interp, border, value):
    """The output pixels of one frame from (sx, sy, fx, fy): warp_ref's tap(), NEAREST and LINEAR sum."""
    img = np.asarray(img, np.uint8)
    sx, sy, fx, fy = coords
    if interp == NEAREST:
        return _tap(img, sx, sy, border, value).astype(np.uint8)
    if img.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    out = ((32 - fx) * (32 - fy) * _tap(img, sx, sy, border, value) +
           fx * (32 - fy) * _tap(img, sx + 1, sy, border, value) +
           (32 - fx) * fy * _tap(img, sx, sy + 1, border, value) +
           fx * fy * _tap(img, sx + 1, sy + 1, border, value) + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def map_coords(map1, map2, map_kind, interp, rows=None):
    if map_kind == FIXED:
        return fixed_coords_of_maps(map1, map2, interp, rows)
    return float_coords(map1, map2, interp, rows)


def remap_ref(img, map1, map2, map_kind, interp, border, value, rows=None):
    """img (h, w) or (h, w, c) uint8 -> (dh, dw[, c]) (or len(rows) rows of it)."""
    img = np.asarray(img, np.uint8)
    dh, dw = np.asarray(map1).shape[:2]
    assert remap_accepts(4 if img.ndim == 3 else 1, img.shape[1], img.shape[0], dw, dh, 1, map_kind, interp, border) == 0
    return sample(img, map_coords(map1, map2, map_kind, interp, rows), interp, border, value)


def perspective_ref(img, m, dw, dh, flags, border, value, rows=None):
    img = np.asarray(img, np.uint8)
    assert perspective_accepts(4 if img.ndim == 3 else 1, img.shape[1], img.shape[0], dw, dh, 1, m, flags, border) == 0
    return sample(img, perspective_coords(m, dw, dh, flags, rows), flags & ~INVERSE_MAP, border, value)


def interior_passes(coords, sw, sh, interp, tile, lane_rows):
    """(row passes whose taps all lie inside the sw x sh frame, row passes): a pass is `lane_rows` output rows of one
    tile (tw, th), the unit for which the kernel votes whether it needs border tests."""
    sx, sy = coords[0], coords[1]
    reach = 1 if interp == LINEAR else 0
    inside = (sx >= 0) & (sx + reach <= sw - 1) & (sy >= 0) & (sy + reach <= sh - 1)
    dh, dw = inside.shape
    tw, th = tile
    n = k = 0
    for ty0 in range(0, dh, th):
        for yb in range(ty0, min(ty0 + th, dh), lane_rows):
            y1 = min(yb + lane_rows, ty0 + th, dh)
            for x0 in range(0, dw, tw):
                n += 1
                k += bool(inside[yb:y1, x0:x0 + tw].all())
    return k, n
