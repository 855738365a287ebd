"""CPU reference of CLAHE on single-channel frames (mi355_clahe_*).

A restatement of the "local contrast" section of include/mi355_imgfilter.h, which follows OpenCV's plain C++ path
(cv::createCLAHE(clip, Size(tiles_x, tiles_y))->apply(), 8-bit branch).  The table stage is Python ints, except for the
one float32 product per bin; the apply stage is numpy float32 array operations in the written order, one row at a time,
so nothing is fused and nothing is widened.  A plain numpy helper for the CLAHE tests, not a fixture module.  Frames are
(h, w) or (n, h, w) uint8; every frame is its own image.
"""
import numpy as np

MAX_TILES = 16
F32 = np.float32


def geometry(w, h, tiles_x, tiles_y):
    """(ew, eh, tw, th): the extended frame and the tile size.  OpenCV's quirk: when either dimension does not divide,
    both are padded, the dividing one by a whole tiles_x / tiles_y."""
    if w % tiles_x == 0 and h % tiles_y == 0:
        ew, eh = w, h
    else:
        ew = w + (tiles_x - w % tiles_x)
        eh = h + (tiles_y - h % tiles_y)
    return ew, eh, ew // tiles_x, eh // tiles_y


def supported(w, h, tiles_x, tiles_y):
    """One reflection serves the pad (anything else is MI355_ERR_UNSUPPORTED)."""
    ew, eh, _, _ = geometry(w, h, tiles_x, tiles_y)
    return ew - w <= w - 1 and eh - h <= h - 1


def extend(y, tiles_x, tiles_y):
    """cv::copyMakeBorder(BORDER_REFLECT_101) on the right and bottom: ext[y][x] = src[r(y, h)][r(x, w)]."""
    h, w = y.shape
    ew, eh, _, _ = geometry(w, h, tiles_x, tiles_y)
    xs = np.arange(ew)
    ys = np.arange(eh)
    xs = np.where(xs < w, xs, 2 * w - 2 - xs)
    ys = np.where(ys < h, ys, 2 * h - 2 - ys)
    return y[np.ix_(ys, xs)]


def clip_of(clip_limit, tot):
    """cl: 0 = no clipping."""
    if clip_limit > 0:
        return max(int(float(clip_limit) * tot / 256.0), 1)
    return 0


def tile_lut(hist, cl, tot, trace=None):
    """One tile's 256-byte table from its 256 counts.  `trace` (a dict) receives batch, residual, step and whether a
    table product fell exactly on .5."""
    hist = [int(v) for v in hist]
    batch = residual = step = 0
    if cl > 0:
        clipped = 0
        for b in range(256):
            if hist[b] > cl:
                clipped += hist[b] - cl
                hist[b] = cl
        batch = clipped // 256
        residual = clipped - batch * 256
        for b in range(256):
            hist[b] += batch
        if residual:
            step = max(256 // residual, 1)
            b, left = 0, residual
            while b < 256 and left > 0:  # OpenCV's loop; the header's closed form says the same
                hist[b] += 1
                b += step
                left -= 1
    lut_scale = F32(255.0) / F32(tot)
    lut = np.zeros(256, np.uint8)
    s = 0
    half = False
    for b in range(256):
        s += hist[b]
        p = F32(s) * lut_scale
        half = half or float(p) % 1.0 == 0.5
        lut[b] = min(255, max(0, int(np.rint(p))))
    if trace is not None:
        trace.update(batch=batch, residual=residual, step=step, half=half, clipped=cl > 0)
    return lut


def luts_ref(y, clip_limit, tiles_x, tiles_y, traces=None):
    """(tiles_y, tiles_x, 256) uint8 tables of one (h, w) frame, (n, tiles_y, tiles_x, 256) of (n, h, w) frames."""
    y = np.asarray(y, np.uint8)
    if y.ndim == 3:
        return np.stack([luts_ref(f, clip_limit, tiles_x, tiles_y, traces) for f in y])
    h, w = y.shape
    _, _, tw, th = geometry(w, h, tiles_x, tiles_y)
    ext = extend(y, tiles_x, tiles_y)
    tot = tw * th
    cl = clip_of(clip_limit, tot)
    out = np.empty((tiles_y, tiles_x, 256), np.uint8)
    for j in range(tiles_y):
        for i in range(tiles_x):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256)
            tr = {} if traces is not None else None
            out[j, i] = tile_lut(hist, cl, tot, tr)
            if traces is not None:
                traces.append(tr)
    return out


def cells(n, inv, tiles):
    """For positions 0 .. n - 1: (c1, c2, a, a1) of the apply stage, float32 in the written order."""
    p = np.arange(n, dtype=np.int64).astype(F32)
    tf = p * F32(inv) - F32(0.5)
    t1f = np.floor(tf)
    a = tf - t1f
    a1 = F32(1.0) - a
    t1 = t1f.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def apply_ref(y, luts, tiles_x, tiles_y, res_out=None):
    """The interpolation stage on one (h, w) frame with its (tiles_y, tiles_x, 256) tables.  `res_out` (a list)
    receives each row's float32 `res` before rounding."""
    h, w = y.shape
    _, _, tw, th = geometry(w, h, tiles_x, tiles_y)
    inv_tw = F32(1.0) / F32(tw)
    inv_th = F32(1.0) / F32(th)
    c1, c2, xa, xa1 = cells(w, inv_tw, tiles_x)
    r1, r2, ya, ya1 = cells(h, inv_th, tiles_y)
    lf = luts.astype(F32)
    out = np.empty((h, w), np.uint8)
    for yy in range(h):
        v = y[yy]
        top = lf[r1[yy], c1, v] * xa1 + lf[r1[yy], c2, v] * xa
        bot = lf[r2[yy], c1, v] * xa1 + lf[r2[yy], c2, v] * xa
        res = top * ya1[yy] + bot * ya[yy]
        assert res.dtype == F32
        if res_out is not None:
            res_out.append(res)
        out[yy] = np.clip(np.rint(res), 0, 255).astype(np.uint8)
    return out


def clahe_ref(y, clip_limit, tiles_x, tiles_y, res_out=None):
    """cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply() of (h, w) or (n, h, w) frames."""
    y = np.asarray(y, np.uint8)
    if y.ndim == 3:
        return np.stack([clahe_ref(f, clip_limit, tiles_x, tiles_y, res_out) for f in y])
    return apply_ref(y, luts_ref(y, clip_limit, tiles_x, tiles_y), tiles_x, tiles_y, res_out)
