"""CPU reference of the hysteresis and Canny calls (mi355_hysteresis_*, mi355_canny_*): the numpy restatement of
include/mi355_imgfilter.h, "from gradients to edges".

Everything is integer arithmetic with one right answer per input.  The non-maximum suppression exists twice: vectorised
(classes) and as a literal per-pixel transcription of the header (classes_literal); test_canny_cpu.py holds them against
each other.  The hysteresis is a stack flood fill from the strong pixels, as OpenCV does it: a different algorithm from
the device's union-find.  kept_by_labels is the same answer from the labelling reference (tests/ccl_ref.py) plus
"component holds a strong pixel": much faster on large frames, and the third algorithm the other two are held against.
"""
import math

import numpy as np

from ccl_ref import label

L2GRADIENT = 1


def thresholds(threshold1, threshold2, flags=0):
    """(low, high): the integer thresholds on the magnitude"""
    lo, hi = min(float(threshold1), float(threshold2)), max(float(threshold1), float(threshold2))
    if flags & L2GRADIENT:
        lo, hi = min(lo, 32767.0), min(hi, 32767.0)
        if lo > 0:
            lo *= lo
        if hi > 0:
            hi *= hi
    return int(math.floor(lo)), int(math.floor(hi))


def gradient(img):
    """(dx, dy) int32 of one (h, w) uint8 frame: the 3x3 Sobel pair, coordinates clamped to the frame"""
    p = np.pad(np.ascontiguousarray(img, np.uint8).astype(np.int32), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def magnitude(dx, dy, flags=0):
    return dx * dx + dy * dy if flags & L2GRADIENT else np.abs(dx) + np.abs(dy)


def directions(dx, dy):
    """0: along the row, 1: along the column, 2: the diagonal with s = 1, 3: the diagonal with s = -1"""
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    tg22x = x * 13573
    tg67x = tg22x + (x << 16)
    return np.where(y < tg22x, 0, np.where(y > tg67x, 1, np.where((dx ^ dy) < 0, 3, 2)))


def classes(img, low, high, flags=0):
    """(h, w) uint8: 0 none, 1 candidate, 2 strong"""
    dx, dy = gradient(img)
    m = magnitude(dx, dy, flags)
    d = directions(dx, dy)
    z = np.pad(m, 1)  # the magnitude of a position outside the frame is 0
    c = z[1:-1, 1:-1]
    left, right, up, down = z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
    ul, ur, dl, dr = z[:-2, :-2], z[:-2, 2:], z[2:, :-2], z[2:, 2:]
    is_max = np.where(d == 0, (c > left) & (c >= right),
                      np.where(d == 1, (c > up) & (c >= down),
                               np.where(d == 2, (c > ul) & (c > dr), (c > ur) & (c > dl))))
    cand = (m > low) & is_max
    return (cand.astype(np.uint8) + (cand & (m > high)).astype(np.uint8))


def classes_literal(img, low, high, flags=0):
    """The header, pixel by pixel, in Python integers."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    px = img.tolist()

    def p(y, x):
        return px[min(max(y, 0), h - 1)][min(max(x, 0), w - 1)]

    def grad(y, x):
        dx = (p(y - 1, x + 1) + 2 * p(y, x + 1) + p(y + 1, x + 1)) - (p(y - 1, x - 1) + 2 * p(y, x - 1) + p(y + 1, x - 1))
        dy = (p(y + 1, x - 1) + 2 * p(y + 1, x) + p(y + 1, x + 1)) - (p(y - 1, x - 1) + 2 * p(y - 1, x) + p(y - 1, x + 1))
        return dx, dy

    def mag(y, x):
        if not (0 <= y < h and 0 <= x < w):
            return 0
        dx, dy = grad(y, x)
        return dx * dx + dy * dy if flags & L2GRADIENT else abs(dx) + abs(dy)

    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            m = mag(y, x)
            if not m > low:
                continue
            dx, dy = grad(y, x)
            ax, ay = abs(dx), abs(dy) << 15
            tg22x = ax * 13573
            tg67x = tg22x + (ax << 16)
            if ay < tg22x:
                ok = m > mag(y, x - 1) and m >= mag(y, x + 1)
            elif ay > tg67x:
                ok = m > mag(y - 1, x) and m >= mag(y + 1, x)
            else:
                s = -1 if (dx ^ dy) < 0 else 1
                ok = m > mag(y - 1, x - s) and m > mag(y + 1, x + s)
            if ok:
                out[y, x] = 2 if m > high else 1
    return out


def kept_by_flood(cand, strong, connectivity=8):
    """(h, w) bool: the candidates a stack flood fill from the strong candidates reaches"""
    assert connectivity in (4, 8)
    cand = np.ascontiguousarray(cand, bool)
    h, w = cand.shape
    ww = w + 2
    pad = np.zeros((h + 2, ww), np.uint8)  # 1: a candidate not reached yet, 2: reached; the rim stays 0
    pad[1:-1, 1:-1] = cand
    seeds = np.zeros((h + 2, ww), bool)
    seeds[1:-1, 1:-1] = np.ascontiguousarray(strong, bool) & cand
    state = pad.ravel().tolist()
    offs = (-ww - 1, -ww, -ww + 1, -1, 1, ww - 1, ww, ww + 1) if connectivity == 8 else (-ww, -1, 1, ww)
    stack = []
    for s in np.flatnonzero(seeds.ravel()).tolist():
        if state[s] == 1:
            state[s] = 2
            stack.append(s)
    while stack:
        q = stack.pop()
        for o in offs:
            n = q + o
            if state[n] == 1:
                state[n] = 2
                stack.append(n)
    return np.array(state, np.uint8).reshape(h + 2, ww)[1:-1, 1:-1] == 2


def kept_by_labels(cand, strong, connectivity=8):
    """The same from the labelling reference: a candidate is kept iff its component holds a strong candidate."""
    cand = np.ascontiguousarray(cand, bool)
    labels, n = label(cand.astype(np.uint8), connectivity)
    holds = np.zeros(n, bool)
    holds[labels[np.ascontiguousarray(strong, bool) & cand]] = True
    holds[0] = False
    return holds[labels]


def hysteresis_ref(resp, low, high, connectivity=8, kept=kept_by_flood):
    """(h, w) or (n, h, w) uint8 response maps -> 255 / 0, every frame on its own"""
    resp = np.ascontiguousarray(resp, np.uint8)
    if resp.ndim == 3:
        return np.stack([hysteresis_ref(f, low, high, connectivity, kept) for f in resp])
    return kept(resp > low, resp > high, connectivity).astype(np.uint8) * 255


def canny_ref(img, threshold1, threshold2, flags=0, kept=kept_by_flood):
    """(h, w) or (n, h, w) uint8 frames -> the edge map, 255 / 0"""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 3:
        return np.stack([canny_ref(f, threshold1, threshold2, flags, kept) for f in img])
    low, high = thresholds(threshold1, threshold2, flags)
    cls = classes(img, low, high, flags)
    return kept(cls > 0, cls > 1, 8).astype(np.uint8) * 255
