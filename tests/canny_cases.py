"""The shapes and contents of the hysteresis and Canny tests (test_canny_cpu.py, test_gpu_canny.py).

Shapes: those of the labelling tests (the union runs on 64 x 32 tiles), the non-maximum-suppression tile (NMS_TW x NMS_TH
of csrc/canny.hip), that size plus one each way, two tiles plus one, and 2 x 2, where every neighbour of every pixel is
the frame's edge.
"""
import numpy as np

import ccl_cases as cc

NMS_TW, NMS_TH = 256, 16

#         (w, h)
SHAPES = list(cc.SHAPES) + [(NMS_TW, 2 * NMS_TH), (NMS_TW + 1, 2 * NMS_TH + 1), (2 * NMS_TW, 3 * NMS_TH),
                            (2 * NMS_TW + 1, 3 * NMS_TH + 1), (2, 2)]
LITERAL_SHAPES = [s for s in SHAPES if s[0] * s[1] <= 67 * 48]  # of the per-pixel Python transcription

# (threshold1, threshold2, flags)
THRESHOLDS = [(50, 150, 0), (150, 50, 0), (30, 90, 0), (0, 0, 0), (37.5, 112.5, 1), (60.5, 200.9, 1)]


# ---- contents for Canny ---------------------------------------------------------------------------------------------
def noise(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def smooth(h, w, seed=1):
    """a 5x5 box mean (edge-replicated, truncated) of uniform noise: edges of every direction, weak and strong"""
    p = np.pad(noise(h, w, seed).astype(np.int32), 2, mode="edge")
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5))
    return (s // 25).astype(np.uint8)


def steps2(h, w):
    """a staircase of two-pixel treads: every step is a two-column plateau of the magnitude"""
    x = np.arange(w)
    return np.broadcast_to(((x // 2 * 37) % 256).astype(np.uint8), (h, w)).copy()


def disc(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    r = max(min(h, w) // 3, 1)
    return (((xx - w // 2) ** 2 + (yy - h // 2) ** 2 <= r * r) * 220).astype(np.uint8)


def diagonal_step(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * h > yy * w) * 200).astype(np.uint8)


def fading_diagonal_step(h, w):
    """a diagonal step whose height falls from 200 to 0 along it: strong at one end, candidates only, then nothing"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * h > yy * w) * (200 * (h - 1 - yy) // max(h - 1, 1))).astype(np.uint8)


def checkerboard(h, w):
    return cc.checkerboard(h, w)


def flat(h, w):
    return np.full((h, w), 77, np.uint8)


CONTENTS = [("noise", noise), ("smooth", smooth), ("steps2", steps2), ("disc", disc), ("diagonal_step", diagonal_step),
            ("fading_diagonal_step", fading_diagonal_step), ("checkerboard", checkerboard), ("flat", flat)]


def frames_of(shape):
    """[(name, (h, w) uint8 frame)] of every Canny content at shape = (w, h)"""
    w, h = shape
    return [(name, make(h, w)) for name, make in CONTENTS]


# ---- contents for the hysteresis --------------------------------------------------------------------------------------
FG, BG, STRONG = 100, 40, 200      # response bytes
LOW, HIGH = 60, 150
VARIANTS = ("last", "first", "random")
# (low, high) beside (LOW, HIGH): low = high, nothing is strong, everything but zero is a candidate
BOUNDARIES = [(100, 100), (60, 255), (0, 150), (0, 0), (255, 255)]


def response(mask, variant):
    """The response map of a mask of the labelling cases: FG on the foreground, BG elsewhere, and STRONG on the last
    foreground pixel in raster order (the mark has to travel the whole of comb, spiral and u_shape to the root at the
    other end), on the first one, or on one foreground pixel in 400 at random"""
    resp = np.where(mask != 0, FG, BG).astype(np.uint8)
    on = np.flatnonzero(mask.ravel() != 0)
    if on.size:
        if variant == "last":
            pick = on[-1:]
        elif variant == "first":
            pick = on[:1]
        else:
            pick = on[np.random.default_rng(on.size).random(on.size) < 1.0 / 400.0]
        resp.ravel()[pick] = STRONG
    return resp


def responses_of(shape):
    """[(name, (h, w) uint8 response)] of every labelling content x variant at shape = (w, h)"""
    return [("%s/%s" % (name, v), response(m, v)) for name, m in cc.frames_of(shape) for v in VARIANTS]
