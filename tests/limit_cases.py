"""Cases of the limit tests (test_limits_cpu.py, test_gpu_limits.py): the geometric calls at the bounds their argument
checks accept, and batches of thousands of tiny frames through them.

The GPU tests of resize, warp_affine, remap and perspective are dense at small shapes and stay far from what the
*_check functions let through: sizes of MI355_MAX_WARP_SIZE, resize rows of 10^5 pixels, affine coordinates next to
2^30, perspective coordinates that saturate, and frame counts in the thousands.  Every case here is a thin or tiny
frame with one reason of its own (the *_WHY strings); test_limits_cpu.py shows on the reference's coordinates that each
reaches what it is there for, test_gpu_limits.py compares every pixel with the numpy references.  A plain numpy helper,
not a fixture module.
"""
import collections

import numpy as np

import remap_cases as rc
from remap_ref import FIXED, INT_MAX, INT_MIN, perspective_inverse
from warp_ref import INVERSE_MAP, LIMIT, LINEAR, MAX_SIZE, NEAREST, accepts, rotation

M = MAX_SIZE                                     # 32766, MI355_MAX_WARP_SIZE
VALUES = (0, 0x80FF407F)
VALUE = 0x80FF407F

# ---- 1. maximum-size thin frames --------------------------------------------------------------------------------------
# (src w, src h, dst w, dst h) -> (axis the size lies along, reason)
THIN_WHY = collections.OrderedDict([
    ((M, 3, M, 2), ("x", "source and output of the largest width: column indices up to 32765 on both sides, 512 tiles")),
    ((3, M, 2, M), ("y", "source and output of the largest height: row indices up to 32765, sy * sw next to 2^17")),
    ((M, 3, 3, 2), ("x", "a one-tile output that reads the far end of the widest source")),
    ((3, 2, M, 3), ("x", "the widest output of a tiny source: source positions up to 32765 that all lie outside")),
])
THIN = tuple(THIN_WHY)
# warp_affine also runs the two one-tile shapes transposed, so that sy meets what sx meets
WARP_THIN_WHY = collections.OrderedDict(THIN_WHY)
WARP_THIN_WHY.update([
    ((3, M, 2, 3), ("y", "(M, 3, 3, 2) transposed: a one-tile output that reads the far end of the tallest source")),
    ((2, 3, 3, M), ("y", "(3, 2, M, 3) transposed: the tallest output of a tiny source")),
])
WARP_THIN = tuple(WARP_THIN_WHY)


def _axis(m6, axis):
    """A 2 x 3 matrix written for x, or the same map with the roles of x and y exchanged."""
    a, b, c, d, e, f = m6
    return [a, b, c, d, e, f] if axis == "x" else [e, d, f, b, a, c]


def warp_thin_matrices(shape):
    """[(name, matrix, why)] of a shape; every matrix runs inverse-mapped and forward (test_limits_cpu.py shows that
    every inverse stays accepted)."""
    sw, sh, dw, dh = shape
    axis = WARP_THIN_WHY[shape][0]
    last = (sw if axis == "x" else sh) - 1       # the last source index along the axis
    out = [("identity", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], "every source index of the axis as it is"),
           ("half", _axis([1.0, 0.0, 0.5, 0.0, 1.0, 0.0], axis),
            "LINEAR: fraction 16 at every index; with the largest source and output the last one's far tap is the seam "
            "index + 1 == M"),
           ("flip", _axis([-1.0, 0.0, float(last), 0.0, 1.0, 0.0], axis),
            "a negative step from the last index: adelta down to -32765 * 1024")]
    if (dw if axis == "x" else dh) == 3 and last == M - 1:
        out.append(("stride16000", _axis([16000.0, 0.0, 0.0, 0.0, 1.0, 0.0], axis),
                    "three in-frame taps 16000 apart: one interior tile that spans the source"))
    if shape in ((M, 3, M, 2), (3, M, 2, M)):
        out.append(("turn0.5", rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 0.5),
                    "half a degree about the centre: the wide tile, interior tiles in the middle and general tiles on "
                    "both sides in one launch"))
    return out


def remap_thin_maps(shape, kind, interp):
    """[(name, map1, map2, why)] of a shape for one map kind."""
    sw, sh, dw, dh = shape
    axis = THIN_WHY[shape][0]
    last = (sw if axis == "x" else sh) - 1
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    half = _axis([1.0, 0.0, 0.5, 0.0, 1.0, 0.0], axis)
    flip = _axis([-1.0, 0.0, float(last), 0.0, 1.0, 0.0], axis)
    flags = interp | INVERSE_MAP
    if kind == FIXED:
        make = lambda m: rc.affine_fixed_maps(m, dw, dh, flags)                     # noqa: E731
        edge = fixed_edge_maps(shape, interp)
    else:
        make = lambda m: rc.affine_float_maps(m, dw, dh, INVERSE_MAP)               # noqa: E731
        edge = float_edge_maps(shape)
    return [("identity",) + make(ident) +
            ("entries up to the last index of the axis: valid pixels where the source is as large",),
            ("half",) + make(half) +
            ("fraction 16 everywhere; index M - 1 with its far tap at M where both sides are largest",),
            ("flip",) + make(flip) + ("the far end first: valid entries from the last index down",),
            ("edge",) + edge + ("entries past the frame planted among valid ones: where the kernel keeps the index and "
                                "the reference clamps it to a short, both must still call it outside",)]


# what the FLOAT edge map holds along its axis from entry 0 on: around the last column, around the short range's ends
FLOAT_EDGE = (M - 1.5, M - 1.0, M - 0.5, float(M), M + 0.5, 32767.0, 32768.0, 40000.0, -32768.5, -40000.0)
# (index along the axis, fraction) the FIXED edge map holds from entry 0 on
FIXED_EDGE = ((M - 1, 16), (32767, 0), (M - 1, 31), (-32768, 0), (M - 2, 16), (32767, 9), (-32768, 31), (M - 1, 0))


def _edge_slots(shape, n):
    """Where the planted entries go: along the long axis of the map from its start, in the first row (column); a map
    that is short along its axis (a one-tile output) takes them row by row."""
    sw, sh, dw, dh = shape
    axis = THIN_WHY[shape][0]
    if axis == "x":
        return [divmod(k, dw) for k in range(min(n, dw * dh))]
    return [(k % dh, k // dh) for k in range(min(n, dw * dh))]


def float_edge_maps(shape):
    """Identity FLOAT maps with FLOAT_EDGE planted along the axis (as x on the wide shapes, as y on the tall one)."""
    sw, sh, dw, dh = shape
    axis = THIN_WHY[shape][0]
    mx, my = rc.identity_float_maps(dw, dh)
    for (y, x), v in zip(_edge_slots(shape, len(FLOAT_EDGE)), FLOAT_EDGE):
        (mx if axis == "x" else my)[y, x] = v
    return mx, my


def fixed_edge_maps(shape, interp):
    """Identity FIXED maps with FIXED_EDGE planted along the axis; the other coordinate stays the identity's."""
    sw, sh, dw, dh = shape
    axis = THIN_WHY[shape][0]
    x, y = np.meshgrid(np.arange(dw), np.arange(dh))
    sx, sy = x.astype(np.int64), y.astype(np.int64)
    fx, fy = np.zeros_like(sx), np.zeros_like(sx)
    for (yy, xx), (idx, frac) in zip(_edge_slots(shape, len(FIXED_EDGE)), FIXED_EDGE):
        if axis == "x":
            sx[yy, xx], fx[yy, xx] = idx, frac
        else:
            sy[yy, xx], fy[yy, xx] = idx, frac
    if interp == NEAREST:
        fx[:], fy[:] = 0, 0
    return rc.pack_fixed(sx, sy, fx, fy)


def keystone_far(shape):
    """A keystone whose denominator grows to about 1.33 along the axis and whose numerator is scaled so that the last
    output index still samples the last source index: sx = a x / (1 + g x) with sx(dw - 1) = sw - 1."""
    sw, sh, dw, dh = shape
    axis = THIN_WHY[shape][0]
    g = 1.0e-5
    n_src, n_dst = (sw, dw) if axis == "x" else (sh, dh)
    a = (n_src - 1) * (1.0 + g * (n_dst - 1)) / (n_dst - 1)
    return [a, 0.0, 0.0, 0.0, 1.0, 0.0, g, 0.0, 1.0] if axis == "x" else [1.0, 0.0, 0.0, 0.0, a, 0.0, 0.0, g, 1.0]


def perspective_thin_matrices(shape):
    """[(name, matrix, why)], all inverse-mapped."""
    return [("identity", rc.embed([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), "w == 1: S / w exact, indices up to 32765"),
            ("keystone", rc.KEYSTONE, "the suite's keystone at column and row indices up to 32765: w up to 33"),
            ("keystone-far", keystone_far(shape), "w grows along the axis and the far end of the source is still sampled")]


# (src w, src h, dst w, dst h) of resize -> reason
RESIZE_WHY = collections.OrderedDict([
    ((100003, 2, 70001, 3), "down in x past 2^16 columns on both sides, up in y; fp32 coordinates with few fraction bits"),
    ((70001, 3, 100003, 2), "up in x past 2^16 columns, down in y"),
    ((3, 100003, 2, 70001), "the same lengths along y: row indices past 2^16, thousands of bands"),
    ((65536, 4, 4096, 2), "AREA 16 x 2 from a row of 2^16 pixels, and LINEAR and NEAREST at an exact factor"),
    ((1, 1, 100003, 1), "one pixel stretched over 391 strips"),
    ((100003, 1, 1, 1), "a row of 10^5 pixels into one"),
])
RESIZE_PAIRS = tuple(RESIZE_WHY)

# the guarded runs: one shape with the widest output (M % 4 == 2: consecutive gray8 rows alternate between the dword
# store and the byte stores of warp_store), one matrix or map per call family
GUARDED_SHAPE = (M, 3, M, 2)
GUARDED_OFFS_OUT = {1: (0, 1, 2, 3), 4: (0, 4)}
GUARDED_RESIZE = (100003, 2, 70001, 3)

# ---- 2. warp_affine matrices just under the 2^20 bound ----------------------------------------------------------------
T_INT = float((1 << 20) - 1 - (M - 1))            # 1015810: with dst w (h) = M the row's sum is 2^20 - 1
NEAR_2_30 = (1 << 30) - (1 << 21)
TIE_BASE = 1015808.0                              # ties far outside: (TIE_BASE + k / 2048) * 1024 = n + 0.5, k odd
VISIBLE_TIE_BASE = 522240.0                       # 510 * 1024: |v * 1024| just under 2^29, and twice it stays under 2^20

BoundCase = collections.namedtuple("BoundCase", "name shape m interp decisive step reach why")
# decisive: the matrix entry whose growth the check must refuse; step "ulp": the next double up in magnitude is refused,
# "one": the entry is an integer one below the bound (the next double keeps the sum below 2^20, the entry + 1 does not).
# reach: the least max |X| or |Y| (rd included) the reference's coordinates must show.


def _largest_accepted(limit_over, shape, make):
    """The largest double v < limit_over for which accepts() takes make(v)."""
    v = float(np.nextafter(limit_over, 0.0))
    sw, sh, dw, dh = shape
    while accepts(1, sw, sh, dw, dh, 1, make(v), LINEAR | INVERSE_MAP, 0) != 0:
        v = float(np.nextafter(v, 0.0))
    return v


def _tie_shift(sign, k, interp):
    """The offset j (in 1/1024 pixel) of a visible tie: with the tie rounded half to even the second output pixel's
    coordinate is B - 1 or B (B = 32 for LINEAR: the first fraction step, 1024 for NEAREST: the first index step), with
    the nearest wrong rounding (half away from zero, half up, truncation, floor) it is on the other side of B."""
    rd, B = (16, 32) if interp == LINEAR else (512, 1024)
    right = {(1, 1): 0, (1, 3): 2, (-1, 1): 0, (-1, 3): -2}[sign, k]        # rint(sign * k / 2), half to even
    wrong_is_larger = (sign, k) in ((1, 1), (-1, 3))
    target = B - 1 if wrong_is_larger else B
    return target - rd - right, target


def bound_cases():
    """Every case of section 2, all inverse-mapped."""
    out = []
    big_x, big_y = (M, 3, M, 2), (3, M, 2, M)
    full, tie, vis = (1 << 30) - 512, int(TIE_BASE) * 1024 - 512, int(VISIBLE_TIE_BASE) * 1024 - 512    # reaches, rd off
    for sign in (1.0, -1.0):
        # a unit step and an integer translation: the row's sum is 2^20 - 1
        out.append(BoundCase("tx%+d" % sign, big_x, [1.0, 0.0, sign * T_INT, 0.0, 1.0, 0.0], None, 2, "one",
                             NEAR_2_30 if sign > 0 else int(T_INT) * 1024 - 512,
                             "X0 + adelta + rd next to +2^30 (sign +) or from -T * 1024 up (sign -): every tap outside"))
        out.append(BoundCase("ty%+d" % sign, big_y, [1.0, 0.0, 0.0, 0.0, 1.0, sign * T_INT], None, 5, "one",
                             NEAR_2_30 if sign > 0 else int(T_INT) * 1024 - 512, "the same for Y0 + rd along rows"))
        # ... and with the step's sign following the translation's, so that -2^30 is reached too; the translation is the
        # largest double the check accepts
        tx = _largest_accepted(LIMIT - (M - 1), big_x, lambda v: [sign, 0.0, sign * v, 0.0, 1.0, 0.0])
        out.append(BoundCase("tight-tx%+d" % sign, big_x, [sign, 0.0, sign * tx, 0.0, 1.0, 0.0], None, 2, "ulp", full,
                             "the largest accepted translation with a step of its sign: |X| reaches 2^30"))
        ty = _largest_accepted(LIMIT - (M - 1), big_y, lambda v: [1.0, 0.0, 0.0, 0.0, sign, sign * v])
        out.append(BoundCase("tight-ty%+d" % sign, big_y, [1.0, 0.0, 0.0, 0.0, sign, sign * ty], None, 5, "ulp", full,
                             "the same for Y"))
        # the largest accepted step with dst w = 3: adelta (bdelta) itself reaches 2^30 at the third column
        small = (5, 3, 3, 2)
        i0 = _largest_accepted(LIMIT / 2.0, small, lambda v: [sign * v, 0.0, 0.0, 0.0, 1.0, 0.0])
        out.append(BoundCase("i0%+d" % sign, small, [sign * i0, 0.0, 0.0, 0.0, 1.0, 0.0], None, 0, "ulp", full,
                             "adelta = rint(i0 * 2 * 1024) = +-2^30 in the third column"))
        i3 = _largest_accepted(LIMIT / 2.0, small, lambda v: [1.0, 0.0, 0.0, sign * v, 0.0, 0.0])
        out.append(BoundCase("i3%+d" % sign, small, [1.0, 0.0, 0.0, sign * i3, 0.0, 0.0], None, 3, "ulp", full,
                             "bdelta = +-2^30 in the third column, on the square tile"))
        # ties at large magnitude, even and odd n: every tap stays outside, so the int conversion itself is what runs
        for k in (1, 3):
            out.append(BoundCase("tie%+d-k%d" % (sign, k), (5, 3, 7, 2),
                                 [1.0, 0.0, sign * (TIE_BASE + k / 2048.0), 0.0, 1.0, 0.0], None, None, None,
                                 tie, "(i1 y + i2) * 1024 = +-(n + 0.5) at |n| > 10^9: a tie for rint"))
            # ... and ties whose rounding decides an output pixel: the second column lands on the first step of the
            # fraction (LINEAR) or of the index (NEAREST) exactly when the tie is rounded half to even
            for interp in (NEAREST, LINEAR):
                j, _ = _tie_shift(int(sign), k, interp)
                i2 = sign * (VISIBLE_TIE_BASE + k / 2048.0)
                i0 = -sign * VISIBLE_TIE_BASE + j / 1024.0
                tag = "visible-tie%+d-k%d-%s" % (sign, k, "linear" if interp == LINEAR else "nearest")
                out.append(BoundCase(tag + "-x", (5, 3, 2, 2), [i0, 0.0, i2, 0.0, 1.0, 0.0], interp, None, None, vis,
                                     "X0 is a tie just under 2^29 and adelta brings the second column back to the first "
                                     "source pixels"))
                out.append(BoundCase(tag + "-y", (3, 5, 2, 2), [0.0, 1.0, 0.0, i0, 0.0, i2], interp, None, None, vis,
                                     "the same for Y0 and bdelta: the second column walks down the first source column"))
    return out


def visible_tie_target(case):
    """(axis, the coordinate X (Y) of output pixel (row 0, column 1) when the tie is rounded half to even, B)."""
    assert case.name.startswith("visible-tie")
    sign = 1 if "+1" in case.name else -1
    k = 1 if "-k1-" in case.name else 3
    _, target = _tie_shift(sign, k, case.interp)
    return case.name[-1], target, 32 if case.interp == LINEAR else 1024


def tie_source(sw, sh, bpp):
    """A source whose neighbours along both axes are 0 and 255 in turn, so a tap or a fraction that moves by one shows."""
    y, x = np.mgrid[0:sh, 0:sw]
    img = (((x + y) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(img[..., None], 4, 2)) if bpp == 4 else img


# ---- 3. perspective saturation ----------------------------------------------------------------------------------------
PERSP_SRC = (40, 36)                              # (src w, src h)
PERSP_DST = ((5, 2), (33, 33))                    # one ragged tile; a 2 x 2 grid of tiles with a one-pixel edge
HIGH, LOW, NAN, PLAIN = "high", "low", "nan", "plain"


def straddle(interp, dw):
    """x and y grow by 2^31 / (3 S) (dst w = 5) or 2^31 / (6 S) per pixel: S * coordinate passes 2^31 - 1 after column
    2 (5), inside the first lane's four columns (between the first lane and the third)."""
    S = 32.0 if interp == LINEAR else 1.0
    a = 2147483648.0 / ((3.0 if dw < 8 else 6.0) * S)
    return [a, 0.0, 0.0, 0.0, a, 0.0, 0.0, 0.0, 1.0]


def saturation_cases(interp, dw):
    """[(name, matrix, branches it is there for, why)], inverse-mapped, entries all finite."""
    return [("+1e9", [1e9, 0.0, 0.0, 0.0, 1e9, 0.0, 0.0, 0.0, 1.0], {HIGH, PLAIN},
             "column 0 and row 0 give 0, everything else is at least 2^31: INT_MAX"),
            ("-1e9", [-1e9, 0.0, 0.0, 0.0, -1e9, 0.0, 0.0, 0.0, 1.0], {LOW, PLAIN},
             "the numerator rows negated (all nine entries negated are the same map): below -2^31, INT_MIN"),
            ("denormal", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1e-320], {NAN, HIGH},
             "w is a nonzero fp64 denormal: S / w is inf, and 0 * inf = NaN at (0, 0), which maps to INT_MAX; a flushed "
             "w would be 0 and give source (0, 0)"),
            ("denormal-shift", [1.0, 0.0, 5.0, 0.0, 1.0, 7.0, 0.0, 0.0, 1e-320], {HIGH},
             "inf without a NaN"),
            ("straddle", straddle(interp, dw), {HIGH, PLAIN},
             "saturated and unsaturated lanes in one row pass")]


def perspective_t(m, dw, dh, flags):
    """(tX, tY) float64 (dh, dw): the coordinates times S before the rounding, in the header's operations (what
    remap_ref.perspective_coords rounds; test_limits_cpu.py ties the two together)."""
    h = perspective_inverse(m, flags)
    S = np.float64(32.0 if (flags & ~INVERSE_MAP) == LINEAR else 1.0)
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        w = (h[6] * x) + (h[7] * y + h[8])
        s = np.where(w != 0, S / np.where(w != 0, w, 1.0), 0.0)
        return ((h[0] * x) + (h[1] * y + h[2])) * s, ((h[3] * x) + (h[4] * y + h[5])) * s


def branch_of(t):
    """Which branch of persp_round each value takes: an array of HIGH / LOW / NAN / PLAIN."""
    out = np.full(t.shape, PLAIN, dtype=object)
    out[t >= 2147483647.0] = HIGH
    out[t < -2147483648.0] = LOW
    out[np.isnan(t)] = NAN
    return out


def round_t(t):
    """persp_round of the header on float64 values -> int64."""
    with np.errstate(all="ignore"):
        f = np.where(~(t < 2147483647.0), 2147483647.0, t)
        f = np.where(f < -2147483648.0, -2147483648.0, f)
        r = np.rint(f).astype(np.int64)
    assert r.min() >= INT_MIN and r.max() <= INT_MAX
    return r


# ---- 4. thousands of tiny frames ---------------------------------------------------------------------------------------
TINY_WHY = collections.OrderedDict([
    ((5, 3, 7, 2), "a ragged frame of 15 source and 14 output pixels: consecutive gray8 frames start at every residue"),
    ((1, 1, 1, 1), "one pixel: a work item whose tile holds one live lane"),
])
TINY_SHAPES = tuple(TINY_WHY)
TINY_N = 3001                                     # warp_affine, perspective: 3001 work items, three padding waves
REMAP_N = (3001, 3002, 3003)                      # chunks of 4 frames: 751 work items whose last holds 1, 2, 3 frames
ADAPTIVE_N, ADAPTIVE_SHAPE, ADAPTIVE_BLOCKS = 2001, (7, 5), (3, 63)      # (w, h); the smallest and the largest block
TINY_VARIANTS = ((NEAREST, 0), (LINEAR, 1))       # (interp, border): both interpolations, one border each
TINY_AFFINE = rotation(2.0, 1.0, 30.0)            # about the centre of the 5 x 3 source: taps inside and outside
TINY_PERSPECTIVE = [1.0, 0.1, -1.0, 0.02, 1.05, -0.5, 1.0e-2, -1.0e-2, 1.0]


def tiny_matrices(shape):
    """(affine matrix, homography) of a tiny shape; the one-pixel frame takes the identity, so that its pixel shows."""
    if shape == (1, 1, 1, 1):
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], rc.embed([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    return TINY_AFFINE, TINY_PERSPECTIVE
