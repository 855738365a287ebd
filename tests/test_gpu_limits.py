"""GPU suite (-m gpu): the geometric calls at the bounds their argument checks accept (cases and reasons:
tests/limit_cases.py; tests/test_limits_cpu.py shows that each case reaches what it is there for).

Frames of MI355_MAX_WARP_SIZE pixels along one side and two or three along the other, resize rows of 10^5 pixels, affine
matrices whose fixed-point coordinates sit next to 2^30, homographies whose coordinates saturate or are NaN, and batches
of thousands of tiny frames through warp_affine, perspective, remap and the adaptive threshold.  Every comparison is
bit identity with the numpy references (warp_ref.py, remap_ref.py, resize_ref.py, box_ref.py) on every pixel; before
every launch the matching *_check binding must return MI355_OK, and every test asserts how many comparisons it ran.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded  # noqa: E402
import limit_cases as lc  # noqa: E402
import remap_cases as rc  # noqa: E402
import tiny_batch_cases as tb  # noqa: E402
from box_ref import BINARY, adaptive_ref  # noqa: E402
from remap_ref import FIXED, FLOAT, map_coords, perspective_coords, perspective_ref, remap_ref, sample  # noqa: E402
from resize_ref import AREA, accepts as resize_accepts, resize_ref  # noqa: E402
from test_gpu_median import extremes, noise  # noqa: E402
from test_gpu_remap import _DeviceMaps  # noqa: E402
from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, warp_ref  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
VALUE = lc.VALUE
KIND_NAME = {FIXED: "fixed", FLOAT: "float"}
INTERP_NAME = {NEAREST: "nearest", LINEAR: "linear", AREA: "area"}


def _id(bpp, interp, border=None, kind=None):
    parts = ["rgba" if bpp == 4 else "gray8", INTERP_NAME[interp]]
    if border is not None:
        parts.append("replicate" if border else "constant")
    if kind is not None:
        parts.append(KIND_NAME[kind])
    return "-".join(parts)


VARIANTS = [(bpp, i, b) for bpp in (4, 1) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)]
REMAP_VARIANTS = [v + (k,) for v in VARIANTS for k in (FIXED, FLOAT)]
BPP_INTERP = [(bpp, i) for bpp in (4, 1) for i in (NEAREST, LINEAR)]
RESIZE_VARIANTS = [(bpp, i) for bpp in (4, 1) for i in (NEAREST, LINEAR, AREA)]


def _two(sw, sh, bpp):
    """Two frames of one shape in one call: noise and 0 / 255 pixels."""
    return np.stack([noise(sh, sw, bpp, sw * 31 + sh), extremes(sh, sw, bpp, sw * 31 + sh + 1)])


def same(got, ref, tag):
    """Every pixel equal, or the first one that is not."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (tag, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        at = tuple(int(v) for v in np.argwhere(got != ref)[0])
        raise AssertionError("%s: %d byte(s) differ, the first at %s: got %d, want %d"
                             % (tag, int((got != ref).sum()), at, int(got[at]), int(ref[at])))


def _warp(ctx, bpp, img, m, dw, dh, flags, border, value):
    fn = ctx.warp_affine if bpp == 4 else ctx.warp_affine_gray8
    return fn(img, m, dw, dh, flags, border, value)


def _remap(ctx, bpp, img, map1, map2, kind, interp, border, value):
    dh, dw = np.asarray(map1).shape[:2]
    fn = ctx.remap if bpp == 4 else ctx.remap_gray8
    return fn(img, map1, map2, dw, dh, kind, interp, border, value)


def _perspective(ctx, bpp, img, m, dw, dh, flags, border, value):
    fn = ctx.warp_perspective if bpp == 4 else ctx.warp_perspective_gray8
    return fn(img, m, dw, dh, flags, border, value)


# ---- 1. maximum-size thin frames --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=[_id(*v) for v in VARIANTS])
def test_thin_warp_affine(ctx, pkg, bpp, interp, border):
    ran = 0
    for shape in lc.WARP_THIN:
        sw, sh, dw, dh = shape
        frames = _two(sw, sh, bpp)
        for name, m, _ in lc.warp_thin_matrices(shape):
            for inv in (INVERSE_MAP, 0):
                flags = interp | inv
                assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK, (shape, name, inv)
                got = _warp(ctx, bpp, frames, m, dw, dh, flags, border, VALUE)
                for f in range(2):
                    same(got[f], warp_ref(frames[f], m, dw, dh, flags, border, VALUE), (shape, name, inv, f))
                    ran += 1
    assert ran == (6 * 3 + 2 + 2) * 2 * 2 == 88


@pytest.mark.parametrize("bpp,interp,border,kind", REMAP_VARIANTS, ids=[_id(*v) for v in REMAP_VARIANTS])
def test_thin_remap(ctx, pkg, bpp, interp, border, kind):
    ran = 0
    for shape in lc.THIN:
        sw, sh, dw, dh = shape
        frames = _two(sw, sh, bpp)
        assert pkg.remap_check(bpp, sw, sh, dw, dh, 2, kind, interp, border) == OK, shape
        for name, map1, map2, _ in lc.remap_thin_maps(shape, kind, interp):
            coords = map_coords(map1, map2, kind, interp)
            got = _remap(ctx, bpp, frames, map1, map2, kind, interp, border, VALUE)
            for f in range(2):
                same(got[f], sample(frames[f], coords, interp, border, VALUE), (shape, name, f))
                ran += 1
    assert ran == 4 * 4 * 2 == 32


@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=[_id(*v) for v in VARIANTS])
def test_thin_perspective(ctx, pkg, bpp, interp, border):
    ran = 0
    flags = interp | INVERSE_MAP
    for shape in lc.THIN:
        sw, sh, dw, dh = shape
        frames = _two(sw, sh, bpp)
        for name, m, _ in lc.perspective_thin_matrices(shape):
            assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK, (shape, name)
            coords = perspective_coords(m, dw, dh, flags)
            got = _perspective(ctx, bpp, frames, m, dw, dh, flags, border, VALUE)
            for f in range(2):
                same(got[f], sample(frames[f], coords, interp, border, VALUE), (shape, name, f))
                ran += 1
    assert ran == 4 * 3 * 2 == 24


@pytest.mark.parametrize("bpp,interp", RESIZE_VARIANTS, ids=[_id(*v) for v in RESIZE_VARIANTS])
def test_long_resize_rows(ctx, pkg, bpp, interp):
    ran = 0
    for sw, sh, dw, dh in lc.RESIZE_PAIRS:
        if not resize_accepts(interp, sw, sh, dw, dh):
            continue
        assert pkg.resize_check(bpp, sw, sh, dw, dh, 2, interp) == OK, (sw, sh, dw, dh)
        frames = _two(sw, sh, bpp)
        got = ctx.resize(frames, dw, dh, interp) if bpp == 4 else ctx.resize_gray8(frames, dw, dh, interp)
        for f in range(2):
            same(got[f], resize_ref(frames[f], dw, dh, interp), ((sw, sh, dw, dh), f))
            ran += 1
    assert ran == (1 if interp == AREA else 6) * 2


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=[_id(*v) for v in BPP_INTERP])
def test_thin_frames_in_the_guarded_arena(ctx, pkg, bpp, interp):
    """The widest output through the guarded arena, one matrix or map per call family: M % 4 == 2, so consecutive gray8
    output rows alternate between the dword store and the byte stores, at every output alignment.  No guard byte
    changes, no payload byte stays unwritten."""
    shape = lc.GUARDED_SHAPE
    sw, sh, dw, dh = shape
    offs = lc.GUARDED_OFFS_OUT[bpp]
    img = noise(sh, sw, bpp, 77)
    flags = interp | INVERSE_MAP
    half = dict((n, m) for n, m, _ in lc.warp_thin_matrices(shape))["half"]
    far = lc.keystone_far(shape)
    edge = {kind: [m[1:3] for m in lc.remap_thin_maps(shape, kind, interp) if m[0] == "edge"][0] for kind in (FIXED, FLOAT)}
    ran = 0
    maps = _DeviceMaps(ctx)
    try:
        d_maps = {kind: (maps.put((kind, 1), edge[kind][0], 0), maps.put((kind, 2), edge[kind][1], 0))
                  for kind in (FIXED, FLOAT)}
        for border in (CONSTANT, REPLICATE):
            assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, 1, half, flags, border) == OK
            assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, 1, far, flags, border) == OK
            calls = [("warp_affine", warp_ref(img, half, dw, dh, flags, border, VALUE),
                      lambda a, b: ctx.warp_affine_dev(a, b, bpp, sw, sh, dw, dh, 1, half, flags, border, VALUE)),
                     ("perspective", perspective_ref(img, far, dw, dh, flags, border, VALUE),
                      lambda a, b: ctx.warp_perspective_dev(a, b, bpp, sw, sh, dw, dh, 1, far, flags, border, VALUE))]
            for kind in (FIXED, FLOAT):
                assert pkg.remap_check(bpp, sw, sh, dw, dh, 1, kind, interp, border) == OK
                d1, d2 = d_maps[kind]
                map1, map2 = edge[kind]
                calls.append(("remap " + KIND_NAME[kind], remap_ref(img, map1, map2, kind, interp, border, VALUE),
                              lambda a, b, kind=kind, d1=d1, d2=d2: ctx.remap_dev(
                                  a, b, bpp, sw, sh, dw, dh, 1, d1, d2, kind, interp, border, VALUE)))
            for name, ref, call in calls:
                for n, off_out in enumerate(offs):
                    off_in = offs[(n + 1) % len(offs)]
                    tag = "%s bpp %d interp %d border %d" % (name, bpp, interp, border)
                    got = guarded.run(ctx, call, img, ref, off_in=off_in, off_out=off_out, tag=tag)
                    guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
                    ran += 1
    finally:
        maps.free()
    # a resize row of 10^5 pixels, at the same alignments
    rw, rh, rdw, rdh = lc.GUARDED_RESIZE
    assert pkg.resize_check(bpp, rw, rh, rdw, rdh, 1, interp) == OK
    img = noise(rh, rw, bpp, 78)
    ref = resize_ref(img, rdw, rdh, interp)
    for n, off_out in enumerate(offs):
        off_in = offs[(n + 1) % len(offs)]
        tag = "resize bpp %d interp %d" % (bpp, interp)
        got = guarded.run(ctx, lambda a, b: ctx.resize_dev(a, b, bpp, rw, rh, rdw, rdh, 1, interp), img, ref,
                          off_in=off_in, off_out=off_out, tag=tag)
        guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
        ran += 1
    assert ran == (2 * 4 + 1) * len(offs)


# ---- 2. warp_affine matrices just under the 2^20 bound ----------------------------------------------------------------
@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=[_id(*v) for v in VARIANTS])
def test_warp_affine_just_under_the_coordinate_bound(ctx, pkg, bpp, interp, border):
    """|X| and |Y| next to 2^30: an int sum that wraps, or a tie rounded another way, moves a tap.  The visible ties sit
    on a source of alternating 0 and 255, where a coordinate that is off by 1 / 1024 pixel changes the output."""
    ran = 0
    flags = interp | INVERSE_MAP
    for c in lc.bound_cases():
        if c.interp not in (None, interp):
            continue
        sw, sh, dw, dh = c.shape
        img = lc.tie_source(sw, sh, bpp) if c.name.startswith("visible-tie") else noise(sh, sw, bpp, 5)
        assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, 1, c.m, flags, border) == OK, c.name
        for value in lc.VALUES:
            same(_warp(ctx, bpp, img, c.m, dw, dh, flags, border, value), warp_ref(img, c.m, dw, dh, flags, border, value),
                 (c.name, hex(value)))
            ran += 1
    assert ran == (2 * (6 + 2) + 8) * 2 == 48


# ---- 3. perspective saturation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=[_id(*v) for v in VARIANTS])
def test_perspective_coordinates_that_saturate(ctx, pkg, bpp, interp, border):
    """t >= 2^31 - 1, t < -2^31 and NaN: INT_MAX, INT_MIN and INT_MAX, far outside on the side the coordinate left the
    frame.  Five frames: one whole chunk of frames and a ragged one."""
    sw, sh = lc.PERSP_SRC
    frames = np.stack([noise(sh, sw, bpp, 31 + f) for f in range(5)])
    flags = interp | INVERSE_MAP
    ran = 0
    for dw, dh in lc.PERSP_DST:
        for name, m, _, _ in lc.saturation_cases(interp, dw):
            assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, 5, m, flags, border) == OK, name
            coords = perspective_coords(m, dw, dh, flags)
            for value in lc.VALUES:
                got = _perspective(ctx, bpp, frames, m, dw, dh, flags, border, value)
                for f in range(5):
                    same(got[f], sample(frames[f], coords, interp, border, value), (name, (dw, dh), hex(value), f))
                    ran += 1
    assert ran == 2 * 5 * 2 * 5 == 100


# ---- 4. thousands of tiny frames ---------------------------------------------------------------------------------------
OFFSETS = {4: ((0, 0), (4, 4)), 1: ((0, 0), (3, 1))}
TINY = [(bpp, i, b) for bpp in (4, 1) for i, b in lc.TINY_VARIANTS]


def compare_frames(got, expected, tag):
    """Every byte of every frame equal, or the first wrong frame by its index."""
    assert got.shape == expected.shape, (tag, got.shape, expected.shape)
    if not np.array_equal(got, expected):
        wrong = np.flatnonzero((got != expected).reshape(got.shape[0], -1).any(axis=1))
        f = int(wrong[0])
        unwritten = int((got == guarded.prefill_of(expected)).sum())
        raise AssertionError("%s: %d of %d frame(s) wrong, the first is frame %d (member %d of the cycle): got %s, want %s"
                             "; %d byte(s) still hold the prefill"
                             % (tag, wrong.size, got.shape[0], f, int(tb.frame_index(got.shape[0])[f]),
                                got[f].ravel()[:16].tolist(), expected[f].ravel()[:16].tolist(), unwritten))


def _each(fn, frames):
    return np.ascontiguousarray(np.stack([fn(f) for f in frames]))


@pytest.mark.parametrize("bpp,interp,border", TINY, ids=[_id(*v) for v in TINY])
def test_thousands_of_tiny_frames_warp_and_perspective(ctx, pkg, bpp, interp, border):
    ran = 0
    n = lc.TINY_N
    for shape in lc.TINY_SHAPES:
        sw, sh, dw, dh = shape
        d, x = tb.distinct(sh, sw, bpp), tb.batch(sh, sw, n, bpp)
        m6, m9 = lc.tiny_matrices(shape)
        assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, n, m6, interp, border) == OK
        assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, n, m9, interp, border) == OK
        calls = [("warp_affine", _each(lambda f: warp_ref(f, m6, dw, dh, interp, border, VALUE), d),
                  lambda a, b: ctx.warp_affine_dev(a, b, bpp, sw, sh, dw, dh, n, m6, interp, border, VALUE)),
                 ("perspective", _each(lambda f: perspective_ref(f, m9, dw, dh, interp, border, VALUE), d),
                  lambda a, b: ctx.warp_perspective_dev(a, b, bpp, sw, sh, dw, dh, n, m9, interp, border, VALUE))]
        for name, ref14, call in calls:
            expected = tb.expand(ref14, n)
            for off in OFFSETS[bpp]:
                tag = "%s %s n %d off %s" % (name, shape, n, off)
                compare_frames(guarded.run(ctx, call, x, expected, off[0], off[1], tag=tag), expected, tag)
                ran += 1
    assert ran == 2 * 2 * 2


TINY_REMAP = [v + (k,) for v in TINY for k in (FIXED, FLOAT)]


@pytest.mark.parametrize("bpp,interp,border,kind", TINY_REMAP, ids=[_id(*v) for v in TINY_REMAP])
def test_thousands_of_tiny_frames_remap(ctx, pkg, bpp, interp, border, kind):
    """3001, 3002 and 3003 frames: 751 chunks of four whose last holds 1, 2 and 3 frames."""
    shape = lc.TINY_SHAPES[0]
    sw, sh, dw, dh = shape
    d = tb.distinct(sh, sw, bpp)
    map1, map2 = rc.affine_fixed_maps(lc.TINY_AFFINE, dw, dh, interp) if kind == FIXED else \
        rc.affine_float_maps(lc.TINY_AFFINE, dw, dh)
    ref14 = _each(lambda f: remap_ref(f, map1, map2, kind, interp, border, VALUE), d)
    ran = 0
    maps = _DeviceMaps(ctx)
    try:
        d1, d2 = maps.put(1, map1, 0), maps.put(2, map2, 0)
        for n in lc.REMAP_N:
            assert pkg.remap_check(bpp, sw, sh, dw, dh, n, kind, interp, border) == OK
            x, expected = tb.batch(sh, sw, n, bpp), tb.expand(ref14, n)
            for off in OFFSETS[bpp]:
                tag = "remap %s %s n %d off %s" % (KIND_NAME[kind], shape, n, off)
                got = guarded.run(ctx, lambda a, b: ctx.remap_dev(a, b, bpp, sw, sh, dw, dh, n, d1, d2, kind, interp, border,
                                                                  VALUE), x, expected, off[0], off[1], tag=tag)
                compare_frames(got, expected, tag)
                ran += 1
    finally:
        maps.free()
    assert ran == 3 * 2


@pytest.mark.parametrize("block", lc.ADAPTIVE_BLOCKS)
def test_thousands_of_tiny_frames_adaptive_threshold(ctx, pkg, block):
    w, h = lc.ADAPTIVE_SHAPE
    n = lc.ADAPTIVE_N
    assert block <= pkg.MAX_BOX_K and pkg.adaptive_threshold_check(w, h, n, 200, BINARY, block, 2) == OK
    ref14 = _each(lambda f: adaptive_ref(f, 200, BINARY, block, 2), tb.distinct(h, w, 1))
    x, expected = tb.batch(h, w, n, 1), tb.expand(ref14, n)
    assert 0 < int((expected == 200).sum()) < expected.size
    ran = 0
    for off in OFFSETS[1]:
        tag = "adaptive block %d n %d off %s" % (block, n, off)
        got = guarded.run(ctx, lambda a, b: ctx.adaptive_threshold_gray8_dev(a, b, w, h, n, 200, BINARY, block, 2), x,
                          expected, off[0], off[1], tag=tag)
        compare_frames(got, expected, tag)
        ran += 1
    assert ran == 2
