"""GPU suite (-m gpu): what the fourteen batched host-buffer entry points share, through raw library calls.

mi355_filter_batched, mi355_resize_batched, mi355_warp_affine_batched, mi355_remap_batched,
mi355_warp_perspective_batched and mi355_adaptive_threshold_gray8_batched, and the feature calls
mi355_clahe_gray8_batched, mi355_ccl_gray8_batched, mi355_dist_gray8_batched, mi355_hysteresis_gray8_batched,
mi355_canny_gray8_batched, mi355_hough_lines_gray8_batched, mi355_yuv_to_rgba8_batched and mi355_rgba8_to_yuv_batched
stage their frames the same way: pointer checks, the call's value checks, the input-format rule, then one round trip
through the context's pooled buffers; the calls with several outputs lay them side by side in the pooled output buffer.
Two things no per-feature test looks at are pinned here: the order in which a call with several faults answers, and that
one context's pooled buffers serve every entry point in any order, growing and shrinking, with and without timestamps.
Every shape is tiny (none above 96 x 64).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canny_cases  # noqa: E402
import ccl_cases  # noqa: E402
import clahe_cases  # noqa: E402
import dist_cases  # noqa: E402
import hough_cases  # noqa: E402
import hough_ref  # noqa: E402
import remap_cases as cases  # noqa: E402
import yuv_cases  # noqa: E402
import yuv_ref  # noqa: E402
from box_ref import BINARY, adaptive_ref  # noqa: E402
from canny_ref import canny_ref, hysteresis_ref  # noqa: E402
from ccl_ref import ccl_ref  # noqa: E402
from clahe_ref import clahe_ref  # noqa: E402
from dist_ref import dist_ref  # noqa: E402
from remap_ref import FIXED, FLOAT, convert_maps, perspective_ref, remap_ref  # noqa: E402
from resize_ref import resize_ref  # noqa: E402
from test_gpu_median import noise  # noqa: E402
from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, warp_ref  # noqa: E402

pytestmark = pytest.mark.gpu

AREA = 3
NAN = float("nan")
PI = hough_cases.PI
VALUE = 0x80FF407F
_u8p = ctypes.POINTER(ctypes.c_uint8)


def _doubles(m):
    return None if m is None else (ctypes.c_double * len(m))(*m)


def _addr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# One builder per entry point: the call's own values -> call(lib, handle, in, out, prof_ns) -> return code
def filter_call(filt, w, h, n, k, sigma):
    return lambda lib, hd, i, o, prof: lib.mi355_filter_batched(hd, filt, i, o, w, h, n, k, sigma, prof)


def resize_call(bpp, sw, sh, dw, dh, n, interp):
    return lambda lib, hd, i, o, prof: lib.mi355_resize_batched(hd, i, o, bpp, sw, sh, dw, dh, n, interp, prof)


def warp_call(bpp, sw, sh, dw, dh, n, m, flags, border):
    return lambda lib, hd, i, o, prof: lib.mi355_warp_affine_batched(hd, i, o, bpp, sw, sh, dw, dh, n, _doubles(m),
                                                                     flags, border, VALUE, prof)


def remap_call(bpp, sw, sh, dw, dh, n, map1, map2, kind, interp, border):
    return lambda lib, hd, i, o, prof: lib.mi355_remap_batched(hd, i, o, bpp, sw, sh, dw, dh, n, _addr(map1),
                                                               _addr(map2), kind, interp, border, VALUE, prof)


def perspective_call(bpp, sw, sh, dw, dh, n, m, flags, border):
    return lambda lib, hd, i, o, prof: lib.mi355_warp_perspective_batched(hd, i, o, bpp, sw, sh, dw, dh, n, _doubles(m),
                                                                          flags, border, VALUE, prof)


def adaptive_call(w, h, n, max_value, type, block, delta):
    return lambda lib, hd, i, o, prof: lib.mi355_adaptive_threshold_gray8_batched(hd, i, o, w, h, n, max_value, type,
                                                                                  block, delta, prof)


def clahe_call(w, h, n, clip_limit, tiles_x, tiles_y):
    return lambda lib, hd, i, o, prof: lib.mi355_clahe_gray8_batched(hd, i, o, w, h, n, clip_limit, tiles_x, tiles_y,
                                                                     prof)


def hysteresis_call(w, h, n, low, high, connectivity):
    return lambda lib, hd, i, o, prof: lib.mi355_hysteresis_gray8_batched(hd, i, o, w, h, n, low, high, connectivity,
                                                                          prof)


def canny_call(w, h, n, threshold1, threshold2, flags):
    return lambda lib, hd, i, o, prof: lib.mi355_canny_gray8_batched(hd, i, o, w, h, n, threshold1, threshold2, flags,
                                                                     prof)


def yuv_decode_call(w, h, n, layout, standard, pitch, rows):
    return lambda lib, hd, i, o, prof: lib.mi355_yuv_to_rgba8_batched(hd, i, o, w, h, n, layout, standard, pitch, rows,
                                                                      prof)


def yuv_encode_call(w, h, n, layout, standard, pitch, rows):
    return lambda lib, hd, i, o, prof: lib.mi355_rgba8_to_yuv_batched(hd, i, o, w, h, n, layout, standard, pitch, rows,
                                                                      prof)


# The calls with several outputs: `out` is the first of them, the call closes over the arrays that take the others
# (None: not taken) and fills them with a pattern before it runs; call.others lists them for the caller to compare.
def _with_others(call, *others):
    def run(lib, hd, i, o, prof):
        for a in run.others:
            a.view(np.uint8)[...] = 0xA5
        return call(lib, hd, i, o, prof)
    run.others = [a for a in others if a is not None]
    return run


def ccl_call(w, h, n, connectivity, stats_rows, count, stats=None, sums=None):
    return _with_others(lambda lib, hd, i, o, prof: lib.mi355_ccl_gray8_batched(
        hd, i, o, _addr(count), _addr(stats), _addr(sums), w, h, n, connectivity, stats_rows, prof), count, stats, sums)


def dist_call(w, h, n, sq=None, nearest=None):
    """out takes the float32 distances, the second of the three outputs: with sq, not the one the round trip reads"""
    return _with_others(lambda lib, hd, i, o, prof: lib.mi355_dist_gray8_batched(
        hd, i, _addr(sq), o, _addr(nearest), w, h, n, prof), sq, nearest)


def hough_call(w, h, n, rho, theta, threshold, max_lines, min_theta, max_theta, votes, count):
    return _with_others(lambda lib, hd, i, o, prof: lib.mi355_hough_lines_gray8_batched(
        hd, i, o, _addr(votes), _addr(count), w, h, n, rho, theta, threshold, max_lines, min_theta, max_theta, prof),
        votes, count)


IDENT6 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
# the further outputs of the feature calls of the table below: no call of it gets as far as writing them
COUNT, VOTES = np.zeros(1, np.int32), np.zeros(8, np.int32)
STATS, SUMS = np.zeros((4, 5), np.int32), np.zeros((4, 2), np.uint64)
IDENT9 = cases.embed(IDENT6)
MAPX, MAPY = cases.identity_float_maps(16, 8)
# every row: (entry point, a valid call on 1-byte frames (the YUV calls: on their own frames), the same call with one
# bad value, or one missing further output, each)
PRECEDENCE = [
    ("filter", filter_call(5, 16, 8, 1, 5, 1.5),                                       # 5: MI355_FILTER_GAUSS_GRAY8
     [filter_call(5, 0, 8, 1, 5, 1.5), filter_call(5, 16, 8, 1, 4, 1.5), filter_call(5, 16, 8, 1, 5, NAN)]),
    ("resize", resize_call(1, 16, 8, 8, 4, 1, LINEAR),
     [resize_call(1, 16, 8, 8, 4, 1, 2), resize_call(1, 0, 8, 8, 4, 1, LINEAR),
      resize_call(1, 16, 8, 8, 0, 1, LINEAR)]),
    ("warp_affine", warp_call(1, 16, 8, 16, 8, 1, IDENT6, LINEAR, CONSTANT),
     [warp_call(1, 16, 8, 16, 8, 1, IDENT6, 3, CONSTANT),
      warp_call(1, 16, 8, 16, 8, 1, IDENT6, LINEAR, 2),
      warp_call(1, 0, 8, 16, 8, 1, IDENT6, LINEAR, CONSTANT),
      warp_call(1, 16, 8, 16, 8, 1, IDENT6[:5] + [NAN], LINEAR, CONSTANT),
      warp_call(1, 16, 8, 16, 8, 1, None, LINEAR, CONSTANT)]),
    ("remap", remap_call(1, 16, 8, 16, 8, 1, MAPX, MAPY, FLOAT, LINEAR, CONSTANT),
     [remap_call(1, 16, 8, 16, 8, 1, MAPX, MAPY, FLOAT, AREA, CONSTANT),
      remap_call(1, 16, 8, 16, 8, 1, MAPX, MAPY, 2, LINEAR, CONSTANT),
      remap_call(1, 16, 8, 16, 8, 1, MAPX, MAPY, FLOAT, LINEAR, 2),
      remap_call(1, 16, 8, 0, 8, 1, MAPX, MAPY, FLOAT, LINEAR, CONSTANT),
      remap_call(1, 16, 8, 16, 8, 1, None, MAPY, FLOAT, LINEAR, CONSTANT)]),
    ("warp_perspective", perspective_call(1, 16, 8, 16, 8, 1, IDENT9, LINEAR, CONSTANT),
     [perspective_call(1, 16, 8, 16, 8, 1, IDENT9, 3, CONSTANT),
      perspective_call(1, 16, 8, 16, 8, 1, IDENT9, LINEAR, 2),
      perspective_call(1, 16, 0, 16, 8, 1, IDENT9, LINEAR, CONSTANT),
      perspective_call(1, 16, 8, 16, 8, 1, [NAN] + IDENT9[1:], LINEAR, CONSTANT)]),
    ("adaptive_threshold", adaptive_call(16, 8, 1, 255, BINARY, 3, 2.0),
     [adaptive_call(0, 8, 1, 255, BINARY, 3, 2.0), adaptive_call(16, 8, 1, 255, 2, 3, 2.0),
      adaptive_call(16, 8, 1, 255, BINARY, 4, 2.0), adaptive_call(16, 8, 1, 256, BINARY, 3, 2.0),
      adaptive_call(16, 8, 1, 255, BINARY, 3, NAN)]),
    ("clahe", clahe_call(16, 8, 1, 2.0, 2, 2),
     [clahe_call(16, 8, 1, 2.0, 0, 2), clahe_call(16, 8, 1, 2.0, 2, 17), clahe_call(16, 8, 1, NAN, 2, 2)]),
    ("ccl", ccl_call(16, 8, 1, 8, 0, COUNT),
     [ccl_call(16, 8, 1, 6, 0, COUNT), ccl_call(16, 8, 1, 8, -1, COUNT), ccl_call(0, 8, 1, 8, 0, COUNT),
      ccl_call(16, 8, 1, 8, 0, None)]),
    ("ccl_stats", ccl_call(16, 8, 1, 8, 4, COUNT, STATS, SUMS),
     [ccl_call(16, 8, 1, 0, 4, COUNT, STATS, SUMS), ccl_call(16, 8, 1, 8, (1 << 24) + 1, COUNT, STATS, SUMS),
      ccl_call(16, 8, 1, 8, 4, COUNT, None, SUMS), ccl_call(16, 8, 1, 8, 4, COUNT, STATS, None)]),
    ("dist", dist_call(16, 8, 1),
     [dist_call(0, 8, 1), dist_call(16385, 1, 1), dist_call(16, 8, 0)]),
    ("hysteresis", hysteresis_call(16, 8, 1, 60, 150, 8),
     [hysteresis_call(16, 8, 1, 60, 150, 6), hysteresis_call(16, 8, 1, -1, 150, 8),
      hysteresis_call(16, 8, 1, 200, 100, 8)]),
    ("canny", canny_call(16, 8, 1, 50.0, 150.0, 0),
     [canny_call(16, 8, 1, -1.0, 150.0, 0), canny_call(16, 8, 1, 50.0, NAN, 0), canny_call(16, 8, 1, 50.0, 150.0, 2)]),
    ("hough_lines", hough_call(16, 8, 1, 1.0, PI / 180, 5, 8, 0.0, PI, VOTES, COUNT),
     [hough_call(16, 8, 1, 0.0, PI / 180, 5, 8, 0.0, PI, VOTES, COUNT),
      hough_call(16, 8, 1, 1.0, NAN, 5, 8, 0.0, PI, VOTES, COUNT),
      hough_call(16, 8, 1, 1.0, PI / 180, 5, 0, 0.0, PI, VOTES, COUNT),
      hough_call(16, 8, 1, 1.0, PI / 180, 5, 8, 0.0, PI, VOTES, None)]),
    ("yuv_to_rgba8", yuv_decode_call(16, 8, 1, yuv_ref.NV12, yuv_ref.BT601, 0, 0),
     [yuv_decode_call(15, 8, 1, yuv_ref.NV12, yuv_ref.BT601, 0, 0), yuv_decode_call(16, 8, 1, 6, yuv_ref.BT601, 0, 0),
      yuv_decode_call(16, 8, 1, yuv_ref.NV12, yuv_ref.BT601, 12, 0)]),
    ("rgba8_to_yuv", yuv_encode_call(16, 8, 1, yuv_ref.NV12, yuv_ref.BT601, 0, 0),
     [yuv_encode_call(16, 7, 1, yuv_ref.NV12, yuv_ref.BT601, 0, 0), yuv_encode_call(16, 8, 1, yuv_ref.NV12, 3, 0, 0),
      yuv_encode_call(16, 8, 1, yuv_ref.NV12, yuv_ref.BT601, 0, 9)]),
]


def test_a_faulty_call_answers_in_the_same_order_at_every_entry_point(ctx, pkg):
    """Under MI355_INPUT_BGR a 1-byte frame has no form, and the YUV calls guess none: a valid call is
    MI355_ERR_UNSUPPORTED (-4), but a null buffer or a bad value is reported first (-1), and so are remap's missing
    second map and a labelling call's missing statistics.  Under RGBA input, resize's AREA with non-integer factors is
    -4."""
    lib, hd = ctx._lib, ctx._h
    buf_in, buf_out = np.zeros(96 * 64 * 4, np.uint8), np.zeros(96 * 64 * 4, np.uint8)
    i, o = buf_in.ctypes.data_as(_u8p), buf_out.ctypes.data_as(_u8p)
    prof = (ctypes.c_uint64 * 6)()
    no_map2 = [remap_call(bpp, 16, 8, 16, 8, 1, MAPX, None, FLOAT, interp, CONSTANT) for bpp in (1, 4)
               for interp in (NEAREST, LINEAR)]
    ran = 0
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for name, valid, bad in PRECEDENCE:
            for p in (None, prof):
                assert valid(lib, hd, i, o, p) == -4, name
                assert valid(lib, hd, None, o, p) == -1 and valid(lib, hd, i, None, p) == -1, name
                for n, call in enumerate(bad):
                    assert call(lib, hd, i, o, p) == -1, (name, n)
                    ran += 1
        for call in no_map2:
            assert call(lib, hd, i, o, None) == -1 and call(lib, hd, i, o, prof) == -1
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
    assert ran == 2 * (3 + 3 + 5 + 5 + 4 + 5) + 2 * (3 + 4 + 4 + 3 + 3 + 3 + 4 + 3 + 3)
    for call in no_map2:
        assert call(lib, hd, i, o, None) == -1
    fixed1, _ = convert_maps(MAPX, MAPY, NEAREST)
    assert remap_call(1, 16, 8, 16, 8, 1, fixed1, None, FIXED, LINEAR, CONSTANT)(lib, hd, i, o, None) == -1
    assert remap_call(1, 16, 8, 16, 8, 1, fixed1, None, FIXED, NEAREST, CONSTANT)(lib, hd, i, o, None) == 0
    assert resize_call(4, 64, 48, 5, 3, 1, AREA)(lib, hd, i, o, None) == -4
    assert resize_call(1, 64, 48, 5, 3, 1, AREA)(lib, hd, i, o, prof) == -4
    assert resize_call(4, 64, 48, 16, 12, 1, AREA)(lib, hd, i, o, None) == 0
    assert not buf_out[16 * 12 * 4:].any()                     # only the accepted calls wrote, and only their frames


def _bytes(a):
    """the bytes of an int32 / float32 output, as `out` of the calls below takes them"""
    return np.ascontiguousarray(a).view(np.uint8)


def _bgr_as_rgba(bgr):
    alpha = np.full(bgr.shape[:2], 255, np.uint8)
    return np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], alpha]))


@pytest.fixture(scope="module")
def steps(oracle, pkg):
    """[(name, input format is BGR, frame, call, reference[, [(array, reference)] of the call's further outputs])] in
    the order they run: the pooled input, staging, output, map and scratch buffers grow and shrink from one step to
    the next."""
    gauss_in = noise(5, 7, 4, 1)
    resize_in = noise(48, 64, 1, 2)
    float_in = noise(3, 5, 4, 3)
    fx, fy = cases.barrel_float_maps(5, 3, 96, 64)
    warp_in = noise(64, 96, 1, 4)
    shrink = [13.0, 2.0, 1.5, -1.0, 12.0, 6.25]               # inverse-mapped: 7 x 5 samples from all over the source
    adaptive_in = noise(5, 7, 1, 5)
    bgr_in = noise(17, 33, 3, 6)
    fixed_in = noise(8, 16, 4, 7)
    m1, m2 = convert_maps(*cases.barrel_float_maps(16, 8, 24, 12), LINEAR)
    persp_in = noise(8, 16, 4, 8)
    clahe_in = clahe_cases.uniform_noise(47, 61, 9)           # 4 x 3 tiles divide neither side: the padded geometry
    ccl_in = np.stack([ccl_cases.noise(48, 64, d) for d in (0.41, 0.59)])
    labels, count, stats, sums = ccl_ref(ccl_in, 8, 8)
    few_in = ccl_cases.noise(3, 5, 0.59)
    few_labels, few_count, _, _ = ccl_ref(few_in, 4)
    dist_in = np.stack([dist_cases.noise(17, 33, d) for d in (0.01, 0.5)])
    sq, dist, nearest = dist_ref(dist_in)
    edges_in = canny_cases.smooth(48, 64)
    hough_in = np.stack([hough_cases.drawn_lines(48, 64), hough_cases.noise(48, 64, 0.01)])
    tab_cos, tab_sin = pkg.hough_trig_table(64, 48, *hough_cases.DEFAULT)
    numrho = pkg.hough_shape(64, 48, *hough_cases.DEFAULT)[1]
    _, lines, votes, peaks = hough_ref.hough_ref(hough_in, tab_cos, tab_sin, numrho, 10, 16, *hough_cases.DEFAULT[:3])
    yuv_in = yuv_ref.pack(yuv_cases.noise_planes(18, 6, False, 10), yuv_ref.NV12, 32, 8, yuv_cases.padding(32 * 12, 10))
    rgba_in = noise(6, 18, 4, 11)

    def like(ref):
        return np.empty(ref.shape, ref.dtype), ref

    got_count, got_stats, got_sums, got_few = like(count), like(stats), like(sums), like(few_count)
    got_sq, got_near, got_votes, got_peaks = like(sq), like(nearest), like(votes), like(peaks)
    return [
        ("gauss", False, gauss_in, filter_call(2, 7, 5, 1, 5, 1.5), oracle.gauss_rgba(gauss_in, 5, 1.5)),
        ("resize_gray8", False, resize_in, resize_call(1, 64, 48, 5, 3, 1, LINEAR),
         resize_ref(resize_in, 5, 3, LINEAR)),
        ("remap_float", False, float_in, remap_call(4, 5, 3, 96, 64, 1, fx, fy, FLOAT, LINEAR, CONSTANT),
         remap_ref(float_in, fx, fy, FLOAT, LINEAR, CONSTANT, VALUE)),
        ("warp_gray8", False, warp_in, warp_call(1, 96, 64, 7, 5, 1, shrink, LINEAR | INVERSE_MAP, REPLICATE),
         warp_ref(warp_in, shrink, 7, 5, LINEAR | INVERSE_MAP, REPLICATE, VALUE)),
        ("adaptive", False, adaptive_in, adaptive_call(7, 5, 1, 255, BINARY, 3, 2.0),
         adaptive_ref(adaptive_in, 255, BINARY, 3, 2.0)),
        ("resize_bgr", True, bgr_in, resize_call(4, 33, 17, 16, 8, 1, LINEAR),
         resize_ref(_bgr_as_rgba(bgr_in), 16, 8, LINEAR)),
        ("remap_fixed", False, fixed_in, remap_call(4, 16, 8, 24, 12, 1, m1, m2, FIXED, LINEAR, REPLICATE),
         remap_ref(fixed_in, m1, m2, FIXED, LINEAR, REPLICATE, VALUE)),
        ("perspective", False, persp_in, perspective_call(4, 16, 8, 40, 24, 1, cases.KEYSTONE, LINEAR, CONSTANT),
         perspective_ref(persp_in, cases.KEYSTONE, 40, 24, LINEAR, CONSTANT, VALUE)),
        ("clahe", False, clahe_in, clahe_call(61, 47, 1, 2.0, 4, 3), clahe_ref(clahe_in, 2.0, 4, 3)),
        ("ccl_stats", False, ccl_in, ccl_call(64, 48, 2, 8, 8, got_count[0], got_stats[0], got_sums[0]), _bytes(labels),
         [got_count, got_stats, got_sums]),
        ("ccl", False, few_in, ccl_call(5, 3, 1, 4, 0, got_few[0]), _bytes(few_labels), [got_few]),
        ("dist_all", False, dist_in, dist_call(33, 17, 2, got_sq[0], got_near[0]), _bytes(dist), [got_sq, got_near]),
        ("dist", False, dist_in[1], dist_call(33, 17, 1), _bytes(dist[1])),
        ("hysteresis", False, edges_in, hysteresis_call(64, 48, 1, 60, 150, 8), hysteresis_ref(edges_in, 60, 150, 8)),
        ("canny", False, edges_in, canny_call(64, 48, 1, 50.0, 150.0, 0), canny_ref(edges_in, 50.0, 150.0, 0)),
        ("hough_lines", False, hough_in, hough_call(64, 48, 2, *hough_cases.DEFAULT[:2], 10, 16,
                                                    *hough_cases.DEFAULT[2:], got_votes[0], got_peaks[0]),
         _bytes(lines), [got_votes, got_peaks]),
        ("yuv_to_rgba8", False, yuv_in, yuv_decode_call(18, 6, 1, yuv_ref.NV12, yuv_ref.BT709, 32, 8),
         yuv_ref.decode(yuv_in, 18, 6, yuv_ref.NV12, yuv_ref.BT709, 32, 8)),
        ("rgba8_to_yuv", False, rgba_in, yuv_encode_call(18, 6, 1, yuv_ref.I420, yuv_ref.BT601, 20, 8),
         yuv_ref.encode(rgba_in, yuv_ref.I420, yuv_ref.BT601, 20, 8)),
    ]


def test_one_context_serves_every_entry_point_in_any_order(pkg, steps):
    """The eighteen calls, then the same eighteen backwards, on one fresh context: each result, every further output
    included, equals its CPU reference whether or not the call takes timestamps, and the six timestamps are ordered."""
    ran = 0
    with pkg.Context(0) as c:
        c.set_gauss_mode(pkg.GAUSS_EXACT)                      # bit-identical to the CPU path
        for name, bgr, frame, call, ref, *others in steps + steps[::-1]:
            c.set_input_format(pkg.INPUT_BGR if bgr else pkg.INPUT_RGBA)
            for prof in (None, (ctypes.c_uint64 * 6)()):
                out = np.full(ref.shape, 0xA5, np.uint8)
                rc = call(c._lib, c._h, frame.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), prof)
                assert rc == 0, (name, ran, rc)
                assert np.array_equal(out, ref), (name, ran, prof is not None)
                for k, (got, want) in enumerate(others[0] if others else ()):
                    assert np.array_equal(_bytes(got), _bytes(want)), (name, ran, prof is not None, k)
                if prof is not None:
                    t = list(prof)
                    assert all(t[k] <= t[k + 1] for k in range(5)) and t[5] > t[0], (name, t)
                ran += 1
    assert ran == 2 * 2 * 18
