"""GPU suite (-m gpu): what the six batched host-buffer entry points share, through raw library calls.

mi355_filter_batched, mi355_resize_batched, mi355_warp_affine_batched, mi355_remap_batched,
mi355_warp_perspective_batched and mi355_adaptive_threshold_gray8_batched stage their frames the same way: pointer
checks, the call's value checks, the input-format rule, then one round trip through the context's pooled buffers.  Two
things no per-feature test looks at are pinned here: the order in which a call with several faults answers, and that one
context's pooled buffers serve every entry point in any order, growing and shrinking, with and without timestamps.
Every shape is tiny (none above 96 x 64).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remap_cases as cases  # noqa: E402
from box_ref import BINARY, adaptive_ref  # noqa: E402
from remap_ref import FIXED, FLOAT, convert_maps, perspective_ref, remap_ref  # noqa: E402
from resize_ref import resize_ref  # noqa: E402
from test_gpu_median import noise  # noqa: E402
from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, warp_ref  # noqa: E402

pytestmark = pytest.mark.gpu

AREA = 3
NAN = float("nan")
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


IDENT6 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
IDENT9 = cases.embed(IDENT6)
MAPX, MAPY = cases.identity_float_maps(16, 8)
# every row: (entry point, a valid call on 1-byte frames, the same call with one bad value each)
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
]


def test_a_faulty_call_answers_in_the_same_order_at_every_entry_point(ctx, pkg):
    """Under MI355_INPUT_BGR a 1-byte frame has no form: a valid call is MI355_ERR_UNSUPPORTED (-4), but a null buffer
    or a bad value is reported first (-1), and so is remap's missing second map.  Under RGBA input, resize's AREA with
    non-integer factors is -4."""
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
    assert ran == 2 * (3 + 3 + 5 + 5 + 4 + 5)
    for call in no_map2:
        assert call(lib, hd, i, o, None) == -1
    fixed1, _ = convert_maps(MAPX, MAPY, NEAREST)
    assert remap_call(1, 16, 8, 16, 8, 1, fixed1, None, FIXED, LINEAR, CONSTANT)(lib, hd, i, o, None) == -1
    assert remap_call(1, 16, 8, 16, 8, 1, fixed1, None, FIXED, NEAREST, CONSTANT)(lib, hd, i, o, None) == 0
    assert resize_call(4, 64, 48, 5, 3, 1, AREA)(lib, hd, i, o, None) == -4
    assert resize_call(1, 64, 48, 5, 3, 1, AREA)(lib, hd, i, o, prof) == -4
    assert resize_call(4, 64, 48, 16, 12, 1, AREA)(lib, hd, i, o, None) == 0
    assert not buf_out[16 * 12 * 4:].any()                     # only the accepted calls wrote, and only their frames


def _bgr_as_rgba(bgr):
    alpha = np.full(bgr.shape[:2], 255, np.uint8)
    return np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], alpha]))


@pytest.fixture(scope="module")
def steps(oracle):
    """[(name, input format is BGR, frame, call, reference)] in the order they run: the pooled input, staging, output
    and map buffers grow and shrink from one step to the next."""
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
    ]


def test_one_context_serves_every_entry_point_in_any_order(pkg, steps):
    """The eight calls, then the same eight backwards, on one fresh context: each result equals its CPU reference
    whether or not the call takes timestamps, and the six timestamps are ordered."""
    ran = 0
    with pkg.Context(0) as c:
        c.set_gauss_mode(pkg.GAUSS_EXACT)                      # bit-identical to the CPU path
        for name, bgr, frame, call, ref in steps + steps[::-1]:
            c.set_input_format(pkg.INPUT_BGR if bgr else pkg.INPUT_RGBA)
            for prof in (None, (ctypes.c_uint64 * 6)()):
                out = np.full(ref.shape, 0xA5, np.uint8)
                rc = call(c._lib, c._h, frame.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), prof)
                assert rc == 0, (name, ran, rc)
                assert np.array_equal(out, ref), (name, ran, prof is not None)
                if prof is not None:
                    t = list(prof)
                    assert all(t[k] <= t[k + 1] for k in range(5)) and t[5] > t[0], (name, t)
                ran += 1
    assert ran == 2 * 2 * 8
