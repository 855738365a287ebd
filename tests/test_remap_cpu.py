"""Remap and perspective warp (mi355_remap_* / mi355_perspective_matrix / mi355_warp_perspective_*): the parts that need
no GPU.

The header's constants and the binding's, the exported symbols, both pure host checks and the host matrix function
against tests/remap_ref.py on tables, the null context, and the reference itself: consistency with tests/warp_ref.py,
convert_maps, and that the special values of tests/remap_cases.py reach the cases the GPU test runs them for.  The GPU
behaviour is in test_gpu_remap.py.
"""
import ctypes
import inspect
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remap_cases as cases  # noqa: E402
from remap_ref import (FIXED, FLOAT, INT_MAX, INT_MIN, convert_maps, fixed_coords_of_maps, float_coords,  # noqa: E402
                       interior_passes, perspective_accepts, perspective_coords, perspective_inverse, perspective_ref,
                       perspective_w, remap_accepts, remap_ref)
from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, rotation, warp_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
ALL = [(i, b) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)]


def test_header_and_binding_constants_agree(pkg):
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}
    assert d["MI355_MAP_FIXED"] == pkg.MAP_FIXED == FIXED == 0
    assert d["MI355_MAP_FLOAT"] == pkg.MAP_FLOAT == FLOAT == 1
    assert "Nobody has compared it with an OpenCV" in text.split("cv::remap and cv::warpPerspective")[1]


SYMBOLS = ("mi355_remap_check", "mi355_remap_dev", "mi355_remap_batched", "mi355_perspective_matrix",
           "mi355_warp_perspective_check", "mi355_warp_perspective_dev", "mi355_warp_perspective_batched")


def test_library_exports_the_symbols_and_the_binding_has_the_methods(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert name in pkg.declared_symbols(), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    p = inspect.signature(pkg.Context.remap).parameters
    assert list(p) == ["self", "rgba", "map1", "map2", "dst_w", "dst_h", "map_kind", "interp", "border_mode",
                       "border_value", "profile"]
    assert p["map_kind"].default == pkg.MAP_FIXED and p["interp"].default == pkg.INTERP_LINEAR
    assert list(inspect.signature(pkg.Context.remap_gray8).parameters) == list(p)[:1] + ["y"] + list(p)[2:-1]
    assert list(inspect.signature(pkg.Context.remap_dev).parameters) == [
        "self", "d_in", "d_out", "bpp", "sw", "sh", "dw", "dh", "nframes", "d_map1", "d_map2", "map_kind", "interp",
        "border_mode", "border_value"]
    for name in ("warp_perspective", "warp_perspective_gray8", "warp_perspective_dev"):
        assert list(inspect.signature(getattr(pkg.Context, name)).parameters) == \
            list(inspect.signature(getattr(pkg.Context, name.replace("perspective", "affine"))).parameters), name


# ---- the pure host checks ---------------------------------------------------------------------------------------------
BAD_SIZES = [(0, 480, 320, 240, 1), (640, 0, 320, 240, 1), (640, 480, 0, 240, 1), (640, 480, 320, 0, 1),
             (-640, 480, 320, 240, 1), (640, 480, 320, -240, 1), (640, 480, 320, 240, 0), (640, 480, 320, 240, -2),
             (32766, 32766, 8, 8, 100)]
TOO_LARGE = [(32767, 8, 8, 8), (8, 32767, 8, 8), (8, 8, 32767, 8), (8, 8, 8, 32767), (40000, 40000, 40000, 40000)]
LARGEST = [(32766, 8, 8, 8), (8, 32766, 8, 8), (8, 8, 32766, 8), (8, 8, 8, 32766), (32766, 32766, 32766, 32766)]

REMAP_TABLE = (
    [((bpp, 640, 480, 320, 240, 2, kind, i, b), OK) for bpp in (1, 4) for kind in (FIXED, FLOAT) for i, b in ALL] +
    [((4, 1, 1, 1, 1, 1, FIXED, LINEAR, CONSTANT), OK)] +
    [((bpp, 640, 480, 320, 240, 1, FIXED, LINEAR, CONSTANT), BAD_ARG) for bpp in (0, 2, 3, -1, 5, 8)] +
    [((4, 640, 480, 320, 240, 1, kind, LINEAR, CONSTANT), BAD_ARG) for kind in (2, 3, -1, 16)] +
    [((4, 640, 480, 320, 240, 1, FLOAT, i, CONSTANT), BAD_ARG) for i in (2, 3, 4, -1, 16, 1 | INVERSE_MAP)] +
    [((4, 640, 480, 320, 240, 1, FLOAT, LINEAR, b), BAD_ARG) for b in (2, 3, 4, -1, 16)] +
    [((4,) + s + (FIXED, LINEAR, CONSTANT), BAD_ARG) for s in BAD_SIZES] +
    [((1,) + s + (1, FLOAT, NEAREST, REPLICATE), UNSUPPORTED) for s in TOO_LARGE] +
    [((1,) + s + (1, FLOAT, NEAREST, REPLICATE), OK) for s in LARGEST])


def _with(m, k, v):
    m = list(m)
    m[k] = v
    return m


PERSPECTIVE_TABLE = (
    [((bpp, 640, 480, 320, 240, 2, m, i | inv, b), OK) for bpp in (1, 4) for i, b in ALL for inv in (0, INVERSE_MAP)
     for m in (IDENTITY, cases.KEYSTONE, cases.W_ZERO)] +
    # the singular matrix is the all-zero map, not an error; neither is a matrix whose inverse overflows
    [((4, 640, 480, 320, 240, 1, [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 1.0, 1.0, 1.0], LINEAR, CONSTANT), OK),
     ((1, 640, 480, 320, 240, 1, [0.0] * 9, NEAREST, REPLICATE), OK),
     ((1, 640, 480, 320, 240, 1, [1e-160, 0.0, 0.0, 0.0, 1e-160, 0.0, 0.0, 0.0, 1e-160], LINEAR, CONSTANT), OK),
     ((1, 640, 480, 320, 240, 1, [1e300, 0.0, 1e300, 0.0, 1e300, 0.0, 0.0, 0.0, 1.0], LINEAR | INVERSE_MAP, CONSTANT), OK)] +
    [((4, 640, 480, 320, 240, 1, None, LINEAR, CONSTANT), BAD_ARG)] +
    [((bpp, 640, 480, 320, 240, 1, IDENTITY, LINEAR, CONSTANT), BAD_ARG) for bpp in (0, 2, 3, -1, 5, 8)] +
    [((4, 640, 480, 320, 240, 1, IDENTITY, f, CONSTANT), BAD_ARG)
     for f in (3, 2, 4, -1, 3 | INVERSE_MAP, 32, 1 | 32, 1 | 8, 1 | 64 | INVERSE_MAP)] +
    [((4, 640, 480, 320, 240, 1, IDENTITY, LINEAR, b), BAD_ARG) for b in (2, 3, 4, -1, 16)] +
    [((4,) + s + (IDENTITY, LINEAR, CONSTANT), BAD_ARG) for s in BAD_SIZES] +
    [((1, 640, 480, 320, 240, 1, _with(IDENTITY, k, v), LINEAR | inv, CONSTANT), BAD_ARG)
     for k in range(9) for v in (float("nan"), float("inf"), float("-inf")) for inv in (0, INVERSE_MAP)] +
    [((1,) + s + (1, IDENTITY, NEAREST, REPLICATE), UNSUPPORTED) for s in TOO_LARGE] +
    [((1,) + s + (1, IDENTITY, NEAREST, REPLICATE), OK) for s in LARGEST])


def test_remap_check_on_a_table(pkg):
    lib = pkg.load_library()
    assert len(REMAP_TABLE) > 50
    for args, want in REMAP_TABLE:
        assert lib.mi355_remap_check(*args) == want, (args, want)
        assert pkg.remap_check(*args) == want, (args, want)
        assert remap_accepts(*args) == want, (args, want)


def test_warp_perspective_check_on_a_table(pkg):
    lib = pkg.load_library()
    assert len(PERSPECTIVE_TABLE) > 120
    for args, want in PERSPECTIVE_TABLE:
        c = list(args)
        c[6] = None if args[6] is None else (ctypes.c_double * 9)(*args[6])
        assert lib.mi355_warp_perspective_check(*c) == want, (args, want)
        assert pkg.warp_perspective_check(*args) == want, (args, want)
        assert perspective_accepts(*args) == want, (args, want)


def test_a_null_context_pointer_or_matrix_is_a_bad_argument(pkg):
    lib = pkg.load_library()
    buf, out, maps = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 256)(), (ctypes.c_uint32 * 64)()
    u8, vp = ctypes.POINTER(ctypes.c_uint8), ctypes.c_void_p
    m = (ctypes.c_double * 9)(*IDENTITY)
    for bpp in (1, 4):
        for kind in (FIXED, FLOAT):
            assert lib.mi355_remap_dev(None, ctypes.cast(buf, vp), ctypes.cast(out, vp), bpp, 4, 4, 2, 2, 1,
                                       ctypes.cast(maps, vp), ctypes.cast(maps, vp), kind, LINEAR, CONSTANT, 0) == BAD_ARG
            assert lib.mi355_remap_batched(None, ctypes.cast(buf, u8), ctypes.cast(out, u8), bpp, 4, 4, 2, 2, 1,
                                           ctypes.cast(maps, vp), ctypes.cast(maps, vp), kind, NEAREST, REPLICATE, 0,
                                           None) == BAD_ARG
        assert lib.mi355_warp_perspective_dev(None, ctypes.cast(buf, vp), ctypes.cast(out, vp), bpp, 4, 4, 2, 2, 1, m,
                                              LINEAR, CONSTANT, 0) == BAD_ARG
        assert lib.mi355_warp_perspective_batched(None, ctypes.cast(buf, u8), ctypes.cast(out, u8), bpp, 4, 4, 2, 2, 1,
                                                  m, NEAREST, REPLICATE, 0, None) == BAD_ARG
    assert lib.mi355_perspective_matrix(None, LINEAR, m) == BAD_ARG
    assert lib.mi355_perspective_matrix(m, LINEAR, None) == BAD_ARG
    assert lib.mi355_perspective_matrix(m, 3, m) == BAD_ARG
    bad = (ctypes.c_double * 9)(*_with(IDENTITY, 7, float("nan")))
    assert lib.mi355_perspective_matrix(bad, LINEAR, m) == BAD_ARG


def test_perspective_matrix_is_bit_identical_to_the_reference(pkg):
    rng = np.random.default_rng(21)
    mats = [rng.standard_normal(9) * np.array([2.0, 2.0, 500.0, 2.0, 2.0, 500.0, 1e-3, 1e-3, 1.0]) for _ in range(200)]
    mats += [np.array(IDENTITY), np.array(cases.KEYSTONE), np.array(cases.W_ZERO), np.zeros(9),
             np.array([1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 1.0, 1.0, 1.0])]
    for m in mats:
        for flags in (LINEAR, NEAREST, LINEAR | INVERSE_MAP):
            got = pkg.perspective_matrix(m, flags).ravel()
            want = perspective_inverse(m, flags)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (m.tolist(), flags, got, want)
    assert np.array_equal(pkg.perspective_matrix([1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 1.0, 1.0, 1.0]), np.zeros((3, 3)))
    assert np.array_equal(pkg.perspective_matrix(np.arange(9.0).reshape(3, 3), INVERSE_MAP), np.arange(9.0).reshape(3, 3))
    # a forward shift inverts to the opposite shift
    assert np.array_equal(pkg.perspective_matrix(cases.embed([1.0, 0.0, 3.0, 0.0, 1.0, -2.0])),
                          np.array(cases.embed([1.0, 0.0, -3.0, 0.0, 1.0, 2.0])).reshape(3, 3))


# ---- the reference ----------------------------------------------------------------------------------------------------
def _images(sh, sw, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8))


AFFINE = [("rot7", lambda sw, sh: rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 7.0)),
          ("rot30", lambda sw, sh: rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)),
          ("shear", lambda sw, sh: [2.3, 0.4, -5.0, -0.2, 0.45, 3.0]),
          ("seam", lambda sw, sh: [1.0, 0.0, sw - 1.5, 0.0, 1.0, 0.0])]


def test_fixed_maps_of_an_affine_matrix_give_the_affine_reference():
    """FIXED maps that hold exactly the (sx, sy, fx, fy) warp_ref takes: remap_ref == warp_ref bit for bit."""
    n = 0
    for sw, sh, dw, dh in ((5, 3, 7, 2), (64, 48, 21, 16), (77, 41, 130, 19)):
        for img in _images(sh, sw, sw + dh):
            for name, make in AFFINE:
                m = make(sw, sh)
                for interp, border in ALL:
                    for inv in (0, INVERSE_MAP):
                        map1, map2 = cases.affine_fixed_maps(m, dw, dh, interp | inv)
                        want = warp_ref(img, m, dw, dh, interp | inv, border, 0x80FF407F)
                        got = remap_ref(img, map1, map2, FIXED, interp, border, 0x80FF407F)
                        assert np.array_equal(got, want), (sw, sh, dw, dh, name, interp, border, inv)
                        n += 1
    assert n == 3 * 2 * 4 * 4 * 2


def test_a_homography_with_last_row_001_and_integer_shifts_gives_the_affine_reference():
    for sw, sh, dw, dh in ((5, 3, 7, 2), (64, 48, 21, 16), (77, 41, 130, 19)):
        for img in _images(sh, sw, sw + dh + 1):
            for m6 in ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 3.0, 0.0, 1.0, -2.0], [1.0, 0.0, -40.0, 0.0, 1.0, 7.0]):
                for interp, border in ALL:
                    for inv in (0, INVERSE_MAP):
                        want = warp_ref(img, m6, dw, dh, interp | inv, border, 0x80FF407F)
                        got = perspective_ref(img, cases.embed(m6), dw, dh, interp | inv, border, 0x80FF407F)
                        assert np.array_equal(got, want), (sw, sh, dw, dh, m6, interp, border, inv)


def test_convert_maps_then_fixed_equals_float():
    for sw, sh, dw, dh in cases.SHAPES:
        img = _images(sh, sw, dw)[1]
        for name, mx, my in cases.remap_maps(sw, sh, dw, dh, FLOAT, LINEAR):
            for interp, border in ALL:
                map1, map2 = convert_maps(mx, my, interp)
                assert map1.dtype == np.int16 and map1.shape == (dh, dw, 2) and map2.dtype == np.uint16
                want = remap_ref(img, mx, my, FLOAT, interp, border, 0x80FF407F)
                assert np.array_equal(remap_ref(img, map1, map2, FIXED, interp, border, 0x80FF407F), want), (name, interp)
                rows = np.arange(0, dh, 3)
                assert np.array_equal(remap_ref(img, mx, my, FLOAT, interp, border, 0x80FF407F, rows=rows), want[rows])


def test_identity_maps_and_matrix_are_a_copy():
    for sh, sw in ((1, 1), (9, 13), (48, 64)):
        for img in _images(sh, sw, sh + sw):
            for interp, border in ALL:
                mx, my = cases.identity_float_maps(sw, sh)
                assert np.array_equal(remap_ref(img, mx, my, FLOAT, interp, border, 0x11223344), img)
                assert np.array_equal(remap_ref(img, *convert_maps(mx, my, interp), FIXED, interp, border, 0x11223344), img)
                assert np.array_equal(perspective_ref(img, IDENTITY, sw, sh, interp, border, 0x11223344), img)


def test_special_float_values_reach_what_they_should():
    sw, sh, dw, dh = 64, 48, 21, 16
    mx, my, at = cases.special_float_maps(sw, sh, dw, dh)
    assert set(at) == set(cases.SPECIAL_FLOATS)
    # the rounded coordinates themselves, before the split: from the FLOAT rule at S = 1
    for interp in (NEAREST, LINEAR):
        sx, sy, fx, fy = (v.ravel() for v in float_coords(mx, my, interp))
        lo, hi = -32768, 32767
        assert (sx[at["nan"]], sy[at["nan"]], fx[at["nan"]], fy[at["nan"]]) == (lo, lo, 0, 0)       # INT_MIN: fx = 0
        assert (sx[at["-inf"]], sy[at["-inf"]], fx[at["-inf"]]) == (lo, lo, 0)
        assert (sx[at["-3e9"]], sy[at["-3e9"]], fx[at["-3e9"]]) == (lo, lo, 0)
        top = 31 if interp == LINEAR else 0                                                          # INT_MAX & 31
        assert (sx[at["+inf"]], sy[at["+inf"]], fx[at["+inf"]], fy[at["+inf"]]) == (hi, hi, top, top)
        assert (sx[at["+3e9"]], sy[at["+3e9"]], fx[at["+3e9"]]) == (hi, hi, top)
        if interp == LINEAR:     # the seam: the left tap is the last column, the right tap lies outside
            assert (sx[at["seam"]], fx[at["seam"]], sy[at["seam"]], fy[at["seam"]]) == (sw - 1, 16, 0, 0)
        else:                    # 63.5 rounds half to even: the first column outside
            assert (sx[at["seam"]], sy[at["seam"]]) == (sw, 0)
    assert INT_MIN >> 5 < -32768 and INT_MAX >> 5 > 32767 and INT_MAX & 31 == 31 and INT_MIN & 31 == 0
    # 3e9 only overflows an int after the multiplication by 32 would have, and also before it
    assert np.float32(3.0e9) >= np.float32(2147483648.0)
    # the values show in the output: the seam pixel is the rounded mean of the last column and the border
    img = _images(sh, sw, 3)[0]
    out = remap_ref(img, mx, my, FLOAT, LINEAR, CONSTANT, 0x40).ravel()
    assert out[at["seam"]] == (int(img[0, sw - 1]) * 16 * 32 + 0x40 * 16 * 32 + 512) >> 10
    assert out[at["nan"]] == out[at["+inf"]] == 0x40
    rep = remap_ref(img, mx, my, FLOAT, LINEAR, REPLICATE, 0).ravel()
    assert rep[at["nan"]] == img[0, 0] and rep[at["+inf"]] == img[-1, -1] and rep[at["seam"]] == img[0, sw - 1]


def test_special_fixed_entries_reach_what_they_should():
    sw, sh, dw, dh = 64, 48, 21, 16
    map1, map2, at = cases.special_fixed_maps(sw, sh, dw, dh)
    assert set(at) == set(cases.SPECIAL_FIXED)
    sx, sy, fx, fy = (v.ravel() for v in fixed_coords_of_maps(map1, map2, LINEAR))
    assert (sx[at["-32768"]], sy[at["-32768"]]) == (-32768, -32768)
    assert (sx[at["32767"]], sy[at["32767"]], fx[at["32767"]], fy[at["32767"]]) == (32767, 32767, 9, 7)
    assert (sx[at["seam"]], fx[at["seam"]], sy[at["seam"]], fy[at["seam"]]) == (sw - 1, 16, 0, 0)
    assert map2.ravel()[at["map2>1023"]] > 1023 and (fx[at["map2>1023"]], fy[at["map2>1023"]]) == (5, 0)
    assert map2.ravel()[at["map2=65535"]] == 65535 and (fx[at["map2=65535"]], fy[at["map2=65535"]]) == (31, 31)
    img = _images(sh, sw, 4)[0]
    out = remap_ref(img, map1, map2, FIXED, LINEAR, CONSTANT, 0x40).ravel()
    assert out[at["-32768"]] == out[at["32767"]] == 0x40
    a = img.astype(np.int64)
    assert out[at["map2>1023"]] == (27 * 32 * a[0, 0] + 5 * 32 * a[0, 1] + 512) >> 10
    assert out[at["map2=65535"]] == (a[0, 0] + 31 * a[0, 1] + 31 * a[1, 0] + 961 * a[1, 1] + 512) >> 10
    # NEAREST ignores map2 altogether
    assert np.array_equal(remap_ref(img, map1, None, FIXED, NEAREST, CONSTANT, 0),
                          remap_ref(img, map1, map2, FIXED, NEAREST, CONSTANT, 0))


def test_special_homographies_reach_what_they_should():
    sw, sh, dw, dh = 64, 48, 21, 16
    w = perspective_w(cases.W_ZERO, dw, dh, LINEAR | INVERSE_MAP)
    assert np.all(w[:, 5] == 0.0) and np.count_nonzero(w == 0.0) == dh
    for interp in (NEAREST, LINEAR):
        sx, sy, fx, fy = perspective_coords(cases.W_ZERO, dw, dh, interp | INVERSE_MAP)
        assert np.all(sx[:, 5] == 0) and np.all(sy[:, 5] == 0) and np.all(fx[:, 5] == 0)     # s = 0: source (0, 0)
        assert np.all(sx[:, 4] == -4) and np.all(sx[:, 6] == 6)                              # x / (x - 5)
    w = perspective_w(cases.W_SIGN, dw, dh, LINEAR | INVERSE_MAP)
    assert np.all(w[:, :4] > 0) and np.all(w[:, 4:] < 0) and not np.any(w == 0)
    sx = perspective_coords(cases.W_SIGN, dw, dh, NEAREST | INVERSE_MAP)[0]
    assert sx[:, 3].min() == 30 and sx[:, 4].max() == -20
    # the singular matrix is the all-zero map: every pixel samples source (0, 0)
    sing = [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 1.0, 1.0, 1.0]
    assert all(np.all(v == 0) for v in perspective_coords(sing, dw, dh, LINEAR))
    img = _images(sh, sw, 5)[1]
    assert np.all(perspective_ref(img, sing, dw, dh, LINEAR, CONSTANT, 0x80FF407F) == img[0, 0])
    # a coordinate that overflows is clamped, not wrapped: far outside on the side it left the frame
    far = [1e300, 0.0, 1e300, 0.0, -1e300, -1e300, 0.0, 0.0, 1.0]
    sx, sy, fx, fy = perspective_coords(far, dw, dh, LINEAR | INVERSE_MAP)
    assert np.all(sx == 32767) and np.all(sy == -32768)


def test_the_gpu_cases_meet_both_paths():
    """Over the shapes of the GPU test every map kind and the homographies have row passes that are fully interior and
    row passes that are not (the counts the GPU test asserts)."""
    for interp in (NEAREST, LINEAR):
        for kind in (FIXED, FLOAT):
            k = n = 0
            for sw, sh, dw, dh in cases.SHAPES:
                for name, map1, map2 in cases.remap_maps(sw, sh, dw, dh, kind, interp):
                    a, b = interior_passes(fixed_coords_of_maps(map1, map2, interp) if kind == FIXED else
                                           float_coords(map1, map2, interp), sw, sh, interp, cases.TILE, cases.LANE_ROWS)
                    k, n = k + a, n + b
            assert 0 < k < n, (interp, kind, k, n)
    # the pass count of one shape by hand: 130 x 19 in tiles of 32 x 32 is 5 tiles across, 3 passes of 8 rows down
    c = float_coords(*cases.identity_float_maps(130, 19), NEAREST)
    assert interior_passes(c, 130, 19, NEAREST, (32, 32), 8) == (15, 15)
    assert interior_passes(c, 129, 19, NEAREST, (32, 32), 8) == (12, 15)
    assert interior_passes(c, 130, 17, NEAREST, (32, 32), 8) == (10, 15)
