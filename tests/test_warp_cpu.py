"""Affine warp (mi355_rotation_matrix / mi355_warp_affine_matrix / _check / _dev / _batched): the parts that need no GPU.

The header's constants and the binding's, the exported symbols, a C99 caller, the pure host check on a table, the host
matrix functions bit for bit, the null context, and the CPU reference tests/warp_ref.py against an independent scalar
loop written straight from the header's text and against properties that need no reference at all.  The GPU behaviour
is in test_gpu_warp.py.
"""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from warp_ref import (CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, accepts, inverse_of, rotation,  # noqa: E402
                      sample_rows, taps_inside, warp_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
F32 = np.float32
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    assert d["MI355_WARP_INVERSE_MAP"] == pkg.WARP_INVERSE_MAP == INVERSE_MAP == 16
    assert d["MI355_BORDER_CONSTANT"] == pkg.BORDER_CONSTANT == CONSTANT == 0
    assert d["MI355_BORDER_REPLICATE"] == pkg.BORDER_REPLICATE == REPLICATE == 1
    assert d["MI355_MAX_WARP_SIZE"] == pkg.MAX_WARP_SIZE == 32766
    assert d["MI355_INTERP_NEAREST"] == NEAREST and d["MI355_INTERP_LINEAR"] == LINEAR


SYMBOLS = ("mi355_rotation_matrix", "mi355_warp_affine_matrix", "mi355_warp_affine_check", "mi355_warp_affine_dev",
           "mi355_warp_affine_batched")


def test_library_exports_the_warp_symbols(pkg):
    lib = pkg.load_library()
    for name in SYMBOLS:
        assert name in pkg.declared_symbols(), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_c_program_using_the_warp_calls_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "warp_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    unsigned char in[64] = {0}, out[64];
    double m[6], inv[6];
    const double id[6] = {1, 0, 0, 0, 1, 0};
    const double far[6] = {1, 0, 2000000.0, 0, 1, 0};
    if (mi355_rotation_matrix(1920.0, 1080.0, 30.0, 1.0, m) != MI355_OK) return 1;
    if (mi355_rotation_matrix(0.0, 0.0, 30.0, 0.0, m) != MI355_ERR_BAD_ARG) return 2;
    if (mi355_rotation_matrix(0.0, 0.0, 30.0, 1.0, (double*)0) != MI355_ERR_BAD_ARG) return 3;
    if (mi355_rotation_matrix(0.0, 0.0, 90.0, 1.0, m) != MI355_OK) return 4;
    if (mi355_warp_affine_matrix(m, MI355_INTERP_LINEAR, inv) != MI355_OK) return 5;
    if (mi355_warp_affine_matrix(id, MI355_INTERP_NEAREST | MI355_WARP_INVERSE_MAP, inv) != MI355_OK || inv[0] != 1.0 ||
        inv[2] != 0.0)
        return 6;
    if (mi355_warp_affine_matrix(id, MI355_INTERP_AREA, inv) != MI355_ERR_BAD_ARG) return 7;
    if (mi355_warp_affine_check(4, 3840, 2160, 3840, 2160, 64, m, MI355_INTERP_LINEAR, MI355_BORDER_CONSTANT) != MI355_OK)
        return 8;
    if (mi355_warp_affine_check(1, 640, 480, 320, 240, 1, id, MI355_INTERP_NEAREST | MI355_WARP_INVERSE_MAP,
                                MI355_BORDER_REPLICATE) != MI355_OK)
        return 9;
    if (mi355_warp_affine_check(4, 640, 480, MI355_MAX_WARP_SIZE + 1, 240, 1, id, MI355_INTERP_LINEAR,
                                MI355_BORDER_CONSTANT) != MI355_ERR_UNSUPPORTED)
        return 10;
    if (mi355_warp_affine_check(4, 640, 480, 320, 240, 1, far, MI355_INTERP_LINEAR, MI355_BORDER_CONSTANT) !=
        MI355_ERR_UNSUPPORTED)
        return 11;
    if (mi355_warp_affine_check(4, 640, 480, 320, 240, 1, id, MI355_INTERP_AREA, MI355_BORDER_CONSTANT) !=
        MI355_ERR_BAD_ARG)
        return 12;
    if (mi355_warp_affine_check(4, 640, 480, 320, 240, 1, (const double*)0, MI355_INTERP_LINEAR,
                                MI355_BORDER_CONSTANT) != MI355_ERR_BAD_ARG)
        return 13;
    if (mi355_warp_affine_dev((mi355_ctx*)0, in, out, 4, 2, 2, 2, 2, 1, id, MI355_INTERP_LINEAR, MI355_BORDER_CONSTANT,
                              0u) != MI355_ERR_BAD_ARG)
        return 14;
    if (mi355_warp_affine_batched((mi355_ctx*)0, in, out, 1, 4, 4, 2, 2, 1, id, MI355_INTERP_NEAREST,
                                  MI355_BORDER_REPLICATE, 0x80FF407Fu, (uint64_t*)0) != MI355_ERR_BAD_ARG)
        return 15;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "warp_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


# ---- mi355_warp_affine_check -----------------------------------------------------------------------------------------
ROT30 = rotation(320.0, 240.0, 30.0)
T_AT = float((1 << 20) - 100)                    # with dst_w = 101: 1 * 100 + t == 2^20 exactly
T_UNDER = float(np.nextafter(T_AT, 0.0))


def _with(m, k, v):
    m = list(m)
    m[k] = v
    return m


CHECK_TABLE = (
    # every good combination of bpp x interp x border x inverse flag
    [((bpp, 640, 480, 320, 240, 2, m, i | inv, b), OK) for bpp in (1, 4) for i in (NEAREST, LINEAR)
     for b in (CONSTANT, REPLICATE) for inv in (0, INVERSE_MAP) for m in (IDENTITY, ROT30)] +
    [((4, 1, 1, 1, 1, 1, IDENTITY, LINEAR, CONSTANT), OK)] +
    # the singular matrix is the all-zero map, not an error
    [((4, 640, 480, 320, 240, 1, [1.0, 2.0, 3.0, 2.0, 4.0, 5.0], LINEAR, CONSTANT), OK),
     ((1, 640, 480, 320, 240, 1, [0.0] * 6, NEAREST, REPLICATE), OK)] +
    # BAD_ARG: the matrix pointer, bytes per pixel, flags (AREA, cubic, stray bits), border mode
    [((4, 640, 480, 320, 240, 1, None, LINEAR, CONSTANT), BAD_ARG)] +
    [((bpp, 640, 480, 320, 240, 1, IDENTITY, LINEAR, CONSTANT), BAD_ARG) for bpp in (0, 2, 3, -1, 5, 8)] +
    [((4, 640, 480, 320, 240, 1, IDENTITY, f, CONSTANT), BAD_ARG)
     for f in (3, 2, 4, -1, 3 | INVERSE_MAP, 2 | INVERSE_MAP, 32, 1 | 32, 1 | 8, 1 | 64 | INVERSE_MAP)] +
    [((4, 640, 480, 320, 240, 1, IDENTITY, LINEAR, b), BAD_ARG) for b in (2, 3, 4, 5, -1, 16)] +
    # BAD_ARG: sizes and the frame count
    [((4,) + s + (IDENTITY, LINEAR, CONSTANT), BAD_ARG)
     for s in ((0, 480, 320, 240, 1), (640, 0, 320, 240, 1), (640, 480, 0, 240, 1), (640, 480, 320, 0, 1),
               (-640, 480, 320, 240, 1), (640, -1, 320, 240, 1), (640, 480, -320, 240, 1), (640, 480, 320, -240, 1),
               (640, 480, 320, 240, 0), (640, 480, 320, 240, -2), (32766, 32766, 8, 8, 100))] +
    # BAD_ARG: a non-finite entry, in every position, inverse-mapped or not
    [((1, 640, 480, 320, 240, 1, _with(IDENTITY, k, v), LINEAR | inv, CONSTANT), BAD_ARG)
     for k in range(6) for v in (float("nan"), float("inf"), float("-inf")) for inv in (0, INVERSE_MAP)] +
    # UNSUPPORTED: a width or height above 32766, in either shape
    [((bpp, 32766, 32766, 32766, 32766, 1, IDENTITY, LINEAR, CONSTANT), OK) for bpp in (1, 4)] +
    [((1,) + s + (1, IDENTITY, NEAREST, REPLICATE), UNSUPPORTED)
     for s in ((32767, 8, 8, 8), (8, 32767, 8, 8), (8, 8, 32767, 8), (8, 8, 8, 32767), (40000, 40000, 40000, 40000))] +
    [((1,) + s + (1, IDENTITY, NEAREST, REPLICATE), OK)
     for s in ((32766, 8, 8, 8), (8, 32766, 8, 8), (8, 8, 32766, 8), (8, 8, 8, 32766))] +
    # UNSUPPORTED: |i0| (dst_w - 1) + |i1| (dst_h - 1) + |i2| at 2^20, and the same for the second row; just under is fine
    [((4, 64, 48, 101, 7, 1, [1.0, 0.0, T_UNDER, 0.0, 1.0, 0.0], LINEAR | INVERSE_MAP, CONSTANT), OK),
     ((4, 64, 48, 101, 7, 1, [1.0, 0.0, T_AT, 0.0, 1.0, 0.0], LINEAR | INVERSE_MAP, CONSTANT), UNSUPPORTED),
     ((4, 64, 48, 101, 7, 1, [1.0, 0.0, -T_UNDER, 0.0, 1.0, 0.0], NEAREST | INVERSE_MAP, REPLICATE), OK),
     ((4, 64, 48, 101, 7, 1, [1.0, 0.0, -T_AT, 0.0, 1.0, 0.0], NEAREST | INVERSE_MAP, REPLICATE), UNSUPPORTED),
     ((1, 64, 48, 7, 101, 1, [1.0, 0.0, 0.0, 0.0, 1.0, T_UNDER], LINEAR | INVERSE_MAP, CONSTANT), OK),
     ((1, 64, 48, 7, 101, 1, [1.0, 0.0, 0.0, 0.0, 1.0, T_AT], LINEAR | INVERSE_MAP, CONSTANT), UNSUPPORTED),
     ((1, 64, 48, 101, 7, 1, [0.0, 0.0, 0.0, 1.0, 0.0, T_UNDER], LINEAR | INVERSE_MAP, CONSTANT), OK),
     ((1, 64, 48, 101, 7, 1, [0.0, 0.0, 0.0, 1.0, 0.0, T_AT], LINEAR | INVERSE_MAP, CONSTANT), UNSUPPORTED),
     # forward: the bound is on the inverse, not on m
     ((4, 64, 48, 101, 7, 1, [1.0, 0.0, T_UNDER, 0.0, 1.0, 0.0], LINEAR, CONSTANT), OK),
     ((4, 64, 48, 101, 7, 1, [1.0, 0.0, T_AT, 0.0, 1.0, 0.0], LINEAR, CONSTANT), UNSUPPORTED),
     ((4, 64, 48, 101, 7, 1, [1e-4, 0.0, 0.0, 0.0, 1e-4, 0.0], LINEAR, CONSTANT), OK),          # 1e4 * 100 < 2^20
     ((4, 64, 48, 101, 7, 1, [1e-5, 0.0, 0.0, 0.0, 1e-5, 0.0], LINEAR, CONSTANT), UNSUPPORTED),  # 1e5 * 100 > 2^20
     ((4, 64, 48, 101, 7, 1, [1e-160, 0.0, 0.0, 0.0, 1e-160, 0.0], LINEAR, CONSTANT), UNSUPPORTED)]  # 1 / D overflows
)


def test_warp_affine_check_on_a_table(pkg):
    lib = pkg.load_library()
    assert len(CHECK_TABLE) > 120
    for args, want in CHECK_TABLE:
        c = list(args)
        c[6] = None if args[6] is None else (ctypes.c_double * 6)(*args[6])
        assert lib.mi355_warp_affine_check(*c) == want, (args, want)
        assert pkg.warp_affine_check(*args) == want, (args, want)
        assert accepts(*args) == want, (args, want)


def test_a_null_context_or_matrix_is_a_bad_argument(pkg):
    lib = pkg.load_library()
    buf, out = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 256)()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    m = (ctypes.c_double * 6)(*IDENTITY)
    for bpp in (1, 4):
        for flags in (NEAREST, LINEAR, LINEAR | INVERSE_MAP):
            assert lib.mi355_warp_affine_dev(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p),
                                             bpp, 4, 4, 2, 2, 1, m, flags, CONSTANT, 0) == BAD_ARG
            assert lib.mi355_warp_affine_batched(None, ctypes.cast(buf, u8), ctypes.cast(out, u8), bpp, 4, 4, 2, 2, 1, m,
                                                 flags, REPLICATE, 0, None) == BAD_ARG
    assert lib.mi355_warp_affine_matrix(None, LINEAR, m) == BAD_ARG
    assert lib.mi355_warp_affine_matrix(m, LINEAR, None) == BAD_ARG
    assert lib.mi355_warp_affine_matrix(m, 3, m) == BAD_ARG


def test_binding_methods(pkg):
    p = inspect.signature(pkg.Context.warp_affine).parameters
    assert list(p) == ["self", "rgba", "m", "dst_w", "dst_h", "flags", "border_mode", "border_value", "profile"]
    assert p["flags"].default == pkg.INTERP_LINEAR and p["border_mode"].default == pkg.BORDER_CONSTANT
    assert p["border_value"].default == 0 and p["profile"].default is False
    assert list(inspect.signature(pkg.Context.warp_affine_gray8).parameters) == [
        "self", "y", "m", "dst_w", "dst_h", "flags", "border_mode", "border_value"]
    assert list(inspect.signature(pkg.Context.warp_affine_dev).parameters) == [
        "self", "d_in", "d_out", "bpp", "sw", "sh", "dw", "dh", "nframes", "m", "flags", "border_mode", "border_value"]


# ---- the host matrix functions ----------------------------------------------------------------------------------------
def _seeded_matrices(n, seed=20):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = rng.standard_normal(6) * np.array([2.0, 2.0, 500.0, 2.0, 2.0, 500.0])
        if k % 5 == 0:
            m = np.array(rotation(rng.uniform(-4096, 4096), rng.uniform(-4096, 4096), rng.uniform(-360, 360),
                                  rng.uniform(0.05, 4.0)))
        out.append(m)
    return out


def test_warp_affine_matrix_is_bit_identical_to_the_reference(pkg):
    mats = _seeded_matrices(200) + [np.array([1.0, 2.0, 3.0, 2.0, 4.0, 5.0]), np.zeros(6), np.array(IDENTITY)]
    for m in mats:
        for flags in (LINEAR, NEAREST, LINEAR | INVERSE_MAP):
            got = pkg.warp_affine_matrix(m, flags).ravel()
            want = inverse_of(m, flags)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (m.tolist(), flags, got, want)
    assert np.array_equal(pkg.warp_affine_matrix([1.0, 2.0, 3.0, 2.0, 4.0, 5.0], LINEAR), np.zeros((2, 3)))
    assert np.array_equal(pkg.warp_affine_matrix(np.arange(6.0).reshape(2, 3), INVERSE_MAP),
                          np.arange(6.0).reshape(2, 3))


def test_rotation_matrix_equals_the_formula(pkg):
    rng = np.random.default_rng(7)
    cases = [(0.0, 0.0, 0.0, 1.0), (1920.0, 1080.0, 30.0, 1.0), (4096.0, -4096.0, 359.0, 4.0), (-4096.0, 4096.0, -90.0, 4.0)]
    cases += [(rng.uniform(-4096, 4096), rng.uniform(-4096, 4096), rng.uniform(-720, 720), rng.uniform(0.01, 4.0))
              for _ in range(300)]
    for cx, cy, ang, sc in cases:
        got = pkg.rotation_matrix(cx, cy, ang, sc).ravel()
        assert np.abs(got - np.array(rotation(cx, cy, ang, sc))).max() <= 1e-9, (cx, cy, ang, sc)
    assert np.array_equal(pkg.rotation_matrix(5.0, 7.0, 0.0, 1.0), np.array(IDENTITY).reshape(2, 3))
    for bad in ((float("nan"), 0, 0, 1), (0, float("inf"), 0, 1), (0, 0, float("nan"), 1), (0, 0, 0, float("inf")),
                (0, 0, 30, 0.0), (0, 0, 30, -0.0)):
        with pytest.raises(pkg.Mi355Error) as e:
            pkg.rotation_matrix(*bad)
        assert e.value.code == BAD_ARG, bad


# ---- the reference ----------------------------------------------------------------------------------------------------
def _rint(v):
    """round half to even of a Python float (fp64), as an int"""
    return int(round(v))


def scalar_warp(img, m, dw, dh, flags, border, value):
    """The header's text, one pixel and one channel at a time, in Python floats (fp64) and ints."""
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    chans = img.reshape(sh, sw, -1)
    nc = chans.shape[2]
    m = [float(v) for v in np.asarray(m, np.float64).ravel()]
    if flags & 16:
        i = m
    else:
        D = m[0] * m[4] - m[1] * m[3]
        D = 1.0 / D if D != 0 else 0.0
        A11, A22 = m[4] * D, m[0] * D
        i = [A11, m[1] * (-D), 0.0, m[3] * (-D), A22, 0.0]
        i[2] = -i[0] * m[2] - i[1] * m[5]
        i[5] = -i[3] * m[2] - i[4] * m[5]
    linear = (flags & ~16) == 1
    rd = 16 if linear else 512

    def tap(u, v, c):
        if 0 <= u < sw and 0 <= v < sh:
            return int(chans[v, u, c])
        if border == CONSTANT:
            return (value >> (8 * c)) & 0xFF
        return int(chans[min(max(v, 0), sh - 1), min(max(u, 0), sw - 1), c])

    out = np.zeros((dh, dw, nc), np.uint8)
    for y in range(dh):
        X0 = _rint((i[1] * y + i[2]) * 1024.0) + rd
        Y0 = _rint((i[4] * y + i[5]) * 1024.0) + rd
        for x in range(dw):
            X = X0 + _rint((i[0] * x) * 1024.0)
            Y = Y0 + _rint((i[3] * x) * 1024.0)
            for c in range(nc):
                if not linear:
                    out[y, x, c] = tap(X >> 10, Y >> 10, c)
                    continue
                XX, YY = X >> 5, Y >> 5
                sx, fx, sy, fy = XX >> 5, XX & 31, YY >> 5, YY & 31
                v = ((32 - fx) * (32 - fy) * tap(sx, sy, c) + fx * (32 - fy) * tap(sx + 1, sy, c) +
                     (32 - fx) * fy * tap(sx, sy + 1, c) + fx * fy * tap(sx + 1, sy + 1, c) + 512) >> 10
                assert 0 <= v <= 255
                out[y, x, c] = v
    return out.reshape((dh, dw) + img.shape[2:])


def _images(sh, sw, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8),
            rng.integers(0, 2, (sh, sw, 4), dtype=np.uint8) * 255)


SMALL = [(1, 1, 1, 1), (5, 3, 7, 2), (13, 9, 7, 5), (21, 16, 25, 13)]


def _small_matrices(sw, sh, dw, dh):
    return [(IDENTITY, INVERSE_MAP), ([1.0, 0.0, 3.0, 0.0, 1.0, -2.0], 0), ([1.0, 0.0, 0.5, 0.0, 1.0, 0.25], INVERSE_MAP),
            (rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0), 0), (rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 7.0), INVERSE_MAP),
            ([2.3, 0.4, -5.0, -0.2, 0.45, 3.0], 0), ([2.3, 0.4, -5.0, -0.2, 0.45, 3.0], INVERSE_MAP),
            ([1.0, 2.0, 3.0, 2.0, 4.0, 5.0], 0), ([1.0, 0.0, 1000.0, 0.0, 1.0, 1000.0], INVERSE_MAP),
            ([-0.7, 0.1, sw + 0.3, 0.05, -1.3, sh - 0.6], INVERSE_MAP)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda p: "%dx%d-%dx%d" % p)
def test_reference_equals_the_scalar_loop(shape):
    sw, sh, dw, dh = shape
    for m, inv in _small_matrices(sw, sh, dw, dh):
        for img in _images(sh, sw, sw * 7 + dh):
            for interp in (NEAREST, LINEAR):
                for border, value in ((CONSTANT, 0x80FF407F), (REPLICATE, 0)):
                    want = scalar_warp(img, m, dw, dh, interp | inv, border, value)
                    got = warp_ref(img, m, dw, dh, interp | inv, border, value)
                    assert got.shape == want.shape and np.array_equal(got, want), (shape, m, inv, interp, border)
                    rows = sample_rows(dh, 3)
                    assert np.array_equal(warp_ref(img, m, dw, dh, interp | inv, border, value, rows=rows), want[rows])


# ---- properties that need no reference --------------------------------------------------------------------------------
ALL = [(i, b) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)]


def test_identity_is_a_copy():
    for sh, sw in ((1, 1), (9, 13), (48, 64), (31, 257)):
        for img in _images(sh, sw, sh + sw):
            for interp, border in ALL:
                for inv in (0, INVERSE_MAP):
                    assert np.array_equal(warp_ref(img, IDENTITY, sw, sh, interp | inv, border, 0x11223344), img)


def test_an_integer_shift_is_the_shifted_frame_with_border_pixels():
    sh, sw, tx, ty = 11, 17, 3, -2
    for img in _images(sh, sw, 3):
        for interp, border in ALL:
            value = 0x80FF407F
            bp = np.array([0x7F, 0x40, 0xFF, 0x80], np.uint8)
            want = np.empty_like(img)
            for y in range(sh):
                for x in range(sw):
                    u, v = x + tx, y + ty
                    if 0 <= u < sw and 0 <= v < sh:
                        want[y, x] = img[v, u]
                    elif border == CONSTANT:
                        want[y, x] = bp if img.ndim == 3 else bp[0]
                    else:
                        want[y, x] = img[min(max(v, 0), sh - 1), min(max(u, 0), sw - 1)]
            m = [1.0, 0.0, float(tx), 0.0, 1.0, float(ty)]
            assert np.array_equal(warp_ref(img, m, sw, sh, interp | INVERSE_MAP, border, value), want)
            fwd = [1.0, 0.0, float(-tx), 0.0, 1.0, float(-ty)]      # the forward matrix of the same map
            assert np.array_equal(warp_ref(img, fwd, sw, sh, interp, border, value), want)


def test_flip_and_quarter_turns():
    for sh, sw in ((9, 13), (16, 16), (5, 40)):
        for img in _images(sh, sw, sh * sw):
            for interp, border in ALL:
                f = interp | INVERSE_MAP
                flip = [-1.0, 0.0, float(sw - 1), 0.0, 1.0, 0.0]
                assert np.array_equal(warp_ref(img, flip, sw, sh, f, border, 9), np.fliplr(img))
                quarter = [0.0, -1.0, float(sw - 1), 1.0, 0.0, 0.0]      # out[y][x] = img[x][sw - 1 - y]
                assert np.array_equal(warp_ref(img, quarter, sh, sw, f, border, 9), np.rot90(img))
                half = [-1.0, 0.0, float(sw - 1), 0.0, -1.0, float(sh - 1)]
                assert np.array_equal(warp_ref(img, half, sw, sh, f, border, 9), np.rot90(img, 2))


def test_half_pixel_shift_is_the_rounded_mean():
    for img in _images(7, 12, 5):
        a = img.astype(np.int64)
        b = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)                # REPLICATE: the last column meets itself
        got = warp_ref(img, [1.0, 0.0, 0.5, 0.0, 1.0, 0.0], 12, 7, LINEAR | INVERSE_MAP, REPLICATE, 0)
        assert np.array_equal(got, ((a + b + 1) >> 1).astype(np.uint8))
        b0 = np.concatenate([a[:, 1:], np.zeros_like(a[:, -1:])], axis=1)  # CONSTANT 0 beyond the last column
        got = warp_ref(img, [1.0, 0.0, 0.5, 0.0, 1.0, 0.0], 12, 7, LINEAR | INVERSE_MAP, CONSTANT, 0)
        assert np.array_equal(got, ((a + b0 + 1) >> 1).astype(np.uint8))


def test_a_frame_translated_wholly_outside():
    for img in _images(7, 12, 6):
        for interp in (NEAREST, LINEAR):
            m = [1.0, 0.0, 10000.0, 0.0, 1.0, 10000.0]
            got = warp_ref(img, m, 9, 5, interp | INVERSE_MAP, CONSTANT, 0x80FF407F)
            want = np.array([0x7F, 0x40, 0xFF, 0x80], np.uint8)
            assert np.all(got == (want if img.ndim == 3 else want[0]))
            got = warp_ref(img, m, 9, 5, interp | INVERSE_MAP, REPLICATE, 0x80FF407F)
            assert np.all(got == img[-1, -1])
            got = warp_ref(img, [1.0, 0.0, -10000.0, 0.0, 1.0, 3.0], 9, 1, interp | INVERSE_MAP, REPLICATE, 0)
            assert np.all(got == img[3, 0])
            assert not taps_inside(m, 12, 7, 9, 5, interp | INVERSE_MAP, 0, 9, 0, 5)
    assert taps_inside(IDENTITY, 12, 7, 11, 6, LINEAR | INVERSE_MAP, 0, 11, 0, 6)
    assert not taps_inside(IDENTITY, 12, 7, 12, 7, LINEAR | INVERSE_MAP, 0, 12, 0, 7)
    assert taps_inside(IDENTITY, 12, 7, 12, 7, NEAREST | INVERSE_MAP, 0, 12, 0, 7)


def test_the_15_bit_weight_table_is_the_5_bit_product():
    """OpenCV builds its bilinear table in fp32: (1 - f/32, f/32) per axis, the outer product, times 32768, rounded to
    short.  Every entry is 32 * wx * wy exactly and each group of four sums to 32768, so (sum + 16384) >> 15 equals the
    header's (sum + 512) >> 10 with 5-bit weights."""
    n = 0
    for fy in range(32):
        ty = (F32(1) - F32(fy) * F32(1.0 / 32), F32(fy) * F32(1.0 / 32))
        for fx in range(32):
            tx = (F32(1) - F32(fx) * F32(1.0 / 32), F32(fx) * F32(1.0 / 32))
            entries = [int(np.rint(F32(F32(ty[k1] * tx[k2]) * F32(32768)))) for k1 in range(2) for k2 in range(2)]
            want = [32 * wy * wx for wy in (32 - fy, fy) for wx in (32 - fx, fx)]
            assert entries == want and sum(entries) == 32768, (fx, fy, entries)
            n += 1
    assert n == 1024
    rng = np.random.default_rng(1)
    for _ in range(200):
        taps = rng.integers(0, 256, 4)
        fx, fy = int(rng.integers(0, 32)), int(rng.integers(0, 32))
        w = [wy * wx for wy in (32 - fy, fy) for wx in (32 - fx, fx)]
        s = int(sum(int(t) * k for t, k in zip(taps, w)))
        assert (32 * s + 16384) >> 15 == (s + 512) >> 10 and 0 <= (s + 512) >> 10 <= 255
