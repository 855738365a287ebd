"""Resize (mi355_resize_check / _dev / _batched): the parts that need no GPU.

The header's constants and the binding's, the exported symbols, a C99 caller, the pure host check on a table, the null
context, and the CPU reference tests/resize_ref.py against an independent scalar loop written straight from the
header's text, a hand-worked vector and the properties the arithmetic must have.  The GPU behaviour is in
test_gpu_resize.py.
"""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resize_ref import (AREA, LINEAR, NEAREST, area_byte, area_factors, linear_cols, linear_rows,  # noqa: E402
                        resize_ref, sample_rows, scale_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
F32 = np.float32

# (src w, src h, dst w, dst h): the GPU suite's shapes that are small enough for the scalar loop, and a few more
SMALL_PAIRS = [(1, 1, 1, 1), (1, 1, 5, 3), (5, 3, 1, 1), (2, 2, 17, 3), (7, 5, 13, 9), (13, 9, 7, 5), (64, 48, 21, 16),
               (21, 16, 64, 48), (10, 9, 25, 3), (3, 50, 5, 117), (12, 8, 6, 4), (14, 10, 7, 5), (48, 32, 3, 2),
               (18, 16, 6, 4), (9, 9, 9, 9)]
# size pairs of the GPU suite and of tools/resize_rate.py, for the column / row tables alone
ALL_PAIRS = SMALL_PAIRS + [(2, 2, 257, 3), (100, 90, 250, 30), (3, 1000, 5, 2333), (75, 75, 240, 240),
                           (1023, 819, 640, 512), (640, 427, 1023, 683), (3840, 2160, 1920, 1080),
                           (3840, 2160, 1280, 720), (1920, 1080, 3840, 2160), (640, 480, 1280, 960)]


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    assert d["MI355_INTERP_NEAREST"] == pkg.INTERP_NEAREST == NEAREST == 0
    assert d["MI355_INTERP_LINEAR"] == pkg.INTERP_LINEAR == LINEAR == 1
    assert d["MI355_INTERP_AREA"] == pkg.INTERP_AREA == AREA == 3
    assert d["MI355_MAX_AREA_FACTOR"] == pkg.MAX_AREA_FACTOR == 16


def test_library_exports_the_resize_symbols(pkg):
    lib = pkg.load_library()
    for name in ("mi355_resize_check", "mi355_resize_dev", "mi355_resize_batched"):
        assert name in pkg.declared_symbols(), name
        assert hasattr(lib, name), name


def test_c_program_using_the_resize_calls_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "resize_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    unsigned char in[16] = {0}, out[16];
    if (mi355_resize_check(4, 3840, 2160, 1920, 1080, 1, MI355_INTERP_LINEAR) != MI355_OK) return 1;
    if (mi355_resize_check(1, 640, 480, 1280, 960, 8, MI355_INTERP_NEAREST) != MI355_OK) return 2;
    if (mi355_resize_check(1, 640, 480, 40, 30, 8, MI355_INTERP_AREA) != MI355_OK) return 3;
    if (mi355_resize_check(4, 640, 480, 427, 320, 1, MI355_INTERP_AREA) != MI355_ERR_UNSUPPORTED) return 4;
    if (mi355_resize_check(4, 17 * MI355_MAX_AREA_FACTOR + 17, 4, 17, 4, 1, MI355_INTERP_AREA) != MI355_ERR_UNSUPPORTED)
        return 5;
    if (mi355_resize_check(3, 640, 480, 320, 240, 1, MI355_INTERP_LINEAR) != MI355_ERR_BAD_ARG) return 6;
    if (mi355_resize_check(4, 640, 480, 320, 240, 1, 2) != MI355_ERR_BAD_ARG) return 7;
    if (mi355_resize_check(4, 640, 480, 0, 240, 1, MI355_INTERP_LINEAR) != MI355_ERR_BAD_ARG) return 8;
    if (mi355_resize_dev((mi355_ctx*)0, in, out, 4, 2, 2, 2, 2, 1, MI355_INTERP_LINEAR) != MI355_ERR_BAD_ARG) return 9;
    if (mi355_resize_batched((mi355_ctx*)0, in, out, 1, 4, 4, 2, 2, 1, MI355_INTERP_AREA, (uint64_t*)0) !=
        MI355_ERR_BAD_ARG)
        return 10;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "resize_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


CHECK_TABLE = (
    # good cases: every interpolation, both bytes per pixel
    [((bpp, 640, 480, 320, 240, 1, i), OK) for bpp in (1, 4) for i in (NEAREST, LINEAR, AREA)] +
    [((bpp, 640, 480, 1023, 683, 3, i), OK) for bpp in (1, 4) for i in (NEAREST, LINEAR)] +
    [((bpp, 1, 1, 1, 1, 1, i), OK) for bpp in (1, 4) for i in (NEAREST, LINEAR, AREA)] +
    # bytes per pixel, interpolation
    [((bpp, 640, 480, 320, 240, 1, LINEAR), BAD_ARG) for bpp in (0, 2, 3, -1, 5, 8)] +
    [((4, 640, 480, 320, 240, 1, i), BAD_ARG) for i in (2, 4, -1, 5)] +
    # zero and negative sizes, in either shape, and the frame count
    [((4,) + s + (LINEAR,), BAD_ARG) for s in ((0, 480, 320, 240, 1), (640, 0, 320, 240, 1), (640, 480, 0, 240, 1),
                                               (640, 480, 320, 0, 1), (-640, 480, 320, 240, 1), (640, -1, 320, 240, 1),
                                               (640, 480, -320, 240, 1), (640, 480, 320, -240, 1), (640, 480, 320, 240, 0),
                                               (640, 480, 320, 240, -2))] +
    [((1, 0, 0, 0, 0, 1, AREA), BAD_ARG), ((1, 640, 480, 0, 0, 1, AREA), BAD_ARG)] +
    # AREA outside the integer factors; LINEAR and NEAREST take the same pairs
    [((bpp, 640, 480, 427, 320, 1, AREA), UNSUPPORTED) for bpp in (1, 4)] +
    [((4, 640, 480, 427, 480, 1, AREA), UNSUPPORTED), ((4, 640, 480, 640, 320 + 1, 1, AREA), UNSUPPORTED),
     ((4, 320, 240, 640, 480, 1, AREA), UNSUPPORTED), ((4, 320, 240, 320, 480, 1, AREA), UNSUPPORTED),
     ((4, 1700, 100, 100, 100, 1, AREA), UNSUPPORTED), ((1, 100, 1700, 100, 100, 1, AREA), UNSUPPORTED),
     ((4, 320, 240, 640, 480, 1, LINEAR), OK), ((4, 1700, 100, 100, 100, 1, LINEAR), OK),
     ((4, 640, 480, 427, 320, 1, NEAREST), OK)] +
    # AREA at 1 x and 16 x, and mixed factors
    [((bpp, 640, 480, 640, 480, 2, AREA), OK) for bpp in (1, 4)] +
    [((bpp, 1600, 160, 100, 10, 2, AREA), OK) for bpp in (1, 4)] +
    [((4, 96, 96, 32, 24, 1, AREA), OK), ((1, 4096, 32, 256, 2, 1, AREA), OK), ((1, 16, 1, 1, 1, 1, AREA), OK)]
)


def test_resize_check_on_a_table(pkg):
    lib = pkg.load_library()
    for args, want in CHECK_TABLE:
        assert lib.mi355_resize_check(*args) == want, (args, want)
        assert pkg.resize_check(*args) == want, (args, want)


def test_a_null_context_is_a_bad_argument(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint8 * 256)()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    for bpp in (1, 4):
        for interp in (NEAREST, LINEAR, AREA):
            assert lib.mi355_resize_dev(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p), bpp,
                                        4, 4, 2, 2, 1, interp) == BAD_ARG
            assert lib.mi355_resize_batched(None, ctypes.cast(buf, u8), ctypes.cast(out, u8), bpp, 4, 4, 2, 2, 1, interp,
                                            None) == BAD_ARG


def test_binding_methods(pkg):
    import inspect
    assert list(inspect.signature(pkg.Context.resize).parameters) == ["self", "rgba", "dst_w", "dst_h", "interp", "profile"]
    assert inspect.signature(pkg.Context.resize).parameters["interp"].default == pkg.INTERP_LINEAR
    assert list(inspect.signature(pkg.Context.resize_gray8).parameters)[:5] == ["self", "y", "dst_w", "dst_h", "interp"]
    assert list(inspect.signature(pkg.Context.resize_dev).parameters)[:10] == [
        "self", "d_in", "d_out", "bpp", "sw", "sh", "dw", "dh", "nframes", "interp"]


# ---- the reference ----------------------------------------------------------------------------------------------------
def _rint_i(v):
    """(int)rintf(v) for a float32 v: half to even"""
    return int(np.rint(F32(v)))


def scalar_resize(img, dw, dh, interp):
    """The header's text, one pixel and one channel at a time.  Python floats are fp64; np.float32 scalars are fp32."""
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    chans = img.reshape(sh, sw, -1)
    nc = chans.shape[2]
    out = np.zeros((dh, dw, nc), np.uint8)
    scale_x = 1.0 / (float(dw) / float(sw))
    scale_y = 1.0 / (float(dh) / float(sh))
    if interp == LINEAR and sw == 2 * dw and sh == 2 * dh:
        interp = AREA
    if interp == NEAREST:
        for dy in range(dh):
            sy = min(int(math.floor(dy * scale_y)), sh - 1)
            for dx in range(dw):
                sx = min(int(math.floor(dx * scale_x)), sw - 1)
                out[dy, dx] = chans[sy, sx]
    elif interp == LINEAR:
        cols = []
        for dx in range(dw):
            fx = F32((dx + 0.5) * scale_x - 0.5)
            sx = int(math.floor(fx))
            fx = F32(fx - F32(sx))
            if sx < 0:
                sx, fx = 0, F32(0)
            if sx >= sw - 1:
                sx, fx = sw - 1, F32(0)
            cols.append((sx, _rint_i((F32(1) - fx) * F32(2048)), _rint_i(fx * F32(2048))))
        for dy in range(dh):
            fy = F32((dy + 0.5) * scale_y - 0.5)
            sy = int(math.floor(fy))
            fy = F32(fy - F32(sy))
            b0, b1 = _rint_i((F32(1) - fy) * F32(2048)), _rint_i(fy * F32(2048))
            r0, r1 = min(max(sy, 0), sh - 1), min(max(sy + 1, 0), sh - 1)
            for dx, (sx, a0, a1) in enumerate(cols):
                sx1 = min(sx + 1, sw - 1)
                for c in range(nc):
                    h0 = int(chans[r0, sx, c]) * a0 + int(chans[r0, sx1, c]) * a1
                    h1 = int(chans[r1, sx, c]) * a0 + int(chans[r1, sx1, c]) * a1
                    v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
                    assert 0 <= v <= 255
                    out[dy, dx, c] = v
    else:
        n, m = sw // dw, sh // dh
        assert n * dw == sw and m * dh == sh and 1 <= n <= 16 and 1 <= m <= 16
        for dy in range(dh):
            for dx in range(dw):
                for c in range(nc):
                    total = int(chans[dy * m:(dy + 1) * m, dx * n:(dx + 1) * n, c].astype(np.int64).sum())
                    if n == 2 and m == 2:
                        v = (total + 2) >> 2
                    else:
                        v = _rint_i(F32(total) * (F32(1) / F32(n * m)))
                    out[dy, dx, c] = min(max(v, 0), 255)
    return out.reshape((dh, dw) + img.shape[2:])


def _images(sh, sw, seed):
    rng = np.random.default_rng(seed)
    ext = rng.integers(0, 2, (sh, sw, 4), dtype=np.uint8) * 255
    return (rng.integers(0, 256, (sh, sw), dtype=np.uint8), rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8), ext,
            np.full((sh, sw), 255, np.uint8))


@pytest.mark.parametrize("pair", SMALL_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_reference_equals_the_scalar_loop(pair):
    sw, sh, dw, dh = pair
    for interp in (NEAREST, LINEAR, AREA):
        if interp == AREA and area_factors(sw, sh, dw, dh) is None:
            continue
        for img in _images(sh, sw, sw * 7 + dh):
            want = scalar_resize(img, dw, dh, interp)
            got = resize_ref(img, dw, dh, interp)
            assert got.shape == want.shape and np.array_equal(got, want), (pair, interp, img.ndim)
            rows = sample_rows(dh, 3)
            assert np.array_equal(resize_ref(img, dw, dh, interp, rows=rows), want[rows]), (pair, interp)


def test_hand_worked_vector():
    """Columns 2 -> 4: fx = -0.25, 0.25, 0.75, 1.25 -> (sx, a0, a1) = (0, 2048, 0), (0, 1536, 512), (0, 512, 1536),
    (1, 2048, 0); one row, b0 = 2048: [0, 100] -> [0, 25, 75, 100]."""
    row = np.array([[0, 100]], np.uint8)
    assert resize_ref(row, 4, 1, LINEAR).tolist() == [[0, 25, 75, 100]]
    assert scalar_resize(row, 4, 1, LINEAR).tolist() == [[0, 25, 75, 100]]
    sx, sx1, a0, a1 = linear_cols(2, 4)
    assert (sx.tolist(), sx1.tolist(), a0.tolist(), a1.tolist()) == ([0, 0, 0, 1], [1, 1, 1, 1], [2048, 1536, 512, 2048],
                                                                     [0, 512, 1536, 0])
    assert resize_ref(row, 4, 1, NEAREST).tolist() == [[0, 0, 100, 100]]
    assert resize_ref(np.array([[10, 20], [30, 41]], np.uint8), 1, 1, AREA).tolist() == [[25]]  # (101 + 2) >> 2


def test_identity_at_equal_sizes():
    for sh, sw in ((1, 1), (9, 13), (48, 64), (31, 257)):
        for img in _images(sh, sw, sh + sw):
            for interp in (NEAREST, LINEAR, AREA):
                assert np.array_equal(resize_ref(img, sw, sh, interp), img), (sh, sw, interp)


def test_linear_at_exactly_half_size_is_area():
    for sh, sw in ((2, 2), (10, 14), (48, 64), (482, 642)):
        for img in _images(sh, sw, sh * sw):
            assert np.array_equal(resize_ref(img, sw // 2, sh // 2, LINEAR), resize_ref(img, sw // 2, sh // 2, AREA))


def test_constant_frames_stay_constant_for_every_byte_value():
    for sw, sh, dw, dh in ((7, 5, 13, 9), (13, 9, 7, 5), (64, 48, 21, 16), (48, 32, 3, 2), (18, 16, 6, 4), (10, 9, 25, 3)):
        for interp in (NEAREST, LINEAR, AREA):
            if interp == AREA and area_factors(sw, sh, dw, dh) is None:
                continue
            for v in range(256):
                out = resize_ref(np.full((sh, sw), v, np.uint8), dw, dh, interp)
                assert out.min() == v and out.max() == v, (sw, sh, dw, dh, interp, v)


def test_coefficient_pairs_sum_to_2048():
    for sw, sh, dw, dh in ALL_PAIRS:
        sx, sx1, a0, a1 = linear_cols(sw, dw)
        r0, r1, b0, b1 = linear_rows(sh, dh)
        assert np.all(a0 + a1 == 2048) and np.all(b0 + b1 == 2048), (sw, sh, dw, dh)
        assert a0.min() >= 0 and a1.min() >= 0 and b0.min() >= 0 and b1.min() >= 0
        assert sx.min() >= 0 and sx1.max() <= sw - 1 and r0.min() >= 0 and r1.max() <= sh - 1
        assert np.all(a1[sx >= sw - 1] == 0)


def test_scale_is_not_the_plain_quotient_everywhere():
    """1.0 / (dst / src) and src / dst differ in the last bit for some size pairs: the header's form is the contract."""
    differ = [(s, d) for s in range(1, 200) for d in range(1, 200) if scale_of(s, d) != float(s) / float(d)]
    assert differ and scale_of(640, 480) == 1.0 / (480.0 / 640.0)


def _exact_quotient_half_even(sums, k):
    q = (2 * sums + k) // (2 * k)                                       # round half up of the exact quotient
    tie = (2 * sums) % (2 * k) == k
    return np.where(tie & (q % 2 == 1), q - 1, q)                       # ties to even


def test_area_is_the_fp32_product_not_the_exact_quotient():
    """sum * (1.f / (float)(n m)) rounded half to even against the exactly rounded quotient.  For 3 x 3 blocks no sum
    tells them apart (all 2296 checked here), so a 3 x 3 case cannot pin the form; the smallest block that can has 14
    pixels (7 x 2): 91 / 14 is the tie 6.5, the exact form gives 6, the fp32 product 6.5000005 gives 7."""
    sums = np.arange(9 * 255 + 1)
    assert np.array_equal(area_byte(sums, 3, 3).astype(np.int64), _exact_quotient_half_even(sums, 9))
    first = None
    for k in range(1, 15):
        for n in range(1, 17):
            if k % n == 0 and k // n <= 16 and (n, k // n) != (2, 2):
                sums = np.arange(k * 255 + 1)
                d = np.flatnonzero(area_byte(sums, n, k // n).astype(np.int64) != _exact_quotient_half_even(sums, k))
                if len(d) and first is None:
                    first = (k, int(d[0]))
    assert first == (14, 91)
    s = 91
    assert int(np.rint(F32(s) * (F32(1) / F32(14)))) == 7 and int(_exact_quotient_half_even(np.array([s]), 14)[0]) == 6
    for n, m in ((7, 2), (2, 7)):
        block = np.zeros((m, n), np.uint8)
        block.flat[:] = [6] * 7 + [7] * 7
        assert int(block.sum()) == s
        assert resize_ref(block, 1, 1, AREA)[0, 0] == 7 and scalar_resize(block, 1, 1, AREA)[0, 0] == 7
    # and over all factors the two forms differ for the 4160 sums the header counts
    n_diff = 0
    for n in range(1, 17):
        for m in range(1, 17):
            if n == 2 and m == 2:
                continue
            sums = np.arange(n * m * 255 + 1)
            n_diff += int((area_byte(sums, n, m).astype(np.int64) != _exact_quotient_half_even(sums, n * m)).sum())
    assert n_diff == 4160
