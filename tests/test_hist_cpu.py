"""Histogram equalization and Otsu thresholding: the parts that need no GPU.

MI355_FILTER_EQUALIZE_GRAY8 (40) and MI355_FILTER_OTSU_GRAY8 (41), 1 byte -> 1 byte, through the pure host functions,
the argument checks that come before any device work, the header, a C99 caller, and the CPU reference tests/hist_ref.py
on hand-worked frames and against independent formulations.  The GPU behaviour is in test_gpu_hist.py.
"""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hist_ref import (equalize_lut, equalize_ref, hist_ref, otsu_ref, otsu_threshold,  # noqa: E402
                      otsu_thresholds_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = {"EQUALIZE_GRAY8": 40, "OTSU_GRAY8": 41}


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    for name, fid in IDS.items():
        assert d["MI355_FILTER_" + name] == getattr(pkg, "FILTER_" + name) == fid


def test_bytes_per_pixel_of_the_statistics_ids(pkg):
    lib = pkg.load_library()
    for f in IDS.values():
        assert (lib.mi355_filter_in_bpp(f), lib.mi355_filter_out_bpp(f)) == (1, 1), f
        assert pkg.imgfilter._in_bpp(f) == pkg.imgfilter._out_bpp(f) == 1
        assert f not in pkg.IN_BPP and f not in pkg.OUT_BPP  # those list the filters 0-7
    for bad in tuple(range(32, 40)) + tuple(range(42, 48)):
        assert lib.mi355_filter_in_bpp(bad) == -1 and lib.mi355_filter_out_bpp(bad) == -1, bad


@pytest.mark.parametrize("filt", sorted(IDS.values()))
def test_statistics_ids_with_a_null_context_are_bad_arguments(pkg, filt):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 4096)()
    out = (ctypes.c_uint8 * 4096)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    assert lib.mi355_filter_dev(None, filt, p_in, p_out, 8, 8, 1, 0, 0.0) == -1
    assert lib.mi355_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, 0.0, None) == -1
    assert lib.mi355_filter_stream(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, 0, 0.0,
                                   None) == -1
    assert lib.mi355_pool_alloc(None, filt, 8, 8, 1, 0, 0.0, 1, None, None, None) == -1
    assert lib.mi355_group_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, 0.0,
                                          None) == -1
    assert lib.mi355_group_filter_dev(None, filt, None, None, 8, 8, None, 0, 0.0) == -1


def test_statistics_calls_with_a_null_context_are_bad_arguments(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 4096)()
    out = (ctypes.c_uint32 * 1024)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    for fn in (lib.mi355_hist_gray8_dev, lib.mi355_otsu_thresholds_gray8_dev):
        assert fn(None, p_in, p_out, 8, 8, 1) == -1
        assert fn(None, None, None, 8, 8, 1) == -1
        assert fn(None, p_in, p_out, 65536, 32768, 1) == -1


def test_c_program_using_the_statistics_ids_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "hist_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    static const int ids[2] = {MI355_FILTER_EQUALIZE_GRAY8, MI355_FILTER_OTSU_GRAY8};
    static uint8_t in[64];
    static uint32_t hist[256];
    static int32_t t[1];
    int i;
    for (i = 0; i < 2; i++) {
        if (mi355_filter_in_bpp(ids[i]) != 1 || mi355_filter_out_bpp(ids[i]) != 1) return 1 + i;
        if (mi355_filter_dev((mi355_ctx*)0, ids[i], in, hist, 8, 8, 1, 0, 0.0f) != MI355_ERR_BAD_ARG) return 10 + i;
    }
    if (mi355_hist_gray8_dev((mi355_ctx*)0, in, hist, 8, 8, 1) != MI355_ERR_BAD_ARG) return 20;
    if (mi355_otsu_thresholds_gray8_dev((mi355_ctx*)0, in, t, 8, 8, 1) != MI355_ERR_BAD_ARG) return 21;
    if (mi355_filter_out_bpp(39) != MI355_ERR_BAD_ARG || mi355_filter_in_bpp(42) != MI355_ERR_BAD_ARG)
        return 30;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "hist_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


def test_binding_methods(pkg):
    import inspect
    for m in ("equalize_hist_gray8", "otsu_gray8", "hist_gray8", "otsu_thresholds_gray8"):
        assert list(inspect.signature(getattr(pkg.Context, m)).parameters) == ["self", "y"], m
    for m in ("hist_gray8_dev", "otsu_thresholds_gray8_dev"):
        assert list(inspect.signature(getattr(pkg.Context, m)).parameters)[3:] == ["w", "h", "nframes"], m


# ---- the reference on hand-worked frames ------------------------------------------------------------------------------
def test_seven_levels_equalize_with_half_even_rounding():
    """scale = 255 / 6 = 42.5 exactly; 42.5 -> 42, 127.5 -> 128, 212.5 -> 212."""
    y = np.arange(7, dtype=np.uint8)[None]
    assert equalize_ref(y).tolist() == [[0, 42, 85, 128, 170, 212, 255]]
    assert otsu_thresholds_ref(y) == 2  # {0,1,2} | {3..6} and {0..3} | {4,5,6} tie: the strict > keeps the first


@pytest.mark.parametrize("v", [0, 1, 37, 128, 254, 255])
def test_constant_frame(v):
    y = np.full((9, 13), v, np.uint8)
    assert np.array_equal(equalize_ref(y), y)
    assert otsu_thresholds_ref(y) == 0
    assert np.array_equal(otsu_ref(y), np.full_like(y, 255 if v > 0 else 0))


def test_two_value_frame():
    y = np.full((30, 40), 50, np.uint8)
    y[:, 25:] = 200
    assert np.array_equal(equalize_ref(y), np.where(y == 200, 255, 0))
    assert otsu_thresholds_ref(y) == 50
    assert np.array_equal(otsu_ref(y), np.where(y == 200, 255, 0))


def test_one_outlier_at_exactly_flt_epsilon_of_the_frame():
    """4096 x 2048 = 2^23 pixels: the outlier's bin holds q1 = 2^-23 = FLT_EPSILON, which is not < FLT_EPSILON, so the
    loop runs at i = 10 and t = 10."""
    y = np.full((2048, 4096), 200, np.uint8)
    y[1000, 3000] = 10
    h = hist_ref(y)
    assert h[10] == 1 and h[200] == 2 ** 23 - 1
    assert otsu_threshold(h) == 10
    o = otsu_ref(y)
    assert o[1000, 3000] == 0 and int(o.sum()) == 255 * (2 ** 23 - 1)
    e = equalize_ref(y)
    assert e[1000, 3000] == 0 and int(e.sum()) == 255 * (2 ** 23 - 1)


def test_one_outlier_below_flt_epsilon_of_the_frame():
    """4096 x 2049 pixels: q1 < FLT_EPSILON up to bin 199 and q2 = 0 from bin 200, so every bin takes the `continue`,
    t = 0 and the outlier (a nonzero value) maps to 255."""
    y = np.full((2049, 4096), 200, np.uint8)
    y[7, 9] = 10
    assert otsu_threshold(hist_ref(y)) == 0
    assert np.all(otsu_ref(y) == 255)


# ---- the reference against independent formulations -----------------------------------------------------------------
def _random_hists(seed, count):
    rng = np.random.default_rng(seed)
    for i in range(count):
        h = np.zeros(256, np.int64)
        k = int(rng.integers(1, 12)) if i % 2 else 256
        bins = rng.choice(256, k, replace=False)
        h[bins] = rng.integers(1, 5000, k)
        yield h


def test_equalize_table_equals_a_vectorised_float32_form():
    for h in _random_hists(1, 200):
        total = int(h.sum())
        i0 = int(np.flatnonzero(h)[0])
        if h[i0] == total:
            continue
        scale = np.float32(255) / np.float32(total - h[i0])
        s = (np.cumsum(h) - h[i0]).astype(np.float32)
        want = np.minimum(np.rint(s * scale), 255).astype(np.uint8)
        got = equalize_lut(h)
        assert np.array_equal(got[i0 + 1:], want[i0 + 1:]) and got[i0] == 0


def test_otsu_threshold_maximises_the_exact_between_class_variance():
    """t's exact (rational) between-class variance is the largest there is, up to rounding of the fp64 loop."""
    for h in _random_hists(2, 40):
        hist = [int(v) for v in h]
        total = sum(hist)
        mu = Fraction(sum(i * v for i, v in enumerate(hist)), total)
        best, var = Fraction(0), {}
        w1 = m1 = 0
        for i in range(256):
            w1 += hist[i]
            m1 += i * hist[i]
            if 0 < w1 < total:
                q1 = Fraction(w1, total)
                mu1 = Fraction(m1, w1)
                mu2 = (mu - q1 * mu1) / (1 - q1)
                var[i] = q1 * (1 - q1) * (mu1 - mu2) ** 2
                best = max(best, var[i])
        t = otsu_threshold(h)
        if best == 0:
            assert t == 0
        else:
            assert float(var[t]) >= float(best) * (1 - 1e-12), (t, float(var[t]), float(best))


def test_frames_are_their_own_images():
    y = np.zeros((3, 5, 7), np.uint8)
    y[1] = 9
    y[2, :, 3:] = 250
    assert hist_ref(y)[0, 0] == 35 and hist_ref(y)[1, 9] == 35 and hist_ref(y)[2, 250] == 20
    assert np.array_equal(equalize_ref(y), np.stack([equalize_ref(f) for f in y]))
    assert otsu_thresholds_ref(y).tolist() == [otsu_threshold(hist_ref(f)) for f in y]
