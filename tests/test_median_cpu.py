"""Median filter: the parts that need no GPU.

MI355_FILTER_MEDIAN (16, RGBA -> RGBA) and MI355_FILTER_MEDIAN_GRAY8 (17, 1 byte -> 1 byte) through the pure host
functions, the argument checks that come before any device work, the header, a C99 caller, and the CPU reference
tests/median_ref.py against a brute-force loop.  The GPU behaviour is in test_gpu_median.py.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from median_ref import median_ref, sample_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}


def test_bytes_per_pixel_of_the_median_ids(pkg):
    lib = pkg.load_library()
    assert (lib.mi355_filter_in_bpp(16), lib.mi355_filter_out_bpp(16)) == (4, 4)
    assert (lib.mi355_filter_in_bpp(17), lib.mi355_filter_out_bpp(17)) == (1, 1)
    for bad in (8, 15, 18):
        assert lib.mi355_filter_in_bpp(bad) == -1 and lib.mi355_filter_out_bpp(bad) == -1, bad
    assert pkg.imgfilter._in_bpp(16) == pkg.imgfilter._out_bpp(16) == 4
    assert pkg.imgfilter._in_bpp(17) == pkg.imgfilter._out_bpp(17) == 1


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    assert d["MI355_FILTER_MEDIAN"] == pkg.FILTER_MEDIAN == 16
    assert d["MI355_FILTER_MEDIAN_GRAY8"] == pkg.FILTER_MEDIAN_GRAY8 == 17
    assert d["MI355_MAX_MEDIAN_K"] == pkg.MAX_MEDIAN_K == 7


@pytest.mark.parametrize("filt", [16, 17])
def test_median_ids_with_a_null_context_are_bad_arguments(pkg, filt):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint8 * 256)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    for k in (3, 5, 7):
        assert lib.mi355_filter_dev(None, filt, p_in, p_out, 8, 8, 1, k, 0.0) == -1
        assert lib.mi355_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, k, 0.0,
                                        None) == -1
        assert lib.mi355_filter_stream(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, k, 0.0,
                                       None) == -1
        assert lib.mi355_pool_alloc(None, filt, 8, 8, 1, k, 0.0, 1, None, None, None) == -1
        assert lib.mi355_group_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, k,
                                              0.0, None) == -1
        assert lib.mi355_group_filter_dev(None, filt, None, None, 8, 8, None, k, 0.0) == -1


def test_c_program_using_the_median_ids_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "median_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    static const int ids[2] = {MI355_FILTER_MEDIAN, MI355_FILTER_MEDIAN_GRAY8};
    static const int bpp[2] = {4, 1};
    int i;
    for (i = 0; i < 2; i++) {
        if (mi355_filter_in_bpp(ids[i]) != bpp[i] || mi355_filter_out_bpp(ids[i]) != bpp[i]) return 1 + i;
        if (mi355_filter_dev((mi355_ctx*)0, ids[i], (const void*)0, (void*)0, 4, 4, 1, MI355_MAX_MEDIAN_K, 0.0f) !=
            MI355_ERR_BAD_ARG)
            return 10 + i;
    }
    if (mi355_filter_in_bpp(8) != MI355_ERR_BAD_ARG || mi355_filter_out_bpp(18) != MI355_ERR_BAD_ARG) return 20;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "median_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


def _brute(img, k):
    h, w = img.shape[:2]
    r = k // 2
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            ys = [min(max(y + d, 0), h - 1) for d in range(-r, r + 1)]
            xs = [min(max(x + d, 0), w - 1) for d in range(-r, r + 1)]
            win = img[np.ix_(ys, xs)].reshape(k * k, *img.shape[2:])
            out[y, x] = np.sort(win, axis=0)[k * k // 2]
    return out


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (6, 1), (2, 3), (9, 9)])
def test_median_ref_is_the_brute_force_median(k, shape):
    rng = np.random.default_rng(k * 100 + shape[0] * 10 + shape[1])
    for img in (rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape + (4,), dtype=np.uint8),
                rng.integers(0, 3, shape, dtype=np.uint8)):  # ties
        want = _brute(img, k)
        assert np.array_equal(median_ref(img, k), want), (k, shape, img.ndim)
        rows = sample_rows(shape[0], k, bands=((0.5, 1),))
        assert np.array_equal(median_ref(img, k, rows=rows), want[rows]), (k, shape)
