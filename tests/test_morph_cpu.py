"""Rectangular morphology: the parts that need no GPU.

MI355_FILTER_ERODE / DILATE / OPEN / CLOSE (24-27, RGBA -> RGBA) and their *_GRAY8 forms (28-31, 1 byte -> 1 byte)
through the pure host functions, the argument checks that come before any device work, the header, a C99 caller, and
the CPU reference tests/morph_ref.py against a brute-force loop over OpenCV's clipped window and against scipy.ndimage.
The GPU behaviour is in test_gpu_morph.py.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from median_ref import sample_rows  # noqa: E402
from morph_ref import OPS, dilate_ref, erode_ref, morph_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBA_IDS = {"erode": 24, "dilate": 25, "open": 26, "close": 27}
GRAY8_IDS = {"erode": 28, "dilate": 29, "open": 30, "close": 31}
KS = tuple(range(3, 18, 2))


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    for op in OPS:
        name = op.upper()
        assert d["MI355_FILTER_" + name] == getattr(pkg, "FILTER_" + name) == RGBA_IDS[op]
        assert d["MI355_FILTER_%s_GRAY8" % name] == getattr(pkg, "FILTER_%s_GRAY8" % name) == GRAY8_IDS[op]
    assert d["MI355_MAX_MORPH_K"] == pkg.MAX_MORPH_K == 17


def test_bytes_per_pixel_of_the_morphology_ids(pkg):
    lib = pkg.load_library()
    for f in RGBA_IDS.values():
        assert (lib.mi355_filter_in_bpp(f), lib.mi355_filter_out_bpp(f)) == (4, 4), f
        assert pkg.imgfilter._in_bpp(f) == pkg.imgfilter._out_bpp(f) == 4
    for f in GRAY8_IDS.values():
        assert (lib.mi355_filter_in_bpp(f), lib.mi355_filter_out_bpp(f)) == (1, 1), f
        assert pkg.imgfilter._in_bpp(f) == pkg.imgfilter._out_bpp(f) == 1
    for bad in (8, 15, 18, 19, 20, 21, 22, 23, 32, 33):
        assert lib.mi355_filter_in_bpp(bad) == -1 and lib.mi355_filter_out_bpp(bad) == -1, bad


@pytest.mark.parametrize("filt", sorted(RGBA_IDS.values()) + sorted(GRAY8_IDS.values()))
def test_morphology_ids_with_a_null_context_are_bad_arguments(pkg, filt):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint8 * 256)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    for k in (3, 9, 17):
        assert lib.mi355_filter_dev(None, filt, p_in, p_out, 8, 8, 1, k, 0.0) == -1
        assert lib.mi355_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, k, 0.0,
                                        None) == -1
        assert lib.mi355_filter_stream(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, k, 0.0,
                                       None) == -1
        assert lib.mi355_pool_alloc(None, filt, 8, 8, 1, k, 0.0, 1, None, None, None) == -1
        assert lib.mi355_group_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, k,
                                              0.0, None) == -1
        assert lib.mi355_group_filter_dev(None, filt, None, None, 8, 8, None, k, 0.0) == -1


def test_c_program_using_the_morphology_ids_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "morph_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    static const int ids[8] = {MI355_FILTER_ERODE, MI355_FILTER_DILATE, MI355_FILTER_OPEN, MI355_FILTER_CLOSE,
                               MI355_FILTER_ERODE_GRAY8, MI355_FILTER_DILATE_GRAY8, MI355_FILTER_OPEN_GRAY8,
                               MI355_FILTER_CLOSE_GRAY8};
    int i;
    for (i = 0; i < 8; i++) {
        const int bpp = i < 4 ? 4 : 1;
        if (mi355_filter_in_bpp(ids[i]) != bpp || mi355_filter_out_bpp(ids[i]) != bpp) return 1 + i;
        if (mi355_filter_dev((mi355_ctx*)0, ids[i], (const void*)0, (void*)0, 4, 4, 1, MI355_MAX_MORPH_K, 0.0f) !=
            MI355_ERR_BAD_ARG)
            return 10 + i;
    }
    if (mi355_filter_out_bpp(18) != MI355_ERR_BAD_ARG || mi355_filter_in_bpp(23) != MI355_ERR_BAD_ARG ||
        mi355_filter_out_bpp(32) != MI355_ERR_BAD_ARG)
        return 20;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "morph_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


# ---- the reference ----------------------------------------------------------------------------------------------------
def _clipped(img, k, fn):
    """OpenCV's default border for erode / dilate: the part of the window outside the frame is left out."""
    h, w = img.shape[:2]
    r = k // 2
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            out[y, x] = fn(img[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1], axis=(0, 1))
    return out


def _images(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape + (4,), dtype=np.uint8),
            rng.integers(0, 3, shape, dtype=np.uint8))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (6, 1), (2, 3), (9, 9), (5, 20)])
def test_clamped_window_equals_opencvs_clipped_window(k, shape):
    for img in _images(shape, k * 100 + shape[0] * 10 + shape[1]):
        ero, dil = _clipped(img, k, np.min), _clipped(img, k, np.max)
        assert np.array_equal(erode_ref(img, k), ero), (k, shape, img.ndim)
        assert np.array_equal(dilate_ref(img, k), dil), (k, shape, img.ndim)
        assert np.array_equal(morph_ref("open", img, k), _clipped(ero, k, np.max)), (k, shape)
        assert np.array_equal(morph_ref("close", img, k), _clipped(dil, k, np.min)), (k, shape)
        rows = sample_rows(shape[0], k, bands=((0.5, 1),))
        for op in OPS:
            assert np.array_equal(morph_ref(op, img, k, rows=rows), morph_ref(op, img, k)[rows]), (op, k, shape)


@pytest.mark.parametrize("k", KS)
def test_reference_equals_scipy_ndimage(k):
    nd = pytest.importorskip("scipy.ndimage")
    fns = {"erode": nd.grey_erosion, "dilate": nd.grey_dilation, "open": nd.grey_opening, "close": nd.grey_closing}
    for shape in [(1, 1), (3, 2), (17, 17), (40, 61)]:
        for img in _images(shape, k + shape[1]):
            size = (k, k) + ((1,) if img.ndim == 3 else ())
            for op in OPS:
                want = fns[op](img, size=size, mode="nearest")
                assert np.array_equal(morph_ref(op, img, k), want), (op, k, shape, img.ndim)


@pytest.mark.parametrize("k", KS)
def test_erosion_and_dilation_are_dual(k):
    for img in _images((23, 31), k):
        assert np.array_equal(erode_ref(img, k), 255 - dilate_ref(255 - img, k))
        assert np.array_equal(morph_ref("open", img, k), 255 - morph_ref("close", 255 - img, k))


def test_iterated_erosion_is_one_larger_erosion():
    """cv::erode(..., iterations = n) with a k x k rectangle equals one erosion of size n(k - 1) + 1."""
    img = _images((30, 37), 7)[1]
    for k, n in ((3, 2), (3, 4), (5, 3)):
        it = img
        for _ in range(n):
            it = erode_ref(it, k)
        assert np.array_equal(it, erode_ref(img, n * (k - 1) + 1)), (k, n)


def test_binding_methods(pkg):
    """erode / dilate / morph_open / morph_close and their _gray8 forms; Context.close() still releases the context."""
    import inspect
    for name in ("erode", "dilate", "morph_open", "morph_close"):
        for m in (name, name + "_gray8"):
            assert list(inspect.signature(getattr(pkg.Context, m)).parameters)[:3] == ["self", "rgba" if "gray8" not in m
                                                                                     else "y", "k"], m
    assert list(inspect.signature(pkg.Context.close).parameters) == ["self"]
