"""Single-channel (gray8) filters: the parts of the C-ABI that need no GPU.

MI355_FILTER_GAUSS_GRAY8 / SOBEL_GRAY8 / PIPELINE_GRAY8 take 1 byte per pixel; mi355_filter_in_bpp reports the input
width of every filter, mi355_filter_out_bpp the output width.  The GPU behaviour is in test_gpu_gray8.py.
"""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_FILTER_\w+) (\d+)", text)}


def test_in_and_out_bytes_per_pixel_of_every_filter(pkg):
    lib = pkg.load_library()
    want_in = {0: 4, 1: 4, 2: 4, 3: 4, 4: 4, 5: 1, 6: 1, 7: 1}
    want_out = {0: 4, 1: 1, 2: 4, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1}
    for f in range(8):
        assert lib.mi355_filter_in_bpp(f) == want_in[f], f
        assert lib.mi355_filter_out_bpp(f) == want_out[f], f
    for bad in (-1, 8, 99):
        assert lib.mi355_filter_in_bpp(bad) == -1
        assert lib.mi355_filter_out_bpp(bad) == -1
    assert pkg.imgfilter.IN_BPP == want_in
    assert pkg.imgfilter.OUT_BPP == want_out


def test_header_and_binding_constants_agree(pkg):
    d = _header_defines()
    assert d["MI355_FILTER_GAUSS_GRAY8"] == pkg.FILTER_GAUSS_GRAY8 == 5
    assert d["MI355_FILTER_SOBEL_GRAY8"] == pkg.FILTER_SOBEL_GRAY8 == 6
    assert d["MI355_FILTER_PIPELINE_GRAY8"] == pkg.FILTER_PIPELINE_GRAY8 == 7
    assert "mi355_filter_in_bpp" in pkg.declared_symbols()
    assert pkg.load_library().mi355_filter_in_bpp.argtypes == [ctypes.c_int]


@pytest.mark.parametrize("filt", [5, 6, 7])
def test_gray8_ids_reject_bad_arguments_without_a_gpu(pkg, filt):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 64)()
    out = (ctypes.c_uint8 * 64)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    # null context (k validation needs a context: tests/test_gpu_gray8.py checks it)
    assert lib.mi355_filter_dev(None, filt, p_in, p_out, 8, 8, 1, 5, 1.5) == -1
    assert lib.mi355_filter_batched(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 5, 1.5, None) == -1
    assert lib.mi355_filter_stream(None, filt, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 0, 5, 1.5,
                                   None) == -1
    assert lib.mi355_pool_alloc(None, filt, 8, 8, 1, 5, 1.5, 1, None, None, None) == -1


def test_c_program_using_the_gray8_ids_links(pkg, tmp_path):
    lib_dir = os.path.dirname(pkg.imgfilter.library_path())
    src = tmp_path / "gray8_host.c"
    src.write_text(r'''
#include <stdio.h>
#include "mi355_imgfilter.h"
int main(void) {
    static const int ids[3] = {MI355_FILTER_GAUSS_GRAY8, MI355_FILTER_SOBEL_GRAY8, MI355_FILTER_PIPELINE_GRAY8};
    int i;
    for (i = 0; i < 3; i++) {
        if (mi355_filter_in_bpp(ids[i]) != 1 || mi355_filter_out_bpp(ids[i]) != 1) return 1 + i;
        if (mi355_filter_dev((mi355_ctx*)0, ids[i], (const void*)0, (void*)0, 4, 4, 1, 5, 1.5f) != MI355_ERR_BAD_ARG)
            return 10 + i;
    }
    if (mi355_filter_in_bpp(MI355_FILTER_PIPELINE) != 4 || mi355_filter_in_bpp(42) != MI355_ERR_BAD_ARG) return 20;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "gray8_host"
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", lib_dir, "-lmi355_imgfilter", "-Wl,-rpath," + lib_dir, "-o", str(exe)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
