"""CLAHE (mi355_clahe_*): the parts that need no GPU.

The header against the binding, the argument checks that come before any device work (mi355_clahe_check is a pure host
function), the CPU reference tests/clahe_ref.py against hand-worked frames, and the case list tests/clahe_cases.py
against the branches of the reference it claims to reach.  The GPU behaviour is in test_gpu_clahe.py.
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_cases as cc  # noqa: E402
import clahe_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
SYMBOLS = ("mi355_clahe_check", "mi355_clahe_gray8_dev", "mi355_clahe_gray8_batched", "mi355_clahe_luts_gray8_dev")


# ---- interface ------------------------------------------------------------------------------------------------------
def test_header_and_binding_constants_agree(pkg):
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}
    assert d["MI355_MAX_CLAHE_TILES"] == pkg.MAX_CLAHE_TILES == cr.MAX_TILES == 16


def test_the_four_symbols_are_declared_and_exported(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def test_a_null_context_or_pointer_is_a_bad_argument_without_a_gpu(pkg):
    lib = pkg.load_library()
    buf, out = (ctypes.c_uint8 * 4096)(), (ctypes.c_uint8 * 4096)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    assert lib.mi355_clahe_gray8_dev(None, p_in, p_out, 8, 8, 1, 2.0, 2, 2) == BAD_ARG
    assert lib.mi355_clahe_luts_gray8_dev(None, p_in, p_out, 8, 8, 1, 2.0, 2, 2) == BAD_ARG
    assert lib.mi355_clahe_gray8_batched(None, ctypes.cast(buf, u8), ctypes.cast(out, u8), 8, 8, 1, 2.0, 2, 2,
                                         None) == BAD_ARG


CHECKS = [
    ((64, 48, 1, 2.0, 8, 8), OK),
    ((1, 1, 1, 1.0, 1, 1), OK),
    ((16, 16, 1, 40.0, 16, 16), OK),
    ((31, 17, 1, 2.0, 16, 16), OK),                  # pads 1 column and 15 rows: 15 <= h - 1
    ((31, 16, 1, 2.0, 16, 16), UNSUPPORTED),         # the quirk pads 16 rows onto 16
    ((16, 31, 1, 2.0, 16, 16), UNSUPPORTED),         # ... and 16 columns onto 16
    ((3, 3, 1, 2.0, 4, 1), OK),                      # pads 1 column, 1 row
    ((2, 5, 1, 2.0, 4, 1), UNSUPPORTED),             # pads 2 columns onto 2
    ((1, 5, 1, 2.0, 2, 1), UNSUPPORTED),             # a 1-pixel row has nothing to reflect
    ((64, 48, 1, 2.0, 0, 8), BAD_ARG),
    ((64, 48, 1, 2.0, 8, 0), BAD_ARG),
    ((64, 48, 1, 2.0, 17, 8), BAD_ARG),
    ((64, 48, 1, 2.0, 8, 17), BAD_ARG),
    ((64, 48, 1, 2.0, -1, 8), BAD_ARG),
    ((64, 48, 1, float("nan"), 8, 8), BAD_ARG),
    ((64, 48, 1, float("inf"), 8, 8), BAD_ARG),
    ((64, 48, 1, float("-inf"), 8, 8), BAD_ARG),
    ((64, 48, 1, -3.0, 8, 8), OK),                   # clip_limit <= 0: no clipping
    ((64, 48, 1, 1e300, 8, 8), OK),                  # the clip limit in counts is capped at the tile size
    ((0, 48, 1, 2.0, 8, 8), BAD_ARG),
    ((64, 0, 1, 2.0, 8, 8), BAD_ARG),
    ((64, 48, 0, 2.0, 8, 8), BAD_ARG),
    ((65536, 32768, 1, 2.0, 8, 8), BAD_ARG),         # ew * eh == 2^31
    ((46341, 46340, 1, 2.0, 8, 8), BAD_ARG),         # w * h < 2^31, the extended 46344 x 46344 is not
    ((46341, 46340, 1, 2.0, 1, 1), OK),              # the same frame, nothing padded
    ((65536, 32767, 1, 2.0, 16, 1), OK),
]


@pytest.mark.parametrize("args,code", CHECKS)
def test_clahe_check_table(pkg, args, code):
    assert pkg.clahe_check(*args) == code
    assert pkg.load_library().mi355_clahe_check(*args) == code
    if code != BAD_ARG:
        w, h, _, _, tx, ty = args
        assert cr.supported(w, h, tx, ty) == (code == OK)


# ---- the reference by hand ------------------------------------------------------------------------------------------
def test_a_constant_frame_is_not_mapped_to_itself():
    y = np.full((48, 64), 7, np.uint8)
    assert np.array_equal(cr.clahe_ref(y, 2.0, 8, 8), np.full_like(y, 16))
    assert np.array_equal(cr.clahe_ref(y, 0.0, 8, 8), np.full_like(y, 255))
    # by hand: tot = 48, cl = (int)(2.0 * 48 / 256) = 0 -> 1; clipped = 47 -> batch 0, residual 47, step 5: bins 0, 5
    # take +1 below 7, bin 7 holds 1: sum = 3 at bin 7, 3 * (255 / 48) = 15.9375 -> 16
    assert cr.clip_of(2.0, 48) == 1
    assert cr.tile_lut(np.bincount([7] * 48, minlength=256), 1, 48)[7] == 16


def _steps(*pairs):
    """a table that is 0 below the first threshold and takes each value from its threshold on"""
    lut = np.zeros(256, np.uint8)
    for first, value in pairs:
        lut[first:] = value
    return lut


def test_a_two_by_two_tile_frame_by_hand():
    y = np.array([[0, 0, 10, 10],
                  [0, 0, 20, 20],
                  [1, 2, 255, 255],
                  [3, 4, 255, 255]], np.uint8)
    # tot = 4, no clipping: lut[b] = rint(cdf[b] * 63.75), ties to even (127.5 -> 128)
    want = np.stack([np.stack([_steps((0, 255)), _steps((10, 128), (20, 255))]),
                     np.stack([_steps((1, 64), (2, 128), (3, 191), (4, 255)), _steps((255, 255))])])
    luts = cr.luts_ref(y, 0.0, 2, 2)
    assert np.array_equal(luts, want)
    out = cr.clahe_ref(y, 0.0, 2, 2)
    assert out[0, 0] == 255    # tx1 = ty1 = -1: the corner tile alone
    assert out[1, 1] == 255    # txf = tyf = 0: xa = ya = 0, tile (0, 0) alone
    assert out[1, 2] == 255    # xa = .5 between tiles (0, 0) and (0, 1) at v = 20: 255 * .5 + 255 * .5
    assert out[2, 1] == 192    # ya = .5 between tiles (0, 0) and (1, 0) at v = 2: 255 * .5 + 128 * .5 = 191.5 -> 192
    assert out[2, 0] == 160    # the same pair at v = 1: 255 * .5 + 64 * .5 = 159.5 -> 160, the even neighbour
    assert out[3, 0] == 191    # tyf = 1: ya = 0, tile (1, 0) alone at v = 3


def test_the_reflected_pad_by_hand():
    """5 x 3 with 2 x 2 tiles: ew = 6, eh = 4; column 5 is column 3 again, row 3 is row 1 again."""
    y = np.arange(15, dtype=np.uint8).reshape(3, 5)
    ext = cr.extend(y, 2, 2)
    assert ext.shape == (4, 6)
    assert np.array_equal(ext[:3, :5], y)
    assert np.array_equal(ext[:3, 5], y[:, 3]) and np.array_equal(ext[3, :5], y[1]) and ext[3, 5] == y[1, 3]
    assert cr.geometry(5, 3, 2, 2) == (6, 4, 3, 2)
    assert cr.geometry(67, 48, 8, 8) == (72, 56, 9, 7)    # the quirk: 48 divides and still gets 8 rows
    assert cr.geometry(64, 50, 8, 8) == (72, 56, 9, 7)
    assert cr.geometry(64, 48, 8, 8) == (64, 48, 8, 6)


@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (48, 64)])
@pytest.mark.parametrize("clip", [0.0, -1.0])
def test_one_tile_without_clipping_is_the_plain_cdf_table(shape, clip):
    h, w = shape
    y = cc.uniform_noise(h, w, 5)
    cdf = np.cumsum(np.bincount(y.ravel(), minlength=256))
    lut = np.rint(cdf.astype(np.float32) * (np.float32(255.0) / np.float32(w * h))).astype(np.uint8)
    assert np.array_equal(cr.clahe_ref(y, clip, 1, 1), lut[y])


# ---- the case list --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _branches():
    """branch name -> the (case, content) pairs that reach it"""
    seen = {}

    def hit(name, where):
        seen.setdefault(name, []).append(where)

    for case in cc.CASES:
        w, h, tx, ty, clip = case
        ew, eh, tw, th = cr.geometry(w, h, tx, ty)
        if w % tx and not h % ty:
            hit("pad_width_only", case)
        if h % ty and not w % tx:
            hit("pad_height_only", case)
        if tw * th == 1:
            hit("one_pixel_tiles", case)
        for name, y in cc.frames_of(case):
            traces, res = [], []
            luts = cr.luts_ref(y, clip, tx, ty, traces)
            cr.apply_ref(y, luts, tx, ty, res)
            res = np.concatenate(res)
            assert res.dtype == np.float32
            assert 0.0 <= float(res.min()) and float(res.max()) <= 255.0, (case, name)
            if np.any(np.mod(res.astype(np.float64), 1.0) == 0.5):
                hit("res_on_half", (case, name))
            for t in traces:
                if t["half"]:
                    hit("table_product_on_half", (case, name))
                if not t["clipped"]:
                    hit("no_clip", (case, name))
                    continue
                hit("batch_positive" if t["batch"] > 0 else "batch_zero", (case, name))
                if t["residual"] == 0:
                    hit("residual_zero", (case, name))
                elif t["step"] == 1:
                    hit("step_1", (case, name))
                elif t["step"] == 2:
                    hit("step_2", (case, name))
                else:
                    hit("step_3_or_more", (case, name))
    return seen


@pytest.mark.parametrize("branch", ["batch_positive", "batch_zero", "residual_zero", "step_1", "step_2", "step_3_or_more",
                                    "table_product_on_half", "res_on_half", "pad_width_only", "pad_height_only",
                                    "one_pixel_tiles", "no_clip"])
def test_the_case_list_reaches_the_branch(branch):
    assert _branches().get(branch), branch


def test_every_case_is_accepted_and_has_the_three_contents(pkg):
    assert len(cc.CASES) == 14
    for case in cc.CASES:
        w, h, tx, ty, clip = case
        assert pkg.clahe_check(w, h, 3, clip, tx, ty) == OK, case
        frames = cc.frames_of(case)
        assert [n for n, _ in frames] == ["uniform_noise", "low_contrast", "wrapped_gradient"]
        assert all(f.shape == (h, w) and f.dtype == np.uint8 for _, f in frames)
        low = frames[1][1]
        assert 100 <= int(low.min()) and int(low.max()) <= 123


def test_the_closed_form_of_the_redistribution():
    """bin b takes the +1 iff b % step == 0 and b // step < residual: OpenCV's loop, for every residual"""
    for residual in range(1, 256):
        step = max(256 // residual, 1)
        loop = np.zeros(256, np.int64)
        b, left = 0, residual
        while b < 256 and left > 0:
            loop[b] += 1
            b += step
            left -= 1
        closed = np.array([1 if b % step == 0 and b // step < residual else 0 for b in range(256)])
        assert np.array_equal(loop, closed) and loop.sum() == residual, residual
