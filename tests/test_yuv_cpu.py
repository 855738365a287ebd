"""YUV frames (mi355_yuv_*): the parts that need no GPU.

The header against the binding and against the CPU reference tests/yuv_ref.py, the argument checks that come before any
device work (mi355_yuv_check and mi355_yuv_frame_bytes are pure host functions), the reference against hand-worked
pixels and byte positions, and the case list tests/yuv_cases.py against the branches it claims to reach.  The GPU
behaviour is in test_gpu_yuv.py.
"""
import ctypes
import functools
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_cases as yc  # noqa: E402
import yuv_ref as yr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_imgfilter.h")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
SYMBOLS = ("mi355_yuv_frame_bytes", "mi355_yuv_check", "mi355_yuv_to_rgba8_dev", "mi355_rgba8_to_yuv_dev",
           "mi355_yuv_to_gray8_dev", "mi355_yuv_to_rgba8_batched", "mi355_rgba8_to_yuv_batched")
DEC_KEYS = ("YOFF", "CY", "CVR", "CVG", "CUG", "CUB")
ENC_KEYS = ("CRY", "CGY", "CBY", "CRU", "CGU", "CBU", "CGV", "CBV")


# ---- interface ------------------------------------------------------------------------------------------------------
def test_header_and_binding_constants_agree(pkg):
    text = open(HEADER).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}
    for i, name in enumerate(("NV12", "NV21", "I420", "YV12", "YUY2", "UYVY")):
        assert d["MI355_YUV_" + name] == getattr(pkg, "YUV_" + name) == getattr(yr, name) == i, name
    for i, name in enumerate(("BT601", "BT709", "BT601_FULL")):
        assert d["MI355_YUV_" + name] == getattr(pkg, "YUV_" + name) == getattr(yr, name) == i, name


def test_the_new_symbols_are_declared_and_exported(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert lib.mi355_yuv_frame_bytes.restype is ctypes.c_size_t
    for name in ("yuv_to_rgba8_dev", "rgba8_to_yuv_dev", "yuv_to_gray8_dev", "yuv_to_rgba8", "rgba8_to_yuv"):
        assert callable(getattr(pkg.Context, name)), name


def test_a_null_context_or_pointer_is_a_bad_argument_without_a_gpu(pkg):
    """the null checks come before anything reads the context: a non-null stand-in for it is never dereferenced"""
    lib = pkg.load_library()
    buf, out, fake = (ctypes.c_uint8 * 4096)(), (ctypes.c_uint8 * 4096)(), (ctypes.c_uint8 * 4096)()
    p_in, p_out, p_ctx = (ctypes.cast(b, ctypes.c_void_p) for b in (buf, out, fake))
    u8 = ctypes.POINTER(ctypes.c_uint8)
    h_in, h_out = ctypes.cast(buf, u8), ctypes.cast(out, u8)
    for fn in (lib.mi355_yuv_to_rgba8_dev, lib.mi355_rgba8_to_yuv_dev):
        assert fn(None, p_in, p_out, 8, 8, 1, 0, 0, 0, 0) == BAD_ARG
        assert fn(p_ctx, None, p_out, 8, 8, 1, 0, 0, 0, 0) == BAD_ARG
        assert fn(p_ctx, p_in, None, 8, 8, 1, 0, 0, 0, 0) == BAD_ARG
    assert lib.mi355_yuv_to_gray8_dev(None, p_in, p_out, 8, 8, 1, 0, 0, 0) == BAD_ARG
    assert lib.mi355_yuv_to_gray8_dev(p_ctx, None, p_out, 8, 8, 1, 0, 0, 0) == BAD_ARG
    assert lib.mi355_yuv_to_gray8_dev(p_ctx, p_in, None, 8, 8, 1, 0, 0, 0) == BAD_ARG
    for fn in (lib.mi355_yuv_to_rgba8_batched, lib.mi355_rgba8_to_yuv_batched):
        assert fn(None, h_in, h_out, 8, 8, 1, 0, 0, 0, 0, None) == BAD_ARG
        assert fn(p_ctx, None, h_out, 8, 8, 1, 0, 0, 0, 0, None) == BAD_ARG
        assert fn(p_ctx, h_in, None, 8, 8, 1, 0, 0, 0, 0, None) == BAD_ARG
    # value checks too come before the context is touched
    assert lib.mi355_yuv_to_rgba8_dev(p_ctx, p_in, p_out, 7, 8, 1, 0, 0, 0, 0) == BAD_ARG
    assert lib.mi355_rgba8_to_yuv_dev(p_ctx, p_out, p_in, 8, 8, 1, yr.YUY2, 0, 0, 0) == UNSUPPORTED
    assert lib.mi355_rgba8_to_yuv_batched(p_ctx, h_in, h_out, 8, 8, 1, yr.UYVY, 0, 0, 0, None) == UNSUPPORTED


# (layout, standard, w, h, nframes, pitch, rows, encode) -> (code, frame bytes when the decode accepts the geometry)
N12, N21, I4, Y12, YUY, UYV = yr.LAYOUTS
CHECKS = [
    ((N12, 0, 1920, 1080, 1, 0, 0, 0), OK, 1920 * 1080 * 3 // 2),
    ((N12, 1, 1920, 1080, 4, 2048, 1088, 0), OK, 2048 * 1088 * 3 // 2),     # a decoder surface
    ((N12, 0, 1920, 1080, 4, 2048, 1088, 1), OK, 2048 * 1088 * 3 // 2),
    ((I4, 2, 2, 2, 1, 0, 0, 1), OK, 6),
    ((Y12, 0, 6, 4, 3, 8, 6, 0), OK, 72),
    ((N21, 0, 6, 4, 1, 9, 4, 0), OK, 54),                                    # semi-planar: an odd pitch is fine
    ((YUY, 0, 6, 3, 1, 0, 0, 0), OK, 36),                                    # packed: any h
    ((UYV, 0, 6, 3, 1, 13, 5, 0), OK, 65),
    ((N12, 0, 7, 4, 1, 0, 0, 0), BAD_ARG, 0),                                # odd w
    ((YUY, 0, 7, 4, 1, 0, 0, 0), BAD_ARG, 0),
    ((N12, 0, 6, 3, 1, 0, 0, 0), BAD_ARG, 0),                                # odd h, 4:2:0
    ((I4, 0, 6, 4, 1, 0, 5, 0), BAD_ARG, 0),                                 # odd rows, 4:2:0
    ((N12, 0, 6, 4, 1, 4, 0, 0), BAD_ARG, 0),                                # pitch < w
    ((YUY, 0, 6, 4, 1, 10, 0, 0), BAD_ARG, 0),                               # pitch < 2 w, packed
    ((I4, 0, 6, 4, 1, 9, 0, 0), BAD_ARG, 0),                                 # odd planar pitch
    ((Y12, 0, 6, 4, 1, 9, 0, 1), BAD_ARG, 0),
    ((N12, 0, 6, 4, 1, 0, 2, 0), BAD_ARG, 0),                                # rows < h
    ((N12, 0, 6, 4, 1, -8, 0, 0), BAD_ARG, 0),
    ((N12, 0, 6, 4, 1, 0, -4, 0), BAD_ARG, 0),
    ((YUY, 0, 6, 4, 1, 0, 0, 1), UNSUPPORTED, 48),                           # packed + encode
    ((UYV, 2, 6, 4, 1, 0, 0, 1), UNSUPPORTED, 48),
    ((YUY, 0, 7, 4, 1, 0, 0, 1), BAD_ARG, 0),                                # a bad argument first
    ((6, 0, 6, 4, 1, 0, 0, 0), BAD_ARG, 0),                                  # unknown layout
    ((-1, 0, 6, 4, 1, 0, 0, 0), BAD_ARG, 0),
    ((N12, 3, 6, 4, 1, 0, 0, 0), BAD_ARG, 6 * 4 * 3 // 2),                   # unknown standard (the size has none)
    ((N12, -1, 6, 4, 1, 0, 0, 0), BAD_ARG, 6 * 4 * 3 // 2),
    ((N12, 0, 0, 4, 1, 0, 0, 0), BAD_ARG, 0),
    ((N12, 0, 6, 0, 1, 0, 0, 0), BAD_ARG, 0),
    ((N12, 0, 6, 4, 0, 0, 0, 0), BAD_ARG, 4 * 6 * 3 // 2),                   # no frames (the size has no count)
    ((N12, 0, 65536, 65536, 16, 0, 0, 0), BAD_ARG, 65536 * 65536 * 3 // 2),  # beyond what every call accepts
    ((N12, 0, 2, 2, 1, 1 << 30, 1 << 30, 0), BAD_ARG, 0),                    # a surface beyond 2^37 bytes
]


@pytest.mark.parametrize("args,code,nbytes", CHECKS)
def test_yuv_check_table(pkg, args, code, nbytes):
    layout, standard, w, h, n, pitch, rows, encode = args
    assert pkg.load_library().mi355_yuv_check(*args) == code
    assert pkg.yuv_check(layout, standard, w, h, n, pitch, rows, bool(encode)) == code
    assert pkg.yuv_frame_bytes(layout, w, h, pitch, rows) == nbytes
    if layout in yr.LAYOUTS and pitch < 2 ** 20:    # the reference knows the geometry rules, not the size limits
        assert yr.frame_bytes(layout, w, h, pitch, rows) == nbytes


def test_every_case_is_accepted_and_sized_as_the_reference_sizes_it(pkg):
    assert len(yc.SIZES) == 9
    for w, h in yc.SIZES:
        for layout in yr.LAYOUTS:
            geoms = yc.geometries(layout, w, h)
            assert len(geoms) == (12 if yr.is_planar(layout) else 15)
            for pitch, rows in geoms:
                for standard in yr.STANDARDS:
                    assert pkg.yuv_check(layout, standard, w, h, 3, pitch, rows) == OK, (layout, w, h, pitch, rows)
                    want = UNSUPPORTED if yr.is_packed(layout) else OK
                    assert pkg.yuv_check(layout, standard, w, h, 3, pitch, rows, True) == want
                assert pkg.yuv_frame_bytes(layout, w, h, pitch, rows) == yr.frame_bytes(layout, w, h, pitch, rows) > 0


# ---- the constants --------------------------------------------------------------------------------------------------
def _header_rows(name):
    """the two rows of integers the header's table has for a standard: decode (6), encode (8)"""
    text = open(HEADER).read()
    rows = re.findall(r"^ \*\s+%s\s+((?:-?\d+\s+)+-?\d+)\s*$" % name, text, flags=re.M)
    assert len(rows) == 2, (name, rows)
    dec, enc = ([int(v) for v in r.split()] for r in rows)
    assert len(dec) == 6 and len(enc) == 8
    return dict(zip(DEC_KEYS, dec)), dict(zip(ENC_KEYS, enc))


def _lround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _derived(kr, kb, sy, sc, yoff):
    """lround(c * 2^20) of the exact matrix of (Kr, Kb) with luma range factor sy and chroma range factor sc"""
    kg = 1.0 - kr - kb
    dec = dict(CY=1 / sy, CVR=2 * (1 - kr) / sc, CVG=-2 * kr * (1 - kr) / kg / sc, CUG=-2 * kb * (1 - kb) / kg / sc,
               CUB=2 * (1 - kb) / sc)
    enc = dict(CRY=kr * sy, CGY=kg * sy, CBY=kb * sy, CRU=-kr / (2 * (1 - kb)) * sc, CGU=-kg / (2 * (1 - kb)) * sc,
               CBU=0.5 * sc, CGV=-kg / (2 * (1 - kr)) * sc, CBV=-kb / (2 * (1 - kr)) * sc)
    dec = {k: _lround(v * 2 ** 20) for k, v in dec.items()}
    dec["YOFF"] = yoff
    return dec, {k: _lround(v * 2 ** 20) for k, v in enc.items()}


@pytest.mark.parametrize("name,std,kr,kb,sy,sc,yoff", [("BT709", yr.BT709, 0.2126, 0.0722, 219 / 255, 224 / 255, 16),
                                                       ("BT601_FULL", yr.BT601_FULL, 0.299, 0.114, 1.0, 1.0, 0)])
def test_the_derived_integers_of_the_header_are_those_of_kr_and_kb(name, std, kr, kb, sy, sc, yoff):
    dec, enc = _header_rows(name)
    want_dec, want_enc = _derived(kr, kb, sy, sc, yoff)
    assert dec == want_dec and enc == want_enc
    assert {k: yr.DECODE[std][k] for k in DEC_KEYS} == dec
    assert {k: yr.ENCODE[std][k] for k in ENC_KEYS} == enc and yr.ENCODE[std]["YOFF"] == yoff


def test_the_bt601_integers_are_opencvs_three_decimals():
    dec, enc = _header_rows("BT601")
    assert dec == dict(YOFF=16, CY=int(1.164 * 2 ** 20), CVR=int(1.596 * 2 ** 20), CVG=int(-0.813 * 2 ** 20),
                       CUG=int(-0.391 * 2 ** 20), CUB=int(2.018 * 2 ** 20))
    assert dec == dict(YOFF=16, CY=1220542, CVR=1673527, CVG=-852492, CUG=-409993, CUB=2116026)
    assert enc == dict(CRY=269484, CGY=528482, CBY=102760, CRU=-155188, CGU=-305135, CBU=460324, CGV=-385875, CBV=-74448)
    assert {k: yr.DECODE[yr.BT601][k] for k in DEC_KEYS} == dec
    assert {k: yr.ENCODE[yr.BT601][k] for k in ENC_KEYS} == enc


def test_every_constant_fits_a_24_bit_multiply_and_every_sum_an_int32():
    for std in yr.STANDARDS:
        d, e = yr.DECODE[std], yr.ENCODE[std]
        assert all(abs(d[k]) < 2 ** 23 for k in DEC_KEYS) and all(abs(e[k]) < 2 ** 23 for k in ENC_KEYS)
        top = 255 * d["CY"] + 2 ** 19 + 128 * max(abs(d["CVR"]), abs(d["CVG"]) + abs(d["CUG"]), abs(d["CUB"]))
        assert top < 2 ** 31
        rows = (("CRY", "CGY", "CBY"), ("CRU", "CGU", "CBU"), ("CBU", "CGV", "CBV"))
        assert all(255 * sum(abs(e[k]) for k in row) + 2 ** 19 + (128 << 20) < 2 ** 31 for row in rows)
    d = yr.DECODE[yr.BT601]
    assert 239 * d["CY"] + 2 ** 19 + 127 * d["CUB"] == 560969128    # the largest BT601 intermediate


# ---- the reference by hand ------------------------------------------------------------------------------------------
def _enc1(r, g, b, std=yr.BT601):
    y, u, v = yr.encode_planes(np.array([[[r, g, b, 9], [0, 0, 0, 0]], [[0, 0, 0, 0], [0, 0, 0, 0]]], np.uint8), std)
    return int(y[0, 0]), int(u[0, 0]), int(v[0, 0])


def _dec1(y, u, v, std=yr.BT601):
    px = yr.decode_planes(np.full((2, 2), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8), std)
    assert (px == px[0, 0]).all()
    return tuple(int(c) for c in px[0, 0])


def test_primaries_black_and_white_by_hand():
    assert _enc1(255, 0, 0) == (82, 90, 240)
    assert _enc1(0, 255, 0) == (145, 54, 34)
    assert _enc1(0, 0, 255) == (41, 240, 110)
    assert _enc1(0, 0, 0) == (16, 128, 128)       # (2^19 + (16 << 20)) >> 20
    assert _enc1(255, 255, 255) == (235, 128, 128)  # 900726 * 255 + 2^19 + 2^24 = 246986634 -> 235; chroma rows sum to 1
    assert _dec1(16, 128, 128) == (0, 0, 0, 255)
    assert _dec1(235, 128, 128) == (255, 255, 255, 255)  # 219 * 1220542 + 2^19 = 267822986 -> 255.4
    assert _dec1(0, 128, 128) == (0, 0, 0, 255)          # Y below YOFF: max(0, .)
    assert _dec1(126, 128, 128) == (128, 128, 128, 255)  # 110 * 1220542 + 2^19 = 134783908 -> 128.5


def test_one_saturating_triple_per_channel_and_direction_by_hand():
    # decode, by the formulas in plain integers: (Y, U, V) -> the channel before sat
    c = yr.DECODE[yr.BT601]

    def raw(y, u, v):
        yy = max(0, y - 16) * c["CY"] + 2 ** 19
        return ((yy + c["CVR"] * (v - 128)) >> 20, (yy + c["CVG"] * (v - 128) + c["CUG"] * (u - 128)) >> 20,
                (yy + c["CUB"] * (u - 128)) >> 20)

    assert raw(255, 128, 255) == (481, 175, 278) and _dec1(255, 128, 255) == (255, 175, 255, 255)   # R above
    assert raw(16, 128, 0)[0] == -204 and _dec1(16, 128, 0)[0] == 0                                 # R below
    assert raw(255, 0, 0)[1] == 432 and _dec1(255, 0, 0)[1] == 255                                  # G above
    assert raw(16, 255, 255)[1] == -153 and _dec1(16, 255, 255)[1] == 0                             # G below
    assert raw(255, 255, 128)[2] == 534 and _dec1(255, 255, 128)[2] == 255                          # B above
    assert raw(16, 0, 128)[2] == -258 and _dec1(16, 0, 128)[2] == 0                                 # B below
    # encode: BT601 and BT709 cannot saturate (their rows stay inside 16 .. 240); the full-range chroma does, above:
    # 524288 * 255 + 2^19 + 2^27 = 2^28 -> 256
    assert _enc1(0, 0, 255, yr.BT601_FULL) == (29, 255, 107)
    assert _enc1(255, 0, 0, yr.BT601_FULL) == (76, 85, 255)
    assert _enc1(255, 255, 255, yr.BT601_FULL) == (255, 128, 128)   # 2^20 * 255 + 2^19: exactly 255, not clamped
    assert _enc1(255, 255, 0, yr.BT601_FULL)[1] == 1                # -524288 * 255 + 2^19 + 2^27 = 2^20: nothing goes below 0


def test_alpha_is_ignored_and_the_chroma_is_the_top_left_pixel():
    a = np.array([[[255, 0, 0, 1], [0, 255, 0, 2]], [[0, 0, 255, 3], [255, 255, 255, 4]]], np.uint8)
    y, u, v = yr.encode_planes(a)
    assert y.tolist() == [[82, 145], [41, 235]] and u.tolist() == [[90]] and v.tolist() == [[240]]
    b = a.copy()
    b[..., 3] = 200
    assert all(np.array_equal(p, q) for p, q in zip(yr.encode_planes(b), (y, u, v)))


def test_the_gray_ramp_round_trip_stays_within_one():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 2, axis=0).repeat(4, axis=2)
    for layout in (yr.NV12, yr.I420):
        buf = yr.encode(ramp, layout)
        y, u, v = yr.unpack(buf[0], layout, 256, 2)
        assert (u == 128).all() and (v == 128).all()
        back = yr.decode(buf, 256, 2, layout)[0]
        assert np.abs(back[..., :3].astype(int) - ramp[..., :3].astype(int)).max() <= 1
        assert (back[..., 3] == 255).all()
        assert np.array_equal(yr.luma(buf, 256, 2, layout)[0], y)


def test_the_tight_layouts_byte_by_byte_on_a_4_x_4_frame():
    """OpenCV's (h * 3 / 2, w) CV_8UC1 matrix: 4 rows of Y, then 2 rows of chroma"""
    y = np.arange(16, dtype=np.uint8).reshape(4, 4)
    u = np.array([[100, 101], [102, 103]], np.uint8)
    v = np.array([[200, 201], [202, 203]], np.uint8)
    want = {yr.I420: [[100, 101, 102, 103], [200, 201, 202, 203]],
            yr.YV12: [[200, 201, 202, 203], [100, 101, 102, 103]],
            yr.NV12: [[100, 200, 101, 201], [102, 202, 103, 203]],
            yr.NV21: [[200, 100, 201, 101], [202, 102, 203, 103]]}
    for layout, chroma in want.items():
        m = yr.pack((y, u, v), layout).reshape(6, 4)
        assert np.array_equal(m[:4], y) and m[4:].tolist() == chroma, layout
        assert all(np.array_equal(a, b) for a, b in zip(yr.unpack(m, layout, 4, 4), (y, u, v)))
        assert yr.pixel_mask(layout, 4, 4).all()
    u2, v2 = np.arange(100, 108, dtype=np.uint8).reshape(4, 2), np.arange(200, 208, dtype=np.uint8).reshape(4, 2)
    assert yr.pack((y, u2, v2), yr.YUY2).reshape(4, 8)[1].tolist() == [4, 102, 5, 202, 6, 103, 7, 203]
    assert yr.pack((y, u2, v2), yr.UYVY).reshape(4, 8)[1].tolist() == [102, 4, 202, 5, 103, 6, 203, 7]


def test_a_pitched_surface_by_hand():
    """6 x 4 in a surface of pitch 8 and 6 rows: chroma starts at 48; planar planes have pitch 4 and 3 rows"""
    y = np.arange(24, dtype=np.uint8).reshape(4, 6)
    u = np.arange(100, 106, dtype=np.uint8).reshape(2, 3)
    v = np.arange(200, 206, dtype=np.uint8).reshape(2, 3)
    nv = yr.pack((y, u, v), yr.NV12, 8, 6, fill=0xEE)
    assert nv.size == 72 and nv[8 * 3 + 5] == 23 and nv[6] == nv[7] == 0xEE
    assert nv[48:54].tolist() == [100, 200, 101, 201, 102, 202] and nv[56:62].tolist() == [103, 203, 104, 204, 105, 205]
    pl = yr.pack((y, u, v), yr.I420, 8, 6, fill=0xEE)
    assert pl[48:51].tolist() == [100, 101, 102] and pl[52:55].tolist() == [103, 104, 105]
    assert pl[60:63].tolist() == [200, 201, 202] and pl[64:67].tolist() == [203, 204, 205]      # 48 + 4 * 3
    assert int(yr.pixel_mask(yr.I420, 6, 4, 8, 6).sum()) == 24 + 12 and (pl[~yr.pixel_mask(yr.I420, 6, 4, 8, 6)] == 0xEE).all()


# ---- the case list --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_branches():
    seen = set()
    for w, h in yc.SIZES:
        for packed in (False, True):
            for _, (y, u, v) in yc.decode_contents(w, h, packed):
                c = yr.DECODE[yr.BT601]
                uu = np.repeat(u, 2, axis=1).astype(np.int64) - 128
                vv = np.repeat(v, 2, axis=1).astype(np.int64) - 128
                if not packed:
                    uu, vv = np.repeat(uu, 2, axis=0), np.repeat(vv, 2, axis=0)
                if (y < c["YOFF"]).any():
                    seen.add("y_below_yoff")
                yy = np.maximum(0, y.astype(np.int64) - c["YOFF"]) * c["CY"] + yr.HALF
                raw = {"r": (yy + c["CVR"] * vv) >> 20, "g": (yy + c["CVG"] * vv + c["CUG"] * uu) >> 20,
                       "b": (yy + c["CUB"] * uu) >> 20}
                inside = np.ones(y.shape, bool)
                for ch, a in raw.items():
                    if (a < 0).any():
                        seen.add(ch + "_below_0")
                    if (a > 255).any():
                        seen.add(ch + "_above_255")
                    inside &= (a >= 0) & (a <= 255)
                if inside.any():
                    seen.add("no_saturation")
                if inside.mean() > 0.5:
                    seen.add("mostly_no_saturation")
    return seen


@pytest.mark.parametrize("branch", ["y_below_yoff", "r_below_0", "g_below_0", "b_below_0", "r_above_255", "g_above_255",
                                    "b_above_255", "no_saturation", "mostly_no_saturation"])
def test_the_decode_contents_reach(branch):
    assert branch in _decode_branches()


@functools.lru_cache(maxsize=None)
def _encode_values():
    ys, us, vs = set(), set(), set()
    for w, h in yc.SIZES:
        for _, rgba in yc.encode_contents(w, h):
            y, u, v = yr.encode_planes(rgba)
            ys |= set(y.ravel().tolist())
            us |= set(u.ravel().tolist())
            vs |= set(v.ravel().tolist())
    return ys, us, vs


@pytest.mark.parametrize("plane,value", [(0, 16), (0, 235), (1, 16), (1, 240), (2, 16), (2, 240)])
def test_the_encode_contents_reach(plane, value):
    assert value in _encode_values()[plane]


def test_a_mean_of_the_block_cannot_pass_for_the_top_left_sample():
    for w, h in yc.SIZES:
        rgba = dict(yc.encode_contents(w, h))["blocks"]
        mean = rgba.reshape(h // 2, 2, w // 2, 2, 4).mean(axis=(1, 3)).round().astype(np.uint8)
        mean = np.repeat(np.repeat(mean, 2, axis=0), 2, axis=1)
        _, u, v = yr.encode_planes(rgba)
        _, um, vm = yr.encode_planes(mean)
        assert not np.array_equal(u, um) and not np.array_equal(v, vm), (w, h)


def test_the_extremes_content_holds_every_listed_value():
    y, u, v = yc.extreme_planes(66, 34, False, 0)
    assert set(y.ravel().tolist()) == set(yc.Y_EXTREMES)
    assert set(u.ravel().tolist()) == set(v.ravel().tolist()) == set(yc.C_EXTREMES)
    assert len(set(zip(u.ravel().tolist(), v.ravel().tolist()))) == 36
