"""The distance transform (mi355_dist_*): the parts that need no GPU.

The header against the binding, the argument checks that come before any device work (mi355_dist_check is a pure host
function), the CPU reference tests/dist_ref.py against an all-pairs search with the tie rule stated directly, against
scipy and against hand-written answers, and the case list tests/dist_cases.py against what it claims to reach.  The GPU
behaviour is in test_gpu_dist.py.
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_cases as dc  # noqa: E402
import dist_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl-development-real-time-image-processing_amd", "csrc")
OK, BAD_ARG = 0, -1
SYMBOLS = ("mi355_dist_check", "mi355_dist_gray8_dev", "mi355_dist_gray8_batched")


# ---- interface ------------------------------------------------------------------------------------------------------
def test_header_and_binding_constants_agree(pkg):
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) +(\d+)\b", text)}
    assert d["MI355_MAX_DIST_DIM"] == pkg.MAX_DIST_DIM == dr.MAX_DIM == 16384
    assert d["MI355_DIST_NONE"] == pkg.DIST_NONE == dr.NONE == 2 ** 31 - 1
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert re.search(r"constexpr int kDistMaxDim = (\d+);", text).group(1) == str(pkg.MAX_DIST_DIM)


def test_the_three_symbols_are_declared_and_exported(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert callable(pkg.dist_check) and hasattr(pkg.Context, "dist_gray8") and hasattr(pkg.Context, "dist_gray8_dev")


def test_the_kernel_geometry_the_cases_assume_is_the_source_s():
    text = open(os.path.join(CSRC, "dist.hip")).read()
    lanes = int(re.search(r"constexpr int kDistColLanes = (\d+);", text).group(1))
    px = int(re.search(r"constexpr int kDistColPx = (\d+);", text).group(1))
    assert lanes * px == dc.COL_W
    assert re.search(r"constexpr int kDistChunk = (\d+);", text).group(1) == str(dc.CHUNK)
    assert re.search(r"constexpr int kDistMaxSegs = (\d+);", text).group(1) == str(dc.MAX_SEGS)
    assert re.search(r"constexpr int kDistLaneRange = (\d+);", text).group(1) == str(dc.LANE_RANGE)
    assert dc.ONE_CHUNK_ROWS == 2048


def test_a_null_context_or_pointer_is_a_bad_argument_without_a_gpu(pkg):
    lib = pkg.load_library()
    buf, out = (ctypes.c_uint8 * 4096)(), (ctypes.c_uint32 * 4096)()
    p_in, p_out = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    fake = ctypes.c_void_p(ctypes.addressof(out))  # never dereferenced: the pointer checks come first
    assert lib.mi355_dist_gray8_dev(None, p_in, p_out, None, None, 8, 8, 1) == BAD_ARG
    assert lib.mi355_dist_gray8_dev(fake, None, p_out, None, None, 8, 8, 1) == BAD_ARG
    assert lib.mi355_dist_gray8_dev(fake, p_in, None, None, None, 8, 8, 1) == BAD_ARG
    assert lib.mi355_dist_gray8_batched(None, ctypes.cast(buf, u8), p_out, None, None, 8, 8, 1, None) == BAD_ARG
    assert lib.mi355_dist_gray8_batched(fake, None, p_out, None, None, 8, 8, 1, None) == BAD_ARG
    assert lib.mi355_dist_gray8_batched(fake, ctypes.cast(buf, u8), None, None, None, 8, 8, 1, None) == BAD_ARG


CHECKS = [
    # (w, h, nframes)
    ((64, 48, 1), OK),
    ((1, 1, 1), OK),
    ((3840, 2160, 256), OK),
    ((16384, 2, 1), OK),
    ((2, 16384, 1), OK),
    ((16384, 16384, 1), OK),
    ((16385, 2, 1), BAD_ARG),
    ((2, 16385, 1), BAD_ARG),
    ((16385, 16385, 1), BAD_ARG),
    ((0, 48, 1), BAD_ARG),
    ((64, 0, 1), BAD_ARG),
    ((-1, 48, 1), BAD_ARG),
    ((64, -48, 1), BAD_ARG),
    ((64, 48, 0), BAD_ARG),
    ((64, 48, -1), BAD_ARG),
    ((16384, 16384, 1000), BAD_ARG),             # more pixels than any call of the library takes
]


@pytest.mark.parametrize("args,code", CHECKS)
def test_dist_check_returns_the_code_of_the_call(pkg, args, code):
    assert pkg.dist_check(*args) == code


# ---- the reference ----------------------------------------------------------------------------------------------------
def _m(rows):
    return np.array([[0 if c == "o" else 255 for c in r] for r in rows], np.uint8)


HAND = [
    # mask ('o' is a site), squared distances, nearest-site indices
    (["o....",
      ".....",
      "....."],
     [[0, 1, 4, 9, 16], [1, 2, 5, 10, 17], [4, 5, 8, 13, 20]],
     [[0] * 5] * 3),
    (["o...o",                                     # (2, y) ties left and right: the smaller column wins
      ".....",
      "o...o"],
     [[0, 1, 4, 1, 0], [1, 2, 5, 2, 1], [0, 1, 4, 1, 0]],
     [[0, 0, 0, 4, 4], [0, 0, 0, 4, 4], [10, 10, 10, 14, 14]]),   # row 1 ties above and below: the upper site wins
    ([".o...",
      "o....",
      "....."],
     [[1, 0, 1, 4, 9], [0, 1, 2, 5, 10], [1, 2, 5, 8, 13]],
     [[5, 1, 1, 1, 1], [5, 5, 1, 1, 1], [5, 5, 5, 1, 1]]),     # (0, 0), (1, 1) and (2, 2) tie: column 0 before column 1
    (["ooooo",
      "ooooo",
      "ooooo"],
     [[0] * 5] * 3,
     [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14]]),
]


@pytest.mark.parametrize("i", range(len(HAND)))
def test_the_reference_gives_the_hand_written_answers(i):
    rows, want_sq, want_near = HAND[i]
    for fn in (lambda m: tuple(a[0] for a in dr.dist_ref(m)), dr.all_pairs):
        sq, dist, near = fn(_m(rows))
        assert sq.dtype == np.int32 and dist.dtype == np.float32 and near.dtype == np.int32
        assert sq.tolist() == want_sq, sq.tolist()
        assert near.tolist() == want_near, near.tolist()
        assert np.array_equal(dist, np.sqrt(np.array(want_sq, np.float32)))


def test_the_reference_marks_a_frame_without_a_site_and_leaves_its_neighbours_alone():
    ms = np.stack([_m(["o....", ".....", "....."]), _m(["....."] * 3), _m(["....o", ".....", "....."])])
    sq, dist, near = dr.dist_ref(ms)
    assert (sq[1] == dr.NONE).all() and np.isposinf(dist[1]).all() and (near[1] == -1).all()
    assert sq[0].tolist() == HAND[0][1] and sq[2].tolist() == [r[::-1] for r in HAND[0][1]]
    assert (near[0] == 0).all() and (near[2] == 4).all()
    for a in dr.all_pairs(ms[1]):
        assert a.shape == (3, 5)
    assert (dr.all_pairs(ms[1])[0] == dr.NONE).all()


def test_the_float_output_rounds_the_integer_to_nearest_even_first():
    sq = np.array([2 ** 24 + 1, 2 ** 24 + 3, 16383 ** 2 + 1, 2 * 16383 ** 2], np.int32)
    f = sq.astype(np.float32)
    assert f.tolist() == [2.0 ** 24, 2.0 ** 24 + 4, 268402688.0, 536805376.0]
    assert np.sqrt(f).dtype == np.float32


@functools.lru_cache(maxsize=None)
def _ref(shape):
    named = dc.frames_of(shape)
    out = dr.dist_ref(np.stack([f for _, f in named]))
    return [(name, f, tuple(a[i] for a in out)) for i, (name, f) in enumerate(named)]


SMALL = [s for s in dc.SHAPES if s[0] * s[1] <= 67 * 48]


@pytest.mark.parametrize("shape", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_the_reference_equals_the_all_pairs_search_with_the_stated_tie_rule(shape):
    for name, f, (sq, dist, near) in _ref(shape):
        sq2, dist2, near2 = dr.all_pairs(f)
        assert np.array_equal(sq, sq2), (name, shape)
        assert np.array_equal(near, near2), (name, shape)
        assert np.array_equal(dist.view(np.uint32), dist2.view(np.uint32)), (name, shape)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=["%dx%d" % s for s in dc.SHAPES])
def test_the_reference_equals_scipy_on_every_case(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    w, h = shape
    for name, f, (sq, dist, near) in _ref(shape):
        if not (f == 0).any():
            assert (sq == dr.NONE).all() and (near == -1).all(), name    # scipy has no answer for a frame without a site
            continue
        d, idx = ndi.distance_transform_edt(f != 0, return_indices=True)
        assert np.array_equal(np.rint(d * d).astype(np.int64), sq.astype(np.int64)), (name, shape)
        # the nearest site: a site, at the stated distance, and scipy's wherever there is only one
        ny, nx = near // w, near % w
        yy, xx = np.mgrid[0:h, 0:w]
        assert (f[ny, nx] == 0).all() and np.array_equal((ny - yy) ** 2 + (nx - xx) ** 2, sq), (name, shape)
        if h * w <= 67 * 48:
            uniq = dr.unique_nearest(f)
            assert np.array_equal((idx[0] * w + idx[1])[uniq], near[uniq]), (name, shape)
        else:
            # scipy's own choice is at the same distance
            assert np.array_equal((idx[0] - yy) ** 2 + (idx[1] - xx) ** 2, sq), (name, shape)


# ---- the case list ----------------------------------------------------------------------------------------------------
def test_the_shapes_span_the_geometry_they_should():
    groups = {s: ((s[0] + dc.COL_W - 1) // dc.COL_W, (s[1] + dc.CHUNK - 1) // dc.CHUNK) for s in dc.SHAPES}
    assert groups[(1, 1)] == (1, 1) and groups[(5, 3)] == (1, 1)
    assert groups[(1, 300)][1] >= 2 and groups[(300, 1)][0] >= 2
    for s in ((67, 48), (250, 130), (130, 250)):
        assert groups[s][0] >= 2 and groups[s][1] >= 2 and s[0] % dc.COL_W and s[1] % dc.CHUNK and s[0] % 4, s
    assert (1030, 3) in dc.SHAPES and (3, 1030) in dc.SHAPES and 1030 > 1024 > dc.LANE_RANGE * 2
    # one chunk per segment up to ONE_CHUNK_ROWS rows, two from the next row on
    per_seg = {s: -(-groups[s][1] // dc.MAX_SEGS) for s in dc.SHAPES}
    assert per_seg[(9, dc.ONE_CHUNK_ROWS)] == 1 and per_seg[(9, dc.ONE_CHUNK_ROWS + 1)] == 2


def test_the_contents_reach_what_they_claim():
    by = {name: (f, out) for name, f, out in _ref((67, 48))}
    assert len(by) == len(dc.CONTENTS) >= 20
    assert not by["all_sites"][0].any() and (by["all_sites"][1][0] == 0).all()
    assert by["no_site"][0].all() and (by["no_site"][1][0] == dr.NONE).all()
    for name in ("site_top_left", "site_top_right", "site_bottom_left", "site_bottom_right", "site_middle"):
        assert (by[name][0] == 0).sum() == 1, name
    assert by["site_bottom_right"][1][0][0, 0] == 66 ** 2 + 47 ** 2       # the longest range a 67 x 48 frame has
    assert (by["left_column"][1][0] == (np.arange(67) ** 2)[None, :]).all()
    assert (by["right_column"][1][0] == (np.arange(67)[::-1] ** 2)[None, :]).all()
    assert (by["top_row"][1][0] == (np.arange(48) ** 2)[:, None]).all()
    assert (by["bottom_row"][1][0] == (np.arange(48)[::-1] ** 2)[:, None]).all()
    # ties: pixels with more than one nearest site, two and four of them
    for name in ("checkerboard", "lattice", "two_columns"):
        f = by[name][0]
        assert not dr.unique_nearest(f)[f != 0].all(), name
    f = by["lattice"][0]
    sy, sx = np.nonzero(f == 0)
    d2 = (4 - sy) ** 2 + (4 - sx) ** 2                                      # (4, 4): the centre of the cell of sites 1 and 7
    assert (d2 == d2.min()).sum() == 4 and by["lattice"][1][2][4, 4] == 1 * 67 + 1
    d2 = (1 - sy) ** 2 + (4 - sx) ** 2
    assert (d2 == d2.min()).sum() == 2 and by["lattice"][1][2][1, 4] == 1 * 67 + 1
    cols = np.flatnonzero((by["two_columns"][0] == 0).all(axis=0))
    assert len(cols) == 2 and (cols[1] - cols[0]) % 2 == 0
    mid = (cols[0] + cols[1]) // 2
    assert (by["two_columns"][1][2][:, mid] % 67 == cols[0]).all()         # the tie goes to the smaller column
    # columns without a site in frames that have sites
    for name in ("seventh_columns", "site_middle", "left_column", "noise_0.01"):
        f = by[name][0]
        assert (f == 0).any() and (f != 0).all(axis=0).any(), name
    f = by["seventh_columns"][0]
    assert set(np.flatnonzero((f == 0).any(axis=0)) % 7) == {3}
    for d in dc.DENSITIES:
        share = (by["noise_%g" % d][0] == 0).mean()
        assert abs(share - d) < 0.02, (d, share)
    vals = set(np.unique(by["other_values"][0]))
    assert {0, 1, 128} <= vals and 255 not in vals
    b = by["blobs"][0]
    assert 0.05 < (b != 0).mean() < 0.95 and by["blobs"][1][0].max() >= 9
    # the maximum-dimension closed form passes 2^24, where int32 -> float32 rounds
    sq = dc.corner_site_sq(2, 16384, 0, 0)
    assert sq.max() == 16383 ** 2 + 1 > 2 ** 24 and (sq.astype(np.float32).astype(np.int64) != sq).any()


def test_the_closed_form_frames_are_what_the_reference_says_on_a_small_size():
    h, w = 37, 90
    sq, _, near = dr.dist_ref(dc.border_sites(h, w))
    assert np.array_equal(sq[0], dc.border_sq(h, w))
    for y0, x0 in ((0, 0), (h - 1, w - 1)):
        m = dc.no_site(h, w)
        m[y0, x0] = 0
        sq, _, near = dr.dist_ref(m)
        assert np.array_equal(sq[0], dc.corner_site_sq(h, w, y0, x0)) and (near == y0 * w + x0).all()
