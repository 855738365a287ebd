"""The Hough line transform (mi355_hough_*): the parts that need no GPU.

The header against the binding, the argument checks that come before any device work (mi355_hough_check, _shape,
_trig_table, _accum_bytes and _plan are pure host functions), the CPU reference tests/hough_ref.py against a per-pixel
transcription of the header and against closed forms, and the case list tests/hough_cases.py against what it claims to
reach.  The GPU behaviour is in test_gpu_hough.py.
"""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hough_cases as hc  # noqa: E402
import hough_ref as hr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG = 0, -1
PI = math.pi
SYMBOLS = ("mi355_hough_check", "mi355_hough_shape", "mi355_hough_trig_table", "mi355_hough_accum_bytes",
           "mi355_hough_plan", "mi355_hough_accum_gray8_dev", "mi355_hough_lines_gray8_dev",
           "mi355_hough_lines_gray8_batched")


# ---- interface ------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_and_exported_without_a_gpu(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def test_header_and_binding_constants_agree(pkg):
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MI355_\w+) (\d+)\b", text)}
    assert d["MI355_MAX_HOUGH_ANGLES"] == pkg.MAX_HOUGH_ANGLES == 1024
    assert d["MI355_MAX_HOUGH_LINES"] == pkg.MAX_HOUGH_LINES == 4096


def test_the_header_names_what_it_is_and_what_it_does_not_offer():
    text = open(os.path.join(ROOT, "include", "mi355_imgfilter.h")).read()
    sec = text[text.index("from edges to lines"):text.index("#define MI355_MAX_HOUGH_ANGLES")]
    flat = " ".join(sec.replace("*", " ").split())
    assert "restated from memory of OpenCV's HoughLinesStandard" in flat
    assert "nobody has compared it with an OpenCV build here" in flat
    for name in ("HoughLinesP", "srn / stn", "HoughLinesPointSet", "use_edgeval", "row pitch and ROI", "streamed, group",
                 "mi355_pool_alloc"):
        assert name in flat, name


INF, NAN = float("inf"), float("nan")
W, H = 64, 48
#          w, h, nframes, rho, theta, threshold, max_lines, min_theta, max_theta
GOOD = dict(w=W, h=H, nframes=1, rho=1.0, theta=PI / 180, threshold=10, max_lines=16, min_theta=0.0, max_theta=PI)
ORDER = ("w", "h", "nframes", "rho", "theta", "threshold", "max_lines", "min_theta", "max_theta")
# each rule of the header: (what is refused, its nearest accepted neighbour)
CHECKS = [
    (dict(w=0), dict(w=1)),
    (dict(w=32767), dict(w=32766)),                      # MI355_MAX_WARP_SIZE
    (dict(h=0), dict(h=1)),
    (dict(h=32767, theta=PI / 7), dict(h=32766, theta=PI / 7)),
    (dict(nframes=0), dict(nframes=1)),
    (dict(rho=0.0), dict(rho=1.0e-3)),
    (dict(rho=-1.0), dict(rho=1.0)),
    (dict(rho=NAN), dict(rho=0.5)),
    (dict(rho=INF), dict(rho=100.0)),
    (dict(rho=1.0e-60), dict(rho=1.0e-3)),               # positive as a double, zero as a float
    (dict(theta=0.0), dict(theta=PI / 1023)),
    (dict(theta=-0.1), dict(theta=0.1)),
    (dict(theta=NAN), dict(theta=1.0)),
    (dict(theta=INF), dict(theta=4.0)),                  # one angle
    (dict(min_theta=-1.0e-9), dict(min_theta=0.0)),
    (dict(max_theta=np.nextafter(PI, 4.0)), dict(max_theta=PI)),       # no slack above M_PI
    (dict(min_theta=1.0, max_theta=np.nextafter(1.0, 0.0)), dict(min_theta=1.0, max_theta=1.0)),
    (dict(min_theta=NAN), dict(min_theta=0.5)),
    (dict(max_theta=NAN), dict(max_theta=0.5)),
    (dict(theta=PI / 1024.75), dict(theta=PI / 1024.25)),              # numangle 1025 and 1024 = MI355_MAX_HOUGH_ANGLES
    (dict(rho=2.0 * (2 * (W + H) + 1)), dict(rho=2.0 * (2 * (W + H) + 1) - 1.0)),   # numrho 0 (0.5 goes to even) and 1
    # an accumulator of 2^31 bytes per frame: (numangle + 2) * (numrho + 2) * 4 with numangle 1024 = 1026 rows, so
    # numrho + 2 >= 523 266 (4104 * 523 265 < 2^31 <= 4104 * 523 266).  At w = h = 32766 numrho = cvRound(131065 / rho)
    (dict(w=32766, h=32766, theta=PI / 1024.25, rho=131065.0 / 523264.0),
     dict(w=32766, h=32766, theta=PI / 1024.25, rho=131065.0 / 523263.0)),
    (dict(threshold=-1), dict(threshold=0)),
    (dict(max_lines=0), dict(max_lines=1)),
    (dict(max_lines=4097), dict(max_lines=4096)),
]


@pytest.mark.parametrize("bad,good", CHECKS, ids=[",".join(sorted(b)) + str(i) for i, (b, _) in enumerate(CHECKS)])
def test_hough_check_refuses_each_rule_and_accepts_its_neighbour(pkg, bad, good):
    assert pkg.hough_check(**GOOD) == OK
    assert pkg.hough_check(**dict(GOOD, **good)) == OK, good
    assert pkg.hough_check(**dict(GOOD, **bad)) == BAD_ARG, bad


def test_the_accumulator_limit_case_is_the_one_it_claims(pkg):
    bad, good = CHECKS[21]
    for kw, over in ((bad, True), (good, False)):
        na, nr = hr.shape(kw["w"], kw["h"], kw["rho"], kw["theta"])
        assert na == 1024 and ((na + 2) * (nr + 2) * 4 >= 2 ** 31) == over, (na, nr)
    assert pkg.hough_accum_bytes(bad["w"], bad["h"], 1, bad["rho"], bad["theta"]) == 0
    na, nr = hr.shape(good["w"], good["h"], good["rho"], good["theta"])
    assert pkg.hough_accum_bytes(good["w"], good["h"], 3, good["rho"], good["theta"]) == 3 * (na + 2) * (nr + 2) * 4


def test_a_null_context_or_pointer_is_a_bad_argument_without_a_gpu(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 65536)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    vp, u8 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8)
    tail = (8, 8, 1, 1.0, PI / 180)
    assert lib.mi355_hough_accum_gray8_dev(None, vp(p), vp(p + 4096), *tail, 0.0, PI) == BAD_ARG
    assert lib.mi355_hough_lines_gray8_dev(None, vp(p), vp(p + 4096), vp(p + 8192), vp(p + 12288), None, *tail, 1, 4, 0.0,
                                           PI) == BAD_ARG
    assert lib.mi355_hough_lines_gray8_batched(None, ctypes.cast(buf, u8), vp(p + 4096), vp(p + 8192), vp(p + 12288), *tail,
                                               1, 4, 0.0, PI, None) == BAD_ARG
    f32 = ctypes.POINTER(ctypes.c_float)
    assert lib.mi355_hough_trig_table(8, 8, 1.0, PI / 180, 0.0, PI, None, ctypes.cast(buf, f32)) == BAD_ARG
    assert lib.mi355_hough_trig_table(8, 8, 1.0, PI / 180, 0.0, PI, ctypes.cast(buf, f32), None) == BAD_ARG


# ---- shape and table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hc.SHAPES + [(3840, 2160), hc.BIG["shape"]], ids=lambda s: "%dx%d" % s)
def test_the_shape_is_the_reference_s_on_the_parameter_grid(pkg, shape):
    w, h = shape
    for rho, theta, lo, hi in hc.SHAPE_GRID:
        want = hr.shape(w, h, rho, theta, lo, hi)
        if want[1] < 1:
            assert pkg.hough_check(w, h, 1, rho, theta, 0, 1, lo, hi) == BAD_ARG
            continue
        assert pkg.hough_shape(w, h, rho, theta, lo, hi) == want, (shape, rho, theta, lo, hi)


def test_known_shapes():
    assert hr.shape(3840, 2160, 1.0, PI / 180) == (180, 12001)
    assert hr.shape(64, 64, 1.0, PI / 7) == (7, 257)          # floor(7) + 1 = 8, and pi - 7 theta = 0 takes one off
    assert hr.shape(64, 64, 1.0, PI) == (1, 257)              # 2 angles, then one off
    assert hr.shape(64, 64, 1.0, PI / 180, 0.3, 2.1)[0] == int(math.floor(1.8 / (PI / 180))) + 1
    assert hr.shape(1, 1, 2.0, PI)[1] == 2                    # 2.5 rounds half to even
    assert hr.shape(1, 2, 2.0, PI)[1] == 4                    # 3.5 too
    assert hr.shape(*hc.BIG["shape"], *hc.BIG["params"]) == (8, 32)


@pytest.mark.parametrize("params", hc.PARAMS + [hc.BIG["params"]], ids=str)
def test_the_trig_table_is_within_one_ulp_of_numpy_s(pkg, params):
    """The bound is 1 ulp, not 0: the library's table comes from the C library's cos and sin and the reference's from
    numpy's, two libms that may round the last bit of a double differently; that bit can move the fp32 result of the
    product by one place and no further.  The GPU tests take the library's table, so this is the only place the two meet."""
    rho, theta, lo, hi = params
    na, _ = hr.shape(64, 64, rho, theta, lo, hi)
    tc, ts = pkg.hough_trig_table(64, 64, rho, theta, lo, hi)
    rc, rs = hr.trig_table(na, rho, theta, lo)
    assert tc.shape == ts.shape == (na,)
    assert int(hr.ulp_distance(tc, rc).max()) <= 1 and int(hr.ulp_distance(ts, rs).max()) <= 1
    assert np.array_equal(tc[:1], np.array([np.cos(np.float64(np.float32(lo))) / np.float32(rho)], np.float32))


def test_the_plan_and_the_boundary_shapes(pkg):
    angles, splits, cells = pkg.hough_plan(3840, 2160, *hc.DEFAULT)
    assert cells * 4 <= 160 * 1024 and splits == 1 and angles == cells // 12001 >= 1
    plans = {tag: (hr.shape(*s, *hc.DEFAULT)[1],) + pkg.hough_plan(*s, *hc.DEFAULT) for tag, s in hc.boundary_shapes(pkg)}
    assert plans["fits_lds"][0] <= cells < plans["split_2"][0] and plans["fits_lds"][1:3] == (1, 1)
    assert plans["split_2"][1:3] == (1, 2) and plans["3x20000"][1:3] == (1, 2) and plans["3x20000"][0] == 40007
    small = hc.small_cells()
    assert plans["small_8"][1] == plans["large_8"][1] == 8
    assert 8 * plans["small_8"][0] <= small < 8 * plans["large_8"][0]
    assert plans["four_rows"][1] == 4
    for s in hc.SHAPES:                                   # the small shapes: whole rows, 8 (or all) angles per block
        for p in hc.PARAMS:
            na, nr = hr.shape(*s, *p)
            assert pkg.hough_plan(*s, *p)[:2] == (min(8, na, cells // nr), 1)


# ---- the reference against itself -----------------------------------------------------------------------------------
def _table(shape, params):
    rho, theta, lo, hi = params
    na, nr = hr.shape(*shape, rho, theta, lo, hi)
    return hr.trig_table(na, rho, theta, lo) + (nr,)


@pytest.mark.parametrize("shape", hc.LITERAL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_vectorised_reference_equals_the_per_pixel_transcription(shape):
    for params in hc.PARAMS:
        tc, ts, nr = _table(shape, params)
        for name, f in hc.frames_of(shape):
            acc = hr.accum_ref(f, tc, ts, nr)
            assert np.array_equal(acc, hr.accum_literal(f, tc, ts, nr)), (name, params)
            assert not acc[0].any() and not acc[-1].any() and not acc[:, 0].any() and not acc[:, -1].any()
            assert int(acc.sum()) == int((f != 0).sum()) * len(tc)          # no vote is dropped at these rho
            for thr in (0, 1, 3):
                assert np.array_equal(hr.peaks_ref(acc, thr), hr.peaks_literal(acc, thr)), (name, params, thr)


def test_the_order_is_votes_descending_then_cell_ascending():
    tc, ts, nr = _table((63, 65), hc.DEFAULT)
    acc = hr.accum_ref(hc.noise(65, 63, 0.10), tc, ts, nr)
    lines, votes, count = hr.lines_ref(acc, 2, 4096, 1.0, PI / 180)
    m = min(count, 4096)
    assert m > 100 and (votes[:m] > 2).all() and not votes[m:].any() and not lines[m:].any()
    assert (np.diff(votes[:m]) <= 0).all() and len(set(votes[:m].tolist())) < m        # ties exist ...
    n = np.rint(lines[:m, 1] / np.float32(PI / 180)).astype(np.int64)
    r = np.rint(lines[:m, 0] + np.float32((nr - 1) * 0.5)).astype(np.int64)
    cell = (n + 1) * (nr + 2) + r + 1
    assert np.array_equal(acc.ravel()[cell], votes[:m])
    tied = np.diff(votes[:m]) == 0
    assert (np.diff(cell)[tied] > 0).all()                                               # ... and go by cell index
    # max_lines cuts the same list short
    l7, v7, c7 = hr.lines_ref(acc, 2, 7, 1.0, PI / 180)
    assert c7 == count and np.array_equal(l7, lines[:7]) and np.array_equal(v7, votes[:7])


# ---- closed forms ---------------------------------------------------------------------------------------------------
def test_a_full_width_horizontal_line():
    w, h = 130, 67
    tc, ts, nr = _table((w, h), hc.DEFAULT)
    for c in (0, 20, h - 1):
        f = np.zeros((h, w), np.uint8)
        f[c] = 255
        lines, votes, count = hr.lines_ref(hr.accum_ref(f, tc, ts, nr), w // 2, 8, 1.0, PI / 180)
        assert count >= 1 and votes[0] == w                         # every pixel of the line in one cell
        assert abs(float(lines[0, 1]) - PI / 2) <= PI / 180         # within one step of pi / 2
        assert abs(float(lines[0, 0]) - c) <= 1.0                   # within rho_f of c


def test_one_pixel_at_threshold_zero():
    for shape in ((9, 1), (5, 4), (64, 64)):
        w, h = shape
        tc, ts, nr = _table(shape, hc.DEFAULT)
        f = hc.one_pixel(h, w)
        acc = hr.accum_ref(f, tc, ts, nr)
        inner = acc[1:-1, 1:-1]
        assert (inner.sum(axis=1) == 1).all() and inner.max() == 1  # one cell with one vote in every angle row
        r = inner.argmax(axis=1)
        # what the asymmetric rule leaves: the angle row above must hold its vote elsewhere (>), the one below may hold it
        # in the same column (>=), so of a vertical run of equal columns only the first row survives
        want = [n for n in range(len(r)) if n == 0 or r[n - 1] != r[n]]
        got = hr.peaks_ref(acc, 0)
        assert [int(b) // (nr + 2) - 1 for b in got] == want
        assert len(got) == len(hr.peaks_literal(acc, 0)) == hr.lines_ref(acc, 0, 1, 1.0, PI / 180)[2]
        assert 1 <= len(got) <= len(r)


def test_a_frame_and_its_transpose_need_not_give_mirrored_peaks():
    """(x, y) -> (y, x) maps the line (rho, theta) to (rho, pi / 2 - theta) for theta <= pi / 2.  With theta = pi / 4 the
    table has angles 0, pi / 4, pi / 2, 3 pi / 4, and a two-pixel frame shows the peak sets are not mirror images."""
    f = np.zeros((3, 3), np.uint8)
    f[0, 1] = f[2, 1] = 255                     # two pixels in a column
    tc, ts, nr = _table((3, 3), (1.0, PI / 4, 0.0, PI))
    peaks = []
    for g in (f, f.T.copy()):
        acc = hr.accum_ref(g, tc, ts, nr)
        b = hr.peaks_ref(acc, 0)
        peaks.append(sorted((int(x) // (nr + 2) - 1, int(x) % (nr + 2) - 1 - (nr - 1) // 2) for x in b))
    mirrored = sorted((2 - n, r) for n, r in peaks[0] if n <= 2)
    assert mirrored != sorted(p for p in peaks[1] if p[0] <= 2), peaks


# ---- the cases reach what they claim ----------------------------------------------------------------------------------
def test_the_big_case_passes_65535_votes_in_one_cell():
    w, h = hc.BIG["shape"]
    rho, theta, lo, hi = hc.BIG["params"]
    na, nr = hr.shape(w, h, rho, theta, lo, hi)
    acc = hr.accum_ref(hc.full(h, w), *hr.trig_table(na, rho, theta, lo), nr)
    assert int(acc.max()) > 65535 and int(acc.sum()) == w * h * na


def test_the_contents_reach_what_they_claim():
    named = dict(hc.frames_of((130, 67)))
    dens = {k: float((v != 0).mean()) for k, v in named.items()}
    assert dens["empty"] == 0 and dens["full"] == 1 and int((named["one_pixel"] != 0).sum()) == 1
    assert 0.005 < dens["noise_1"] < 0.02 and 0.08 < dens["noise_10"] < 0.12 and 0.45 < dens["noise_50"] < 0.55
    assert 0.01 < dens["canny"] < 0.5 and set(np.unique(named["canny"])) == {0, 255}
    assert len(np.unique(named["noise_50"])) > 200              # nonzero means any value but 0
    tc, ts, nr = _table((130, 67), hc.DEFAULT)
    acc = hr.accum_ref(named["lines"], tc, ts, nr)
    assert int(acc.max()) == 130                                 # the drawn row
    # run aggregation meets both kinds of angle: near pi / 2 a row's pixels share a cell, near 0 they never do
    assert abs(tc[90]) < 0.5 < abs(tc[0])
    # the selection cases: more peaks than max_lines at threshold 0, fewer at a high threshold
    acc = hr.accum_ref(named["noise_10"], tc, ts, nr)
    assert len(hr.peaks_ref(acc, 0)) > 4096 and 0 < len(hr.peaks_ref(acc, 24)) < 7
