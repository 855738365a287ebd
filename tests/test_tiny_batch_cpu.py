"""What test_gpu_tiny_batch.py claims to reach, checked without a GPU: that every frame count of tiny_batch_cases.COUNTS
stands on the side of its launch-size rule it was chosen for (through the launch plans restated there from
slide_common.hpp, gauss.hip, gauss_slide.hip, gauss_wide.hip, gauss_exact.hip, sobel_slide.hip, pipe_slide.hip and
resize.hip), that the sources still hold the lines the restatement follows, what the batches contain, and that every CPU
reference takes every shape, one pixel included.  If a threshold, a band height or a strip width moves, a test here
fails and asks for new counts instead of the GPU suite silently standing on one side of the rule.
"""
import os

import numpy as np
import pytest

import resize_cases
import tiny_batch_cases as tb
from hist_ref import equalize_ref, hist_ref, otsu_ref, otsu_thresholds_ref
from median_ref import median_ref
from morph_ref import OPS, morph_ref
from resize_ref import AREA, LINEAR, NEAREST, accepts, resize_ref


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_every_shape_has_its_reason():
    assert tb.RGBA_SHAPES == ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 4), (3, 5), (5, 7), (13, 17), (9, 8), (7, 12),
                              (6, 252), (16, 64), (75, 75))
    assert tb.G8_SHAPES == tb.RGBA_SHAPES + ((4, 4), (1, 17), (1, 33), (32, 129))
    assert all(tb.G8_WHY[s] for s in tb.G8_SHAPES)
    assert set(tb.THRESHOLD_SHAPES) <= set(tb.RGBA_SHAPES) and set(tb.ODD_SHAPES) <= set(tb.RGBA_SHAPES)
    assert set(tb.COUNTS) == {(f, s) for f in tb.FAMILIES for s in tb.RGBA_SHAPES}
    assert (4 * 4, 1 * 17, 1 * 33, 32 * 129) == (16, 16 + 1, 32 + 1, 32 * (128 + 1))


@pytest.mark.parametrize("name,line", tb.SOURCE_LINES, ids=["%s:%d" % (n, i) for i, (n, _) in enumerate(tb.SOURCE_LINES)])
def test_the_sources_still_hold_the_restated_lines(name, line):
    text = " ".join(open(os.path.join(tb.CSRC, name)).read().split())
    assert " ".join(line.split()) in text, "%s no longer says `%s`: restate it in tiny_batch_cases.py and re-derive COUNTS" \
        % (name, line)


def test_strip_plans():
    assert tb.make_strip_plan(1) == (1, 1, 1) and tb.make_strip_plan(75) == (19, 1, 19)
    assert tb.make_strip_plan(248) == (62, 1, 62) and tb.make_strip_plan(252) == (63, 2, 32)
    assert tb.make_strip_plan(3840) == (960, 16, 60) and tb.make_strip_plan(3840, 48) == (960, 20, 48)


@pytest.mark.parametrize("family", tb.FAMILIES, ids=lambda f: "%s%d" % f)
def test_counts_stand_on_both_sides_of_the_2800_rule(family):
    """At n_hi the launch has at least 2800 work items of the production band height and takes that height; at
    n_lo = n_hi - 1 it has fewer and is left with the halved one.  Where the table gives no n_lo, either a tiled kernel
    serves the shape or no count below SLIDE_CAP reaches the production height."""
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        n_lo, n_hi = tb.counts(family, shape)
        key = tb.rows_key(family, w)
        hi = tb.launch_of(family, h, w, n_hi)
        assert h * w * 4 * n_hi <= tb.SLIDE_CAP, (family, shape)
        if n_lo is None:
            if hi.rows is None:
                assert hi.kernel in ("gauss_tile", "pipeline_tile") and n_hi == tb.tile_count(h, w, 4), (family, shape)
                assert h * w * 4 * n_hi <= tb.TILE_CAP and hi.nwork == n_hi * -(-w // 64) * -(-h // 16)
            else:
                top = tb.SLIDE_CAP // (h * w * 4)
                assert all(tb.launch_of(family, h, w, n).rows != tb.PRODUCTION_ROWS[key] for n in range(1, top + 1)), \
                    (family, shape)
            continue
        lo = tb.launch_of(family, h, w, n_lo)
        assert n_lo == n_hi - 1 and lo.kernel == hi.kernel and hi.rows is not None, (family, shape)
        assert hi.rows == tb.PRODUCTION_ROWS[key] and hi.nwork >= tb.SMALL_LAUNCH, (family, shape, hi)
        assert lo.rows == tb.HALVED_ROWS[key] and lo.rows < hi.rows, (family, shape, lo)
        # n_hi is the first such count: the height never falls as a batch grows
        assert all(tb.launch_of(family, h, w, n).rows == lo.rows for n in (1, 3, n_lo // 2)), (family, shape)


def test_the_counts_the_rules_give_for_the_named_shapes():
    c = tb.counts
    assert c(("gauss", 3), (75, 75)) == (399, 400)            # 7 bands of 12 rows
    assert c(("sobel", 0), (75, 75)) == (559, 560)            # 5 bands of 16 rows
    assert c(("gauss", 5), (75, 75)) == (699, 700)            # 4 bands of 24 rows
    assert c(("gauss", 5), (16, 64)) == (2799, 2800)
    assert c(("gauss", 3), (5, 7)) == c(("sobel", 0), (1, 1)) == c(("pipe", 7), (2, 4)) == (2799, 2800)
    # k = 5: the aligned kernel takes 15 rows from 2800 work items on, the ragged one keeps 24
    assert tb.launch_of(("gauss", 5), 16, 64, 2800) == ("gauss_slide", 15, 2 * 2800)
    assert tb.launch_of(("gauss", 5), 16, 64, 2799) == ("gauss_slide", 12, 2 * 2799)
    assert tb.launch_of(("gauss", 5), 75, 75, 700) == ("gauss_slide", 24, 4 * 700)
    assert tb.launch_of(("gauss", 5), 75, 75, 699) == ("gauss_slide", 12, 7 * 699)
    assert tb.launch_of(("gauss", 3), 75, 75, 400).rows == 12 and tb.launch_of(("gauss", 3), 75, 75, 399).rows == 6
    assert tb.launch_of(("sobel", 0), 75, 75, 560).rows == 16 and tb.launch_of(("sobel", 0), 75, 75, 559).rows == 8
    for k, rows in ((3, 16), (5, 24), (7, 40)):                # gauss_exact's and pipe_slide's own kRows
        assert tb.PRODUCTION_ROWS["exact", k] == tb.PRODUCTION_ROWS["pipe", k] == rows
        assert tb.HALVED_ROWS["exact", k] == tb.HALVED_ROWS["pipe", k] == rows // 2
        assert tb.launch_of(("exact", k), 16, 64, 2800) == ("gauss_exact", rows, 2800)
        assert tb.launch_of(("pipe", k), 16, 64, 2800) == ("pipe_slide", rows, 2800)


def test_sizes_stay_small():
    """The largest batch is 75 x 75 x 700 RGBA; the tiled kernels' batches stay below 4 MiB."""
    sizes = {(f, s): s[0] * s[1] * 4 * n for (f, s), (_, n) in tb.COUNTS.items()}
    assert max(sizes.values()) == 75 * 75 * 4 * 700 == 15750000
    assert sizes[("gauss", 5), (16, 64)] == 11468800
    over = sorted({s for (f, s), b in sizes.items() if b > tb.TILE_CAP})
    assert over == [(6, 252), (16, 64), (75, 75)], over
    for h, w in tb.G8_SHAPES:
        for bpp in (1, 4):
            n = tb.tile_count(h, w, bpp)
            assert n % 2 == 1 and n % tb.SLIDE_WAVES_PER_BLOCK and h * w * bpp * n <= tb.TILE_CAP
            assert n == 3001 or h * w * bpp * 3001 > tb.TILE_CAP
    assert tb.tile_count(5, 7, 1) == tb.tile_count(5, 7, 4) == tb.tile_count(13, 17, 4) == 3001 and tb.tile_count(32, 129, 1) == 699
    assert tb.tile_count(75, 75, 1) == 699 and tb.tile_count(75, 75, 4) == 101 and tb.tile_count(16, 64, 4) == 699


def test_tile_grids():
    assert tb.tile_grid(64, 16, 3001, 64, 16) == (1, 1, 3001) and tb.tile_grid(75, 75, 101, 64, 16) == (2, 5, 1010)
    assert tb.tile_grid(129, 32, 3001, 128, 32) == (2, 1, 6002)


# ---- the other launch-size rules -----------------------------------------------------------------------------------------
def test_matrix_core_rule_at_one_tile():
    h, w = tb.MATRIX_SHAPE
    n_lo, n_hi = tb.MATRIX_COUNTS
    assert (h, w) == tb.RGBA_TILE and w >= tb.MFMA_MIN_W and n_lo == n_hi - 1
    assert h * w * n_lo == 64512 < tb.MFMA_MIN_PIXELS == 65536 == h * w * n_hi
    for k in (7, 17):
        assert not tb.auto_takes_matrix_cores(h, w, n_lo, k) and tb.auto_takes_matrix_cores(h, w, n_hi, k)
    assert not tb.auto_takes_matrix_cores(h, w, n_hi, 5) and not tb.auto_takes_matrix_cores(75, 75, 700, 7)
    # the shapes wide enough for the matrix cores: 6 x 252 is past 2^16 pixels at both of its counts
    assert [s for s in tb.RGBA_SHAPES if s[1] >= tb.MFMA_MIN_W and s[1] % 4 == 0] == [(6, 252), (16, 64)]


@pytest.mark.parametrize("pair", tb.RESIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_resize_counts_stand_on_both_sides_of_4096(pair):
    sw, sh, dw, dh = pair
    n_lo, n_hi = tb.RESIZE_COUNTS
    rows_lo, work_lo = tb.resize_band_rows(dw, dh, n_lo)
    rows_hi, work_hi = tb.resize_band_rows(dw, dh, n_hi)
    assert n_lo == n_hi - 1 and rows_hi == tb.RESIZE_BAND_MAX == 16 and work_hi == n_hi >= tb.RESIZE_MIN_WORK
    assert rows_lo < rows_hi and n_lo < tb.RESIZE_MIN_WORK
    # the suite's other restatement, which reads the constants from resize.hip itself
    assert resize_cases.plan_constants() == (tb.RESIZE_STRIP, tb.RESIZE_BAND_MAX, tb.RESIZE_MIN_WORK)
    assert resize_cases.band_rows(dw, dh, n_lo) == rows_lo and resize_cases.band_rows(dw, dh, n_hi) == rows_hi
    assert max(sw * sh, dw * dh) * 4 * n_hi <= tb.TILE_CAP


def test_resize_pairs():
    assert {(7, 5, 4, 3), (1, 1, 3, 3), (4, 4, 2, 2), (8, 6, 2, 3)} <= set(tb.RESIZE_PAIRS)
    area = [p for p in tb.RESIZE_PAIRS if accepts(AREA, *p)]
    assert (4, 4, 2, 2) in area and (8, 6, 2, 3) in area and (12, 8, 6, 4) in area and len(area) >= 6
    assert all(accepts(i, *p) for i in (NEAREST, LINEAR) for p in tb.RESIZE_PAIRS)


# ---- what the batches hold ---------------------------------------------------------------------------------------------
def test_odd_frame_sizes_start_at_every_residue():
    for h, w in tb.ODD_SHAPES:
        for family in (("sobel", 0), ("pipe", 5)):
            n = tb.counts(family, (h, w))[1]
            starts = np.arange(n) * (h * w)                   # 1-byte outputs: frame f starts at f * h * w
            assert set(starts % 16) == set(range(16)) and set(starts % 4) == set(range(4)), (h, w)
    assert [h * w for h, w in tb.ODD_SHAPES] == [15, 35, 221]


@pytest.mark.parametrize("bpp", [4, 1])
def test_the_batch_cycles_through_eleven_frames(bpp):
    for (h, w), n in (((5, 7), 3001), ((1, 1), 2800), ((13, 17), 64), ((2, 4), 2799), ((75, 75), 101)):
        d, x, idx = tb.distinct(h, w, bpp), tb.batch(h, w, n, bpp), tb.frame_index(n)
        assert x.shape[0] == n and d.shape[0] == tb.NDISTINCT == 14 and len(set(idx.tolist())) == 13
        for f in range(1, n - 1):
            assert idx[f] == f % tb.P == f % 11
        assert np.array_equal(x[1:-1], d[np.arange(1, n - 1) % 11])
        assert idx[0] == tb.FIRST and idx[-1] in (tb.LAST_LOW, tb.LAST_HIGH)
        assert np.array_equal(x[0], d[tb.FIRST]) and np.array_equal(x[-1], d[idx[-1]])
        ranges = [tb.member_range(int(i)) for i in idx]
        assert all(a != b for a, b in zip(ranges, ranges[1:])), "adjacent frames share a range"
        colour = x[..., :3] if bpp == 4 else x
        for f in (0, 1, 2, 10, 11, n - 2, n - 1):
            lo, hi = ranges[f]
            assert lo <= colour[f].min() and colour[f].max() <= hi
    assert np.array_equal(tb.expand(np.arange(14), 25), tb.frame_index(25))


def test_member_ranges_and_alpha():
    r = [tb.member_range(i) for i in range(tb.P)]
    assert r[:10] == [tb.LOW, tb.HIGH] * 5 and r[10] == tb.MID and tb.LOW[1] < tb.HIGH[0]
    assert r[10] != r[9] and r[10] != r[0]                     # 11 is odd: the cycle's last member takes the third range
    d = tb.distinct(13, 17, 4)
    kinds = [tb.member_alpha(i) for i in range(tb.P)]
    assert set(kinds) == {tb.ALPHA_NOISE, tb.ALPHA_255, tb.ALPHA_77}
    for i, kind in enumerate(kinds):
        a = d[i, ..., 3]
        assert (kind == tb.ALPHA_255) == bool((a == 255).all()) and (kind == tb.ALPHA_77) == bool((a == 77).all())
    flat = tb.distinct(13, 17, 1).reshape(tb.NDISTINCT, -1)
    assert len({f.tobytes() for f in flat}) == tb.NDISTINCT
    assert not tb.distinct(1, 1, 1).flags.writeable


# ---- the references take every shape -------------------------------------------------------------------------------------
def test_the_oracle_takes_every_rgba_shape(oracle):
    for h, w in tb.RGBA_SHAPES:
        x = tb.distinct(h, w, 4)[0]
        assert oracle.gray_rgba(x).shape == (h, w, 4) and oracle.gray_rgba_1ch(x).shape == (h, w)
        assert oracle.sobel_rgba(x).shape == (h, w)
        for k, s in tb.SIGMA.items():
            assert oracle.gauss_rgba(x, k, s).shape == (h, w, 4)
        for k in (3, 5, 7):
            assert oracle.pipeline_rgba(x, k, tb.SIGMA[k]).shape == (h, w)
    one = tb.distinct(1, 1, 4)[0]
    for k, s in tb.SIGMA.items():                              # every tap clamps to the one pixel
        assert np.abs(oracle.gauss_rgba(one, k, s).astype(int) - one).max() <= 1
    assert oracle.sobel_rgba(one)[0, 0] == 0


def test_the_plane_references_take_every_gray8_shape(oracle):
    for h, w in tb.G8_SHAPES:
        y = tb.distinct(h, w, 1)
        assert oracle.sobel_gray(y[0]).shape == (h, w)
        assert hist_ref(y).shape == (tb.NDISTINCT, 256) and (hist_ref(y).sum(axis=1) == h * w).all()
        assert equalize_ref(y).shape == y.shape and otsu_ref(y).shape == y.shape
        assert otsu_thresholds_ref(y).shape == (tb.NDISTINCT,)
        for k in (3, 5, 7):
            assert median_ref(y[1], k).shape == (h, w) and median_ref(tb.distinct(h, w, 4)[1], k).shape == (h, w, 4)
        for op in OPS:
            for k in (3, 9, 17):
                assert morph_ref(op, y[2], k).shape == (h, w)
    for h, w in tb.RGBA_SHAPES:
        for op in OPS:
            assert morph_ref(op, tb.distinct(h, w, 4)[2], 17).shape == (h, w, 4)


def test_one_pixel_frames():
    """A one-pixel frame is its own median, minimum and maximum; it equalizes to itself and has threshold 0."""
    y = tb.distinct(1, 1, 1)
    for i in range(tb.NDISTINCT):
        assert median_ref(y[i], 7)[0, 0] == y[i, 0, 0]
        assert all(morph_ref(op, y[i], 17)[0, 0] == y[i, 0, 0] for op in OPS)
    assert np.array_equal(equalize_ref(y), y)
    assert (otsu_thresholds_ref(y) == 0).all()
    assert np.array_equal(otsu_ref(y), np.where(y > 0, 255, 0))


def test_resize_ref_takes_every_pair():
    for sw, sh, dw, dh in tb.RESIZE_PAIRS:
        for bpp in (4, 1):
            x = tb.distinct(sh, sw, bpp)[0]
            for interp in (NEAREST, LINEAR, AREA):
                if accepts(interp, sw, sh, dw, dh):
                    assert resize_ref(x, dw, dh, interp).shape == ((dh, dw, 4) if bpp == 4 else (dh, dw))
    one = tb.distinct(1, 1, 1)[3]
    assert (resize_ref(one, 3, 3, LINEAR) == one[0, 0]).all() and (resize_ref(one, 3, 3, NEAREST) == one[0, 0]).all()


# ---- the comparison ------------------------------------------------------------------------------------------------------
def test_a_stray_byte_names_its_frame():
    """What the GPU file relies on: in a payload prefilled 128 away from the reference, one byte stored into a
    neighbour's frame, or one byte never written, is a PayloadError whose index gives the frame, row and byte."""
    import guarded
    h, w, n = 5, 7, 3001
    ref = tb.batch(h, w, n, 1)
    for f, y, x in ((0, 0, 0), (1500, 4, 6), (n - 1, 4, 6)):
        got = ref.copy()
        got[f, y, x] = guarded.prefill_of(ref)[f, y, x]       # never written
        with pytest.raises(guarded.PayloadError) as e:
            guarded.check(got, ref, 1)
        assert e.value.unwritten == 1 and e.value.index == (f * h + y) * w + x
        assert tb.where(e.value.index, h * w, w).startswith("frame %d row %d byte %d " % (f, y, x))
    got = ref.copy()
    got[1501, 0, :4] = got[1500, 4, 3:]                       # a 4-byte store that ran 4 bytes past frame 1500's end
    with pytest.raises(guarded.PayloadError) as e:
        guarded.check(got, ref, 1)
    assert tb.where(e.value.index, h * w, w).startswith("frame 1501 row 0 byte 0 ") and e.value.unwritten == 0
