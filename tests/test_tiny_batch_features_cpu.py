"""What test_gpu_tiny_batch_features.py claims to reach, checked without a GPU and on the CPU references alone: that every
(feature, shape, parameters) row of tiny_feature_cases.py is accepted by the feature's argument check and fits the arena
budget at its count, that the frames of the odd shapes start at every alignment, and that the mask and response contents
are sensitive to a leak across a frame boundary: two neighbouring frames stacked as one raster (the model of a kernel
that takes the next frame's rows for its own) label, keep and count differently from the two frames on their own.
"""
import numpy as np
import pytest

import canny_cases as kc
import canny_ref as cr
import ccl_cases as cc
import hough_ref as hr
import tiny_batch_cases as tb
import tiny_feature_cases as tf
from box_ref import adaptive_ref
from ccl_ref import ccl_ref
from clahe_ref import clahe_ref, supported

FEATURES = list(tf.ROWS)


def _counts_in_use(pkg):
    return sorted({r.n for name in FEATURES for r in tf.ROWS[name](pkg)} | {64, 301})


# ---- the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FEATURES)
def test_every_row_is_accepted_and_fits_the_arena(pkg, name):
    rows = tf.ROWS[name](pkg)
    assert len(rows) >= tf.MIN_ROWS[name], "%s: a check refuses shapes it took before (%d rows)" % (name, len(rows))
    assert len(set((r.shape, r.params) for r in rows)) == len(rows)
    for r in rows:
        h, w = r.shape
        assert r.n in tb.TILE_COUNTS and r.n % 2 == 1 and r.n % 8 != 0
        assert tf.arena_bytes(r.n * h * w, r.n * r.out_bytes + 8) <= tf.ARENA_CAP, r
        bigger = [n for n in tb.TILE_COUNTS if n > r.n]
        assert all(tf.arena_bytes(n * h * w, n * r.out_bytes + 8) > tf.ARENA_CAP for n in bigger), r


def test_the_rows_hold_the_shapes_they_were_built_for(pkg):
    shapes = {name: tf.shapes_of(tf.ROWS[name](pkg)) for name in FEATURES}
    for name in ("adaptive", "ccl", "hysteresis", "canny"):
        assert set(tb.G8_SHAPES) <= set(shapes[name]), name
    assert tf.SEAM_SHAPE in shapes["ccl"] and tf.SEAM_SHAPE in shapes["hysteresis"] and tf.NMS_SHAPE in shapes["canny"]
    assert -(-tf.SEAM_SHAPE[1] // cc.TILE_W) * -(-tf.SEAM_SHAPE[0] // cc.TILE_H) == 4      # four tiles, their seams
    assert -(-tf.NMS_SHAPE[1] // kc.NMS_TW) * -(-tf.NMS_SHAPE[0] // kc.NMS_TH) == 4
    assert set(shapes["hough"]) == set(tf.hough_shapes()) >= {(1, 17), (3, 5), (5, 7), (13, 17), (1, 1)}
    assert all(h <= 13 and w <= 17 for h, w in shapes["hough"])
    grids = {g: [r.shape for r in tf.clahe_rows(pkg) if r.params == g] for g in tf.CLAHE_GRIDS}
    assert grids[1, 1] == list(tb.G8_SHAPES) and len(grids[2, 2]) >= 11 and len(grids[8, 8]) >= 7
    assert (5, 7) in grids[8, 8] and (13, 17) in grids[8, 8] and (75, 75) in grids[8, 8]   # 1-pixel tiles; padded both ways
    for g, ss in grids.items():                               # the check and the reference agree on what is served
        assert ss == [s for s in tb.G8_SHAPES if supported(s[1], s[0], g[0], g[1])], g


def test_counts_follow_the_arena_budget(pkg):
    """The int32 labels, the 8 x 8 CLAHE tables and the Hough accumulators are what the budget bites on: 16 KB of tables
    per frame, 19.6 KB of accumulator per 5 x 7 frame at theta = pi / 180, 45.9 KB per 13 x 17 frame."""
    assert tf.ARENA_CAP == tb.SLIDE_CAP == 16 << 20
    hough = {(r.shape, r.params): r for r in tf.hough_rows(pkg)}
    assert 4 * 182 * 27 == 19656 and 4 * 182 * 63 == 45864
    assert hough[(5, 7), tf.HOUGH_GEOMS[0]].out_bytes == 19656 + 12 * 64 + 4
    assert hough[(5, 7), tf.HOUGH_GEOMS[0]].n == 699 and hough[(13, 17), tf.HOUGH_GEOMS[0]].n == 301
    assert hough[(1, 1), tf.HOUGH_GEOMS[1]].n == hough[(3, 1), tf.HOUGH_GEOMS[1]].n == 3001
    ccl = {(r.shape, r.params): r for r in tf.ccl_rows(pkg)}
    assert ccl[(13, 17), (8, 4)].n == ccl[(16, 64), (8, 4)].n == 3001 and ccl[(32, 129), (8, 4)].n == 699
    assert ccl[(75, 75), (8, 4)].n == ccl[(75, 75), (4, 0)].n == 301 and ccl[tf.SEAM_SHAPE, (8, 4)].n == 699
    clahe = {(r.shape, r.params): r for r in tf.clahe_rows(pkg)}
    assert clahe[(13, 17), (8, 8)].n == 699 and clahe[(13, 17), (2, 2)].n == clahe[(16, 64), (1, 1)].n == 3001
    for name in ("adaptive", "hysteresis", "canny"):           # a byte in, a byte out: thousands up to 33 x 65
        assert all(r.n == (3001 if r.shape[0] * r.shape[1] <= 33 * 65 else 699) for r in tf.ROWS[name](pkg)), name


def test_odd_frame_sizes_start_at_every_residue(pkg):
    for name in FEATURES:
        for r in tf.ROWS[name](pkg):
            if r.shape in tb.ODD_SHAPES:
                h, w = r.shape
                assert tf.starts_mod(r.n, h * w) == set(range(16)), (name, r)           # inputs and 1-byte outputs
                assert tf.starts_mod(r.n, 4 * h * w) == {0, 4, 8, 12}, (name, r)        # int32 labels
    for (h, w), row in (((3, 5), 256), ((5, 7), 4 * 256)):    # CLAHE tables: 256 bytes per tile, frames stay aligned
        assert tf.starts_mod(3001, row) == {0}


# ---- the contents ------------------------------------------------------------------------------------------------------
def test_mask_members(pkg):
    for h, w in tf.shapes_of(tf.ccl_rows(pkg)):
        m = tf.mask_distinct(h, w)
        assert m.shape == (tb.NDISTINCT, h, w) and not m.flags.writeable
        for i in range(tb.NDISTINCT):
            flat = m[i].ravel()
            assert (flat[tf.corners(h, w)] != 0).all()
            values = set(flat[flat != 0].tolist())
            assert values <= ({255} if i % 2 == 0 else set(tf.FOREGROUND_VALUES)), (h, w, i)
        x = tf.mask_batch(h, w, 64)
        assert np.array_equal(x, m[tb.frame_index(64)])
    big = tf.mask_distinct(*tf.SEAM_SHAPE)
    for i in range(tb.P):                                      # the densities, within 5 % on 2145 pixels
        assert abs((big[i] != 0).mean() - cc.DENSITIES[i % 4]) < 0.05
    assert tf.corners(1, 1) == [0] and tf.corners(1, 17) == [0, 16] and tf.corners(3, 1) == [0, 2]
    assert tf.corners(3, 5) == [0, 4, 10, 14]


def test_a_link_across_any_frame_boundary_merges_two_components(pkg):
    """The stacked model: the corners are foreground, so the last row of a frame and the first row of the next touch in
    the first and the last column, and a labelling that links across the boundary counts fewer components."""
    pairs = tf.neighbour_pairs(_counts_in_use(pkg))
    assert len(pairs) >= 12 and (tb.FIRST, 1) in pairs and (10, 0) in pairs
    for h, w in tf.shapes_of(tf.ccl_rows(pkg)):
        m = tf.mask_distinct(h, w)
        for conn in cc.CONNECTIVITIES:
            own = ccl_ref(m, conn)[1] - 1                      # components per member (N counts the background)
            for a, b in pairs:
                both = int(ccl_ref(tf.stacked(m[a], m[b]), conn)[1][0]) - 1
                assert both < own[a] + own[b], (h, w, conn, a, b)


def test_a_strong_pixel_across_a_weak_frame_s_boundary_shows_in_it(pkg):
    """Weak frames have no strong pixel and an all-zero reference.  At every weak / strong boundary the stacked raster
    keeps pixels inside the weak frame: its corner candidates touch the strong corners of the other frame."""
    counts = _counts_in_use(pkg)
    pairs = tf.neighbour_pairs(counts)
    for h, w in tf.shapes_of(tf.hyst_rows(pkg)):
        r = tf.response_distinct(h, w)
        for i in range(tb.NDISTINCT):
            strong = tf.is_strong(i)
            assert bool((r[i] > kc.HIGH).any()) == strong and (r[i].ravel()[tf.corners(h, w)] > kc.LOW).all()
            assert set(np.unique(r[i]).tolist()) <= {kc.BG, kc.FG, kc.STRONG}
            for conn in cc.CONNECTIVITIES:
                assert bool(cr.hysteresis_ref(r[i], kc.LOW, kc.HIGH, conn).any()) == strong
        assert not cr.hysteresis_ref(r, kc.LOW, 255, 8).any()  # nothing exceeds 255
        for a, b in pairs:
            if tf.is_strong(a) == tf.is_strong(b):
                continue
            for conn in cc.CONNECTIVITIES:
                both = cr.hysteresis_ref(tf.stacked(r[a], r[b]), kc.LOW, kc.HIGH, conn)
                weak = both[:h] if tf.is_strong(b) else both[h:]
                assert weak.any(), (h, w, conn, a, b)


def test_one_boundary_per_cycle_is_between_two_weak_frames(pkg):
    """A condition on the inputs: 11 is odd, so one pair of neighbours of the cycle shares a class: member 10 next to
    member 0, both weak.  Every other boundary, the batch's two ends included, is between a weak and a strong frame."""
    cycle = [(i, (i + 1) % tb.P) for i in range(tb.P)]
    assert [p for p in cycle if tf.is_strong(p[0]) == tf.is_strong(p[1])] == [(10, 0)]
    assert not tf.is_strong(10) and not tf.is_strong(0) and not tf.is_strong(tb.FIRST)
    for n in _counts_in_use(pkg):
        idx = tb.frame_index(n).tolist()
        same = [(a, b) for a, b in zip(idx, idx[1:]) if tf.is_strong(a) == tf.is_strong(b)]
        assert set(same) <= {(10, 0)} and len(same) == sum(1 for f in range(1, n - 2) if f % tb.P == 10), n
        assert len(same) <= -(-n // tb.P)
        assert tf.is_strong(idx[1]) and not tf.is_strong(idx[0])
        assert tf.is_strong(idx[-1]) != tf.is_strong(idx[-2]), n
        weak = tf.weak_frames(n)
        assert weak[0] and not weak[1] and weak.sum() > n // 2


def test_point_counts_differ_between_the_frames_of_a_batch(pkg):
    """A per-frame Hough counter or list offset taken from another frame changes the accumulator only if the frames hold
    different numbers of points.  1 x 1, 1 x 2 and 2 x 1 are all corners: every frame is full."""
    for h, w in tf.hough_shapes():
        points = (tf.mask_distinct(h, w) != 0).reshape(tb.NDISTINCT, -1).sum(axis=1)
        if len(tf.corners(h, w)) == h * w:
            assert (points == h * w).all() and (h, w) in ((1, 1), (1, 2), (2, 1))
            continue
        assert len(set(points[:tb.P].tolist())) > 1, (h, w)
        differ = [points[a] != points[b] for a, b in tf.neighbour_pairs([64, 699, 3001])]
        assert any(differ), (h, w)


def test_a_vote_across_a_frame_boundary_changes_the_accumulator(pkg):
    """The stacked model for the votes: the points of the next frame, taken at rows h and below, land in other cells."""
    for h, w in ((3, 5), (13, 17)):
        m = tf.mask_distinct(h, w)
        for geom in tf.HOUGH_GEOMS:
            tc, ts = pkg.hough_trig_table(w, h, *geom)
            _, nr = pkg.hough_shape(w, h, *geom)
            for a, b in tf.neighbour_pairs([699, 3001]):
                assert not np.array_equal(hr.accum_ref(tf.stacked(m[a], m[b]), tc, ts, nr), hr.accum_ref(m[a], tc, ts, nr))


# ---- the references take every row -----------------------------------------------------------------------------------------
def test_the_references_take_every_row(pkg):
    for r in tf.clahe_rows(pkg):
        y = tb.distinct(r.shape[0], r.shape[1], 1)[3]
        assert clahe_ref(y, 2.0, *r.params).shape == r.shape
    for r in tf.adaptive_rows(pkg):
        y = tb.distinct(r.shape[0], r.shape[1], 1)[4]
        out = adaptive_ref(y, *r.params)
        assert out.shape == r.shape and set(np.unique(out).tolist()) <= {0, r.params[0]}
    for r in tf.canny_rows(pkg):
        assert cr.canny_ref(tb.distinct(r.shape[0], r.shape[1], 1)[5], *r.params).shape == r.shape
    for r in tf.hough_rows(pkg):
        h, w = r.shape
        na, nr = pkg.hough_shape(w, h, *r.params)
        assert (na, nr) == hr.shape(w, h, *r.params)
        tc, ts = pkg.hough_trig_table(w, h, *r.params)
        acc, lines, votes, count = hr.hough_ref(tf.mask_distinct(h, w)[:2], tc, ts, nr, 0, 7, *r.params[:3])
        assert acc.shape == (2, na + 2, nr + 2) and lines.shape == (2, 7, 2) and 4 * acc[0].size + 772 == r.out_bytes
        assert acc[0].sum() > 0
    one = tf.mask_distinct(1, 1)
    assert ccl_ref(one, 8, 4)[1].tolist() == [2] * tb.NDISTINCT


def test_selection_has_more_and_fewer_peaks_than_lines(pkg):
    """threshold 0 with 7 lines: every frame from 2 x 4 up has more peaks than lines, so the select runs in every frame's
    block; threshold 2 with 64 lines: every frame up to 3 x 5 (and some of 5 x 7) has fewer, so rows are zero-filled.
    The smallest frames have fewer than 7 peaks and 13 x 17 more than 64 under either: both sides of both."""
    (t0, m0), (t1, m1) = tf.HOUGH_SELECT
    for geom in tf.HOUGH_GEOMS:
        counts = {}
        for h, w in tf.hough_shapes():
            tc, ts = pkg.hough_trig_table(w, h, *geom)
            _, nr = pkg.hough_shape(w, h, *geom)
            m = tf.mask_distinct(h, w)
            more = hr.hough_ref(m, tc, ts, nr, t0, m0, geom[0], geom[1])
            few = hr.hough_ref(m, tc, ts, nr, t1, m1, geom[0], geom[1])
            counts[h, w] = (more[3], few[3])
            short = few[3] < m1
            assert not few[2][short][:, -1].any() and not few[1][short][:, -1].any()      # the zero fill
            assert (more[2][more[3] >= m0] > t0).all()
        for s in ((2, 4), (3, 5), (5, 7), (13, 17)):
            assert (counts[s][0] > m0).all(), s
        for s in ((1, 1), (1, 3), (2, 4), (3, 5)):
            assert (counts[s][1] < m1).all(), s
        assert (counts[5, 7][1] < m1).any() and (counts[13, 17][1] > m1).all() and (counts[1, 1][0] < m0).all()
