"""The inputs of test_gpu_resize_walk.py, checked without a GPU: they reach what they claim to reach.

tests/resize_cases.py mirrors the band plan of csrc/resize.hip to choose batch sizes, and builds index frames and AREA
blocks.  None of that is an oracle for a pixel, so it is checked here: the plan's constants are read from the source, the
existing GPU shapes are shown to run one row per band (the gap the walk tests close), each walk case reaches each band
height, the row cache is exercised in all its classes inside a band, a wrong scale or an fp32 coordinate changes the
sweep's own output bytes, and the AREA blocks hold the sums on which the two roundings differ.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc  # noqa: E402
import test_gpu_resize as existing  # noqa: E402
from resize_ref import AREA, LINEAR, NEAREST, area_byte, linear_cols, resize_ref  # noqa: E402


# ---- band plan and existing shapes ------------------------------------------------------------------------------------
def test_band_rows_reads_its_constants_from_the_source(tmp_path):
    assert rc.plan_constants() == (256, 16, 4096)
    text = open(rc.RESIZE_HIP).read()
    for name in ("kResizePx", "kResizeBandMax", "kResizeMinWork", "kResizeStrip"):
        gone = tmp_path / (name + ".hip")
        gone.write_text(text.replace("constexpr int %s =" % name, "constexpr int x%s =" % name)
                        .replace("constexpr size_t %s =" % name, "constexpr size_t x%s =" % name))
        try:
            rc.plan_constants(str(gone))
        except AssertionError as e:
            assert name in str(e)
        else:
            raise AssertionError("a source without %s was accepted" % name)
    # the rule itself, by hand: 64 x 48 has 1 strip; 16 rows -> 3 bands, so 1366 frames reach 4096 and 1365 do not
    assert rc.band_rows(64, 48, 1366) == 16 and rc.band_rows(64, 48, 1365) == 8
    assert rc.band_rows(64, 48, 1) == 1 and rc.band_rows(257, 1, 10 ** 6) == 16 and rc.band_rows(256, 4096, 1) == 1
    assert rc.band_rows(256, 4097, 1) == 1 and rc.band_rows(256, 8192, 1) == 2


def test_the_existing_gpu_shapes_run_one_row_per_band():
    """What test_gpu_resize.py reaches of the band walk: one row per band everywhere but two 4K cases."""
    for sw, sh, dw, dh in existing.SHAPES:
        assert rc.band_rows(dw, dh, 1) == 1, (sw, sh, dw, dh)
    for shapes in existing.GUARDED_SHAPES.values():
        for sw, sh, dw, dh in shapes:
            assert rc.band_rows(dw, dh, 1) == 1, (sw, sh, dw, dh)
    # test_frames_are_independent (3 and 6 frames) and test_host_call_equals_device_call_and_profiles (2 frames)
    for dw, dh in ((33, 19), (64, 48)):
        assert rc.band_rows(dw, dh, 3) == 1 and rc.band_rows(dw, dh, 6) == 1
    for dw, dh in ((200, 19), (97, 151), (64, 60)):
        assert rc.band_rows(dw, dh, 2) == 1
    want = {(3840, 2160, 1280, 720): 1, (3840, 2160, 1920, 1080): 2, (1920, 1080, 3840, 2160): 4}
    assert {s: rc.band_rows(s[2], s[3], 1) for s in existing.LARGE} == want


# ---- band-walk cases --------------------------------------------------------------------------------------------------
def test_every_walk_case_reaches_every_band_height():
    for sw, sh, dw, dh in rc.WALK_CASES + rc.AREA_WALK_CASES:
        counts = [rc.frames_for(dw, dh, r) for r in rc.BAND_HEIGHTS]
        assert [rc.band_rows(dw, dh, n) for n in counts] == list(rc.BAND_HEIGHTS), (dw, dh, counts)
        assert counts == sorted(counts) and len(set(counts)) == 4
        assert all(n >= 2 * rc.NDISTINCT for n in counts)               # every distinct frame runs at least twice
    assert [rc.frames_for(64, 48, r) for r in rc.BAND_HEIGHTS] == [171, 342, 683, 1366]
    assert [rc.frames_for(520, 45, r) for r in rc.BAND_HEIGHTS] == [60, 114, 228, 456]
    for interp, cases in rc.GUARDED_WALK.items():
        for rows, (sw, sh, dw, dh) in cases:
            assert (sw, sh, dw, dh) in rc.walk_cases(interp)
            bpp_bytes = rc.frames_for(dw, dh, rows) * dw * dh * 4
            assert bpp_bytes <= 20 << 20, (interp, rows, bpp_bytes)


def test_neighbouring_frames_of_a_batch_differ():
    """A wave that took a neighbouring frame's rows would store other bytes: the 7 frames differ pairwise, also after
    resizing, so frames f and f + 1 .. f + 6 of a batch never expect the same output."""
    for interp in (NEAREST, LINEAR, AREA):
        for sw, sh, dw, dh in rc.walk_cases(interp):
            for bpp in (1, 4):
                frames = rc.distinct_frames(sw, sh, bpp)
                assert len({f.tobytes() for f in frames}) == rc.NDISTINCT, (sw, sh)
                assert len({resize_ref(f, dw, dh, interp).tobytes() for f in frames}) == rc.NDISTINCT, (sw, sh, interp)


def test_the_walk_cases_show_every_row_cache_class_inside_a_band():
    seen = {}
    for sw, sh, dw, dh in rc.WALK_CASES:
        classes = {c for _, c in rc.row_cache_walk(sh, dh, 16)}
        seen[(sw, sh, dw, dh)] = classes
        assert not rc.row_cache_walk(sh, dh, 1)                       # one row per band: the cache is never used
    assert set(rc.ROW_CLASSES) <= set().union(*seen.values()), seen
    # what each case is in the table for
    assert {rc.KEEP, rc.HANDOVER_FETCH, rc.HANDOVER_ONLY, rc.H1_FETCH} <= seen[(21, 16, 64, 48)]
    assert {rc.HANDOVER_FETCH, rc.FETCH_BOTH} <= seen[(100, 66, 77, 50)]
    assert rc.FETCH_BOTH in seen[(77, 41, 33, 19)] and rc.KEEP not in seen[(77, 41, 33, 19)]
    assert {rc.KEEP, rc.HANDOVER_ONLY} <= seen[(9, 3, 6, 40)] and {rc.KEEP, rc.H1_FETCH} <= seen[(5, 7, 9, 50)]
    # and at every band height every case uses the cache at some row
    for sw, sh, dw, dh in rc.WALK_CASES:
        for r in rc.BAND_HEIGHTS:
            assert rc.row_cache_walk(sh, dh, r), (sh, dh, r)


def test_a_broken_row_cache_shows_on_the_walk_cases_and_not_at_one_row_per_band():
    """The kernel's band loop restated with one step broken.  Dropping the H0 <- H1 hand-over, or keeping H1 across a step
    that fetched H0 afresh, changes bytes of the walk cases' own frames at every band height 2 .. 16 and none at one row
    per band, which is all the shapes of test_gpu_resize.py run but two.  Not updating row0 changes no byte anywhere:
    the loop then fetches or hands over again what it already held, which costs time and nothing else."""
    seen = {rc.NO_HANDOVER: set(), rc.H1_REUSED: set()}
    for sw, sh, dw, dh in rc.WALK_CASES:
        frames = rc.distinct_frames(sw, sh, 1)[:2]
        refs = [resize_ref(f, dw, dh, LINEAR) for f in frames]
        for rows in (1,) + rc.BAND_HEIGHTS:
            for f, ref in zip(frames, refs):
                assert np.array_equal(rc.linear_banded(f, dw, dh, rows), ref), (dw, dh, rows)
                assert np.array_equal(rc.linear_banded(f, dw, dh, rows, rc.ROW0_NOT_UPDATED), ref), (dw, dh, rows)
            for mutant in seen:
                wrong = any(not np.array_equal(rc.linear_banded(f, dw, dh, rows, mutant), ref)
                            for f, ref in zip(frames, refs))
                assert not (wrong and rows == 1), (mutant, dw, dh)
                if wrong:
                    seen[mutant].add(rows)
    assert seen == {rc.NO_HANDOVER: set(rc.BAND_HEIGHTS), rc.H1_REUSED: set(rc.BAND_HEIGHTS)}, seen


def test_the_last_band_is_ragged():
    for case in rc.WALK_CASES + rc.AREA_WALK_CASES:
        assert (case[3] % 16 != 0) != (case in rc.FULL_BAND_CASES), case
    assert (100, 66, 77, 50)[3] % 16 == 2 and (77, 41, 33, 19)[3] % 16 == 3
    assert any(c[2] > 256 and c[0] == 4 * c[2] for c in rc.AREA_WALK_CASES)          # x-factor 4 over a full strip
    assert any(c[2] > 256 and c[2] % 256 and c[0] == 2 * c[2] for c in rc.AREA_WALK_CASES)


# ---- sweep mutants ----------------------------------------------------------------------------------------------------
def test_the_unmutated_helpers_are_the_reference():
    for s, d in rc.SWEEP_PAIRS[::7] + rc.decisive_pairs():
        for f in rc.sweep_frames(s):
            assert np.array_equal(rc.nearest_with(f, d, d), resize_ref(f, d, d, NEAREST)), (s, d)
            if s != 2 * d:
                assert np.array_equal(rc.linear_with(f, d, d), resize_ref(f, d, d, LINEAR)), (s, d)
        sx, _, a0, a1 = linear_cols(s, d)
        mx, m0, m1 = rc.linear_table(s, d)
        assert np.array_equal(sx, mx) and np.array_equal(a0, m0) and np.array_equal(a1, m1), (s, d)


def test_the_plain_quotient_changes_nearest_bytes_of_the_sweep():
    """scale = src / dst instead of 1.0 / (dst / src).  Counted here: the source index changes for 98 pairs of
    1..64 x 1..64, and on the sweep's index frames every one of them changes output bytes (the column-index frame shows
    sx, the row-index frame sy), so the decisive set has 98 pairs."""
    index_pairs = [(s, d) for s, d in rc.SWEEP_PAIRS
                   if not np.array_equal(rc.nearest_index(s, d), rc.nearest_index(s, d, rc.plain_quotient))]
    decisive = rc.decisive_pairs()
    assert len(index_pairs) == 98 and decisive == index_pairs
    assert len(decisive) >= 90
    assert {(6, 34), (14, 18), (21, 27)} <= set(decisive)
    for s, d in decisive:
        col, row, _ = rc.sweep_frames(s)
        assert not np.array_equal(rc.nearest_with(col, d, d), rc.nearest_with(col, d, d, rc.plain_quotient)), (s, d)
        assert not np.array_equal(rc.nearest_with(row, d, d), rc.nearest_with(row, d, d, rc.plain_quotient)), (s, d)
    rgba = rc.rgba_sweep_pairs()
    assert set(decisive) <= set(rgba) and (64, 64) in rgba and (32, 64) in rgba and (64, 32) in rgba
    for s, d in decisive[::9]:
        for f in rc.sweep_frames(s, 4)[:2]:
            assert not np.array_equal(rc.nearest_with(f, d, d), rc.nearest_with(f, d, d, rc.plain_quotient)), (s, d)


def test_an_fp32_coordinate_changes_linear_bytes_of_the_sweep():
    """The LINEAR coordinate evaluated in fp32 throughout.  Counted here: (sx, a0) changes for 49 pairs of 1..64 x 1..64
    with src >= 2.  None of them can change a byte of any frame: at every such column the contract's fx is an exact
    integer k, giving (sx, a0, a1) = (k, 2048, 0), and fp32 lands just below it, giving (k - 1, 0, 2048); both are
    2048 * src[k].  The rows behave the same way.  So the sweep also runs LINEAR on the square pairs with a size in
    65..96 at which the mutant moves a weight at an unmoved sx: 114 pairs, and on every one of them it changes bytes of
    the sweep's frames.  Counted with the reference alone."""
    table_pairs = []
    for s, d in rc.SWEEP_PAIRS:
        if s < 2:
            continue
        sx, a0, a1 = rc.linear_table(s, d)
        mx, m0, m1 = rc.linear_table(s, d, rc.coord_fp32)
        cols = np.flatnonzero((sx != mx) | (a0 != m0))
        if len(cols):
            table_pairs.append((s, d))
            assert np.array_equal(mx[cols], sx[cols] - 1) and np.all(a0[cols] == 2048) and np.all(a1[cols] == 0), (s, d)
            assert np.all(m0[cols] == 0) and np.all(m1[cols] == 2048) and np.all(sx[cols] < s - 1), (s, d)
            if s != 2 * d:
                for f in rc.sweep_frames(s):
                    assert np.array_equal(rc.linear_with(f, d, d), rc.linear_with(f, d, d, rc.coord_fp32)), (s, d)
    assert len(table_pairs) == 49 and len(table_pairs) >= 40
    assert {(3, 37), (7, 23), (13, 11)} <= set(table_pairs)
    byte_pairs = rc.fp32_decisive_pairs()
    assert len(byte_pairs) == 114 and len(byte_pairs) >= 1
    assert all(rc.SWEEP_MAX < max(p) <= rc.LINEAR_EXTRA_MAX for p in byte_pairs)
    index_only = 0
    for s, d in byte_pairs:
        frames = rc.sweep_frames(s)
        changed = [not np.array_equal(rc.linear_with(f, d, d), rc.linear_with(f, d, d, rc.coord_fp32)) for f in frames]
        assert any(changed), (s, d)
        index_only += changed[0] or changed[1]
        assert all(np.array_equal(resize_ref(f, d, d, LINEAR), rc.linear_with(f, d, d)) for f in frames), (s, d)
    assert index_only == 106                                            # the index frames alone show most of them


# ---- AREA inputs ------------------------------------------------------------------------------------------------------
def test_area_blocks_realise_their_sums():
    for n, m in rc.AREA_FACTORS:
        for bpp in (1, 4):
            frame, want = rc.area_frame(n, m, bpp)
            assert frame.dtype == np.uint8 and frame.shape[:2] == (want.shape[0] * m, rc.AREA_DW * n), (n, m, bpp)
            assert want.shape[0] >= 2 and np.array_equal(rc.block_sums_of(frame, n, m), want), (n, m, bpp)
            listed = set(rc.area_sums(n, m).tolist())
            chans = want.reshape(want.shape[0] * rc.AREA_DW, -1)
            for c in range(chans.shape[1]):
                assert listed <= set(chans[:, c].tolist()), (n, m, bpp, c)       # every listed sum is in every channel
            if bpp == 4:
                assert want[0, 0].tolist() == [n * m * 255] * 4 and want[0, 1].tolist() == [0] * 4
                assert frame[:m, :n].min() == 255 and frame[:m, n:2 * n].max() == 0
            # the reference gives each block the byte of its sum
            if (n, m) in ((1, 1), (2, 2), (7, 2), (4, 3), (16, 16)):
                assert np.array_equal(resize_ref(frame, rc.AREA_DW, want.shape[0], AREA), area_byte(want, n, m))
    # a block's extra ones are spread: the last row and the last column of blocks hold some of them
    frame, want = rc.area_frame(5, 3, 1)
    blocks = frame.astype(np.int64).reshape(-1, 3, rc.AREA_DW, 5)
    assert (blocks[:, 2].sum(-1) > (want // 15) * 5).any() and (blocks[..., 4].sum(1) > (want // 15) * 3).any()


def test_area_lists_contain_every_sum_the_two_forms_differ_on():
    total, pairs = 0, 0
    for n, m in rc.AREA_FACTORS:
        diff = rc.area_differing_sums(n, m)
        listed = set(rc.area_sums(n, m).tolist())
        assert set(diff.tolist()) <= listed and {0, n * m * 255} <= listed, (n, m)
        k = n * m
        sums = np.arange(k * 255 + 1)
        assert set(sums[(2 * sums) % (2 * k) == k].tolist()) <= listed, (n, m)                  # every exact tie
        if (n, m) != (2, 2):
            total += len(diff)
            pairs += bool(len(diff))
    assert (total, pairs) == (4160, 50)
