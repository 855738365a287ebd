"""What test_gpu_large_k.py claims to reach, checked without a GPU: the LDS carve of every launch it makes (restated in
large_k_cases.py from gauss_tile.hip, sobel_tile.hip and gray8.hip), the tables of its (k, sigma) grid, which side of
gray8.hip's delta_bound_k < 0.01 each of them falls on, what its frames hold, what its CPU references cost, and that its
comparison helper reports a single bad byte.  If a layout or a threshold moves, a test here fails and asks for another
k or sigma instead of the GPU suite silently testing less.
"""
import time

import numpy as np
import pytest

import large_k_cases as lk
from test_gauss_tables_cpu import delta_bound_k, separable_factor, symmetric, upper_clamp, wsum

GRID = [(k, s) for k in lk.KS for s in lk.SIGMAS(k)]


@pytest.fixture(scope="module")
def deltas(pkg):
    out = {}
    for k, s in GRID:
        t = pkg.gauss_weights(k, s)
        out[k, s] = delta_bound_k(separable_factor(t)[0], t)
    return out


# ---- sizes -----------------------------------------------------------------------------------------------------------
def test_every_size_has_its_reason():
    assert tuple(lk.KS_WHY) == lk.KS and all(k % 2 == 1 and 17 < k <= 63 for k in lk.KS)
    assert tuple(sorted(lk.KS)) == lk.KS and lk.KS[-1] == 63
    assert set(lk.IMAGE_KS) <= set(lk.KS) and min(lk.IMAGE_KS) == 27      # kImgMaxFastK = 25 (image2d.hip)
    assert 25 in lk.KS and 27 in lk.KS
    for k in lk.KS:
        assert lk.SIGMAS(k) == (0.35, k / 6.0, 50.0)


# ---- carves ----------------------------------------------------------------------------------------------------------
def test_carves_at_the_maximum_size():
    assert lk.gauss_tile_layout(False, 63).bytes == 71820
    assert lk.gauss_tile_layout(True, 63).bytes == 55188
    assert lk.pipe_tile_layout(False, 63).bytes == 55180
    assert lk.pipe_tile_layout(True, 63).bytes == 61588
    assert lk.g8_layout(lk.OP_PIPE, lk.GM_EXC, 63).bytes == 107424       # the largest carve of the library
    assert max(lk.all_carves(63).values()) == 107424


def test_the_tiled_gaussian_crosses_64_kib_between_57_and_59():
    assert lk.gauss_tile_layout(False, 57).bytes == 65508 <= lk.LDS_DEFAULT
    assert lk.gauss_tile_layout(False, 59).bytes == 67580 > lk.LDS_DEFAULT
    assert 57 in lk.KS and 59 in lk.KS
    # the other RGBA carves never leave the default limit: only FAST at 59 and 63 shows that raising it works there
    for k in lk.KS:
        assert lk.gauss_tile_layout(True, k).bytes <= lk.LDS_DEFAULT
        assert lk.pipe_tile_layout(False, k).bytes <= lk.LDS_DEFAULT and lk.pipe_tile_layout(True, k).bytes <= lk.LDS_DEFAULT
        assert (lk.gauss_tile_layout(False, k).bytes > lk.LDS_DEFAULT) == (k >= 59)


def test_the_single_channel_kernels_cross_64_kib_inside_the_range():
    """First size of KS above 64 KiB per launch, from the restated g8_layout: the FAST Gaussian (kGmSep) 45, exact by
    exception 33 (Gaussian) and every size (pipeline: 71,088 B at 19); tap by tap never (63,904 B at 63)."""
    def first_above(op, gm):
        return next((k for k in lk.KS if lk.g8_layout(op, gm, k).bytes > lk.LDS_DEFAULT), None)
    assert first_above(lk.OP_GAUSS, lk.GM_SEP) == 45 and lk.g8_layout(lk.OP_GAUSS, lk.GM_SEP, 45).bytes == 69888
    assert first_above(lk.OP_GAUSS, lk.GM_EXC) == 33 and lk.g8_layout(lk.OP_GAUSS, lk.GM_EXC, 33).bytes == 68000
    assert first_above(lk.OP_PIPE, lk.GM_EXC) == 19 and lk.g8_layout(lk.OP_PIPE, lk.GM_EXC, 19).bytes == 71088
    assert first_above(lk.OP_GAUSS, lk.GM_TAP) is None and first_above(lk.OP_PIPE, lk.GM_TAP) is None
    assert lk.g8_layout(lk.OP_PIPE, lk.GM_TAP, 63).bytes == 63904
    # the largest carve a launch of the GPU tests really makes: exact by exception is refused from 57 on (below)
    assert lk.g8_layout(lk.OP_PIPE, lk.GM_EXC, 49).bytes == 94720 and lk.g8_layout(lk.OP_GAUSS, lk.GM_EXC, 49).bytes == 81248


def test_the_carve_table_of_the_gpu_file():
    """The table in test_gpu_large_k.py's docstring, column by column."""
    table = {   # k: gauss_tile FAST, EXACT, pipeline_tile FAST, EXACT, gray8 Gaussian Sep, Exc, Tap, gray8 pipeline Exc, Tap
        19: (32220, 12596, 22972, 18292, 57744, 59200, 24128, 71088, 33552),
        25: (36708, 16580, 26452, 22372, 60272, 62784, 26944, 74720, 36368),
        27: (38268, 18036, 27676, 23860, 61104, 64032, 27936, 75984, 37360),
        33: (43140, 22788, 31540, 28708, 63632, 68000, 31136, 81056, 41616),
        45: (53748, 34020, 40132, 40132, 69888, 78000, 39600, 90128, 49056),
        49: (57540, 38276, 43252, 44452, 71632, 81248, 42336, 94720, 53104),
        57: (65508, 47556, 49876, 53860, 76528, 89536, 49600, 101792, 59088),
        59: (67580, 50036, 51612, 56372, 77424, 91360, 51168, 103632, 60656),
        63: (71820, 55188, 55180, 61588, 79232, 95120, 54416, 107424, 63904)}
    assert tuple(table) == lk.KS
    for k, row in table.items():
        assert tuple(lk.all_carves(k).values()) == row, k


def test_every_carve_fits_a_workgroup():
    """gfx950 has 160 KiB of LDS per workgroup (MI355X_MICROARCH.md: 160 KB per CU, all of it allocatable by one
    workgroup): hipFuncSetAttribute refuses more."""
    assert lk.LDS_WORKGROUP == 160 * 1024
    for k in lk.KS:
        for name, size in lk.all_carves(k).items():
            assert 0 < size <= lk.LDS_WORKGROUP, (k, name, size)


def test_carve_regions_do_not_overlap_and_stay_aligned():
    for k in lk.KS:
        for exact in (False, True):
            g = lk.gauss_tile_layout(exact, k)
            assert g.off_raw % 16 == 0 and g.off_wt == g.off_raw + g.RH * g.RW * 4 and g.bytes > g.off_wt
            p = lk.pipe_tile_layout(exact, k)
            assert 0 < p.off_v <= p.off_b < p.off_wt and p.bytes > 4 * p.off_wt
        for op in (lk.OP_GAUSS, lk.OP_PIPE):
            for gm in (lk.GM_SEP, lk.GM_EXC, lk.GM_TAP):
                L = lk.g8_layout(op, gm, k)
                offs = (L.off_v, L.off_w2, L.off_w1, L.off_raw, L.off_g, L.off_o, L.bytes)
                assert all(o % 16 == 0 for o in offs) and list(offs) == sorted(offs), (k, op, gm)
                assert L.RWS >= L.RW and L.RWS % 16 == 0 and L.RH == 32 + 2 * L.H and L.H == k // 2 + (op == lk.OP_PIPE)


# ---- tables ----------------------------------------------------------------------------------------------------------
def test_tables_of_the_grid(pkg, oracle):
    for k, s in GRID:
        t = pkg.gauss_weights(k, s)
        assert t.shape == (k, k) and np.array_equal(t, oracle.gauss_weights(k, s)), (k, s)
        assert np.isfinite(t).all() and (t >= 0).all(), (k, s)
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 1e-5, (k, s)
        w1, ok = separable_factor(t)
        # the separable kernels take it, the pair form applies, no CLAMP instantiation
        assert ok and symmetric(w1) and not upper_clamp(wsum(w1)) and not upper_clamp(wsum(w1), 0.01), (k, s)


def test_small_sigma_is_the_centre_tap_alone(pkg):
    for k in lk.KS:
        t = pkg.gauss_weights(k, 0.35)
        c = k // 2
        assert t[c, c] > 0.9 and t[c - 1:c + 2, c - 1:c + 2].sum() > 0.9999 and np.count_nonzero(t > 1e-12) <= 25, k


def test_large_sigma_is_a_box_within_rounding(pkg):
    for k in lk.KS:
        t = pkg.gauss_weights(k, 50.0).astype(np.float64)
        assert t.min() * k * k > 0.6 and t.max() * k * k < 1.25, k


# ---- the exact-by-exception range ------------------------------------------------------------------------------------
def test_no_grid_point_sits_on_the_threshold(deltas):
    for (k, s), d in deltas.items():
        assert abs(d / lk.DELTA_LIMIT - 1.0) > lk.DELTA_MARGIN, (k, s, d)


def test_the_exception_arithmetic_serves_every_table_up_to_33_and_none_from_57(deltas):
    for (k, s), d in deltas.items():
        if k <= 33:
            assert d < lk.DELTA_LIMIT, (k, s, d)
        if k >= 57:
            assert d >= lk.DELTA_LIMIT, (k, s, d)


@pytest.mark.parametrize("k", [45, 49])
def test_the_hand_over_sizes_have_a_sigma_on_each_side(deltas, k):
    sides = [deltas[k, s] < lk.DELTA_LIMIT for s in lk.SIGMAS(k)]
    assert any(sides) and not all(sides), (k, [deltas[k, s] for s in lk.SIGMAS(k)])


def test_the_bound_is_exercised_up_to_its_limit(deltas):
    """The largest delta below 0.01 on the grid: the kernel is run with a bound in the top 5 % of what it accepts."""
    below = [d for d in deltas.values() if d < lk.DELTA_LIMIT]
    assert max(below) > 0.95 * lk.DELTA_LIMIT
    assert max(deltas.values()) > 2 * lk.DELTA_LIMIT       # and refused with a bound twice as wide


def test_which_arithmetic_each_single_channel_call_runs(deltas):
    """The dispatch table of test_gpu_large_k.py's docstring, from the restated predicate."""
    exc = {k: [bool(deltas[k, s] < lk.DELTA_LIMIT) for s in lk.SIGMAS(k)] for k in lk.KS}
    assert exc == {19: [True] * 3, 25: [True] * 3, 27: [True] * 3, 33: [True] * 3, 45: [True, True, False],
                   49: [True, False, False], 57: [False] * 3, 59: [False] * 3, 63: [False] * 3}
    for (k, s), d in deltas.items():
        for pipe in (False, True):
            assert lk.g8_gm(d, fast=False, tile=True, pipe=pipe) == lk.GM_TAP
            assert lk.g8_gm(d, fast=False, tile=False, pipe=pipe) == (lk.GM_EXC if d < lk.DELTA_LIMIT else lk.GM_TAP)
            assert lk.g8_gm(d, fast=True, tile=False, pipe=pipe) == (lk.g8_gm(d, False, False, True) if pipe else lk.GM_SEP)


# ---- shapes and content ----------------------------------------------------------------------------------------------
def _tiles(h, w, tile):
    return (h + tile[0] - 1) // tile[0], (w + tile[1] - 1) // tile[1]


def test_shapes_reach_what_they_promise():
    h, w, n = lk.RGBA_BIG
    assert _tiles(h, w, lk.RGBA_TILE) == (3, 3) and h % 16 and w % 64 and n == 3
    assert (h * w * 4) % 16 == 8                      # frame 1 starts off a 16-byte boundary
    assert lk.RGBA_SHAPES[1][:2] == lk.RGBA_TILE
    small = lk.RGBA_SHAPES[2:]
    assert any(w < 4 for _, w, _ in small) and any(h < 2 for h, _, _ in small)
    assert all(min(h, w) <= min(lk.KS) // 2 for h, w, _ in small)     # every size's window leaves the frame on both sides
    assert any(n > 1 for _, _, n in small)
    assert any(h > 63 // 2 and w <= min(lk.KS) // 2 for h, w, _ in small)      # one axis alone

    h, w, n = lk.G8_SHAPES[0]
    assert _tiles(h, w, lk.G8_TILE) == (3, 2) and h % 32 and w % 256 and n == 2
    h, w, n = lk.G8_SHAPES[1]
    assert _tiles(h, w, lk.G8_TILE) == (3, 2) and (h * w) % 2 == 1 and n == 2     # frame 1 starts at an odd byte
    assert lk.G8_SHAPES[2][:2] == lk.G8_TILE
    assert {(1, 1, 1), (5, 300, 1), (300, 5, 1)} <= set(lk.G8_SHAPES)


def _constant_windows(y, k):
    """How many pixels of plane y have a constant k x k window under clamp-to-edge taps."""
    r = k // 2
    p = np.pad(y, r, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (k, k))
    return int((win.max(axis=(2, 3)) == win.min(axis=(2, 3))).sum())


def test_content_holds_what_it_promises():
    assert lk.PATCH > 63 and lk.PERIOD > lk.PATCH
    for h, w, n in lk.RGBA_SHAPES:
        for x in lk.rgba_batches((h, w, n)):
            assert x.shape == (n, h, w, 4) and x.dtype == np.uint8 and x.flags["C_CONTIGUOUS"]
        assert all(np.array_equal(a, b) for a, b in zip(lk.rgba_batches((h, w, n)), lk.rgba_batches((h, w, n))))
    x = lk.rgba_batches(lk.RGBA_BIG)[0]
    assert len(np.unique(x[0])) == 256 and len(np.unique(x[0, ..., 3])) > 200         # noise, alpha noise
    assert (x[1, ..., 3] == 255).all() and set(np.unique(x[2])) == {0, 255}
    for c in range(3):
        assert _constant_windows(x[1, ..., c], 63) >= 37 and _constant_windows(x[0, ..., c], 19) == 0
        assert not np.array_equal(x[0, ..., c], x[0, ..., (c + 1) % 4])
    h, w, _ = lk.RGBA_BIG
    assert len(np.unique(x[1, :, lk.PATCH:lk.PERIOD, 0])) > 100                       # noise between the patches
    for shape in lk.G8_SHAPES:
        for y in lk.g8_batches(shape):
            assert y.shape == (shape[2], shape[0], shape[1]) and y.dtype == np.uint8 and y.flags["C_CONTIGUOUS"]
    for shape in lk.G8_SHAPES[:2]:
        y = lk.g8_batches(shape)[0]
        assert _constant_windows(y[1], 63) >= 64 and _constant_windows(y[0], 19) == 0
    assert set(np.unique(lk.g8_batches(lk.G8_SHAPES[1])[0][0])) == {0, 255}
    assert len(np.unique(lk.g8_batches(lk.G8_SHAPES[0])[0][0])) == 256
    assert _constant_windows(lk.g8_batches(lk.G8_SHAPES[2])[1][0], 63) >= 32


def test_constant_windows_are_flagged_by_the_exception_test(pkg, deltas):
    """Why the patches are there: over a constant window of value c the separable sum is c * sum(table), within a few
    1e-6 of the integer c, far inside every delta of the grid: each such pixel takes the exception."""
    for k, s in GRID:
        t = pkg.gauss_weights(k, s).astype(np.float64)
        assert 255.0 * abs(t.sum() - 1.0) < 0.1 * deltas[k, s], (k, s)


# ---- references ------------------------------------------------------------------------------------------------------
def test_the_single_threaded_plane_reference_is_gauss_r(oracle):
    from test_gpu_gray8 import gauss_r
    y = lk.noise(21, 45, 9)
    for k, s in ((19, 0.35), (63, 10.5)):
        assert np.array_equal(lk.gauss_plane(oracle, y, k, s), gauss_r(oracle, y, k, s))


def test_cpu_references_stay_cheap(oracle):
    """The largest frames of test_gpu_large_k.py at k = 63, one thread each as the GPU file runs them.  Measured:
    RGBA Gaussian 0.10 s, RGBA pipeline 0.07 s, single-channel plane 0.31 s, image mode 0.19 s.  The cap is generous:
    it is there so that a change of shape by an order of magnitude is noticed."""
    cap = 3.0
    h, w, _ = lk.RGBA_BIG
    x = lk.rgba_batches(lk.RGBA_BIG)[0][0]
    h8, w8, _ = max(lk.G8_SHAPES, key=lambda s: s[0] * s[1])
    y = lk.noise(h8, w8, 1)
    for name, fn in (("gauss", lambda: oracle.gauss_rgba(x, 63, 10.5)), ("pipeline", lambda: oracle.pipeline_rgba(x, 63, 10.5)),
                     ("plane", lambda: lk.gauss_plane(oracle, y, 63, 10.5)), ("image", lambda: oracle.image2d_gauss(x, 63, 10.5))):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        print("%s: %.3f s" % (name, dt))
        assert dt < cap, (name, dt)


# ---- the comparison helper -------------------------------------------------------------------------------------------
@pytest.fixture
def pair():
    ref = lk.rgba_frames(9, 11, 3, 7)
    return ref, ref.copy()


def test_report_accepts_equal_arrays(pair):
    ref, got = pair
    rep = lk.Report()
    rep.same(got, ref, "a")
    rep.within(got, ref, 1, "b")
    rep.done()


def test_report_names_one_wrong_byte(pair):
    ref, got = pair
    got[2, 4, 10, 1] ^= 1
    rep = lk.Report()
    rep.within(got, ref, 1, "fast")        # one LSB: inside the FAST Gaussian's tolerance
    assert not rep.bad
    rep.same(got, ref, "exact", 63)
    assert len(rep.bad) == 1
    msg = rep.bad[0]
    assert "1 values differ" in msg and "max |d| 1" in msg and "exact" in msg and "63" in msg
    assert "frame 2..2, row 4..4, col 10..10, channel 1..1" in msg
    with pytest.raises(AssertionError) as e:
        rep.done()
    assert "1 failed comparisons" in str(e.value) and "frame 2..2" in str(e.value)


def test_report_names_one_unwritten_byte(pair):
    """A byte that still holds a prefill 128 away from the reference (guarded.prefill_of) fails both comparisons."""
    import guarded
    ref, got = pair
    got[1, 8, 0, 3] = guarded.prefill_of(ref)[1, 8, 0, 3]
    rep = lk.Report()
    rep.same(got, ref, "exact")
    rep.within(got, ref, 1, "fast")
    assert len(rep.bad) == 2
    for msg in rep.bad:
        assert "128" in msg and "frame 1..1, row 8..8, col 0..0, channel 3..3" in msg
    assert "1 values differ" in rep.bad[0] and "max |d| 128 > 1 at 1 values" in rep.bad[1]


def test_report_on_planes_and_single_frames():
    ref = lk.noise(5, 7, 1)
    got = ref.copy()
    got[3, 6] ^= 0x80
    rep = lk.Report()
    rep.same(got[None], ref[None], "plane")
    rep.same(got, ref, "2-d")
    assert "frame 0..0, row 3..3, col 6..6" in rep.bad[0] and "axis 0 3..3, axis 1 6..6" in rep.bad[1]


def test_report_collects_every_failure(pair):
    ref, got = pair
    got[0, 0, 0, 0] ^= 0x40
    rep = lk.Report()
    for i in range(3):
        rep.same(got, ref, "call %d" % i)
    with pytest.raises(AssertionError) as e:
        rep.done()
    assert "3 failed comparisons" in str(e.value) and "call 2" in str(e.value)
