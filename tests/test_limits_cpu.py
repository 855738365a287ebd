"""The limit cases (tests/limit_cases.py): the parts that need no GPU.

On the reference's coordinates each case reaches what it is there for, every case is accepted by the numpy restatement
of the argument checks and by the library's own *_check functions (pure host code), and the references stay cheap at
these sizes.  The GPU behaviour is in test_gpu_limits.py.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limit_cases as lc  # noqa: E402
import remap_cases as rc  # noqa: E402
import tiny_batch_cases as tb  # noqa: E402
from box_ref import BINARY, adaptive_ref  # noqa: E402
from remap_ref import (FIXED, FLOAT, INT_MAX, INT_MIN, _round_float, fixed_coords_of_maps, float_coords,  # noqa: E402
                       interior_passes, map_coords, perspective_accepts, perspective_coords, perspective_ref,
                       remap_accepts, remap_ref)
from resize_ref import AREA, accepts as resize_accepts, area_factors, linear_cols, resize_ref  # noqa: E402
from test_gpu_median import noise  # noqa: E402
from test_gpu_warp import WIDE, interior_tiles, tile_of  # noqa: E402
from warp_ref import (CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, accepts, border_pixel, fixed_coords,  # noqa: E402
                      warp_ref)

M = lc.M
OK, UNSUPPORTED = 0, -4
INTERPS = (NEAREST, LINEAR)


def test_every_case_carries_its_reason():
    for table in (lc.THIN_WHY, lc.WARP_THIN_WHY):
        assert all(axis in ("x", "y") and len(why) > 20 for axis, why in table.values())
    assert all(len(why) > 20 for why in list(lc.RESIZE_WHY.values()) + list(lc.TINY_WHY.values()))
    assert lc.THIN == ((M, 3, M, 2), (3, M, 2, M), (M, 3, 3, 2), (3, 2, M, 3)) and M == 32766 and M % 4 == 2
    for shape in lc.WARP_THIN:
        assert all(len(why) > 20 for _, _, why in lc.warp_thin_matrices(shape))
    for shape in lc.THIN:
        assert all(len(why) > 10 for _, _, why in lc.perspective_thin_matrices(shape))
        for kind in (FIXED, FLOAT):
            assert all(len(m[3]) > 20 for m in lc.remap_thin_maps(shape, kind, LINEAR))
    assert all(len(c.why) > 10 for c in lc.bound_cases())
    for interp in INTERPS:
        assert all(len(why) > 10 and want for _, _, want, why in lc.saturation_cases(interp, 5))
    # every frame of sections 1 to 3 that the warp calls see is under 400 KB, every resize frame near 1 MB
    assert max(w * h * 4 for s in lc.WARP_THIN for w, h in (s[:2], s[2:])) < 400 * 1024
    assert max(w * h * 4 for s in lc.RESIZE_PAIRS for w, h in (s[:2], s[2:])) <= 3 * 100003 * 4


# ---- 1. maximum-size thin frames --------------------------------------------------------------------------------------
def test_thin_warp_cases_are_accepted_and_reach_their_reasons(pkg):
    names = set()
    for interp in INTERPS:
        interior = general = 0
        for shape in lc.WARP_THIN:
            sw, sh, dw, dh = shape
            for name, m, _ in lc.warp_thin_matrices(shape):
                names.add(name)
                for inv in (INVERSE_MAP, 0):
                    flags = interp | inv
                    for bpp in (1, 4):
                        for border in (CONSTANT, REPLICATE):
                            assert accepts(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK, (shape, name, inv)
                            assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK, (shape, name, inv)
                    k, n = interior_tiles(m, sw, sh, dw, dh, flags)
                    interior, general = interior + k, general + n - k
                    if name == "stride16000" and inv:
                        X, Y = fixed_coords(m, dw, dh, flags)
                        along = (X if shape[0] == M else Y) >> 10
                        assert sorted(set(along.ravel().tolist())) == [0, 16000, 32000]
                        assert (k, n) == (1, 1) and tile_of(m, flags) == WIDE, (shape, k, n)
                    if name == "turn0.5":
                        assert 0 < k < n and tile_of(m, flags) == WIDE and n >= 512, (shape, inv, k, n)
        assert interior >= 1 and general >= 1, (interp, interior, general)
    assert names == {"identity", "half", "flip", "stride16000", "turn0.5"}
    # the half-pixel shift: fraction 16 on every column, and the last column's far tap is index M, one past the frame
    X, Y = fixed_coords([1.0, 0.0, 0.5, 0.0, 1.0, 0.0], M, 2, LINEAR | INVERSE_MAP)
    assert np.all((X >> 5) & 31 == 16) and (X[0, -1] >> 10) == M - 1 and (X[0, -1] >> 10) + 1 == M
    m = dict((n, v) for n, v, _ in lc.warp_thin_matrices((3, M, 2, M)))["half"]
    X, Y = fixed_coords(m, 2, M, LINEAR | INVERSE_MAP)
    assert np.all((Y >> 5) & 31 == 16) and (Y[-1, 0] >> 10) == M - 1 and np.all(X >> 10 == np.arange(2)[None, :])
    # the flip reads valid pixels at indices far above the widest frame the other GPU tests use
    m = dict((n, v) for n, v, _ in lc.warp_thin_matrices((M, 3, 3, 2)))["flip"]
    X, _ = fixed_coords(m, 3, 2, NEAREST | INVERSE_MAP)
    assert (X[0] >> 10).tolist() == [M - 1, M - 2, M - 3]


def _unclamped(map1, map2, kind, interp):
    """(sx, sy) as the kernel holds them: the split without the clamp to short."""
    if kind == FIXED:
        return fixed_coords_of_maps(map1, map2, interp)[:2]
    S = np.float32(32.0 if interp == LINEAR else 1.0)
    with np.errstate(all="ignore"):
        X, Y = _round_float(map1 * S), _round_float(map2 * S)
    return (X >> 5, Y >> 5) if interp == LINEAR else (X, Y)


def test_thin_remap_cases_are_accepted_and_reach_their_reasons(pkg):
    for interp in INTERPS:
        for kind in (FIXED, FLOAT):
            interior = general = differ = far_valid = seams = 0
            for shape in lc.THIN:
                sw, sh, dw, dh = shape
                for bpp in (1, 4):
                    for border in (CONSTANT, REPLICATE):
                        assert remap_accepts(bpp, sw, sh, dw, dh, 2, kind, interp, border) == OK
                        assert pkg.remap_check(bpp, sw, sh, dw, dh, 2, kind, interp, border) == OK
                maps = lc.remap_thin_maps(shape, kind, interp)
                assert [m[0] for m in maps] == ["identity", "half", "flip", "edge"]
                for name, map1, map2, _ in maps:
                    assert map1.shape[:2] == (dh, dw)
                    coords = map_coords(map1, map2, kind, interp)
                    k, n = interior_passes(coords, sw, sh, interp, rc.TILE, rc.LANE_ROWS)
                    interior, general = interior + k, general + n - k
                    sx, sy, fx, fy = coords
                    valid = (sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)
                    far_valid += int((valid & ((sx >= 4096) | (sy >= 4096))).sum())
                    seams += int(((sx == sw - 1) & (fx > 0) & (sw == M)).sum())
                    seams += int(((sy == sh - 1) & (fy > 0) & (sh == M)).sum())
                    # the kernel keeps the index where the reference clamps it to a short: every tap is inside for both
                    # or outside for both, and the clamp into the frame gives one index
                    ux, uy = _unclamped(map1, map2, kind, interp)
                    differ += int(((ux != sx) | (uy != sy)).sum())
                    for d in (0, 1):
                        for a, b, size in ((ux, sx, sw), (uy, sy, sh)):
                            u, v = a + d, b + d
                            assert np.array_equal((u >= 0) & (u < size), (v >= 0) & (v < size)), (shape, name)
                            assert np.array_equal(np.clip(u, 0, size - 1), np.clip(v, 0, size - 1)), (shape, name)
            assert interior >= 1 and general >= 1, (interp, kind, interior, general)
            assert far_valid > 100000, (interp, kind, far_valid)       # valid pixels at indices of 4096 and above
            if interp == LINEAR:
                assert seams >= 4, (kind, seams)                       # index M - 1 with a fraction: the far tap is M
            if kind == FLOAT:
                assert differ >= 4, (interp, differ)                   # 32768, 40000, -32768.5, -40000 leave a short
    # the planted entries themselves, on the widest shape
    shape = (M, 3, M, 2)
    map1, map2 = lc.fixed_edge_maps(shape, LINEAR)
    sx, sy, fx, fy = fixed_coords_of_maps(map1, map2, LINEAR)
    assert list(zip(sx[0, :8].tolist(), fx[0, :8].tolist())) == list(lc.FIXED_EDGE) and sx[0, 8] == 8 and np.all(sy[0] == 0)
    mx, my = lc.float_edge_maps(shape)
    assert mx[0, :10].tolist() == list(lc.FLOAT_EDGE) and mx[0, 10] == 10.0 and np.all(my[1] == 1.0)
    sx, sy, fx, fy = float_coords(mx, my, LINEAR)
    assert list(zip(sx[0, :5].tolist(), fx[0, :5].tolist())) == [(M - 2, 16), (M - 1, 0), (M - 1, 16), (M, 0), (M, 16)]
    assert sx[0, 5:10].tolist() == [32767, 32767, 32767, -32768, -32768] and fx[0, 8] == 16
    # as y on the tall shape
    mx, my = lc.float_edge_maps((3, M, 2, M))
    assert my[:10, 0].tolist() == list(lc.FLOAT_EDGE) and np.all(mx[:, 1] == 1.0) and my[10, 0] == 10.0


def test_thin_perspective_cases_are_accepted_and_reach_their_reasons(pkg):
    for interp in INTERPS:
        interior = general = 0
        for shape in lc.THIN:
            sw, sh, dw, dh = shape
            mats = lc.perspective_thin_matrices(shape)
            assert [n for n, _, _ in mats] == ["identity", "keystone", "keystone-far"]
            for name, m, _ in mats:
                flags = interp | INVERSE_MAP
                for bpp in (1, 4):
                    for border in (CONSTANT, REPLICATE):
                        assert perspective_accepts(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK
                        assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, 2, m, flags, border) == OK
                coords = perspective_coords(m, dw, dh, flags)
                k, n = interior_passes(coords, sw, sh, interp, rc.TILE, rc.LANE_ROWS)
                interior, general = interior + k, general + n - k
                if name == "keystone-far" and max(sw, sh) == M:
                    # the far edge of the largest source is sampled, from the far edge of the output
                    along, size = (coords[0][0], sw) if sw == M else (coords[1][:, 0], sh)
                    assert along[-1] in (size - 1, size - 2) and along.max() <= size - 1, (shape, along[-1])
                    assert np.all(np.diff(along) >= 0) and along[0] == 0, shape
        assert interior >= 1 and general >= 1, (interp, interior, general)


def test_long_resize_rows_are_accepted_and_leave_few_fraction_bits(pkg):
    ran = 0
    for sw, sh, dw, dh in lc.RESIZE_PAIRS:
        for interp in (NEAREST, LINEAR, AREA):
            want = OK if resize_accepts(interp, sw, sh, dw, dh) else UNSUPPORTED
            for bpp in (1, 4):
                assert pkg.resize_check(bpp, sw, sh, dw, dh, 1, interp) == want, (sw, sh, dw, dh, interp)
            ran += want == OK
    assert ran == 13 and area_factors(65536, 4, 4096, 2) == (16, 2)
    assert [p for p in lc.RESIZE_PAIRS if resize_accepts(AREA, *p)] == [(65536, 4, 4096, 2)]
    # past 2^16 the fp32 coordinate keeps 7 fraction bits: the weights of the far columns are multiples of 2048 / 128
    sx, sx1, a0, a1 = linear_cols(70001, 100003)
    far = sx >= 65536
    assert far.sum() > 6000 and np.all(a1[far] % 16 == 0) and np.any(a1[~far] % 16 != 0) and sx.max() == 70000


# ---- 2. warp_affine matrices just under the 2^20 bound ----------------------------------------------------------------
def test_bound_cases_are_accepted_refused_one_step_on_and_reach_2_to_the_30(pkg):
    cases = lc.bound_cases()
    # per sign: two translations one below the bound, two tight ones, two tight steps; per k one tie and four visible ones
    assert len(cases) == 2 * (6 + 2 * 5) == 32 and len({c.name for c in cases}) == 32
    assert lc.T_INT == 1015810.0
    near = 0
    for c in cases:
        sw, sh, dw, dh = c.shape
        for interp in (INTERPS if c.interp is None else (c.interp,)):
            flags = interp | INVERSE_MAP
            for bpp in (1, 4):
                assert accepts(bpp, sw, sh, dw, dh, 1, c.m, flags, CONSTANT) == OK, c.name
                assert pkg.warp_affine_check(bpp, sw, sh, dw, dh, 1, c.m, flags, REPLICATE) == OK, c.name
            X, Y = fixed_coords(c.m, dw, dh, flags)
            reach = max(abs(X).max(), abs(Y).max())
            assert c.reach <= reach < (1 << 30) + 1024, (c.name, reach)
            near += reach >= lc.NEAR_2_30
            if c.decisive is not None:
                m = list(c.m)
                v = m[c.decisive]
                away = np.copysign(np.inf, v)
                m[c.decisive] = float(np.nextafter(v, away)) if c.step == "ulp" else v + np.copysign(1.0, v)
                assert accepts(4, sw, sh, dw, dh, 1, m, flags, CONSTANT) == UNSUPPORTED, c.name
                assert pkg.warp_affine_check(4, sw, sh, dw, dh, 1, m, flags, CONSTANT) == UNSUPPORTED, c.name
                # every tap lies outside the frame
                sx, sy = X >> 10, Y >> 10
                if c.name[0] == "t":
                    assert np.all((sx + 1 < 0) | (sx >= sw) | (sy + 1 < 0) | (sy >= sh)), c.name
    assert near == 2 * (2 + 8)                                    # the + translations, the tight translations and steps
    by = {c.name: c for c in cases}
    # [1, 0, T, 0, 1, 0] with dst w = M under LINEAR: X from T * 1024 + 16 up to 2^30 - 1008
    X, _ = fixed_coords(by["tx+1"].m, M, 2, LINEAR | INVERSE_MAP)
    assert (X.min(), X.max()) == (1040189456, 1073740816)
    # its negative stays 2^25 away from -2^30 (the step is +1): the tight cases step with the translation's sign
    X, _ = fixed_coords(by["tx-1"].m, M, 2, LINEAR | INVERSE_MAP)
    assert (X.min(), X.max()) == (-1040189424, -1006638064)
    X, _ = fixed_coords(by["tight-tx-1"].m, M, 2, NEAREST | INVERSE_MAP)
    assert X.min() == -(1 << 30) + 512
    X, _ = fixed_coords(by["i0+1"].m, 3, 2, LINEAR | INVERSE_MAP)
    assert X[0].tolist() == [16, (1 << 29) + 16, (1 << 30) + 16]
    # the ties: (i2 * 1024) is n + 0.5 exactly, with even and odd n, and rounds to the even neighbour
    for sign in (1, -1):
        for k, n, want in ((1, 1040187392, 1040187392), (3, 1040187393, 1040187394)):
            v = by["tie%+d-k%d" % (sign, k)].m[2] * 1024.0
            assert abs(v) == n + 0.5 and np.rint(v) == sign * want


def test_visible_ties_decide_an_output_pixel():
    """With the tie rounded half to even the second output column lands one step below, or exactly on, the first step of
    the fraction (LINEAR) or of the index (NEAREST); one unit further, where another rounding puts it, the output
    differs."""
    ran = 0
    for c in lc.bound_cases():
        if not c.name.startswith("visible-tie"):
            continue
        sw, sh, dw, dh = c.shape
        axis, target, B = lc.visible_tie_target(c)
        flags = c.interp | INVERSE_MAP
        X, Y = fixed_coords(c.m, dw, dh, flags)
        assert (X if axis == "x" else Y)[0, 1] == target and target in (B - 1, B), (c.name, X[0], Y[0])
        assert abs((X if axis == "x" else Y)[0, 0]) > (1 << 29) - (1 << 22)
        v = (c.m[2] if axis == "x" else c.m[5]) * 1024.0
        assert v != np.rint(v) and abs(v - np.trunc(v)) == 0.5
        # moving the decisive entry by 1 / 1024 towards the other side of B changes the output
        for bpp in (1, 4):
            img = lc.tie_source(sw, sh, bpp)
            ref = warp_ref(img, c.m, dw, dh, flags, REPLICATE, 0)
            m = list(c.m)
            m[0 if axis == "x" else 3] += (1.0 if target == B - 1 else -1.0) / 1024.0
            assert not np.array_equal(warp_ref(img, m, dw, dh, flags, REPLICATE, 0)[0, 1], ref[0, 1]), c.name
        ran += 1
    assert ran == 16


# ---- 3. perspective saturation ----------------------------------------------------------------------------------------
def test_saturation_cases_take_every_branch_of_the_rounding(pkg):
    sw, sh = lc.PERSP_SRC
    total = {b: 0 for b in (lc.HIGH, lc.LOW, lc.NAN, lc.PLAIN)}
    table = []
    for interp in INTERPS:
        flags = interp | INVERSE_MAP
        for dw, dh in lc.PERSP_DST:
            for name, m, want, _ in lc.saturation_cases(interp, dw):
                assert np.all(np.isfinite(m))
                for bpp in (1, 4):
                    for border in (CONSTANT, REPLICATE):
                        assert perspective_accepts(bpp, sw, sh, dw, dh, 5, m, flags, border) == OK, name
                        assert pkg.warp_perspective_check(bpp, sw, sh, dw, dh, 5, m, flags, border) == OK, name
                tX, tY = lc.perspective_t(m, dw, dh, flags)
                # the helper computes what the reference rounds
                sx, sy, fx, fy = perspective_coords(m, dw, dh, flags)
                for t, s, f in ((tX, sx, fx), (tY, sy, fy)):
                    r = lc.round_t(t)
                    assert np.array_equal(np.clip(r >> 5 if interp == LINEAR else r, -32768, 32767), s)
                    assert np.array_equal(r & 31 if interp == LINEAR else 0 * r, f)
                branches = np.concatenate([lc.branch_of(tX).ravel(), lc.branch_of(tY).ravel()])
                count = {b: int((branches == b).sum()) for b in total}
                for b in want:
                    assert count[b] >= 1, (name, interp, (dw, dh), count)
                assert all(count[b] == 0 for b in (lc.HIGH, lc.LOW, lc.NAN) if b not in want), (name, count)
                for b in total:
                    total[b] += count[b]
                table.append((name, "linear" if interp else "nearest", (dw, dh), count))
                high = lc.branch_of(tX) == lc.HIGH
                if name == "straddle":
                    # one row holds saturated and unsaturated columns; on the wide shape a whole lane of each kind
                    row = high[0]
                    assert row.any() and not row.all()
                    if dw >= 12:
                        assert not row[:4].any() and row[8:12].all() and row[4:8].any() and not row[4:8].all()
                    assert lc.round_t(tX)[0].max() == INT_MAX and 0 < lc.round_t(tX)[0, 1] < INT_MAX
                if lc.HIGH in want:
                    # NEAREST holds INT_MAX itself, LINEAR INT_MAX >> 5 with fraction 31
                    at = np.argwhere(high)[0]
                    r = lc.round_t(tX)[at[0], at[1]]
                    assert r == INT_MAX and (sx[at[0], at[1]], fx[at[0], at[1]]) == (32767, 31 if interp == LINEAR else 0)
                    assert INT_MAX >> 5 == 67108863 and INT_MAX & 31 == 31
                if lc.LOW in want:
                    assert lc.round_t(tX).min() == INT_MIN and sx.min() == -32768
                if name == "denormal":
                    assert np.isnan(tX[0, 0]) and np.isnan(tY[0, 0]) and np.isinf(tX[0, 1]) and np.isnan(tY[0, 1])
                    assert (sx[0, 0], sy[0, 0]) == (32767, 32767)          # a flushed denominator would give (0, 0)
                    assert not np.isnan(lc.perspective_t(lc.saturation_cases(interp, dw)[3][1], dw, dh, flags)[0]).any()
    assert all(total[b] >= 1 for b in (lc.HIGH, lc.LOW, lc.NAN)), total
    print("\nperspective saturation, coordinates per branch (x and y together; shown with -s or on a failure):")
    for row in table:
        print("  %-15s %-8s %-9s %s" % row)
    print("  total %s" % total)
    assert total == {lc.HIGH: 16327, lc.LOW: 4109, lc.NAN: 146, lc.PLAIN: 1398}
    # the denormal shows in the output under both borders: the corner the saturated index clamps to, the border pixel
    # and source pixel (0, 0) all differ
    for bpp in (1, 4):
        img = noise(sh, sw, bpp, 31)
        assert not np.array_equal(img[0, 0], img[-1, -1])
        m = lc.saturation_cases(NEAREST, 5)[2][1]
        assert np.all(perspective_ref(img, m, 5, 2, NEAREST | INVERSE_MAP, REPLICATE, 0) == img[-1, -1])
        out = perspective_ref(img, m, 5, 2, NEAREST | INVERSE_MAP, CONSTANT, lc.VALUE)
        assert np.all(out == border_pixel(lc.VALUE, img)) and not np.array_equal(out[0, 0], img[0, 0])


# ---- 4. thousands of tiny frames ---------------------------------------------------------------------------------------
def test_tiny_batches_cut_into_the_chunks_they_are_there_for():
    assert lc.TINY_N == 3001 and lc.TINY_N % 4 == 1                        # three padding waves in the last block
    assert rc.FRAMES_PER_ITEM == 4
    chunks = [-(-n // rc.FRAMES_PER_ITEM) for n in lc.REMAP_N]
    assert chunks == [751, 751, 751] and [n - 750 * 4 for n in lc.REMAP_N] == [1, 2, 3]
    assert [(-c) % 4 for c in chunks] == [1, 1, 1]
    assert lc.TINY_SHAPES == ((5, 3, 7, 2), (1, 1, 1, 1)) and lc.ADAPTIVE_BLOCKS == (3, 63)
    # the batch cycles through 11 distinct frames, the first and the last frame have content of their own
    idx = tb.frame_index(3003)
    assert sorted(set(idx[1:-1].tolist())) == list(range(11)) and idx[0] == tb.FIRST and idx[-1] >= tb.LAST_LOW
    for sw, sh, dw, dh in lc.TINY_SHAPES:
        for bpp in (1, 4):
            assert accepts(bpp, sw, sh, dw, dh, lc.TINY_N, lc.TINY_AFFINE, LINEAR, CONSTANT) == OK
            assert perspective_accepts(bpp, sw, sh, dw, dh, lc.TINY_N, lc.TINY_PERSPECTIVE, LINEAR, CONSTANT) == OK
    # 11 and 4 are coprime: every distinct frame meets every place in a chunk
    assert len({(f % 11, f % 4) for f in range(1, 3000)}) == 44


# ---- the references stay cheap ------------------------------------------------------------------------------------------
def test_a_full_pass_of_the_references_is_cheap():
    """Every case of sections 1 to 3 through its reference once, on RGBA noise (the dearer pixel size), both
    interpolations, one border each: seconds, and the bar is half a minute; one thin warp of 32766 x 3 RGBA pixels
    alone takes a few hundredths of a second, and the bar is one second."""
    t0 = time.perf_counter()
    img = noise(3, M, 4, 1)
    t1 = time.perf_counter()
    warp_ref(img, [1.0, 0.0, 0.5, 0.0, 1.0, 0.0], M, 2, LINEAR | INVERSE_MAP, CONSTANT, lc.VALUE)
    one = time.perf_counter() - t1
    ran = 0
    for interp, border in ((NEAREST, CONSTANT), (LINEAR, REPLICATE)):
        for shape in lc.WARP_THIN:
            sw, sh, dw, dh = shape
            img = noise(sh, sw, 4, 3)
            for name, m, _ in lc.warp_thin_matrices(shape):
                for inv in (INVERSE_MAP, 0):
                    warp_ref(img, m, dw, dh, interp | inv, border, lc.VALUE)
                    ran += 1
        for shape in lc.THIN:
            sw, sh, dw, dh = shape
            img = noise(sh, sw, 4, 3)
            for kind in (FIXED, FLOAT):
                for name, map1, map2, _ in lc.remap_thin_maps(shape, kind, interp):
                    remap_ref(img, map1, map2, kind, interp, border, lc.VALUE)
                    ran += 1
            for name, m, _ in lc.perspective_thin_matrices(shape):
                perspective_ref(img, m, dw, dh, interp | INVERSE_MAP, border, lc.VALUE)
                ran += 1
        for c in lc.bound_cases():
            if c.interp in (None, interp):
                sw, sh, dw, dh = c.shape
                warp_ref(noise(sh, sw, 4, 3), c.m, dw, dh, interp | INVERSE_MAP, border, lc.VALUE)
                ran += 1
        img = noise(lc.PERSP_SRC[1], lc.PERSP_SRC[0], 4, 3)
        for dw, dh in lc.PERSP_DST:
            for name, m, _, _ in lc.saturation_cases(interp, dw):
                perspective_ref(img, m, dw, dh, interp | INVERSE_MAP, border, lc.VALUE)
                ran += 1
    for sw, sh, dw, dh in lc.RESIZE_PAIRS:
        img = noise(sh, sw, 4, 3)
        for interp in (NEAREST, LINEAR, AREA):
            if resize_accepts(interp, sw, sh, dw, dh):
                resize_ref(img, dw, dh, interp)
                ran += 1
    d = tb.distinct(lc.ADAPTIVE_SHAPE[1], lc.ADAPTIVE_SHAPE[0], 1)
    for block in lc.ADAPTIVE_BLOCKS:
        for f in d:
            adaptive_ref(f, 200, BINARY, block, 2)
    total = time.perf_counter() - t0
    assert ran > 250 and total < 30.0 and one < 1.0, (ran, total, one)
