"""Conditions that the inputs and tables of test_gpu_gauss_tables.py must meet, checked with the CPU oracle alone.

The GPU suite claims to reach the CLAMP instantiations of the sliding-window kernels, the matrix-core kernel's
acceptance limit and the exact-by-exception stage's refusal.  Which table reaches which is decided by host formulas in
csrc/common.hpp (gauss_upper_clamp), csrc/gauss_mfma_reg.hip (gauss_mfma_reg_supported), csrc/exact_common.hpp
(delta_bound_k, exact_tables_ok) and csrc/capi.hip (separable_factor).  They are restated here in numpy: if a threshold
moves, one of these tests asks for another gain instead of the GPU suite silently testing less.
"""
import math

import numpy as np
import pytest

import gauss_tables_ref as gt


# ---- the library's host formulas, restated ---------------------------------------------------------------------------
def separable_factor(table):
    """capi.hip: rowsum / sqrt(total) in double, stored as float; ok = the factor reproduces the table within 1e-6 of
    its largest entry and nothing is negative."""
    k = table.shape[0]
    rs = [0.0] * k
    tot = 0.0
    for i in range(k):
        for j in range(k):
            rs[i] += float(table[i, j])
        tot += rs[i]
    if (table < 0).any() or not tot > 0.0:
        return np.zeros(k, np.float32), False
    w1 = np.array([r / math.sqrt(tot) for r in rs]).astype(np.float32)
    dev = np.abs(table.astype(np.float64) - np.outer(w1.astype(np.float64), w1.astype(np.float64))).max()
    return w1, bool(dev <= 1.0e-6 * float(np.abs(table).max()))


def wsum(w1):
    s = 0.0
    for v in w1:
        s += float(v)
    return s


def upper_clamp(s, slack=0.0):
    """common.hpp gauss_upper_clamp: the CLAMP instantiation unless 255 * wsum^2 stays below 256."""
    return not (255.0 * s * s * 1.0001 + slack < 256.0)


def mfma_accepts(w1):
    """gauss_mfma_reg.hip gauss_mfma_reg_supported, the part that depends on the table."""
    return 3 <= len(w1) <= 17 and 256.0 * 255.0 * wsum(w1) < 65400.0


def half_ulp(x):
    if not x > 0.0:
        return 0.0
    _, e = math.frexp(x)
    return math.ldexp(1.0, e - 25)


def delta_bound_k(w1, w2):
    """exact_common.hpp delta_bound_k, term by term."""
    k = len(w1)
    r = k // 2
    w1 = [float(v) for v in w1]
    w2 = [float(v) for v in np.asarray(w2).reshape(-1)]
    sum1 = sum(w1)
    mismatch = sum(abs(w1[i] * w1[j] - w2[i * k + j]) for i in range(k) for j in range(k))
    e_cpu = cum = 0.0
    for v in w2:
        cum += v
        e_cpu += half_ulp(255.0 * v) + half_ulp(255.0 * cum + 1e-3)
    tv = 255.0 * sum1
    c_d = w1[r]
    e_v = half_ulp(255.0 * c_d)
    for d in range(1, r + 1):
        c_d += 2.0 * w1[r - d]
        e_v += half_ulp(255.0 * c_d + 1e-3)
    e_pairs = sum(w1[r - d] * half_ulp(2.0 * tv + 1e-3) for d in range(1, r + 1))
    c_d = w1[r]
    e_chain = half_ulp(tv * c_d + 0.011)
    for d in range(1, r + 1):
        c_d += 2.0 * w1[r - d]
        e_chain += half_ulp(tv * c_d + 0.011)
    e_h = e_v * sum1 + e_pairs + e_chain
    return 1.02 * (e_cpu + e_h + 255.0 * mismatch) + 1e-7


def symmetric(w1):
    return all(w1[j] == w1[len(w1) - 1 - j] for j in range(len(w1) // 2))


# ---- shared inputs ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(oracle):
    return gt.frames(131, 512, seed=131512)


@pytest.fixture(scope="module")
def bases(oracle):
    return {(k, s): oracle.gauss_weights(k, s) for k, s in gt.BASES}


def _threads(oracle):
    return max(1, min(oracle.max_threads(), 16))


def _near_block(h, w, which, r):
    y0, x0 = gt.block_origin(h, w, which)
    m = np.zeros((h, w), bool)
    m[max(0, y0 - r):y0 + gt.BLOCK + r, max(0, x0 - r):x0 + gt.BLOCK + r] = True
    return m


# ---- the builders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", gt.SHAPES)
def test_frames_hold_what_they_promise(h, w):
    x = gt.frames(h, w, seed=h * 1000 + w)
    assert x.shape == (3, h, w, 4) and x.dtype == np.uint8
    assert np.array_equal(x[0, ..., :3], x[1, ..., :3]) and np.array_equal(x[0, ..., :3], x[2, ..., :3])
    assert len(np.unique(x[0, ..., 3])) > 200 and (x[1, ..., 3] == 255).all() and (x[2, ..., 3] == 128).all()
    assert np.array_equal(x, gt.frames(h, w, seed=h * 1000 + w))
    outside = ~(_near_block(h, w, 255, 0) | _near_block(h, w, 0, 0))
    left, right = outside.copy(), outside.copy()
    left[:, w // 2:] = False
    right[:, :w // 2] = False
    rgb = x[0, ..., :3]
    assert rgb[left].min() < 16 and rgb[left].max() > 240         # noise over the whole range
    assert rgb[right].min() >= 192 and len(np.unique(rgb[right])) == 64
    for which in (255, 0):   # whole blocks, wider than a 17 x 17 window, away from the frame's edge
        y0, x0 = gt.block_origin(h, w, which)
        assert y0 >= 1 and x0 >= 1 and y0 + gt.BLOCK < h and x0 + gt.BLOCK < w
        assert (rgb[y0:y0 + gt.BLOCK, x0:x0 + gt.BLOCK] == which).all()
    assert gt.BLOCK > 17 + 2
    # the shapes' alignment classes
    assert (w % 4, (h * w * 4) % 16) in ((0, 0), (2, 8), (1, 4))
    assert np.array_equal(gt.gray_plane(x), x[1, ..., 0])


def test_scaled_is_one_float_multiply(bases):
    t = bases[(5, 1.5)]
    s = gt.scaled(t, 1.25)
    assert s.dtype == np.float32 and np.array_equal(s, t * np.float32(1.25))
    assert np.array_equal(gt.scaled(t, 1.0), t)


def test_gray8_reference_is_a_channel_of_the_rgba_reference(oracle):
    """test_gpu_gray8.py's gauss_r — the R channel of the CPU Gaussian of (y, y, y, 255) — equals the R channel of the
    CPU Gaussian of the frame the plane was taken from: the CPU path sums each channel on its own."""
    from test_gpu_gray8 import gauss_r
    x = gt.frames(53, 501, seed=1)
    y = gt.gray_plane(x)
    for k, s in ((5, 1.5), (9, 0.35)):
        assert np.array_equal(gauss_r(oracle, y, k, s), oracle.gauss_rgba(x[1], k, s)[..., 0])
    t = gt.scaled(oracle.gauss_weights(7, 2.0), 1.25)
    assert np.array_equal(gauss_r(oracle, y, 7, weights=t), oracle.gauss_rgba(x[1], 7, weights=t)[..., 0])


# ---- part 1: generated tables ----------------------------------------------------------------------------------------
def test_generated_tables_on_the_sigma_grid_are_normalised(pkg, oracle):
    grid = [(k, s) for k in gt.GRID_KS for s in gt.GRID_SIGMAS] + [(k, s) for k in gt.EDGE_KS for s in gt.EDGE_SIGMAS]
    for k, s in grid:
        t = pkg.gauss_weights(k, s)
        assert t.shape == (k, k) and np.isfinite(t).all() and (t >= 0).all(), (k, s)
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 1e-5, (k, s)
        assert np.array_equal(t, oracle.gauss_weights(k, s)), (k, s)
        # every one is a table the separable kernels take without their upper clamp
        w1, ok = separable_factor(t)
        assert ok and symmetric(w1) and not upper_clamp(wsum(w1)) and not upper_clamp(wsum(w1), 0.01), (k, s)
        if k in (3, 5, 7):   # ... and one the exact-by-exception stage takes
            assert delta_bound_k(w1, t) < 0.01, (k, s)


def test_small_sigma_puts_every_sum_next_to_an_integer(pkg):
    """What makes sigma = 0.2 a case of its own: the centre tap is 1 within float rounding."""
    for k in gt.GRID_KS:
        t = pkg.gauss_weights(k, 0.2)
        assert t[k // 2, k // 2] > 0.9999 and t.sum() - t[k // 2, k // 2] < 1e-4


# ---- part 2: what each gain reaches ----------------------------------------------------------------------------------
def test_classification_of_the_gains(bases):
    want = {   # gain: (CLAMP in gauss_slide / pipe_slide, matrix cores accept)
        0.5: (False, True), 1.0035: (False, True), 1.0038: (False, False), 1.0039: (True, False),
        1.25: (True, False), 2.0: (True, False), 100.0: (True, False)}
    assert tuple(want) == gt.GAINS
    for (k, s), base in bases.items():
        for gain, (clamp, mfma) in want.items():
            t = gt.scaled(base, gain)
            w1, ok = separable_factor(t)
            assert ok and symmetric(w1), (k, gain)    # the separable kernels take it; the pair form applies
            assert upper_clamp(wsum(w1)) == clamp, (k, gain)
            assert mfma_accepts(w1) == mfma, (k, gain)
            # the matrix-core kernel's own clamp flag can therefore never be set where its launcher runs
            assert not (mfma_accepts(w1) and upper_clamp(wsum(w1))), (k, gain)
            # gauss_exact.hip adds a slack of 0.01 to the shared test: its CLAMP starts one gain earlier
            assert upper_clamp(wsum(w1), 0.01) == (gain >= 1.0038), (k, gain)
            if k in (3, 5, 7):
                assert (delta_bound_k(w1, t) < 0.01) == (gain <= 2.0), (k, gain, delta_bound_k(w1, t))


def test_matrix_core_clamp_instantiation_has_no_table(bases):
    """gauss_mfma_reg_supported needs 65280 * wsum < 65400, launch_gauss_mfma_reg sets clamp from 255 * wsum^2 * 1.0001
    >= 256: the largest accepted wsum gives 255.96, so no wsum at all satisfies both."""
    s = 65400.0 / 65280.0
    assert 255.0 * s * s * 1.0001 < 256.0


def test_asymmetric_tables_are_separable_clamped_and_refused_by_the_pair_form():
    for k in gt.ASYM_FACTORS:
        t = gt.scaled(gt.asym_table(k), gt.ASYM_GAIN)
        w1, ok = separable_factor(t)
        assert ok and not symmetric(w1) and upper_clamp(wsum(w1)) and not mfma_accepts(w1), k


def test_gains_above_one_saturate_a_share_of_the_frame(oracle, big, bases):
    for (k, s), base in bases.items():
        for gain, lo, hi in ((1.25, 0.25, 0.85), (2.0, 0.25, 0.85)):
            ref = oracle.gauss_rgba(big[0], k, weights=gt.scaled(base, gain), threads=_threads(oracle))
            share = float((ref == 255).mean())
            assert lo <= share <= hi, (k, gain, share)


def test_the_255_block_overflows_a_byte_from_the_first_clamp_gain_on(oracle, big, bases):
    h, w = big.shape[1:3]
    cy, cx = gt.block_centre(h, w, 255)
    crop = np.ascontiguousarray(big[0, :cy + 20, :cx + 20])
    for (k, s), base in bases.items():
        for gain in (1.0035, 1.0038, 1.0039):
            t = gt.scaled(base, gain)
            ref = oracle.gauss_rgba(crop, k, weights=t)
            assert ref[cy, cx, :3].tolist() == [255, 255, 255], (k, gain)
        assert 255.0 * float(gt.scaled(base, 1.0039).astype(np.float64).sum()) >= 255.9, k
        assert 255.0 * float(gt.scaled(base, 1.0038).astype(np.float64).sum()) < 256.0, k


def test_half_gain_and_hundredfold_gain(oracle, bases):
    h, w = 97, 250
    x = gt.frames(h, w, seed=97250)
    for (k, s), base in bases.items():
        ref = oracle.gauss_rgba(x[1], k, weights=gt.scaled(base, 0.5), threads=_threads(oracle))
        assert (ref[..., 3] == 127).all(), k
        ref = oracle.gauss_rgba(x[0], k, weights=gt.scaled(base, 100.0), threads=_threads(oracle))
        far = ~_near_block(h, w, 0, k // 2)
        assert (ref[far] == 255).all(), k
        assert ref[~far][..., :3].min() == 0, k      # and the block itself stays black
