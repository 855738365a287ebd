"""GPU suite (-m gpu): batches of thousands of tiny frames through every filter (cases and reasons: tiny_batch_cases.py).

Frames smaller than a lane's quad, a 16-byte vector, a strip, a tile or a band, back to back with no padding, by the
thousand: every frame's first and last row is a frame boundary some other wave owns the far side of, consecutive frames
start at every byte alignment, and the launches have enough work items for the production band plans (12 rows for the
Gaussian at k = 3, 15 and 24 at k = 5, 16 for Sobel, gauss_exact's and pipe_slide's own) that the rest of the suite only
meets in launches of gigabytes.  The frame counts stand on either side of each launch-size rule (2800 work items,
2^16 pixels for the matrix cores, 4096 work items for resize); test_tiny_batch_cpu.py ties them to the rules, nothing
here asserts which kernel ran.

Every call is device-resident through the guarded arena (tests/guarded.py) at offsets (0, 0) and at the one other pair
the header allows per pixel size, (4, 4) for 4-byte pixels and (3, 1) for 1-byte planes: the payload is prefilled
128 away from the expected bytes, so a byte that is never written, or a byte stored into a neighbour's frame, fails
deterministically, and the guards catch the batch's two ends.  A batch repeats 11 frames whose neighbours draw from
other byte ranges, with a first and a last frame of their own; the CPU reference is computed once per distinct frame and
EVERY frame, row and byte of the GPU result is compared with it.

No new tolerances: bit-identity with the CPU path everywhere, except the FAST Gaussian, which is within 1 LSB of it and
gives the same bytes under IMPL_VALU and IMPL_TILE.  Where the FAST pipeline runs on the tiled kernel (IMPL_TILE, w < 4
or h < 2) it is the three FAST calls chained (include/mi355_imgfilter.h), as in test_gpu_guarded.py.
"""
import numpy as np
import pytest

import guarded
import tiny_batch_cases as tb
from hist_ref import equalize_ref, hist_ref, otsu_ref, otsu_thresholds_ref
from median_ref import median_ref
from morph_ref import OPS, morph_ref
from resize_ref import AREA, LINEAR, NEAREST, accepts, resize_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _reset_kernel_selection(ctx, pkg):
    yield
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_input_format(pkg.INPUT_RGBA)


_refs = {}


def ref_of(key, make):
    """One CPU reference per (filter, parameters, shape): (NDISTINCT, ...), shared by every test, never modified."""
    if key not in _refs:
        _refs[key] = np.ascontiguousarray(make())
        _refs[key].setflags(write=False)
    return _refs[key]


def each(fn, frames):
    return np.stack([fn(f) for f in frames])


def compare(got, expected, tol, tag):
    """guarded.check on the whole payload; a failure also names the frame, row and byte."""
    try:
        guarded.check(got, expected, tol, tag)
    except guarded.PayloadError as e:
        frame_bytes = expected[0].size * expected.itemsize
        row_bytes = frame_bytes // expected.shape[1] if expected.ndim > 2 else frame_bytes
        raise AssertionError("%s: %s" % (e, tb.where(e.index, frame_bytes, row_bytes))) from None


# (off_in, off_out): 16-byte aligned, and the one other pair per pixel size: 4-byte pixels on a dword that is no multiple
# of 16 (the RAGGED sliding kernels, with band plans of their own), 1-byte planes on odd bytes
OFFSETS = {4: ((0, 0), (4, 4)), 1: ((0, 0), (3, 1))}


def run(ctx, filt, x, expected, k=0, sigma=0.0, tol=0, tag="", against=None, off=(0, 0)):
    """mi355_filter_dev on the batch x through the arena, prefilled from `expected`; every byte within tol of it (and
    within 1 of `against`, the CPU path, where `expected` is another kernel's result).  Returns the payload."""
    n, h, w = x.shape[:3]
    tag = "%s filter %d k %d (h, w, n) = (%d, %d, %d) off %s" % (tag, filt, k, h, w, n, off)
    got = guarded.run(ctx, lambda a, b: ctx.filter_dev(filt, a, b, w, h, n, k, sigma), x, expected, off[0], off[1], tag=tag)
    compare(got, expected, tol, tag)
    if against is not None:
        compare(got, against, 1, tag + " (against the CPU path)")
    return got


def counts_to_run(family, shape):
    """n_hi for every shape, n_lo before it for the threshold shapes."""
    n_lo, n_hi = tb.counts(family, shape)
    return ([n_lo] if n_lo is not None and shape in tb.THRESHOLD_SHAPES else []) + [n_hi]


def gauss_ref(oracle, shape, k):
    d = tb.distinct(shape[0], shape[1], 4)
    return ref_of(("gauss", shape, k), lambda: each(lambda f: oracle.gauss_rgba(f, k, tb.SIGMA[k]), d))


# ---- Gaussian ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 17])
def test_gauss_fast_valu_and_tile(ctx, pkg, oracle, k):
    """gauss_slide (k 3, 5; its two-kernel form for k 7, 9), gauss_wide (k 11, 17, even widths) and the tiled kernel:
    within 1 LSB of the CPU path, and VALU gives the tiled kernel's bytes.  Frames with noise, constant 255 and
    constant 77 in alpha share every launch."""
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        ref14 = gauss_ref(oracle, shape, k)
        for n in counts_to_run(("gauss", k), shape):
            x, ref = tb.batch(h, w, n, 4), tb.expand(ref14, n)
            ctx.set_impl(pkg.IMPL_TILE)
            tiled = run(ctx, pkg.FILTER_GAUSS, x, ref, k, tb.SIGMA[k], 1, "tile")
            ctx.set_impl(pkg.IMPL_VALU)
            for off in OFFSETS[4]:
                run(ctx, pkg.FILTER_GAUSS, x, tiled, k, tb.SIGMA[k], 0, "valu", against=ref, off=off)


@pytest.mark.parametrize("order", ["shrinking", "growing"])
@pytest.mark.parametrize("k", [7, 9])
def test_gauss_two_kernel_flags_sized_by_another_plan(pkg, oracle, k, order):
    """k = 7, 9 run an opaque pass and a general pass that talk through one flag per work item in the context's pooled
    buffer.  A context of its own per order: n_hi before n_lo (the buffer is larger than the second launch needs, its
    tail holds the first launch's flags) and n_lo before n_hi (it has to grow)."""
    shapes = [s for s in tb.THRESHOLD_SHAPES if tb.counts(("gauss", k), s)[0] is not None]
    assert len(shapes) >= 4
    with pkg.Context(0) as own:
        own.set_gauss_mode(pkg.GAUSS_FAST)
        own.set_impl(pkg.IMPL_VALU)
        for shape in (shapes[::-1] if order == "shrinking" else shapes):
            h, w = shape
            n_lo, n_hi = tb.counts(("gauss", k), shape)
            ref14 = gauss_ref(oracle, shape, k)
            for n in ((n_hi, n_lo) if order == "shrinking" else (n_lo, n_hi)):
                run(own, pkg.FILTER_GAUSS, tb.batch(h, w, n, 4), tb.expand(ref14, n), k, tb.SIGMA[k], 1, order)


@pytest.mark.parametrize("impl", ["AUTO", "MFMA"])
@pytest.mark.parametrize("k", [7, 17])
def test_gauss_matrix_core_rule(ctx, pkg, oracle, k, impl):
    """16 x 64 frames on both sides of 2^16 pixels: under AUTO 63 frames stay on the VALU kernels and 64 go to the matrix
    cores, under IMPL_MFMA both do.  Within 1 LSB of the CPU path."""
    h, w = tb.MATRIX_SHAPE
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    ref14 = gauss_ref(oracle, tb.MATRIX_SHAPE, k)
    for n in tb.MATRIX_COUNTS + (2800,):
        for off in OFFSETS[4]:                                # off 16 bytes the matrix-core kernel does not apply
            run(ctx, pkg.FILTER_GAUSS, tb.batch(h, w, n, 4), tb.expand(ref14, n), k, tb.SIGMA[k], 1, impl, off=off)


@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_gauss_exact(ctx, pkg, oracle, k, impl):
    """gauss_exact (widths that are multiples of 4) and the tiled kernel: the CPU path's bytes."""
    ctx.set_gauss_mode(pkg.GAUSS_EXACT)
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        ref14 = gauss_ref(oracle, shape, k)
        for n in counts_to_run(("exact", k), shape):
            x, ref = tb.batch(h, w, n, 4), tb.expand(ref14, n)
            for off in OFFSETS[4]:
                run(ctx, pkg.FILTER_GAUSS, x, ref, k, tb.SIGMA[k], 0, "exact " + impl, off=off)


# ---- Sobel, pipeline, gray ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
def test_sobel(ctx, pkg, oracle, impl):
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        ref14 = ref_of(("sobel", shape), lambda: each(oracle.sobel_rgba, tb.distinct(h, w, 4)))
        for n in counts_to_run(("sobel", 0), shape):
            x, ref = tb.batch(h, w, n, 4), tb.expand(ref14, n)
            for off in OFFSETS[4]:
                run(ctx, pkg.FILTER_SOBEL, x, ref, tag=impl, off=off)


def _fast_chain(ctx, pkg, oracle, shape, k):
    """sobel(gauss(gray(x))) of the distinct frames: the three FAST calls chained, each through the arena against the CPU
    path of its own input."""
    def make():
        d = tb.distinct(shape[0], shape[1], 4)
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        ctx.set_impl(pkg.IMPL_TILE)
        gray = run(ctx, pkg.FILTER_GRAY, d, each(oracle.gray_rgba, d), tag="chain")
        blur_ref = each(lambda f: oracle.gauss_rgba(f, k, tb.SIGMA[k]), gray)
        blur = run(ctx, pkg.FILTER_GAUSS, gray, blur_ref, k, tb.SIGMA[k], 1, "chain")
        return run(ctx, pkg.FILTER_SOBEL, blur, each(oracle.sobel_rgba, blur), tag="chain")
    return ref_of(("chain", shape, k), make)


@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_pipeline(ctx, pkg, oracle, k, impl):
    """pipe_slide (w >= 4, h >= 2) gives the CPU chain's bytes in both Gaussian modes, the tiled kernel in EXACT mode; the
    FAST tiled kernel gives the three FAST calls chained."""
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        d = tb.distinct(h, w, 4)
        ref14 = ref_of(("pipe", shape, k), lambda: each(lambda f: oracle.pipeline_rgba(f, k, tb.SIGMA[k]), d))
        slides = impl == "AUTO" and w >= 4 and h >= 2
        fast14 = ref14 if slides else _fast_chain(ctx, pkg, oracle, shape, k)
        ctx.set_impl(getattr(pkg, "IMPL_" + impl))
        for n in counts_to_run(("pipe", k), shape):
            x = tb.batch(h, w, n, 4)
            for off in OFFSETS[4]:
                ctx.set_gauss_mode(pkg.GAUSS_EXACT)
                run(ctx, pkg.FILTER_PIPELINE, x, tb.expand(ref14, n), k, tb.SIGMA[k], 0, impl + " exact", off=off)
                ctx.set_gauss_mode(pkg.GAUSS_FAST)
                run(ctx, pkg.FILTER_PIPELINE, x, tb.expand(fast14, n), k, tb.SIGMA[k], 0, impl + " fast", off=off)


def test_gray_and_bgr(ctx, pkg, oracle):
    for shape in tb.RGBA_SHAPES:
        h, w = shape
        n = tb.tile_count(h, w, 4)
        d, x = tb.distinct(h, w, 4), tb.batch(h, w, n, 4)
        for off in OFFSETS[4]:
            run(ctx, pkg.FILTER_GRAY, x, tb.expand(ref_of(("gray", shape), lambda: each(oracle.gray_rgba, d)), n), off=off)
            run(ctx, pkg.FILTER_GRAY1, x, tb.expand(ref_of(("gray1", shape), lambda: each(oracle.gray_rgba_1ch, d)), n),
                off=off)
        bgr = np.ascontiguousarray(x[..., :3])                # 3-byte pixels: frames start at every byte alignment
        ref = np.concatenate([bgr[..., ::-1], np.full((n, h, w, 1), 255, np.uint8)], axis=-1)
        tag = "bgr (h, w, n) = (%d, %d, %d)" % (h, w, n)
        got = guarded.run(ctx, lambda a, b: ctx.bgr_to_rgba_dev(a, b, w, h, n), bgr, ref, 0, 0, tag=tag)
        compare(got, ref, 0, tag)


# ---- median and morphology, RGBA and gray8 -------------------------------------------------------------------------------
def _planes(bpp):
    return tb.RGBA_SHAPES if bpp == 4 else tb.G8_SHAPES


@pytest.mark.parametrize("bpp", [4, 1], ids=["rgba", "gray8"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_median(ctx, pkg, k, bpp):
    filt = pkg.FILTER_MEDIAN if bpp == 4 else pkg.FILTER_MEDIAN_GRAY8
    for shape in _planes(bpp):
        h, w = shape
        n = tb.tile_count(h, w, bpp)
        ref14 = ref_of(("median", shape, k, bpp), lambda: each(lambda f: median_ref(f, k), tb.distinct(h, w, bpp)))
        x, ref = tb.batch(h, w, n, bpp), tb.expand(ref14, n)
        for impl in (pkg.IMPL_AUTO, pkg.IMPL_TILE):           # compare networks (k 3, 5) / the LDS counting kernel
            ctx.set_impl(impl)
            for off in OFFSETS[bpp]:
                run(ctx, filt, x, ref, k, tag="impl %d" % impl, off=off)


@pytest.mark.parametrize("bpp", [4, 1], ids=["rgba", "gray8"])
@pytest.mark.parametrize("k", [3, 9, 17])
@pytest.mark.parametrize("op", OPS)
def test_morphology(ctx, pkg, op, k, bpp):
    filt = getattr(pkg, "FILTER_" + op.upper() + ("" if bpp == 4 else "_GRAY8"))
    for shape in _planes(bpp):
        h, w = shape
        n = tb.tile_count(h, w, bpp)
        ref14 = ref_of((op, shape, k, bpp), lambda: each(lambda f: morph_ref(op, f, k), tb.distinct(h, w, bpp)))
        x, ref = tb.batch(h, w, n, bpp), tb.expand(ref14, n)
        for off in OFFSETS[bpp]:
            run(ctx, filt, x, ref, k, tag=op, off=off)


# ---- the single-channel Gaussian, Sobel and their chain ------------------------------------------------------------------
def _blur_plane(oracle, y, k):
    rgba = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
    return np.ascontiguousarray(oracle.gauss_rgba(rgba, k, tb.SIGMA[k])[..., 0])


def _g8_blur_ref(oracle, shape, k):
    return ref_of(("g8 gauss", shape, k), lambda: each(lambda f: _blur_plane(oracle, f, k), tb.distinct(shape[0], shape[1], 1)))


@pytest.mark.parametrize("k", [5, 9])
def test_gauss_gray8(ctx, pkg, oracle, k):
    for shape in tb.G8_SHAPES:
        h, w = shape
        n = tb.tile_count(h, w, 1)
        x, ref = tb.batch(h, w, n, 1), tb.expand(_g8_blur_ref(oracle, shape, k), n)
        for off in OFFSETS[1]:
            ctx.set_gauss_mode(pkg.GAUSS_EXACT)
            run(ctx, pkg.FILTER_GAUSS_GRAY8, x, ref, k, tb.SIGMA[k], 0, "exact", off=off)
            ctx.set_gauss_mode(pkg.GAUSS_FAST)
            run(ctx, pkg.FILTER_GAUSS_GRAY8, x, ref, k, tb.SIGMA[k], 1, "fast", off=off)


def test_sobel_gray8(ctx, pkg, oracle):
    for shape in tb.G8_SHAPES:
        h, w = shape
        n = tb.tile_count(h, w, 1)
        ref14 = ref_of(("g8 sobel", shape), lambda: each(oracle.sobel_gray, tb.distinct(h, w, 1)))
        x, ref = tb.batch(h, w, n, 1), tb.expand(ref14, n)
        for off in OFFSETS[1]:
            run(ctx, pkg.FILTER_SOBEL_GRAY8, x, ref, off=off)


@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
@pytest.mark.parametrize("k", [3, 5, 9])
def test_pipeline_gray8(ctx, pkg, oracle, k, impl):
    """sobel(EXACT gauss(y)) in either Gaussian mode."""
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    for shape in tb.G8_SHAPES:
        h, w = shape
        n = tb.tile_count(h, w, 1)
        ref14 = ref_of(("g8 pipe", shape, k), lambda: each(oracle.sobel_gray, _g8_blur_ref(oracle, shape, k)))
        x, ref = tb.batch(h, w, n, 1), tb.expand(ref14, n)
        for mode in (pkg.GAUSS_EXACT, pkg.GAUSS_FAST):
            ctx.set_gauss_mode(mode)
            for off in OFFSETS[1]:
                run(ctx, pkg.FILTER_PIPELINE_GRAY8, x, ref, k, tb.SIGMA[k], 0, "%s mode %d" % (impl, mode), off=off)


# ---- whole-frame statistics ------------------------------------------------------------------------------------------------
def _stats(ctx, call, x, expected, tag):
    """A statistics call (n x 256 uint32 counts, or n int32 thresholds) through the arena, compared as bytes."""
    want = np.ascontiguousarray(expected).view(np.uint8).reshape(x.shape[0], -1)
    n, h, w = x.shape
    tag = "%s (h, w, n) = (%d, %d, %d)" % (tag, h, w, n)
    got = guarded.run(ctx, lambda a, b: call(a, b, w, h, n), x, want, 0, 0, tag=tag)
    compare(got, want, 0, tag)
    return got.view(expected.dtype).reshape(expected.shape)


def test_equalize_otsu_and_their_statistics(ctx, pkg):
    """One histogram, one table and one threshold per frame: thousands of frames first and 64 after them, so that the
    pooled histograms and tables are larger than the second call."""
    for shape in tb.G8_SHAPES:
        h, w = shape
        d = tb.distinct(h, w, 1)
        hist14 = ref_of(("hist", shape), lambda: hist_ref(d))
        thr14 = ref_of(("thr", shape), lambda: otsu_thresholds_ref(d))
        eq14 = ref_of(("equalize", shape), lambda: equalize_ref(d))
        otsu14 = ref_of(("otsu", shape), lambda: otsu_ref(d))
        for n in (tb.tile_count(h, w, 1), 64):
            x = tb.batch(h, w, n, 1)
            for off in OFFSETS[1]:
                run(ctx, pkg.FILTER_EQUALIZE_GRAY8, x, tb.expand(eq14, n), tag="equalize", off=off)
                run(ctx, pkg.FILTER_OTSU_GRAY8, x, tb.expand(otsu14, n), tag="otsu", off=off)
            _stats(ctx, ctx.hist_gray8_dev, x, tb.expand(hist14, n), "hist")
            thr = _stats(ctx, ctx.otsu_thresholds_gray8_dev, x, tb.expand(thr14, n), "thresholds")
            if shape == (1, 1):                               # a one-pixel frame equalizes to itself, threshold 0
                assert np.array_equal(tb.expand(eq14, n), x) and (thr == 0).all()


# ---- resize ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp", [4, 1], ids=["rgba", "gray8"])
@pytest.mark.parametrize("interp", [NEAREST, LINEAR, AREA], ids=["nearest", "linear", "area"])
def test_resize(ctx, interp, bpp):
    """Both sides of 4096 work items: 4095 frames run in bands cut finer than the frame, 4096 in 16-row bands."""
    ran = 0
    for sw, sh, dw, dh in tb.RESIZE_PAIRS:
        if not accepts(interp, sw, sh, dw, dh):
            continue
        ref14 = ref_of(("resize", sw, sh, dw, dh, interp, bpp),
                       lambda: each(lambda f: resize_ref(f, dw, dh, interp), tb.distinct(sh, sw, bpp)))
        for n in tb.RESIZE_COUNTS:
            x, ref = tb.batch(sh, sw, n, bpp), tb.expand(ref14, n)
            for off in OFFSETS[bpp]:
                tag = "resize %d bpp %d %dx%d -> %dx%d n %d off %s" % (interp, bpp, sw, sh, dw, dh, n, off)
                got = guarded.run(ctx, lambda a, b: ctx.resize_dev(a, b, bpp, sw, sh, dw, dh, n, interp), x, ref, off[0],
                                  off[1], tag=tag)
                compare(got, ref, 0, tag)
            ran += 1
    assert ran >= 12


# ---- host paths: the entry points pass such batches on unchanged -------------------------------------------------------------
HOST_SHAPE, HOST_N = (5, 7), 3001


def _device_result(ctx, filt, x, ref, k, sigma, tol):
    return run(ctx, filt, x, ref, k, sigma, tol, "device")


def test_host_batched_and_stream_rgba(ctx, pkg, oracle):
    h, w = HOST_SHAPE
    x = tb.batch(h, w, HOST_N, 4)
    ref = tb.expand(gauss_ref(oracle, HOST_SHAPE, 5), HOST_N)
    dev = _device_result(ctx, pkg.FILTER_GAUSS, x, ref, 5, tb.SIGMA[5], 1)
    assert np.array_equal(ctx.gauss(x, 5, tb.SIGMA[5]), dev)
    for chunk in (0, 1000):
        out, _ = ctx.stream(pkg.FILTER_GAUSS, x, k=5, sigma=tb.SIGMA[5], chunk_frames=chunk)
        assert np.array_equal(out, dev), chunk


def test_host_batched_stream_and_group_gray8(ctx, pkg):
    h, w = HOST_SHAPE
    x = tb.batch(h, w, HOST_N, 1)
    ref = tb.expand(ref_of(("median", HOST_SHAPE, 5, 1), lambda: each(lambda f: median_ref(f, 5), tb.distinct(h, w, 1))),
                    HOST_N)
    dev = _device_result(ctx, pkg.FILTER_MEDIAN_GRAY8, x, ref, 5, 0.0, 0)
    assert np.array_equal(ctx.median_gray8(x, 5), dev)
    for chunk in (0, 1000):
        out, _ = ctx.stream(pkg.FILTER_MEDIAN_GRAY8, x, k=5, chunk_frames=chunk)
        assert np.array_equal(out, dev), chunk
    # three members on one GPU: shards of 1001 / 1000 / 1000 frames of 35 bytes start at odd host byte offsets
    assert [pkg.group_shard(m, 3, HOST_N) for m in range(3)] == [(0, 1001), (1001, 1000), (2001, 1000)]
    with pkg.Group([0, 0, 0]) as g:
        out, _ = g.filter_batched(pkg.FILTER_MEDIAN_GRAY8, x, k=5)
    assert np.array_equal(out, dev)


def test_host_bgr_input(ctx, pkg, oracle):
    """BGR frames of 3 x 5 x 2800: the conversion and the Gaussian of the host path against the device-resident call on
    the same pixels as RGBA."""
    h, w, n = 3, 5, 2800
    x = tb.batch(h, w, n, 4).copy()
    x[..., 3] = 255
    d = tb.distinct(h, w, 4).copy()
    d[..., 3] = 255
    ref = tb.expand(each(lambda f: oracle.gauss_rgba(f, 5, tb.SIGMA[5]), d), n)
    dev = _device_result(ctx, pkg.FILTER_GAUSS, x, ref, 5, tb.SIGMA[5], 1)
    bgr = np.ascontiguousarray(x[..., 2::-1])
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        assert np.array_equal(ctx.gauss(bgr, 5, tb.SIGMA[5]), dev)
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
