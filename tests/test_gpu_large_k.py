"""GPU suite (-m gpu): Gaussian window sizes 19 .. 63 on every kernel that takes them, against the CPU path.

include/mi355_imgfilter.h promises the Gaussian for every odd k <= MI355_MAX_GAUSS_K = 63.  Above 17 only the runtime-k
LDS-tiled kernels serve it, and their LDS carve grows with k.  large_k_cases.py holds the sizes (KS, one reason each),
the sigmas (0.35: the centre tap, dense exception flags; k / 6; 50: a box, the widest error bound), the shapes (several
ragged tiles, one tile, frames smaller than the radius) and their content (noise, 0 / 255, flat 70 x 70 patches with
noise between them); test_large_k_cpu.py asserts every number below from the restated formulas.

Which kernel each call reaches and how much dynamic LDS it carves (bytes; * = above the 64 KiB a kernel gets without
launch_tiles(..., kLdsRaise) raising its limit):

  RGBA Gaussian, every impl (AUTO, TILE, VALU, MFMA all end in gauss_tile above 17): gauss_tile_kernel<EXACT>
  RGBA pipeline, AUTO and TILE: pipeline_tile_kernel<EXACT>
  single channel: gray8_tile_kernel<op, 0, gm>, gm = kGmSep for the FAST Gaussian; for the EXACT Gaussian and the
  pipeline (both modes) kGmTap under TILE and, under AUTO, kGmExc while delta_bound_k < 0.01, else kGmTap

      k   gauss_tile     pipeline_tile    gray8 Gaussian              gray8 pipeline     kGmExc under AUTO at
          FAST    EXACT  FAST    EXACT    kGmSep  kGmExc   kGmTap     kGmExc    kGmTap   sigma 0.35  k / 6  50
     19   32220   12596  22972   18292    57744   59200    24128      71088*    33552    yes         yes    yes
     25   36708   16580  26452   22372    60272   62784    26944      74720*    36368    yes         yes    yes
     27   38268   18036  27676   23860    61104   64032    27936      75984*    37360    yes         yes    yes
     33   43140   22788  31540   28708    63632   68000*   31136      81056*    41616    yes         yes    yes
     45   53748   34020  40132   40132    69888*  78000*   39600      90128*    49056    yes         yes    no
     49   57540   38276  43252   44452    71632*  81248*   42336      94720*    53104    yes         no     no
     57   65508   47556  49876   53860    76528*  (none)   49600      (none)    59088    no          no     no
     59   67580*  50036  51612   56372    77424*  (none)   51168      (none)    60656    no          no     no
     63   71820*  55188  55180   61588    79232*  (none)   54416      (none)    63904    no          no     no

  The three thresholds inside the range: gauss_tile FAST passes 64 KiB between 57 (65,508 B) and 59 (67,580 B), the only
  RGBA launches that need the raised limit; delta_bound_k of a generated table passes 0.01 between k = 45 (0.0083 /
  0.0096 / 0.0107 at the three sigmas) and k = 49 (0.0098 / 0.0113 / 0.0127), so the exception arithmetic runs with a
  bound up to 0.0098 of the 0.01 it accepts; image mode leaves its LDS-tiled kernel after kImgMaxFastK = 25 and runs
  image2d_gauss_kernel, one thread per pixel and no LDS, at 27, 33 and 63.

Bars, the project's own: EXACT Gaussian, both pipelines and gauss_gray8 EXACT bit-identical to the CPU path; FAST
Gaussian within 1 LSB of it, and under every impl the same bytes; the FAST tiled RGBA pipeline the same bytes as the
three FAST calls chained (its distance to the CPU chain is not asserted above 17: test_gpu_gauss_tables.py says why).

Measured on an MI355X: the whole file (32 tests) 5.9 s; the slowest test is test_gray8_gaussian_and_pipeline[63] at
0.94 s, nearly all of it the CPU references; no RGBA test takes more than 0.10 s.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import large_k_cases as lk

pytestmark = pytest.mark.gpu

WORKERS = 12


@pytest.fixture(scope="module")
def rgba():
    """[(shape, batch)]: every batch of every RGBA shape, built once."""
    return [(shape, x) for shape in lk.RGBA_SHAPES for x in lk.rgba_batches(shape)]


@pytest.fixture(scope="module")
def planes():
    return [(shape, y) for shape in lk.G8_SHAPES for y in lk.g8_batches(shape)]


@pytest.fixture(autouse=True)
def _restore_selection(ctx, pkg):
    yield
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)


def _per_frame(fn, batches, k):
    """{(batch index, sigma): the CPU path's result of every frame, stacked}, on a few host threads."""
    jobs = [(b, s, f) for b, (_, x) in enumerate(batches) for s in lk.SIGMAS(k) for f in range(x.shape[0])]
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        done = dict(zip(jobs, pool.map(lambda j: fn(batches[j[0]][1][j[2]], k, j[1]), jobs)))
    return {(b, s): np.stack([done[b, s, f] for f in range(x.shape[0])])
            for b, (_, x) in enumerate(batches) for s in lk.SIGMAS(k)}


def _impls(pkg, *names):
    return [(n, getattr(pkg, "IMPL_" + n)) for n in names]


# ---- 1. RGBA Gaussian ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", lk.KS)
def test_rgba_gaussian(ctx, pkg, oracle, rgba, k):
    refs = _per_frame(oracle.gauss_rgba, rgba, k)
    rep = lk.Report()
    for b, (shape, x) in enumerate(rgba):
        for sigma in lk.SIGMAS(k):
            ref, tag = refs[b, sigma], (k, round(sigma, 3), shape, b)
            ctx.set_gauss_mode(pkg.GAUSS_EXACT)
            for name, impl in _impls(pkg, "AUTO", "TILE"):
                ctx.set_impl(impl)
                rep.same(ctx.gauss(x, k, sigma), ref, tag, "gauss EXACT", name)
            ctx.set_gauss_mode(pkg.GAUSS_FAST)
            fast = {}
            for name, impl in _impls(pkg, "AUTO", "TILE", "VALU", "MFMA"):
                ctx.set_impl(impl)
                fast[name] = ctx.gauss(x, k, sigma)
                rep.within(fast[name], ref, 1, tag, "gauss FAST vs CPU", name)
            for name in ("AUTO", "VALU", "MFMA"):
                rep.same(fast[name], fast["TILE"], tag, "gauss FAST %s vs TILE" % name)
    rep.done()


# ---- 2. RGBA pipeline ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", lk.KS)
def test_rgba_pipeline(ctx, pkg, oracle, rgba, k):
    refs = _per_frame(oracle.pipeline_rgba, rgba, k)
    rep = lk.Report()
    for b, (shape, x) in enumerate(rgba):
        for sigma in lk.SIGMAS(k):
            ref, tag = refs[b, sigma], (k, round(sigma, 3), shape, b)
            ctx.set_gauss_mode(pkg.GAUSS_EXACT)
            for name, impl in _impls(pkg, "AUTO", "TILE"):
                ctx.set_impl(impl)
                rep.same(ctx.pipeline(x, k, sigma), ref, tag, "pipeline EXACT", name)
            ctx.set_gauss_mode(pkg.GAUSS_FAST)
            ctx.set_impl(pkg.IMPL_TILE)
            chained = ctx.sobel(ctx.gauss(ctx.gray(x), k, sigma))
            for name, impl in _impls(pkg, "AUTO", "TILE"):
                ctx.set_impl(impl)
                rep.same(ctx.pipeline(x, k, sigma), chained, tag, "pipeline FAST vs the three FAST calls chained", name)
    rep.done()


# ---- 3. single-channel Gaussian and pipeline -------------------------------------------------------------------------
@pytest.mark.parametrize("k", lk.KS)
def test_gray8_gaussian_and_pipeline(ctx, pkg, oracle, planes, k):
    blurred = _per_frame(lambda y, k_, s: lk.gauss_plane(oracle, y, k_, s), planes, k)
    rep = lk.Report()
    for b, (shape, y) in enumerate(planes):
        for sigma in lk.SIGMAS(k):
            ref, tag = blurred[b, sigma], (k, round(sigma, 3), shape, b)
            edges = np.stack([oracle.sobel_gray(g) for g in ref])
            for name, impl in _impls(pkg, "AUTO", "TILE"):
                ctx.set_impl(impl)
                ctx.set_gauss_mode(pkg.GAUSS_EXACT)
                rep.same(ctx.gauss_gray8(y, k, sigma), ref, tag, "gauss_gray8 EXACT", name)
                rep.same(ctx.pipeline_gray8(y, k, sigma), edges, tag, "pipeline_gray8 EXACT", name)
                ctx.set_gauss_mode(pkg.GAUSS_FAST)
                rep.within(ctx.gauss_gray8(y, k, sigma), ref, 1, tag, "gauss_gray8 FAST", name)
                rep.same(ctx.pipeline_gray8(y, k, sigma), edges, tag, "pipeline_gray8 FAST", name)
    rep.done()


# ---- 4. image mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", lk.IMAGE_KS)
def test_image_mode_per_pixel_kernel(ctx, pkg, oracle, k):
    sigma = k / 6.0
    rep = lk.Report()
    for h, w in ((37, 150), (3, 5)):
        x = lk.rgba_frames(h, w, 1, h * 1000 + w)[0]
        got, _ = ctx.image2d(pkg.FILTER_GAUSS, x, k, sigma)
        rep.same(got[None], oracle.image2d_gauss(x, k, sigma)[None], (k, h, w), "image2d gauss")
    rep.done()


# ---- 5. other entry points -------------------------------------------------------------------------------------------
def test_streamed_calls_equal_the_batched_calls_at_the_maximum_size(ctx, pkg):
    """mi355_filter_stream with chunks of 2 frames on the 3-frame batch, k = 63: the second chunk holds one frame."""
    k, sigma = 63, 63 / 6.0
    x = lk.rgba_batches(lk.RGBA_BIG)[0]
    y = np.ascontiguousarray(np.moveaxis(x[0, ..., :3], -1, 0))     # three planes of (37, 150)
    assert x.shape[0] == 3 and y.shape == (3,) + x.shape[1:3]
    rep = lk.Report()
    for mode_name, mode in (("FAST", pkg.GAUSS_FAST), ("EXACT", pkg.GAUSS_EXACT)):
        ctx.set_gauss_mode(mode)
        out, _ = ctx.stream(pkg.FILTER_GAUSS, x, k=k, sigma=sigma, chunk_frames=2)
        rep.same(out, ctx.gauss(x, k, sigma), mode_name, "stream FILTER_GAUSS")
        out, _ = ctx.stream(pkg.FILTER_PIPELINE_GRAY8, y, k=k, sigma=sigma, chunk_frames=2)
        rep.same(out, ctx.pipeline_gray8(y, k, sigma), mode_name, "stream FILTER_PIPELINE_GRAY8")
    rep.done()


def test_a_small_window_after_the_largest_one(ctx, pkg, oracle):
    """launch_tiles sets a kernel's dynamic-LDS limit to the carve of each launch: after k = 63 (gauss_tile FAST 71,820 B,
    gray8 kGmSep 79,232 B) a k = 5 launch of the same kernels lowers it to a few KiB again, and must give what it gave
    before.  IMPL_TILE, so that k = 5 runs the runtime-k kernels that k = 63 ran."""
    x = lk.rgba_batches(lk.RGBA_BIG)[0]
    y = np.ascontiguousarray(np.moveaxis(x[0, ..., :3], -1, 0))

    def run(k, sigma):
        out = {}
        for impl_name, impl in _impls(pkg, "TILE", "AUTO"):
            ctx.set_impl(impl)
            for mode_name, mode in (("FAST", pkg.GAUSS_FAST), ("EXACT", pkg.GAUSS_EXACT)):
                ctx.set_gauss_mode(mode)
                out[impl_name, mode_name, "gauss"] = ctx.gauss(x, k, sigma)
                out[impl_name, mode_name, "pipeline"] = ctx.pipeline(x, k, sigma)
                out[impl_name, mode_name, "gauss_gray8"] = ctx.gauss_gray8(y, k, sigma)
                out[impl_name, mode_name, "pipeline_gray8"] = ctx.pipeline_gray8(y, k, sigma)
        return out

    before = run(5, 1.5)
    run(63, 63 / 6.0)
    after = run(5, 1.5)
    rep = lk.Report()
    for key in before:
        rep.same(after[key], before[key], key, "k = 5 after k = 63 vs before")
    ref = np.stack([oracle.gauss_rgba(f, 5, 1.5) for f in x])
    ref_y = np.stack([lk.gauss_plane(oracle, p, 5, 1.5) for p in y])
    for impl_name in ("TILE", "AUTO"):
        rep.same(after[impl_name, "EXACT", "gauss"], ref, impl_name, "k = 5 after k = 63, gauss EXACT vs CPU")
        rep.within(after[impl_name, "FAST", "gauss"], ref, 1, impl_name, "k = 5 after k = 63, gauss FAST vs CPU")
        rep.same(after[impl_name, "EXACT", "gauss_gray8"], ref_y, impl_name, "k = 5 after k = 63, gauss_gray8 EXACT vs CPU")
        rep.same(after[impl_name, "EXACT", "pipeline"], np.stack([oracle.pipeline_rgba(f, 5, 1.5) for f in x]), impl_name,
                 "k = 5 after k = 63, pipeline EXACT vs CPU")
        rep.same(after[impl_name, "EXACT", "pipeline_gray8"], np.stack([oracle.sobel_gray(g) for g in ref_y]), impl_name,
                 "k = 5 after k = 63, pipeline_gray8 EXACT vs CPU")
    rep.done()
