"""GPU suite (-m gpu): every kernel that promises the CPU path's bytes, on frames built from integer-straddling windows.

The bit-exact Gaussian code — gauss_exact.hip, pipe_slide.hip at 4 and 8 pixels per lane, gray8.hip's kGmExc
instantiations, and the literal chains gauss_tile_kernel<EXACT>, pipeline_tile_kernel<EXACT> and kGmTap — differs from a
subtly wrong version of itself (another visiting order in the exception chain, a neighbour lane taken from the wrong
side, a contracted multiply-add, a bound delta that is too small) only where the CPU sum sits within ~1e-5 of an
integer: less than one value per (pixel position, walking direction, ring slot) in the noise frames of the other suites.
The frames here (straddle_cases.py) are tiled with mined windows on which each such fault provably changes the byte;
test_straddle_cpu.py shows that every frame used below loses at least 16 bytes (8 of the pipeline's edge image) to every
alternate.  Every comparison is np.array_equal against the oracle; a failure names the alternates whose bytes the GPU
produced instead.

Which kernel each call reaches is listed in test_gpu_gauss_tables.py; in short, under AUTO:
  RGBA Gaussian EXACT  k 3, 5, 7 on (131, 512): gauss_exact (4-channel and opaque walks); (97, 250), k 9, 17, TILE: tiled
  RGBA pipeline        k 3, 5, 7: pipe_slide with 4 pixels per lane (RAGGED on (97, 250)); TILE: pipeline_tile
                       8 pixels per lane: the tuning build with MI355_PIPE8=1 in a child process
  gray8                k 3, 5, 7: constant-k kGmExc in both modes; k 9, 17, 33: runtime-k kGmExc; TILE: kGmTap
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import __graft_entry__ as entry
import straddle_cases as sc
from large_k_cases import Report

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_selection(ctx, pkg):
    yield
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)


@pytest.fixture(scope="module")
def tables(oracle):
    return {k: oracle.gauss_weights(k, s) for k, s in sc.SIZES}


def _map(fn, jobs):
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(fn, jobs))


def _channels_first(x):
    return np.moveaxis(x, -1, 1)


class _Check:
    """Report plus the diagnosis: a failed comparison says which alternates the GPU's bytes agree with."""

    def __init__(self, w2):
        self.rep, self.w2 = Report(), w2

    def same(self, got, ref, planes, post, *tag):
        n = len(self.rep.bad)
        self.rep.same(got, ref, *tag)
        if len(self.rep.bad) > n and planes is not None:
            if got.ndim == 4:      # RGBA: one blurred plane per channel
                got, ref, planes = _channels_first(got), _channels_first(ref), _channels_first(planes)
            self.rep.bad[-1] += "\n" + sc.matched_alternates(got, ref, planes, self.w2, post)

    def done(self):
        self.rep.done()


# ---- RGBA Gaussian ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9, 17])
def test_rgba_gaussian_on_straddle_frames(ctx, pkg, oracle, tables, k):
    """EXACT under AUTO and TILE equals the CPU path; FAST stays within 1 LSB under every selection and the VALU kernels
    equal the tiled one."""
    sigma, chk = sc.SIGMA[k], _Check(tables[k])
    cases = [(shape, kind, opaque) for shape in sc.gauss_rgba_shapes(k) for kind in sc.kinds_of(k) for opaque in (False, True)]
    batches = [sc.rgba_gauss_batch(kind, shape[0], shape[1], k, opaque) for shape, kind, opaque in cases]
    refs = _map(lambda x: np.stack([oracle.gauss_rgba(f, k, sigma) for f in x]), batches)
    for (shape, kind, opaque), x, ref in zip(cases, batches, refs):
        tag = (k, shape, kind, "opaque" if opaque else "4 channels")
        ctx.set_gauss_mode(pkg.GAUSS_EXACT)
        for name in ("AUTO", "TILE"):
            ctx.set_impl(getattr(pkg, "IMPL_" + name))
            chk.same(ctx.gauss(x, k, sigma), ref, x, None, tag, "gauss EXACT", name)
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        fast = {}
        for name in ("AUTO", "TILE", "VALU"):
            ctx.set_impl(getattr(pkg, "IMPL_" + name))
            fast[name] = ctx.gauss(x, k, sigma)
            chk.rep.within(fast[name], ref, 1, tag, "gauss FAST vs CPU", name)
        chk.rep.same(fast["VALU"], fast["TILE"], tag, "gauss FAST VALU vs TILE")
    chk.done()


# ---- RGBA pipeline ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sc.SLIDE_KS)
def test_rgba_pipeline_on_straddle_frames(ctx, pkg, oracle, tables, k):
    """AUTO (pipe_slide, 4 pixels per lane, aligned and RAGGED) in both modes and the tiled kernel in EXACT mode equal the
    CPU chain.  The tiled kernel's FAST mode is separable by contract: it equals the three FAST calls chained."""
    sigma, chk = sc.SIGMA[k], _Check(tables[k])
    post = sc.rgba_pipe_post(oracle)
    cases = [(shape, kind, col) for shape in sc.PIPE_SHAPES for kind in sc.kinds_of(k) for col in (False, True)]
    built = [sc.rgba_pipe_batch(oracle, kind, shape[0], shape[1], k, col) for shape, kind, col in cases]
    refs = _map(lambda b: np.stack([oracle.pipeline_rgba(f, k, sigma) for f in b[0]]), built)
    for (shape, kind, col), (x, planes), ref in zip(cases, built, refs):
        tag = (k, shape, kind, "coloured" if col else "grey")
        for mode in ("FAST", "EXACT"):
            ctx.set_gauss_mode(getattr(pkg, "GAUSS_" + mode))
            ctx.set_impl(pkg.IMPL_AUTO)
            chk.same(ctx.pipeline(x, k, sigma), ref, planes, post, tag, "pipeline AUTO", mode)
        ctx.set_impl(pkg.IMPL_TILE)
        chk.same(ctx.pipeline(x, k, sigma), ref, planes, post, tag, "pipeline TILE EXACT")
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        chained = ctx.sobel(ctx.gauss(ctx.gray(x), k, sigma))
        chk.rep.same(ctx.pipeline(x, k, sigma), chained, tag, "pipeline TILE FAST vs the three FAST calls chained")
    chk.done()


_PIPE8_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import straddle_cases as sc
pkg = entry.load_package(); oracle = entry.load_oracle()
bad = []
post = sc.rgba_pipe_post(oracle)
with pkg.Context(0) as ctx:
    for k in sc.PIPE8_KS:
        sigma, w2 = sc.SIGMA[k], oracle.gauss_weights(k, sc.SIGMA[k])
        cases = [(sc.SHAPE_PIPE8, kind, col) for kind in sc.kinds_of(k) for col in (False, True)] + [((2, 16), "dense", False)]
        for shape, kind, col in cases:
            x, planes = sc.rgba_pipe_batch(oracle, kind, shape[0], shape[1], k, col)
            ref = np.stack([oracle.pipeline_rgba(f, k, sigma) for f in x])
            for mode in ("FAST", "EXACT"):
                ctx.set_gauss_mode(getattr(pkg, "GAUSS_" + mode))
                got = ctx.pipeline(x, k, sigma)
                if not np.array_equal(got, ref):
                    bad.append("%r\n%s" % ((k, shape, kind, col, mode), sc.matched_alternates(got, ref, planes, w2, post)))
print("\n".join(bad))
print(len(bad))
"""


def test_rgba_pipeline_eight_pixels_per_lane_on_straddle_frames():
    """pipe_slide.hip's PX = 8 kernel, k = 3 and 5, both modes, forced by the tuning build (MI355_PIPE8=1) in a child
    process of its own as in test_gpu_configs.py: test_pipeline_eight_pixels_per_lane; (131, 1000) is three strips of 42
    lanes, (2, 16) the smallest frame the kernel takes."""
    tune_lib = os.path.join(entry.ROOT, "tools", "lib", "libmi355_imgfilter_tune.so")
    assert os.path.exists(tune_lib), "run __graft_entry__.build()"
    env = dict(os.environ, MI355_IMGFILTER_LIB=tune_lib, MI355_PIPE8="1")
    out = subprocess.run([sys.executable, "-c", _PIPE8_SCRIPT, entry.ROOT], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "0", out.stdout[-4000:]


# ---- single-channel filters ------------------------------------------------------------------------------------------
def _gray8_refs(oracle, tables, k):
    cases = [(shape, kind) for shape in sc.gray8_shapes(k) for kind in sc.kinds_of(k)]
    planes = [sc.plane_pair(kind, shape[0], shape[1], k) for shape, kind in cases]

    def blur(y):   # the R channel of the CPU Gaussian of (y, y, y, 255): test_gpu_gray8.py's gauss_r
        rgba = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
        return np.ascontiguousarray(oracle.gauss_rgba(rgba, k, weights=tables[k])[..., 0])
    flat = _map(blur, [y for pair in planes for y in pair])
    refs = [np.stack(flat[2 * i:2 * i + 2]) for i in range(len(cases))]
    return cases, planes, refs


@pytest.mark.parametrize("k", [k for k, _ in sc.SIZES])
def test_gauss_gray8_on_straddle_frames(ctx, pkg, oracle, tables, k):
    """EXACT under AUTO (kGmExc: constant k for 3, 5, 7, runtime k above) equals the CPU path; k = 3, 5, 7 do so in FAST
    mode too; the tap-by-tap kernel (TILE) for one small and one large k."""
    sigma, chk = sc.SIGMA[k], _Check(tables[k])
    cases, planes, refs = _gray8_refs(oracle, tables, k)
    for (shape, kind), y, ref in zip(cases, planes, refs):
        tag = (k, shape, kind)
        ctx.set_impl(pkg.IMPL_AUTO)
        ctx.set_gauss_mode(pkg.GAUSS_EXACT)
        chk.same(ctx.gauss_gray8(y, k, sigma), ref, y, None, tag, "gauss_gray8 EXACT AUTO")
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        fast = ctx.gauss_gray8(y, k, sigma)
        chk.rep.within(fast, ref, 1, tag, "gauss_gray8 FAST AUTO")
        if k in sc.SLIDE_KS:
            chk.same(fast, ref, y, None, tag, "gauss_gray8 FAST AUTO (exact by exception)")
        if k in (3, 33):
            ctx.set_impl(pkg.IMPL_TILE)
            ctx.set_gauss_mode(pkg.GAUSS_EXACT)
            chk.same(ctx.gauss_gray8(y, k, sigma), ref, y, None, tag, "gauss_gray8 EXACT TILE")
    chk.done()


@pytest.mark.parametrize("k", sc.GRAY8_PIPE_KS)
def test_pipeline_gray8_on_straddle_frames(ctx, pkg, oracle, tables, k):
    """The single-channel chain is the Sobel of the EXACT Gaussian in both modes, under AUTO (kGmExc) and TILE (kGmTap)."""
    sigma, chk = sc.SIGMA[k], _Check(tables[k])
    cases, planes, refs = _gray8_refs(oracle, tables, k)
    for (shape, kind), y, blurred in zip(cases, planes, refs):
        ref = np.stack([oracle.sobel_gray(b) for b in blurred])
        for impl in ("AUTO", "TILE"):
            ctx.set_impl(getattr(pkg, "IMPL_" + impl))
            for mode in ("FAST", "EXACT"):
                ctx.set_gauss_mode(getattr(pkg, "GAUSS_" + mode))
                chk.same(ctx.pipeline_gray8(y, k, sigma), ref, y, oracle.sobel_gray, (k, shape, kind), "pipeline_gray8", impl,
                         mode)
    chk.done()
