"""GPU suite (-m gpu): every Gaussian path on a (k, sigma) grid of generated tables and on installed tables whose gain
is not 1, against the CPU oracle.

Part 1 — generated tables.  mi355 accepts any finite sigma > 0; the exact-by-exception stage (exact_common.hpp, used by
gauss_exact.hip, pipe_slide.hip and gray8.hip's kGmExc kernels) is only correct if delta_bound_k() holds for the table in
use, the matrix-core kernel splits the weights into fp16 hi / lo parts, and the constant-alpha bytes are evaluated on
the host from the table.  At sigma = 0.2 the centre tap is 1 within rounding, every sum sits next to an integer and
5-15 % of all pixels are flagged: dense flags on content that is not flat.

Part 2 — installed tables = a generated table times a gain (gauss_tables_ref.GAINS; test_gauss_tables_cpu.py derives
what each gain reaches from the library's host formulas):
    0.5                no clamp; alpha 255 blurs to 127 through the constant-alpha tables
    1.0035             the largest class the matrix-core kernel accepts (intermediates next to the fp16 maximum)
    1.0038             no clamp in gauss_slide / pipe_slide (sums up to 255.97), CLAMP in gauss_exact; matrix cores refuse
    1.0039, 1.25, 2.0  the CLAMP instantiations of gauss_slide, gauss_exact and pipe_slide; many saturated bytes
    100                delta_bound_k >= 0.01: the exact-by-exception stage refuses the table
Bars as everywhere: EXACT Gaussian, pipeline and gray8 chain bit-identical to the CPU path, FAST within 1 LSB, the
VALU kernels bit-identical to the tiled kernel.

Which kernel each call is expected to reach (csrc/gauss.hip choose(), sobel_tile.hip launch_pipeline, gray8.hip).  In
every batch frame 0 (alpha noise) takes the 4-channel pass of the sliding-window kernels, frame 1 the opaque pass and
frame 2 (alpha 128) the constant-alpha pass.
  Gaussian FAST   TILE  any k, any shape                         gauss_tile, separable
                  VALU  k 3..9: (131, 512)                        gauss_slide aligned (k 7, 9: its two kernels with flags)
                                (97, 250), (53, 501)              gauss_slide RAGGED
                        k 11, 17: (131, 512), (97, 250)           gauss_wide;  (53, 501): gauss_tile
                        k 1, 31                                   gauss_tile
                        CLAMP instantiations of gauss_slide from gain 1.0039 on
                  MFMA  k 3..17 on (131, 512), generated tables and gains 0.5, 1.0035: gauss_mfma_reg<false>;
                        any other shape, k or gain: as VALU
                  AUTO  as MFMA for k 7..17, as VALU otherwise
  Gaussian EXACT  AUTO  k 3, 5, 7 on (131, 512), symmetric factor, gain <= 2: gauss_exact (CLAMP from gain 1.0038 on);
                        everything else, and TILE: gauss_tile tap by tap
  pipeline        AUTO  k 3, 5, 7, symmetric factor, gain <= 2: pipe_slide with 4 pixels per lane, RAGGED on (97, 250) and
                        (53, 501), CLAMP from gain 1.0039 on; everything else, and TILE: pipeline_tile (FAST: separable,
                        EXACT: tap by tap).  8 pixels per lane: the child-process test at the end
  gray8           AUTO  k 3, 5, 7: constant-k kernels, kGmExc in both modes and in the chain while delta_bound_k < 0.01
                        (gain <= 2); at gain 100 kGmSep (FAST Gaussian) and kGmTap (EXACT, chain).  Other k: runtime-k
                        kernels, kGmSep (FAST), kGmExc or kGmTap (EXACT, chain).  Asymmetric factor: kGmTap
                  TILE  runtime k, kGmSep (FAST Gaussian), kGmTap (EXACT, chain)
Not reached: the LOCKSTEP instantiations (launches of >= 8192 work items) and gauss_mfma_reg_kernel<true>, which no table
can select (test_gauss_tables_cpu.py: test_matrix_core_clamp_instantiation_has_no_table).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import __graft_entry__ as entry
import gauss_tables_ref as gt
from large_k_cases import Report as _Report
from test_gpu_parity import _mfma_takes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batches():
    return {(h, w): gt.frames(h, w, seed=h * 1000 + w) for h, w in gt.SHAPES}


@pytest.fixture(scope="module")
def own(pkg):
    """Installed tables are never evicted and a key keeps its table: they go into a context of this module's own."""
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _restore_selection(request, pkg):
    yield
    for name in ("ctx", "own"):
        if name in request.fixturenames:
            c = request.getfixturevalue(name)
            c.set_impl(pkg.IMPL_AUTO)
            c.set_gauss_mode(pkg.GAUSS_FAST)


def _references(oracle, batches, k, sigma=None, weights=None):
    """{shape: (gauss (3, h, w, 4), pipeline (3, h, w))} from the CPU path, frame by frame, on a few host threads."""
    def one(job):
        kind, shape, f = job
        fn = oracle.gauss_rgba if kind == "gauss" else oracle.pipeline_rgba
        return fn(batches[shape][f], k, sigma, weights=weights)
    jobs = [(kind, shape, f) for kind in ("gauss", "pipe") for shape in batches for f in range(3)]
    with ThreadPoolExecutor(max_workers=12) as pool:
        done = dict(zip(jobs, pool.map(one, jobs)))
    return {shape: (np.stack([done[("gauss", shape, f)] for f in range(3)]),
                    np.stack([done[("pipe", shape, f)] for f in range(3)])) for shape in batches}


def _away_from_the_255_block(h, w):
    """Where the tiled FAST pipeline is held to 6 grey levels of the CPU chain: everywhere but within one Sobel tap of
    the 255-block.  That bound is the effect of ONE blurred pixel being 1 LSB off (gx and gy move by at most 4 each).
    Over a window of 255s the sum is 255 within rounding and the CPU's float chain lands on 254 or 255 depending on the
    table (254 at (5, 3.0) and (7, 10.0), 255 at (3, 0.6)); the FAST arithmetic may land on the other one, which the
    1-LSB tolerance allows, and then EVERY blurred pixel of the block is 1 off.  Sobel's own luminance step doubles it
    (the CPU formula gives luma(254, 254, 254) = 253, luma(255, 255, 255) = 255), and along the block's straight edge a
    whole row of three taps differs: |d gx| = (1 + 2 + 1) * 2 = 8, measured |d| = 8..9 on about 270 pixels of the block's
    perimeter, reproduced with the CPU path alone by adding 1 to its own blurred block.  No kernel is wrong there, so this
    one comparison leaves those pixels out; they stay covered by the bit-identity of the same output with the three
    FAST calls chained, whose links are each compared with the CPU path."""
    y0, x0 = gt.block_origin(h, w, 255)
    away = np.ones((h, w), bool)
    away[max(0, y0 - 1):y0 + gt.BLOCK + 1, max(0, x0 - 1):x0 + gt.BLOCK + 1] = False
    return away


def _check_all_paths(c, pkg, oracle, rep, x, ref_gauss, ref_pipe, k, sigma, tag, mfma_table_ok=True, asymmetric=False):
    """Every entry that takes a Gaussian table, in both modes and under every kernel selection, on one batch."""
    n, h, w = x.shape[:3]
    impls = {"AUTO": pkg.IMPL_AUTO, "TILE": pkg.IMPL_TILE, "VALU": pkg.IMPL_VALU, "MFMA": pkg.IMPL_MFMA}
    # where the matrix-core kernel takes the launch (csrc/gauss.hip: choose)
    mfma_pinned = mfma_table_ok and 3 <= k <= 17 and w % 4 == 0
    mfma_auto = mfma_table_ok and 7 <= k <= 17 and _mfma_takes(h, w, n)

    # -- RGBA Gaussian
    c.set_gauss_mode(pkg.GAUSS_EXACT)
    for name in ("AUTO", "TILE"):
        c.set_impl(impls[name])
        rep.same(c.gauss(x, k, sigma), ref_gauss, tag, "gauss EXACT", name)
    c.set_gauss_mode(pkg.GAUSS_FAST)
    fast = {}
    for name, impl in impls.items():
        c.set_impl(impl)
        fast[name] = c.gauss(x, k, sigma)
        rep.within(fast[name], ref_gauss, 1, tag, "gauss FAST vs CPU", name)
    rep.same(fast["VALU"], fast["TILE"], tag, "gauss FAST VALU vs TILE")
    if not mfma_auto:
        rep.same(fast["AUTO"], fast["TILE"], tag, "gauss FAST AUTO vs TILE")
    if not mfma_pinned:
        rep.same(fast["MFMA"], fast["TILE"], tag, "gauss FAST MFMA (fallen back) vs TILE")

    # -- fused pipeline
    pipe = {}
    for mode_name, mode in (("FAST", pkg.GAUSS_FAST), ("EXACT", pkg.GAUSS_EXACT)):
        c.set_gauss_mode(mode)
        for name in ("AUTO", "TILE"):
            c.set_impl(impls[name])
            pipe[mode_name, name] = c.pipeline(x, k, sigma)
    c.set_gauss_mode(pkg.GAUSS_FAST)
    c.set_impl(pkg.IMPL_TILE)
    chained = c.sobel(c.gauss(c.gray(x), k, sigma))
    if asymmetric:      # the sliding-window kernels need a symmetric factor: AUTO must take the tiled path
        for mode_name in ("FAST", "EXACT"):
            rep.same(pipe[mode_name, "AUTO"], pipe[mode_name, "TILE"], tag, "pipeline AUTO vs TILE", mode_name)
    elif k <= 7:
        for mode_name in ("FAST", "EXACT"):
            rep.same(pipe[mode_name, "AUTO"], ref_pipe, tag, "pipeline AUTO", mode_name)
    rep.same(pipe["EXACT", "TILE"], ref_pipe, tag, "pipeline TILE EXACT")
    rep.same(pipe["FAST", "TILE"], chained, tag, "pipeline TILE FAST vs the three FAST calls chained")
    if k <= 7:
        away = _away_from_the_255_block(h, w)
        rep.within(pipe["FAST", "TILE"][:, away], ref_pipe[:, away], 6, tag, "pipeline TILE FAST vs CPU")

    # -- single-channel filters: the plane is frame 1's R channel, whose CPU Gaussian is that channel of the reference
    y = gt.gray_plane(x)
    ref_y = np.ascontiguousarray(ref_gauss[1, ..., 0])
    ref_edges = oracle.sobel_gray(ref_y)
    for name in ("AUTO", "TILE"):
        c.set_impl(impls[name])
        c.set_gauss_mode(pkg.GAUSS_EXACT)
        rep.same(c.gauss_gray8(y, k, sigma), ref_y, tag, "gauss_gray8 EXACT", name)
        rep.same(c.pipeline_gray8(y, k, sigma), ref_edges, tag, "pipeline_gray8 EXACT", name)
        c.set_gauss_mode(pkg.GAUSS_FAST)
        got = c.gauss_gray8(y, k, sigma)
        rep.within(got, ref_y, 1, tag, "gauss_gray8 FAST", name)
        if name == "AUTO" and k in (3, 5, 7) and not asymmetric:   # exact by exception in FAST mode too
            rep.same(got, ref_y, tag, "gauss_gray8 FAST AUTO")
        rep.same(c.pipeline_gray8(y, k, sigma), ref_edges, tag, "pipeline_gray8 FAST", name)
    c.set_impl(pkg.IMPL_AUTO)


# ---- part 1: generated tables on a sigma grid ------------------------------------------------------------------------
@pytest.mark.parametrize("k", gt.GRID_KS + gt.EDGE_KS)
def test_generated_tables_on_a_sigma_grid(ctx, pkg, oracle, batches, k):
    """sigma from 0.2 (the centre tap alone: dense flags on noise, then no flat window, then the per-position chains) to
    50 (a box filter within rounding); k = 1 and k = 31 at two of them."""
    rep = _Report()
    for sigma in (gt.GRID_SIGMAS if k in gt.GRID_KS else gt.EDGE_SIGMAS):
        refs = _references(oracle, batches, k, sigma)
        for shape, x in batches.items():
            _check_all_paths(ctx, pkg, oracle, rep, x, refs[shape][0], refs[shape][1], k, sigma, (k, sigma, shape))
    rep.done()


# ---- part 2: installed tables with a gain ----------------------------------------------------------------------------
@pytest.mark.parametrize("gain", gt.GAINS)
@pytest.mark.parametrize("k,base_sigma", gt.BASES)
def test_installed_tables_with_a_gain(own, pkg, oracle, batches, k, base_sigma, gain):
    """gain >= 1.0039 launches the CLAMP instantiations of gauss_slide / pipe_slide (gauss_exact: >= 1.0038), where an
    unclamped sum would carry into the next channel's byte; gain >= 1.0038 is refused by the matrix-core kernel
    (IMPL_MFMA and AUTO then give the tiled kernel's bits); gain 100 is refused by the exact-by-exception stage."""
    table = gt.scaled(oracle.gauss_weights(k, base_sigma), gain)
    sigma = 100.0 + gt.GAINS.index(gain)      # the key: no generated or installed table anywhere else uses it
    own.set_gauss_weights(k, sigma, table)
    refs = _references(oracle, batches, k, weights=table)
    rep = _Report()
    for shape, x in batches.items():
        _check_all_paths(own, pkg, oracle, rep, x, refs[shape][0], refs[shape][1], k, sigma, (k, gain, shape),
                         mfma_table_ok=gain < 1.0038)
    rep.done()


@pytest.mark.parametrize("k", sorted(gt.ASYM_FACTORS))
def test_asymmetric_factor_with_a_gain(own, pkg, oracle, batches, k):
    """u (x) u with an asymmetric u, times 1.25: CLAMP together with taps whose orientation matters, in bands that walk
    upward too.  The pair-form kernels (pipe_slide, gauss_exact, gray8's separable ones) must refuse it."""
    table = gt.scaled(gt.asym_table(k), gt.ASYM_GAIN)
    sigma = 120.0
    own.set_gauss_weights(k, sigma, table)
    refs = _references(oracle, batches, k, weights=table)
    rep = _Report()
    for shape, x in batches.items():
        _check_all_paths(own, pkg, oracle, rep, x, refs[shape][0], refs[shape][1], k, sigma, (k, "asym", shape),
                         mfma_table_ok=False, asymmetric=True)
    rep.done()


# ---- the fused pipeline with 8 pixels per lane and a CLAMP table -----------------------------------------------------
_PIPE8_GAIN_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import gauss_tables_ref as gt
from large_k_cases import Report as _Report
pkg = entry.load_package(); oracle = entry.load_oracle()
bad = []
with pkg.Context(0) as ctx:
    for k, s in ((3, 0.8), (5, 1.5)):
        table = gt.scaled(oracle.gauss_weights(k, s), 1.25)
        ctx.set_gauss_weights(k, 104.0, table)
        for (n, h, w) in [(2, 131, 1000), (1, 40, 504)]:
            x = np.ascontiguousarray(gt.frames(h, w, seed=h + w)[:n])
            for mode in (pkg.GAUSS_FAST, pkg.GAUSS_EXACT):
                ctx.set_gauss_mode(mode)
                got = ctx.pipeline(x, k, 104.0)
                for f in range(n):
                    if not np.array_equal(got[f], oracle.pipeline_rgba(x[f], k, weights=table)):
                        bad.append((n, h, w, k, mode, f))
print(bad)
"""


def test_pipeline_eight_pixels_per_lane_with_a_gain():
    """pipe_slide.hip's PX = 8 kernel, CLAMP instantiation: forced by the tuning build (MI355_PIPE8=1) in a child process
    of its own, as in test_gpu_configs.py: test_pipeline_eight_pixels_per_lane."""
    tune_lib = os.path.join(entry.ROOT, "tools", "lib", "libmi355_imgfilter_tune.so")
    assert os.path.exists(tune_lib), "run __graft_entry__.build()"
    env = dict(os.environ, MI355_IMGFILTER_LIB=tune_lib, MI355_PIPE8="1")
    out = subprocess.run([sys.executable, "-c", _PIPE8_GAIN_SCRIPT, entry.ROOT], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
