"""GPU suite (-m gpu): every kernel route through the guarded arena of tests/guarded.py.

What the rest of the suite cannot see: an output byte that is never written (the pooled output of the host-buffer calls
still holds the previous kernel's equal byte there) and a write outside the output (nothing reads those bytes).  Here
every call is device-resident, into a payload prefilled 128 away from the reference between two pattern guards, with the
input between two noise blocks; and every pointer takes every alignment the header allows: 4-byte pixels any dword,
1-byte-per-pixel outputs any byte.  The (filter, impl, k) rows follow the dispatch code (csrc/gauss.hip,
sobel_tile.hip, gray.hip, util.hip), the offsets its alignment predicates; which kernel ran is not asserted.

No new tolerances: bit-identity with the CPU path for everything but the FAST Gaussian, which is within 1 LSB of it
(north_star) and, under IMPL_VALU and IMPL_TILE, the same bytes at every alignment ("TILE and VALU give identical
bits", include/mi355_imgfilter.h); the FAST tiled pipeline is the three FAST calls chained.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import guarded
from conftest import rand_rgba
from hist_ref import equalize_ref, otsu_ref
from median_ref import median_ref
from morph_ref import morph_ref

pytestmark = pytest.mark.gpu

# (h, w, n): w < 4 (per-pixel forms, the pipeline goes to the tiled kernel); one partial strip of whole quads; two strips
# with an edge strip and >= 2 bands; ragged widths whose frames 1 and 2 start at other alignments
SHAPES = [(3, 3, 2), (9, 8, 2), (40, 252, 2), (37, 75, 3), (33, 250, 3)]
FULL = (40, 252, 2)          # the shape that gets the whole off_in x off_out product
MATRIX = (260, 256, 1)       # >= 2^16 pixels, w >= 64, w % 4 == 0: AUTO gives k >= 7 to the matrix cores when aligned
OFF4 = (0, 4, 8, 12)         # pointers to 4-byte pixels
OFF1 = (0, 1, 2, 3, 4, 8, 12)  # 1-byte-per-pixel outputs
SIGMA = {3: 0.8, 5: 1.5, 7: 2.0, 9: 2.5, 11: 3.0, 17: 6.0, 31: 10.0, 63: 20.0}


def reduced(ins, outs):
    """(0, 0), every input offset and every output offset at least once, and pairs with only one side off."""
    n = max(len(ins), len(outs))
    pairs = [(ins[i % len(ins)], outs[i % len(outs)]) for i in range(n)]
    pairs += [(ins[i % len(ins)], outs[(i + 1) % len(outs)]) for i in range(n)]
    pairs = sorted(set(pairs))
    assert (0, 0) in pairs and {p[0] for p in pairs} == set(ins) and {p[1] for p in pairs} == set(outs)
    return pairs


def offsets(shape, ins, outs):
    return [(a, b) for a in ins for b in outs] if shape == FULL else reduced(ins, outs)


@pytest.fixture(autouse=True)
def _reset_kernel_selection(ctx, pkg):
    yield
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)


_frames, _refs = {}, {}


def frames_of(shape, opaque=False):
    key = (shape, opaque)
    if key not in _frames:
        h, w, n = shape
        _frames[key] = rand_rgba(h, w, seed=h * 1000 + w, alpha=255 if opaque else None, n=n)
        _frames[key].setflags(write=False)
    return _frames[key]


def ref_of(key, make):
    """One CPU reference per (filter, parameters, shape), shared by every offset and test, never modified."""
    if key not in _refs:
        _refs[key] = np.ascontiguousarray(make())
        _refs[key].setflags(write=False)
    return _refs[key]


def per_frame(fn, frames):
    return np.stack([fn(f) for f in frames])


def gauss_ref(oracle, shape, opaque, k):
    x = frames_of(shape, opaque)
    return ref_of(("gauss", shape, opaque, k), lambda: per_frame(lambda f: oracle.gauss_rgba(f, k, SIGMA[k], threads=8), x))


def dev(ctx, filt, x, expected, off_in, off_out, k=0, sigma=0.0, tag=""):
    n, h, w = x.shape[:3]
    return guarded.run(ctx, lambda a, b: ctx.filter_dev(filt, a, b, w, h, n, k, sigma), x, expected, off_in, off_out,
                       tag="%s filter %d k %d (h, w, n) = (%d, %d, %d)" % (tag, filt, k, h, w, n))


def sweep(ctx, filt, shape, x, expected, ins, outs, k=0, sigma=0.0, tol=0, also=None, tag=""):
    """The call at every offset pair of the shape: guards intact, payload within tol of `expected` (and within 1 LSB of
    `also`, the CPU path, where `expected` is another kernel's result)."""
    for off_in, off_out in offsets(shape, ins, outs):
        got = dev(ctx, filt, x, expected, off_in, off_out, k, sigma, tag)
        t = "%s filter %d k %d shape %s off_in=%d off_out=%d" % (tag, filt, k, shape, off_in, off_out)
        guarded.check(got, expected, tol, t)
        if also is not None:
            guarded.check(got, also, 1, t + " (against the CPU path)")


# ---- Gaussian ---------------------------------------------------------------------------------------------------------
def _fast_gauss_same_bits(ctx, pkg, oracle, shape, opaque, k, impl):
    """FAST under IMPL_VALU / IMPL_TILE: within 1 LSB of the CPU path, and at every alignment the bytes the tiled kernel
    gives at (0, 0)."""
    x, ref = frames_of(shape, opaque), gauss_ref(oracle, shape, opaque, k)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_impl(pkg.IMPL_TILE)
    tiled = dev(ctx, pkg.FILTER_GAUSS, x, ref, 0, 0, k, SIGMA[k], "tile")
    guarded.check(tiled, ref, 1, "tile k %d %s" % (k, shape))
    ctx.set_impl(impl)
    sweep(ctx, pkg.FILTER_GAUSS, shape, x, tiled, OFF4, OFF4, k, SIGMA[k], 0, also=ref,
          tag="impl %d%s" % (impl, " opaque" if opaque else ""))


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 17])
def test_gauss_fast_valu_kernels(ctx, pkg, oracle, k):
    """gauss_slide (k 3, 5; two kernels for k 7, 9) and its RAGGED form when a pointer is off 16; gauss_wide (k 11, 17,
    even widths) at +8 / +8 and the tiled kernel at +4 / +12.  Opaque frames as well: the 3-channel pass and its flag
    handshake."""
    for shape in SHAPES + ([MATRIX] if k >= 7 else []):
        for opaque in (False, True):
            if opaque and shape == MATRIX:
                continue
            _fast_gauss_same_bits(ctx, pkg, oracle, shape, opaque, k, pkg.IMPL_VALU)


@pytest.mark.parametrize("k", [5, 31, 63])
def test_gauss_tiled_kernel(ctx, pkg, oracle, k):
    """IMPL_TILE at k 5 and, under AUTO, k 31 and 63, which only the tiled kernel takes; at 63 the halo is 31 pixels on
    frames of 3 x 3 and 9 x 8 and the carve (71,820 B) needs the raised dynamic-LDS limit."""
    for shape in SHAPES:
        _fast_gauss_same_bits(ctx, pkg, oracle, shape, False, k, pkg.IMPL_TILE if k == 5 else pkg.IMPL_AUTO)


@pytest.mark.parametrize("impl", ["AUTO", "MFMA"])
@pytest.mark.parametrize("k", [7, 17])
def test_gauss_matrix_core_shape(ctx, pkg, oracle, k, impl):
    """gauss_mfma_reg when both pointers are 16-byte aligned; off that, the sliding kernel (k 7) or gauss_wide at + 8 / + 8
    and the tiled kernel elsewhere (k 17).  Every one within 1 LSB of the CPU path."""
    x, ref = frames_of(MATRIX), gauss_ref(oracle, MATRIX, False, k)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    sweep(ctx, pkg.FILTER_GAUSS, MATRIX, x, ref, OFF4, OFF4, k, SIGMA[k], 1, tag=impl)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_gauss_exact(ctx, pkg, oracle, k):
    """gauss_exact, and the tiled kernel when a pointer is off 16 (or the width is ragged): the CPU path's bytes."""
    ctx.set_gauss_mode(pkg.GAUSS_EXACT)
    for shape in SHAPES:
        for opaque in (False, True):
            sweep(ctx, pkg.FILTER_GAUSS, shape, frames_of(shape, opaque), gauss_ref(oracle, shape, opaque, k), OFF4, OFF4,
                  k, SIGMA[k], 0, tag="exact%s" % (" opaque" if opaque else ""))


# ---- Sobel, pipeline, gray: 1-byte-per-pixel outputs at any byte ------------------------------------------------------
@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
def test_sobel(ctx, pkg, oracle, impl):
    """sobel_slide / its RAGGED form; the tiled kernel with vector stores / byte stores."""
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    for shape in SHAPES:
        x = frames_of(shape)
        ref = ref_of(("sobel", shape), lambda: per_frame(oracle.sobel_rgba, x))
        sweep(ctx, pkg.FILTER_SOBEL, shape, x, ref, OFF4, OFF1, tag=impl)


def _fast_chain(ctx, pkg, oracle, shape, k):
    """sobel(gauss(gray(x))), the three FAST calls chained at (0, 0), each one through the arena against the CPU path of
    its own input."""
    def make():
        x = frames_of(shape)
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        ctx.set_impl(pkg.IMPL_TILE)
        gray_ref = per_frame(oracle.gray_rgba, x)
        gray = dev(ctx, pkg.FILTER_GRAY, x, gray_ref, 0, 0, tag="chain")
        guarded.check(gray, gray_ref, 0, "chain gray %s" % (shape,))
        blur_ref = per_frame(lambda f: oracle.gauss_rgba(f, k, SIGMA[k], threads=8), gray)
        blur = dev(ctx, pkg.FILTER_GAUSS, gray, blur_ref, 0, 0, k, SIGMA[k], "chain")
        guarded.check(blur, blur_ref, 1, "chain gauss %s" % (shape,))
        edge_ref = per_frame(oracle.sobel_rgba, blur)
        edge = dev(ctx, pkg.FILTER_SOBEL, blur, edge_ref, 0, 0, tag="chain")
        guarded.check(edge, edge_ref, 0, "chain sobel %s" % (shape,))
        return edge
    return ref_of(("chain", shape, k), make)


@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
@pytest.mark.parametrize("k", [3, 5, 7, 9, 63])
def test_pipeline(ctx, pkg, oracle, k, impl):
    """pipe_slide (k <= 7, w >= 4, h >= 2; RAGGED when a pointer is off) gives the CPU chain's bytes in both Gaussian
    modes, the tiled kernel in EXACT mode too; the FAST tiled kernel (k 9 and 63, IMPL_TILE, w < 4) gives the three FAST
    calls chained, and is prefilled from them.  At 63 the halo is 32 pixels on frames of 3 x 3 and 9 x 8."""
    for shape in SHAPES:
        h, w, _ = shape
        x = frames_of(shape)
        ref = ref_of(("pipe", shape, k), lambda: per_frame(lambda f: oracle.pipeline_rgba(f, k, SIGMA[k]), x))
        slides = impl == "AUTO" and k <= 7 and w >= 4 and h >= 2
        chain = None if slides else _fast_chain(ctx, pkg, oracle, shape, k)
        ctx.set_impl(getattr(pkg, "IMPL_" + impl))
        ctx.set_gauss_mode(pkg.GAUSS_EXACT)
        sweep(ctx, pkg.FILTER_PIPELINE, shape, x, ref, OFF4, OFF1, k, SIGMA[k], tag=impl + " exact")
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        sweep(ctx, pkg.FILTER_PIPELINE, shape, x, ref if slides else chain, OFF4, OFF1, k, SIGMA[k], tag=impl + " fast")


def test_gray(ctx, pkg, oracle):
    """gray_vec when both pointers are aligned (16 / 16, or 16 / 4 for the 1-byte output), gray_px otherwise."""
    for shape in SHAPES:
        x = frames_of(shape)
        sweep(ctx, pkg.FILTER_GRAY, shape, x, ref_of(("gray", shape), lambda: per_frame(oracle.gray_rgba, x)), OFF4, OFF4)
        sweep(ctx, pkg.FILTER_GRAY1, shape, x, ref_of(("gray1", shape), lambda: per_frame(oracle.gray_rgba_1ch, x)),
              OFF4, OFF1)


def test_bgr_to_rgba_dev(ctx, pkg):
    """mi355_bgr_to_rgba8_dev: d_bgr at any byte, d_rgba at any dword; the vector form at 4 / 16, the scalar form off it."""
    for h, w, n in SHAPES:
        bgr = np.ascontiguousarray(frames_of((h, w, n))[..., :3])
        ref = np.concatenate([bgr[..., ::-1], np.full((n, h, w, 1), 255, np.uint8)], axis=-1)
        for off_in in (0, 1, 2, 3):
            for off_out in OFF4:
                tag = "bgr (h, w, n) = (%d, %d, %d)" % (h, w, n)
                got = guarded.run(ctx, lambda a, b: ctx.bgr_to_rgba_dev(a, b, w, h, n), bgr, ref, off_in, off_out, tag=tag)
                guarded.check(got, ref, 0, "%s off_in=%d off_out=%d" % (tag, off_in, off_out))


# ---- median and morphology on RGBA frames: dword offsets --------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7])
def test_median(ctx, pkg, k):
    for impl in (pkg.IMPL_AUTO, pkg.IMPL_TILE):   # compare networks (k 3, 5) / the LDS counting kernel
        ctx.set_impl(impl)
        for shape in SHAPES:
            x = frames_of(shape)
            ref = ref_of(("median", shape, k), lambda: per_frame(lambda f: median_ref(f, k), x))
            sweep(ctx, pkg.FILTER_MEDIAN, shape, x, ref, OFF4, OFF4, k, tag="impl %d" % impl)


@pytest.mark.parametrize("k", [3, 17])
@pytest.mark.parametrize("op", ["erode", "dilate", "open", "close"])
def test_morphology(ctx, pkg, op, k):
    filt = getattr(pkg, "FILTER_" + op.upper())
    for shape in SHAPES:
        x = frames_of(shape)
        ref = ref_of((op, shape, k), lambda: per_frame(lambda f: morph_ref(op, f, k), x))
        sweep(ctx, filt, shape, x, ref, OFF4, OFF4, k, tag=op)


# ---- the single-channel family: write footprint and unwritten pixels (its alignment sweeps are in its own files) ------
GRAY8_SHAPE = (37, 101, 3)


def _gray8_refs(pkg, oracle, y):
    def blur(f):
        rgba = np.ascontiguousarray(np.dstack([f, f, f, np.full_like(f, 255)]))
        return np.ascontiguousarray(oracle.gauss_rgba(rgba, 5, 1.5)[..., 0])
    g = per_frame(blur, y)
    refs = {"GAUSS_GRAY8": g, "SOBEL_GRAY8": per_frame(oracle.sobel_gray, y), "PIPELINE_GRAY8": per_frame(oracle.sobel_gray, g),
            "MEDIAN_GRAY8": per_frame(lambda f: median_ref(f, 5), y), "EQUALIZE_GRAY8": equalize_ref(y),
            "OTSU_GRAY8": otsu_ref(y)}
    for op in ("erode", "dilate", "open", "close"):
        refs[op.upper() + "_GRAY8"] = per_frame(lambda f: morph_ref(op, f, 5), y)
    return refs


@pytest.mark.parametrize("name", ["GAUSS_GRAY8", "SOBEL_GRAY8", "PIPELINE_GRAY8", "MEDIAN_GRAY8", "ERODE_GRAY8",
                                  "DILATE_GRAY8", "OPEN_GRAY8", "CLOSE_GRAY8", "EQUALIZE_GRAY8", "OTSU_GRAY8"])
def test_gray8_family(ctx, pkg, oracle, name):
    h, w, n = GRAY8_SHAPE
    y = np.ascontiguousarray(frames_of((h, w, n))[..., 1])
    if "gray8" not in _refs:
        _refs["gray8"] = _gray8_refs(pkg, oracle, y)
    ref = _refs["gray8"][name]
    filt = getattr(pkg, "FILTER_" + name)
    for mode in (pkg.GAUSS_EXACT, pkg.GAUSS_FAST):
        ctx.set_gauss_mode(mode)
        # the FAST single-channel Gaussian is within 1 LSB of the CPU path; everything else is its bytes in both modes
        tol = 1 if (name == "GAUSS_GRAY8" and mode == pkg.GAUSS_FAST) else 0
        for off_in, off_out in ((0, 0), (1, 3)):
            got = dev(ctx, filt, y, ref, off_in, off_out, 5, 1.5, name)
            guarded.check(got, ref, tol, "%s mode %d off_in=%d off_out=%d" % (name, mode, off_in, off_out))


# ---- kernels that normally serve launches of 2^28 .. 10^9 pixels, forced by the tuning build --------------------------
_FORCED_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import guarded
from conftest import rand_rgba
pkg = entry.load_package(); oracle = entry.load_oracle()
rows = {"sobel": [(pkg.FILTER_SOBEL, 0, 0.0, oracle.sobel_rgba, 1)],
        "gray": [(pkg.FILTER_GRAY, 0, 0.0, oracle.gray_rgba, 4), (pkg.FILTER_GRAY1, 0, 0.0, oracle.gray_rgba_1ch, 1)],
        "pipe8": [(pkg.FILTER_PIPELINE, k, s, (lambda f, k=k, s=s: oracle.pipeline_rgba(f, k, s)), 1)
                  for k, s in ((3, 0.8), (5, 1.5))]}[sys.argv[2]]
bad = []
with pkg.Context(0) as ctx:
    for (h, w, n) in [(40, 512, 2), (19, 64, 2)]:
        x = rand_rgba(h, w, seed=h + w, alpha=None, n=n)
        for filt, k, s, fn, bpp in rows:
            ref = np.stack([fn(f) for f in x])
            for off_out in (0, 1, 4, 8, 12):   # aligned: the forced kernel; off: dispatch must leave it (8: pipe8 stays)
                if off_out % bpp:
                    continue
                try:
                    got = guarded.run(ctx, lambda a, b: ctx.filter_dev(filt, a, b, w, h, n, k, s), x, ref, 0, off_out)
                    guarded.check(got, ref)
                except AssertionError as e:
                    bad.append((filt, k, h, w, n, off_out, str(e)))
print(bad)
"""


@pytest.mark.parametrize("which,var,value", [("sobel", "MI355_TUNE_SOBEL_STRIP", "2"), ("gray", "MI355_TUNE_GRAY_STRIP", "3"),
                                             ("pipe8", "MI355_PIPE8", "1")])
def test_big_batch_kernels_forced_on_small_shapes(which, var, value):
    """sobel_strip_kernel, gray_strip_kernel and pipe_slide with 8 pixels per lane, which AUTO keeps for launches of
    2^28 .. 10^9 pixels: the tuning build (csrc/Makefile `make tune`) forces each at any size through one variable,
    read once per process, hence one short child each.  Aligned pointers, where the forced kernel runs, and output
    offsets 1, 4 and 12, where dispatch must leave it (at + 4 the 8-pixel pipeline lacks its 8-byte output alignment
    and falls back to 4 pixels per lane): the CPU path's bytes, guards intact."""
    tune_lib = os.path.join(entry.ROOT, "tools", "lib", "libmi355_imgfilter_tune.so")
    assert os.path.exists(tune_lib), "run __graft_entry__.build()"
    env = dict(os.environ, MI355_IMGFILTER_LIB=tune_lib)
    env[var] = value
    out = subprocess.run([sys.executable, "-c", _FORCED_SCRIPT, entry.ROOT, which], env=env, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
