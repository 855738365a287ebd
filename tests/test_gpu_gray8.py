"""GPU suite (-m gpu): the single-channel filters MI355_FILTER_GAUSS_GRAY8 / SOBEL_GRAY8 / PIPELINE_GRAY8.

Bars: SOBEL_GRAY8 is bit-identical to the reference CPU edge detector on the plane itself (oracle.sobel_gray,
src/EdgeDetection/EdgeDetection.cpp:219-240 on an IMREAD_GRAYSCALE image); GAUSS_GRAY8 in EXACT mode is bit-identical
to the R channel of the CPU Gaussian of (y, y, y, 255), FAST within 1 LSB; PIPELINE_GRAY8 is bit-identical to
Sobel(EXACT Gaussian) in both modes.
"""
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from test_published_mae import NAMES, _committed

pytestmark = pytest.mark.gpu

KS = (1, 3, 5, 7, 9, 17, 63)


def _sigma(k):
    return max(0.8, k / 6.0)


def _threads(oracle):
    return max(1, min(oracle.max_threads(), 16))


def _rgba(y):
    return np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))


def gauss_r(oracle, y, k, sigma=None, weights=None):
    """The CPU path's Gaussian of one channel: the R channel of the RGBA Gaussian of (y, y, y, 255)."""
    sigma = _sigma(k) if sigma is None and weights is None else sigma
    return np.ascontiguousarray(oracle.gauss_rgba(_rgba(y), k, sigma, weights=weights, threads=_threads(oracle))[..., 0])


def hash_noise(h, w, seed):
    i = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    v = (i + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(32)
    return (v & np.uint64(0xFF)).astype(np.uint8)


def flat_patches(h, w, seed):
    ph, pw = (h + 63) // 64, (w + 63) // 64
    vals = hash_noise(ph, pw, seed)
    return np.ascontiguousarray(np.repeat(np.repeat(vals, 64, 0), 64, 1)[:h, :w])


def extremes(h, w, seed):
    return np.where(hash_noise(h, w, seed) & 1, 255, 0).astype(np.uint8)


@pytest.fixture(scope="module")
def luma_planes():
    out = {}
    for n in NAMES:
        c = _committed(n)
        if c is not None:
            out[n] = np.ascontiguousarray(c[1])
    assert len(out) >= 5
    return out


@pytest.fixture
def modes(ctx, pkg):
    yield
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_input_format(pkg.INPUT_RGBA)


# ---- Sobel ----------------------------------------------------------------------------------------------------------
def test_sobel_gray8_is_the_cpu_edge_detector_on_the_decoder_luma_planes(ctx, oracle, luma_planes):
    """What test_gpu_published.py's test_hip_sobel_on_the_decoder_luma_plane could only check where luma(v,v,v) = v."""
    for n, y in luma_planes.items():
        got = ctx.sobel_gray8(y)
        assert np.array_equal(got, oracle.sobel_gray(y)), n
        # the RGBA path re-grays the plane first and so cannot produce this answer
        assert not np.array_equal(ctx.sobel(_rgba(y)), got), n


@pytest.mark.parametrize("make", [hash_noise, flat_patches, extremes])
def test_sobel_gray8_on_synthetic_content(ctx, oracle, make):
    for h, w in ((480, 640), (333, 1021)):
        y = make(h, w, 7)
        got = ctx.sobel_gray8(y)
        assert np.array_equal(got, oracle.sobel_gray(y)), (make.__name__, h, w)
        if make is not extremes:  # luma(v, v, v) = v for v = 0 and 255: only there do the two paths agree
            assert not np.array_equal(ctx.sobel(_rgba(y)), got), (make.__name__, h, w)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (9, 1), (2, 2), (75, 75), (1023, 819), (1022, 5), (2160, 3840)])
def test_sobel_gray8_shapes(ctx, oracle, shape):
    y = hash_noise(*shape, seed=shape[0] * 7 + shape[1])
    assert np.array_equal(ctx.sobel_gray8(y), oracle.sobel_gray(y)), shape


def test_sobel_gray8_batch_of_eight(ctx, oracle):
    ys = np.stack([hash_noise(121, 203, s) if s % 2 else flat_patches(121, 203, s) for s in range(8)])
    got = ctx.sobel_gray8(ys)
    assert got.shape == ys.shape
    for f in range(8):
        assert np.array_equal(got[f], oracle.sobel_gray(ys[f])), f


# ---- Gaussian -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
@pytest.mark.parametrize("k", KS)
def test_gauss_gray8_exact_and_fast(ctx, pkg, oracle, modes, impl, k):
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    frames = [hash_noise(67, 203, k), flat_patches(130, 77, k), np.ascontiguousarray(luma_planes_one())]
    if k in (5, 17):
        frames.append(hash_noise(2160, 3840, k))
    for y in frames:
        ref = gauss_r(oracle, y, k)
        ctx.set_gauss_mode(pkg.GAUSS_EXACT)
        assert np.array_equal(ctx.gauss_gray8(y, k, _sigma(k)), ref), (impl, k, y.shape)
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        fast = ctx.gauss_gray8(y, k, _sigma(k))
        assert np.abs(fast.astype(int) - ref.astype(int)).max() <= 1, (impl, k, y.shape)
        if impl == "AUTO" and k in (3, 5, 7):  # exact by exception in FAST mode too
            assert np.array_equal(fast, ref), (k, y.shape)


def luma_planes_one():
    c = _committed("Tulips_square75")
    return c[1] if c is not None else hash_noise(75, 75, 75)


@pytest.mark.parametrize("impl", ["AUTO", "TILE"])
def test_gauss_gray8_nonseparable_table_is_applied_tap_by_tap(ctx, pkg, oracle, modes, impl):
    ctx.set_impl(getattr(pkg, "IMPL_" + impl))
    k, sigma = 5, 1.3
    table = np.arange(1, k * k + 1, dtype=np.float32).reshape(k, k)
    table = (table / table.sum()).astype(np.float32)
    table[0, 4] = 0.0  # asymmetric, not an outer product
    ctx.set_gauss_weights(k, sigma, table)
    y = hash_noise(61, 333, 3)
    ref = gauss_r(oracle, y, k, sigma, weights=table)
    for mode in (pkg.GAUSS_FAST, pkg.GAUSS_EXACT):
        ctx.set_gauss_mode(mode)
        assert np.array_equal(ctx.gauss_gray8(y, k, sigma), ref), (impl, mode)
        assert np.array_equal(ctx.pipeline_gray8(y, k, sigma), oracle.sobel_gray(ref)), (impl, mode)


# ---- fused chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9, 17, 31, 45])
def test_pipeline_gray8_is_sobel_of_the_exact_gaussian(ctx, pkg, oracle, modes, k):
    sigma = _sigma(k)
    frames = [hash_noise(97, 301, k), flat_patches(200, 130, k), extremes(1, 9, k), extremes(5, 1, k),
              hash_noise(1, 1, k), luma_planes_one()]
    if k == 5:
        frames.append(hash_noise(2160, 3840, 5))
    for y in frames:
        y = np.ascontiguousarray(y)
        g = gauss_r(oracle, y, k)
        ref = oracle.sobel_gray(g)
        for impl in (pkg.IMPL_AUTO, pkg.IMPL_TILE):
            ctx.set_impl(impl)
            for mode in (pkg.GAUSS_FAST, pkg.GAUSS_EXACT):
                ctx.set_gauss_mode(mode)
                assert np.array_equal(ctx.pipeline_gray8(y, k, sigma), ref), (k, y.shape, impl, mode)
            ctx.set_gauss_mode(pkg.GAUSS_EXACT)
            chain = ctx.sobel_gray8(ctx.gauss_gray8(y, k, sigma))
            assert np.array_equal(chain, ref), (k, y.shape, impl)


# ---- alignment, aliasing, device-resident calls ---------------------------------------------------------------------
def test_any_byte_alignment_and_the_aliasing_rules(ctx, pkg, oracle):
    n, h, w = 3, 37, 101
    ys = np.stack([hash_noise(h, w, s) for s in range(n)])
    nb = n * h * w
    refs = {pkg.FILTER_SOBEL_GRAY8: np.stack([oracle.sobel_gray(y) for y in ys]),
            pkg.FILTER_GAUSS_GRAY8: np.stack([gauss_r(oracle, y, 5, 1.5) for y in ys])}
    refs[pkg.FILTER_PIPELINE_GRAY8] = np.stack([oracle.sobel_gray(g) for g in refs[pkg.FILTER_GAUSS_GRAY8]])
    ctx.set_gauss_mode(pkg.GAUSS_EXACT)
    base = ctx.alloc(4 * nb + 64)
    try:
        for filt, ref in refs.items():
            for off_in in (0, 1, 2, 3):
                for off_out in (0, 1, 2, 3):
                    d_in = base + off_in
                    d_out = base + 2 * nb + 16 + off_out
                    ctx.h2d(d_in, ys)
                    ctx.filter_dev(filt, d_in, d_out, w, h, n, 5, 1.5)
                    ctx.sync()
                    got = np.empty((n, h, w), np.uint8)
                    ctx.d2h(got, d_out)
                    assert np.array_equal(got, ref), (filt, off_in, off_out)
            # in place and overlapping calls are refused (every range below stays inside the allocation)
            d_in = base + nb + 64
            for d_out in (d_in, d_in + 1, d_in + nb - 1, d_in - nb + 1):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_out, w, h, n, 5, 1.5)
                assert e.value.code == -1
            # an output right after the 1-byte input is fine
            ctx.h2d(base + 1, ys)
            ctx.filter_dev(filt, base + 1, base + 1 + nb, w, h, n, 5, 1.5)
            ctx.sync()
            got = np.empty((n, h, w), np.uint8)
            ctx.d2h(got, base + 1 + nb)
            assert np.array_equal(got, ref), filt
    finally:
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        ctx.sync()
        ctx.free(base)


def test_gray8_gaussian_ids_reject_a_bad_k(ctx, pkg):
    """A bad k or sigma of the four Gaussian ids (gray8 and RGBA) is MI355_ERR_BAD_ARG through every entry point."""
    y = hash_noise(8, 8, 1)
    d_in, d_out = ctx.alloc(256), ctx.alloc(256)
    bad = [(k, 1.5) for k in (0, 2, 4, 65, -3)] + [(5, s) for s in (0.0, float("inf"), float("nan"))]
    try:
        ctx.h2d(d_in, _rgba(y))
        with pkg.Group([0]) as g:
            for filt in (pkg.FILTER_GAUSS_GRAY8, pkg.FILTER_PIPELINE_GRAY8, pkg.FILTER_GAUSS, pkg.FILTER_PIPELINE):
                gray8 = filt in (pkg.FILTER_GAUSS_GRAY8, pkg.FILTER_PIPELINE_GRAY8)
                frames = y[None] if gray8 else _rgba(y)[None]
                calls = {
                    "filter_dev": lambda k, s: ctx.filter_dev(filt, d_in, d_out, 8, 8, 1, k, s),
                    "host": lambda k, s: (ctx._host_gray8 if gray8 else ctx._host)(filt, frames, k, s),
                    "stream": lambda k, s: ctx.stream(filt, frames, k=k, sigma=s),
                    "pool_alloc": lambda k, s: ctx.pool_alloc(filt, 8, 8, 1, k=k, sigma=s, tries=1),
                    "group.filter_batched": lambda k, s: g.filter_batched(filt, frames, k=k, sigma=s),
                    "group.filter_dev": lambda k, s: g.filter_dev(filt, [d_in], [d_out], 8, 8, [1], k, s),
                }
                for k, sigma in bad:
                    for name, call in calls.items():
                        with pytest.raises(pkg.Mi355Error) as e:
                            call(k, sigma)
                        assert e.value.code == -1, (filt, k, sigma, name)
    finally:
        ctx.sync()
        ctx.free(d_in)
        ctx.free(d_out)


# ---- host paths -----------------------------------------------------------------------------------------------------
def _dev_reference(ctx, filt, ys, k=5, sigma=1.5):
    n, h, w = ys.shape
    d_in, d_out = ctx.alloc(ys.nbytes), ctx.alloc(ys.nbytes)
    try:
        ctx.h2d(d_in, ys)
        ctx.filter_dev(filt, d_in, d_out, w, h, n, k, sigma)
        ctx.sync()
        out = np.empty_like(ys)
        ctx.d2h(out, d_out)
        return out
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


def test_batched_and_streamed_host_paths_equal_filter_dev(ctx, pkg):
    n, h, w = 7, 90, 131
    ys = np.stack([hash_noise(h, w, 100 + s) for s in range(n)])
    pinned = ctx.pinned_empty(ys.shape)
    pinned[...] = ys
    pinned_out = ctx.pinned_empty(ys.shape)
    try:
        for filt in (pkg.FILTER_GAUSS_GRAY8, pkg.FILTER_SOBEL_GRAY8, pkg.FILTER_PIPELINE_GRAY8):
            ref = _dev_reference(ctx, filt, ys)
            assert np.array_equal(ctx._host_gray8(filt, ys, 5, 1.5), ref), filt
            out, _ = ctx.stream(filt, ys, k=5, sigma=1.5, chunk_frames=3)  # pageable, 3 does not divide 7
            assert np.array_equal(out, ref), filt
            out, _ = ctx.stream(filt, pinned, out=pinned_out, k=5, sigma=1.5, chunk_frames=3)
            assert np.array_equal(out, ref), filt
    finally:
        ctx.pinned_free(pinned)
        ctx.pinned_free(pinned_out)


def test_two_member_group_equals_one_context(pkg):
    n, h, w = 5, 64, 150
    ys = np.stack([hash_noise(h, w, 200 + s) for s in range(n)])
    with pkg.Group([0, 0]) as g, pkg.Context(0) as one:
        for filt in (pkg.FILTER_GAUSS_GRAY8, pkg.FILTER_SOBEL_GRAY8, pkg.FILTER_PIPELINE_GRAY8):
            ref = _dev_reference(one, filt, ys)
            out, _ = g.filter_batched(filt, ys, k=5, sigma=1.5)
            assert np.array_equal(out, ref), filt
            counts = [pkg.group_shard(m, 2, n)[1] for m in range(2)]
            firsts = [pkg.group_shard(m, 2, n)[0] for m in range(2)]
            ptrs = []
            for m in range(2):
                mc = g.member(m)
                d_in, d_out = mc.alloc(ys.nbytes), mc.alloc(ys.nbytes)
                mc.h2d(d_in, ys[firsts[m]:firsts[m] + counts[m]])
                ptrs.append((mc, d_in, d_out))
            g.filter_dev(filt, [p[1] for p in ptrs], [p[2] for p in ptrs], w, h, counts, 5, 1.5)
            for m, (mc, d_in, d_out) in enumerate(ptrs):
                got = np.empty((counts[m], h, w), np.uint8)
                mc.d2h(got, d_out)
                assert np.array_equal(got, ref[firsts[m]:firsts[m] + counts[m]]), (filt, m)
                mc.free(d_in)
                mc.free(d_out)


def test_bgr_input_format_refuses_gray8_ids(ctx, pkg, modes):
    y = hash_noise(16, 16, 1)
    ctx.set_input_format(pkg.INPUT_BGR)
    for call in (lambda: ctx.gauss_gray8(y, 5, 1.5), lambda: ctx.sobel_gray8(y), lambda: ctx.pipeline_gray8(y, 5, 1.5),
                 lambda: ctx.stream(pkg.FILTER_SOBEL_GRAY8, y[None].copy())):
        with pytest.raises(pkg.Mi355Error) as e:
            call()
        assert e.value.code == -4
    with pkg.Group([0]) as g:
        g.set_input_format(pkg.INPUT_BGR)
        with pytest.raises(pkg.Mi355Error) as e:
            g.filter_batched(pkg.FILTER_SOBEL_GRAY8, y[None].copy())
        assert e.value.code == -4


# ---- stream capture -------------------------------------------------------------------------------------------------
_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from test_gpu_gray8 import gauss_r, hash_noise
pkg = entry.load_package(); oracle = entry.load_oracle()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h = 641, 479
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    frames = [hash_noise(h, w, 1), hash_noise(h, w, 2)]
    d_in = torch.from_numpy(frames[0]).to(dev)
    o_gauss = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    o_sobel = torch.zeros((h, w), dtype=torch.uint8, device=dev)

    def chain():   # one stream, one linear chain: no parallel branches
        c.filter_dev(pkg.FILTER_GAUSS_GRAY8, d_in.data_ptr(), o_gauss.data_ptr(), w, h, 1, 5, 1.5)
        c.filter_dev(pkg.FILTER_SOBEL_GRAY8, o_gauss.data_ptr(), o_sobel.data_ptr(), w, h, 1)

    c.set_gauss_mode(pkg.GAUSS_EXACT)
    chain()                             # first use: table installed - not capturable, by contract
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for n, f in enumerate(frames):
        d_in.copy_(torch.from_numpy(f).to(dev))
        o_gauss.zero_(); o_sobel.zero_()
        g.replay()
        s.synchronize()
        ref = gauss_r(oracle, f, 5, 1.5)
        if not np.array_equal(o_gauss.cpu().numpy(), ref): bad.append((n, "gauss"))
        if not np.array_equal(o_sobel.cpu().numpy(), oracle.sobel_gray(ref)): bad.append((n, "sobel"))
    del g
    c.close()
print(bad)
"""


def test_gray8_device_calls_can_be_captured_into_a_hip_graph():
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
