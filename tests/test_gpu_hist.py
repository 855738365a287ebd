"""GPU suite (-m gpu): whole-frame statistics of single-channel frames, MI355_FILTER_EQUALIZE_GRAY8 and
MI355_FILTER_OTSU_GRAY8, and the two device-resident calls behind them (mi355_hist_gray8_dev,
mi355_otsu_thresholds_gray8_dev).

Every comparison is bit-identity with the CPU reference tests/hist_ref.py (cv::calcHist, cv::equalizeHist and
cv::threshold with THRESH_OTSU, OpenCV's float and double arithmetic step by step): histograms, thresholds and
output frames.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
from hist_ref import equalize_ref, hist_ref, otsu_ref, otsu_thresholds_ref  # noqa: E402
from morph_ref import morph_ref  # noqa: E402
from test_gpu_median import constant, extremes, impulses, noise, patches  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 45), (45, 1), (2, 3), (5, 7), (17, 17), (33, 19), (75, 75), (427, 640), (1023, 819)]


def two_level(h, w, c, seed):
    img = np.full((h, w), 40 + seed % 50, np.uint8)
    img[:, w // 3:] = 180 + seed % 60
    return img


def all_255(h, w, c, seed):
    return np.full((h, w), 255, np.uint8)


def dark_noise(h, w, c, seed):
    """noise squeezed into a few low bins: many empty bins above, an uneven histogram"""
    return (noise(h, w, 1, seed) >> 5).astype(np.uint8)


CONTENTS = [noise, patches, constant, two_level, all_255, extremes, impulses, dark_noise]


def _check_all(ctx, y, what):
    assert np.array_equal(ctx.hist_gray8(y), hist_ref(y)), what
    assert np.array_equal(ctx.otsu_thresholds_gray8(y), otsu_thresholds_ref(y)), what
    assert np.array_equal(ctx.equalize_hist_gray8(y), equalize_ref(y)), what
    assert np.array_equal(ctx.otsu_gray8(y), otsu_ref(y)), what


def test_bit_identical_to_the_cpu_reference(ctx):
    for shape in SHAPES:
        for make in CONTENTS:
            y = make(shape[0], shape[1], 1, shape[0] * 31 + shape[1])
            _check_all(ctx, y, (shape, make.__name__))


def test_hand_worked_frames(ctx):
    y = np.arange(7, dtype=np.uint8)[None]
    assert ctx.equalize_hist_gray8(y).tolist() == [[0, 42, 85, 128, 170, 212, 255]]
    for v in (0, 1, 37, 255):
        c = np.full((19, 23), v, np.uint8)
        assert np.array_equal(ctx.equalize_hist_gray8(c), c), v
        assert int(ctx.otsu_thresholds_gray8(c)) == 0, v


@pytest.mark.parametrize("rows,t", [(2048, 10), (2049, 0)])
def test_frames_at_the_flt_epsilon_boundary(ctx, rows, t):
    """4096 x 2048 = 2^23 pixels with one pixel of 10 in 200s: q1 = FLT_EPSILON, no `continue`, t = 10.
    4096 x 2049: every bin takes the `continue`, t = 0, the outlier maps to 255."""
    y = np.full((rows, 4096), 200, np.uint8)
    y[rows // 3, 1234] = 10
    assert int(ctx.otsu_thresholds_gray8(y)) == t == int(otsu_thresholds_ref(y))
    o = ctx.otsu_gray8(y)
    assert o[rows // 3, 1234] == (0 if t == 10 else 255)
    assert np.array_equal(o, otsu_ref(y))
    assert np.array_equal(ctx.equalize_hist_gray8(y), equalize_ref(y))
    assert np.array_equal(ctx.hist_gray8(y), hist_ref(y))


def test_4k_frames(ctx):
    ys = np.stack([noise(2160, 3840, 1, 1), patches(2160, 3840, 1, 2), constant(2160, 3840, 1, 3),
                   dark_noise(2160, 3840, 1, 4)])
    _check_all(ctx, ys, "4k")


def test_batches_equal_calls_on_one_frame_at_a_time(ctx):
    h, w = 61, 97
    ys = np.stack([make(h, w, 1, s) for s, make in enumerate(CONTENTS * 2)])
    _check_all(ctx, ys, "batch")
    for fn in (ctx.equalize_hist_gray8, ctx.otsu_gray8, ctx.hist_gray8, ctx.otsu_thresholds_gray8):
        assert np.array_equal(fn(ys), np.stack([fn(y) for y in ys])), fn.__name__


def test_any_byte_alignment(ctx, pkg):
    """Byte offsets 0-15 of the input and of the output (frames of odd sizes, so frame f > 0 starts at every offset)."""
    n, h, w = 3, 29, 53
    ys = np.stack([noise(h, w, 1, 1), patches(h, w, 1, 2), two_level(h, w, 1, 3)])
    nb = ys.nbytes
    base = ctx.alloc(2 * nb + 4096 + 96)
    try:
        d_hist = base + (2 * nb + 64 + 15) // 16 * 16  # 1 KiB per frame, 4-byte aligned
        d_t = d_hist + 3 * 1024
        for filt, ref in ((pkg.FILTER_EQUALIZE_GRAY8, equalize_ref(ys)), (pkg.FILTER_OTSU_GRAY8, otsu_ref(ys))):
            for off_in in range(16):
                for off_out in range(16):
                    d_in, d_out = base + off_in, base + nb + 32 + off_out
                    ctx.h2d(d_in, ys)
                    ctx.filter_dev(filt, d_in, d_out, w, h, n, 0, 0.0)
                    ctx.sync()
                    got = np.empty_like(ys)
                    ctx.d2h(got, d_out)
                    assert np.array_equal(got, ref), (filt, off_in, off_out)
        for off_in in range(16):
            d_in = base + off_in
            ctx.h2d(d_in, ys)
            ctx.hist_gray8_dev(d_in, d_hist, w, h, n)
            ctx.otsu_thresholds_gray8_dev(d_in, d_t, w, h, n)
            ctx.sync()
            hist = np.empty((n, 256), np.uint32)
            t = np.empty(n, np.int32)
            ctx.d2h(hist, d_hist)
            ctx.d2h(t, d_t)
            assert np.array_equal(hist, hist_ref(ys)), off_in
            assert np.array_equal(t, otsu_thresholds_ref(ys)), off_in
    finally:
        ctx.sync()
        ctx.free(base)


def test_hist_call_overwrites_its_output(ctx):
    h, w = 40, 50
    ys = np.stack([noise(h, w, 1, 5), constant(h, w, 1, 6)])
    d_in, d_hist = ctx.alloc(ys.nbytes), ctx.alloc(2 * 1024)
    try:
        ctx.h2d(d_in, ys)
        ctx.h2d(d_hist, np.full((2, 256), 0xDEAD, np.uint32))
        for _ in range(2):
            ctx.hist_gray8_dev(d_in, d_hist, w, h, 2)
        ctx.sync()
        got = np.empty((2, 256), np.uint32)
        ctx.d2h(got, d_hist)
        assert np.array_equal(got, hist_ref(ys))
    finally:
        ctx.sync()
        ctx.free(d_in)
        ctx.free(d_hist)


# ---- host paths -----------------------------------------------------------------------------------------------------
def test_batched_stream_and_pool(ctx, pkg):
    n, h, w = 5, 67, 129
    ys = np.stack([make(h, w, 1, s) for s, make in enumerate(CONTENTS[:n])])
    for filt, ref in ((pkg.FILTER_EQUALIZE_GRAY8, equalize_ref(ys)), (pkg.FILTER_OTSU_GRAY8, otsu_ref(ys))):
        assert np.array_equal(ctx._host_gray8(filt, ys), ref), filt
        for chunk in (1, 3, 0):
            out, _ = ctx.stream(filt, ys, chunk_frames=chunk)
            assert np.array_equal(out, ref), (filt, chunk)
        pin_in, pin_out = ctx.pinned_empty(ys.shape), ctx.pinned_empty(ys.shape)
        try:
            pin_in[...] = ys
            ctx.stream(filt, pin_in, out=pin_out, chunk_frames=2)
            assert np.array_equal(pin_out, ref), filt
        finally:
            ctx.pinned_free(pin_in)
            ctx.pinned_free(pin_out)
        d_in, d_out, _ = ctx.pool_alloc(filt, w, h, n, k=0, sigma=float("nan"), tries=2)
        try:
            ctx.h2d(d_in, ys)
            ctx.filter_dev(filt, d_in, d_out, w, h, n, 0, 0.0)
            ctx.sync()
            got = np.empty_like(ys)
            ctx.d2h(got, d_out)
            assert np.array_equal(got, ref), filt
        finally:
            ctx.pool_free(d_in, d_out)


@pytest.mark.parametrize("members", [1, 2, 3])
def test_group_on_one_gpu(pkg, members):
    n, h, w = 7, 53, 91
    ys = np.stack([CONTENTS[s % len(CONTENTS)](h, w, 1, s + 50) for s in range(n)])
    with pkg.Group([0] * members) as g:
        for filt, ref in ((pkg.FILTER_EQUALIZE_GRAY8, equalize_ref(ys)), (pkg.FILTER_OTSU_GRAY8, otsu_ref(ys))):
            out, _ = g.filter_batched(filt, ys)
            assert np.array_equal(out, ref), (members, filt)
        mcs = [g.member(i) for i in range(members)]
        shards = [pkg.group_shard(i, members, n) for i in range(members)]
        bufs = []
        try:
            for i, (first, cnt) in enumerate(shards):
                nb = max(1, cnt) * h * w
                d_in, d_out = mcs[i].alloc(nb), mcs[i].alloc(nb)
                bufs.append((d_in, d_out))
                if cnt:
                    mcs[i].h2d(d_in, ys[first:first + cnt])
            g.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, [b[0] for b in bufs], [b[1] for b in bufs], w, h,
                         [s[1] for s in shards])
            for i, (first, cnt) in enumerate(shards):
                if cnt:
                    got = np.empty_like(ys[first:first + cnt])
                    mcs[i].d2h(got, bufs[i][1])
                    assert np.array_equal(got, equalize_ref(ys[first:first + cnt])), i
        finally:
            for i, (d_in, d_out) in enumerate(bufs):
                mcs[i].free(d_in)
                mcs[i].free(d_out)


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_argument_checks(ctx, pkg):
    h, w = 8, 8
    base = ctx.alloc(4096)
    try:
        d_in, d_out = base, base + 1024
        ctx.h2d(d_in, noise(h, w, 1, 1))
        for filt in (pkg.FILTER_EQUALIZE_GRAY8, pkg.FILTER_OTSU_GRAY8):
            # in place and overlapping input and output
            for d_o in (d_in, d_in + 4, d_in + h * w - 1):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_o, w, h, 1, 0, 0.0)
                assert e.value.code == -1, filt
            ctx.filter_dev(filt, d_in, d_out, w, h, 1, 3, float("nan"))  # k and sigma are ignored
            # w * h of 2^31 or more: rejected before any device work
            for bw, bh in ((65536, 32768), (2 ** 30, 2), (46341, 46341)):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_out, bw, bh, 1, 0, 0.0)
                assert e.value.code == -1, (filt, bw, bh)
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.pool_alloc(filt, 65536, 32768, 1, k=0, sigma=0.0, tries=1)
            assert e.value.code == -1, filt
        for fn in (ctx.hist_gray8_dev, ctx.otsu_thresholds_gray8_dev):
            for d_o in (d_in, d_in + 4, d_in + h * w - 4):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_in, d_o, w, h, 1)
                assert e.value.code == -1, fn.__name__
            with pytest.raises(pkg.Mi355Error) as e:
                fn(d_in, d_out + 2, w, h, 1)  # 4-byte outputs need 4-byte alignment
            assert e.value.code == -1, fn.__name__
            with pytest.raises(pkg.Mi355Error) as e:
                fn(d_in, d_out, 65536, 32768, 1)
            assert e.value.code == -1, fn.__name__
            for bad in ((0, h, 1), (w, 0, 1), (w, h, 0)):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_in, d_out, *bad)
                assert e.value.code == -1, (fn.__name__, bad)
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        y = noise(31, 17, 1, 3)
        for filt in (pkg.FILTER_EQUALIZE_GRAY8, pkg.FILTER_OTSU_GRAY8):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx._host_gray8(filt, y)
            assert e.value.code == -4, filt
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.stream(filt, y[None].copy())
            assert e.value.code == -4, filt
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


# ---- chains -----------------------------------------------------------------------------------------------------------
def test_edge_mask_chain(pkg, oracle):
    """PIPELINE -> OTSU_GRAY8 -> CLOSE_GRAY8, device-resident, against the composed references."""
    n, h, w, k, sigma = 3, 120, 161, 5, 1.5
    frames = oracle.synth_rgba(w, h, n, first_frame=0, seed=0x5EED, mode=1)
    with pkg.Context(0) as c:
        c.set_gauss_mode(pkg.GAUSS_EXACT)
        d_rgba, d_mag = c.alloc(frames.nbytes), c.alloc(n * h * w)
        d_mask, d_closed = c.alloc(n * h * w), c.alloc(n * h * w)
        try:
            c.h2d(d_rgba, frames)
            c.filter_dev(pkg.FILTER_PIPELINE, d_rgba, d_mag, w, h, n, k, sigma)
            c.filter_dev(pkg.FILTER_OTSU_GRAY8, d_mag, d_mask, w, h, n)
            c.filter_dev(pkg.FILTER_CLOSE_GRAY8, d_mask, d_closed, w, h, n, 3)
            c.sync()
            got = np.empty((n, h, w), np.uint8)
            c.d2h(got, d_closed)
        finally:
            c.sync()
            for p in (d_rgba, d_mag, d_mask, d_closed):
                c.free(p)
    for f in range(n):
        mag = oracle.pipeline_rgba(frames[f], k, sigma)
        want = morph_ref("close", otsu_ref(mag), 3)
        assert np.array_equal(got[f], want), f


def test_gray1_then_equalize(ctx, pkg, oracle):
    frames = oracle.synth_rgba(97, 61, 2, first_frame=0, seed=0x5EED, mode=1)
    y = ctx.gray1(frames)
    assert np.array_equal(ctx.equalize_hist_gray8(y), equalize_ref(y))


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from hist_ref import equalize_ref, hist_ref, otsu_ref
from test_gpu_median import noise, patches
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n = 640, 480, 2
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    ys = [np.stack([noise(h, w, 1, 11), patches(h, w, 1, 12)]), np.stack([patches(h, w, 1, 21), noise(h, w, 1, 22) >> 3])]
    d_in = torch.from_numpy(ys[0]).to(dev)
    o_hist = torch.zeros((n, 256), dtype=torch.int32, device=dev)
    o_eq = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    o_otsu = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)

    def chain():
        c.hist_gray8_dev(d_in.data_ptr(), o_hist.data_ptr(), w, h, n)
        c.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, d_in.data_ptr(), o_eq.data_ptr(), w, h, n)
        c.filter_dev(pkg.FILTER_OTSU_GRAY8, d_in.data_ptr(), o_otsu.data_ptr(), w, h, n)

    chain()                             # warm-up: sizes the pooled scratch
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for r in range(2):
        y = ys[1 - r]
        d_in.copy_(torch.from_numpy(y).to(dev))
        o_hist.zero_()
        o_eq.zero_()
        o_otsu.zero_()
        g.replay()
        s.synchronize()
        if not np.array_equal(o_hist.cpu().numpy().view(np.uint32), hist_ref(y)): bad.append((r, "hist"))
        if not np.array_equal(o_eq.cpu().numpy(), equalize_ref(y)): bad.append((r, "equalize"))
        if not np.array_equal(o_otsu.cpu().numpy(), otsu_ref(y)): bad.append((r, "otsu"))
    del g
    c.close()
print(bad)
"""


def test_statistics_calls_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled histograms and tables, hist -> equalize -> Otsu allocate nothing and
    synchronise nothing (the zeroing is an in-stream memset), so the chain is captured into a hipGraph and replayed on
    new content.  Own process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
