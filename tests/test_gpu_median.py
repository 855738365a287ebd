"""GPU suite (-m gpu): the median filter, MI355_FILTER_MEDIAN (RGBA) and MI355_FILTER_MEDIAN_GRAY8 (1 byte per pixel).

The output of a median is an input byte, so every comparison here is bit-identity: against the CPU reference
tests/median_ref.py (cv::medianBlur semantics: clamp-to-edge window, every channel, alpha included), and between the
two independent GPU implementations (AUTO: packed-u16 compare networks for k = 3, 5; TILE: LDS counting selection).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from median_ref import median_ref, sample_rows  # noqa: E402
from test_published_mae import NAMES, _committed  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (3, 5, 7)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 5), (75, 75), (250, 17), (1022, 33), (1023, 819), (480, 640)]


def _hash(n, seed):
    i = np.arange(n, dtype=np.uint64)
    v = (i + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    v ^= v >> np.uint64(29)
    v *= np.uint64(0xBF58476D1CE4E5B9)
    v ^= v >> np.uint64(32)
    return (v & np.uint64(0xFF)).astype(np.uint8)


def noise(h, w, c, seed):
    """hash noise in every channel (for RGBA: per-pixel random alpha)"""
    return _hash(h * w * c, seed).reshape((h, w, c) if c > 1 else (h, w))


def patches(h, w, c, seed):
    ph, pw = (h + 63) // 64, (w + 63) // 64
    v = noise(ph, pw, c, seed)
    return np.ascontiguousarray(np.repeat(np.repeat(v, 64, 0), 64, 1)[:h, :w])


def extremes(h, w, c, seed):
    return np.where(noise(h, w, c, seed) & 1, 255, 0).astype(np.uint8)


def constant(h, w, c, seed):
    return np.full((h, w, c) if c > 1 else (h, w), 37 + seed % 200, np.uint8)


def impulses(h, w, c, seed):
    """smooth gradient with 5 % salt-and-pepper pixels"""
    yy, xx = np.mgrid[0:h, 0:w]
    g = ((yy * 3 + xx * 5) % 256).astype(np.uint8)
    img = np.repeat(g[..., None], c, 2) if c > 1 else g
    img = img.copy()
    r = _hash(h * w, seed + 1).reshape(h, w)
    img[r < 7] = 0
    img[r > 248] = 255
    return np.ascontiguousarray(img)


CONTENTS = [noise, patches, extremes, constant, impulses]


def _run(ctx, pkg, impl, gray8, img, k):
    ctx.set_impl(impl)
    try:
        return ctx.median_gray8(img, k) if gray8 else ctx.median(img, k)
    finally:
        ctx.set_impl(pkg.IMPL_AUTO)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
@pytest.mark.parametrize("k", KS)
def test_median_is_bit_identical_to_the_cpu_reference(ctx, pkg, gray8, k):
    c = 1 if gray8 else 4
    for shape in SHAPES:
        for make in CONTENTS:
            img = make(shape[0], shape[1], c, shape[0] * 31 + shape[1] + k)
            auto = _run(ctx, pkg, pkg.IMPL_AUTO, gray8, img, k)
            tile = _run(ctx, pkg, pkg.IMPL_TILE, gray8, img, k)
            assert np.array_equal(auto, tile), (shape, make.__name__, k)
            big = shape[0] * shape[1] > 100000
            rows = sample_rows(shape[0], k) if big else None
            ref = median_ref(img, k, rows=rows)
            assert np.array_equal(auto if rows is None else auto[rows], ref), (shape, make.__name__, k)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_median_of_a_4k_frame(ctx, pkg, gray8):
    c = 1 if gray8 else 4
    h, w = 2160, 3840
    for make in (noise, impulses):
        img = make(h, w, c, 4)
        for k in KS:
            auto = _run(ctx, pkg, pkg.IMPL_AUTO, gray8, img, k)
            tile = _run(ctx, pkg, pkg.IMPL_TILE, gray8, img, k)
            assert np.array_equal(auto, tile), (make.__name__, k)
            rows = sample_rows(h, k)
            assert np.array_equal(auto[rows], median_ref(img, k, rows=rows)), (make.__name__, k)


def test_gray8_any_byte_alignment(ctx, pkg):
    n, h, w = 2, 41, 77
    ys = np.stack([noise(h, w, 1, s) for s in range(n)])
    nb = ys.nbytes
    base = ctx.alloc(2 * nb + 64)
    try:
        for k in (3, 5, 7):
            ref = np.stack([median_ref(y, k) for y in ys])
            for off_in in range(16):
                off_out = (off_in * 7 + 3) % 16
                d_in, d_out = base + off_in, base + nb + 32 + off_out
                ctx.h2d(d_in, ys)
                ctx.filter_dev(pkg.FILTER_MEDIAN_GRAY8, d_in, d_out, w, h, n, k, 0.0)
                ctx.sync()
                got = np.empty_like(ys)
                ctx.d2h(got, d_out)
                assert np.array_equal(got, ref), (k, off_in, off_out)
    finally:
        ctx.sync()
        ctx.free(base)


@pytest.mark.parametrize("k", KS)
def test_gray8_median_is_the_r_channel_of_the_rgba_median(ctx, k):
    y = noise(123, 201, 1, k)
    rgba = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
    assert np.array_equal(ctx.median_gray8(y, k), ctx.median(rgba, k)[..., 0])


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_frames_never_leak_into_each_other(ctx, pkg, gray8):
    n, h, w = 64, 480, 640
    shape = (n, h, w) if gray8 else (n, h, w, 4)
    frames = np.zeros(shape, np.uint8)
    frames[1::2] = 255
    for k in KS:
        for impl in (pkg.IMPL_AUTO, pkg.IMPL_TILE):
            got = _run(ctx, pkg, impl, gray8, frames, k)
            assert np.array_equal(got, frames), (k, impl)


def test_salt_and_pepper_on_the_reference_photographs(ctx):
    rng = np.random.default_rng(2024)
    seen = 0
    for name in NAMES:
        c = _committed(name)
        if c is None:
            continue
        seen += 1
        clean = np.ascontiguousarray(np.dstack([c[0], np.full(c[0].shape[:2], 255, np.uint8)]))
        noisy = clean.copy()
        r = rng.random(clean.shape[:2])
        noisy[r < 0.025, :3] = 0
        noisy[r > 0.975, :3] = 255
        got = ctx.median(noisy, 3)
        assert np.array_equal(got, median_ref(noisy, 3)), name
        # the impulses are gone: the filtered noisy photo is within a fraction of the noise's error of the filtered clean
        # one.  (Against the clean photo itself the 3x3 median of these small, detailed thumbnails loses more detail than
        # the noise costs: 11.3 vs 4.1 on Tulips_square75, and only Artemis_medium640 gains, 2.7 vs 4.8.)
        mae_noisy = np.abs(noisy.astype(int) - clean).mean()
        mae_med = np.abs(got.astype(int) - ctx.median(clean, 3)).mean()
        assert mae_med < 0.5 * mae_noisy, (name, mae_med, mae_noisy)
        y = np.ascontiguousarray(c[1])
        ny = y.copy()
        ny[r < 0.025] = 0
        ny[r > 0.975] = 255
        assert np.array_equal(ctx.median_gray8(ny, 3), median_ref(ny, 3)), name
    assert seen >= 5


# ---- host paths -----------------------------------------------------------------------------------------------------
def test_batched_stream_and_pool(ctx, pkg):
    n, h, w = 6, 67, 129
    for filt, c in ((pkg.FILTER_MEDIAN, 4), (pkg.FILTER_MEDIAN_GRAY8, 1)):
        frames = np.stack([noise(h, w, c, s) for s in range(n)])
        for k in KS:
            ref = np.stack([median_ref(f, k) for f in frames])
            batched = ctx.median_gray8(frames, k) if c == 1 else ctx.median(frames, k)
            assert np.array_equal(batched, ref), (filt, k)
            out, ms = ctx.stream(filt, frames, k=k, chunk_frames=4)  # pageable
            assert np.array_equal(out, ref), (filt, k)
            pin_in, pin_out = ctx.pinned_empty(frames.shape), ctx.pinned_empty(frames.shape)
            try:
                pin_in[...] = frames
                out, ms = ctx.stream(filt, pin_in, out=pin_out, k=k, chunk_frames=2)
                assert np.array_equal(pin_out, ref), (filt, k)
            finally:
                ctx.pinned_free(pin_in)
                ctx.pinned_free(pin_out)
        d_in, d_out, probe = ctx.pool_alloc(filt, w, h, n, k=3, sigma=float("nan"), tries=2)
        try:
            ctx.h2d(d_in, frames)
            ctx.filter_dev(filt, d_in, d_out, w, h, n, 3, 0.0)
            ctx.sync()
            got = np.empty_like(frames)
            ctx.d2h(got, d_out)
            assert np.array_equal(got, np.stack([median_ref(f, 3) for f in frames])), filt
        finally:
            ctx.pool_free(d_in, d_out)


def test_bgr_input(ctx, pkg):
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for k in KS:
            assert np.array_equal(ctx.median(bgr, k), median_ref(rgba, k)), k
        out, _ = ctx.stream(pkg.FILTER_MEDIAN, bgr[None].copy(), k=5)
        assert np.array_equal(out[0], median_ref(rgba, 5))
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.median_gray8(bgr[..., 0], 3)
        assert e.value.code == -4
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


@pytest.mark.parametrize("members", [1, 2, 3])
def test_group_on_one_gpu(pkg, members):
    n, h, w = 7, 53, 91
    rgba = np.stack([noise(h, w, 4, s) for s in range(n)])
    ys = np.stack([noise(h, w, 1, s + 50) for s in range(n)])
    with pkg.Group([0] * members) as g:
        for filt, frames in ((pkg.FILTER_MEDIAN, rgba), (pkg.FILTER_MEDIAN_GRAY8, ys)):
            for k in KS:
                out, _ = g.filter_batched(filt, frames, k=k)
                assert np.array_equal(out, np.stack([median_ref(f, k) for f in frames])), (members, filt, k)
            for bad in (0, 4, 9, -3, 1 << 30):
                with pytest.raises(pkg.Mi355Error) as e:
                    g.filter_batched(filt, frames, k=bad)
                assert e.value.code == -1, (filt, bad)
        # device-resident: every member filters its own shard
        mcs = [g.member(i) for i in range(members)]
        shards = [pkg.group_shard(i, members, n) for i in range(members)]
        bufs = []
        try:
            for i, (first, cnt) in enumerate(shards):
                nb = max(1, cnt) * h * w * 4
                d_in, d_out = mcs[i].alloc(nb), mcs[i].alloc(nb)
                bufs.append((d_in, d_out))
                if cnt:
                    mcs[i].h2d(d_in, rgba[first:first + cnt])
            g.filter_dev(pkg.FILTER_MEDIAN, [b[0] for b in bufs], [b[1] for b in bufs], w, h, [s[1] for s in shards],
                         k=5)
            for i, (first, cnt) in enumerate(shards):
                if cnt:
                    got = np.empty_like(rgba[first:first + cnt])
                    mcs[i].d2h(got, bufs[i][1])
                    assert np.array_equal(got, np.stack([median_ref(f, 5) for f in rgba[first:first + cnt]])), i
        finally:
            for i, (d_in, d_out) in enumerate(bufs):
                mcs[i].free(d_in)
                mcs[i].free(d_out)


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_argument_checks(ctx, pkg):
    h, w = 8, 8
    base = ctx.alloc(4 * h * w * 3 + 64)
    try:
        d_in, d_out = base, base + 4 * h * w + 16
        ctx.h2d(d_in, noise(h, w, 4, 1))
        for filt in (pkg.FILTER_MEDIAN, pkg.FILTER_MEDIAN_GRAY8):
            for k in (-3, 0, 1, 2, 4, 9, 63):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_out, w, h, 1, k, 0.0)
                assert e.value.code == -1, (filt, k)
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.stream(filt, np.zeros((1, h, w, 4) if filt == pkg.FILTER_MEDIAN else (1, h, w), np.uint8), k=k)
                assert e.value.code == -1, (filt, k)
            # overlapping input and output
            for d_o in (d_in, d_in + 4, d_in + h * w - 4):  # inside the input range of both layouts
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_o, w, h, 1, 3, 0.0)
                assert e.value.code == -1, filt
            # sigma is ignored: NaN is fine
            ctx.filter_dev(filt, d_in, d_out, w, h, 1, 3, float("nan"))
        with pytest.raises(pkg.Mi355Error) as e:
            ctx._host(pkg.FILTER_MEDIAN, noise(h, w, 4, 1), 11)
        assert e.value.code == -1
        # RGBA needs dword-aligned pointers, in and out
        for a, b in ((d_in + 1, d_out), (d_in, d_out + 2)):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.filter_dev(pkg.FILTER_MEDIAN, a, b, w, h, 1, 3, 0.0)
            assert e.value.code == -1
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)
