"""GPU suite (-m gpu): mi355_resize_dev / mi355_resize_batched, cv::resize of RGBA and gray8 frames.

Every comparison is bit-identity against the CPU reference tests/resize_ref.py (the header's arithmetic in numpy):
NEAREST, LINEAR (11-bit fixed point, AREA's result at exactly half size) and AREA with integer factors.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded  # noqa: E402
from resize_ref import AREA, LINEAR, NEAREST, accepts, resize_ref, sample_rows  # noqa: E402
from test_gpu_median import constant, extremes, noise  # noqa: E402

pytestmark = pytest.mark.gpu

INTERPS = (NEAREST, LINEAR, AREA)
NAMES = {NEAREST: "nearest", LINEAR: "linear", AREA: "area"}
BPP_INTERP = [(bpp, i) for bpp in (4, 1) for i in INTERPS]
BPP_INTERP_IDS = ["%s-%s" % ("rgba" if b == 4 else "gray8", NAMES[i]) for b, i in BPP_INTERP]

# (src w, src h, dst w, dst h): the smallest at which the kernel can go wrong — one pixel, fewer columns than a lane
# owns, a ragged last lane and last strip (dst w % 4, dst w % 256), more than one strip and band, up in one direction
# and down in the other, many band boundaries, the 2 x rule on even and odd halves, and every AREA path (2 and 4 in x
# with 16-byte loads, other factors pixel by pixel, 16 x)
SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (5, 3, 1, 1), (2, 2, 257, 3), (7, 5, 13, 9), (13, 9, 7, 5), (64, 48, 21, 16),
          (21, 16, 64, 48), (100, 90, 250, 30), (3, 1000, 5, 2333), (75, 75, 240, 240), (640, 480, 320, 240),
          (642, 482, 321, 241), (1023, 819, 640, 512), (640, 427, 1023, 683), (3840, 6, 1280, 2), (4096, 32, 256, 2),
          (96, 96, 32, 24)]
LARGE = [(3840, 2160, 1920, 1080), (3840, 2160, 1280, 720), (1920, 1080, 3840, 2160)]


def one_bright_pixel(h, w, c, seed):
    img = np.zeros((h, w, c) if c > 1 else (h, w), np.uint8)
    img[(seed * 7) % h, (seed * 13) % w] = 255
    return img


def horizontal_ramp(h, w, c, seed):
    g = np.broadcast_to(((np.arange(w) * 255) // max(1, w - 1)).astype(np.uint8)[None, :], (h, w))
    return np.ascontiguousarray(np.repeat(g[..., None], c, 2) if c > 1 else g)


def vertical_ramp(h, w, c, seed):
    g = np.broadcast_to(((np.arange(h) * 255) // max(1, h - 1)).astype(np.uint8)[:, None], (h, w))
    return np.ascontiguousarray(np.repeat(g[..., None], c, 2) if c > 1 else g)


CONTENTS = [noise, extremes, constant, one_bright_pixel, horizontal_ramp, vertical_ramp]


def _run(ctx, bpp, img, dw, dh, interp):
    return ctx.resize(img, dw, dh, interp) if bpp == 4 else ctx.resize_gray8(img, dw, dh, interp)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_resize_is_bit_identical_to_the_cpu_reference(ctx, bpp, interp):
    ran = 0
    for sw, sh, dw, dh in SHAPES:
        if not accepts(interp, sw, sh, dw, dh):
            continue
        for make in CONTENTS:
            img = make(sh, sw, bpp, sw * 31 + sh + dw)
            got = _run(ctx, bpp, img, dw, dh, interp)
            ref = resize_ref(img, dw, dh, interp)
            assert got.shape == ref.shape and np.array_equal(got, ref), ((sw, sh, dw, dh), make.__name__)
            ran += 1
    assert ran == (7 if interp == AREA else len(SHAPES)) * len(CONTENTS)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_large_frames_on_sampled_rows(ctx, bpp, interp):
    for sw, sh, dw, dh in LARGE:
        if not accepts(interp, sw, sh, dw, dh):
            continue
        img = noise(sh, sw, bpp, dw)
        img[sh // 2:sh // 2 + 100, sw // 3:sw // 3 + 300] = 200
        got = _run(ctx, bpp, img, dw, dh, interp)
        rows = sample_rows(dh)
        assert np.array_equal(got[rows], resize_ref(img, dw, dh, interp, rows=rows)), (sw, sh, dw, dh)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_frames_are_independent(ctx, bpp, interp):
    """Three frames of different content equal three single-frame calls, and on frames that alternate between 0 and 255
    no output pixel mixes in a neighbouring frame at a frame's last row or column."""
    for sw, sh, dw, dh in ((77, 41, 33, 19), (21, 16, 64, 48), (66, 38, 33, 19), (132, 57, 33, 19)):
        if not accepts(interp, sw, sh, dw, dh):
            continue
        frames = np.stack([noise(sh, sw, bpp, 5), extremes(sh, sw, bpp, 6), horizontal_ramp(sh, sw, bpp, 7)])
        got = _run(ctx, bpp, frames, dw, dh, interp)
        for f in range(3):
            assert np.array_equal(got[f], _run(ctx, bpp, frames[f], dw, dh, interp)), (sw, sh, dw, dh, f)
            assert np.array_equal(got[f], resize_ref(frames[f], dw, dh, interp)), (sw, sh, dw, dh, f)
        flat = np.zeros((6,) + frames.shape[1:], np.uint8)
        flat[1::2] = 255
        want = np.zeros((6,) + got.shape[1:], np.uint8)
        want[1::2] = 255
        assert np.array_equal(_run(ctx, bpp, flat, dw, dh, interp), want), (sw, sh, dw, dh)


GUARDED_SHAPES = {NEAREST: [(21, 16, 64, 48), (1023, 9, 640, 5), (77, 41, 33, 19)],
                  LINEAR: [(21, 16, 64, 48), (1023, 9, 640, 5), (77, 41, 33, 19)],
                  # AREA takes integer factors only: 2 x 2 over full and ragged strips, 3 x 4, 4 x 3
                  AREA: [(1320, 10, 660, 5), (154, 82, 77, 41), (99, 76, 33, 19), (132, 57, 33, 19)]}


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_guarded_arena(ctx, bpp, interp):
    """No guard byte changes and no payload byte is left unwritten, at every pointer alignment the call accepts."""
    offs_in = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3)
    offs_out = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3, 5, 15)
    for sw, sh, dw, dh in GUARDED_SHAPES[interp]:
        img = noise(sh, sw, bpp, sw + dh)
        ref = resize_ref(img, dw, dh, interp)
        for off_in in offs_in:
            for off_out in offs_out:
                tag = "%s bpp %d %dx%d->%dx%d" % (NAMES[interp], bpp, sw, sh, dw, dh)
                got = guarded.run(ctx, lambda a, b: ctx.resize_dev(a, b, bpp, sw, sh, dw, dh, 1, interp), img, ref,
                                  off_in=off_in, off_out=off_out, tag=tag)
                guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))


def test_host_call_equals_device_call_and_profiles(ctx):
    for bpp in (4, 1):
        for interp, (sw, sh, dw, dh) in ((NEAREST, (77, 41, 200, 19)), (LINEAR, (201, 123, 97, 151)),
                                         (AREA, (192, 120, 64, 60))):
            n = 2
            frames = np.stack([noise(sh, sw, bpp, s) for s in range(n)])
            out_shape = (n, dh, dw, 4) if bpp == 4 else (n, dh, dw)
            d_in, d_out = ctx.alloc(frames.nbytes), ctx.alloc(int(np.prod(out_shape)))
            try:
                ctx.h2d(d_in, frames)
                ctx.resize_dev(d_in, d_out, bpp, sw, sh, dw, dh, n, interp)
                ctx.sync()
                dev = np.empty(out_shape, np.uint8)
                ctx.d2h(dev, d_out)
            finally:
                ctx.sync()
                ctx.free(d_in)
                ctx.free(d_out)
            assert np.array_equal(_run(ctx, bpp, frames, dw, dh, interp), dev), (bpp, interp)
            assert np.array_equal(dev, np.stack([resize_ref(f, dw, dh, interp) for f in frames])), (bpp, interp)
    out, prof = ctx.resize(noise(123, 201, 4, 1), 97, 151, LINEAR, profile=True)
    assert out.shape == (151, 97, 4) and len(prof) == 6
    assert all(prof[i] <= prof[i + 1] for i in range(5)) and prof[5] > prof[0], prof


def test_bgr_input(ctx, pkg):
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for interp, (dw, dh) in ((NEAREST, (50, 201)), (LINEAR, (250, 31)), (AREA, (19, 97))):
            assert np.array_equal(ctx.resize(bgr, dw, dh, interp), resize_ref(rgba, dw, dh, interp)), interp
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.resize_gray8(bgr[..., 0], dw, dh, interp)
            assert e.value.code == -4, interp
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
    assert np.array_equal(ctx.resize(rgba, 50, 201, LINEAR), resize_ref(rgba, 50, 201, LINEAR))


def test_rejections(ctx, pkg):
    sw, sh, dw, dh = 16, 8, 32, 16                              # in: 512 B (RGBA), out: 2048 B
    base = ctx.alloc(8192)
    try:
        ctx.h2d(base, noise(sh, sw, 4, 1))
        for bpp in (4, 1):
            nin, nout = sw * sh * bpp, dw * dh * bpp
            for interp in (NEAREST, LINEAR):
                # in place; the output starts inside the input; only the larger (output) side reaches over the input
                for d_in, d_out in ((base, base), (base, base + nin - 4), (base + nout - 4, base),
                                    (base + 4096, base + 4096 + nin - 4), (base + nout // 2, base)):
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.resize_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, interp)
                    assert e.value.code == -1, (bpp, interp, d_in - base, d_out - base)
                ctx.resize_dev(base, base + nin, bpp, sw, sh, dw, dh, 1, interp)       # touching ranges are fine
                ctx.resize_dev(base + nout, base, bpp, sw, sh, dw, dh, 1, interp)
            # downscaling: only the larger (input) side reaches over the output
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.resize_dev(base, base + nout - 4, bpp, dw, dh, sw, sh, 1, AREA)
            assert e.value.code == -1, bpp
        for a, b in ((base + 1, base + 4096), (base, base + 4098), (base + 2, base + 4099)):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.resize_dev(a, b, 4, sw, sh, dw, dh, 1, LINEAR)
            assert e.value.code == -1, (a - base, b - base)
            ctx.resize_dev(a, b, 1, sw, sh, dw, dh, 1, LINEAR)                        # gray8 takes any alignment
        for s in ((640, 480, 427, 320), (320, 240, 640, 480), (1700, 100, 100, 100)):
            for bpp in (4, 1):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.resize_dev(base, base + 4096, bpp, s[0], s[1], s[2], s[3], 1, AREA)
                assert e.value.code == -4, (s, bpp)
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.resize(np.zeros((240, 320, 4), np.uint8), 640, 480, AREA)
        assert e.value.code == -4
        for interp in (2, 4, -1):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.resize_dev(base, base + 4096, 4, sw, sh, dw, dh, 1, interp)
            assert e.value.code == -1, interp
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_resized_frame_feeds_the_pipeline(ctx, pkg):
    """4K -> 1080p on the device, then MI355_FILTER_PIPELINE on that buffer, equals the pipeline of the reference-resized
    frame: the output is an ordinary frame for every other call."""
    sw, sh, dw, dh = 3840, 2160, 1920, 1080
    img = noise(sh, sw, 4, 3)
    img[..., 3] = 255
    small = resize_ref(img, dw, dh, LINEAR)                     # the 2 x rule: AREA
    d_in, d_mid, d_out = ctx.alloc(img.nbytes), ctx.alloc(small.nbytes), ctx.alloc(dw * dh)
    try:
        ctx.h2d(d_in, img)
        ctx.resize_dev(d_in, d_mid, 4, sw, sh, dw, dh, 1, LINEAR)
        ctx.filter_dev(pkg.FILTER_PIPELINE, d_mid, d_out, dw, dh, 1, 5, 1.5)
        ctx.sync()
        mid, got = np.empty_like(small), np.empty((dh, dw), np.uint8)
        ctx.d2h(mid, d_mid)
        ctx.d2h(got, d_out)
    finally:
        ctx.sync()
        ctx.free(d_in)
        ctx.free(d_mid)
        ctx.free(d_out)
    assert np.array_equal(mid, small)
    assert np.array_equal(got, ctx.pipeline(small, 5, 1.5))
