"""GPU suite (-m gpu): the box mean, MI355_FILTER_BOX (RGBA) and MI355_FILTER_BOX_GRAY8, and the mean adaptive threshold
of gray8 frames (mi355_adaptive_threshold_gray8_*).

Both are integer-exact, so every comparison here is bit-identity with tests/box_ref.py: cv::blur with BORDER_REPLICATE as
out = floor((2 s + d) / (2 d)), and cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) on top of it.  tests/box_cases.py
restates the kernel's strip and band rule to choose the shapes and batch sizes that reach its seams.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import box_cases as bc  # noqa: E402
import guarded  # noqa: E402
from box_ref import BINARY, BINARY_INV, adaptive_ref, box_ref  # noqa: E402
from median_ref import sample_rows  # noqa: E402
from test_gpu_median import noise  # noqa: E402

pytestmark = pytest.mark.gpu

GRAY8 = pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])


def _run(ctx, gray8, img, k):
    return ctx.box_gray8(img, k) if gray8 else ctx.box(img, k)


def _fid(pkg, gray8):
    return pkg.FILTER_BOX_GRAY8 if gray8 else pkg.FILTER_BOX


def _cycle(distinct, n):
    """n frames: the few distinct ones repeated cyclically; and the index of each frame's reference."""
    idx = np.arange(n) % len(distinct)
    return np.ascontiguousarray(np.stack(distinct)[idx]), idx


# ---- 1. against the reference ---------------------------------------------------------------------------------------
@GRAY8
@pytest.mark.parametrize("k", bc.KS)
def test_box_is_bit_identical_to_the_cpu_reference(ctx, gray8, k):
    c = 1 if gray8 else 4
    for shape in bc.SHAPES:
        rows = sample_rows(shape[0], 2 * k) if shape[0] * shape[1] > 100000 else None
        for make in bc.CONTENTS:
            img = make(shape[0], shape[1], c, shape[0] * 31 + shape[1] + k)
            got = _run(ctx, gray8, img, k)
            assert np.array_equal(got if rows is None else got[rows], box_ref(img, k, rows=rows)), (k, shape, make.__name__)
    for v in (0, 127, 254):
        img = bc.staircase(k, v, c)
        assert np.array_equal(_run(ctx, gray8, img, k), box_ref(img, k)), (k, v)


# ---- 2. running sums down many bands, clamped ends ------------------------------------------------------------------
@GRAY8
@pytest.mark.parametrize("k", bc.KS)
def test_running_sums_do_not_drift_and_clamp_at_both_ends(ctx, gray8, k):
    """The top r + 1 rows subtract the same clamped row again and again and the bottom rows add it; alternating 0 / 255
    rows make every add and subtract the largest there is.  Every row is compared."""
    c = 1 if gray8 else 4
    h = 3 * bc.band_heights(k)[0] + 1
    for w in (5, bc.strip_cols(k, gray8) + 1):
        for img in (bc.alternating_rows(h, w, c), noise(h, w, c, k)):
            assert np.array_equal(_run(ctx, gray8, img, k), box_ref(img, k)), (k, w)


# ---- 3. seams -------------------------------------------------------------------------------------------------------
@GRAY8
@pytest.mark.parametrize("k", (3, 17, 63))
def test_strip_seams(ctx, gray8, k):
    c = 1 if gray8 else 4
    strip = bc.strip_cols(k, gray8)
    h = 2 * bc.band_heights(k)[-1] + 1
    for w in (strip - 1, strip, strip + 1, 2 * strip + 1):
        for make in (noise, bc.all_255):
            img = make(h, w, c, w + k)
            assert np.array_equal(_run(ctx, gray8, img, k), box_ref(img, k)), (k, w, make.__name__)


@GRAY8
@pytest.mark.parametrize("k", (3, 17, 63))
def test_every_band_height_the_plan_can_choose(ctx, gray8, k):
    """Batches sized so that the launch takes each band height in turn, on frames of 2 bands + 1 row; three distinct
    frames repeated cyclically."""
    c = 1 if gray8 else 4
    w = 5
    for rows in bc.band_heights(k):
        h = 2 * rows + 1
        n = bc.frames_for(k, w, h, rows, gray8)
        distinct = [noise(h, w, c, 1 + rows), bc.alternating_rows(h, w, c), bc.impulses(h, w, c, 2)]
        frames, idx = _cycle(distinct, n)
        ref = np.stack([box_ref(f, k) for f in distinct])
        assert np.array_equal(_run(ctx, gray8, frames, k), ref[idx]), (k, rows, n)
    # one strip seam under the tallest band
    if k == 3:
        rows = bc.band_heights(k)[0]
        w, h = bc.strip_cols(k, gray8) + 1, 2 * rows + 1
        n = bc.frames_for(k, w, h, rows, gray8)
        distinct = [noise(h, w, c, 7), bc.extremes(h, w, c, 8)]
        frames, idx = _cycle(distinct, n)
        ref = np.stack([box_ref(f, k) for f in distinct])
        assert np.array_equal(_run(ctx, gray8, frames, k), ref[idx]), (k, rows, n)


# ---- 4. frames are independent --------------------------------------------------------------------------------------
@GRAY8
def test_frames_never_leak_into_each_other(ctx, gray8):
    frames = np.zeros((3, 40, 70) if gray8 else (3, 40, 70, 4), np.uint8)
    frames[1] = 255
    assert np.array_equal(_run(ctx, gray8, frames, 63), frames)


@GRAY8
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (5, 7), (13, 17)], ids=lambda s: "%dx%d" % s)
def test_two_thousand_tiny_frames(ctx, gray8, shape):
    c = 1 if gray8 else 4
    n = 2000
    frames = noise(n * shape[0], shape[1], c, 17).reshape((n,) + shape + ((4,) if c > 1 else ()))
    for k in (3, 63):
        got = _run(ctx, gray8, frames, k)
        assert np.array_equal(got, np.stack([box_ref(f, k) for f in frames])), k


# ---- 5. guarded arena -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 17, 63))
def test_guarded_gray8_at_every_alignment(ctx, pkg, k):
    for h, w in ((9, 37), (5, bc.strip_cols(k, True))):
        y = noise(h, w, 1, k)
        mean = box_ref(y, k)
        thr = adaptive_ref(y, 200, BINARY, k, 2, mean=mean)
        for off_in in range(16):
            for off_out in range(16):
                got = guarded.run(ctx, lambda a, b: ctx.filter_dev(pkg.FILTER_BOX_GRAY8, a, b, w, h, 1, k, 0.0), y, mean,
                                  off_in, off_out, tag="box_gray8 k=%d %dx%d" % (k, h, w))
                guarded.check(got, mean, tag="box_gray8 k=%d %dx%d in %d out %d" % (k, h, w, off_in, off_out))
                got = guarded.run(ctx, lambda a, b: ctx.adaptive_threshold_gray8_dev(a, b, w, h, 1, 200, BINARY, k, 2),
                                  y, thr, off_in, off_out, tag="adaptive block=%d %dx%d" % (k, h, w))
                guarded.check(got, thr, tag="adaptive block=%d %dx%d in %d out %d" % (k, h, w, off_in, off_out))


@pytest.mark.parametrize("k", (3, 17, 63))
def test_guarded_rgba_at_every_dword_alignment(ctx, pkg, k):
    for h, w in ((9, 37), (5, bc.strip_cols(k, False))):
        img = noise(h, w, 4, k)
        ref = box_ref(img, k)
        for off_in in (0, 4, 8, 12):
            for off_out in (0, 4, 8, 12):
                got = guarded.run(ctx, lambda a, b: ctx.filter_dev(pkg.FILTER_BOX, a, b, w, h, 1, k, 0.0), img, ref,
                                  off_in, off_out, tag="box k=%d %dx%d" % (k, h, w))
                guarded.check(got, ref, tag="box k=%d %dx%d in %d out %d" % (k, h, w, off_in, off_out))


# ---- 6. adaptive threshold ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", bc.ADAPTIVE_BLOCKS)
def test_adaptive_threshold_is_bit_identical_to_the_cpu_reference(ctx, pkg, block):
    shapes = [s for s in bc.SHAPES if s[0] * s[1] <= 427 * 640]
    assert (427, 640) in shapes and len(shapes) == 9
    for h, w in shapes:
        y = noise(h, w, 1, h + w) if (h, w) != (75, 75) else bc.noise_frame()
        mean = box_ref(y, block)
        gpu_mean = ctx.box_gray8(y, block)
        assert np.array_equal(gpu_mean, mean), (block, h, w)
        big = h * w > 100000
        for type in (BINARY, BINARY_INV):
            for delta in bc.ADAPTIVE_DELTAS:
                for max_value in (bc.ADAPTIVE_MAX_VALUES if not big or delta in (-2.5, 2) else (200,)):
                    got = ctx.adaptive_threshold_gray8(y, max_value, type, block, delta)
                    # the fused launch equals thresholding the mean of a separate BOX_GRAY8 call
                    assert np.array_equal(got, adaptive_ref(y, max_value, type, block, delta, mean=gpu_mean)), \
                        (block, h, w, type, delta, max_value)


def test_adaptive_types_are_not_complements_at_a_fractional_delta(ctx):
    y = bc.noise_frame()
    a = ctx.adaptive_threshold_gray8(y, 255, BINARY, 15, 2.5)
    b = ctx.adaptive_threshold_gray8(y, 255, BINARY_INV, 15, 2.5)
    assert np.any((a == 255) & (b == 255)) and not np.any((a == 0) & (b == 0))
    a = ctx.adaptive_threshold_gray8(y, 255, BINARY, 15, 2.0)
    b = ctx.adaptive_threshold_gray8(y, 255, BINARY_INV, 15, 2.0)
    assert np.array_equal(a, 255 - b)


def test_adaptive_batches_and_profile(ctx):
    frames = np.stack([noise(61, 83, 1, s) for s in range(5)])
    got, prof = ctx.adaptive_threshold_gray8(frames, 255, BINARY_INV, 9, 4, profile=True)
    assert np.array_equal(got, np.stack([adaptive_ref(f, 255, BINARY_INV, 9, 4) for f in frames]))
    assert len(prof) == 6 and all(prof[i] <= prof[i + 1] for i in range(5)) and prof[0] > 0


# ---- 7. contract ----------------------------------------------------------------------------------------------------
BAD_KS = (0, 1, 2, 4, 65, -1)


def test_argument_checks(ctx, pkg):
    h, w = 8, 8
    base = ctx.alloc(4 * h * w * 3 + 64)
    try:
        d_in, d_out = base, base + 4 * h * w + 16
        ctx.h2d(d_in, noise(h, w, 4, 1))
        for gray8 in (False, True):
            filt = _fid(pkg, gray8)
            shape = (1, h, w) if gray8 else (1, h, w, 4)
            for k in BAD_KS:
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_out, w, h, 1, k, 0.0)
                assert e.value.code == -1, (filt, k)
                with pytest.raises(pkg.Mi355Error) as e:
                    _run(ctx, gray8, np.zeros(shape, np.uint8), k)
                assert e.value.code == -1, (filt, k)
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.stream(filt, np.zeros(shape, np.uint8), k=k)
                assert e.value.code == -1, (filt, k)
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.pool_alloc(filt, w, h, 1, k=k, sigma=0.0, tries=1)
                assert e.value.code == -1, (filt, k)
            for d_o in (d_in, d_in + 4, d_in + h * w - 4):          # in place and overlapping
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, d_in, d_o, w, h, 1, 3, 0.0)
                assert e.value.code == -1, filt
            for bad_in, bad_out in ((0, d_out), (d_in, 0)):           # null pointers
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(filt, bad_in, bad_out, w, h, 1, 3, 0.0)
                assert e.value.code == -1, filt
            ctx.filter_dev(filt, d_in, d_out, w, h, 1, 3, float("nan"))  # sigma is ignored
        for a, b in ((d_in + 1, d_out), (d_in, d_out + 2)):           # RGBA needs dword-aligned pointers
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.filter_dev(pkg.FILTER_BOX, a, b, w, h, 1, 3, 0.0)
            assert e.value.code == -1
        # the adaptive call: every value wrong in turn, null and overlapping pointers
        good = dict(max_value=255, type=BINARY, block=3, delta=0.0)
        for bad in (dict(max_value=-1), dict(max_value=256), dict(type=2), dict(type=-1), dict(block=1), dict(block=4),
                    dict(block=65), dict(block=0), dict(delta=float("nan")), dict(delta=float("inf"))):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.adaptive_threshold_gray8_dev(d_in, d_out, w, h, 1, **dict(good, **bad))
            assert e.value.code == -1, bad
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.adaptive_threshold_gray8(np.zeros((h, w), np.uint8), **dict(good, **bad))
            assert e.value.code == -1, bad
        for a, b in ((0, d_out), (d_in, 0), (d_in, d_in), (d_in, d_in + h * w - 1)):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.adaptive_threshold_gray8_dev(a, b, w, h, 1, **good)
            assert e.value.code == -1, (a - d_in, b - d_in)
        ctx.adaptive_threshold_gray8_dev(d_in, d_in + h * w, w, h, 1, **good)  # adjacent ranges are fine
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_sigma_is_ignored(ctx, pkg):
    n, h, w = 2, 31, 45
    for gray8 in (False, True):
        frames = np.stack([noise(h, w, 1 if gray8 else 4, s) for s in range(n)])
        ref = np.stack([box_ref(f, 5) for f in frames])
        for sigma in (0.0, -1.0, 7.5, float("nan")):
            out, _ = ctx.stream(_fid(pkg, gray8), frames, k=5, sigma=sigma)
            assert np.array_equal(out, ref), (gray8, sigma)


def test_batched_stream_and_pool(ctx, pkg):
    n, h, w = 5, 67, 129
    for gray8 in (False, True):
        frames = np.stack([noise(h, w, 1 if gray8 else 4, s) for s in range(n)])
        filt = _fid(pkg, gray8)
        for k in (3, 9, 63):
            ref = np.stack([box_ref(f, k) for f in frames])
            assert np.array_equal(_run(ctx, gray8, frames, k), ref), (gray8, k)
            out, _ = ctx.stream(filt, frames, k=k, chunk_frames=2)  # pageable, ragged last chunk
            assert np.array_equal(out, ref), (gray8, k)
        d_in, d_out, _ = ctx.pool_alloc(filt, w, h, n, k=5, sigma=float("nan"), tries=2)
        try:
            ctx.h2d(d_in, frames)
            ctx.filter_dev(filt, d_in, d_out, w, h, n, 5, 0.0)
            ctx.sync()
            got = np.empty_like(frames)
            ctx.d2h(got, d_out)
            assert np.array_equal(got, np.stack([box_ref(f, 5) for f in frames])), gray8
        finally:
            ctx.pool_free(d_in, d_out)
    rgba = noise(h, w, 4, 9)
    out, prof = ctx.box(rgba, 7, profile=True)
    assert np.array_equal(out, box_ref(rgba, 7)) and len(prof) == 6


def test_bgr_input(ctx, pkg):
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for k in (3, 63):
            assert np.array_equal(ctx.box(bgr, k), box_ref(rgba, k)), k
        out, _ = ctx.stream(pkg.FILTER_BOX, bgr[None].copy(), k=5)
        assert np.array_equal(out[0], box_ref(rgba, 5))
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.box_gray8(bgr[..., 0], 3)
        assert e.value.code == -4
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.adaptive_threshold_gray8(bgr[..., 0], 255, BINARY, 3, 0)
        assert e.value.code == -4
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


def test_two_member_group_on_one_gpu_equals_one_context(ctx, pkg):
    n, h, w = 7, 53, 91
    rgba = np.stack([noise(h, w, 4, s) for s in range(n)])
    ys = np.stack([noise(h, w, 1, s + 50) for s in range(n)])
    with pkg.Group([0, 0]) as g:
        for gray8, frames in ((False, rgba), (True, ys)):
            for k in (3, 63):
                out, _ = g.filter_batched(_fid(pkg, gray8), frames, k=k)
                assert np.array_equal(out, _run(ctx, gray8, frames, k)), (gray8, k)
                assert np.array_equal(out, np.stack([box_ref(f, k) for f in frames])), (gray8, k)
            for bad in BAD_KS:
                with pytest.raises(pkg.Mi355Error) as e:
                    g.filter_batched(_fid(pkg, gray8), frames, k=bad)
                assert e.value.code == -1, (gray8, bad)


# ---- 8. hipGraph capture --------------------------------------------------------------------------------------------
_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from box_ref import BINARY_INV, adaptive_ref, box_ref
from test_gpu_median import noise
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h = 640, 480
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    rgba = [noise(h, w, 4, 11), noise(h, w, 4, 12)]
    gray = [noise(h, w, 1, 21), noise(h, w, 1, 22)]
    d_rgba = torch.from_numpy(rgba[0]).to(dev)
    d_gray = torch.from_numpy(gray[0]).to(dev)
    o_box = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    o_thr = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    s.synchronize()

    def chain():
        c.filter_dev(pkg.FILTER_BOX, d_rgba.data_ptr(), o_box.data_ptr(), w, h, 1, 31, 0.0)
        c.adaptive_threshold_gray8_dev(d_gray.data_ptr(), o_thr.data_ptr(), w, h, 1, 255, BINARY_INV, 15, 2.5)

    # the library's code object is loaded by a call of another kind; the two captured calls are the first of their kind
    # on the context: they have no table to install and no scratch to size
    c.filter_dev(pkg.FILTER_GRAY, d_rgba.data_ptr(), o_box.data_ptr(), w, h, 1)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for n in range(2):
        d_rgba.copy_(torch.from_numpy(rgba[1 - n]).to(dev))
        d_gray.copy_(torch.from_numpy(gray[1 - n]).to(dev))
        o_box.zero_()
        o_thr.zero_()
        g.replay()
        s.synchronize()
        if not np.array_equal(o_box.cpu().numpy(), box_ref(rgba[1 - n], 31)): bad.append((n, "box31"))
        if not np.array_equal(o_thr.cpu().numpy(), adaptive_ref(gray[1 - n], 255, BINARY_INV, 15, 2.5)): bad.append((n, "thr15"))
    del g
    c.close()
print(bad)
"""


def test_box_and_adaptive_threshold_can_be_captured_into_a_hip_graph_from_the_first_call():
    """mi355_filter_dev(BOX) and mi355_adaptive_threshold_gray8_dev make no table, allocate nothing and wait for nothing,
    so they are captured into a hipGraph as the first calls of their kind on a fresh context (after a grayscale call,
    which loads the library's kernels) and replayed on new input."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]


# ---- 9. one 4K frame ------------------------------------------------------------------------------------------------
@GRAY8
def test_box_of_a_4k_frame(ctx, gray8):
    h, w = 2160, 3840
    img = noise(h, w, 1 if gray8 else 4, 4)
    img[1000:1100, 2000:2300] = 200
    for k in (3, 31, 63):
        got = _run(ctx, gray8, img, k)
        rows = sample_rows(h, 2 * k)
        assert np.array_equal(got[rows], box_ref(img, k, rows=rows)), k


def test_adaptive_threshold_of_a_4k_frame(ctx):
    h, w = 2160, 3840
    y = noise(h, w, 1, 6)
    rows = sample_rows(h, 62)
    for type in (BINARY, BINARY_INV):
        got = ctx.adaptive_threshold_gray8(y, 255, type, 31, 2.5)
        assert np.array_equal(got[rows], adaptive_ref(y, 255, type, 31, 2.5, rows=rows)), type
