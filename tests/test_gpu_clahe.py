"""GPU suite (-m gpu): CLAHE of single-channel frames, mi355_clahe_gray8_dev / _batched / mi355_clahe_luts_gray8_dev.

Every comparison is bit-identity with the CPU reference tests/clahe_ref.py, tables and frames alike: the table stage is
integer arithmetic with one fp32 product per bin, the apply stage single IEEE fp32 operations on host-supplied scales.
There is no tolerance anywhere in this file.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import clahe_cases as cc  # noqa: E402
import guarded  # noqa: E402
from clahe_ref import clahe_ref, luts_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _frames(y):
    y = np.ascontiguousarray(y, np.uint8)
    return y[None] if y.ndim == 2 else y


def _dev(ctx, y, clip, tx, ty):
    """(frames, tables) of (n, h, w) frames through the two device-resident calls"""
    ys = _frames(y)
    n, h, w = ys.shape
    out = np.empty_like(ys)
    luts = np.empty((n, ty, tx, 256), np.uint8)
    d_in, d_out, d_luts = ctx.alloc(ys.nbytes), ctx.alloc(ys.nbytes), ctx.alloc(luts.nbytes)
    try:
        ctx.h2d(d_in, ys)
        ctx.h2d(d_out, np.full_like(ys, 0xA5))
        ctx.h2d(d_luts, np.full_like(luts, 0x5A))
        ctx.clahe_luts_gray8_dev(d_in, d_luts, w, h, n, clip, tx, ty)
        ctx.clahe_gray8_dev(d_in, d_out, w, h, n, clip, tx, ty)
        ctx.sync()
        ctx.d2h(out, d_out)
        ctx.d2h(luts, d_luts)
    finally:
        ctx.sync()
        for p in (d_in, d_out, d_luts):
            ctx.free(p)
    return out, luts


@functools.lru_cache(maxsize=None)
def _case(i):
    """(frames (3, h, w), reference tables, reference frames) of case i, computed once"""
    case = cc.CASES[i]
    ys = np.stack([f for _, f in cc.frames_of(case)])
    _, _, tx, ty, clip = case
    want_luts, want = luts_ref(ys, clip, tx, ty), clahe_ref(ys, clip, tx, ty)
    for a in (ys, want_luts, want):
        a.setflags(write=False)
    return ys, want_luts, want


@pytest.mark.parametrize("i", range(len(cc.CASES)), ids=["%dx%d_%dx%d_%g" % c for c in cc.CASES])
def test_tables_and_frames_are_bit_identical_to_the_cpu_reference(ctx, i):
    _, _, tx, ty, clip = cc.CASES[i]
    ys, want_luts, want = _case(i)
    for f, (name, _) in enumerate(cc.frames_of(cc.CASES[i])):
        got, luts = _dev(ctx, ys[f], clip, tx, ty)
        assert np.array_equal(luts[0], want_luts[f]), (cc.CASES[i], name, "tables")
        assert np.array_equal(got[0], want[f]), (cc.CASES[i], name, "frame")


def test_a_constant_frame_is_not_mapped_to_itself(ctx):
    y = np.full((48, 64), 7, np.uint8)
    assert np.array_equal(ctx.clahe_gray8(y, 2.0, 8, 8), np.full_like(y, 16))
    assert np.array_equal(ctx.clahe_gray8(y, 0.0, 8, 8), np.full_like(y, 255))


@pytest.mark.parametrize("i", [3, 5, 10])
def test_a_batch_equals_one_call_per_frame(ctx, i):
    _, _, tx, ty, clip = cc.CASES[i]
    ys, want_luts, want = _case(i)
    got, luts = _dev(ctx, ys, clip, tx, ty)
    assert np.array_equal(luts, want_luts) and np.array_equal(got, want)
    for f in range(3):
        one, one_luts = _dev(ctx, ys[f], clip, tx, ty)
        assert np.array_equal(one[0], got[f]) and np.array_equal(one_luts[0], luts[f]), f


@pytest.mark.parametrize("i", [3, 10], ids=["67x48", "250x130"])
def test_any_byte_alignment_in_a_guarded_arena(ctx, i):
    """Every input and every output offset 0 .. 15, two frames (250 x 130 is no multiple of 16: the second frame starts
    at yet another alignment): no byte outside the output is written, none inside is left unwritten."""
    w, h, tx, ty, clip = cc.CASES[i]
    assert (w, h) in ((67, 48), (250, 130))
    ys, want_luts, want = _case(i)
    ys, want = ys[:2], want[:2]
    for off_in in range(16):
        for off_out in range(16):
            got = guarded.run(ctx, lambda d_in, d_out: ctx.clahe_gray8_dev(d_in, d_out, w, h, 2, clip, tx, ty), ys, want,
                              off_in=off_in, off_out=off_out, tag="clahe %dx%d" % (w, h))
            guarded.check(got, want, tag="clahe %dx%d in+%d out+%d" % (w, h, off_in, off_out))
    for off_in in range(16):
        for off_out in (0, 4, 8, 12):
            got = guarded.run(ctx, lambda d_in, d_out: ctx.clahe_luts_gray8_dev(d_in, d_out, w, h, 2, clip, tx, ty), ys,
                              want_luts[:2], off_in=off_in, off_out=off_out, tag="clahe tables %dx%d" % (w, h))
            guarded.check(got, want_luts[:2], tag="clahe tables %dx%d in+%d out+%d" % (w, h, off_in, off_out))


def _hd_frame(h, w, seed):
    """noise over flat 64 x 64 patches over a gradient: every tile has its own histogram, some far above the clip"""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    base = ((xx * 255) // w + (yy * 64) // h) & 0xFF
    flat = rng.integers(0, 256, ((h + 63) // 64, (w + 63) // 64))[yy // 64, xx // 64]
    img = np.where(((xx // 64 + yy // 64) % 3) == 0, flat, base + rng.integers(0, 24, (h, w)))
    return (img & 0xFF).astype(np.uint8)


@pytest.mark.parametrize("shape,clip", [((1080, 1920), 2.0), ((2160, 3840), 40.0)], ids=["1080p", "4k"])
def test_full_size_frames(ctx, shape, clip):
    y = _hd_frame(shape[0], shape[1], shape[0])
    got, luts = _dev(ctx, y, clip, 8, 8)
    assert np.array_equal(luts[0], luts_ref(y, clip, 8, 8))
    assert np.array_equal(got[0], clahe_ref(y, clip, 8, 8))


@pytest.mark.parametrize("w,h,tx,ty", [(40000, 3, 16, 1), (3, 40000, 1, 16), (40003, 5, 7, 2), (40000, 3, 1, 1)],
                         ids=["wide", "tall", "wide_padded", "wide_one_tile"])
def test_rows_longer_than_a_block_and_tiles_of_many_bands(ctx, w, h, tx, ty):
    """Rows of more bytes than an apply block takes (one row per block), and a tile row of more bytes than a histogram
    band (one tile row per block, three bands)."""
    y = cc.low_contrast(h, w, 9)
    y[:, ::3] = cc.uniform_noise(h, w, 10)[:, ::3]
    got, luts = _dev(ctx, y, 3.0, tx, ty)
    assert np.array_equal(luts[0], luts_ref(y, 3.0, tx, ty))
    assert np.array_equal(got[0], clahe_ref(y, 3.0, tx, ty))


def test_the_device_form_equals_the_batched_form(ctx):
    for i in (0, 3, 4, 10):
        _, _, tx, ty, clip = cc.CASES[i]
        ys, _, want = _case(i)
        got, _ = _dev(ctx, ys, clip, tx, ty)
        host, prof = ctx.clahe_gray8(ys, clip, tx, ty, profile=True)
        assert np.array_equal(host, got) and np.array_equal(host, want), cc.CASES[i]
        assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
        assert np.array_equal(ctx.clahe_gray8(ys[1], clip, tx, ty), want[1])


def test_argument_checks(ctx, pkg):
    w, h = 64, 48
    base = ctx.alloc(64 * 1024)
    try:
        d_in, d_out, d_luts = base, base + 8192, base + 16384
        ctx.h2d(d_in, cc.uniform_noise(h, w, 1))
        calls = ((ctx.clahe_gray8_dev, d_out, w * h), (ctx.clahe_luts_gray8_dev, d_luts, 64 * 256))
        for fn, d_o, nout in calls:
            fn(d_in, d_o, w, h, 1, 2.0, 8, 8)
            for bad_in, bad_out in ((0, d_o), (d_in, 0)):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(bad_in, bad_out, w, h, 1, 2.0, 8, 8)
                assert e.value.code == -1, fn.__name__
            # in place, and overlapping from either side
            for d_bad in (d_in, d_in + w * h - 4, d_in - nout + 4):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_in, d_bad, w, h, 1, 2.0, 8, 8)
                assert e.value.code == -1, (fn.__name__, d_bad - d_in)
            for bad in ((w, h, 1, 2.0, 0, 8), (w, h, 1, 2.0, 8, 17), (w, h, 1, float("nan"), 8, 8),
                        (w, h, 1, float("inf"), 8, 8), (0, h, 1, 2.0, 8, 8), (w, h, 0, 2.0, 8, 8),
                        (65536, 32768, 1, 2.0, 8, 8)):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_in, d_o, *bad)
                assert e.value.code == -1, (fn.__name__, bad)
            with pytest.raises(pkg.Mi355Error) as e:
                fn(d_in, d_o, 31, 16, 1, 2.0, 16, 16)
            assert e.value.code == -4, fn.__name__
        for off in (1, 2, 3):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.clahe_luts_gray8_dev(d_in, d_luts + off, w, h, 1, 2.0, 8, 8)
            assert e.value.code == -1, off
        ctx.clahe_gray8_dev(d_in, d_out + 3, w, h, 1, 2.0, 8, 8)  # frames take any byte alignment
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.clahe_gray8(cc.uniform_noise(17, 31, 3), 2.0, 4, 4)
        assert e.value.code == -4
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import clahe_cases as cc
from clahe_ref import clahe_ref, luts_ref
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n, clip, tx, ty = 250, 130, 2, 4.0, 8, 8
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    ys = [np.stack([cc.uniform_noise(h, w, 11), cc.low_contrast(h, w, 12)]),
          np.stack([cc.wrapped_gradient(h, w, 21), cc.uniform_noise(h, w, 22) >> 3])]
    d_in = torch.from_numpy(ys[0]).to(dev)
    o_luts = torch.zeros((n, ty, tx, 256), dtype=torch.uint8, device=dev)
    o_out = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)

    def chain():
        c.clahe_luts_gray8_dev(d_in.data_ptr(), o_luts.data_ptr(), w, h, n, clip, tx, ty)
        c.clahe_gray8_dev(d_in.data_ptr(), o_out.data_ptr(), w, h, n, clip, tx, ty)

    chain()                             # the first call of this size: sizes the pooled scratch
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()                         # the second: allocates nothing, waits for nothing
    for r in range(2):
        y = ys[1 - r]
        d_in.copy_(torch.from_numpy(y).to(dev))
        o_luts.zero_()
        o_out.zero_()
        g.replay()
        s.synchronize()
        if not np.array_equal(o_luts.cpu().numpy(), luts_ref(y, clip, tx, ty)): bad.append((r, "tables"))
        if not np.array_equal(o_out.cpu().numpy(), clahe_ref(y, clip, tx, ty)): bad.append((r, "frames"))
    del g
    c.close()
print(bad)
"""


def test_the_second_call_of_a_size_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled histograms and tables, a CLAHE call allocates nothing and synchronises
    nothing (the zeroing is an in-stream memset), so it is captured into a hipGraph and replayed on new content.  Own
    process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
