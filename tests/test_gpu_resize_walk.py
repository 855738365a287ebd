"""GPU suite (-m gpu): the parts of mi355_resize_dev / mi355_resize_batched that one small frame never reaches.

  * the band walk: batches sized (tests/resize_cases.py) so that the launch plan gives a wave 2, 4, 8 and 16 output rows;
    LINEAR's row cache, the ragged last band and multi-row stores into a guarded arena only run there;
  * the scale contract: every size pair of 1..64 x 1..64 on index frames, where a wrong source index is a wrong byte,
    and LINEAR on the larger pairs on which an fp32 coordinate shows;
  * AREA at all 256 factor pairs, on blocks whose sums are the ones the fp32 product rounds differently from the exact
    quotient, and on all-255 blocks beside all-0 blocks (the packed u16 sums of RGBA);
  * a captured graph of two device-resident resize calls.

Every comparison is bit-identity against tests/resize_ref.py.  test_resize_walk_cpu.py shows, without a GPU, that these
inputs reach what they claim and that a wrong scale, an fp32 coordinate or an exact-quotient AREA would change them.
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import guarded  # noqa: E402
import resize_cases as rc  # noqa: E402
from resize_ref import AREA, LINEAR, NEAREST, resize_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INTERPS = (NEAREST, LINEAR, AREA)
BPP_NAME = {4: "rgba", 1: "gray8"}
WALK = [(bpp, i, r) for bpp in (4, 1) for i in INTERPS for r in rc.BAND_HEIGHTS]
WALK_IDS = ["%s-%s-%drows" % (BPP_NAME[b], rc.NAMES[i], r) for b, i, r in WALK]
BPP_INTERP = [(bpp, i) for bpp in (4, 1) for i in INTERPS]
BPP_INTERP_IDS = ["%s-%s" % (BPP_NAME[b], rc.NAMES[i]) for b, i in BPP_INTERP]


@functools.lru_cache(maxsize=None)
def _case(shape, bpp, interp):
    """(the 7 distinct frames, their references): computed once per (shape, bpp, interp), read-only afterwards."""
    sw, sh, dw, dh = shape
    frames = rc.distinct_frames(sw, sh, bpp)
    refs = np.stack([resize_ref(f, dw, dh, interp) for f in frames])
    frames.setflags(write=False)
    refs.setflags(write=False)
    return frames, refs


def _out_shape(n, dw, dh, bpp):
    return (n, dh, dw, 4) if bpp == 4 else (n, dh, dw)


def _resize_dev(ctx, bpp, batch, dw, dh, interp):
    """One mi355_resize_dev call on a whole batch through plain device buffers."""
    n, sh, sw = batch.shape[:3]
    out = np.empty(_out_shape(n, dw, dh, bpp), np.uint8)
    d_in = ctx.alloc(batch.nbytes)
    try:
        d_out = ctx.alloc(out.nbytes)
        try:
            ctx.h2d(d_in, batch)
            ctx.resize_dev(d_in, d_out, bpp, sw, sh, dw, dh, n, interp)
            ctx.sync()
            ctx.d2h(out, d_out)
        finally:
            ctx.sync()
            ctx.free(d_out)
    finally:
        ctx.free(d_in)
    return out


def _assert_batch(got, refs, tag):
    """Every frame of `got` equals the reference of its source frame; the first wrong pixel is named."""
    want_index = np.arange(got.shape[0]) % len(refs)
    assert got.shape[1:] == refs.shape[1:], (tag, got.shape, refs.shape)
    bad = got != refs[want_index]
    if bad.any():
        f, y, x = [int(v) for v in np.argwhere(bad.reshape(bad.shape[:3] + (-1,)).any(-1))[0]]
        raise AssertionError("%s: %d byte(s) wrong, the first in frame %d (content %d) row %d column %d: got %s, want %s"
                             % (tag, int(bad.sum()), f, f % len(refs), y, x, got[f, y, x], refs[f % len(refs)][y, x]))


def _tag(shape, bpp, interp, rows):
    return "%dx%d->%dx%d %s %s %d rows per band" % (shape + (BPP_NAME[bpp], rc.NAMES[interp], rows))


# ---- the band walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp,interp,rows", WALK, ids=WALK_IDS)
def test_band_walk_is_bit_identical_on_every_frame(ctx, bpp, interp, rows):
    """A batch of 7 distinct frames repeated to the frame count at which a wave walks `rows` output rows."""
    for shape in rc.walk_cases(interp):
        sw, sh, dw, dh = shape
        n = rc.frames_for(dw, dh, rows)
        frames, refs = _case(shape, bpp, interp)
        got = _resize_dev(ctx, bpp, rc.cycled(frames, n), dw, dh, interp)
        _assert_batch(got, refs, _tag(shape, bpp, interp, rows))


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_band_walk_in_the_guarded_arena(ctx, bpp, interp):
    """Bands of 16 and of 2 rows store every payload byte and nothing outside it, at two pointer alignments."""
    offsets = ((0, 0), (4, 12)) if bpp == 4 else ((1, 3), (3, 5))
    for rows, shape in rc.GUARDED_WALK[interp]:
        sw, sh, dw, dh = shape
        n = rc.frames_for(dw, dh, rows)
        frames, refs = _case(shape, bpp, interp)
        batch, expected = rc.cycled(frames, n), rc.cycled(refs, n)
        for off_in, off_out in offsets:
            tag = _tag(shape, bpp, interp, rows)
            got = guarded.run(ctx, lambda a, b: ctx.resize_dev(a, b, bpp, sw, sh, dw, dh, n, interp), batch, expected,
                              off_in=off_in, off_out=off_out, tag=tag)
            guarded.check(got, expected, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
            _assert_batch(got, refs, tag)


@pytest.mark.parametrize("interp", INTERPS, ids=[rc.NAMES[i] for i in INTERPS])
def test_host_call_walks_16_row_bands(ctx, interp):
    """mi355_resize_batched with a batch large enough for 16-row bands, RGBA and gray8."""
    shape = (99, 76, 33, 19) if interp == AREA else (100, 66, 77, 50)
    sw, sh, dw, dh = shape
    n = rc.frames_for(dw, dh, 16)
    for bpp in (4, 1):
        frames, refs = _case(shape, bpp, interp)
        batch = rc.cycled(frames, n)
        got = ctx.resize(batch, dw, dh, interp) if bpp == 4 else ctx.resize_gray8(batch, dw, dh, interp)
        _assert_batch(got, refs, "host call " + _tag(shape, bpp, interp, 16))


# ---- the size-pair sweep ----------------------------------------------------------------------------------------------
def _sweep(ctx, bpp, interp, pairs):
    frames = {}
    gpu_s = 0.0
    for s, d in pairs:
        if s not in frames:
            frames[s] = rc.sweep_frames(s, bpp)
        t0 = time.perf_counter()
        got = ctx.resize(frames[s], d, d, interp) if bpp == 4 else ctx.resize_gray8(frames[s], d, d, interp)
        gpu_s += time.perf_counter() - t0
        want = np.stack([resize_ref(f, d, d, interp) for f in frames[s]])
        if not np.array_equal(got, want):
            f, y, x = [int(v) for v in np.argwhere((got != want).reshape(3, d, d, -1).any(-1))[0]]
            raise AssertionError("%d -> %d %s %s: frame %d (%s) row %d column %d: got %s, want %s"
                                 % (s, d, BPP_NAME[bpp], rc.NAMES[interp], f, ("column index", "row index", "noise")[f],
                                    y, x, got[f, y, x], want[f, y, x]))
    print("sweep %s %s: %d calls, %.2f s in the library" % (BPP_NAME[bpp], rc.NAMES[interp], len(pairs), gpu_s))


@pytest.mark.parametrize("interp", (NEAREST, LINEAR), ids=("nearest", "linear"))
def test_every_size_pair_up_to_64_on_index_frames(ctx, interp):
    """gray8, s x s -> d x d for all 4096 pairs: frame 0 holds the column index, frame 1 the row index, frame 2 noise.
    NEAREST shows the chosen source column and row directly; for 98 of the pairs scale = src / dst picks another one.
    LINEAR also runs the 114 pairs with a size in 65..96 on which an all-fp32 coordinate changes these frames' bytes
    (inside 1..64 it cannot change any)."""
    pairs = rc.SWEEP_PAIRS + (rc.fp32_decisive_pairs() if interp == LINEAR else [])
    _sweep(ctx, 1, interp, pairs)


@pytest.mark.parametrize("interp", (NEAREST, LINEAR), ids=("nearest", "linear"))
def test_decisive_size_pairs_rgba(ctx, interp):
    """RGBA on the pairs where the plain quotient changes a NEAREST byte, the diagonal, and exactly double and half."""
    _sweep(ctx, 4, interp, rc.rgba_sweep_pairs())


# ---- every AREA factor pair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpp", (4, 1), ids=("rgba", "gray8"))
def test_area_at_every_factor_pair(ctx, bpp):
    """All 16 x 16 factor pairs on blocks that hold chosen sums: both ends, every sum on which rint(sum * (1.f / (n m)))
    is not the exactly rounded quotient (4160 over 50 pairs) with its neighbours, every exact tie, 64 seeded sums.
    301 output columns: one full strip (16-byte loads at factors 2 and 4) and a ragged one; gray8 at factor 2 has every
    other source row off a dword boundary.  RGBA starts with an all-255 block beside an all-0 one: at 16 x 16 each
    packed u16 sum is 65280, and a carry into the neighbouring half or pixel would show."""
    for n, m in rc.AREA_FACTORS:
        frame, sums = rc.area_frame(n, m, bpp)
        dh = sums.shape[0]
        got = ctx.resize(frame, rc.AREA_DW, dh, AREA) if bpp == 4 else ctx.resize_gray8(frame, rc.AREA_DW, dh, AREA)
        want = resize_ref(frame, rc.AREA_DW, dh, AREA)
        if not np.array_equal(got, want):
            y, x = [int(v) for v in np.argwhere((got != want).reshape(dh, rc.AREA_DW, -1).any(-1))[0]]
            raise AssertionError("AREA %d x %d %s: row %d column %d: block sum %s, got %s, want %s"
                                 % (n, m, BPP_NAME[bpp], y, x, sums[y, x], got[y, x], want[y, x]))


def test_area_wide_loads_fall_back_on_unaligned_gray8_rows(ctx):
    """x-factors 2 and 4 with the gray8 input 1 and 2 bytes off a dword boundary: the per-pixel path instead of the wide
    loads, in the guarded arena."""
    for n in (2, 4):
        for m in range(1, 17):
            frame, sums = rc.area_frame(n, m, 1)
            sh, sw = frame.shape
            dh = sums.shape[0]
            want = resize_ref(frame, rc.AREA_DW, dh, AREA)
            for off_in in (1, 2):
                tag = "AREA %d x %d gray8" % (n, m)
                got = guarded.run(ctx, lambda a, b: ctx.resize_dev(a, b, 1, sw, sh, rc.AREA_DW, dh, 1, AREA), frame, want,
                                  off_in=off_in, off_out=0, tag=tag)
                guarded.check(got, want, tag="%s off_in=%d" % (tag, off_in))


# ---- hipGraph ---------------------------------------------------------------------------------------------------------
_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import resize_cases as rc
from resize_ref import LINEAR, NEAREST, resize_ref
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
sw, sh, mw, mh, dw, dh = 77, 41, 33, 19, 64, 48
n = max(rc.frames_for(mw, mh, 16), rc.frames_for(dw, dh, 16))
assert rc.band_rows(mw, mh, n) == 16 and rc.band_rows(dw, dh, n) == 16
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    distinct = rc.distinct_frames(sw, sh, 4)
    want = np.stack([resize_ref(resize_ref(f, mw, mh, LINEAR), dw, dh, NEAREST) for f in distinct])
    # replay 0 runs the batch shifted by 3 frames, replay 1 by 5: neither is what the warm-up and the capture saw
    batches = [rc.cycled(np.roll(distinct, -k, 0), n) for k in (0, 3, 5)]
    d_in = torch.from_numpy(batches[0]).to(dev)
    d_mid = torch.zeros((n, mh, mw, 4), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((n, dh, dw, 4), dtype=torch.uint8, device=dev)

    def chain():
        c.resize_dev(d_in.data_ptr(), d_mid.data_ptr(), 4, sw, sh, mw, mh, n, LINEAR)
        c.resize_dev(d_mid.data_ptr(), d_out.data_ptr(), 4, mw, mh, dw, dh, n, NEAREST)

    chain()                             # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for i, k in ((1, 3), (2, 5)):
        d_in.copy_(torch.from_numpy(batches[i]).to(dev))
        d_mid.zero_()
        d_out.zero_()
        g.replay()
        s.synchronize()
        got = d_out.cpu().numpy()
        if not np.array_equal(got, np.roll(want, -k, 0)[np.arange(n) % len(want)]): bad.append((i, k))
    del g
    c.close()
print(bad)
"""


def test_device_resident_resize_can_be_captured_into_a_hip_graph():
    """mi355_resize_dev allocates nothing and synchronises nothing, so a linear chain of two calls on one stream (a
    LINEAR downscale of a batch large enough for 16-row bands, then a NEAREST upscale of its result) is captured into a
    hipGraph after a warm-up call and replayed twice on new content.  Capturing without the warm-up call is not tested."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
