"""GPU suite (-m gpu): the exact Euclidean distance transform, mi355_dist_gray8_dev / _batched.

Every comparison is bit-identity with the CPU reference tests/dist_ref.py (or a closed form): the squared distance and
the nearest-site index are integers with one right answer per input, and the float output is one correctly rounded
function of the integer; it is compared as bits.  There is no tolerance anywhere in this file.
"""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import dist_cases as dc  # noqa: E402
import guarded  # noqa: E402
from dist_ref import NONE, dist_ref  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("sq", "dist", "nearest")
DTYPES = (np.int32, np.float32, np.int32)
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(range(3), k)]


def _frames(m):
    m = np.ascontiguousarray(m, np.uint8)
    return m[None] if m.ndim == 2 else m


def _dev(ctx, masks, which=(0, 1, 2)):
    """[sq, dist, nearest] (None where not asked for) of (n, h, w) masks through the device-resident call; every output
    is prefilled with a non-zero pattern first"""
    ms = _frames(masks)
    n, h, w = ms.shape
    outs = [np.empty((n, h, w), dt) if i in which else None for i, dt in enumerate(DTYPES)]
    d_in = ctx.alloc(max(ms.nbytes, 8))
    ptrs = [ctx.alloc(a.nbytes) if a is not None else 0 for a in outs]
    try:
        ctx.h2d(d_in, ms)
        for p, a in zip(ptrs, outs):
            if a is not None:
                ctx.h2d(p, np.full(a.nbytes, 0xA5, np.uint8))
        ctx.dist_gray8_dev(d_in, ptrs[0], ptrs[1], ptrs[2], w, h, n)
        ctx.sync()
        for p, a in zip(ptrs, outs):
            if a is not None:
                ctx.d2h(a, p)
    finally:
        ctx.sync()
        for p in [d_in] + [p for p in ptrs if p]:
            ctx.free(p)
    return outs


def _same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name, g.shape, w.shape, g.dtype)
        gb, wb = g.view(np.uint32), w.view(np.uint32)
        if not np.array_equal(gb, wb):
            i = int(np.flatnonzero(gb.ravel() != wb.ravel())[0])
            raise AssertionError("%s: %s differ, the first at flat index %d: got %r, want %r (%d wrong)"
                                 % (tag, name, i, g.ravel()[i], w.ravel()[i], int((gb != wb).sum())))


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(names, masks (n, h, w), reference outputs) of every content at `shape`, computed once"""
    named = dc.frames_of(shape)
    ms = np.stack([f for _, f in named])
    want = dist_ref(ms)
    for a in (ms,) + want:
        a.setflags(write=False)
    return [name for name, _ in named], ms, want


def _pick(want, idx):
    return tuple(a[idx] for a in want)


@pytest.mark.parametrize("shape", dc.SHAPES, ids=["%dx%d" % s for s in dc.SHAPES])
def test_every_case_is_bit_identical_to_the_cpu_reference(ctx, shape):
    names, ms, want = _case(shape)
    for f, name in enumerate(names):
        _same(_dev(ctx, ms[f]), _pick(want, slice(f, f + 1)), "%s %dx%d" % ((name,) + shape))


def test_a_batch_equals_one_call_per_frame_and_frames_do_not_leak(ctx):
    names, ms, want = _case((250, 130))
    # a frame without a site between two ordinary ones; a frame whose last row is all sites in front of one whose first
    # row is: the two rows are neighbours in memory, not in any frame
    for pick in (("noise_0.01", "no_site", "blobs"), ("bottom_row", "top_row", "seventh_columns"),
                 ("top_row", "bottom_row", "site_middle")):
        idx = [names.index(p) for p in pick]
        got = _dev(ctx, ms[idx])
        _same(got, _pick(want, idx), "batch %s" % (pick,))
        for k, f in enumerate(idx):
            _same(_dev(ctx, ms[f]), tuple(a[k:k + 1] for a in got), "single %s" % names[f])
    got = _dev(ctx, ms[[names.index("noise_0.01"), names.index("no_site"), names.index("blobs")]])
    assert (got[0][1] == NONE).all() and np.isposinf(got[1][1]).all() and (got[2][1] == -1).all()
    got = _dev(ctx, ms[[names.index("bottom_row"), names.index("top_row")]])
    rows = np.arange(130, dtype=np.int32)[:, None]
    assert np.array_equal(got[0][0], np.broadcast_to((129 - rows) ** 2, (130, 250)))
    assert np.array_equal(got[0][1], np.broadcast_to(rows ** 2, (130, 250)))


def test_every_subset_of_the_outputs_gives_the_same_bytes(ctx):
    for shape, pick in (((250, 130), ("lattice", "noise_0.5", "no_site")), ((67, 48), ("two_columns", "site_top_right")),
                        ((1030, 3), ("seventh_columns", "left_column"))):
        names, ms, want = _case(shape)
        idx = [names.index(p) for p in pick]
        for which in SUBSETS:
            got = _dev(ctx, ms[idx], which)
            assert [g is not None for g in got] == [i in which for i in range(3)]
            _same(got, _pick(want, idx), "%dx%d outputs %s" % (shape + (which,)))


def _arena_blob(want):
    """The three outputs as one payload with 64-byte gaps between them: (bytes expected after the call, [(name, offset,
    nbytes)], gap mask)"""
    parts, at = [], 0
    for name, a in zip(NAMES, want):
        parts.append((name, at, a.nbytes))
        at += a.nbytes + 64
    total = at - 64
    blob = np.full(total, 0x3C, np.uint8)
    gap = np.ones(total, bool)
    for (name, o, nb), a in zip(parts, want):
        blob[o:o + nb] = np.ascontiguousarray(a).view(np.uint8).ravel()
        gap[o:o + nb] = False
    return blob, parts, gap


@pytest.mark.parametrize("shape", [(67, 48), (250, 130)], ids=["67x48", "250x130"])
def test_any_byte_alignment_in_a_guarded_arena(ctx, shape):
    """Input offsets 0 .. 15, output offsets 0, 4, 8 and 12, two frames per call, the three outputs in one arena with gaps
    between them: no byte outside any output is written, none inside is left unwritten."""
    w, h = shape
    names, ms, want_all = _case(shape)
    idx = [names.index("noise_0.01"), names.index("other_values")]
    pair, want = ms[idx], _pick(want_all, idx)
    blob, parts, gap = _arena_blob(want)
    at = {name: o for name, o, _ in parts}
    for off_in in range(16):
        for off_out in (0, 4, 8, 12):

            def call(d_in, d_out):
                ctx.dist_gray8_dev(d_in, d_out + at["sq"], d_out + at["dist"], d_out + at["nearest"], w, h, 2)

            tag = "dist %dx%d in+%d out+%d" % (w, h, off_in, off_out)
            got = guarded.run(ctx, call, pair, blob, off_in=off_in, off_out=off_out, tag=tag)
            for name, o, nb in parts:
                guarded.check(got[o:o + nb], blob[o:o + nb], tag=tag + " " + name)
            assert np.array_equal(got[gap], guarded.prefill_of(blob)[gap]), tag + ": a byte between outputs changed"


def test_two_1080p_frames_with_closed_form_answers(ctx):
    h, w = 1080, 1920
    y0, x0 = 700, 1234
    one = dc.no_site(h, w)
    one[y0, x0] = 0
    sq, dist, near = _dev(ctx, np.stack([one, dc.border_sites(h, w)]))
    want = np.stack([dc.corner_site_sq(h, w, y0, x0), dc.border_sq(h, w)])
    assert np.array_equal(sq, want)
    assert np.array_equal(dist.view(np.uint32), np.sqrt(want.astype(np.float32)).view(np.uint32))
    assert (near[0] == y0 * w + x0).all()
    # the border frame: the nearest site is a border pixel at the stated distance
    ny, nx = near[1] // w, near[1] % w
    yy, xx = np.mgrid[0:h, 0:w]
    assert ((ny == 0) | (ny == h - 1) | (nx == 0) | (nx == w - 1)).all()
    assert np.array_equal((ny - yy) ** 2 + (nx - xx) ** 2, want[1])
    # ties go to the smaller column first, then the smaller row: the centre of the upper-left quadrant's diagonal
    assert near[1][300, 300] == 300 * w + 0 and near[1][5, 5] == 5 * w and near[1][5, 1000] == 1000


@pytest.mark.parametrize("shape,site", [((16384, 2), (0, 0)), ((16384, 2), (1, 16383)), ((2, 16384), (0, 0)),
                                        ((2, 16384), (16383, 1))],
                         ids=["16384x2_first", "16384x2_last", "2x16384_first", "2x16384_last"])
def test_the_largest_side_with_a_single_corner_site(ctx, shape, site):
    """MI355_MAX_DIST_DIM on either side: squared distances up to 16383^2 + 1, where int32 -> float32 rounds"""
    w, h = shape
    y0, x0 = site
    m = dc.no_site(h, w)
    m[y0, x0] = 0
    sq, dist, near = _dev(ctx, m)
    want = dc.corner_site_sq(h, w, y0, x0)
    assert want.max() == 16383 ** 2 + 1 > 1 << 24
    assert np.array_equal(sq[0], want)
    assert np.array_equal(dist[0].view(np.uint32), np.sqrt(want.astype(np.float32)).view(np.uint32))
    assert (near[0] == y0 * w + x0).all()


def test_the_device_form_equals_the_batched_form(ctx):
    for shape in ((67, 48), (250, 130), (1, 300)):
        names, ms, want = _case(shape)
        _same(_dev(ctx, ms), want, "device %dx%d" % shape)
        dist, sq, near, prof = ctx.dist_gray8(ms, squared=True, nearest=True, profile=True)
        _same((sq, dist, near), want, "batched %dx%d" % shape)
        assert (sq.dtype, dist.dtype, near.dtype) == (np.int32, np.float32, np.int32)
        assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
        # the distances alone, one optional output at a time, and one frame
        only = ctx.dist_gray8(ms)
        assert isinstance(only, np.ndarray) and np.array_equal(only.view(np.uint32), want[1].view(np.uint32))
        d2, s2 = ctx.dist_gray8(ms, squared=True)
        _same((s2, d2, None), want, "batched squared %dx%d" % shape)
        d3, n3 = ctx.dist_gray8(ms, nearest=True)
        _same((None, d3, n3), want, "batched nearest %dx%d" % shape)
        f = names.index("blobs")
        d1, s1, n1 = ctx.dist_gray8(ms[f], squared=True, nearest=True)
        assert d1.shape == (shape[1], shape[0])
        _same((s1[None], d1[None], n1[None]), _pick(want, slice(f, f + 1)), "one frame %dx%d" % shape)


def test_two_calls_on_the_same_input_give_identical_bytes(ctx):
    m = np.stack([dc.noise(1080, 1920, 0.01, seed=5), dc.blobs(1080, 1920)])
    _same(_dev(ctx, m), _dev(ctx, m), "repeat")


def test_argument_checks(ctx, pkg):
    w, h = 64, 48
    px = w * h
    base = ctx.alloc(256 * 1024)
    try:
        d_in, d_sq, d_dist, d_near = base + 65536, base + 2 * 65536, base + 2 * 65536 + 16384, base + 2 * 65536 + 32768
        ctx.h2d(d_in, dc.noise(h, w, 0.01))
        good = dict(d_in=d_in, d_sq=d_sq, d_dist=d_dist, d_nearest=d_near, w=w, h=h, nframes=1)

        def bad(code=-1, **kw):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.dist_gray8_dev(**dict(good, **kw))
            assert e.value.code == code, kw

        ctx.dist_gray8_dev(**good)
        outs = ("d_sq", "d_dist", "d_nearest")
        for which in SUBSETS:                                                  # any output may be null ...
            ctx.dist_gray8_dev(**dict(good, **{name: 0 for i, name in enumerate(outs) if i not in which}))
        bad(d_sq=0, d_dist=0, d_nearest=None)                                  # ... not all three
        bad(d_in=0)
        for kw in (dict(w=0), dict(h=0), dict(nframes=0), dict(w=-1), dict(w=16385, h=1), dict(w=1, h=16385)):
            bad(**kw)
        for off in (1, 2, 3):
            for name in outs:
                bad(**{name: good[name] + off})
                bad(**dict({o: 0 for o in outs}, **{name: good[name] + off}))
        ctx.dist_gray8_dev(**dict(good, d_in=d_in + 3))                         # the mask takes any byte alignment
        ctx.dist_gray8_dev(**dict(good, d_in=d_in + 1, d_sq=0, d_nearest=0))
        # every output against the input, from either side, and against every other output; a null output overlaps nothing
        for name in outs:
            bad(**{name: d_in})
            bad(**{name: d_in + px - 4})
            bad(**{name: d_in - 4 * px + 4})
            ctx.dist_gray8_dev(**dict(good, **{name: d_in + px + (-px) % 4}))   # right behind the input
            ctx.dist_gray8_dev(**dict(good, **{name: d_in - 4 * px}))           # right in front of it
            for other in outs:
                if other != name:
                    bad(**{name: good[other]})
                    bad(**{name: good[other] + 4 * px - 4})
                    bad(**{name: good[other] - 4 * px + 4})
                    ctx.dist_gray8_dev(**dict(good, **{name: good[other], other: 0}))
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.dist_gray8(dc.noise(17, 31, 0.5), squared=True)
        assert e.value.code == -4
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


@pytest.mark.parametrize("shape", [(5, 3), (1, 1)], ids=["5x3", "1x1"])
def test_three_thousand_tiny_frames_in_one_call(ctx, shape):
    w, h = shape
    rng = np.random.default_rng(17)
    ms = (rng.random((3000, h, w)) < 0.7).astype(np.uint8) * 255    # a 1 x 1 frame is a site or has none
    ms[7] = 255
    ms[8] = 0
    want = dist_ref(ms)
    assert (want[0] == NONE).any() and (want[0] == 0).any()
    _same(_dev(ctx, ms), want, "3000 frames of %dx%d" % shape)


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import dist_cases as dc
from dist_ref import dist_ref
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n = 250, 130, 2
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    ms = [np.stack([dc.noise(h, w, 0.01, 11), dc.lattice(h, w)]), np.stack([dc.blobs(h, w, 21), dc.no_site(h, w)])]
    d_in = torch.from_numpy(ms[0]).to(dev)
    o_sq = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    o_dist = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    o_near = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    outs = (o_sq, o_dist, o_near)

    def chain():
        c.dist_gray8_dev(d_in.data_ptr(), o_sq.data_ptr(), o_dist.data_ptr(), o_near.data_ptr(), w, h, n)

    chain()                             # the first call of this size: sizes the pooled scratch
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()                         # the second: allocates nothing, waits for nothing
    for r in range(2):
        m = ms[1 - r]
        d_in.copy_(torch.from_numpy(m).to(dev))
        for o in outs:
            o.fill_(-7)
        g.replay()
        s.synchronize()
        want = dist_ref(m)
        for name, o, wnt in zip(("sq", "dist", "nearest"), outs, want):
            got = o.cpu().numpy()
            if not np.array_equal(got.view(np.uint32), wnt.view(np.uint32)): bad.append((r, name))
    del g
    c.close()
print(bad)
"""


def test_the_second_call_of_a_size_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled scratch, a distance call allocates nothing and synchronises nothing, so it
    is captured into a hipGraph and replayed on new content.  Own process: torch's HIP runtime has to initialise before
    the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
