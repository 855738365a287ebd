"""GPU suite (-m gpu): connected-component labelling, mi355_ccl_gray8_dev / _batched.

Every comparison is bit-identity with the CPU reference tests/ccl_ref.py (or a closed form): labels, counts, statistics
and coordinate sums are integers with one right answer per input.  There is no tolerance anywhere in this file.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import ccl_cases as cc  # noqa: E402
import guarded  # noqa: E402
from ccl_ref import centroids_of, ccl_ref, stats_of  # noqa: E402

pytestmark = pytest.mark.gpu


def _frames(m):
    m = np.ascontiguousarray(m, np.uint8)
    return m[None] if m.ndim == 2 else m


def _dev(ctx, masks, conn, rows, null_stats=False):
    """(labels, count, stats, sums) of (n, h, w) masks through the device-resident call; every output is prefilled with
    a non-zero pattern first.  null_stats: pass null pointers for the two optional outputs (rows must be 0)."""
    ms = _frames(masks)
    n, h, w = ms.shape
    labels = np.empty((n, h, w), np.int32)
    count = np.empty(n, np.int32)
    stats = np.empty((n, rows, 5), np.int32)
    sums = np.empty((n, rows, 2), np.uint64)
    outs = (labels, count, stats, sums)
    ptrs = [ctx.alloc(max(a.nbytes, 8)) for a in (ms,) + outs]
    try:
        ctx.h2d(ptrs[0], ms)
        for p, a in zip(ptrs[1:], outs):
            if a.nbytes:
                ctx.h2d(p, np.full(a.nbytes, 0xA5, np.uint8))
        ctx.ccl_gray8_dev(ptrs[0], ptrs[1], ptrs[2], None if null_stats else ptrs[3], None if null_stats else ptrs[4],
                          w, h, n, conn, rows)
        ctx.sync()
        for p, a in zip(ptrs[1:], outs):
            if a.nbytes:
                ctx.d2h(a, p)
    finally:
        ctx.sync()
        for p in ptrs:
            ctx.free(p)
    return outs


def _same(got, want, tag):
    for name, g, w in zip(("labels", "count", "stats", "sums"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g.ravel() != w.ravel())[0])
            raise AssertionError("%s: %s differ, the first at flat index %d: got %d, want %d (%d wrong)"
                                 % (tag, name, i, g.ravel()[i], w.ravel()[i], int((g != w).sum())))


@functools.lru_cache(maxsize=None)
def _case(shape, conn):
    """(names, masks (n, h, w), reference outputs at cc.STATS_ROWS rows) of every content at `shape`, computed once"""
    named = cc.frames_of(shape)
    ms = np.stack([f for _, f in named])
    want = ccl_ref(ms, conn, cc.STATS_ROWS)
    for a in (ms,) + want:
        a.setflags(write=False)
    return [name for name, _ in named], ms, want


def _one(want, f):
    return tuple(a[f:f + 1] for a in want)


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=["%dx%d" % s for s in cc.SHAPES])
def test_every_case_is_bit_identical_to_the_cpu_reference(ctx, shape, conn):
    names, ms, want = _case(shape, conn)
    for f, name in enumerate(names):
        _same(_dev(ctx, ms[f], conn, cc.STATS_ROWS), _one(want, f), "%s %dx%d conn %d" % ((name,) + shape + (conn,)))


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
def test_a_batch_equals_one_call_per_frame_and_frames_and_rows_do_not_leak(ctx, conn):
    names, ms, want = _case((250, 130), conn)
    # last_row then first_row: the two rows are neighbours in memory, not in any frame; row_ends: (w - 1, y) and
    # (0, y + 1) likewise
    for pick in (("noise_0.59", "spiral", "other_values"), ("last_row", "first_row", "row_ends")):
        idx = [names.index(p) for p in pick]
        got = _dev(ctx, ms[idx], conn, cc.STATS_ROWS)
        _same(got, tuple(a[idx] for a in want), "batch %s conn %d" % (pick, conn))
        for k, f in enumerate(idx):
            _same(_dev(ctx, ms[f], conn, cc.STATS_ROWS), _one(got, k), "single %s conn %d" % (names[f], conn))
    f = names.index("last_row")
    pair = np.stack([ms[f], ms[names.index("first_row")]])
    got = _dev(ctx, pair, conn, 4)
    assert got[1].tolist() == [2, 2] and got[0][0, -1].tolist() == [1] * 250 and got[0][1, 0].tolist() == [1] * 250
    assert got[2][0, 1].tolist() == [0, 129, 250, 1, 250] and got[2][1, 1].tolist() == [0, 0, 250, 1, 250]


def test_statistics_rows_below_at_and_above_the_label_count(ctx):
    names, ms, _ = _case((250, 130), 4)
    m = ms[names.index("noise_0.3")]
    full = ccl_ref(m, 4, 4137 + 50)
    n = int(full[1][0])
    assert n == 4137
    for rows in (0, 1, n, n - 1, 1000, n + 50):
        got = _dev(ctx, m, 4, rows)
        _same(got, ccl_ref(m, 4, rows), "rows %d" % rows)
        assert np.array_equal(got[0], full[0]) and got[1][0] == n           # labels and count are unaffected
        assert np.array_equal(got[2][0], full[2][0][:rows]) and np.array_equal(got[3][0], full[3][0][:rows])
    assert not full[2][0][n:].any() and not full[3][0][n:].any()            # rows past N are zero
    got = _dev(ctx, m, 4, 0, null_stats=True)
    assert np.array_equal(got[0], full[0]) and got[1][0] == n


def _arena_blob(want, off_out):
    """The four outputs as one payload with 64-byte gaps between them (labels at its start, the sums on an 8-byte
    boundary of the device address): (bytes expected after the call, [(name, offset, nbytes)], gap mask)"""
    parts, at = [], 0
    for name, a in zip(("labels", "count", "stats", "sums"), want):
        if name == "sums":
            at += (-(off_out + at)) % 8
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
    """Input offsets 0 .. 15, label offsets 0, 4, 8 and 12, two frames per call, the four outputs in one arena with gaps
    between them: no byte outside any output is written, none inside is left unwritten."""
    w, h = shape
    rows = 40
    names, ms, _ = _case(shape, 8)
    pair = ms[[names.index("noise_0.41"), names.index("other_values")]]
    for conn in cc.CONNECTIVITIES:
        want = ccl_ref(pair, conn, rows)
        for off_in in range(16):
            for off_out in (0, 4, 8, 12):
                blob, parts, gap = _arena_blob(want, off_out)
                at = {name: o for name, o, _ in parts}

                def call(d_in, d_out):
                    ctx.ccl_gray8_dev(d_in, d_out + at["labels"], d_out + at["count"], d_out + at["stats"],
                                      d_out + at["sums"], w, h, 2, conn, rows)

                tag = "ccl %dx%d conn %d in+%d out+%d" % (w, h, conn, off_in, off_out)
                got = guarded.run(ctx, call, pair, blob, off_in=off_in, off_out=off_out, tag=tag)
                for name, o, nb in parts:
                    guarded.check(got[o:o + nb], blob[o:o + nb], tag=tag + " " + name)
                assert np.array_equal(got[gap], guarded.prefill_of(blob)[gap]), tag + ": a byte between outputs changed"


@functools.lru_cache(maxsize=None)
def _hd_closed_forms():
    h, w = 1080, 1920
    sp = cc.spiral(h, w)
    grid, grid_labels = cc.grid_of_rectangles(h, w)
    return sp, (sp != 0).astype(np.int32), grid, grid_labels


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
def test_two_1080p_frames_with_closed_form_answers(ctx, conn):
    sp, sp_labels, grid, grid_labels = _hd_closed_forms()
    rows = 600
    labels, count, stats, sums = _dev(ctx, np.stack([sp, grid]), conn, rows)
    assert count.tolist() == [2, 30 * 17 + 1]
    assert np.array_equal(labels[0], sp_labels) and np.array_equal(labels[1], grid_labels)
    # the spiral: one component over the whole frame
    area = int(sp_labels.sum())
    ys, xs = np.nonzero(sp_labels)
    assert stats[0, 1].tolist() == [0, 0, 1920, 1080, area]
    assert sums[0, 1].tolist() == [int(xs.sum()), int(ys.sum())]
    assert stats[0, 0, 4] == 1920 * 1080 - area and not stats[0, 2:].any() and not sums[0, 2:].any()
    # the rectangles: label i is cell i - 1, the box is the rectangle, the sums are those of a rectangle
    for i in (1, 2, 30, 31, 255, 510):
        cy, cx = divmod(i - 1, 30)
        rw, rh = 5 + (cx * 7 + cy * 3) % 40, 4 + (cx * 5 + cy * 11) % 30
        x0, y0 = cx * 64 + 3, cy * 64 + 2
        rh = min(rh, 1080 - y0)
        assert stats[1, i].tolist() == [x0, y0, rw, rh, rw * rh], i
        assert sums[1, i].tolist() == [rh * (rw * x0 + rw * (rw - 1) // 2), rw * (rh * y0 + rh * (rh - 1) // 2)], i
    want_stats, want_sums = stats_of(grid_labels, 511, rows)
    assert np.array_equal(stats[1], want_stats) and np.array_equal(sums[1], want_sums)


def test_a_1080p_noise_frame_at_the_percolation_threshold(ctx):
    m = cc.noise(1080, 1920, 0.59, seed=3)
    _same(_dev(ctx, m, 4, 1000), ccl_ref(m, 4, 1000), "1080p noise 0.59 conn 4")


def test_the_device_form_equals_the_batched_form(ctx):
    for shape, conn in (((67, 48), 4), ((250, 130), 8), ((1, 300), 8)):
        names, ms, want = _case(shape, conn)
        got = _dev(ctx, ms, conn, cc.STATS_ROWS)
        _same(got, want, "device %dx%d" % shape)
        labels, count, stats, centroids, prof = ctx.ccl_gray8(ms, conn, cc.STATS_ROWS, profile=True)
        assert np.array_equal(labels, got[0]) and np.array_equal(count, got[1]) and np.array_equal(stats, got[2])
        assert np.array_equal(centroids, centroids_of(got[2], got[3]), equal_nan=True)
        assert labels.dtype == np.int32 and centroids.dtype == np.float64
        assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
        # one frame, and no statistics
        f = names.index("noise_0.41")
        one = ctx.ccl_gray8(ms[f], conn, cc.STATS_ROWS)
        assert np.array_equal(one[0], want[0][f]) and one[1] == want[1][f] and np.array_equal(one[2], want[2][f])
        labels2, count2 = ctx.ccl_gray8(ms, conn)
        assert np.array_equal(labels2, want[0]) and np.array_equal(count2, want[1])


def test_two_calls_on_the_same_input_give_identical_bytes(ctx):
    m = cc.noise(1080, 1920, 0.59, seed=5)
    a, b = _dev(ctx, m, 8, 2000), _dev(ctx, m, 8, 2000)
    _same(a, b, "repeat")


def test_argument_checks(ctx, pkg):
    w, h, rows = 64, 48, 8
    base = ctx.alloc(256 * 1024)
    try:
        d_in, d_lab, d_cnt, d_st, d_sm = base, base + 16384, base + 65536, base + 65536 + 256, base + 65536 + 1024
        ctx.h2d(d_in, cc.noise(h, w, 0.41))
        good = dict(d_in=d_in, d_labels=d_lab, d_count=d_cnt, d_stats=d_st, d_sums=d_sm, w=w, h=h, nframes=1,
                    connectivity=8, stats_rows=rows)

        def bad(code=-1, **kw):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.ccl_gray8_dev(**dict(good, **kw))
            assert e.value.code == code, kw

        ctx.ccl_gray8_dev(**good)
        ctx.ccl_gray8_dev(**dict(good, d_stats=0, d_sums=0, stats_rows=0))   # the optional pair may be null
        for name in ("d_in", "d_labels", "d_count", "d_stats", "d_sums"):
            bad(**{name: 0})
        for kw in (dict(connectivity=0), dict(connectivity=6), dict(stats_rows=-1), dict(stats_rows=(1 << 24) + 1),
                   dict(w=0), dict(h=0), dict(nframes=0), dict(w=65536, h=32768)):
            bad(**kw)
        for off in (1, 2, 3):
            for name in ("d_labels", "d_count", "d_stats"):
                bad(**{name: good[name] + off})
        for off in (1, 2, 4, 7):
            bad(d_sums=d_sm + off)
        ctx.ccl_gray8_dev(**dict(good, d_in=d_in + 3))                       # the mask takes any byte alignment
        # every output against the input, from either side, and against every other output
        nbytes = dict(d_labels=4 * w * h, d_count=4, d_stats=20 * rows, d_sums=16 * rows)
        for name, nb in nbytes.items():
            bad(**{name: d_in})
            bad(**{name: d_in + w * h - 8})
            bad(**{name: d_in - nb + 8})
            for other, nbo in nbytes.items():
                if other != name:
                    bad(**{name: good[other]})
                    bad(**{name: good[other] + nbo - 8 if nbo > 8 else good[other]})
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.ccl_gray8(cc.noise(17, 31, 0.41), 8, 4)
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
import ccl_cases as cc
from ccl_ref import ccl_ref
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n, conn, rows = 250, 130, 2, 8, 100
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    ms = [np.stack([cc.noise(h, w, 0.41, 11), cc.spiral(h, w)]), np.stack([cc.noise(h, w, 0.59, 21), cc.comb(h, w)])]
    d_in = torch.from_numpy(ms[0]).to(dev)
    o_labels = torch.zeros((n, h, w), dtype=torch.int32, device=dev)
    o_count = torch.zeros((n,), dtype=torch.int32, device=dev)
    o_stats = torch.zeros((n, rows, 5), dtype=torch.int32, device=dev)
    o_sums = torch.zeros((n, rows, 2), dtype=torch.int64, device=dev)
    outs = (o_labels, o_count, o_stats, o_sums)

    def chain():
        c.ccl_gray8_dev(d_in.data_ptr(), o_labels.data_ptr(), o_count.data_ptr(), o_stats.data_ptr(), o_sums.data_ptr(),
                        w, h, n, conn, rows)

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
        want = ccl_ref(m, conn, rows)
        for name, o, wnt in zip(("labels", "count", "stats", "sums"), outs, want):
            got = o.cpu().numpy()
            if not np.array_equal(got.view(wnt.dtype), wnt): bad.append((r, name))
    del g
    c.close()
print(bad)
"""


def test_the_second_call_of_a_size_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled block counts, a labelling call allocates nothing and synchronises
    nothing, so it is captured into a hipGraph and replayed on new content.  Own process: torch's HIP runtime has to
    initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
