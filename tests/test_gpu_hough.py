"""GPU suite (-m gpu): the Hough line transform, mi355_hough_accum_gray8_dev / mi355_hough_lines_gray8_*.

Every comparison is bit-identity with the CPU reference tests/hough_ref.py fed the library's own trig table
(mi355_hough_trig_table: the platform's cos and sin are part of the contract; test_hough_cpu.py holds that table within
1 ulp of numpy's).  The float outputs are compared as their uint32 bit patterns.  There is no tolerance in this file.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import guarded  # noqa: E402
import hough_cases as hc  # noqa: E402
import hough_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in hc.SHAPES]
FILL = 0xA5


def _frames(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a[None] if a.ndim == 2 else a


@functools.lru_cache(maxsize=None)
def _geometry(shape, params):
    """(numangle, numrho, tab_cos, tab_sin) of the library for shape = (w, h)"""
    pkg = entry.load_package()
    na, nr = pkg.hough_shape(*shape, *params)
    assert (na, nr) == hr.shape(*shape, *params)
    tc, ts = pkg.hough_trig_table(*shape, *params)
    return na, nr, tc, ts


def _want(frames, params, threshold, max_lines):
    fs = _frames(frames)
    _, nr, tc, ts = _geometry((fs.shape[2], fs.shape[1]), params)
    return hr.hough_ref(fs, tc, ts, nr, threshold, max_lines, params[0], params[1], params[2])


def _run(ctx, frames, params, threshold, max_lines, votes=True, own_accum=True, accum_only=False):
    """(accum, lines, votes, count) of one device-resident call on (n, h, w) / (h, w) frames; absent outputs are None.
    Every output is prefilled with a pattern first."""
    fs = _frames(frames)
    n, h, w = fs.shape
    na, nr, _, _ = _geometry((w, h), params)
    acc = np.empty((n, na + 2, nr + 2), np.int32)
    lines, vts, cnt = np.empty((n, max_lines, 2), np.float32), np.empty((n, max_lines), np.int32), np.empty(n, np.int32)
    bufs = [fs, acc, lines, vts, cnt]
    ptr = [ctx.alloc(max(b.nbytes, 16)) for b in bufs]
    try:
        ctx.h2d(ptr[0], fs)
        for p, b in zip(ptr[1:], bufs[1:]):
            ctx.h2d(p, np.full(b.nbytes, FILL, np.uint8))
        if accum_only:
            ctx.hough_accum_gray8_dev(ptr[0], ptr[1], w, h, n, *params)
        else:
            ctx.hough_lines_gray8_dev(ptr[0], ptr[2], ptr[3] if votes else 0, ptr[4], ptr[1] if own_accum else 0, w, h, n,
                                      params[0], params[1], threshold, max_lines, params[2], params[3])
        ctx.sync()
        for p, b in zip(ptr[1:], bufs[1:]):
            ctx.d2h(b, p)
    finally:
        ctx.sync()
        for p in ptr:
            ctx.free(p)
    untouched = lambda b: (b.view(np.uint8) == FILL).all()      # noqa: E731
    if accum_only:
        assert untouched(lines) and untouched(vts) and untouched(cnt)
        return acc, None, None, None
    if not votes:
        assert untouched(vts), "d_votes = NULL and yet written"
        vts = None
    if not own_accum:
        assert untouched(acc)
        acc = None
    return acc, lines, vts, cnt


def _same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    g, v = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(g, v):
        i = int(np.flatnonzero(g.ravel() != v.ravel())[0])
        raise AssertionError("%s: the first difference at flat index %d: got %r, want %r (%d wrong)"
                             % (tag, i, got.ravel()[i], want.ravel()[i], int((g != v).sum())))


def _same_all(got, want, tag):
    for name, g, v in zip(("accum", "lines", "votes", "count"), got, want):
        if g is not None:
            _same(g, v, tag + " " + name)


@pytest.mark.parametrize("shape", hc.SHAPES, ids=IDS)
def test_accumulator_and_lines_are_bit_identical_to_the_cpu_reference(ctx, shape):
    named = hc.frames_of(shape)
    for params in hc.PARAMS:
        for name, f in named:
            tag = "%s %dx%d %r" % ((name,) + shape + (params,))
            for threshold, max_lines in ((0, 64), (2, 7)):
                want = _want(f, params, threshold, max_lines)
                _same_all(_run(ctx, f, params, threshold, max_lines), want, tag + " thr %d" % threshold)
            _same(_run(ctx, f, params, 0, 1, accum_only=True)[0], want[0], tag + " accum call")


def test_rows_beyond_the_lds_budget_and_each_side_of_every_path_boundary(ctx, pkg):
    for btag, shape in hc.boundary_shapes(pkg):
        w, h = shape
        for name, f in (("few", hc.few_pixels(h, w)), ("noise_1", hc.noise(h, w, 0.01))):
            want = _want(f, hc.DEFAULT, 1, 16)
            assert want[0].any()
            _same_all(_run(ctx, f, hc.DEFAULT, 1, 16), want, "%s %dx%d %s" % (btag, w, h, name))


def test_a_cell_beyond_65535_votes(ctx):
    w, h = hc.BIG["shape"]
    f = hc.full(h, w)
    want = _want(f, hc.BIG["params"], 65535, 8)
    assert int(want[0].max()) > 65535 and want[3][0] >= 1 and int(want[2][0, 0]) > 65535
    _same_all(_run(ctx, f, hc.BIG["params"], 65535, 8), want, "1024x1024 full, rho 128")


def test_selection_with_more_and_fewer_peaks_than_max_lines(ctx):
    f = dict(hc.frames_of((130, 67)))["noise_10"]
    for threshold, more in ((0, True), (24, False)):
        for max_lines in (1, 7, 4096):
            want = _want(f, hc.DEFAULT, threshold, max_lines)
            count = int(want[3][0])
            assert (count > 4096) if more else (0 < count < 7)
            got = _run(ctx, f, hc.DEFAULT, threshold, max_lines)
            _same_all(got, want, "selection thr %d max_lines %d" % (threshold, max_lines))
            m = min(count, max_lines)
            assert (got[2][0, :m] > threshold).all() and not got[2][0, m:].any() and not got[1][0, m:].any()   # zero fill


def test_no_votes_pointer_and_the_pooled_accumulator_give_the_same_lines(ctx):
    for shape in ((130, 67), (257, 3)):
        for name, f in hc.frames_of(shape):
            want = _want(f, hc.DEFAULT, 1, 32)
            for votes, own in ((False, True), (True, False), (False, False)):
                _same_all(_run(ctx, f, hc.DEFAULT, 1, 32, votes=votes, own_accum=own), want,
                          "%s votes=%r own_accum=%r" % (name, votes, own))


def test_a_batch_of_five_frames_equals_the_five_single_calls(ctx):
    named = dict(hc.frames_of((130, 67)))
    fs = np.stack([named[k] for k in ("noise_10", "empty", "lines", "full", "canny")])
    for params in (hc.DEFAULT, hc.PARAMS[2]):
        want = _want(fs, params, 3, 40)
        got = _run(ctx, fs, params, 3, 40)
        _same_all(got, want, "batch %r" % (params,))
        for i in range(len(fs)):
            one = _run(ctx, fs[i], params, 3, 40)
            _same_all(one, [g[i:i + 1] for g in got], "single %d %r" % (i, params))


def _packed(want):
    """the four outputs as one byte string: lines, votes, count, accumulator"""
    acc, lines, votes, count = want
    return np.concatenate([a.ravel().view(np.uint8) for a in (lines, votes, count, acc)])


def test_a_guarded_arena_around_the_input_and_all_outputs(ctx):
    """The input at byte offsets 0, 1, 7 and 15 in seeded noise; lines, votes, count and the accumulator back to back
    between two guards, at 4-byte offsets: no byte outside is written, none inside is left unwritten."""
    w, h = 63, 65
    named = dict(hc.frames_of((w, h)))
    pair = np.stack([named["noise_10"], named["lines"]])
    max_lines, threshold = 24, 4
    want = _want(pair, hc.DEFAULT, threshold, max_lines)
    expect = _packed(want)
    at_votes, at_count = want[1].nbytes, want[1].nbytes + want[2].nbytes
    at_accum = at_count + want[3].nbytes

    def lines_call(d_in, d_out):
        ctx.hough_lines_gray8_dev(d_in, d_out, d_out + at_votes, d_out + at_count, d_out + at_accum, w, h, 2,
                                  hc.DEFAULT[0], hc.DEFAULT[1], threshold, max_lines, hc.DEFAULT[2], hc.DEFAULT[3])

    def accum_call(d_in, d_out):
        ctx.hough_accum_gray8_dev(d_in, d_out, w, h, 2, *hc.DEFAULT)

    acc_bytes = want[0].ravel().view(np.uint8)
    for off_in in (0, 1, 7, 15):
        for off_out in (0, 4, 12):
            tag = "in+%d out+%d" % (off_in, off_out)
            got = guarded.run(ctx, lines_call, pair, expect, off_in=off_in, off_out=off_out, tag="lines " + tag)
            guarded.check(got, expect, tag="lines " + tag)
            got = guarded.run(ctx, accum_call, pair, acc_bytes, off_in=off_in, off_out=off_out, tag="accum " + tag)
            guarded.check(got, acc_bytes, tag="accum " + tag)


def test_the_batched_form_equals_the_device_form(ctx):
    named = dict(hc.frames_of((130, 67)))
    fs = np.stack([named["lines"], named["noise_10"], named["empty"]])
    want = _want(fs, hc.DEFAULT, 5, 50)
    lines, votes, count, prof = ctx.hough_lines_gray8(fs, hc.DEFAULT[0], hc.DEFAULT[1], 5, 50, profile=True)
    _same_all((None, lines, votes, count), want, "batched")
    assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
    lines, votes, count = ctx.hough_lines_gray8(fs[0], hc.DEFAULT[0], hc.DEFAULT[1], 5, 50)
    assert lines.shape == (50, 2) and votes.shape == (50,) and count == int(want[3][0])
    _same(lines, want[1][0], "batched, one frame")


def test_argument_checks(ctx, pkg):
    w, h, max_lines = 64, 48, 16
    na, nr, _, _ = _geometry((w, h), hc.DEFAULT)
    acc_bytes = (na + 2) * (nr + 2) * 4
    base = ctx.alloc(4 * 65536 + acc_bytes)
    try:
        ctx.h2d(base, hc.drawn_lines(h, w))
        good = dict(d_in=base, d_lines=base + 65536, d_votes=base + 2 * 65536, d_count=base + 3 * 65536,
                    d_accum=base + 4 * 65536, w=w, h=h, nframes=1, rho=1.0, theta=hc.PI / 180, threshold=10,
                    max_lines=max_lines, min_theta=0.0, max_theta=hc.PI)

        def bad(code=-1, **kw):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.hough_lines_gray8_dev(**dict(good, **kw))
            assert e.value.code == code, kw

        ctx.hough_lines_gray8_dev(**good)
        ctx.hough_lines_gray8_dev(**dict(good, d_in=base + 3))           # the input takes any byte alignment
        ctx.hough_lines_gray8_dev(**dict(good, d_votes=0, d_accum=0))    # the two optional pointers
        for name in ("d_in", "d_lines", "d_count"):
            bad(**{name: 0})
        for name in ("d_lines", "d_votes", "d_count", "d_accum"):        # outputs are 4-byte aligned
            bad(**{name: good[name] + 2})
        for kw in (dict(w=0), dict(h=0), dict(nframes=0), dict(w=32767), dict(rho=0.0), dict(theta=float("nan")),
                   dict(min_theta=-0.1), dict(max_theta=3.2), dict(min_theta=2.0, max_theta=1.0), dict(threshold=-1),
                   dict(max_lines=0), dict(max_lines=4097), dict(theta=hc.PI / 2000)):
            bad(**kw)
        # overlapping ranges: each output against the input and against another output
        lines_bytes = max_lines * 8
        bad(d_lines=base + w * h - 4)
        bad(d_count=base)
        bad(d_votes=good["d_lines"] + lines_bytes - 4)
        bad(d_count=good["d_votes"] + max_lines * 4 - 4)
        bad(d_accum=good["d_count"])
        bad(d_accum=good["d_lines"] - acc_bytes + 4)
        ctx.hough_lines_gray8_dev(**dict(good, d_votes=good["d_lines"] + lines_bytes))     # back to back is fine
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.hough_accum_gray8_dev(base, base + 64, w, h, 1, 1.0, hc.PI / 180)
        assert e.value.code == -1
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.hough_accum_gray8_dev(base, 0, w, h, 1, 1.0, hc.PI / 180)
        assert e.value.code == -1
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.hough_lines_gray8(hc.drawn_lines(17, 31), 1.0, hc.PI / 180, 5, 8)
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
import hough_cases as hc
import hough_ref as hr
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n, thr, ml = 130, 67, 2, 3, 40
rho, theta, lo, hi = hc.DEFAULT
na, nr = pkg.hough_shape(w, h, rho, theta, lo, hi)
tc, ts = pkg.hough_trig_table(w, h, rho, theta, lo, hi)
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    fs = [np.stack([hc.noise(h, w, 0.10), hc.drawn_lines(h, w)]), np.stack([hc.drawn_lines(h, w), hc.noise(h, w, 0.01)])]
    d_f = torch.from_numpy(fs[0]).to(dev)
    o_l = torch.zeros((n, ml, 2), dtype=torch.float32, device=dev)
    o_v = torch.zeros((n, ml), dtype=torch.int32, device=dev)
    o_c = torch.zeros((n,), dtype=torch.int32, device=dev)

    def call():
        c.hough_lines_gray8_dev(d_f.data_ptr(), o_l.data_ptr(), o_v.data_ptr(), o_c.data_ptr(), 0, w, h, n, rho, theta,
                                thr, ml, lo, hi)

    call()                              # the first call of this shape: sizes the pooled buffers, uploads the table
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()                          # the second: allocates nothing, waits for nothing
    d_f.copy_(torch.from_numpy(fs[1]).to(dev))
    o_l.fill_(7); o_v.fill_(7); o_c.fill_(7)
    g.replay()                          # once
    s.synchronize()
    _, lines, votes, count = hr.hough_ref(fs[1], tc, ts, nr, thr, ml, rho, theta, lo)
    if not np.array_equal(o_l.cpu().numpy().view(np.uint32), lines.view(np.uint32)): bad.append("lines")
    if not np.array_equal(o_v.cpu().numpy(), votes): bad.append("votes")
    if not np.array_equal(o_c.cpu().numpy(), count): bad.append("count")
    del g
    c.close()
print(bad)
"""


def test_the_second_call_of_a_shape_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled scratch and accumulator and uploaded the trig table, a lines call
    allocates nothing and synchronises nothing, so it is captured into a hipGraph and replayed once on new content.  Own
    process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
