"""GPU suite (-m gpu): hysteresis thresholding and Canny, mi355_hysteresis_gray8_* / mi355_canny_gray8_*.

Every comparison is bit-identity with the CPU reference tests/canny_ref.py (or a closed form): the edge map is integer
arithmetic with one right answer per input.  There is no tolerance anywhere in this file.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import canny_cases as kc  # noqa: E402
import canny_ref as cr  # noqa: E402
import ccl_cases as cc  # noqa: E402
import guarded  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in kc.SHAPES]


def _frames(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a[None] if a.ndim == 2 else a


def _dev(ctx, call, frames):
    """The (n, h, w) output of call(d_in, d_out, w, h, n) on (n, h, w) / (h, w) frames; the output is prefilled with a
    pattern that is neither 0 nor 255 first."""
    fs = _frames(frames)
    n, h, w = fs.shape
    out = np.empty((n, h, w), np.uint8)
    d_in, d_out = ctx.alloc(max(fs.nbytes, 16)), ctx.alloc(max(out.nbytes, 16))
    try:
        ctx.h2d(d_in, fs)
        ctx.h2d(d_out, np.full(out.nbytes, 0xA5, np.uint8))
        call(d_in, d_out, w, h, n)
        ctx.sync()
        ctx.d2h(out, d_out)
    finally:
        ctx.sync()
        ctx.free(d_in)
        ctx.free(d_out)
    return out


def _canny(ctx, frames, t1, t2, flags):
    return _dev(ctx, lambda i, o, w, h, n: ctx.canny_gray8_dev(i, o, w, h, n, t1, t2, flags), frames)


def _hyst(ctx, frames, low, high, conn):
    return _dev(ctx, lambda i, o, w, h, n: ctx.hysteresis_gray8_dev(i, o, w, h, n, low, high, conn), frames)


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got.ravel() != want.ravel())[0])
        raise AssertionError("%s: the first difference at flat index %d: got %d, want %d (%d wrong)"
                             % (tag, i, got.ravel()[i], want.ravel()[i], int((got != want).sum())))


@functools.lru_cache(maxsize=None)
def _canny_case(shape):
    """(names, frames (n, h, w), {thresholds: reference edge maps (n, h, w)}) of every content at `shape`, once"""
    named = kc.frames_of(shape)
    fs = np.stack([f for _, f in named])
    want = {t: cr.canny_ref(fs, *t) for t in kc.THRESHOLDS}
    for a in [fs] + list(want.values()):
        a.setflags(write=False)
    return [name for name, _ in named], fs, want


@functools.lru_cache(maxsize=None)
def _hyst_case(shape, conn):
    named = kc.responses_of(shape)
    rs = np.stack([r for _, r in named])
    want = cr.hysteresis_ref(rs, kc.LOW, kc.HIGH, conn)
    rs.setflags(write=False)
    want.setflags(write=False)
    return [name for name, _ in named], rs, want


@pytest.mark.parametrize("shape", kc.SHAPES, ids=IDS)
def test_canny_is_bit_identical_to_the_cpu_reference(ctx, shape):
    names, fs, want = _canny_case(shape)
    for t in kc.THRESHOLDS:
        for f, name in enumerate(names):
            _same(_canny(ctx, fs[f], *t), want[t][f:f + 1], "canny %s %dx%d %r" % ((name,) + shape + (t,)))


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
@pytest.mark.parametrize("shape", kc.SHAPES, ids=IDS)
def test_hysteresis_is_bit_identical_to_the_cpu_reference(ctx, shape, conn):
    names, rs, want = _hyst_case(shape, conn)
    for f, name in enumerate(names):
        tag = "hysteresis %s %dx%d conn %d" % ((name,) + shape + (conn,))
        _same(_hyst(ctx, rs[f], kc.LOW, kc.HIGH, conn), want[f:f + 1], tag)
        if name.endswith("/random"):
            for low, high in kc.BOUNDARIES:
                # (the labelling form of the reference: test_canny_cpu.py holds it against the flood fill)
                _same(_hyst(ctx, rs[f], low, high, conn),
                      cr.hysteresis_ref(rs[f:f + 1], low, high, conn, cr.kept_by_labels),
                      tag + " low %d high %d" % (low, high))


def test_a_batch_equals_one_call_per_frame_and_frames_do_not_leak(ctx):
    names, fs, want = _canny_case((250, 130))
    for t in (kc.THRESHOLDS[0], kc.THRESHOLDS[4]):
        got = _canny(ctx, fs, *t)
        _same(got, want[t], "canny batch %r" % (t,))
        for f, name in enumerate(names):
            _same(_canny(ctx, fs[f], *t), got[f:f + 1], "canny single %s" % name)
    for conn in cc.CONNECTIVITIES:
        names, rs, want = _hyst_case((250, 130), conn)
        got = _hyst(ctx, rs, kc.LOW, kc.HIGH, conn)
        _same(got, want, "hysteresis batch conn %d" % conn)
        for f in range(0, len(names), 7):
            _same(_hyst(ctx, rs[f], kc.LOW, kc.HIGH, conn), got[f:f + 1], "hysteresis single %s" % names[f])
        # a last row of candidates, then a first row that is strong: neighbours in memory, not in any frame; and
        # row_ends: (w - 1, y) and (0, y + 1) likewise
        masks = dict(cc.frames_of((250, 130)))
        a = np.where(masks["last_row"] != 0, kc.FG, kc.BG).astype(np.uint8)
        b = np.where(masks["first_row"] != 0, kc.STRONG, kc.BG).astype(np.uint8)
        c = kc.response(masks["row_ends"], "first")
        got = _hyst(ctx, np.stack([a, b, c, a]), kc.LOW, kc.HIGH, conn)
        assert not got[0].any() and not got[3].any(), "a strong row of the next frame leaked into this one"
        assert (got[1][0] == 255).all() and not got[1][1:].any()
        assert got[2][0, 0] == 255 and int((got[2] != 0).sum()) == 1
    # the same through Canny: a frame whose last rows hold a weak edge, in front of one whose first rows hold a strong one
    weak, strong = np.zeros((130, 250), np.uint8), np.zeros((130, 250), np.uint8)
    weak[-1] = 20           # |dy| = 80 on the rows h - 2 and h - 1: candidates under (50, 150), never strong
    strong[0] = 200
    got = _canny(ctx, np.stack([weak, strong]), 50, 150, 0)
    _same(got, cr.canny_ref(np.stack([weak, strong]), 50, 150), "canny weak / strong pair")
    assert not got[0].any() and got[1].any()


def test_canny_equals_the_hysteresis_of_the_reference_s_class_map(ctx):
    for shape in ((250, 130), kc.SHAPES[-2]):
        names, fs, want = _canny_case(shape)
        for t in kc.THRESHOLDS:
            low, high = cr.thresholds(*t)
            cls = np.stack([cr.classes(f, low, high, t[2]) for f in fs])
            assert cls.max() <= 2
            _same(_hyst(ctx, cls, 0, 1, 8), want[t], "classes -> hysteresis %dx%d %r" % (shape + (t,)))


@pytest.mark.parametrize("which", ["canny", "hysteresis"])
@pytest.mark.parametrize("shape", [(67, 48), (257, 65)], ids=["67x48", "257x65"])
def test_any_byte_alignment_in_a_guarded_arena(ctx, shape, which):
    """Input offsets 0 .. 15 x output offsets 0 .. 15, two frames per call: no byte outside the output is written, none
    inside is left unwritten."""
    w, h = shape
    if which == "canny":
        names, fs, want = _canny_case(shape)
        idx = [names.index("smooth"), names.index("noise")]
        pair, expect = fs[idx], want[kc.THRESHOLDS[0]][idx]

        def call(d_in, d_out):
            ctx.canny_gray8_dev(d_in, d_out, w, h, 2, *kc.THRESHOLDS[0])
    else:
        names, rs, want = _hyst_case(shape, 8)
        idx = [names.index("noise_0.41/random"), names.index("spiral/last")]
        pair, expect = rs[idx], want[idx]

        def call(d_in, d_out):
            ctx.hysteresis_gray8_dev(d_in, d_out, w, h, 2, kc.LOW, kc.HIGH, 8)
    assert expect.any() and not expect.all()
    for off_in in range(16):
        for off_out in range(16):
            tag = "%s %dx%d in+%d out+%d" % (which, w, h, off_in, off_out)
            got = guarded.run(ctx, call, pair, expect, off_in=off_in, off_out=off_out, tag=tag)
            guarded.check(got, expect, tag=tag)


@functools.lru_cache(maxsize=None)
def _hd():
    h, w = 1080, 1920
    sm = kc.smooth(h, w)
    sp = cc.spiral(h, w)
    ys, xs = np.nonzero(sp)
    inner = int(np.argmin((ys - h // 2) ** 2 + (xs - w // 2) ** 2))     # the spiral pixel nearest the centre
    resp = np.where(sp != 0, kc.FG, kc.BG).astype(np.uint8)
    resp[ys[inner], xs[inner]] = kc.STRONG
    return sm, cr.canny_ref(sm, 50, 150, 0, cr.kept_by_labels), resp, (sp != 0).astype(np.uint8) * 255


def test_a_1080p_smooth_frame(ctx):
    sm, want, _, _ = _hd()
    assert 0 < int((want != 0).sum()) < want.size // 2     # the input reaches both answers (the reference gives a third)
    _same(_canny(ctx, sm, 50, 150, 0), want[None], "1080p smooth")


@pytest.mark.parametrize("conn", cc.CONNECTIVITIES)
def test_a_1080p_spiral_response_with_the_strong_pixel_at_its_inner_end(ctx, conn):
    _, _, resp, want = _hd()
    assert int((resp == kc.STRONG).sum()) == 1
    _same(_hyst(ctx, resp, kc.LOW, kc.HIGH, conn), want[None], "1080p spiral conn %d" % conn)   # the whole spiral
    _same(_hyst(ctx, resp, kc.LOW, kc.STRONG, conn), np.zeros_like(want)[None], "1080p spiral, nothing strong")


def test_the_device_form_equals_the_batched_form(ctx):
    for shape in ((67, 48), (250, 130), (1, 300)):
        names, fs, want = _canny_case(shape)
        for t in (kc.THRESHOLDS[0], kc.THRESHOLDS[5]):
            out, prof = ctx.canny_gray8(fs, *t, profile=True)
            _same(out, want[t], "canny batched %dx%d" % shape)
            _same(out, _canny(ctx, fs, *t), "canny device %dx%d" % shape)
            assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
        one = ctx.canny_gray8(fs[1], 50, 150)
        assert one.shape == fs[1].shape and np.array_equal(one, want[kc.THRESHOLDS[0]][1])
        names, rs, want = _hyst_case(shape, 8)
        out, prof = ctx.hysteresis_gray8(rs, kc.LOW, kc.HIGH, 8, profile=True)
        _same(out, want, "hysteresis batched %dx%d" % shape)
        _same(out, _hyst(ctx, rs, kc.LOW, kc.HIGH, 8), "hysteresis device %dx%d" % shape)
        assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5]
        one = ctx.hysteresis_gray8(rs[4], kc.LOW, kc.HIGH)
        assert one.shape == rs[4].shape and np.array_equal(one, want[4])


def test_two_calls_on_the_same_input_give_identical_bytes(ctx):
    sm, want, resp, _ = _hd()
    a, b = _canny(ctx, sm, 50, 150, 0), _canny(ctx, sm, 50, 150, 0)
    _same(a, b, "canny repeat")
    noisy = kc.response(cc.noise(1080, 1920, 0.59, seed=5), "random")
    a, b = _hyst(ctx, noisy, kc.LOW, kc.HIGH, 4), _hyst(ctx, noisy, kc.LOW, kc.HIGH, 4)
    _same(a, b, "hysteresis repeat")


def test_argument_checks(ctx, pkg):
    w, h = 64, 48
    base = ctx.alloc(64 * 1024)
    try:
        d_in, d_out = base, base + 16384
        ctx.h2d(d_in, kc.smooth(h, w))
        table = [
            (ctx.hysteresis_gray8_dev, dict(d_in=d_in, d_out=d_out, w=w, h=h, nframes=1, low=60, high=150, connectivity=8),
             [dict(connectivity=0), dict(connectivity=6), dict(low=-1), dict(high=256), dict(low=151), dict(low=200, high=100),
              dict(low=256, high=256)]),
            (ctx.canny_gray8_dev, dict(d_in=d_in, d_out=d_out, w=w, h=h, nframes=1, threshold1=50.0, threshold2=150.0,
                                       flags=0),
             [dict(threshold1=-1.0), dict(threshold2=float("nan")), dict(threshold1=float("inf")), dict(threshold2=2.0e9),
              dict(flags=2), dict(flags=3), dict(flags=-1)]),
        ]
        for fn, good, bad_values in table:
            def bad(code=-1, **kw):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(**dict(good, **kw))
                assert e.value.code == code, (fn.__name__, kw)

            fn(**good)
            fn(**dict(good, d_in=d_in + 3, d_out=d_out + 5))             # both sides take any byte alignment
            for name in ("d_in", "d_out"):
                bad(**{name: 0})
            for kw in bad_values + [dict(w=0), dict(h=0), dict(nframes=0), dict(w=-1), dict(w=65536, h=32768)]:
                bad(**kw)
            # the output against the input: in place, and from either side
            for d in (d_in, d_in + w * h - 1, d_in - w * h + 1, d_in + 16):
                bad(d_out=d)
            fn(**dict(good, d_out=d_in + w * h))                           # back to back is fine
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


def test_bgr_input_is_refused(ctx, pkg):
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for fn, args in ((ctx.canny_gray8, (50, 150)), (ctx.hysteresis_gray8, (60, 150))):
            with pytest.raises(pkg.Mi355Error) as e:
                fn(kc.smooth(17, 31), *args)
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
import canny_cases as kc
import ccl_cases as cc
import canny_ref as cr
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n = 250, 130, 2
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    fs = [np.stack([kc.smooth(h, w, 11), kc.disc(h, w)]), np.stack([kc.smooth(h, w, 21), kc.noise(h, w, 3)])]
    rs = [np.stack([kc.response(cc.noise(h, w, 0.41, 11), "random"), kc.response(cc.spiral(h, w), "last")]),
          np.stack([kc.response(cc.noise(h, w, 0.59, 21), "random"), kc.response(cc.comb(h, w), "last")])]
    d_f = torch.from_numpy(fs[0]).to(dev)
    d_r = torch.from_numpy(rs[0]).to(dev)
    o_c = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    o_h = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)

    def chain():
        c.canny_gray8_dev(d_f.data_ptr(), o_c.data_ptr(), w, h, n, 50.0, 150.0, 0)
        c.hysteresis_gray8_dev(d_r.data_ptr(), o_h.data_ptr(), w, h, n, kc.LOW, kc.HIGH, 4)

    chain()                             # the first call of this size: sizes the pooled parent array
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()                         # the second: allocates nothing, waits for nothing
    for r in range(2):
        d_f.copy_(torch.from_numpy(fs[1 - r]).to(dev))
        d_r.copy_(torch.from_numpy(rs[1 - r]).to(dev))
        o_c.fill_(7)
        o_h.fill_(7)
        g.replay()
        s.synchronize()
        if not np.array_equal(o_c.cpu().numpy(), cr.canny_ref(fs[1 - r], 50, 150)): bad.append((r, "canny"))
        if not np.array_equal(o_h.cpu().numpy(), cr.hysteresis_ref(rs[1 - r], kc.LOW, kc.HIGH, 4)): bad.append((r, "hyst"))
    del g
    c.close()
print(bad)
"""


def test_the_second_call_of_a_size_can_be_captured_into_a_hip_graph():
    """After the first call has sized the pooled parent array, a Canny or hysteresis call allocates nothing and
    synchronises nothing, so it is captured into a hipGraph and replayed on new content.  Own process: torch's HIP
    runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
