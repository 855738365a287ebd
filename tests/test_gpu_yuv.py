"""GPU suite (-m gpu): YUV frames to and from RGBA and their luma planes, mi355_yuv_to_rgba8_dev / mi355_rgba8_to_yuv_dev /
mi355_yuv_to_gray8_dev and the two host-buffer calls.

Every comparison is bit identity with the CPU reference tests/yuv_ref.py: the arithmetic is int32, so there is no
tolerance anywhere in this file.  Inputs carry arbitrary bytes in their padding; outputs are compared whole, padding
included, against what was there before the call.
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
import yuv_cases as yc  # noqa: E402
import yuv_ref as yr  # noqa: E402

pytestmark = pytest.mark.gpu

ENCODE_LAYOUTS = (yr.NV12, yr.NV21, yr.I420, yr.YV12)


class _Arena:
    """two device buffers that grow to the largest request: one allocation per test, not per call"""

    def __init__(self, ctx):
        self.ctx, self.size, self.ptr = ctx, [0, 0], [0, 0]

    def get(self, i, nbytes):
        if nbytes > self.size[i]:
            if self.ptr[i]:
                self.ctx.sync()
                self.ctx.free(self.ptr[i])
            self.ptr[i], self.size[i] = self.ctx.alloc(nbytes + 64), nbytes + 64
        return self.ptr[i]

    def close(self):
        self.ctx.sync()
        for p in self.ptr:
            if p:
                self.ctx.free(p)


@pytest.fixture
def arena(ctx):
    a = _Arena(ctx)
    yield a
    a.close()


def _run(arena, call, inp, out_before):
    """call(d_in, d_out) on `inp` with the output holding `out_before`; returns the output bytes"""
    ctx = arena.ctx
    inp = np.ascontiguousarray(inp, np.uint8)
    out = np.ascontiguousarray(out_before, np.uint8).copy()
    d_in, d_out = arena.get(0, inp.nbytes), arena.get(1, out.nbytes)
    ctx.h2d(d_in, inp)
    ctx.h2d(d_out, out)
    call(d_in, d_out)
    ctx.sync()
    ctx.d2h(out, d_out)
    ctx.sync()
    return out


def _decode(arena, buf, w, h, n, layout, std, pitch, rows):
    return _run(arena, lambda a, b: arena.ctx.yuv_to_rgba8_dev(a, b, w, h, n, layout, std, pitch, rows), buf,
                np.full((n, h, w, 4), 0x5A, np.uint8))


def _luma(arena, buf, w, h, n, layout, pitch, rows):
    return _run(arena, lambda a, b: arena.ctx.yuv_to_gray8_dev(a, b, w, h, n, layout, pitch, rows), buf,
                np.full((n, h, w), 0x5A, np.uint8))


def _encode(arena, rgba, layout, std, pitch, rows, before):
    n, h, w = rgba.shape[:3]
    return _run(arena, lambda a, b: arena.ctx.rgba8_to_yuv_dev(a, b, w, h, n, layout, std, pitch, rows), rgba, before)


@functools.lru_cache(maxsize=None)
def _decode_case(w, h, packed):
    """(contents, {standard: reference RGBA (3, h, w, 4)}, reference luma), computed once"""
    contents = yc.decode_contents(w, h, packed)
    ref = {s: np.stack([yr.decode_planes(*p, s) for _, p in contents]) for s in yr.STANDARDS}
    y = np.stack([p[0] for _, p in contents])
    for a in list(ref.values()) + [y]:
        a.setflags(write=False)
    return contents, ref, y


@functools.lru_cache(maxsize=None)
def _encode_case(w, h):
    """(RGBA (2, h, w, 4), {standard: [(Y, U, V) per frame]}), computed once"""
    rgba = np.stack([a for _, a in yc.encode_contents(w, h)])
    rgba.setflags(write=False)
    return rgba, {s: [yr.encode_planes(f, s) for f in rgba] for s in yr.STANDARDS}


def _encode_want(w, h, layout, std, pitch, rows, before):
    """the reference frames over `before`: pixel bytes replaced, padding kept"""
    _, planes = _encode_case(w, h)
    return np.stack([yr.pack(p, layout, pitch, rows, before[i]) for i, p in enumerate(planes[std])])


# ---- every case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", yc.SIZES, ids=["%dx%d" % s for s in yc.SIZES])
def test_decode_and_luma_of_every_layout_geometry_and_standard(arena, w, h):
    """three-frame batches (noise, legal, extremes) of every layout, pitch and row count, under every standard"""
    for layout in yr.LAYOUTS:
        contents, ref, y = _decode_case(w, h, yr.is_packed(layout))
        for pitch, rows in yc.geometries(layout, w, h):
            buf = yc.pack_batch(contents, layout, pitch, rows)
            tag = (yr.LAYOUT_NAMES[layout], w, h, pitch, rows)
            for std in yr.STANDARDS:
                got = _decode(arena, buf, w, h, 3, layout, std, pitch, rows)
                assert np.array_equal(got, ref[std]), tag + (std,)
            assert np.array_equal(_luma(arena, buf, w, h, 3, layout, pitch, rows), y), tag


@pytest.mark.parametrize("w,h", yc.SIZES, ids=["%dx%d" % s for s in yc.SIZES])
def test_encode_of_every_layout_geometry_and_standard(arena, w, h):
    """two-frame batches (cube corners in noise, strongly differing blocks); the padding keeps its bytes"""
    rgba, _ = _encode_case(w, h)
    for layout in ENCODE_LAYOUTS:
        for pitch, rows in yc.geometries(layout, w, h):
            fb = yr.frame_bytes(layout, w, h, pitch, rows)
            before = yc.padding(2 * fb, pitch + rows).reshape(2, fb)
            for std in yr.STANDARDS:
                got = _encode(arena, rgba, layout, std, pitch, rows, before)
                want = _encode_want(w, h, layout, std, pitch, rows, before)
                assert np.array_equal(got, want), (yr.LAYOUT_NAMES[layout], w, h, pitch, rows, std)


@pytest.mark.parametrize("w,h", [(18, 6), (250, 130)], ids=["18x6", "250x130"])
def test_a_batch_equals_one_call_per_frame(arena, w, h):
    for layout in (yr.NV12, yr.YV12, yr.UYVY):
        pitch, rows = yc.geometries(layout, w, h)[7]      # + 62 bytes, + 2 rows
        contents, ref, y = _decode_case(w, h, yr.is_packed(layout))
        fb = yr.frame_bytes(layout, w, h, pitch, rows)
        buf = yc.pack_batch(contents, layout, pitch, rows).reshape(3, fb)
        for n in (2, 3):
            got = _decode(arena, buf[:n], w, h, n, layout, yr.BT709, pitch, rows)
            assert np.array_equal(got, ref[yr.BT709][:n])
            assert np.array_equal(_luma(arena, buf[:n], w, h, n, layout, pitch, rows), y[:n])
            for f in range(n):
                one = _decode(arena, buf[f], w, h, 1, layout, yr.BT709, pitch, rows)
                assert np.array_equal(one[0], got[f]), (layout, n, f)
        if layout in ENCODE_LAYOUTS:
            rgba, _ = _encode_case(w, h)
            before = yc.padding(2 * fb, 5).reshape(2, fb)
            got = _encode(arena, rgba, layout, yr.BT709, pitch, rows, before)
            for f in range(2):
                one = _encode(arena, rgba[f:f + 1], layout, yr.BT709, pitch, rows, before[f:f + 1])
                assert np.array_equal(one[0], got[f]), (layout, f)


# ---- more frames than the grid has rows ------------------------------------------------------------------------------
BIG_N, BIG_K = 65537, 251      # gridDim.y holds 65535 frames; 65535 % 251 == 24: frame f - 65535 has other content than f


@functools.lru_cache(maxsize=None)
def _big_decode_table(packed):
    """251 distinct 2 x 2 frames as (Y, U, V): the three kinds of decode content in turn, each under a seed of its own"""
    kinds = (yc.noise_planes, yc.legal_planes, yc.extreme_planes)
    planes = [kinds[k % 3](2, 2, packed, 7000 + k) for k in range(BIG_K)]
    assert len({b"".join(a.tobytes() for a in p) for p in planes}) == BIG_K
    return planes


@functools.lru_cache(maxsize=None)
def _big_encode_table():
    """251 distinct 2 x 2 RGBA frames: the two kinds of encode content in turn"""
    rgba = np.stack([(yc.cube_rgba, yc.blocks_rgba)[k % 2](2, 2, 9000 + k) for k in range(BIG_K)])
    assert len({f.tobytes() for f in rgba}) == BIG_K
    rgba.setflags(write=False)
    return rgba


def _check_big(arena, call, table, want_table, tag):
    """frame f of the batch is table[f % 251]; the output starts as the complement of a part of every expected byte"""
    idx = np.arange(BIG_N) % BIG_K
    want = np.asarray(want_table)[idx]
    got = _run(arena, call, np.asarray(table)[idx], want ^ 0xA5)
    bad = np.flatnonzero((got != want).reshape(BIG_N, -1).any(axis=1))
    assert bad.size == 0, (tag, bad.size, bad[:8].tolist())


def test_a_batch_of_more_frames_than_the_grid_has_rows(arena):
    """65537 tight 2 x 2 frames: the kernels' frame loop takes its second trip for frames 65535 and 65536.  The reference
    is computed for the 251 distinct frames only; a loop that stops after one trip leaves the prefill in the last two
    frames, and one that serves frame f from frame f - 65535 returns content 24 places off."""
    ctx, w, h = arena.ctx, 2, 2
    for layout, std in ((yr.NV12, yr.BT709), (yr.I420, yr.BT601), (yr.YUY2, yr.BT601_FULL)):
        planes = _big_decode_table(yr.is_packed(layout))
        _check_big(arena, lambda a, b: ctx.yuv_to_rgba8_dev(a, b, w, h, BIG_N, layout, std, 0, 0),
                   [yr.pack(p, layout) for p in planes], [yr.decode_planes(*p, std) for p in planes],
                   "decode " + yr.LAYOUT_NAMES[layout])
    for layout in (yr.NV12, yr.UYVY):
        planes = _big_decode_table(yr.is_packed(layout))
        _check_big(arena, lambda a, b: ctx.yuv_to_gray8_dev(a, b, w, h, BIG_N, layout, 0, 0),
                   [yr.pack(p, layout) for p in planes], [p[0] for p in planes], "luma " + yr.LAYOUT_NAMES[layout])
    rgba = _big_encode_table()
    for layout, std in ((yr.NV12, yr.BT601), (yr.I420, yr.BT709)):
        _check_big(arena, lambda a, b: ctx.rgba8_to_yuv_dev(a, b, w, h, BIG_N, layout, std, 0, 0), rgba,
                   [yr.pack(yr.encode_planes(f, std), layout) for f in rgba], "encode " + yr.LAYOUT_NAMES[layout])


# ---- guarded arena ---------------------------------------------------------------------------------------------------
def _guard_geometries(layout, w, h):
    g = yc.geometries(layout, w, h)
    return [g[0], g[10]]      # tight, and rounded up to 256 with two more rows (aligned accesses at offsets 0 and 8)


@pytest.mark.parametrize("w,h", [(18, 6), (250, 130)], ids=["18x6", "250x130"])
def test_decode_at_any_byte_alignment_in_a_guarded_arena(ctx, w, h):
    """two frames, every d_yuv offset 0 .. 15 against every dword offset of d_rgba"""
    for layout in yr.LAYOUTS:
        contents, ref, _ = _decode_case(w, h, yr.is_packed(layout))
        std = yr.STANDARDS[layout % 3]
        for pitch, rows in _guard_geometries(layout, w, h):
            buf = yc.pack_batch(contents[:2], layout, pitch, rows)
            want = ref[std][:2]
            tag = "decode %s %dx%d pitch %d rows %d" % (yr.LAYOUT_NAMES[layout], w, h, pitch, rows)
            for off_in in range(16):
                for off_out in (0, 4, 8, 12):
                    got = guarded.run(ctx, lambda a, b: ctx.yuv_to_rgba8_dev(a, b, w, h, 2, layout, std, pitch, rows), buf,
                                      want, off_in=off_in, off_out=off_out, tag=tag)
                    guarded.check(got, want, tag="%s in+%d out+%d" % (tag, off_in, off_out))


@pytest.mark.parametrize("w,h", [(18, 6), (250, 130)], ids=["18x6", "250x130"])
def test_encode_at_any_byte_alignment_in_a_guarded_arena(ctx, w, h):
    """two frames, every d_yuv offset 0 .. 15; guarded.run prefills the payload with expected ^ 0x80, so the padding
    positions of `expected` hold arbitrary bytes and must come back as that prefill: never written"""
    rgba, _ = _encode_case(w, h)
    for layout in ENCODE_LAYOUTS:
        std = yr.STANDARDS[layout % 3]
        for pitch, rows in _guard_geometries(layout, w, h):
            fb = yr.frame_bytes(layout, w, h, pitch, rows)
            expected = _encode_want(w, h, layout, std, pitch, rows, yc.padding(2 * fb, 11).reshape(2, fb))
            pixel = np.tile(yr.pixel_mask(layout, w, h, pitch, rows), (2, 1))
            prefill = guarded.prefill_of(expected)
            tag = "encode %s %dx%d pitch %d rows %d" % (yr.LAYOUT_NAMES[layout], w, h, pitch, rows)
            for off_out in range(16):
                off_in = 4 * (off_out % 4)
                got = guarded.run(ctx, lambda a, b: ctx.rgba8_to_yuv_dev(a, b, w, h, 2, layout, std, pitch, rows), rgba,
                                  expected, off_in=off_in, off_out=off_out, tag=tag)
                assert np.array_equal(got[pixel], expected[pixel]), (tag, off_out, "pixel bytes")
                assert np.array_equal(got[~pixel], prefill[~pixel]), (tag, off_out, "padding was written")


@pytest.mark.parametrize("w,h", [(18, 6), (250, 130)], ids=["18x6", "250x130"])
def test_luma_at_any_byte_alignment_in_a_guarded_arena(ctx, w, h):
    """two frames, every d_yuv offset against every d_gray offset, 0 .. 15 each (NV12 stands for the four 4:2:0
    layouts: the luma plane is the same bytes)"""
    for layout in (yr.NV12, yr.YUY2, yr.UYVY):
        contents, _, y = _decode_case(w, h, yr.is_packed(layout))
        for pitch, rows in _guard_geometries(layout, w, h):
            buf = yc.pack_batch(contents[:2], layout, pitch, rows)
            tag = "luma %s %dx%d pitch %d rows %d" % (yr.LAYOUT_NAMES[layout], w, h, pitch, rows)
            for off_in in range(16):
                for off_out in range(16):
                    got = guarded.run(ctx, lambda a, b: ctx.yuv_to_gray8_dev(a, b, w, h, 2, layout, pitch, rows), buf,
                                      y[:2], off_in=off_in, off_out=off_out, tag=tag)
                    guarded.check(got, y[:2], tag="%s in+%d out+%d" % (tag, off_in, off_out))


# ---- realistic shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pitch,rows,layout,std", [(1920, 1080, 2048, 1088, yr.NV12, yr.BT709),
                                                       (3840, 2160, 0, 0, yr.I420, yr.BT601),
                                                       (64, 4096, 0, 0, yr.YUY2, yr.BT601_FULL),
                                                       (64, 4096, 0, 0, yr.NV21, yr.BT601)],
                         ids=["1080p_decoder_surface", "4k_tight", "64x4096_yuy2", "64x4096_nv21"])
def test_realistic_shapes(arena, w, h, pitch, rows, layout, std):
    packed = yr.is_packed(layout)
    planes = yc.noise_planes(w, h, packed, 3)
    planes = (planes[0],) + yc.legal_planes(w, h, packed, 4)[1:]      # noise luma over legal chroma: both kinds of pixel
    buf = yr.pack(planes, layout, pitch, rows, yc.padding(yr.frame_bytes(layout, w, h, pitch, rows), 1))
    got = _decode(arena, buf, w, h, 1, layout, std, pitch, rows)
    want = yr.decode_planes(*planes, std)
    assert np.array_equal(got[0], want)
    assert np.array_equal(_luma(arena, buf, w, h, 1, layout, pitch, rows)[0], planes[0])
    if not packed:
        before = yc.padding(buf.size, 2)[None]
        back = _encode(arena, want[None], layout, std, pitch, rows, before)
        assert np.array_equal(back[0], yr.pack(yr.encode_planes(want, std), layout, pitch, rows, before[0]))


# ---- chains ----------------------------------------------------------------------------------------------------------
def test_decode_gauss_encode_on_the_device_equals_the_chain_through_the_reference(ctx, pkg):
    w, h, n, k, sigma = 250, 130, 2, 5, 1.5
    pitch, rows = 256, 136
    contents, ref, _ = _decode_case(w, h, False)
    buf = yc.pack_batch(contents[:n], yr.NV12, pitch, rows)
    blurred = ctx.gauss(ref[yr.BT601][:n], k, sigma)                   # the filter's own host path
    want = yr.encode(blurred, yr.NV12, yr.BT601, pitch, rows, fill=0)
    d_yuv, d_a, d_b, d_out = ctx.alloc(buf.size), ctx.alloc(n * w * h * 4), ctx.alloc(n * w * h * 4), ctx.alloc(buf.size)
    try:
        ctx.h2d(d_yuv, buf)
        ctx.h2d(d_out, np.zeros(buf.size, np.uint8))
        ctx.yuv_to_rgba8_dev(d_yuv, d_a, w, h, n, yr.NV12, yr.BT601, pitch, rows)
        ctx.filter_dev(pkg.FILTER_GAUSS, d_a, d_b, w, h, n, k, sigma)
        ctx.rgba8_to_yuv_dev(d_b, d_out, w, h, n, yr.NV12, yr.BT601, pitch, rows)
        ctx.sync()
        got = np.empty_like(want)
        ctx.d2h(got, d_out)
        ctx.sync()
    finally:
        ctx.sync()
        for p in (d_yuv, d_a, d_b, d_out):
            ctx.free(p)
    assert np.array_equal(got, want)


def test_the_luma_planes_feed_a_gray8_filter(ctx, pkg):
    w, h, n = 250, 130, 3
    for layout, (pitch, rows) in ((yr.NV12, (256, 136)), (yr.UYVY, (503, 131))):
        contents, _, y = _decode_case(w, h, yr.is_packed(layout))
        buf = yc.pack_batch(contents, layout, pitch, rows)
        want = ctx.median_gray8(y, 3)
        d_yuv, d_y, d_out = ctx.alloc(buf.size), ctx.alloc(n * w * h), ctx.alloc(n * w * h)
        try:
            ctx.h2d(d_yuv, buf)
            ctx.yuv_to_gray8_dev(d_yuv, d_y, w, h, n, layout, pitch, rows)
            ctx.filter_dev(pkg.FILTER_MEDIAN_GRAY8, d_y, d_out, w, h, n, 3)
            ctx.sync()
            got = np.empty_like(want)
            ctx.d2h(got, d_out)
            ctx.sync()
        finally:
            ctx.sync()
            for p in (d_yuv, d_y, d_out):
                ctx.free(p)
        assert np.array_equal(got, want), layout


# ---- host-buffer calls -----------------------------------------------------------------------------------------------
def test_the_host_buffer_calls_equal_the_device_calls(ctx, arena, pkg):
    w, h = 66, 34
    for layout, pitch, rows in ((yr.NV12, 128, 40), (yr.I420, 0, 0), (yr.YUY2, 135, 34)):
        contents, ref, _ = _decode_case(w, h, yr.is_packed(layout))
        buf = yc.pack_batch(contents, layout, pitch, rows)
        dev = _decode(arena, buf, w, h, 3, layout, yr.BT709, pitch, rows)
        host, prof = ctx.yuv_to_rgba8(buf, w, h, layout, yr.BT709, pitch, rows, profile=True)
        assert np.array_equal(host, dev) and np.array_equal(host, ref[yr.BT709])
        assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5] and prof[5] > prof[0] > 0
        fb = yr.frame_bytes(layout, w, h, pitch, rows)
        assert np.array_equal(ctx.yuv_to_rgba8(buf[:fb], w, h, layout, yr.BT709, pitch, rows)[0], dev[0])
        if layout in ENCODE_LAYOUTS:
            rgba, _ = _encode_case(w, h)
            zeros = np.zeros((2, fb), np.uint8)
            dev = _encode(arena, rgba, layout, yr.BT601_FULL, pitch, rows, zeros)
            host, prof = ctx.rgba8_to_yuv(rgba, layout, yr.BT601_FULL, pitch, rows, profile=True)
            assert host.shape == (2, fb) and np.array_equal(host, dev)       # the padding of a host result is zero
            assert np.array_equal(host, _encode_want(w, h, layout, yr.BT601_FULL, pitch, rows, zeros))
            assert prof[0] <= prof[1] <= prof[2] <= prof[3] <= prof[4] <= prof[5] and prof[5] > prof[0] > 0
            assert np.array_equal(ctx.rgba8_to_yuv(rgba[1], layout, yr.BT601_FULL, pitch, rows), dev[1])


def test_the_host_buffer_calls_are_unsupported_under_bgr_input(ctx, pkg):
    contents, _, _ = _decode_case(18, 6, False)
    buf = yc.pack_batch(contents, yr.NV12, 0, 0)
    rgba, _ = _encode_case(18, 6)
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.yuv_to_rgba8(buf, 18, 6, yr.NV12)
        assert e.value.code == -4
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.rgba8_to_yuv(rgba, yr.NV12)
        assert e.value.code == -4
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
    assert ctx.yuv_to_rgba8(buf, 18, 6, yr.NV12).shape == (3, 6, 18, 4)


# ---- argument checks -------------------------------------------------------------------------------------------------
def test_argument_checks_of_the_device_calls(ctx, pkg):
    w, h = 16, 8
    fb = yr.frame_bytes(yr.NV12, w, h)
    base = ctx.alloc(64 * 1024)
    try:
        d_yuv, d_rgba, d_gray = base, base + 8192, base + 16384
        ctx.h2d(d_yuv, np.zeros(8192, np.uint8))
        ctx.h2d(d_rgba, np.zeros(8192, np.uint8))
        dec = lambda a, b, *t: ctx.yuv_to_rgba8_dev(a, b, *t)                          # noqa: E731
        enc = lambda a, b, *t: ctx.rgba8_to_yuv_dev(b, a, *t)                          # noqa: E731
        gray = lambda a, b, w, h, n, lay, std, p, r: ctx.yuv_to_gray8_dev(a, b, w, h, n, lay, p, r)  # noqa: E731
        ok = (w, h, 1, yr.NV12, yr.BT601, 0, 0)
        for fn, d_o, bpp in ((dec, d_rgba, 4), (enc, d_rgba, 4), (gray, d_gray, 1)):
            fn(d_yuv, d_o, *ok)
            fn(d_yuv + 3, d_o, *ok)                                                     # the YUV side: any alignment
            for a, b in ((0, d_o), (d_yuv, 0)):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(a, b, *ok)
                assert e.value.code == -1
            # in place and overlapping from either side, the YUV side counted with its own bytes
            for d_bad in (d_yuv, d_yuv + fb - 4, d_yuv - w * h * bpp + 4):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_yuv, d_bad, *ok)
                assert e.value.code == -1, d_bad - d_yuv
            for bad in ((15, h, 1, yr.NV12, 0, 0, 0), (w, 7, 1, yr.NV12, 0, 0, 0), (w, h, 1, yr.NV12, 0, 12, 0),
                        (w, h, 1, yr.I420, 0, 17, 0), (w, h, 1, yr.NV12, 0, 0, 6), (w, h, 1, yr.NV12, 0, 0, 9),
                        (w, h, 0, yr.NV12, 0, 0, 0), (0, h, 1, yr.NV12, 0, 0, 0), (w, h, 1, 6, 0, 0, 0),
                        (w, h, 1, -1, 0, 0, 0)):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_yuv, d_o, *bad)
                assert e.value.code == -1, bad
        for fn in (dec, enc):
            with pytest.raises(pkg.Mi355Error) as e:
                fn(d_yuv, d_rgba, w, h, 1, yr.NV12, 3, 0, 0)                            # unknown standard
            assert e.value.code == -1
            for off in (1, 2, 3):
                with pytest.raises(pkg.Mi355Error) as e:
                    fn(d_yuv, d_rgba + off, *ok)                                        # RGBA is dword-aligned
                assert e.value.code == -1, off
        gray(d_yuv, d_gray + 3, *ok)                                                    # gray8: any alignment
        # a pitched surface reaches further: tight it clears the output, pitched it overlaps it
        ctx.yuv_to_rgba8_dev(d_rgba - fb, d_rgba, w, h, 1, yr.NV12, 0, 0, 0)
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.yuv_to_rgba8_dev(d_rgba - fb, d_rgba, w, h, 1, yr.NV12, 0, 32, 0)
        assert e.value.code == -1
        for lay in (yr.YUY2, yr.UYVY):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.rgba8_to_yuv_dev(d_rgba, d_yuv, w, h, 1, lay, 0, 0, 0)
            assert e.value.code == -4
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


# ---- stream capture --------------------------------------------------------------------------------------------------
_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import yuv_cases as yc
import yuv_ref as yr
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
w, h, n, pitch, rows = 250, 130, 2, 256, 136
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    bufs = [yc.pack_batch(yc.decode_contents(w, h, False)[i:i + 2], yr.NV12, pitch, rows, seed=i) for i in (0, 1)]
    d_yuv = torch.from_numpy(bufs[0]).to(dev)
    o_rgba = torch.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
    o_gray = torch.zeros((n, h, w), dtype=torch.uint8, device=dev)
    o_yuv = torch.zeros(bufs[0].size, dtype=torch.uint8, device=dev)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):     # the first calls this context makes: nothing to size, nothing to wait for
        c.yuv_to_rgba8_dev(d_yuv.data_ptr(), o_rgba.data_ptr(), w, h, n, yr.NV12, yr.BT709, pitch, rows)
        c.yuv_to_gray8_dev(d_yuv.data_ptr(), o_gray.data_ptr(), w, h, n, yr.NV12, pitch, rows)
        c.rgba8_to_yuv_dev(o_rgba.data_ptr(), o_yuv.data_ptr(), w, h, n, yr.I420, yr.BT709, pitch, rows)
    for r in range(2):
        buf = bufs[1 - r]
        d_yuv.copy_(torch.from_numpy(buf).to(dev))
        o_rgba.zero_(); o_gray.zero_(); o_yuv.zero_()
        g.replay()
        s.synchronize()
        rgba = yr.decode(buf, w, h, yr.NV12, yr.BT709, pitch, rows)
        if not np.array_equal(o_rgba.cpu().numpy(), rgba): bad.append((r, "decode"))
        if not np.array_equal(o_gray.cpu().numpy(), yr.luma(buf, w, h, yr.NV12, pitch, rows)): bad.append((r, "luma"))
        if not np.array_equal(o_yuv.cpu().numpy(), yr.encode(rgba, yr.I420, yr.BT709, pitch, rows).ravel()): bad.append((r, "encode"))
    del g
    c.close()
print(bad)
"""


def test_the_three_device_calls_can_be_captured_into_a_hip_graph():
    """The calls allocate nothing and wait for nothing, from the first one on: they are captured into a hipGraph and
    replayed on new content.  Own process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
