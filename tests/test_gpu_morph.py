"""GPU suite (-m gpu): rectangular morphology, MI355_FILTER_ERODE / DILATE / OPEN / CLOSE (RGBA) and their *_GRAY8 forms.

Every output byte is an input byte, so every comparison here is bit-identity: against the CPU reference
tests/morph_ref.py (k x k rectangle, clamp-to-edge borders, every channel, alpha included; OPEN / CLOSE with the
intermediate frame's own clamped border), and between the one-launch OPEN / CLOSE and two single-stage calls.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
from median_ref import sample_rows  # noqa: E402
from morph_ref import OPS, morph_ref  # noqa: E402
from test_gpu_median import constant, extremes, impulses, noise, patches  # noqa: E402

pytestmark = pytest.mark.gpu

KS = tuple(range(3, 18, 2))
SHAPES = [(1, 1), (1, 45), (45, 1), (2, 3), (5, 7), (17, 17), (33, 19), (75, 75), (427, 640), (1023, 819)]


def one_bright_pixel(h, w, c, seed):
    img = np.zeros((h, w, c) if c > 1 else (h, w), np.uint8)
    img[(seed * 7) % h, (seed * 13) % w] = 255
    return img


CONTENTS = [noise, patches, extremes, constant, impulses, one_bright_pixel]


def _fid(pkg, op, gray8):
    return getattr(pkg, "FILTER_%s%s" % (op.upper(), "_GRAY8" if gray8 else ""))


def _run(ctx, op, gray8, img, k):
    name = op if op in ("erode", "dilate") else "morph_" + op  # Context.close() releases the context
    return getattr(ctx, name + ("_gray8" if gray8 else ""))(img, k)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
@pytest.mark.parametrize("op", OPS)
def test_morphology_is_bit_identical_to_the_cpu_reference(ctx, op, gray8):
    c = 1 if gray8 else 4
    for k in KS:
        for shape in SHAPES:
            for make in CONTENTS:
                img = make(shape[0], shape[1], c, shape[0] * 31 + shape[1] + k)
                got = _run(ctx, op, gray8, img, k)
                rows = sample_rows(shape[0], 2 * k) if shape[0] * shape[1] > 100000 else None
                ref = morph_ref(op, img, k, rows=rows)
                assert np.array_equal(got if rows is None else got[rows], ref), (op, k, shape, make.__name__)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_dilating_one_bright_pixel_gives_a_k_by_k_square(ctx, gray8):
    h, w = 61, 83
    c = 1 if gray8 else 4
    for k in KS:
        for y, x in ((30, 40), (0, 0), (h - 1, w - 1), (2, w - 3)):
            img = np.zeros((h, w, c) if c > 1 else (h, w), np.uint8)
            img[y, x] = 255
            want = np.zeros_like(img)
            r = k // 2
            want[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = 255
            assert np.array_equal(_run(ctx, "dilate", gray8, img, k), want), (k, y, x)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_morphology_of_a_4k_frame(ctx, gray8):
    c = 1 if gray8 else 4
    h, w = 2160, 3840
    img = noise(h, w, c, 4)
    img[1000:1100, 2000:2300] = 200
    for op in OPS:
        for k in (3, 9, 17):
            got = _run(ctx, op, gray8, img, k)
            rows = sample_rows(h, 2 * k)
            assert np.array_equal(got[rows], morph_ref(op, img, k, rows=rows)), (op, k)


def test_gray8_any_byte_alignment(ctx, pkg):
    n, h, w = 2, 41, 77
    ys = np.stack([noise(h, w, 1, s) for s in range(n)])
    nb = ys.nbytes
    base = ctx.alloc(2 * nb + 64)
    try:
        for op in OPS:
            for k in (3, 7, 17):
                ref = np.stack([morph_ref(op, y, k) for y in ys])
                for off_in in range(4):
                    off_out = (off_in * 3 + 1) % 4
                    d_in, d_out = base + off_in, base + nb + 32 + off_out
                    ctx.h2d(d_in, ys)
                    ctx.filter_dev(_fid(pkg, op, True), d_in, d_out, w, h, n, k, 0.0)
                    ctx.sync()
                    got = np.empty_like(ys)
                    ctx.d2h(got, d_out)
                    assert np.array_equal(got, ref), (op, k, off_in, off_out)
    finally:
        ctx.sync()
        ctx.free(base)


def test_gray8_is_the_r_channel_of_rgba(ctx):
    y = noise(123, 201, 1, 9)
    rgba = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
    for op in OPS:
        for k in (3, 11, 17):
            assert np.array_equal(_run(ctx, op, True, y, k), _run(ctx, op, False, rgba, k)[..., 0]), (op, k)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_one_launch_open_close_equal_two_calls(ctx, pkg, gray8):
    """The intermediate's border: OPEN from one call equals ERODE then DILATE from two calls, on frames whose edges
    differ from their interior (where a first stage extended past the edge would give other border pixels)."""
    n, h, w = 3, 70, 133
    c = 1 if gray8 else 4
    frames = np.stack([impulses(h, w, c, s) for s in range(n)])
    frames[:, :, :5] = 255
    frames[:, -3:] = 0
    nb = frames.nbytes
    base = ctx.alloc(3 * nb + 64)
    try:
        d_in, d_mid, d_out = base, base + nb, base + 2 * nb
        ctx.h2d(d_in, frames)
        for op, first, second in (("open", "erode", "dilate"), ("close", "dilate", "erode")):
            for k in KS:
                ctx.filter_dev(_fid(pkg, first, gray8), d_in, d_mid, w, h, n, k, 0.0)
                ctx.filter_dev(_fid(pkg, second, gray8), d_mid, d_out, w, h, n, k, 0.0)
                ctx.sync()
                two = np.empty_like(frames)
                ctx.d2h(two, d_out)
                one = _run(ctx, op, gray8, frames, k)
                assert np.array_equal(one, two), (op, k)
                assert np.array_equal(one, np.stack([morph_ref(op, f, k) for f in frames])), (op, k)
    finally:
        ctx.sync()
        ctx.free(base)


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_order_and_idempotence(ctx, gray8):
    c = 1 if gray8 else 4
    img = noise(97, 151, c, 3)
    for k in (3, 9, 17):
        ero, dil = _run(ctx, "erode", gray8, img, k), _run(ctx, "dilate", gray8, img, k)
        opn, cls = _run(ctx, "open", gray8, img, k), _run(ctx, "close", gray8, img, k)
        assert np.all(ero <= opn) and np.all(opn <= img) and np.all(img <= cls) and np.all(cls <= dil), k
        assert np.array_equal(_run(ctx, "open", gray8, opn, k), opn), k
        assert np.array_equal(_run(ctx, "close", gray8, cls, k), cls), k


@pytest.mark.parametrize("gray8", [False, True], ids=["rgba", "gray8"])
def test_frames_never_leak_into_each_other(ctx, gray8):
    n, h, w = 16, 48, 200
    frames = np.zeros((n, h, w) if gray8 else (n, h, w, 4), np.uint8)
    frames[1::2] = 255
    for op in OPS:
        for k in (3, 17):
            assert np.array_equal(_run(ctx, op, gray8, frames, k), frames), (op, k)


# ---- host paths -----------------------------------------------------------------------------------------------------
def test_batched_stream_and_pool(ctx, pkg):
    n, h, w = 5, 67, 129
    for gray8 in (False, True):
        c = 1 if gray8 else 4
        frames = np.stack([noise(h, w, c, s) for s in range(n)])
        for op in OPS:
            filt = _fid(pkg, op, gray8)
            for k in (3, 9, 17):
                ref = np.stack([morph_ref(op, f, k) for f in frames])
                assert np.array_equal(_run(ctx, op, gray8, frames, k), ref), (op, gray8, k)
                out, _ = ctx.stream(filt, frames, k=k, chunk_frames=2)  # pageable, ragged last chunk
                assert np.array_equal(out, ref), (op, gray8, k)
                pin_in, pin_out = ctx.pinned_empty(frames.shape), ctx.pinned_empty(frames.shape)
                try:
                    pin_in[...] = frames
                    ctx.stream(filt, pin_in, out=pin_out, k=k, chunk_frames=3)
                    assert np.array_equal(pin_out, ref), (op, gray8, k)
                finally:
                    ctx.pinned_free(pin_in)
                    ctx.pinned_free(pin_out)
            d_in, d_out, _ = ctx.pool_alloc(filt, w, h, n, k=5, sigma=float("nan"), tries=2)
            try:
                ctx.h2d(d_in, frames)
                ctx.filter_dev(filt, d_in, d_out, w, h, n, 5, 0.0)
                ctx.sync()
                got = np.empty_like(frames)
                ctx.d2h(got, d_out)
                assert np.array_equal(got, np.stack([morph_ref(op, f, 5) for f in frames])), (op, gray8)
            finally:
                ctx.pool_free(d_in, d_out)


def test_bgr_input(ctx, pkg):
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for op in OPS:
            for k in (3, 17):
                assert np.array_equal(_run(ctx, op, False, bgr, k), morph_ref(op, rgba, k)), (op, k)
            out, _ = ctx.stream(_fid(pkg, op, False), bgr[None].copy(), k=5)
            assert np.array_equal(out[0], morph_ref(op, rgba, 5)), op
            with pytest.raises(pkg.Mi355Error) as e:
                _run(ctx, op, True, bgr[..., 0], 3)
            assert e.value.code == -4, op
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)


@pytest.mark.parametrize("members", [1, 2, 3])
def test_group_on_one_gpu(pkg, members):
    n, h, w = 7, 53, 91
    rgba = np.stack([noise(h, w, 4, s) for s in range(n)])
    ys = np.stack([noise(h, w, 1, s + 50) for s in range(n)])
    with pkg.Group([0] * members) as g:
        for gray8, frames in ((False, rgba), (True, ys)):
            for op in OPS:
                filt = _fid(pkg, op, gray8)
                for k in (3, 17):
                    out, _ = g.filter_batched(filt, frames, k=k)
                    assert np.array_equal(out, np.stack([morph_ref(op, f, k) for f in frames])), (members, op, k)
                for bad in (-1, 0, 1, 2, 4, 18, 19, 65):
                    with pytest.raises(pkg.Mi355Error) as e:
                        g.filter_batched(filt, frames, k=bad)
                    assert e.value.code == -1, (filt, bad)
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
            g.filter_dev(pkg.FILTER_CLOSE, [b[0] for b in bufs], [b[1] for b in bufs], w, h, [s[1] for s in shards],
                         k=7)
            for i, (first, cnt) in enumerate(shards):
                if cnt:
                    got = np.empty_like(rgba[first:first + cnt])
                    mcs[i].d2h(got, bufs[i][1])
                    assert np.array_equal(got, np.stack([morph_ref("close", f, 7) for f in rgba[first:first + cnt]])), i
            for bad in (-1, 0, 2, 18, 65):
                with pytest.raises(pkg.Mi355Error) as e:
                    g.filter_dev(pkg.FILTER_CLOSE, [b[0] for b in bufs], [b[1] for b in bufs], w, h,
                                 [s[1] for s in shards], k=bad)
                assert e.value.code == -1, bad
        finally:
            for i, (d_in, d_out) in enumerate(bufs):
                mcs[i].free(d_in)
                mcs[i].free(d_out)


# ---- argument checks ------------------------------------------------------------------------------------------------
BAD_KS = (-1, 0, 1, 2, 4, 18, 19, 65)


def test_argument_checks(ctx, pkg):
    h, w = 8, 8
    base = ctx.alloc(4 * h * w * 3 + 64)
    try:
        d_in, d_out = base, base + 4 * h * w + 16
        ctx.h2d(d_in, noise(h, w, 4, 1))
        for gray8 in (False, True):
            for op in OPS:
                filt = _fid(pkg, op, gray8)
                shape = (1, h, w) if gray8 else (1, h, w, 4)
                for k in BAD_KS:
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.filter_dev(filt, d_in, d_out, w, h, 1, k, 0.0)
                    assert e.value.code == -1, (filt, k)
                    with pytest.raises(pkg.Mi355Error) as e:
                        if gray8:
                            ctx._host_gray8(filt, np.zeros(shape, np.uint8), k)
                        else:
                            ctx._host(filt, np.zeros(shape, np.uint8), k)
                    assert e.value.code == -1, (filt, k)
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.stream(filt, np.zeros(shape, np.uint8), k=k)
                    assert e.value.code == -1, (filt, k)
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.pool_alloc(filt, w, h, 1, k=k, sigma=0.0, tries=1)
                    assert e.value.code == -1, (filt, k)
                # in place and overlapping input and output
                for d_o in (d_in, d_in + 4, d_in + h * w - 4):
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.filter_dev(filt, d_in, d_o, w, h, 1, 3, 0.0)
                    assert e.value.code == -1, filt
                ctx.filter_dev(filt, d_in, d_out, w, h, 1, 3, float("nan"))  # sigma is ignored
        # RGBA needs dword-aligned pointers, in and out
        for op in OPS:
            for a, b in ((d_in + 1, d_out), (d_in, d_out + 2)):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.filter_dev(_fid(pkg, op, False), a, b, w, h, 1, 3, 0.0)
                assert e.value.code == -1, op
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from morph_ref import morph_ref
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
    o_open = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    o_ero = torch.zeros((h, w), dtype=torch.uint8, device=dev)

    def chain():
        c.filter_dev(pkg.FILTER_OPEN, d_rgba.data_ptr(), o_open.data_ptr(), w, h, 1, 9, 0.0)
        c.filter_dev(pkg.FILTER_ERODE_GRAY8, d_gray.data_ptr(), o_ero.data_ptr(), w, h, 1, 17, 0.0)

    chain()                             # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for n in range(2):
        d_rgba.copy_(torch.from_numpy(rgba[1 - n]).to(dev))
        d_gray.copy_(torch.from_numpy(gray[1 - n]).to(dev))
        o_open.zero_()
        o_ero.zero_()
        g.replay()
        s.synchronize()
        if not np.array_equal(o_open.cpu().numpy(), morph_ref("open", rgba[1 - n], 9)): bad.append((n, "open9"))
        if not np.array_equal(o_ero.cpu().numpy(), morph_ref("erode", gray[1 - n], 17)): bad.append((n, "erode17"))
    del g
    c.close()
print(bad)
"""


def test_device_resident_morphology_can_be_captured_into_a_hip_graph():
    """mi355_filter_dev with the morphology ids allocates nothing and synchronises nothing (there is no table), so a
    linear chain of them on one stream is captured into a hipGraph after a warm-up and replayed on new content."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, entry.ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]
