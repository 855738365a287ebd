"""GPU suite (-m gpu): mi355_warp_affine_dev / mi355_warp_affine_batched, cv::warpAffine of RGBA and gray8 frames.

Every comparison is bit-identity against the CPU reference tests/warp_ref.py (the header's arithmetic in numpy):
NEAREST and LINEAR, BORDER_CONSTANT and BORDER_REPLICATE, forward and inverse-mapped matrices.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded  # noqa: E402
from test_gpu_median import constant, extremes, noise  # noqa: E402
from warp_ref import (CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, fixed_coords, inverse_of, rotation,  # noqa: E402
                      sample_rows, warp_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# The kernel's tiles, restated from csrc/kernels.hpp: one wave owns a tile of output pixels and decides per tile whether
# it runs without border tests.  A launch takes the wide tile (kWarpWideLanesLog2 = 4 lanes of 4 pixels, kWarpWideH rows)
# while |i3| * 64 <= kWarpWideMaxRows, the square tile (kWarpSquareLanesLog2 = 3, kWarpSquareH) otherwise.
WIDE, SQUARE, WIDE_MAX_ROWS = (64, 16), (32, 32), 3.0


def tile_of(m, flags):
    return WIDE if abs(inverse_of(m, flags)[3]) * 64.0 <= WIDE_MAX_ROWS else SQUARE


# (src w, src h, dst w, dst h): one pixel, fewer columns than a lane owns, ragged last lanes and tiles, more than one tile
# in each direction, a wide flat and a tall thin frame; then for each tile shape a dst one tile wide plus 1, two tiles high
# plus 1, exactly one tile (every matrix runs on every shape, so each tile shape meets each of them).
SHAPES = [(1, 1, 1, 1), (5, 3, 7, 2), (64, 48, 21, 16), (21, 16, 64, 48), (77, 41, 130, 19), (1023, 9, 640, 5),
          (3, 1000, 5, 700)]
for _tw, _th in (WIDE, SQUARE):
    SHAPES += [(80, 50, _tw + 1, 7), (50, 80, 9, 2 * _th + 1), (100, 60, _tw, _th)]
VALUES = (0, 0x80FF407F)
VARIANTS = [(bpp, i, b) for bpp in (4, 1) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)]
VARIANT_IDS = ["%s-%s-%s" % ("rgba" if bpp == 4 else "gray8", "linear" if i else "nearest",
                             "replicate" if b else "constant") for bpp, i, b in VARIANTS]
BPP_INTERP = [(bpp, i) for bpp in (4, 1) for i in (NEAREST, LINEAR)]
BPP_INTERP_IDS = ["%s-%s" % ("rgba" if bpp == 4 else "gray8", "linear" if i else "nearest") for bpp, i in BPP_INTERP]


def one_bright_pixel(h, w, c, seed):
    img = np.zeros((h, w, c) if c > 1 else (h, w), np.uint8)
    img[(seed * 7) % h, (seed * 13) % w] = 255
    return img


CONTENTS = [noise, extremes, constant, one_bright_pixel]


def matrices(sw, sh):
    """The twelve matrices of a source shape; each runs inverse-mapped and forward."""
    cx, cy = (sw - 1) / 2.0, (sh - 1) / 2.0
    return [("identity", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
            ("shift+3-2", [1.0, 0.0, 3.0, 0.0, 1.0, -2.0]),
            ("shift.5.25", [1.0, 0.0, 0.5, 0.0, 1.0, 0.25]),
            ("rot7", rotation(cx, cy, 7.0)), ("rot30", rotation(cx, cy, 30.0)),
            ("rot90", rotation(cx, cy, 90.0)), ("rot180", rotation(cx, cy, 180.0)),
            ("shear", [2.3, 0.4, -5.0, -0.2, 0.45, 3.0]),
            ("flip", [-1.0, 0.0, float(sw - 1), 0.0, 1.0, 0.0]),
            ("singular", [1.0, 2.0, 3.0, 2.0, 4.0, 5.0]),
            ("outside", [1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0]),
            # inverse-mapped, output column 1 samples sx = src_w - 1 with fx = 16: its right tap is the seam sx + 1 == src_w
            ("seam", [1.0, 0.0, sw - 1.5, 0.0, 1.0, 0.0])]


def interior_tiles(m, sw, sh, dw, dh, flags):
    """(tiles whose taps all lie inside the frame, tiles) from the reference's coordinates."""
    X, Y = fixed_coords(m, dw, dh, flags)
    sx, sy = X >> 10, Y >> 10
    reach = 1 if (flags & ~INVERSE_MAP) == LINEAR else 0
    inside = (sx >= 0) & (sx + reach <= sw - 1) & (sy >= 0) & (sy + reach <= sh - 1)
    tw, th = tile_of(m, flags)
    n = k = 0
    for y0 in range(0, dh, th):
        for x0 in range(0, dw, tw):
            n += 1
            k += bool(inside[y0:y0 + th, x0:x0 + tw].all())
    return k, n


def _run(ctx, bpp, img, m, dw, dh, flags, border, value):
    if bpp == 4:
        return ctx.warp_affine(img, m, dw, dh, flags, border, value)
    return ctx.warp_affine_gray8(img, m, dw, dh, flags, border, value)


@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=VARIANT_IDS)
def test_warp_is_bit_identical_to_the_cpu_reference(ctx, bpp, interp, border):
    ran = all_interior = none_interior = 0
    tiles_seen = set()
    for sw, sh, dw, dh in SHAPES:
        frames = np.stack([make(sh, sw, bpp, sw * 31 + sh + dw) for make in CONTENTS])
        for name, m in matrices(sw, sh):
            for inv in (INVERSE_MAP, 0):
                flags = interp | inv
                k, n = interior_tiles(m, sw, sh, dw, dh, flags)
                tiles_seen.add(tile_of(m, flags))
                all_interior += k == n
                none_interior += k == 0
                for value in VALUES:
                    got = _run(ctx, bpp, frames, m, dw, dh, flags, border, value)
                    for f, make in enumerate(CONTENTS):
                        ref = warp_ref(frames[f], m, dw, dh, flags, border, value)
                        assert got[f].shape == ref.shape and np.array_equal(got[f], ref), (
                            (sw, sh, dw, dh), name, inv, hex(value), make.__name__)
                        ran += 1
    assert ran == len(SHAPES) * 12 * 2 * len(VALUES) * len(CONTENTS) == 2496 and tiles_seen == {WIDE, SQUARE}
    # neither the interior path nor the general path goes untested
    assert all_interior >= 1 and none_interior >= 1, (all_interior, none_interior)


@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=VARIANT_IDS)
def test_interior_and_general_tiles_agree(ctx, bpp, interp, border):
    """A turn about the centre by 30 degrees (square tiles) and by 2 degrees (wide tiles): the middle tiles run the interior
    path, the tiles that reach over the frame's edges the general one, and every row equals the reference."""
    sw, sh, dw, dh = 300, 200, 300, 200
    img = noise(sh, sw, bpp, 11)
    for angle, tile in ((30.0, SQUARE), (2.0, WIDE)):
        m = rotation((sw - 1) / 2.0, (sh - 1) / 2.0, angle)
        assert tile_of(m, interp) == tile
        k, n = interior_tiles(m, sw, sh, dw, dh, interp)
        assert 0 < k < n, (angle, k, n)
        for value in VALUES:
            got = _run(ctx, bpp, img, m, dw, dh, interp, border, value)
            assert np.array_equal(got, warp_ref(img, m, dw, dh, interp, border, value)), (angle, hex(value))


@pytest.mark.parametrize("bpp,interp,border", VARIANTS, ids=VARIANT_IDS)
def test_tile_grids_with_a_one_pixel_ragged_edge(ctx, bpp, interp, border):
    """The work-item decode at its smallest: one ragged tile alone in a frame (5 x 3, on either tile shape), and a 2 x 2
    grid of tiles whose second column and second row hold one pixel each, on the square tile (33 x 33 under a turn by 30
    degrees) and on the wide tile (65 x 17 under the identity).  Three frames, so that tile column, tile row and frame
    each show up in the output when one is taken for another."""
    sw, sh = 70, 40
    frames = np.stack([noise(sh, sw, bpp, 21), extremes(sh, sw, bpp, 22), noise(sh, sw, bpp, 23)])
    # inverse-mapped: the identity, and a turn by 30 degrees that starts inside the source and leaves it within 33 rows
    identity, turn = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.866, -0.5, 20.0, 0.5, 0.866, 10.0]
    flags = interp | INVERSE_MAP
    for (dw, dh), m, tile in (((5, 3), identity, WIDE), ((5, 3), turn, SQUARE), ((33, 33), turn, SQUARE),
                              ((65, 17), identity, WIDE)):
        assert tile_of(m, flags) == tile
        assert (dw, dh) == (5, 3) or (dw, dh) == (tile[0] + 1, tile[1] + 1)
        got = _run(ctx, bpp, frames, m, dw, dh, flags, border, 0x80FF407F)
        for f in range(3):
            assert np.array_equal(got[f], warp_ref(frames[f], m, dw, dh, flags, border, 0x80FF407F)), ((dw, dh), f)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_frames_are_independent(ctx, bpp, interp):
    """Three frames of different content equal three single-frame calls, and on frames that alternate between 0 and 255
    no output pixel mixes in a neighbouring frame, although the turned frame reaches over every edge."""
    for sw, sh, dw, dh in ((77, 41, 130, 19), (21, 16, 64, 48)):
        m = rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)
        frames = np.stack([noise(sh, sw, bpp, 5), extremes(sh, sw, bpp, 6), one_bright_pixel(sh, sw, bpp, 7)])
        for border in (CONSTANT, REPLICATE):
            got = _run(ctx, bpp, frames, m, dw, dh, interp, border, 0x80FF407F)
            for f in range(3):
                assert np.array_equal(got[f], _run(ctx, bpp, frames[f], m, dw, dh, interp, border, 0x80FF407F)), f
                assert np.array_equal(got[f], warp_ref(frames[f], m, dw, dh, interp, border, 0x80FF407F)), f
        flat = np.zeros((6,) + frames.shape[1:], np.uint8)
        flat[1::2] = 255
        out_shape = (6, dh, dw, 4) if bpp == 4 else (6, dh, dw)
        want = np.zeros(out_shape, np.uint8)
        want[1::2] = 255
        assert np.array_equal(_run(ctx, bpp, flat, m, dw, dh, interp, REPLICATE, 0x80FF407F), want), (sw, sh)
        # CONSTANT with the value equal to a frame's own colour: those frames stay flat
        assert np.array_equal(_run(ctx, bpp, flat, m, dw, dh, interp, CONSTANT, 0)[0::2], want[0::2]), (sw, sh)
        assert np.array_equal(_run(ctx, bpp, flat, m, dw, dh, interp, CONSTANT, 0xFFFFFFFF)[1::2], want[1::2]), (sw, sh)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=BPP_INTERP_IDS)
def test_guarded_arena(ctx, bpp, interp):
    """No guard byte changes and no payload byte is left unwritten, at every pointer alignment the call accepts.  The
    input lies in noise, so a tap read outside the frame and used shows up as a mismatch."""
    offs_in = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3)
    offs_out = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3, 5, 15)
    ran = 0
    for sw, sh, dw, dh in ((77, 41, 130, 19), (1023, 9, 640, 5)):
        img = noise(sh, sw, bpp, sw + dh)
        for name, m in (("rot30", rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)),
                        ("outside", [1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0])):
            for border in (CONSTANT, REPLICATE):
                ref = warp_ref(img, m, dw, dh, interp, border, 0x80FF407F)
                for off_in in offs_in:
                    for off_out in offs_out:
                        tag = "%s bpp %d interp %d border %d %dx%d->%dx%d" % (name, bpp, interp, border, sw, sh, dw, dh)
                        got = guarded.run(ctx, lambda a, b: ctx.warp_affine_dev(a, b, bpp, sw, sh, dw, dh, 1, m, interp,
                                                                                border, 0x80FF407F),
                                          img, ref, off_in=off_in, off_out=off_out, tag=tag)
                        guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
                        ran += 1
    assert ran == 2 * 2 * 2 * len(offs_in) * len(offs_out)


@pytest.mark.parametrize("bpp", (4, 1), ids=("rgba", "gray8"))
def test_large_frames_on_sampled_rows(ctx, bpp):
    sw, sh = 3840, 2160
    img = noise(sh, sw, bpp, 4)
    img[sh // 2:sh // 2 + 100, sw // 3:sw // 3 + 300] = 200
    cases = ((rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0), 3840, 2160, CONSTANT),
             ([0.5, 0.0, 0.0, 0.0, 0.5, 0.0], 1920, 1080, REPLICATE))
    for m, dw, dh, border in cases:
        got = _run(ctx, bpp, img, m, dw, dh, LINEAR, border, 0)
        rows = sample_rows(dh)
        assert np.array_equal(got[rows], warp_ref(img, m, dw, dh, LINEAR, border, 0, rows=rows)), (dw, dh)


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
from test_gpu_median import noise
from warp_ref import warp_ref, rotation
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
sw, sh, dw, dh = 201, 123, 150, 97
m = rotation(100.0, 61.0, 30.0)
bad = []
with torch.cuda.stream(s):
    c = pkg.Context(0, stream=s.cuda_stream)
    for bpp in (4, 1):
        frames = [noise(sh, sw, bpp, 91), noise(sh, sw, bpp, 92)]
        d_in = torch.from_numpy(frames[0]).to(dev)
        d_out = torch.zeros((dh, dw, 4) if bpp == 4 else (dh, dw), dtype=torch.uint8, device=dev)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):      # the first warp call this context ever makes is the captured one
            c.warp_affine_dev(d_in.data_ptr(), d_out.data_ptr(), bpp, sw, sh, dw, dh, 1, m, pkg.INTERP_LINEAR,
                              pkg.BORDER_CONSTANT, 0x80FF407F)
        for n, f in enumerate(frames):
            d_in.copy_(torch.from_numpy(f).to(dev))
            d_out.zero_()
            g.replay()
            s.synchronize()
            if not np.array_equal(d_out.cpu().numpy(), warp_ref(f, m, dw, dh, 1, 0, 0x80FF407F)): bad.append((bpp, n))
        del g
    c.close()
print(bad)
"""


def test_device_call_can_be_captured_from_the_first_call_on():
    """mi355_warp_affine_dev allocates nothing, waits for nothing and has no table, so the first call a fresh context
    makes can be the captured one: one launch in a linear graph, replayed on the captured frame and on new content.  Own
    process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]


def test_rejections_and_bgr_input(ctx, pkg):
    sw, sh, dw, dh = 16, 8, 32, 16                              # in: 512 B (RGBA), out: 2048 B
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    base = ctx.alloc(8192)
    try:
        ctx.h2d(base, noise(sh, sw, 4, 1))
        for bpp in (4, 1):
            nin, nout = sw * sh * bpp, dw * dh * bpp
            for flags in (NEAREST, LINEAR | INVERSE_MAP):
                # in place; the output starts inside the input; only the larger (output) side reaches over the input
                for d_in, d_out in ((base, base), (base, base + nin - 4), (base + nout - 4, base),
                                    (base + 4096, base + 4096 + nin - 4), (base + nout // 2, base)):
                    with pytest.raises(pkg.Mi355Error) as e:
                        ctx.warp_affine_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, ident, flags)
                    assert e.value.code == -1, (bpp, flags, d_in - base, d_out - base)
                ctx.warp_affine_dev(base, base + nin, bpp, sw, sh, dw, dh, 1, ident, flags)   # touching ranges are fine
                ctx.warp_affine_dev(base + nout, base, bpp, sw, sh, dw, dh, 1, ident, flags)
        for a, b in ((base + 1, base + 4096), (base, base + 4098), (base + 2, base + 4099)):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.warp_affine_dev(a, b, 4, sw, sh, dw, dh, 1, ident, LINEAR)
            assert e.value.code == -1, (a - base, b - base)
            ctx.warp_affine_dev(a, b, 1, sw, sh, dw, dh, 1, ident, LINEAR)                    # gray8 takes any alignment
        for flags in (3, 2, 32 | LINEAR):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.warp_affine_dev(base, base + 4096, 4, sw, sh, dw, dh, 1, ident, flags)
            assert e.value.code == -1, flags
        with pytest.raises(pkg.Mi355Error) as e:
            ctx.warp_affine_dev(base, base + 4096, 4, sw, sh, dw, dh, 1, [1.0, 0.0, 2.0e6, 0.0, 1.0, 0.0], LINEAR)
        assert e.value.code == -4
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    m = rotation(66.0, 48.0, 30.0)
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for flags, border in ((NEAREST, CONSTANT), (LINEAR, REPLICATE), (LINEAR | INVERSE_MAP, CONSTANT)):
            assert np.array_equal(ctx.warp_affine(bgr, m, 150, 80, flags, border, 0x80FF407F),
                                  warp_ref(rgba, m, 150, 80, flags, border, 0x80FF407F)), flags
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.warp_affine_gray8(bgr[..., 0], m, 150, 80, flags, border)
            assert e.value.code == -4, flags
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
    out, prof = ctx.warp_affine(rgba, m, 150, 80, profile=True)
    assert np.array_equal(out, warp_ref(rgba, m, 150, 80, LINEAR, CONSTANT, 0)) and len(prof) == 6
    assert all(prof[i] <= prof[i + 1] for i in range(5)) and prof[5] > prof[0], prof
