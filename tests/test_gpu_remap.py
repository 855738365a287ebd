"""GPU suite (-m gpu): mi355_remap_* and mi355_warp_perspective_*, cv::remap and cv::warpPerspective of RGBA and gray8
frames.

Every comparison is bit-identity against the CPU reference tests/remap_ref.py (the header's arithmetic in numpy): both
map kinds, NEAREST and LINEAR, BORDER_CONSTANT and BORDER_REPLICATE, forward and inverse-mapped homographies.  The
shapes, maps and matrices come from tests/remap_cases.py; tests/test_remap_cpu.py shows on the reference's coordinates
that they reach the cases they are there for.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded  # noqa: E402
import remap_cases as cases  # noqa: E402
from remap_ref import (FIXED, FLOAT, convert_maps, interior_passes, map_coords, perspective_coords, remap_ref,  # noqa: E402
                       sample)
from test_gpu_median import constant, extremes, noise  # noqa: E402
from test_gpu_warp import one_bright_pixel  # noqa: E402
from warp_ref import CONSTANT, INVERSE_MAP, LINEAR, NEAREST, REPLICATE, rotation, sample_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONTENTS = [noise, extremes, constant, one_bright_pixel]
VALUES = cases.VALUES
KIND_NAME = {FIXED: "fixed", FLOAT: "float"}


def _id(bpp, interp, border=None, kind=None):
    parts = ["rgba" if bpp == 4 else "gray8", "linear" if interp else "nearest"]
    if border is not None:
        parts.append("replicate" if border else "constant")
    if kind is not None:
        parts.append(KIND_NAME[kind])
    return "-".join(parts)


REMAP_VARIANTS = [(bpp, i, b, k) for bpp in (4, 1) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)
                  for k in (FIXED, FLOAT)]
WARP_VARIANTS = [(bpp, i, b) for bpp in (4, 1) for i in (NEAREST, LINEAR) for b in (CONSTANT, REPLICATE)]
BPP_INTERP = [(bpp, i) for bpp in (4, 1) for i in (NEAREST, LINEAR)]
BPP_INTERP_KIND = [(bpp, i, k) for bpp, i in BPP_INTERP for k in (FIXED, FLOAT)]


def _remap(ctx, bpp, img, map1, map2, kind, interp, border, value):
    dh, dw = np.asarray(map1).shape[:2]
    fn = ctx.remap if bpp == 4 else ctx.remap_gray8
    return fn(img, map1, map2, dw, dh, kind, interp, border, value)


def _perspective(ctx, bpp, img, m, dw, dh, flags, border, value):
    fn = ctx.warp_perspective if bpp == 4 else ctx.warp_perspective_gray8
    return fn(img, m, dw, dh, flags, border, value)


def _contents(sw, sh, dw, bpp):
    return np.stack([make(sh, sw, bpp, sw * 31 + sh + dw) for make in CONTENTS])


@pytest.mark.parametrize("bpp,interp,border,kind", REMAP_VARIANTS, ids=[_id(*v) for v in REMAP_VARIANTS])
def test_remap_is_bit_identical_to_the_cpu_reference(ctx, bpp, interp, border, kind):
    ran = interior = general = 0
    for sw, sh, dw, dh in cases.SHAPES:
        frames = _contents(sw, sh, dw, bpp)
        for name, map1, map2 in cases.remap_maps(sw, sh, dw, dh, kind, interp):
            coords = map_coords(map1, map2, kind, interp)
            k, n = interior_passes(coords, sw, sh, interp, cases.TILE, cases.LANE_ROWS)
            interior, general = interior + k, general + n - k
            for value in VALUES:
                got = _remap(ctx, bpp, frames, map1, map2, kind, interp, border, value)
                for f, make in enumerate(CONTENTS):
                    ref = sample(frames[f], coords, interp, border, value)
                    assert got[f].shape == ref.shape and np.array_equal(got[f], ref), (
                        (sw, sh, dw, dh), name, hex(value), make.__name__)
                    ran += 1
    assert ran == len(cases.SHAPES) * 5 * len(VALUES) * len(CONTENTS) == 360
    # neither the path without border tests nor the general path goes untested
    assert interior >= 1 and general >= 1, (interior, general)


def test_fixed_nearest_takes_no_second_map(ctx):
    sw, sh, dw, dh = 77, 41, 130, 19
    map1, map2 = cases.affine_fixed_maps(rotation(38.0, 20.0, 30.0), dw, dh, NEAREST)
    for bpp in (4, 1):
        img = noise(sh, sw, bpp, 3)
        got = _remap(ctx, bpp, img, map1, None, FIXED, NEAREST, CONSTANT, 0x80FF407F)
        assert np.array_equal(got, remap_ref(img, map1, None, FIXED, NEAREST, CONSTANT, 0x80FF407F))


AFFINE = [("rot7", lambda sw, sh: rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 7.0)),
          ("rot30", lambda sw, sh: rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)),
          ("shear", lambda sw, sh: [2.3, 0.4, -5.0, -0.2, 0.45, 3.0]),
          ("seam", lambda sw, sh: [1.0, 0.0, sw - 1.5, 0.0, 1.0, 0.0])]


@pytest.mark.parametrize("bpp,interp,border", WARP_VARIANTS, ids=[_id(*v) for v in WARP_VARIANTS])
def test_affine_maps_equal_the_affine_kernel(ctx, bpp, interp, border):
    """FIXED maps holding an affine matrix's coordinates give what mi355_warp_affine gives on the GPU, bit for bit; and
    FLOAT maps give what their convert_maps() form gives under FIXED."""
    ran = 0
    for sw, sh, dw, dh in ((64, 48, 21, 16), (77, 41, 130, 19), (80, 50, cases.TILE[0] + 1, 7)):
        img = noise(sh, sw, bpp, sw + dh)
        warp = ctx.warp_affine if bpp == 4 else ctx.warp_affine_gray8
        for name, make in AFFINE:
            m = make(sw, sh)
            for inv in (INVERSE_MAP, 0):
                map1, map2 = cases.affine_fixed_maps(m, dw, dh, interp | inv)
                for value in VALUES:
                    want = warp(img, m, dw, dh, interp | inv, border, value)
                    got = _remap(ctx, bpp, img, map1, map2, FIXED, interp, border, value)
                    assert np.array_equal(got, want), ((sw, sh, dw, dh), name, inv, hex(value))
                    ran += 1
            mx, my = cases.affine_float_maps(m, dw, dh)
            c1, c2 = convert_maps(mx, my, interp)
            got = _remap(ctx, bpp, img, mx, my, FLOAT, interp, border, 0x80FF407F)
            assert np.array_equal(got, _remap(ctx, bpp, img, c1, c2, FIXED, interp, border, 0x80FF407F)), name
            assert np.array_equal(got, remap_ref(img, mx, my, FLOAT, interp, border, 0x80FF407F)), name
    assert ran == 3 * 4 * 2 * len(VALUES)


@pytest.mark.parametrize("bpp,interp,border", WARP_VARIANTS, ids=[_id(*v) for v in WARP_VARIANTS])
def test_perspective_is_bit_identical_to_the_cpu_reference(ctx, bpp, interp, border):
    ran = interior = general = 0
    for sw, sh, dw, dh in cases.SHAPES:
        frames = _contents(sw, sh, dw, bpp)
        for name, m in cases.homographies(sw, sh):
            for inv in (INVERSE_MAP, 0):
                flags = interp | inv
                coords = perspective_coords(m, dw, dh, flags)
                k, n = interior_passes(coords, sw, sh, interp, cases.TILE, cases.LANE_ROWS)
                interior, general = interior + k, general + n - k
                for value in VALUES:
                    got = _perspective(ctx, bpp, frames, m, dw, dh, flags, border, value)
                    for f, make in enumerate(CONTENTS):
                        ref = sample(frames[f], coords, interp, border, value)
                        assert got[f].shape == ref.shape and np.array_equal(got[f], ref), (
                            (sw, sh, dw, dh), name, inv, hex(value), make.__name__)
                        ran += 1
    assert ran == len(cases.SHAPES) * 8 * 2 * len(VALUES) * len(CONTENTS) == 1152
    assert interior >= 1 and general >= 1, (interior, general)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=[_id(*v) for v in BPP_INTERP])
def test_tile_grids_with_a_one_pixel_ragged_edge(ctx, bpp, interp):
    """The work-item decode at its smallest: one ragged tile alone in a frame (5 x 3), and a 2 x 2 grid of tiles whose
    second column and second row hold one pixel each (33 x 33), from every coordinate source.  Five frames: one whole
    chunk of frames and a ragged one, so that tile column, tile row and chunk each show up in the output when one is
    taken for another."""
    sw, sh = 40, 36
    assert cases.FRAMES_PER_ITEM == 4
    frames = np.stack([noise(sh, sw, bpp, 31 + f) for f in range(5)])
    for dw, dh in ((5, 3), (cases.TILE[0] + 1, cases.TILE[1] + 1)):
        assert (dw, dh) in ((5, 3), (33, 33))
        for border in (CONSTANT, REPLICATE):
            for kind in (FIXED, FLOAT):
                for name, map1, map2 in cases.remap_maps(sw, sh, dw, dh, kind, interp)[:3]:
                    coords = map_coords(map1, map2, kind, interp)
                    got = _remap(ctx, bpp, frames, map1, map2, kind, interp, border, 0x80FF407F)
                    for f in range(5):
                        assert np.array_equal(got[f], sample(frames[f], coords, interp, border, 0x80FF407F)), (
                            (dw, dh), KIND_NAME[kind], name, f)
            for name, m in cases.homographies(sw, sh)[2:4]:
                coords = perspective_coords(m, dw, dh, interp)
                got = _perspective(ctx, bpp, frames, m, dw, dh, interp, border, 0x80FF407F)
                for f in range(5):
                    assert np.array_equal(got[f], sample(frames[f], coords, interp, border, 0x80FF407F)), (
                        (dw, dh), name, f)


def _sources(sw, sh, dw, dh, interp):
    """One runner per coordinate source: (name, run(ctx, bpp, frames, border, value), coords)."""
    rot30 = rotation((sw - 1) / 2.0, (sh - 1) / 2.0, 30.0)
    f1, f2 = cases.affine_fixed_maps(rot30, dw, dh, interp)
    bx, by = cases.barrel_float_maps(sw, sh, dw, dh)
    return [("fixed", lambda c, bpp, fr, b, v: _remap(c, bpp, fr, f1, f2, FIXED, interp, b, v),
             map_coords(f1, f2, FIXED, interp)),
            ("float", lambda c, bpp, fr, b, v: _remap(c, bpp, fr, bx, by, FLOAT, interp, b, v),
             map_coords(bx, by, FLOAT, interp)),
            ("perspective", lambda c, bpp, fr, b, v: _perspective(c, bpp, fr, cases.KEYSTONE, dw, dh, interp, b, v),
             perspective_coords(cases.KEYSTONE, dw, dh, interp))]


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=[_id(*v) for v in BPP_INTERP])
def test_frames_are_independent(ctx, bpp, interp):
    """Batches of 3, 5 and (frames per work item) + 1 frames equal single-frame calls and the reference, and on frames
    that alternate between 0 and 255 no output pixel mixes in a neighbouring frame under REPLICATE."""
    makers = [noise, extremes, one_bright_pixel, constant, noise]
    for sw, sh, dw, dh in ((77, 41, 130, 19), (21, 16, 64, 48)):
        for name, run, coords in _sources(sw, sh, dw, dh, interp):
            for nfr in sorted({3, 5, cases.FRAMES_PER_ITEM + 1}):
                frames = np.stack([makers[f](sh, sw, bpp, 5 + f) for f in range(nfr)])
                for border in (CONSTANT, REPLICATE):
                    got = run(ctx, bpp, frames, border, 0x80FF407F)
                    assert got.shape[0] == nfr
                    for f in range(nfr):
                        assert np.array_equal(got[f], run(ctx, bpp, frames[f], border, 0x80FF407F)), (name, nfr, f)
                        assert np.array_equal(got[f], sample(frames[f], coords, interp, border, 0x80FF407F)), (name, nfr, f)
            flat = np.zeros((7,) + frames.shape[1:], np.uint8)
            flat[1::2] = 255
            want = np.zeros((7, dh, dw, 4) if bpp == 4 else (7, dh, dw), np.uint8)
            want[1::2] = 255
            assert np.array_equal(run(ctx, bpp, flat, REPLICATE, 0x80FF407F), want), (name, sw, sh)
            assert np.array_equal(run(ctx, bpp, flat, CONSTANT, 0)[0::2], want[0::2]), (name, sw, sh)
            assert np.array_equal(run(ctx, bpp, flat, CONSTANT, 0xFFFFFFFF)[1::2], want[1::2]), (name, sw, sh)


class _DeviceMaps:
    """Device copies of host maps at chosen pointer offsets, each in an allocation of its own between 256 bytes of seeded
    noise: an entry read outside the map and used shows up as a mismatch."""

    def __init__(self, ctx):
        self.ctx, self.raw, self.at = ctx, [], {}

    def put(self, key, arr, off):
        if (key, off) not in self.at:
            data = np.ascontiguousarray(arr).view(np.uint8).ravel()
            host = np.random.default_rng(len(self.raw) + 7).integers(0, 256, 256 + off + data.size + 256, dtype=np.uint8)
            host[256 + off:256 + off + data.size] = data
            raw = self.ctx.alloc(host.size + 256)
            self.raw.append(raw)
            base = (raw + 255) // 256 * 256
            self.ctx.h2d(base, host)
            self.at[(key, off)] = base + 256 + off
        return self.at[(key, off)]

    def free(self):
        self.ctx.sync()
        for raw in self.raw:
            self.ctx.free(raw)


@pytest.mark.parametrize("bpp,interp,kind", BPP_INTERP_KIND, ids=[_id(b, i, None, k) for b, i, k in BPP_INTERP_KIND])
def test_guarded_arena_remap(ctx, bpp, interp, kind):
    """No guard byte changes and no payload byte is left unwritten, at every pointer alignment the call accepts for the
    frames and for the maps.  Input and maps lie in noise."""
    offs_in = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3)
    offs_out = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3, 5, 15)
    offs_map = [(a, b) for a in (0, 4, 8, 12) for b in ((0, 2, 6) if kind == FIXED else (0, 4, 8, 12))]
    ran, seen = 0, set()
    maps = _DeviceMaps(ctx)
    try:
        for sw, sh, dw, dh in ((77, 41, 130, 19), (1023, 9, 640, 5)):
            img = noise(sh, sw, bpp, sw + dh)
            for name, map1, map2 in cases.remap_maps(sw, sh, dw, dh, kind, interp):
                if name not in ("rot30", "outside"):
                    continue
                for border in (CONSTANT, REPLICATE):
                    ref = remap_ref(img, map1, map2, kind, interp, border, 0x80FF407F)
                    for off_in in offs_in:
                        for off_out in offs_out:
                            o1, o2 = offs_map[ran % len(offs_map)]
                            seen.add((o1, o2))
                            d1 = maps.put((sw, name, 1), map1, o1)
                            d2 = maps.put((sw, name, 2), map2, o2)
                            tag = "%s bpp %d interp %d kind %d border %d %dx%d->%dx%d maps +%d +%d" % (
                                name, bpp, interp, kind, border, sw, sh, dw, dh, o1, o2)
                            got = guarded.run(ctx, lambda a, b: ctx.remap_dev(a, b, bpp, sw, sh, dw, dh, 1, d1, d2, kind,
                                                                              interp, border, 0x80FF407F),
                                              img, ref, off_in=off_in, off_out=off_out, tag=tag)
                            guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
                            ran += 1
    finally:
        maps.free()
    assert ran == 2 * 2 * 2 * len(offs_in) * len(offs_out) and seen == set(offs_map)


@pytest.mark.parametrize("bpp,interp", BPP_INTERP, ids=[_id(*v) for v in BPP_INTERP])
def test_guarded_arena_perspective(ctx, bpp, interp):
    offs_in = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3)
    offs_out = (0, 4, 8, 12) if bpp == 4 else (0, 1, 2, 3, 5, 15)
    ran = 0
    for sw, sh, dw, dh in ((77, 41, 130, 19), (1023, 9, 640, 5)):
        img = noise(sh, sw, bpp, sw + dh)
        for name, m in (("keystone", cases.KEYSTONE), ("outside", cases.embed([1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0]))):
            coords = perspective_coords(m, dw, dh, interp)
            for border in (CONSTANT, REPLICATE):
                ref = sample(img, coords, interp, border, 0x80FF407F)
                for off_in in offs_in:
                    for off_out in offs_out:
                        tag = "%s bpp %d interp %d border %d %dx%d->%dx%d" % (name, bpp, interp, border, sw, sh, dw, dh)
                        got = guarded.run(ctx, lambda a, b: ctx.warp_perspective_dev(a, b, bpp, sw, sh, dw, dh, 1, m,
                                                                                     interp, border, 0x80FF407F),
                                          img, ref, off_in=off_in, off_out=off_out, tag=tag)
                        guarded.check(got, ref, tag="%s off_in=%d off_out=%d" % (tag, off_in, off_out))
                        ran += 1
    assert ran == 2 * 2 * 2 * len(offs_in) * len(offs_out)


def test_large_frames_on_sampled_rows(ctx):
    sw, sh, dw, dh = 3840, 2160, 3840, 2160
    img = noise(sh, sw, 4, 4)
    img[sh // 2:sh // 2 + 100, sw // 3:sw // 3 + 300] = 200
    rows = sample_rows(dh)
    map1, map2 = convert_maps(*cases.barrel_float_maps(sw, sh, dw, dh), LINEAR)
    got = ctx.remap(img, map1, map2, dw, dh, FIXED, LINEAR, CONSTANT, 0x80FF407F)
    assert np.array_equal(got[rows], remap_ref(img, map1, map2, FIXED, LINEAR, CONSTANT, 0x80FF407F, rows=rows))
    del map1, map2
    m = cases.keystone_4k(sw, sh)
    got = ctx.warp_perspective(img, m, dw, dh, LINEAR, REPLICATE, 0)
    ref = sample(img, perspective_coords(m, dw, dh, LINEAR, rows=rows), LINEAR, REPLICATE, 0)
    assert np.array_equal(got[rows], ref)


_GRAPH_SCRIPT = r"""
import sys
import numpy as np
import torch                       # first: torch brings its own HIP runtime and must initialise it before the library loads
torch.cuda.init()
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as entry
import remap_cases as cases
from remap_ref import perspective_ref, remap_ref
from test_gpu_median import noise
pkg = entry.load_package()
dev = torch.device("cuda", 0)
s = torch.cuda.Stream(dev)
sw, sh, dw, dh = 201, 123, 150, 97
mx, my = cases.barrel_float_maps(sw, sh, dw, dh)
bad = []
with torch.cuda.stream(s):
    d_mx, d_my = torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev)
    for call in ("remap", "perspective"):
        c = pkg.Context(0, stream=s.cuda_stream)     # a fresh context: its first call is the captured one
        for bpp in (4, 1):
            frames = [noise(sh, sw, bpp, 91), noise(sh, sw, bpp, 92)]
            d_in = torch.from_numpy(frames[0]).to(dev)
            d_out = torch.zeros((dh, dw, 4) if bpp == 4 else (dh, dw), dtype=torch.uint8, device=dev)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                if call == "remap":
                    c.remap_dev(d_in.data_ptr(), d_out.data_ptr(), bpp, sw, sh, dw, dh, 1, d_mx.data_ptr(), d_my.data_ptr(),
                                pkg.MAP_FLOAT, pkg.INTERP_LINEAR, pkg.BORDER_CONSTANT, 0x80FF407F)
                else:
                    c.warp_perspective_dev(d_in.data_ptr(), d_out.data_ptr(), bpp, sw, sh, dw, dh, 1, cases.KEYSTONE,
                                           pkg.INTERP_LINEAR, pkg.BORDER_CONSTANT, 0x80FF407F)
            for n, f in enumerate(frames):
                d_in.copy_(torch.from_numpy(f).to(dev))
                d_out.zero_()
                g.replay()
                s.synchronize()
                ref = remap_ref(f, mx, my, 1, 1, 0, 0x80FF407F) if call == "remap" else \
                    perspective_ref(f, cases.KEYSTONE, dw, dh, 1, 0, 0x80FF407F)
                if not np.array_equal(d_out.cpu().numpy(), ref): bad.append((call, bpp, n))
            del g
        c.close()
print(bad)
"""


def test_device_calls_can_be_captured_from_the_first_call_on():
    """mi355_remap_dev and mi355_warp_perspective_dev allocate nothing, wait for nothing and have no table, so the first
    call a fresh context makes can be the captured one: one launch in a linear graph, replayed on the captured frame and
    on new content.  Own process: torch's HIP runtime has to initialise before the library is loaded."""
    out = subprocess.run([sys.executable, "-c", _GRAPH_SCRIPT, ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "[]", out.stdout[-2000:]


def test_rejections_and_bgr_input(ctx, pkg):
    sw, sh, dw, dh = 16, 8, 32, 16            # RGBA in: 512 B, out: 2048 B; maps: 2048 B (map1, FLOAT map2), 1024 B (FIXED map2)
    base = ctx.alloc(32768)
    try:
        ctx.h2d(base, np.zeros(32768, np.uint8))
        ctx.sync()
        d_in, d_out, d_m1, d_m2 = base + 4096, base + 8192, base + 16384, base + 24576
        ident = cases.embed([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])

        def bad(*a, **kw):
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.remap_dev(*a, **kw)
            assert e.value.code == -1, (a, kw)

        for bpp in (4, 1):
            nin, nout = sw * sh * bpp, dw * dh * bpp
            for kind in (FIXED, FLOAT):
                n2 = dw * dh * (2 if kind == FIXED else 4)
                ctx.remap_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, kind, LINEAR)
                # the output overlaps the input, map1, map2: by its first bytes and by its last
                for o in (d_in, d_in + nin - 4, d_in - nout + 4, d_m1 - nout + 4, d_m1 + 2048 - 4, d_m2 - nout + 4,
                          d_m2 + n2 - 4):
                    bad(d_in, o, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, kind, LINEAR)
                ctx.remap_dev(d_in, d_m1 - nout, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, kind, LINEAR)   # touching is fine
                ctx.remap_dev(d_in, d_m2 + n2, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, kind, LINEAR)
                # misaligned maps
                for o1 in (1, 2, 3):
                    bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1 + o1, d_m2, kind, LINEAR)
                for o2 in ((1, 3) if kind == FIXED else (1, 2, 3)):
                    bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, d_m2 + o2, kind, LINEAR)
                if kind == FIXED:
                    ctx.remap_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, d_m2 + 2, kind, LINEAR)
                # a missing map
                bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, 0, d_m2, kind, LINEAR)
                bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, 0, kind, LINEAR)
                if kind == FIXED:
                    ctx.remap_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, 0, kind, NEAREST)
                    ctx.remap_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, None, kind, NEAREST)
                else:
                    bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, 0, kind, NEAREST)
                for interp in (3, 2, LINEAR | INVERSE_MAP, -1):
                    bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, kind, interp)
            bad(d_in, d_out, bpp, sw, sh, dw, dh, 1, d_m1, d_m2, 2, LINEAR)
            # perspective: overlap, flags
            for a, b in ((d_in, d_in), (d_in, d_in + nin - 4), (d_in + nout - 4, d_in)):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.warp_perspective_dev(a, b, bpp, sw, sh, dw, dh, 1, ident, LINEAR)
                assert e.value.code == -1, (bpp, a - base, b - base)
            ctx.warp_perspective_dev(d_in, d_in + nin, bpp, sw, sh, dw, dh, 1, ident, LINEAR | INVERSE_MAP)
            for flags in (3, 2, 32 | LINEAR):
                with pytest.raises(pkg.Mi355Error) as e:
                    ctx.warp_perspective_dev(d_in, d_out, bpp, sw, sh, dw, dh, 1, ident, flags)
                assert e.value.code == -1, flags
        # RGBA pointers must be dword-aligned, gray8 takes any alignment
        for a, b in ((d_in + 1, d_out), (d_in, d_out + 2)):
            bad(a, b, 4, sw, sh, dw, dh, 1, d_m1, d_m2, FLOAT, LINEAR)
            ctx.remap_dev(a, b, 1, sw, sh, dw, dh, 1, d_m1, d_m2, FLOAT, LINEAR)
            with pytest.raises(pkg.Mi355Error) as e:
                ctx.warp_perspective_dev(a, b, 4, sw, sh, dw, dh, 1, ident, LINEAR)
            assert e.value.code == -1
            ctx.warp_perspective_dev(a, b, 1, sw, sh, dw, dh, 1, ident, LINEAR)
        ctx.sync()
    finally:
        ctx.sync()
        ctx.free(base)
    bgr = noise(97, 133, 3, 5)
    rgba = np.ascontiguousarray(np.dstack([bgr[..., 2], bgr[..., 1], bgr[..., 0], np.full(bgr.shape[:2], 255, np.uint8)]))
    mx, my = cases.barrel_float_maps(133, 97, 150, 80)
    ctx.set_input_format(pkg.INPUT_BGR)
    try:
        for interp, border in ((NEAREST, CONSTANT), (LINEAR, REPLICATE)):
            assert np.array_equal(ctx.remap(bgr, mx, my, 150, 80, FLOAT, interp, border, 0x80FF407F),
                                  remap_ref(rgba, mx, my, FLOAT, interp, border, 0x80FF407F)), interp
            assert np.array_equal(ctx.warp_perspective(bgr, cases.KEYSTONE, 150, 80, interp, border, 0x80FF407F),
                                  sample(rgba, perspective_coords(cases.KEYSTONE, 150, 80, interp), interp, border,
                                         0x80FF407F)), interp
            for call in (lambda: ctx.remap_gray8(bgr[..., 0], mx, my, 150, 80, FLOAT, interp, border),
                         lambda: ctx.warp_perspective_gray8(bgr[..., 0], cases.KEYSTONE, 150, 80, interp, border)):
                with pytest.raises(pkg.Mi355Error) as e:
                    call()
                assert e.value.code == -4, interp
    finally:
        ctx.set_input_format(pkg.INPUT_RGBA)
    out, prof = ctx.remap(rgba, mx, my, 150, 80, FLOAT, profile=True)
    assert np.array_equal(out, remap_ref(rgba, mx, my, FLOAT, LINEAR, CONSTANT, 0)) and len(prof) == 6
    assert all(prof[i] <= prof[i + 1] for i in range(5)) and prof[5] > prof[0], prof
    out, prof = ctx.warp_perspective(rgba, cases.KEYSTONE, 150, 80, profile=True)
    assert len(prof) == 6 and all(prof[i] <= prof[i + 1] for i in range(5)) and prof[5] > prof[0], prof
