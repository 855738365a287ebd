"""Cases of the large-k Gaussian tests (test_large_k_cpu.py, test_gpu_large_k.py): window sizes 19 .. 63, which only the
runtime-k LDS-tiled kernels serve (gauss_tile.hip, sobel_tile.hip, gray8.hip) and, in image mode, the per-pixel kernel
of image2d.hip.  The LDS carve of those kernels grows with k, and gray8.hip chooses its arithmetic from
delta_bound_k(k, w1, w2) < 0.01; KS puts a size on each side of every threshold in that range.

Holds the sizes and sigmas, the frame shapes and their content, the three LDS carves restated term by term from the
sources (as test_gauss_tables_cpu.py restates delta_bound_k), and Report, the comparison helper of the GPU table tests.
A plain numpy helper for those tests, not a fixture module.
"""
import collections

import numpy as np

from test_gpu_gray8 import extremes as _extremes, hash_noise

KS = (19, 25, 27, 33, 45, 49, 57, 59, 63)
KS_WHY = {
    19: "the first size past every VALU and matrix-core kernel (gauss_slide <= 9, gauss_wide and gauss_mfma_reg <= 17)",
    25: "kImgMaxFastK: the last size of image mode's LDS-tiled kernel",
    27: "the first size of image mode's per-pixel kernel",
    33: "the first size above what the rest of the suite runs on every kernel (31)",
    45: "delta_bound_k crosses 0.01 between sigma 7.5 and 50: gray8's kGmExc and kGmTap in one test",
    49: "delta_bound_k crosses 0.01 between sigma 0.35 and 49 / 6: the last size kGmExc serves",
    57: "gauss_tile FAST carves 65,508 B: the last size inside the 64 KiB a kernel gets without asking",
    59: "gauss_tile FAST carves 67,580 B: the first launch that needs the raised dynamic-LDS limit",
    63: "MI355_MAX_GAUSS_K",
}
IMAGE_KS = (27, 33, 63)           # image mode: the per-pixel kernel takes every k >= 27

LDS_DEFAULT = 64 * 1024           # a kernel's dynamic LDS without hipFuncSetAttribute
LDS_WORKGROUP = 160 * 1024        # gfx950: LDS per workgroup

# delta_bound_k of a generated table is kept this far (relative) from gray8.hip's 0.01: the library evaluates the
# predicate in double on the host, and a restatement must not be asked to break a tie
DELTA_LIMIT = 0.01
DELTA_MARGIN = 0.02


def SIGMAS(k):
    """0.35: the centre tap alone, every sum next to an integer (dense exception flags).  k / 6: the ordinary table.
    50: a box within rounding; all k * k taps count, the CPU chain carries its largest accumulated rounding and
    delta_bound_k is at its largest."""
    return (0.35, k / 6.0, 50.0)


# ---- shapes (h, w, n) ------------------------------------------------------------------------------------------------
RGBA_TILE = (16, 64)              # tile_common.hpp: kRgbaTH x kRgbaTW
G8_TILE = (32, 256)               # gray8.hip: kG8TH x kG8TW
# 3 x 3 tiles, ragged on both axes, frame 1 starts 8 B off a 16-byte boundary; exactly one tile; smaller than the
# radius on both axes / one pixel / on one axis (w < 4 and h < 2 are the pipeline's per-pixel store forms)
RGBA_SHAPES = ((37, 150, 3), (16, 64, 1), (3, 5, 2), (1, 1, 1), (70, 9, 1))
RGBA_BIG = RGBA_SHAPES[0]
# 3 x 2 tiles, ragged on both axes; the same with an odd frame size, so that frame 1 starts at an odd byte; exactly one
# tile; one pixel; smaller than the radius on one axis
G8_SHAPES = ((70, 300, 2), (71, 301, 2), (32, 256, 1), (1, 1, 1), (5, 300, 1), (300, 5, 1))

PATCH = 70                        # flat patches of 70 x 70, wider than a 63 x 63 window ...
PERIOD = 80                       # ... with 10 rows / columns of noise between them


_STRIDE = 1000003                 # hash_noise adds the seed to the pixel index: seeds this far apart never overlap


def noise(h, w, seed):
    return hash_noise(h, w, seed * _STRIDE)


def extremes(h, w, seed):
    """0 or 255 per pixel: the largest steps, and sums that reach 255 * sum(table)."""
    return _extremes(h, w, seed * _STRIDE)


def patches(h, w, seed):
    """Flat PATCH x PATCH blocks, one value each, on a PERIOD grid with noise in the gaps (test_gpu_gray8's
    flat_patches has 64-pixel blocks and no gaps).  With clamp-to-edge taps a block that touches the frame's edge gives
    constant windows up to k = 63: the separable sum then sits within a few 1e-6 of an integer, which is where the
    exact-by-exception arithmetic takes its exception for every pixel."""
    out = noise(h, w, seed)
    vals = noise((h + PERIOD - 1) // PERIOD, (w + PERIOD - 1) // PERIOD, seed + 500)
    yy, xx = np.arange(h), np.arange(w)
    flat = ((yy % PERIOD) < PATCH)[:, None] & ((xx % PERIOD) < PATCH)[None, :]
    full = vals[yy // PERIOD][:, xx // PERIOD]
    out[flat] = full[flat]
    return out


CONTENT = (noise, patches, extremes)


def rgba_frames(h, w, n, seed):
    """(n, h, w, 4): frame f holds CONTENT[f % 3] in every channel (its own seed each).  Alpha is noise in frame 0,
    255 in frame 1 and 0 / 255 in frame 2.  Patches share their geometry over the channels, so a flat window is flat in
    all four."""
    out = np.empty((n, h, w, 4), np.uint8)
    for f in range(n):
        for c in range(4):
            out[f, ..., c] = CONTENT[f % 3](h, w, seed * 100 + f * 4 + c)
    if n > 1:
        out[1, ..., 3] = 255
    return out


def rgba_batches(shape):
    """The batches of one RGBA shape: one for the multi-frame shapes (their frames differ in content), noise and
    0 / 255 for the one-frame shapes."""
    h, w, n = shape
    seed = h * 1000 + w
    if n > 1:
        return [rgba_frames(h, w, n, seed)]
    x = rgba_frames(h, w, 1, seed)
    e = np.stack([extremes(h, w, seed * 100 + 50 + c) for c in range(4)], axis=-1)[None]
    return [x, np.ascontiguousarray(e)]


def g8_batches(shape):
    """The batches of one single-channel shape, (n, h, w) each: noise + patches and 0 / 255 + patches in the two-frame
    shapes, noise and patches in the one-tile shape, noise alone in the small ones."""
    h, w, n = shape
    seed = h * 1000 + w
    if n == 2:
        first = noise if (h * w) % 2 == 0 else extremes
        return [np.stack([first(h, w, seed), patches(h, w, seed + 1)])]
    if (h, w) == G8_TILE:
        return [noise(h, w, seed)[None], patches(h, w, seed + 1)[None]]
    return [noise(h, w, seed)[None]]


def gauss_plane(oracle, y, k, sigma):
    """test_gpu_gray8's gauss_r — the R channel of the CPU Gaussian of (y, y, y, 255) — on one thread, so that a pool
    can run many of them side by side."""
    rgba = np.ascontiguousarray(np.dstack([y, y, y, np.full_like(y, 255)]))
    return np.ascontiguousarray(oracle.gauss_rgba(rgba, k, sigma)[..., 0])


# ---- the LDS carves, restated ----------------------------------------------------------------------------------------
def _up(v, m):
    return (v + m - 1) // m * m


GaussTileLayout = collections.namedtuple("GaussTileLayout", "RW RH off_raw off_wt bytes")
PipeTileLayout = collections.namedtuple("PipeTileLayout", "GW GH off_v off_b off_wt bytes")
G8Layout = collections.namedtuple("G8Layout", "H RH RW RWS GH GW GWS off_v off_w2 off_w1 off_raw off_g off_o bytes")


def gauss_tile_layout(exact, k):
    """gauss_tile.hip gauss_tile_layout: [V float4 TH * RW (FAST only)] [raw u32 RH * RW] [weights], in bytes."""
    th, tw = RGBA_TILE
    r = k >> 1
    rw, rh = tw + 2 * r, th + 2 * r
    off_raw = 0 if exact else th * rw * 16
    off_wt = off_raw + rh * rw * 4
    return GaussTileLayout(rw, rh, off_raw, off_wt, off_wt + (k * k if exact else k) * 4)


def pipe_tile_layout(exact, k):
    """sobel_tile.hip pipe_tile_layout: [G float GH * GW] [V float kLH * GW (FAST)] [B int kLH * kLW] [weights];
    offsets in 4-byte words, `bytes` in bytes."""
    th, tw = RGBA_TILE
    lw, lh = tw + 2, th + 2
    r = k >> 1
    gw, gh = tw + 2 * r + 2, th + 2 * r + 2
    off_v = gh * gw
    off_b = off_v + (0 if exact else lh * gw)
    off_wt = off_b + lh * lw
    return PipeTileLayout(gw, gh, off_v, off_b, off_wt, (off_wt + (k * k if exact else k)) * 4)


OP_GAUSS, OP_SOBEL, OP_PIPE = 0, 1, 2      # gray8.hip G8Op
GM_SEP, GM_EXC, GM_TAP = 0, 1, 2           # gray8.hip G8Gm


def g8_layout(op, gm, k):
    """gray8.hip g8_layout: [V float GH * RW (not kGmTap)] [w2 k * k (not kGmSep)] [w1 k] [raw RH * RWS]
    [G GH * GWS (pipeline)] [O TH * TW], every region rounded up to 16 bytes."""
    th, tw = G8_TILE
    r, o = k // 2, 1 if op == OP_PIPE else 0
    hh = 1 if op == OP_SOBEL else r + o
    rh, rw = th + 2 * hh, tw + 2 * hh
    rws = _up(rw, 16)
    gh, gw = th + 2 * o, tw + 2 * o
    gws = _up(gw, 4)
    gauss = op != OP_SOBEL
    off_v = 0
    off_w2 = off_v + _up(gh * rw * 4 if gauss and gm != GM_TAP else 0, 16)
    off_w1 = off_w2 + _up(k * k * 4 if gauss and gm != GM_SEP else 0, 16)
    off_raw = off_w1 + _up(k * 4 if gauss else 0, 16)
    off_g = off_raw + _up(rh * rws, 16)
    off_o = off_g + _up(gh * gws if op == OP_PIPE else 0, 16)
    return G8Layout(hh, rh, rw, rws, gh, gw, gws, off_v, off_w2, off_w1, off_raw, off_g, off_o, off_o + th * tw)


def g8_gm(delta, fast, tile, pipe):
    """gray8.hip launch_gauss_gray8 / launch_pipeline_gray8 for a runtime k and a table with a symmetric separable
    factor: which arithmetic runs.  delta = delta_bound_k of the table."""
    exc = delta < DELTA_LIMIT and not tile
    if pipe or not fast:
        return GM_EXC if exc else GM_TAP
    return GM_SEP


def all_carves(k):
    """{name: bytes} of every launch the GPU tests make at k."""
    out = {"gauss_tile FAST": gauss_tile_layout(False, k).bytes, "gauss_tile EXACT": gauss_tile_layout(True, k).bytes,
           "pipeline_tile FAST": pipe_tile_layout(False, k).bytes, "pipeline_tile EXACT": pipe_tile_layout(True, k).bytes}
    for op, op_name in ((OP_GAUSS, "gauss"), (OP_PIPE, "pipeline")):
        for gm, gm_name in ((GM_SEP, "kGmSep"), (GM_EXC, "kGmExc"), (GM_TAP, "kGmTap")):
            if not (op == OP_PIPE and gm == GM_SEP):
                out["gray8 %s %s" % (op_name, gm_name)] = g8_layout(op, gm, k).bytes
    return out


# ---- the comparison helper -------------------------------------------------------------------------------------------
class Report:
    """Collects every failed comparison of one test with where it failed: which frames, channels, rows and columns."""

    def __init__(self):
        self.bad = []

    def _where(self, wrong):
        idx = np.nonzero(wrong)
        names = {4: ("frame", "row", "col", "channel"), 3: ("frame", "row", "col"), 2: ("axis 0", "axis 1")}[wrong.ndim]
        return ", ".join("%s %d..%d" % (n, i.min(), i.max()) for n, i in zip(names, idx))

    def same(self, got, ref, *tag):
        if not np.array_equal(got, ref):
            wrong = got != ref
            d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
            self.bad.append("%s: %d values differ (max |d| %d; %s)" % (tag, int(wrong.sum()), int(d.max()), self._where(wrong)))

    def within(self, got, ref, tol, *tag):
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        if d.max() > tol:
            self.bad.append("%s: max |d| %d > %d at %d values (%s)" % (tag, int(d.max()), tol, int((d > tol).sum()),
                                                                      self._where(d > tol)))

    def done(self):
        assert not self.bad, "%d failed comparisons:\n%s" % (len(self.bad), "\n".join(self.bad[:40]))
