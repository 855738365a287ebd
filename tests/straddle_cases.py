"""Integer-straddling blur windows: what test_straddle_cpu.py, test_gpu_straddle.py and golden/make_straddle.py share.

About half of the Gaussian code promises the CPU path's bytes.  The CPU byte is trunc(S_cpu), S_cpu = the k * k-term
float sum in the CPU path's own order (ky outer, kx inner, float multiply, then float add).  A kernel that evaluates the
window in another order, or with a fused multiply-add, or that skips the exception it owes (exact_common.hpp), moves
the sum by about one ulp, and that changes the byte only where S_cpu sits within ~1e-5 of an integer: a handful of values
in a frame of noise.  A *critical window* is a k x k block of bytes on which the truncated byte of at least one
*alternate* differs from the CPU path's:

    a  rows visited bottom to top                 c  columns visited right to left
    b  kx outer, ky inner                         d  the exact sum (float64: exact for these tables, span_ok())
    e  the contracted chain, sum = fma(v, w, sum)

golden/straddle_windows.json holds mined critical windows (golden/make_straddle.py); the builders here tile frames with
them, so that a kernel with one of those faults gets thousands of bytes wrong instead of none.

  * numerics      visit_order / accumulate / window_bytes / blur_plane: the CPU chain and the alternates in numpy, on
                  windows and on whole planes; span_ok: the argument that makes d and e exact in double
  * fixture       load_fixture, edge_maps / expand_edge: windows whose centre sits c < R pixels from an image edge hold
                  their in-image part expanded by the CPU path's clamp-to-edge rule
  * frames        dense_plane / sparse_plane / beside_flat_plane, rgba_gauss_batch, rgba_pipe_batch, gray_lut
  * strip plan    strip_plan / strip_quads: slide_common.hpp's make_strip_plan restated (it depends on the width only)
  * pair form     pair_form_sum: exact_blur_row's separable sum S' with every fma rounded once, in integer arithmetic
  * diagnosis     matched_alternates: which alternate a wrong GPU result agrees with

A plain numpy helper for those tests, not a fixture module.
"""
import functools
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "straddle_windows.json")
F32, F64 = np.float32, np.float64

# gauss_tables_ref.BASES without k = 11, plus k = 33 for the runtime-k kGmExc range of gray8.hip
SIZES = ((3, 0.8), (5, 1.5), (7, 2.0), (9, 2.5), (17, 6.0), (33, 5.5))
SIGMA = dict(SIZES)
ALTS = ("a", "b", "c", "d", "e")
ALT_NAMES = {"a": "rows bottom to top", "b": "kx outer, ky inner", "c": "columns right to left",
             "d": "exact sum (exception skipped, or a correctly rounded separable sum)", "e": "contracted multiply-add"}
EDGE_KS = (3, 5, 7)
EDGE_KINDS = ("top", "bottom", "left", "right", "top-left", "bottom-right")
EDGE_QUOTA = 8


def quota(k):
    return 16 if k == 33 else 32


# ---- numerics --------------------------------------------------------------------------------------------------------
def visit_order(k, alt=None):
    """[(ky, kx)] in the order the chain visits the taps: the CPU path's (alt None, d, e) or a reordered one."""
    ys, xs = range(k), range(k)
    if alt == "a":
        return [(ky, kx) for ky in reversed(ys) for kx in xs]
    if alt == "b":
        return [(ky, kx) for kx in xs for ky in ys]
    if alt == "c":
        return [(ky, kx) for ky in ys for kx in reversed(xs)]
    assert alt in (None, "d", "e"), alt
    return [(ky, kx) for ky in ys for kx in xs]


def accumulate(tap, k, w2, alt=None):
    """The sum of one chain.  tap(ky, kx) -> uint8 array (any shape, the same for every tap); w2 the (k, k) float32
    table.  float32 for the CPU chain and a, b, c, e; float64 for d."""
    w2 = np.asarray(w2, F32)
    if alt == "d":
        s = 0.0
        for ky, kx in visit_order(k):
            s = s + tap(ky, kx).astype(F64) * F64(w2[ky, kx])
        return s
    if alt == "e":   # byte * float32 is exact in double and the sum stays within 53 bits (span_ok): one rounding
        s = None
        for ky, kx in visit_order(k):
            p = tap(ky, kx).astype(F64) * F64(w2[ky, kx])
            s = (p if s is None else p + s.astype(F64)).astype(F32)
        return s
    s = None
    for ky, kx in visit_order(k, alt):
        p = tap(ky, kx).astype(F32) * w2[ky, kx]          # rounded product
        s = p if s is None else s + p                     # rounded sum (0 + p = p)
    return s


def to_byte(s):
    """The CPU path's store: clamp to [0, 255], truncate (every sum here is >= 0)."""
    return np.minimum(s, 255.0).astype(np.uint8)


def span_ok(w2):
    """True if every partial sum of byte * weight terms below 2^8 is exact in double: the lowest bit any product can set
    is the lowest bit of the smallest weight's float32 significand (times a byte >= 1), and from there up to 2^8 must
    fit 53 bits."""
    w2 = np.asarray(w2, F32)
    assert (w2 > 0).all() and 255.0 * float(w2.astype(F64).sum()) < 256.0
    lowest = min(math.frexp(float(v))[1] - 24 for v in w2.reshape(-1))     # v = m 2^e, m in [0.5, 1): ulp 2^(e - 24)
    return 8 - lowest <= 53


def window_sums(wins, w2, alt=None):
    wins = np.asarray(wins, np.uint8)
    k = wins.shape[-1]
    return accumulate(lambda ky, kx: wins[..., ky, kx], k, w2, alt)


def window_bytes(wins, w2, alt=None):
    return to_byte(window_sums(wins, w2, alt))


def critical_letters(wins, w2):
    """Per window, the alternates whose byte differs from the CPU path's, as a string of letters."""
    ref = window_bytes(wins, w2)
    diff = {a: window_bytes(wins, w2, a) != ref for a in ALTS}
    return ["".join(a for a in ALTS if diff[a][i]) for i in range(len(ref))]


def plane_sums(plane, w2, alt=None):
    plane = np.asarray(plane, np.uint8)
    h, w = plane.shape
    k = np.asarray(w2).shape[0]
    r = k // 2
    pad = np.pad(plane, r, mode="edge")                   # the CPU path clamps its taps to the image
    return accumulate(lambda ky, kx: pad[ky:ky + h, kx:kx + w], k, w2, alt)


def blur_plane(plane, w2, alt=None):
    """The CPU path's Gaussian of one channel (alt None: equal to the oracle's, test_straddle_cpu.py checks it), or the
    whole-frame blur a kernel with fault `alt` would produce."""
    return to_byte(plane_sums(plane, w2, alt))


def alternate_blurs(plane, w2):
    """(ref, {alt: blurred plane}) = blur_plane for the CPU chain and all five alternates, at the price of about one.
    Any float32 chain of k * k non-negative terms below 256 is within k * k * 2^-16 of the exact sum (two roundings of
    at most 2^-17 per tap), so two chains can truncate differently only where the exact sum lies within that of an
    integer; the chains are evaluated on those windows alone, everywhere else every alternate's byte is trunc(exact)."""
    plane = np.asarray(plane, np.uint8)
    k = np.asarray(w2).shape[0]
    r = k // 2
    exact = plane_sums(plane, w2, "d")
    near = np.abs(exact - np.rint(exact)) <= k * k * 2.0 ** -16
    ys, xs = np.nonzero(near)
    wins = np.lib.stride_tricks.sliding_window_view(np.pad(plane, r, mode="edge"), (k, k))[ys, xs]
    ref = to_byte(exact)
    out = {}
    for a in (None,) + ALTS:
        b = ref.copy()
        b[ys, xs] = window_bytes(wins, w2, a)
        out[a] = b
    return out.pop(None), out


def critical_mask(plane, w2):
    """{alt: bool (h, w)}: where alternate `alt` changes the byte."""
    ref, alts = alternate_blurs(plane, w2)
    return {a: alts[a] != ref for a in ALTS}


# ---- fixture ---------------------------------------------------------------------------------------------------------
def edge_maps(kind, cy, cx, k):
    """(rows, cols): window row ky reads the window's row rows[ky] (clamp-to-edge for a centre cy rows from the top or
    bottom edge, cx columns from the left or right one); identity on the axis the kind does not touch."""
    r = k // 2
    idx = np.arange(k)
    rows, cols = idx.copy(), idx.copy()
    if kind in ("top", "top-left"):
        rows = np.maximum(idx, r - cy)
    if kind in ("bottom", "bottom-right"):
        rows = np.minimum(idx, r + cy)
    if kind in ("left", "top-left"):
        cols = np.maximum(idx, r - cx)
    if kind in ("right", "bottom-right"):
        cols = np.minimum(idx, r + cx)
    return rows, cols


def expand_edge(win, kind, cy, cx):
    rows, cols = edge_maps(kind, cy, cx, win.shape[-1])
    return win[..., rows, :][..., cols]


def _unhex(s, k):
    return np.frombuffer(bytes.fromhex(s), np.uint8).reshape(k, k).copy()


@functools.lru_cache(maxsize=None)
def load_fixture():
    """({k: (windows (N, k, k) uint8, [letters])}, {k: [(kind, cy, cx, window (k, k), letters)]})."""
    data = json.load(open(FIXTURE))
    interior, edges = {}, {}
    for key, entry in data["interior"].items():
        k = int(key)
        interior[k] = (np.stack([_unhex(s, k) for s in entry["windows"]]), list(entry["alternates"]))
    for key, items in data["edges"].items():
        k = int(key)
        edges[k] = [(e["kind"], e["cy"], e["cx"], _unhex(e["window"], k), e["alternates"]) for e in items]
    return interior, edges


def ranked_windows(k):
    """The interior windows of size k, those critical for the most alternates first (stable)."""
    wins, letters = load_fixture()[0][k]
    order = sorted(range(len(wins)), key=lambda i: -len(letters[i]))
    return wins[order], [letters[i] for i in order]


# ---- frames ----------------------------------------------------------------------------------------------------------
# the smallest with more than one strip and several bands walking each way: aligned / width % 4 == 2 / odd width (gray8
# and the tiled kernels) / the 8-pixel pipeline kernel
SHAPE_ALIGNED, SHAPE_RAGGED, SHAPE_ODD, SHAPE_PIPE8 = (131, 512), (97, 250), (53, 501), (131, 1000)
SPARSE_PERIOD = 256


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _put_edges(out, k, phase):
    """Edge windows onto the four edges and two corners: only their in-image part is written."""
    h, w = out.shape
    if k not in EDGE_KS or h < 4 * k or w < 8 * k:
        return
    r = k // 2
    items = load_fixture()[1][k]
    by_kind = {kind: [e for e in items if e[0] == kind] for kind in EDGE_KINDS}
    step = 2 * k + 1                                      # odd: the centres walk through every residue mod 8

    def part(e):                                          # the window's in-image rows and columns
        _, cy, cx, win, _ = e
        rows, cols = edge_maps(e[0], cy, cx, k)
        return win[np.unique(rows)][:, np.unique(cols)]

    for n, pos in enumerate(range(2 * k, w - 3 * k, step)):
        e = by_kind["top"][(n + phase) % len(by_kind["top"])]
        out[0:e[1] + r + 1, pos - r:pos + r + 1] = part(e)
        e = by_kind["bottom"][(n + phase) % len(by_kind["bottom"])]
        out[h - 1 - e[1] - r:h, pos - r:pos + r + 1] = part(e)
    for n, pos in enumerate(range(2 * k, h - 3 * k, step)):
        e = by_kind["left"][(n + phase) % len(by_kind["left"])]
        out[pos - r:pos + r + 1, 0:e[2] + r + 1] = part(e)
        e = by_kind["right"][(n + phase) % len(by_kind["right"])]
        out[pos - r:pos + r + 1, w - 1 - e[2] - r:w] = part(e)
    e = by_kind["top-left"][phase % len(by_kind["top-left"])]
    out[0:e[1] + r + 1, 0:e[2] + r + 1] = part(e)
    e = by_kind["bottom-right"][phase % len(by_kind["bottom-right"])]
    out[h - 1 - e[1] - r:h, w - 1 - e[2] - r:w] = part(e)


def dense_plane(h, w, k, seed, phase=0, flat_rows=False, y_off=0):
    """Tiled by k x k critical windows from row y_off down: block-row j starts j % k pixels to the right, so the critical
    centres reach every column (k is odd: every residue mod 8 as well); noise in the gaps; the windows cycle through the
    fixture from `phase` on.  flat_rows: every other block-row is one constant instead (the beside-flat frame)."""
    wins, _ = load_fixture()[0][k]
    out = _noise(h, w, seed)
    flat = _noise(h // k + 1, 1, seed + 1)[:, 0]
    n = phase
    for j in range((h - y_off) // k):
        y = y_off + j * k
        if flat_rows and j % 2 == 1:
            out[y:y + k] = flat[j]
            continue
        for x in range(j % k, w - k + 1, k):
            out[y:y + k, x:x + k] = wins[n % len(wins)]
            n += 1
    _put_edges(out, k, phase)
    return out


def beside_flat_plane(h, w, k, seed, phase=0, y_off=0):
    return dense_plane(h, w, k, seed, phase, flat_rows=True, y_off=y_off)


def sparse_plane(h, w, k, seed, phase=0, y_off=0):
    """Seeded noise with one critical block per 256 columns and per block-row, the windows that are critical for the most
    alternates first.  The block's column moves by 37 from one block-row to the next."""
    wins, _ = ranked_windows(k)
    out = _noise(h, w, seed)
    n = phase
    for j in range((h - y_off) // k):
        for x in range((37 * j) % (SPARSE_PERIOD - k), w - k + 1, SPARSE_PERIOD):
            out[y_off + j * k:y_off + (j + 1) * k, x:x + k] = wins[n % len(wins)]
            n += 1
    _put_edges(out, k, phase)
    return out


KINDS = {"dense": dense_plane, "sparse": sparse_plane, "beside-flat": beside_flat_plane}
SLIDE_KS = (3, 5, 7)               # the register-resident exact-by-exception kernels (gauss_exact, pipe_slide)


def kinds_of(k):
    """The sparse frame is about exact_blur_row's dense_flags() branch, which only k <= 7 has; above that one block per
    256 columns leaves too few critical bytes in a frame of these sizes for the bar of test_straddle_cpu.py."""
    return ("dense", "sparse", "beside-flat") if k in SLIDE_KS else ("dense", "beside-flat")


def gauss_rgba_shapes(k):
    """k <= 7: gauss_exact on the aligned shape, the tiled kernel on the ragged one; k = 9, 17: tiled on both."""
    return (SHAPE_ALIGNED, SHAPE_RAGGED) if k in SLIDE_KS else (SHAPE_ALIGNED, SHAPE_ODD)


PIPE_SHAPES = (SHAPE_ALIGNED, SHAPE_RAGGED)
PIPE8_KS = (3, 5)                  # pipe_slide.hip has no 8-pixel kernel for k = 7
GRAY8_PIPE_KS = (5, 9, 33)


def gray8_shapes(k):
    """One plane has to hold enough blocks of k x k for every alternate: the odd shape up to k = 9, the largest above."""
    return (SHAPE_ODD,) if k <= 9 else (SHAPE_PIPE8,)


def plane_pair(kind, h, w, k, phase=0):
    """(2, h, w): two planes with the same blocks and another seed for the noise.  The second one's blocks start
    k / 2 + 1 rows further down: its critical rows fall on other ring slots of the sliding kernels' bands."""
    seed = 1000 * h + w + 17 * k
    return np.stack([KINDS[kind](h, w, k, seed, phase), KINDS[kind](h, w, k, seed + 500, phase, y_off=k // 2 + 1)])


def rgba_gauss_batch(kind, h, w, k, opaque):
    """(2, h, w, 4) for the RGBA Gaussian: critical planes in all four channels (the 4-channel EXACT walk), or in RGB with
    A = 255 (the opaque walk).  Channel c starts 11 c windows further into the fixture."""
    out = np.empty((2, h, w, 4), np.uint8)
    for c in range(4):
        out[..., c] = plane_pair(kind, h, w, k, phase=11 * c)
    if opaque:
        out[..., 3] = 255
    return out


@functools.lru_cache(maxsize=None)
def gray_lut(oracle):
    """(grey (256, 3), coloured (256, 8, 3)) pixels whose oracle luminance is the level.  grey: R = G = B where such a
    pixel exists (the CPU formula truncates 0.299 r + 0.587 g + 0.114 b in double, so luma(u, u, u) is u or u - 1 and
    some levels have no grey pixel), else the nearest-to-grey coloured one.  coloured: 8 seeded pixels per level."""
    rng = np.random.default_rng(2024)
    levels = np.repeat(np.arange(256), 4000)
    cand = np.clip(levels[:, None] + rng.integers(-60, 61, (len(levels), 3)), 0, 255).astype(np.uint8)
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    cand = np.concatenate([greys, cand])
    rgba = np.concatenate([cand, np.full((len(cand), 1), 255, np.uint8)], 1)[None]
    luma = oracle.gray_rgba_1ch(np.ascontiguousarray(rgba))[0]
    assert all(int(luma[i]) == oracle.gray_px(*cand[i]) for i in range(0, len(cand), 997))
    spread = np.abs(cand.astype(int) - cand.astype(int).mean(1, keepdims=True)).sum(1)
    grey = np.empty((256, 3), np.uint8)
    coloured = np.empty((256, 8, 3), np.uint8)
    for v in range(256):
        idx = np.nonzero(luma == v)[0]
        assert len(idx) >= 1, v
        grey[v] = cand[idx[np.argmin(spread[idx], axis=0)]]
        col = idx[spread[idx] > 0] if (spread[idx] > 0).any() else idx
        coloured[v] = cand[col[np.arange(8) % len(col)]]
    return grey, coloured


def rgba_pipe_batch(oracle, kind, h, w, k, coloured):
    """((2, h, w, 4), planes (2, h, w)) for the fused pipeline: the oracle's gray image of the batch is `planes`.  Grey
    pixels (R = G = B wherever the level has one) or coloured pixels picked per level from gray_lut; alpha is noise."""
    planes = plane_pair(kind, h, w, k)
    grey, col = gray_lut(oracle)
    out = np.empty((2, h, w, 4), np.uint8)
    if coloured:
        pick = np.random.default_rng(h * w + k).integers(0, 8, planes.shape)
        out[..., :3] = col[planes, pick]
    else:
        out[..., :3] = grey[planes]
    out[..., 3] = np.random.default_rng(h + w + k).integers(0, 256, planes.shape, dtype=np.uint8)
    return out, planes


@functools.lru_cache(maxsize=None)
def _grey_luma(oracle):
    return np.array([oracle.gray_px(v, v, v) for v in range(256)], np.uint8)


def rgba_pipe_post(oracle):
    """What the RGBA pipeline does with the blurred gray image b: the Sobel's luminance formula is applied again to the
    pixel (b, b, b) — which is b or b - 1 — before the edge detector (the single-channel chain is sobel_gray alone)."""
    lut = _grey_luma(oracle)
    return lambda blurred: oracle.sobel_gray(np.ascontiguousarray(lut[blurred]))


# ---- the strip plan --------------------------------------------------------------------------------------------------
LANES_OUT_MAX = 62                 # slide_common.hpp kSlideLanesOutMax


def strip_plan(w, px=4):
    """(nstrips, lanes_out) of a row of w pixels: make_strip_plan (px = 4; a ragged last quad counts) and pipe_slide.hip's
    launch_r for 8 pixels per lane (w / 8 octets)."""
    quads = (w + 3) // 4 if px == 4 else w // 8
    nstrips = (quads + LANES_OUT_MAX - 1) // LANES_OUT_MAX
    return nstrips, (quads + nstrips - 1) // nstrips


def strip_quads(w, px=4):
    """Per strip: {"first", "last": its first and last storing lane, "halo_left", "halo_right": the halo lanes} as quad
    (lane-column) indices; a halo lane outside the image is None."""
    quads = (w + px - 1) // px
    nstrips, lanes = strip_plan(w, px)
    out = []
    for s in range(nstrips):
        first, end = s * lanes, min((s + 1) * lanes, quads)
        out.append({"first": first, "last": end - 1, "halo_left": first - 1 if first > 0 else None,
                    "halo_right": end if end < quads else None})
    return out


# ---- the kernels' pair-form sum, every fma rounded once ---------------------------------------------------------------
def _split(x):
    """float (a float32 value) -> (M, E), x = M 2^E exactly."""
    if x == 0.0:
        return 0, 0
    m, e = math.frexp(float(x))
    M = int(math.ldexp(m, 24))
    assert math.ldexp(M, e - 24) == float(x)
    return M, e - 24


def _round24(M, E):
    """(M, E) >= 0 rounded to a 24-bit significand, nearest even (no value here is subnormal or overflows)."""
    n = M.bit_length() - 24
    if n <= 0:
        return M, E
    q, rem, half = M >> n, M & ((1 << n) - 1), 1 << (n - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return q, E + n


def _fma(a, b, c):
    """round(a * b + c) for (M, E) pairs: exact integers, one rounding."""
    (ma, ea), (mb, eb), (mc, ec) = a, b, c
    mp, ep = ma * mb, ea + eb
    e = min(ep, ec)
    return _round24((mp << (ep - e)) + (mc << (ec - e)), e)


_ONE = (1, 0)


def _value(v):
    return math.ldexp(v[0], v[1])


def pair_form_sum(win, w1, delta):
    """exact_blur_row's S' for the centre of one k x k window (gray8.hip's kGmExc pass is the same chain): vertical
    acc = w(0) g_c, acc = fma(w(d), g_{c-d} + g_{c+d}, acc); horizontal acc = fma(w(0), v_c, delta),
    acc = fma(w(d), v_{c-d} + v_{c+d}, acc) with the pair sum v + v a rounded float addition.  Returned as a Python float
    holding the float32 result exactly."""
    k = len(w1)
    r = k // 2
    wd = [_split(w1[r + d]) for d in range(r + 1)]
    win = [[int(v) for v in row] for row in np.asarray(win)]
    v = []
    for x in range(k):
        acc = _fma(wd[0], (win[r][x], 0), (0, 0))
        for d in range(1, r + 1):
            acc = _fma(wd[d], (win[r - d][x] + win[r + d][x], 0), acc)
        v.append(acc)
    acc = _fma(wd[0], v[r], _split(delta))
    for d in range(1, r + 1):
        acc = _fma(wd[d], _fma(_ONE, v[r - d], v[r + d]), acc)
    return _value(acc)


# ---- diagnosis -------------------------------------------------------------------------------------------------------
def matched_alternates(got, ref, planes, w2, post=None):
    """Text for a failed comparison: of the values where `got` differs from `ref`, how many equal what each alternate
    computes.  planes: (..., h, w) uint8, the blurred channel(s) in the layout of got / ref before `post` (e.g. the
    oracle's Sobel for the pipeline; per plane)."""
    got, ref, planes = np.asarray(got), np.asarray(ref), np.asarray(planes)
    wrong = got != ref
    lines = ["%d of %d values differ" % (int(wrong.sum()), wrong.size)]
    for a in ALTS:
        flat = planes.reshape((-1,) + planes.shape[-2:])
        alt = np.stack([blur_plane(p, w2, a) for p in flat])
        if post is not None:
            alt = np.stack([post(p) for p in alt])
        alt = alt.reshape(planes.shape)
        lines.append("  %s (%s): equals the GPU at %d of them" % (a, ALT_NAMES[a], int((alt == got)[wrong].sum())))
    return "\n".join(lines)
