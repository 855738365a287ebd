"""GPU suite (-m gpu): batches of thousands of tiny frames through CLAHE, the mean adaptive threshold, connected-component
labelling, hysteresis, Canny and the Hough transform (cases and reasons: tiny_feature_cases.py; what the contents are
for: test_tiny_batch_features_cpu.py).

As in test_gpu_tiny_batch.py every call is device-resident through the guarded arena (tests/guarded.py), the payload
prefilled 128 away from the expected bytes, at offsets (0, 0) and (3, 1) where the output is bytes and (3, 0) and (3, 4)
where it is 4-byte data; a call with several outputs has them back to back in one payload, each on the alignment the
header demands, and the bytes of a gap must keep their prefill.  A batch repeats 11 frames with a first and a last frame
of their own; the CPU reference is computed once per distinct frame and EVERY frame, row and byte of the GPU result is
compared with it.

No tolerance anywhere: bit identity with ccl_ref, canny_ref, hough_ref (fed the library's trig table), clahe_ref and
box_ref.adaptive_ref; floats are compared as their bytes.
"""
import numpy as np
import pytest

import canny_ref as cr
import guarded
import hough_ref as hr
import tiny_batch_cases as tb
import tiny_feature_cases as tf
from box_ref import adaptive_ref
from ccl_ref import ccl_ref
from clahe_ref import apply_ref, luts_ref
from hist_ref import equalize_ref, otsu_ref

pytestmark = pytest.mark.gpu

OFF_BYTES = ((0, 0), (3, 1))     # 1-byte outputs
OFF_WORDS = ((3, 0), (3, 4))     # 4-byte outputs (and the CLAHE tables, which are 4-byte aligned)
POOL_N = 64                      # the small batch of the pooled-scratch orders
CHAIN_SHAPE, CHAIN_N = (13, 17), 301
HIST_SHAPE = (13, 17)
HOUGH_POOL_N = 699               # the accumulators are the library's: nothing but lines, votes and counts in the arena


@pytest.fixture(autouse=True)
def _reset_kernel_selection(ctx, pkg):
    yield
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_input_format(pkg.INPUT_RGBA)


_refs = {}


def ref_of(key, make):
    """One CPU reference per (feature, parameters, shape): arrays of (NDISTINCT, ...), shared by every test, read-only."""
    if key not in _refs:
        made = make()
        made = tuple(np.ascontiguousarray(a) for a in made) if isinstance(made, tuple) else np.ascontiguousarray(made)
        for a in (made if isinstance(made, tuple) else (made,)):
            a.setflags(write=False)
        _refs[key] = made
    return _refs[key]


def each(fn, frames):
    return np.stack([fn(f) for f in frames])


def shape_ids(shapes):
    return ["%dx%d" % s for s in shapes]


def rows_by_shape(rows):
    by = {}
    for r in rows:
        by.setdefault(r.shape, []).append(r)
    return by


# ---- the arena with several outputs ------------------------------------------------------------------------------------
GAP = 0x3C


def layout(parts, off_out):
    """parts: [(name, expected array (n, ...), alignment)].  -> (payload bytes expected after the call, {name: offset}):
    the outputs back to back, each moved up to its alignment of the device address (the payload starts at 16 m + off_out)"""
    at, where, total = {}, 0, 0
    for name, a, align in parts:
        where += (-(off_out + where)) % align
        at[name] = where
        where += a.nbytes
    total = where
    blob = np.full(total, GAP, np.uint8)
    for name, a, _ in parts:
        blob[at[name]:at[name] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()
    return blob, at


def compare(got, parts, at, blob, tag):
    """Every byte of every output, and the prefill of every gap; a failure names the output, frame, row and byte."""
    if np.array_equal(got, blob):
        return
    gap = np.ones(blob.size, bool)
    for name, a, _ in parts:
        o = at[name]
        gap[o:o + a.nbytes] = False
        try:
            guarded.check(got[o:o + a.nbytes], blob[o:o + a.nbytes], 0, "%s %s" % (tag, name))
        except guarded.PayloadError as e:
            frame_bytes = a[0].nbytes
            row_bytes = frame_bytes // a.shape[1] if a.ndim > 2 else frame_bytes
            raise AssertionError("%s: %s" % (e, tb.where(e.index, frame_bytes, row_bytes))) from None
    assert np.array_equal(got[gap], guarded.prefill_of(blob)[gap]), tag + ": a byte between two outputs changed"


def arena(ctx, call, x, parts, off, tag):
    """call(d_in, {name: device address}) on the input x through the arena; returns {name: output as the part's dtype}"""
    blob, at = layout(parts, off[1])
    tag = "%s n %d off %s" % (tag, parts[0][1].shape[0], off)
    got = guarded.run(ctx, lambda d_in, d_out: call(d_in, {k: d_out + v for k, v in at.items()}), x, blob, off[0], off[1],
                      tag=tag)
    compare(got, parts, at, blob, tag)
    return {name: got[at[name]:at[name] + a.nbytes].view(a.dtype).reshape(a.shape) for name, a, _ in parts}


def one_output(ctx, call, x, expected, off, tag, align=1):
    return arena(ctx, lambda d_in, d: call(d_in, d["out"]), x, [("out", expected, align)], off, tag)["out"]


# ---- the calls and their references ----------------------------------------------------------------------------------------
def clahe_refs(shape, grid, clip):
    """(frames, tables) of the distinct gray frames"""
    def make():
        d = tb.distinct(shape[0], shape[1], 1)
        luts = luts_ref(d, clip, grid[0], grid[1])
        return each(lambda i: apply_ref(d[i], luts[i], grid[0], grid[1]), range(tb.NDISTINCT)), luts
    return ref_of(("clahe", shape, grid, clip), make)


def run_clahe(ctx, shape, grid, clip, n, offs=OFF_BYTES, tables=True, lut_offs=OFF_WORDS):
    h, w = shape
    frames14, luts14 = clahe_refs(shape, grid, clip)
    x = tb.batch(h, w, n, 1)
    tag = "clahe %dx%d grid %s clip %g" % (h, w, grid, clip)
    for off in offs:
        one_output(ctx, lambda a, b: ctx.clahe_gray8_dev(a, b, w, h, n, clip, grid[0], grid[1]), x, tb.expand(frames14, n),
                   off, tag)
    for off in (lut_offs if tables else ()):
        one_output(ctx, lambda a, b: ctx.clahe_luts_gray8_dev(a, b, w, h, n, clip, grid[0], grid[1]), x,
                   tb.expand(luts14, n), off, tag + " tables", align=4)


def adaptive_refs(shape, params):
    d = tb.distinct(shape[0], shape[1], 1)
    return ref_of(("adaptive", shape, params), lambda: each(lambda f: adaptive_ref(f, *params), d))


def ccl_refs(shape, conn, rows):
    return ref_of(("ccl", shape, conn, rows), lambda: ccl_ref(tf.mask_distinct(*shape), conn, rows))


def run_ccl(ctx, shape, conn, rows, n, offs=OFF_WORDS, tag=""):
    """stats_rows 0: null statistics pointers; otherwise labels, count, stats and sums all in the arena"""
    h, w = shape
    want = [tb.expand(a, n) for a in ccl_refs(shape, conn, rows)]
    parts = [("labels", want[0], 4), ("count", want[1], 4)]
    if rows:
        parts += [("stats", want[2], 4), ("sums", want[3], 8)]

    def call(d_in, d):
        ctx.ccl_gray8_dev(d_in, d["labels"], d["count"], d.get("stats"), d.get("sums"), w, h, n, conn, rows)

    for off in offs:
        arena(ctx, call, tf.mask_batch(h, w, n), parts, off, "%sccl %dx%d conn %d rows %d" % (tag, h, w, conn, rows))


def hyst_refs(shape, params):
    return ref_of(("hyst", shape, params), lambda: cr.hysteresis_ref(tf.response_distinct(*shape), *params))


def run_hyst(ctx, shape, params, n, offs=OFF_BYTES, tag=""):
    h, w = shape
    tag = "%shysteresis %dx%d %r" % (tag, h, w, params)
    for off in offs:
        got = one_output(ctx, lambda a, b: ctx.hysteresis_gray8_dev(a, b, w, h, n, *params), tf.response_batch(h, w, n),
                         tb.expand(hyst_refs(shape, params), n), off, tag)
        lit = got.reshape(n, -1).any(axis=1) & tf.weak_frames(n)
        assert not lit.any(), "%s: weak frame %d is not all zero" % (tag, int(np.flatnonzero(lit)[0]))


def canny_refs(shape, params):
    return ref_of(("canny", shape, params), lambda: cr.canny_ref(tb.distinct(shape[0], shape[1], 1), *params))


def run_canny(ctx, shape, params, n, offs=OFF_BYTES, tag=""):
    h, w = shape
    for off in offs:
        one_output(ctx, lambda a, b: ctx.canny_gray8_dev(a, b, w, h, n, *params), tb.batch(h, w, n, 1),
                   tb.expand(canny_refs(shape, params), n), off, "%scanny %dx%d %r" % (tag, h, w, params))


def hough_of(pkg, frames, geom, threshold, max_lines):
    """(accum, lines, votes, count) of (k, h, w) frames by the reference, with the library's trig table"""
    h, w = frames.shape[1:]
    tc, ts = pkg.hough_trig_table(w, h, *geom)
    _, nr = pkg.hough_shape(w, h, *geom)
    return hr.hough_ref(frames, tc, ts, nr, threshold, max_lines, geom[0], geom[1], geom[2])


def hough_refs(pkg, shape, geom, select):
    return ref_of(("hough", shape, geom, select), lambda: hough_of(pkg, tf.mask_distinct(*shape), geom, *select))


def hough_parts(want, n, votes, own_accum, suffix=""):
    acc, lines, vts, count = [tb.expand(a, n) for a in want]
    parts = [("lines" + suffix, lines, 4)] + ([("votes" + suffix, vts, 4)] if votes else []) + [("count" + suffix, count, 4)]
    return parts + ([("accum" + suffix, acc, 4)] if own_accum else [])


def hough_call(ctx, d_in, d, w, h, n, geom, select, suffix=""):
    ctx.hough_lines_gray8_dev(d_in, d["lines" + suffix], d.get("votes" + suffix, 0), d["count" + suffix],
                              d.get("accum" + suffix, 0), w, h, n, geom[0], geom[1], select[0], select[1], geom[2], geom[3])


def run_hough(ctx, pkg, shape, geom, select, n, votes, own_accum, offs=OFF_WORDS):
    h, w = shape
    parts = hough_parts(hough_refs(pkg, shape, geom, select), n, votes, own_accum)
    tag = "hough %dx%d theta pi/%d thr %d max_lines %d votes %r own accum %r" % (
        h, w, round(np.pi / geom[1]), select[0], select[1], votes, own_accum)
    for off in offs:
        arena(ctx, lambda d_in, d: hough_call(ctx, d_in, d, w, h, n, geom, select), tf.mask_batch(h, w, n), parts, off, tag)


# ---- CLAHE and the adaptive threshold ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tb.G8_SHAPES, ids=shape_ids(tb.G8_SHAPES))
def test_clahe_frames_and_tables(ctx, pkg, shape):
    rows = rows_by_shape(tf.clahe_rows(pkg)).get(shape, [])
    assert rows and rows[0].params == (1, 1)
    for r in rows:
        for clip in tf.CLAHE_CLIPS:
            run_clahe(ctx, shape, r.params, clip, r.n)


def test_adaptive_threshold(ctx, pkg):
    rows = tf.adaptive_rows(pkg)
    assert len(rows) >= tf.MIN_ROWS["adaptive"]
    for r in rows:
        h, w = r.shape
        x, ref = tb.batch(h, w, r.n, 1), tb.expand(adaptive_refs(r.shape, r.params), r.n)
        for off in OFF_BYTES:
            one_output(ctx, lambda a, b: ctx.adaptive_threshold_gray8_dev(a, b, w, h, r.n, *r.params), x, ref, off,
                       "adaptive %dx%d %r" % (h, w, r.params))


# ---- labelling, hysteresis, Canny ----------------------------------------------------------------------------------------------
CCL_SHAPES = tb.G8_SHAPES + (tf.SEAM_SHAPE,)
CANNY_SHAPES = tb.G8_SHAPES + (tf.NMS_SHAPE,)


@pytest.mark.parametrize("shape", CCL_SHAPES, ids=shape_ids(CCL_SHAPES))
def test_labels_counts_and_statistics(ctx, pkg, shape):
    rows = rows_by_shape(tf.ccl_rows(pkg)).get(shape, [])
    assert len(rows) == 4
    for r in rows:
        run_ccl(ctx, shape, r.params[0], r.params[1], r.n)


def test_hysteresis(ctx, pkg):
    rows = tf.hyst_rows(pkg)
    assert len(rows) >= tf.MIN_ROWS["hysteresis"]
    for r in rows:
        run_hyst(ctx, r.shape, r.params, r.n)


def test_canny(ctx, pkg):
    rows = tf.canny_rows(pkg)
    assert len(rows) >= tf.MIN_ROWS["canny"]
    for r in rows:
        run_canny(ctx, r.shape, r.params, r.n)


# ---- Hough ------------------------------------------------------------------------------------------------------------------
HOUGH_SHAPES = tf.hough_shapes()


@pytest.mark.parametrize("shape", HOUGH_SHAPES, ids=shape_ids(HOUGH_SHAPES))
def test_hough_accumulator_and_lines(ctx, pkg, shape):
    """The accumulator call; the lines call at both theta steps, with more and with fewer peaks than lines, with and
    without d_votes, with the caller's accumulator in the arena and with the pooled one."""
    rows = rows_by_shape(tf.hough_rows(pkg)).get(shape, [])
    assert [r.params for r in rows] == list(tf.HOUGH_GEOMS)
    h, w = shape
    fine, coarse = rows
    more, fewer = tf.HOUGH_SELECT
    acc = tb.expand(hough_refs(pkg, shape, fine.params, more)[0], fine.n)
    for off in OFF_WORDS:
        one_output(ctx, lambda a, b: ctx.hough_accum_gray8_dev(a, b, w, h, fine.n, *fine.params),
                   tf.mask_batch(h, w, fine.n), acc, off, "hough accum %dx%d" % shape, align=4)
    run_hough(ctx, pkg, shape, fine.params, more, fine.n, votes=True, own_accum=True)
    run_hough(ctx, pkg, shape, fine.params, fewer, fine.n, votes=False, own_accum=False)
    run_hough(ctx, pkg, shape, fine.params, more, fine.n, votes=False, own_accum=False)
    run_hough(ctx, pkg, shape, coarse.params, more, coarse.n, votes=False, own_accum=True)
    run_hough(ctx, pkg, shape, coarse.params, fewer, coarse.n, votes=True, own_accum=False)
    run_hough(ctx, pkg, shape, coarse.params, fewer, coarse.n, votes=True, own_accum=True, offs=OFF_WORDS[:1])


# ---- pooled scratch in other orders ---------------------------------------------------------------------------------------------
POOL_SHAPES = {"ccl": ((5, 7), (13, 17), tf.SEAM_SHAPE), "hysteresis": ((5, 7), (13, 17), tf.SEAM_SHAPE),
               "canny": ((5, 7), (13, 17), tf.NMS_SHAPE)}


@pytest.mark.parametrize("order", ["shrinking", "growing"])
@pytest.mark.parametrize("feature", ["ccl", "hysteresis", "canny"])
def test_pooled_scratch_sized_by_another_call(pkg, feature, order):
    """The flat-block counts of the labelling and the parent array of hysteresis and Canny live in the context's pooled
    buffers.  A context of its own per order: thousands of frames before 64 (the buffer is larger than the second call
    needs, its tail holds the first call's content) and 64 before thousands (it has to grow)."""
    rows = {r.shape: r for r in tf.ROWS[feature](pkg)}
    with pkg.Context(0) as own:
        for shape in POOL_SHAPES[feature]:
            big = rows[shape].n
            for n in ((big, POOL_N) if order == "shrinking" else (POOL_N, big)):
                if feature == "ccl":
                    run_ccl(own, shape, 8, 4, n, OFF_WORDS[:1], order + " ")
                    run_ccl(own, shape, 4, 0, n, OFF_WORDS[1:], order + " ")
                elif feature == "hysteresis":
                    run_hyst(own, shape, tf.HYST_PARAMS[1], n, OFF_BYTES[:1], order + " ")
                    run_hyst(own, shape, tf.HYST_PARAMS[0], n, OFF_BYTES[1:], order + " ")
                else:
                    run_canny(own, shape, tf.CANNY_PARAMS[0], n, OFF_BYTES[:1], order + " ")
                    run_canny(own, shape, tf.CANNY_PARAMS[1], n, OFF_BYTES[1:], order + " ")


def test_histogram_and_table_rows_change_meaning_between_calls(pkg):
    """Equalize, CLAHE 8 x 8, Otsu, CLAHE 2 x 2 on one shape in a context of its own: the pooled histograms and tables
    hold one row per frame, then 64 per frame, then one, then four."""
    shape = HIST_SHAPE
    n = min(r.n for r in tf.clahe_rows(pkg) if r.shape == shape)     # the count of its 8 x 8 tables
    h, w = shape
    d, x = tb.distinct(h, w, 1), tb.batch(h, w, n, 1)
    with pkg.Context(0) as own:
        for step in range(2):                                  # twice: the second round starts from CLAHE 2 x 2's rows
            one_output(own, lambda a, b: own.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, a, b, w, h, n, 0, 0.0), x,
                       tb.expand(ref_of(("equalize", shape), lambda: equalize_ref(d)), n), OFF_BYTES[step], "equalize")
            run_clahe(own, shape, (8, 8), 2.0, n, OFF_BYTES[step:step + 1], lut_offs=OFF_WORDS[step:step + 1])
            one_output(own, lambda a, b: own.filter_dev(pkg.FILTER_OTSU_GRAY8, a, b, w, h, n, 0, 0.0), x,
                       tb.expand(ref_of(("otsu", shape), lambda: otsu_ref(d)), n), OFF_BYTES[step], "otsu")
            run_clahe(own, shape, (2, 2), 40.0, n, OFF_BYTES[step:step + 1], lut_offs=OFF_WORDS[step:step + 1])


def test_hough_pooled_accumulator_and_table_change_hands_without_a_sync(pkg):
    """Three lines calls on the pooled accumulator with nothing between them: theta = pi / 180, then pi / 90 (another
    table key, a smaller accumulator), then pi / 180 on a larger shape (a larger one).  The library orders the table
    upload itself; the one sync is the arena's, after the third call."""
    small, large, n, select = (5, 7), (13, 17), HOUGH_POOL_N, tf.HOUGH_SELECT[0]
    steps = [(small, tf.HOUGH_GEOMS[0], "a"), (small, tf.HOUGH_GEOMS[1], "b"), (large, tf.HOUGH_GEOMS[0], "c")]
    xs = {s: tf.mask_batch(s[0], s[1], n) for s in (small, large)}
    x = np.concatenate([xs[small].ravel(), xs[large].ravel()])
    at_in = {small: 0, large: xs[small].size}
    parts = []
    for shape, geom, suffix in steps:
        parts += hough_parts(hough_refs(pkg, shape, geom, select), n, True, False, suffix)

    with pkg.Context(0) as own:
        def call(d_in, d):
            for shape, geom, suffix in steps:
                hough_call(own, d_in + at_in[shape], d, shape[1], shape[0], n, geom, select, suffix)

        for off in OFF_WORDS:
            arena(own, call, x, parts, off, "hough pooled, three calls")


# ---- two chains on the device, one sync at the end ------------------------------------------------------------------------------
def _with_intermediate(ctx, nbytes, body):
    d_mid = ctx.alloc(nbytes)
    try:
        ctx.h2d(d_mid, np.full(nbytes, 0xA5, np.uint8))
        ctx.sync()
        return body(d_mid)
    finally:
        ctx.sync()
        ctx.free(d_mid)


def test_clahe_feeds_canny(ctx):
    """The intermediate is the output of one multi-launch call and the input of the next on the same stream."""
    (h, w), n = CHAIN_SHAPE, CHAIN_N
    grid, clip, params = (2, 2), 2.0, tf.CANNY_PARAMS[0]
    mid14, _ = clahe_refs(CHAIN_SHAPE, grid, clip)
    want = tb.expand(ref_of(("clahe-canny", CHAIN_SHAPE), lambda: cr.canny_ref(mid14, *params)), n)

    def chain(d_mid, off):
        def call(d_in, d_out):
            ctx.clahe_gray8_dev(d_in, d_mid, w, h, n, clip, grid[0], grid[1])
            ctx.canny_gray8_dev(d_mid, d_out, w, h, n, *params)
        one_output(ctx, call, tb.batch(h, w, n, 1), want, off, "clahe -> canny")

    for off in OFF_BYTES:
        _with_intermediate(ctx, n * h * w + 16, lambda d_mid: chain(d_mid + off[1], off))


def test_canny_feeds_hough_lines(ctx, pkg):
    (h, w), n = CHAIN_SHAPE, CHAIN_N
    params, geom, select = tf.CANNY_PARAMS[0], tf.HOUGH_GEOMS[0], (2, 16)
    edges14 = canny_refs(CHAIN_SHAPE, params)
    assert edges14[:tb.P].any(axis=(1, 2)).all()               # every member of the cycle has edges to vote with
    parts = hough_parts(ref_of(("canny-hough", CHAIN_SHAPE), lambda: hough_of(pkg, edges14, geom, *select)), n, True, False)

    def chain(d_mid, off):
        def call(d_in, d):
            ctx.canny_gray8_dev(d_in, d_mid, w, h, n, *params)
            hough_call(ctx, d_mid, d, w, h, n, geom, select)
        arena(ctx, call, tb.batch(h, w, n, 1), parts, off, "canny -> hough lines")

    for off in OFF_WORDS:
        _with_intermediate(ctx, n * h * w + 16, lambda d_mid: chain(d_mid + off[0], off))
