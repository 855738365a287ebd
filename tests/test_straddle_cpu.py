"""What test_gpu_straddle.py's inputs must be for its bit-identity checks to mean something, shown with the CPU oracle
and numpy alone (no GPU).

straddle_cases.py builds frames out of mined windows on which the CPU path's truncated Gaussian sum differs from the sum
a subtly wrong kernel would compute (rows bottom-up, kx outer, columns right to left, the exact sum, a contracted
multiply-add).  Here: the numpy chain IS the oracle's; every committed window is critical for the alternates it is
listed under and the maker reproduces them; in every frame the GPU suite runs, every alternate changes bytes (of the
Gaussian and, for the pipeline frames, of the final edge image); the critical pixels reach every pixel position of a
lane, the first, last and halo lanes of the strips, and in the sparse frames mostly fewer than three lanes of a strip per
row; and the separable pair-form sum the exact-by-exception kernels evaluate stays within delta_bound_k of the CPU
chain, on every fixture window and under a hill-climb that maximises the distance.
"""
import importlib.util
import os

import numpy as np
import pytest

import straddle_cases as sc
from test_gauss_tables_cpu import delta_bound_k, separable_factor, symmetric
from test_gpu_gray8 import gauss_r

MIN_GAUSS_BYTES = 16      # bytes of the Gaussian result every alternate must change, per frame
MIN_PIPE_BYTES = 8        # bytes of the pipeline's edge image


@pytest.fixture(scope="module")
def tables(oracle):
    return {k: oracle.gauss_weights(k, s) for k, s in sc.SIZES}


_analysed = {}


def analysed(tables, kind, shape, k, phase=0):
    """[(plane, ref, {alt: blurred})] for the two planes of plane_pair, computed once per module."""
    key = (kind, shape, k, phase)
    if key not in _analysed:
        planes = sc.plane_pair(kind, shape[0], shape[1], k, phase)
        _analysed[key] = [(p,) + sc.alternate_blurs(p, tables[k]) for p in planes]
    return _analysed[key]


def changed(tables, kind, shape, k, phase, frame):
    """{alt: bytes of plane `frame` the alternate changes}"""
    _, ref, alts = analysed(tables, kind, shape, k, phase)[frame]
    return {a: int((alts[a] != ref).sum()) for a in sc.ALTS}


def any_critical(tables, kind, shape, k, frame=0):
    _, ref, alts = analysed(tables, kind, shape, k)[frame]
    return np.any([alts[a] != ref for a in sc.ALTS], axis=0)


# ---- the numpy restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [k for k, _ in sc.SIZES])
def test_numpy_chain_is_the_oracle(oracle, tables, k):
    y = sc.dense_plane(41, 83, k, seed=k) if k <= 17 else sc.dense_plane(70, 75, k, seed=k)
    assert np.array_equal(sc.blur_plane(y, tables[k]), gauss_r(oracle, y, k, weights=tables[k]))
    ref, _ = sc.alternate_blurs(y, tables[k])
    assert np.array_equal(ref, sc.blur_plane(y, tables[k]))


def test_alternates_on_candidate_windows_equal_the_whole_frame_chains(tables):
    """alternate_blurs evaluates the chains only where the exact sum is within k^2 2^-16 of an integer."""
    for k, shape in ((3, (40, 90)), (7, (50, 64)), (17, (40, 60))):
        y = sc.beside_flat_plane(shape[0], shape[1], k, seed=5)
        _, alts = sc.alternate_blurs(y, tables[k])
        for a in sc.ALTS:
            assert np.array_equal(alts[a], sc.blur_plane(y, tables[k], a)), (k, a)


def test_double_holds_every_partial_sum_exactly(tables):
    """Alternates d and e are evaluated in double; exact only while the smallest weight's last bit and 2^8 fit 53 bits."""
    for k, t in tables.items():
        assert sc.span_ok(t), k
    assert not sc.span_ok(np.array([[1e-20, 0.5]], np.float32))
    # and the fused chain is not the plain one: on random windows the sums differ in the last bit somewhere
    wins = np.random.default_rng(1).integers(0, 256, (2000, 5, 5), dtype=np.uint8)
    assert (sc.window_sums(wins, tables[5], "e") != sc.window_sums(wins, tables[5])).any()


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_fixture_windows_are_critical_and_the_quotas_hold(tables):
    interior, edges = sc.load_fixture()
    assert sorted(interior) == sorted(k for k, _ in sc.SIZES) and sorted(edges) == sorted(sc.EDGE_KS)
    for k, (wins, letters) in interior.items():
        assert wins.shape[1:] == (k, k) and wins.dtype == np.uint8
        assert letters == sc.critical_letters(wins, tables[k]), k
        assert all(letters), k
        for a in sc.ALTS:
            assert sum(a in lt for lt in letters) >= sc.quota(k), (k, a)
        assert len(np.unique(wins.reshape(len(wins), -1), axis=0)) == len(wins), k


def test_edge_windows_are_clamped_expansions_and_critical(tables):
    _, edges = sc.load_fixture()
    for k, items in edges.items():
        r = k // 2
        wins = np.stack([e[3] for e in items])
        assert [e[4] for e in items] == sc.critical_letters(wins, tables[k]), k
        for kind in sc.EDGE_KINDS:
            mine = [e for e in items if e[0] == kind]
            assert len(mine) >= sc.EDGE_QUOTA, (k, kind)
            for _, cy, cx, win, letters in mine:
                assert letters and 0 <= cy < r and 0 <= cx < r
                assert np.array_equal(win, sc.expand_edge(win, kind, cy, cx)), (k, kind, cy, cx)
                rows, cols = sc.edge_maps(kind, cy, cx, k)
                assert (rows != np.arange(k)).any() or (cols != np.arange(k)).any()     # really at an edge
            assert {(e[1] if kind not in ("left", "right") else e[2]) for e in mine} == set(range(r)), (k, kind)


def test_edge_windows_sit_on_the_frame_edges_where_the_oracle_sees_them(oracle, tables):
    """A window placed on an edge is read by the CPU path through its clamp rule: the blurred byte at its centre is the
    window's own byte."""
    for k in sc.EDGE_KS:
        h, w = 97, 250
        y = sc.dense_plane(h, w, k, seed=3)
        ref = gauss_r(oracle, y, k, weights=tables[k])
        pad = np.pad(y, k // 2, mode="edge")
        seen = set()
        for kind, cy, cx, win, _ in sc.load_fixture()[1][k]:
            ys = {"top": [cy], "top-left": [cy], "bottom": [h - 1 - cy], "bottom-right": [h - 1 - cy]}.get(kind, range(h))
            xs = {"left": [cx], "top-left": [cx], "right": [w - 1 - cx], "bottom-right": [w - 1 - cx]}.get(kind, range(w))
            for yy in ys:
                for xx in xs:
                    if np.array_equal(pad[yy:yy + k, xx:xx + k], win):
                        assert ref[yy, xx] == sc.window_bytes(win[None], tables[k])[0]
                        seen.add(kind)
        assert seen == set(sc.EDGE_KINDS), (k, seen)


def test_the_maker_reproduces_the_committed_fixture(oracle):
    """For k = 3 and 5 here (every size draws from its own generator); the whole file takes the maker a quarter of a
    minute."""
    spec = importlib.util.spec_from_file_location("make_straddle", os.path.join(sc.HERE, "golden", "make_straddle.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    import json
    committed = json.load(open(sc.FIXTURE))
    made = maker.build(oracle, sizes=sc.SIZES[:2])
    for part in ("interior", "edges"):
        for k in ("3", "5"):
            assert made[part][k] == committed[part][k], (part, k)
    assert open(sc.FIXTURE).read() == maker.dumps(committed)
    assert os.path.getsize(sc.FIXTURE) < 1 << 20


# ---- every alternate changes bytes of every frame --------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 7, 9, 17])
def test_every_alternate_changes_bytes_of_every_rgba_gaussian_frame(tables, k):
    for shape in sc.gauss_rgba_shapes(k):
        for kind in sc.kinds_of(k):
            batch = sc.rgba_gauss_batch(kind, shape[0], shape[1], k, opaque=False)
            for c in range(4):      # the batch's channels are the analysed planes
                assert np.array_equal(batch[..., c], sc.plane_pair(kind, shape[0], shape[1], k, phase=11 * c))
            opaque = sc.rgba_gauss_batch(kind, shape[0], shape[1], k, opaque=True)
            assert np.array_equal(opaque[..., :3], batch[..., :3]) and (opaque[..., 3] == 255).all()
            for frame in range(2):
                per = [changed(tables, kind, shape, k, 11 * c, frame) for c in range(4)]
                for a in sc.ALTS:
                    assert sum(p[a] for p in per) >= MIN_GAUSS_BYTES, (k, shape, kind, frame, a)
                    assert sum(p[a] for p in per[:3]) >= MIN_GAUSS_BYTES, (k, shape, kind, frame, a, "opaque")
                    if kind == "dense":      # the 4-channel walk is not carried by one channel alone
                        assert all(p[a] > 0 for p in per), (k, shape, kind, frame, a)


@pytest.mark.parametrize("k", [k for k, _ in sc.SIZES])
def test_every_alternate_changes_bytes_of_every_gray8_frame(tables, k):
    for shape in sc.gray8_shapes(k):
        for kind in sc.kinds_of(k):
            for frame in range(2):
                n = changed(tables, kind, shape, k, 0, frame)
                for a in sc.ALTS:
                    assert n[a] >= MIN_GAUSS_BYTES, (k, shape, kind, frame, a, n)


@pytest.mark.parametrize("k", sc.SLIDE_KS)
def test_every_alternate_changes_the_rgba_pipeline_output(oracle, tables, k):
    """Neither the second luminance step nor the Sobel may hide the flipped byte: at least 8 bytes of the final edge image
    move, per frame."""
    post = sc.rgba_pipe_post(oracle)
    shapes = sc.PIPE_SHAPES + ((sc.SHAPE_PIPE8,) if k <= 5 else ())
    for shape in shapes:
        for kind in sc.kinds_of(k):
            for frame, (_, ref, alts) in enumerate(analysed(tables, kind, shape, k)):
                edges = post(ref)
                for a in sc.ALTS:
                    n = int((post(alts[a]) != edges).sum())
                    assert n >= MIN_PIPE_BYTES, (k, shape, kind, frame, a, n)


@pytest.mark.parametrize("k", sc.GRAY8_PIPE_KS)
def test_every_alternate_changes_the_gray8_pipeline_output(oracle, tables, k):
    for shape in sc.gray8_shapes(k):
        for kind in sc.kinds_of(k):
            for frame, (_, ref, alts) in enumerate(analysed(tables, kind, shape, k)):
                edges = oracle.sobel_gray(ref)
                for a in sc.ALTS:
                    n = int((oracle.sobel_gray(alts[a]) != edges).sum())
                    assert n >= MIN_PIPE_BYTES, (k, shape, kind, frame, a, n)


@pytest.mark.parametrize("coloured", [False, True])
def test_pipeline_frames_have_the_critical_plane_as_their_gray_image(oracle, tables, coloured):
    for k, shape, kind in ((3, sc.SHAPE_RAGGED, "dense"), (5, sc.SHAPE_ALIGNED, "sparse"), (7, sc.SHAPE_RAGGED, "beside-flat")):
        batch, planes = sc.rgba_pipe_batch(oracle, kind, shape[0], shape[1], k, coloured)
        assert np.array_equal(planes, sc.plane_pair(kind, shape[0], shape[1], k))
        for f in range(2):
            assert np.array_equal(oracle.gray_rgba_1ch(batch[f]), planes[f]), (k, f)
            ref = oracle.pipeline_rgba(batch[f], k, weights=tables[k])
            assert np.array_equal(ref, sc.rgba_pipe_post(oracle)(sc.blur_plane(planes[f], tables[k]))), (k, f)
        grey = (batch[..., 0] == batch[..., 1]) & (batch[..., 1] == batch[..., 2])
        if coloured:
            assert grey.mean() < 0.05
        else:   # R = G = B wherever some grey pixel has the level: the CPU formula's truncation skips one level in five
            has_grey = np.isin(np.arange(256), [oracle.gray_px(u, u, u) for u in range(256)])
            assert has_grey.mean() > 0.75 and np.array_equal(grey, has_grey[planes]), k
    lut_grey, lut_col = sc.gray_lut(oracle)
    for v in range(256):
        assert oracle.gray_px(*lut_grey[v]) == v and all(oracle.gray_px(*p) == v for p in lut_col[v])


# ---- where the critical pixels sit -----------------------------------------------------------------------------------
def _cases_px(k):
    out = [(sc.SHAPE_ALIGNED, 4), (sc.SHAPE_RAGGED, 4)]
    if k <= 5:
        out += [(sc.SHAPE_PIPE8, 4), (sc.SHAPE_PIPE8, 8)]
    return out


@pytest.mark.parametrize("k", sc.SLIDE_KS)
def test_critical_pixels_reach_every_pixel_position_and_the_strip_edges(tables, k):
    for shape, px in _cases_px(k):
        h, w = shape
        cols = np.nonzero(any_critical(tables, "dense", shape, k).any(axis=0))[0]
        assert set(cols % 8) == set(range(8)), (k, shape)
        quads = set(cols // px)
        strips = sc.strip_quads(w, px)
        assert len(strips) >= 2, (k, shape, px)
        for s, lanes in enumerate(strips):
            for name, q in lanes.items():
                assert q is None or q in quads, (k, shape, px, s, name, q)
        # both halo lanes of a strip lie in the image for every strip but the first and the last
        assert all(lanes["halo_left"] is not None and lanes["halo_right"] is not None for lanes in strips[1:-1])
        if w >= 1000:
            assert len(strips) - 2 >= (2 if px == 4 else 1)
        # rows: every group of 8 rows holds critical pixels, and the two frames of a batch put them on different rows
        # mod k (the block rows of the second start k / 2 + 1 rows lower), so on different ring slots of a band
        res = []
        for frame in range(2):
            rows = np.nonzero(any_critical(tables, "dense", shape, k, frame).any(axis=1))[0]
            assert len(set(rows // 8)) == (h + 7) // 8, (k, shape, frame)
            inner = np.nonzero(any_critical(tables, "dense", shape, k, frame)[:, 2 * k:w - 2 * k].any(axis=1))[0]
            res.append(set(inner[(inner >= k) & (inner < h - 2 * k)] % k))    # away from the edge windows
        assert res == [{k // 2}, {0}], (k, shape, res)


def test_strip_plan_restated():
    assert sc.strip_plan(3840) == (16, 60) and sc.strip_plan(3840, 8) == (8, 60)      # slide_common.hpp's own examples
    assert sc.strip_plan(512) == (3, 43) and sc.strip_plan(250) == (2, 32) and sc.strip_plan(1000, 8) == (3, 42)
    assert sc.strip_quads(250)[-1] == {"first": 32, "last": 62, "halo_left": 31, "halo_right": None}


@pytest.mark.parametrize("k", sc.SLIDE_KS)
def test_sparse_frames_mostly_flag_fewer_than_three_lanes_of_a_strip(tables, k):
    """exact_blur_row enters flat_windows only when three or more lanes of the wave are flagged; rows with one or two
    critical pixels per strip go straight to the chain."""
    for shape in sc.PIPE_SHAPES:
        crit = any_critical(tables, "sparse", shape, k)
        nstrips, lanes = sc.strip_plan(shape[1])
        per_strip = np.stack([crit[:, s * lanes * 4:(s + 1) * lanes * 4].sum(axis=1) for s in range(nstrips)])
        holds = crit.any(axis=1)
        few = holds & (per_strip.max(axis=0) < 3)
        assert holds.sum() >= 10 and few.sum() * 2 >= holds.sum(), (k, shape, int(few.sum()), int(holds.sum()))
        # the same with the widest strips there are, 62 lanes of 4 pixels
        per248 = np.stack([crit[:, x:x + 248].sum(axis=1) for x in range(0, shape[1], 248)])
        assert (holds & (per248.max(axis=0) < 3)).sum() * 2 >= holds.sum(), (k, shape)


# ---- the bound delta -------------------------------------------------------------------------------------------------
def _delta_tables(tables, k):
    w1, ok = separable_factor(tables[k])
    assert ok and symmetric(w1)
    bound = delta_bound_k(w1, tables[k])
    assert bound < 0.01          # the table takes the exact-by-exception arithmetic
    return w1, np.float32(bound)


def _distance(win, w1, w2, delta):
    """(|S - S_cpu|, S', S_cpu): S' = the kernels' pair-form sum with delta riding on the centre tap, S = S' - delta."""
    s_cpu = float(sc.window_sums(win[None], w2)[0])
    s_sep = sc.pair_form_sum(win, w1, float(delta))
    return abs(s_sep - float(delta) - s_cpu), s_sep, s_cpu


def _check_exception_rule(win, w1, w2, delta):
    """The kernel's own decision: where fract(S') >= 2 delta it stores trunc(S') without asking the chain."""
    d, s_sep, s_cpu = _distance(win, w1, w2, delta)
    two_delta = float(np.float32(2.0) * delta)
    if s_sep - np.floor(s_sep) >= two_delta:
        assert min(int(s_sep), 255) == min(int(s_cpu), 255), (win.tolist(), s_sep, s_cpu)
    return d


def test_pair_form_sum_rounds_once():
    """The integer fma: ties go to even, a value just above a tie goes up where the route through double loses the bit
    that says so, and on the kernel's own magnitudes the result is the float32 nearest to the exact rational."""
    from fractions import Fraction
    one, tie = sc._split(1.0), sc._split(2.0 ** -24)
    assert sc._value(sc._fma(one, one, tie)) == 1.0                                    # 1 + 2^-24: tie, to even
    assert sc._value(sc._fma(sc._split(1.0 + 2.0 ** -23), one, tie)) == 1.0 + 2.0 ** -22   # odd neighbour: tie goes up
    assert sc._value(sc._round24((1 << 60) + (1 << 36) + 1, -60)) == 1.0 + 2.0 ** -23   # 1 + 2^-24 + 2^-60: above the tie
    assert float(np.float32(np.float64(1.0) + np.float64(2.0 ** -24 + 2.0 ** -60))) == 1.0   # double drops 2^-60 first
    rng = np.random.default_rng(0)
    for _ in range(300):
        x, y, z = (float(np.float32(v)) for v in rng.random(3) * (510.0, 0.3, 255.0))
        got = sc._value(sc._fma(sc._split(x), sc._split(y), sc._split(z)))
        assert got == float(np.float32(got))
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        for other in (np.nextafter(np.float32(got), np.float32(-1.0)), np.nextafter(np.float32(got), np.float32(1e9))):
            assert abs(Fraction(got) - exact) <= abs(Fraction(float(other)) - exact)


@pytest.mark.parametrize("k", [k for k, _ in sc.SIZES])
def test_pair_form_sum_stays_within_delta_on_every_fixture_window(tables, k):
    w1, delta = _delta_tables(tables, k)
    interior, edges = sc.load_fixture()
    wins = list(interior[k][0]) + [e[3] for e in edges.get(k, [])]
    worst = max(_check_exception_rule(w, w1, tables[k], delta) for w in wins)
    print("k = %d: max |S - S_cpu| / delta over %d fixture windows = %.4f (delta = %.3e)" % (k, len(wins), worst / float(delta),
                                                                                             float(delta)))
    assert worst <= float(delta), (k, worst, float(delta))


@pytest.mark.parametrize("k", sc.SLIDE_KS)
def test_hill_climb_cannot_push_the_pair_form_sum_past_delta(tables, k):
    """Seeded: 4 starts of 1000 steps; a step changes one byte (to a random value, or by one) and is kept when the
    distance does not fall.  A ratio above 1 is a bug in delta_bound_k even where no byte has moved yet."""
    w1, delta = _delta_tables(tables, k)
    rng = np.random.default_rng(900 + k)
    best = 0.0
    for start in range(4):
        win = rng.integers(0, 256, (k, k), dtype=np.uint8)
        if start == 0:      # the worst fixture window
            cands = sc.load_fixture()[0][k][0]
            win = max(cands, key=lambda c: _distance(c, w1, tables[k], delta)[0]).copy()
        cur = _check_exception_rule(win, w1, tables[k], delta)
        for _ in range(1000):
            y, x = rng.integers(0, k, 2)
            old = win[y, x]
            win[y, x] = rng.integers(0, 256) if rng.random() < 0.5 else np.clip(int(old) + rng.choice((-1, 1)), 0, 255)
            new = _check_exception_rule(win, w1, tables[k], delta)
            if new >= cur:
                cur = new
            else:
                win[y, x] = old
        best = max(best, cur)
    print("k = %d: hill-climbed max |S - S_cpu| / delta = %.4f" % (k, best / float(delta)))
    assert best <= float(delta), (k, best, float(delta))
