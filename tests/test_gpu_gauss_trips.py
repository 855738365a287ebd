"""GPU suite (-m gpu): the row loop of gauss_slide.hip, position by position.

A 3-channel pass over a band runs a prologue of warm-up rows, whole trips of K rows and a guarded remainder; a row that
stops the pass is only recorded and the pass ends at the trip's end, the rows of that trip stored regardless and the
band redone by the pass that follows.  So what matters is WHERE in that structure an event falls: every case here puts
one at every row of a frame whose bands walk down and up and whose last band's height takes every residue against the
trip length.  Every output is compared bit for bit with the LDS-tiled kernel (IMPL_TILE computes alpha like any other
channel and has no such structure) and within 1 LSB per channel with the CPU path, the FAST Gaussian's tolerance.

The cases of one frame height travel as ONE batch, frame y carrying the event at row y: a work item is one wave on one
(frame, band, strip), so a batch of h frames is h independent cases in two launches."""
import numpy as np
import pytest

from conftest import rand_rgba

pytestmark = pytest.mark.gpu

W = 512          # 3 strips
_X = 241         # the event column of the single-pixel cases
HEIGHTS = (49, 50, 51, 52, 53)
KS = [(3, 0.8), (5, 1.5), (7, 2.0)]


def _both(ctx, pkg, frames, k, sigma):
    ctx.set_gauss_mode(pkg.GAUSS_FAST)
    ctx.set_impl(pkg.IMPL_TILE)
    tiled = ctx.gauss(frames, k, sigma)
    ctx.set_impl(pkg.IMPL_VALU)
    slide = ctx.gauss(frames, k, sigma)
    ctx.set_impl(pkg.IMPL_AUTO)
    return tiled, slide


def _check_batch(ctx, pkg, oracle, frames, k, sigma, what):
    tiled, slide = _both(ctx, pkg, frames, k, sigma)
    for f in range(frames.shape[0]):
        assert np.array_equal(slide[f], tiled[f]), (what, frames.shape, k, f)
        ref = oracle.gauss_rgba(frames[f], k, sigma)
        assert np.abs(slide[f].astype(np.int16) - ref.astype(np.int16)).max() <= 1, (what, frames.shape, k, f)


@pytest.fixture(scope="module")
def bases(oracle):
    """One opaque frame per height, shared and never written to."""
    out = {}
    for h in HEIGHTS:
        b = oracle.synth_rgba(W, h, 1, first_frame=h, mode=1)[0]
        assert (b[..., 3] == 255).all()
        b.setflags(write=False)
        out[h] = b
    return out


@pytest.mark.parametrize("k,sigma", KS)
def test_single_pixel_at_every_row(ctx, pkg, oracle, bases, k, sigma):
    """One alpha = 7 pixel at (y, 241) for every row y: the alpha = 255 pass meets a row of mixed alphas at every trip
    position, in the warm-up rows, in the remainder, at the clamped top and bottom rows and in a neighbour band's halo,
    and the 4-channel pass redoes the band."""
    for h in HEIGHTS:
        frames = np.repeat(bases[h][None], h, axis=0)
        for y in range(h):
            frames[y, y, _X, 3] = 7
        _check_batch(ctx, pkg, oracle, frames, k, sigma, "pixel")


@pytest.mark.parametrize("k,sigma", KS)
def test_constant_alpha_from_every_row(ctx, pkg, oracle, bases, k, sigma):
    """Alpha = 128 from row y to the bottom over the whole width: the alpha = 255 pass stops at a uniform row at every
    trip position and the constant-alpha pass takes the band — from its first row (y = 0, and y = a band's first input
    row) with the rows already in flight handed over."""
    for h in HEIGHTS:
        frames = np.repeat(bases[h][None], h, axis=0)
        for y in range(h):
            frames[y, y:, :, 3] = 128
        _check_batch(ctx, pkg, oracle, frames, k, sigma, "const from row")


@pytest.mark.parametrize("k,sigma", KS)
def test_uniform_then_change(ctx, pkg, oracle, bases, k, sigma):
    """Alpha = 128 from row y, 9 from row y + 2: the constant-alpha pass meets a window that spans two values two rows
    after it took over, at every trip position."""
    for h in HEIGHTS:
        frames = np.repeat(bases[h][None], h, axis=0)
        for y in range(h):
            frames[y, y:, :, 3] = 128
            frames[y, y + 2:, :, 3] = 9
        _check_batch(ctx, pkg, oracle, frames, k, sigma, "128 then 9")


@pytest.mark.parametrize("k,sigma", [(5, 1.5), (7, 2.0), (9, 2.5)])
@pytest.mark.parametrize("w", [75, 250, 1022, 1023])
def test_ragged_widths_with_constant_alpha(ctx, pkg, oracle, k, sigma, w):
    """Rows that are not a multiple of 4 pixels (w % 4 = 3, 2, 2, 3), noisy RGB up to the right-most column, alpha
    constant or piecewise constant by rows: every band of the frame hands its first row from the alpha = 255 pass to the
    constant-alpha pass, in an edge strip whose lanes past the row's end shift that row into place — once."""
    h = 53
    img = rand_rgba(h, w, seed=w + k, alpha=128)
    by_rows = img.copy()
    by_rows[..., 3] = (10 + np.arange(h) // 7)[:, None]
    top_opaque = img.copy()
    top_opaque[:20, :, 3] = 255
    frames = np.stack([img, by_rows, top_opaque])
    _check_batch(ctx, pkg, oracle, frames, k, sigma, "ragged")
    for f in range(3):   # and as single frames: frame 0 of a ragged batch is the only 16-byte-aligned one
        _check_batch(ctx, pkg, oracle, frames[f:f + 1], k, sigma, "ragged, single")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k,sigma", [(3, 0.8), (5, 1.5)])
def test_lockstep_strips_stop_at_different_rows_of_one_trip(ctx, pkg, oracle, k, sigma):
    """1100 frames of 960 x 48: four strips, so a workgroup is the four strips of one band, and >= 8192 work items, the
    launcher's lock-step threshold.  The four strips of one workgroup meet their events at different rows of ONE trip
    (k = 5: four rows; k = 3: the three a trip has), in a band that walks down and in one that walks up; each then
    runs on to the trip's end, barriers included, and starts the next pass while its partners are still in this one."""
    w, h, n = 960, 48, 1100
    per = w * h * 4
    assert (w // 4) % 60 == 0 and ((w // 4) // 60) % 4 == 0 and 4 * (-(-h // 24)) * n >= 8192
    d_in = ctx.alloc(per * n)
    ctx.synth_dev(d_in, w, h, n, first_frame=0, seed=0x5EED, mode=0)
    frames = np.empty((n, h, w, 4), np.uint8)
    ctx.d2h(frames, d_in)
    rng = np.random.default_rng(k)
    K = k
    # rows of one trip: a band of the top half walks down from y = 0 (arrival i <-> row i - R, trips start at arrival
    # 2R), a band of the bottom half walks up from y = 47 (arrival i <-> row 47 + R - i)
    R = k // 2
    down = [2 * R + K - R + u for u in range(K)]          # second trip of the band at y0 = 0
    up = [47 + R - (2 * R + K + u) for u in range(K)]     # second trip of the bottom band
    touched = [2, 4, 6, 8, 10, 12, 1099]
    for f, rows in ((2, down), (4, up)):                  # one pixel per strip, four rows of the trip
        for s in range(4):
            frames[f, rows[s % K], 240 * s + 17, 3] = 7
    for f, rows in ((6, down), (8, up)):                  # a constant from that row on, per strip
        for s in range(4):
            y = rows[s % K]
            if rows is down:
                frames[f, y:, 240 * s:240 * (s + 1), 3] = 128
            else:
                frames[f, :y + 1, 240 * s:240 * (s + 1), 3] = 128
    for s in range(4):                                    # mixed: pixel, constant, noise, nothing
        y = down[s % K]
        if s == 0:
            frames[10, y, 5, 3] = 0
        elif s == 1:
            frames[10, y:, 240:480, 3] = 200
        elif s == 2:
            frames[10, y:, 480:720, 3] = rng.integers(0, 256, (h - y, 240), dtype=np.uint8)
    frames[12, :, :, 3] = 77                              # the constant-alpha pass everywhere, from every first row
    frames[1099, h - 1, w - 1, 3] = 1                     # the very last pixel of the launch
    ctx.h2d(d_in, frames)
    outs = {}
    for impl in (pkg.IMPL_TILE, pkg.IMPL_VALU):
        ctx.set_gauss_mode(pkg.GAUSS_FAST)
        ctx.set_impl(impl)
        d_out = ctx.alloc(per * n)
        ctx.filter_dev(pkg.FILTER_GAUSS, d_in, d_out, w, h, n, k, sigma)
        got = np.empty((n, h, w, 4), np.uint8)
        ctx.d2h(got, d_out)
        ctx.free(d_out)
        outs[impl] = got
    ctx.set_impl(pkg.IMPL_AUTO)
    ctx.free(d_in)
    assert np.array_equal(outs[pkg.IMPL_VALU], outs[pkg.IMPL_TILE])
    for f in touched + [0]:
        ref = oracle.gauss_rgba(frames[f], k, sigma)
        assert np.abs(outs[pkg.IMPL_VALU][f].astype(np.int16) - ref.astype(np.int16)).max() <= 1, f
