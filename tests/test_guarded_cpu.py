"""tests/guarded.py against a fake context (a bytearray for device memory) and fake kernels written in numpy: the arena
accepts a correct writer and sees every kind of mistake it exists for.  No GPU."""
import numpy as np
import pytest

import guarded


class FakeCtx:
    """ctx.alloc / free / h2d / d2h / sync over one bytearray.  Like a pooled allocator it hands the same address out
    again after a free and never clears it; the address is deliberately not 256-byte aligned."""
    BASE = 0x7F0000001010

    def __init__(self, size=1 << 16):
        self.mem = np.zeros(size, np.uint8)
        self.live = None
        self.syncs = 0
        self.touched = []   # (lo, hi) of every access: nothing may leave the live allocation

    def _at(self, p, n):
        assert self.live is not None
        lo = p - self.BASE
        assert 0 <= lo and lo + n <= self.live, "access outside the allocation"
        self.touched.append((lo, lo + n))
        return self.mem[lo:lo + n]

    def alloc(self, n):
        assert self.live is None and n <= self.mem.size
        self.live = n
        return self.BASE

    def free(self, p):
        assert p == self.BASE and self.live is not None
        self.live = None

    def h2d(self, d, arr):
        self._at(d, arr.nbytes)[:] = np.ascontiguousarray(arr).view(np.uint8).ravel()

    def d2h(self, arr, d):
        arr.view(np.uint8).ravel()[:] = self._at(d, arr.nbytes)

    def sync(self):
        self.syncs += 1


N = 75 * 3   # a ragged 1-byte-per-pixel row length: no multiple of 4


def reference(x):
    """out[i] = x[i] + x[i + 1] (mod 256), clamp-to-edge."""
    return x + np.append(x[1:], x[-1:])


def writer(ctx, span=None, skip=None, clamp=True):
    """A kernel: the reference operation written to d_out; `span` = (first, last) byte offsets relative to the output
    that are overwritten with 0xEE as well, `skip` = (first, last) output bytes that are not stored, clamp=False reads
    the byte after the input instead of clamping."""
    def call(d_in, d_out):
        x = ctx._at(d_in, N + 1).copy()
        out = reference(x[:N])
        if not clamp:
            out[-1] = x[N - 1] + x[N]
        keep = ctx._at(d_out, N).copy()
        if skip:
            out[skip[0]:skip[1]] = keep[skip[0]:skip[1]]
        ctx._at(d_out, N)[:] = out
        if span:
            ctx._at(d_out + span[0], span[1] - span[0])[:] = 0xEE
    return call


@pytest.fixture
def case():
    x = np.random.default_rng(5).integers(0, 256, N, dtype=np.uint8)
    return FakeCtx(), x, reference(x)


@pytest.mark.parametrize("off_in,off_out", [(0, 0), (4, 1), (12, 3), (3, 255)])
def test_a_correct_writer_passes_at_every_offset(case, off_in, off_out):
    ctx, x, ref = case
    seen = {}

    def call(d_in, d_out):
        seen["p"] = (d_in, d_out)
        writer(ctx)(d_in, d_out)

    got = guarded.run(ctx, call, x, ref, off_in, off_out)
    guarded.check(got, ref)
    assert seen["p"][0] % 16 == off_in % 16 and seen["p"][1] % 16 == off_out % 16
    assert ctx.live is None and ctx.syncs >= 2
    # >= 256 bytes of noise on both sides of the input, >= 256 bytes of slack after the last guard byte read back
    total = max(hi for _, hi in ctx.touched)
    d_in, d_out = (p - ctx.BASE for p in seen["p"])
    first = _up256(ctx.BASE) - ctx.BASE
    assert d_in - first >= 256 and d_out - guarded.GUARD - off_out - (d_in + N) >= 256
    read_back = [t for t in ctx.touched if t[0] == d_out - guarded.GUARD - off_out][-1]
    assert read_back[1] == d_out + N + guarded.GUARD and total - read_back[1] >= 256


def _up256(p):
    return (p + 255) // 256 * 256


def test_the_base_is_rounded_up_to_256(case):
    ctx, x, ref = case
    ptrs = []
    guarded.run(ctx, lambda a, b: (ptrs.append((a, b)), writer(ctx)(a, b)), x, ref, 0, 0)
    assert ptrs[0][0] % 256 == 0 and ptrs[0][1] % 256 == 0 and ctx.BASE % 256 != 0


def test_guards_depend_on_the_position():
    g = guarded.pattern(512, 4096)
    assert len(np.unique(g)) > 200
    quads = g.reshape(-1, 4)
    assert not (quads == quads[:, :1]).all(axis=1).any()           # no constant quad: a splat store shows
    assert not np.array_equal(g[:-1], g[1:]) and not np.array_equal(g[4:], g[:-4])   # nor a shifted copy of itself


def test_one_byte_overrun(case):
    ctx, x, ref = case
    with pytest.raises(guarded.GuardError) as e:
        guarded.run(ctx, writer(ctx, span=(N, N + 1)), x, ref, 0, 3)
    assert e.value.distance == 1 and e.value.count == 1 and "+1" in str(e.value)


def test_whole_quad_store_on_a_partial_last_quad(case):
    ctx, x, ref = case   # N % 4 == 1: a dword store at the last quad runs 3 bytes over
    with pytest.raises(guarded.GuardError) as e:
        guarded.run(ctx, writer(ctx, span=(N - 1, N + 3)), x, ref, 0, 0)
    assert e.value.distance == 1 and e.value.count == 3


def test_one_byte_underrun(case):
    ctx, x, ref = case
    for off_out in (0, 2):   # with off_out the bytes between the guard and the payload are guard too
        with pytest.raises(guarded.GuardError) as e:
            guarded.run(ctx, writer(ctx, span=(-1, 0)), x, ref, 0, off_out)
        assert e.value.distance == -1 and e.value.count == 1


def test_sixteen_byte_overrun_at_the_far_end_of_the_trailing_guard(case):
    ctx, x, ref = case
    with pytest.raises(guarded.GuardError) as e:
        guarded.run(ctx, writer(ctx, span=(N + guarded.GUARD - 16, N + guarded.GUARD)), x, ref, 4, 1)
    assert e.value.distance == guarded.GUARD - 15 and e.value.count == 16
    with pytest.raises(guarded.GuardError) as e:   # and the far end of the leading one
        guarded.run(ctx, writer(ctx, span=(-1 - guarded.GUARD, -1 - guarded.GUARD + 16)), x, ref, 4, 1)
    assert e.value.distance == -guarded.GUARD - 1


def test_constant_stores_into_the_guard_show(case):
    ctx, x, ref = case

    def splat(value):
        def call(d_in, d_out):
            writer(ctx)(d_in, d_out)
            ctx._at(d_out + N, 8)[:] = value
        return call
    for value in (0, 255):
        with pytest.raises(guarded.GuardError):
            guarded.run(ctx, splat(value), x, ref)


def test_unwritten_span_that_holds_the_previous_calls_reference(case):
    """The gap itself: the second of two calls skips 4 bytes.  Straight into a reused, uncleared buffer the result is
    the reference, byte for byte, because the first call's output is still there; in the arena it is not."""
    ctx, x, ref = case
    bad = writer(ctx, skip=(100, 104))
    raw = ctx.alloc(4096)
    ctx.h2d(raw, np.append(x, x[-1:]))
    out = np.empty(N, np.uint8)
    for call in (writer(ctx), bad):        # same input, same pooled output: what the host-buffer tests do
        call(raw, raw + 1024)
        ctx.d2h(out, raw + 1024)
    ctx.free(raw)
    assert np.array_equal(out, ref)        # the skipped store goes unseen
    guarded.check(guarded.run(ctx, writer(ctx), x, ref), ref)
    got = guarded.run(ctx, bad, x, ref)    # the same address again (FakeCtx.alloc), now prefilled
    assert np.array_equal(got[100:104], ref[100:104] ^ 0x80)
    for tol in (0, 1):                     # 128 away: outside the FAST Gaussian's +-1 LSB as well
        with pytest.raises(guarded.PayloadError) as e:
            guarded.check(got, ref, tol=tol)
        assert e.value.index == 100 and e.value.count == 4 and e.value.unwritten == 4


def test_reader_that_uses_a_byte_just_outside_the_input(case):
    ctx, x, ref = case
    for off_in in (0, 1):
        got = guarded.run(ctx, writer(ctx, clamp=False), x, ref, off_in, 0)   # no guard byte changes ...
        with pytest.raises(guarded.PayloadError) as e:                         # ... the value does
            guarded.check(got, ref)
        assert e.value.index == N - 1 and e.value.unwritten == 0


def test_check_takes_a_tolerance(case):
    _, _, ref = case
    near = np.clip(ref.astype(np.int16) + 1, 0, 255).astype(np.uint8)
    guarded.check(near, ref, tol=1)
    with pytest.raises(guarded.PayloadError):
        guarded.check(near, ref, tol=0)
