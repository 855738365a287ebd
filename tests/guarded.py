"""A guarded arena for device-resident calls: sees a pixel that was never written and a write outside the output.

The host-buffer calls run every kernel into the context's pooled, never-cleared output buffer, and most tests run two
kernels on one image and compare them: a store the second kernel skips leaves the first kernel's byte there, which is the
byte the comparison expects.  And nothing reads a byte before or after an output.  run() closes both gaps for any
callable that takes (d_in, d_out), with ctx.alloc / free / h2d / d2h / sync only (a plain module, not a conftest):

    one allocation, its base rounded up to 256:

    | noise 256 | off_in | input | noise 256 | pad | GUARD 256 | off_out | payload | GUARD 256 | slack >= 256 |
                          ^ d_in                                            ^ d_out

  * 256 is a condition, not a tuned number: a multiple of 16, so off_in / off_out alone are the pointers' alignment,
    and two 128-byte lines, so a store span rounded outward to a whole line still lands in a guard.
  * The input sits in seeded noise: a kernel that reads outside its frames and uses the value disagrees with the
    reference.  Nothing is placed at the end of the allocation: no test depends on an access outside it.
  * The guards (off_out bytes included) hold a position-dependent pattern, so zeros, 255s and copied pixels all show.
  * The payload is prefilled with expected ^ 0x80: every byte is exactly 128 away from what must be written, so an
    unwritten byte fails any comparison deterministically, the FAST Gaussian's +-1 LSB one included.

After the call: sync, one d2h of guard + payload + guard.  run() returns the payload and raises GuardError with the signed
distance of the first changed guard byte: -1 is the byte just before the payload, +1 the byte just after it.
check() compares a payload with its reference and says whether the first bad byte still holds the prefill.
"""
import numpy as np

GUARD = 256


class GuardError(AssertionError):
    """A byte outside the payload changed.  distance < 0: bytes before the payload start (-1 = the one just before it);
    distance > 0: bytes after the payload end (+1 = the one just after it)."""

    def __init__(self, distance, count, was, now, tag):
        self.distance, self.count = distance, count
        side = "before the payload start" if distance < 0 else "after the payload end"
        super().__init__("%s: %d guard byte(s) changed, the first at distance %+d (%s): 0x%02x -> 0x%02x"
                         % (tag, count, distance, side, was, now))


class PayloadError(AssertionError):
    """A payload byte is further than `tol` from the reference; unwritten = it still holds the prefill."""

    def __init__(self, index, count, unwritten, got, want, tag):
        self.index, self.count, self.unwritten = index, count, unwritten
        super().__init__("%s: %d payload byte(s) wrong, the first at byte %d: got %d, want %d%s"
                         % (tag, count, index, got, want, " (never written: %d byte(s) still hold the prefill)" % unwritten
                            if unwritten else ""))


def pattern(start, n):
    """n guard bytes for arena offsets start .. start + n - 1: a function of the position, never constant over a quad."""
    i = np.arange(start, start + n, dtype=np.uint32)
    v = i * np.uint32(0x9E3779B1)
    return ((v >> np.uint32(24)) ^ (i * np.uint32(37) + np.uint32(0x5B))).astype(np.uint8)


def _up(x, m):
    return (x + m - 1) // m * m


def prefill_of(expected):
    return np.ascontiguousarray(expected, np.uint8) ^ np.uint8(0x80)


def run(ctx, call, inp, expected, off_in=0, off_out=0, seed=1, tag=""):
    """call(d_in, d_out) with `inp` (uint8, any shape) at d_in = 16n + off_in and an output of expected.shape at
    d_out = 16m + off_out, prefilled with expected ^ 0x80 between two guards.  Returns the payload; GuardError if a guard
    byte changed."""
    inp = np.ascontiguousarray(inp, np.uint8).ravel()
    expected = np.ascontiguousarray(expected, np.uint8)
    nin, nout = inp.size, expected.size
    assert 0 <= off_in < GUARD and 0 <= off_out < GUARD
    in_at = GUARD + off_in
    out_region = _up(in_at + nin + GUARD, 256)          # the leading guard starts on a 256-byte boundary
    out_at = out_region + GUARD + off_out
    window = GUARD + off_out + nout + GUARD               # what is read back
    total = _up(out_region + window + GUARD, 256)         # >= 256 bytes of slack after the trailing guard
    host = np.empty(total, np.uint8)
    host[:out_region] = np.random.default_rng(seed).integers(0, 256, out_region, dtype=np.uint8)
    host[in_at:in_at + nin] = inp
    host[out_region:] = pattern(out_region, total - out_region)
    host[out_at:out_at + nout] = prefill_of(expected).ravel()
    raw = ctx.alloc(total + 256)
    try:
        base = _up(raw, 256)
        assert base % 256 == 0 and base + total <= raw + total + 256
        ctx.h2d(base, host)
        ctx.sync()
        try:
            call(base + in_at, base + out_at)
        finally:
            ctx.sync()
        back = np.empty(window, np.uint8)
        ctx.d2h(back, base + out_region)
        ctx.sync()
    finally:
        ctx.free(raw)
    lead = GUARD + off_out
    want = host[out_region:out_region + window]
    changed = back != want
    changed[lead:lead + nout] = False
    if changed.any():
        i = int(np.flatnonzero(changed)[0])
        dist = i - lead if i < lead else i - (lead + nout) + 1
        raise GuardError(dist, int(changed.sum()), int(want[i]), int(back[i]),
                         "%s off_in=%d off_out=%d" % (tag, off_in, off_out))
    return back[lead:lead + nout].reshape(expected.shape).copy()


def check(got, expected, tol=0, tag=""):
    """Every byte of `got` within `tol` of `expected`, or PayloadError naming the first one."""
    expected = np.ascontiguousarray(expected, np.uint8)
    assert got.shape == expected.shape and got.dtype == np.uint8
    bad = np.abs(got.astype(np.int16) - expected.astype(np.int16)) > tol
    if bad.any():
        i = int(np.flatnonzero(bad.ravel())[0])
        unwritten = int((got == prefill_of(expected)).sum())
        raise PayloadError(i, int(bad.sum()), unwritten, int(got.ravel()[i]), int(expected.ravel()[i]), tag)
