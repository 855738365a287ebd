#!/usr/bin/env python3
"""Regenerates tests/golden/straddle_windows.json: k x k blocks of bytes on which the CPU path's truncated Gaussian sum
differs from the sum taken in another order, exactly, or with a fused multiply-add (tests/straddle_cases.py says what
the alternates a .. e are and what the frames built from these windows are for).  Seeded and deterministic: a second
run writes the same bytes.  Needs the oracle's tables only (oracle.gauss_weights).

Mining.  A random window's sum is near an integer with probability ~1e-5, so the centre byte is swept instead: with S0
the exact sum of the other taps and W the centre's weight, the centre values c for which S0 + c W lies within EPS of an
integer are the candidates (256 tries for the price of one), and the float32 chains are evaluated on those alone.
About one candidate in ten is critical for some alternate.  Edge windows are mined the same way from the in-image
part of a window whose centre sits cy < R rows / cx < R columns from an edge, expanded by the CPU path's clamp-to-edge
rule; there the centre pixel may be replicated, and W is the sum of the weights of its copies.

  interior[k]  at least quota(k) windows per alternate (32; 16 at k = 33) and quota(k) / 2 that are critical for all five
  edges[k]     k in {3, 5, 7}: at least 8 windows per kind (four edges, two opposite corners)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository root

import straddle_cases as sc  # noqa: E402


def eps_of(k):
    """Half-width of the candidate band around an integer: a few times the chains' rounding error, which grows with the
    number of taps (measured spread of S_cpu - exact: ~1e-5 at k = 3, ~2e-4 at k = 33).  Only the yield depends on it."""
    return 2.0e-5 * k


def candidates(rng, k, w2, rows, cols, batch):
    """Windows (expanded through rows / cols) whose exact sum lies within eps of an integer in 1 .. 254."""
    r = k // 2
    base = rng.integers(0, 256, (batch, k, k), dtype=np.uint8)[:, rows][:, :, cols]
    copies = (rows[:, None] == r) & (cols[None, :] == r)      # where the centre pixel is read
    wd = w2.astype(np.float64)
    s0 = (base.astype(np.float64) * np.where(copies, 0.0, wd)).sum(axis=(1, 2))
    s = s0[:, None] + np.arange(256)[None, :] * wd[copies].sum()
    near = (np.abs(s - np.rint(s)) < eps_of(k)) & (np.rint(s) >= 1) & (np.rint(s) <= 254)
    wi, ci = np.nonzero(near)
    out = base[wi]
    out[:, copies] = ci[:, None].astype(np.uint8)
    return out


def mine(rng, k, w2, want, want_all, rows=None, cols=None, batch=None):
    """Greedy: walk the candidates in order and keep a window while it adds to an alternate that is short of `want`, or is
    critical for all five while fewer than `want_all` such windows are kept."""
    idx = np.arange(k)
    rows = idx if rows is None else rows
    cols = idx if cols is None else cols
    batch = batch or max(2000, min(20000, 2000000 // (k * k)))
    have = dict.fromkeys(sc.ALTS, 0)
    n_all = 0
    kept, letters = [], []
    for _ in range(200):          # a few rounds are enough; an alternate that never differs must not loop for ever
        if min(have.values()) >= want and n_all >= want_all:
            break
        cand = candidates(rng, k, w2, rows, cols, batch)
        for win, lt in zip(cand, sc.critical_letters(cand, w2)):
            full = len(lt) == len(sc.ALTS)
            if lt and (any(have[a] < want for a in lt) or (full and n_all < want_all)):
                kept.append(win)
                letters.append(lt)
                n_all += full
                for a in lt:
                    have[a] += 1
    if min(have.values()) < want or n_all < want_all:
        raise RuntimeError("k = %d: quotas not met after 200 rounds: %r, %d for all five" % (k, have, n_all))
    return kept, letters


def _hex(win):
    return np.ascontiguousarray(win, np.uint8).tobytes().hex()


def build(oracle, sizes=sc.SIZES):
    """The fixture as a dict; every size draws from a generator of its own, so a subset of `sizes` gives the same entries."""
    out = {"about": "critical Gaussian windows, row-major bytes as hex; see tests/golden/make_straddle.py",
           "interior": {}, "edges": {}}
    for k, sigma in sizes:
        w2 = oracle.gauss_weights(k, sigma)
        assert sc.span_ok(w2), (k, sigma)      # alternates d and e are evaluated exactly in double only under this
        rng = np.random.default_rng(7000 + k)
        wins, letters = mine(rng, k, w2, sc.quota(k), sc.quota(k) // 2)
        # the greedy walk keeps windows of the rarest alternate last: shuffle, so that a frame which cycles through a
        # part of the list meets every alternate
        order = rng.permutation(len(wins))
        wins, letters = [wins[i] for i in order], [letters[i] for i in order]
        out["interior"][str(k)] = {"sigma": sigma, "windows": [_hex(w) for w in wins], "alternates": letters}
        if k not in sc.EDGE_KS:
            continue
        r = k // 2
        items = []
        for kind in sc.EDGE_KINDS:
            per_c = -(-sc.EDGE_QUOTA // r)     # spread the quota over the distances 0 .. R - 1
            for c in range(r):
                cy = c if kind in ("top", "bottom", "top-left", "bottom-right") else 0
                cx = (r - 1 - c if "-" in kind else c) if kind not in ("top", "bottom") else 0
                rows, cols = sc.edge_maps(kind, cy, cx, k)
                ws, lts = mine(rng, k, w2, per_c, 0, rows, cols, batch=8000)
                items += [{"kind": kind, "cy": cy, "cx": cx, "window": _hex(w), "alternates": lt}
                          for w, lt in zip(ws, lts)]
        out["edges"][str(k)] = items
    return out


def dumps(data):
    return json.dumps(data, indent=0, sort_keys=True) + "\n"


def main():
    import __graft_entry__ as entry
    text = dumps(build(entry.load_oracle()))
    with open(sc.FIXTURE, "w") as f:
        f.write(text)
    print("wrote %s: %d bytes" % (os.path.relpath(sc.FIXTURE, HERE), len(text)))


if __name__ == "__main__":
    main()
