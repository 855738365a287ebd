#!/usr/bin/env python3
"""tools/gray8_rate.py — device-resident rate of the single-channel filters against the RGBA call a gray-frame user
has to make without them, same process, same buffers.

For every row: n frames of w x h gray bytes (hash noise) through MI355_FILTER_{GAUSS,SOBEL,PIPELINE}_GRAY8, and the
same planes expanded once to (y, y, y, 255) through MI355_FILTER_{GAUSS,SOBEL,PIPELINE} (the expansion is not timed).
HIP events around `iters` launches after `warmup`; rates from the median of `reps` such groups.  GB/s counts the
algorithmic bytes of the gray filter (2 B/px); the fraction is of the 8 TB/s spec peak.

  python3 tools/gray8_rate.py [--w 3840 --h 2160 --n 256 --k 5 --sigma 1.5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def _time(ctx, fn, warmup, iters, reps):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_begin()
        for _ in range(iters):
            fn()
        ms.append(ctx.timer_end() / iters)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", default="fast,exact")
    a = ap.parse_args()
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    w, h, n = a.w, a.h, a.n
    npx = w * h * n
    d_y = ctx.alloc(npx)
    d_rgba = ctx.alloc(npx * 4)
    d_out = ctx.alloc(npx * 4)
    # gray planes: the GRAY1 filter of synthetic frames (mode 1: smooth gradient + noise); the RGBA alternative reads
    # their (y, y, y, 255) expansion, made once through the host and not timed
    ctx.synth_dev(d_rgba, w, h, n, 0, 0x5EED, 1)
    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y, w, h, n)
    ctx.sync()
    frame = np.empty((h, w), np.uint8)
    for f in range(n):
        ctx.d2h(frame, d_y + f * w * h)
        ctx.h2d(d_rgba + f * w * h * 4, np.dstack([frame, frame, frame, np.full_like(frame, 255)]))
    ctx.sync()
    rows = []
    pairs = [("gauss", pkg.FILTER_GAUSS_GRAY8, pkg.FILTER_GAUSS), ("sobel", pkg.FILTER_SOBEL_GRAY8, pkg.FILTER_SOBEL),
             ("pipeline", pkg.FILTER_PIPELINE_GRAY8, pkg.FILTER_PIPELINE)]
    for mode_name in a.modes.split(","):
        ctx.set_gauss_mode(pkg.GAUSS_EXACT if mode_name == "exact" else pkg.GAUSS_FAST)
        for name, g8, rgba in pairs:
            if name == "sobel" and mode_name != a.modes.split(",")[0]:
                continue  # no Gaussian mode in the Sobel
            t_g8 = _time(ctx, lambda: ctx.filter_dev(g8, d_y, d_out, w, h, n, a.k, a.sigma), a.warmup, a.iters, a.reps)
            t_rgba = _time(ctx, lambda: ctx.filter_dev(rgba, d_rgba, d_out, w, h, n, a.k, a.sigma), a.warmup, a.iters,
                           a.reps)
            mpx = npx / (t_g8 * 1e-3) / 1e6
            gbs = 2.0 * npx / (t_g8 * 1e-3) / 1e9
            row = {"filter": name + "_gray8", "mode": mode_name if name != "sobel" else "-", "w": w, "h": h, "n": n,
                   "k": a.k if name != "sobel" else None, "ms": round(t_g8, 3), "mpx_s": round(mpx, 1),
                   "gb_s_2Bpx": round(gbs, 1), "frac_8TBs": round(gbs / 8000.0, 3),
                   "rgba_alt_ms": round(t_rgba, 3), "rgba_alt_mpx_s": round(npx / (t_rgba * 1e-3) / 1e6, 1),
                   "ratio_vs_rgba": round(t_rgba / t_g8, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    for p in (d_y, d_rgba, d_out):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
