#!/usr/bin/env python3
"""tools/ccl_rate.py — device-resident rate of connected-component labelling on gray8 masks (mi355_ccl_gray8_dev), with
and without statistics, 4- and 8-connected, with two yardsticks from the same process and the same buffers:

  * mi355_stream_copy_dev of 2.5 bytes per pixel (reads 2.5, writes 2.5): the 5 B/px a labelling call has to move at
    the very least, 1 B/px of mask read and 4 B/px of labels written.  The call itself moves several times that: the
    label array is written, merged in place, flattened and renumbered;
  * MI355_FILTER_OTSU_GRAY8 on the same mask (reads 2 B/px, writes 1 B/px): the step before it in the chain.

Contents:
  otsu      the Otsu mask of the synthetic gradient-plus-noise frames (synth mode 1 through GRAY1 and OTSU_GRAY8)
  noise0.3  site noise at density 0.3: tens of thousands of small components per frame
  noise0.59 site noise at density 0.59: the 4-connected percolation threshold, tortuous components across every tile
  spiral    a one-pixel spiral, one component: the longest chain a frame can hold
The noise and spiral masks are made on the host (tests/ccl_cases.py), four distinct noise frames repeated over the batch.

Every row: HIP events around `iters` calls after `warmup`, the median of `reps` such groups; GB/s counts 5 B/px.  Each
labelling row checks the first frame's labels, count and statistics against tests/ccl_ref.py (--no-check skips it).

  python3 tools/ccl_rate.py [--shapes 3840x2160x256] [--stats-rows 1000]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 400 python3 tools/ccl_rate.py > profiles/ccl_rate.txt && ...
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--shapes", default="3840x2160x256")
    ap.add_argument("--stats-rows", type=int, default=1000)
    ap.add_argument("--contents", default="otsu,noise0.3,noise0.59,spiral")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import ccl_cases as cc
    from ccl_ref import ccl_ref
    pkg = entry.load_package()
    rows = a.stats_rows
    ctx = pkg.Context(0)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        fpx, npx = w * h, w * h * n
        ncopy = (5 * npx // 2 + 15) // 16 * 16
        d_rgba = ctx.alloc(fpx * 4 * min(n, 16))
        d_gray, d_mask, d_tmp = ctx.alloc(npx), ctx.alloc(npx), ctx.alloc(ncopy)
        d_labels, d_count = ctx.alloc(max(4 * npx, ncopy)), ctx.alloc(4 * n)
        d_stats, d_sums = ctx.alloc(20 * n * rows), ctx.alloc(16 * n * rows)
        t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_tmp, d_labels, ncopy), a.warmup, a.iters, a.reps)
        for content in a.contents.split(","):
            if content == "otsu":
                for f0 in range(0, n, 16):
                    nf = min(16, n - f0)
                    ctx.synth_dev(d_rgba, w, h, nf, f0, 0x5EED, 1)
                    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_gray + f0 * fpx, w, h, nf)
                ctx.filter_dev(pkg.FILTER_OTSU_GRAY8, d_gray, d_mask, w, h, n)
            else:
                if content == "spiral":
                    frames = [cc.spiral(h, w)]
                else:
                    rng = np.random.default_rng(17)
                    frames = [(rng.random((h, w)) < float(content[5:])).astype(np.uint8) * 255 for _ in range(4)]
                for f in range(n):
                    ctx.h2d(d_mask + f * fpx, frames[f % len(frames)])
            ctx.sync()
            first = np.empty((h, w), np.uint8)
            ctx.d2h(first, d_mask)
            t_otsu = _time(ctx, lambda: ctx.filter_dev(pkg.FILTER_OTSU_GRAY8, d_mask, d_tmp, w, h, n), a.warmup, a.iters,
                           a.reps)
            base = {"content": content, "w": w, "h": h, "n": n, "foreground": round(float((first != 0).mean()), 3),
                    "copy_ms": round(t_copy, 3), "otsu_ms": round(t_otsu, 3)}
            for conn in (4, 8):
                want = None if a.no_check else ccl_ref(first, conn, rows)
                for r in (0, rows):
                    t = _time(ctx, lambda: ctx.ccl_gray8_dev(d_mask, d_labels, d_count, d_stats, d_sums, w, h, n, conn, r),
                              a.warmup, a.iters, a.reps)
                    row = dict(base, op="ccl", connectivity=conn, stats_rows=r, ms=round(t, 3),
                               gb_s=round(5 * npx / t / 1e6, 1), ratio_vs_copy=round(t / t_copy, 2),
                               ratio_vs_otsu=round(t / t_otsu, 2))
                    labels, count = np.empty((h, w), np.int32), np.empty(1, np.int32)
                    ctx.d2h(labels, d_labels)
                    ctx.d2h(count, d_count)
                    row["labels_per_frame"] = int(count[0])
                    if want is not None:
                        ok = np.array_equal(labels, want[0][0]) and count[0] == want[1][0]
                        if r:
                            stats, sums = np.empty((r, 5), np.int32), np.empty((r, 2), np.uint64)
                            ctx.d2h(stats, d_stats)
                            ctx.d2h(sums, d_sums)
                            ok = ok and np.array_equal(stats, want[2][0]) and np.array_equal(sums, want[3][0])
                        row["equal_ref"] = bool(ok)
                    print(json.dumps(row), flush=True)
        for p in (d_rgba, d_gray, d_mask, d_tmp, d_labels, d_count, d_stats, d_sums):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
