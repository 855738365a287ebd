#!/usr/bin/env python3
"""tools/clahe_rate.py — device-resident rate of CLAHE on single-channel frames (mi355_clahe_gray8_dev), with two
yardsticks from the same process and the same buffers:

  * mi355_stream_copy_dev of the frames (reads and writes w h n bytes: 2 B/px).  CLAHE reads the frame twice and writes
    it once (3 B/px), so its floor is 1.5x the copy time;
  * MI355_FILTER_EQUALIZE_GRAY8, the global equalization with the same traffic and the same three-launch shape.

Also timed: mi355_clahe_luts_gray8_dev alone (the tile histograms and the tables: 1 B/px), which splits a call into its
table half and its apply half without a profiler.

Contents: noise (hash noise from mi355_synth_rgba8_dev through GRAY1) and flat 64 x 64 patches (synth mode 2 through
GRAY1).  Every row: HIP events around `iters` calls after `warmup`, the median of `reps` such groups; GB/s counts
3 B/px for CLAHE and equalize and 1 B/px for the tables.  Each CLAHE row checks the first frame's result against
tests/clahe_ref.py.

  python3 tools/clahe_rate.py [--shapes 3840x2160x64,3840x2160x256] [--tiles 8x8] [--clips 2.0,40.0]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 300 python3 tools/clahe_rate.py > profiles/clahe_rate.txt && ...
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
    ap.add_argument("--shapes", default="3840x2160x64,3840x2160x256")
    ap.add_argument("--tiles", default="8x8")
    ap.add_argument("--clips", default="2.0,40.0")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as entry
    from clahe_ref import clahe_ref
    pkg = entry.load_package()
    tx, ty = (int(v) for v in a.tiles.split("x"))
    clips = [float(v) for v in a.clips.split(",")]
    ctx = pkg.Context(0)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        npx = w * h * n
        d_rgba = ctx.alloc(w * h * 4 * min(n, 16))
        d_y, d_out, d_luts = ctx.alloc(npx), ctx.alloc(npx), ctx.alloc(n * tx * ty * 256)
        for content in ("noise", "patches"):
            for f0 in range(0, n, 16):
                nf = min(16, n - f0)
                ctx.synth_dev(d_rgba, w, h, nf, f0, 0x5EED, 0 if content == "noise" else 2)
                ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y + f0 * w * h, w, h, nf)
            ctx.sync()
            frame = np.empty((h, w), np.uint8)
            ctx.d2h(frame, d_y)
            t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_out, d_y, npx), a.warmup, a.iters, a.reps)
            t_eq = _time(ctx, lambda: ctx.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, d_y, d_out, w, h, n), a.warmup, a.iters,
                         a.reps)
            base = {"content": content, "w": w, "h": h, "n": n, "copy_ms": round(t_copy, 3)}
            print(json.dumps(dict(base, op="equalize", ms=round(t_eq, 3), gb_s=round(3 * npx / t_eq / 1e6, 1),
                                  ratio_vs_copy=round(t_eq / t_copy, 3))), flush=True)
            for clip in clips:
                t_luts = _time(ctx, lambda: ctx.clahe_luts_gray8_dev(d_y, d_luts, w, h, n, clip, tx, ty), a.warmup,
                               a.iters, a.reps)
                t = _time(ctx, lambda: ctx.clahe_gray8_dev(d_y, d_out, w, h, n, clip, tx, ty), a.warmup, a.iters, a.reps)
                got = np.empty_like(frame)
                ctx.d2h(got, d_out)
                print(json.dumps(dict(base, op="clahe", tiles="%dx%d" % (tx, ty), clip=clip, ms=round(t, 3),
                                      gb_s=round(3 * npx / t / 1e6, 1), ratio_vs_copy=round(t / t_copy, 3),
                                      equalize_ms=round(t_eq, 3), ratio_vs_equalize=round(t / t_eq, 3),
                                      tables_ms=round(t_luts, 3), tables_gb_s=round(npx / t_luts / 1e6, 1),
                                      apply_ms=round(t - t_luts, 3),
                                      equal_ref=bool(np.array_equal(got, clahe_ref(frame, clip, tx, ty))))), flush=True)
        for p in (d_rgba, d_y, d_out, d_luts):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
