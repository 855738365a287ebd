#!/usr/bin/env python3
"""tools/canny_rate.py — device-resident rate of Canny and hysteresis thresholding on gray8 frames
(mi355_canny_gray8_dev, mi355_hysteresis_gray8_dev), with three yardsticks from the same process and the same buffers:

  * mi355_stream_copy_dev of 1 byte per pixel (reads 1, writes 1): the 2 B/px the non-maximum-suppression launch has to
    move at the very least;
  * MI355_FILTER_SOBEL_GRAY8 on the same frames: the other 3x3 gradient kernel of the library, also 2 B/px;
  * mi355_ccl_gray8_dev without statistics on the candidate mask: the labelling call whose union launches the hysteresis
    shares.

Contents, four distinct frames repeated over the batch:
  blurred   uniform noise through MI355_FILTER_GAUSS_GRAY8 (k = 5, sigma = 1.4): dense short edges of every direction
  photo     a reference photograph (tests/golden/ref_images, its luma plane) tiled over the frame, after the same blur
  flat      one value: no candidate anywhere

Rows per content:
  canny       the whole call, thresholds (50, 150)
  hysteresis  mi355_hysteresis_gray8_dev(low 0, high 1, 8-connected) on the class map (0 none, 1 candidate, 2 strong) of
              the same frames: what the Canny call runs behind its first launch.  The class maps come from the CPU
              reference (tests/canny_ref.py), four frames of them
  nms         canny - hysteresis: the non-maximum-suppression launch alone.  The library has no entry that stops after
              it, and the launches of a call run in order on one stream, so the difference of the two medians is reported
  sobel, ccl, copy   the yardsticks

Every row: HIP events around `iters` calls after `warmup`, the median of `reps` such groups.  The canny row checks the
first frame against tests/canny_ref.py (--no-check skips it).

  python3 tools/canny_rate.py [--shapes 3840x2160x256]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 500 python3 tools/canny_rate.py > profiles/canny_rate.txt && ...
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T1, T2 = 50.0, 150.0
DISTINCT = 4


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


def _sources(content, h, w):
    """The distinct (h, w) frames of a content before the blur"""
    if content == "blurred":
        rng = np.random.default_rng(17)
        return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(DISTINCT)]
    if content == "photo":
        from PIL import Image
        y = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "ref_images", "Artemis_medium640_y.png")).convert("L"))
        reps = ((h + y.shape[0] - 1) // y.shape[0] + 1, (w + y.shape[1] - 1) // y.shape[1] + 1)
        big = np.tile(y, reps)
        return [np.ascontiguousarray(big[s:s + h, 3 * s:3 * s + w]) for s in range(0, 4 * DISTINCT, 4)]
    return [np.full((h, w), 77, np.uint8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x256")
    ap.add_argument("--contents", default="blurred,photo,flat")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import canny_ref as cr
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        fpx, npx = w * h, w * h * n
        d_src, d_in, d_cls, d_out = (ctx.alloc(npx) for _ in range(4))
        d_labels, d_count = ctx.alloc(4 * npx), ctx.alloc(4 * n)
        t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_out, d_in, npx), a.warmup, a.iters, a.reps)
        for content in a.contents.split(","):
            srcs = _sources(content, h, w)
            for f in range(n):
                ctx.h2d(d_src + f * fpx, srcs[f % len(srcs)])
            if content == "flat":
                ctx.stream_copy_dev(d_in, d_src, npx)
            else:
                ctx.filter_dev(pkg.FILTER_GAUSS_GRAY8, d_src, d_in, w, h, n, 5, 1.4)
            ctx.sync()
            low, high = cr.thresholds(T1, T2)
            frames, classes = [], []
            for f in range(len(srcs)):
                fr = np.empty((h, w), np.uint8)
                ctx.d2h(fr, d_in + f * fpx)
                frames.append(fr)
                classes.append(cr.classes(fr, low, high))
            for f in range(n):
                ctx.h2d(d_cls + f * fpx, classes[f % len(classes)])
            ctx.sync()
            t_canny = _time(ctx, lambda: ctx.canny_gray8_dev(d_in, d_out, w, h, n, T1, T2, 0), a.warmup, a.iters, a.reps)
            first = np.empty((h, w), np.uint8)
            ctx.d2h(first, d_out)
            t_hyst = _time(ctx, lambda: ctx.hysteresis_gray8_dev(d_cls, d_out, w, h, n, 0, 1, 8), a.warmup, a.iters, a.reps)
            first_h = np.empty((h, w), np.uint8)
            ctx.d2h(first_h, d_out)
            t_sobel = _time(ctx, lambda: ctx.filter_dev(pkg.FILTER_SOBEL_GRAY8, d_in, d_out, w, h, n), a.warmup, a.iters,
                            a.reps)
            t_ccl = _time(ctx, lambda: ctx.ccl_gray8_dev(d_cls, d_labels, d_count, None, None, w, h, n, 8, 0), a.warmup,
                          a.iters, a.reps)
            count = np.empty(1, np.int32)
            ctx.d2h(count, d_count)
            t_nms = t_canny - t_hyst
            row = {"content": content, "w": w, "h": h, "n": n,
                   "candidates": round(float((classes[0] > 0).mean()), 4), "edges": round(float((first != 0).mean()), 4),
                   "candidate_components": int(count[0]) - 1,
                   "canny_ms": round(t_canny, 3), "hysteresis_ms": round(t_hyst, 3), "nms_ms": round(t_nms, 3),
                   "sobel_ms": round(t_sobel, 3), "ccl_ms": round(t_ccl, 3), "copy_ms": round(t_copy, 3),
                   "canny_gpx_s": round(npx / t_canny / 1e6, 2), "nms_gb_s": round(2 * npx / t_nms / 1e6, 1),
                   "canny_vs_copy": round(t_canny / t_copy, 2), "nms_vs_copy": round(t_nms / t_copy, 2),
                   "nms_vs_sobel": round(t_nms / t_sobel, 2), "canny_vs_ccl": round(t_canny / t_ccl, 2),
                   "hysteresis_vs_ccl": round(t_hyst / t_ccl, 2)}
            if not a.no_check:
                want = cr.canny_ref(frames[0], T1, T2, 0, cr.kept_by_labels)
                row["equal_ref"] = bool(np.array_equal(first, want) and np.array_equal(first_h, want))
            print(json.dumps(row), flush=True)
        for p in (d_src, d_in, d_cls, d_out, d_labels, d_count):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
