#!/usr/bin/env python3
"""tools/hough_rate.py — device-resident rate of the Hough line transform on gray8 edge maps
(mi355_hough_lines_gray8_dev, mi355_hough_accum_gray8_dev), rho = 1, theta = pi / 180, threshold 200, 256 lines, with
three yardsticks from the same process:

  * mi355_stream_copy_dev of the mask bytes plus the accumulator bytes: what a call must at least read and write;
  * mi355_canny_gray8_dev on the frames the masks came from: the step in front of it in the chain;
  * for scale only (--torch): the same votes as torch ops on one frame (nonzero, two products, a sum, round, bincount
    per angle), timed with a host clock around a synchronise.

Contents, four distinct frames repeated over the batch:
  photo     the library's Canny (50, 150) of a reference photograph (tests/golden/ref_images, its luma plane) tiled over
            the frame and blurred (MI355_FILTER_GAUSS_GRAY8, k = 5, sigma = 1.4)
  blurred   the same of uniform noise
  dense50   a mask with every second pixel set at random

Rows per content:
  lines     the whole call with the pooled accumulator
  accum     the accumulator call alone: the point list and the votes.  accum / lines is the share of the call that votes
  votes/s   points x angles over the accum time

Every row: HIP events around `iters` calls after `warmup`, the median of `reps` such groups.  The first frame's result is
checked against tests/hough_ref.py fed the library's table (--no-check skips it).

--ab: the same-process A/B of the voting launch's choices through the tune build (tools/lib/libmi355_imgfilter_tune.so:
MI355_TUNE_HOUGH_AGG = 0 never / 1 always merge equal neighbours, unset: by the angle's step; MI355_TUNE_HOUGH_ANGLES =
angle rows per workgroup; MI355_TUNE_HOUGH_UNROLL = 1: one point per thread and trip instead of four), the candidates
alternating inside every repetition, on the accum call.

  python3 tools/hough_rate.py [--shapes 3840x2160x64] [--ab] [--torch]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 500 python3 tools/hough_rate.py > profiles/hough_rate.txt && ...
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RHO, THETA, THRESHOLD, MAX_LINES = 1.0, math.pi / 180, 200, 256
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
    """The distinct (h, w) frames of a content before the blur and Canny (dense50: the masks themselves)"""
    rng = np.random.default_rng(17)
    if content == "blurred":
        return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(DISTINCT)]
    if content == "photo":
        from PIL import Image
        y = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "ref_images", "Artemis_medium640_y.png")).convert("L"))
        reps = ((h + y.shape[0] - 1) // y.shape[0] + 1, (w + y.shape[1] - 1) // y.shape[1] + 1)
        big = np.tile(y, reps)
        return [np.ascontiguousarray(big[s:s + h, 3 * s:3 * s + w]) for s in range(0, 4 * DISTINCT, 4)]
    return [((rng.random((h, w)) < 0.5) * 255).astype(np.uint8) for _ in range(DISTINCT)]


def _fill(ctx, pkg, content, bufs, w, h, n):
    """The masks of `content` into bufs["mask"] (and the frames they came from into bufs["in"])"""
    fpx = w * h
    srcs = _sources(content, h, w)
    dst = bufs["mask"] if content == "dense50" else bufs["src"]
    for f in range(n):
        ctx.h2d(dst + f * fpx, srcs[f % len(srcs)])
    if content != "dense50":
        ctx.filter_dev(pkg.FILTER_GAUSS_GRAY8, bufs["src"], bufs["in"], w, h, n, 5, 1.4)
        ctx.canny_gray8_dev(bufs["in"], bufs["mask"], w, h, n, T1, T2, 0)
    ctx.sync()
    first = np.empty((h, w), np.uint8)
    ctx.d2h(first, bufs["mask"])
    return first


def _torch_votes(first, tc, ts, numrho):
    """ms of the same votes of one frame as torch ops; the library must already be loaded after torch (see main)"""
    import torch
    dev = torch.device("cuda", 0)
    m = torch.from_numpy(first).to(dev)
    c, s = torch.from_numpy(tc).to(dev), torch.from_numpy(ts).to(dev)
    half = (numrho - 1) // 2

    def run():
        ys, xs = torch.nonzero(m, as_tuple=True)
        fx, fy = xs.float(), ys.float()
        acc = torch.zeros((len(tc), numrho), dtype=torch.int64, device=dev)
        for k in range(len(tc)):
            r = torch.round(fx * c[k] + fy * s[k]).long() + half
            acc[k] = torch.bincount(r, minlength=numrho)[:numrho]
        return acc

    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, acc.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x64")
    ap.add_argument("--contents", default="photo,blurred,dense50")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--torch", action="store_true", help="the torch formulation of one frame's votes, for scale")
    ap.add_argument("--ab", action="store_true", help="A/B of the voting launch's choices through the tune build")
    a = ap.parse_args()
    if a.torch:
        import torch  # first: torch brings its own HIP runtime and must initialise it before the library loads
        torch.cuda.init()
    import __graft_entry__ as entry
    import hough_ref as hr
    pkg = entry.load_package()
    lib = None
    if a.ab:
        tune = os.path.join(ROOT, "tools", "lib", "libmi355_imgfilter_tune.so")
        if not os.path.exists(tune):
            sys.exit("%s is missing: run __graft_entry__.build()" % tune)
        lib = pkg.load_library(tune)
    ctx = pkg.Context(0, lib=lib)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        fpx, npx = w * h, w * h * n
        na, nr = pkg.hough_shape(w, h, RHO, THETA)
        tc, ts = pkg.hough_trig_table(w, h, RHO, THETA)
        acc_bytes = pkg.hough_accum_bytes(w, h, n, RHO, THETA)
        plan = pkg.hough_plan(w, h, RHO, THETA)
        bufs = {"src": ctx.alloc(npx), "in": ctx.alloc(npx), "mask": ctx.alloc(npx), "accum": ctx.alloc(acc_bytes),
                "copy_a": ctx.alloc(npx + acc_bytes), "copy_b": ctx.alloc(npx + acc_bytes),
                "lines": ctx.alloc(n * MAX_LINES * 8), "votes": ctx.alloc(n * MAX_LINES * 4), "count": ctx.alloc(4 * n)}
        t_copy = _time(ctx, lambda: ctx.stream_copy_dev(bufs["copy_b"], bufs["copy_a"], npx + acc_bytes), a.warmup,
                       a.iters, a.reps)

        def lines_call():
            ctx.hough_lines_gray8_dev(bufs["mask"], bufs["lines"], bufs["votes"], bufs["count"], 0, w, h, n, RHO, THETA,
                                      THRESHOLD, MAX_LINES)

        def accum_call():
            ctx.hough_accum_gray8_dev(bufs["mask"], bufs["accum"], w, h, n, RHO, THETA)

        for content in a.contents.split(","):
            first = _fill(ctx, pkg, content, bufs, w, h, n)
            points = int((first != 0).sum())
            row = {"content": content, "w": w, "h": h, "n": n, "numangle": na, "numrho": nr,
                   "angles_per_block": plan[0], "rho_splits": plan[1], "density": round(points / fpx, 4)}
            if a.ab:
                cands = [("agg_by_step", {}), ("agg_never", {"MI355_TUNE_HOUGH_AGG": "0"}),
                         ("agg_always", {"MI355_TUNE_HOUGH_AGG": "1"})]
                cands += [("angles_%d" % k, {"MI355_TUNE_HOUGH_ANGLES": str(k)}) for k in range(1, plan[0] + 1)]
                cands += [("one_point_per_trip", {"MI355_TUNE_HOUGH_UNROLL": "1"})]
                ms = {name: [] for name, _ in cands}
                for rep in range(a.reps + 1):               # the first round warms every candidate up and is dropped
                    for name, env in cands:
                        os.environ.update(env)
                        t = _time(ctx, accum_call, 0, a.iters, 1)
                        for k in env:
                            os.environ.pop(k)
                        if rep:
                            ms[name].append(t)
                row.update({"ab_accum_ms": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
                            "ab_spread_ms": {k: round(float(max(v) - min(v)), 3) for k, v in ms.items()}})
                print(json.dumps(row), flush=True)
                continue
            t_lines = _time(ctx, lines_call, a.warmup, a.iters, a.reps)
            got_l, got_v, got_c = np.empty((MAX_LINES, 2), np.float32), np.empty(MAX_LINES, np.int32), np.empty(1, np.int32)
            ctx.d2h(got_l, bufs["lines"])
            ctx.d2h(got_v, bufs["votes"])
            ctx.d2h(got_c, bufs["count"])
            t_accum = _time(ctx, accum_call, a.warmup, a.iters, a.reps)
            got_a = np.empty((na + 2, nr + 2), np.int32)
            ctx.d2h(got_a, bufs["accum"])
            votes = points * na            # of the first frame; the four distinct frames have about the same density
            row.update({"peaks": int(got_c[0]), "lines_ms": round(t_lines, 3), "accum_ms": round(t_accum, 3),
                        "select_ms": round(t_lines - t_accum, 3), "voting_share": round(t_accum / t_lines, 3),
                        "gvotes_s": round(votes * n / t_accum / 1e6, 1), "copy_ms": round(t_copy, 3),
                        "copy_gb_s": round((npx + acc_bytes) * 2 / t_copy / 1e6, 1),
                        "lines_vs_copy": round(t_lines / t_copy, 2)})
            if content != "dense50":
                t_canny = _time(ctx, lambda: ctx.canny_gray8_dev(bufs["in"], bufs["src"], w, h, n, T1, T2, 0), a.warmup,
                                a.iters, a.reps)
                row.update({"canny_ms": round(t_canny, 3), "lines_vs_canny": round(t_lines / t_canny, 2)})
            if a.torch:
                t_torch, acc_t = _torch_votes(first, tc, ts, nr)
                row.update({"torch_one_frame_ms": round(t_torch, 2),
                            "torch_one_frame_vs_accum_per_frame": round(t_torch / (t_accum / n), 1),
                            "torch_equal": bool(np.array_equal(acc_t, got_a[1:-1, 1:-1]))})
            if not a.no_check:
                want = hr.hough_ref(first, tc, ts, nr, THRESHOLD, MAX_LINES, RHO, THETA)
                row["equal_ref"] = bool(np.array_equal(got_a, want[0][0]) and
                                        np.array_equal(got_l.view(np.uint32), want[1][0].view(np.uint32)) and
                                        np.array_equal(got_v, want[2][0]) and int(got_c[0]) == int(want[3][0]))
            print(json.dumps(row), flush=True)
        for p in bufs.values():
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
