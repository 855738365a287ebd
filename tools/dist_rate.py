#!/usr/bin/env python3
"""tools/dist_rate.py — device-resident rate of the exact Euclidean distance transform on gray8 masks
(mi355_dist_gray8_dev), the distances alone and all three outputs, with two yardsticks from the same process and the same
buffers:

  * mi355_stream_copy_dev of half the bytes the call has to move at the very least (it reads them and writes them):
    1 B/px of mask read and 4 B/px of distances written, or 12 B/px with the squared distances and the nearest sites.
    The call itself also writes and reads its 2 B/px of column offsets;
  * mi355_ccl_gray8_dev without statistics on the same mask (8-connected): the step after it in the chain.

Contents (a pixel whose byte is zero is a site):
  otsu        the Otsu mask of the synthetic gradient-plus-noise frames (synth mode 1 through GRAY1 and OTSU_GRAY8)
  noise0.01   site noise, 1 % of the pixels are sites: every pixel looks a few columns either way
  noise0.5    half the pixels are sites
  noise0.99   nearly all are
  single      one site in the middle of the frame: every column but one has none, the longest candidate ranges
  left        one site column at the left edge: every row's minimiser is column 0
  none        no site at all: every output is the sentinel
The noise masks are made on the host, four distinct frames repeated over the batch.  The ratio of the slowest content to
the fastest, printed per shape and configuration, is the check on "the work of a row is bounded by its width alone".

Every row: HIP events around `iters` calls after `warmup`, the median of `reps` such groups.  Each row checks the first
frame against scipy.ndimage.distance_transform_edt where scipy is installed (squared distances equal; the nearest site is a
site at that distance); --no-check skips it.

  python3 tools/dist_rate.py [--shapes 3840x2160x1,3840x2160x8,3840x2160x64,3840x2160x256]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 500 python3 tools/dist_rate.py > profiles/dist_rate.txt && ...
The share of each launch comes from a kernel trace of a short run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/dist_rate.py --shapes 3840x2160x64 --contents otsu \
      --iters 1 --reps 1 --no-check
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


def _host_frames(content, h, w):
    if content.startswith("noise"):
        rng = np.random.default_rng(17)
        return [(rng.random((h, w)) >= float(content[5:])).astype(np.uint8) * 255 for _ in range(4)]
    m = np.full((h, w), 255, np.uint8)
    if content == "single":
        m[h // 2, w // 2] = 0
    elif content == "left":
        m[:, 0] = 0
    elif content != "none":
        raise SystemExit("unknown content %r" % content)
    return [m]


def _check(first, sq, dist, near):
    """whether the first frame's outputs are right, by scipy; None without scipy"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    h, w = first.shape
    if not (first == 0).any():
        return bool((sq == 2147483647).all() and np.isposinf(dist).all() and (near == -1).all())
    d = ndimage.distance_transform_edt(first != 0)
    want = np.rint(d * d).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    ny, nx = near // w, near % w
    return bool(np.array_equal(sq, want) and np.array_equal(dist, np.sqrt(sq.astype(np.float32))) and
                (first[ny, nx] == 0).all() and np.array_equal((ny - yy) ** 2 + (nx - xx) ** 2, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x1,3840x2160x8,3840x2160x64,3840x2160x256")
    ap.add_argument("--contents", default="otsu,noise0.01,noise0.5,noise0.99,single,left,none")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        fpx, npx = w * h, w * h * n
        ncopy = {1: (5 * npx // 2 + 15) // 16 * 16, 3: (13 * npx // 2 + 15) // 16 * 16}
        d_rgba = ctx.alloc(fpx * 4 * min(n, 16))
        d_gray, d_mask, d_tmp = ctx.alloc(npx), ctx.alloc(npx), ctx.alloc(ncopy[3])
        d_sq, d_dist, d_near, d_count = ctx.alloc(max(4 * npx, ncopy[3])), ctx.alloc(4 * npx), ctx.alloc(4 * npx), ctx.alloc(4 * n)
        t_copy = {k: _time(ctx, lambda: ctx.stream_copy_dev(d_tmp, d_sq, ncopy[k]), a.warmup, a.iters, a.reps) for k in (1, 3)}
        times = {1: {}, 3: {}}
        for content in a.contents.split(","):
            if content == "otsu":
                for f0 in range(0, n, 16):
                    nf = min(16, n - f0)
                    ctx.synth_dev(d_rgba, w, h, nf, f0, 0x5EED, 1)
                    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_gray + f0 * fpx, w, h, nf)
                ctx.filter_dev(pkg.FILTER_OTSU_GRAY8, d_gray, d_mask, w, h, n)
            else:
                frames = _host_frames(content, h, w)
                for f in range(n):
                    ctx.h2d(d_mask + f * fpx, frames[f % len(frames)])
            ctx.sync()
            first = np.empty((h, w), np.uint8)
            ctx.d2h(first, d_mask)
            t_ccl = _time(ctx, lambda: ctx.ccl_gray8_dev(d_mask, d_sq, d_count, None, None, w, h, n, 8, 0), a.warmup,
                          a.iters, a.reps)
            for outputs in (1, 3):
                ptrs = (d_sq, d_dist, d_near) if outputs == 3 else (0, d_dist, 0)
                t = _time(ctx, lambda: ctx.dist_gray8_dev(d_mask, ptrs[0], ptrs[1], ptrs[2], w, h, n), a.warmup, a.iters,
                          a.reps)
                times[outputs][content] = t
                bpp = 1 + 4 * outputs
                row = {"content": content, "w": w, "h": h, "n": n, "sites": round(float((first == 0).mean()), 4),
                       "outputs": "dist" if outputs == 1 else "sq+dist+nearest", "ms": round(t, 3),
                       "ms_per_frame": round(t / n, 4), "gb_s": round(bpp * npx / t / 1e6, 1),
                       "copy_ms": round(t_copy[outputs], 3), "ratio_vs_copy": round(t / t_copy[outputs], 2),
                       "ccl_ms": round(t_ccl, 3), "ratio_vs_ccl": round(t / t_ccl, 2)}
                if outputs == 3 and not a.no_check:
                    sq, dist, near = np.empty((h, w), np.int32), np.empty((h, w), np.float32), np.empty((h, w), np.int32)
                    ctx.d2h(sq, d_sq)
                    ctx.d2h(dist, d_dist)
                    ctx.d2h(near, d_near)
                    row["equal_scipy"] = _check(first, sq, dist, near)
                print(json.dumps(row), flush=True)
        for outputs in (1, 3):
            t = times[outputs]
            if len(t) > 1:
                slow, fast = max(t, key=t.get), min(t, key=t.get)
                print(json.dumps({"w": w, "h": h, "n": n, "outputs": "dist" if outputs == 1 else "sq+dist+nearest",
                                  "slowest": slow, "fastest": fast, "slowest_over_fastest": round(t[slow] / t[fast], 2)}),
                      flush=True)
        for p in (d_rgba, d_gray, d_mask, d_tmp, d_sq, d_dist, d_near, d_count):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
