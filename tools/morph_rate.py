#!/usr/bin/env python3
"""tools/morph_rate.py — device-resident rate of rectangular morphology (MI355_FILTER_ERODE / DILATE / OPEN / CLOSE and
their *_GRAY8 forms), with two yardsticks from the same process and the same buffers:

  * the Gaussian k = 3 (FAST; GAUSS for RGBA, GAUSS_GRAY8 for gray8), which moves the same bytes: the ratio
    gauss_ms / morph_ms is the figure that travels between machines;
  * what a user does today without the filter: torch on the GPU, uint8 -> float16, replicate pad + max_pool2d (erode as
    -max_pool2d(-x); OPEN / CLOSE as two such stages, each padding its own input), -> uint8.  The two conversions are
    INSIDE the timed region (max_pool2d does not take uint8 on the GPU).  It runs on as many frames as fit in ~8 GB of
    temporaries, and its output is checked against tests/morph_ref.py once, on sampled rows.

For every row: n frames of w x h (hash noise from mi355_synth_rgba8_dev; gray8 planes are its GRAY1 output), HIP events
around `iters` launches after `warmup`, the median of `reps` such groups.  GB/s counts algorithmic bytes (RGBA 8 B/px,
gray8 2 B/px); the fraction is of the 8 TB/s spec peak.

  python3 tools/morph_rate.py [--w 3840 --h 2160 --n 256] [--ks 3,5,9,17] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OPS = ("erode", "dilate", "open", "close")


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


def torch_morph(torch, x, k, op):
    """x: (N, C, H, W) uint8 on the GPU -> the morphology with replicated borders, (N, C, H, W) uint8."""
    F = torch.nn.functional
    r = k // 2

    def dilate(v):
        return F.max_pool2d(F.pad(v, (r, r, r, r), mode="replicate"), k, stride=1)

    def erode(v):
        return -dilate(-v)

    v = x.to(torch.float16)
    v = {"erode": erode, "dilate": dilate, "open": lambda t: dilate(erode(t)),
         "close": lambda t: erode(dilate(t))}[op](v)
    return v.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--ks", default="3,5,9,17")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-gb", type=float, default=8.0)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    torch = None
    if not a.no_torch:
        import torch  # first: torch brings its own HIP runtime and must initialise it before the library loads
        torch.cuda.init()
    import __graft_entry__ as entry
    from median_ref import sample_rows
    from morph_ref import morph_ref
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    w, h, n = a.w, a.h, a.n
    npx = w * h * n
    d_rgba = ctx.alloc(npx * 4)
    d_y = ctx.alloc(npx)
    d_out = ctx.alloc(npx * 4)
    ctx.synth_dev(d_rgba, w, h, n, 0, 0x5EED, 0)
    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y, w, h, n)
    ctx.sync()
    ks = [int(k) for k in a.ks.split(",")]
    for layout, gauss, d_in, bpp in (("rgba", pkg.FILTER_GAUSS, d_rgba, 4), ("gray8", pkg.FILTER_GAUSS_GRAY8, d_y, 1)):
        t_gauss = _time(ctx, lambda: ctx.filter_dev(gauss, d_in, d_out, w, h, n, 3, 0.8), a.warmup, a.iters, a.reps)
        frame = np.empty((h, w, 4) if bpp == 4 else (h, w), np.uint8)
        ctx.d2h(frame, d_in)
        for op in OPS:
            filt = getattr(pkg, "FILTER_" + op.upper() + ("_GRAY8" if bpp == 1 else ""))
            for k in ks:
                t = _time(ctx, lambda: ctx.filter_dev(filt, d_in, d_out, w, h, n, k, 0.0), a.warmup, a.iters, a.reps)
                gbs = 2.0 * bpp * npx / (t * 1e-3) / 1e9
                row = {"filter": op + "_" + layout, "w": w, "h": h, "n": n, "k": k, "ms": round(t, 3),
                       "mpx_s": round(npx / (t * 1e-3) / 1e6, 1), "gb_s": round(gbs, 1),
                       "frac_8TBs": round(gbs / 8000.0, 3), "gauss3_ms": round(t_gauss, 3),
                       "ratio_vs_gauss3": round(t_gauss / t, 3)}
                # the kernel's own output on the first frame, on sampled rows
                got = np.empty_like(frame)
                ctx.d2h(got, d_out)
                rows = sample_rows(h, 2 * k)
                ref = morph_ref(op, frame, k, rows=rows)
                row["equal_ref"] = bool(np.array_equal(got[rows], ref))
                if torch is not None:
                    # frames that fit: the fp16 copy, the padded copy and the pooled result, two stages
                    per_frame = h * w * bpp * 2 * 6
                    nt = max(1, min(n, int(a.torch_gb * 1e9 // per_frame)))
                    x = torch.from_numpy(np.repeat(frame[None], nt, 0)).cuda()
                    x = x.permute(0, 3, 1, 2).contiguous() if bpp == 4 else x[:, None].contiguous()
                    out = torch_morph(torch, x, k, op)
                    torch.cuda.synchronize()
                    tg = out[0].permute(1, 2, 0).cpu().numpy() if bpp == 4 else out[0, 0].cpu().numpy()
                    same = bool(np.array_equal(tg[rows], ref))
                    ts = []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        torch_morph(torch, x, k, op)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    tt = float(np.median(ts))
                    row.update({"torch_frames": nt, "torch_ms_per_frame": round(tt / nt, 3),
                                "torch_mpx_s": round(nt * h * w / (tt * 1e-3) / 1e6, 1),
                                "speedup_vs_torch": round((tt / nt) / (t / n), 1), "torch_equal_ref": same})
                    del x, out
                    torch.cuda.empty_cache()
                print(json.dumps(row), flush=True)
    for p in (d_rgba, d_y, d_out):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
