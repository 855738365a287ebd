#!/usr/bin/env python3
"""tools/box_rate.py — device-resident rate of the box mean (MI355_FILTER_BOX / BOX_GRAY8) and of the mean adaptive
threshold (mi355_adaptive_threshold_gray8_dev), with three yardsticks from the same process and the same buffers:

  * mi355_stream_copy_dev over the same algorithmic bytes (RGBA 8 B/px, gray8 2 B/px): the box's own "read N, write N";
  * the FAST Gaussian that moves the same bytes: GAUSS k = 5 for RGBA, GAUSS_GRAY8 k = 3 for gray8;
  * what a user does today without the filter: torch on the GPU, uint8 -> float32, replicate pad + avg_pool2d, + 0.5,
    -> uint8, the conversions INSIDE the timed region, on as many frames as fit in ~8 GB of temporaries.  Its output is
    checked once within 1 LSB of tests/box_ref.py on sampled rows (torch's fp32 mean and rounding are not the contract).

For every row: n frames of w x h (hash noise from mi355_synth_rgba8_dev; gray8 planes are its GRAY1 output), HIP events
around `iters` launches after `warmup`, the median of `reps` such groups.  The last lines state the two expectations:
BOX k = 5 against the Gaussian k = 5, and t(k = 63) / t(k = 3) against (B + 62) / (B + 2) for the plan's band height B.

  python3 tools/box_rate.py [--shapes 3840x2160x256,640x480x1024] [--ks 3,5,9,17,31,63] [--blocks 3,15,63] [--no-torch]
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


def torch_box(torch, x, k):
    """x: (N, C, H, W) uint8 on the GPU -> the rounded k x k mean with replicated borders, (N, C, H, W) uint8."""
    F = torch.nn.functional
    r = k // 2
    v = F.avg_pool2d(F.pad(x.to(torch.float32), (r, r, r, r), mode="replicate"), k, stride=1)
    return (v + 0.5).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x256,640x480x1024")
    ap.add_argument("--ks", default="3,5,9,17,31,63")
    ap.add_argument("--blocks", default="3,15,63")
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
    import box_cases as bc
    from box_ref import BINARY, adaptive_ref, box_ref
    from median_ref import sample_rows
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    ks = [int(k) for k in a.ks.split(",")]
    blocks = [int(k) for k in a.blocks.split(",")]
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        npx = w * h * n
        d_rgba, d_y, d_out = ctx.alloc(npx * 4), ctx.alloc(npx), ctx.alloc(npx * 4)
        ctx.synth_dev(d_rgba, w, h, n, 0, 0x5EED, 0)
        ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y, w, h, n)
        ctx.sync()
        for layout, d_in, bpp, gauss, gk in (("rgba", d_rgba, 4, pkg.FILTER_GAUSS, 5),
                                             ("gray8", d_y, 1, pkg.FILTER_GAUSS_GRAY8, 3)):
            gray8 = bpp == 1
            t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_out, d_in, npx * bpp), a.warmup, a.iters, a.reps)
            t_gauss = _time(ctx, lambda: ctx.filter_dev(gauss, d_in, d_out, w, h, n, gk, 0.3 * ((gk - 1) * 0.5 - 1) + 0.8),
                            a.warmup, a.iters, a.reps)
            frame = np.empty((h, w, 4) if bpp == 4 else (h, w), np.uint8)
            ctx.d2h(frame, d_in)
            calls = [("box_" + layout, k) for k in ks] + ([("adaptive_gray8", k) for k in blocks] if gray8 else [])
            t_of = {}
            for name, k in calls:
                if name.startswith("box"):
                    filt = pkg.FILTER_BOX_GRAY8 if gray8 else pkg.FILTER_BOX

                    def fn():
                        ctx.filter_dev(filt, d_in, d_out, w, h, n, k, 0.0)
                else:
                    def fn():
                        ctx.adaptive_threshold_gray8_dev(d_in, d_out, w, h, n, 255, BINARY, k, 2.5)
                t = _time(ctx, fn, a.warmup, a.iters, a.reps)
                t_of[(name, k)] = t
                gbs = 2.0 * bpp * npx / (t * 1e-3) / 1e9
                row = {"call": name, "w": w, "h": h, "n": n, "k": k, "band_rows": bc.band_rows(k, w, h, n, gray8),
                       "ms": round(t, 3), "gb_s": round(gbs, 1), "frac_8TBs": round(gbs / 8000.0, 3),
                       "copy_ms": round(t_copy, 3), "ratio_vs_copy": round(t_copy / t, 3),
                       "gauss_k": gk, "gauss_ms": round(t_gauss, 3), "ratio_vs_gauss": round(t_gauss / t, 3)}
                got = np.empty_like(frame)
                ctx.d2h(got, d_out)
                rows = sample_rows(h, 2 * k)
                ref = box_ref(frame, k, rows=rows)
                if name.startswith("box"):
                    row["equal_ref"] = bool(np.array_equal(got[rows], ref))
                else:
                    row["equal_ref"] = bool(np.array_equal(got[rows], adaptive_ref(frame, 255, BINARY, k, 2.5, rows=rows,
                                                                                   mean=ref)))
                if torch is not None and name.startswith("box"):
                    per_frame = h * w * bpp * 4 * 4  # the fp32 copy, the padded copy, the pooled result, the sum
                    nt = max(1, min(n, int(a.torch_gb * 1e9 // per_frame)))
                    x = torch.from_numpy(np.repeat(frame[None], nt, 0)).cuda()
                    x = x.permute(0, 3, 1, 2).contiguous() if bpp == 4 else x[:, None].contiguous()
                    out = torch_box(torch, x, k)
                    torch.cuda.synchronize()
                    tg = out[0].permute(1, 2, 0).cpu().numpy() if bpp == 4 else out[0, 0].cpu().numpy()
                    lsb = int(np.abs(tg[rows].astype(np.int16) - ref.astype(np.int16)).max())
                    ts = []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        torch_box(torch, x, k)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    tt = float(np.median(ts))
                    row.update({"torch_frames": nt, "torch_ms_per_frame": round(tt / nt, 3),
                                "speedup_vs_torch": round((tt / nt) / (t / n), 1), "torch_max_lsb": lsb})
                    del x, out
                    torch.cuda.empty_cache()
                print(json.dumps(row), flush=True)
            name = "box_" + layout
            if (name, 3) in t_of and (name, 63) in t_of:
                b = bc.band_rows(63, w, h, n, gray8)
                print(json.dumps({"expectation": "t(k=63) / t(k=3) <= (B + 62) / (B + 2)", "layout": layout, "w": w, "h": h,
                                  "n": n, "B": b, "measured": round(t_of[(name, 63)] / t_of[(name, 3)], 3),
                                  "bound": round((b + 62) / (b + 2), 3)}), flush=True)
            if not gray8 and (name, 5) in t_of:
                print(json.dumps({"expectation": "box k=5 takes no longer than FAST gauss k=5 (+-4 %)", "w": w, "h": h,
                                  "n": n, "box_ms": round(t_of[(name, 5)], 3), "gauss_ms": round(t_gauss, 3),
                                  "box_over_gauss": round(t_of[(name, 5)] / t_gauss, 3)}), flush=True)
        for p in (d_rgba, d_y, d_out):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
