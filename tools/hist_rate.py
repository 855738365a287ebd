#!/usr/bin/env python3
"""tools/hist_rate.py — device-resident rate of the whole-frame statistics of single-channel frames: the histogram
(mi355_hist_gray8_dev), MI355_FILTER_EQUALIZE_GRAY8 and MI355_FILTER_OTSU_GRAY8, with two yardsticks from the same
process and the same buffers:

  * mi355_stream_copy_dev of the frames (reads and writes w h n bytes: 2 B/px).  The histogram reads 1 B/px, so its
    floor is 0.5x the copy time; equalize and Otsu read the frame twice and write it once (3 B/px), floor 1.5x;
  * what a user does today without the calls: torch on the GPU, a frame-offset bincount, cumsum and the table
    arithmetic, and a gather through the table, all inside the timed region.  It runs on as many frames as fit in
    ~8 GB of temporaries; its Otsu is the vectorised between-class-variance argmax (not OpenCV's serial loop), so it
    is a timing yardstick only, and its equality with tests/hist_ref.py is reported per row.

Contents: noise (hash noise from mi355_synth_rgba8_dev through GRAY1), flat 64 x 64 patches (synth mode 2 through
GRAY1) and constant frames (every pixel in one bin).  Every row: HIP events around `iters` calls after `warmup`, the
median of `reps` such groups; GB/s counts 1 B/px for the histogram and 3 B/px for equalize and Otsu.  Each row checks
the first frame's result against tests/hist_ref.py.  The last rows give the latency of one call on one 640 x 480
frame (each call timed alone).

  python3 tools/hist_rate.py [--shapes 3840x2160x256,640x480x1024] [--no-torch]
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


def torch_stats(torch, x, op):
    """x: (n, h, w) uint8 on the GPU -> (n, 256) histogram, or the equalized / thresholded frames."""
    n = x.shape[0]
    total = x.shape[1] * x.shape[2]
    off = (torch.arange(n, device=x.device) * 256)[:, None]
    idx = x.view(n, -1).long() + off
    hist = torch.bincount(idx.view(-1), minlength=256 * n).view(n, 256)
    if op == "hist":
        return hist
    bins = torch.arange(256, device=x.device)
    if op == "equalize":
        i0 = (hist > 0).int().argmax(1, keepdim=True)
        h0 = hist.gather(1, i0)
        scale = 255.0 / (total - h0).clamp(min=1).float()
        lut = torch.round((hist.cumsum(1) - h0).float() * scale).clamp(0, 255)
        lut = torch.where(bins[None] > i0, lut, torch.zeros_like(lut))
        lut = torch.where(h0 == total, i0.float().expand(-1, 256), lut).to(torch.uint8)
    else:
        p = hist.double() / total
        q1 = p.cumsum(1)
        m1 = (p * bins).cumsum(1)
        mu = m1[:, -1:]
        sigma = torch.nan_to_num((mu * q1 - m1) ** 2 / (q1 * (1.0 - q1)), nan=0.0, posinf=0.0)
        t = sigma.argmax(1, keepdim=True)
        lut = ((bins[None] > t) * 255).to(torch.uint8)
    return lut.view(-1)[idx].view_as(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x256,640x480x1024")
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
    from hist_ref import equalize_ref, hist_ref, otsu_ref
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        npx = w * h * n
        d_rgba = ctx.alloc(w * h * 4 * min(n, 16))
        d_y, d_out, d_hist = ctx.alloc(npx), ctx.alloc(npx), ctx.alloc(n * 1024)
        for content in ("noise", "patches", "constant"):
            if content == "constant":
                frame = np.full((h, w), 77, np.uint8)
                for f in range(n):
                    ctx.h2d(d_y + f * w * h, frame)
            else:
                for f0 in range(0, n, 16):
                    nf = min(16, n - f0)
                    ctx.synth_dev(d_rgba, w, h, nf, f0, 0x5EED, 0 if content == "noise" else 2)
                    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y + f0 * w * h, w, h, nf)
            ctx.sync()
            frame = np.empty((h, w), np.uint8)
            ctx.d2h(frame, d_y)
            t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_out, d_y, npx), a.warmup, a.iters, a.reps)
            calls = {
                "hist": (lambda: ctx.hist_gray8_dev(d_y, d_hist, w, h, n), 1),
                "equalize": (lambda: ctx.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, d_y, d_out, w, h, n), 3),
                "otsu": (lambda: ctx.filter_dev(pkg.FILTER_OTSU_GRAY8, d_y, d_out, w, h, n), 3),
            }
            refs = {"hist": lambda: hist_ref(frame), "equalize": lambda: equalize_ref(frame),
                    "otsu": lambda: otsu_ref(frame)}
            for op, (fn, bpp) in calls.items():
                t = _time(ctx, fn, a.warmup, a.iters, a.reps)
                gbs = bpp * npx / (t * 1e-3) / 1e9
                if op == "hist":
                    got = np.empty(256, np.uint32)
                    ctx.d2h(got, d_hist)
                else:
                    got = np.empty_like(frame)
                    ctx.d2h(got, d_out)
                ref = refs[op]()
                row = {"op": op, "content": content, "w": w, "h": h, "n": n, "ms": round(t, 3),
                       "gb_s": round(gbs, 1), "copy_ms": round(t_copy, 3), "ratio_vs_copy": round(t / t_copy, 3),
                       "equal_ref": bool(np.array_equal(got, ref))}
                if torch is not None:
                    per_frame = h * w * (1 + 8 + 8 + 1)  # uint8 frame, int64 index, int64 offset index, output
                    nt = max(1, min(n, int(a.torch_gb * 1e9 // per_frame)))
                    x = torch.from_numpy(np.repeat(frame[None], nt, 0)).cuda()
                    out = torch_stats(torch, x, op)
                    torch.cuda.synchronize()
                    tg = out[0].cpu().numpy()
                    same = bool(np.array_equal(tg.astype(ref.dtype), ref))
                    ts = []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        torch_stats(torch, x, op)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    tt = float(np.median(ts))
                    row.update({"torch_frames": nt, "torch_ms_per_frame": round(tt / nt, 4),
                                "speedup_vs_torch": round((tt / nt) / (t / n), 1), "torch_equal_ref": same})
                    del x, out
                    torch.cuda.empty_cache()
                print(json.dumps(row), flush=True)
        for p in (d_rgba, d_y, d_out, d_hist):
            ctx.free(p)
    # latency of one call on one 640 x 480 frame, each call timed alone
    w, h = 640, 480
    d_y, d_out, d_hist = ctx.alloc(w * h), ctx.alloc(w * h), ctx.alloc(1024)
    d_rgba = ctx.alloc(w * h * 4)
    ctx.synth_dev(d_rgba, w, h, 1, 0, 0x5EED, 0)
    ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y, w, h, 1)
    for op, fn in (("copy", lambda: ctx.stream_copy_dev(d_out, d_y, w * h)),
                   ("hist", lambda: ctx.hist_gray8_dev(d_y, d_hist, w, h, 1)),
                   ("otsu_thresholds", lambda: ctx.otsu_thresholds_gray8_dev(d_y, d_hist, w, h, 1)),
                   ("equalize", lambda: ctx.filter_dev(pkg.FILTER_EQUALIZE_GRAY8, d_y, d_out, w, h, 1)),
                   ("otsu", lambda: ctx.filter_dev(pkg.FILTER_OTSU_GRAY8, d_y, d_out, w, h, 1))):
        t = _time(ctx, fn, 20, 1, 101)
        print(json.dumps({"latency_op": op, "w": w, "h": h, "n": 1, "ms_one_call": round(t, 4)}), flush=True)
    for p in (d_rgba, d_y, d_out, d_hist):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
