#!/usr/bin/env python3
"""tools/yuv_rate.py — device-resident rate of the YUV conversions (mi355_yuv_to_rgba8_dev / mi355_rgba8_to_yuv_dev) with
two yardsticks from the same process and the same buffers:

  * mi355_stream_copy_dev of the same TOTAL bytes: a 4:2:0 conversion moves 5.5 bytes per pixel (1.5 on the YUV side, 4
    on the RGBA side), the packed decode 6, so the copy yardstick copies 2.75 (3) bytes per pixel from one RGBA buffer
    to the other: it reads N / 2 and writes N / 2 for the same N;
  * MI355_FILTER_GRAY1, the nearest existing kernel (reads 4, writes 1 byte per pixel), with its own copy yardstick of
    2.5 bytes per pixel.  The claim under test is that the conversions are memory-bound: their share of the copy rate
    should be GRAY1's.

Every row also gives the bytes it WRITES per second beside the copy's: the decode writes 4 of its 5.5 bytes, the copy half
of them, and mi355_bgr_to_rgba8_dev (3 bytes read, 4 written per pixel) is timed as the existing write-heavy kernel.

Rows: NV12 and I420 decode, NV12 encode, YUY2 decode; tight, and with a pitch of 4096 (4:2:0) / 8192 (packed) whose
padding is never touched (the bytes counted are the pixel bytes only).  Content: hash noise (mi355_synth_rgba8_dev)
encoded to the layout on the device; the first frame of every decode row is checked against tests/yuv_ref.py.
Every figure: HIP events around `iters` calls after `warmup`, `reps` such groups; the median and the spread
(max - min) / median of the groups are printed.  GB/s counts the pixel bytes a conversion must move.

  python3 tools/yuv_rate.py [--shapes 3840x2160x64,3840x2160x256] [--iters 10] [--reps 9]

On a shared GPU run it as one step under its own time limit, chained to whatever follows with &&:
  timeout -k 10 300 python3 tools/yuv_rate.py > profiles/yuv_rate.txt && ...
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
    """(median ms per call, (max - min) / median) over `reps` groups of `iters` calls"""
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_begin()
        for _ in range(iters):
            fn()
        ms.append(ctx.timer_end() / iters)
    med = float(np.median(ms))
    return med, (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3840x2160x64,3840x2160x256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import __graft_entry__ as entry
    import yuv_ref as yr
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    t = lambda fn: _time(ctx, fn, a.warmup, a.iters, a.reps)  # noqa: E731
    rows = [("decode", yr.NV12, 0), ("decode", yr.NV12, 4096), ("decode", yr.I420, 0), ("decode", yr.I420, 4096),
            ("encode", yr.NV12, 0), ("encode", yr.NV12, 4096), ("decode", yr.YUY2, 0), ("decode", yr.YUY2, 8192)]
    for shape in a.shapes.split(","):
        w, h, n = (int(v) for v in shape.split("x"))
        npx = w * h * n
        d_rgba, d_back = ctx.alloc(npx * 4), ctx.alloc(npx * 4)
        d_yuv = ctx.alloc(max(pkg.yuv_frame_bytes(lay, w, h, p, 0) for _, lay, p in rows) * n)
        for f0 in range(0, n, 16):
            ctx.synth_dev(d_rgba + f0 * w * h * 4, w, h, min(16, n - f0), f0, 0x5EED, 0)
        ctx.sync()
        base = {"w": w, "h": h, "n": n}
        # the second yardstick: GRAY1 and the copy of its 5 B/px, on the same buffers
        g_ms, g_sp = t(lambda: ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_yuv, w, h, n))
        gc_ms, gc_sp = t(lambda: ctx.stream_copy_dev(d_back, d_rgba, npx * 5 // 2))
        gray1_share = gc_ms / g_ms
        print(json.dumps(dict(base, op="gray1", ms=round(g_ms, 3), spread=round(g_sp, 3), gb_s=round(5 * npx / g_ms / 1e6, 1),
                              copy_ms=round(gc_ms, 3), copy_spread=round(gc_sp, 3),
                              copy_gb_s=round(5 * npx / gc_ms / 1e6, 1), share_of_copy=round(gray1_share, 3))), flush=True)
        # a third figure for the write-heavy decode rows: mi355_bgr_to_rgba8_dev, the existing kernel that also writes
        # 4 of its 7 bytes per pixel (one 16-byte store per lane, lanes side by side), on the same output buffer
        b_ms, b_sp = t(lambda: ctx.bgr_to_rgba_dev(d_rgba, d_back, w, h, n))
        print(json.dumps(dict(base, op="bgr_to_rgba", ms=round(b_ms, 3), spread=round(b_sp, 3),
                              gb_s=round(7 * npx / b_ms / 1e6, 1), write_gb_s=round(4 * npx / b_ms / 1e6, 1),
                              copy_write_gb_s=round(2.5 * npx / gc_ms / 1e6, 1))), flush=True)
        for op, layout, pitch in rows:
            packed = yr.is_packed(layout)
            bpp2 = 12 if packed else 11            # twice the bytes per pixel a conversion moves
            fb = pkg.yuv_frame_bytes(layout, w, h, pitch, 0)
            # content: the synthetic frames encoded on the device; the packed layouts, which have no encode, take the
            # RGBA noise bytes as they are
            if packed:
                ctx.stream_copy_dev(d_yuv, d_rgba, fb * n)
            else:
                ctx.rgba8_to_yuv_dev(d_rgba, d_yuv, w, h, n, layout, yr.BT601, pitch, 0)
            ctx.sync()
            c_ms, c_sp = t(lambda: ctx.stream_copy_dev(d_back, d_rgba, npx * bpp2 // 4))
            if op == "decode":
                fn = lambda: ctx.yuv_to_rgba8_dev(d_yuv, d_back, w, h, n, layout, yr.BT601, pitch, 0)  # noqa: E731
            else:
                fn = lambda: ctx.rgba8_to_yuv_dev(d_rgba, d_yuv, w, h, n, layout, yr.BT601, pitch, 0)  # noqa: E731
            ms, sp = t(fn)
            ok = None
            if op == "decode":
                frame, got = np.empty(fb, np.uint8), np.empty((h, w, 4), np.uint8)
                ctx.d2h(frame, d_yuv)
                ctx.d2h(got, d_back)
                ctx.sync()
                ok = bool(np.array_equal(got, yr.decode(frame, w, h, layout, yr.BT601, pitch, 0)[0]))
            share = c_ms / ms
            print(json.dumps(dict(base, op=op, layout=yr.LAYOUT_NAMES[layout], pitch=pitch or "tight", ms=round(ms, 3),
                                  spread=round(sp, 3), gb_s=round(bpp2 * npx / 2 / ms / 1e6, 1),
                                  write_gb_s=round((4 if op == "decode" else 1.5) * npx / ms / 1e6, 1),
                                  copy_write_gb_s=round(bpp2 * npx / 4 / c_ms / 1e6, 1), copy_ms=round(c_ms, 3),
                                  copy_spread=round(c_sp, 3), copy_gb_s=round(bpp2 * npx / 2 / c_ms / 1e6, 1),
                                  share_of_copy=round(share, 3), gray1_share_of_copy=round(gray1_share, 3),
                                  vs_gray1_share=round(share / gray1_share, 3), equal_ref=ok)), flush=True)
        for p in (d_rgba, d_back, d_yuv):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
