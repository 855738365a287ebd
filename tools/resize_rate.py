#!/usr/bin/env python3
"""tools/resize_rate.py — device-resident rate of mi355_resize_dev (NEAREST / LINEAR / AREA, RGBA and gray8), with one
yardstick from the same process and the same buffers: mi355_stream_copy_dev over the same byte count (the source bytes
once plus the output bytes, so a copy of half that many bytes).  copy_ms / ms is the figure that travels between
machines; 1.0 means the resize moves its bytes as fast as the box copies them.

For every row: n frames of sw x sh (hash noise from mi355_synth_rgba8_dev; gray8 planes are its GRAY1 output) to
dw x dh, HIP events (timer_begin / timer_end) around `iters` launches after `warmup`, the median of `reps` such groups.
Mpx/s counts output pixels; GB/s counts algorithmic bytes.  Each row's first output frame is compared with
tests/resize_ref.py on sampled rows (equal_ref).

  python3 tools/resize_rate.py [--scale 1.0] > profiles/resize_rate.txt
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEAREST, LINEAR, AREA = 0, 1, 3
NAMES = {NEAREST: "nearest", LINEAR: "linear", AREA: "area"}
# (frames, src w, src h, dst w, dst h, interpolation)
CASES = [
    (256, 3840, 2160, 1920, 1080, LINEAR),    # the 2 x rule: AREA 2 x 2
    (256, 3840, 2160, 1280, 720, LINEAR),
    (64, 1920, 1080, 3840, 2160, LINEAR),
    (256, 3840, 2160, 1920, 1080, NEAREST),
    (256, 3840, 2160, 960, 540, AREA),        # AREA 4 x 4
    (1024, 640, 480, 320, 240, LINEAR),
    (1024, 640, 480, 1280, 960, LINEAR),
]


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
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every case's frame count")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as entry
    from resize_ref import resize_ref, sample_rows
    pkg = entry.load_package()
    ctx = pkg.Context(0)
    for n, sw, sh, dw, dh, interp in CASES:
        n = max(1, int(n * a.scale))
        src_px, dst_px = sw * sh * n, dw * dh * n
        d_rgba = ctx.alloc(src_px * 4)
        d_y = ctx.alloc(src_px)
        d_out = ctx.alloc(dst_px * 4)
        ctx.synth_dev(d_rgba, sw, sh, n, 0, 0x5EED, 0)
        ctx.filter_dev(pkg.FILTER_GRAY1, d_rgba, d_y, sw, sh, n)
        ctx.sync()
        for layout, d_in, bpp in (("rgba", d_rgba, 4), ("gray8", d_y, 1)):
            t = _time(ctx, lambda: ctx.resize_dev(d_in, d_out, bpp, sw, sh, dw, dh, n, interp), a.warmup, a.iters, a.reps)
            got = np.empty((dh, dw, 4) if bpp == 4 else (dh, dw), np.uint8)
            ctx.d2h(got, d_out)
            frame = np.empty((sh, sw, 4) if bpp == 4 else (sh, sw), np.uint8)
            ctx.d2h(frame, d_in)
            rows = sample_rows(dh)
            equal = bool(np.array_equal(got[rows], resize_ref(frame, dw, dh, interp, rows=rows)))
            # the copy of as many bytes as the resize moves: read nbytes / 2, write nbytes / 2, on the same buffers
            nbytes = (src_px + dst_px) * bpp
            half = min(nbytes // 2, src_px * bpp, dst_px * 4) // 16 * 16
            t_copy = _time(ctx, lambda: ctx.stream_copy_dev(d_out, d_in, half), a.warmup, a.iters, a.reps)
            t_copy *= (nbytes / 2.0) / half       # where a buffer is shorter than half the bytes, per byte
            gbs = nbytes / (t * 1e-3) / 1e9
            print(json.dumps({"case": "%s_%s" % (NAMES[interp], layout), "src": "%dx%d" % (sw, sh),
                              "dst": "%dx%d" % (dw, dh), "n": n, "ms": round(t, 3),
                              "mpx_s": round(dst_px / (t * 1e-3) / 1e6, 1), "gb_s": round(gbs, 1),
                              "copy_ms": round(t_copy, 3), "copy_gb_s": round(nbytes / (t_copy * 1e-3) / 1e9, 1),
                              "ratio_vs_copy": round(t_copy / t, 3), "equal_ref": equal}), flush=True)
        for p in (d_rgba, d_y, d_out):
            ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
