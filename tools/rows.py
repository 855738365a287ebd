#!/usr/bin/env python3
"""tools/rows.py — one line per bench.py run, for tables of kernel rates on ONE box (boxes differ by +-10 %).

    python3 tools/rows.py table | mfma | content          a named row set (ROW_SETS below)
    python3 tools/rows.py sweep <filter> <ENV_VAR> <v1> [<v2> ...] [-- <bench args>]
                                                          A/B of one MI355_TUNE_* knob through the tuning build
                                                          (tools/lib/libmi355_imgfilter_tune.so, `make tune`)

This script never opens the GPU.  Every row is a fresh child, `timeout -k 10 <s> python3 bench.py <args>`, and the
run stops at the first row whose exit status is not 0 — a failed parity check (3), a time limit (124 / 137), an abort
(134) or a segfault (139) alike — after printing that row's stderr tail; the script then exits non-zero.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
TUNE_LIB = os.path.join(ROOT, "tools", "lib", "libmi355_imgfilter_tune.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

COMMON = "--no-cpu-baseline --no-ceiling --no-side-figures"
QUICK = COMMON + " --pool-candidates 1 --steps 20 --warmup 5"   # one plain allocation, 20 launches
LIMIT_S = 180  # a bench.py row takes 10-30 s; the limit only has to end a hang


def row(args, common=COMMON, env=None, limit=LIMIT_S, label=None):
    return {"args": (common + " " + args).split(), "env": env or {}, "limit": limit, "label": label or args}


def table_rows():
    """Every kernel's steady-state rate: 4K, 1080p, ragged, small launches, forced
    implementations, EXACT mode.  The first row also measures the box's streaming ceiling."""
    rows = [row("--filter gray", common=COMMON.replace("--no-ceiling", ""))]
    rows += [row(a) for a in (
        "--filter gray1",
        "--filter gauss --k 3",
        "--filter gauss",
        "--filter gauss --random-alpha",
        "--filter gauss --const-alpha 128",
        "--filter gauss --k 7 --sigma 2.0",
        "--filter gauss --k 9 --sigma 2.5",
        "--filter gauss --k 11 --sigma 3.0 --frames 64",
        "--filter gauss --k 13 --sigma 3.3 --frames 64",
        "--filter gauss --k 17 --sigma 6 --frames 64",
        "--filter sobel",
        # mid-size Sobel launches (8 x 10^7 .. 2^28 pixels: the halo-lane kernel with rows in lock-step), >= 100 ms
        "--filter sobel --frames 16 --steps 800 --warmup 80",
        "--filter sobel --frames 32 --steps 400 --warmup 40",
        "--filter sobel --width 1920 --height 1080 --frames 64 --steps 800 --warmup 80",
        "--filter pipeline --k 3",
        "--filter pipeline",
        "--filter pipeline --k 7",
        "--filter gauss --width 1023 --height 819 --frames 2048",
        "--filter sobel --width 1023 --height 819 --frames 2048",
        "--filter pipeline --width 1023 --height 819 --frames 2048",
        "--filter gauss --frames 1 --steps 300",
        "--filter gauss --frames 8 --steps 200",
        "--filter gauss --frames 64",
        # one rank of an 8-GPU strong-scaling job (BASELINE config 5: 64 x 4K through the pipeline), >= 200 ms
        "--filter pipeline --frames 64 --steps 400 --warmup 40",
        "--filter pipeline --frames 128 --steps 200 --warmup 20",
        "--filter gauss --frames 32 --steps 600 --warmup 60",
        # BASELINE.json config 2 and friends: 1080p frames (1024 frames = the 4K batches' byte count)
        "--filter gauss --width 1920 --height 1080 --frames 1024",
        "--filter gauss --width 1920 --height 1080 --frames 1024 --random-alpha",
        "--filter sobel --width 1920 --height 1080 --frames 1024",
        "--filter pipeline --width 1920 --height 1080 --frames 1024",
        "--filter gauss --width 1920 --height 1080 --frames 1",
        "--filter gauss --k 17 --sigma 6 --width 1920 --height 1080 --frames 256",
        # config 5, N = 1 leg: 512 x 4K through the fused pipeline
        "--filter pipeline --total-frames 512",
        # the matrix-core Gaussian forced at small k, the VALU kernels forced where AUTO no longer takes them
        "--filter gauss --k 5 --frames 64 --impl mfma",
        "--filter gauss --k 7 --sigma 2.0 --impl mfma",
        "--filter gauss --k 9 --sigma 2.5 --impl valu",
        "--filter gauss --k 11 --sigma 3.0 --frames 64 --impl valu",
        "--filter gauss --k 17 --sigma 6 --frames 64 --impl valu",
        "--filter gauss --k 17 --sigma 6 --frames 256",
        "--filter gauss --k 17 --sigma 6 --frames 256 --random-alpha",
        # EXACT mode (bit-identical to the CPU path): exact-by-exception sliding kernel (k = 3, 5), tiled kernel (k >= 7)
        "--filter gauss --mode exact --k 3 --sigma 0.8",
        "--filter gauss --mode exact",
        "--filter gauss --mode exact --random-alpha",
        "--filter gauss --mode exact --frames 64 --impl tile",
        "--filter gauss --mode exact --k 7 --sigma 2.0 --frames 64",
    )]
    return rows


def mfma_rows():
    """The matrix-core Gaussian (--impl mfma) beside the library's own choice (--impl auto), 64 x 4K frames."""
    rows = []
    for k, sigma in ((5, 1.5), (7, 2.0), (9, 2.5), (11, 3.0), (13, 3.3), (17, 6.0)):
        for impl in ("auto", "mfma"):
            rows.append(row("--filter gauss --k %d --sigma %s --frames 64 --impl %s" % (k, sigma, impl), common=QUICK))
    rows += [row(a, common=QUICK) for a in (
        "--filter gauss --k 17 --sigma 6 --frames 256 --impl mfma",
        "--filter gauss --k 17 --sigma 6 --frames 64 --impl mfma --random-alpha",
        "--filter gauss --k 17 --sigma 6 --frames 64 --impl auto --random-alpha",
        "--filter gauss --k 17 --sigma 6 --frames 256 --width 1920 --height 1080 --impl mfma",
    )]
    return rows


def content_rows():
    """How much each kernel's rate depends on frame content (256 x 4K frames): mode 0 hash noise (the bench workload),
    1 gradient + noise, 2 flat 64 x 64 patches (every window constant: the exact-by-exception kernels' table path),
    3 gray noise (r = g = b: the luminance's ambiguous case on every pixel), and the reference's own test photographs
    (decoded pixels, tests/golden) tiled to 4K — Tulips (colour), Artemis (near-gray)."""
    contents = [("--synth-mode %d" % m, None) for m in range(4)]
    for png in ("tulips_medium640_rgb.png", os.path.join("ref_images", "Artemis_medium640_rgb.png")):
        contents.append(("--photo " + os.path.join(GOLDEN, png), "--photo " + png))
    rows = []
    for f in ("gauss", "gauss --mode exact", "sobel", "pipeline", "gray"):
        for args, label in contents:
            rows.append(row("--filter %s %s" % (f, args), common=QUICK,
                            label="--filter %s %s" % (f, label or args)))
    return rows


def sweep_rows(argv):
    """sweep <filter> <ENV_VAR> <v1> [<v2> ...] [-- <bench args>]: the default, then one row per value, all through
    the tuning build (the only one that reads MI355_TUNE_*: slide_common.hpp, gray.hip, sobel_slide.hip, ...)."""
    if len(argv) < 3:
        sys.exit("usage: rows.py sweep <filter> <ENV_VAR> <v1> [<v2> ...] [-- <bench args>]")
    filt, var, rest = argv[0], argv[1], argv[2:]
    values, extra = (rest[:rest.index("--")], rest[rest.index("--") + 1:]) if "--" in rest else (rest, [])
    args = " ".join(["--filter", filt] + extra)
    rows = [row(args, env={"MI355_IMGFILTER_LIB": TUNE_LIB}, label="%s default" % args)]
    for v in values:
        rows.append(row(args, env={"MI355_IMGFILTER_LIB": TUNE_LIB, var: v}, label="%s %s=%s" % (args, var, v)))
    return rows


ROW_SETS = {"table": table_rows, "mfma": mfma_rows, "content": content_rows}
SIGNALS = {124: "time limit", 137: "killed at the time limit", 134: "abort", 139: "segmentation fault",
           3: "parity violation"}


def fmt(label, d):
    r = d["roofline"]
    p = d.get("parity") or {}
    par = "-" if not p else "max|d| %s" % p.get("max_abs_diff")
    if p.get("mismatch_frac") is not None:
        par += " mism %.2e" % p["mismatch_frac"]
    line = "%-64s %6.0f GB/s  %5.1f %%  %7.3f ms  %9.0f Mpx/s  parity %s" % (
        label, r["achieved"], 100 * r["frac"], r["avg_launch_ms"], d["value"], par)
    if r.get("copy_ceiling_GBs"):
        line += "  | box ceiling %.0f GB/s (%s)" % (r["copy_ceiling_GBs"], r.get("copy_ceiling_kernel", ""))
    return line


def run(rows):
    for i, rw in enumerate(rows):
        cmd = ["timeout", "-k", "10", str(rw["limit"]), sys.executable, BENCH] + rw["args"]
        out = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **rw["env"]), capture_output=True, text=True)
        d = None
        if out.returncode == 0:
            try:
                d = json.loads(out.stdout.strip().splitlines()[-1])
            except (ValueError, IndexError):
                pass
        if d is None:
            why = SIGNALS.get(out.returncode, "no JSON line" if out.returncode == 0 else "error")
            print("row %d/%d FAILED (exit %d, %s): %s" % (i + 1, len(rows), out.returncode, why, " ".join(cmd)))
            print("  stderr tail:\n" + "\n".join("    " + s for s in out.stderr[-3000:].splitlines()[-25:]))
            print("stopped: %d row(s) not run" % (len(rows) - i - 1))
            return out.returncode or 1
        print(fmt(rw["label"], d), flush=True)
    return 0


def main(argv):
    if argv and argv[0] == "sweep":
        rows = sweep_rows(argv[1:])
    elif len(argv) == 1 and argv[0] in ROW_SETS:
        rows = ROW_SETS[argv[0]]()
    else:
        sys.exit(__doc__)
    return run(rows)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
