"""CPU reference of the Hough line transform (mi355_hough_*), the rules of include/mi355_imgfilter.h "from edges to lines"
restated in numpy, twice: vectorised (per angle: two fp32 products, an fp32 sum, np.rint, np.bincount; the peak rule by
shifted comparisons; np.lexsort for the order) and, for tiny frames, loop by loop as the header reads.  test_hough_cpu.py
holds the two against each other.

The trig table is an argument everywhere: the GPU tests pass the library's own (mi355_hough_trig_table), because the
platform's cos and sin are part of the contract; trig_table() below is numpy's, which the CPU test compares within 1 ulp.
"""
import math

import numpy as np

F32 = np.float32


def shape(w, h, rho, theta, min_theta=0.0, max_theta=math.pi):
    """(numangle, numrho)"""
    numangle = int(math.floor((max_theta - min_theta) / theta)) + 1
    if numangle > 1 and abs(math.pi - (numangle - 1) * theta) < theta / 2:
        numangle -= 1
    numrho = int(np.rint(F32(2 * (w + h) + 1) / F32(rho)))      # fp32 division, half to even
    return numangle, numrho


def trig_table(numangle, rho, theta, min_theta=0.0):
    """(tab_cos, tab_sin) with numpy's cos and sin: ang is an fp32 variable, the products are taken in double"""
    irho = F32(1.0) / F32(rho)
    tc, ts = np.empty(numangle, F32), np.empty(numangle, F32)
    ang = F32(min_theta)
    for n in range(numangle):
        tc[n] = F32(np.cos(np.float64(ang)) * np.float64(irho))
        ts[n] = F32(np.sin(np.float64(ang)) * np.float64(irho))
        ang = F32(ang + F32(theta))
    return tc, ts


def accum_ref(img, tab_cos, tab_sin, numrho):
    """The (numangle + 2, numrho + 2) int32 accumulator of one (h, w) frame, its zero ring included.  A vote outside
    0 .. numrho - 1 is dropped."""
    numangle = len(tab_cos)
    ys, xs = np.nonzero(img)
    fx, fy = xs.astype(F32), ys.astype(F32)
    acc = np.zeros((numangle + 2, numrho + 2), np.int32)
    half = (numrho - 1) // 2
    for n in range(numangle):
        s = (fx * F32(tab_cos[n])) + (fy * F32(tab_sin[n]))      # three fp32 roundings: numpy fuses nothing
        assert s.dtype == F32
        r = np.rint(s).astype(np.int64) + half
        r = r[(r >= 0) & (r < numrho)]
        acc[n + 1, 1:numrho + 1] = np.bincount(r, minlength=numrho)
    return acc


def accum_literal(img, tab_cos, tab_sin, numrho):
    """accum_ref pixel by pixel, as the header's "votes" paragraph reads"""
    numangle = len(tab_cos)
    h, w = img.shape
    acc = np.zeros((numangle + 2) * (numrho + 2), np.int32)
    for y in range(h):
        for x in range(w):
            if img[y, x] == 0:
                continue
            for n in range(numangle):
                a = F32(F32(x) * F32(tab_cos[n]))
                b = F32(F32(y) * F32(tab_sin[n]))
                r = int(np.rint(F32(a + b))) + (numrho - 1) // 2
                if 0 <= r < numrho:
                    acc[(n + 1) * (numrho + 2) + r + 1] += 1
    return acc.reshape(numangle + 2, numrho + 2)


def peaks_ref(acc, threshold):
    """flat indices b (into the accumulator with its ring) of the peaks, ascending"""
    a = acc.astype(np.int64)
    c = a[1:-1, 1:-1]
    peak = (c > threshold) & (c > a[1:-1, :-2]) & (c >= a[1:-1, 2:]) & (c > a[:-2, 1:-1]) & (c >= a[2:, 1:-1])
    n, r = np.nonzero(peak)
    return (n + 1) * acc.shape[1] + r + 1


def peaks_literal(acc, threshold):
    numangle, numrho = acc.shape[0] - 2, acc.shape[1] - 2
    a = [int(v) for v in acc.ravel()]
    out = []
    for n in range(numangle):
        for r in range(numrho):
            b = (n + 1) * (numrho + 2) + r + 1
            if (a[b] > threshold and a[b] > a[b - 1] and a[b] >= a[b + 1] and a[b] > a[b - numrho - 2]
                    and a[b] >= a[b + numrho + 2]):
                out.append(b)
    return np.array(out, np.int64)


def lines_ref(acc, threshold, max_lines, rho, theta, min_theta=0.0):
    """(lines (max_lines, 2) float32, votes (max_lines,) int32, count) of one accumulator: peaks by votes descending, then
    cell index ascending; rows past min(count, max_lines) are zero"""
    numrho = acc.shape[1] - 2
    b = peaks_ref(acc, threshold)
    v = acc.ravel()[b].astype(np.int64)
    order = np.lexsort((b, -v))[:max_lines]
    b, v = b[order], v[order]
    n, r = b // (numrho + 2) - 1, b % (numrho + 2) - 1
    lines = np.zeros((max_lines, 2), F32)
    votes = np.zeros(max_lines, np.int32)
    centre = F32(F32(numrho - 1) * F32(0.5))
    lines[:len(b), 0] = (r.astype(F32) - centre) * F32(rho)
    lines[:len(b), 1] = F32(min_theta) + n.astype(F32) * F32(theta)
    votes[:len(b)] = v
    return lines, votes, len(peaks_ref(acc, threshold))


def hough_ref(frames, tab_cos, tab_sin, numrho, threshold, max_lines, rho, theta, min_theta=0.0):
    """(accum (n, numangle + 2, numrho + 2), lines (n, max_lines, 2), votes (n, max_lines), count (n,)) of (n, h, w) frames"""
    frames = frames[None] if frames.ndim == 2 else frames
    acc = np.stack([accum_ref(f, tab_cos, tab_sin, numrho) for f in frames])
    out = [lines_ref(a, threshold, max_lines, rho, theta, min_theta) for a in acc]
    return (acc, np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32))


def ulp_distance(a, b):
    """|a - b| in units of the last place of float32 arrays (sign-magnitude bit patterns mapped onto a line)"""
    def key(x):
        u = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))
