"""CPU reference of the whole-frame statistics of single-channel frames (MI355_FILTER_EQUALIZE_GRAY8 / OTSU_GRAY8).

A restatement of include/mi355_imgfilter.h, which follows OpenCV's plain C++ path: cv::calcHist, cv::equalizeHist and
cv::threshold(src, dst, 0, 255, THRESH_BINARY | THRESH_OTSU).  Every arithmetic step is a numpy float32 or a Python
float (IEEE binary64) scalar operation in the written order, so the results are the bits OpenCV computes.  A plain
numpy helper for the histogram tests, not a fixture module.  Frames are (h, w) or (n, h, w) uint8; every frame is its
own image.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)  # 2^-23


def _frames(y):
    y = np.asarray(y, np.uint8)
    return y[None] if y.ndim == 2 else y


def hist_ref(y):
    """(n, 256) uint32 bin counts, (256,) for one (h, w) frame."""
    f = _frames(y)
    out = np.stack([np.bincount(fr.ravel(), minlength=256) for fr in f]).astype(np.uint32)
    return out[0] if np.asarray(y).ndim == 2 else out


def equalize_lut(hist):
    """cv::equalizeHist's table of one frame's histogram (bins below the first occupied one map to 0: no pixel has
    them)."""
    hist = [int(v) for v in hist]
    total = sum(hist)
    i0 = next(i for i in range(256) if hist[i])
    if hist[i0] == total:
        return np.full(256, i0, np.uint8)
    scale = np.float32(255.0) / np.float32(total - hist[i0])
    lut = np.zeros(256, np.uint8)
    s = 0
    for i in range(i0 + 1, 256):
        s += hist[i]
        v = np.rint(np.float32(s) * scale)  # float32 product, round half to even (cvRound)
        lut[i] = min(255, int(v))
    return lut


def otsu_threshold(hist):
    """OpenCV's getThreshVal_Otsu_8u: the fp64 loop, operation by operation."""
    hist = [int(v) for v in hist]
    total = sum(hist)
    scale = 1.0 / float(total)
    mu = 0.0
    for i in range(256):
        mu += i * float(hist[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    t = 0
    for i in range(256):
        p = hist[i] * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma = sigma
            t = i
    return t


def otsu_thresholds_ref(y):
    """(n,) int32 thresholds, a 0-d array for one (h, w) frame."""
    t = np.array([otsu_threshold(h) for h in np.atleast_2d(hist_ref(y))], np.int32)
    return t[0] if np.asarray(y).ndim == 2 else t


def equalize_ref(y):
    f = _frames(y)
    out = np.stack([equalize_lut(h)[fr] for h, fr in zip(np.atleast_2d(hist_ref(f)), f)])
    return out[0] if np.asarray(y).ndim == 2 else out


def otsu_ref(y):
    f = _frames(y)
    out = np.stack([np.where(fr > t, 255, 0).astype(np.uint8) for t, fr in zip(np.atleast_1d(otsu_thresholds_ref(f)), f)])
    return out[0] if np.asarray(y).ndim == 2 else out
