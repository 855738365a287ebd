"""The oracle against the reference's OWN PUBLISHED OUTPUTS.  No GPU.

The reference ships no golden images, but its three benchmark applications wrote, for each of its eight test images,
`Error_MAE` = mean |CPU path - OpenCL path| (src/*/results/Linux_100_*_sorted_results.csv; committed here as
tests/golden/published_mae.json, 6 significant digits as the applications printed them).  Both operands are restated
here — the CPU path in oracle/imgfilter_oracle.c (what the product is checked against), the OpenCL buffer-mode kernels in
oracle/opencl_path.py — and run on the decoded pixels of the reference's images (tests/golden/ref_images; the two
largest, which are not stored decoded, are decoded live from the JPEG files committed in tests/golden/ref_jpeg):

  grayscale   8 of 8 published numbers reproduced to the last printed digit (1, 12, 135, 299, 401, 3162, 21824, 36137
              differing pixels); on the near-gray Artemis photographs 5-8 % of the pixels sit on the r = g = b colours
              where the reference's double-precision formula truncates one below the integer formula, so those four
              numbers pin exactly the 3,464-colour exception set the product's fast luminance has to honour
  Gaussian    8 of 8 (0, 0, 0, 2, 1, 2, 11, 42 differing blue-channel bytes)
  Sobel       Linux run (buffer kernel): 4 of 8 to the last digit, the other four inside the bracket spanned by a
              correctly rounded and a 1-ulp-high device sqrt (the OpenCL side's magnitude * 255 lands on exact integers
              wherever the gradient has one direction only, so the unknown device's sqrt rounding decides those pixels;
              the CPU side — what the oracle restates: decoder luma, filter2D as correlation with BORDER_REFLECT_101,
              magnitude, round-to-nearest + saturate — has no such freedom).  Windows run (image2d kernel, no luminance
              arithmetic on the OpenCL side): 5 of 8 to the last digit, all 8 within 2e-5 relative
and the negative controls show that the comparison discriminates: plausible misreadings of the CPU path (integer
luminance, REPLICATE / REFLECT borders, truncation, luma recomputed from RGB) miss the published numbers.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import sys
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import opencl_path as CL  # noqa: E402  (test infrastructure, like oracle.py)

REF_JPEG = os.path.join(GOLDEN, "ref_jpeg")  # the reference's images/*.jpg, byte for byte
NAMES = ["Tulips_square75", "Tulips_small240", "Tulips_medium640", "Tulips_large1024",
         "Artemis_square75", "Artemis_small240", "Artemis_medium640", "Artemis_large1024"]
PUBLISHED = json.load(open(os.path.join(GOLDEN, "published_mae.json")))


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _committed(name):
    rgb = os.path.join(GOLDEN, "tulips_medium640_rgb.png") if name == "Tulips_medium640" else \
        os.path.join(GOLDEN, "ref_images", name + "_rgb.png")
    y = os.path.join(GOLDEN, "ref_images", name + "_y.png")
    if os.path.exists(rgb) and os.path.exists(y):
        from PIL import Image
        return np.asarray(Image.open(rgb).convert("RGB")), _png(y)
    return None


def _live(name):
    path = os.path.join(REF_JPEG, name + ".jpg")
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert("RGB"))
    im = Image.open(path)
    im.draft("L", im.size)
    return rgb, np.asarray(im)


@pytest.fixture(scope="module")
def images():
    return {n: _committed(n) or _live(n) for n in NAMES}


def rgba_of(rgb):
    return np.ascontiguousarray(np.dstack([rgb, np.full(rgb.shape[:2], 255, np.uint8)]))


def printed(x):
    """The value as the applications' `file << mae` printed it: 6 significant digits."""
    return float("%.6g" % x)


def published(app, name, osname="Linux"):
    return float(PUBLISHED[app][osname][name]["Error_MAE"])


def mae(a, b):
    """cv::mean(cv::absdiff(a, b))[0] — OpenCV multiplies the sum by the reciprocal of the element count, which decides
    the last printed digit when the quotient is a decimal tie (3162 / 38400 = 0.08234375)."""
    return float(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum()) * (1.0 / a.size)


def test_committed_pixels_are_the_reference_images(images):
    """The committed PNGs are exactly what the reference's JPEGs (tests/golden/ref_jpeg) decode to."""
    for n in NAMES:
        c, lv = _committed(n), _live(n)
        if c is not None:
            assert np.array_equal(c[0], lv[0]) and np.array_equal(c[1], lv[1]), n
        res = PUBLISHED["gray"]["Linux"][n]["resolution"]
        assert res == "%dx%d" % (lv[0].shape[1], lv[0].shape[0])


# ---- grayscale -------------------------------------------------------------------------------------------------
def test_gray_reproduces_every_published_number(oracle, images):
    """grayscale.cpp:437: ComputeMAE(cpu 1-channel, OpenCL (g,g,g,255)); cv::cvtColor(RGBA2GRAY) of a gray pixel is
    the identity (fixed-point weights sum to 2^14), so the comparison is byte against byte."""
    for n, (rgb, _) in images.items():
        cpu = oracle.gray_bgr(np.ascontiguousarray(rgb[..., ::-1]))  # cv::imread hands the CPU loop BGR
        ocl = CL.cl_gray(rgba_of(rgb))
        assert printed(mae(cpu, ocl)) == published("gray", n), (n, mae(cpu, ocl) * cpu.size)
        # the same pixels through the RGBA entry points of the oracle (what the GPU tests compare against)
        assert np.array_equal(cpu, oracle.gray_rgba_1ch(rgba_of(rgb)))


def test_gray_device_identification_is_unique(oracle, images):
    """Of the contraction patterns x division forms an OpenCL compiler may pick, exactly one reproduces all published
    numbers — so the agreement above is not one of many lucky combinations."""
    hits = []
    for contraction in ("none", "published", "fma_chain", "fma_last", "fma_first"):
        for division in ("rcp", "ieee"):
            ok = all(printed(mae(oracle.gray_bgr(np.ascontiguousarray(rgb[..., ::-1])),
                                 CL.cl_gray(rgba_of(rgb), contraction, division))) == published("gray", n)
                     for n, (rgb, _) in images.items())
            if ok:
                hits.append((contraction, division))
    assert hits == [("published", "rcp")]


def test_gray_windows_numbers_are_the_image2d_path(oracle, images):
    """The reference's WINDOWS grayscale run went through grayscale_images.cl (normalised texels, R/FLOAT output,
    ConvertToUChar): CPU path against oracle_image2d_gray reproduces all 8 numbers of
    src/Grayscale/results/Windows_100_*_sorted_results.csv to the last digit (2, 11, 159, 363, 401, 3162, 21818, 36127
    differing pixels) — with the same contraction of the luminance expression as the Linux device chose, and with none
    other (the uncontracted form gives 1, 14, 172, 392, ...).  A second set of eight published numbers behind
    oracle_gray_*, and the pin of oracle_image2d_gray / the product's image2d grayscale."""
    for n, (rgb, _) in images.items():
        cpu = oracle.gray_bgr(np.ascontiguousarray(rgb[..., ::-1]))
        img = oracle.image2d_gray(rgba_of(rgb)).reshape(cpu.shape)
        assert printed(mae(cpu, img)) == published("gray", n, "Windows"), (n, (cpu != img).sum())
    # the uncontracted form is rejected
    rgb = images["Tulips_medium640"][0]
    x, y, z = (rgb[..., i].astype(np.float32) / np.float32(255.0) for i in range(3))
    plain = ((np.float32(0.299) * x + np.float32(0.587) * y) + np.float32(0.114) * z) * np.float32(255.0)
    cpu = oracle.gray_bgr(np.ascontiguousarray(rgb[..., ::-1]))
    assert printed(mae(cpu, plain.astype(np.uint8))) != published("gray", "Tulips_medium640", "Windows")


def test_gray_negative_controls(oracle, images):
    """Misreadings of the CPU path (grayscale.cpp:237) that the published numbers reject."""
    miss_int = miss_f32 = 0
    for n, (rgb, _) in images.items():
        r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
        ocl = CL.cl_gray(rgba_of(rgb))
        as_int = ((299 * r + 587 * g + 114 * b) // 1000).astype(np.uint8)  # "the same formula in integers"
        as_f32 = (np.float32(0.299) * r.astype(np.float32) + np.float32(0.587) * g.astype(np.float32)
                  + np.float32(0.114) * b.astype(np.float32)).astype(np.uint8)  # float instead of double
        miss_int += printed(mae(as_int, ocl)) != published("gray", n)
        miss_f32 += printed(mae(as_f32, ocl)) != published("gray", n)
    assert miss_int >= len(images) - 1 and miss_f32 >= len(images) - 1
    # and the size of the effect: on the gray photograph the integer formula changes thousands of pixels
    rgb = images["Artemis_medium640"][0]
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    as_int = ((299 * r + 587 * g + 114 * b) // 1000).astype(np.uint8)
    cpu = oracle.gray_bgr(np.ascontiguousarray(rgb[..., ::-1]))
    assert (as_int != cpu).sum() > 10000


# ---- Gaussian --------------------------------------------------------------------------------------------------
def test_gauss_reproduces_every_published_number(oracle, images):
    """GaussianBlur.cpp:405-418: both images go RGBA -> BGR and ComputeMAE returns cv::mean(...)[0], the BLUE plane;
    k = 5, sigma = 1.5 (GaussianBlur.cpp:15-16).  The table's float sum is exactly 1.0f, so `sum /= total_weight` is the
    identity and the only freedom of the OpenCL side is fma contraction."""
    wt = oracle.gauss_weights(5, 1.5)
    assert np.float32(np.cumsum(wt.reshape(-1), dtype=np.float32)[-1]) == np.float32(1.0)
    for n, (rgb, _) in images.items():
        rgba = rgba_of(rgb)
        cpu = oracle.gauss_rgba(rgba, 5, 1.5, threads=oracle.max_threads())
        ocl = CL.cl_gauss(rgba, 5, wt)
        assert printed(mae(cpu[..., 2], ocl[..., 2])) == published("gauss", n), (n, (cpu[..., 2] != ocl[..., 2]).sum())
        assert int(np.abs(cpu.astype(int) - ocl.astype(int)).max()) <= 1


def test_gauss_controls(oracle, images):
    """(a) the numpy restatement WITHOUT fma is the CPU algorithm (GaussianBlur.cpp:243-256) and equals the C oracle bit
    for bit; (b) so without contraction every published number would be 0 — five of them are not; (c) a CPU path that
    fused its multiply-adds, or that did not truncate, misses them."""
    wt = oracle.gauss_weights(5, 1.5)
    nonzero = 0
    for n in ("Tulips_square75", "Artemis_square75", "Artemis_small240", "Tulips_small240"):
        rgba = rgba_of(images[n][0])
        cpu = oracle.gauss_rgba(rgba, 5, 1.5)
        assert np.array_equal(cpu, CL.cl_gauss(rgba, 5, wt, fma=False)), n
        nonzero += published("gauss", n) != 0.0
    assert nonzero == 2
    rgba = rgba_of(images["Artemis_medium640"][0])
    cpu = oracle.gauss_rgba(rgba, 5, 1.5, threads=oracle.max_threads())
    ocl = CL.cl_gauss(rgba, 5, wt)
    assert printed(mae(cpu[..., 2], ocl[..., 2])) == published("gauss", "Artemis_medium640") != 0.0
    assert printed(mae(ocl[..., 2], ocl[..., 2])) != published("gauss", "Artemis_medium640")  # (c) fused CPU path


# ---- Sobel -----------------------------------------------------------------------------------------------------
def _sobel_np(gray, pad_mode, rounding="nearest"):
    """numpy twin of the CPU Sobel (EdgeDetection.cpp:219-240) with a selectable border rule / rounding."""
    p = np.pad(gray.astype(np.int64), 1, mode=pad_mode)
    h, w = gray.shape
    win = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]  # noqa: E731
    gx = (win(-1, 1) + 2 * win(0, 1) + win(1, 1)) - (win(-1, -1) + 2 * win(0, -1) + win(1, -1))
    gy = (win(1, -1) + 2 * win(1, 0) + win(1, 1)) - (win(-1, -1) + 2 * win(-1, 0) + win(-1, 1))
    m = np.sqrt((gx * gx + gy * gy).astype(np.float32))
    m = np.rint(m) if rounding == "nearest" else np.floor(m)
    return np.clip(m, 0, 255).astype(np.uint8)


def test_sobel_published_numbers(oracle, images):
    """EdgeDetection.cpp:396: CPU = OpenCV Sobel of imread(IMREAD_GRAYSCALE); OpenCL = edge_base.cl on the RGBA
    pixels, border never written.  4 numbers to the last digit, all 8 inside the device-sqrt bracket."""
    exact = 0
    for n, (rgb, y) in images.items():
        cpu = oracle.sobel_gray(np.ascontiguousarray(y))
        assert np.array_equal(cpu, _sobel_np(y, "reflect")), n  # numpy 'reflect' = BORDER_REFLECT_101
        hi = mae(cpu, CL.cl_sobel(rgba_of(rgb)))              # correctly rounded sqrt
        lo = mae(cpu, CL.cl_sobel(rgba_of(rgb), sqrt_ulps=1))  # a sqrt one ulp high
        pub = published("sobel", n)
        exact += printed(hi) == pub
        assert printed(lo) - 1e-9 <= pub <= printed(hi) + 1e-9, (n, lo, pub, hi)
        assert (hi - lo) / pub < 0.02  # the bracket is narrow: < 2 % of the number it brackets
    assert exact >= (4 if len(images) == 8 else 4)


def test_sobel_windows_numbers_are_the_image2d_path(oracle, images):
    """The reference's WINDOWS EdgeDetection run (src/EdgeDetection/results/Windows_100_*_sorted_results.csv, MAE 8-48)
    went through the image2d_t kernel (edge_images.cl: red channel, no luminance): the CPU Sobel against the image-mode
    restatement reproduces 5 of its 8 numbers to the last digit and all 8 inside the bracket of a correctly rounded / a
    1-ulp-low device sqrt.  A second, independent tie of oracle_sobel_gray to the OpenCV build the author ran — with no
    luminance arithmetic on the OpenCL side at all — and the pin of oracle_image2d_sobel."""
    exact = 0
    for n, (rgb, y) in images.items():
        rgba = rgba_of(rgb)
        cpu = oracle.sobel_gray(np.ascontiguousarray(y))
        img0 = CL.cl_sobel_image2d(rgba)
        assert np.array_equal(img0, oracle.image2d_sobel(rgba).reshape(img0.shape)), n
        a, b = mae(cpu, img0), mae(cpu, CL.cl_sobel_image2d(rgba, sqrt_ulps=-1))
        pub = published("sobel", n, "Windows")
        exact += printed(a) == pub
        lo, hi = sorted((printed(a), printed(b)))
        assert lo - 1e-9 <= pub <= hi + 1e-9, (n, a, pub, b)
        assert abs(a - pub) / pub < 2e-5, n  # the correctly rounded form alone is within 2e-5 of every number
    assert exact >= (5 if len(images) == 8 else 3)


def test_sobel_negative_controls(oracle, images):
    """CPU-side misreadings fall OUTSIDE the bracket on every image: other border rules, truncation instead of
    rounding, luminance recomputed from RGB instead of the decoder's luma plane."""
    for n, (rgb, y) in images.items():
        rgba = rgba_of(rgb)
        hi_img, lo_img = CL.cl_sobel(rgba), CL.cl_sobel(rgba, sqrt_ulps=1)
        pub = published("sobel", n)

        def outside(cpu):
            lo, hi = sorted((mae(cpu, lo_img), mae(cpu, hi_img)))
            return not (printed(lo) - 1e-9 <= pub <= printed(hi) + 1e-9)
        assert outside(_sobel_np(y, "edge")), n       # BORDER_REPLICATE
        assert outside(_sobel_np(y, "symmetric")), n  # BORDER_REFLECT
        assert outside(_sobel_np(y, "constant")), n   # zero border
        assert outside(_sobel_np(y, "reflect", rounding="floor")), n
        assert outside(oracle.sobel_rgba(rgba)), n    # luma from RGB (the product's RGBA entry point: a3 then a10)
