"""ctypes binding of include/mi355_imgfilter.h.

Mirrors, for Python hosts, what host/Controller.cpp does for C++ hosts: the three Perform* calls of
the reference `Controller` (include/Controller.hpp:37-47 in the reference) plus the fused pipeline,
in a host-buffer form (numpy in / numpy out, with the six profiling timestamps) and a
device-resident form (raw device pointers, e.g. torch tensors' data_ptr()).

There is no fallback: if the shared library is missing or cannot be loaded this module raises.
"""
import ctypes
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "lib", "libmi355_imgfilter.so")
_HEADER = os.path.join(_ROOT, "include", "mi355_imgfilter.h")

FILTER_GRAY, FILTER_GRAY1, FILTER_GAUSS, FILTER_SOBEL, FILTER_PIPELINE = 0, 1, 2, 3, 4
# single-channel filters: 1 byte per pixel in and out (include/mi355_imgfilter.h, MI355_FILTER_*_GRAY8)
FILTER_GAUSS_GRAY8, FILTER_SOBEL_GRAY8, FILTER_PIPELINE_GRAY8 = 5, 6, 7
# median filter (MI355_FILTER_MEDIAN*): ids 16 and 17, k in {3, 5, 7}, sigma ignored
FILTER_MEDIAN, FILTER_MEDIAN_GRAY8 = 16, 17
MAX_MEDIAN_K = 7
# rectangular morphology (MI355_FILTER_ERODE ... CLOSE_GRAY8): ids 24-31 (18-23 unassigned), odd 3 <= k <= MAX_MORPH_K, sigma ignored
FILTER_ERODE, FILTER_DILATE, FILTER_OPEN, FILTER_CLOSE = 24, 25, 26, 27
FILTER_ERODE_GRAY8, FILTER_DILATE_GRAY8, FILTER_OPEN_GRAY8, FILTER_CLOSE_GRAY8 = 28, 29, 30, 31
MAX_MORPH_K = 17
# whole-frame statistics (MI355_FILTER_EQUALIZE_GRAY8 / OTSU_GRAY8): ids 40 and 41 (32-39 unassigned), k and sigma ignored
FILTER_EQUALIZE_GRAY8, FILTER_OTSU_GRAY8 = 40, 41
# box mean, cv::blur with BORDER_REPLICATE (MI355_FILTER_BOX*): ids 48 and 49 (42-47 unassigned), odd 3 <= k <= MAX_BOX_K,
# sigma ignored
FILTER_BOX, FILTER_BOX_GRAY8 = 48, 49
MAX_BOX_K = 63
# cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) types (mi355_adaptive_threshold_*): cv::THRESH_BINARY / THRESH_BINARY_INV
ADAPTIVE_BINARY, ADAPTIVE_BINARY_INV = 0, 1
# CLAHE (mi355_clahe_*): 1 <= tiles_x, tiles_y <= MAX_CLAHE_TILES
MAX_CLAHE_TILES = 16
# connected components (mi355_ccl_*): connectivity 4 or 8, 0 <= stats_rows <= MAX_CCL_STATS_ROWS
MAX_CCL_STATS_ROWS = 1 << 24
# cv::distanceTransform (mi355_dist_*): sides of 1 .. MAX_DIST_DIM; DIST_NONE is the squared distance of a frame without
# a zero pixel
MAX_DIST_DIM = 16384
DIST_NONE = 2147483647
# cv::Canny (mi355_canny_*): flags = 0 or CANNY_L2GRADIENT (magnitude dx^2 + dy^2 instead of |dx| + |dy|)
CANNY_L2GRADIENT = 1
# cv::HoughLines (mi355_hough_*): at most MAX_HOUGH_ANGLES angle rows and 1 .. MAX_HOUGH_LINES lines per frame
MAX_HOUGH_ANGLES = 1024
MAX_HOUGH_LINES = 4096
# cv::resize (mi355_resize_*): OpenCV's enum values; AREA only with integer factors 1 .. MAX_AREA_FACTOR
INTERP_NEAREST, INTERP_LINEAR, INTERP_AREA = 0, 1, 3
MAX_AREA_FACTOR = 16
# cv::warpAffine (mi355_warp_affine_*): flags = INTERP_NEAREST or INTERP_LINEAR, optionally | WARP_INVERSE_MAP
WARP_INVERSE_MAP = 16
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1
MAX_WARP_SIZE = 32766
# cv::remap (mi355_remap_*): FIXED = int16 (sx, sy) pairs + uint16 fy*32+fx (cv::convertMaps), FLOAT = float x and y planes
MAP_FIXED, MAP_FLOAT = 0, 1
# YUV frames (mi355_yuv_*): the layouts (YUY2 and UYVY decode only) and the conversion standards
YUV_NV12, YUV_NV21, YUV_I420, YUV_YV12, YUV_YUY2, YUV_UYVY = 0, 1, 2, 3, 4, 5
YUV_BT601, YUV_BT709, YUV_BT601_FULL = 0, 1, 2
GAUSS_FAST, GAUSS_EXACT = 0, 1
INPUT_RGBA, INPUT_BGR = 0, 1
IMPL_AUTO, IMPL_TILE, IMPL_MFMA, IMPL_VALU = 0, 1, 2, 3
OUT_BPP = {FILTER_GRAY: 4, FILTER_GRAY1: 1, FILTER_GAUSS: 4, FILTER_SOBEL: 1, FILTER_PIPELINE: 1,
           FILTER_GAUSS_GRAY8: 1, FILTER_SOBEL_GRAY8: 1, FILTER_PIPELINE_GRAY8: 1}
IN_BPP = {FILTER_GRAY: 4, FILTER_GRAY1: 4, FILTER_GAUSS: 4, FILTER_SOBEL: 4, FILTER_PIPELINE: 4,
          FILTER_GAUSS_GRAY8: 1, FILTER_SOBEL_GRAY8: 1, FILTER_PIPELINE_GRAY8: 1}


def _in_bpp(filt):
    """Bytes per input pixel of any filter id (None for an unknown id, which the library then rejects)."""
    n = load_library().mi355_filter_in_bpp(int(filt))
    return n if n > 0 else None


def _out_bpp(filt):
    n = load_library().mi355_filter_out_bpp(int(filt))
    return n if n > 0 else None


_u8p = ctypes.POINTER(ctypes.c_uint8)
_f32p = ctypes.POINTER(ctypes.c_float)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_ci = ctypes.c_int
_cd = ctypes.c_double
_f64p = ctypes.POINTER(ctypes.c_double)


class Mi355Error(RuntimeError):
    def __init__(self, fn, code, detail=""):
        self.fn, self.code = fn, code
        super().__init__("%s failed: %d (%s)%s" % (fn, code, detail, ""))


def library_path():
    return _LIB


def build_library(jobs=8):
    """Compile csrc/*.hip for gfx950 into lib/libmi355_imgfilter.so (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", os.path.join(_HERE, "csrc"), "all", "tune"], check=True)
    return _LIB


def declared_symbols():
    """Every function name include/mi355_imgfilter.h declares."""
    text = open(_HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi355_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load_library(path=None):
    """The product library (cached).  `path`: another build of the same library, bound the same way and NOT cached —
    several builds can live in one process (tools/abx.py: same-process A/B timing on the same buffers)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    other = path is not None
    # MI355_IMGFILTER_LIB: another build of the same library (A/B timing of kernel changes, tools/abx.py)
    path = path or os.environ.get("MI355_IMGFILTER_LIB", _LIB)
    if not os.path.exists(path):
        raise Mi355Error("load_library", -1, "%s is missing: run __graft_entry__.build()" % path)
    lib = ctypes.CDLL(path)
    sig = {
        "mi355_device_count": [ctypes.POINTER(_ci)],
        "mi355_ctx_create": [_ci, ctypes.POINTER(_vp)],
        "mi355_ctx_create_on_stream": [_ci, _vp, ctypes.POINTER(_vp)],
        "mi355_ctx_destroy": [_vp],
        "mi355_ctx_device_name": [_vp, ctypes.c_char_p, ctypes.c_size_t],
        "mi355_sync": [_vp],
        "mi355_last_hip_error": [_vp],
        "mi355_ctx_set_gauss_mode": [_vp, _ci],
        "mi355_ctx_set_input_format": [_vp, _ci],
        "mi355_bgr_to_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_ctx_set_impl": [_vp, _ci],
        "mi355_gauss_weights": [_ci, ctypes.c_float, _f32p],
        "mi355_ctx_set_gauss_weights": [_vp, _ci, ctypes.c_float, _f32p],
        "mi355_gauss_weights_image2d": [_ci, ctypes.c_float, _f32p],
        "mi355_image2d_rgba8": [_vp, _ci, _u8p, _u8p, _ci, _ci, _ci, ctypes.c_float, _u64p],
        "mi355_gray_rgba8": [_vp, _u8p, _u8p, _ci, _ci, _u64p],
        "mi355_gray1_rgba8": [_vp, _u8p, _u8p, _ci, _ci, _u64p],
        "mi355_gauss_rgba8": [_vp, _u8p, _u8p, _ci, _ci, _ci, ctypes.c_float, _u64p],
        "mi355_sobel_rgba8": [_vp, _u8p, _u8p, _ci, _ci, _u64p],
        "mi355_pipeline_rgba8": [_vp, _u8p, _u8p, _ci, _ci, _ci, ctypes.c_float, _u64p],
        "mi355_filter_batched": [_vp, _ci, _u8p, _u8p, _ci, _ci, _ci, _ci, ctypes.c_float, _u64p],
        "mi355_filter_out_bpp": [_ci],
        "mi355_filter_in_bpp": [_ci],
        "mi355_filter_stream": [_vp, _ci, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, ctypes.c_float,
                                ctypes.POINTER(ctypes.c_double)],
        "mi355_host_alloc": [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)],
        "mi355_host_free": [_vp, _vp],
        "mi355_gray_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_gray1_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_gauss_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, ctypes.c_float],
        "mi355_sobel_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_pipeline_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, ctypes.c_float],
        "mi355_filter_dev": [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, ctypes.c_float],
        "mi355_hist_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_otsu_thresholds_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_resize_check": [_ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_resize_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_resize_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _u64p],
        "mi355_rotation_matrix": [_cd, _cd, _cd, _cd, _f64p],
        "mi355_warp_affine_matrix": [_f64p, _ci, _f64p],
        "mi355_warp_affine_check": [_ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci],
        "mi355_warp_affine_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci, ctypes.c_uint32],
        "mi355_warp_affine_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci, ctypes.c_uint32,
                                      _u64p],
        "mi355_remap_check": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_remap_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, ctypes.c_uint32],
        "mi355_remap_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, ctypes.c_uint32,
                                _u64p],
        "mi355_perspective_matrix": [_f64p, _ci, _f64p],
        "mi355_warp_perspective_check": [_ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci],
        "mi355_warp_perspective_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci, ctypes.c_uint32],
        "mi355_warp_perspective_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _f64p, _ci, _ci,
                                           ctypes.c_uint32, _u64p],
        "mi355_adaptive_threshold_check": [_ci, _ci, _ci, _ci, _ci, _ci, ctypes.c_double],
        "mi355_adaptive_threshold_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, ctypes.c_double],
        "mi355_adaptive_threshold_gray8_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, ctypes.c_double,
                                                   _u64p],
        "mi355_clahe_check": [_ci, _ci, _ci, ctypes.c_double, _ci, _ci],
        "mi355_clahe_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, ctypes.c_double, _ci, _ci],
        "mi355_clahe_gray8_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, ctypes.c_double, _ci, _ci, _u64p],
        "mi355_clahe_luts_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, ctypes.c_double, _ci, _ci],
        "mi355_ccl_check": [_ci, _ci, _ci, _ci, _ci],
        "mi355_ccl_gray8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci],
        "mi355_ccl_gray8_batched": [_vp, _u8p, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _u64p],
        "mi355_dist_check": [_ci, _ci, _ci],
        "mi355_dist_gray8_dev": [_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci],
        "mi355_dist_gray8_batched": [_vp, _u8p, _vp, _vp, _vp, _ci, _ci, _ci, _u64p],
        "mi355_hysteresis_check": [_ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_hysteresis_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_hysteresis_gray8_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _u64p],
        "mi355_canny_check": [_ci, _ci, _ci, _cd, _cd, _ci],
        "mi355_canny_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _ci],
        "mi355_canny_gray8_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _cd, _cd, _ci, _u64p],
        "mi355_hough_check": [_ci, _ci, _ci, _cd, _cd, _ci, _ci, _cd, _cd],
        "mi355_hough_shape": [_ci, _ci, _cd, _cd, _cd, _cd, ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
        "mi355_hough_trig_table": [_ci, _ci, _cd, _cd, _cd, _cd, _f32p, _f32p],
        "mi355_hough_plan": [_ci, _ci, _cd, _cd, _cd, _cd, ctypes.POINTER(_ci), ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
        "mi355_hough_accum_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _cd, _cd],
        "mi355_hough_lines_gray8_dev": [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _ci, _ci, _cd, _cd],
        "mi355_hough_lines_gray8_batched": [_vp, _u8p, _vp, _vp, _vp, _ci, _ci, _ci, _cd, _cd, _ci, _ci, _cd, _cd, _u64p],
        "mi355_yuv_check": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_yuv_to_rgba8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_rgba8_to_yuv_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_yuv_to_gray8_dev": [_vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci],
        "mi355_yuv_to_rgba8_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _u64p],
        "mi355_rgba8_to_yuv_batched": [_vp, _u8p, _u8p, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _u64p],
        "mi355_synth_rgba8_dev": [_vp, _vp, _ci, _ci, _ci, _ci, ctypes.c_uint32, _ci],
        "mi355_checksum_dev": [_vp, _vp, ctypes.c_size_t, ctypes.c_uint64, _u64p],
        "mi355_stream_copy_dev": [_vp, _vp, _vp, ctypes.c_size_t],
        "mi355_selftest": [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)],
        "mi355_dev_alloc": [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)],
        "mi355_pool_alloc": [_vp, _ci, _ci, _ci, _ci, _ci, ctypes.c_float, _ci, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                             _f32p],
        "mi355_pool_free": [_vp, _vp, _vp],
        "mi355_dev_free": [_vp, _vp],
        "mi355_copy_h2d": [_vp, _vp, _vp, ctypes.c_size_t],
        "mi355_copy_d2h": [_vp, _vp, _vp, ctypes.c_size_t],
        "mi355_group_create": [_ci, ctypes.POINTER(_ci), ctypes.POINTER(_vp)],
        "mi355_group_destroy": [_vp],
        "mi355_group_size": [_vp, ctypes.POINTER(_ci)],
        "mi355_group_member_ctx": [_vp, _ci, ctypes.POINTER(_vp)],
        "mi355_group_member_status": [_vp, _ci],
        "mi355_group_shard": [_ci, _ci, _ci, ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
        "mi355_group_set_gauss_mode": [_vp, _ci],
        "mi355_group_set_impl": [_vp, _ci],
        "mi355_group_set_input_format": [_vp, _ci],
        "mi355_group_set_gauss_weights": [_vp, _ci, ctypes.c_float, _f32p],
        "mi355_group_filter_batched": [_vp, _ci, _u8p, _u8p, _ci, _ci, _ci, _ci, ctypes.c_float,
                                       ctypes.POINTER(ctypes.c_double)],
        "mi355_group_filter_dev": [_vp, _ci, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _ci, _ci, ctypes.POINTER(_ci), _ci,
                                   ctypes.c_float],
        "mi355_timer_begin": [_vp],
        "mi355_timer_end": [_vp, _f32p],
    }
    for name, args in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if path == _LIB:
                raise
            continue  # an older build under MI355_IMGFILTER_LIB
        fn.argtypes = args
        fn.restype = _ci
    if hasattr(lib, "mi355_yuv_frame_bytes") or path == _LIB:
        lib.mi355_yuv_frame_bytes.argtypes = [_ci, _ci, _ci, _ci, _ci]
        lib.mi355_yuv_frame_bytes.restype = ctypes.c_size_t
    if hasattr(lib, "mi355_hough_accum_bytes") or path == _LIB:
        lib.mi355_hough_accum_bytes.argtypes = [_ci, _ci, _ci, _cd, _cd, _cd, _cd]
        lib.mi355_hough_accum_bytes.restype = ctypes.c_size_t
    lib.mi355_strerror.argtypes = [_ci]
    lib.mi355_strerror.restype = ctypes.c_char_p
    lib.mi355_build_info.argtypes = []
    lib.mi355_build_info.restype = ctypes.c_char_p
    if not other:
        _lib = lib
    return lib


def _check(fn, rc, ctx=None):
    if rc != 0:
        lib = load_library()
        detail = lib.mi355_strerror(rc).decode()
        if ctx is not None and rc == -2:
            detail += ", hipError=%d" % lib.mi355_last_hip_error(ctx)
        raise Mi355Error(fn, rc, detail)


def gauss_weights(k, sigma):
    """Host coefficient table — replaces Controller::_GenerateGaussianKernelBuffers."""
    out = np.empty((k, k), np.float32) if k > 0 else np.empty((1, 1), np.float32)
    rc = load_library().mi355_gauss_weights(int(k), float(sigma), out.ctypes.data_as(_f32p))
    _check("mi355_gauss_weights", rc)
    return out


def gauss_weights_image2d(k, sigma):
    """The image-mode table — replaces Controller::_GenerateGaussianKernelImage2D (last row / column zero)."""
    out = np.empty((k, k), np.float32) if k > 0 else np.empty((1, 1), np.float32)
    rc = load_library().mi355_gauss_weights_image2d(int(k), float(sigma), out.ctypes.data_as(_f32p))
    _check("mi355_gauss_weights_image2d", rc)
    return out


def _batch_shape(filt, frames, in_ch):
    """(n, h, w) of a host batch: (n, h, w, in_ch) frames, or (n, h, w) planes for the single-channel filters (under
    a BGR input format those reach the library, which refuses them with MI355_ERR_UNSUPPORTED)."""
    if _in_bpp(filt) == 1:
        assert frames.ndim == 3, "single-channel filters take (n, h, w) uint8 planes"
        return frames.shape
    assert frames.ndim == 4
    n, h, w, c = frames.shape
    assert c == in_ch
    return n, h, w


def resize_check(bpp, src_w, src_h, dst_w, dst_h, nframes=1, interp=INTERP_LINEAR):
    """mi355_resize_check, a pure host function: the code (0 ok, -1 bad argument, -4 unsupported) a resize call with
    these values returns before any device work."""
    return load_library().mi355_resize_check(int(bpp), int(src_w), int(src_h), int(dst_w), int(dst_h), int(nframes),
                                             int(interp))


def _matrix(m):
    """Six doubles for the C calls from any 2 x 3 or flat sequence (None stays a null pointer)."""
    if m is None:
        return None
    v = np.asarray(m, np.float64).ravel()
    if v.size != 6:
        raise Mi355Error("warp_affine", -1, "expected a 2 x 3 matrix")
    return (ctypes.c_double * 6)(*v.tolist())


def rotation_matrix(cx, cy, angle_deg, scale=1.0):
    """mi355_rotation_matrix, cv::getRotationMatrix2D: the (2, 3) float64 matrix of a rotation by angle_deg
    (counter-clockwise, the origin at the top-left corner) about (cx, cy) with an isotropic scale."""
    m = (ctypes.c_double * 6)()
    _check("mi355_rotation_matrix", load_library().mi355_rotation_matrix(float(cx), float(cy), float(angle_deg),
                                                                         float(scale), m))
    return np.array(list(m), np.float64).reshape(2, 3)


def warp_affine_matrix(m, flags=INTERP_LINEAR):
    """mi355_warp_affine_matrix: the (2, 3) float64 map from an output pixel to its source position that a warp call
    with (m, flags) uses: m itself under WARP_INVERSE_MAP, else OpenCV's inversion."""
    inv = (ctypes.c_double * 6)()
    _check("mi355_warp_affine_matrix", load_library().mi355_warp_affine_matrix(_matrix(m), int(flags), inv))
    return np.array(list(inv), np.float64).reshape(2, 3)


def warp_affine_check(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags=INTERP_LINEAR, border_mode=BORDER_CONSTANT):
    """mi355_warp_affine_check, a pure host function: the code (0 ok, -1 bad argument, -4 unsupported) a warp call with
    these values returns before any device work."""
    return load_library().mi355_warp_affine_check(int(bpp), int(src_w), int(src_h), int(dst_w), int(dst_h),
                                                  int(nframes), _matrix(m), int(flags), int(border_mode))


def _matrix9(m):
    """Nine doubles for the C calls from any 3 x 3 or flat sequence (None stays a null pointer)."""
    if m is None:
        return None
    v = np.asarray(m, np.float64).ravel()
    if v.size != 9:
        raise Mi355Error("warp_perspective", -1, "expected a 3 x 3 matrix")
    return (ctypes.c_double * 9)(*v.tolist())


def perspective_matrix(m, flags=INTERP_LINEAR):
    """mi355_perspective_matrix: the (3, 3) float64 map from an output pixel to its source position that a perspective
    call with (m, flags) uses: m itself under WARP_INVERSE_MAP, else the adjugate times 1 / det."""
    inv = (ctypes.c_double * 9)()
    _check("mi355_perspective_matrix", load_library().mi355_perspective_matrix(_matrix9(m), int(flags), inv))
    return np.array(list(inv), np.float64).reshape(3, 3)


def warp_perspective_check(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags=INTERP_LINEAR,
                           border_mode=BORDER_CONSTANT):
    """mi355_warp_perspective_check, a pure host function: the code (0 ok, -1 bad argument, -4 unsupported) a
    perspective call with these values returns before any device work."""
    return load_library().mi355_warp_perspective_check(int(bpp), int(src_w), int(src_h), int(dst_w), int(dst_h),
                                                       int(nframes), _matrix9(m), int(flags), int(border_mode))


def remap_check(bpp, src_w, src_h, dst_w, dst_h, nframes=1, map_kind=MAP_FIXED, interp=INTERP_LINEAR,
                border_mode=BORDER_CONSTANT):
    """mi355_remap_check, a pure host function: the code (0 ok, -1 bad argument, -4 unsupported) a remap call with these
    values returns before any device work."""
    return load_library().mi355_remap_check(int(bpp), int(src_w), int(src_h), int(dst_w), int(dst_h), int(nframes),
                                            int(map_kind), int(interp), int(border_mode))


def _host_maps(fn, map1, map2, map_kind, dst_w, dst_h):
    """The two maps of a host remap call as contiguous arrays of the kind's types and of dst_h x dst_w entries (map2
    None stays a null pointer: FIXED + NEAREST does not read it)."""
    fixed = int(map_kind) == MAP_FIXED
    m1 = np.ascontiguousarray(map1, np.int16 if fixed else np.float32)
    m2 = None if map2 is None else np.ascontiguousarray(map2, np.uint16 if fixed else np.float32)
    n = int(dst_w) * int(dst_h)
    if m1.size != (2 * n if fixed else n) or (m2 is not None and m2.size != n):
        raise Mi355Error(fn, -1, "expected maps of dst_h x dst_w entries")
    return m1, m2


def adaptive_threshold_check(w, h, nframes=1, max_value=255, type=ADAPTIVE_BINARY, block=3, delta=0.0):
    """mi355_adaptive_threshold_check, a pure host function: the code (0 ok, -1 bad argument) an adaptive-threshold call
    with these values returns before any device work."""
    return load_library().mi355_adaptive_threshold_check(int(w), int(h), int(nframes), int(max_value), int(type),
                                                         int(block), float(delta))


def clahe_check(w, h, nframes=1, clip_limit=40.0, tiles_x=8, tiles_y=8):
    """mi355_clahe_check, a pure host function: the code (0 ok, -1 bad argument, -4 a pad one reflection cannot serve) a
    CLAHE call with these values returns before any device work."""
    return load_library().mi355_clahe_check(int(w), int(h), int(nframes), float(clip_limit), int(tiles_x), int(tiles_y))


def ccl_check(w, h, nframes=1, connectivity=8, stats_rows=0):
    """mi355_ccl_check, a pure host function: the code (0 ok, -1 bad argument) a labelling call with these values returns
    before any device work."""
    return load_library().mi355_ccl_check(int(w), int(h), int(nframes), int(connectivity), int(stats_rows))


def dist_check(w, h, nframes=1):
    """mi355_dist_check, a pure host function: the code (0 ok, -1 bad argument) a distance-transform call with these values
    returns before any device work."""
    return load_library().mi355_dist_check(int(w), int(h), int(nframes))


def hysteresis_check(w, h, nframes=1, low=0, high=0, connectivity=8):
    """mi355_hysteresis_check, a pure host function: the code (0 ok, -1 bad argument) a hysteresis call with these values
    returns before any device work."""
    return load_library().mi355_hysteresis_check(int(w), int(h), int(nframes), int(low), int(high), int(connectivity))


def canny_check(w, h, nframes=1, threshold1=50.0, threshold2=150.0, flags=0):
    """mi355_canny_check, a pure host function: the code (0 ok, -1 bad argument) a Canny call with these values returns
    before any device work."""
    return load_library().mi355_canny_check(int(w), int(h), int(nframes), float(threshold1), float(threshold2), int(flags))


def hough_check(w, h, nframes=1, rho=1.0, theta=np.pi / 180, threshold=0, max_lines=1, min_theta=0.0, max_theta=np.pi):
    """mi355_hough_check, a pure host function: the code (0 ok, -1 bad argument) a Hough lines call with these values
    returns before any device work."""
    return load_library().mi355_hough_check(int(w), int(h), int(nframes), float(rho), float(theta), int(threshold),
                                            int(max_lines), float(min_theta), float(max_theta))


def hough_shape(w, h, rho=1.0, theta=np.pi / 180, min_theta=0.0, max_theta=np.pi):
    """mi355_hough_shape, a pure host function: (numangle, numrho) of the accumulator, whose frames are
    (numangle + 2, numrho + 2) int32 with a zero ring."""
    na, nr = _ci(0), _ci(0)
    rc = load_library().mi355_hough_shape(int(w), int(h), float(rho), float(theta), float(min_theta), float(max_theta),
                                          ctypes.byref(na), ctypes.byref(nr))
    _check("mi355_hough_shape", rc)
    return na.value, nr.value


def hough_trig_table(w, h, rho=1.0, theta=np.pi / 180, min_theta=0.0, max_theta=np.pi):
    """mi355_hough_trig_table, a pure host function: (tab_cos, tab_sin), numangle float32 each, as the kernels get them."""
    na, _ = hough_shape(w, h, rho, theta, min_theta, max_theta)
    tc, ts = np.empty(na, np.float32), np.empty(na, np.float32)
    rc = load_library().mi355_hough_trig_table(int(w), int(h), float(rho), float(theta), float(min_theta), float(max_theta),
                                               tc.ctypes.data_as(_f32p), ts.ctypes.data_as(_f32p))
    _check("mi355_hough_trig_table", rc)
    return tc, ts


def hough_accum_bytes(w, h, nframes=1, rho=1.0, theta=np.pi / 180, min_theta=0.0, max_theta=np.pi):
    """mi355_hough_accum_bytes, a pure host function: the bytes of nframes accumulators, 0 for rejected values."""
    return int(load_library().mi355_hough_accum_bytes(int(w), int(h), int(nframes), float(rho), float(theta),
                                                      float(min_theta), float(max_theta)))


def hough_plan(w, h, rho=1.0, theta=np.pi / 180, min_theta=0.0, max_theta=np.pi):
    """mi355_hough_plan, a pure host function: (angle rows per workgroup, rho ranges per row, LDS budget in cells) of the
    voting launch for these values."""
    a, s, c = _ci(0), _ci(0), _ci(0)
    rc = load_library().mi355_hough_plan(int(w), int(h), float(rho), float(theta), float(min_theta), float(max_theta),
                                         ctypes.byref(a), ctypes.byref(s), ctypes.byref(c))
    _check("mi355_hough_plan", rc)
    return a.value, s.value, c.value


def yuv_frame_bytes(layout, w, h, pitch=0, rows=0):
    """mi355_yuv_frame_bytes, a pure host function: the bytes from one YUV frame to the next (pitch 0 = tight, rows 0 = h),
    0 for arguments the YUV calls reject."""
    return int(load_library().mi355_yuv_frame_bytes(int(layout), int(w), int(h), int(pitch), int(rows)))


def yuv_check(layout, standard, w, h, nframes=1, pitch=0, rows=0, encode=False):
    """mi355_yuv_check, a pure host function: the code (0 ok, -1 bad argument, -4 the encode of a packed layout) a YUV
    call with these values returns before any device work."""
    return load_library().mi355_yuv_check(int(layout), int(standard), int(w), int(h), int(nframes), int(pitch),
                                          int(rows), 1 if encode else 0)


def device_count():
    n = _ci(0)
    _check("mi355_device_count", load_library().mi355_device_count(ctypes.byref(n)))
    return n.value


class Context:
    """One GPU + one HIP stream + pooled buffers + cached coefficient tables."""

    def __init__(self, device=0, stream=None, lib=None):
        self._lib = lib if lib is not None else load_library()
        self._h = _vp()
        if stream is None:
            rc = self._lib.mi355_ctx_create(int(device), ctypes.byref(self._h))
            fn = "mi355_ctx_create"
        else:
            rc = self._lib.mi355_ctx_create_on_stream(int(device), _vp(int(stream)), ctypes.byref(self._h))
            fn = "mi355_ctx_create_on_stream"
        _check(fn, rc)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if self._h:
            self._lib.mi355_ctx_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        _check("mi355_ctx_device_name", self._lib.mi355_ctx_device_name(self._h, buf, 256), self._h)
        return buf.value.decode()

    def sync(self):
        _check("mi355_sync", self._lib.mi355_sync(self._h), self._h)

    def set_gauss_mode(self, mode):
        _check("mi355_ctx_set_gauss_mode", self._lib.mi355_ctx_set_gauss_mode(self._h, int(mode)), self._h)

    def set_input_format(self, fmt):
        """INPUT_RGBA (default) or INPUT_BGR: host-buffer calls then take (h, w, 3) / (n, h, w, 3) BGR frames."""
        _check("mi355_ctx_set_input_format", self._lib.mi355_ctx_set_input_format(self._h, int(fmt)), self._h)
        self._in_ch = 3 if fmt == INPUT_BGR else 4

    def set_impl(self, impl):
        _check("mi355_ctx_set_impl", self._lib.mi355_ctx_set_impl(self._h, int(impl)), self._h)

    def set_gauss_weights(self, k, sigma, table):
        table = np.ascontiguousarray(table, np.float32)
        if table.size != k * k:
            raise Mi355Error("mi355_ctx_set_gauss_weights", -1, "table must hold k*k floats")
        rc = self._lib.mi355_ctx_set_gauss_weights(self._h, int(k), float(sigma), table.ctypes.data_as(_f32p))
        _check("mi355_ctx_set_gauss_weights", rc, self._h)

    # -- host-buffer calls (numpy) ------------------------------------------------------------
    def _frames(self, fn, a, bpp):
        """What the host-buffer call `fn` sends for `a`: contiguous uint8 (n, h, w, c) frames with the input format's
        channel count (bpp 4) or (n, h, w) planes (bpp 1), and whether `a` was one frame, so that the result drops its
        first axis."""
        a = np.ascontiguousarray(a, np.uint8)
        one_ndim = 3 if bpp == 4 else 2
        if a.ndim not in (one_ndim, one_ndim + 1):
            raise Mi355Error(fn, -1, "expected (h, w, 4) or (n, h, w, 4) uint8" if bpp == 4 else
                             "expected (h, w) or (n, h, w) uint8")
        frames = a[None] if a.ndim == one_ndim else a
        in_ch = getattr(self, "_in_ch", 4)
        if bpp == 4 and frames.shape[3] != in_ch:
            raise Mi355Error(fn, -1, "expected %d channels per pixel" % in_ch)
        return frames, a.ndim == one_ndim

    def _host(self, filt, rgba, k=0, sigma=0.0, profile=False):
        frames, one = self._frames("filter", rgba, 4)
        n, h, w = frames.shape[:3]
        bpp = _out_bpp(filt)
        out = np.empty((n, h, w, 4) if bpp == 4 else (n, h, w), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_filter_batched(self._h, filt, frames.ctypes.data_as(_u8p),
                                            out.ctypes.data_as(_u8p), w, h, n, int(k), float(sigma), prof)
        _check("mi355_filter_batched", rc, self._h)
        out = out[0] if one else out
        return (out, list(prof)) if profile else out

    def gray(self, rgba, profile=False):
        """Controller::PerformCLImageGrayscaling (buffer mode): (g,g,g,255) per pixel."""
        return self._host(FILTER_GRAY, rgba, profile=profile)

    def gray1(self, rgba, profile=False):
        return self._host(FILTER_GRAY1, rgba, profile=profile)

    def gauss(self, rgba, k, sigma, profile=False):
        """Controller::PerformCLGaussianBlur."""
        return self._host(FILTER_GAUSS, rgba, k, sigma, profile=profile)

    def sobel(self, rgba, profile=False):
        """Controller::PerformCLImageEdgeDetection: one byte per pixel."""
        return self._host(FILTER_SOBEL, rgba, profile=profile)

    def pipeline(self, rgba, k, sigma, profile=False):
        return self._host(FILTER_PIPELINE, rgba, k, sigma, profile=profile)

    # -- single-channel frames: (h, w) or (n, h, w) uint8 in, the same shape out --------------------
    def _host_gray8(self, filt, y, k=0, sigma=0.0):
        frames, one = self._frames("filter", y, 1)
        n, h, w = frames.shape
        out = np.empty((n, h, w), np.uint8)
        rc = self._lib.mi355_filter_batched(self._h, filt, frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p),
                                            w, h, n, int(k), float(sigma), None)
        _check("mi355_filter_batched", rc, self._h)
        return out[0] if one else out

    def gauss_gray8(self, y, k, sigma):
        """GaussianBlur.cpp:234-261 on one channel (MI355_FILTER_GAUSS_GRAY8)."""
        return self._host_gray8(FILTER_GAUSS_GRAY8, y, k, sigma)

    def sobel_gray8(self, y):
        """EdgeDetection.cpp:219-240 on the given plane, no luminance step (MI355_FILTER_SOBEL_GRAY8)."""
        return self._host_gray8(FILTER_SOBEL_GRAY8, y)

    def pipeline_gray8(self, y, k, sigma):
        """sobel_gray8(EXACT gauss_gray8(y)) in either Gaussian mode (MI355_FILTER_PIPELINE_GRAY8)."""
        return self._host_gray8(FILTER_PIPELINE_GRAY8, y, k, sigma)

    def median(self, rgba, k, profile=False):
        """cv::medianBlur on every channel of (h, w, 4) / (n, h, w, 4) frames (MI355_FILTER_MEDIAN); k in {3, 5, 7}."""
        return self._host(FILTER_MEDIAN, rgba, k, 0.0, profile=profile)

    def median_gray8(self, y, k):
        """cv::medianBlur of (h, w) / (n, h, w) single-channel frames (MI355_FILTER_MEDIAN_GRAY8)."""
        return self._host_gray8(FILTER_MEDIAN_GRAY8, y, k)

    def erode(self, rgba, k, profile=False):
        """cv::erode with a k x k rectangle on every channel of (h, w, 4) / (n, h, w, 4) frames (MI355_FILTER_ERODE);
        odd 3 <= k <= MAX_MORPH_K, clamp-to-edge borders."""
        return self._host(FILTER_ERODE, rgba, k, 0.0, profile=profile)

    def dilate(self, rgba, k, profile=False):
        """cv::dilate with a k x k rectangle on every channel (MI355_FILTER_DILATE)."""
        return self._host(FILTER_DILATE, rgba, k, 0.0, profile=profile)

    def morph_open(self, rgba, k, profile=False):
        """cv::morphologyEx(MORPH_OPEN) with a k x k rectangle, dilate(erode(x)) in one launch (MI355_FILTER_OPEN)."""
        return self._host(FILTER_OPEN, rgba, k, 0.0, profile=profile)

    def morph_close(self, rgba, k, profile=False):
        """cv::morphologyEx(MORPH_CLOSE) with a k x k rectangle, erode(dilate(x)) in one launch (MI355_FILTER_CLOSE).
        (Named morph_*: Context.close() releases the context.)"""
        return self._host(FILTER_CLOSE, rgba, k, 0.0, profile=profile)

    def erode_gray8(self, y, k):
        """cv::erode of (h, w) / (n, h, w) single-channel frames (MI355_FILTER_ERODE_GRAY8)."""
        return self._host_gray8(FILTER_ERODE_GRAY8, y, k)

    def dilate_gray8(self, y, k):
        """cv::dilate of single-channel frames (MI355_FILTER_DILATE_GRAY8)."""
        return self._host_gray8(FILTER_DILATE_GRAY8, y, k)

    def morph_open_gray8(self, y, k):
        """MORPH_OPEN of single-channel frames (MI355_FILTER_OPEN_GRAY8)."""
        return self._host_gray8(FILTER_OPEN_GRAY8, y, k)

    def morph_close_gray8(self, y, k):
        """MORPH_CLOSE of single-channel frames (MI355_FILTER_CLOSE_GRAY8)."""
        return self._host_gray8(FILTER_CLOSE_GRAY8, y, k)

    def equalize_hist_gray8(self, y):
        """cv::equalizeHist of (h, w) / (n, h, w) single-channel frames, each frame on its own
        (MI355_FILTER_EQUALIZE_GRAY8)."""
        return self._host_gray8(FILTER_EQUALIZE_GRAY8, y)

    def otsu_gray8(self, y):
        """cv::threshold(THRESH_BINARY | THRESH_OTSU) to 0 / 255 of single-channel frames (MI355_FILTER_OTSU_GRAY8)."""
        return self._host_gray8(FILTER_OTSU_GRAY8, y)

    def box(self, rgba, k, profile=False):
        """cv::blur(Size(k, k), BORDER_REPLICATE) on every channel of (h, w, 4) / (n, h, w, 4) frames (MI355_FILTER_BOX);
        odd 3 <= k <= MAX_BOX_K."""
        return self._host(FILTER_BOX, rgba, k, 0.0, profile=profile)

    def box_gray8(self, y, k):
        """cv::blur(Size(k, k), BORDER_REPLICATE) of (h, w) / (n, h, w) single-channel frames (MI355_FILTER_BOX_GRAY8)."""
        return self._host_gray8(FILTER_BOX_GRAY8, y, k)

    # -- single-output gray8 calls: (frames, out, w, h, n, <the call's own>, prof_ns) -----------------------
    def _gray8_host(self, fn_name, y, profile, *tail):
        frames, one = self._frames(fn_name[len("mi355_"):-len("_batched")], y, 1)
        n, h, w = frames.shape
        out = np.empty((n, h, w), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = getattr(self._lib, fn_name)(self._h, frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), w, h, n, *tail,
                                         prof if profile else None)
        _check(fn_name, rc, self._h)
        out = out[0] if one else out
        return (out, list(prof)) if profile else out

    def adaptive_threshold_gray8(self, y, max_value, type, block, delta, profile=False):
        """cv::adaptiveThreshold(y, max_value, ADAPTIVE_THRESH_MEAN_C, type, block, delta) of (h, w) / (n, h, w)
        single-channel frames (mi355_adaptive_threshold_gray8_batched); type is ADAPTIVE_BINARY or ADAPTIVE_BINARY_INV."""
        return self._gray8_host("mi355_adaptive_threshold_gray8_batched", y, profile, int(max_value), int(type),
                                int(block), float(delta))

    def clahe_gray8(self, y, clip_limit=40.0, tiles_x=8, tiles_y=8, profile=False):
        """cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply() of (h, w) / (n, h, w) single-channel frames
        (mi355_clahe_gray8_batched); the defaults are OpenCV's."""
        return self._gray8_host("mi355_clahe_gray8_batched", y, profile, float(clip_limit), int(tiles_x), int(tiles_y))

    def ccl_gray8(self, mask, connectivity=8, stats_rows=0, profile=False):
        """cv::connectedComponentsWithStats of (h, w) / (n, h, w) single-channel masks (mi355_ccl_gray8_batched): int32
        labels numbered by first pixel and the label count N (background included; an int for one frame, else (n,)
        int32).  With stats_rows > 0 also stats (stats_rows, 5) int32 {left, top, width, height, area} and centroids
        (stats_rows, 2) float64 = coordinate sums / area, NaN for a row without a pixel; each with a leading n for a
        batch.  Returns (labels, count) or (labels, count, stats, centroids); with profile, the six timestamps follow."""
        frames, one = self._frames("ccl_gray8", mask, 1)
        n, h, w = frames.shape
        rows = int(stats_rows)
        labels = np.empty((n, h, w), np.int32)
        count = np.empty(n, np.int32)
        stats = np.empty((n, max(rows, 0), 5), np.int32)
        sums = np.empty((n, max(rows, 0), 2), np.uint64)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_ccl_gray8_batched(
            self._h, frames.ctypes.data_as(_u8p), labels.ctypes.data_as(_vp), count.ctypes.data_as(_vp),
            stats.ctypes.data_as(_vp) if rows > 0 else None, sums.ctypes.data_as(_vp) if rows > 0 else None, w, h, n,
            int(connectivity), rows, prof if profile else None)
        _check("mi355_ccl_gray8_batched", rc, self._h)
        out = (labels[0], int(count[0])) if one else (labels, count)
        if rows > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                centroids = sums.astype(np.float64) / stats[:, :, 4:5].astype(np.float64)
            out += (stats[0], centroids[0]) if one else (stats, centroids)
        return out + (list(prof),) if profile else out

    def dist_gray8(self, masks, squared=False, nearest=False, profile=False):
        """cv::distanceTransform(mask, DIST_L2, DIST_MASK_PRECISE, CV_32F) of (h, w) / (n, h, w) single-channel masks
        (mi355_dist_gray8_batched): float32 distances to the nearest zero pixel.  With squared also the exact int32 squared
        distances, with nearest also the int32 index y' * w + x' of the nearest zero pixel (smallest column, then smallest
        row among equally near ones); a frame without a zero pixel holds +inf, DIST_NONE and -1.  Returns dist, or a tuple
        (dist[, sq][, nearest]); with profile, the six timestamps follow."""
        frames, one = self._frames("dist_gray8", masks, 1)
        n, h, w = frames.shape
        dist = np.empty((n, h, w), np.float32)
        sq = np.empty((n, h, w), np.int32) if squared else None
        near = np.empty((n, h, w), np.int32) if nearest else None
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_dist_gray8_batched(
            self._h, frames.ctypes.data_as(_u8p), _vp(sq.ctypes.data) if squared else None, _vp(dist.ctypes.data),
            _vp(near.ctypes.data) if nearest else None, w, h, n, prof if profile else None)
        _check("mi355_dist_gray8_batched", rc, self._h)
        out = tuple(a[0] if one else a for a in (dist, sq, near) if a is not None)
        out += (list(prof),) if profile else ()
        return out[0] if len(out) == 1 else out

    def hysteresis_gray8(self, y, low, high, connectivity=8, profile=False):
        """Hysteresis threshold of (h, w) / (n, h, w) single-channel response maps (mi355_hysteresis_gray8_batched): 255
        where the byte > low and the pixel's component of such pixels holds a byte > high, else 0."""
        return self._gray8_host("mi355_hysteresis_gray8_batched", y, profile, int(low), int(high), int(connectivity))

    def canny_gray8(self, y, threshold1, threshold2, flags=0, profile=False):
        """cv::Canny(y, edges, threshold1, threshold2, 3, flags & CANNY_L2GRADIENT) of (h, w) / (n, h, w) single-channel
        frames (mi355_canny_gray8_batched): 255 on edges, else 0.  No blur of its own: chain gauss_gray8 in front."""
        return self._gray8_host("mi355_canny_gray8_batched", y, profile, float(threshold1), float(threshold2),
                                int(flags))

    def hough_lines_gray8(self, edges, rho, theta, threshold, max_lines=256, min_theta=0.0, max_theta=np.pi,
                          profile=False):
        """cv::HoughLines(edges, lines, rho, theta, threshold, 0, 0, min_theta, max_theta) of (h, w) / (n, h, w)
        single-channel edge maps (mi355_hough_lines_gray8_batched).  Returns (lines, votes, count): float32
        (max_lines, 2) rows of (rho, theta) by votes descending then accumulator cell ascending, their int32 votes, and the
        number of peaks, which may exceed max_lines; rows past min(count, max_lines) are zero."""
        frames, one = self._frames("hough_lines_gray8", edges, 1)
        n, h, w = frames.shape
        lines = np.empty((n, int(max_lines), 2), np.float32) if max_lines > 0 else np.empty((n, 0, 2), np.float32)
        votes = np.empty((n, lines.shape[1]), np.int32)
        count = np.empty(n, np.int32)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_hough_lines_gray8_batched(
            self._h, frames.ctypes.data_as(_u8p), _vp(lines.ctypes.data), _vp(votes.ctypes.data), _vp(count.ctypes.data),
            w, h, n, float(rho), float(theta), int(threshold), int(max_lines), float(min_theta), float(max_theta),
            prof if profile else None)
        _check("mi355_hough_lines_gray8_batched", rc, self._h)
        out = (lines[0], votes[0], int(count[0])) if one else (lines, votes, count)
        return out + (list(prof),) if profile else out

    # -- frames from a decoder or a camera (mi355_yuv_to_rgba8_batched / mi355_rgba8_to_yuv_batched) -----
    def yuv_to_rgba8(self, yuv, w, h, layout, standard=YUV_BT601, pitch=0, rows=0, profile=False):
        """cv::cvtColor(COLOR_YUV2RGBA_*) of whole frames in host memory: `yuv` holds n frames of yuv_frame_bytes(layout,
        w, h, pitch, rows) bytes each, back to back, in any shape; returns (n, h, w, 4) RGBA with A = 255."""
        yuv = np.ascontiguousarray(yuv, np.uint8).ravel()
        fb = yuv_frame_bytes(layout, w, h, pitch, rows)
        n = yuv.size // fb if fb else 1
        if fb and (n < 1 or n * fb != yuv.size):
            raise Mi355Error("yuv_to_rgba8", -1, "expected a whole number of frames of %d bytes" % fb)
        out = np.empty((n, int(h), int(w), 4), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_yuv_to_rgba8_batched(self._h, yuv.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), int(w),
                                                  int(h), n, int(layout), int(standard), int(pitch), int(rows),
                                                  prof if profile else None)
        _check("mi355_yuv_to_rgba8_batched", rc, self._h)
        return (out, list(prof)) if profile else out

    def rgba8_to_yuv(self, rgba, layout, standard=YUV_BT601, pitch=0, rows=0, profile=False):
        """cv::cvtColor(COLOR_RGBA2YUV_I420 / _YV12), and the same arithmetic for NV12 / NV21, of (h, w, 4) / (n, h, w, 4)
        RGBA frames in host memory (always RGBA, whatever the context's input format): returns (n, frame bytes) uint8,
        or (frame bytes,) for one frame; the padding of a pitched result is zero."""
        a = np.ascontiguousarray(rgba, np.uint8)
        if a.ndim not in (3, 4) or a.shape[-1] != 4:
            raise Mi355Error("rgba8_to_yuv", -1, "expected (h, w, 4) or (n, h, w, 4) uint8")
        frames = a[None] if a.ndim == 3 else a
        n, h, w = frames.shape[:3]
        fb = yuv_frame_bytes(layout, w, h, pitch, rows)
        out = np.empty((n, max(fb, 1)), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_rgba8_to_yuv_batched(self._h, frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), w, h, n,
                                                  int(layout), int(standard), int(pitch), int(rows),
                                                  prof if profile else None)
        _check("mi355_rgba8_to_yuv_batched", rc, self._h)
        out = out[0] if a.ndim == 3 else out
        return (out, list(prof)) if profile else out

    # -- calls that change the frame size: (frames, out, bpp, w, h, dst_w, dst_h, n, <the call's own>, prof_ns) -----
    def _geom_host(self, fn_name, frames, bpp, dst_w, dst_h, profile, *tail):
        n, h, w = frames.shape[:3]
        out = np.empty((n, int(dst_h), int(dst_w), 4) if bpp == 4 else (n, int(dst_h), int(dst_w)), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = getattr(self._lib, fn_name)(self._h, frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), bpp, w, h,
                                         int(dst_w), int(dst_h), n, *tail, prof if profile else None)
        _check(fn_name, rc, self._h)
        return out, list(prof)

    # -- changing the frame size (mi355_resize_batched) ---------------------------------------------
    def resize(self, rgba, dst_w, dst_h, interp=INTERP_LINEAR, profile=False):
        """cv::resize of (h, w, 4) / (n, h, w, 4) frames to (dst_h, dst_w), every channel on its own; interp is
        INTERP_NEAREST, INTERP_LINEAR or INTERP_AREA (integer factors only).  Under INPUT_BGR the frames have 3 channels
        and the result is RGBA."""
        frames, one = self._frames("resize", rgba, 4)
        out, prof = self._geom_host("mi355_resize_batched", frames, 4, dst_w, dst_h, profile, int(interp))
        out = out[0] if one else out
        return (out, prof) if profile else out

    def resize_gray8(self, y, dst_w, dst_h, interp=INTERP_LINEAR):
        """cv::resize of (h, w) / (n, h, w) single-channel frames to (dst_h, dst_w)."""
        frames, one = self._frames("resize_gray8", y, 1)
        out, _ = self._geom_host("mi355_resize_batched", frames, 1, dst_w, dst_h, False, int(interp))
        return out[0] if one else out

    # -- rotating, shifting and deskewing frames (mi355_warp_affine_batched) ---------------------------
    def warp_affine(self, rgba, m, dst_w, dst_h, flags=INTERP_LINEAR, border_mode=BORDER_CONSTANT, border_value=0,
                    profile=False):
        """cv::warpAffine of (h, w, 4) / (n, h, w, 4) frames through the 2 x 3 matrix m to (dst_h, dst_w), every channel
        on its own; flags is INTERP_NEAREST or INTERP_LINEAR, optionally | WARP_INVERSE_MAP; border_value is
        R | G << 8 | B << 16 | A << 24, used under BORDER_CONSTANT.  Under INPUT_BGR the frames have 3 channels and the
        result is RGBA."""
        frames, one = self._frames("warp_affine", rgba, 4)
        out, prof = self._geom_host("mi355_warp_affine_batched", frames, 4, dst_w, dst_h, profile, _matrix(m),
                                    int(flags), int(border_mode), int(border_value) & 0xFFFFFFFF)
        out = out[0] if one else out
        return (out, prof) if profile else out

    def warp_affine_gray8(self, y, m, dst_w, dst_h, flags=INTERP_LINEAR, border_mode=BORDER_CONSTANT, border_value=0):
        """cv::warpAffine of (h, w) / (n, h, w) single-channel frames to (dst_h, dst_w); border_value's low byte is the
        border under BORDER_CONSTANT."""
        frames, one = self._frames("warp_affine_gray8", y, 1)
        out, _ = self._geom_host("mi355_warp_affine_batched", frames, 1, dst_w, dst_h, False, _matrix(m), int(flags),
                                 int(border_mode), int(border_value) & 0xFFFFFFFF)
        return out[0] if one else out

    # -- undistorting and rectifying frames (mi355_remap_batched, mi355_warp_perspective_batched) ----
    def remap(self, rgba, map1, map2, dst_w, dst_h, map_kind=MAP_FIXED, interp=INTERP_LINEAR,
              border_mode=BORDER_CONSTANT, border_value=0, profile=False):
        """cv::remap of (h, w, 4) / (n, h, w, 4) frames through one map to (dst_h, dst_w), every channel on its own.
        MAP_FIXED: map1 (dst_h, dst_w, 2) int16 (sx, sy), map2 (dst_h, dst_w) uint16 fy*32+fx (None with
        INTERP_NEAREST); MAP_FLOAT: map1 and map2 (dst_h, dst_w) float32 x and y.  border_value is
        R | G << 8 | B << 16 | A << 24, used under BORDER_CONSTANT.  Under INPUT_BGR the frames have 3 channels and the
        result is RGBA."""
        frames, one = self._frames("remap", rgba, 4)
        m1, m2 = _host_maps("remap", map1, map2, map_kind, dst_w, dst_h)
        out, prof = self._geom_host("mi355_remap_batched", frames, 4, dst_w, dst_h, profile, _vp(m1.ctypes.data),
                                    None if m2 is None else _vp(m2.ctypes.data), int(map_kind), int(interp),
                                    int(border_mode), int(border_value) & 0xFFFFFFFF)
        out = out[0] if one else out
        return (out, prof) if profile else out

    def remap_gray8(self, y, map1, map2, dst_w, dst_h, map_kind=MAP_FIXED, interp=INTERP_LINEAR,
                    border_mode=BORDER_CONSTANT, border_value=0):
        """cv::remap of (h, w) / (n, h, w) single-channel frames to (dst_h, dst_w); border_value's low byte is the
        border under BORDER_CONSTANT."""
        frames, one = self._frames("remap_gray8", y, 1)
        m1, m2 = _host_maps("remap", map1, map2, map_kind, dst_w, dst_h)
        out, _ = self._geom_host("mi355_remap_batched", frames, 1, dst_w, dst_h, False, _vp(m1.ctypes.data),
                                 None if m2 is None else _vp(m2.ctypes.data), int(map_kind), int(interp),
                                 int(border_mode), int(border_value) & 0xFFFFFFFF)
        return out[0] if one else out

    def warp_perspective(self, rgba, m, dst_w, dst_h, flags=INTERP_LINEAR, border_mode=BORDER_CONSTANT, border_value=0,
                         profile=False):
        """cv::warpPerspective of (h, w, 4) / (n, h, w, 4) frames through the 3 x 3 matrix m to (dst_h, dst_w), every
        channel on its own; flags, border_value and INPUT_BGR as in warp_affine."""
        frames, one = self._frames("warp_perspective", rgba, 4)
        out, prof = self._geom_host("mi355_warp_perspective_batched", frames, 4, dst_w, dst_h, profile, _matrix9(m),
                                    int(flags), int(border_mode), int(border_value) & 0xFFFFFFFF)
        out = out[0] if one else out
        return (out, prof) if profile else out

    def warp_perspective_gray8(self, y, m, dst_w, dst_h, flags=INTERP_LINEAR, border_mode=BORDER_CONSTANT,
                               border_value=0):
        """cv::warpPerspective of (h, w) / (n, h, w) single-channel frames to (dst_h, dst_w); border_value's low byte is
        the border under BORDER_CONSTANT."""
        frames, one = self._frames("warp_perspective_gray8", y, 1)
        out, _ = self._geom_host("mi355_warp_perspective_batched", frames, 1, dst_w, dst_h, False, _matrix9(m),
                                 int(flags), int(border_mode), int(border_value) & 0xFFFFFFFF)
        return out[0] if one else out

    def _stats_gray8(self, fn, y, per_frame, dtype):
        frames, one = self._frames(fn, y, 1)
        n, h, w = frames.shape
        out = np.empty((n, per_frame), dtype)
        d_in = self.alloc(frames.nbytes)
        try:
            d_out = self.alloc(out.nbytes)
            try:
                self.h2d(d_in, frames)
                rc = getattr(self._lib, fn)(self._h, _vp(d_in), _vp(d_out), w, h, n)
                _check(fn, rc, self._h)
                self.sync()
                self.d2h(out, d_out)
            finally:
                self.sync()
                self.free(d_out)
        finally:
            self.free(d_in)
        return out[0] if one else out

    def hist_gray8(self, y):
        """The 256 bin counts of each single-channel frame (cv::calcHist), through mi355_hist_gray8_dev: (n, 256)
        uint32 for (n, h, w) frames, (256,) for one (h, w) frame."""
        return self._stats_gray8("mi355_hist_gray8_dev", y, 256, np.uint32)

    def otsu_thresholds_gray8(self, y):
        """The Otsu threshold t of each single-channel frame (what cv::threshold returns), through
        mi355_otsu_thresholds_gray8_dev: (n,) int32 for (n, h, w) frames, a 0-d array for one (h, w) frame."""
        out = self._stats_gray8("mi355_otsu_thresholds_gray8_dev", y, 1, np.int32)
        return out[..., 0]

    def image2d(self, filt, rgba, k=0, sigma=0.0):
        """mi355_image2d_rgba8: the reference's image2d_t-mode semantics.  Returns (out, six timestamps)."""
        rgba = np.ascontiguousarray(rgba, np.uint8)
        h, w, _ = rgba.shape
        out = np.empty((h, w, 4) if filt == FILTER_GAUSS else (h, w), np.uint8)
        prof = (ctypes.c_uint64 * 6)()
        rc = self._lib.mi355_image2d_rgba8(self._h, int(filt), rgba.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p),
                                           w, h, int(k), float(sigma), prof)
        _check("mi355_image2d_rgba8", rc, self._h)
        return out, list(prof)

    def pinned_empty(self, shape, dtype=np.uint8):
        """numpy array over pinned host memory (mi355_host_alloc); release with pinned_free(arr)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = _vp()
        _check("mi355_host_alloc", self._lib.mi355_host_alloc(self._h, nbytes, ctypes.byref(p)), self._h)
        buf = (ctypes.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def pinned_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            _check("mi355_host_free", self._lib.mi355_host_free(self._h, _vp(p)), self._h)

    def stream(self, filt, frames, out=None, k=0, sigma=0.0, chunk_frames=0):
        """mi355_filter_stream: overlapped H2D / kernel / D2H over a host batch.  Returns (out, elapsed_ms).
        frames: (n, h, w, c), or (n, h, w) for the single-channel filters."""
        assert frames.flags["C_CONTIGUOUS"] and frames.dtype == np.uint8
        n, h, w = _batch_shape(filt, frames, getattr(self, "_in_ch", 4))
        bpp = _out_bpp(filt)
        if out is None:
            out = np.empty((n, h, w, 4) if bpp == 4 else (n, h, w), np.uint8)
        ms = ctypes.c_double(0)
        rc = self._lib.mi355_filter_stream(self._h, int(filt), frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p),
                                           w, h, n, int(chunk_frames), int(k), float(sigma), ctypes.byref(ms))
        _check("mi355_filter_stream", rc, self._h)
        return out, ms.value

    def single(self, name, rgba, *args):
        """The per-frame C entry points themselves (mi355_gray_rgba8, ...), one frame."""
        rgba = np.ascontiguousarray(rgba, np.uint8)
        h, w, _ = rgba.shape
        prof = (ctypes.c_uint64 * 6)()
        one = name in ("gray1", "sobel", "pipeline")
        out = np.empty((h, w) if one else (h, w, 4), np.uint8)
        fn = getattr(self._lib, "mi355_%s_rgba8" % name)
        extra = [int(args[0]), float(args[1])] if name in ("gauss", "pipeline") else []
        rc = fn(self._h, rgba.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p), w, h, *extra, prof)
        _check("mi355_%s_rgba8" % name, rc, self._h)
        return out, list(prof)

    # -- device-resident calls (raw pointers) -------------------------------------------------
    def filter_dev(self, filt, d_in, d_out, w, h, nframes, k=0, sigma=0.0):
        rc = self._lib.mi355_filter_dev(self._h, int(filt), _vp(int(d_in)), _vp(int(d_out)), int(w), int(h),
                                        int(nframes), int(k), float(sigma))
        _check("mi355_filter_dev", rc, self._h)

    def resize_dev(self, d_in, d_out, bpp, sw, sh, dw, dh, nframes, interp=INTERP_LINEAR):
        """mi355_resize_dev: nframes frames of sw x sh at d_in to dw x dh at d_out, bpp 4 (RGBA) or 1 (gray8); one
        launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_resize_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(bpp), int(sw), int(sh), int(dw),
                                        int(dh), int(nframes), int(interp))
        _check("mi355_resize_dev", rc, self._h)

    def warp_affine_dev(self, d_in, d_out, bpp, sw, sh, dw, dh, nframes, m, flags=INTERP_LINEAR,
                        border_mode=BORDER_CONSTANT, border_value=0):
        """mi355_warp_affine_dev: nframes frames of sw x sh at d_in through m to dw x dh at d_out, bpp 4 (RGBA) or 1
        (gray8); one launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_warp_affine_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(bpp), int(sw), int(sh),
                                             int(dw), int(dh), int(nframes), _matrix(m), int(flags), int(border_mode),
                                             int(border_value) & 0xFFFFFFFF)
        _check("mi355_warp_affine_dev", rc, self._h)

    def remap_dev(self, d_in, d_out, bpp, sw, sh, dw, dh, nframes, d_map1, d_map2, map_kind=MAP_FIXED,
                  interp=INTERP_LINEAR, border_mode=BORDER_CONSTANT, border_value=0):
        """mi355_remap_dev: nframes frames of sw x sh at d_in through the device maps d_map1 / d_map2 (dw x dh entries;
        d_map2 0 or None with MAP_FIXED and INTERP_NEAREST) to dw x dh at d_out, bpp 4 (RGBA) or 1 (gray8); one launch,
        no synchronisation, no allocation."""
        rc = self._lib.mi355_remap_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(bpp), int(sw), int(sh), int(dw),
                                       int(dh), int(nframes), _vp(int(d_map1 or 0)), _vp(int(d_map2 or 0)),
                                       int(map_kind), int(interp), int(border_mode), int(border_value) & 0xFFFFFFFF)
        _check("mi355_remap_dev", rc, self._h)

    def warp_perspective_dev(self, d_in, d_out, bpp, sw, sh, dw, dh, nframes, m, flags=INTERP_LINEAR,
                             border_mode=BORDER_CONSTANT, border_value=0):
        """mi355_warp_perspective_dev: nframes frames of sw x sh at d_in through the 3 x 3 matrix m to dw x dh at d_out,
        bpp 4 (RGBA) or 1 (gray8); one launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_warp_perspective_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(bpp), int(sw), int(sh),
                                                  int(dw), int(dh), int(nframes), _matrix9(m), int(flags),
                                                  int(border_mode), int(border_value) & 0xFFFFFFFF)
        _check("mi355_warp_perspective_dev", rc, self._h)

    def adaptive_threshold_gray8_dev(self, d_in, d_out, w, h, nframes, max_value, type, block, delta):
        """mi355_adaptive_threshold_gray8_dev: nframes gray8 frames at d_in thresholded against their block x block mean
        into d_out; one launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_adaptive_threshold_gray8_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(w), int(h),
                                                          int(nframes), int(max_value), int(type), int(block),
                                                          float(delta))
        _check("mi355_adaptive_threshold_gray8_dev", rc, self._h)

    def clahe_gray8_dev(self, d_in, d_out, w, h, nframes, clip_limit=40.0, tiles_x=8, tiles_y=8):
        """mi355_clahe_gray8_dev: CLAHE of nframes gray8 frames at d_in to d_out, no synchronisation."""
        rc = self._lib.mi355_clahe_gray8_dev(self._h, _vp(int(d_in)), _vp(int(d_out)), int(w), int(h), int(nframes),
                                             float(clip_limit), int(tiles_x), int(tiles_y))
        _check("mi355_clahe_gray8_dev", rc, self._h)

    def clahe_luts_gray8_dev(self, d_in, d_luts, w, h, nframes, clip_limit=40.0, tiles_x=8, tiles_y=8):
        """mi355_clahe_luts_gray8_dev: the nframes x tiles_y x tiles_x x 256 table bytes of a CLAHE call to d_luts (4-byte
        aligned), no synchronisation."""
        rc = self._lib.mi355_clahe_luts_gray8_dev(self._h, _vp(int(d_in)), _vp(int(d_luts)), int(w), int(h),
                                                  int(nframes), float(clip_limit), int(tiles_x), int(tiles_y))
        _check("mi355_clahe_luts_gray8_dev", rc, self._h)

    def ccl_gray8_dev(self, d_in, d_labels, d_count, d_stats, d_sums, w, h, nframes, connectivity=8, stats_rows=0):
        """mi355_ccl_gray8_dev: labels (int32 per pixel) of nframes gray8 masks at d_in to d_labels, N per frame to
        d_count, and with stats_rows > 0 that many rows per frame of 5 int32 to d_stats and 2 uint64 to d_sums (both may
        be 0 / None otherwise); no synchronisation."""
        rc = self._lib.mi355_ccl_gray8_dev(self._h, _vp(int(d_in or 0)), _vp(int(d_labels or 0)), _vp(int(d_count or 0)),
                                           _vp(int(d_stats or 0)), _vp(int(d_sums or 0)), int(w), int(h), int(nframes),
                                           int(connectivity), int(stats_rows))
        _check("mi355_ccl_gray8_dev", rc, self._h)

    def dist_gray8_dev(self, d_in, d_sq, d_dist, d_nearest, w, h, nframes):
        """mi355_dist_gray8_dev: the distance transform of nframes gray8 masks at d_in: int32 squared distances to d_sq,
        float32 distances to d_dist, int32 nearest-site indices to d_nearest (each may be 0 / None, not all three); two
        launches, no synchronisation; the scratch (2 bytes per pixel) is pooled in the context."""
        rc = self._lib.mi355_dist_gray8_dev(self._h, _vp(int(d_in or 0)), _vp(int(d_sq or 0)), _vp(int(d_dist or 0)),
                                            _vp(int(d_nearest or 0)), int(w), int(h), int(nframes))
        _check("mi355_dist_gray8_dev", rc, self._h)

    def hysteresis_gray8_dev(self, d_in, d_out, w, h, nframes, low, high, connectivity=8):
        """mi355_hysteresis_gray8_dev: the hysteresis threshold of nframes gray8 response maps at d_in to d_out; up to
        five launches, no synchronisation; the parent array (4 bytes per pixel) is pooled in the context."""
        rc = self._lib.mi355_hysteresis_gray8_dev(self._h, _vp(int(d_in or 0)), _vp(int(d_out or 0)), int(w), int(h),
                                                  int(nframes), int(low), int(high), int(connectivity))
        _check("mi355_hysteresis_gray8_dev", rc, self._h)

    def canny_gray8_dev(self, d_in, d_out, w, h, nframes, threshold1, threshold2, flags=0):
        """mi355_canny_gray8_dev: cv::Canny (aperture 3) of nframes gray8 frames at d_in to d_out; up to six launches,
        no synchronisation; the parent array (4 bytes per pixel) is pooled in the context."""
        rc = self._lib.mi355_canny_gray8_dev(self._h, _vp(int(d_in or 0)), _vp(int(d_out or 0)), int(w), int(h),
                                             int(nframes), float(threshold1), float(threshold2), int(flags))
        _check("mi355_canny_gray8_dev", rc, self._h)

    def hough_accum_gray8_dev(self, d_in, d_accum, w, h, nframes, rho, theta, min_theta=0.0, max_theta=np.pi):
        """mi355_hough_accum_gray8_dev: the int32 accumulators (hough_accum_bytes) of nframes gray8 edge maps at d_in to
        d_accum; two launches behind a memset, no synchronisation."""
        rc = self._lib.mi355_hough_accum_gray8_dev(self._h, _vp(int(d_in or 0)), _vp(int(d_accum or 0)), int(w), int(h),
                                                   int(nframes), float(rho), float(theta), float(min_theta),
                                                   float(max_theta))
        _check("mi355_hough_accum_gray8_dev", rc, self._h)

    def hough_lines_gray8_dev(self, d_in, d_lines, d_votes, d_count, d_accum, w, h, nframes, rho, theta, threshold,
                              max_lines, min_theta=0.0, max_theta=np.pi):
        """mi355_hough_lines_gray8_dev: cv::HoughLines of nframes gray8 edge maps at d_in: (max_lines, 2) float32 rows per
        frame to d_lines, their votes to d_votes (0: not wanted), the peak counts to d_count; d_accum 0: the accumulator
        is pooled in the context.  Four launches behind two memsets, no synchronisation."""
        rc = self._lib.mi355_hough_lines_gray8_dev(
            self._h, _vp(int(d_in or 0)), _vp(int(d_lines or 0)), _vp(int(d_votes or 0)), _vp(int(d_count or 0)),
            _vp(int(d_accum or 0)), int(w), int(h), int(nframes), float(rho), float(theta), int(threshold),
            int(max_lines), float(min_theta), float(max_theta))
        _check("mi355_hough_lines_gray8_dev", rc, self._h)

    def hist_gray8_dev(self, d_in, d_hist, w, h, nframes):
        """mi355_hist_gray8_dev: nframes x 256 uint32 counts to d_hist (overwritten), no synchronisation."""
        rc = self._lib.mi355_hist_gray8_dev(self._h, _vp(int(d_in)), _vp(int(d_hist)), int(w), int(h), int(nframes))
        _check("mi355_hist_gray8_dev", rc, self._h)

    def otsu_thresholds_gray8_dev(self, d_in, d_thresh, w, h, nframes):
        """mi355_otsu_thresholds_gray8_dev: one int32 Otsu threshold per frame to d_thresh, no synchronisation."""
        rc = self._lib.mi355_otsu_thresholds_gray8_dev(self._h, _vp(int(d_in)), _vp(int(d_thresh)), int(w), int(h),
                                                       int(nframes))
        _check("mi355_otsu_thresholds_gray8_dev", rc, self._h)

    def synth_dev(self, d_out, w, h, nframes, first_frame=0, seed=0x5EED, mode=0):
        rc = self._lib.mi355_synth_rgba8_dev(self._h, _vp(int(d_out)), int(w), int(h), int(nframes),
                                             int(first_frame), ctypes.c_uint32(seed), int(mode))
        _check("mi355_synth_rgba8_dev", rc, self._h)

    def bgr_to_rgba_dev(self, d_bgr, d_rgba, w, h, nframes):
        """mi355_bgr_to_rgba8_dev: packed 3-byte BGR frames (any byte alignment) to RGBA with A = 255 (dword-aligned),
        no synchronisation."""
        rc = self._lib.mi355_bgr_to_rgba8_dev(self._h, _vp(int(d_bgr)), _vp(int(d_rgba)), int(w), int(h), int(nframes))
        _check("mi355_bgr_to_rgba8_dev", rc, self._h)

    def yuv_to_rgba8_dev(self, d_yuv, d_rgba, w, h, nframes, layout, standard=YUV_BT601, pitch=0, rows=0):
        """mi355_yuv_to_rgba8_dev: nframes YUV frames at d_yuv (any byte alignment) to RGBA at d_rgba (dword-aligned); one
        launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_yuv_to_rgba8_dev(self._h, _vp(int(d_yuv)), _vp(int(d_rgba)), int(w), int(h), int(nframes),
                                              int(layout), int(standard), int(pitch), int(rows))
        _check("mi355_yuv_to_rgba8_dev", rc, self._h)

    def rgba8_to_yuv_dev(self, d_rgba, d_yuv, w, h, nframes, layout, standard=YUV_BT601, pitch=0, rows=0):
        """mi355_rgba8_to_yuv_dev: nframes RGBA frames at d_rgba to 4:2:0 frames at d_yuv (any byte alignment; padding is
        not written); one launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_rgba8_to_yuv_dev(self._h, _vp(int(d_rgba)), _vp(int(d_yuv)), int(w), int(h), int(nframes),
                                              int(layout), int(standard), int(pitch), int(rows))
        _check("mi355_rgba8_to_yuv_dev", rc, self._h)

    def yuv_to_gray8_dev(self, d_yuv, d_gray, w, h, nframes, layout, pitch=0, rows=0):
        """mi355_yuv_to_gray8_dev: the luma bytes of nframes YUV frames, unchanged, to tightly packed (n, h, w) planes at
        d_gray; one launch, no synchronisation, no allocation."""
        rc = self._lib.mi355_yuv_to_gray8_dev(self._h, _vp(int(d_yuv)), _vp(int(d_gray)), int(w), int(h), int(nframes),
                                              int(layout), int(pitch), int(rows))
        _check("mi355_yuv_to_gray8_dev", rc, self._h)

    def checksum_dev(self, d_buf, nbytes, index_base=0):
        out = ctypes.c_uint64(0)
        rc = self._lib.mi355_checksum_dev(self._h, _vp(int(d_buf)), int(nbytes), ctypes.c_uint64(index_base),
                                          ctypes.byref(out))
        _check("mi355_checksum_dev", rc, self._h)
        return out.value

    def stream_copy_dev(self, d_dst, d_src, nbytes):
        rc = self._lib.mi355_stream_copy_dev(self._h, _vp(int(d_dst)), _vp(int(d_src)), int(nbytes))
        _check("mi355_stream_copy_dev", rc, self._h)

    def selftest(self):
        """(bad_luma, bad_mag): exhaustive on-device check of the fast luminance / magnitude forms; (0, 0) = good."""
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check("mi355_selftest", self._lib.mi355_selftest(self._h, ctypes.byref(a), ctypes.byref(b)), self._h)
        return a.value, b.value

    def pool_alloc(self, filt, w, h, nframes, k=5, sigma=1.5, tries=4):
        """(d_in, d_out, probe_ms): input (0xFF-filled) and output frame pools, the output pool placed by a short
        search over physical placements (see mi355_pool_alloc); release with pool_free."""
        a, b = _vp(), _vp()
        ms = (ctypes.c_float * max(1, tries))()
        rc = self._lib.mi355_pool_alloc(self._h, int(filt), int(w), int(h), int(nframes), int(k), float(sigma),
                                        int(tries), ctypes.byref(a), ctypes.byref(b), ms)
        _check("mi355_pool_alloc", rc, self._h)
        return a.value, b.value, [float(x) for x in ms][:max(1, tries)]

    def pool_free(self, d_in, d_out):
        _check("mi355_pool_free", self._lib.mi355_pool_free(self._h, _vp(int(d_in or 0)), _vp(int(d_out or 0))),
               self._h)

    def alloc(self, nbytes):
        p = _vp()
        _check("mi355_dev_alloc", self._lib.mi355_dev_alloc(self._h, int(nbytes), ctypes.byref(p)), self._h)
        return p.value

    def free(self, d_ptr):
        _check("mi355_dev_free", self._lib.mi355_dev_free(self._h, _vp(int(d_ptr))), self._h)

    def h2d(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        rc = self._lib.mi355_copy_h2d(self._h, _vp(int(d_dst)), _vp(arr.ctypes.data), arr.nbytes)
        _check("mi355_copy_h2d", rc, self._h)

    def d2h(self, arr, d_src):
        assert arr.flags["C_CONTIGUOUS"]
        rc = self._lib.mi355_copy_d2h(self._h, _vp(arr.ctypes.data), _vp(int(d_src)), arr.nbytes)
        _check("mi355_copy_d2h", rc, self._h)

    def timer_begin(self):
        _check("mi355_timer_begin", self._lib.mi355_timer_begin(self._h), self._h)

    def timer_end(self):
        ms = ctypes.c_float(0)
        _check("mi355_timer_end", self._lib.mi355_timer_end(self._h, ctypes.byref(ms)), self._h)
        return ms.value


def group_shard(member, nmembers, nframes):
    """(first_frame, count) of one member: mi355_group_shard, a pure host function (= bench.shard_range's strong split)."""
    a, b = _ci(0), _ci(0)
    _check("mi355_group_shard", load_library().mi355_group_shard(int(member), int(nmembers), int(nframes),
                                                                  ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


class Group:
    """mi355_group_*: one batch of frames sharded over several GPUs, one context + one host thread per member.
    `devices`: HIP ordinals, one per member (an ordinal may repeat: members then share that GPU)."""

    def __init__(self, devices):
        self._lib = load_library()
        self._h = _vp()
        devs = (_ci * len(devices))(*[int(d) for d in devices])
        _check("mi355_group_create", self._lib.mi355_group_create(len(devices), devs, ctypes.byref(self._h)))
        self.size = len(devices)

    def close(self):
        if self._h:
            self._lib.mi355_group_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, i):
        """A borrowed Context of member i (device memory, copies, checksums); do not close it."""
        h = _vp()
        _check("mi355_group_member_ctx", self._lib.mi355_group_member_ctx(self._h, int(i), ctypes.byref(h)))
        c = Context.__new__(Context)
        c._lib, c._h = self._lib, h
        c.close = lambda: None
        return c

    def member_status(self, i):
        return self._lib.mi355_group_member_status(self._h, int(i))

    def set_gauss_mode(self, mode):
        _check("mi355_group_set_gauss_mode", self._lib.mi355_group_set_gauss_mode(self._h, int(mode)))

    def set_impl(self, impl):
        _check("mi355_group_set_impl", self._lib.mi355_group_set_impl(self._h, int(impl)))

    def set_input_format(self, fmt):
        _check("mi355_group_set_input_format", self._lib.mi355_group_set_input_format(self._h, int(fmt)))
        self._in_ch = 3 if fmt == INPUT_BGR else 4

    def set_gauss_weights(self, k, sigma, table):
        table = np.ascontiguousarray(table, np.float32)
        rc = self._lib.mi355_group_set_gauss_weights(self._h, int(k), float(sigma), table.ctypes.data_as(_f32p))
        _check("mi355_group_set_gauss_weights", rc)

    def filter_batched(self, filt, frames, k=0, sigma=0.0, out=None):
        """Host frames (n, h, w, c), or (n, h, w) for the single-channel filters -> (out, elapsed_ms): every member
        streams its contiguous range."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w = _batch_shape(filt, frames, getattr(self, "_in_ch", 4))
        bpp = _out_bpp(filt)
        if out is None:
            out = np.empty((n, h, w, 4) if bpp == 4 else (n, h, w), np.uint8)
        ms = ctypes.c_double(0)
        rc = self._lib.mi355_group_filter_batched(self._h, int(filt), frames.ctypes.data_as(_u8p), out.ctypes.data_as(_u8p),
                                                  w, h, n, int(k), float(sigma), ctypes.byref(ms))
        _check("mi355_group_filter_batched", rc)
        return out, ms.value

    def filter_dev(self, filt, d_in, d_out, w, h, nframes, k=0, sigma=0.0):
        """Device-resident: d_in[m] / d_out[m] / nframes[m] per member; launches everywhere, returns when all are done."""
        m = self.size
        a = (_vp * m)(*[_vp(int(x or 0)) for x in d_in])
        b = (_vp * m)(*[_vp(int(x or 0)) for x in d_out])
        nf = (_ci * m)(*[int(x) for x in nframes])
        rc = self._lib.mi355_group_filter_dev(self._h, int(filt), a, b, int(w), int(h), nf, int(k), float(sigma))
        _check("mi355_group_filter_dev", rc)
