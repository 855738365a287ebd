// kernels.hpp — host-callable launchers of the gfx950 kernels (one .hip file each).
// All launchers enqueue on `stream` and return the hipError_t of the launch.
// The LDS-tiled kernels (gauss_tile, sobel_tile, gray8, morph, median, image2d) share their frame: tile_common.hpp;
// the register-resident sliding-window kernels theirs: slide_common.hpp; the kernels in which one wave walks one work
// item alone (box, resize, warp, remap) theirs: wave_common.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355 {

// Coefficients of one (k, sigma), device-resident, owned by the context.
//   w2d : k*k floats, the reference's table (RT/src/Controller.cpp:352-372), row-major.
//   w1d : k floats, the separable factor used by the FAST arithmetic:
//         w1d[i] = rowsum_i(w2d) / sqrt(sum(w2d)) evaluated in double, rounded to float.
struct GaussCoef {
    int k;
    const float* d_w2d;
    const float* d_w1d;
    float h_w1d[64];  // host copy, passed by value to the register-resident kernels
    const float* h_w2d;  // host copy of w2d (owned by the context), passed by value to the fused pipeline kernel
    // true when w2d == w1d (x) w1d up to float rounding, with non-negative entries: the FAST (separable) kernels
    // may stand in for the 2-D table.  Externally installed tables that are not (mi355_ctx_set_gauss_weights) are
    // applied tap by tap by the tiled kernels, as the reference kernel applies them (RT/kernel/gaussian_base.cl:23-44).
    bool separable;
    // alpha_tab[A] = (the FAST kernels' output byte for a channel whose whole window holds A) << 24: the canonical
    // separable chains on an all-A window, evaluated on the host with the same float operations
    // (gauss_const_alpha).  The constant-alpha fast path of the sliding-window kernels reads it.
    const uint32_t* d_alpha_tab;
    uint32_t h_alpha_tab[256];
    // alpha_cpu[A] = (the CPU path's byte for a channel whose whole k x k window holds A — its own k*k-term float chain,
    // src/GaussianBlur/GaussianBlur.cpp:243-256) << 16: what the matrix-core kernel stores for constant-alpha windows
    // (its alpha = 255 constant since round 2, now for every A).
    const uint32_t* d_alpha_cpu;
    uint32_t h_alpha_cpu[256];
};

// The FAST arithmetic's result for one channel of a pixel whose k x k window holds the value `a` everywhere:
// v = w[0]*a; v = fma(w[j], a, v) down the column, o = w[0]*v; o = fma(w[t], v, o) along the row,
// uchar(std::clamp(o, 0, 255)) — the kernels' own chain, so the byte is the one they would have computed.
uint32_t gauss_const_alpha(const float* w1d, int k, uint32_t a);

hipError_t launch_gray(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                       int nframes, bool one_channel);

// impl: 0 = choose, 1 = force the LDS-tiled kernel, 2 = the matrix-core kernel wherever it applies.
// d_flags: device scratch of gauss_flag_items(...) uint32 (one per work item of the two-kernel opaque/fallback
// scheme, see gauss_wide.hip); may be null when that returns 0.
size_t gauss_flag_items(const uint8_t* d_in, const uint8_t* d_out, int w, int h, int nframes, const GaussCoef& coef,
                        bool exact, int impl);
hipError_t launch_gauss(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                        int nframes, const GaussCoef& coef, bool exact, int impl, uint32_t* d_flags);

// the two implementations launch_gauss chooses between
hipError_t launch_gauss_tile(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                             int nframes, const GaussCoef& coef, bool exact);

// register-resident sliding-window kernel (k = 3,5,7,9; any width, dword-aligned pointers)
bool gauss_slide_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, int k);
size_t gauss_slide_flag_items(int w, int h, int nframes, int k);
hipError_t launch_gauss_slide(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                              int nframes, const GaussCoef& coef, uint32_t* d_flags);

// register-resident kernel for k = 11..17 (2 px per lane, LDS row exchange); width % 2 == 0, 8-byte aligned
bool gauss_wide_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, int k);
size_t gauss_wide_flag_items(int w, int h, int nframes, int k);
hipError_t launch_gauss_wide(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                             const GaussCoef& coef, uint32_t* d_flags);

// EXACT-mode sliding-window kernel (gauss_exact.hip): k in {3,5,7}, width % 4 == 0, 16-byte aligned buffers;
// bit-identical to the CPU path ("exact by exception")
bool gauss_exact_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, const GaussCoef& coef);
hipError_t launch_gauss_exact(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                              const GaussCoef& coef);

// matrix-core kernel (gauss_mfma_reg.hip): any odd k <= 17, width % 4 == 0, 16-byte aligned buffers, frames below
// 2 GiB, FAST arithmetic
bool gauss_mfma_reg_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, const GaussCoef& coef);
hipError_t launch_gauss_mfma_reg(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                                 const GaussCoef& coef);

// impl: 0 = choose (sliding window when width % 4 == 0 and buffers aligned), 1 = force the LDS-tiled kernel
hipError_t launch_sobel(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                        int nframes, int impl);
bool sobel_slide_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h);
hipError_t launch_sobel_slide(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes);

hipError_t launch_pipeline(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h,
                           int nframes, const GaussCoef& coef, bool exact, int impl);
// fused register-resident kernel (pipe_slide.hip), px pixels per lane.  px = 4: k in {3,5,7}, any width >= 4;
// px = 8: k in {3,5}, width % 8 == 0, aligned buffers; the same bits
bool pipe_slide_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, const GaussCoef& coef, int px);
hipError_t launch_pipe_slide(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                             const GaussCoef& coef, int px);

// single-channel (1 byte per pixel) filters (gray8.hip): any width, any byte alignment.  impl 1 (TILE) forces the
// runtime-k kernels and the CPU chain for every EXACT pixel; otherwise k in {3, 5, 7} runs with a constant k and both
// Gaussian modes exact by exception.  The pipeline's Gaussian is the EXACT one in both modes.
hipError_t launch_gauss_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                              const GaussCoef& coef, bool exact, int impl);
hipError_t launch_sobel_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes);
hipError_t launch_pipeline_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                                 const GaussCoef& coef, int impl);

// median filter (median.hip), cv::medianBlur semantics, odd k in 3..MI355_MAX_MEDIAN_K; gray8 = 1 byte per pixel (any
// byte alignment), else RGBA (dword-aligned).  impl 1 (TILE) forces the LDS counting kernel, which AUTO also takes for
// k = 7; k = 3 and 5 otherwise run the packed-u16 compare networks.
hipError_t launch_median(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                         bool gray8, int impl);

// rectangular morphology (morph.hip): op 0 erode, 1 dilate, 2 open, 3 close, k x k MORPH_RECT, odd k in
// 3..MI355_MAX_MORPH_K, clamp-to-edge borders; gray8 = 1 byte per pixel (any byte alignment), else RGBA (dword-aligned).
// One LDS-tiled kernel for every op and k, one launch per call (OPEN / CLOSE included); there is no impl choice.
hipError_t launch_morph(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                        int op, bool gray8);

// whole-frame statistics of single-channel frames (hist.hip): frame f is the flat byte range [f w h, (f + 1) w h),
// w * h < 2^31, any byte alignment.  launch_hist ADDS each frame's 256 bin counts into d_hist[f * 256 ..] (the caller
// zeroes it first; 4-byte aligned).
hipError_t launch_hist(hipStream_t stream, const uint8_t* d_in, uint32_t* d_hist, int w, int h, int nframes);
// one wave per frame: the 256-byte table of cv::equalizeHist (otsu false) or of the Otsu threshold (lut[v] = v > t ?
// 255 : 0) from 16-byte aligned histograms; d_lut (256 B per frame, 4-byte aligned) and d_thresh (Otsu's t per frame)
// may each be null
hipError_t launch_hist_table(hipStream_t stream, const uint32_t* d_hist, uint8_t* d_lut, int32_t* d_thresh, int w,
                             int h, int nframes, bool otsu);
// out byte = d_lut[f * 256 + in byte] for every pixel of frame f
hipError_t launch_lut_apply(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, const uint8_t* d_lut, int w, int h,
                            int nframes);

// CLAHE of single-channel frames (clahe.hip; semantics: include/mi355_imgfilter.h, "local contrast").  ClaheGeom is the
// call's geometry, computed once on the host: the tile size tw x th of the extended frame (tiles_x tw >= w, tiles_y th >=
// h, each pad served by one reflection, tiles_x tw tiles_y th < 2^31), the clip limit in counts (0 = none) and the three
// fp32 scales 255 / (tw th), 1 / tw and 1 / th, which go to the kernels by value.
//   launch_clahe_hist   ADDS every tile's 256 bin counts into d_hist[(f tiles + tile) * 256 ..] (tile = j tiles_x + i;
//                       the caller zeroes it first; 16-byte aligned)
//   launch_clahe_table  one wave per (frame, tile): clip, redistribute, prefix sum -> d_luts, 256 bytes per tile in the
//                       same order (4-byte aligned)
//   launch_clahe_apply  blends the four nearest tiles' table entries per pixel, d_luts 4-byte aligned
constexpr int kClaheMaxTiles = 16;
struct ClaheGeom {
    int w, h, tiles_x, tiles_y;
    int tw, th;
    int cl;
    float lut_scale, inv_tw, inv_th;
};
hipError_t launch_clahe_hist(hipStream_t stream, const uint8_t* d_in, uint32_t* d_hist, const ClaheGeom& g, int nframes);
hipError_t launch_clahe_table(hipStream_t stream, const uint32_t* d_hist, uint8_t* d_luts, const ClaheGeom& g,
                              int nframes);
hipError_t launch_clahe_apply(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, const uint8_t* d_luts,
                              const ClaheGeom& g, int nframes);

// cv::connectedComponentsWithStats of single-channel masks (ccl.hip; semantics: include/mi355_imgfilter.h, "the blobs of
// a mask"): frames of w * h < 2^31 pixels at any byte alignment, a pixel is foreground iff its byte is not zero.
// d_labels (int32 per pixel, 4-byte aligned) is the union-find parent array until the last launch; d_count takes N per
// frame; d_scratch takes ccl_scratch_bytes(): one count, then offset, per kCclFlatPx raster-consecutive pixels, nothing
// per pixel.  stats_rows 0 .. kCclMaxStatsRows rows per frame of d_stats (5 int32) and d_sums (2 uint64, 8-byte aligned),
// both unused (may be null) when it is 0.  Up to eight launches on the stream, no allocation, no wait.
constexpr int kCclFlatPx = 2048;
constexpr int kCclMaxStatsRows = 1 << 24;
size_t ccl_scratch_bytes(int w, int h, int nframes);  // 0 for sizes launch_ccl rejects
hipError_t launch_ccl(hipStream_t stream, const uint8_t* d_in, int32_t* d_labels, int32_t* d_count, int32_t* d_stats,
                      uint64_t* d_sums, uint32_t* d_scratch, int w, int h, int nframes, bool conn8, int stats_rows);
// The union launches of launch_ccl alone (local, seam, compress: up to three), with foreground = byte > low, 0 <= low <=
// 255 (launch_ccl itself runs them with low = 0).  Afterwards d_parent (int32 per pixel, 4-byte aligned) holds 0 for
// background and, for a foreground pixel q, a value a = (a pixel index of q's component) + 1 such that d_parent[a - 1] is
// q's root value; a root's entry is its own index + 1.  Every pixel reaches its root in two loads.
hipError_t launch_ccl_unite(hipStream_t stream, const uint8_t* d_in, int32_t* d_parent, int w, int h, int nframes,
                            bool conn8, int low);

// cv::Canny(aperture 3) and hysteresis thresholding of single-channel frames (canny.hip; semantics:
// include/mi355_imgfilter.h, "from gradients to edges"): frames of w * h < 2^31 pixels at any byte alignment.
//   launch_canny_nms   one launch: source bytes -> a class byte per pixel (0 none, 1 candidate, 2 strong); low and high
//                      are the integer thresholds on the magnitude (|dx| + |dy|, or dx^2 + dy^2 with l2)
//   launch_hysteresis  out = 255 where in > low and the pixel's component of such pixels holds one > high, else 0;
//                      0 <= low <= high <= 255.  Up to five launches: launch_ccl_unite into d_parent (4 B/px), mark,
//                      emit.  d_out may be d_in itself (every thread reads only the bytes it writes), and must not
//                      overlap it in any other way.  No allocation, no wait, nothing the host reads.
hipError_t launch_canny_nms(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int low,
                            int high, bool l2);
hipError_t launch_hysteresis(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int32_t* d_parent, int w, int h,
                             int nframes, int low, int high, bool conn8);

// cv::HoughLines of single-channel edge maps (hough.hip; semantics: include/mi355_imgfilter.h, "from edges to lines").
// The caller (capi.hip) derives numangle, numrho and the trig table on the host; d_tab holds numangle cosines * irho, then
// numangle sines * irho.  d_scratch: hough_scratch_bytes(g) bytes, 16-byte aligned (per-frame counters, then the point
// lists of the voting launch and the candidate lists of the selection, which share their bytes).
//   hough_plan          how a row of numrho cells is voted: up to kHoughBlockAngles whole rows per block while they fit
//                       kHoughLdsCells cells of LDS, else one angle per block and ceil(numrho / kHoughLdsCells) rho ranges
//                       of kHoughLdsCells cells; the fields are 0 for arguments no call accepts
//   launch_hough_accum  one memset node and two launches: the (numangle + 2) x (numrho + 2) int32 accumulator of every
//                       frame, the zero ring included
//   launch_hough_lines  one memset node and two launches: d_count = the peaks of d_accum above threshold, d_lines / d_votes
//                       (d_votes may be null) the first max_lines of them by votes descending, cell ascending, zero filled
// No allocation, no wait, nothing the host reads.
constexpr int kHoughMaxAngles = 1024;
constexpr int kHoughMaxLines = 4096;
constexpr int kHoughLdsCells = 36864;  // 144 KiB of the CU's 160: three rows of a 4K frame at rho = 1 (12 001 cells each)
constexpr int kHoughBlockAngles = 8;
struct HoughGeom {
    int w, h, nframes, numangle, numrho;
    float rho_f, theta_f, min_theta_f;
};
struct HoughPlan {
    int angles_per_block, rho_splits, span, lds_cells;
};
HoughPlan hough_plan(int numangle, int numrho);
size_t hough_scratch_bytes(const HoughGeom& g);  // 0 for a geometry the launches reject
hipError_t launch_hough_accum(hipStream_t stream, const uint8_t* d_in, int32_t* d_accum, const float* d_tab, void* d_scratch,
                              const HoughGeom& g);
hipError_t launch_hough_lines(hipStream_t stream, const int32_t* d_accum, float* d_lines, int32_t* d_votes, int32_t* d_count,
                              void* d_scratch, const HoughGeom& g, int threshold, int max_lines);

// cv::distanceTransform(DIST_L2, DIST_MASK_PRECISE) of single-channel masks (dist.hip; semantics:
// include/mi355_imgfilter.h, "how far from the background"): frames of 1 .. kDistMaxDim pixels a side at any byte
// alignment, a pixel is a site iff its byte is zero.  d_sq (int32), d_dist (float) and d_nearest (int32), each 4-byte
// aligned and each optional (at least one is not null), take one entry per pixel.  d_scratch takes dist_scratch_bytes():
// the signed row offset to the nearest site of the pixel's own column, one int16 per pixel, rows padded to four entries.
// Two launches on the stream (columns, rows), no allocation, no wait, nothing the host reads.  dist_col_lds_bytes is the
// LDS of the column launch for a frame of h rows (it grows with h: 144 KiB at kDistMaxDim); 0 for an h no call accepts.
constexpr int kDistMaxDim = 16384;
int dist_col_lds_bytes(int h);
size_t dist_scratch_bytes(int w, int h, int nframes);  // 0 for sizes launch_dist rejects
hipError_t launch_dist(hipStream_t stream, const uint8_t* d_in, int32_t* d_sq, float* d_dist, int32_t* d_nearest,
                       int16_t* d_scratch, int w, int h, int nframes);

// cv::resize of tightly packed 8-bit frames (resize.hip): bpp 4 (RGBA, dword-aligned) or 1 (gray8, any byte alignment);
// interp 0 nearest, 1 linear (11-bit fixed point; AREA's result at exactly half size), 3 area with integer factors
// 1 .. kResizeMaxAreaFactor (resize_area_factors says whether a size pair has them; anything else is
// hipErrorInvalidValue).  Scales go to the kernel by value: no table, no allocation, one launch.
constexpr int kResizeMaxAreaFactor = 16;
bool resize_area_factors(int src_w, int src_h, int dst_w, int dst_h, int* nx, int* ny);
hipError_t launch_resize(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                         int dst_w, int dst_h, int nframes, int interp);

// cv::warpAffine of tightly packed 8-bit frames (warp.hip): bpp 4 (RGBA, dword-aligned) or 1 (gray8, any byte alignment);
// interp 0 nearest, 1 linear (10-bit fixed-point coordinates, 1/32-pixel weights); border_mode 0 constant (border_value:
// the pixel's four bytes in memory order, gray8 its low byte), 1 replicate.  inv maps an output pixel to its source
// position (the caller inverts; the bound of the header's "Limits" holds).  The six doubles and the sizes go to the kernel
// by value: no table, no allocation, one launch.  A wave owns a tile of output pixels, 4 per lane: the wide tile (64 x 16)
// while a 64-pixel output row crosses at most kWarpWideMaxRows source rows (|inv[3]| * 64: identity, shifts, scales, a
// deskew by a degree or two), the square tile (32 x 32) for every steeper map.  Both shapes and the rule are measured
// choices (profiles/warp_rate.txt).  warp_work_items is the number of tiles (a launch takes fewer than 2^31).
constexpr int kWarpMaxSize = 32766;
constexpr int kWarpWideLanesLog2 = 4;    // 16 lanes of 4 pixels side by side
constexpr int kWarpWideH = 16;
constexpr int kWarpSquareLanesLog2 = 3;  // 8 lanes of 4 pixels side by side
constexpr int kWarpSquareH = 32;
constexpr double kWarpWideMaxRows = 3.0;
bool warp_tile_is_wide(const double inv[6]);
uint64_t warp_work_items(const double inv[6], int dst_w, int dst_h, int nframes);
hipError_t launch_warp_affine(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                              int dst_w, int dst_h, int nframes, const double inv[6], int interp, int border_mode,
                              uint32_t border_value);

// cv::remap and cv::warpPerspective of tightly packed 8-bit frames (remap.hip), with the frame, interp and border rules
// of launch_warp_affine.  launch_remap: one map of dst_w x dst_h entries for all frames; map_kind 0 (FIXED) takes int16
// (sx, sy) pairs at d_map1 (dword-aligned) and uint16 fy*32+fx at d_map2 (2-byte aligned; may be null for NEAREST),
// map_kind 1 (FLOAT) takes the x plane and the y plane (both dword-aligned).  launch_warp_perspective: inv maps an
// output pixel to its source position (the caller inverts); the nine doubles go to the kernel by value.  No table, no
// allocation, one launch each.  A wave owns a tile of output pixels, 4 per lane, across kRemapFrames consecutive frames
// (the map entry or the division is paid once per chunk), and votes per row pass whether it needs border tests.  The
// tile (32 x 32, warp.hip's square tile) and kRemapFrames are measured choices (profiles/remap_rate.txt): 4 frames are
// the best candidate or within 2.5 % of it for every map and save up to 38 % on a keystone, at up to 7 % on a homography
// that is a steep turn; the square tile beats the wide one on RGBA and on every turned map.
// remap_work_items is the number of work items of a launch (a launch takes fewer than 2^31).
constexpr int kRemapLanesLog2 = 3;  // 8 lanes of 4 pixels side by side
constexpr int kRemapTileH = 32;
constexpr int kRemapFrames = 4;  // frames per work item
uint64_t remap_work_items(int dst_w, int dst_h, int nframes);
hipError_t launch_remap(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                        int dst_w, int dst_h, int nframes, const void* d_map1, const void* d_map2, int map_kind,
                        int interp, int border_mode, uint32_t border_value);
hipError_t launch_warp_perspective(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w,
                                   int src_h, int dst_w, int dst_h, int nframes, const double inv[9], int interp,
                                   int border_mode, uint32_t border_value);

// cv::blur with BORDER_REPLICATE (box.hip): k x k mean, odd k in 3..MI355_MAX_BOX_K, every channel on its own; gray8 = 1
// byte per pixel (any byte alignment), else RGBA (dword-aligned).  One register-resident running-sum kernel for every k:
// no table, no scratch, one launch.
hipError_t launch_box(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                      bool gray8);
// cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) of gray8 frames, the same kernel with a compare behind the mean:
// out = (src - mean > -idelta) ? max_value : 0, or with `inverse` (src - mean <= -idelta) ? max_value : 0; one launch
hipError_t launch_adaptive_threshold(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                                     int block, int max_value, bool inverse, int idelta);

// image2d_t-mode semantics of the reference (image2d.hip): filter 0 gray / 2 gauss / 3 sobel
hipError_t launch_image2d(hipStream_t stream, int filter, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                          int k, const float* d_table);

hipError_t launch_synth(hipStream_t stream, uint8_t* d_out, int w, int h, int nframes,
                        int first_frame, uint32_t seed, int mode);

// packed BGR (3 B/px) -> RGBA (A = 255), cv::cvtColor(BGR2RGBA)
hipError_t launch_bgr_to_rgba(hipStream_t stream, const uint8_t* d_bgr, uint8_t* d_rgba, size_t npx);

// 8-bit YUV frames <-> RGBA and their luma planes (yuv.hip; semantics: include/mi355_imgfilter.h, "frames from a decoder
// or a camera").  YuvFrames is a call's surface with pitch and rows resolved (never 0) and checked by the caller: layout
// 0 NV12, 1 NV21, 2 I420, 3 YV12 (4:2:0: w, h, rows even, planar pitch even), 4 YUY2, 5 UYVY (packed, 2 bytes per pixel).
// The coefficients go to the kernels by value; ybias = 2^19 + (YOFF << 20).  d_rgba is dword-aligned; d_yuv and d_gray
// take any byte alignment.  One launch each; no table, no scratch, no allocation.  Only pixel bytes are stored: the
// padding of a pitched surface is never written.  launch_rgba_to_yuv takes the 4:2:0 layouts only.
struct YuvFrames {
    int layout, w, h, nframes, pitch, rows;
};
struct YuvDecodeCoef {
    int yoff, cy, cvr, cvg, cug, cub;
};
struct YuvEncodeCoef {
    int cry, cgy, cby, cru, cgu, cbu, cgv, cbv, ybias;
};
inline bool yuv_layout_packed(int layout) { return layout >= 4; }
size_t yuv_frame_size(const YuvFrames& s);  // bytes from one frame to the next
hipError_t launch_yuv_to_rgba(hipStream_t stream, const uint8_t* d_yuv, uint8_t* d_rgba, const YuvFrames& s,
                              const YuvDecodeCoef& c);
hipError_t launch_rgba_to_yuv(hipStream_t stream, const uint8_t* d_rgba, uint8_t* d_yuv, const YuvFrames& s,
                              const YuvEncodeCoef& c);
hipError_t launch_yuv_to_gray(hipStream_t stream, const uint8_t* d_yuv, uint8_t* d_gray, const YuvFrames& s);

// streaming device-to-device copy (non-temporal, 16 B/lane): the on-box "read N + write N bytes" ceiling
hipError_t launch_stream_copy(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, size_t nbytes);

// *d_acc += order-independent checksum of nbytes at d_buf (see include/mi355_imgfilter.h)
hipError_t launch_selftest(hipStream_t stream, unsigned long long* d_acc);
hipError_t launch_checksum(hipStream_t stream, const uint8_t* d_buf, size_t nbytes,
                           uint64_t index_base, unsigned long long* d_acc);

}  // namespace mi355
