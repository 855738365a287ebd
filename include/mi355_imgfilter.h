/*
 * mi355_imgfilter.h — C-ABI of libmi355_imgfilter.so, the MI355X (gfx950) image-filter hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Every entry point
 * names the reference interface it replaces (paths relative to the reference repository root;
 * RT/ = src/RealtimeImageProcessing/).  The C++ classes in host/ (Controller, ProgramHandler)
 * forward to these functions; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Pixel layout everywhere: interleaved 8-bit RGBA, row-major, tightly packed (stride = 4*width),
 * as produced by cv::cvtColor(BGR2RGBA) at RT/src/ProgramHandler.cpp:127.
 *
 * Conventions: every function returns MI355_OK (0) or a negative MI355_ERR_* code; nothing throws,
 * nothing calls exit().  A context is bound to one GPU and one HIP stream and must be used from one
 * host thread at a time (the reference Controller is single-threaded too: include/Controller.hpp:50).
 * There is no CPU fallback: without a usable gfx950 device mi355_ctx_create fails.
 */
#ifndef MI355_IMGFILTER_H
#define MI355_IMGFILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK 0
#define MI355_ERR_BAD_ARG (-1)     /* null pointer, non-positive size, even/oversized kernel_size */
#define MI355_ERR_HIP (-2)         /* a HIP runtime call failed; see mi355_last_hip_error */
#define MI355_ERR_NO_DEVICE (-3)   /* no GPU / device index out of range */
#define MI355_ERR_UNSUPPORTED (-4) /* request outside what the kernels implement */
#define MI355_ERR_NOMEM (-5)

/* Largest Gaussian kernel_size accepted (odd).  The reference's own default is 17
 * (include/ProgramHandler.hpp:9). */
#define MI355_MAX_GAUSS_K 63

/* Gaussian arithmetic selection (mi355_ctx_set_gauss_mode):
 *   FAST  — separable, FMA, vertical pass then horizontal pass; within +-1 LSB per channel of the
 *           reference CPU path (src/GaussianBlur/GaussianBlur.cpp:234-261).  Default.
 *   EXACT — the reference CPU path's own arithmetic (k*k taps, ky outer / kx inner, separate float
 *           multiply and add, truncation): bit-identical output, several times slower. */
#define MI355_GAUSS_FAST 0
#define MI355_GAUSS_EXACT 1

typedef struct mi355_ctx mi355_ctx;

/* ---- context -------------------------------------------------------------------------------
 * Replaces the OpenCL bootstrap of Controller (RT/src/Controller.cpp:13-197: GetPlatforms,
 * GetDevices, CreateContext, CreateCommandQueue w/ CL_QUEUE_PROFILING_ENABLE :118, CreateProgram,
 * CreateKernel).  One context = {HIP device, stream, timing events, pooled device/pinned staging
 * buffers, cached Gaussian coefficient table}.  The reference allocates and frees device buffers on
 * every call (:234-244, :515-516); the pool here grows to the largest frame seen and is reused. */
int mi355_device_count(int* count);
int mi355_ctx_create(int device, mi355_ctx** out);
/* Same, but launches on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)
 * so the caller's stream-ordered allocator and events see the kernels. */
int mi355_ctx_create_on_stream(int device, void* hip_stream, mi355_ctx** out);
int mi355_ctx_destroy(mi355_ctx* ctx);
int mi355_ctx_device_name(mi355_ctx* ctx, char* buf, size_t buflen);
int mi355_sync(mi355_ctx* ctx);
int mi355_last_hip_error(mi355_ctx* ctx);
const char* mi355_strerror(int code);

int mi355_ctx_set_gauss_mode(mi355_ctx* ctx, int mode);

/* Kernel selection (a tuning / test knob):
 *   AUTO — the fastest kernel that applies.  Gaussian, FAST mode: the register-resident sliding-window kernels for
 *          k in {3,5} (any width); the matrix-core kernel for odd 7 <= k <= 17 when width % 4 == 0, width >= 64,
 *          the launch has >= 2^16 pixels and the device buffers are 16-byte aligned, the VALU kernels otherwise
 *          (k in {7,9} any width; k in {11,13,15,17} with an even width); the LDS-tiled kernel for everything else.
 *          EXACT mode: the exact-by-exception sliding kernel for k in {3,5,7} and width % 4 == 0, the tiled kernel
 *          otherwise.  Pipeline: k in {3,5,7}, w >= 4, h >= 2 sliding (8 pixels per lane for k = 5 launches of
 *          >= 10^9 pixels with width % 8 == 0), tiled otherwise.
 *          Single-channel filters (MI355_FILTER_*_GRAY8): k in {3,5,7} with a constant k, both Gaussian modes
 *          exact by exception; the runtime-k kernel otherwise.
 *   TILE — always the LDS-tiled kernels (for the single-channel filters: runtime k, EXACT pixels by the CPU chain).
 *   VALU — as AUTO but never the matrix cores.  TILE and VALU give identical bits. */
#define MI355_IMPL_AUTO 0
#define MI355_IMPL_TILE 1
/*   MFMA — the Gaussian on the matrix cores (csrc/gauss_mfma_reg.hip) wherever it applies (FAST mode, odd k <= 17,
 *          width % 4 == 0, 16-byte aligned device buffers); AUTO elsewhere.  Within 1 LSB of the CPU path like every
 *          FAST kernel, but not bit-identical to the VALU kernels (other rounding). */
#define MI355_IMPL_MFMA 2
#define MI355_IMPL_VALU 3
int mi355_ctx_set_impl(mi355_ctx* ctx, int impl);

/* Input pixel format of the HOST-buffer calls (mi355_*_rgba8, mi355_filter_batched, mi355_filter_stream):
 *   RGBA — 4 bytes per pixel, what the reference hands its Controller after cv::cvtColor(BGR2RGBA)
 *          (RT/src/ProgramHandler.cpp:127).  Default.
 *   BGR  — 3 bytes per pixel, tightly packed, as cv::imread / the camera deliver frames
 *          (RT/src/ProgramHandler.cpp:116, RT/RealtimeImageProcessing.cpp:325) and as the reference's CPU
 *          grayscale reads them (src/Grayscale/grayscale.cpp:234-236).  The frame crosses PCIe as 3 B/px and a
 *          device kernel performs the BGR2RGBA expansion (A = 255) ahead of the filter: 25 % less H2D traffic
 *          on a path that is PCIe-bound, and no host-side cvtColor.  Results equal the RGBA path on the
 *          converted frame.  Device-resident calls always take RGBA; mi355_bgr_to_rgba8_dev is the converter. */
#define MI355_INPUT_RGBA 0
#define MI355_INPUT_BGR 1
int mi355_ctx_set_input_format(mi355_ctx* ctx, int format);
int mi355_bgr_to_rgba8_dev(mi355_ctx* ctx, const void* d_bgr, void* d_rgba, int w, int h, int nframes);

/* ---- Gaussian coefficients -----------------------------------------------------------------
 * mi355_gauss_weights replaces Controller::_GenerateGaussianKernelBuffers
 * (RT/src/Controller.cpp:352-372 = src/GaussianBlur/src/Controller.cpp:342-362): k*k floats,
 * row-major [(y+k/2)*k + (x+k/2)], same promotion chain (float argument, exp in double, divide by
 * the double 2*M_PI*sigma^2, store float, float running sum, divide by it).  Pure host function.
 * The reference regenerates and re-uploads the table on every frame (:667,:674, leaking the
 * cl_mem); here the table is cached per (k, sigma) inside the context.
 *
 * mi355_ctx_set_gauss_weights installs an externally supplied k*k table (multi-GPU mode: rank 0
 * generates it, RCCL broadcasts it, every rank installs the same bytes) for the given (k, sigma)
 * key; later calls with that (k, sigma) use it instead of regenerating.  The table is applied as given: when it
 * is not w (x) w for one non-negative vector w up to float rounding (a non-separable or asymmetric table, negative
 * lobes), the separable FAST kernels do not apply and every call with that key runs the tap-by-tap (EXACT
 * arithmetic) kernel, as the reference kernel would (RT/kernel/gaussian_base.cl:23-44).  Non-finite entries are
 * rejected (MI355_ERR_BAD_ARG).  Installed tables are never evicted (at most 64 per context, one more is
 * MI355_ERR_BAD_ARG); of the tables the library generates itself a context keeps the 16 most recently used.  The
 * first call with a new (k, sigma) key — and mi355_ctx_set_gauss_weights itself — synchronises the context's stream
 * (allocation + blocking upload of the table); calls with a cached key do not. */
int mi355_gauss_weights(int k, float sigma, float* out_k2);
int mi355_ctx_set_gauss_weights(mi355_ctx* ctx, int k, float sigma, const float* w_k2);

/* ---- host-buffer calls: what Controller::PerformCL* forwards to ----------------------------
 * Each call = H2D, one kernel, D2H, synchronous on return, exactly like the reference
 * (RT/src/Controller.cpp:429-519, :521-613, :615-744).  prof_ns (may be NULL) receives the six
 * timestamps the reference appends to profiling_events via _profileEvent (:66-74, :471,:489,:513):
 * write-start, write-end, kernel-start, kernel-end, read-start, read-end, in ns on one clock.
 *
 * mi355_gray_rgba8     replaces PerformCLImageGrayscaling (buffer mode): out = w*h*4 bytes,
 *                      (g,g,g,255) per pixel.  g follows the CPU path src/Grayscale/grayscale.cpp:237
 *                      (double arithmetic, truncation) bit-exactly — not the float kernel
 *                      RT/kernel/grayscale_base.cl:14.
 * mi355_gray1_rgba8    same gray value, one byte per pixel (the CPU path's output shape,
 *                      grayscale.cpp:216).
 * mi355_gauss_rgba8    replaces PerformCLGaussianBlur: out = w*h*4 bytes; clamp-to-edge taps, all
 *                      four channels, truncation; semantics of the CPU path GaussianBlur.cpp:234-261
 *                      (no division by the accumulated weight, unlike gaussian_base.cl:48).
 * mi355_sobel_rgba8    replaces PerformCLImageEdgeDetection: out = w*h bytes.  Semantics of the CPU
 *                      path src/EdgeDetection/EdgeDetection.cpp:219-240 applied to
 *                      gray = grayscale.cpp:237 of each pixel: 3x3 correlation, BORDER_REFLECT_101,
 *                      float magnitude, round-half-even, saturate — every pixel written (the OpenCL
 *                      kernel edge_base.cl:12 leaves the border unwritten).
 * mi355_pipeline_rgba8 fused gray -> Gaussian -> Sobel, defined as the exact composition of the three
 *                      calls above (SURVEY.md §8a "a-pipe"): out = w*h bytes. */
int mi355_gray_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out_rgba, int w, int h,
                     uint64_t prof_ns[6]);
int mi355_gray1_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out_gray, int w, int h,
                      uint64_t prof_ns[6]);
int mi355_gauss_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out_rgba, int w, int h, int k,
                      float sigma, uint64_t prof_ns[6]);
int mi355_sobel_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out_gray, int w, int h,
                      uint64_t prof_ns[6]);
int mi355_pipeline_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out_gray, int w, int h, int k,
                         float sigma, uint64_t prof_ns[6]);

/* ---- image2d_t mode ---------------------------------------------------------
 * What the reference computes when image support is NOT bypassed (BYPASS_IMAGE_SUPPORT = false; no shipped
 * application does that): its *_images.cl kernels and the host code around them, which differ from the buffer path
 * in WHAT they compute —
 *   MI355_FILTER_GRAY   RT/kernel/grayscale_images.cl:15-22 + Controller.cpp:256-258,76-85: fp32 luminance of the
 *                       normalised texel, R/FLOAT image, host truncation of f * 255       -> out = w*h bytes
 *   MI355_FILTER_GAUSS  RT/kernel/gaussian_images.cl:1-36 + Controller.cpp:374-403: taps outside the image read the
 *                       border colour 0 (CLK_ADDRESS_CLAMP), no renormalisation, the image-mode table (its last row
 *                       and column are 0), round-to-nearest into UNORM_INT8              -> out = w*h*4 bytes
 *   MI355_FILTER_SOBEL  RT/kernel/edge_images.cl:3-47: RED channel only, interior pixels only (border 0), magnitude
 *                       clamped to [0, 1], host truncation of f * 255                     -> out = w*h bytes
 * Same call shape and profiling contract as the buffer-mode calls.  mi355_gauss_weights_image2d is the image-mode
 * table generator (Controller::_GenerateGaussianKernelImage2D), bit-identical to the reference's. */
int mi355_image2d_rgba8(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w, int h, int k,
                        float sigma, uint64_t prof_ns[6]);
int mi355_gauss_weights_image2d(int k, float sigma, float* out_k2);

/* Batched host-buffer form: nframes frames back to back in `rgba` and in `out`; one H2D, one launch
 * (grid.z-style frame index), one D2H.  filter: MI355_FILTER_*. */
#define MI355_FILTER_GRAY 0     /* RGBA -> RGBA (g,g,g,255) */
#define MI355_FILTER_GRAY1 1    /* RGBA -> 1 byte            */
#define MI355_FILTER_GAUSS 2    /* RGBA -> RGBA              */
#define MI355_FILTER_SOBEL 3    /* RGBA -> 1 byte            */
#define MI355_FILTER_PIPELINE 4 /* RGBA -> 1 byte            */
/* Single-channel filters: 1 byte per pixel in, 1 byte per pixel out, frames tightly packed (stride = width) — a mono
 * camera frame, the luma plane of a decoded video frame, a cv::Mat read with cv::IMREAD_GRAYSCALE, a torch (N, H, W)
 * uint8 tensor, or this library's own GRAY1 output.  Device buffers may have any byte alignment and any width >= 1
 * (the dword alignment rule of the RGBA filters does not apply).  The host-buffer calls return MI355_ERR_UNSUPPORTED
 * under MI355_INPUT_BGR: a gray plane is never converted.  mi355_image2d_rgba8 does not take these ids.
 *   GAUSS_GRAY8     src/GaussianBlur/GaussianBlur.cpp:234-261 on one channel: clamp-to-edge taps, the same table,
 *                   truncation — the R channel of mi355_gauss_rgba8 of (y, y, y, 255).  EXACT mode is bit-identical
 *                   to it, FAST mode within 1 LSB (bit-identical too for k in {3, 5, 7} outside MI355_IMPL_TILE).  Any
 *                   odd k <= MI355_MAX_GAUSS_K; an installed non-separable table is applied tap by tap.
 *   SOBEL_GRAY8     src/EdgeDetection/EdgeDetection.cpp:219-240 on the given plane itself (the reference reads it with
 *                   cv::IMREAD_GRAYSCALE, :202): filter2D CV_32F with BORDER_REFLECT_101, magnitude, convertTo CV_8U.
 *                   No luminance step — unlike MI355_FILTER_SOBEL, whose luminance of (v, v, v) is v - 1 for 65 byte
 *                   values.
 *   PIPELINE_GRAY8  SOBEL_GRAY8 of the EXACT-mode GAUSS_GRAY8, bit-identical to that chain in both Gaussian modes.
 *                   Deliberately NOT MI355_FILTER_PIPELINE on (y, y, y, 255): the input is already a gray plane, so no
 *                   luminance is re-applied. */
#define MI355_FILTER_GAUSS_GRAY8 5    /* 1 byte -> 1 byte */
#define MI355_FILTER_SOBEL_GRAY8 6    /* 1 byte -> 1 byte */
#define MI355_FILTER_PIPELINE_GRAY8 7 /* 1 byte -> 1 byte */
/* Median filter, cv::medianBlur(src, dst, k): every channel on its own (alpha included), a k x k window with clamp-to-edge
 * (BORDER_REPLICATE) borders — the clamp of the CPU Gaussian — and the middle one of the k*k values.  The output is an
 * input byte, so every implementation is bit-identical; there is no rounding contract.  Frames are independent (a
 * window never reads a neighbouring frame).  k must be 3, 5 or 7 (MI355_MAX_MEDIAN_K), anything else is
 * MI355_ERR_BAD_ARG; sigma is ignored and no weight table is made; the Gaussian mode does not apply.  Kernels: AUTO,
 * VALU and MFMA all choose the packed 16-bit compare networks for k in {3, 5} and the LDS counting kernel for k = 7;
 * MI355_IMPL_TILE forces the counting kernel for every k.
 *   MEDIAN        RGBA -> RGBA, dword-aligned device buffers; takes BGR host frames (expanded to RGBA, A = 255) under
 *                 MI355_INPUT_BGR.
 *   MEDIAN_GRAY8  1 byte -> 1 byte with the single-channel rules above (any byte alignment, UNSUPPORTED under BGR).
 * The ids start at 16, leaving 8-15 unassigned: id 8 has always been rejected, and callers (this library's own tests
 * among them) rely on the first ids after the gray8 block staying invalid. */
#define MI355_MAX_MEDIAN_K 7
#define MI355_FILTER_MEDIAN 16       /* RGBA -> RGBA     */
#define MI355_FILTER_MEDIAN_GRAY8 17 /* 1 byte -> 1 byte */
/* Rectangular grey-level morphology with a k x k MORPH_RECT element anchored at the centre:
 *   ERODE  = cv::erode(src, dst, rect)             min over the window
 *   DILATE = cv::dilate(src, dst, rect)            max over the window
 *   OPEN   = cv::morphologyEx(MORPH_OPEN, rect)   = DILATE(ERODE(x)), the same k
 *   CLOSE  = cv::morphologyEx(MORPH_CLOSE, rect)  = ERODE(DILATE(x)), the same k
 * Every channel is filtered on its own (alpha included).  Borders clamp to the edge (BORDER_REPLICATE); for a
 * rectangle and a min or a max this is the same as OpenCV's default border for erode and dilate, which leaves the
 * outside out of the window (the clipped window), because a clamped window holds only values of the clipped one.
 * OPEN / CLOSE treat the intermediate frame as a full frame with its own clamp-to-edge border: outside the frame it is
 * the intermediate at the clamped position, not the first stage extended past the edge.  Frames are independent.  The
 * output is an input byte, so there is no rounding contract.  k must be odd with 3 <= k <= MI355_MAX_MORPH_K, anything
 * else is MI355_ERR_BAD_ARG; sigma is ignored and no table is made; the Gaussian mode does not apply.  OPEN / CLOSE run
 * as one launch with no intermediate frame in device memory.  One kernel serves every id and k: the impl knob
 * (MI355_IMPL_*) does not affect these ids.
 *   ERODE, DILATE, OPEN, CLOSE  RGBA -> RGBA, dword-aligned device buffers; take BGR host frames (expanded to RGBA,
 *                               A = 255) under MI355_INPUT_BGR.
 *   *_GRAY8                     1 byte -> 1 byte with the single-channel rules above (any byte alignment, UNSUPPORTED
 *                               under BGR).
 * The ids are 24-31, leaving 18-23 unassigned: as with 8-15 after the gray8 block, callers (this library's own tests
 * among them) rely on id 18, the first after the median block, staying invalid. */
#define MI355_MAX_MORPH_K 17
#define MI355_FILTER_ERODE 24        /* RGBA -> RGBA     */
#define MI355_FILTER_DILATE 25       /* RGBA -> RGBA     */
#define MI355_FILTER_OPEN 26         /* RGBA -> RGBA     */
#define MI355_FILTER_CLOSE 27        /* RGBA -> RGBA     */
#define MI355_FILTER_ERODE_GRAY8 28  /* 1 byte -> 1 byte */
#define MI355_FILTER_DILATE_GRAY8 29 /* 1 byte -> 1 byte */
#define MI355_FILTER_OPEN_GRAY8 30   /* 1 byte -> 1 byte */
#define MI355_FILTER_CLOSE_GRAY8 31  /* 1 byte -> 1 byte */
/* Whole-frame statistics of single-channel frames, OpenCV's plain C++ path (not its IPP or OpenCL paths).  Both ids
 * follow the single-channel rules above (tightly packed, any byte alignment, any width >= 1, UNSUPPORTED under BGR);
 * k and sigma are ignored and no table is made.  Each frame is its own image: its histogram never includes a
 * neighbouring frame.  A call whose w * h is 2^31 or more is MI355_ERR_BAD_ARG (OpenCV counts pixels in an int).
 * hist = the frame's 256 bin counts, total = w * h.
 *   EQUALIZE_GRAY8  cv::equalizeHist.  i0 = the first bin with a nonzero count.  If hist[i0] == total every output
 *                   byte is i0.  Otherwise, in fp32 with no fused multiply-add: scale = 255.f / (float)(total -
 *                   hist[i0]); lut[i0] = 0; for i > i0: sum += hist[i] (int), lut[i] = saturate_u8(rint_half_even(
 *                   (float)sum * scale)).  Output byte = lut[input byte].
 *   OTSU_GRAY8      cv::threshold(src, dst, 0, 255, THRESH_BINARY | THRESH_OTSU).  The threshold t is OpenCV's fp64
 *                   loop, operation by operation, no fused multiply-add, left to right:
 *                     scale = 1.0 / (double)(w*h);  mu = sum_i i*(double)hist[i];  mu *= scale
 *                     mu1 = q1 = max_sigma = 0;  t = 0
 *                     for i in 0..255:
 *                         p = hist[i]*scale;  mu1 *= q1;  q1 += p;  q2 = 1.0 - q1
 *                         if min(q1,q2) < FLT_EPSILON or max(q1,q2) > 1.0 - FLT_EPSILON: continue
 *                         mu1 = (mu1 + i*p) / q1;  mu2 = (mu - q1*mu1) / q2
 *                         sigma = q1*q2*(mu1-mu2)*(mu1-mu2)
 *                         if sigma > max_sigma: max_sigma = sigma; t = i
 *                   Output byte = src > t ? 255 : 0.  Two quirks of that loop are kept: on a `continue` mu1 has been
 *                   multiplied by q1 and not divided again (visible only when a bin holds less than FLT_EPSILON of
 *                   the frame, i.e. frames of more than 2^23 pixels), and empty bins between occupied ones can move
 *                   sigma in its last bits, where the strict > decides the winner.  A constant frame has t = 0.
 * Three launches per call (histogram, table, apply) on the context's stream.  The scratch (1 KiB of histogram and
 * 256 B of table per frame) is pooled in the context: after the first call for a given frame count a call allocates
 * nothing and waits for nothing.  The impl knob (MI355_IMPL_*) does not affect these ids.
 * The ids are 40 and 41, leaving 32-39 unassigned: id 42, the first after this block, stays invalid as callers expect.
 * mi355_hist_gray8_dev and mi355_otsu_thresholds_gray8_dev (device-resident calls, below) expose the two steps. */
#define MI355_FILTER_EQUALIZE_GRAY8 40 /* 1 byte -> 1 byte */
#define MI355_FILTER_OTSU_GRAY8 41     /* 1 byte -> 1 byte */
/* Box mean: cv::blur(src, dst, Size(k, k), Point(-1, -1), BORDER_REPLICATE).  Every channel on its own, alpha included;
 * the window is k x k, centred, with clamp-to-edge borders (the Gaussian's and the median's clamp); frames are
 * independent.  With s = the int sum of the k * k clamped taps and d = k * k:
 *     out = floor((2 s + d) / (2 d))
 * the integer nearest to s / d (k is odd, so d is odd and a tie cannot occur).  Both of OpenCV's column-sum forms give
 * exactly this — the 23-bit fixed-point form it uses when k * k <= 256, and cvRound(s * (1.0 / d)) in fp64 otherwise:
 * both were evaluated on a CPU for every odd k from 3 to 63 and every s from 0 to 255 d, with 0 mismatches against the
 * formula.  OpenCV is not installed where this library is built and tested, so the formula above is the contract.
 * k must be odd with 3 <= k <= MI355_MAX_BOX_K, anything else is MI355_ERR_BAD_ARG.  sigma is ignored, no table is
 * made, and neither the Gaussian mode nor the impl knob (MI355_IMPL_*) applies.  cv::blur's DEFAULT border is
 * BORDER_REFLECT_101; that border is not offered — pass BORDER_REPLICATE to cv::blur when comparing.
 * MI355_FILTER_BOX follows the RGBA rules (dword-aligned device pointers; BGR host frames under MI355_INPUT_BGR, as
 * MEDIAN does), MI355_FILTER_BOX_GRAY8 the single-channel rules (any byte alignment, any width >= 1, UNSUPPORTED under
 * BGR).  One launch per call, whose cost does not grow with k (running column sums down a band of rows, a prefix sum
 * along the row); nothing is allocated and nothing is waited for, from the first call on.
 * The ids are 48 and 49; 42 to 47 stay unassigned and invalid, as callers expect. */
#define MI355_MAX_BOX_K 63
#define MI355_FILTER_BOX 48       /* RGBA -> RGBA     */
#define MI355_FILTER_BOX_GRAY8 49 /* 1 byte -> 1 byte */
int mi355_filter_batched(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w, int h,
                         int nframes, int k, float sigma, uint64_t prof_ns[6]);
/* bytes per output pixel of a filter (4 or 1), or MI355_ERR_BAD_ARG.  Pure host function. */
int mi355_filter_out_bpp(int filter);
/* bytes per input pixel of a filter: 4 for the RGBA filters (ids 0-4, 16, 24-27, 48), 1 for the *_GRAY8 ids, or MI355_ERR_BAD_ARG.
 * Pure host function.  Every buffer size of the batched, streamed, pool and group calls is counted in these bytes. */
int mi355_filter_in_bpp(int filter);

/* Streamed host-buffer form: nframes frames in `rgba` -> `out`, both on the host, moved
 * in chunks of chunk_frames (0 = choose) through three device slots with three stages in flight on three HIP
 * streams — H2D of chunk i+1, the kernel of chunk i, D2H of chunk i-1 — instead of the reference's
 * write / wait / kernel / wait / read / wait per frame (RT/src/Controller.cpp:470,488,512).  Results are
 * identical to mi355_filter_batched.  Any host memory works; the copies run at PCIe DMA rate and overlap in
 * both directions only when `rgba` and `out` are pinned (mi355_host_alloc).  elapsed_ms (may be NULL)
 * receives the wall time of the whole call, PCIe included. */
int mi355_filter_stream(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w, int h,
                        int nframes, int chunk_frames, int k, float sigma, double* elapsed_ms);
/* Pinned (page-locked) host memory for frames: hipHostMalloc / hipHostFree. */
int mi355_host_alloc(mi355_ctx* ctx, size_t nbytes, void** h_ptr);
int mi355_host_free(mi355_ctx* ctx, void* h_ptr);

/* ---- device-resident calls -----------------------------------------------------------------
 * d_in / d_out are device pointers on the context's GPU holding nframes tightly packed frames;
 * the call enqueues the kernel(s) on the context's stream and returns without synchronising.
 * [d_in, d_in + in_bpp*w*h*nframes) (mi355_filter_in_bpp) and the output range must not overlap: the stencil filters (Gaussian, Sobel,
 * pipeline) read neighbouring rows and halo pixels that another wave may already have overwritten, and the
 * grayscale kernels, although pointwise, are compiled with non-aliasing (__restrict__) pointers and non-temporal
 * accesses — so an in-place or overlapping call is rejected with MI355_ERR_BAD_ARG, for every filter, instead of
 * returning corrupted pixels.  (The reference never aliases them either: two clCreateBuffer objects per call.)
 * These are what a caller that already owns device memory (torch, a capture pipeline) binds, and
 * what the roofline measurement times (no PCIe in the timed region).
 * Stream capture: after the first call with a given (k, sigma) and frame size — which installs the weight table and
 * sizes the scratch buffers, synchronising the stream — these calls allocate nothing and wait for nothing, so they may
 * be issued while the context's stream is being captured into a hipGraph and replayed later
 * (tests/test_gpu_configs.py: test_device_resident_calls_can_be_captured_into_a_hip_graph; tools/graph_probe.py). */
int mi355_gray_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes);
int mi355_gray1_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes);
int mi355_gauss_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes,
                          int k, float sigma);
int mi355_sobel_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes);
int mi355_pipeline_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes,
                             int k, float sigma);
int mi355_filter_dev(mi355_ctx* ctx, int filter, const void* d_in, void* d_out, int w, int h,
                     int nframes, int k, float sigma);
/* The statistics behind MI355_FILTER_EQUALIZE_GRAY8 / OTSU_GRAY8, with the rules of mi355_filter_dev (no
 * synchronisation, overlapping buffers rejected, the same stream-capture promise) and the single-channel input rules.
 *   mi355_hist_gray8_dev             writes nframes x 256 exact counts (cv::calcHist of each frame) to d_hist, which
 *                                    it overwrites (it is zeroed in-stream first, not added to); d_hist needs 4-byte
 *                                    alignment.
 *   mi355_otsu_thresholds_gray8_dev  writes one t per frame (the value cv::threshold returns with THRESH_OTSU) to
 *                                    d_thresh (4-byte aligned).
 * w * h of 2^31 or more is MI355_ERR_BAD_ARG. */
int mi355_hist_gray8_dev(mi355_ctx* ctx, const void* d_in, uint32_t* d_hist, int w, int h, int nframes);
int mi355_otsu_thresholds_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_thresh, int w, int h, int nframes);

/* ---- changing the frame size: cv::resize of 8-bit frames ----------------------------------------
 * nframes tightly packed, independent frames of src_w x src_h become nframes frames of dst_w x dst_h.  bpp is 4 (RGBA,
 * every channel on its own, alpha included; dword-aligned device pointers) or 1 (gray8; any byte alignment, any width
 * >= 1).  These are entry points of their own, not filter ids: the output size differs from the input size.  The
 * interpolations keep OpenCV's enum values.  The contract is the arithmetic below — OpenCV's plain C++ path
 * (resize.cpp), not its IPP or OpenCL paths — operation by operation.  The library is built with -ffp-contract=off:
 * nothing below fuses a multiply with an add.
 *   scales    doubles, computed on the host and passed to the kernel by value:
 *               scale_x = 1.0 / ((double)dst_w / (double)src_w),  scale_y likewise from the heights.
 *             This is not src_w / dst_w: the two differ in the last bit for many size pairs.
 *   identity  dst == src in both dimensions: every interpolation is a copy.
 *   NEAREST   sx = min((int)floor(dx * scale_x), src_w - 1), sy likewise; out[dy][dx] = src[sy][sx].
 *   LINEAR    If src_w == 2*dst_w and src_h == 2*dst_h the result is AREA's (OpenCV switches there).  Otherwise
 *             OpenCV's fixed-point path, INTER_RESIZE_COEF_BITS = 11.
 *             Columns, for each output column dx:
 *               fx = (float)((dx + 0.5) * scale_x - 0.5)      evaluated in fp64, rounded once
 *               sx = (int)floorf(fx);  fx = fx - (float)sx
 *               if sx < 0:          sx = 0,         fx = 0
 *               if sx >= src_w - 1: sx = src_w - 1, fx = 0
 *               a0 = (int)rintf((1.f - fx) * 2048.f);  a1 = (int)rintf(fx * 2048.f)
 *             (rintf rounds half to even; each coefficient is rounded on its own.)
 *             Rows, for each output row dy:
 *               fy = (float)((dy + 0.5) * scale_y - 0.5)
 *               sy = (int)floorf(fy);  fy = fy - (float)sy      fy is NOT clamped
 *               b0 = (int)rintf((1.f - fy) * 2048.f);  b1 = (int)rintf(fy * 2048.f)
 *               r0 = clamp(sy, 0, src_h - 1);  r1 = clamp(sy + 1, 0, src_h - 1)
 *             (both rows may be the same row; the weights stay split.)
 *             Per channel, in int:
 *               H(r) = src[r][sx] * a0 + src[r][min(sx + 1, src_w - 1)] * a1
 *               out  = (((b0 * (H(r0) >> 4)) >> 16) + ((b1 * (H(r1) >> 4)) >> 16) + 2) >> 2
 *             The result always lies in 0..255; no saturation is needed.
 *   AREA      Offered only when src_w == n * dst_w and src_h == m * dst_h with integers 1 <= n, m <=
 *             MI355_MAX_AREA_FACTOR; anything else (upscaling, fractional factors: different OpenCV algorithms) is
 *             MI355_ERR_UNSUPPORTED.  sum = the int sum of the n x m block.
 *               n == m == 2:  out = (sum + 2) >> 2
 *               otherwise:    scale = 1.f / (float)(n * m);  out = saturate_u8(rintf((float)sum * scale))
 *             The second form is an fp32 product rounded half to even, NOT the exactly rounded quotient (over all
 *             n, m <= 16 the two differ for 4160 of the possible sums).
 * MI355_ERR_BAD_ARG: a null pointer or context; bpp other than 1 or 4; an unknown interp (2 included); either shape with
 * a size <= 0 or beyond what every call here accepts (more than 6e10 pixels, or a width of 2^29 or more); for bpp 4 a
 * device pointer that is not dword-aligned; input and output ranges that overlap, each counted with its own shape.
 *   mi355_resize_check    pure host function: MI355_OK, MI355_ERR_BAD_ARG or MI355_ERR_UNSUPPORTED for these values,
 *                         before any device work.
 *   mi355_resize_dev      the rules of mi355_filter_dev: enqueues one launch on the context's stream and returns without
 *                         synchronising.  It allocates nothing and waits for nothing — there is no table: scales and
 *                         sizes go by value and the per-column set-up happens in the kernel — so it can be captured into
 *                         a hipGraph from the first call on.
 *   mi355_resize_batched  host buffers: H2D, one launch, D2H through the context's pooled buffers, each side sized by its
 *                         own shape; prof_ns (may be NULL) gets the six timestamps of mi355_filter_batched.  Under
 *                         MI355_INPUT_BGR bpp 4 takes 3-byte BGR frames (the expansion counts as kernel time) and bpp 1
 *                         is MI355_ERR_UNSUPPORTED.
 * Not offered: streamed and group forms, mi355_pool_alloc, cubic / Lanczos / INTER_LINEAR_EXACT, row pitch and ROI. */
#define MI355_INTERP_NEAREST 0
#define MI355_INTERP_LINEAR 1
#define MI355_INTERP_AREA 3
#define MI355_MAX_AREA_FACTOR 16
int mi355_resize_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int interp);
int mi355_resize_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h,
                     int dst_w, int dst_h, int nframes, int interp);
int mi355_resize_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                         int dst_w, int dst_h, int nframes, int interp, uint64_t prof_ns[6]);

/* ---- rotating, shifting and deskewing frames: cv::warpAffine of 8-bit frames ---------------------
 * nframes tightly packed, independent frames of src_w x src_h become nframes frames of dst_w x dst_h, all through the
 * same 2 x 3 matrix m = {m0, m1, m2, m3, m4, m5} (row-major, as cv::Mat(2, 3, CV_64F)).  bpp is 4 (RGBA, every channel
 * warped on its own, alpha included; dword-aligned device pointers) or 1 (gray8; any byte alignment, any width >= 1).
 * Entry points of their own, not filter ids.  flags is MI355_INTERP_NEAREST or MI355_INTERP_LINEAR, optionally or-ed
 * with MI355_WARP_INVERSE_MAP; anything else is MI355_ERR_BAD_ARG, MI355_INTERP_AREA included (OpenCV silently turns
 * AREA into LINEAR; this library does not).  border_value holds the four bytes of a border pixel in memory order: R in
 * bits 0-7, then G, B and A; gray8 uses bits 0-7 and ignores the rest.  It is used only under MI355_BORDER_CONSTANT.
 * OpenCV is not installed where this library is built and tested, so THE ARITHMETIC BELOW IS THE CONTRACT.  It is the
 * classic fixed-point path of cv::warpAffine (WarpAffineInvoker followed by remapNearest / remapBilinear), restated
 * from OpenCV's source from memory — not its IPP or OpenCL paths, and not the float kernels newer OpenCV releases use.
 * Nobody has compared it with an OpenCV build here.
 *   matrix    mi355_warp_affine_matrix, a pure host function, fp64, no fused multiply-add (-ffp-contract=off):
 *               with MI355_WARP_INVERSE_MAP: inv = m.  Otherwise OpenCV's inversion, operation by operation:
 *                 D = m0*m4 - m1*m3;  D = (D != 0) ? 1.0/D : 0.0
 *                 A11 = m4*D;  A22 = m0*D
 *                 i0 = A11;  i1 = m1*(-D);  i3 = m3*(-D);  i4 = A22
 *                 i2 = -i0*m2 - i1*m5;  i5 = -i3*m2 - i4*m5
 *               A singular matrix gives the all-zero map, as in OpenCV: every output pixel samples source (0, 0).
 *   coordinates  per output pixel (x, y), in int; rint is round-half-even (cvRound); >> is an arithmetic shift:
 *                 adelta(x) = rint((i0 * x) * 1024.0)         bdelta(x) = rint((i3 * x) * 1024.0)
 *                 X0(y) = rint((i1 * y + i2) * 1024.0) + rd   Y0(y) = rint((i4 * y + i5) * 1024.0) + rd
 *                 NEAREST: rd = 512;  sx = (X0 + adelta) >> 10;  sy = (Y0 + bdelta) >> 10
 *                 LINEAR:  rd = 16;   X = (X0 + adelta) >> 5;  Y likewise
 *                          sx = X >> 5;  fx = X & 31;  sy = Y >> 5;  fy = Y & 31
 *               (so NEAREST rounds to the nearest source pixel and LINEAR works on a grid of 1/32 pixel.)
 *   sampling  per channel.  tap(u, v) = src[v][u] inside the frame; outside it is the border byte under
 *             MI355_BORDER_CONSTANT and src[clamp(v)][clamp(u)] under MI355_BORDER_REPLICATE.
 *               NEAREST: out = tap(sx, sy)
 *               LINEAR:  out = ((32-fx)*(32-fy)*tap(sx, sy)   + fx*(32-fy)*tap(sx+1, sy)
 *                             + (32-fx)*fy*tap(sx, sy+1)     + fx*fy*tap(sx+1, sy+1) + 512) >> 10
 *             This equals OpenCV's 15-bit weight table followed by (sum + 16384) >> 15: the table entry is
 *             32 * (32-fx or fx) * (32-fy or fy) exactly and its rows sum to 32768 with no correction step (all 1024
 *             entries checked in fp32).  The result always lies in 0..255.  Frames are independent: a tap never reads a
 *             neighbouring frame.
 *   limits    MI355_ERR_BAD_ARG: a null pointer or context; bpp other than 1 or 4; bad flags or border mode; a size or
 *             frame count <= 0 (or more than 6e10 pixels, or 2^31 tiles of work, in a call); a non-finite matrix entry;
 *             for bpp 4 a device pointer that is not dword-aligned; input and output ranges that overlap, each counted
 *             with its own shape.
 *             MI355_ERR_UNSUPPORTED: a width or height above MI355_MAX_WARP_SIZE (below it OpenCV's saturation of sx,
 *             sy to short cannot be observed, so the formula omits it); a matrix for which
 *             |i0|*(dst_w-1) + |i1|*(dst_h-1) + |i2| >= 2^20, or the same sum for i3, i4, i5 (below that no int sum
 *             above can overflow, and OpenCV's int saturation cannot be observed either).
 *   mi355_rotation_matrix      cv::getRotationMatrix2D, a pure host function:
 *                                a = cos(angle_deg*pi/180)*scale;  b = sin(angle_deg*pi/180)*scale
 *                                m = {a, b, (1-a)*cx - b*cy, -b, a, b*cx + (1-a)*cy}
 *                              MI355_ERR_BAD_ARG for a null m, a non-finite input and scale == 0.
 *   mi355_warp_affine_matrix   the inverse map above; MI355_ERR_BAD_ARG for a null pointer, bad flags or a non-finite
 *                              entry of m.
 *   mi355_warp_affine_check    pure host function: MI355_OK, MI355_ERR_BAD_ARG or MI355_ERR_UNSUPPORTED for these
 *                              values, before any device work.
 *   mi355_warp_affine_dev      the rules of mi355_resize_dev: enqueues one launch on the context's stream and returns
 *                              without synchronising.  No allocation, table or scratch: the six doubles and the sizes
 *                              go by value, so it can be captured into a hipGraph from the first call on.
 *   mi355_warp_affine_batched  host buffers: H2D, one launch, D2H through the context's pooled buffers, each side sized
 *                              by its own shape; prof_ns (may be NULL) gets the six timestamps of mi355_filter_batched.
 *                              Under MI355_INPUT_BGR bpp 4 takes 3-byte BGR frames (the expansion counts as kernel
 *                              time) and bpp 1 is MI355_ERR_UNSUPPORTED.
 * Not offered: cubic and Lanczos, BORDER_TRANSPARENT / REFLECT* / WRAP, streamed and group forms, mi355_pool_alloc, row
 * pitch and ROI, and one matrix per frame (a stabiliser calls once per frame).  warpPerspective and remap have their own
 * section below. */
#define MI355_WARP_INVERSE_MAP 16 /* cv::WARP_INVERSE_MAP, or-ed into flags */
#define MI355_BORDER_CONSTANT 0   /* cv::BORDER_CONSTANT  */
#define MI355_BORDER_REPLICATE 1  /* cv::BORDER_REPLICATE */
#define MI355_MAX_WARP_SIZE 32766 /* largest width / height of either shape */
int mi355_rotation_matrix(double cx, double cy, double angle_deg, double scale, double m[6]);
int mi355_warp_affine_matrix(const double m[6], int flags, double inv[6]);
int mi355_warp_affine_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, const double m[6],
                            int flags, int border_mode);
int mi355_warp_affine_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h, int dst_w,
                          int dst_h, int nframes, const double m[6], int flags, int border_mode,
                          uint32_t border_value);
int mi355_warp_affine_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                              int dst_w, int dst_h, int nframes, const double m[6], int flags, int border_mode,
                              uint32_t border_value, uint64_t prof_ns[6]);

/* ---- undistorting and rectifying frames: cv::remap and cv::warpPerspective of 8-bit frames -------
 * The frame rules are those of mi355_warp_affine_*: nframes tightly packed, independent frames of src_w x src_h become
 * nframes frames of dst_w x dst_h; bpp 4 (RGBA, every channel on its own, dword-aligned device pointers) or 1 (gray8, any
 * byte alignment, any width >= 1); border_mode MI355_BORDER_CONSTANT or MI355_BORDER_REPLICATE with border_value as
 * there; sizes up to MI355_MAX_WARP_SIZE.  interp is MI355_INTERP_NEAREST or MI355_INTERP_LINEAR only.
 * OpenCV is not installed where this library is built and tested, so THE ARITHMETIC BELOW IS THE CONTRACT.  It restates
 * OpenCV's classic fixed-point path (cv::remap on CV_16SC2 + CV_16UC1 maps, cv::convertMaps for float maps,
 * WarpPerspectiveInvoker followed by remapNearest / remapBilinear) from memory.  Nobody has compared it with an OpenCV
 * build here.
 *   maps      mi355_remap_*: ONE map of dst_w x dst_h entries, row-major and tightly packed, serves all nframes frames.
 *               MI355_MAP_FIXED  map1: int16 (sx, sy) pairs, dword-aligned; map2: uint16 fy*32+fx, 2-byte aligned; map2
 *                                may be NULL with MI355_INTERP_NEAREST, which does not read it.
 *               MI355_MAP_FLOAT  map1: the float x plane, map2: the float y plane, both dword-aligned.
 *             Any other NULL and any misalignment is MI355_ERR_BAD_ARG, and so is an output range that overlaps the
 *             input or either map.
 *   remap coordinates  per output pixel i = y * dst_w + x; clamp16(v) = min(max(v, -32768), 32767):
 *               FIXED:  sx = map1[2i];  sy = map1[2i+1];  LINEAR adds a = map2[i] & 1023;  fx = a & 31;  fy = a >> 5
 *               FLOAT:  tx = map_x[i] * S in fp32, S = 32.0f for LINEAR and 1.0f for NEAREST (exact short of overflow)
 *                       X = (int)rint(tx), round half even; a NaN tx gives INT_MIN; tx <= -2^31 gives INT_MIN and
 *                       tx >= 2^31 gives INT_MAX.  Y likewise from map_y.
 *                       NEAREST: sx = clamp16(X);  sy = clamp16(Y)
 *                       LINEAR:  sx = clamp16(X >> 5);  fx = X & 31;  sy = clamp16(Y >> 5);  fy = Y & 31
 *             (cv::convertMaps followed by FIXED gives what FLOAT gives.  With sizes <= MI355_MAX_WARP_SIZE the clamp to
 *             short cannot be observed: a saturated index lies outside the frame either way.)
 *   perspective matrix  mi355_perspective_matrix, a pure host function, fp64, no fused multiply-add; m is row-major, as
 *             cv::Mat(3, 3, CV_64F).  With MI355_WARP_INVERSE_MAP: inv = m.  Otherwise the adjugate times 1 / det:
 *               det = m0*(m4*m8 - m5*m7) - m1*(m3*m8 - m5*m6) + m2*(m3*m7 - m4*m6);  d = (det != 0) ? 1.0/det : 0.0
 *               inv0 = (m4*m8 - m5*m7)*d;  inv1 = (m2*m7 - m1*m8)*d;  inv2 = (m1*m5 - m2*m4)*d
 *               inv3 = (m5*m6 - m3*m8)*d;  inv4 = (m0*m8 - m2*m6)*d;  inv5 = (m2*m3 - m0*m5)*d
 *               inv6 = (m3*m7 - m4*m6)*d;  inv7 = (m1*m6 - m0*m7)*d;  inv8 = (m0*m4 - m1*m3)*d
 *             A singular matrix gives the all-zero map: w == 0 everywhere and every pixel samples source (0, 0), like
 *             the affine call.  No range limit is needed: the clamp below is part of the formula.
 *   perspective coordinates  per output pixel (x, y) from inv = h0 .. h8, all fp64, IEEE division, nothing fused; the
 *             round brackets fix the order of operations:
 *               w  = (h6*x) + (h7*y + h8);  s = (w != 0) ? S / w : 0      S = 32.0 for LINEAR, 1.0 for NEAREST
 *               tX = ((h0*x) + (h1*y + h2)) * s;  tY = ((h3*x) + (h4*y + h5)) * s
 *               fX = !(tX < 2147483647.0) ? 2147483647.0 : tX;  fX = fX < -2147483648.0 ? -2147483648.0 : fX
 *               X  = (int)rint(fX);  Y likewise        (a NaN gives INT_MAX, as OpenCV's min / max order does)
 *             then sx, fx, sy, fy from X and Y exactly as under FLOAT above.
 *             One known difference: OpenCV evaluates X0 + M[0]*x1 per 32-column block from the block's first column,
 *             which can differ from the formula above in the last bit of a double.  That cannot change a pixel unless a
 *             coordinate lies within about 1e-12 of a rounding boundary.
 *   sampling  tap(), NEAREST, the LINEAR sum (... + 512) >> 10 and both border rules are those of the warpAffine
 *             section above, applied to (sx, sy, fx, fy).
 *   limits    MI355_ERR_BAD_ARG: a null pointer or context (but see map2); bpp other than 1 or 4; an unknown map_kind,
 *             interp (remap: anything but NEAREST and LINEAR; perspective: bad flags) or border mode; a size or frame
 *             count <= 0 (or more than 6e10 pixels, or 2^31 tiles of work, in a call); a non-finite matrix entry; the
 *             alignment and overlap rules above.  MI355_ERR_UNSUPPORTED: a width or height above MI355_MAX_WARP_SIZE.
 *   mi355_remap_check, mi355_warp_perspective_check   pure host functions: the code a call with these values returns
 *             before any device work.
 *   mi355_remap_dev, mi355_warp_perspective_dev   the rules of mi355_warp_affine_dev: one launch on the context's
 *             stream, no synchronisation, no allocation, table or scratch (the nine doubles go by value; the maps are the
 *             caller's), so the first call a fresh context makes can be the captured one.
 *   mi355_remap_batched, mi355_warp_perspective_batched   host buffers through the context's pooled buffers; the maps
 *             (host pointers here) are uploaded on every call and count as H2D time; prof_ns (may be NULL) gets the six
 *             timestamps of mi355_filter_batched.  MI355_INPUT_BGR behaves as in mi355_warp_affine_batched.
 * Not offered: building undistortion maps (initUndistortRectifyMap), convertMaps as an entry point, cubic and Lanczos,
 * other border modes, one map or one matrix per frame, group and streamed forms, row pitch and ROI. */
#define MI355_MAP_FIXED 0 /* map1: int16 (sx, sy) pairs, map2: uint16 fy*32+fx  (CV_16SC2 + CV_16UC1, cv::convertMaps) */
#define MI355_MAP_FLOAT 1 /* map1: float x plane, map2: float y plane           (CV_32FC1 + CV_32FC1) */
int mi355_remap_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int map_kind, int interp,
                      int border_mode);
int mi355_remap_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h, int dst_w, int dst_h,
                    int nframes, const void* d_map1, const void* d_map2, int map_kind, int interp, int border_mode,
                    uint32_t border_value);
int mi355_remap_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h, int dst_w,
                        int dst_h, int nframes, const void* map1, const void* map2, int map_kind, int interp,
                        int border_mode, uint32_t border_value, uint64_t prof_ns[6]);
int mi355_perspective_matrix(const double m[9], int flags, double inv[9]);
int mi355_warp_perspective_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, const double m[9],
                                 int flags, int border_mode);
int mi355_warp_perspective_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h, int dst_w,
                               int dst_h, int nframes, const double m[9], int flags, int border_mode,
                               uint32_t border_value);
int mi355_warp_perspective_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                                   int dst_w, int dst_h, int nframes, const double m[9], int flags, int border_mode,
                                   uint32_t border_value, uint64_t prof_ns[6]);

/* ---- local threshold: cv::adaptiveThreshold(src, dst, max_value, ADAPTIVE_THRESH_MEAN_C, type, block, delta) -------
 * gray8 frames only (the single-channel rules: tightly packed, any byte alignment, any width >= 1).  Entry points of
 * their own, not filter ids: the parameters do not fit (k, sigma).  The argument order is OpenCV's.
 *   mean    MI355_FILTER_BOX_GRAY8's value with k = block (OpenCV's own call uses BORDER_REPLICATE there).
 *   idelta  computed on the host: (int)ceil(delta) for MI355_ADAPTIVE_BINARY, (int)floor(delta) for
 *           MI355_ADAPTIVE_BINARY_INV, then clamped to [-256, 256] (beyond that the output is constant anyway).
 *   BINARY      out = (src - mean >  -idelta) ? max_value : 0
 *   BINARY_INV  out = (src - mean <= -idelta) ? max_value : 0
 * OpenCV's quirk is kept: with a fractional delta the two types are not complements (ceil for one, floor for the
 * other) — at delta = 2.5 a pixel with src - mean == -2 is "on" in both.
 * MI355_ERR_BAD_ARG: a null pointer or context; sizes the filter calls reject; block even, below 3 or above
 * MI355_MAX_BOX_K; max_value outside 0..255; a type other than the two below; a non-finite delta; overlapping ranges.
 *   mi355_adaptive_threshold_check        pure host function: MI355_OK or MI355_ERR_BAD_ARG for these values.
 *   mi355_adaptive_threshold_gray8_dev    the rules of mi355_filter_dev: ONE launch on the context's stream (the mean
 *                                         frame never exists in memory: the compare is the epilogue of the box
 *                                         kernel), no synchronisation, no allocation, no table, no scratch — so it can
 *                                         be captured into a hipGraph from the first call on.
 *   mi355_adaptive_threshold_gray8_batched  host buffers: H2D, the launch, D2H through the context's pooled buffers;
 *                                         prof_ns (may be NULL) gets the six timestamps of mi355_filter_batched.
 *                                         MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR (a gray plane has no BGR form).
 * Not offered: ADAPTIVE_THRESH_GAUSSIAN_C, RGBA frames, streamed and group forms, row pitch and ROI. */
#define MI355_ADAPTIVE_BINARY 0     /* cv::THRESH_BINARY     */
#define MI355_ADAPTIVE_BINARY_INV 1 /* cv::THRESH_BINARY_INV */
int mi355_adaptive_threshold_check(int w, int h, int nframes, int max_value, int type, int block, double delta);
int mi355_adaptive_threshold_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes,
                                       int max_value, int type, int block, double delta);
int mi355_adaptive_threshold_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                                           int max_value, int type, int block, double delta, uint64_t prof_ns[6]);

/* ---- local contrast: cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(src, dst), 8-bit ------------------------
 * Contrast-limited adaptive histogram equalization.  gray8 frames only (the single-channel rules: tightly packed, any
 * byte alignment, any width >= 1, frames are independent, MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR).  Entry points of
 * their own, not filter ids: the parameters do not fit (k, sigma).  OpenCV is not installed where this library is built
 * and tested: the arithmetic below restates OpenCV's plain C++ path (modules/imgproc/src/clahe.cpp, 8-bit branch) from
 * memory, and it — not OpenCV — is the contract.  The library is built with -ffp-contract=off: nothing fuses.
 * Geometry (host, int).  If w % tiles_x == 0 and h % tiles_y == 0: ew = w, eh = h.  Otherwise ew = w + (tiles_x - w %
 * tiles_x) and eh = h + (tiles_y - h % tiles_y): OpenCV's quirk is kept — when only one dimension fails to divide, the
 * other is still padded, by a full tiles_x or tiles_y.  tw = ew / tiles_x, th = eh / tiles_y, tot = tw * th.  The extended
 * frame is cv::copyMakeBorder(BORDER_REFLECT_101) on the right and bottom only:
 *     ext[y][x] = src[r(y, h)][r(x, w)],   r(p, n) = p < n ? p : 2n - 2 - p
 * and never exists in memory.
 * Tile tables (int except where marked).  For every tile (j, i), hist = the 256 counts of ext[j*th .. (j+1)*th)[i*tw ..
 * (i+1)*tw).
 *     cl = clip_limit > 0 ? max((int)(clip_limit * tot / 256.0), 1) : 0        fp64, truncation (capped at tot, which
 *                                                                              cannot be observed: no bin exceeds tot)
 *     if cl > 0:
 *         clipped = sum over bins of max(hist[b] - cl, 0);  hist[b] = min(hist[b], cl)
 *         batch = clipped / 256;  residual = clipped - batch * 256;  hist[b] += batch
 *         if residual: step = max(256 / residual, 1);  bins 0, step, 2*step, ... (residual of them) get +1,
 *                      i.e. bin b gets it iff b % step == 0 && b / step < residual
 *     lut_scale = 255.0f / (float)tot                                          fp32, on the host
 *     sum += hist[b];  lut[b] = saturate_u8(rint_half_even((float)sum * lut_scale))
 * A constant frame is therefore NOT mapped to itself: a frame of 7s, 64 x 48 with 8 x 8 tiles, gives 16 with clip_limit
 * 2.0 and 255 with clip_limit 0.
 * Apply (fp32, in the written order, no fused multiply-add).  inv_tw = 1.0f / (float)tw and inv_th = 1.0f / (float)th are
 * computed on the host and passed by value (the device's own fp32 division is not the contract).
 *     txf = (float)x * inv_tw - 0.5f;  tx1 = (int)floorf(txf);  xa = txf - (float)tx1;  xa1 = 1.0f - xa
 *     c1 = max(tx1, 0);  c2 = min(tx1 + 1, tiles_x - 1)        (rows likewise: tyf, ya, ya1, r1, r2 from y and inv_th)
 *     v = src[y][x]
 *     res = ((float)L[r1][c1][v] * xa1 + (float)L[r1][c2][v] * xa) * ya1
 *         + ((float)L[r2][c1][v] * xa1 + (float)L[r2][c2][v] * xa) * ya
 *     out = saturate_u8(rint_half_even(res))
 * Only the w x h pixels of the source are written.
 * MI355_ERR_BAD_ARG: a null pointer or context; sizes the filter calls reject; ew * eh >= 2^31 (the limit of the
 * histogram calls, applied to the extended frame); tiles_x or tiles_y outside 1 .. MI355_MAX_CLAHE_TILES; a non-finite
 * clip_limit; overlapping ranges; a d_luts that is not 4-byte aligned.
 * MI355_ERR_UNSUPPORTED: a pad that one reflection cannot serve, ew - w > w - 1 or eh - h > h - 1 (31 x 16 with 16 x 16
 * tiles: the quirk pads 16 rows onto 16).  OpenCV reflects repeatedly there; this library does not.
 *   mi355_clahe_check           pure host function returning exactly these codes for these values.
 *   mi355_clahe_gray8_dev       the rules of mi355_filter_dev: three launches (tile histograms, tables, apply) and one
 *                               memset on the context's stream, no synchronisation.  The scratch, tiles x (1 KiB + 256 B)
 *                               per frame, is pooled in the context: after the first call for a given (nframes, tiles_x,
 *                               tiles_y) a call allocates nothing and waits for nothing, so it can be captured into a
 *                               hipGraph.
 *   mi355_clahe_luts_gray8_dev  the tables only: nframes x tiles_y x tiles_x x 256 bytes to d_luts (4-byte aligned),
 *                               frame-major then tile-row-major.  To CLAHE what mi355_hist_gray8_dev is to equalize.
 *   mi355_clahe_gray8_batched   host buffers: H2D, the launches, D2H through the context's pooled buffers; prof_ns (may be
 *                               NULL) gets the six timestamps of mi355_filter_batched.
 * Not offered: RGBA or Lab frames, 16-bit frames, the streamed, group and mi355_pool_alloc forms, row pitch and ROI. */
#define MI355_MAX_CLAHE_TILES 16
int mi355_clahe_check(int w, int h, int nframes, double clip_limit, int tiles_x, int tiles_y);
int mi355_clahe_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes, double clip_limit,
                          int tiles_x, int tiles_y);
int mi355_clahe_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                              double clip_limit, int tiles_x, int tiles_y, uint64_t prof_ns[6]);
int mi355_clahe_luts_gray8_dev(mi355_ctx* ctx, const void* d_in, uint8_t* d_luts, int w, int h, int nframes,
                               double clip_limit, int tiles_x, int tiles_y);

/* ---- the blobs of a mask: cv::connectedComponentsWithStats(mask, labels, stats, centroids, connectivity, CV_32S) --------
 * Connected-component labelling of gray8 masks, with the per-label boxes, areas and coordinate sums.  gray8 frames only
 * (the single-channel rules: tightly packed, any byte alignment, any width >= 1, frames are independent,
 * MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR in the host form).  Entry points of their own, not filter ids: the outputs
 * do not fit (k, sigma).  OpenCV is not installed where this library is built and tested: nobody has compared these
 * calls with an OpenCV build; the rules below — not OpenCV — are the contract.  Everything is integer arithmetic.
 * Foreground.  A pixel is foreground iff its byte is not zero.
 * Connectivity.  4: left, right, up, down.  8: the four diagonals as well.  Row ends do not wrap: (w - 1, y) and
 * (0, y + 1) are not neighbours; nor are the last row of frame f and the first row of frame f + 1.
 * Labels.  int32 d_labels[nframes][h][w].  Background is 0.  The components of a frame are numbered 1 .. N - 1 in raster
 * order of their first pixel: component A has a smaller number than component B iff the smallest y * w + x in A is
 * smaller than the smallest in B.  One right answer per input, the same bits on every run and for every work
 * decomposition; it is what scipy.ndimage.label produces.  OpenCV numbers components in the order in which its
 * block-based scan creates provisional labels, so its labels may be a PERMUTATION of these; the partition of the pixels
 * into components, and therefore the set of stats rows, is the same.
 * Count.  int32 d_count[nframes] = N, the number of labels including the background: the value
 * cv::connectedComponents returns.  An all-background frame has N = 1.
 * Statistics (optional).  stats_rows is the number of rows per frame; 0: none, and d_stats and d_sums may be NULL.  Row l
 * describes label l; row 0 is the background, as in OpenCV.
 *     int32  d_stats[nframes][stats_rows][5] = {left, top, width, height, area}        (CC_STAT_LEFT .. CC_STAT_AREA)
 *     uint64 d_sums[nframes][stats_rows][2]  = {sum of x, sum of y} over the label's pixels
 * The centroid is ((double)sum_x / (double)area, (double)sum_y / (double)area), taken on the host: no floating-point sum
 * runs on the device, so nothing depends on the order in which pixels arrive.  A row whose label has no pixel (l >= N,
 * or row 0 of an all-foreground frame) is five zeros and two zeros: every byte of both buffers is defined.  Labels
 * >= stats_rows are still labelled and counted; they have no row.  Compare d_count with stats_rows to see a truncation.
 * MI355_ERR_BAD_ARG, before any device work: a null context or pointer (d_stats and d_sums only when stats_rows > 0);
 * sizes the histogram calls reject (w * h >= 2^31 among them: a provisional label is a pixel index plus one in an
 * int32); a connectivity other than 4 or 8; stats_rows < 0 or > MI355_MAX_CCL_STATS_ROWS; a d_labels, d_count or d_stats
 * that is not 4-byte aligned; a d_sums that is not 8-byte aligned; an output range that overlaps the input or another
 * output.
 *   mi355_ccl_check          pure host function returning the code a call with these values returns before any device work.
 *   mi355_ccl_gray8_dev      the rules of mi355_filter_dev: up to eight launches on the context's stream, no
 *                            synchronisation.  d_labels itself is the union-find parent array; nothing else is kept per
 *                            pixel.  The scratch, 4 bytes per 2048 pixels (per-block component counts, then their
 *                            offsets), is pooled in the context: after the first call for a given (w, h, nframes) a call
 *                            allocates nothing and waits for nothing, so it can be captured into a hipGraph.
 *   mi355_ccl_gray8_batched  host buffers: H2D, the launches, D2H through the context's pooled buffers; prof_ns (may be
 *                            NULL) gets the six timestamps of mi355_filter_batched.  The copies of count, stats and sums
 *                            are enqueued ahead of the labels' and fall into the kernel interval.
 * Not offered: CV_16U labels, OpenCV's exact label permutation, contours, moments beyond the first, per-label pixel
 * lists, RGBA input, the streamed and group forms, row pitch and ROI. */
#define MI355_MAX_CCL_STATS_ROWS 16777216 /* 2^24 */
int mi355_ccl_check(int w, int h, int nframes, int connectivity, int stats_rows);
int mi355_ccl_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_labels, int32_t* d_count, int32_t* d_stats,
                        uint64_t* d_sums, int w, int h, int nframes, int connectivity, int stats_rows);
int mi355_ccl_gray8_batched(mi355_ctx* ctx, const uint8_t* in, int32_t* labels, int32_t* count, int32_t* stats,
                            uint64_t* sums, int w, int h, int nframes, int connectivity, int stats_rows,
                            uint64_t prof_ns[6]);

/* ---- how far from the background: cv::distanceTransform(mask, dist, DIST_L2, DIST_MASK_PRECISE, CV_32F) -----------------
 * The exact Euclidean distance transform of gray8 masks: per pixel the squared distance to the nearest zero pixel, its
 * square root, and which zero pixel that is (the step between "mask" and "what to do with each blob": watershed seeds that
 * split touching blobs, thickness, clearance, chamfer matching, nearest-seed lookups).  gray8 frames only (the
 * single-channel rules: tightly packed, any byte alignment, any width >= 1, frames are independent,
 * MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR in the host form).  Entry points of their own, not filter ids: the outputs
 * do not fit (k, sigma).  OpenCV is not installed where this library is built and tested: nobody has compared these
 * calls with an OpenCV build; the rules below — not OpenCV — are the contract, this library's own.
 * Polarity.  OpenCV's: a pixel whose byte is zero is a SITE.  Every pixel gets its distance to the nearest site of its
 * frame; a site gets 0.
 * Squared distance.  int32 d_sq[nframes][h][w] = the minimum over the frame's sites (x', y') of
 * (x - x')^2 + (y - y')^2, exactly.  With w, h <= MI355_MAX_DIST_DIM the largest value is 2 * 16383^2 < 2^30: that is
 * why the limit exists.
 * Distance.  float d_dist[nframes][h][w] = sqrtf((float)sq): the int32 -> fp32 conversion rounds to nearest, ties to
 * even (it matters above 2^24, which a side above 4096 can reach), the square root is the correctly rounded fp32 one.
 * In numpy: np.sqrt(sq.astype(np.float32)).  It corresponds to DIST_L2 with DIST_MASK_PRECISE and CV_32F.
 * Nearest site.  int32 d_nearest[nframes][h][w] = y' * w + x' of the nearest site, within its frame.  Among equally near
 * sites the one with the smallest column x' is taken, and among those the one with the smallest row y' — COLUMN first,
 * not raster order.  A site's nearest site is itself.  (DIST_LABEL_PIXEL numbers the sites instead; this is the index.)
 * A frame without a site gets MI355_DIST_NONE, +INFINITY and -1 in every pixel; the other frames of the batch are
 * unaffected.  A column without a site in a frame that has one is an ordinary case.
 * Optional outputs.  Any of d_sq, d_dist, d_nearest may be NULL, not all three.  An output that is present holds the
 * same bytes whatever the others are.
 * MI355_ERR_BAD_ARG, before any device work: a null context or input, or all three outputs null; sizes the histogram
 * calls reject; w or h above MI355_MAX_DIST_DIM; an output that is not 4-byte aligned; a present output range that
 * overlaps the input or another present output.
 *   mi355_dist_check          pure host function returning the code a call with these values returns before any device work.
 *   mi355_dist_gray8_dev      the rules of mi355_filter_dev: two launches on the context's stream (columns, rows), no
 *                             synchronisation.  The scratch, 2 BYTES PER PIXEL (rows padded to four pixels: the signed row
 *                             offset to the nearest site of the pixel's own column), is pooled in the context: after the
 *                             first call for a given (w, h, nframes) a call allocates nothing and waits for nothing, so it
 *                             can be captured into a hipGraph.  The work of a row is bounded by its width alone
 *                             (O(w log w)), never by the content.
 *   mi355_dist_gray8_batched  host buffers: H2D, the launches, D2H through the context's pooled buffers; prof_ns (may be
 *                             NULL) gets the six timestamps of mi355_filter_batched.  The first output the caller takes is
 *                             the read that is timed; the copies of the others are enqueued ahead of it and fall into the
 *                             kernel interval.
 * Not offered: DIST_L1 and DIST_C, the 3x3 and 5x5 chamfer approximations, CV_8U output, DIST_LABEL_CCOMP, RGBA input,
 * the streamed and group forms, row pitch and ROI. */
#define MI355_MAX_DIST_DIM 16384
#define MI355_DIST_NONE    2147483647      /* d_sq of a frame without a zero pixel */
int mi355_dist_check(int w, int h, int nframes);
int mi355_dist_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_sq, float* d_dist, int32_t* d_nearest, int w, int h,
                         int nframes);
int mi355_dist_gray8_batched(mi355_ctx* ctx, const uint8_t* in, int32_t* sq, float* dist, int32_t* nearest, int w, int h,
                             int nframes, uint64_t prof_ns[6]);

/* ---- from gradients to edges: hysteresis thresholding, and cv::Canny(image, edges, threshold1, threshold2, 3, L2gradient) --
 * The step between "gradient magnitude" and "mask": one-pixel-wide, connected edges without leaving the device.  gray8
 * frames only, in and out (the single-channel rules: tightly packed, any byte alignment of input and output, any width
 * >= 1, frames are independent, MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR in the host form).  Entry points of their
 * own, not filter ids: the parameters do not fit (k, sigma).  OpenCV is not installed where this library is built and
 * tested: the rules below are restated from memory of OpenCV's code; nobody has compared it with an OpenCV build here;
 * the rules below are the contract.  All arithmetic is integer; every byte of the output is written; there is one right
 * answer per input, the same bits on every run.
 *
 * 1. Hysteresis threshold of a response map (this library's SOBEL_GRAY8 or CLAHE output, any gray8 frame).
 *     candidate   a pixel whose byte > low
 *     strong      a pixel whose byte > high
 *     out         255 where the pixel is a candidate and its connected component of candidates holds at least one
 *                 strong pixel, else 0
 *   Connectivity is 4 or 8, the component rule of mi355_ccl_*: row ends do not wrap, frames do not link.
 *   MI355_ERR_BAD_ARG, before any device work: a null context or pointer; sizes the labelling call rejects (w * h >= 2^31
 *   among them); a connectivity other than 4 or 8; low or high outside 0..255; low > high; a d_out range that overlaps
 *   d_in.  high = 255 is accepted: nothing is strong and the output is all zero.
 *
 * 2. Canny, aperture 3.  No colour step and no blur of its own: chain MI355_FILTER_GAUSS_GRAY8 in front, as a
 *    cv::GaussianBlur + cv::Canny user does.
 *   thresholds  lo = min(threshold1, threshold2), hi = max(threshold1, threshold2), in double.  With
 *               MI355_CANNY_L2GRADIENT: lo = min(lo, 32767.0), hi = min(hi, 32767.0), then each one that is > 0 is
 *               squared.  low = (int)floor(lo), high = (int)floor(hi).
 *   gradient    the 3x3 Sobel pair with coordinates clamped to the frame (BORDER_REPLICATE), p[y][x] the source byte:
 *                   dx = (p[y-1][x+1] + 2 p[y][x+1] + p[y+1][x+1]) - (p[y-1][x-1] + 2 p[y][x-1] + p[y+1][x-1])
 *                   dy = (p[y+1][x-1] + 2 p[y+1][x] + p[y+1][x+1]) - (p[y-1][x-1] + 2 p[y-1][x] + p[y-1][x+1])
 *               This is NOT the Sobel of MI355_FILTER_SOBEL_GRAY8: that one is the reference program's reflect-101
 *               magnitude.
 *   magnitude   m = |dx| + |dy|, or dx * dx + dy * dy with MI355_CANNY_L2GRADIENT; both fit an int32 (|dx|, |dy| <=
 *               1020).  The magnitude of a position outside the frame is 0.
 *   non-maximum suppression   a pixel with m > low is a candidate iff it is a local maximum along its quantised
 *               direction.  With x = |dx|, y = |dy| << 15, tg22x = x * 13573, tg67x = tg22x + (x << 16) (all below 2^27):
 *                   y < tg22x            m > m(x-1, y)    and  m >= m(x+1, y)
 *                   else y > tg67x       m > m(x, y-1)    and  m >= m(x, y+1)
 *                   else                 m > m(x-s, y-1)  and  m >  m(x+s, y+1),   s = ((dx ^ dy) < 0) ? -1 : 1
 *               The > / >= asymmetry is part of the contract: it decides which column of a two-pixel plateau survives
 *               (the one on the left, the one above), so the mirror image of a frame need not give the mirrored edges.
 *   hysteresis  a candidate is strong iff m > high; out = 255 where the pixel is a candidate and its 8-connected
 *               component of candidates holds a strong one, else 0: rule 1 on the candidates.
 *   MI355_ERR_BAD_ARG, before any device work: a null context or pointer; sizes the labelling call rejects; a threshold
 *   that is not finite, is negative or exceeds 1e9; flag bits other than MI355_CANNY_L2GRADIENT; a d_out range that
 *   overlaps d_in.
 *
 *   mi355_hysteresis_check, mi355_canny_check   pure host functions returning the code a call with these values returns
 *                            before any device work.
 *   mi355_hysteresis_gray8_dev   the rules of mi355_filter_dev: up to five launches on the context's stream (the three
 *                            union launches of mi355_ccl_gray8_dev with "byte > low" as foreground, mark, emit), no
 *                            synchronisation.  The union-find parent array, 4 BYTES PER PIXEL, is pooled in the context:
 *                            after the first call for a given (w, h, nframes) a call allocates nothing and waits for
 *                            nothing, so it can be captured into a hipGraph.
 *   mi355_canny_gray8_dev    the same with one launch in front: source bytes -> a class byte per pixel (0 none,
 *                            1 candidate, 2 strong) in d_out itself, which the hysteresis then rewrites in place.  Up to
 *                            six launches; the same pooled 4 bytes per pixel and nothing else; the same graph rule.
 *   mi355_*_gray8_batched    host buffers: H2D, the launches, D2H through the context's pooled buffers; prof_ns (may be
 *                            NULL) gets the six timestamps of mi355_filter_batched.
 * Not offered: apertures 5 and 7, RGBA input, the (dx, dy) overload of cv::Canny, 16-bit responses, the streamed, group
 * and mi355_pool_alloc forms, row pitch and ROI. */
#define MI355_CANNY_L2GRADIENT 1
int mi355_hysteresis_check(int w, int h, int nframes, int low, int high, int connectivity);
int mi355_hysteresis_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes, int low,
                               int high, int connectivity);
int mi355_hysteresis_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes, int low,
                                   int high, int connectivity, uint64_t prof_ns[6]);
int mi355_canny_check(int w, int h, int nframes, double threshold1, double threshold2, int flags);
int mi355_canny_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes, double threshold1,
                          double threshold2, int flags);
int mi355_canny_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                              double threshold1, double threshold2, int flags, uint64_t prof_ns[6]);

/* ---- from edges to lines: cv::HoughLines(edges, lines, rho, theta, threshold, 0, 0, min_theta, max_theta) ------------------
 * The standard Hough transform of gray8 edge maps (this library's Canny or hysteresis output, any mask): one byte per
 * pixel in, a few hundred bytes of (rho, theta) pairs per frame out.  gray8 frames only (the single-channel rules: tightly
 * packed, any byte alignment of the input, frames are independent, MI355_ERR_UNSUPPORTED under MI355_INPUT_BGR in the
 * host form).  Entry points of their own, not filter ids: the parameters do not fit (k, sigma).  OpenCV is not installed
 * where this library is built and tested: the rules below are restated from memory of OpenCV's HoughLinesStandard; nobody
 * has compared it with an OpenCV build here; the rules below are the contract.
 *   parameters  rho_f = (float)rho;  theta_f = (float)theta;  irho = 1.0f / rho_f, in fp32.
 *   numangle    in double: floor((max_theta - min_theta) / theta) + 1; if that is greater than 1 and
 *               |pi - (numangle - 1) * theta| < theta / 2, one less.  pi is M_PI.
 *   numrho      cvRound((float)(2 * (w + h) + 1) / rho_f): the division in fp32, the rounding half to even.
 *   trig table  ang is an fp32 variable that starts at (float)min_theta and grows by theta_f per entry (an fp32 add):
 *                 tab_cos[n] = (float)(cos((double)ang) * (double)irho),  tab_sin[n] likewise with sin.
 *               The table is made on the host (mi355_hough_trig_table returns it) and handed to the kernels: whatever the
 *               platform's cos and sin return is part of the contract.
 *   votes       every pixel (x, y) whose byte is not zero votes once for every angle n, in the cell
 *                 r = rne(fl32(fl32(x * tab_cos[n]) + fl32(y * tab_sin[n]))) + (numrho - 1) / 2      (integer division)
 *               counted in accum[(n + 1) * (numrho + 2) + r + 1].  The two products and the sum are three separately
 *               rounded fp32 operations (no fused multiply-add); rne converts to the nearest integer, ties to even.  The
 *               accumulator is int32, (numangle + 2) x (numrho + 2) per frame, frames back to back; its border ring (row 0,
 *               row numangle + 1, column 0, column numrho + 1) is zero and IS written.  A vote whose r falls outside
 *               0 .. numrho - 1 is dropped: that can happen only when rho is of the order of the frame size (rows of a handful
 *               of cells; never while (w + h + 0.5 - sqrt(w^2 + h^2)) / rho >= 1.75), where OpenCV itself would count it in
 *               the ring or beside the row.  Counters are 32-bit throughout.
 *   peaks       a cell b inside the ring is a peak iff a[b] > threshold and a[b] > a[b - 1] and a[b] >= a[b + 1] and
 *               a[b] > a[b - (numrho + 2)] and a[b] >= a[b + (numrho + 2)].  The > / >= asymmetry is part of the
 *               contract (of a plateau of two the left or upper cell survives), so a frame and its transpose need not give
 *               mirrored peaks.  The angle axis does not wrap: row 1 and row numangle see the zero ring.
 *   order       peaks are ordered by votes descending, then by cell index b ascending: a total order, one right answer.
 *               (OpenCV's own std::sort leaves the order of equal votes to the implementation.)
 *   outputs     int32 d_count[f] = the number of peaks of frame f; it may exceed max_lines.
 *               float d_lines[f][max_lines][2]: the first min(count, max_lines) rows hold, for cell (n, r),
 *                 rho   = fl32(fl32((float)r - fl32((float)(numrho - 1) * 0.5f)) * rho_f)
 *                 theta = fl32((float)min_theta + fl32((float)n * theta_f))
 *               int32 d_votes[f][max_lines] (may be NULL): the votes of those rows.  Every remaining row of both, up to
 *               max_lines, is written as zero: the output is a function of the input alone.
 *   MI355_ERR_BAD_ARG, before any device work: a null context or pointer (d_votes and d_accum excepted); w or h outside
 *   1 .. MI355_MAX_WARP_SIZE, nframes < 1; rho or theta that is not finite or not positive (as a double or as a float);
 *   min_theta < 0, max_theta > M_PI (the double; OpenCV's own check has no slack here either, and none is given),
 *   max_theta < min_theta, either not finite; numangle > MI355_MAX_HOUGH_ANGLES; numrho < 1 (rho of 2 (2 (w + h) + 1) or more); an
 *   accumulator of 2^31 bytes or more per frame (or more than 2.4e11 bytes per call); threshold < 0; max_lines outside
 *   1 .. MI355_MAX_HOUGH_LINES; an output pointer that is not 4-byte aligned; ranges that overlap (the input and every
 *   output of the call, each with its own bytes).
 *   mi355_hough_check       pure host function returning the code a lines call with these values returns before any
 *                           device work.
 *   mi355_hough_shape       pure host function: numangle and numrho (either pointer may be NULL).
 *   mi355_hough_trig_table  pure host function: numangle floats each.
 *   mi355_hough_accum_bytes pure host function: nframes * (numangle + 2) * (numrho + 2) * 4, or 0 for rejected values.
 *   mi355_hough_plan        pure host function: how the voting launch cuts these values up — the angle rows a workgroup
 *                           holds in LDS at once, the number of rho ranges a row is split into (1: the row fits), and the
 *                           LDS budget in cells that decides both.  Tests read the limits here instead of restating them.
 *   mi355_hough_accum_gray8_dev   the rules of mi355_filter_dev: the accumulator alone, two launches (point list, votes)
 *                           behind one in-stream memset, no synchronisation.
 *   mi355_hough_lines_gray8_dev   the same and two more launches (peaks, selection) behind a second memset.  d_accum may be
 *                           NULL: the accumulator is then pooled in the context like Canny's parent array; otherwise the
 *                           caller's receives it.  The scratch (4 bytes per frame, then the larger of 4 bytes per pixel
 *                           for the point lists and 8 bytes per numangle * ceil(numrho / 2) for the peak candidates, an
 *                           exact upper bound, not a guess) and the trig table are pooled too: after the first call with
 *                           a given shape and (rho, theta, min_theta, max_theta) — which may allocate and which uploads the
 *                           table, synchronising the stream — a call allocates nothing, waits for nothing and can be
 *                           captured into a hipGraph.  No host round trip between the launches; kernel boundaries are the
 *                           only ordering between workgroups; every loop is bounded.
 *   mi355_hough_lines_gray8_batched   host buffers: H2D, the launches, D2H through the context's pooled buffers; votes may
 *                           be NULL; prof_ns (may be NULL) gets the six timestamps of mi355_filter_batched.  The copies
 *                           of count and votes are enqueued ahead of the lines' and fall into the kernel interval.
 * Not offered: HoughLinesP, the multi-scale form (srn / stn), HoughLinesPointSet, the use_edgeval weighted votes of newer
 * OpenCV, row pitch and ROI, the streamed, group and mi355_pool_alloc forms. */
#define MI355_MAX_HOUGH_ANGLES 1024
#define MI355_MAX_HOUGH_LINES 4096
int mi355_hough_check(int w, int h, int nframes, double rho, double theta, int threshold, int max_lines, double min_theta,
                      double max_theta);
int mi355_hough_shape(int w, int h, double rho, double theta, double min_theta, double max_theta, int* numangle,
                      int* numrho);
int mi355_hough_trig_table(int w, int h, double rho, double theta, double min_theta, double max_theta, float* tab_cos,
                           float* tab_sin);
size_t mi355_hough_accum_bytes(int w, int h, int nframes, double rho, double theta, double min_theta, double max_theta);
int mi355_hough_plan(int w, int h, double rho, double theta, double min_theta, double max_theta, int* angles_per_block,
                     int* rho_splits, int* lds_cells);
int mi355_hough_accum_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_accum, int w, int h, int nframes, double rho,
                                double theta, double min_theta, double max_theta);
int mi355_hough_lines_gray8_dev(mi355_ctx* ctx, const void* d_in, float* d_lines, int32_t* d_votes, int32_t* d_count,
                                int32_t* d_accum, int w, int h, int nframes, double rho, double theta, int threshold,
                                int max_lines, double min_theta, double max_theta);
int mi355_hough_lines_gray8_batched(mi355_ctx* ctx, const uint8_t* in, float* lines, int32_t* votes, int32_t* count, int w,
                                    int h, int nframes, double rho, double theta, int threshold, int max_lines,
                                    double min_theta, double max_theta, uint64_t prof_ns[6]);

/* ---- frames from a decoder or a camera: 8-bit YUV <-> RGBA, cv::cvtColor(COLOR_YUV2RGBA_* / COLOR_RGBA2YUV_*) --------
 * The video decoder writes NV12 surfaces with a pitch, software decoders write I420, webcams deliver YUY2, and an
 * encoder wants NV12 or I420 back.  These calls are the first and the last step of a chain that stays on the device:
 * mi355_yuv_to_rgba8_dev -> mi355_filter_dev ... -> mi355_rgba8_to_yuv_dev, and mi355_yuv_to_gray8_dev in front of every
 * MI355_FILTER_*_GRAY8 id.  Entry points of their own, not filter ids and not a context input format.
 * OpenCV is not installed where this library is built and tested, so THE ARITHMETIC BELOW IS THE CONTRACT.  The BT601
 * constants restate OpenCV's color_yuv code from memory; nobody has compared the result with an OpenCV build here.
 *   geometry  One rule serves a cv::Mat and a decoder surface alike.  A frame is one block of bytes:
 *               pitch  the luma row stride in bytes; 0 = tight: w, or 2 * w for the packed layouts
 *               rows   the number of luma rows the surface holds; 0 = h
 *               frames follow each other at mi355_yuv_frame_bytes(layout, w, h, pitch, rows)
 *             4:2:0 (NV12, NV21, I420, YV12): Y(x, y) is at y * pitch + x; the chroma area starts at rows * pitch.
 *               semi-planar: the pair of pixel (x, y) is at rows * pitch + (y / 2) * pitch + 2 * (x / 2)
 *               planar:      the first chroma plane has pitch / 2 bytes per row and rows / 2 rows, the sample of pixel
 *                            (x, y) at (y / 2) * (pitch / 2) + x / 2 in it; the second plane follows it directly
 *               frame bytes = pitch * rows * 3 / 2.  With pitch = w and rows = h this is exactly OpenCV's
 *               (h * 3 / 2, w) CV_8UC1 layout; a rocDecode / VA-API surface is (its pitch, its aligned height).
 *             packed (YUY2, UYVY): row y is at y * pitch, pixel pair (x, x + 1) at 2 * x in it; frame bytes = pitch * rows.
 *             RGBA and gray8 frames are tightly packed as everywhere else: (nframes, h, w, 4) and (nframes, h, w).
 *   accepted  w, h, nframes as every call here accepts them; w even; for 4:2:0 also h and rows even, and for the planar
 *             layouts pitch even; pitch >= w (>= 2 * w packed); rows >= h; pitch * rows * nframes <= 1.2e11.  Anything
 *             else, an unknown layout or standard included, is MI355_ERR_BAD_ARG.  The encode with a packed layout is
 *             MI355_ERR_UNSUPPORTED.
 *   pointers  d_rgba is dword-aligned (the RGBA rule above); d_yuv and d_gray may have ANY byte alignment, and so may
 *             pitch.  Null pointers and ranges that overlap (the YUV side counted as nframes * frame bytes) are
 *             MI355_ERR_BAD_ARG.  All argument checks come before any device work.
 *   decode    int32 throughout; >> is an arithmetic shift (floor); sat clamps to 0 .. 255:
 *               u = U - 128;  v = V - 128;  y = max(0, Y - YOFF) * CY
 *               R = sat((y + 2^19 + CVR*v) >> 20)
 *               G = sat((y + 2^19 + CVG*v + CUG*u) >> 20)
 *               B = sat((y + 2^19 + CUB*u) >> 20);  A = 255
 *             The chroma sample of a 2 x 2 block (4:2:0) or of a pixel pair (packed) serves all of its pixels; nothing
 *             is interpolated.
 *   encode    Y = sat((CRY*r + CGY*g + CBY*b + 2^19 + (YOFF << 20)) >> 20)     for every pixel
 *             U = sat((CRU*r + CGU*g + CBU*b + 2^19 + (128 << 20)) >> 20)
 *             V = sat((CBU*r + CGV*g + CBV*b + 2^19 + (128 << 20)) >> 20)
 *             U and V are taken from the TOP-LEFT pixel of each 2 x 2 block: OpenCV's rule, not a mean.  Alpha is
 *             ignored.  OpenCV offers the encode for I420 / YV12 only; the NV12 / NV21 encode here is the same
 *             arithmetic stored in the interleaved layout.  Only bytes of pixels are written: the padding of a pitched
 *             surface (columns past w, rows past h) keeps what it held.
 *   constants                  YOFF  CY       CVR      CVG      CUG      CUB
 *               BT601          16    1220542  1673527  -852492  -409993  2116026
 *               BT709          16    1220945  1879825  -558796  -223607  2215014
 *               BT601_FULL     0     1048576  1470104  -748826  -360853  1858077
 *                              CRY     CGY     CBY     CRU      CGU      CBU     CGV      CBV
 *               BT601          269484  528482  102760  -155188  -305135  460324  -385875  -74448
 *               BT709          191455  644067  65019   -105533  -355018  460551  -418321  -42230
 *               BT601_FULL     313524  615514  119538  -176932  -347356  524288  -439026  -85262
 *             BT601 is OpenCV's: (int)(c * 2^20) of its three-decimal 1.164, 1.596, -0.813, -0.391, 2.018 and its own
 *             encode integers — the bit-exact contract with cv::cvtColor.  The other two rows are lround(c * 2^20), in
 *             fp64, of the exact matrix of (Kr, Kb) = (0.2126, 0.0722) and (0.299, 0.114), Kg = 1 - Kr - Kb, with the
 *             range factors sy = 219/255, sc = 224/255 (BT709) and sy = sc = 1 (BT601_FULL):
 *               CY = 1/sy;  CVR = 2(1-Kr)/sc;  CUB = 2(1-Kb)/sc;  CVG = -2Kr(1-Kr)/Kg/sc;  CUG = -2Kb(1-Kb)/Kg/sc
 *               CRY = Kr*sy;  CGY = Kg*sy;  CBY = Kb*sy;  CBU = sc/2
 *               CRU = -Kr/(2(1-Kb))*sc;  CGU = -Kg/(2(1-Kb))*sc;  CGV = -Kg/(2(1-Kr))*sc;  CBV = -Kb/(2(1-Kr))*sc
 *             Every intermediate stays below 2^31 in magnitude for every byte triple and every row of the table.
 *   mi355_yuv_frame_bytes   pure host function: the bytes from one frame to the next, 0 for arguments the calls reject.
 *   mi355_yuv_check         pure host function: the code a call with these values returns before any device work
 *                           (encode != 0: the RGBA -> YUV direction).
 *   mi355_yuv_to_rgba8_dev, mi355_rgba8_to_yuv_dev   the rules of mi355_filter_dev: one launch on the context's stream,
 *                           no synchronisation, no allocation, table or scratch (the constants go by value), so the first
 *                           call a fresh context makes can be captured into a hipGraph.
 *   mi355_yuv_to_gray8_dev  cv::cvtColor(COLOR_YUV2GRAY_*): the Y bytes unchanged, with no range expansion, packed into
 *                           (nframes, h, w) — the feeder of every MI355_FILTER_*_GRAY8 id.  The same rules.
 *   mi355_yuv_to_rgba8_batched, mi355_rgba8_to_yuv_batched   host buffers: H2D, the launch, D2H through the context's
 *                           pooled buffers, each side sized by its own bytes; prof_ns (may be NULL) gets the six
 *                           timestamps of mi355_filter_batched.  The padding of a pitched host result is zero.  The
 *                           context's input format describes the frames of the filter calls, not these: under
 *                           MI355_INPUT_BGR both return MI355_ERR_UNSUPPORTED.
 * Not offered: a YUV input format of the filter calls, 10-bit (P010) and 4:4:4 frames, chroma interpolation, a mean-of-four
 * chroma on encode, one pointer per plane, streamed and group forms. */
#define MI355_YUV_NV12 0 /* Y plane, then rows of interleaved (U, V) pairs     cv::COLOR_YUV2RGBA_NV12 */
#define MI355_YUV_NV21 1 /* Y plane, then rows of interleaved (V, U) pairs     cv::COLOR_YUV2RGBA_NV21 */
#define MI355_YUV_I420 2 /* Y plane, U plane, V plane                          cv::COLOR_YUV2RGBA_I420 / COLOR_RGBA2YUV_I420 */
#define MI355_YUV_YV12 3 /* Y plane, V plane, U plane                          cv::COLOR_YUV2RGBA_YV12 / COLOR_RGBA2YUV_YV12 */
#define MI355_YUV_YUY2 4 /* packed Y0 U Y1 V, 2 bytes per pixel (decode only)  cv::COLOR_YUV2RGBA_YUY2 */
#define MI355_YUV_UYVY 5 /* packed U Y0 V Y1, 2 bytes per pixel (decode only)  cv::COLOR_YUV2RGBA_UYVY */
#define MI355_YUV_BT601 0      /* limited range; OpenCV's constants, the bit-exact contract with cv::cvtColor */
#define MI355_YUV_BT709 1      /* limited range, HD video */
#define MI355_YUV_BT601_FULL 2 /* full range (JFIF / MJPEG cameras) */
size_t mi355_yuv_frame_bytes(int layout, int w, int h, int pitch, int rows);
int mi355_yuv_check(int layout, int standard, int w, int h, int nframes, int pitch, int rows, int encode);
int mi355_yuv_to_rgba8_dev(mi355_ctx* ctx, const void* d_yuv, void* d_rgba, int w, int h, int nframes, int layout,
                           int standard, int pitch, int rows);
int mi355_rgba8_to_yuv_dev(mi355_ctx* ctx, const void* d_rgba, void* d_yuv, int w, int h, int nframes, int layout,
                           int standard, int pitch, int rows);
int mi355_yuv_to_gray8_dev(mi355_ctx* ctx, const void* d_yuv, void* d_gray, int w, int h, int nframes, int layout,
                           int pitch, int rows);
int mi355_yuv_to_rgba8_batched(mi355_ctx* ctx, const uint8_t* yuv, uint8_t* rgba, int w, int h, int nframes, int layout,
                               int standard, int pitch, int rows, uint64_t prof_ns[6]);
int mi355_rgba8_to_yuv_batched(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* yuv, int w, int h, int nframes, int layout,
                               int standard, int pitch, int rows, uint64_t prof_ns[6]);

/* Synthetic frames: px = hash(seed, first_frame + f, y, x), A = 255; mode 1 = smooth
 * gradient + 4-bit noise, mode 2 = flat 64 x 64 patches (constant windows: the content that sends the
 * exact-by-exception kernels down their exception path), mode 3 = gray noise (r = g = b: every pixel on the
 * luminance's ambiguous case).  Bit-identical to oracle_synth_rgba. */
int mi355_synth_rgba8_dev(mi355_ctx* ctx, void* d_out, int w, int h, int nframes, int first_frame,
                          uint32_t seed, int mode);
/* Order-independent 64-bit checksum of nbytes at d_buf (sum of per-word hashes mod 2^64; word i is
 * hashed with index index_base + i), written to *out after synchronising the stream.  Sharding a
 * batch over GPUs and adding the per-rank values gives the single-GPU value. */
int mi355_checksum_dev(mi355_ctx* ctx, const void* d_buf, size_t nbytes, uint64_t index_base,
                       uint64_t* out);

/* Streaming device-to-device copy of nbytes (non-overlapping) on the context's stream, no synchronisation: 16 B per
 * lane, non-temporal loads and stores.  A measurement helper: bench.py times it on the same buffers as the filter
 * to report the box's own "read N + write N bytes" ceiling beside the 8 TB/s spec peak (hipMemcpy D2D is ~25 %
 * slower than this form on MI355X and is not a ceiling).  Replaces nothing in the reference. */
int mi355_stream_copy_dev(mi355_ctx* ctx, void* d_dst, const void* d_src, size_t nbytes);

/* Device self-test of the two fast arithmetic forms the kernels use in place of the reference's FP64 luminance
 * (src/Grayscale/grayscale.cpp:237) and sqrt + round + saturate (src/EdgeDetection/EdgeDetection.cpp:236-240):
 * every one of the 2^24 colours and every (|gx|, |gy|) <= 1020 pair is compared with the exact definition on
 * the GPU the context is bound to.  Both counts are 0 on a correct device / build.  ~1 ms. */
int mi355_selftest(mi355_ctx* ctx, uint32_t* bad_luma, uint32_t* bad_mag);

/* ---- device memory + timing helpers for hosts that do not bring their own ------------------- */
int mi355_dev_alloc(mi355_ctx* ctx, size_t nbytes, void** d_ptr);
/* Frame pools with a placement search.  On MI355X the PHYSICAL placement of a streaming kernel's input and output
 * buffers decides up to 8 % of its rate (the same command reads 5.5 or 6.0 TB/s from one process to the next), and
 * an allocation cannot be steered, only re-drawn.  This call allocates the input pool
 * (nframes x w x h pixels of mi355_filter_in_bpp(filter) bytes, filled with 0xFF) and up to `tries` (<= 16) candidate output pools side by side — all
 * alive at once, hence all in different places; fewer if memory runs short — runs a few launches of `filter` on
 * each, keeps the fastest and frees the others.  tries <= 1: plain allocation, no probing.  probe_ms (optional,
 * `tries` floats): average launch time per candidate, -1 for candidates that were not allocated.  Synchronises
 * the context's stream.  Release with mi355_pool_free.  (Replaces nothing in the reference, which allocates and
 * frees its buffers per frame, RT/src/Controller.cpp:646-652,742-744.) */
int mi355_pool_alloc(mi355_ctx* ctx, int filter, int w, int h, int nframes, int k, float sigma, int tries,
                     void** d_in, void** d_out, float* probe_ms);
int mi355_pool_free(mi355_ctx* ctx, void* d_in, void* d_out);
int mi355_dev_free(mi355_ctx* ctx, void* d_ptr);
int mi355_copy_h2d(mi355_ctx* ctx, void* d_dst, const void* h_src, size_t nbytes);
int mi355_copy_d2h(mi355_ctx* ctx, void* h_dst, const void* d_src, size_t nbytes);
/* hipEvent pair on the context's stream: begin records, end records + synchronises and returns the
 * elapsed milliseconds.  This is the HIP-event timing the roofline figure is computed from. */
int mi355_timer_begin(mi355_ctx* ctx);
int mi355_timer_end(mi355_ctx* ctx, float* elapsed_ms);

/* ---- device group: one batch sharded over several GPUs (SURVEY.md §8b "Threading", §8e) -----------------------------
 * The reference owns one queue on one device (RT/src/ProgramHandler.cpp:108) and has nothing to match; this is the
 * product form of what BASELINE.json's north_star calls the batched-frame mode: independent frames, contiguous
 * frame ranges per GPU, no pixel ever crosses GPUs, no collective.
 *
 * A group = one mi355_ctx + one host worker thread per member.  `devices` lists the HIP device ordinal of each
 * member (NULL = 0 .. ndev-1); an ordinal may repeat (two members then share that GPU on two streams — how the
 * one-GPU tests run it).  Member m of an n-member group owns the frames mi355_group_shard(m, n, nframes) names:
 * base = nframes / n, the first nframes % n members take one extra, ranges contiguous in member order (the same
 * split bench.py's shard_range makes over ranks).
 *
 *   mi355_group_filter_batched  host buffers, nframes frames back to back in `rgba` / `out`: every member streams its
 *                               range through its own mi355_filter_stream (H2D / kernel / D2H overlapped), all
 *                               members at once; returns when all are done.  elapsed_ms (may be NULL): wall time.
 *   mi355_group_filter_dev      device-resident: d_in[m] / d_out[m] are pointers on member m's GPU holding
 *                               nframes[m] frames (0 = member idle); every member launches on its own stream and
 *                               synchronises it; returns when all are done.
 * Gaussian coefficients: a table for (k, sigma) is generated ONCE on the host (mi355_gauss_weights) and the same bytes
 * are installed on every member before the first call that uses the key; mi355_group_set_gauss_weights installs a
 * caller's table on every member.  Mode / impl / input-format setters apply to every member.
 * Status: MI355_OK, or the first failing member's code in member order (mi355_group_member_status gives each
 * member's code of the last call).  One call at a time per group (calls are serialised internally). */
typedef struct mi355_group mi355_group;
int mi355_group_create(int ndev, const int* devices, mi355_group** out);
int mi355_group_destroy(mi355_group* g);
int mi355_group_size(mi355_group* g, int* ndev);
int mi355_group_member_ctx(mi355_group* g, int member, mi355_ctx** ctx); /* borrowed; for alloc / copies / checksums */
int mi355_group_member_status(mi355_group* g, int member);
int mi355_group_shard(int member, int nmembers, int nframes, int* first_frame, int* count); /* pure host function */
int mi355_group_set_gauss_mode(mi355_group* g, int mode);
int mi355_group_set_impl(mi355_group* g, int impl);
int mi355_group_set_input_format(mi355_group* g, int format);
int mi355_group_set_gauss_weights(mi355_group* g, int k, float sigma, const float* w_k2);
int mi355_group_filter_batched(mi355_group* g, int filter, const uint8_t* rgba, uint8_t* out, int w, int h,
                               int nframes, int k, float sigma, double* elapsed_ms);
int mi355_group_filter_dev(mi355_group* g, int filter, const void* const* d_in, void* const* d_out, int w, int h,
                           const int* nframes, int k, float sigma);

/* Library build info: "gfx950;<git-or-date>" */
const char* mi355_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_IMGFILTER_H */
