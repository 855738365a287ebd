// warp_common.hpp — the sampling pieces the geometric kernels share (warp.hip: cv::warpAffine; remap.hip: cv::remap and
// cv::warpPerspective) on top of the wave-per-item frame of wave_common.hpp.  Both give a lane kItemPx = 4 adjacent
// output columns of a row and differ only in where a pixel's source position (sx, sy, fx, fy) comes from; what is done
// with it lives here:
//   load_px     one source pixel by its index in the frame;
//   blend       the LINEAR sum of include/mi355_imgfilter.h, RGBA as (R, B) / (G, A) u16 pairs;
//   sample_at   one output pixel from (sx, sy, fx, fy): with INTERIOR no tap is tested (RGBA LINEAR: the two
//               horizontally adjacent taps of a source row as one 8-byte load), otherwise every index is clamped into
//               the frame and, under BORDER_CONSTANT, the taps that lay outside are replaced.
// No access leaves the frame.
#pragma once

#include "wave_common.hpp"

namespace mi355 {

namespace {

template <int BPP>
__device__ __forceinline__ uint32_t load_px(global_ptr<const uint8_t> src, uint32_t pixel)
{
    return load_px_at<BPP>(src + pixel * (uint32_t)BPP);
}

// (wx0 p00 + wx1 p01) wy0 + (wx0 p10 + wx1 p11) wy1 + 512 >> 10 per channel: the four products of the header's sum,
// regrouped (integers, nothing is rounded in between).  RGBA rows are blended as (R, B) and (G, A) u16 pairs:
// 32 * 255 < 65536.
template <int BPP>
__device__ __forceinline__ uint32_t blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t fx,
                                          uint32_t fy)
{
    const uint32_t wx0 = 32u - fx, wx1 = fx, wy0 = 32u - fy, wy1 = fy;
    if constexpr (BPP == 4) {
        const uint32_t m = 0x00FF00FFu;
        const uint32_t h0rb = (p00 & m) * wx0 + (p01 & m) * wx1, h0ga = ((p00 >> 8) & m) * wx0 + ((p01 >> 8) & m) * wx1;
        const uint32_t h1rb = (p10 & m) * wx0 + (p11 & m) * wx1, h1ga = ((p10 >> 8) & m) * wx0 + ((p11 >> 8) & m) * wx1;
        const uint32_t r = ((h0rb & 0xFFFFu) * wy0 + (h1rb & 0xFFFFu) * wy1 + 512u) >> 10;
        const uint32_t b = ((h0rb >> 16) * wy0 + (h1rb >> 16) * wy1 + 512u) >> 10;
        const uint32_t g = ((h0ga & 0xFFFFu) * wy0 + (h1ga & 0xFFFFu) * wy1 + 512u) >> 10;
        const uint32_t al = ((h0ga >> 16) * wy0 + (h1ga >> 16) * wy1 + 512u) >> 10;
        return r | (g << 8) | (b << 16) | (al << 24);
    } else {
        return ((p00 * wx0 + p01 * wx1) * wy0 + (p10 * wx0 + p11 * wx1) * wy1 + 512u) >> 10;
    }
}

// one output pixel from its source position: the tap (sx, sy), and for LINEAR its three neighbours weighted by the
// 1/32-pixel fractions (fx, fy); `border` is the RGBA border pixel or the gray8 border byte
template <int BPP, int INTERP, int BORDER, bool INTERIOR, class Args>
__device__ __forceinline__ uint32_t sample_at(global_ptr<const uint8_t> src, const Args& a, int sx, int sy, uint32_t fx,
                                              uint32_t fy)
{
    if constexpr (INTERP == kNearest) {
        if constexpr (INTERIOR) {
            return load_px<BPP>(src, (uint32_t)sy * (uint32_t)a.sw + (uint32_t)sx);
        } else {
            const bool in = (unsigned)sx < (unsigned)a.sw && (unsigned)sy < (unsigned)a.sh;
            const uint32_t v = load_px<BPP>(src, (uint32_t)clampi(sy, 0, a.sh - 1) * (uint32_t)a.sw +
                                                     (uint32_t)clampi(sx, 0, a.sw - 1));
            return (BORDER == kConstant && !in) ? a.border : v;
        }
    } else {
        uint32_t p00, p01, p10, p11;
        if constexpr (INTERIOR) {
            const uint32_t at = (uint32_t)sy * (uint32_t)a.sw + (uint32_t)sx;
            if constexpr (BPP == 4) {
                const u32x2 r0 = gload_a4<u32x2>(src + at * 4u);
                const u32x2 r1 = gload_a4<u32x2>(src + (at + (uint32_t)a.sw) * 4u);
                p00 = r0.x;
                p01 = r0.y;
                p10 = r1.x;
                p11 = r1.y;
            } else {
                p00 = load_px<1>(src, at);
                p01 = load_px<1>(src, at + 1u);
                p10 = load_px<1>(src, at + (uint32_t)a.sw);
                p11 = load_px<1>(src, at + (uint32_t)a.sw + 1u);
            }
        } else {
            const bool x0in = (unsigned)sx < (unsigned)a.sw, x1in = (unsigned)(sx + 1) < (unsigned)a.sw;
            const bool y0in = (unsigned)sy < (unsigned)a.sh, y1in = (unsigned)(sy + 1) < (unsigned)a.sh;
            const uint32_t u0 = (uint32_t)clampi(sx, 0, a.sw - 1), u1 = (uint32_t)clampi(sx + 1, 0, a.sw - 1);
            const uint32_t v0 = (uint32_t)clampi(sy, 0, a.sh - 1) * (uint32_t)a.sw;
            const uint32_t v1 = (uint32_t)clampi(sy + 1, 0, a.sh - 1) * (uint32_t)a.sw;
            p00 = load_px<BPP>(src, v0 + u0);
            p01 = load_px<BPP>(src, v0 + u1);
            p10 = load_px<BPP>(src, v1 + u0);
            p11 = load_px<BPP>(src, v1 + u1);
            if constexpr (BORDER == kConstant) {
                p00 = (x0in && y0in) ? p00 : a.border;
                p01 = (x1in && y0in) ? p01 : a.border;
                p10 = (x0in && y1in) ? p10 : a.border;
                p11 = (x1in && y1in) ? p11 : a.border;
            }
        }
        return blend<BPP>(p00, p01, p10, p11, fx, fy);
    }
}

}  // namespace

}  // namespace mi355
