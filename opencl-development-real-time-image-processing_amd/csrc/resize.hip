// resize.hip — cv::resize of 8-bit frames (include/mi355_imgfilter.h, "Changing the frame size"): NEAREST, LINEAR
// (OpenCV's 11-bit fixed-point path) and AREA with integer factors, RGBA (every channel on its own) and gray8.
//
// One kernel template over <bytes per pixel, interpolation, AREA vector width>.  A work item is one wave walking one
// (frame, band of output rows, strip of 256 output columns): a lane owns kResizePx = 4 adjacent output columns, so a
// full RGBA lane stores 16 bytes per row and a full gray8 lane one dword where the row's address allows it (byte stores
// at a ragged right end and at odd alignments).  Scales and sizes come by value; a lane works out its columns' source
// offsets and weights once, in the fp64 / fp32 operations the header states, then walks its band:
//   LINEAR   keeps H(r0) >> 4 and H(r1) >> 4 of its columns in registers as int (OpenCV's row cache).  When the next
//            output row's (r0, r1) moves on by one source row the old H(r1) becomes H(r0) and one row is fetched; when it
//            does not move (upscaling) nothing is fetched.  (sy, b0, b1) is wave-uniform, once per row.
//   NEAREST  one gather per output pixel, no band state.
//   AREA     each lane sums its nx x ny blocks, RGBA as packed (R,B) / (G,A) u16 pairs (16 * 16 * 255 < 65536).  Factors
//            2 and 4 in x read the lane's contiguous source span with 16-byte loads (gray8: where the row is
//            dword-aligned); other factors, ragged strips and odd alignments read pixel by pixel.
// Source reads go straight from global memory; neighbouring lanes share cache lines.  Every source index is clamped into
// the frame (lanes past the right end repeat the last column and store nothing), so no access leaves a frame.
#include "wave_common.hpp"

namespace mi355 {

namespace {

constexpr int kResizePx = 4;                      // output columns per lane
constexpr int kResizeStrip = kWave * kResizePx;   // output columns per wave
static_assert(kResizePx == kItemPx, "wave_item and warp_store give a lane kItemPx columns");
constexpr int kResizeBandMax = 16;                // output rows per band, halved while the launch has few waves
constexpr size_t kResizeMinWork = 4096;           // ~4 waves per SIMD before bands grow

constexpr int kArea = 3;  // MI355_INTERP_AREA, beside kNearest and kLinear

struct ResizeArgs {
    const uint8_t* in;
    uint8_t* out;
    int sw, sh, dw, dh;
    int nstrips, nbands, band_rows;
    uint32_t nwork;
    double scale_x, scale_y;  // 1.0 / ((double)dst / (double)src), from the host
    int nx, ny;               // AREA: integer factors
    float area_scale;         // AREA: 1.f / (float)(nx * ny), from the host
};

// LINEAR: H(row) >> 4 of the lane's columns, every channel: src[sx] * a0 + src[min(sx + 1, sw - 1)] * a1
template <int BPP>
__device__ __forceinline__ void fetch_h(global_ptr<const uint8_t> rowp, const uint32_t (&off0)[kResizePx],
                                        const uint32_t (&off1)[kResizePx], const int (&a0)[kResizePx],
                                        const int (&a1)[kResizePx], int (&H)[kResizePx * BPP])
{
    uint32_t p0[kResizePx], p1[kResizePx];
#pragma unroll
    for (int j = 0; j < kResizePx; j++) {
        p0[j] = load_px_at<BPP>(rowp + off0[j]);
        p1[j] = load_px_at<BPP>(rowp + off1[j]);
    }
#pragma unroll
    for (int j = 0; j < kResizePx; j++)
#pragma unroll
        for (int c = 0; c < BPP; c++)
            H[j * BPP + c] = ((int)((p0[j] >> (8 * c)) & 0xFFu) * a0[j] + (int)((p1[j] >> (8 * c)) & 0xFFu) * a1[j]) >> 4;
}

// AREA: one channel's block sum to its output byte
__device__ __forceinline__ uint32_t area_byte(uint32_t sum, float scale)
{
    const float v = __builtin_rintf((float)sum * scale);  // fp32 product, half to even; never the exact quotient
    return __builtin_amdgcn_cvt_pk_u8_f32(v, 0u, 0u);     // saturates; v is an integer already
}

template <int BPP, int INTERP, int NX>
__global__ __launch_bounds__(kItemWaves* kWave) void resize_kernel(const ResizeArgs a)
{
    // The decode stays in place, not wave_item's: through it the argument loads come in other groups, and LINEAR RGBA
    // 4K -> 720p ran 0.5 % slower in three of four runs (profiles/wave_frame_ab.txt).
    const uint32_t work = __builtin_amdgcn_readfirstlane(blockIdx.x * kItemWaves + (uint32_t)(threadIdx.x >> 6));
    if (work >= a.nwork)
        return;
    const int lane = threadIdx.x & 63;
    const int strip = (int)(work % (uint32_t)a.nstrips);
    const uint32_t t = work / (uint32_t)a.nstrips;
    const int band = (int)(t % (uint32_t)a.nbands);
    const size_t frame = t / (uint32_t)a.nbands;
    const int y0 = band * a.band_rows, y1 = min(y0 + a.band_rows, a.dh);
    const int x0 = strip * kResizeStrip + lane * kResizePx;
    const bool ragged = (strip + 1) * kResizeStrip > a.dw;  // wave-uniform: the last strip of a row that does not fill it
    const size_t src_row = (size_t)a.sw * BPP, dst_row = (size_t)a.dw * BPP;
    const uint8_t* src = a.in + frame * (src_row * (size_t)a.sh);
    uint8_t* dst = a.out + frame * (dst_row * (size_t)a.dh);
    uint32_t px[kResizePx];

    if constexpr (INTERP == kLinear) {
        uint32_t off0[kResizePx], off1[kResizePx];
        int a0[kResizePx], a1[kResizePx];
#pragma unroll
        for (int j = 0; j < kResizePx; j++) {
            const int dx = min(x0 + j, a.dw - 1);
            float fx = (float)(((double)dx + 0.5) * a.scale_x - 0.5);
            int sx = (int)__builtin_floorf(fx);
            fx = fx - (float)sx;
            if (sx < 0) {
                sx = 0;
                fx = 0.0f;
            }
            if (sx >= a.sw - 1) {
                sx = a.sw - 1;
                fx = 0.0f;
            }
            a0[j] = (int)__builtin_rintf((1.0f - fx) * 2048.0f);
            a1[j] = (int)__builtin_rintf(fx * 2048.0f);
            off0[j] = (uint32_t)sx * BPP;
            off1[j] = (uint32_t)min(sx + 1, a.sw - 1) * BPP;
        }
        int H0[kResizePx * BPP], H1[kResizePx * BPP];
        int row0 = -1, row1 = -1;  // the source rows H0 / H1 hold
        for (int dy = y0; dy < y1; dy++) {
            float fy = (float)(((double)dy + 0.5) * a.scale_y - 0.5);
            const int sy = (int)__builtin_floorf(fy);
            fy = fy - (float)sy;
            const int b0 = (int)__builtin_rintf((1.0f - fy) * 2048.0f);
            const int b1 = (int)__builtin_rintf(fy * 2048.0f);
            const int r0 = __builtin_amdgcn_readfirstlane(clampi(sy, 0, a.sh - 1));
            const int r1 = __builtin_amdgcn_readfirstlane(clampi(sy + 1, 0, a.sh - 1));
            if (r0 != row0) {
                if (r0 == row1) {
#pragma unroll
                    for (int i = 0; i < kResizePx * BPP; i++)
                        H0[i] = H1[i];
                } else {
                    fetch_h<BPP>(uniform_ptr(src + (size_t)r0 * src_row), off0, off1, a0, a1, H0);
                }
                row0 = r0;
            }
            if (r1 != row1) {
                if (r1 == row0) {
#pragma unroll
                    for (int i = 0; i < kResizePx * BPP; i++)
                        H1[i] = H0[i];
                } else {
                    fetch_h<BPP>(uniform_ptr(src + (size_t)r1 * src_row), off0, off1, a0, a1, H1);
                }
                row1 = r1;
            }
#pragma unroll
            for (int j = 0; j < kResizePx; j++) {
                px[j] = 0u;
#pragma unroll
                for (int c = 0; c < BPP; c++) {
                    const int v = (((b0 * H0[j * BPP + c]) >> 16) + ((b1 * H1[j * BPP + c]) >> 16) + 2) >> 2;
                    px[j] |= (uint32_t)v << (8 * c);
                }
            }
            warp_store<BPP>(uniform_ptr(dst + (size_t)dy * dst_row), x0, a.dw, px);
        }
    } else if constexpr (INTERP == kNearest) {
        uint32_t off[kResizePx];
#pragma unroll
        for (int j = 0; j < kResizePx; j++) {
            const int dx = min(x0 + j, a.dw - 1);
            off[j] = (uint32_t)min((int)__builtin_floor((double)dx * a.scale_x), a.sw - 1) * BPP;
        }
        for (int dy = y0; dy < y1; dy++) {
            const int sy =
                __builtin_amdgcn_readfirstlane(min((int)__builtin_floor((double)dy * a.scale_y), a.sh - 1));
            const global_ptr<const uint8_t> rowp = uniform_ptr(src + (size_t)sy * src_row);
#pragma unroll
            for (int j = 0; j < kResizePx; j++)
                px[j] = load_px_at<BPP>(rowp + off[j]);
            warp_store<BPP>(uniform_ptr(dst + (size_t)dy * dst_row), x0, a.dw, px);
        }
    } else {
        const int nx = a.nx, ny = a.ny;
        uint32_t col[kResizePx];  // byte offset of each column's block inside a source row
#pragma unroll
        for (int j = 0; j < kResizePx; j++)
            col[j] = (uint32_t)min(x0 + j, a.dw - 1) * (uint32_t)nx * BPP;
        const bool shift2 = nx == 2 && ny == 2;
        for (int dy = y0; dy < y1; dy++) {
            // RGBA: lo = (R, B), hi = (G, A) as u16 pairs; gray8: lo alone
            uint32_t lo[kResizePx] = {0u, 0u, 0u, 0u}, hi[kResizePx] = {0u, 0u, 0u, 0u};
            for (int r = 0; r < ny; r++) {
                const global_ptr<const uint8_t> rowp = uniform_ptr(src + ((size_t)dy * ny + r) * src_row);
                bool wide = NX != 0 && !ragged;
                if constexpr (NX != 0 && BPP == 1)
                    wide = wide && (reinterpret_cast<uint64_t>(rowp) & 3u) == 0;
                if (wide) {  // wave-uniform: the lane's 4 * NX source pixels are one contiguous, dword-aligned span
                    if constexpr (NX != 0 && BPP == 4) {
#pragma unroll
                        for (int q = 0; q < NX; q++) {
                            const u32x4 v = gload_a4<u32x4>(rowp + col[0] + 16u * q);
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                lo[(4 * q + e) / NX] += v[e] & 0x00FF00FFu;
                                hi[(4 * q + e) / NX] += (v[e] >> 8) & 0x00FF00FFu;
                            }
                        }
                    } else if constexpr (NX != 0) {
                        uint32_t v[NX];
                        if constexpr (NX == 2) {
                            const u32x2 d = gload_a4<u32x2>(rowp + col[0]);
                            v[0] = d.x;
                            v[1] = d.y;
                        } else {
                            const u32x4 d = gload_a4<u32x4>(rowp + col[0]);
                            v[0] = d.x;
                            v[1] = d.y;
                            v[2] = d.z;
                            v[3] = d.w;
                        }
#pragma unroll
                        for (int e = 0; e < 4 * NX; e++)
                            lo[e / NX] += (v[e / 4] >> (8 * (e % 4))) & 0xFFu;
                    }
                } else {
                    for (int i = 0; i < nx; i++) {
#pragma unroll
                        for (int j = 0; j < kResizePx; j++) {
                            const uint32_t p = load_px_at<BPP>(rowp + col[j] + (uint32_t)i * BPP);
                            if constexpr (BPP == 4) {
                                lo[j] += p & 0x00FF00FFu;
                                hi[j] += (p >> 8) & 0x00FF00FFu;
                            } else {
                                lo[j] += p;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kResizePx; j++) {
                if constexpr (BPP == 4) {
                    if (shift2) {
                        px[j] = (((lo[j] + 0x00020002u) >> 2) & 0x00FF00FFu) |
                                ((((hi[j] + 0x00020002u) >> 2) & 0x00FF00FFu) << 8);
                    } else {
                        px[j] = area_byte(lo[j] & 0xFFFFu, a.area_scale) | (area_byte(hi[j] & 0xFFFFu, a.area_scale) << 8) |
                                (area_byte(lo[j] >> 16, a.area_scale) << 16) | (area_byte(hi[j] >> 16, a.area_scale) << 24);
                    }
                } else {
                    px[j] = shift2 ? (lo[j] + 2u) >> 2 : area_byte(lo[j], a.area_scale);
                }
            }
            warp_store<BPP>(uniform_ptr(dst + (size_t)dy * dst_row), x0, a.dw, px);
        }
    }
}

}  // namespace

bool resize_area_factors(int src_w, int src_h, int dst_w, int dst_h, int* nx, int* ny)
{
    if (dst_w <= 0 || dst_h <= 0 || src_w % dst_w != 0 || src_h % dst_h != 0)
        return false;
    const int n = src_w / dst_w, m = src_h / dst_h;
    if (n < 1 || m < 1 || n > kResizeMaxAreaFactor || m > kResizeMaxAreaFactor)
        return false;
    *nx = n;
    *ny = m;
    return true;
}

hipError_t launch_resize(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                         int dst_w, int dst_h, int nframes, int interp)
{
    if ((bpp != 1 && bpp != 4) || (interp != kNearest && interp != kLinear && interp != kArea))
        return hipErrorInvalidValue;
    // lane offsets inside a row are 32-bit
    if ((size_t)src_w * 4 > 0x7FFFFFFFull || (size_t)dst_w * 4 > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    ResizeArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.sw = src_w;
    a.sh = src_h;
    a.dw = dst_w;
    a.dh = dst_h;
    a.scale_x = 1.0 / ((double)dst_w / (double)src_w);  // not src_w / dst_w: the two differ in the last bit
    a.scale_y = 1.0 / ((double)dst_h / (double)src_h);
    a.nx = a.ny = 1;
    a.area_scale = 1.0f;
    if (interp == kLinear && src_w == 2 * (int64_t)dst_w && src_h == 2 * (int64_t)dst_h)
        interp = kArea;  // OpenCV switches there
    if (interp == kArea) {
        if (!resize_area_factors(src_w, src_h, dst_w, dst_h, &a.nx, &a.ny))
            return hipErrorInvalidValue;
        a.area_scale = 1.0f / (float)(a.nx * a.ny);
    }
    a.nstrips = (dst_w + kResizeStrip - 1) / kResizeStrip;
    a.band_rows = kResizeBandMax;
    auto nwork = [&](int rows) { return band_items(a.nstrips, dst_h, rows, nframes); };
    while (a.band_rows > 1 && nwork(a.band_rows) < kResizeMinWork)
        a.band_rows /= 2;
    if (!plan_bands(&a, dst_h, nframes))
        return hipErrorInvalidValue;
    // AREA reads its lane's span of x-factor 2 or 4 in 16-byte loads
    const int nx_wide = (interp == kArea && (a.nx == 2 || a.nx == 4)) ? a.nx : 0;
    return dispatch_int(bpp, std::integer_sequence<int, 1, 4>{}, [&](auto BPP) {
        return dispatch_int(interp, std::integer_sequence<int, kNearest, kLinear, kArea>{}, [&](auto INTERP) {
            return dispatch_int(nx_wide, std::integer_sequence<int, 0, 2, 4>{}, [&](auto NX) {
                if constexpr (INTERP.value == kArea || NX.value == 0)
                    return launch_items(resize_kernel<BPP.value, INTERP.value, NX.value>, stream, a);
                else
                    return hipErrorInvalidValue;
            });
        });
    });
}

}  // namespace mi355
