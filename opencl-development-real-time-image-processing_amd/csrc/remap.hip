// remap.hip — cv::remap through one per-pixel map and cv::warpPerspective of 8-bit frames (include/mi355_imgfilter.h,
// "Undistorting and rectifying frames"): NEAREST and LINEAR on the 1/32-pixel grid, BORDER_CONSTANT and
// BORDER_REPLICATE, RGBA (every channel on its own) and gray8.
//
// One kernel template over <bytes per pixel, interpolation, border mode, coordinate source>.  The work decomposition
// is warp.hip's: one wave owns a 2-D tile of output pixels, a lane owns kItemPx = 4 adjacent output columns, 2^lx_log2
// lanes sit side by side and the 64 >> lx_log2 lane rows walk the tile top to bottom one row pass at a time; tiles are
// ordered row-major and blocks go through xcd_remap.  What differs is where a pixel's source position comes from:
//   perspective  the nine doubles by value; a lane keeps h0 x, h3 x, h6 x of its four columns in registers, computes
//                the three row terms once per row it walks and pays one fp64 division per pixel;
//   FIXED map    16 bytes of (sx, sy) int16 pairs per lane and row, then for LINEAR 8 bytes of fy*32+fx words;
//   FLOAT map    16 bytes of x and 16 bytes of y per lane and row, converted as the header states.
// A lane whose four columns reach past the row's end reads the entries one by one with the column clamped (it repeats
// the last column and stores nothing); a lane row past the tile's last row repeats that row and stores nothing.  So no
// access leaves a map, and every lane always holds four valid source positions.
// One map or matrix serves all frames, so a work item may own its tile across a chunk of `fchunk` consecutive frames
// (the last chunk of a batch is ragged): the positions of a row pass stay in registers and are applied frame by frame.
// The chunk length and the tile are measured choices (kernels.hpp, profiles/remap_rate.txt).
// Whether a row pass runs without border tests does not rest on geometry — a map has none.  Every lane tests its own
// four positions, the wave votes, and a uniform branch takes either the path with no per-tap test (RGBA LINEAR: 8-byte
// paired loads) or the one that clamps every index and replaces outside taps.  The vote is exact by construction.
#include <cmath>
#include <cstdio>

#include "warp_common.hpp"

namespace mi355 {

namespace {

constexpr int kSrcPerspective = 0, kSrcFixed = 1, kSrcFloat = 2;

struct RemapArgs {
    const uint8_t* in;
    uint8_t* out;
    const uint8_t* map1;  // FIXED: int16 (sx, sy) pairs; FLOAT: the x plane; perspective: unused
    const uint8_t* map2;  // FIXED: uint16 fy*32+fx (LINEAR only); FLOAT: the y plane
    int sw, sh, dw, dh;
    int lx_log2;  // lanes side by side in a tile: tile width = kItemPx << lx_log2
    int tile_h;   // output rows per tile, a multiple of 64 >> lx_log2
    int tiles_x, tiles_y;
    int nframes;
    int fchunk;  // consecutive frames per work item
    uint32_t nwork;
    uint32_t border;  // RGBA: the border pixel; gray8: its byte
    double h0, h1, h2, h3, h4, h5, h6, h7, h8;
};

template <typename V>
__device__ __forceinline__ V gload_a2(global_ptr<const uint8_t> p)
{
    typedef V __attribute__((aligned(2))) VA;
    return *(global_ptr<const VA>)p;
}

// a FLOAT map entry, already multiplied by S, as int: round half even; NaN and anything <= -2^31 give INT_MIN,
// anything >= 2^31 gives INT_MAX
__device__ __forceinline__ int map_round(float t)
{
    const int r = (int)__builtin_rintf(t);
    return !(t > -2147483648.0f) ? (int)0x80000000 : (t >= 2147483648.0f ? 0x7FFFFFFF : r);
}

// a perspective coordinate, already multiplied by s, as int: NaN and anything >= 2^31 - 1 give INT_MAX
__device__ __forceinline__ int persp_round(double t)
{
    double f = !(t < 2147483647.0) ? 2147483647.0 : t;
    f = f < -2147483648.0 ? -2147483648.0 : f;
    return (int)__builtin_rint(f);
}

// (X, Y) of the header -> the tap and its 1/32-pixel fractions.  OpenCV's saturation of sx, sy to short is dropped: with
// sizes up to kWarpMaxSize a saturated index lies outside the frame just as the unsaturated one does.
template <int INTERP>
__device__ __forceinline__ void split(int X, int Y, int& sx, int& sy, uint32_t& fx, uint32_t& fy)
{
    if constexpr (INTERP == kLinear) {
        sx = X >> 5;
        sy = Y >> 5;
        fx = (uint32_t)X & 31u;
        fy = (uint32_t)Y & 31u;
    } else {
        sx = X;
        sy = Y;
        fx = fy = 0;
    }
}

// the source positions of the lane's four columns of output row y, read from the map
template <int INTERP, int SOURCE>
__device__ __forceinline__ void map_coords(const RemapArgs& a, global_ptr<const uint8_t> map1,
                                           global_ptr<const uint8_t> map2, int x0, int y, int (&sx)[kItemPx],
                                           int (&sy)[kItemPx], uint32_t (&fx)[kItemPx], uint32_t (&fy)[kItemPx])
{
    const uint32_t row = (uint32_t)y * (uint32_t)a.dw;  // entries are 32-bit indices (launch: dw, dh <= kWarpMaxSize)
    uint32_t e1[kItemPx], e2[kItemPx] = {};
    constexpr bool second = SOURCE == kSrcFloat || INTERP == kLinear;
    if (x0 + kItemPx <= a.dw) {
        const uint64_t at = (uint64_t)(row + (uint32_t)x0);
        const u32x4 v = gload_a4<u32x4>(map1 + at * 4u);
        e1[0] = v.x, e1[1] = v.y, e1[2] = v.z, e1[3] = v.w;
        if constexpr (SOURCE == kSrcFloat) {
            const u32x4 u = gload_a4<u32x4>(map2 + at * 4u);
            e2[0] = u.x, e2[1] = u.y, e2[2] = u.z, e2[3] = u.w;
        } else if constexpr (second) {
            const u32x2 u = gload_a2<u32x2>(map2 + at * 2u);
            e2[0] = u.x & 0xFFFFu, e2[1] = u.x >> 16, e2[2] = u.y & 0xFFFFu, e2[3] = u.y >> 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kItemPx; j++) {
            const uint64_t at = (uint64_t)(row + (uint32_t)min(x0 + j, a.dw - 1));
            e1[j] = gload<uint32_t>(map1 + at * 4u);
            if constexpr (SOURCE == kSrcFloat)
                e2[j] = gload<uint32_t>(map2 + at * 4u);
            else if constexpr (second)
                e2[j] = gload<uint16_t>(map2 + at * 2u);
        }
    }
#pragma unroll
    for (int j = 0; j < kItemPx; j++) {
        if constexpr (SOURCE == kSrcFloat) {
            constexpr float S = INTERP == kLinear ? 32.0f : 1.0f;
            split<INTERP>(map_round(__uint_as_float(e1[j]) * S), map_round(__uint_as_float(e2[j]) * S), sx[j], sy[j],
                          fx[j], fy[j]);
        } else {
            sx[j] = (int)(int16_t)(e1[j] & 0xFFFFu);
            sy[j] = (int)e1[j] >> 16;
            fx[j] = e2[j] & 31u;
            fy[j] = (e2[j] >> 5) & 31u;
        }
    }
}

// one row pass: the lane's four positions applied to the `nf` frames of the chunk
template <int BPP, int INTERP, int BORDER, bool INTERIOR>
__device__ __forceinline__ void row_pass(const RemapArgs& a, global_ptr<const uint8_t> src, global_ptr<uint8_t> dst,
                                         int nf, int x0, int y, bool live, const int (&sx)[kItemPx],
                                         const int (&sy)[kItemPx], const uint32_t (&fx)[kItemPx],
                                         const uint32_t (&fy)[kItemPx])
{
    const size_t src_frame = (size_t)a.sw * a.sh * BPP, dst_frame = (size_t)a.dw * a.dh * BPP;
    const uint32_t row = (uint32_t)y * (uint32_t)a.dw * (uint32_t)BPP;
    for (int f = 0; f < nf; f++) {
        uint32_t px[kItemPx];
#pragma unroll
        for (int j = 0; j < kItemPx; j++)
            px[j] = sample_at<BPP, INTERP, BORDER, INTERIOR>(src, a, sx[j], sy[j], fx[j], fy[j]);
        if (live)
            warp_store<BPP>(dst + row, x0, a.dw, px);
        src += src_frame;
        dst += dst_frame;
    }
}

template <int BPP, int INTERP, int BORDER, int SOURCE>
__global__ __launch_bounds__(kItemWaves* kWave) void remap_kernel(const RemapArgs a)
{
    WaveItem it;
    if (!wave_item(xcd_remap(blockIdx.x, gridDim.x), a.nwork, a.tiles_x, a.tiles_y, a.lx_log2, a.tile_h, a.dh, &it))
        return;
    const int frame0 = (int)it.frame * a.fchunk;  // the chunk's first frame
    const int nf = min(a.fchunk, a.nframes - frame0);
    const int x0 = it.x0, ty0 = it.y0, ty_end = it.y_end, ly = it.ly, y_step = it.y_step;
    const global_ptr<const uint8_t> src = uniform_ptr(a.in + (size_t)frame0 * ((size_t)a.sw * a.sh * BPP));
    const global_ptr<uint8_t> dst = uniform_ptr(a.out + (size_t)frame0 * ((size_t)a.dw * a.dh * BPP));
    const global_ptr<const uint8_t> map1 = uniform_ptr(a.map1), map2 = uniform_ptr(a.map2);

    // perspective: the column terms of the lane's four columns
    double cx[kItemPx], cy[kItemPx], cw[kItemPx];
    if constexpr (SOURCE == kSrcPerspective) {
#pragma unroll
        for (int j = 0; j < kItemPx; j++) {
            const double x = (double)min(x0 + j, a.dw - 1);
            cx[j] = a.h0 * x;
            cy[j] = a.h3 * x;
            cw[j] = a.h6 * x;
        }
    }

    constexpr int reach = INTERP == kLinear ? 1 : 0;
    for (int yb = ty0; yb < ty_end; yb += y_step) {  // wave-uniform: every lane takes part in every pass's vote
        const bool live = yb + ly < ty_end;
        const int y = min(yb + ly, ty_end - 1);
        int sx[kItemPx], sy[kItemPx];
        uint32_t fx[kItemPx], fy[kItemPx];
        if constexpr (SOURCE == kSrcPerspective) {
            constexpr double S = INTERP == kLinear ? 32.0 : 1.0;
            const double yd = (double)y;
            const double rx = a.h1 * yd + a.h2, ry = a.h4 * yd + a.h5, rw = a.h7 * yd + a.h8;
#pragma unroll
            for (int j = 0; j < kItemPx; j++) {
                const double w = cw[j] + rw;
                const double s = (w != 0.0) ? S / w : 0.0;
                split<INTERP>(persp_round((cx[j] + rx) * s), persp_round((cy[j] + ry) * s), sx[j], sy[j], fx[j], fy[j]);
            }
        } else {
            map_coords<INTERP, SOURCE>(a, map1, map2, x0, y, sx, sy, fx, fy);
        }
        bool inside = true;
#pragma unroll
        for (int j = 0; j < kItemPx; j++)
            inside = inside && (unsigned)sx[j] < (unsigned)(a.sw - reach) && (unsigned)sy[j] < (unsigned)(a.sh - reach);
        if (__all(inside))
            row_pass<BPP, INTERP, BORDER, true>(a, src, dst, nf, x0, y, live, sx, sy, fx, fy);
        else
            row_pass<BPP, INTERP, BORDER, false>(a, src, dst, nf, x0, y, live, sx, sy, fx, fy);
    }
}

// The tile and the frames per work item of a launch (kernels.hpp).  The tune build takes
// MI355_TUNE_REMAP_TILE=<lanes across, log2>x<rows> and MI355_TUNE_REMAP_FRAMES=<frames> for the A/B of
// tools/remap_rate.py.
void work_shape(int* lx_log2, int* tile_h, int* fchunk)
{
    *lx_log2 = kRemapLanesLog2;
    *tile_h = kRemapTileH;
    *fchunk = kRemapFrames;
    tune_tile("MI355_TUNE_REMAP_TILE", lx_log2, tile_h);
    if (const char* e = tune_env("MI355_TUNE_REMAP_FRAMES")) {
        int f = 0;
        if (sscanf(e, "%d", &f) == 1 && f >= 1 && f <= 64)
            *fchunk = f;
    }
}

hipError_t launch(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h, int dst_w,
                  int dst_h, int nframes, int source, const void* d_map1, const void* d_map2, const double* h,
                  int interp, int border_mode, uint32_t border_value)
{
    RemapArgs a{};
    work_shape(&a.lx_log2, &a.tile_h, &a.fchunk);
    if (!tile_args(&a, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, remap_work_items(dst_w, dst_h, nframes), interp,
                   border_mode, border_value))
        return hipErrorInvalidValue;
    a.map1 = static_cast<const uint8_t*>(d_map1);
    a.map2 = static_cast<const uint8_t*>(d_map2);
    a.nframes = nframes;
    if (h) {
        a.h0 = h[0], a.h1 = h[1], a.h2 = h[2];
        a.h3 = h[3], a.h4 = h[4], a.h5 = h[5];
        a.h6 = h[6], a.h7 = h[7], a.h8 = h[8];
    }
    return dispatch_geom(bpp, interp, border_mode, [&](auto BPP, auto INTERP, auto BORDER) {
        constexpr std::integer_sequence<int, kSrcPerspective, kSrcFixed, kSrcFloat> sources{};
        return dispatch_int(source, sources, [&](auto SOURCE) {
            return launch_items(remap_kernel<BPP.value, INTERP.value, BORDER.value, SOURCE.value>, stream, a);
        });
    });
}

}  // namespace

uint64_t remap_work_items(int dst_w, int dst_h, int nframes)
{
    if (dst_w <= 0 || dst_h <= 0 || nframes <= 0)
        return 0;
    int lx_log2 = 0, tile_h = 0, fchunk = 1;
    work_shape(&lx_log2, &tile_h, &fchunk);
    return tile_items(dst_w, dst_h, lx_log2, tile_h, (nframes + fchunk - 1) / fchunk);
}

hipError_t launch_remap(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                        int dst_w, int dst_h, int nframes, const void* d_map1, const void* d_map2, int map_kind,
                        int interp, int border_mode, uint32_t border_value)
{
    if ((map_kind != 0 && map_kind != 1) || !d_map1 || (!d_map2 && !(map_kind == 0 && interp == kNearest)))
        return hipErrorInvalidValue;
    return launch(stream, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, nframes, map_kind == 0 ? kSrcFixed : kSrcFloat,
                  d_map1, d_map2, nullptr, interp, border_mode, border_value);
}

hipError_t launch_warp_perspective(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w,
                                   int src_h, int dst_w, int dst_h, int nframes, const double inv[9], int interp,
                                   int border_mode, uint32_t border_value)
{
    return launch(stream, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, nframes, kSrcPerspective, nullptr, nullptr, inv,
                  interp, border_mode, border_value);
}

}  // namespace mi355
