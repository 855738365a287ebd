// warp.hip — cv::warpAffine of 8-bit frames (include/mi355_imgfilter.h, "Rotating, shifting and deskewing frames"):
// NEAREST and LINEAR (OpenCV's classic fixed-point path: 10 fractional bits per coordinate, a 1/32-pixel weight grid),
// BORDER_CONSTANT and BORDER_REPLICATE, RGBA (every channel on its own) and gray8.
//
// One kernel template over <bytes per pixel, interpolation, border mode>.  A work item is one wave owning a 2-D tile of
// output pixels: a lane owns kItemPx = 4 adjacent output columns (16 bytes per RGBA store, one dword per gray8 store where
// the address allows it, byte stores at ragged ends and odd alignments), 2^lx_log2 lanes sit side by side and the
// 64 >> lx_log2 lane rows walk the tile top to bottom, so the source lines of one pass are the lines the pass before
// touched.  The host picks one of two tile shapes per launch from the map's slant (launch_warp_affine).  Tiles are ordered
// row-major inside a frame and blocks go through xcd_remap, so the tiles of one XCD are
// neighbours and share source lines in its L2.  The inverse map (six doubles) and the sizes come by value; per lane:
//   adelta / bdelta  of its four columns once, in registers;
//   X0(y) / Y0(y)    once per row it walks;
// in the fp64 and int operations the header states.  Nothing is read from a table.
// Whether every tap of a tile lies inside the frame is decided once per tile from the tile's four corners: adelta and X0
// are each monotone (rint of a monotone function), so the extremes of X0(y) + adelta(x) over the tile are corner values
// and the test is exact.  Interior tiles run with no per-tap test (RGBA LINEAR: the two horizontally adjacent taps of a
// source row as one 8-byte load); all other tiles clamp every index into the frame and, under BORDER_CONSTANT, replace
// the taps that lay outside.  Lanes past the right end repeat the last column and store nothing.  No access leaves a
// frame.
#include <cmath>

#include "warp_common.hpp"

namespace mi355 {

namespace {

struct WarpArgs {
    const uint8_t* in;
    uint8_t* out;
    int sw, sh, dw, dh;
    int lx_log2;  // lanes side by side in a tile: tile width = kItemPx << lx_log2
    int tile_h;   // output rows per tile, a multiple of 64 >> lx_log2
    int tiles_x, tiles_y;
    uint32_t nwork;
    uint32_t border;  // RGBA: the border pixel; gray8: its byte
    double i0, i1, i2, i3, i4, i5;
};

// rint(v * 1024.0) as int: cvRound of a coordinate in 10-bit fixed point (|v| < 2^20, so it fits)
__device__ __forceinline__ int fix10(double v)
{
    return (int)__builtin_rint(v * 1024.0);
}

// one output pixel from its fixed-point source position (X, Y), rd already added
template <int BPP, int INTERP, int BORDER, bool INTERIOR>
__device__ __forceinline__ uint32_t sample(global_ptr<const uint8_t> src, const WarpArgs& a, int X, int Y)
{
    return sample_at<BPP, INTERP, BORDER, INTERIOR>(src, a, X >> 10, Y >> 10, (uint32_t)(X >> 5) & 31u,
                                                    (uint32_t)(Y >> 5) & 31u);
}

// the lane's rows of the tile, top to bottom
template <int BPP, int INTERP, int BORDER, bool INTERIOR>
__device__ __forceinline__ void walk_rows(const WarpArgs& a, global_ptr<const uint8_t> src, global_ptr<uint8_t> dst,
                                          int x0, int y_first, int y_end, int y_step, const int (&adelta)[kItemPx],
                                          const int (&bdelta)[kItemPx])
{
    constexpr int rd = INTERP == kLinear ? 16 : 512;
    for (int y = y_first; y < y_end; y += y_step) {
        const int X0 = fix10(a.i1 * (double)y + a.i2) + rd;
        const int Y0 = fix10(a.i4 * (double)y + a.i5) + rd;
        uint32_t px[kItemPx];
#pragma unroll
        for (int j = 0; j < kItemPx; j++)
            px[j] = sample<BPP, INTERP, BORDER, INTERIOR>(src, a, X0 + adelta[j], Y0 + bdelta[j]);
        warp_store<BPP>(dst + (uint32_t)y * (uint32_t)a.dw * (uint32_t)BPP, x0, a.dw, px);
    }
}

template <int BPP, int INTERP, int BORDER>
__global__ __launch_bounds__(kItemWaves* kWave) void warp_kernel(const WarpArgs a)
{
    WaveItem it;
    if (!wave_item(xcd_remap(blockIdx.x, gridDim.x), a.nwork, a.tiles_x, a.tiles_y, a.lx_log2, a.tile_h, a.dh, &it))
        return;
    const size_t frame = it.frame;
    const int x0 = it.x0, ty0 = it.y0, ty_end = it.y_end;
    const int tile_w = kItemPx << a.lx_log2;
    const int tx0 = it.tx * tile_w, tx1 = min(tx0 + tile_w, a.dw) - 1;  // first and last column of the tile
    const global_ptr<const uint8_t> src = uniform_ptr(a.in + frame * ((size_t)a.sw * a.sh * BPP));
    const global_ptr<uint8_t> dst = uniform_ptr(a.out + frame * ((size_t)a.dw * a.dh * BPP));

    int adelta[kItemPx], bdelta[kItemPx];
#pragma unroll
    for (int j = 0; j < kItemPx; j++) {
        const double x = (double)min(x0 + j, a.dw - 1);
        adelta[j] = fix10(a.i0 * x);
        bdelta[j] = fix10(a.i3 * x);
    }

    // every tap of the tile inside the frame?  The extremes of X0(y) + adelta(x) over the tile are corner values.
    constexpr int rd = INTERP == kLinear ? 16 : 512;
    constexpr int reach = INTERP == kLinear ? 1 : 0;
    const int ax0 = fix10(a.i0 * (double)tx0), ax1 = fix10(a.i0 * (double)tx1);
    const int bx0 = fix10(a.i3 * (double)tx0), bx1 = fix10(a.i3 * (double)tx1);
    const int Xa = fix10(a.i1 * (double)ty0 + a.i2) + rd, Xb = fix10(a.i1 * (double)(ty_end - 1) + a.i2) + rd;
    const int Ya = fix10(a.i4 * (double)ty0 + a.i5) + rd, Yb = fix10(a.i4 * (double)(ty_end - 1) + a.i5) + rd;
    const int sx_min = (min(Xa, Xb) + min(ax0, ax1)) >> 10, sx_max = ((max(Xa, Xb) + max(ax0, ax1)) >> 10) + reach;
    const int sy_min = (min(Ya, Yb) + min(bx0, bx1)) >> 10, sy_max = ((max(Ya, Yb) + max(bx0, bx1)) >> 10) + reach;
    const bool interior =
        __builtin_amdgcn_readfirstlane((int)(sx_min >= 0 && sx_max <= a.sw - 1 && sy_min >= 0 && sy_max <= a.sh - 1)) != 0;

    if (interior)
        walk_rows<BPP, INTERP, BORDER, true>(a, src, dst, x0, ty0 + it.ly, ty_end, it.y_step, adelta, bdelta);
    else
        walk_rows<BPP, INTERP, BORDER, false>(a, src, dst, x0, ty0 + it.ly, ty_end, it.y_step, adelta, bdelta);
}

// The tile of a launch (kernels.hpp; both shapes and the rule between them come from the A/B of tools/warp_rate.py): the
// wide tile while an output row stays within a few source rows, the square tile for every steeper map.  The tune build
// takes MI355_TUNE_WARP_TILE=<lanes across, log2>x<rows> for that A/B.
void tile_shape(const double inv[6], int* lx_log2, int* tile_h)
{
    const bool wide = warp_tile_is_wide(inv);
    *lx_log2 = wide ? kWarpWideLanesLog2 : kWarpSquareLanesLog2;
    *tile_h = wide ? kWarpWideH : kWarpSquareH;
    tune_tile("MI355_TUNE_WARP_TILE", lx_log2, tile_h);
}

}  // namespace

bool warp_tile_is_wide(const double inv[6])
{
    return std::fabs(inv[3]) * (double)(kItemPx << kWarpWideLanesLog2) <= kWarpWideMaxRows;
}

uint64_t warp_work_items(const double inv[6], int dst_w, int dst_h, int nframes)
{
    int lx_log2 = 0, tile_h = 0;
    tile_shape(inv, &lx_log2, &tile_h);
    return tile_items(dst_w, dst_h, lx_log2, tile_h, nframes);
}

hipError_t launch_warp_affine(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h,
                              int dst_w, int dst_h, int nframes, const double inv[6], int interp, int border_mode,
                              uint32_t border_value)
{
    WarpArgs a{};
    tile_shape(inv, &a.lx_log2, &a.tile_h);
    if (!tile_args(&a, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, warp_work_items(inv, dst_w, dst_h, nframes),
                   interp, border_mode, border_value))
        return hipErrorInvalidValue;
    a.i0 = inv[0];
    a.i1 = inv[1];
    a.i2 = inv[2];
    a.i3 = inv[3];
    a.i4 = inv[4];
    a.i5 = inv[5];
    return dispatch_geom(bpp, interp, border_mode, [&](auto BPP, auto INTERP, auto BORDER) {
        return launch_items(warp_kernel<BPP.value, INTERP.value, BORDER.value>, stream, a);
    });
}

}  // namespace mi355
