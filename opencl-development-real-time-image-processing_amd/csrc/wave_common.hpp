// wave_common.hpp — the frame of the kernels in which one wave owns one work item and walks it alone, with no LDS tile
// and no BandPlan (box, resize: strip x band x frame; warp, remap: tile x frame chunk).  Items are numbered x fastest,
// then y, then frame, and a block holds kItemWaves of them.
//   host    band_items / plan_bands: item count, band count and the 2^31 refusal of a strip x band x frame launch (the
//           halving of the band height stays with each kernel's constants); tile_items: the item
//           count of a tile launch; tune_tile: the MI355_TUNE_*_TILE override; tile_args: the argument refusal and the
//           geometry of a tile launch; dispatch_geom: <bytes per pixel, interpolation, border> as template arguments;
//           launch_items: the launch, its error returned.
//   device  wave_item: block and wave -> the item's place and the lane's place in it; warp_store: a lane's four output
//           pixels; load_px_at: one source pixel.
// Every launch takes fewer than 2^31 items (kItemsMax).  What stays per kernel is what it does on its rows.
#pragma once
#include <cstdio>

#include "kernels.hpp"
#include "slide_common.hpp"

namespace mi355 {

namespace {

constexpr int kItemWaves = 4;  // waves (work items) per block
constexpr int kItemPx = 4;     // output columns per lane of resize, warp and remap
constexpr uint64_t kItemsMax = 0x7FFFFFF0ull;

constexpr int kNearest = 0, kLinear = 1;      // MI355_INTERP_*
constexpr int kConstant = 0, kReplicate = 1;  // MI355_BORDER_*

// ---- host ----------------------------------------------------------------------------------------------------------
// The argument blocks stay per kernel, each in its own field order: one shared base for them changed the order in which
// hipcc fetches the fields at the start of a wave, and with it the speed of box (up to 0.9 % faster) and of three remap
// cases (0.1 - 0.2 % slower), where a refactor wants neither (profiles/wave_frame_ab.txt).  The helpers below fill
// them by field name.
//
// work items of a strip x band x frame launch with bands of `rows` rows
inline size_t band_items(int nstrips, int h, int rows, int nframes)
{
    return (size_t)nstrips * (size_t)((h + rows - 1) / rows) * (size_t)nframes;
}

// Args with int nstrips and band_rows (set by the caller), nbands and uint32_t nwork; false above kItemsMax items.  The
// caller halves band_rows first, with band_items, while its launch has too few waves: that loop stays in box.hip and
// resize.hip, each with its own floor, where tests/box_cases.py and tests/tiny_batch_cases.py read it.
template <typename Args>
bool plan_bands(Args* a, int h, int nframes)
{
    const size_t nwork = band_items(a->nstrips, h, a->band_rows, nframes);
    if (nwork > kItemsMax)
        return false;
    a->nbands = (h + a->band_rows - 1) / a->band_rows;
    a->nwork = (uint32_t)nwork;
    return true;
}

inline int tiles_across(int n, int tile)
{
    return (n + tile - 1) / tile;
}

// tiles of a w x h frame times nchunks, for any int arguments (the *_check entry points pass theirs unfiltered)
inline uint64_t tile_items(int w, int h, int lx_log2, int tile_h, int nchunks)
{
    return (uint64_t)tiles_across(w, kItemPx << lx_log2) * (uint64_t)tiles_across(h, tile_h) * (uint64_t)nchunks;
}

// <lanes across, log2>x<rows> in the tune build's variable `name` replaces the tile when it is one a wave can walk
inline void tune_tile(const char* name, int* lx_log2, int* tile_h)
{
    if (const char* e = tune_env(name)) {
        int l = 0, h = 0;
        if (sscanf(e, "%dx%d", &l, &h) == 2 && l >= 0 && l <= 6 && h >= (kWave >> l) && h <= 4096 &&
            h % (kWave >> l) == 0) {
            *lx_log2 = l;
            *tile_h = h;
        }
    }
}

// The refusal of the geometric calls and the geometry of their launch: pixel and map-entry indices inside a frame are
// 32-bit (times 4 bytes), so no size exceeds kWarpMaxSize.  Args with in, out, sw, sh, dw, dh, lx_log2 and tile_h (set
// by the caller), tiles_x, tiles_y, nwork and border; nwork is the caller's *_work_items.
template <typename Args>
bool tile_args(Args* a, const uint8_t* d_in, uint8_t* d_out, int bpp, int src_w, int src_h, int dst_w,
                      int dst_h, uint64_t nwork, int interp, int border_mode, uint32_t border_value)
{
    if ((bpp != 1 && bpp != 4) || (interp != kNearest && interp != kLinear) ||
        (border_mode != kConstant && border_mode != kReplicate))
        return false;
    if (src_w > kWarpMaxSize || src_h > kWarpMaxSize || dst_w > kWarpMaxSize || dst_h > kWarpMaxSize)
        return false;
    if (nwork == 0 || nwork > kItemsMax)
        return false;
    a->in = d_in;
    a->out = d_out;
    a->sw = src_w;
    a->sh = src_h;
    a->dw = dst_w;
    a->dh = dst_h;
    a->tiles_x = tiles_across(dst_w, kItemPx << a->lx_log2);
    a->tiles_y = tiles_across(dst_h, a->tile_h);
    a->nwork = (uint32_t)nwork;
    a->border = bpp == 4 ? border_value : (border_value & 0xFFu);
    return true;
}

// f(BPP, INTERP, BORDER) as integral constants, for arguments tile_args has let through
template <typename F>
hipError_t dispatch_geom(int bpp, int interp, int border_mode, F&& f)
{
    return dispatch_int(bpp, std::integer_sequence<int, 1, 4>{}, [&](auto BPP) {
        return dispatch_int(interp, std::integer_sequence<int, kNearest, kLinear>{}, [&](auto INTERP) {
            return dispatch_int(border_mode, std::integer_sequence<int, kConstant, kReplicate>{},
                                [&](auto BORDER) { return f(BPP, INTERP, BORDER); });
        });
    });
}

#ifdef __HIPCC__
// a.nwork items, kItemWaves to a block
template <typename Args>
hipError_t launch_items(void (*kernel)(Args), hipStream_t stream, const Args& a)
{
    hipLaunchKernelGGL(kernel, dim3((a.nwork + kItemWaves - 1) / kItemWaves), dim3(kItemWaves * kWave), 0, stream, a);
    return hipGetLastError();
}

// ---- device --------------------------------------------------------------------------------------------------------
// Which item this wave owns, wave-uniform, and where the lane sits in it.  The item is 2^lx_log2 lanes of kItemPx
// columns wide and item_h rows tall; its 64 >> lx_log2 lane rows take y_step rows per pass, the lane's own at ly.  A
// strip kernel is lx_log2 = 6: ly = 0 and y_step = 1 fold away (box; resize_kernel keeps its decode in place).
struct WaveItem {
    int tx, ty;      // strip or tile column; band or tile row
    uint32_t frame;  // frame, or chunk of frames
    int x0;          // the lane's first column
    int y0, y_end;   // the item's first row and one past its last
    int ly, y_step;
};

// `block` is blockIdx.x or a bijective remap of it.  False for the padding waves of the last block.  The decode is
// not put behind that test: returned through an early exit it moved remap_kernel<4, 1, 0, 2> from 112 VGPRs and 4 waves
// per SIMD to 95 and 5 (profiles/wave_frame_vgpr.txt).  It reads no memory; hipcc issues its first division ahead of
// the caller's exit, in the wait for the readfirstlane, so the up to three padding waves of a launch pay that much.
__device__ __forceinline__ bool wave_item(uint32_t block, uint32_t nwork, int nx, int ny, int lx_log2, int item_h,
                                          int h, WaveItem* it)
{
    const uint32_t work = __builtin_amdgcn_readfirstlane(block * kItemWaves + (uint32_t)(threadIdx.x >> 6));
    __builtin_assume(work < 0x80000000u);  // nwork <= kItemsMax: what an exit test ahead of the decode tells hipcc
    const int lane = threadIdx.x & 63;
    it->tx = (int)(work % (uint32_t)nx);
    const uint32_t t = work / (uint32_t)nx;
    it->ty = (int)(t % (uint32_t)ny);
    it->frame = t / (uint32_t)ny;
    it->x0 = it->tx * (kItemPx << lx_log2) + (lane & ((1 << lx_log2) - 1)) * kItemPx;
    it->y0 = it->ty * item_h;
    it->y_end = min(it->y0 + item_h, h);
    it->ly = lane >> lx_log2;
    it->y_step = kWave >> lx_log2;
    return work < nwork;
}

// four output pixels of a lane (RGBA: dwords; gray8: byte values) to columns x0 .. x0 + 3 of the row at `rowp`, whole
// where the address and the row's end allow it
template <int BPP>
__device__ __forceinline__ void warp_store(global_ptr<uint8_t> rowp, int x0, int dw, const uint32_t (&px)[kItemPx])
{
    if constexpr (BPP == 4) {
        if (x0 + kItemPx <= dw) {
            gstore_a4<u32x4>(rowp + (uint32_t)x0 * 4u, u32x4{px[0], px[1], px[2], px[3]});
        } else {
#pragma unroll
            for (int j = 0; j < kItemPx; j++)
                if (x0 + j < dw)
                    gstore_a4<uint32_t>(rowp + (uint32_t)(x0 + j) * 4u, px[j]);
        }
    } else {
        global_ptr<uint8_t> p = rowp + (uint32_t)x0;
        if (x0 + kItemPx <= dw && (reinterpret_cast<uint64_t>(p) & 3u) == 0) {
            gstore_a4<uint32_t>(p, px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24));
        } else {
#pragma unroll
            for (int j = 0; j < kItemPx; j++)
                if (x0 + j < dw)
                    p[j] = (uint8_t)px[j];
        }
    }
}

// the pixel at p: RGBA its dword, gray8 its byte
template <int BPP>
__device__ __forceinline__ uint32_t load_px_at(global_ptr<const uint8_t> p)
{
    if constexpr (BPP == 4)
        return gload<uint32_t>(p);
    else
        return gload<uint8_t>(p);
}
#endif

}  // namespace

}  // namespace mi355
