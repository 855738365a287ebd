// tile_common.hpp — the frame every LDS-tiled kernel shares (gauss_tile, sobel_tile, gray8, morph, median, image2d):
// a workgroup owns one TW x TH output tile of one frame; the grid is the 1-D list of all tiles of all frames.
//   host    TileGrid counts the tiles, launch_tiles refuses more than 2^31 - 1 of them, raises the dynamic-LDS limit
//           where the kernel's carve needs more than the default 64 KiB allows, launches, and returns the launch error
//           (dispatch_int, which turns a runtime k / op / layout into a template argument, is common.hpp's).
//   device  tile_decode: tile index -> (tx, ty, frame, x0, y0); the border rule of a filter is common.hpp's
//           border_index<B>; the reduced-alignment 16-byte row chunk types and store_chunk16 (one vector store inside
//           the row, pixel by pixel across its right edge); the packed-u16 words of the min / max kernels.
// Every device helper is __forceinline__: nothing here adds a call or a runtime switch to a kernel.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi355 {

// the 64 x 16 RGBA tile of 256 threads: gauss_tile.hip, sobel_tile.hip, image2d.hip
constexpr int kRgbaTW = 64;
constexpr int kRgbaTH = 16;
constexpr int kRgbaTileThreads = 256;

// ---- host -----------------------------------------------------------------------------------------------------------
struct TileGrid {
    int tiles_x, tiles_y;
    uint64_t ntiles;
    TileGrid(int w, int h, int nframes, int tw, int th)
        : tiles_x((w + tw - 1) / tw), tiles_y((h + th - 1) / th), ntiles((uint64_t)tiles_x * tiles_y * nframes)
    {
    }
    bool ok() const { return ntiles <= 0x7FFFFFFFull; }  // a grid dimension, and the kernels index tiles in 32 bits
    uint32_t n() const { return (uint32_t)ntiles; }
};

// kLdsRaise: the carve may pass 64 KiB (runtime k), so the function's dynamic-LDS limit is set to `lds` first
enum LdsLimit { kLdsDefault, kLdsRaise };

template <typename... KArgs, typename... Args>
hipError_t launch_tiles(void (*kernel)(KArgs...), const TileGrid& g, int threads, size_t lds, LdsLimit limit,
                        hipStream_t stream, Args... args)
{
    if (!g.ok())
        return hipErrorInvalidValue;
    if (limit == kLdsRaise) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kernel, dim3(g.n()), dim3(threads), lds, stream, static_cast<KArgs>(args)...);
    return hipGetLastError();
}

// ---- device ---------------------------------------------------------------------------------------------------------
struct TilePos {
    int tx, ty;
    size_t frame;
    int x0, y0;  // image position of the tile's first output pixel
};

// `tile` is xcd_remap(blockIdx.x, ntiles) (neighbouring tiles, which share halo rows and columns, on one XCD) or plain
// blockIdx.x: the caller's choice, measured per kernel
__device__ __forceinline__ TilePos tile_decode(uint32_t tile, int tiles_x, int tiles_y, int tw, int th)
{
    TilePos t;
    t.tx = (int)(tile % (uint32_t)tiles_x);
    t.ty = (int)((tile / (uint32_t)tiles_x) % (uint32_t)tiles_y);
    t.frame = tile / ((uint32_t)tiles_x * (uint32_t)tiles_y);
    t.x0 = t.tx * tw;
    t.y0 = t.ty * th;
    return t;
}

// 16 bytes of a frame row.  RGBA rows are dword-aligned, gray8 rows may start at any byte; gfx950 global accesses need
// no alignment, and the reduced-alignment type is what tells the compiler so.
typedef u32x4 __attribute__((aligned(1))) u32x4_a1;
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
typedef u32x2 __attribute__((aligned(1))) u32x2_a1;
template <int BPP>
using chunk16 = typename std::conditional<BPP == 1, u32x4_a1, u32x4_a4>::type;

// 16 bytes = 16 / BPP pixels of `row` (w pixels of BPP bytes) from column gx >= 0 on: one vector store inside the row,
// pixel (byte) stores across the ragged right edge.  (There is no load_chunk16: as a helper the load's two arms come
// back from the compiler's pre-inlining pass as selects, which measured 0.5 - 1.5 % on gray8 and morph
// (profiles/tile_frame_ab.txt); the three kernels that load chunks keep their own few lines, on these types.)
template <int BPP>
__device__ __forceinline__ void store_chunk16(uint8_t* row, int gx, int w, const u32x4& v)
{
    static_assert(BPP == 1 || BPP == 4, "gray8 or RGBA");
    if (gx + 16 / BPP <= w) {
        *reinterpret_cast<chunk16<BPP>*>(row + (size_t)gx * BPP) = v;
    } else if constexpr (BPP == 4) {
        for (int p = 0; gx + p < w; p++)
            reinterpret_cast<uint32_t*>(row)[gx + p] = v[p];
    } else {
        for (int p = 0; gx + p < w; p++)
            row[gx + p] = (uint8_t)(v[p >> 2] >> (8 * (p & 3)));
    }
}

// Two u16 lanes per word: one v_pk_min_u16 / v_pk_max_u16 compares two values.  An RGBA pixel p splits once into
// (R, B) = p & 0x00ff00ff and (G, A) = v_perm_b32(p, zero-fill) and repacks with one v_lshl_or_b32.
using u16x2 = __attribute__((ext_vector_type(2))) unsigned short;

__device__ __forceinline__ u16x2 pmin(u16x2 a, u16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ u16x2 pmax(u16x2 a, u16x2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ void split_rgba(uint32_t p, u16x2& rb, u16x2& ga)
{
    rb = as_u16x2(p & 0x00FF00FFu);
    ga = as_u16x2(__builtin_amdgcn_perm(0u, p, 0x0C030C01u));
}
__device__ __forceinline__ uint32_t join_rgba(u16x2 rb, u16x2 ga) { return as_u32(rb) | (as_u32(ga) << 8); }

}  // namespace mi355
