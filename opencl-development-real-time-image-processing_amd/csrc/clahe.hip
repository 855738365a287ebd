// clahe.hip — contrast-limited adaptive histogram equalization of single-channel frames (cv::createCLAHE(clip,
// Size(tiles_x, tiles_y))->apply(), 8-bit).  Semantics: include/mi355_imgfilter.h, "local contrast".
//
// The frame is extended on the right and bottom to ew x eh = tiles_x tw x tiles_y th by one reflection
// (BORDER_REFLECT_101); the extended frame never exists in memory.  The three launches, the block histogram frame, the
// byte-range walk and the table scan are hist_common.hpp's (DESIGN.md sections 6d and 6d.1):
//   clahe_hist_kernel   a block owns a band of rows of one (frame, tile).  A tile row is tw bytes of the source at
//                       whatever alignment it has: a thread takes one aligned chunk of one row (mask_common.hpp), as a
//                       vector if the row covers all of it and byte by byte otherwise, or the row's reflected columns (at
//                       most tiles_x: a run of the same source row, read backwards).  Reflected rows are source rows;
//   clahe_table_kernel  one wave per (frame, tile): the clip, the closed-form redistribution, the table scan;
//   clahe_apply_kernel  the rows of a frame fall into tiles_y + 1 groups that share one pair (r1, r2) of tile rows.  A
//                       block owns up to kApplyBlockBytes of consecutive rows of one group as one byte range aligned on
//                       the output, stages the two tile rows' tables in LDS with the four bytes a pixel blends side by
//                       side ((tiles_x + 1) x 256 dwords, one per pair of neighbouring tile columns and source byte: one
//                       ds_read_b32 per pixel instead of four ds_read_u8), and blends them in fp32.
//                       The group boundaries are found on the host with the function the kernel uses for its weights
//                       (clahe_cell: one IEEE multiply, one subtract, one floor), so both agree on every row.
#include "common.hpp"
#include "hist_common.hpp"
#include "kernels.hpp"
#include "tile_common.hpp"

#include <cmath>

namespace mi355 {

namespace {

constexpr int kGroups = kClaheMaxTiles + 1;

// The apply stage's cell of position p along one axis: tf = (float)p * inv - 0.5f, t1 = floor(tf), *a = tf - t1.
__host__ __device__ __forceinline__ int clahe_cell(int p, float inv, float* a)
{
    const float tf = (float)p * inv - 0.5f;
    const float t1 = floorf(tf);
    *a = tf - t1;
    return (int)t1;
}

// row groups of the apply stage: group g (rows with floor(tyf) == g - 1) is rows y0[g] .. y0[g + 1] - 1 and blocks
// blk0[g] .. blk0[g + 1] - 1 of a frame; entries past tiles_y + 1 repeat the last one
struct ClaheRows {
    int y0[kGroups + 1];
    uint32_t blk0[kGroups + 1];
};

__global__ __launch_bounds__(kHistThreads) void clahe_hist_kernel(const uint8_t* __restrict__ in,
                                                                  uint32_t* __restrict__ hist, ClaheGeom g,
                                                                  uint32_t band_rows, uint32_t nbands)
{
    __shared__ uint32_t sh[kHistWaves * 256];
    const int tid = threadIdx.x;
    uint32_t* hw = block_hists_begin(sh);
    const uint32_t w = (uint32_t)g.w, h = (uint32_t)g.h, tw = (uint32_t)g.tw, th = (uint32_t)g.th;
    const uint32_t ntiles = (uint32_t)(g.tiles_x * g.tiles_y);
    const uint32_t ft = blockIdx.x / nbands, band = blockIdx.x - ft * nbands;  // ft = frame * ntiles + tile
    const uint32_t f = ft / ntiles, tile = ft - f * ntiles;
    const uint32_t tj = tile / (uint32_t)g.tiles_x, ti = tile - tj * (uint32_t)g.tiles_x;
    const uint8_t* p = in + (size_t)f * w * h;
    const uint32_t x0 = ti * tw;
    const uint32_t n = x0 < w ? (tw < w - x0 ? tw : w - x0) : 0;  // columns x0 .. x0 + n - 1 are source columns
    const uint32_t m = tw - n;                                    // the rest are reflected: source column 2w - 2 - x
    const uint32_t refl0 = m ? 2 * w - 1 - x0 - tw : 0;           // the lowest of them
    // per row: the aligned chunks of its n <= tw source bytes, and one slot for the reflected columns
    const uint32_t slots = aligned_chunks_of(tw) + 1;
    const uint32_t r0 = band * band_rows;
    const uint32_t r1 = r0 + band_rows < th ? r0 + band_rows : th;
    const uint32_t items = (r1 - r0) * slots;
    for (uint32_t k0 = 0; k0 < items; k0 += kHistThreads) {
        const uint32_t k = k0 + tid;
        bool full = false;
        u32x4 v = {0, 0, 0, 0};
        const uint8_t* row = p;
        uint32_t lo = 0, hi = 0;  // source columns of `row` this thread counts byte by byte
        if (k < items) {
            const uint32_t r = k / slots, s = k - r * slots;
            const uint32_t ye = tj * th + r0 + r;
            const uint32_t sy = ye < h ? ye : 2 * h - 2 - ye;
            row = p + (size_t)sy * w;
            if (s + 1 == slots) {
                lo = refl0;
                hi = refl0 + m;
            } else {
                const int mis = (int)(reinterpret_cast<uintptr_t>(row + x0) & 15u);
                const AlignedChunk<int> c = aligned_chunk<int>(mis, (int)s, (int)n);  // of the row's n source bytes
                if (c.whole()) {
                    full = true;
                    v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row + x0 + c.first));
                } else if (c.b1 > c.b0) {
                    lo = x0 + (uint32_t)(c.first + c.b0);
                    hi = x0 + (uint32_t)(c.first + c.b1);
                }
            }
        }
        count_vec(hw, v, full);
        for (uint32_t x = lo; x < hi; x++)
            lds_add(hw, row[x], 1);
    }
    block_hists_flush(sh, hist + (size_t)ft * 256);
}

// one wave per (frame, tile): lane l holds bins 4 l .. 4 l + 3
__global__ __launch_bounds__(kWave) void clahe_table_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ lut,
                                                            uint32_t cl, float lut_scale)
{
    const size_t t = blockIdx.x;
    const int lane = threadIdx.x;
    u32x4 hv = reinterpret_cast<const u32x4*>(hist + t * 256)[lane];
    if (cl > 0) {
        uint32_t clipped = 0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (hv[j] > cl) {
                clipped += hv[j] - cl;
                hv[j] = cl;
            }
#pragma unroll
        for (int d = kWave / 2; d >= 1; d /= 2)
            clipped += __shfl_xor(clipped, d);
        const uint32_t batch = clipped >> 8, residual = clipped & 255u;
        const uint32_t step = residual ? 256u / residual : 1u;  // residual < 256: at least 1
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t b = 4 * (uint32_t)lane + j, q = b / step;
            hv[j] += batch + (residual && q * step == b && q < residual ? 1u : 0u);
        }
    }
    uint32_t c = bins_below(hv, lane), out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        c += hv[j];
        out |= table_byte(c, lut_scale) << (8 * j);
    }
    reinterpret_cast<uint32_t*>(lut + t * 256)[lane] = out;
}

// One pixel: source byte v in column x of a row with the weights wy1 / wy on the two table rows.  sq[pc * 256 + v] holds
// the four table bytes of the column pair pc = floor(txf) + 1: L[r1][c1][v], L[r1][c2][v], L[r2][c1][v], L[r2][c2][v]
// from the low byte up.  Returns the rounded result as a float in 0 .. 255.
__device__ __forceinline__ float clahe_px(const uint32_t* sq, uint32_t v, uint32_t x, float inv_tw, float wy, float wy1)
{
    float xa;
    const int tx1 = clahe_cell((int)x, inv_tw, &xa);
    const float xa1 = 1.0f - xa;
    const uint32_t e = sq[(uint32_t)(tx1 + 1) * 256u + v];
    const float t = (float)(e & 0xFFu) * xa1 + (float)((e >> 8) & 0xFFu) * xa;
    const float b = (float)((e >> 16) & 0xFFu) * xa1 + (float)(e >> 24) * xa;
    return __builtin_rintf(t * wy1 + b * wy);
}

// 16 consecutive pixels from column x of row y; kWrap: the run may cross into the next rows
template <bool kWrap>
__device__ __forceinline__ u32x4 clahe_vec(const uint32_t* sq, const u32x4& v, uint32_t x, int y, uint32_t w,
                                           float inv_tw, float inv_th)
{
    float wy;
    (void)clahe_cell(y, inv_th, &wy);
    float wy1 = 1.0f - wy;
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        uint32_t ow = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // the value is a whole number in 0 .. 255: the conversion is exact, the pack saturates
            ow = __builtin_amdgcn_cvt_pk_u8_f32(clahe_px(sq, chunk_byte(v, 4 * d + e), x, inv_tw, wy, wy1), e, ow);
            x++;
            if (kWrap && x == w) {
                x = 0;
                (void)clahe_cell(++y, inv_th, &wy);
                wy1 = 1.0f - wy;
            }
        }
        o[d] = ow;
    }
    return o;
}

__global__ __launch_bounds__(kHistThreads) void clahe_apply_kernel(const uint8_t* __restrict__ in,
                                                                   uint8_t* __restrict__ out,
                                                                   const uint8_t* __restrict__ lut, ClaheGeom g,
                                                                   ClaheRows rows, uint32_t chunk_rows)
{
    __shared__ u32x4 sq4[(kClaheMaxTiles + 1) * 64];
    const int tid = threadIdx.x;
    const uint32_t bpf = rows.blk0[kGroups];  // blocks per frame
    const uint32_t f = blockIdx.x / bpf, b = blockIdx.x - f * bpf;
    // the last group that starts at or before block b (an empty group starts where the next one does)
    int grp = 0, y_lo = rows.y0[0], y_hi = rows.y0[1];
    uint32_t bbase = 0;
#pragma unroll
    for (int i = 1; i < kGroups; i++)
        if (i <= g.tiles_y && b >= rows.blk0[i]) {
            grp = i;
            y_lo = rows.y0[i];
            y_hi = rows.y0[i + 1];
            bbase = rows.blk0[i];
        }
    y_lo += (int)((b - bbase) * chunk_rows);
    if ((uint32_t)(y_hi - y_lo) > chunk_rows)
        y_hi = y_lo + (int)chunk_rows;
    // rows of group grp have floor(tyf) == grp - 1
    const int r1 = grp > 1 ? grp - 1 : 0, r2 = grp < g.tiles_y - 1 ? grp : g.tiles_y - 1;
    const uint32_t row_dwords = (uint32_t)g.tiles_x * 64u;
    const size_t frame_lut = (size_t)f * (size_t)(g.tiles_x * g.tiles_y) * 256;
    const uint32_t* top_g = reinterpret_cast<const uint32_t*>(lut + frame_lut + (size_t)r1 * row_dwords * 4);
    const uint32_t* bot_g = reinterpret_cast<const uint32_t*>(lut + frame_lut + (size_t)r2 * row_dwords * 4);
    // stage the two tile rows' tables, the four bytes of a column pair and a source byte side by side: one LDS read per
    // pixel.  Pair pc = floor(txf) + 1 in 0 .. tiles_x is the columns c1 = max(pc - 1, 0), c2 = min(pc, tiles_x - 1).
    for (uint32_t i = tid; i < ((uint32_t)g.tiles_x + 1u) * 64u; i += kHistThreads) {
        const uint32_t pc = i / 64u, v4 = i - pc * 64u;  // source bytes 4 v4 .. 4 v4 + 3
        const uint32_t c1 = pc > 0 ? pc - 1 : 0, c2 = pc < (uint32_t)g.tiles_x - 1 ? pc : (uint32_t)g.tiles_x - 1;
        const uint32_t ta = top_g[c1 * 64 + v4], tb = top_g[c2 * 64 + v4];
        const uint32_t ba = bot_g[c1 * 64 + v4], bb = bot_g[c2 * 64 + v4];
        u32x4 e;
#pragma unroll
        for (int j = 0; j < 4; j++)
            e[j] = ((ta >> (8 * j)) & 0xFFu) | (((tb >> (8 * j)) & 0xFFu) << 8) | (((ba >> (8 * j)) & 0xFFu) << 16) |
                   (((bb >> (8 * j)) & 0xFFu) << 24);
        sq4[i] = e;
    }
    __syncthreads();
    const uint32_t* sq = reinterpret_cast<const uint32_t*>(sq4);
    const uint32_t w = (uint32_t)g.w;
    const size_t at = (size_t)f * w * (uint32_t)g.h + (size_t)y_lo * w;
    const uint8_t* p = in + at;
    uint8_t* q = out + at;
    const uint32_t nb = (uint32_t)(y_hi - y_lo) * w;  // this block's bytes: rows y_lo .. y_hi - 1 as one flat range
    const ByteRange r = byte_range(q, nb);
    for (uint32_t j = tid; j < r.nvec; j += kHistThreads) {
        const uint32_t i0 = r.head + 16 * j;
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a1*>(p + i0));
        const uint32_t yr = i0 / w, x = i0 - yr * w;
        const u32x4 o = x + 16 <= w ? clahe_vec<false>(sq, v, x, y_lo + (int)yr, w, g.inv_tw, g.inv_th)
                                    : clahe_vec<true>(sq, v, x, y_lo + (int)yr, w, g.inv_tw, g.inv_th);
        __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(q + i0));
    }
    for_edge_byte(r, nb, tid, [&](uint32_t i) {
        const uint32_t yr = i / w, x = i - yr * w;
        float wy;
        (void)clahe_cell(y_lo + (int)yr, g.inv_th, &wy);
        q[i] = (uint8_t)(uint32_t)clahe_px(sq, p[i], x, g.inv_tw, wy, 1.0f - wy);
    });
}

bool clahe_sizes_ok(const ClaheGeom& g, int nframes)
{
    return hist_frames_ok(g.w, g.h, nframes) && g.tiles_x >= 1 && g.tiles_x <= kClaheMaxTiles &&
           g.tiles_y >= 1 && g.tiles_y <= kClaheMaxTiles && g.tw >= 1 && g.th >= 1 &&
           (uint64_t)g.tw * g.tiles_x * (uint64_t)g.th * g.tiles_y < (1ull << 31) &&
           g.tw * g.tiles_x - g.w <= g.w - 1 && g.th * g.tiles_y - g.h <= g.h - 1;
}

// the first row of 0 .. h whose floor(tyf) is at least t (tyf does not decrease with the row)
int clahe_first_row(int h, float inv_th, int t)
{
    int lo = 0, hi = h;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        float a;
        if (clahe_cell(mid, inv_th, &a) >= t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

}  // namespace

hipError_t launch_clahe_hist(hipStream_t stream, const uint8_t* d_in, uint32_t* d_hist, const ClaheGeom& g, int nframes)
{
    if (!clahe_sizes_ok(g, nframes))
        return hipErrorInvalidValue;
    uint32_t band_rows = kHistBlockBytes / (uint32_t)g.tw;
    band_rows = band_rows < 1 ? 1 : (band_rows > (uint32_t)g.th ? (uint32_t)g.th : band_rows);
    const uint32_t nbands = ((uint32_t)g.th + band_rows - 1) / band_rows;
    band_rows = ((uint32_t)g.th + nbands - 1) / nbands;  // bands of equal size
    const FrameGrid fg = frame_grid((uint64_t)(g.tiles_x * g.tiles_y) * nbands, 1, nframes);
    if (!fg.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(clahe_hist_kernel, dim3(fg.blocks), dim3(kHistThreads), 0, stream, d_in, d_hist, g,
                       band_rows, nbands);
    return hipGetLastError();
}

hipError_t launch_clahe_table(hipStream_t stream, const uint32_t* d_hist, uint8_t* d_luts, const ClaheGeom& g,
                              int nframes)
{
    if (!clahe_sizes_ok(g, nframes) || g.cl < 0)
        return hipErrorInvalidValue;
    const FrameGrid fg = frame_grid(g.tiles_x * g.tiles_y, 1, nframes);
    if (!fg.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(clahe_table_kernel, dim3(fg.blocks), dim3(kWave), 0, stream, d_hist, d_luts,
                       (uint32_t)g.cl, g.lut_scale);
    return hipGetLastError();
}

hipError_t launch_clahe_apply(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, const uint8_t* d_luts,
                              const ClaheGeom& g, int nframes)
{
    if (!clahe_sizes_ok(g, nframes))
        return hipErrorInvalidValue;
    uint32_t chunk_rows = kApplyBlockBytes / (uint32_t)g.w;
    chunk_rows = chunk_rows < 1 ? 1 : chunk_rows;
    ClaheRows rows;
    uint64_t blk = 0;
    for (int i = 0; i <= kGroups; i++) {
        rows.y0[i] = i <= g.tiles_y ? clahe_first_row(g.h, g.inv_th, i - 1) : g.h;
        if (i > 0)
            blk += ((uint64_t)(rows.y0[i] - rows.y0[i - 1]) + chunk_rows - 1) / chunk_rows;
        rows.blk0[i] = (uint32_t)blk;
    }
    const uint64_t blocks = blk * (uint64_t)nframes;
    if (blk == 0 || !grid_fits(blocks))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(clahe_apply_kernel, dim3((uint32_t)blocks), dim3(kHistThreads), 0, stream, d_in, d_out, d_luts,
                       g, rows, chunk_rows);
    return hipGetLastError();
}

}  // namespace mi355
