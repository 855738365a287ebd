// median.hip — the median filter (MI355_FILTER_MEDIAN, MI355_FILTER_MEDIAN_GRAY8): cv::medianBlur semantics, k in
// {3, 5, 7}, every channel on its own (alpha included), clamp-to-edge (BORDER_REPLICATE) windows, frames independent.
// The output byte is always one of the window's input bytes, so every kernel here is bit-identical to any other
// correct median: there is no arithmetic to round.
//
// Two implementations that share no selection code:
//
// 1. Compare networks on packed 16-bit lanes (k = 3 and 5, both layouts): median_net_kernel.
//    A thread walks a strip of kMedStrip output rows down one column group, keeping the last k input rows in registers
//    (a ring of k rows indexed by a compile-time phase, so it never moves a register).  Values live two per 32-bit word
//    as u16 lanes, and every compare-exchange is one v_pk_min_u16 + one v_pk_max_u16 on two lanes at once:
//      RGBA   a column group is 4 pixels (one 16-byte load); each pixel dword splits once into (R, B) and (G, A)
//             (split_rgba, tile_common.hpp), so alpha rides along with G, and repacks with one v_lshl_or_b32;
//      gray8  a column group is 8 pixels; word c of a row holds the pixels (x0 + c, x0 + c + 4), so the same 4-column
//             network yields pixels x0 .. x0 + 7 in its two lanes.
//    Halo columns (k / 2 on each side) are separate clamped loads that hit the cache lines the neighbouring thread
//    loads; rows are clamped before loading.  Column groups that cross the image's left or right edge load pixel by
//    pixel at clamped columns, so any width and (gray8) any byte alignment works.
//      k = 3: every column of the window is sorted once (3 compare-exchanges) and shared by the 3 horizontal
//             neighbours that read it; median9 = med3(max3(lows), med3(mids), min3(highs)) — exact (the classic
//             pruning argument: after the column sorts, the lows' maximum, mids' median and highs' minimum bound the
//             median and it lies among them).  Per output word: 6 columns x 3 / 4 outputs = 4.5 column
//             compare-exchanges (9 min/max) and 2 + 4 + 2 + 4 = 12 min/max for the selection, 1 of each pairwise
//             max / min shared by two neighbours: 20 v_pk_min/max_u16 per word (ISA: 480 per 12 RGBA pixels).
//      k = 5: forgetful selection over the 25 window values: keep 14, drop the minimum and maximum (neither can be the
//             13th smallest), add the next value, drop again, ..., med3 of the last three.  Dropping the extremes of s
//             values is 2s - 3 compare-exchanges: sum_{s=4..14}(2s - 3) = 165 compare-exchanges + med3, of whose
//             330 + 4 min/max the last min and max of every drop are dead: 312 v_pk_min/max_u16 per word (ISA: 12480
//             per 20 RGBA pixels), i.e. ~624 per RGBA pixel and ~156 per gray8 pixel.  Issue-bound, not memory-bound.
// 2. Counting selection in an LDS tile (any odd k <= 7, both layouts): median_tile_kernel, on the tile frame of
//    tile_common.hpp.  The tile and its clamped halo are staged as one dword per pixel; each channel's median is the
//    smallest t with #(window values <= t) >= (k*k + 1) / 2, found by an 8-step bisection on t.  AUTO runs it for
//    k = 7, MI355_IMPL_TILE for every k; it is the on-GPU cross-check of the networks.
#include "../../include/mi355_imgfilter.h"
#include "common.hpp"
#include "kernels.hpp"
#include "tile_common.hpp"

namespace mi355 {

namespace {

constexpr int kMedThreads = 256;
constexpr int kMedStrip = 64;  // output rows per thread of the network kernel

__device__ __forceinline__ void cex(u16x2& a, u16x2& b)
{
    const u16x2 lo = pmin(a, b);
    b = pmax(a, b);
    a = lo;
}
__device__ __forceinline__ u16x2 pmed3(u16x2 a, u16x2 b, u16x2 c) { return pmax(pmin(a, b), pmin(pmax(a, b), c)); }

// k = 3: out[p] = median of columns p .. p + 2 (rows a, b, c), p = 0 .. 3
__device__ __forceinline__ void median9_x4(const u16x2* a, const u16x2* b, const u16x2* c, u16x2* out)
{
    u16x2 lo[6], mid[6], hi[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        u16x2 x = a[i], y = b[i], z = c[i];
        cex(x, y);
        cex(y, z);
        cex(x, y);
        lo[i] = x;
        mid[i] = y;
        hi[i] = z;
    }
    // neighbours 0/1 and 2/3 share the max of lows / min of highs of their two common columns
#pragma unroll
    for (int p = 0; p < 4; p += 2) {
        const u16x2 lmax = pmax(lo[p + 1], lo[p + 2]), hmin = pmin(hi[p + 1], hi[p + 2]);
        out[p] = pmed3(pmax(lo[p], lmax), pmed3(mid[p], mid[p + 1], mid[p + 2]), pmin(hi[p], hmin));
        out[p + 1] = pmed3(pmax(lmax, lo[p + 3]), pmed3(mid[p + 1], mid[p + 2], mid[p + 3]), pmin(hmin, hi[p + 3]));
    }
}

// exact median of the N = 2m + 1 values v[0..N) (v is clobbered), forgetful selection
template <int N>
__device__ __forceinline__ u16x2 median_forgetful(u16x2* v)
{
    constexpr int m = N / 2;
    int s = m + 2;  // live values: v[base .. base + s)
    int base = 0;
#pragma unroll
    for (int next = m + 2; next <= N; next++) {
        if (s == 3 && next == N)
            break;
        // minimum to v[base], maximum to v[base + s - 1]; drop both
#pragma unroll
        for (int i = 1; i < s; i++)
            cex(v[base], v[base + i]);
#pragma unroll
        for (int i = 1; i < s - 1; i++)
            cex(v[base + i], v[base + s - 1]);
        // the value v[base + s - 1] is dropped: refill that slot with the next input, drop the minimum by moving base
        if (next < N)
            v[base + s - 1] = v[next];
        base += 1;
        s -= 1;
    }
    return pmed3(v[base], v[base + 1], v[base + 2]);
}

// one row of a column group as u16x2 words: NW words per column (RGBA 2: (R,B) and (G,A); gray8 1), NC columns
template <bool G8, int R>
__device__ __forceinline__ void load_row(const uint8_t* __restrict__ row, int x0, int w, u16x2 (&dst)[4 + 2 * R][G8 ? 1 : 2])
{
    constexpr int NC = 4 + 2 * R;
    if constexpr (!G8) {
        const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row);
        uint32_t px[NC];
        if (x0 + 4 <= w) {
            const u32x4 q = *reinterpret_cast<const u32x4_a4*>(r32 + x0);
            px[R] = q[0];
            px[R + 1] = q[1];
            px[R + 2] = q[2];
            px[R + 3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                px[R + j] = r32[min(x0 + j, w - 1)];
        }
#pragma unroll
        for (int j = 0; j < R; j++) {
            px[j] = r32[max(x0 - R + j, 0)];
            px[R + 4 + j] = r32[min(x0 + 4 + j, w - 1)];
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
            split_rgba(px[c], dst[c][0], dst[c][1]);
    } else {
        // bytes x0 - R .. x0 + 7 + R; word c = (x0 - R + c, x0 - R + c + 4)
        constexpr int NB = 8 + 2 * R;
        uint32_t b[NB];
        if (x0 >= 4 && x0 + 12 <= w) {
            const u32x4 q = *reinterpret_cast<const u32x4_a1*>(row + x0 - 4);  // bytes x0 - 4 .. x0 + 11
#pragma unroll
            for (int i = 0; i < NB; i++) {
                const int j = i - R + 4;
                b[i] = (q[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NB; i++)
                b[i] = row[clampi(x0 - R + i, 0, w - 1)];
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
            dst[c][0] = as_u16x2(b[c] | (b[c + 4] << 16));
    }
}

template <bool G8, int K>
__global__ __launch_bounds__(kMedThreads) void median_net_kernel(const uint8_t* __restrict__ in,
                                                                 uint8_t* __restrict__ out, int w, int h, int ncg,
                                                                 int nstrips, uint64_t nitems)
{
    constexpr int R = K / 2, NC = 4 + 2 * R, NW = G8 ? 1 : 2, BPP = G8 ? 1 : 4, PX = G8 ? 8 : 4;
    const uint64_t item = (uint64_t)blockIdx.x * kMedThreads + threadIdx.x;
    if (item >= nitems)
        return;
    const int cg = (int)(item % (uint64_t)ncg);
    const uint64_t rest = item / (uint64_t)ncg;
    const int strip = (int)(rest % (uint64_t)nstrips);
    const uint64_t frame = rest / (uint64_t)nstrips;
    const size_t stride = (size_t)w * BPP;
    const uint8_t* fin = in + frame * stride * (size_t)h;
    uint8_t* fout = out + frame * stride * (size_t)h;
    const int x0 = cg * PX;
    const int ys = strip * kMedStrip, ye = min(ys + kMedStrip, h);

    u16x2 ring[K][NC][NW];
#pragma unroll
    for (int j = 0; j < K - 1; j++)
        load_row<G8, R>(fin + (size_t)clampi(ys - R + j, 0, h - 1) * stride, x0, w, ring[j]);

    for (int yb = ys; yb < ye; yb += K) {
#pragma unroll
        for (int ph = 0; ph < K; ph++) {
            const int y = yb + ph;
            if (y >= ye)
                break;
            // rows y - R .. y + R sit in slots (ph + j) % K; row y + R goes to slot (ph + K - 1) % K
            load_row<G8, R>(fin + (size_t)min(y + R, h - 1) * stride, x0, w, ring[(ph + K - 1) % K]);
            u16x2 med[4][NW];
#pragma unroll
            for (int q = 0; q < NW; q++) {
                if constexpr (K == 3) {
                    u16x2 a[NC], b[NC], c[NC], o[4];
#pragma unroll
                    for (int i = 0; i < NC; i++) {
                        a[i] = ring[ph % K][i][q];
                        b[i] = ring[(ph + 1) % K][i][q];
                        c[i] = ring[(ph + 2) % K][i][q];
                    }
                    median9_x4(a, b, c, o);
#pragma unroll
                    for (int p = 0; p < 4; p++)
                        med[p][q] = o[p];
                } else {
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        u16x2 v[K * K];
#pragma unroll
                        for (int j = 0; j < K; j++)
#pragma unroll
                            for (int i = 0; i < K; i++)
                                v[j * K + i] = ring[(ph + j) % K][p + i][q];
                        med[p][q] = median_forgetful<K * K>(v);
                    }
                }
            }
            uint8_t* orow = fout + (size_t)y * stride;
            if constexpr (!G8) {
                u32x4 px;
#pragma unroll
                for (int p = 0; p < 4; p++)
                    px[p] = join_rgba(med[p][0], med[p][1]);
                store_chunk16<4>(orow, x0, w, px);
            } else {
                uint32_t o[4];
#pragma unroll
                for (int p = 0; p < 4; p++)
                    o[p] = as_u32(med[p][0]);
                // pixel x0 + p is the low lane of word p, x0 + 4 + p its high lane
                const uint32_t d0 = __builtin_amdgcn_perm(o[1], o[0], 0x0C0C0400u) |
                                    (__builtin_amdgcn_perm(o[3], o[2], 0x0C0C0400u) << 16);
                const uint32_t d1 = __builtin_amdgcn_perm(o[1], o[0], 0x0C0C0602u) |
                                    (__builtin_amdgcn_perm(o[3], o[2], 0x0C0C0602u) << 16);
                uint8_t* dp = orow + x0;
                if (x0 + 8 <= w) {
                    *reinterpret_cast<u32x2_a1*>(dp) = u32x2{d0, d1};
                } else {
                    for (int j = 0; x0 + j < w; j++)
                        dp[j] = (uint8_t)((j < 4 ? d0 : d1) >> (8 * (j & 3)));
                }
            }
        }
    }
}

template <bool G8, int K>
hipError_t launch_net(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes)
{
    const int px = G8 ? 8 : 4;
    const int ncg = (w + px - 1) / px, nstrips = (h + kMedStrip - 1) / kMedStrip;
    const uint64_t nitems = (uint64_t)ncg * nstrips * nframes;
    const uint64_t nblocks = (nitems + kMedThreads - 1) / kMedThreads;
    if (nblocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((median_net_kernel<G8, K>), dim3((unsigned)nblocks), dim3(kMedThreads), 0, stream, d_in, d_out,
                       w, h, ncg, nstrips, nitems);
    return hipGetLastError();
}

// ---- counting selection in an LDS tile ------------------------------------------------------------------------------
constexpr int kTileW = 32, kTileH = 8;  // output tile; one thread per output pixel
constexpr int kTileHalo = MI355_MAX_MEDIAN_K / 2;
constexpr int kTileSW = kTileW + 2 * kTileHalo, kTileSH = kTileH + 2 * kTileHalo;

template <bool G8>
__global__ __launch_bounds__(kTileW* kTileH) void median_tile_kernel(const uint8_t* __restrict__ in,
                                                                     uint8_t* __restrict__ out, int w, int h, int k,
                                                                     int tiles_x, int tiles_y)
{
    __shared__ uint32_t s[kTileSH][kTileSW];  // one pixel per dword (gray8: the byte in bits 0-7)
    constexpr int BPP = G8 ? 1 : 4;
    const int R = k / 2;
    const TilePos tp = tile_decode(blockIdx.x, tiles_x, tiles_y, kTileW, kTileH);  // no XCD remap: not measured here
    const size_t fpx = (size_t)w * h;
    const uint8_t* fin = in + tp.frame * fpx * BPP;
    uint8_t* fout = out + tp.frame * fpx * BPP;
    const int x0 = tp.x0, y0 = tp.y0;
    const int tid = threadIdx.x;
    for (int i = tid; i < (kTileH + 2 * R) * (kTileW + 2 * R); i += kTileW * kTileH) {
        const int r = i / (kTileW + 2 * R), c = i - r * (kTileW + 2 * R);
        const int gy = clampi(y0 - R + r, 0, h - 1), gx = clampi(x0 - R + c, 0, w - 1);
        const size_t idx = (size_t)gy * w + gx;
        s[r][c] = G8 ? (uint32_t)fin[idx] : reinterpret_cast<const uint32_t*>(fin)[idx];
    }
    __syncthreads();
    const int c = tid % kTileW, r = tid / kTileW;
    const int gx = x0 + c, gy = y0 + r;
    if (gx >= w || gy >= h)
        return;
    const int need = (k * k + 1) / 2;
    uint32_t res = 0;
    for (int ch = 0; ch < BPP; ch++) {
        // smallest t in [0, 255] with #(values <= t) >= need
        int lo = 0, hi = 255;
        while (lo < hi) {
            const int t = (lo + hi) >> 1;
            int cnt = 0;
            for (int dy = 0; dy < k; dy++)
                for (int dx = 0; dx < k; dx++)
                    cnt += (int)((s[r + dy][c + dx] >> (8 * ch)) & 0xFFu) <= t;
            if (cnt >= need)
                hi = t;
            else
                lo = t + 1;
        }
        res |= (uint32_t)lo << (8 * ch);
    }
    const size_t idx = (size_t)gy * w + gx;
    if (G8)
        fout[idx] = (uint8_t)res;
    else
        reinterpret_cast<uint32_t*>(fout)[idx] = res;
}

template <bool G8>
hipError_t launch_tile(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k)
{
    const TileGrid g(w, h, nframes, kTileW, kTileH);
    return launch_tiles(median_tile_kernel<G8>, g, kTileW * kTileH, 0, kLdsDefault, stream, d_in, d_out, w, h, k,
                        g.tiles_x, g.tiles_y);
}

}  // namespace

hipError_t launch_median(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                         bool gray8, int impl)
{
    if (k < 3 || k > MI355_MAX_MEDIAN_K || (k & 1) == 0)
        return hipErrorInvalidValue;
    if (impl == 1 || k == 7)
        return gray8 ? launch_tile<true>(stream, d_in, d_out, w, h, nframes, k)
                     : launch_tile<false>(stream, d_in, d_out, w, h, nframes, k);
    return dispatch_int(k, std::integer_sequence<int, 3, 5>{}, [&](auto K) {
        constexpr int kc = decltype(K)::value;
        return gray8 ? launch_net<true, kc>(stream, d_in, d_out, w, h, nframes)
                     : launch_net<false, kc>(stream, d_in, d_out, w, h, nframes);
    });
}

}  // namespace mi355
