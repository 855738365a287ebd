// dist.hip — cv::distanceTransform(mask, DIST_L2, DIST_MASK_PRECISE, CV_32F) of single-channel masks: the exact squared
// Euclidean distance to the nearest zero pixel (a "site"), its square root and the nearest site's index.  Semantics:
// include/mi355_imgfilter.h, "how far from the background"; design, the bounds of every loop and the measurements:
// DESIGN.md section 6m.  Integer arithmetic up to the one int32 -> fp32 conversion and the one square root of the float
// output.  Two launches, no flag between workgroups, no retry.
//
//   dist_cols_kernel   per pixel the signed row offset dy = y' - y to the nearest site of its own column (a tie goes to
//                      the site above, kDistNoSite marks a column without a site), as int16 into the pooled scratch whose
//                      rows are padded to four entries.  A workgroup owns kDistColW = 64 adjacent columns of one frame
//                      over the whole height; 16 lanes of 4 columns stand side by side (a dword of input, 8 bytes of
//                      output per lane and row) and the workgroup's threads / 16 segments stand below each other, each a
//                      run of whole 32-row chunks.
//                        1. every lane reads its segment once, 32 rows in flight, and leaves one 32-bit site mask per
//                           column and chunk in LDS, and per column the segment's first and last site row;
//                        2. 128 threads (64 columns x up / down) turn those into "nearest site row above / below the
//                           segment" by one serial pass over the <= 64 segments;
//                        3. every lane answers its rows from the chunk's mask (count leading / trailing zeros of the bits
//                           above / below the row) and, where the mask has none, from the carried rows.
//                      Every loop is bounded by the geometry: nothing depends on the content.
//   dist_rows_kernel   one wave per row.  The row's dy lies in LDS (2 B per column) beside the leftmost minimiser
//                      opt[x] of (x - x')^2 + dy(x')^2 (2 B per column).  The minimisers are resolved by monotone divide
//                      and conquer in levels: level l solves the positions (2 k + 1) * 2^(L - 1 - l), each over the
//                      candidates between the minimisers of its two solved neighbours (the cost matrix is Monge, so
//                      opt is non-decreasing), cut to |x - x'| <= |dy(x)| (the column's own site is a candidate, so
//                      nothing farther can win or tie).  The ranges of a level sum to at most w plus its queries.  On
//                      the first six levels, which have fewer queries than lanes, g = 64 >> level lanes share a query,
//                      sweep its range side by side and reduce on (value, x'); from then on a lane takes one query
//                      (g = 1).  A range longer than kDistLaneRange * g is instead swept by all 64 lanes, so no lane
//                      holds its wave for more than kDistLaneRange candidates.  A sweep keeps kDistIlp LDS reads in flight.
//                      kDistNoSite squared (2^30 - 65535) is the finite value of a column without a site:
//                      above 2 * 16383^2, every real candidate beats it, and with 16383^2 added it stays inside an int32.
//                      The last sweep writes the three outputs, one dword per lane, 256 bytes per wave and store.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355 {

namespace {

constexpr int kDistColLanes = 16;                         // lanes side by side in the column launch ...
constexpr int kDistColPx = 4;                             // ... of four columns each
constexpr int kDistColW = kDistColLanes * kDistColPx;     // columns of a workgroup
constexpr int kDistChunk = 32;                            // rows of a site mask
constexpr int kDistMaxSegs = 64;                          // segments of a workgroup: 1024 threads
constexpr int kDistNoSite = 32767;                        // dy of a column without a site; also "no row" in the carries
constexpr int kDistLaneRange = 64;                        // candidates one lane sweeps alone in the row launch
constexpr int kDistGroupLevels = 6;                       // the levels with fewer queries than lanes: 64 >> level lanes per query
constexpr int kDistIlp = 4;                               // candidates a lane has in flight
static_assert((1 << kDistGroupLevels) == kWave && kDistLaneRange % kDistIlp == 0, "the row launch's wave geometry");
constexpr uint32_t kDistMaxBlocks = 1u << 24;             // both launches walk their work list with a grid stride
static_assert(kDistMaxDim <= 16384, "a row index and a minimiser fit an int16, 2 * (kDistMaxDim - 1)^2 stays below 32767^2");
static_assert((int64_t)kDistNoSite * kDistNoSite + (int64_t)(kDistMaxDim - 1) * (kDistMaxDim - 1) < (1ll << 31), "int32 cost");
static_assert(2ll * (kDistMaxDim - 1) * (kDistMaxDim - 1) < (int64_t)kDistNoSite * kDistNoSite, "a real candidate wins");

typedef uint32_t __attribute__((aligned(1))) u32_a1;
using i16x4 = __attribute__((ext_vector_type(4))) int16_t;

// How the column launch cuts a frame of h rows: whole chunks per segment, segments rounded up to whole waves
struct DistColPlan {
    int chunks, chunks_per_seg, segs, threads;
    size_t lds;
};

DistColPlan dist_col_plan(int h)
{
    DistColPlan p;
    p.chunks = (h + kDistChunk - 1) / kDistChunk;
    p.chunks_per_seg = (p.chunks + kDistMaxSegs - 1) / kDistMaxSegs;
    const int segs = (p.chunks + p.chunks_per_seg - 1) / p.chunks_per_seg;
    p.segs = (segs + 3) & ~3;  // 16 lanes each: whole waves
    p.threads = p.segs * kDistColLanes;
    p.lds = (size_t)p.chunks * kDistColW * sizeof(uint32_t) + 2 * (size_t)p.segs * kDistColW * sizeof(int16_t);
    return p;
}

__global__ __launch_bounds__(kDistMaxSegs* kDistColLanes) void dist_cols_kernel(const uint8_t* __restrict__ in,
                                                                                int16_t* __restrict__ dy, int w, int ws,
                                                                                int h, uint32_t groups_x, uint64_t items,
                                                                                int chunks, int cps, int segs)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* mask = reinterpret_cast<uint32_t*>(smem);                                          // [chunks][kDistColW]
    int16_t* up = reinterpret_cast<int16_t*>(smem + (size_t)chunks * kDistColW * sizeof(uint32_t));  // [segs][kDistColW]
    int16_t* dn = up + segs * kDistColW;                                                         // [segs][kDistColW]
    const int tid = threadIdx.x, seg = tid / kDistColLanes, cl = tid % kDistColLanes;
    const int c0 = min(seg * cps, chunks), c1 = min(c0 + cps, chunks);

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {  // bound: items / gridDim.x trips, rounded up
        const size_t frame = item / groups_x;
        const int x0 = (int)(item % groups_x) * kDistColW + kDistColPx * cl;
        const uint8_t* fin = in + frame * (size_t)w * h;
        const bool lane_in = x0 < w, whole = x0 + kDistColPx <= w;

        // 1. the segment's site masks, and its first and last site row per column
        int first[kDistColPx], last[kDistColPx];
#pragma unroll
        for (int j = 0; j < kDistColPx; j++) {
            first[j] = kDistNoSite;
            last[j] = -1;
        }
        for (int c = c0; c < c1; c++) {  // bound: cps <= 8
            uint32_t m[kDistColPx] = {0u, 0u, 0u, 0u};
            if (lane_in) {
                const int ybase = c * kDistChunk, rows = min(h - ybase, kDistChunk);
                uint32_t v[kDistChunk];
                if (whole) {
#pragma unroll
                    for (int r = 0; r < kDistChunk; r++)  // rows past the frame re-read its last row; their bits are dropped
                        v[r] = *reinterpret_cast<const u32_a1*>(fin + (size_t)min(ybase + r, h - 1) * w + x0);
                } else {
#pragma unroll
                    for (int r = 0; r < kDistChunk; r++) {
                        const uint8_t* p = fin + (size_t)min(ybase + r, h - 1) * w;
                        v[r] = 0u;
#pragma unroll
                        for (int j = 0; j < kDistColPx; j++)  // columns past the row re-read its last byte; nothing reads their dy
                            v[r] |= (uint32_t)p[min(x0 + j, w - 1)] << (8 * j);
                    }
                }
#pragma unroll
                for (int r = 0; r < kDistChunk; r++)
#pragma unroll
                    for (int j = 0; j < kDistColPx; j++)
                        m[j] |= (((v[r] >> (8 * j)) & 0xFFu) == 0u ? 1u : 0u) << r;
                const uint32_t keep = rows >= kDistChunk ? 0xFFFFFFFFu : (1u << rows) - 1u;
#pragma unroll
                for (int j = 0; j < kDistColPx; j++) {
                    m[j] &= keep;
                    if (m[j] != 0u) {
                        if (first[j] == kDistNoSite)
                            first[j] = ybase + __builtin_ctz(m[j]);
                        last[j] = ybase + 31 - __builtin_clz(m[j]);
                    }
                }
            }
            *reinterpret_cast<u32x4*>(mask + c * kDistColW + kDistColPx * cl) = u32x4{m[0], m[1], m[2], m[3]};
        }
        *reinterpret_cast<i16x4*>(up + seg * kDistColW + kDistColPx * cl) =
            i16x4{(int16_t)last[0], (int16_t)last[1], (int16_t)last[2], (int16_t)last[3]};
        *reinterpret_cast<i16x4*>(dn + seg * kDistColW + kDistColPx * cl) =
            i16x4{(int16_t)first[0], (int16_t)first[1], (int16_t)first[2], (int16_t)first[3]};
        __syncthreads();

        // 2. per column: up[s] becomes the nearest site row above segment s (-1: none), dn[s] the nearest below it
        for (int t = tid; t < 2 * kDistColW; t += blockDim.x) {  // bound: two trips of a one-wave workgroup
            const int col = t % kDistColW;
            if (t < kDistColW) {
                int run = -1;
                for (int s = 0; s < segs; s++) {  // bound: segs <= 64
                    const int own = up[s * kDistColW + col];
                    up[s * kDistColW + col] = (int16_t)run;
                    run = own >= 0 ? own : run;
                }
            } else {
                int run = kDistNoSite;
                for (int s = segs - 1; s >= 0; s--) {
                    const int own = dn[s * kDistColW + col];
                    dn[s * kDistColW + col] = (int16_t)run;
                    run = own != kDistNoSite ? own : run;
                }
            }
        }
        __syncthreads();

        // 3. the rows of the segment, chunk by chunk downwards
        if (lane_in) {
            const i16x4 up4 = *reinterpret_cast<const i16x4*>(up + seg * kDistColW + kDistColPx * cl);
            const i16x4 dn4 = *reinterpret_cast<const i16x4*>(dn + seg * kDistColW + kDistColPx * cl);
            int uprow[kDistColPx] = {up4[0], up4[1], up4[2], up4[3]};
            int16_t* fdy = dy + frame * (size_t)h * ws + x0;
            for (int c = c0; c < c1; c++) {  // bound: cps <= 8
                const u32x4 m = *reinterpret_cast<const u32x4*>(mask + c * kDistColW + kDistColPx * cl);
                int dnrow[kDistColPx] = {dn4[0], dn4[1], dn4[2], dn4[3]};
                for (int k = c1 - 1; k > c; k--) {  // bound: cps - 1; the nearest chunk below is written last
                    const u32x4 mk = *reinterpret_cast<const u32x4*>(mask + k * kDistColW + kDistColPx * cl);
#pragma unroll
                    for (int j = 0; j < kDistColPx; j++)
                        dnrow[j] = mk[j] != 0u ? k * kDistChunk + __builtin_ctz(mk[j]) : dnrow[j];
                }
                const int ybase = c * kDistChunk;
#pragma unroll
                for (int r = 0; r < kDistChunk; r++) {
                    const int y = ybase + r;
                    if (y < h) {
                        int d[kDistColPx];
#pragma unroll
                        for (int j = 0; j < kDistColPx; j++) {
                            const uint32_t upm = m[j] & (0xFFFFFFFFu >> (31 - r)), dnm = m[j] >> r;
                            const int du = upm != 0u ? r - 31 + __builtin_clz(upm) : (uprow[j] >= 0 ? y - uprow[j] : kDistNoSite);
                            const int dd = dnm != 0u ? __builtin_ctz(dnm) : (dnrow[j] != kDistNoSite ? dnrow[j] - y : kDistNoSite);
                            d[j] = (du <= dd && du != kDistNoSite) ? -du : dd;  // a tie goes to the site above
                        }
                        *reinterpret_cast<u32x2*>(fdy + (size_t)y * ws) =
                            u32x2{((uint32_t)d[0] & 0xFFFFu) | ((uint32_t)d[1] << 16), ((uint32_t)d[2] & 0xFFFFu) | ((uint32_t)d[3] << 16)};
                    }
                }
#pragma unroll
                for (int j = 0; j < kDistColPx; j++)
                    uprow[j] = m[j] != 0u ? ybase + 31 - __builtin_clz(m[j]) : uprow[j];
            }
        }
        __syncthreads();  // the next item's masks and carries go over these
    }
}

// (x - xp)^2 + dy(xp)^2; both factors are below 2^15: the 24-bit multiplier
__device__ __forceinline__ int dist_cost(const int16_t* dyl, int x, int xp)
{
    const int d = dyl[xp], dx = x - xp;
    return __mul24(dx, dx) + __mul24(d, d);
}

// The candidates of query k of a level (position p = (2 k + 1) s, counted from 1): between the minimisers of the two
// solved neighbours, and no farther from x than the site of x's own column.  An idle lane (k >= nq) gets the empty range.
__device__ __forceinline__ void dist_range(const int16_t* dyl, const uint16_t* opt, int k, int nq, int s, int w, int& x,
                                           int& lo, int& hi)
{
    if (k < nq) {
        const int p = (2 * k + 1) * s;
        x = p - 1;
        lo = p == s ? 0 : (int)opt[p - s - 1];
        hi = p + s > w ? w - 1 : (int)opt[p + s - 1];
        const int r = abs((int)dyl[x]);
        lo = max(lo, x - r);
        hi = min(hi, x + r);
    }
}

// kDistIlp candidates xp, xp + step, ... of query x, their LDS reads in flight together.  A candidate past hi is hi once
// more: it cannot beat what hi left behind, since only a smaller value or the same value at a smaller x' takes over.
__device__ __forceinline__ void dist_sweep(const int16_t* dyl, int x, int xp, int step, int hi, int& best, int& bx)
{
    int c[kDistIlp], at[kDistIlp];
#pragma unroll
    for (int u = 0; u < kDistIlp; u++) {
        at[u] = min(xp + u * step, hi);
        c[u] = dist_cost(dyl, x, at[u]);
    }
#pragma unroll
    for (int u = 0; u < kDistIlp; u++)
        if (c[u] < best) {  // a lane's candidates ascend: the leftmost minimum stays
            best = c[u];
            bx = at[u];
        }
}

// (best, bx) = the smaller of it and lane ^ off's, by value, then by x'
__device__ __forceinline__ void dist_min_xor(int& best, int& bx, int off)
{
    const int ob = __shfl_xor(best, off), ox = __shfl_xor(bx, off);
    const bool take = ob < best || (ob == best && ox < bx);
    best = take ? ob : best;
    bx = take ? ox : bx;
}

__global__ __launch_bounds__(kWave) void dist_rows_kernel(const int16_t* __restrict__ dy, int32_t* __restrict__ sq,
                                                          float* __restrict__ dist, int32_t* __restrict__ nearest, int w,
                                                          int ws, int h, uint64_t rows, int levels)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int16_t* dyl = reinterpret_cast<int16_t*>(smem);              // [ws]
    uint16_t* opt = reinterpret_cast<uint16_t*>(smem) + ws;       // [ws]
    const int lane = threadIdx.x;

    for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {  // bound: rows / gridDim.x trips, rounded up
        const uint32_t* src = reinterpret_cast<const uint32_t*>(dy + row * (size_t)ws);
        for (int i = lane; i < ws / 2; i += kWave)  // bound: ws / 128 trips, rounded up
            reinterpret_cast<uint32_t*>(dyl)[i] = src[i];
        __syncthreads();

        for (int lev = 0; lev < levels; lev++) {  // bound: levels <= 15
            const int s = 1 << (levels - 1 - lev);
            const int nq = (w / s + 1) >> 1;  // the positions p = (2 k + 1) s <= w, counted from 1; nq <= 2^lev
            // g lanes share a query: 64 >> lev on the levels with fewer queries than lanes, one from then on
            const int gshift = lev < kDistGroupLevels ? kDistGroupLevels - lev : 0, g = 1 << gshift;
            const int sub = lane & (g - 1), mine = kDistLaneRange * g;  // what a group sweeps itself
            for (int k0 = 0; k0 < nq; k0 += kWave >> gshift) {  // bound: one trip while g > 1, then nq / 64 trips, rounded up
                int x = 0, lo = 0, hi = -1;
                dist_range(dyl, opt, k0 + (lane >> gshift), nq, s, w, x, lo, hi);
                const int len = hi - lo + 1;  // 0 in an idle lane
                int cb = 0x7FFFFFFF, cx = 0x7FFFFFFF;
                if (len <= mine && sub < len) {  // the first candidate alone: most ranges of the late levels end here
                    cb = dist_cost(dyl, x, lo + sub);
                    cx = lo + sub;
                }
                for (int j = sub + g;; j += kDistIlp * g) {  // bound: kDistLaneRange / 4 trips
                    const bool go = len <= mine && j < len;
                    if (__builtin_amdgcn_ballot_w64(go) == 0)
                        break;
                    if (go)
                        dist_sweep(dyl, x, lo + j, g, hi, cb, cx);
                }
                if (g > 1) {
#pragma unroll
                    for (int off = kWave / 2; off > 0; off >>= 1)  // minimum of (value, x') over the group
                        if (off < g)
                            dist_min_xor(cb, cx, off);
                }
                // the longer ranges, one after the other by the whole wave; a level's ranges sum to at most w + nq, so at
                // most (w + nq) / (kDistLaneRange g) of them exist per level, and their sweeps take (w + nq) / 256 + that
                // many trips at the most
                uint64_t pending = __builtin_amdgcn_ballot_w64(sub == 0 && len > mine);
                while (pending != 0) {  // bound: 64
                    const int owner = __builtin_ctzll(pending);
                    pending &= pending - 1;
                    const int qlo = __builtin_amdgcn_readlane(lo, owner), qhi = __builtin_amdgcn_readlane(hi, owner);
                    const int qx = __builtin_amdgcn_readlane(x, owner);
                    int wb = 0x7FFFFFFF, wx = 0x7FFFFFFF;
                    for (int j = 0; qlo + j <= qhi; j += kDistIlp * kWave)  // bound: (qhi - qlo) / 256 + 1
                        if (qlo + j + lane <= qhi)
                            dist_sweep(dyl, qx, qlo + j + lane, kWave, qhi, wb, wx);
#pragma unroll
                    for (int off = kWave / 2; off > 0; off >>= 1)  // minimum of (value, x') over the wave
                        dist_min_xor(wb, wx, off);
                    if (lane == owner)
                        cx = wx;
                }
                if (sub == 0 && len > 0)
                    opt[x] = (uint16_t)cx;
            }
            __syncthreads();
        }

        const int y = (int)(row % (uint64_t)h);
        const size_t at = row * (size_t)w;
        for (int x = lane; x < w; x += kWave) {  // bound: w / 64 trips, rounded up
            const int o = opt[x], d = dyl[o], dx = x - o;
            const int v = __mul24(dx, dx) + __mul24(d, d);
            const bool none = d == kDistNoSite;  // the row's best column has no site: the frame has none
            if (sq)
                sq[at + x] = none ? 0x7FFFFFFF : v;
            if (dist)
                dist[at + x] = none ? __builtin_inff() : __builtin_sqrtf((float)v);
            if (nearest)
                nearest[at + x] = none ? -1 : (y + d) * w + o;
        }
        __syncthreads();  // the next row goes over dyl and opt
    }
}

hipError_t raise_lds(const void* kernel, size_t lds)
{
    return lds > 48 * 1024 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

}  // namespace

int dist_col_lds_bytes(int h)
{
    return h >= 1 && h <= kDistMaxDim ? (int)dist_col_plan(h).lds : 0;
}

size_t dist_scratch_bytes(int w, int h, int nframes)
{
    if (w < 1 || h < 1 || nframes < 1 || w > kDistMaxDim || h > kDistMaxDim)
        return 0;
    return (size_t)nframes * (size_t)h * (size_t)((w + 3) & ~3) * sizeof(int16_t);
}

hipError_t launch_dist(hipStream_t stream, const uint8_t* d_in, int32_t* d_sq, float* d_dist, int32_t* d_nearest,
                       int16_t* d_scratch, int w, int h, int nframes)
{
    if (dist_scratch_bytes(w, h, nframes) == 0 || (!d_sq && !d_dist && !d_nearest) || !d_in || !d_scratch)
        return hipErrorInvalidValue;
    const int ws = (w + 3) & ~3;
    const DistColPlan cp = dist_col_plan(h);
    const uint32_t groups_x = (uint32_t)((w + kDistColW - 1) / kDistColW);
    const uint64_t items = (uint64_t)groups_x * (uint64_t)nframes;
    hipError_t e = raise_lds(reinterpret_cast<const void*>(dist_cols_kernel), cp.lds);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dist_cols_kernel, dim3((uint32_t)(items < kDistMaxBlocks ? items : kDistMaxBlocks)), dim3(cp.threads),
                       cp.lds, stream, d_in, d_scratch, w, ws, h, groups_x, items, cp.chunks, cp.chunks_per_seg, cp.segs);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    int levels = 1;
    while ((1 << levels) <= w)  // the smallest L with 2^L > w
        levels++;
    const uint64_t rows = (uint64_t)nframes * (uint64_t)h;
    const size_t lds = (size_t)ws * (sizeof(int16_t) + sizeof(uint16_t));
    e = raise_lds(reinterpret_cast<const void*>(dist_rows_kernel), lds);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dist_rows_kernel, dim3((uint32_t)(rows < kDistMaxBlocks ? rows : kDistMaxBlocks)), dim3(kWave), lds,
                       stream, d_scratch, d_sq, d_dist, d_nearest, w, ws, h, rows, levels);
    return hipGetLastError();
}

}  // namespace mi355
