// ccl.hip — connected-component labelling with statistics of single-channel masks
// (cv::connectedComponentsWithStats(mask, labels, stats, centroids, connectivity, CV_32S)).  Semantics:
// include/mi355_imgfilter.h, "the blobs of a mask"; design, loop bounds and the staleness argument: DESIGN.md section 6j.
//
// The int32 label output is the union-find parent array from the first launch to the last; the only scratch is one
// count (then offset) per kCclFlatPx pixels.  A pixel's entry holds a LABEL VALUE v = (index of another pixel of the
// same frame and component) + 1, never larger than the pixel's own index + 1; a root holds its own index + 1;
// background holds 0.  Kernel boundaries are the only ordering between workgroups: no flag, no grid barrier, no ticket.
// Grids, chunk walk and prefix sums: mask_common.hpp.  Union-find and neighbour rule: once, below.
//   ccl_local_kernel     a block owns a 64 x 32 tile: row masks in LDS from 16-byte aligned vectors of the source (a
//                        row is at any alignment: chunks the row does not cover whole go byte by byte), every pixel
//                        starts at the first pixel of its row run (bit operations on the 64-bit row mask), runs of
//                        neighbouring rows are united in LDS, and every pixel stores its tile root's value;
//   ccl_seam_kernel      one thread per pixel of a tile's top row or left column (not the frame's): unions with the
//                        foreground neighbours across the border, in global memory, agent-scope atomics only;
//   ccl_compress_kernel  the same threads and the pixel opposite each: parent[q] and parent[parent[q]] take q's root.
//                        Only tile roots ever get a new parent in the seam launch, and a tile root with a new parent
//                        has a border pixel in its tile component, so afterwards EVERY tile root holds its root;
//   ccl_flatten_kernel   a block owns kCclFlatPx raster-consecutive pixels: two loads give a pixel its root (no walk);
//                        a root takes -(its rank among the roots of the block + 1) instead, the block stores its count;
//   ccl_scan_kernel      one block per frame: counts -> exclusive offsets, in place, and the frame's N;
//   ccl_relabel_kernel   final number = block offset + rank + 1 from the root's entry; with statistics every wave
//                        finds its row runs of equal labels (one accumulate per run, closed-form sums), a block merges
//                        runs in a 64-slot LDS table and adds each occupied slot once to the global row;
//   ccl_stats_init / _finish   the accumulators' identities before, {left, top, width, height, area} and the empty rows
//                        after.
// The first three take a wave-uniform `low`: a pixel is foreground iff its byte > low.  The labelling call passes 0
// ("not zero"); the hysteresis of canny.hip runs just these three (launch_ccl_unite) with its lower threshold.
#include "common.hpp"
#include "kernels.hpp"
#include "mask_common.hpp"

namespace mi355 {

namespace {

constexpr int kTileW = 64;  // one wave lane per tile column: a tile row's foreground is one 64-bit mask
constexpr int kTileH = 32;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRowsPerWave = kTileH / kWaves;
constexpr int kRowChunks = aligned_chunks_of(kTileW);  // of a tile row, at any alignment
constexpr int kFlatIters = kCclFlatPx / kThreads;  // a wave owns kFlatIters x 64 consecutive pixels of a flat block
constexpr int kSlots = 64;                         // of a block's LDS statistics table
static_assert(kTileW == kWave && kTileH * kRowChunks <= kThreads && kCclFlatPx % kThreads == 0, "tile geometry");

struct CclGeom {
    uint32_t w, h, npx;  // npx = w h < 2^31
    uint32_t ntx, nty;   // tiles per frame
    uint32_t seam_h;     // (nty - 1) w: the pixels of the tiles' top rows, the frame's first row apart
    uint32_t seam;       // seam_h + (ntx - 1) h: with the pixels of the tiles' left columns
    uint32_t nflat;      // flat blocks per frame
};

// ---- lock-free union-find by fetch_min -------------------------------------------------------------------------------------
// Element v = index + kBias; its entry lab[v - kBias] holds a member of its set that is not larger, a root itself.  Twice:
// a tile in LDS (kWg, bias 0) and a frame's parent array while other workgroups write it (kAgent, bias 1: 0 is background).
// bound of find: the walk goes to strictly smaller values, fewer steps than elements (kTileW kTileH, w h).  A value read
// late or early is still an ancestor: an entry only ever decreases, and only to an ancestor of what it held.
// bound of union: max(a, b) strictly decreases with every trip, fewer trips than elements; no CAS, nothing is retried.
constexpr int kWg = __HIP_MEMORY_SCOPE_WORKGROUP, kAgent = __HIP_MEMORY_SCOPE_AGENT;
template <int kScope, int kBias, class T>
__device__ __forceinline__ T uf_find(T* lab, T v)
{
    for (;;) {
        const T nx = __hip_atomic_load(lab + (v - kBias), __ATOMIC_RELAXED, kScope);
        if (nx == v)
            return v;
        v = nx;
    }
}

template <int kScope, int kBias, class T>
__device__ __forceinline__ void uf_union(T* lab, T a, T b)
{
    a = uf_find<kScope, kBias>(lab, a);
    b = uf_find<kScope, kBias>(lab, b);
    while (a != b) {
        if (a < b) {
            const T t = a;
            a = b;
            b = t;
        }
        const T old = __hip_atomic_fetch_min(lab + (a - kBias), b, __ATOMIC_RELAXED, kScope);
        if (old == a)
            break;
        a = old;
    }
}

// A foreground pixel and `up`, the pixel above it; c_l / c_r its own left and right neighbours, u_l / u_r those of `up`.
// unite(d): with the pixel d columns from `up`.  A pair of runs is united once: the left neighbours do it if both are set.
template <class F>
__device__ __forceinline__ void unite_with_row_above(bool up, bool c_l, bool c_r, bool u_l, bool u_r, int conn8, F unite)
{
    if (up) {
        if (!(c_l && u_l))
            unite(0);
    } else if (conn8) {  // the pixel above is background: the two diagonal neighbours are in runs of their own
        if (u_l && !c_l)
            unite(-1);
        if (u_r && !c_r)
            unite(1);
    }
}

// ---- the tile in LDS ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t row_mask(const uint32_t* smask, int r)
{
    return (uint64_t)smask[2 * r] | ((uint64_t)smask[2 * r + 1] << 32);
}

__global__ __launch_bounds__(kThreads) void ccl_local_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ labels,
                                                             CclGeom g, int conn8, uint32_t low)
{
    __shared__ uint32_t smask[kTileH * 2];
    __shared__ uint32_t lab[kTileH * kTileW];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const auto [f, t, item] = frame_block(g.ntx * g.nty, 1);
    const uint32_t tj = t / g.ntx, ti = t - tj * g.ntx;
    const uint32_t x0 = ti * kTileW, y0 = tj * kTileH;
    const int n = (int)(g.w - x0 < (uint32_t)kTileW ? g.w - x0 : (uint32_t)kTileW);     // columns of the frame
    const int rows = (int)(g.h - y0 < (uint32_t)kTileH ? g.h - y0 : (uint32_t)kTileH);  // rows of the frame
    const uint8_t* p = in + (size_t)f * g.npx;
    if (tid < kTileH * 2)
        smask[tid] = 0;
    __syncthreads();
    // the foreground bits of (row r, aligned chunk s)
    if (tid < kTileH * kRowChunks) {
        const int r = tid / kRowChunks, s = tid - r * kRowChunks;
        if (r < rows) {
            const uint8_t* row = p + (size_t)(y0 + (uint32_t)r) * g.w + x0;
            const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15u);
            const AlignedChunk<int> c = aligned_chunk<int>(mis, s, n);  // of the row's n bytes
            const uint8_t* chunk = row + c.first;
            uint32_t bits = 0;  // bit i: byte b0 + i of the chunk is foreground (> low)
            if (c.whole()) {
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(chunk));
#pragma unroll
                for (int j = 0; j < 16; j++)
                    bits |= (chunk_byte(v, j) > low ? 1u : 0u) << j;
            } else {
                for (int j = c.b0; j < c.b1; j++)  // bound: fewer than 16 bytes
                    bits |= (chunk[j] > low ? 1u : 0u) << (j - c.b0);
            }
            if (bits) {
                const uint64_t m = (uint64_t)bits << (c.first + c.b0);
                if ((uint32_t)m)
                    __hip_atomic_fetch_or(smask + 2 * r, (uint32_t)m, MI355_RELAXED_WG);
                if ((uint32_t)(m >> 32))
                    __hip_atomic_fetch_or(smask + 2 * r + 1, (uint32_t)(m >> 32), MI355_RELAXED_WG);
            }
        }
    }
    __syncthreads();
    // every pixel starts at the first pixel of its row run
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) {
        const int r = wv + kWaves * i;
        const uint64_t m = row_mask(smask, r);
        const uint64_t z = ~m & ((1ull << lane) - 1);  // the background pixels left of the lane
        const int start = z ? 64 - __clzll((long long)z) : 0;
        lab[r * kTileW + lane] = (uint32_t)(r * kTileW + start);
    }
    __syncthreads();
    // unite the runs of neighbouring rows: once per pair of runs where the row masks show that a left neighbour does it
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) {
        const int r = wv + kWaves * i;
        if (r == 0)
            continue;
        const uint64_t cur = row_mask(smask, r), up = row_mask(smask, r - 1);
        if (!((cur >> lane) & 1u))
            continue;
        const bool c_l = lane > 0 && ((cur >> (lane - 1)) & 1u), c_r = lane < 63 && ((cur >> (lane + 1)) & 1u);
        const bool u_l = lane > 0 && ((up >> (lane - 1)) & 1u), u_r = lane < 63 && ((up >> (lane + 1)) & 1u);
        const uint32_t me = (uint32_t)(r * kTileW + lane), above = me - kTileW;
        unite_with_row_above((up >> lane) & 1u, c_l, c_r, u_l, u_r, conn8,
                             [&](int d) { uf_union<kWg, 0>(lab, me, above + (uint32_t)d); });
    }
    __syncthreads();
    int32_t* out = labels + (size_t)f * g.npx;
#pragma unroll
    for (int i = 0; i < kRowsPerWave; i++) {
        const int r = wv + kWaves * i;
        if (r >= rows || lane >= n)
            continue;
        int32_t v = 0;
        if ((row_mask(smask, r) >> lane) & 1u) {
            const uint32_t root = uf_find<kWg, 0>(lab, (uint32_t)(r * kTileW + lane));
            v = (int32_t)((y0 + root / kTileW) * g.w + x0 + (root & (kTileW - 1)) + 1u);
        }
        out[(size_t)(y0 + (uint32_t)r) * g.w + x0 + (uint32_t)lane] = v;
    }
}

// ---- the parent array in global memory while other workgroups write it ----------------------------------------------------
// The seam pixel of item i of a frame: (x, y) in the top row of a tile (horizontal = true, y > 0) or in the left column
// of a tile (x > 0).  A tile's corner pixel appears once as each.
struct SeamPixel {
    bool horizontal;
    uint32_t x, y;
};
__device__ __forceinline__ SeamPixel seam_pixel(const CclGeom& g, uint32_t i)
{
    if (i < g.seam_h) {
        const uint32_t k = i / g.w;
        return {true, i - k * g.w, (k + 1) * kTileH};
    }
    const uint32_t j = i - g.seam_h, k = j / g.h;
    return {false, (k + 1) * kTileW, j - k * g.h};
}

__global__ __launch_bounds__(kThreads) void ccl_seam_kernel(const uint8_t* __restrict__ in, int32_t* labels, CclGeom g,
                                                            uint32_t bpf, int conn8, uint32_t low)
{
    const auto [f, blk, i] = frame_block(bpf, kThreads);
    if (i >= g.seam)
        return;
    const auto [hor, x, y] = seam_pixel(g, i);
    const uint8_t* p = in + (size_t)f * g.npx;
    int32_t* lab = labels + (size_t)f * g.npx;
    const uint32_t w = g.w, at = y * w + x;
    auto fg = [&](uint32_t q) { return p[q] > low; };  // foreground, as the local kernel saw it
    if (!fg(at))
        return;
    const int32_t me = (int32_t)at + 1;
    if (hor) {
        // the row above belongs to another tile: the local kernel's rule, on the frame's rows
        const bool c_l = x > 0 && fg(at - 1), c_r = x + 1 < w && fg(at + 1);
        const bool u_l = x > 0 && fg(at - w - 1), u_r = x + 1 < w && fg(at - w + 1);
        unite_with_row_above(fg(at - w), c_l, c_r, u_l, u_r, conn8,
                             [&](int d) { uf_union<kAgent, 1>(lab, me, me - (int32_t)w + d); });
    } else {
        // the column on the left belongs to another tile; the pair one row up does it when both its pixels are set and
        // the local kernel has united this pixel with the one above it (a tile's top row is united with the row above
        // by the branch above, which may itself count on this union: no skipping there)
        if (fg(at - 1)) {
            if (!(y % kTileH != 0 && fg(at - w) && fg(at - w - 1)))
                uf_union<kAgent, 1>(lab, me, me - 1);
        } else if (conn8) {
            if (y > 0 && fg(at - w - 1) && !fg(at - w))
                uf_union<kAgent, 1>(lab, me, me - (int32_t)w - 1);
            if (y + 1 < g.h && fg(at + w - 1) && !fg(at + w))
                uf_union<kAgent, 1>(lab, me, me + (int32_t)w - 1);
        }
    }
}

// parent[q] and parent[parent[q]] take q's root.  No union runs in this launch, so a root stays a root and every store
// writes the one final value of its entry; concurrent readers see the old ancestor or the root
__device__ __forceinline__ void compress_pixel(int32_t* lab, uint32_t q)
{
    const int32_t a = __hip_atomic_load(lab + q, MI355_RELAXED_AGENT);
    const int32_t r = uf_find<kAgent, 1>(lab, a);
    if (a != r)
        __hip_atomic_store(lab + (a - 1), r, MI355_RELAXED_AGENT);
    if (a != r)
        __hip_atomic_store(lab + q, r, MI355_RELAXED_AGENT);
}

__global__ __launch_bounds__(kThreads) void ccl_compress_kernel(const uint8_t* __restrict__ in, int32_t* labels,
                                                                CclGeom g, uint32_t bpf, uint32_t low)
{
    const auto [f, blk, i] = frame_block(bpf, kThreads);
    if (i >= g.seam)
        return;
    const auto [hor, x, y] = seam_pixel(g, i);
    const uint8_t* p = in + (size_t)f * g.npx;
    int32_t* lab = labels + (size_t)f * g.npx;
    const uint32_t at = y * g.w + x, opposite = hor ? at - g.w : at - 1;
    if (p[at] > low)
        compress_pixel(lab, at);
    if (p[opposite] > low)
        compress_pixel(lab, opposite);
}

// ---- flat blocks: kCclFlatPx raster-consecutive pixels, a wave kFlatIters x 64 of them in order -------------------------
__device__ __forceinline__ uint32_t flat_pixel(uint32_t b, int wv, int i, int lane)
{
    return b * kCclFlatPx + (uint32_t)((wv * kFlatIters + i) * kWave + lane);
}

__global__ __launch_bounds__(kThreads) void ccl_flatten_kernel(int32_t* labels, uint32_t* __restrict__ counts, CclGeom g)
{
    __shared__ uint32_t s_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const auto [f, b, item] = frame_block(g.nflat, kCclFlatPx);
    int32_t* lab = labels + (size_t)f * g.npx;
    int rank[kFlatIters];  // of the roots among the wave's roots, -1: not a root
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < kFlatIters; i++) {
        const uint32_t px = flat_pixel(b, wv, i, lane);
        bool is_root = false;
        if (px < g.npx) {
            // only this thread writes lab[px]; lab[a - 1] is a tile root's entry: its root since the compress launch, or
            // itself, or already its rank (negative) if it is a root of this launch
            const int32_t a = lab[px];
            if (a > 0) {
                const int32_t v = __hip_atomic_load(lab + (a - 1), MI355_RELAXED_WG);
                const int32_t root = v < 0 ? a : v;
                is_root = root == (int32_t)px + 1;
                if (!is_root && root != a)
                    __hip_atomic_store(lab + px, root, MI355_RELAXED_WG);
            }
        }
        const uint64_t m = __ballot(is_root);
        rank[i] = is_root ? (int)(cnt + lanes_below(m, lane)) : -1;
        cnt += (uint32_t)__popcll(m);
    }
    const BlockOffsets o = block_offsets<kWaves>(cnt, s_cnt, lane, wv);  // cnt is the same in every lane
#pragma unroll
    for (int i = 0; i < kFlatIters; i++)
        if (rank[i] >= 0)
            __hip_atomic_store(lab + flat_pixel(b, wv, i, lane), -(int32_t)(o.before + (uint32_t)rank[i] + 1u),
                               MI355_RELAXED_WG);
    if (tid == 0)
        counts[(size_t)f * g.nflat + b] = o.total;
}

// one block per frame: the frame's block counts become exclusive offsets in place; N = the roots + 1 (the background)
__global__ __launch_bounds__(kThreads) void ccl_scan_kernel(uint32_t* __restrict__ counts, int32_t* __restrict__ count,
                                                            uint32_t nflat)
{
    __shared__ uint32_t s_sum[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    uint32_t* c = counts + (size_t)blockIdx.x * nflat;
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < nflat; k0 += kThreads) {  // bound: nflat / 256 trips, rounded up
        const uint32_t k = k0 + tid;
        const uint32_t own = k < nflat ? c[k] : 0;
        const uint32_t inc = wave_scan_inclusive(own, lane);
        const BlockOffsets o = block_offsets<kWaves>(inc, s_sum, lane, wv);
        if (k < nflat)
            c[k] = carry + o.before + inc - own;
        carry += o.total;
        __syncthreads();  // s_sum is written again in the next trip
    }
    if (tid == 0)
        count[blockIdx.x] = (int32_t)(carry + 1u);
}

// ---- statistics -----------------------------------------------------------------------------------------------------------
// While they accumulate, a row of d_stats is {min x, min y, max x, max y, area} and a row of d_sums {sum x, sum y}.
struct RunStats {
    int x0, x1, y;
    uint32_t n;
    uint64_t sx, sy;
};

__device__ __forceinline__ void stats_to_global(int32_t* st, unsigned long long* sm, int minx, int miny, int maxx,
                                                int maxy, uint32_t area, uint64_t sx, uint64_t sy)
{
    __hip_atomic_fetch_min(st + 0, minx, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_min(st + 1, miny, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_max(st + 2, maxx, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_max(st + 3, maxy, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_add(st + 4, (int32_t)area, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_add(sm + 0, (unsigned long long)sx, MI355_RELAXED_AGENT);
    __hip_atomic_fetch_add(sm + 1, (unsigned long long)sy, MI355_RELAXED_AGENT);
}

struct BlockStats {
    int32_t key[kSlots];  // the slot's label, -1: free
    int32_t minx[kSlots], miny[kSlots], maxx[kSlots], maxy[kSlots];
    uint32_t area[kSlots];
    unsigned long long sx[kSlots], sy[kSlots];
};

template <bool kStats>
__global__ __launch_bounds__(kThreads) void ccl_relabel_kernel(int32_t* labels, const uint32_t* __restrict__ offsets,
                                                               int32_t* stats, unsigned long long* sums, CclGeom g,
                                                               uint32_t stats_rows)
{
    __shared__ BlockStats bs;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const auto [f, b, item] = frame_block(g.nflat, kCclFlatPx);
    int32_t* lab = labels + (size_t)f * g.npx;
    const uint32_t* offs = offsets + (size_t)f * g.nflat;
    int32_t* st = kStats ? stats + (size_t)f * stats_rows * 5 : nullptr;
    unsigned long long* sm = kStats ? sums + (size_t)f * stats_rows * 2 : nullptr;
    if (kStats) {
        if (tid < kSlots) {
            bs.key[tid] = -1;
            bs.minx[tid] = bs.miny[tid] = 0x7FFFFFFF;
            bs.maxx[tid] = bs.maxy[tid] = -1;
            bs.area[tid] = 0;
            bs.sx[tid] = bs.sy[tid] = 0;
        }
        __syncthreads();
    }
    const uint32_t own_off = offs[b];
#pragma unroll 2
    for (int i = 0; i < kFlatIters; i++) {
        const uint32_t px = flat_pixel(b, wv, i, lane);
        const bool valid = px < g.npx;
        int32_t fin = 0;
        if (valid) {
            // only this thread writes lab[px].  A root's entry is its rank (negative) or, once its own thread has been
            // here, its final number (positive): both give the same number
            const int32_t a = lab[px];
            if (a < 0) {
                fin = (int32_t)own_off - a;
            } else if (a > 0) {
                const int32_t v = __hip_atomic_load(lab + (a - 1), MI355_RELAXED_WG);
                fin = v < 0 ? (int32_t)offs[(uint32_t)(a - 1) / kCclFlatPx] - v : v;
            }
            if (a != 0)
                __hip_atomic_store(lab + px, fin, MI355_RELAXED_WG);
        }
        if (!kStats)
            continue;
        // the wave's 64 pixels are consecutive: a run is a stretch of one label in one row, its first lane accumulates it
        const uint32_t y = px / g.w, x = px - y * g.w;
        const int32_t left = __shfl_up(fin, 1);
        const bool head = valid && (lane == 0 || x == 0 || left != fin);
        const uint64_t hm = __ballot(head);
        const int nvalid = __popcll(__ballot(valid));  // the valid lanes are the first ones
        if (!head || (uint32_t)fin >= stats_rows)
            continue;
        const uint64_t later = lane < 63 ? hm & ~((2ull << lane) - 1) : 0;
        const uint32_t n = (uint32_t)((later ? __ffsll((long long)later) - 1 : nvalid) - lane);
        const uint64_t sx = (uint64_t)n * x + (uint64_t)n * (n - 1) / 2, sy = (uint64_t)n * y;
        const int x1 = (int)(x + n - 1);
        const int s = fin & (kSlots - 1);
        int32_t expected = -1;
        const bool mine = __hip_atomic_compare_exchange_strong(&bs.key[s], &expected, fin, __ATOMIC_RELAXED,
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ||
                          expected == fin;
        if (mine) {
            __hip_atomic_fetch_min(&bs.minx[s], (int32_t)x, MI355_RELAXED_WG);
            __hip_atomic_fetch_min(&bs.miny[s], (int32_t)y, MI355_RELAXED_WG);
            __hip_atomic_fetch_max(&bs.maxx[s], x1, MI355_RELAXED_WG);
            __hip_atomic_fetch_max(&bs.maxy[s], (int32_t)y, MI355_RELAXED_WG);
            __hip_atomic_fetch_add(&bs.area[s], n, MI355_RELAXED_WG);
            __hip_atomic_fetch_add(&bs.sx[s], (unsigned long long)sx, MI355_RELAXED_WG);
            __hip_atomic_fetch_add(&bs.sy[s], (unsigned long long)sy, MI355_RELAXED_WG);
        } else {
            // the slot holds another label of this block
            stats_to_global(st + (size_t)fin * 5, sm + (size_t)fin * 2, (int)x, (int)y, x1, (int)y, n, sx, sy);
        }
    }
    if (kStats) {
        __syncthreads();
        if (tid < kSlots && bs.key[tid] >= 0) {
            const size_t l = (size_t)bs.key[tid];
            stats_to_global(st + l * 5, sm + l * 2, bs.minx[tid], bs.miny[tid], bs.maxx[tid], bs.maxy[tid], bs.area[tid],
                            bs.sx[tid], bs.sy[tid]);
        }
    }
}

__global__ __launch_bounds__(kThreads) void ccl_stats_init_kernel(int32_t* __restrict__ stats,
                                                                  unsigned long long* __restrict__ sums, uint64_t rows)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows)
        return;
    int32_t* st = stats + r * 5;
    st[0] = st[1] = 0x7FFFFFFF;
    st[2] = st[3] = -1;
    st[4] = 0;
    sums[r * 2] = sums[r * 2 + 1] = 0;
}

// {min x, min y, max x, max y, area} -> {left, top, width, height, area}; a row without a pixel is all zeros
__global__ __launch_bounds__(kThreads) void ccl_stats_finish_kernel(int32_t* __restrict__ stats, uint64_t rows)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows)
        return;
    int32_t* st = stats + r * 5;
    if (st[4] == 0) {
        st[0] = st[1] = st[2] = st[3] = 0;
    } else {
        st[2] = st[2] - st[0] + 1;
        st[3] = st[3] - st[1] + 1;
    }
}

bool ccl_geom(int w, int h, int nframes, CclGeom* g)
{
    if (!hist_frames_ok(w, h, nframes))
        return false;
    const uint32_t uw = (uint32_t)w, uh = (uint32_t)h, npx = uw * uh;
    const uint32_t ntx = (uw + kTileW - 1) / kTileW, nty = (uh + kTileH - 1) / kTileH;
    const uint32_t seam_h = (nty - 1) * uw;
    *g = {uw, uh, npx, ntx, nty, seam_h, seam_h + (ntx - 1) * uh, (npx + kCclFlatPx - 1) / kCclFlatPx};
    return true;
}

// The union launches: local, and where the frame has more than one tile, seam and compress.  Afterwards a foreground
// pixel q reaches its root in two loads: labels[q] is a tile root's value (or already the root's), and a tile root's
// entry holds its root's value.  Their grids: a block per tile, a thread per seam pixel
FrameGrid tile_grid(const CclGeom& g, int nframes) { return frame_grid((uint64_t)g.ntx * g.nty, 1, nframes); }
FrameGrid seam_grid(const CclGeom& g, int nframes) { return frame_grid(g.seam, kThreads, nframes); }

hipError_t enqueue_unite(hipStream_t stream, const uint8_t* d_in, int32_t* d_labels, const CclGeom& g, int nframes,
                         bool conn8, uint32_t low)
{
    const FrameGrid tiles = tile_grid(g, nframes), seam = seam_grid(g, nframes);
    if (!tiles.ok || !seam.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles.blocks), dim3(kThreads), 0, stream, d_in, d_labels, g, conn8 ? 1 : 0,
                       low);
    if (g.seam) {
        hipLaunchKernelGGL(ccl_seam_kernel, dim3(seam.blocks), dim3(kThreads), 0, stream, d_in, d_labels, g, seam.bpf,
                           conn8 ? 1 : 0, low);
        hipLaunchKernelGGL(ccl_compress_kernel, dim3(seam.blocks), dim3(kThreads), 0, stream, d_in, d_labels, g, seam.bpf,
                           low);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ccl_unite(hipStream_t stream, const uint8_t* d_in, int32_t* d_parent, int w, int h, int nframes,
                            bool conn8, int low)
{
    CclGeom g;
    if (!ccl_geom(w, h, nframes, &g) || low < 0 || low > 255)
        return hipErrorInvalidValue;
    return enqueue_unite(stream, d_in, d_parent, g, nframes, conn8, (uint32_t)low);
}

size_t ccl_scratch_bytes(int w, int h, int nframes)
{
    CclGeom g;
    return ccl_geom(w, h, nframes, &g) ? (size_t)nframes * g.nflat * sizeof(uint32_t) : 0;
}

hipError_t launch_ccl(hipStream_t stream, const uint8_t* d_in, int32_t* d_labels, int32_t* d_count, int32_t* d_stats,
                      uint64_t* d_sums, uint32_t* d_scratch, int w, int h, int nframes, bool conn8, int stats_rows)
{
    CclGeom g;
    if (!ccl_geom(w, h, nframes, &g) || stats_rows < 0 || stats_rows > kCclMaxStatsRows)
        return hipErrorInvalidValue;
    const FrameGrid flat = frame_grid(g.npx, kCclFlatPx, nframes);  // flat.bpf is g.nflat
    const uint64_t rows = (uint64_t)nframes * (uint64_t)stats_rows;
    const FrameGrid rowg = frame_grid(rows, kThreads, 1);
    if (!tile_grid(g, nframes).ok || !seam_grid(g, nframes).ok || !flat.ok || !rowg.ok)
        return hipErrorInvalidValue;  // before the first launch
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(d_sums);
    if (rows)
        hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(rowg.blocks), dim3(kThreads), 0, stream, d_stats, sums, rows);
    const hipError_t ue = enqueue_unite(stream, d_in, d_labels, g, nframes, conn8, 0u);  // foreground: not zero
    if (ue != hipSuccess)
        return ue;
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(flat.blocks), dim3(kThreads), 0, stream, d_labels, d_scratch, g);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3((uint32_t)nframes), dim3(kThreads), 0, stream, d_scratch, d_count, g.nflat);
    if (rows) {
        hipLaunchKernelGGL(ccl_relabel_kernel<true>, dim3(flat.blocks), dim3(kThreads), 0, stream, d_labels, d_scratch,
                           d_stats, sums, g, (uint32_t)stats_rows);
        hipLaunchKernelGGL(ccl_stats_finish_kernel, dim3(rowg.blocks), dim3(kThreads), 0, stream, d_stats, rows);
    } else {
        hipLaunchKernelGGL(ccl_relabel_kernel<false>, dim3(flat.blocks), dim3(kThreads), 0, stream, d_labels, d_scratch,
                           (int32_t*)nullptr, (unsigned long long*)nullptr, g, 0u);
    }
    return hipGetLastError();
}

}  // namespace mi355
