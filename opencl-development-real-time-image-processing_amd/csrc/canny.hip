// canny.hip — cv::Canny(image, edges, threshold1, threshold2, 3, L2gradient) and hysteresis thresholding of
// single-channel frames.  Semantics: include/mi355_imgfilter.h, "from gradients to edges"; design, the two-load-root
// argument and the loop bounds: DESIGN.md section 6k.  Everything is integer arithmetic; there is no float in this file.
//
//   canny_nms_kernel   the hot path, on the tile frame of tile_common.hpp as gray8.hip uses it.  A workgroup (256
//                      threads) turns the source bytes of a 256 x 16 tile into one class byte per pixel (0 none,
//                      1 candidate, 2 strong):
//                        1. stage the tile with a 2-pixel clamped halo as raw bytes in LDS, in 16-byte chunks;
//                        2. the 3x3 Sobel pair of the tile plus one ring, four positions side by side per thread and
//                           trip (six dword reads of staged bytes, one 16-byte write).  A position leaves one LDS word:
//                           magnitude << 2 | direction, the direction being all the non-maximum test needs of (dx, dy):
//                           0 along the row, 1 along the column, 2 the (-1, -1) / (+1, +1) diagonal, 3 the other one.
//                           Positions outside the frame leave 0.  Ring rows are 260 words apart, so a thread's four
//                           words and its neighbours' are 16-byte aligned: consecutive lanes read and write consecutive
//                           16-byte pieces;
//                        3. classify the 256 x 16 pixels, four side by side per thread, from 6 x 3 words of the ring;
//                        4. the class tile leaves LDS as one 16-byte store per thread and row piece (store_chunk16).
//                      Algorithmic bytes: 2 B/px.
//   the union          ccl.hip's local, seam and compress launches (launch_ccl_unite), foreground = byte > low.
//   hyst_mark_kernel   every strong pixel finds its root with two loads and sets bit 31 of the root's own entry.
//   hyst_emit_kernel   every pixel: 255 iff it is a candidate and its root's entry has bit 31, else 0; 16 pixels per thread,
//                      one 16-byte store where the chunk lies inside the frame.  It may write over its own input.
//                      Both walk the frame's aligned chunks (mask_common.hpp) and share root_is_marked.
// Kernel boundaries are the only ordering between workgroups: no flag, no grid barrier, no retry.  The mark and emit
// kernels have no loop but the 16 bytes of a chunk.
#include "common.hpp"
#include "kernels.hpp"
#include "mask_common.hpp"
#include "tile_common.hpp"

namespace mi355 {

namespace {

constexpr int kCnTW = 256;  // output tile width (bytes)
constexpr int kCnTH = 16;   // output tile height
constexpr int kCnThreads = 256;
constexpr int kCnRawH = kCnTH + 4;                     // the tile and a 2-pixel halo: the Sobel of the ring reads it
constexpr int kCnRawS = (kCnTW + 4 + 15) / 16 * 16;    // staged row stride, whole 16-byte chunks
constexpr int kCnMagH = kCnTH + 2;                     // the tile and one ring: kCnTW + 2 columns ...
constexpr int kCnGroups = (kCnTW + 2 + 3) / 4;         // ... in groups of four side by side, one thread each
constexpr int kCnMagS = 4 * kCnGroups;                 // ring row stride in words: rows start on 16-byte boundaries
static_assert(kCnRawS % 16 == 0 && (kCnTH * kCnTW) % kCnThreads == 0 && kCnTW % 16 == 0, "tile geometry");
static_assert(kCnMagS + 4 <= kCnRawS, "the last group's two dword reads stay inside the staged row");

// |dx|, |dy| <= 4 * 255 = 1020, so dx^2 + dy^2 <= 2 080 800 < 2^21 and the word magnitude << 2 | direction fits 23 bits.
// The direction test in 32 bits: y = |dy| << 15 <= 1020 * 2^15 < 2^25, tg22x = |dx| * 13573 < 2^24,
// tg67x = tg22x + (|dx| << 16) < 2^24 + 2^26: nothing comes near 2^31.
template <bool L2>
__global__ __launch_bounds__(kCnThreads) void canny_nms_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                               int w, int h, int tiles_x, int tiles_y, uint32_t ntiles,
                                                               int low, int high)
{
    __shared__ __attribute__((aligned(16))) uint8_t raw[kCnRawH * kCnRawS];
    __shared__ __attribute__((aligned(16))) uint32_t mag[kCnMagH * kCnMagS];
    __shared__ __attribute__((aligned(16))) uint8_t O[kCnTH * kCnTW];
    const TilePos t = tile_decode(xcd_remap(blockIdx.x, ntiles), tiles_x, tiles_y, kCnTW, kCnTH);
    const uint8_t* fin = in + t.frame * (size_t)w * h;
    uint8_t* fout = out + t.frame * (size_t)w * h;
    const int x0 = t.x0, y0 = t.y0;
    const int sy0 = y0 - 2, sx0 = x0 - 2;  // image position of staged byte (0, 0)
    const int tid = threadIdx.x;

    // 1. stage: staged (s, c) = image (clamp(sy0 + s), clamp(sx0 + c))
    constexpr int kStagePieces = kCnRawS / 16;
    for (int i = tid; i < kCnRawH * kStagePieces; i += kCnThreads) {  // bound: (kCnTH + 4) * 17 / 256 trips, rounded up
        const int s = i / kStagePieces, p = i - s * kStagePieces;
        const uint8_t* row = fin + (size_t)border_index<kBorderClamp>(sy0 + s, h) * w;
        const int gx = sx0 + 16 * p;
        u32x4 v;
        if (gx >= 0 && gx + 16 <= w) {
            v = *reinterpret_cast<const u32x4_a1*>(row + gx);
        } else {
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++)
                b[j] = row[border_index<kBorderClamp>(gx + j, w)];
#pragma unroll
            for (int q = 0; q < 4; q++)
                v[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
        }
        *reinterpret_cast<u32x4*>(raw + s * kCnRawS + 16 * p) = v;
    }
    __syncthreads();

    // 2. ring position (r, c) is image (y0 - 1 + r, x0 - 1 + c); its 3x3 window starts at staged (r, c).  A thread takes
    //    four positions side by side: six staged bytes of three rows (two dword reads each) give six column sums
    //    V = a + 2 m + b and six column differences D = b - a; dx = V[j + 2] - V[j], dy = D[j] + 2 D[j + 1] + D[j + 2]
    for (int i = tid; i < kCnMagH * kCnGroups; i += kCnThreads) {  // bound: (kCnTH + 2) * 65 / 256 trips, rounded up
        const int r = i / kCnGroups, c = 4 * (i - r * kCnGroups);
        const int gy = y0 - 1 + r, gx = x0 - 1 + c;
        const uint8_t* a = raw + r * kCnRawS + c;
        const uint32_t* ra = reinterpret_cast<const uint32_t*>(a);
        const uint32_t* rm = reinterpret_cast<const uint32_t*>(a + kCnRawS);
        const uint32_t* rb = reinterpret_cast<const uint32_t*>(a + 2 * kCnRawS);
        const uint32_t va[2] = {ra[0], ra[1]}, vm[2] = {rm[0], rm[1]}, vb[2] = {rb[0], rb[1]};
        int V[6], D[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int sh = 8 * (k & 3);  // one v_bfe_u32 per byte
            const int pa = (int)((va[k >> 2] >> sh) & 0xFFu), pm = (int)((vm[k >> 2] >> sh) & 0xFFu);
            const int pb = (int)((vb[k >> 2] >> sh) & 0xFFu);
            V[k] = pa + 2 * pm + pb;
            D[k] = pb - pa;
        }
        const bool row_in = gy >= 0 && gy < h;
        u32x4 words;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int dx = V[j + 2] - V[j], dy = D[j] + 2 * D[j + 1] + D[j + 2];
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            // every factor is below 2^24: the full-rate 24-bit multiplier
            const int mg = L2 ? __mul24(dx, dx) + __mul24(dy, dy) : ax + ay;
            const int y = ay << 15, tg22x = __mul24(ax, 13573), tg67x = tg22x + (ax << 16);
            const int dir = y < tg22x ? 0 : (y > tg67x ? 1 : ((dx ^ dy) < 0 ? 3 : 2));
            const bool inside = row_in && gx + j >= 0 && gx + j < w;  // outside the frame: magnitude 0
            words[j] = inside ? ((uint32_t)mg << 2) | (uint32_t)dir : 0u;
        }
        *reinterpret_cast<u32x4*>(mag + r * kCnMagS + c) = words;
    }
    __syncthreads();

    // 3. a pixel above `low` is a candidate iff it is a maximum along its direction: > the neighbour before it, >= the one
    //    after it along a row or a column, > both along a diagonal.  A thread takes four pixels side by side: ring
    //    columns c .. c + 5 of three ring rows, one 16-byte and one 8-byte read each.  The thresholds go onto the words'
    //    scale first: (m << 2) > (t << 2 | 3) iff m > t, and no magnitude reaches 2^22
    const uint32_t low_w = ((uint32_t)min(low, 1 << 22) << 2) | 3u, high_w = ((uint32_t)min(high, 1 << 22) << 2) | 3u;
    for (int i = tid; i < kCnTH * (kCnTW / 4); i += kCnThreads) {  // bound: kCnTH / 4 trips
        const int r = i / (kCnTW / 4), c = 4 * (i - r * (kCnTW / 4));
        uint32_t up[6], mid[6], dn[6];
        {
            const uint32_t* q = mag + r * kCnMagS + c;
            const u32x4 u4 = *reinterpret_cast<const u32x4*>(q), m4 = *reinterpret_cast<const u32x4*>(q + kCnMagS);
            const u32x4 d4 = *reinterpret_cast<const u32x4*>(q + 2 * kCnMagS);
            const u32x2 u2 = *reinterpret_cast<const u32x2*>(q + 4), m2 = *reinterpret_cast<const u32x2*>(q + kCnMagS + 4);
            const u32x2 d2 = *reinterpret_cast<const u32x2*>(q + 2 * kCnMagS + 4);
#pragma unroll
            for (int k = 0; k < 6; k++) {
                up[k] = k < 4 ? u4[k & 3] : u2[k & 1];
                mid[k] = k < 4 ? m4[k & 3] : m2[k & 1];
                dn[k] = k < 4 ? d4[k & 3] : d2[k & 1];
            }
        }
        // The words are compared as they are, the two direction bits of a neighbour included: with m the centre's
        // magnitude and n the neighbour's word, (m << 2) > n iff m > n's magnitude, and (m << 2 | 3) >= n iff m >= it
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t word = mid[j + 1], d = word & 3u, gt = word & ~3u, ge = word | 3u;
            // the four tests as a bit each, the direction picks one (a select chain over the twelve neighbours comes back
            // from the compiler as a table in scratch memory)
            const uint32_t tests = (gt > mid[j] && ge >= mid[j + 2] ? 1u : 0u) | (gt > up[j + 1] && ge >= dn[j + 1] ? 2u : 0u) |
                                   (gt > up[j] && gt > dn[j + 2] ? 4u : 0u) | (gt > up[j + 2] && gt > dn[j] ? 8u : 0u);
            const bool is_max = gt > low_w && ((tests >> d) & 1u);
            packed |= (is_max ? (gt > high_w ? 2u : 1u) : 0u) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(O + r * kCnTW + c) = packed;
    }
    __syncthreads();

    // 4. one 16-byte store per thread and row piece
    constexpr int kPieces = kCnTW / 16;
    for (int i = tid; i < kCnTH * kPieces; i += kCnThreads) {  // bound: kCnTH / 16 trips
        const int r = i / kPieces, p = i - r * kPieces;
        const int gy = y0 + r, gx = x0 + 16 * p;
        if (gy >= h || gx >= w)
            continue;
        store_chunk16<1>(fout + (size_t)gy * w, gx, w, *reinterpret_cast<const u32x4*>(O + r * kCnTW + 16 * p));
    }
}

// ---- hysteresis on the parent array of launch_ccl_unite ---------------------------------------------------------------------
constexpr uint32_t kMarked = 0x80000000u;  // bit 31 of a root's own entry: a label value is at most 2^31 - 1
constexpr int kHystThreads = 256;

// Two loads from candidate a (not 0) to its root: a's entry e is the root's value, or a's own entry if a is the root.  True
// iff the root has bit 31, else *root is its value.  kAtomic: the mark launch, where roots' own entries gain bit 31 meanwhile.
template <bool kAtomic>
__device__ __forceinline__ bool root_is_marked(const uint32_t* lab, uint32_t a, uint32_t* root)
{
    auto entry = [&](uint32_t v) { return kAtomic ? __hip_atomic_load(lab + (v - 1), MI355_RELAXED_AGENT) : lab[v - 1]; };
    const uint32_t e = entry(a);
    *root = e;
    return (e & kMarked) || (e != a && (entry(e) & kMarked));
}

// A thread owns one aligned chunk (mask_common.hpp) of a frame's npx bytes, in the mark kernel of the input and in the emit
// kernel of the output.  Frames are cut apart: a chunk that straddles two is visited once for each, with disjoint bytes.
__global__ __launch_bounds__(kHystThreads) void hyst_mark_kernel(const uint8_t* in, uint32_t* parent, uint32_t npx,
                                                                 uint32_t bpf, uint32_t high)
{
    const FrameBlock fb = frame_block(bpf, kHystThreads);
    const uint8_t* fin = in + (size_t)fb.frame * npx;
    uint32_t* lab = parent + (size_t)fb.frame * npx;
    const AlignedChunk<int64_t> c = aligned_chunk<int64_t>((int)(reinterpret_cast<uintptr_t>(fin) & 15u), fb.item, npx);
    if (c.b0 >= c.b1)
        return;
    const uint8_t* src = fin + c.first;
    const u32x4 v = c.whole() ? *reinterpret_cast<const u32x4*>(src) : load_chunk_bytes(src, c.b0, c.b1);
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (j < c.b0 || j >= c.b1 || chunk_byte(v, j) <= high)
            continue;
        const uint32_t a = __hip_atomic_load(lab + (c.first + j), MI355_RELAXED_AGENT) & ~kMarked;
        if (a == 0)
            continue;  // not a candidate (cannot happen while low <= high)
        uint32_t root;
        if (!root_is_marked<true>(lab, a, &root))
            __hip_atomic_fetch_or(lab + (root - 1), kMarked, MI355_RELAXED_AGENT);
    }
}

// `in` and `out` may be the same buffer: a thread reads exactly the bytes it writes.  Nothing writes `parent` here.
__global__ __launch_bounds__(kHystThreads) void hyst_emit_kernel(const uint8_t* in, uint8_t* out, const uint32_t* parent,
                                                                 uint32_t npx, uint32_t bpf, uint32_t low)
{
    const FrameBlock fb = frame_block(bpf, kHystThreads);
    const uint8_t* fin = in + (size_t)fb.frame * npx;
    uint8_t* fout = out + (size_t)fb.frame * npx;
    const uint32_t* lab = parent + (size_t)fb.frame * npx;
    const AlignedChunk<int64_t> c = aligned_chunk<int64_t>((int)(reinterpret_cast<uintptr_t>(fout) & 15u), fb.item, npx);
    if (c.b0 >= c.b1)
        return;
    const uint8_t* src = fin + c.first;
    const u32x4 v = c.whole() ? *reinterpret_cast<const u32x4_a1*>(src) : load_chunk_bytes(src, c.b0, c.b1);
    u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (j < c.b0 || j >= c.b1 || chunk_byte(v, j) <= low)
            continue;
        const uint32_t a = lab[c.first + j] & ~kMarked;
        if (a == 0)
            continue;  // not foreground for the union (cannot happen: it ran on these bytes with this `low`)
        uint32_t root;
        o[j >> 2] |= (root_is_marked<false>(lab, a, &root) ? 0xFFu : 0u) << (8 * (j & 3));
    }
    if (c.whole())
        *reinterpret_cast<u32x4*>(fout + c.first) = o;
    else
        store_chunk_bytes(fout + c.first, o, c.b0, c.b1);
}

}  // namespace

hipError_t launch_canny_nms(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int low,
                            int high, bool l2)
{
    if (!hist_frames_ok(w, h, nframes) || low < 0 || high < low)
        return hipErrorInvalidValue;
    const TileGrid g(w, h, nframes, kCnTW, kCnTH);
    if (l2)
        return launch_tiles(canny_nms_kernel<true>, g, kCnThreads, 0, kLdsDefault, stream, d_in, d_out, w, h, g.tiles_x,
                            g.tiles_y, g.n(), low, high);
    return launch_tiles(canny_nms_kernel<false>, g, kCnThreads, 0, kLdsDefault, stream, d_in, d_out, w, h, g.tiles_x,
                        g.tiles_y, g.n(), low, high);
}

hipError_t launch_hysteresis(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int32_t* d_parent, int w, int h,
                             int nframes, int low, int high, bool conn8)
{
    if (!hist_frames_ok(w, h, nframes) || low < 0 || high < low || high > 255)
        return hipErrorInvalidValue;
    const uint32_t npx = (uint32_t)w * (uint32_t)h;
    const FrameGrid g = frame_grid(aligned_chunks_of(npx), kHystThreads, nframes);  // a thread per aligned chunk
    if (!g.ok)
        return hipErrorInvalidValue;
    const hipError_t e = launch_ccl_unite(stream, d_in, d_parent, w, h, nframes, conn8, low);
    if (e != hipSuccess)
        return e;
    uint32_t* parent = reinterpret_cast<uint32_t*>(d_parent);
    if (high < 255)  // nothing exceeds 255: no pixel is strong, no root is marked
        hipLaunchKernelGGL(hyst_mark_kernel, dim3(g.blocks), dim3(kHystThreads), 0, stream, d_in, parent, npx, g.bpf,
                           (uint32_t)high);
    hipLaunchKernelGGL(hyst_emit_kernel, dim3(g.blocks), dim3(kHystThreads), 0, stream, d_in, d_out, parent, npx, g.bpf,
                       (uint32_t)low);
    return hipGetLastError();
}

}  // namespace mi355
