// mask_common.hpp — what the gray8 mask and feature kernels share (hist.hip and clahe.hip through hist_common.hpp,
// ccl.hip, canny.hip's hysteresis, hough.hip).  Frames are flat ranges of w h < 2^31 bytes at any
// address; kernel boundaries are the only ordering between workgroups.
//   host    hist_frames_ok, grid_fits; frame_grid: blocks per frame and in all, refused where the grid does not fit.
//   device  frame_block: block -> (frame, block of the frame, the thread's item); wave_scan_inclusive / block_offsets:
//           prefix sums over lanes and waves; lanes_below / wave_add_once: compaction by ballot, one add per wave;
//           aligned_chunk, chunk_byte, load_ / store_chunk_bytes: the 16-byte aligned chunks of bytes at any address.
#pragma once
#include "common.hpp"

namespace mi355 {

#define MI355_RELAXED_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define MI355_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// host: frames of w x h < 2^31 pixels (OpenCV counts pixels in an int), and a block count that fits a grid
inline bool hist_frames_ok(int w, int h, int nframes)
{
    return w > 0 && h > 0 && nframes > 0 && (uint64_t)w * (uint64_t)h < (1ull << 31);
}
inline bool grid_fits(uint64_t blocks) { return blocks <= 0x7FFFFFFFull; }

// host: `items` per frame, `per_block` of them to a block: bpf blocks per frame, bpf nframes in all; !ok: too many
struct FrameGrid {
    uint32_t bpf = 0, blocks = 0;
    bool ok = false;
};
inline FrameGrid frame_grid(uint64_t items, uint64_t per_block, int nframes)
{
    const uint64_t bpf = (items + per_block - 1) / per_block, blocks = bpf * (uint64_t)nframes;
    return grid_fits(bpf) && grid_fits(blocks) ? FrameGrid{(uint32_t)bpf, (uint32_t)blocks, true} : FrameGrid{};
}

// frame_grid's other half: the block's frame, its number in the frame, and item = block * per_block + threadIdx.x (the
// thread's item where a thread owns one; a kernel whose block walks its per_block items itself takes frame and block only)
struct FrameBlock {
    uint32_t frame, block, item;
};
__device__ __forceinline__ FrameBlock frame_block(uint32_t bpf, uint32_t per_block)
{
    const uint32_t f = blockIdx.x / bpf, b = blockIdx.x - f * bpf;
    return {f, b, b * per_block + threadIdx.x};
}

__device__ __forceinline__ void lds_add(uint32_t* hw, uint32_t bin, uint32_t n)
{
    __hip_atomic_fetch_add(hw + bin, n, MI355_RELAXED_WG);
}

// the sum of v over lanes 0 .. lane of the wave.  bound: 6 doublings
__device__ __forceinline__ uint32_t wave_scan_inclusive(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d)
            v += o;
    }
    return v;
}

// From every wave's total (valid in its last lane, as wave_scan_inclusive leaves it): the totals of the waves below the
// caller's and of the block.  s: kWaves words of the caller's LDS.  One __syncthreads() inside; the caller must
// synchronise again before s is written a second time (other waves may still be reading it).
struct BlockOffsets {
    uint32_t before, total;
};
template <int kWaves>
__device__ __forceinline__ BlockOffsets block_offsets(uint32_t wave_total, uint32_t* s, int lane, int wave)
{
    if (lane == kWave - 1)
        s[wave] = wave_total;
    __syncthreads();
    BlockOffsets o = {0, 0};
#pragma unroll
    for (int k = 0; k < kWaves; k++) {
        o.before += k < wave ? s[k] : 0u;
        o.total += s[k];
    }
    return o;
}

// the set lanes of the ballot m below `lane`: a set lane's rank among them
__device__ __forceinline__ uint32_t lanes_below(uint64_t m, int lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1)); }
// The set lanes of m (not empty; the whole wave calls this) take popcount(m) consecutive places from *counter with one
// add by the first of them; returns the first place, in every lane.  A lane's own: that + lanes_below(m, lane)
__device__ __forceinline__ uint32_t wave_add_once(uint32_t* counter, uint64_t m, int lane)
{
    const int leader = __ffsll((unsigned long long)m) - 1;
    const uint32_t base = lane == leader ? __hip_atomic_fetch_add(counter, (uint32_t)__popcll(m), MI355_RELAXED_AGENT) : 0u;
    return (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
}

// n bytes start `mis` (0 .. 15) bytes past a 16-byte boundary.  Aligned chunk s is their bytes [first, first + 16), first =
// 16 s - mis, of which [first + b0, first + b1) exist (b0 >= b1: none); aligned_chunks_of(n) chunks can touch the n bytes.
template <class T>
struct AlignedChunk {
    T first;
    int b0, b1;
    constexpr bool whole() const { return b1 - b0 == 16; }
};
template <class T>
constexpr AlignedChunk<T> aligned_chunk(int mis, T s, T n)
{
    const T first = 16 * s - mis, last = n - first;  // last: bytes from `first` to the end
    return {first, first < 0 ? mis : 0, last < 16 ? (int)last : 16};
}
template <class T>
constexpr T aligned_chunks_of(T n) { return (n + 15) / 16 + 1; }

// every mis and every n up to three chunks: the pieces are disjoint, in order, and cover exactly [0, n)
template <class T>
constexpr bool aligned_chunks_cover()
{
    for (int mis = 0; mis < 16; mis++)
        for (T n = 0; n <= 48; n++) {
            T at = 0;  // the first byte no piece has taken yet
            for (T s = 0; s < aligned_chunks_of(n); s++) {
                const AlignedChunk<T> c = aligned_chunk<T>(mis, s, n);
                if (c.b0 < c.b1 && (c.b0 < 0 || c.b1 > 16 || c.first + c.b0 != at))
                    return false;
                at = c.b0 < c.b1 ? c.first + c.b1 : at;
            }
            if (at != n)
                return false;
        }
    return true;
}
static_assert(aligned_chunks_cover<int>() && aligned_chunks_cover<int64_t>(), "the aligned chunks cut n bytes exactly");

__device__ __forceinline__ uint32_t chunk_byte(const u32x4& v, int j) { return (v[j >> 2] >> (8 * (j & 3))) & 0xFFu; }
// bytes b0 .. b1 - 1 of the chunk at p, the others zero.  bound: fewer than 16 bytes (a whole chunk is one vector load)
__device__ __forceinline__ u32x4 load_chunk_bytes(const uint8_t* p, int b0, int b1)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    for (int j = b0; j < b1; j++)
        v[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    return v;
}

// bytes b0 .. b1 - 1 of v to the chunk at p.  bound: fewer than 16 bytes
__device__ __forceinline__ void store_chunk_bytes(uint8_t* p, const u32x4& v, int b0, int b1)
{
    for (int j = b0; j < b1; j++)
        p[j] = (uint8_t)chunk_byte(v, j);
}

}  // namespace mi355
