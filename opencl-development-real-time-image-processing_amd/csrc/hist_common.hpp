// hist_common.hpp — what the histogram kernels share (hist.hip: whole frames, clahe.hip: tiles of a frame; DESIGN.md
// section 6d).  Both run three launches on one stream, the kernel boundaries being the only cross-workgroup
// synchronisation: count into a zeroed global histogram, make a 256-byte table of every 256-bin row, apply the tables.
//   counting     into a wave's private 256-bin LDS histogram, equal bytes merged first.  Flat content would put up to 64
//                lanes of one ds_add on one address (64-way serialised): lanes whose 16 bytes all equal the wave's first
//                such value add one count for all of them, other lanes with 16 equal bytes add 16 once, dwords of 4
//                equal bytes add 4 once, and only the rest add byte by byte;
//   block frame  block_hists_begin / _flush around the counting loop: the block sums its waves' histograms and adds
//                every nonzero bin once into a global row (agent-scope integer atomics: exact in any arrival order);
//   byte range   16-byte vectors from the first 16-byte-aligned byte of one side (the input when counting, the output
//                when applying; the other side at whatever alignment it then has); the head and the tail, < 16 bytes
//                each, go byte by byte in threads 0..15 and 16..31 of one block;
//   table scan   lane l of one wave holds bins 4 l .. 4 l + 3: an integer prefix sum across lanes (exact in any order),
//                then one fp32 multiply and rint per bin (-ffp-contract=off: nothing fuses).
#pragma once
#include "mask_common.hpp"

namespace mi355 {

constexpr int kHistThreads = 256;  // of every block that counts or applies
constexpr int kHistWaves = kHistThreads / kWave;
constexpr int kHistVec = 16;  // 16-byte vectors per thread of a counting block
constexpr int kApplyVec = 8;  // per thread of an applying block
constexpr uint32_t kHistBlockBytes = kHistThreads * kHistVec * 16;    // 64 KiB per block, 256 atomics per flush
constexpr uint32_t kApplyBlockBytes = kHistThreads * kApplyVec * 16;  // 32 KiB per block

__device__ __forceinline__ void count_dword(uint32_t* hw, uint32_t d)
{
    const uint32_t b = d & 0xFFu;
    if (d == b * 0x01010101u) {
        lds_add(hw, b, 4);
    } else {
        lds_add(hw, b, 1);
        lds_add(hw, (d >> 8) & 0xFFu, 1);
        lds_add(hw, (d >> 16) & 0xFFu, 1);
        lds_add(hw, d >> 24, 1);
    }
}

// count the 16 bytes of v (valid lanes only) into the wave's LDS histogram hw
__device__ __forceinline__ void count_vec(uint32_t* hw, const u32x4& v, bool valid)
{
    const uint32_t b = v.x & 0xFFu, rep = b * 0x01010101u;
    const bool uni = valid && v.x == rep && v.y == rep && v.z == rep && v.w == rep;
    const uint64_t um = __ballot(uni);
    if (um) {
        // the lanes whose 16 bytes all hold the first uniform lane's value: one add for all of them
        const int leader = __ffsll((unsigned long long)um) - 1;
        const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)b, leader);
        const uint64_t m = __ballot(uni && b == lb);
        if ((int)__lane_id() == leader)
            lds_add(hw, lb, 16u * (uint32_t)__popcll(m));
        if ((m >> __lane_id()) & 1u)
            return;
    }
    if (!valid)
        return;
    if (uni) {
        lds_add(hw, b, 16);
        return;
    }
    count_dword(hw, v.x);
    count_dword(hw, v.y);
    count_dword(hw, v.z);
    count_dword(hw, v.w);
}

// zeroes the block's kHistWaves x 256 LDS bins sh; returns the calling wave's 256
__device__ __forceinline__ uint32_t* block_hists_begin(uint32_t* sh)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < kHistWaves * 256; i += kHistThreads)
        sh[i] = 0;
    __syncthreads();
    return sh + (tid / kWave) * 256;
}

// after the block's counting: thread t adds bin t of the waves' sum into the global histogram `row`, if it is not zero
__device__ __forceinline__ void block_hists_flush(const uint32_t* sh, uint32_t* row)
{
    const int tid = threadIdx.x;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int wv = 0; wv < kHistWaves; wv++)
        s += sh[wv * 256 + tid];
    if (s)
        __hip_atomic_fetch_add(row + tid, s, MI355_RELAXED_AGENT);
}

// nbytes bytes: head bytes [0, head), nvec vectors that are 16-byte aligned at `aligned_side`, tail bytes from body_end
struct ByteRange {
    uint32_t head, nvec, body_end;
};
__device__ __forceinline__ ByteRange byte_range(const void* aligned_side, uint32_t nbytes)
{
    const uint32_t hb = (uint32_t)((16u - (reinterpret_cast<uintptr_t>(aligned_side) & 15u)) & 15u);
    const uint32_t head = hb < nbytes ? hb : nbytes;  // a range shorter than its head is all head
    const uint32_t nvec = (nbytes - head) / 16;
    return {head, nvec, head + 16 * nvec};
}

// f(i) in the thread that owns byte i of the range's head (threads 0..15) or tail (threads 16..31), if tid owns one.
// A callback, not an index to test: the kernels then compile to the two-branch code they had with the walk written out.
template <class F>
__device__ __forceinline__ void for_edge_byte(const ByteRange& r, uint32_t nbytes, int tid, F f)
{
    if ((uint32_t)tid < r.head)
        f((uint32_t)tid);
    else if (tid >= 16 && tid < 32 && r.body_end + (uint32_t)(tid - 16) < nbytes)
        f(r.body_end + (uint32_t)(tid - 16));
}

// the sum of every bin of the wave below lane's four, hv: the inclusive scan of the per-lane sums, less the lane's own
__device__ __forceinline__ uint32_t bins_below(const u32x4& hv, int lane)
{
    const uint32_t lsum = hv.x + hv.y + hv.z + hv.w;
    return wave_scan_inclusive(lsum, lane) - lsum;
}

// a table entry from a cumulative count: (float)count * scale, cvRound, saturated to a byte
__device__ __forceinline__ uint32_t table_byte(uint32_t count, float scale)
{
    const float v = __builtin_rintf((float)(int)count * scale);
    return v >= 255.0f ? 255u : (uint32_t)v;
}

}  // namespace mi355
