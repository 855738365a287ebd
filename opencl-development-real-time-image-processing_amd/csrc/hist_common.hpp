// hist_common.hpp — what the histogram kernels share (hist.hip: whole frames, clahe.hip: tiles of a frame): where the
// 16-byte body of a byte range starts, and counting bytes into a wave's private 256-bin LDS histogram with equal bytes
// merged first.  Flat content would put up to 64 lanes of one ds_add on one address (64-way serialised): lanes whose 16
// bytes all equal the wave's first such value add one count for all of them, other lanes with 16 equal bytes add 16
// once, dwords of 4 equal bytes add 4 once, and only the rest add byte by byte.
#pragma once
#include "common.hpp"

namespace mi355 {

// where the 16-byte body of a frame starts, relative to the frame, for a frame at address a of npx bytes
__device__ __forceinline__ uint32_t head_bytes(uintptr_t a, uint32_t npx)
{
    const uint32_t hb = (uint32_t)((16u - (a & 15u)) & 15u);
    return hb < npx ? hb : npx;
}

__device__ __forceinline__ void lds_add(uint32_t* hw, uint32_t bin, uint32_t n)
{
    __hip_atomic_fetch_add(hw + bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

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

}  // namespace mi355
