// box_common.hpp — the division of the box mean (include/mi355_imgfilter.h, "Box mean"), for the kernel and for the CPU.
//
// out = floor((2 s + d) / (2 d)), d = k * k odd, 0 <= s <= 255 d: the integer nearest to s / d (no tie: d is odd).
// Computed as round-to-nearest of the fp32 product (float)s * inv with inv = box_inv(k) = fl(1.0f / d) from the host:
//   * s <= 255 * 3969 = 1,012,095 < 2^24, so (float)s is exact;
//   * inv and the product each carry a relative error of at most 2^-24, so the product is within 255 * 2^-23 = 3.1e-5 of
//     s / d;
//   * s / d = n + j / d is at least 1 / (2 d) >= 1.26e-4 (d <= 3969) away from every half-integer n + 1/2.
// So the rounded product is the nearest integer to s / d whichever way a tie of the PRODUCT would go.  One IEEE fp32
// multiply (the library is built with -ffp-contract=off) and one round-to-nearest convert; no reciprocal instruction,
// no approximate operation.  tests/test_box_cpu.py compiles this header for the host and checks box_mean against the
// integer formula for every odd k in 3..63 and every s in 0..255 k^2.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else  // a plain C++ compiler: the CPU's check of box_mean
#define __host__
#define __device__
#endif
#include <stdint.h>

namespace mi355 {

constexpr int kBoxMaxK = 63;  // MI355_MAX_BOX_K

__host__ __device__ inline float box_inv(int k) { return 1.0f / (float)(k * k); }

__host__ __device__ inline uint32_t box_mean(uint32_t sum, float inv)
{
    return (uint32_t)__builtin_rintf((float)sum * inv);  // round to nearest (even on a tie, which cannot decide here)
}

#if defined(__HIPCC__)
// box_mean(sum, inv) placed into byte `byte` of `old`: v_cvt_pk_u8_f32 rounds to nearest even and saturates, i.e. the
// same integer (the quotient never exceeds 255)
__device__ __forceinline__ uint32_t box_mean_pack(uint32_t sum, float inv, uint32_t byte, uint32_t old)
{
    return __builtin_amdgcn_cvt_pk_u8_f32((float)sum * inv, byte, old);
}
#endif

}  // namespace mi355
