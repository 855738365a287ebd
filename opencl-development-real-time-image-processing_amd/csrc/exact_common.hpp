// exact_common.hpp — "exact by exception": what the fused pipeline (pipe_slide.hip) and the EXACT-mode Gaussian
// (gauss_exact.hip) share.  The CPU path's byte is trunc(S_cpu), S_cpu = its k*k-term float sum in its own order
// (src/GaussianBlur/GaussianBlur.cpp:243-256: ky outer, kx inner, separate multiply and add).  A separable fp32
// evaluation S differs from S_cpu by at most delta_bound(); wherever S is further than that from an integer,
// trunc(S) IS the CPU byte, and the few values within it are recomputed with exact_sum(), the CPU path's own chain.
// exact_blur_row() is that stage for one row of one channel, ExactTables / make_exact_tables() / exact_tables_ok() its
// host side; gray8.hip's LDS-tiled stage shares only delta_bound_k().
#pragma once
#include <cmath>
#include <utility>

#include "common.hpp"
#include "kernels.hpp"
#include "slide_common.hpp"

namespace mi355 {

// The CPU path's own sum for pixel J of every lane (GaussianBlur.cpp:243-256: ky outer, kx inner, float multiply
// then float add, starting from 0), from the ring of gray rows: the window's arrival rows sit in slots
// (u + 1 + t) % K, t = 0 .. K-1, and the rows are visited in IMAGE order, top to bottom — arrival order for a band
// walking down, the reverse for a band walking up (UP).  u is a constant after unrolling, so every register index
// is static.  Runs under a wave-uniform branch: EXEC is full, the DPP reads see every lane.
// PX = pixels per lane (4 or 8).
template <int K, int J, bool UP, int PX>
__device__ __forceinline__ float exact_sum(const float (&g)[K][PX], int u, const float* __restrict__ w2)
{
    constexpr int R = K / 2;
    float sum = 0.0f;
#pragma unroll
    for (int ky = 0; ky < K; ky++) {
        const float* r = g[(u + 1 + (UP ? K - 1 - ky : ky)) % K];
#pragma unroll
        for (int kx = 0; kx < K; kx++) {
            const int col = J - R + kx;
            const float val = (col < 0) ? dpp_left(r[PX + col]) : ((col > PX - 1) ? dpp_right(r[col - PX]) : r[col]);
            sum = sum + val * w2[ky * K + kx];  // -ffp-contract=off: v_mul_f32 then v_add_f32
        }
    }
    return sum;
}

// Constant windows.  Where the image is flat the separable value sits a few 1e-6 under an integer (the table sums to
// just under one), so EVERY pixel is flagged, and paying the 2 k^2-operation chain for all of them made flat content —
// letterbox bars, saturated regions, graphics, the blocks of a decoded JPEG sky — the worst case (256 x 4K frames of
// 64 x 64 flat patches: fused pipeline 2.6 TB/s against 4.9 on noise, EXACT Gaussian 1.4 against 4.8).  But the CPU path's
// chain over a window whose k^2 values all equal c is a function of c alone: flat_chain() tabulates it once per
// workgroup (256 floats in LDS), and flat_windows() replaces the chain by a table read for every flagged pixel whose
// window is constant: per row, column minima / maxima over the ring (2 (K - 1) operations per column, neighbour columns
// through DPP), per pixel a 2R + 1-column minimum / maximum and one comparison.  Called under a wave-uniform branch, and
// only when many lanes are flagged at once (dense_flags): noise-like frames never enter it.
template <int K>
__device__ __forceinline__ float flat_chain(float c, const float* __restrict__ w2)
{
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < K * K; i++)
        sum = sum + c * w2[i];  // -ffp-contract=off: the CPU path's multiply, then its add (GaussianBlur.cpp:249-252)
    return sum;
}

__device__ __forceinline__ bool dense_flags(uint64_t ballot)
{
    // wave-uniform.  On noise-like frames a flagged row has ONE flagged lane (a lane-row is flagged with probability
    // ~3e-3: three at once once in a thousand rows); a flat area a few lanes wide is worth the ~130-instruction search,
    // which costs about two chains.
    return __builtin_popcountll(ballot) >= 3;
}

// g = the ring exact_sum() reads (all K slots are the window's rows).  For every pixel J whose flag is up (t[J] <
// two_delta) and whose K x K window is constant: S[J] = flat[c], the flag goes down (t[J] = 1).
template <int K, int PX>
__device__ __forceinline__ void flat_windows(const float (&g)[K][PX], float (&S)[PX], float (&t)[PX], float two_delta,
                                             const float* flat)
{
    constexpr int R = K / 2;
    float mn[PX + 2 * R], mx[PX + 2 * R];
#pragma unroll
    for (int e = 0; e < PX; e++) {
        float a = g[0][e], b = g[0][e];
#pragma unroll
        for (int s = 1; s < K; s++) {
            a = fminf(a, g[s][e]);
            b = fmaxf(b, g[s][e]);
        }
        mn[R + e] = a;
        mx[R + e] = b;
    }
#pragma unroll
    for (int i = 0; i < R; i++) {
        mn[R - 1 - i] = dpp_left(mn[R + PX - 1 - i]);  // column -1 - i = the left lane's column PX - 1 - i
        mx[R - 1 - i] = dpp_left(mx[R + PX - 1 - i]);
        mn[R + PX + i] = dpp_right(mn[R + i]);          // column PX + i = the right lane's column i
        mx[R + PX + i] = dpp_right(mx[R + i]);
    }
#pragma unroll
    for (int J = 0; J < PX; J++) {
        float a = mn[J], b = mx[J];
#pragma unroll
        for (int c = 1; c <= 2 * R; c++) {
            a = fminf(a, mn[J + c]);
            b = fmaxf(b, mx[J + c]);
        }
        const bool is_flat = (a == b) && (t[J] < two_delta);
        if (__builtin_amdgcn_ballot_w64(is_flat) != 0) {
            const float val = flat[(uint32_t)a];  // a is a byte value held as a float
            S[J] = is_flat ? val : S[J];
            t[J] = is_flat ? 1.0f : t[J];
        }
    }
}

template <int N>
__device__ __forceinline__ float min_tree(const float* t)
{
    if constexpr (N == 1)
        return t[0];
    else
        return fminf(min_tree<N / 2>(t), min_tree<N / 2>(t + N / 2));
}

// Pixel position J of every lane: one wave-uniform branch, only positions some lane flagged pay the chain.
template <int K, int PX, int J>
__device__ __forceinline__ void exact_position(const float (&g)[K][PX], int u, bool up, const float* __restrict__ w2,
                                               float (&S)[PX], const float (&t)[PX], float two_delta)
{
    if (__builtin_amdgcn_ballot_w64(t[J] < two_delta) != 0) {
        if (up) {
            S[J] = exact_sum<K, J, true, PX>(g, u, w2);
            // keeps the two chains in arms of their own.  hipcc simplifies this helper before it inlines it, while g is
            // still a pointer: it then sinks both chains into one whose ring slots are a run-time select, and the
            // callers' rings leave the registers for scratch memory.
            asm volatile("; band walks upward");
        } else {
            S[J] = exact_sum<K, J, false, PX>(g, u, w2);
        }
    }
}

template <int K, int PX, int... J>
__device__ __forceinline__ void exact_positions(const float (&g)[K][PX], int u, bool up, const float* __restrict__ w2,
                                                float (&S)[PX], const float (&t)[PX], float two_delta,
                                                std::integer_sequence<int, J...>)
{
    (exact_position<K, PX, J>(g, u, up, w2, S, t, two_delta), ...);
}

// PX per-pixel values of a lane, local to exact_blur_row.  A struct and not a bare array: hipcc optimises the stage as a
// function of its own before it inlines it, and there AMDGPUPromoteAlloca turns a bare float[PX] into a <PX x float>
// vector, which stays one in the kernels (register tuples: 58 spilled VGPRs in the 8-pixel k = 5 pipeline).  A struct
// it leaves alone, and SROA splits it into scalars once the caller's row loop is unrolled.
template <int PX>
struct LaneRow {
    float a[PX];
};

// The blurred row whose window just completed, for one channel: S[0 .. PX-1] = the CPU path's sums of this lane's
// pixels (+ delta where no exception was taken: the same truncation), after CLAMP, ready for the caller's truncation.
//   g, u      : the ring; the window's arrival rows i-2R .. i sit in slots (u + 1 + t) % K, u a constant after unrolling
//   up        : the band walks upward (wave-uniform)
//   wv[d]     : the separable factor at distance d from the centre; delta = ExactTables::delta, two_delta = 2 delta
//   w2, flat  : the 2-D table and the workgroup's flat_chain() table in LDS
//   stores, keep_px : a lane that stores nothing takes no exceptions in the flat-window detour except for pixel keep_px,
//               the one a neighbour lane reads from it (-1: none)
//   FLAT      : compile the flat-window detour in
// Must be called with EXEC full (DPP reads, ballots).
template <int K, int PX, bool CLAMP, bool FLAT = true>
__device__ __forceinline__ void exact_blur_row(const float (&g)[K][PX], int u, bool up, const float (&wv)[K / 2 + 1],
                                               float delta, float two_delta, const float* __restrict__ w2,
                                               const float* flat, bool stores, int keep_px, float (&S)[PX])
{
    constexpr int R = K / 2;
    // vertical pass, symmetric pair form (the pair sums are exact integers <= 510; reads the same whichever way the band
    // walks)
    LaneRow<PX> v, t;  // t = fract(S'): exact; S' > 0
#pragma unroll
    for (int e = 0; e < PX; e++) {
        float acc = wv[0] * g[(u + 1 + R) % K][e];
#pragma unroll
        for (int d = 1; d <= R; d++)
            acc = __builtin_fmaf(wv[d], g[(u + 1 + R - d) % K][e] + g[(u + 1 + R + d) % K][e], acc);
        v.a[e] = acc;
    }
    // horizontal pass, same form; neighbour-lane taps through DPP.  S' = S + delta rides on the centre tap, so "S within
    // delta of an integer n" reads "fract(S') < 2 delta", one-sided, and floor(S') = floor(S) everywhere else
#pragma unroll
    for (int px = 0; px < PX; px++) {
        float acc = __builtin_fmaf(wv[0], v.a[px], delta);
#pragma unroll
        for (int d = 1; d <= R; d++) {
            const int a = px - d, b = px + d;
            const float va = (a < 0) ? dpp_left(v.a[PX + a]) : v.a[a];
            const float vb = (b > PX - 1) ? dpp_right(v.a[b - PX]) : v.a[b];
            acc = __builtin_fmaf(wv[d], va + vb, acc);
        }
        S[px] = acc;
        t.a[px] = __builtin_amdgcn_fractf(acc);
    }
    const uint64_t flagged = __builtin_amdgcn_ballot_w64(min_tree<PX>(t.a) < two_delta);
    if (__builtin_expect(flagged != 0, 0)) {
        if (FLAT && dense_flags(flagged)) {  // flat content: constant windows take a table read, not the chain
            if (!stores) {
#pragma unroll
                for (int J = 0; J < PX; J++)
                    if (J != keep_px)
                        t.a[J] = 1.0f;
            }
            flat_windows<K, PX>(g, S, t.a, two_delta, flat);
        }
        exact_positions<K, PX>(g, u, up, w2, S, t.a, two_delta, std::make_integer_sequence<int, PX>{});
    }
    if constexpr (CLAMP) {
#pragma unroll
        for (int px = 0; px < PX; px++)
            S[px] = fminf(S[px], 255.0f);
    }
}

// u(x) = half an ulp of a float of magnitude <= x
inline double half_ulp(double x)
{
    if (!(x > 0.0))
        return 0.0;
    int e = 0;
    std::frexp(x, &e);  // x = m * 2^e, m in [0.5, 1)  ->  ulp = 2^(e - 24)
    return std::ldexp(1.0, e - 25);
}

// |S - S_cpu| <= delta for every window of bytes, where S is the kernel's separable pair-form evaluation with w1 and
// S_cpu the CPU path's k*k-term float sum with w2.  Everything is non-negative (checked by the caller), so partial
// sums never exceed the final ones.
inline double delta_bound_k(int K, const float* w1, const float* w2)
{
    const int R = K / 2;
    double sum1 = 0.0, mismatch = 0.0;
    for (int i = 0; i < K; i++)
        sum1 += (double)w1[i];
    for (int i = 0; i < K; i++)
        for (int j = 0; j < K; j++)
            mismatch += std::fabs((double)w1[i] * (double)w1[j] - (double)w2[i * K + j]);
    // CPU path (GaussianBlur.cpp:243-256): term i (row-major, ky outer / kx inner) is a product of a byte and w2[i],
    // rounded (error <= half an ulp of 255 * w2[i]), added to the running sum, rounded again — and the running sum
    // after term i cannot exceed 255 * (w2[0] + ... + w2[i]) plus the error made so far (every term is non-negative),
    // so the early additions happen in low binades.  (Round 2, second half: the bound used to charge every product
    // with the largest weight's ulp and every addition with the final sum's: 2.1e-4 at k = 5, now 1.4e-4.)
    double e_cpu = 0.0, cum = 0.0;
    for (int i = 0; i < K * K; i++) {
        cum += (double)w2[i];
        e_cpu += half_ulp(255.0 * (double)w2[i]) + half_ulp(255.0 * cum + 1e-3);
    }
    // kernel, vertical: acc = w(0) g_c, then acc = fma(w(d), g_{c-d} + g_{c+d}, acc), d = 1 .. R (the integer pair sums
    // are exact): R + 1 roundings, the one after distance d of a value <= 255 * c_d, c_d = w(0) + 2 (w(1) + ... + w(d))
    const double tv = 255.0 * sum1;
    double c_d = (double)w1[R];
    double e_v = half_ulp(255.0 * c_d);
    for (int d = 1; d <= R; d++) {
        c_d += 2.0 * (double)w1[R - d];
        e_v += half_ulp(255.0 * c_d + 1e-3);
    }
    // kernel, horizontal: acc = fma(w(0), v_c, delta), then acc = fma(w(d), v_{c-d} + v_{c+d}, acc): the R pair sums are
    // rounded float additions of values <= tv (weighted by w(d) afterwards), the R + 1 fused operations round values
    // <= tv * c_d + delta (delta < 0.01, checked by the callers); the vertical error arrives through weights summing to sum1
    double e_pairs = 0.0;
    for (int d = 1; d <= R; d++)
        e_pairs += (double)w1[R - d] * half_ulp(2.0 * tv + 1e-3);
    c_d = (double)w1[R];
    double e_chain = half_ulp(tv * c_d + 0.011);
    for (int d = 1; d <= R; d++) {
        c_d += 2.0 * (double)w1[R - d];
        e_chain += half_ulp(tv * c_d + 0.011);
    }
    const double e_h = e_v * sum1 + e_pairs + e_chain;
    // every term above is a worst case already; the margin only covers the double arithmetic of this function
    return 1.02 * (e_cpu + e_h + 255.0 * mismatch) + 1e-7;
}

// The kernels' tables: host values, passed by value as a kernel argument.
template <int K>
struct ExactTables {
    float w1[K];      // separable factor (symmetric: w1[j] == w1[K-1-j])
    float w2[K * K];  // the reference's 2-D table, row-major [ky][kx] — read only by the exact chains
    float delta;      // |S - S_cpu| bound
};

// *wsum = the factor's sum in double: 255 wsum^2 bounds S, which decides the callers' CLAMP instantiation
template <int K>
inline ExactTables<K> make_exact_tables(const GaussCoef& coef, double* wsum)
{
    ExactTables<K> tab;
    *wsum = 0.0;
    for (int j = 0; j < K; j++) {
        tab.w1[j] = coef.h_w1d[j];
        *wsum += (double)coef.h_w1d[j];
    }
    for (int j = 0; j < K * K; j++)
        tab.w2[j] = coef.h_w2d[j];
    tab.delta = (float)delta_bound_k(K, tab.w1, tab.w2);
    return tab;
}

// The exact-by-exception kernels need a separable table whose factor is symmetric (the pair form) and a useful error
// bound; anything else is only reachable through mi355_ctx_set_gauss_weights.  coef.k is odd and at most 7 here.
inline bool exact_tables_ok(const GaussCoef& coef)
{
    const int k = coef.k;
    if (!coef.separable || !coef.h_w2d)
        return false;
    for (int j = 0; j < k / 2; j++)
        if (coef.h_w1d[j] != coef.h_w1d[k - 1 - j])
            return false;
    return delta_bound_k(k, coef.h_w1d, coef.h_w2d) < 0.01;
}

}  // namespace mi355
