// gauss_exact.hip — the EXACT-mode Gaussian (bit-identical to the reference CPU path,
// src/GaussianBlur/GaussianBlur.cpp:234-261) at sliding-window speed, k in {3, 5, 7}.  gfx950 only.
// (k = 7: four channels x 49-tap chains x two walking directions per row is more code than LLVM's default budget for
// `#pragma unroll` — the loop stayed rolled and the ring went to scratch memory; the Makefile raises the budget for
// this file.)
//
// MI355_GAUSS_EXACT used to mean the LDS-tiled kernel evaluating the CPU path's own k*k-term chain for every value
// (2 k^2 operations per channel: 1.0 TB/s at k = 5 on 64 x 4K frames; this kernel: 4.7 TB/s, same box).  This kernel is "exact by exception" (exact_common.hpp, the
// idea of pipe_slide.hip applied to four channels): a separable fp32 evaluation S (2k operations) is within
// delta_bound() of the CPU sum, so trunc(S) is the CPU byte unless S sits within that bound of an integer; only
// those values (7.5e-4 of them at k = 5 on noise-like frames) are recomputed with the CPU path's chain, from the ring
// of input rows the wave keeps in registers anyway.  Flat regions take the chain for every value: still exact,
// slower there.
//
// Structure: one wave per (frame, band, strip of <= 62 lanes + 1 halo lane per side), a lane owns 4 pixels; the ring
// holds the last K rows as floats, per channel; vertical sums in the symmetric pair form (reads the same whichever way
// the band walks: odd bands walk upward, shared boundary rows hit L2), horizontal taps through DPP.
// Frames whose alpha is constant (255 everywhere: every frame after cvtColor(BGR2RGBA); round 3: any value A, named by the
// band's first pixel) run a 3-channel pass; the alpha of an all-A window is what the CPU chain gives for it (flat[A], the
// table the constant-window path uses anyway).  The pass tests every loaded row (halo lanes included) and at the first
// other alpha abandons — the rows stored so far are correct — and the band is redone with four channels, as in
// gauss_slide.hip.  (A constant alpha channel is flat content: in the 4-channel walk every one of its values took the
// constant-window search — alpha = 128 everywhere: 3.41 TB/s, now 4.73, the opaque rate.)
#include <type_traits>

#include "common.hpp"
#include "exact_common.hpp"
#include "kernels.hpp"
#include "slide_common.hpp"

namespace mi355 {

namespace {

template <int R, bool CLAMP>
__global__ __launch_bounds__(kSlideWavesPerBlock * 64) void gauss_exact_kernel(
    const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int w, int h, int nstrips, int lanes_out, BandPlan plan,
    ExactTables<2 * R + 1> tab, uint32_t alpha255)
{
    constexpr int K = 2 * R + 1;
    __shared__ float flat[256];  // flat[c] = the CPU path's chain over a window that is c everywhere (exact_common.hpp)
    flat[threadIdx.x] = flat_chain<K>((float)threadIdx.x, tab.w2);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    SlideItem it;
    if (!slide_item(plan, nstrips, h, &it))
        return;  // after the only barrier
    const bool up = (it.band & 1) != 0;  // wave-uniform
    const SlideGeom G = slide_geom<4>(it.strip, lanes_out, lane, w, 16u, 16u);  // w % 4 == 0 (gauss_exact_supported)
    // output rows y0 .. y0+nout-1 need input rows y0-R .. y0+nout-1+R, clamp-to-edge (GaussianBlur.cpp:241)
    const BandWalk W = band_walk(up, it.y0, it.nout, R, h);
    const int nin = W.nin, nout = it.nout;

    const size_t row_bytes = (size_t)w * 4;
    const auto fin = uniform_ptr(in + it.frame * row_bytes * h);
    const auto fout = uniform_ptr(out + it.frame * row_bytes * h);
    uint32_t in_off = G.in_off, out_off = G.out_off;

    float wv[R + 1];  // wv[d] = weight at distance d from the centre
#pragma unroll
    for (int d = 0; d <= R; d++)
        wv[d] = tab.w1[R - d];
    const float delta = tab.delta, two_delta = 2.0f * tab.delta;

    auto load_row = [&](int i) -> u32x4 {
        const auto rowp = fin + (size_t)in_row<kBorderClamp>(W, i) * row_bytes;
        lane_offset_here(in_off);
        return gload<u32x4>(rowp + in_off);
    };

    // One walk over the band with NCH channels.  Returns false when a 3-channel walk met a non-opaque pixel.
    auto walk = [&](auto nch_tag) -> bool {
        constexpr int NCH = decltype(nch_tag)::value;
        constexpr int PF = 3;
        u32x4 q[K];
#pragma unroll
        for (int u = 0; u < PF; u++)
            q[u] = load_row(u);
        uint32_t n_alpha = 0u, alpha_hi = alpha255;  // 3-channel walk: (A ^ 0xFF) << 24 and the byte of an all-A window
        float g[NCH][K][4];  // ring of the last K rows, per channel; slot = arrival index % K
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int s = 0; s < K; s++)
#pragma unroll
                for (int e = 0; e < 4; e++)
                    g[c][s][e] = 0.0f;

        for (int base = 0; base < nin; base += K) {
#pragma unroll
            for (int u = 0; u < K; u++) {
                const int i = base + u;
                u32x4 p = q[u];
                q[(u + PF) % K] = load_row(i + PF);
                if constexpr (NCH == 3) {
                    // The band's first pixel names the alpha value A the 3-channel walk bets on (255 for every frame that
                    // went through cvtColor; round 3: any constant).  Every loaded row, all 64 lanes: the first pixel with
                    // another alpha ends the walk BEFORE the first output row whose window contains it is computed.  The
                    // alpha of an all-A window is what the CPU chain gives for it: flat[A], clamped and truncated.
                    if (i == 0) {  // wave-uniform
                        const uint32_t a0 = ((uint32_t)__builtin_amdgcn_readfirstlane((int)p.x) >> 24) & 0xFFu;
                        n_alpha = (a0 ^ 0xFFu) << 24;
                        float ca = flat[a0];
                        ca = ca < 0.0f ? 0.0f : (ca > 255.0f ? 255.0f : ca);
                        alpha_hi = __builtin_amdgcn_readfirstlane((uint32_t)ca << 24);
                    }
                    const uint32_t a = ((p.x ^ n_alpha) & (p.y ^ n_alpha)) & ((p.z ^ n_alpha) & (p.w ^ n_alpha));
                    if (__builtin_amdgcn_ballot_w64(a < 0xFF000000u) != 0 && i < nin)
                        return false;
                }
                if (G.edge_strip)
                    edge_clamp_cols(p, G.left_of_image, G.right_of_image);
#pragma unroll
                for (int c = 0; c < NCH; c++)
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        g[c][u][e] = (float)((p[e] >> (8 * c)) & 0xFFu);  // v_cvt_f32_ubyteN
                if (i >= 2 * R) {
                    uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int c = 0; c < NCH; c++) {
                        // the row whose window (arrival rows i-2R .. i) just completed.  Halo and idle lanes store
                        // nothing: no exceptions on their behalf (keep_px = -1).  The constant-window detour is left out
                        // at k = 7: with the ring of 4 x 7 rows its extra live values push the kernel from 198 VGPRs into
                        // scratch memory.
                        float S[4];
                        exact_blur_row<K, 4, CLAMP, (R <= 2)>(g[c], u, up, wv, delta, two_delta, tab.w2, flat, G.stores,
                                                              -1, S);
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            px[e] |= (uint32_t)S[e] << (8 * c);  // uchar(clamp(sum, 0, 255)): truncation
                    }
                    if constexpr (NCH == 3) {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            px[e] |= alpha_hi;
                    }
                    const int cidx = i - 2 * R;  // completed output row in arrival order
                    if (G.stores && cidx < nout) {
                        const auto rowp = fout + (size_t)out_row(W, cidx) * row_bytes;
                        lane_offset_here(out_off);
                        gstore_nt<u32x4>(rowp + out_off, u32x4{px[0], px[1], px[2], px[3]});
                    }
                }
            }
        }
        return true;
    };
    if (!walk(std::integral_constant<int, 3>{}))
        walk(std::integral_constant<int, 4>{});
}

template <int R>
hipError_t launch_r(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                    const GaussCoef& coef)
{
    constexpr int K = 2 * R + 1;
    const StripPlan sp = make_strip_plan(w);
    BandPlan plan;
    constexpr int kRows = (R == 1) ? 16 : (R == 2 ? 24 : 40);
    constexpr int kWavesPerSimd = (R == 1) ? 5 : (R == 2 ? 3 : 2);
    if (!make_band_plan(h, sp.nstrips, nframes, kWavesPerSimd, kRows, kRows, kRows, 0.0, kRows / 2, &plan))
        return hipErrorInvalidValue;
    double wsum;
    const ExactTables<K> tab = make_exact_tables<K>(coef, &wsum);
    // the CPU path's value for an all-255 window: its own chain (this translation unit is built with
    // -ffp-contract=off: one float multiply and one float add per tap), clamped and truncated
    float chain = 0.0f;
    for (int j = 0; j < K * K; j++)
        chain += 255.0f * coef.h_w2d[j];
    chain = chain < 0.0f ? 0.0f : (chain > 255.0f ? 255.0f : chain);
    const uint32_t alpha255 = (uint32_t)chain << 24;  // already shifted to bits 31:24
    // (the 0.01 on top of the shared test is this launcher's own, of unrecorded origin: kept as it is)
    return dispatch_bool(gauss_upper_clamp(wsum, 0.01), [&](auto CL) {
        return launch_slide(gauss_exact_kernel<R, CL.value>, plan, stream, d_in, d_out, w, h, sp.nstrips, sp.lanes_out,
                            plan, tab, alpha255);
    });
}

}  // namespace

// k in {3, 5, 7}, width a multiple of 4, 16-byte aligned buffers, a separable table with a symmetric factor and a
// useful error bound (everything mi355_gauss_weights generates qualifies)
bool gauss_exact_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, const GaussCoef& coef)
{
    (void)h;
    const int k = coef.k;
    if (k != 3 && k != 5 && k != 7)
        return false;
    if (rows_ragged(w, d_in, 16, d_out, 16))
        return false;
    return exact_tables_ok(coef);
}

hipError_t launch_gauss_exact(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                              const GaussCoef& coef)
{
    return dispatch_int(coef.k, std::integer_sequence<int, 3, 5, 7>{},
                        [&](auto K) { return launch_r<K.value / 2>(stream, d_in, d_out, w, h, nframes, coef); });
}

}  // namespace mi355
