// pipe_slide.hip — fused gray -> Gaussian -> Sobel on RGBA8 frames, register-resident sliding window,
// k in {3,5,7}, width >= 4, height >= 2 (RAGGED instantiation when width % 4 != 0 or the pointers are not
// 16-byte aligned); 4 pixels per lane, or 8 (PX) for k in {3,5}, width % 8 == 0 and aligned buffers.  gfx950 only.
// BIT-EXACT with the reference's CPU chain in both Gaussian modes.
//
// Definition (SURVEY.md §8a "a-pipe", oracle_pipeline_rgba): exactly the composition of the three API calls
//   g = luma(R,G,B)                                   src/Grayscale/grayscale.cpp:237
//   b = trunc(clamp(Gaussian_k(g)))  clamp-to-edge     src/GaussianBlur/GaussianBlur.cpp:234-261 on (g,g,g,255)
//   l = luma(b,b,b)                  RE-APPLIED        (l != b for 65 byte values)
//   out = Sobel(l)                   reflect-101       src/EdgeDetection/EdgeDetection.cpp:219-240
//
// The Gaussian stage is "exact by exception" (the same idea as the luminance, common.hpp): the CPU path's value
// is trunc(S_cpu), S_cpu = the k*k-term float sum in its own order (ky outer, kx inner, separate multiply and
// add).  A separable fp32 evaluation S (2k multiply-adds instead of 2k*k operations) differs from S_cpu by at
// most delta, a bound the host derives rigorously from the two tables (make_exact_tables: rounding errors of both
// evaluations + the mismatch of w1 (x) w1 against the 2-D table; ~3e-4 at k = 5).  So wherever S is further
// than delta from an integer, trunc(S) IS the CPU path's byte; the few pixels within delta (6e-4 of them on
// noise-like images) are recomputed with the CPU path's own operation sequence from the ring of gray rows the
// wave holds anyway, constant windows by a table read (exact_blur_row, exact_common.hpp).
//
// One wave per (frame, band, strip of <= 62 lanes + 1 halo lane per side), a lane owns PX pixels:
//   row in -> luma (PX floats) -> ring of the last K gray rows -> exact_blur_row: vertical sums of the row whose window
//   is complete, horizontal taps (neighbour lanes through DPP) -> S -> flag test -> [exact chain] -> trunc -> l = LUT[b]
//   (256-byte table in LDS: luma(b,b,b) always sits on the ambiguous S % 1000 == 0 case, so it is tabulated once per
//   workgroup with the FP64 formula) -> 3-row ring of l -> Sobel row in fp32 -> PX bytes stored.
// 4 B read + 1 B written per pixel; nothing intermediate touches memory (the three separate calls move
// 8 + 8 + 5 B/px).  Odd bands walk UPWARD: a band and its lower neighbour then reach their 2R+2 shared boundary
// rows at the same moment (the end of both walks, or the start), and the second reader hits L2 instead of HBM.
// Border rules: gray columns/rows clamp (replicated halo lane / clamped row index); the blurred image reflects:
// column x=-1 takes x=1 and x=w takes x=w-2 by a DPP fix-up in the two edge strips, and a blurred row outside the
// image is replaced by its mirror, which is the OTHER neighbour row of the Sobel stencil.
//
// Why PX = 8: at PX = 4 the kernel is bound by the work of its waves (its rate is proportional to the lanes a strip
// uses, measured by a lane sweep), ~160 instructions per wave-row of 240 pixels.  With 8 pixels per lane a wave-row
// covers 480 pixels and everything that is per ROW rather than per pixel is paid half as often — row control and
// address arithmetic, the flag test's tree / ballot / branch, the neighbour-lane taps of both stencils (4 + 4 DPP reads
// per row either way), the two halo lanes — and the 1-byte output leaves as 8 bytes per lane (480-byte spans = whole
// 32-byte sectors).  The price is registers: two 8-float rings instead of 4-float ones, 4-5 waves per SIMD instead of
// 8.  launch_pipeline (sobel_tile.hip) chooses.
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "kernels.hpp"
#include "slide_common.hpp"
#include "exact_common.hpp"

namespace mi355 {

namespace {

// One input row of a lane: PX RGBA pixels, one 16-byte load per four.
template <int PX>
struct PixRow {
    u32x4 v[PX / 4];
};

// RAGGED = width % 4 != 0 or unaligned buffers (see gauss_slide.hip / sobel_slide.hip): unaligned 16-byte row
// accesses in interior strips, per-pixel clamped loads and per-byte stores in the two edge strips, and the
// reflected column x = w of the blurred image may sit anywhere inside a lane.  PX = 4 only.
// PX = 8 holds twice the registers per lane: it is compiled for 4 waves per SIMD (PX = 4 asks for nothing: 1).
template <int R, int PX, bool CLAMP, bool RAGGED>
__global__ __launch_bounds__(kSlideWavesPerBlock * 64, PX == 8 ? 4 : 1) void pipe_slide_kernel(
    const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int w, int h, int nstrips,
    int lanes_out, BandPlan plan, ExactTables<2 * R + 1> tab)
{
    static_assert(PX == 4 || (PX == 8 && !RAGGED), "8 pixels per lane: aligned rows only");
    constexpr int K = 2 * R + 1;
    __shared__ uint8_t lut[256];  // lut[b] = luma(b, b, b), the reference double-precision formula
    __shared__ float flat[256];   // flat[c] = the CPU path's chain over a window that is c everywhere (exact_common.hpp)
    lut[threadIdx.x] = (uint8_t)luma_rgb(threadIdx.x, threadIdx.x, threadIdx.x);
    flat[threadIdx.x] = flat_chain<K>((float)threadIdx.x, tab.w2);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    SlideItem it;
    if (!slide_item(plan, nstrips, h, &it))
        return;  // (pipeline: after the only barrier)
    const int y0 = it.y0, nout = it.nout;
    const bool up = (it.band & 1) != 0;  // wave-uniform

    // a "quad" is the PX pixels of one lane; one byte out per pixel
    const SlideGeom G = slide_geom<PX>(it.strip, lanes_out, lane, w, 4u * PX, (uint32_t)PX);
    const int jw = w - G.x_lane;  // RAGGED: position of column x = w inside this lane, if 0 <= jw <= 3
    // the pixel a halo lane's neighbour reads
    const int keep_px = (lane == 0) ? PX - 1 : ((G.q_lane == G.q_end) ? 0 : -1);

    // output rows y0 .. y0+nout-1 need blurred rows y0-1 .. y0+nout, which need gray rows y0-1-R .. y0+nout+R
    // (clamp-to-edge)
    const BandWalk W = band_walk(up, y0, nout, R + 1, h);
    const int nin = W.nin;

    const size_t row_bytes = (size_t)w * 4;
    const auto fin = uniform_ptr(in + it.frame * row_bytes * h);
    const auto fout = uniform_ptr(out + it.frame * (size_t)w * h);
    uint32_t in_off = G.in_off, out_off = G.out_off;
    uint32_t px_off[4];  // RAGGED edge strips: the gray image clamps
    ragged_px_offsets<kBorderClamp>(G.x_lane, w, px_off);

    float wv[R + 1];  // wv[d] = weight at distance d from the centre
#pragma unroll
    for (int d = 0; d <= R; d++)
        wv[d] = tab.w1[R - d];
    const float delta = tab.delta, two_delta = 2.0f * tab.delta;

    auto load_row = [&](int i) -> PixRow<PX> {
        // SGPR pair; + 32-bit lane offset = saddr form
        const auto rowp = fin + (size_t)in_row<kBorderClamp>(W, i) * row_bytes;
        lane_offset_here(in_off);
        PixRow<PX> r;
        if constexpr (RAGGED) {
            r.v[0] = ragged_row_load(rowp, G, w, in_off, px_off);
        } else {
#pragma unroll
            for (int n = 0; n < PX / 4; n++)
                r.v[n] = gload<u32x4>(rowp + in_off + 16 * n);
        }
        return r;
    };

    constexpr int PF = 3;
    PixRow<PX> q[K];
#pragma unroll
    for (int u = 0; u < PF; u++)
        q[u] = load_row(u);

    float g[K][PX];  // ring of the last K gray rows; slot = arrival index % K
    float l[3][PX];  // l rows of the last three blurred rows; slot = arrival index % 3
#pragma unroll
    for (int s = 0; s < K; s++)
#pragma unroll
        for (int e = 0; e < PX; e++)
            g[s][e] = 0.0f;
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int e = 0; e < PX; e++)
            l[s][e] = 0.0f;

    // One trip = K input rows: the gray ring's slots are static (slot = u).  The 3-row ring of l starts every trip
    // in the same phase — the previous trip's last two rows sit in slots 0 (older) and 1 (newer), row u writes slot
    // (u + 2) % 3 — which costs 8 register moves per trip when K % 3 != 0 and keeps its slots static as well.
    // (A 3K-row trip needs no moves, but with the exact chains in the body it is past what hipcc unrolls: it kept
    // the ring in LDS with computed slots instead.)
    for (int base = 0; base < nin; base += K) {
#pragma unroll
        for (int u = 0; u < K; u++) {
            const int i = base + u;
            const int s3 = (u + 2) % 3;  // static after unrolling
            PixRow<PX> p = q[u];
            q[(u + PF) % K] = load_row(i + PF);
            if constexpr (!RAGGED) {
                if (G.edge_strip) {  // (in place, not edge_clamp_cols: slide_common.hpp says why)
                    if (G.left_of_image) {  // gray image clamps: replicate column 0
                        const uint32_t c0 = p.v[0].x;
#pragma unroll
                        for (int n = 0; n < PX / 4; n++)
                            p.v[n] = u32x4{c0, c0, c0, c0};
                    }
                    if (G.right_of_image) {  // replicate column w-1
                        const uint32_t c1 = p.v[PX / 4 - 1].w;
#pragma unroll
                        for (int n = 0; n < PX / 4; n++)
                            p.v[n] = u32x4{c1, c1, c1, c1};
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < PX / 4; n++)
                luma_quad_int(p.v[n], &g[u][4 * n], lut);
            // Stage gating with scalar branches (i, y0, nout live in SGPRs, EXEC stays full for the DPP
            // reads): the first 2R rows of a band only fill the gray ring, the next two only fill the
            // 3-row ring, and rows past the band's last output are never stored.
            if (i >= 2 * R) {
                // the blurred row that just completed (window = arrival rows i-2R .. i = slots (u+1+t) % K); a halo
                // lane owes its neighbour one blurred pixel, idle lanes none
                float S[PX];
                exact_blur_row<K, PX, CLAMP>(g, u, up, wv, delta, two_delta, tab.w2, flat, G.stores, keep_px, S);
                float* lb = l[s3];
#pragma unroll
                for (int px = 0; px < PX; px++) {
                    const uint32_t bq = (uint32_t)S[px];  // truncation, as the Gaussian call stores it
                    lb[px] = (float)lut[bq];              // luma(b,b,b) re-applied
                }
                if (G.edge_strip) {
                    // the blurred image reflects (BORDER_REFLECT_101): x = -1 <- x = 1, x = w <- x = w-2
                    const float from_right = dpp_right(lb[1]);      // lane+1's pixel 1
                    const float from_left = dpp_left(lb[PX - 2]);  // lane-1's last pixel but one
                    if (G.left_of_image)
                        lb[PX - 1] = from_right;
                    if constexpr (!RAGGED) {
                        if (G.right_of_image)
                            lb[0] = from_left;
                    } else {
                        // column x = w is pixel jw of this lane; its mirror x = w-2 is pixel jw-2 of this
                        // lane or pixel jw+2 of the lane to the left (w >= 4 here)
                        const float from_left3 = dpp_left(lb[3]);
                        const float l0 = lb[0], l1 = lb[1];
                        if (jw == 0)
                            lb[0] = from_left;
                        if (jw == 1)
                            lb[1] = from_left3;
                        if (jw == 2)
                            lb[2] = l0;
                        if (jw == 3)
                            lb[3] = l1;
                    }
                }
                // blurred arrival row c = i - 2R sits at image row yb(c); the Sobel row between the last
                // three blurred rows is m = yb(c - 1)
                const int c = i - 2 * R;
                const int m = out_row(W, c - 2);
                if (c >= 2 && m >= y0 && m < y0 + nout) {
                    const float* lm = l[(s3 + 2) % 3];  // blurred row m
                    const float* lo = l[(s3 + 1) % 3];  // the neighbour row that arrived first
                    float cs[PX], cd[PX];
                    // A neighbour row outside the image is replaced by its mirror, which is the other
                    // neighbour (reflect-101): only at m = 0 and m = h-1.  Wave-uniform and rare: a branch.
                    if (__builtin_expect(m == 0 || m == h - 1, 0)) {
                        // keeps this a real (never-taken) branch: hipcc otherwise if-converts both arms into
                        // 2 PX v_cndmask per row on the common path
                        asm volatile("; first / last image row");
                        const int y_new = up ? m - 1 : m + 1;  // image row of the newest blurred row (lb)
                        const bool new_outside = y_new < 0 || y_new >= h;
#pragma unroll
                        for (int j = 0; j < PX; j++) {
                            const float nb = new_outside ? lo[j] : lb[j];  // (h >= 2: exactly one is outside)
                            cs[j] = __builtin_fmaf(2.0f, lm[j], nb) + nb;
                            cd[j] = 0.0f;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < PX; j++) {
                            cs[j] = __builtin_fmaf(2.0f, lm[j], lo[j]) + lb[j];
                            cd[j] = lb[j] - lo[j];  // sign depends on the walking direction; only gy^2 is used
                        }
                    }
                    const float csl = dpp_left(cs[PX - 1]), csr = dpp_right(cs[0]);
                    const float cdl = dpp_left(cd[PX - 1]), cdr = dpp_right(cd[0]);
                    float gxs[PX], gys[PX];
#pragma unroll
                    for (int j = 0; j < PX; j++) {
                        const float sl = (j == 0) ? csl : cs[j - 1], sr = (j == PX - 1) ? csr : cs[j + 1];
                        const float dl = (j == 0) ? cdl : cd[j - 1], dr = (j == PX - 1) ? cdr : cd[j + 1];
                        gxs[j] = sr - sl;
                        gys[j] = __builtin_fmaf(2.0f, cd[j], dl) + dr;
                    }
                    uint32_t r[PX / 4];
#pragma unroll
                    for (int n = 0; n < PX / 4; n++)
                        r[n] = sobel_mag_quad(&gxs[4 * n], &gys[4 * n]);
                    // computed by all 64 lanes, BEFORE the store's lane mask: hipcc otherwise sinks the stencil
                    // into the masked region and keeps the four lane shifts outside it as separate
                    // v_mov_b32_dpp (a DPP read under a partial EXEC sees zeros); here three of them fold into
                    // their consumers.  (3 of 160 instructions per row: +0.2 %, within noise.)
                    if constexpr (PX == 8)
                        asm volatile("" : "+v"(r[0]), "+v"(r[1]));
                    else
                        asm volatile("" : "+v"(r[0]));
                    if (G.stores) {
                        const auto rowp = fout + (size_t)m * w;
                        lane_offset_here(out_off);
                        if constexpr (RAGGED) {
                            if (G.edge_strip && G.x_lane + 3 >= w) {  // the last quad of a row may be partial
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    if (G.x_lane + j < w)
                                        rowp[out_off + j] = (uint8_t)(r[0] >> (8 * j));
                            } else {
                                gstore_a1<uint32_t>(rowp + out_off, r[0]);
                            }
                        } else if constexpr (PX == 8) {
                            gstore_nt<u32x2>(rowp + out_off, u32x2{r[0], r[1]});
                        } else {
                            gstore_nt<uint32_t>(rowp + out_off, r[0]);
                        }
                    }
                }
            }
        }
        // the last two rows written sit in slots K % 3 (older) and (K + 1) % 3 (newer): bring them to 0 and 1
        if constexpr (K % 3 == 2) {  // K = 5: older in 2, newer in 0
#pragma unroll
            for (int e = 0; e < PX; e++) {
                l[1][e] = l[0][e];
                l[0][e] = l[2][e];
            }
        } else if constexpr (K % 3 == 1) {  // K = 7: older in 1, newer in 2
#pragma unroll
            for (int e = 0; e < PX; e++) {
                l[0][e] = l[1][e];
                l[1][e] = l[2][e];
            }
        }
    }
}

template <int R, int PX>
hipError_t launch_r(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                    const GaussCoef& coef)
{
    constexpr int K = 2 * R + 1;
    int nstrips, lanes_out;
    BandPlan plan;
    bool planned;
    if constexpr (PX == 8) {
        const int octs = w / 8;
        nstrips = (octs + kSlideLanesOutMax - 1) / kSlideLanesOutMax;
        lanes_out = (octs + nstrips - 1) / nstrips;  // 4K: 480 octets = 8 strips x 60 lanes
        // Tall bands: these waves are few and long (4-5 per SIMD), and each band pays 2R + 2 warm-up rows.  Same
        // box, 256 x 4K frames: k = 5: 24 rows 4.44 TB/s, 48: 4.70, 72: 4.73, 96: 4.82, 144: 4.80,
        // 216: 4.70 (PX = 4: 4.67); k = 3: 16 rows 4.91, 32: 5.14, 48: 5.24, 72: 5.33 (PX = 4: 4.94).
        // Smaller launches get shorter bands (make_band_plan).
        constexpr int kRowsMin = (R == 1) ? 16 : 24, kRowsMax = (R == 1) ? 72 : 96;
        int rows_min = kRowsMin, rows_max = kRowsMax;
        if (const char* e = tune_env("MI355_TUNE_PIPE8_ROWS"))
            rows_min = rows_max = atoi(e);
        planned = make_band_plan(h, nstrips, nframes, (R == 1) ? 5 : 4, rows_min, rows_max, rows_min, 0.0, kRowsMin / 2,
                                 &plan);
    } else {
        const StripPlan sp = make_strip_plan(w);
        nstrips = sp.nstrips;
        lanes_out = sp.lanes_out;
        constexpr int kRows = (R == 1) ? 16 : (R == 2 ? 24 : 40);
        planned = make_band_plan(h, nstrips, nframes, 8, kRows, kRows, kRows, 0.0, kRows / 2, &plan);
    }
    if (!planned)
        return hipErrorInvalidValue;
    double wsum;
    const ExactTables<K> tab = make_exact_tables<K>(coef, &wsum);
    const bool ragged = PX == 4 && rows_ragged(w, d_in, 16, d_out, 4);
    return dispatch_bool(gauss_upper_clamp(wsum), [&](auto CL) {
        return dispatch_bool(ragged, [&](auto RG) {
            if constexpr (PX == 4 || !RG.value)  // 8 pixels per lane: aligned rows only
                return launch_slide(pipe_slide_kernel<R, PX, CL.value, RG.value>, plan, stream, d_in, d_out, w, h,
                                    nstrips, lanes_out, plan, tab);
            else
                return hipErrorInvalidValue;  // (never reached: ragged implies PX == 4)
        });
    });
}

}  // namespace

// px = 4: k in {3,5,7}, width >= 4, height >= 2, dword-aligned input, and a table the exact-by-exception stage can
// take (anything else goes to the tiled kernel).  px = 8 also: k in {3,5}, width a multiple of 8 (>= 16), 16-byte
// aligned input, 8-byte aligned output.
bool pipe_slide_supported(const uint8_t* d_in, const uint8_t* d_out, int w, int h, const GaussCoef& coef, int px)
{
    const int k = coef.k;
    if (k != 3 && k != 5 && k != 7)
        return false;
    if (w < 4 || h < 2 || !exact_tables_ok(coef) || !aligned_to(d_in, 4))
        return false;
    if (px == 4)
        return true;
    if (px != 8 || k == 7 || (w & 7) != 0 || w < 16)
        return false;
    return aligned_to(d_in, 16) && aligned_to(d_out, 8);
}

hipError_t launch_pipe_slide(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                             const GaussCoef& coef, int px)
{
    return dispatch_int(coef.k, std::integer_sequence<int, 3, 5, 7>{}, [&](auto K) {
        return dispatch_int(px, std::integer_sequence<int, 4, 8>{}, [&](auto PX) {
            if constexpr (PX.value == 4 || K.value <= 5)  // 8 pixels per lane: k = 3, 5
                return launch_r<K.value / 2, PX.value>(stream, d_in, d_out, w, h, nframes, coef);
            else
                return hipErrorInvalidValue;
        });
    });
}

}  // namespace mi355
