// gray8.hip — the single-channel (1 byte per pixel) filters: Gaussian, Sobel and the fused Gaussian -> Sobel chain on
// frames that are already gray (mono cameras, the luma plane of a decoded frame, this library's own GRAY1 output).
//
// Semantics (include/mi355_imgfilter.h, MI355_FILTER_*_GRAY8):
//   Gaussian  src/GaussianBlur/GaussianBlur.cpp:234-261 on one channel: clamp-to-edge taps, the reference table,
//             truncation.  The R channel of the RGBA Gaussian of (y, y, y, 255).
//   Sobel     src/EdgeDetection/EdgeDetection.cpp:219-240 on the given plane: 3x3 correlation, BORDER_REFLECT_101,
//             round-half-even magnitude, saturation.  No luminance step.
//   Pipeline  Sobel of the EXACT Gaussian, in both Gaussian modes.
//
// One LDS-staged kernel template for all three, on the tile frame of tile_common.hpp.  A workgroup (256 threads)
// produces a 256 x 32 output tile:
//   1. stage the tile plus its halo as raw bytes in LDS, in 16-byte chunks under the filter's border
//      rule: clamp for the Gaussian, reflect-101 for the Sobel alone;
//   2. Gaussian: vertical then horizontal pass in the pair form of exact_common.hpp (acc = w_c g_c, then
//      acc = fma(w_d, g_{c-d} + g_{c+d}, acc)), one pixel per thread, consecutive threads on consecutive columns
//      (no LDS bank conflicts).  "Exact by exception": with delta = delta_bound() of the two tables, a pixel whose
//      separable sum lies further than delta from an integer truncates to the CPU path's byte; the few within delta are
//      recomputed with the CPU path's own k*k chain from the staged bytes.  A table that is not a symmetric
//      non-negative separable product runs that chain for every pixel (tap by tap, as the reference kernel applies it);
//   3. Sobel from the staged bytes (Sobel alone) or from the blurred tile, which the pipeline computes one pixel wider
//      on each side at reflect-101 coordinates, so the Sobel stage itself has no border cases;
//   4. the output tile leaves LDS as one 16-byte store per thread and row piece (store_chunk16; the MI355X store path
//      prices a dword store at ~6x a dwordx4 per byte; MI355X_MICROARCH.md).
// Algorithmic bytes: 2 B/px.  k in {3, 5, 7} is compiled with a constant k (unrolled taps); everything else takes the
// runtime-k instantiation.
#include <cmath>

#include "common.hpp"
#include "exact_common.hpp"
#include "kernels.hpp"
#include "slide_common.hpp"
#include "tile_common.hpp"

namespace mi355 {

namespace {

constexpr int kG8TW = 256;  // output tile width (bytes)
constexpr int kG8TH = 32;   // output tile height
constexpr int kG8Threads = 256;

enum G8Op { kOpGauss = 0, kOpSobel = 1, kOpPipe = 2 };
// Gaussian arithmetic: separable sum only (FAST, within 1 LSB), exact by exception, the CPU chain for every pixel
enum G8Gm { kGmSep = 0, kGmExc = 1, kGmTap = 2 };

__host__ __device__ constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// LDS carve, shared by the kernel and the launcher (byte offsets)
struct G8Layout {
    int H, RH, RW, RWS, GH, GW, GWS;
    int off_v, off_w2, off_w1, off_raw, off_g, off_o, bytes;
};

__host__ __device__ inline G8Layout g8_layout(int op, int gm, int k)
{
    G8Layout L{};
    const int R = k / 2, o = op == kOpPipe ? 1 : 0;
    L.H = op == kOpSobel ? 1 : R + o;
    L.RH = kG8TH + 2 * L.H;
    L.RW = kG8TW + 2 * L.H;
    L.RWS = round_up(L.RW, 16);
    L.GH = kG8TH + 2 * o;
    L.GW = kG8TW + 2 * o;
    L.GWS = round_up(L.GW, 4);
    const bool gauss = op != kOpSobel;
    // every region starts on a 16-byte boundary: the staged and output tiles are accessed as ds_*_b128, which replay
    // when misaligned (a k*k table is 4 mod 8 bytes long for odd k)
    int off = 0;
    L.off_v = off;
    off += round_up((gauss && gm != kGmTap) ? L.GH * L.RW * 4 : 0, 16);
    L.off_w2 = off;
    off += round_up((gauss && gm != kGmSep) ? k * k * 4 : 0, 16);
    L.off_w1 = off;
    off += round_up(gauss ? k * 4 : 0, 16);
    L.off_raw = off;
    off += round_up(L.RH * L.RWS, 16);
    L.off_g = off;
    off += round_up(op == kOpPipe ? L.GH * L.GWS : 0, 16);
    L.off_o = off;
    off += kG8TH * kG8TW;
    L.bytes = off;
    return L;
}

// the CPU path's sum (GaussianBlur.cpp:243-256: ky outer, kx inner, float multiply then float add) for the pixel whose
// window's top-left byte sits at raw[0]
template <int KC>
__device__ __forceinline__ float g8_chain(const uint8_t* raw, int rws, int k_rt, const float* w2)
{
    const int k = KC > 0 ? KC : k_rt;
    constexpr int kUnroll = KC > 0 ? KC : 1;
    float sum = 0.0f;
#pragma unroll kUnroll
    for (int ky = 0; ky < k; ky++) {
        const uint8_t* r = raw + ky * rws;
#pragma unroll kUnroll
        for (int kx = 0; kx < k; kx++)
            sum = sum + (float)r[kx] * w2[ky * k + kx];  // -ffp-contract=off: multiply, then add
    }
    return sum;
}

template <int OP, int KC, int GM>
__global__ __launch_bounds__(kG8Threads) void gray8_tile_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                int w, int h, int tiles_x, int tiles_y, uint32_t ntiles,
                                                                int k_rt, const float* __restrict__ d_w2,
                                                                const float* __restrict__ d_w1, float delta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kGauss = OP != kOpSobel;
    const int k = OP == kOpSobel ? 1 : (KC > 0 ? KC : k_rt);
    const int R = k / 2;
    constexpr int o = OP == kOpPipe ? 1 : 0;
    constexpr int kUnrollR = KC > 0 ? KC / 2 : 1;
    const G8Layout L = g8_layout(OP, GM, k);
    float* V = reinterpret_cast<float*>(smem + L.off_v);
    float* w2 = reinterpret_cast<float*>(smem + L.off_w2);
    float* w1 = reinterpret_cast<float*>(smem + L.off_w1);  // w1[d] = weight at distance d from the centre
    uint8_t* raw = smem + L.off_raw;
    uint8_t* G = smem + L.off_g;
    uint8_t* O = smem + L.off_o;

    constexpr Border kBorder = OP == kOpSobel ? kBorderReflect101 : kBorderClamp;  // of the staged tile
    const TilePos t = tile_decode(xcd_remap(blockIdx.x, ntiles), tiles_x, tiles_y, kG8TW, kG8TH);
    const uint8_t* fin = in + t.frame * (size_t)w * h;
    uint8_t* fout = out + t.frame * (size_t)w * h;
    const int x0 = t.x0, y0 = t.y0;
    const int sy0 = y0 - L.H, sx0 = x0 - L.H;  // image position of staged byte (0, 0)
    const int tid = threadIdx.x;

    if constexpr (kGauss) {
        if constexpr (GM != kGmSep)
            for (int i = tid; i < k * k; i += kG8Threads)
                w2[i] = d_w2[i];
        for (int i = tid; i <= R; i += kG8Threads)
            w1[i] = d_w1[R + i];
    }
    // 1. stage: staged (s, c) = image (border(sy0 + s), border(sx0 + c))
    const int npieces = L.RWS / 16;
    for (int i = tid; i < L.RH * npieces; i += kG8Threads) {
        const int s = i / npieces, p = i - s * npieces;
        const uint8_t* row = fin + (size_t)border_index<kBorder>(sy0 + s, h) * w;
        const int gx = sx0 + 16 * p;
        u32x4 v;
        if (gx >= 0 && gx + 16 <= w) {
            v = *reinterpret_cast<const u32x4_a1*>(row + gx);
        } else {
            uint32_t b[16];
#pragma unroll
            for (int j = 0; j < 16; j++)
                b[j] = row[border_index<kBorder>(gx + j, w)];
#pragma unroll
            for (int q = 0; q < 4; q++)
                v[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
        }
        *reinterpret_cast<u32x4*>(raw + s * L.RWS + 16 * p) = v;
    }
    __syncthreads();

    if constexpr (kGauss) {
        // blurred tile row r / column c sits at image row gmap_y(r) / column gmap_x(c): the output tile itself for the
        // Gaussian; for the pipeline one more row / column on each side, at reflect-101 positions (the Sobel's border
        // rule applied to the blurred image), clamped first so that rows far past the image stay inside the staged tile
        auto gmap_y = [&](int r) { return o ? border_index<kBorderReflect101>(y0 - 1 + r, h) : min(y0 + r, h - 1); };
        auto gmap_x = [&](int c) { return o ? border_index<kBorderReflect101>(x0 - 1 + c, w) : min(x0 + c, w - 1); };
        uint8_t* dst = o ? G : O;
        const int dst_stride = o ? L.GWS : kG8TW;
        if constexpr (GM == kGmTap) {
            for (int i = tid; i < L.GH * L.GW; i += kG8Threads) {
                const int r = i / L.GW, c = i - r * L.GW;
                const int sr = gmap_y(r) - R - sy0, sc = gmap_x(c) - R - sx0;
                dst[r * dst_stride + c] = (uint8_t)f2u8(g8_chain<KC>(raw + sr * L.RWS + sc, L.RWS, k, w2));
            }
        } else {
            // 2a. vertical pass over every staged column of the blurred rows
            for (int i = tid; i < L.GH * L.RW; i += kG8Threads) {
                const int r = i / L.RW, c = i - r * L.RW;
                const uint8_t* col = raw + (gmap_y(r) - sy0) * L.RWS + c;  // centre tap
                float acc = w1[0] * (float)col[0];
#pragma unroll kUnrollR
                for (int d = 1; d <= R; d++)
                    acc = __builtin_fmaf(w1[d], (float)((uint32_t)col[-d * L.RWS] + (uint32_t)col[d * L.RWS]), acc);
                V[r * L.RW + c] = acc;
            }
            __syncthreads();
            // 2b. horizontal pass; S' = S + delta rides on the centre tap (pipe_slide.hip), so "S within delta of an
            // integer" reads "fract(S') < 2 delta"
            const float d0 = GM == kGmExc ? delta : 0.0f, two_delta = 2.0f * delta;
            for (int i = tid; i < L.GH * L.GW; i += kG8Threads) {
                const int r = i / L.GW, c = i - r * L.GW;
                const int cc = gmap_x(c) - sx0;
                const float* vr = V + r * L.RW + cc;
                float acc = __builtin_fmaf(w1[0], vr[0], d0);
#pragma unroll kUnrollR
                for (int d = 1; d <= R; d++)
                    acc = __builtin_fmaf(w1[d], vr[-d] + vr[d], acc);
                if constexpr (GM == kGmExc) {
                    if (__builtin_amdgcn_fractf(acc) < two_delta)
                        acc = g8_chain<KC>(raw + (gmap_y(r) - R - sy0) * L.RWS + cc - R, L.RWS, k, w2);
                }
                dst[r * dst_stride + c] = (uint8_t)f2u8(acc);
            }
        }
        if constexpr (OP == kOpPipe)
            __syncthreads();
    }

    if constexpr (OP != kOpGauss) {
        // 3. Sobel of the centre of src: staged bytes (Sobel alone) or the blurred tile, both one pixel wider per side
        //    and already at reflect-101 positions
        const uint8_t* src = OP == kOpSobel ? raw : G;
        const int ss = OP == kOpSobel ? L.RWS : L.GWS;
        for (int i = tid; i < kG8TH * kG8TW; i += kG8Threads) {
            const int r = i / kG8TW, c = i - r * kG8TW;
            const uint8_t* t = src + r * ss + c;
            const uint8_t* m = t + ss;
            const uint8_t* b = m + ss;
            const int gx = ((int)t[2] + 2 * (int)m[2] + (int)b[2]) - ((int)t[0] + 2 * (int)m[0] + (int)b[0]);
            const int gy = ((int)b[0] + 2 * (int)b[1] + (int)b[2]) - ((int)t[0] + 2 * (int)t[1] + (int)t[2]);
            O[i] = (uint8_t)sobel_mag_fast((float)gx, (float)gy);  // |gx|, |gy| <= 1020: exact (common.hpp)
        }
    }
    __syncthreads();

    // 4. one 16-byte store per thread and row piece
    constexpr int kPieces = kG8TW / 16;
    for (int i = tid; i < kG8TH * kPieces; i += kG8Threads) {
        const int r = i / kPieces, p = i - r * kPieces;
        const int gy = y0 + r, gx = x0 + 16 * p;
        if (gy >= h || gx >= w)
            continue;
        store_chunk16<1>(fout + (size_t)gy * w, gx, w, *reinterpret_cast<const u32x4*>(O + r * kG8TW + 16 * p));
    }
}

template <int OP, int KC, int GM>
hipError_t launch_g8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                     const float* d_w2, const float* d_w1, float delta)
{
    const TileGrid g(w, h, nframes, kG8TW, kG8TH);
    const G8Layout L = g8_layout(OP, GM, OP == kOpSobel ? 1 : k);
    return launch_tiles(gray8_tile_kernel<OP, KC, GM>, g, kG8Threads, L.bytes, kLdsRaise, stream, d_in, d_out, w, h,
                        g.tiles_x, g.tiles_y, g.n(), k, d_w2, d_w1, delta);
}

// const_k: k is 3, 5 or 7 and gets its own instantiation; otherwise the runtime-k one (KC = 0)
template <int OP, int GM>
hipError_t launch_g8_k(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                       const GaussCoef& coef, bool const_k, float delta)
{
    return dispatch_int(const_k ? coef.k : 0, std::integer_sequence<int, 0, 3, 5, 7>{}, [&](auto KC) {
        return launch_g8<OP, decltype(KC)::value, GM>(stream, d_in, d_out, w, h, nframes, coef.k, coef.d_w2d, coef.d_w1d,
                                                      delta);
    });
}

// The pair-form separable sum stands in for the table when the table is a symmetric non-negative separable product
// (coef.separable, w1 symmetric): within 1 LSB of the CPU path (FAST).
bool g8_separable(const GaussCoef& coef)
{
    const int k = coef.k;
    if (!coef.separable || !coef.h_w2d)
        return false;
    for (int j = 0; j < k / 2; j++)
        if (coef.h_w1d[j] != coef.h_w1d[k - 1 - j])
            return false;
    return true;
}

// delta for the exact-by-exception arithmetic, or a negative value when it does not apply (not separable, or a bound
// too wide to leave few exceptions)
double g8_delta(const GaussCoef& coef)
{
    if (!g8_separable(coef))
        return -1.0;
    const double delta = delta_bound_k(coef.k, coef.h_w1d, coef.h_w2d);
    return delta < 0.01 ? delta : -1.0;
}

}  // namespace

hipError_t launch_gauss_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                              const GaussCoef& coef, bool exact, int impl)
{
    const bool tile = impl == 1;
    const bool const_k = !tile && (coef.k == 3 || coef.k == 5 || coef.k == 7);
    // `exact` is also set for tables that are not separable (dispatch_dev): those always take the CPU chain
    const bool separable = g8_separable(coef);
    const double delta = g8_delta(coef);
    if (!exact) {
        // FAST: the separable sum; exact by exception for the constant-k instantiations, which costs them next to nothing
        if (const_k && delta >= 0.0)
            return launch_g8_k<kOpGauss, kGmExc>(stream, d_in, d_out, w, h, nframes, coef, const_k, (float)delta);
        if (separable)
            return launch_g8_k<kOpGauss, kGmSep>(stream, d_in, d_out, w, h, nframes, coef, const_k, 0.0f);
        return launch_g8_k<kOpGauss, kGmTap>(stream, d_in, d_out, w, h, nframes, coef, const_k, 0.0f);
    }
    // EXACT: the CPU chain only where it is needed (AUTO) or for every pixel (TILE, and tables the bound does not cover)
    if (!tile && delta >= 0.0)
        return launch_g8_k<kOpGauss, kGmExc>(stream, d_in, d_out, w, h, nframes, coef, const_k, (float)delta);
    return launch_g8_k<kOpGauss, kGmTap>(stream, d_in, d_out, w, h, nframes, coef, const_k, 0.0f);
}

hipError_t launch_sobel_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes)
{
    return launch_g8<kOpSobel, 0, kGmSep>(stream, d_in, d_out, w, h, nframes, 1, nullptr, nullptr, 0.0f);
}

hipError_t launch_pipeline_gray8(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                                 const GaussCoef& coef, int impl)
{
    // the blurred image is the EXACT Gaussian in both modes
    const bool tile = impl == 1;
    const bool const_k = !tile && (coef.k == 3 || coef.k == 5 || coef.k == 7);
    const double delta = g8_delta(coef);
    if (delta < 0.0 || tile)
        return launch_g8_k<kOpPipe, kGmTap>(stream, d_in, d_out, w, h, nframes, coef, const_k, 0.0f);
    return launch_g8_k<kOpPipe, kGmExc>(stream, d_in, d_out, w, h, nframes, coef, const_k, (float)delta);
}

}  // namespace mi355
