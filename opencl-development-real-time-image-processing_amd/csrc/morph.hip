// morph.hip — rectangular grey-level morphology (MI355_FILTER_ERODE / DILATE / OPEN / CLOSE and their *_GRAY8 forms):
// cv::erode / cv::dilate / cv::morphologyEx(MORPH_OPEN / MORPH_CLOSE) with a k x k MORPH_RECT element anchored at the
// centre, odd 3 <= k <= MI355_MAX_MORPH_K, every channel on its own (alpha included), clamp-to-edge (BORDER_REPLICATE)
// borders, frames independent.  Every output byte is an input byte: the kernel is tested for bit-identity only.
//
// One kernel, morph_kernel<G8, K, OP>, serves all eight ids (the impl knob does not select anything here), on the tile
// frame of tile_common.hpp.  A block of 256 threads owns a TW x TH output tile of one frame:
//   load    the tile plus a halo of H = r (one stage) or 2r (OPEN / CLOSE) rows and HC >= H columns (HC rounded up to
//           one 16-byte chunk) goes to the LDS buffer `raw` as pixels, rows clamped, 16-byte loads inside the frame, clamped pixel loads across its edges;
//   stage   a separable min (ERODE) or max (DILATE): the H pass reads runs of NR pixels (+ 2r halo) of a row of `raw`
//           (consecutive lanes: consecutive rows), takes the window min of each and writes words to `hb`; the V pass
//           reads NV rows (+ 2r) of a word column of `hb` (consecutive lanes: consecutive columns) and writes the
//           window min back to `raw` as pixels.  Both LDS buffers have odd dword pitches, so either walk spreads a
//           wave over all banks.  OPEN is a min stage then a max stage, CLOSE the other order;
//   fix-up  (OPEN / CLOSE, border tiles only) the first stage produced the tile plus r on every side; its positions
//           outside the frame are overwritten with the value at the clamped position, so the second stage sees the
//           clamp-to-edge border of the intermediate frame, not a first stage extended past the edge;
//   store   16-byte global stores of the tile (store_chunk16).
// Words are two u16 lanes and every min is one v_pk_min_u16 for two values: RGBA splits each pixel into (R, B) and
// (G, A) (split_rgba); gray8 packs pixels (x, x + NR / 2) of one run.  The window min of a run of N
// outputs is either the plain k - 1 mins per output or window doubling (m_2s[i] = min(m_s[i], m_s[i + s]) up to the
// largest power of two P <= k, then min(m_P[i], m_P[i + k - P])), whichever costs fewer mins at compile time: about
// log2(k) + 1 per output instead of k - 1, so k = 17 costs no more than a few times k = 3.
#include "../../include/mi355_imgfilter.h"
#include "common.hpp"
#include "kernels.hpp"
#include "tile_common.hpp"

namespace mi355 {

namespace {

constexpr int kMorThreads = 256;

template <bool MAX>
__device__ __forceinline__ u16x2 pop(u16x2 a, u16x2 b) { return MAX ? pmax(a, b) : pmin(a, b); }

constexpr int pow2_floor(int k) { return k >= 16 ? 16 : k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1; }

// packed mins for N outputs of a k-window: plain, and by doubling
constexpr int plain_cost(int n, int k) { return n * (k - 1); }
constexpr int doubling_cost(int n, int k)
{
    int c = n;  // the final min(m_P[i], m_P[i + k - P])
    for (int s = 1; s < pow2_floor(k); s *= 2)
        c += n + k - 2 * s;  // entries of m_2s that are valid: L - 2s + 1, L = n + k - 1
    return c;
}

// out[i] = min (MAX: max) of v[i .. i + K - 1] for i in [0, N); v is clobbered
template <int N, int K, bool MAX>
__device__ __forceinline__ void window_min(u16x2 (&v)[N + K - 1], u16x2 (&out)[N])
{
    constexpr int L = N + K - 1;
    if constexpr (plain_cost(N, K) <= doubling_cost(N, K)) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            u16x2 m = v[i];
#pragma unroll
            for (int d = 1; d < K; d++)
                m = pop<MAX>(m, v[i + d]);
            out[i] = m;
        }
    } else {
        constexpr int P = pow2_floor(K);
        // in place, ascending i: v[i + s] is still the previous level when v[i] reads it
#pragma unroll
        for (int s = 1; s < P; s *= 2)
#pragma unroll
            for (int i = 0; i + 2 * s <= L; i++)
                v[i] = pop<MAX>(v[i], v[i + s]);
#pragma unroll
        for (int i = 0; i < N; i++)
            out[i] = pop<MAX>(v[i], v[i + K - P]);
    }
}

template <bool G8, int K, bool TWO>
struct Geom {
    static constexpr int R = K / 2;
    static constexpr int H = TWO ? 2 * R : R;               // halo rows of the loaded tile
    static constexpr int PXC = G8 ? 16 : 4;                 // pixels per 16-byte chunk
    static constexpr int HC = (H + PXC - 1) / PXC * PXC;    // halo columns of the loaded tile (whole chunks)
    static constexpr int TW = G8 ? 128 : 64, TH = 32;       // output tile
    static constexpr int NR = G8 ? 16 : 8;                  // pixels per run of the H pass
    static constexpr int NV = 8;                            // rows per run of the V pass
    static constexpr int NWR = G8 ? NR / 2 : NR;            // words per run and plane
    static constexpr int PLANES = G8 ? 1 : 2;
    static constexpr int RAWH = TH + 2 * H;
    // a run reads NR + 2r pixels (gray8: rounded out to dwords) from at most TW + HC + H + NR + 3: pad the pitch, to an
    // odd number of dwords, so that the H pass (one lane per row) and the V pass (one lane per column) hit 32 banks
    static constexpr int RAWP = G8 ? TW + 2 * HC + NR + 20 : TW + 2 * HC + NR + 17;  // pixels
    static constexpr int RAWP_DW = RAWP * (G8 ? 1 : 4) / 4;
    static constexpr int RAW_DW = RAWH * RAWP_DW;
    static constexpr int OW_MAX = TW + 2 * (H - R);          // widest stage output (the first stage)
    static constexpr int NRUNS_MAX = (OW_MAX + NR - 1) / NR;
    static constexpr int HBP = NRUNS_MAX * NWR + 1;          // words per hb row and plane (odd)
    static constexpr int HBH = RAWH + NV;                    // V runs read up to NV - 1 rows past the last one
    static constexpr int HB_DW = PLANES * HBH * HBP;
    static_assert(RAWP * (G8 ? 1 : 4) % 4 == 0 && RAWP_DW % 2 == 1 && HBP % 2 == 1, "odd dword pitches");
};

// one min stage: raw (input of this stage) -> hb -> raw (its output).  Ho = output halo of the stage (r for the first
// of two stages, 0 otherwise); the output is rows / columns -Ho .. TH / TW + Ho of the tile.
template <bool G8, int K, bool TWO, int Ho, bool MAX>
__device__ __forceinline__ void minmax_stage(uint32_t* raw, uint32_t* hb)
{
    using G = Geom<G8, K, TWO>;
    constexpr int R = G::R, NR = G::NR, NV = G::NV, NWR = G::NWR;
    const int tid = threadIdx.x;
    constexpr int OW = G::TW + 2 * Ho, OH = G::TH + 2 * Ho;
    constexpr int RI = OH + 2 * R;                 // input rows of the stage
    constexpr int row0 = G::H - Ho - R;            // raw row of the first input row
    constexpr int off = G::HC - Ho - R;            // raw column of output column 0's window start
    constexpr int nruns = (OW + NR - 1) / NR;

    // H pass: hb[plane][i][run * NWR + c] = min over the k-window of input row i
    for (int item = tid; item < RI * nruns; item += kMorThreads) {
        const int q = item / RI, i = item - q * RI;  // consecutive lanes take consecutive rows
        const int col = q * NR + off;              // raw column of this run's first input pixel
        if constexpr (!G8) {
            const uint32_t* src = raw + (size_t)(row0 + i) * G::RAWP + col;
            u16x2 rb[NR + K - 1], ga[NR + K - 1], orb[NR], oga[NR];
#pragma unroll
            for (int j = 0; j < NR + K - 1; j++)
                split_rgba(src[j], rb[j], ga[j]);
            window_min<NR, K, MAX>(rb, orb);
            window_min<NR, K, MAX>(ga, oga);
            uint32_t* d0 = hb + (size_t)i * G::HBP + q * NWR;
            uint32_t* d1 = d0 + (size_t)G::HBH * G::HBP;
#pragma unroll
            for (int c = 0; c < NR; c++) {
                d0[c] = as_u32(orb[c]);
                d1[c] = as_u32(oga[c]);
            }
        } else {
            // bytes col .. col + NR + 2r - 1 from whole dwords; col % 4 is the same for every run of the stage
            const uint8_t* r8 = reinterpret_cast<const uint8_t*>(raw) + (size_t)(row0 + i) * G::RAWP;
            constexpr int sh = off & 3;  // NR is a multiple of 4: the same for every run
            const uint32_t* src = reinterpret_cast<const uint32_t*>(r8 + (col - sh));
            constexpr int NB = NR + K - 1, ND = (NB + 3) / 4 + 1;
            uint32_t d[ND];
#pragma unroll
            for (int j = 0; j < ND; j++)
                d[j] = src[j];
            uint32_t b[NB];
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const uint64_t pair = (uint64_t)d[j / 4] | ((uint64_t)d[j / 4 + 1] << 32);
                b[j] = (uint32_t)(pair >> (8 * ((j & 3) + sh))) & 0xFFu;
            }
            // word c = pixels (c, c + NR / 2) of the run
            u16x2 v[NWR + K - 1], o[NWR];
#pragma unroll
            for (int c = 0; c < NWR + K - 1; c++)
                v[c] = as_u16x2(b[c] | (b[c + NWR] << 16));
            window_min<NWR, K, MAX>(v, o);
            uint32_t* dst = hb + (size_t)i * G::HBP + q * NWR;
#pragma unroll
            for (int c = 0; c < NWR; c++)
                dst[c] = as_u32(o[c]);
        }
    }
    __syncthreads();

    // V pass: output row t of the stage = min over hb rows t .. t + 2r; written to raw row H - Ho + t
    constexpr int ncol = G8 ? nruns * NWR : OW;
    constexpr int nvr = (OH + NV - 1) / NV;
    for (int item = tid; item < ncol * nvr; item += kMorThreads) {
        const int rr = item / ncol, c = item - rr * ncol;
        const int t0 = rr * NV;
        const int orow = G::H - Ho + t0;
        if constexpr (!G8) {
            const uint32_t* s0 = hb + (size_t)t0 * G::HBP + c;
            const uint32_t* s1 = s0 + (size_t)G::HBH * G::HBP;
            u16x2 rb[NV + K - 1], ga[NV + K - 1], orb[NV], oga[NV];
#pragma unroll
            for (int j = 0; j < NV + K - 1; j++) {
                rb[j] = as_u16x2(s0[(size_t)j * G::HBP]);
                ga[j] = as_u16x2(s1[(size_t)j * G::HBP]);
            }
            window_min<NV, K, MAX>(rb, orb);
            window_min<NV, K, MAX>(ga, oga);
            uint32_t* dst = raw + (size_t)orow * G::RAWP + (G::HC - Ho) + c;
#pragma unroll
            for (int j = 0; j < NV; j++)
                if (t0 + j < OH)
                    dst[(size_t)j * G::RAWP] = join_rgba(orb[j], oga[j]);
        } else {
            const uint32_t* s0 = hb + (size_t)t0 * G::HBP + c;
            u16x2 v[NV + K - 1], o[NV];
#pragma unroll
            for (int j = 0; j < NV + K - 1; j++)
                v[j] = as_u16x2(s0[(size_t)j * G::HBP]);
            window_min<NV, K, MAX>(v, o);
            const int q = c / NWR, cc = c - q * NWR;
            const int p0 = q * NR + cc, p1 = p0 + NWR;  // output columns of the low and high lane
            uint8_t* dst = reinterpret_cast<uint8_t*>(raw) + (size_t)orow * G::RAWP + (G::HC - Ho);
#pragma unroll
            for (int j = 0; j < NV; j++) {
                if (t0 + j < OH) {
                    const uint32_t x = as_u32(o[j]);
                    if (p0 < OW)
                        dst[(size_t)j * G::RAWP + p0] = (uint8_t)x;
                    if (p1 < OW)
                        dst[(size_t)j * G::RAWP + p1] = (uint8_t)(x >> 16);
                }
            }
        }
    }
    __syncthreads();
}

// OP: 0 erode, 1 dilate, 2 open (min stage, then max stage), 3 close (max, then min)
template <bool G8, int K, int OP>
__global__ __launch_bounds__(kMorThreads) void morph_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                            int w, int h, int tiles_x, int tiles_y)
{
    constexpr bool TWO = OP >= 2;
    using G = Geom<G8, K, TWO>;
    constexpr int BPP = G8 ? 1 : 4, PXC = G::PXC;
    __shared__ __attribute__((aligned(16))) uint32_t raw[G::RAW_DW];
    __shared__ __attribute__((aligned(16))) uint32_t hb[G::HB_DW];
    const int tid = threadIdx.x;
    const TilePos tp = tile_decode(blockIdx.x, tiles_x, tiles_y, G::TW, G::TH);  // no XCD remap: not measured here
    const size_t fbytes = (size_t)w * h * BPP;
    const uint8_t* fin = in + tp.frame * fbytes;
    uint8_t* fout = out + tp.frame * fbytes;
    const int x0 = tp.x0, y0 = tp.y0;
    uint8_t* raw8 = reinterpret_cast<uint8_t*>(raw);

    // load: raw row a, column l = frame (clamp(y0 - H + a), clamp(x0 - HC + l))
    {
        constexpr int NCH = (G::TW + 2 * G::HC) / PXC;
        for (int item = tid; item < G::RAWH * NCH; item += kMorThreads) {
            const int a = item / NCH, j = item - a * NCH;
            const int gy = clampi(y0 - G::H + a, 0, h - 1);
            const int gx = x0 - G::HC + j * PXC;
            const uint8_t* row = fin + (size_t)gy * w * BPP;
            u32x4 v;
            if (gx >= 0 && gx + PXC <= w) {
                v = *reinterpret_cast<const chunk16<BPP>*>(row + (size_t)gx * BPP);
            } else if constexpr (!G8) {
                const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row);
#pragma unroll
                for (int p = 0; p < 4; p++)
                    v[p] = r32[clampi(gx + p, 0, w - 1)];
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    v[p] = (uint32_t)row[clampi(gx + 4 * p, 0, w - 1)] |
                           ((uint32_t)row[clampi(gx + 4 * p + 1, 0, w - 1)] << 8) |
                           ((uint32_t)row[clampi(gx + 4 * p + 2, 0, w - 1)] << 16) |
                           ((uint32_t)row[clampi(gx + 4 * p + 3, 0, w - 1)] << 24);
            }
            uint32_t* d = raw + (size_t)a * G::RAWP_DW + 4 * j;  // dword stores: the odd pitch leaves rows 4-byte aligned
#pragma unroll
            for (int p = 0; p < 4; p++)
                d[p] = v[p];
        }
    }
    __syncthreads();

    if constexpr (TWO) {
        constexpr int R = G::R;
        minmax_stage<G8, K, TWO, G::R, OP == 3>(raw, hb);
        // the intermediate outside the frame is the intermediate at the clamped position
        if (y0 - R < 0 || y0 + G::TH + R > h || x0 - R < 0 || x0 + G::TW + R > w) {
            const int OW = G::TW + 2 * R, OH = G::TH + 2 * R;
            for (int item = tid; item < OW * OH; item += kMorThreads) {
                const int t = item / OW, c = item - t * OW;
                const int fy = y0 - R + t, fx = x0 - R + c;
                const int cy = clampi(fy, 0, h - 1), cx = clampi(fx, 0, w - 1);
                if (cy != fy || cx != fx) {
                    const size_t d = (size_t)(G::H - R + t) * G::RAWP + (G::HC - R + c);
                    const size_t s = (size_t)(cy - y0 + G::H) * G::RAWP + (cx - x0 + G::HC);
                    if constexpr (G8)
                        raw8[d] = raw8[s];
                    else
                        raw[d] = raw[s];
                }
            }
            __syncthreads();
        }
        minmax_stage<G8, K, TWO, 0, OP == 2>(raw, hb);
    } else {
        minmax_stage<G8, K, TWO, 0, OP == 1>(raw, hb);
    }

    // store: tile rows y0 .. y0 + TH, 16-byte chunks
    constexpr int NCO = G::TW / PXC;
    for (int item = tid; item < G::TH * NCO; item += kMorThreads) {
        const int t = item / NCO, j = item - t * NCO;
        const int gy = y0 + t, gx = x0 + j * PXC;
        if (gy >= h || gx >= w)
            continue;
        const uint32_t* sp = raw + (size_t)(G::H + t) * G::RAWP_DW + (G::HC * BPP) / 4 + 4 * j;
        const u32x4 v = {sp[0], sp[1], sp[2], sp[3]};
        store_chunk16<BPP>(fout + (size_t)gy * w * BPP, gx, w, v);
    }
}

template <bool G8, int K, int OP>
hipError_t launch_k(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes)
{
    using G = Geom<G8, K, (OP >= 2)>;
    const TileGrid g(w, h, nframes, G::TW, G::TH);
    return launch_tiles(morph_kernel<G8, K, OP>, g, kMorThreads, 0, kLdsDefault, stream, d_in, d_out, w, h, g.tiles_x,
                        g.tiles_y);
}

}  // namespace

hipError_t launch_morph(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                        int op, bool gray8)
{
    static_assert(MI355_MAX_MORPH_K == 17, "the list below instantiates k = 3 .. 17");
    if (k < 3 || k > MI355_MAX_MORPH_K || (k & 1) == 0 || op < 0 || op > 3)
        return hipErrorInvalidValue;
    return dispatch_int(op, std::make_integer_sequence<int, 4>{}, [&](auto OP) {
        return dispatch_int(k, std::integer_sequence<int, 3, 5, 7, 9, 11, 13, 15, 17>{}, [&](auto K) {
            constexpr int kc = decltype(K)::value, opc = decltype(OP)::value;
            return gray8 ? launch_k<true, kc, opc>(stream, d_in, d_out, w, h, nframes)
                         : launch_k<false, kc, opc>(stream, d_in, d_out, w, h, nframes);
        });
    });
}

}  // namespace mi355
