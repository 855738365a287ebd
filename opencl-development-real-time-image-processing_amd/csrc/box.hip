// box.hip — cv::blur with BORDER_REPLICATE (include/mi355_imgfilter.h, "Box mean") for RGBA and gray8 frames, and
// cv::adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) of gray8 frames as an epilogue of the same kernel.
//
// One kernel template over <gray8, epilogue>.  A work item is one wave walking one (frame, band of output rows, strip of
// columns) top down; a lane owns the 16 bytes of a row at its place: 4 RGBA pixels or 16 gray8 pixels (gray8 takes 16
// and not 4 so that both layouts move 16 bytes per lane and row and share every line below; at 4 a wave would move 256
// bytes per row and pay the same scan).  halo_lanes = r / PX + 1 lanes on each side of the strip hold the halo columns,
// the 64 - 2 halo_lanes lanes between them store.  Columns are clamped into the frame: a lane whose 16 bytes lie inside
// the row loads and stores them at once (RGBA dword-aligned, gray8 at any alignment), a halo lane wholly outside it loads
// the one edge pixel all its columns clamp to, and a lane across a row end goes pixel by pixel.
//   vertical    the column sums of the lane's 16 bytes, as u16 pairs in 8 registers (even bytes / odd bytes of each
//               dword: (R, B) and (G, A), or two pixels each; 63 * 255 < 65536).  A band starts by summing its k clamped
//               rows; every further row adds the entering row min(y + r, h - 1) and subtracts the leaving row
//               max(y - r - 1, 0), one u32 add and one u32 sub per pair (no field carries or borrows: the leaving row
//               is part of the sum).
//   horizontal  independent of k.  The lane scans its own columns, the wave scans the lane totals (one scan per
//               channel) with DPP row shifts and row broadcasts, and the inclusive prefix P of every column goes to the
//               wave's 4 KiB LDS row, column c of the strip at plane c % PX, lane c / PX (both the stores and the loads
//               of a plane are consecutive across lanes: no bank conflict).  window(x) = P[x + r] - P[x - r - 1], in u32
//               modulo 2^32 (a window is below 2^20, the prefix of a strip below 2^23).
//   division    box_common.hpp: one fp32 multiply by 1 / k^2 (from the host) and a round-to-nearest convert, exact.
//   threshold   the centre row is one more load; out = (src - mean > -idelta) ? on : off per pixel, in registers.
// Bands are kBoxBandPerK * k rows (at least kBoxBandFloor) so that the k start-up rows stay a fixed share, halved while
// the launch has fewer than kBoxMinWork waves.  No cross-workgroup synchronisation, no atomics, no allocation.
#include "box_common.hpp"
#include "wave_common.hpp"

namespace mi355 {

namespace {

constexpr int kBoxBandPerK = 4;           // rows of the tallest band per row of the window
constexpr int kBoxBandFloor = 32;         // ... and its least height
constexpr int kBoxBandMin = 4;            // halving stops here
constexpr size_t kBoxMinWork = 4096;      // ~4 waves per SIMD before bands grow

constexpr int kMean = 0, kThreshold = 1;

struct BoxArgs {
    const uint8_t* in;
    uint8_t* out;
    int w, h, r;
    int halo_lanes, strip_cols;
    int nstrips, nbands, band_rows;
    uint32_t nwork;
    float inv;       // box_inv(k)
    int thr;         // threshold: -idelta
    uint32_t on, off;  // threshold: the byte where src - mean > thr, and elsewhere
};

template <typename V>
__device__ __forceinline__ V gload_a1(global_ptr<const uint8_t> p)
{
    typedef V __attribute__((aligned(1))) VA;
    return *(global_ptr<const VA>)p;
}

// where a lane's 16 bytes lie: inside the row (one vector load), wholly outside it (every column clamps to the same edge
// column: one pixel, replicated — the halo lanes left of column 0 and right of column w - 1), or across a row end
enum LaneSpan { kInside, kOutside, kAcross };

// the 16 bytes of a row at the lane's columns x_lane .. x_lane + PX - 1, columns clamped into [0, w)
template <bool GRAY8>
__device__ __forceinline__ u32x4 box_load(global_ptr<const uint8_t> rowp, int x_lane, int w, LaneSpan span)
{
    u32x4 v;
    if (span == kInside) {
        if constexpr (GRAY8)
            v = gload_a1<u32x4>(rowp + (uint32_t)x_lane);
        else
            v = gload_a4<u32x4>(rowp + (uint32_t)x_lane * 4u);
    } else if (span == kOutside) {
        const uint32_t xe = x_lane < 0 ? 0u : (uint32_t)(w - 1);
        uint32_t p;
        if constexpr (GRAY8)
            p = (uint32_t)gload<uint8_t>(rowp + xe) * 0x01010101u;
        else
            p = gload<uint32_t>(rowp + xe * 4u);
        v = u32x4{p, p, p, p};
    } else if constexpr (GRAY8) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] = 0u;
#pragma unroll
            for (int b = 0; b < 4; b++)
                v[j] |= (uint32_t)gload<uint8_t>(rowp + (uint32_t)clampi(x_lane + 4 * j + b, 0, w - 1)) << (8 * b);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[j] = gload<uint32_t>(rowp + (uint32_t)clampi(x_lane + j, 0, w - 1) * 4u);
    }
    return v;
}

// lane l <- the DPP source lane's value, 0 where that lane does not exist or the row is masked out
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}

// inclusive prefix sum across the 64 lanes: row_shr 1, 2, 4, 8 inside each row of 16, then row_bcast:15 into rows 1 and
// 3 and row_bcast:31 into rows 2 and 3
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v)
{
    v += dpp_or_zero<0x111, 0xF>(v);
    v += dpp_or_zero<0x112, 0xF>(v);
    v += dpp_or_zero<0x114, 0xF>(v);
    v += dpp_or_zero<0x118, 0xF>(v);
    v += dpp_or_zero<0x142, 0xA>(v);
    v += dpp_or_zero<0x143, 0xC>(v);
    return v;
}

template <bool GRAY8, int EPI>
__global__ __launch_bounds__(kItemWaves* kWave) void box_kernel(const BoxArgs a)
{
    static_assert(GRAY8 || EPI == kMean, "the threshold is gray8 only");
    constexpr int PX = GRAY8 ? 16 : 4, LOG_PX = GRAY8 ? 4 : 2;  // columns per lane
    constexpr int CH = 16 / PX;                                  // channels = bytes per pixel
    using PVec = typename std::conditional<GRAY8, uint32_t, u32x4>::type;  // the CH prefixes of one column
    __shared__ __attribute__((aligned(16))) uint32_t prefix_rows[kItemWaves][16 * kWave];

    const int wave = threadIdx.x >> 6;
    WaveItem it;
    if (!wave_item(blockIdx.x, a.nwork, a.nstrips, a.nbands, 6, a.band_rows, a.h, &it))  // it.x0 unused: halo lanes
        return;
    const int lane = threadIdx.x & 63;
    const int strip = it.tx, y0 = it.y0, y1 = it.y_end;
    const size_t frame = it.frame;
    const int r = a.r;
    const int x_lane = strip * a.strip_cols + (lane - a.halo_lanes) * PX;
    const LaneSpan span = (x_lane >= 0 && x_lane + PX <= a.w) ? kInside
                          : (x_lane + PX <= 0 || x_lane >= a.w)  ? kOutside
                                                                 : kAcross;
    const bool stores = lane >= a.halo_lanes && lane < kWave - a.halo_lanes && x_lane < a.w;
    const size_t row_bytes = (size_t)a.w * CH;
    const uint8_t* src = a.in + frame * (row_bytes * (size_t)a.h);
    uint8_t* dst = a.out + frame * (row_bytes * (size_t)a.h);
    auto row = [&](int y) { return box_load<GRAY8>(uniform_ptr(src + (size_t)y * row_bytes), x_lane, a.w, span); };

    // where the prefixes of columns x + r and x - r - 1 of the lane's columns lie in the wave's LDS row (dword index);
    // halo lanes, which store nothing, clamp into the row
    PVec* const prow = reinterpret_cast<PVec*>(prefix_rows[wave]);
    auto slot = [](int c) {
        c = clampi(c, 0, kWave * PX - 1);
        return (c & (PX - 1)) * kWave + (c >> LOG_PX);
    };

    // column sums of the band's first window: rows y0 - r .. y0 + r, clamped
    uint32_t even[4] = {0u, 0u, 0u, 0u}, odd[4] = {0u, 0u, 0u, 0u};
    for (int dy = -r; dy <= r; dy++) {
        const u32x4 v = row(clampi(y0 + dy, 0, a.h - 1));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            even[j] += v[j] & 0x00FF00FFu;
            odd[j] += (v[j] >> 8) & 0x00FF00FFu;
        }
    }

    for (int y = y0; y < y1; y++) {
        // the rows the NEXT output row needs, in flight during this row's horizontal pass (clamped: always loadable)
        const u32x4 enter = row(min(y + 1 + r, a.h - 1));
        const u32x4 leave = row(max(y - r, 0));
        u32x4 centre;
        if constexpr (EPI == kThreshold)
            centre = row(y);

        // S[4 j + b]: the sum under byte b of dword j — RGBA: column j, channel b; gray8: column 4 j + b
        uint32_t S[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            S[4 * j + 0] = even[j] & 0xFFFFu;
            S[4 * j + 1] = odd[j] & 0xFFFFu;
            S[4 * j + 2] = even[j] >> 16;
            S[4 * j + 3] = odd[j] >> 16;
        }
        // the lane's own columns, then the lanes to its left
#pragma unroll
        for (int u = CH; u < 16; u++)
            S[u] += S[u - CH];
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const uint32_t total = S[16 - CH + c];
            const uint32_t before = wave_scan_add(total) - total;
#pragma unroll
            for (int u = c; u < 16; u += CH)
                S[u] += before;
        }
#pragma unroll
        for (int col = 0; col < PX; col++) {
            if constexpr (GRAY8)
                prow[col * kWave + lane] = S[col];
            else
                prow[col * kWave + lane] = u32x4{S[4 * col], S[4 * col + 1], S[4 * col + 2], S[4 * col + 3]};
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t win[16];
#pragma unroll
        for (int col = 0; col < PX; col++) {
            const PVec hi = prow[slot(lane * PX + col + r)];
            const PVec lo = prow[slot(lane * PX + col - r - 1)];
            if constexpr (GRAY8) {
                win[col] = hi - lo;
            } else {
#pragma unroll
                for (int c = 0; c < 4; c++)
                    win[4 * col + c] = hi[c] - lo[c];
            }
        }
        // the next row's prefixes overwrite this LDS row
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();

        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if constexpr (EPI == kMean) {
                o[u / 4] = box_mean_pack(win[u], a.inv, u % 4, o[u / 4]);
            } else {
                const int s = (int)((centre[u / 4] >> (8 * (u % 4))) & 0xFFu);
                const int mean = (int)box_mean(win[u], a.inv);
                o[u / 4] |= (s - mean > a.thr ? a.on : a.off) << (8 * (u % 4));
            }
        }
        if (stores) {
            const global_ptr<uint8_t> rowp = uniform_ptr(dst + (size_t)y * row_bytes);
            if (x_lane + PX <= a.w) {
                if constexpr (GRAY8)
                    gstore_a1<u32x4>(rowp + (uint32_t)x_lane, o);
                else
                    gstore_a4<u32x4>(rowp + (uint32_t)x_lane * 4u, o);
            } else if constexpr (GRAY8) {
#pragma unroll
                for (int u = 0; u < 16; u++)
                    if (x_lane + u < a.w)
                        rowp[(uint32_t)(x_lane + u)] = (uint8_t)(o[u / 4] >> (8 * (u % 4)));
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (x_lane + j < a.w)
                        gstore_a4<uint32_t>(rowp + (uint32_t)(x_lane + j) * 4u, o[j]);
            }
        }

#pragma unroll
        for (int j = 0; j < 4; j++) {
            even[j] = even[j] + (enter[j] & 0x00FF00FFu) - (leave[j] & 0x00FF00FFu);
            odd[j] = odd[j] + ((enter[j] >> 8) & 0x00FF00FFu) - ((leave[j] >> 8) & 0x00FF00FFu);
        }
    }
}

bool box_plan(const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k, bool gray8, BoxArgs* out)
{
    if (k < 3 || k > kBoxMaxK || (k & 1) == 0 || w <= 0 || h <= 0 || nframes <= 0)
        return false;
    if ((size_t)w * 4 > 0x7FFFFFFFull)  // lane offsets inside a row are 32-bit
        return false;
    const int px = gray8 ? 16 : 4;
    BoxArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.w = w;
    a.h = h;
    a.r = k / 2;
    a.halo_lanes = a.r / px + 1;
    a.strip_cols = (kWave - 2 * a.halo_lanes) * px;
    a.nstrips = (w + a.strip_cols - 1) / a.strip_cols;
    a.inv = box_inv(k);
    a.band_rows = kBoxBandPerK * k > kBoxBandFloor ? kBoxBandPerK * k : kBoxBandFloor;
    auto nwork = [&](int rows) { return band_items(a.nstrips, h, rows, nframes); };
    while (a.band_rows / 2 >= kBoxBandMin && nwork(a.band_rows) < kBoxMinWork)
        a.band_rows /= 2;
    if (!plan_bands(&a, h, nframes))
        return false;
    *out = a;
    return true;
}

}  // namespace

hipError_t launch_box(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes, int k,
                      bool gray8)
{
    BoxArgs a;
    if (!box_plan(d_in, d_out, w, h, nframes, k, gray8, &a))
        return hipErrorInvalidValue;
    return dispatch_bool(gray8, [&](auto GRAY8) { return launch_items(box_kernel<GRAY8.value, kMean>, stream, a); });
}

hipError_t launch_adaptive_threshold(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, int w, int h, int nframes,
                                     int block, int max_value, bool inverse, int idelta)
{
    BoxArgs a;
    if (!box_plan(d_in, d_out, w, h, nframes, block, true, &a) || max_value < 0 || max_value > 255)
        return hipErrorInvalidValue;
    a.thr = -idelta;
    a.on = inverse ? 0u : (uint32_t)max_value;
    a.off = inverse ? (uint32_t)max_value : 0u;
    return launch_items(box_kernel<true, kThreshold>, stream, a);
}

}  // namespace mi355
