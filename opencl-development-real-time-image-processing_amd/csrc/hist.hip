// hist.hip — whole-frame statistics of single-channel frames: the 256-bin histogram (cv::calcHist), histogram
// equalization (MI355_FILTER_EQUALIZE_GRAY8, cv::equalizeHist) and Otsu thresholding (MI355_FILTER_OTSU_GRAY8,
// cv::threshold(THRESH_BINARY | THRESH_OTSU)).  Semantics: include/mi355_imgfilter.h.
//
// Every frame is the flat byte range [f * npx, (f + 1) * npx), npx = w * h < 2^31.  The three launches, the block
// histogram frame, the byte-range walk and the table scan are hist_common.hpp's, the grid mask_common.hpp's:
//   hist_kernel   256 x kHistVec vectors of a frame's body per block, aligned on the input; head and tail in its first;
//   table_kernel  one wave per frame makes its histogram a 256-byte table (LUT).  Equalize: the table scan from the
//                 first occupied bin.  Otsu: OpenCV's serial fp64 loop in one lane, operation by operation (no fused
//                 multiply-add; the fp64 divisions are the IEEE correctly rounded sequence), then lut[v] = v > t;
//   apply_kernel  the frame's LUT in LDS, one ds_read_u8 per pixel; 256 x kApplyVec vectors per block, aligned on the
//                 output (non-temporal stores).
#include "common.hpp"
#include "hist_common.hpp"
#include "kernels.hpp"
#include "tile_common.hpp"

#include <cfloat>

namespace mi355 {

namespace {

__global__ __launch_bounds__(kHistThreads) void hist_kernel(const uint8_t* __restrict__ in, uint32_t* __restrict__ hist,
                                                            uint32_t npx, uint32_t tiles)
{
    __shared__ uint32_t sh[kHistWaves * 256];
    const int tid = threadIdx.x;
    uint32_t* hw = block_hists_begin(sh);
    const auto [f, tile, j0] = frame_block(tiles, kHistThreads * kHistVec);
    const uint8_t* p = in + (size_t)f * npx;
    const ByteRange r = byte_range(p, npx);
    const u32x4* vp = reinterpret_cast<const u32x4*>(p + r.head);
#pragma unroll
    for (int u0 = 0; u0 < kHistVec; u0 += 4) {
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t j = j0 + (u0 + u) * kHistThreads;
            v[u] = j < r.nvec ? __builtin_nontemporal_load(vp + j) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            count_vec(hw, v[u], j0 + (u0 + u) * kHistThreads < r.nvec);
    }
    if (tile == 0)
        for_edge_byte(r, npx, tid, [&](uint32_t e) { lds_add(hw, p[e], 1); });
    block_hists_flush(sh, hist + (size_t)f * 256);
}

// OpenCV's getThreshVal_Otsu_8u loop (include/mi355_imgfilter.h), one lane; h = the frame's 256 counts in LDS
__device__ int otsu_threshold(const uint32_t* h, uint32_t total, double mu)
{
    const double scale = 1.0 / (double)total;
    mu *= scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int t = 0;
    const double eps = (double)FLT_EPSILON;
    for (int i = 0; i < 256; i++) {
        const double p = (double)h[i] * scale;
        mu1 *= q1;
        q1 += p;
        const double q2 = 1.0 - q1;
        const double lo = q2 < q1 ? q2 : q1, hi = q1 < q2 ? q2 : q1;  // std::min / std::max
        if (lo < eps || hi > 1.0 - eps)
            continue;
        mu1 = (mu1 + (double)i * p) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double d = mu1 - mu2;
        const double sigma = q1 * q2 * d * d;
        if (sigma > max_sigma) {
            max_sigma = sigma;
            t = i;
        }
    }
    return t;
}

// one wave per frame; lut may be null (thresholds only), thresh may be null (Otsu without reporting t)
__global__ __launch_bounds__(kWave) void table_kernel(const uint32_t* __restrict__ hist, uint8_t* __restrict__ lut,
                                                      int32_t* __restrict__ thresh, uint32_t total, int otsu)
{
    __shared__ uint32_t sh[256];
    __shared__ int s_t;
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const u32x4 hv = reinterpret_cast<const u32x4*>(hist + (size_t)f * 256)[lane];  // bins 4 lane .. 4 lane + 3
    uint32_t out = 0;
    if (!otsu) {
        // i0 = the first occupied bin (there is one: total >= 1)
        const uint64_t nz = __ballot((hv.x | hv.y | hv.z | hv.w) != 0);
        const int l0 = __ffsll((unsigned long long)nz) - 1;
        const int j_own = hv.x ? 0 : (hv.y ? 1 : (hv.z ? 2 : 3));
        const uint32_t c_own = hv.x ? hv.x : (hv.y ? hv.y : (hv.z ? hv.z : hv.w));
        const int i0 = 4 * l0 + __builtin_amdgcn_readlane(j_own, l0);
        const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)c_own, l0);
        if (h0 == total) {
            out = (uint32_t)i0 * 0x01010101u;
        } else {
            const float scale = 255.0f / (float)(int)(total - h0);
            uint32_t c = bins_below(hv, lane);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c += hv[j];
                // bin i > i0: the sum of the bins i0 + 1 .. i (the bins below i0 are empty)
                out |= (4 * lane + j > i0 ? table_byte(c - h0, scale) : 0u) << (8 * j);
            }
        }
    } else {
        // mu = sum i * hist[i]: every partial sum is an integer below 2^53, so the serial double sum is this exact
        // integer whatever the order of the additions
        uint64_t m = (uint64_t)(4 * lane) * hv.x + (uint64_t)(4 * lane + 1) * hv.y + (uint64_t)(4 * lane + 2) * hv.z +
                     (uint64_t)(4 * lane + 3) * hv.w;
#pragma unroll
        for (int d = kWave / 2; d >= 1; d /= 2)
            m += __shfl_xor(m, d);
        reinterpret_cast<u32x4*>(sh)[lane] = hv;
        __syncthreads();
        if (lane == 0) {
            const int t = otsu_threshold(sh, total, (double)m);
            s_t = t;
            if (thresh)
                thresh[f] = t;
        }
        __syncthreads();
        const int t = s_t;
#pragma unroll
        for (int j = 0; j < 4; j++)
            out |= (4 * lane + j > t ? 0xFFu : 0u) << (8 * j);
    }
    if (lut)
        reinterpret_cast<uint32_t*>(lut + (size_t)f * 256)[lane] = out;
}

__device__ __forceinline__ uint32_t lut_dword(const uint8_t* sl, uint32_t d)
{
    return (uint32_t)sl[d & 0xFFu] | ((uint32_t)sl[(d >> 8) & 0xFFu] << 8) | ((uint32_t)sl[(d >> 16) & 0xFFu] << 16) |
           ((uint32_t)sl[d >> 24] << 24);
}

__global__ __launch_bounds__(kHistThreads) void apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                             const uint8_t* __restrict__ lut, uint32_t npx,
                                                             uint32_t tiles)
{
    __shared__ uint8_t sl[256];
    const int tid = threadIdx.x;
    const auto [f, tile, j0] = frame_block(tiles, kHistThreads * kApplyVec);
    sl[tid] = lut[(size_t)f * 256 + tid];
    __syncthreads();
    const uint8_t* p = in + (size_t)f * npx;
    uint8_t* q = out + (size_t)f * npx;
    const ByteRange r = byte_range(q, npx);
    u32x4 v[kApplyVec];
#pragma unroll
    for (int u = 0; u < kApplyVec; u++) {
        const uint32_t j = j0 + u * kHistThreads;
        if (j < r.nvec)
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a1*>(p + r.head + 16 * (size_t)j));
    }
#pragma unroll
    for (int u = 0; u < kApplyVec; u++) {
        const uint32_t j = j0 + u * kHistThreads;
        if (j < r.nvec) {
            const u32x4 o = {lut_dword(sl, v[u].x), lut_dword(sl, v[u].y), lut_dword(sl, v[u].z), lut_dword(sl, v[u].w)};
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(q + r.head) + j);
        }
    }
    if (tile == 0)
        for_edge_byte(r, npx, tid, [&](uint32_t e) { q[e] = sl[p[e]]; });
}

// the grid for `per_block` 16-byte vectors of a frame per block; not ok if the sizes are refused or it is too large
FrameGrid grid_of(int w, int h, int nframes, int per_block)
{
    const uint64_t nvec = (uint64_t)w * (uint64_t)h / 16;  // a frame shorter than one has its head / tail block all the same
    return hist_frames_ok(w, h, nframes) ? frame_grid(nvec ? nvec : 1, per_block, nframes) : FrameGrid{};
}

}  // namespace

hipError_t launch_hist(hipStream_t stream, const uint8_t* d_in, uint32_t* d_hist, int w, int h, int nframes)
{
    const FrameGrid g = grid_of(w, h, nframes, kHistThreads * kHistVec);
    if (!g.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hist_kernel, dim3(g.blocks), dim3(kHistThreads), 0, stream, d_in, d_hist, (uint32_t)(w * h),
                       g.bpf);
    return hipGetLastError();
}

hipError_t launch_hist_table(hipStream_t stream, const uint32_t* d_hist, uint8_t* d_lut, int32_t* d_thresh, int w,
                             int h, int nframes, bool otsu)
{
    if (!hist_frames_ok(w, h, nframes))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(table_kernel, dim3((unsigned)nframes), dim3(kWave), 0, stream, d_hist, d_lut, d_thresh,
                       (uint32_t)(w * h), otsu ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_lut_apply(hipStream_t stream, const uint8_t* d_in, uint8_t* d_out, const uint8_t* d_lut, int w, int h,
                            int nframes)
{
    const FrameGrid g = grid_of(w, h, nframes, kHistThreads * kApplyVec);
    if (!g.ok)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(apply_kernel, dim3(g.blocks), dim3(kHistThreads), 0, stream, d_in, d_out, d_lut, (uint32_t)(w * h),
                       g.bpf);
    return hipGetLastError();
}

}  // namespace mi355
