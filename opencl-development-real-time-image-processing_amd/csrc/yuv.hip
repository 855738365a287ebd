// yuv.hip — 8-bit YUV (NV12 / NV21 / I420 / YV12 / YUY2 / UYVY) <-> RGBA and the luma plane of such frames.
// Semantics: include/mi355_imgfilter.h, "frames from a decoder or a camera".  All arithmetic is int32; every constant is
// below 2^23 in magnitude and every other factor is a byte or a byte minus 128, so each product is exact in the full-rate
// 24-bit multiply (v_mul_i32_i24 / v_mad_i32_i24).
//
// Lane geometry.  A lane owns 8 consecutive pixels of a row pair (4:2:0) or of one row (packed), the chroma of which is
// shared by construction: a 2 x 2 block never straddles two lanes.  4:2:0 decode = two 8-byte luma loads, one 8-byte
// (semi-planar) or two 4-byte (planar) chroma loads and four 16-byte RGBA stores; the encode is its mirror image.  A wave
// covers 512 pixels of a row (pair): every load and store instruction of a wave touches one contiguous span.
// Work items are numbered inside a frame (row pair major), frames go over blockIdx.y; all byte offsets are size_t.
// The fast path wants the whole 8 pixels inside the row and 8-byte aligned luma / chroma addresses (base and pitch
// multiples of 8), and for the 16-byte RGBA accesses a 16-byte aligned base with w % 4 == 0; it is chosen per launch for
// the alignment and per lane for the row tail.  Every other lane takes byte accesses for the YUV side and dword accesses
// for the RGBA side, in the same launch, with the same arithmetic.  Only bytes of pixels are ever stored: the padding of
// a pitched surface is never written.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355 {

namespace {

constexpr int kThreads = 256;
constexpr int kPx = 8;  // pixels of a row per lane

enum { SEMI = 0, PLANAR = 1, PACKED = 2 };

// what a launch knows about its surface, by value
struct YuvGeom {
    int w, h;
    uint32_t ngx;        // lanes per row: ceil(w / 8)
    uint64_t items;      // work items per frame
    size_t pitch;        // luma (or packed) row stride in bytes
    size_t chroma_at;    // offset of the chroma area in a frame: rows * pitch
    size_t plane2_at;    // planar: offset of the second chroma plane
    size_t frame_bytes;  // distance between frames
    int yuv8;            // YUV side: 8-byte accesses are aligned for every full lane
    int rgba16;          // RGBA side: 16-byte accesses are aligned for every full lane
    int nframes;
};

// sat(v >> 20), clamped BEFORE the shift.  The plain form, clamp((v >> 20), 0, 255) packed two to a register, is selected
// as v_ashr_pk_u8_i32 by the compiler, which then ORs the blue byte into bits 16-23 of that result as if they were zero;
// on the MI355X they came back holding bits 16-23 of the destination's previous value (the red sum) and every blue byte
// was wrong by those bits (found by tests/test_gpu_yuv.py, the first run of this kernel).  Clamping the 28-bit value first
// gives the same byte and does not match that pattern.
__device__ __forceinline__ uint32_t sat_shr20(int v) { return (uint32_t)clampi(v, 0, (256 << 20) - 1) >> 20; }

// the work item of this lane inside a frame -> (row or row pair, first pixel); false past the end
__device__ __forceinline__ bool item_of(const YuvGeom& g, uint64_t i, uint32_t* row, int* x0)
{
    if (i >= g.items)
        return false;
    if (g.items >> 32) {  // frames of more than 2^32 items (a few 10^10 pixels two wide): the long division
        const uint64_t r = i / g.ngx;
        *row = (uint32_t)r;
        *x0 = (int)(i - r * g.ngx) * kPx;
    } else {
        const uint32_t r = (uint32_t)i / g.ngx;
        *row = r;
        *x0 = (int)((uint32_t)i - r * g.ngx) * kPx;
    }
    return true;
}

__device__ __forceinline__ u32x2 load8(const uint8_t* p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
}

// n (<= 8) bytes at p into the low bytes of two dwords, the rest 0
__device__ __forceinline__ u32x2 load_bytes(const uint8_t* p, int n)
{
    u32x2 v = {0u, 0u};
    for (int j = 0; j < n; j++) {
        const uint32_t b = p[j];
        if (j < 4)
            v.x |= b << (8 * j);
        else
            v.y |= b << (8 * (j - 4));
    }
    return v;
}

__device__ __forceinline__ void store_bytes(uint8_t* p, u32x2 v, int n)
{
    for (int j = 0; j < n; j++)
        p[j] = (uint8_t)((j < 4 ? v.x >> (8 * j) : v.y >> (8 * (j - 4))) & 0xFFu);
}

__device__ __forceinline__ uint32_t byte_of(const u32x2& v, int j)
{
    return ((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xFFu;
}

// ---- decode ----------------------------------------------------------------------------------------------------------
// One row of 8 pixels from 8 luma bytes and the three chroma terms of its 4 pixel pairs.
__device__ __forceinline__ void decode_row(const YuvDecodeCoef& c, const u32x2& yv, const int rv[4], const int gv[4],
                                           const int bu[4], uint32_t px[kPx])
{
#pragma unroll
    for (int j = 0; j < kPx; j++) {
        const int yl = max((int)byte_of(yv, j) - c.yoff, 0);
        const int y = __mul24(yl, c.cy) + (1 << 19);
        const uint32_t r = sat_shr20(y + rv[j >> 1]);
        const uint32_t g = sat_shr20(y + gv[j >> 1]);
        const uint32_t b = sat_shr20(y + bu[j >> 1]);
        px[j] = r | (g << 8) | (b << 16) | 0xFF000000u;
    }
}

__device__ __forceinline__ void chroma_terms(const YuvDecodeCoef& c, const uint32_t ub[4], const uint32_t vb[4],
                                             int rv[4], int gv[4], int bu[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int u = (int)ub[j] - 128, v = (int)vb[j] - 128;
        rv[j] = __mul24(c.cvr, v);
        gv[j] = __mul24(c.cvg, v) + __mul24(c.cug, u);
        bu[j] = __mul24(c.cub, u);
    }
}

__device__ __forceinline__ void store_px(uint32_t* dst, const uint32_t px[kPx], int n, bool wide)
{
    if (wide) {
        const u32x4 a = {px[0], px[1], px[2], px[3]}, b = {px[4], px[5], px[6], px[7]};
        __builtin_nontemporal_store(a, reinterpret_cast<u32x4*>(dst));
        __builtin_nontemporal_store(b, reinterpret_cast<u32x4*>(dst) + 1);
    } else {
#pragma unroll
        for (int j = 0; j < kPx; j++)
            if (j < n)
                dst[j] = px[j];
    }
}

// CLS SEMI / PLANAR: a lane owns 8 pixels of two rows.  SWAP: V comes first (NV21, YV12).
template <int CLS, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv420_decode_kernel(const uint8_t* __restrict__ yuv,
                                                                 uint32_t* __restrict__ rgba, YuvGeom g, YuvDecodeCoef c)
{
    uint32_t rp;
    int x0;
    if (!item_of(g, (uint64_t)blockIdx.x * kThreads + threadIdx.x, &rp, &x0))
        return;
    const int n = min(kPx, g.w - x0);  // even, >= 2
    const bool full = n == kPx;
    const size_t frame_px = (size_t)g.w * g.h;
    for (int f = blockIdx.y; f < g.nframes; f += gridDim.y) {
        const uint8_t* fr = yuv + (size_t)f * g.frame_bytes;
        const uint8_t* y0 = fr + (size_t)(2 * (size_t)rp) * g.pitch + x0;
        const uint8_t* y1 = y0 + g.pitch;
        u32x2 ya, yb;
        uint32_t ub[4], vb[4];
        if (full && g.yuv8) {
            ya = load8(y0);
            yb = load8(y1);
            if (CLS == SEMI) {
                const u32x2 cv = load8(fr + g.chroma_at + (size_t)rp * g.pitch + x0);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t d = j < 2 ? cv.x : cv.y;
                    ub[j] = (d >> (16 * (j & 1))) & 0xFFu;
                    vb[j] = (d >> (16 * (j & 1) + 8)) & 0xFFu;
                }
            } else {
                const uint8_t* p1 = fr + g.chroma_at + (size_t)rp * (g.pitch >> 1) + (x0 >> 1);
                const uint32_t a = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p1));
                const uint32_t b = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p1 + (g.plane2_at - g.chroma_at)));
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    ub[j] = (a >> (8 * j)) & 0xFFu;
                    vb[j] = (b >> (8 * j)) & 0xFFu;
                }
            }
        } else {
            ya = load_bytes(y0, n);
            yb = load_bytes(y1, n);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                ub[j] = vb[j] = 128u;
                if (2 * j < n) {
                    if (CLS == SEMI) {
                        const uint8_t* p = fr + g.chroma_at + (size_t)rp * g.pitch + x0 + 2 * j;
                        ub[j] = p[0];
                        vb[j] = p[1];
                    } else {
                        const uint8_t* p = fr + g.chroma_at + (size_t)rp * (g.pitch >> 1) + (x0 >> 1) + j;
                        ub[j] = p[0];
                        vb[j] = p[g.plane2_at - g.chroma_at];
                    }
                }
            }
        }
        int rv[4], gv[4], bu[4];
        if (SWAP)
            chroma_terms(c, vb, ub, rv, gv, bu);
        else
            chroma_terms(c, ub, vb, rv, gv, bu);
        uint32_t px[kPx];
        uint32_t* o0 = rgba + (size_t)f * frame_px + (size_t)(2 * (size_t)rp) * g.w + x0;
        decode_row(c, ya, rv, gv, bu, px);
        store_px(o0, px, n, full && g.rgba16);
        decode_row(c, yb, rv, gv, bu, px);
        store_px(o0 + g.w, px, n, full && g.rgba16);
    }
}

// Packed 4:2:2: a lane owns 8 pixels = 16 bytes of one row.  SWAP: chroma comes first (UYVY).
template <bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv422_decode_kernel(const uint8_t* __restrict__ yuv,
                                                                 uint32_t* __restrict__ rgba, YuvGeom g, YuvDecodeCoef c)
{
    uint32_t row;
    int x0;
    if (!item_of(g, (uint64_t)blockIdx.x * kThreads + threadIdx.x, &row, &x0))
        return;
    const int n = min(kPx, g.w - x0);
    const bool full = n == kPx;
    const size_t frame_px = (size_t)g.w * g.h;
    for (int f = blockIdx.y; f < g.nframes; f += gridDim.y) {
        const uint8_t* p = yuv + (size_t)f * g.frame_bytes + (size_t)row * g.pitch + 2 * (size_t)x0;
        uint32_t d[4];  // one dword per pixel pair
        if (full && g.yuv8) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                d[j] = 0x80808080u;
                if (2 * j < n)
                    d[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) | ((uint32_t)p[4 * j + 2] << 16) |
                           ((uint32_t)p[4 * j + 3] << 24);
            }
        }
        u32x2 yv = {0u, 0u};
        uint32_t ub[4], vb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = SWAP ? d[j] >> 8 : d[j];  // luma in bytes 0 and 2
            const uint32_t k = SWAP ? d[j] : d[j] >> 8;  // U in byte 0, V in byte 2
            const uint32_t two = (q & 0xFFu) | ((q >> 8) & 0xFF00u);
            if (j < 2)
                yv.x |= two << (16 * j);
            else
                yv.y |= two << (16 * (j - 2));
            ub[j] = k & 0xFFu;
            vb[j] = (k >> 16) & 0xFFu;
        }
        int rv[4], gv[4], bu[4];
        chroma_terms(c, ub, vb, rv, gv, bu);
        uint32_t px[kPx];
        decode_row(c, yv, rv, gv, bu, px);
        store_px(rgba + (size_t)f * frame_px + (size_t)row * g.w + x0, px, n, full && g.rgba16);
    }
}

// ---- luma ------------------------------------------------------------------------------------------------------------
// The Y bytes of every frame, unchanged, into tightly packed (n, h, w) planes; a lane owns 8 pixels of one row.
// g.yuv8: aligned 8-byte (16-byte for packed) loads; g.rgba16 here: aligned 8-byte stores.
template <bool PACKED_LAYOUT, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv_luma_kernel(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ gray,
                                                            YuvGeom g)
{
    uint32_t row;
    int x0;
    if (!item_of(g, (uint64_t)blockIdx.x * kThreads + threadIdx.x, &row, &x0))
        return;
    const int n = min(kPx, g.w - x0);
    const bool full = n == kPx;
    const size_t frame_px = (size_t)g.w * g.h;
    for (int f = blockIdx.y; f < g.nframes; f += gridDim.y) {
        const uint8_t* p = yuv + (size_t)f * g.frame_bytes + (size_t)row * g.pitch + (PACKED_LAYOUT ? 2 : 1) * (size_t)x0;
        u32x2 yv = {0u, 0u};
        if (!PACKED_LAYOUT) {
            yv = (full && g.yuv8) ? load8(p) : load_bytes(p, n);
        } else if (full && g.yuv8) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t q = SWAP ? d[j] >> 8 : d[j];
                const uint32_t two = (q & 0xFFu) | ((q >> 8) & 0xFF00u);
                if (j < 2)
                    yv.x |= two << (16 * j);
                else
                    yv.y |= two << (16 * (j - 2));
            }
        } else {
            for (int j = 0; j < n; j++) {
                const uint32_t b = p[2 * j + (SWAP ? 1 : 0)];
                if (j < 4)
                    yv.x |= b << (8 * j);
                else
                    yv.y |= b << (8 * (j - 4));
            }
        }
        uint8_t* o = gray + (size_t)f * frame_px + (size_t)row * g.w + x0;
        if (full && g.rgba16)
            __builtin_nontemporal_store(yv, reinterpret_cast<u32x2*>(o));
        else
            store_bytes(o, yv, n);
    }
}

// ---- encode ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_px(const uint32_t* src, uint32_t px[kPx], int n, bool wide)
{
    if (wide) {
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
        const u32x4 b = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + 1);
        px[0] = a.x, px[1] = a.y, px[2] = a.z, px[3] = a.w;
        px[4] = b.x, px[5] = b.y, px[6] = b.z, px[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; j++)
            px[j] = j < n ? src[j] : 0u;
    }
}

__device__ __forceinline__ u32x2 encode_luma(const YuvEncodeCoef& c, const uint32_t px[kPx])
{
    u32x2 yv = {0u, 0u};
#pragma unroll
    for (int j = 0; j < kPx; j++) {
        const int r = px[j] & 0xFFu, g = (px[j] >> 8) & 0xFFu, b = (px[j] >> 16) & 0xFFu;
        const uint32_t y = sat_shr20(__mul24(c.cry, r) + __mul24(c.cgy, g) + __mul24(c.cby, b) + c.ybias);
        if (j < 4)
            yv.x |= y << (8 * j);
        else
            yv.y |= y << (8 * (j - 4));
    }
    return yv;
}

// A lane owns 8 pixels of two rows; U and V come from the top-left pixel of each 2 x 2 block.  SWAP: V first.
template <int CLS, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv420_encode_kernel(const uint32_t* __restrict__ rgba,
                                                                 uint8_t* __restrict__ yuv, YuvGeom g, YuvEncodeCoef c)
{
    uint32_t rp;
    int x0;
    if (!item_of(g, (uint64_t)blockIdx.x * kThreads + threadIdx.x, &rp, &x0))
        return;
    const int n = min(kPx, g.w - x0);
    const bool full = n == kPx;
    const size_t frame_px = (size_t)g.w * g.h;
    const int cbias = (1 << 19) + (128 << 20);
    for (int f = blockIdx.y; f < g.nframes; f += gridDim.y) {
        const uint32_t* s0 = rgba + (size_t)f * frame_px + (size_t)(2 * (size_t)rp) * g.w + x0;
        uint32_t p0[kPx], p1[kPx];
        load_px(s0, p0, n, full && g.rgba16);
        load_px(s0 + g.w, p1, n, full && g.rgba16);
        const u32x2 ya = encode_luma(c, p0), yb = encode_luma(c, p1);
        uint32_t first = 0u, second = 0u;  // 4 bytes each, in storage order
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = p0[2 * j];
            const int r = q & 0xFFu, gg = (q >> 8) & 0xFFu, b = (q >> 16) & 0xFFu;
            const uint32_t u = sat_shr20(__mul24(c.cru, r) + __mul24(c.cgu, gg) + __mul24(c.cbu, b) + cbias);
            const uint32_t v = sat_shr20(__mul24(c.cbu, r) + __mul24(c.cgv, gg) + __mul24(c.cbv, b) + cbias);
            first |= (SWAP ? v : u) << (8 * j);
            second |= (SWAP ? u : v) << (8 * j);
        }
        uint8_t* fr = yuv + (size_t)f * g.frame_bytes;
        uint8_t* y0 = fr + (size_t)(2 * (size_t)rp) * g.pitch + x0;
        const bool wide = full && g.yuv8;
        if (wide) {
            __builtin_nontemporal_store(ya, reinterpret_cast<u32x2*>(y0));
            __builtin_nontemporal_store(yb, reinterpret_cast<u32x2*>(y0 + g.pitch));
        } else {
            store_bytes(y0, ya, n);
            store_bytes(y0 + g.pitch, yb, n);
        }
        if (CLS == SEMI) {
            u32x2 cv;  // interleave: first0 second0 first1 second1 | ...
            cv.x = (first & 0xFFu) | ((second & 0xFFu) << 8) | ((first & 0xFF00u) << 8) | ((second & 0xFF00u) << 16);
            cv.y = ((first >> 16) & 0xFFu) | (((second >> 16) & 0xFFu) << 8) | ((first >> 24) << 16) | ((second >> 24) << 24);
            uint8_t* pc = fr + g.chroma_at + (size_t)rp * g.pitch + x0;
            if (wide)
                __builtin_nontemporal_store(cv, reinterpret_cast<u32x2*>(pc));
            else
                store_bytes(pc, cv, n);
        } else {
            uint8_t* p1c = fr + g.chroma_at + (size_t)rp * (g.pitch >> 1) + (x0 >> 1);
            uint8_t* p2c = p1c + (g.plane2_at - g.chroma_at);
            if (wide) {
                __builtin_nontemporal_store(first, reinterpret_cast<uint32_t*>(p1c));
                __builtin_nontemporal_store(second, reinterpret_cast<uint32_t*>(p2c));
            } else {
                const u32x2 a = {first, 0u}, b = {second, 0u};
                store_bytes(p1c, a, n >> 1);
                store_bytes(p2c, b, n >> 1);
            }
        }
    }
}

// the geometry of a launch over `rows_of_items` rows (or row pairs) of ceil(w / 8) lanes each
YuvGeom geom_of(const YuvFrames& s, size_t rows_of_items)
{
    YuvGeom g;
    g.w = s.w;
    g.h = s.h;
    g.ngx = (uint32_t)((s.w + kPx - 1) / kPx);
    g.items = (uint64_t)rows_of_items * g.ngx;
    g.pitch = (size_t)s.pitch;
    g.chroma_at = (size_t)s.rows * s.pitch;
    g.plane2_at = g.chroma_at + (size_t)(s.pitch / 2) * (size_t)(s.rows / 2);
    g.frame_bytes = yuv_frame_size(s);
    g.nframes = s.nframes;
    g.yuv8 = 0;
    g.rgba16 = 0;
    return g;
}

template <class K, class... A>
hipError_t launch(hipStream_t stream, K kernel, const YuvGeom& g, A... args)
{
    const uint64_t blocks = (g.items + kThreads - 1) / kThreads;
    if (blocks == 0 || blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const unsigned gy = (unsigned)(g.nframes < 65535 ? g.nframes : 65535);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, gy), dim3(kThreads), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace

size_t yuv_frame_size(const YuvFrames& s)
{
    const size_t luma = (size_t)s.pitch * (size_t)s.rows;
    return yuv_layout_packed(s.layout) ? luma : luma / 2 * 3;  // rows is even for 4:2:0
}

hipError_t launch_yuv_to_rgba(hipStream_t stream, const uint8_t* d_yuv, uint8_t* d_rgba, const YuvFrames& s,
                              const YuvDecodeCoef& c)
{
    const bool packed = yuv_layout_packed(s.layout);
    YuvGeom g = geom_of(s, packed ? (size_t)s.h : (size_t)s.h / 2);
    // 8-byte luma and chroma (4-byte planar chroma) accesses; packed rows are read 16 bytes at a time
    g.yuv8 = packed ? aligned_to(d_yuv, 16) && s.pitch % 16 == 0 : aligned_to(d_yuv, 8) && s.pitch % 8 == 0;
    g.rgba16 = aligned_to(d_rgba, 16) && s.w % 4 == 0;
    uint32_t* out = reinterpret_cast<uint32_t*>(d_rgba);
    switch (s.layout) {
    case 0:
        return launch(stream, yuv420_decode_kernel<SEMI, false>, g, d_yuv, out, g, c);
    case 1:
        return launch(stream, yuv420_decode_kernel<SEMI, true>, g, d_yuv, out, g, c);
    case 2:
        return launch(stream, yuv420_decode_kernel<PLANAR, false>, g, d_yuv, out, g, c);
    case 3:
        return launch(stream, yuv420_decode_kernel<PLANAR, true>, g, d_yuv, out, g, c);
    case 4:
        return launch(stream, yuv422_decode_kernel<false>, g, d_yuv, out, g, c);
    case 5:
        return launch(stream, yuv422_decode_kernel<true>, g, d_yuv, out, g, c);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_rgba_to_yuv(hipStream_t stream, const uint8_t* d_rgba, uint8_t* d_yuv, const YuvFrames& s,
                              const YuvEncodeCoef& c)
{
    if (yuv_layout_packed(s.layout))
        return hipErrorInvalidValue;
    YuvGeom g = geom_of(s, (size_t)s.h / 2);
    g.yuv8 = aligned_to(d_yuv, 8) && s.pitch % 8 == 0;
    g.rgba16 = aligned_to(d_rgba, 16) && s.w % 4 == 0;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(d_rgba);
    switch (s.layout) {
    case 0:
        return launch(stream, yuv420_encode_kernel<SEMI, false>, g, in, d_yuv, g, c);
    case 1:
        return launch(stream, yuv420_encode_kernel<SEMI, true>, g, in, d_yuv, g, c);
    case 2:
        return launch(stream, yuv420_encode_kernel<PLANAR, false>, g, in, d_yuv, g, c);
    case 3:
        return launch(stream, yuv420_encode_kernel<PLANAR, true>, g, in, d_yuv, g, c);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_yuv_to_gray(hipStream_t stream, const uint8_t* d_yuv, uint8_t* d_gray, const YuvFrames& s)
{
    const bool packed = yuv_layout_packed(s.layout);
    YuvGeom g = geom_of(s, (size_t)s.h);
    g.yuv8 = packed ? aligned_to(d_yuv, 16) && s.pitch % 16 == 0 : aligned_to(d_yuv, 8) && s.pitch % 8 == 0;
    g.rgba16 = aligned_to(d_gray, 8) && s.w % 8 == 0;  // here: aligned 8-byte stores
    if (!packed)
        return launch(stream, yuv_luma_kernel<false, false>, g, d_yuv, d_gray, g);
    if (s.layout == 4)
        return launch(stream, yuv_luma_kernel<true, false>, g, d_yuv, d_gray, g);
    return launch(stream, yuv_luma_kernel<true, true>, g, d_yuv, d_gray, g);
}

}  // namespace mi355
