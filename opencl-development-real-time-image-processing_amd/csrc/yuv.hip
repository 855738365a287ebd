// yuv.hip — 8-bit YUV (NV12 / NV21 / I420 / YV12 / YUY2 / UYVY) <-> RGBA and the luma plane of such frames.
// Semantics: include/mi355_imgfilter.h, "frames from a decoder or a camera".  All arithmetic is int32; every constant is
// below 2^23 in magnitude and every other factor is a byte or a byte minus 128, so each product is exact in the full-rate
// 24-bit multiply (v_mul_i32_i24 / v_mad_i32_i24).
//
// Lane geometry (for_lane_frames).  A lane owns 8 consecutive pixels of a row pair (4:2:0) or of one row (packed and
// luma), the chroma of which is shared by construction: a 2 x 2 block never straddles two lanes.  A wave covers 512
// pixels of a row (pair): every load and store instruction of a wave touches one contiguous span.  Work items are
// numbered inside a frame (row pair major), frames go over blockIdx.y; all byte offsets are size_t.
// Surfaces.  A layout is a class (SEMI, PLANAR, PACKED) and a byte order (SWAP); dispatch_layout maps the layout number
// to the pair.  Per class: load_chroma / store_chroma (4:2:0), load_pairs / pairs_luma / pairs_chroma (packed); luma
// rows of 4:2:0 are plain 8-byte spans.  4:2:0 decode = two 8-byte luma loads, one 8-byte (semi-planar) or two 4-byte
// (planar) chroma loads and four 16-byte RGBA stores, the encode is its mirror image; a packed row is one 16-byte load.
// Paths.  The wide accesses want the whole 8 pixels inside the row (LaneItem::full, per lane) and, per launch, aligned
// addresses: YuvGeom::yuv_wide for the YUV side, other_wide for the RGBA or gray side.  Every other lane takes byte
// accesses for the YUV and gray sides and dword accesses for the RGBA side, in the same launch, with the same
// arithmetic.  Only bytes of pixels are ever loaded or stored: the padding of a pitched surface is never written.
#include "common.hpp"
#include "kernels.hpp"

namespace mi355 {

namespace {

constexpr int kThreads = 256;
constexpr int kPx = 8;  // pixels of a row per lane

enum { SEMI = 0, PLANAR = 1, PACKED = 2 };  // layout >> 1; layout & 1 is SWAP: V (4:2:0) or chroma (packed) comes first

// what a launch knows about its surface, by value
struct YuvGeom {
    int w, h;
    uint32_t ngx;        // lanes per row: ceil(w / 8)
    uint64_t items;      // work items per frame
    size_t pitch;        // luma (or packed) row stride in bytes
    size_t chroma_at;    // offset of the chroma area in a frame: rows * pitch
    size_t plane2_at;    // planar: offset of the second chroma plane
    size_t frame_bytes;  // distance between frames
    int yuv_wide;        // YUV side: the wide accesses (8 bytes; 4 of a planar chroma row, 16 of a packed one) are aligned
    int other_wide;      // RGBA or gray side: its widest access (16-byte RGBA, 8-byte gray) is aligned
    int nframes;
};

// the work item of a lane inside a frame: 8 pixels from x0 on of a row (or row pair), n (even, >= 2) of them in the row
struct LaneItem {
    uint32_t row;
    int x0, n;
    bool full;  // n == 8
};

__device__ __forceinline__ bool lane_item(const YuvGeom& g, LaneItem* it)  // false past the end
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.items)
        return false;
    if (g.items >> 32) {  // frames of more than 2^32 items (a few 10^10 pixels two wide): the long division
        const uint64_t r = i / g.ngx;
        it->row = (uint32_t)r;
        it->x0 = (int)(i - r * g.ngx) * kPx;
    } else {
        const uint32_t r = (uint32_t)i / g.ngx;
        it->row = r;
        it->x0 = (int)((uint32_t)i - r * g.ngx) * kPx;
    }
    it->n = min(kPx, g.w - it->x0);
    it->full = it->n == kPx;
    return true;
}

// body(item, frame) for the item of this lane in every frame of its blockIdx.y
template <class F>
__device__ __forceinline__ void for_lane_frames(const YuvGeom& g, F body)
{
    LaneItem it;
    if (!lane_item(g, &it))
        return;
    for (int f = blockIdx.y; f < g.nframes; f += gridDim.y)
        body(it, (size_t)f);
}

// sat(v >> 20), clamped BEFORE the shift.  The plain form, clamp((v >> 20), 0, 255) packed two to a register, is selected
// as v_ashr_pk_u8_i32 by the compiler, which then ORs the blue byte into bits 16-23 of that result as if they were zero;
// on the MI355X they came back holding bits 16-23 of the destination's previous value (the red sum) and every blue byte
// was wrong by those bits (found by tests/test_gpu_yuv.py, the first run of this kernel).  Clamping the 28-bit value first
// gives the same byte and does not match that pattern.
__device__ __forceinline__ uint32_t sat_shr20(int v) { return (uint32_t)clampi(v, 0, (256 << 20) - 1) >> 20; }

// ---- byte lanes: eight bytes in two dwords ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t byte_of(const u32x2& v, int j)
{
    return ((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xFFu;
}

__device__ __forceinline__ void put_byte(u32x2& v, int j, uint32_t b)  // into a byte that is still 0
{
    if (j < 4)
        v.x |= b << (8 * j);
    else
        v.y |= b << (8 * (j - 4));
}

// n (<= 8) bytes at p into the low bytes of two dwords, the rest 0
__device__ __forceinline__ u32x2 load_bytes(const uint8_t* p, int n)
{
    u32x2 v = {0u, 0u};
    for (int j = 0; j < n; j++)
        put_byte(v, j, p[j]);
    return v;
}

__device__ __forceinline__ void store_bytes(uint8_t* p, const u32x2& v, int n)
{
    for (int j = 0; j < n; j++)
        p[j] = (uint8_t)byte_of(v, j);
}

// the n (<= W) bytes of a lane in a row of bytes (W = 8: luma, semi-planar chroma, gray; 4: a planar chroma plane), in
// the low bytes of two dwords: one W-byte access where `wide` says that all W are in the row and aligned
template <int W>
__device__ __forceinline__ u32x2 load_span(const uint8_t* p, int n, bool wide)
{
    if (!wide)
        return load_bytes(p, n);
    if constexpr (W == 8)
        return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    return u32x2{__builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)), 0u};
}

template <int W>
__device__ __forceinline__ void store_span(uint8_t* p, const u32x2& v, int n, bool wide)
{
    if (!wide)
        store_bytes(p, v, n);
    else if constexpr (W == 8)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p));
    else
        __builtin_nontemporal_store(v.x, reinterpret_cast<uint32_t*>(p));
}

// ---- surfaces --------------------------------------------------------------------------------------------------------
// 4:2:0 chroma of row pair rp for the n pixels from x0 on, one value per pixel pair, in storage order: `first` is U
// unless the layout is SWAP.  SEMI: n bytes, first and second interleaved, in a row of the luma pitch; PLANAR: n / 2 bytes in a
// row of half the pitch in each of the two planes.  Pairs past the row are loaded as 128 and not stored.
template <int CLS>
__device__ __forceinline__ size_t chroma_off(const YuvGeom& g, uint32_t rp, int x0)
{
    return g.chroma_at + (CLS == SEMI ? (size_t)rp * g.pitch + x0 : (size_t)rp * (g.pitch >> 1) + (x0 >> 1));
}

template <int CLS>
__device__ __forceinline__ void load_chroma(const YuvGeom& g, const uint8_t* fr, uint32_t rp, int x0, int n, bool wide,
                                            uint32_t first[4], uint32_t second[4])
{
    constexpr int step = CLS == SEMI ? 2 : 1;  // bytes from one pair's value to the next
    const uint8_t* p = fr + chroma_off<CLS>(g, rp, x0);
    const uint8_t* p2 = p + (CLS == SEMI ? 1 : g.plane2_at - g.chroma_at);  // the second value of the first pair
    if (wide) {
        const u32x2 cv = CLS == SEMI ? load_span<8>(p, 8, true)
                                     : u32x2{load_span<4>(p, 4, true).x, load_span<4>(p2, 4, true).x};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            first[j] = byte_of(cv, step * j);
            second[j] = byte_of(cv, CLS == SEMI ? 2 * j + 1 : j + 4);
        }
    } else {  // byte loads that do not wait for each other: load_bytes' loop per plane measured 4 - 7 % on the decode
#pragma unroll
        for (int j = 0; j < 4; j++) {
            first[j] = second[j] = 128u;
            if (2 * j < n) {
                first[j] = p[step * j];
                second[j] = p2[step * j];
            }
        }
    }
}

// first / second: the four values of each kind packed into a dword, as the encode accumulates them
template <int CLS>
__device__ __forceinline__ void store_chroma(const YuvGeom& g, uint8_t* fr, uint32_t rp, int x0, int n, bool wide,
                                             uint32_t first, uint32_t second)
{
    uint8_t* p = fr + chroma_off<CLS>(g, rp, x0);
    if (CLS == SEMI) {
        u32x2 cv;  // interleave: first0 second0 first1 second1 | ...
        cv.x = (first & 0xFFu) | ((second & 0xFFu) << 8) | ((first & 0xFF00u) << 8) | ((second & 0xFF00u) << 16);
        cv.y = ((first >> 16) & 0xFFu) | (((second >> 16) & 0xFFu) << 8) | ((first >> 24) << 16) | ((second >> 24) << 24);
        store_span<8>(p, cv, n, wide);
    } else {
        store_span<4>(p, u32x2{first, 0u}, n >> 1, wide);
        store_span<4>(p + (g.plane2_at - g.chroma_at), u32x2{second, 0u}, n >> 1, wide);
    }
}

// Packed 4:2:2: the n pixels of a lane are n / 2 pairs of 4 bytes at p, one dword each; pairs past the row are 0.
__device__ __forceinline__ void load_pairs(const uint8_t* p, int n, bool wide, uint32_t d[4])
{
    if (wide) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            d[j] = 2 * j < n ? load_bytes(p + 4 * j, 4).x : 0u;
    }
}

// SWAP: chroma comes first (UYVY), else luma (YUY2)
template <bool SWAP>
__device__ __forceinline__ u32x2 pairs_luma(const uint32_t d[4])
{
    u32x2 yv = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t q = SWAP ? d[j] >> 8 : d[j];  // luma in bytes 0 and 2
        put_byte(yv, 2 * j, q & 0xFFu);
        put_byte(yv, 2 * j + 1, (q >> 16) & 0xFFu);
    }
    return yv;
}

template <bool SWAP>
__device__ __forceinline__ void pairs_chroma(const uint32_t d[4], uint32_t ub[4], uint32_t vb[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t k = SWAP ? d[j] : d[j] >> 8;  // U in byte 0, V in byte 2
        ub[j] = k & 0xFFu;
        vb[j] = (k >> 16) & 0xFFu;
    }
}

// 8 RGBA pixels of a row, n of them in it: two 16-byte accesses where `wide` says so, else dwords
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

// ---- decode ----------------------------------------------------------------------------------------------------------
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

// An item is 8 pixels of ROWS rows that share their chroma: a row pair of 4:2:0, one row of packed 4:2:2.
template <int CLS, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv_decode_kernel(const uint8_t* __restrict__ yuv,
                                                              uint32_t* __restrict__ rgba, YuvGeom g, YuvDecodeCoef c)
{
    constexpr int ROWS = CLS == PACKED ? 1 : 2;
    for_lane_frames(g, [&](const LaneItem& it, size_t f) {
        const uint8_t* fr = yuv + f * g.frame_bytes;
        const size_t row0 = (size_t)ROWS * it.row;
        const bool wide = it.full && g.yuv_wide;
        u32x2 yv[ROWS];
        uint32_t ub[4], vb[4];
        if constexpr (CLS == PACKED) {
            uint32_t d[4];
            load_pairs(fr + row0 * g.pitch + 2 * (size_t)it.x0, it.n, wide, d);
            yv[0] = pairs_luma<SWAP>(d);
            pairs_chroma<SWAP>(d, ub, vb);
        } else {
#pragma unroll
            for (int r = 0; r < ROWS; r++)
                yv[r] = load_span<8>(fr + (row0 + r) * g.pitch + it.x0, it.n, wide);
            load_chroma<CLS>(g, fr, it.row, it.x0, it.n, wide, SWAP ? vb : ub, SWAP ? ub : vb);
        }
        int rv[4], gv[4], bu[4];
        chroma_terms(c, ub, vb, rv, gv, bu);
        uint32_t* o = rgba + f * ((size_t)g.w * g.h) + row0 * g.w + it.x0;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            uint32_t px[kPx];
            decode_row(c, yv[r], rv, gv, bu, px);
            store_px(o + (size_t)r * g.w, px, it.n, it.full && g.other_wide);
        }
    });
}

// ---- luma ------------------------------------------------------------------------------------------------------------
// The Y bytes of every frame, unchanged, into tightly packed (n, h, w) planes; an item is 8 pixels of one row.  SEMI
// stands for the four 4:2:0 layouts: their luma planes are the same bytes.
template <int CLS, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv_luma_kernel(const uint8_t* __restrict__ yuv, uint8_t* __restrict__ gray,
                                                            YuvGeom g)
{
    for_lane_frames(g, [&](const LaneItem& it, size_t f) {
        const uint8_t* row = yuv + f * g.frame_bytes + (size_t)it.row * g.pitch;
        const bool wide = it.full && g.yuv_wide;
        u32x2 yv;
        if constexpr (CLS == PACKED) {
            uint32_t d[4];
            load_pairs(row + 2 * (size_t)it.x0, it.n, wide, d);
            yv = pairs_luma<SWAP>(d);
        } else {
            yv = load_span<8>(row + it.x0, it.n, wide);
        }
        store_span<8>(gray + f * ((size_t)g.w * g.h) + (size_t)it.row * g.w + it.x0, yv, it.n, it.full && g.other_wide);
    });
}

// ---- encode ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32x2 encode_luma(const YuvEncodeCoef& c, const uint32_t px[kPx])
{
    u32x2 yv = {0u, 0u};
#pragma unroll
    for (int j = 0; j < kPx; j++) {
        const int r = px[j] & 0xFFu, g = (px[j] >> 8) & 0xFFu, b = (px[j] >> 16) & 0xFFu;
        put_byte(yv, j, sat_shr20(__mul24(c.cry, r) + __mul24(c.cgy, g) + __mul24(c.cby, b) + c.ybias));
    }
    return yv;
}

// U and V of the four 2 x 2 blocks of an item, from the top-left pixel of each (the even pixels of the even row), four
// bytes to a dword in storage order: SWAP puts V into `first`
template <bool SWAP>
__device__ __forceinline__ void encode_chroma(const YuvEncodeCoef& c, const uint32_t px[kPx], uint32_t& first,
                                              uint32_t& second)
{
    const int cbias = (1 << 19) + (128 << 20);
    first = second = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t q = px[2 * j];
        const int r = q & 0xFFu, g = (q >> 8) & 0xFFu, b = (q >> 16) & 0xFFu;
        const uint32_t u = sat_shr20(__mul24(c.cru, r) + __mul24(c.cgu, g) + __mul24(c.cbu, b) + cbias);
        const uint32_t v = sat_shr20(__mul24(c.cbu, r) + __mul24(c.cgv, g) + __mul24(c.cbv, b) + cbias);
        first |= (SWAP ? v : u) << (8 * j);
        second |= (SWAP ? u : v) << (8 * j);
    }
}

// The mirror image of the 4:2:0 decode: an item is 8 pixels of a row pair.
template <int CLS, bool SWAP>
__global__ __launch_bounds__(kThreads) void yuv_encode_kernel(const uint32_t* __restrict__ rgba,
                                                              uint8_t* __restrict__ yuv, YuvGeom g, YuvEncodeCoef c)
{
    for_lane_frames(g, [&](const LaneItem& it, size_t f) {
        const size_t row0 = 2 * (size_t)it.row;
        const uint32_t* s = rgba + f * ((size_t)g.w * g.h) + row0 * g.w + it.x0;
        uint32_t p0[kPx], p1[kPx];
        load_px(s, p0, it.n, it.full && g.other_wide);
        load_px(s + g.w, p1, it.n, it.full && g.other_wide);
        const u32x2 ya = encode_luma(c, p0), yb = encode_luma(c, p1);
        uint32_t first, second;
        encode_chroma<SWAP>(c, p0, first, second);
        uint8_t* fr = yuv + f * g.frame_bytes;
        uint8_t* y0 = fr + row0 * g.pitch + it.x0;
        const bool wide = it.full && g.yuv_wide;
        if (wide) {  // both rows in one arm, not a store_span each (profiles/yuv_frame_vgpr.txt)
            __builtin_nontemporal_store(ya, reinterpret_cast<u32x2*>(y0));
            __builtin_nontemporal_store(yb, reinterpret_cast<u32x2*>(y0 + g.pitch));
        } else {
            store_bytes(y0, ya, it.n);
            store_bytes(y0 + g.pitch, yb, it.n);
        }
        store_chroma<CLS>(g, fr, it.row, it.x0, it.n, wide, first, second);
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the geometry of a launch over `rows_of_items` rows (or row pairs) of ceil(w / 8) lanes each.  The YUV side takes its
// wide accesses when base and pitch are multiples of 8 (16 for packed rows, read 16 bytes at a time): frame sizes,
// chroma offsets and half pitches then are multiples of what their accesses need.
YuvGeom geom_of(const YuvFrames& s, size_t rows_of_items, const uint8_t* d_yuv, bool other_wide)
{
    const size_t yuv_align = yuv_layout_packed(s.layout) ? 16 : 8;
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
    g.yuv_wide = aligned_to(d_yuv, yuv_align) && s.pitch % yuv_align == 0;
    g.other_wide = other_wide;
    return g;
}

// f(CLS, SWAP) for a layout number (kernels.hpp: 0 NV12, 1 NV21, 2 I420, 3 YV12, 4 YUY2, 5 UYVY); hipErrorInvalidValue
// for any other.  f is instantiated for all six pairs: a launcher whose kernel does not tell some of them apart (the luma
// plane of every 4:2:0 layout is the same bytes) folds them onto one before it names the kernel.
template <typename F>
hipError_t dispatch_layout(int layout, F&& f)
{
    return dispatch_int(layout >> 1, std::integer_sequence<int, SEMI, PLANAR, PACKED>{}, [&](auto CLS) {
        return dispatch_bool(layout & 1, [&](auto SWAP) { return f(CLS, SWAP); });
    });
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
    const size_t rows_of_items = yuv_layout_packed(s.layout) ? (size_t)s.h : (size_t)s.h / 2;
    const YuvGeom g = geom_of(s, rows_of_items, d_yuv, aligned_to(d_rgba, 16) && s.w % 4 == 0);
    return dispatch_layout(s.layout, [&](auto CLS, auto SWAP) {
        return launch(stream, yuv_decode_kernel<CLS.value, SWAP.value>, g, d_yuv, reinterpret_cast<uint32_t*>(d_rgba), g,
                      c);
    });
}

hipError_t launch_rgba_to_yuv(hipStream_t stream, const uint8_t* d_rgba, uint8_t* d_yuv, const YuvFrames& s,
                              const YuvEncodeCoef& c)
{
    if (yuv_layout_packed(s.layout))
        return hipErrorInvalidValue;  // there is no packed encode
    const YuvGeom g = geom_of(s, (size_t)s.h / 2, d_yuv, aligned_to(d_rgba, 16) && s.w % 4 == 0);
    return dispatch_layout(s.layout, [&](auto CLS, auto SWAP) {
        constexpr int cls = CLS.value == PLANAR ? PLANAR : SEMI;  // (PACKED, refused above, instantiates nothing new)
        return launch(stream, yuv_encode_kernel<cls, SWAP.value>, g, reinterpret_cast<const uint32_t*>(d_rgba), d_yuv, g,
                      c);
    });
}

hipError_t launch_yuv_to_gray(hipStream_t stream, const uint8_t* d_yuv, uint8_t* d_gray, const YuvFrames& s)
{
    const YuvGeom g = geom_of(s, (size_t)s.h, d_yuv, aligned_to(d_gray, 8) && s.w % 8 == 0);
    return dispatch_layout(s.layout, [&](auto CLS, auto SWAP) {
        constexpr bool packed = CLS.value == PACKED;
        return launch(stream, yuv_luma_kernel<packed ? PACKED : SEMI, packed && SWAP.value>, g, d_yuv, d_gray, g);
    });
}

}  // namespace mi355
