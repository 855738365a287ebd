// capi.hip — the C-ABI of libmi355_imgfilter.so (include/mi355_imgfilter.h): context, pooled
// buffers, coefficient cache, HIP-event profiling, and the host-buffer / device-resident entry
// points.  No CPU fallback anywhere: every filter call ends in a gfx950 kernel launch or an error.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>
#include <vector>

#include "../../include/mi355_imgfilter.h"
#include "kernels.hpp"

using namespace mi355;

namespace {

struct CoefEntry {
    int k;
    uint32_t sigma_bits;
    GaussCoef coef;
    float* d_buf;  // [k*k w2d][k w1d][256 constant-alpha bytes << 24, as uint32][256 CPU-chain bytes << 16]
    std::vector<float> h_tab;  // host copy of the same block (its heap storage stays put when entries move)
    uint64_t last_use;
    bool installed;  // came through mi355_ctx_set_gauss_weights: never evicted (it cannot be regenerated)
};

// Distinct GENERATED (k, sigma) tables kept per context; the least recently used one goes.  Tables a caller installed
// (mi355_ctx_set_gauss_weights: a box filter, a non-separable table, the bytes rank 0 broadcast) are kept outside
// this cap and are never evicted — a miss would silently regenerate the default Gaussian under the same key; at most
// kMaxInstalledCoefs of them per context, one more is MI355_ERR_BAD_ARG.
constexpr size_t kMaxCoefEntries = 16;
constexpr size_t kMaxInstalledCoefs = 64;

// a pooled device buffer of the context: freed by mi355_ctx_destroy, grown by ensure() / ensure_slots()
struct DevBuf {
    void* p;
    size_t cap;
};

}  // namespace

struct mi355_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[6] = {};
    hipEvent_t t0 = nullptr, t1 = nullptr;
    DevBuf d_in = {}, d_out = {};
    DevBuf d_raw = {};    // BGR staging of the host-buffer calls
    DevBuf d_flags = {};  // per-work-item flags of the two-kernel Gaussian (gauss_wide.hip)
    DevBuf d_hist = {};   // per-frame 256-bin histograms of EQUALIZE_GRAY8 / OTSU_GRAY8 (hist.hip)
    DevBuf d_lut = {};    // their per-frame 256-byte tables
    DevBuf d_ccl = {};    // per-block component counts, then offsets, of the labelling calls (ccl.hip)
    DevBuf d_dist = {};   // per-pixel int16 row offsets to the column's nearest site of the distance calls (dist.hip)
    DevBuf d_parent = {};  // the union-find parent array, 4 bytes per pixel, of the hysteresis and Canny calls (canny.hip)
    DevBuf d_hough = {};      // counters, point lists and candidate lists of the Hough calls (hough.hip)
    DevBuf d_hough_acc = {};  // their accumulator when the caller passes none
    float* d_hough_tab = nullptr;  // the trig table on the device (2 * MI355_MAX_HOUGH_ANGLES floats) ...
    double hough_key[4] = {};      // ... and the (rho, theta, min_theta, numangle) it was made for; numangle 0: none yet
    DevBuf d_map1 = {}, d_map2 = {};  // the maps of mi355_remap_batched
    unsigned long long* d_acc = nullptr;
    float* d_img_table = nullptr;  // image2d-mode Gaussian table (k*k floats, MI355_MAX_GAUSS_K^2 capacity)
    // streamed path: copy streams, per-slot events and device slots (created on first use)
    static constexpr int kSlots = 3;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_h2d[kSlots] = {}, ev_k[kSlots] = {}, ev_d2h[kSlots] = {};
    DevBuf slot_in[kSlots] = {}, slot_out[kSlots] = {}, slot_raw[kSlots] = {};
    int input_format = MI355_INPUT_RGBA;
    int gauss_mode = MI355_GAUSS_FAST;
    int impl = MI355_IMPL_AUTO;
    int last_hip = 0;
    char name[256] = {};
    std::vector<CoefEntry> coefs;
    uint64_t coef_clock = 0;
    std::vector<void*> pinned;  // mi355_host_alloc blocks still outstanding (freed at destroy)
};

namespace {

#define HIP_TRY(ctx, expr)                     \
    do {                                       \
        hipError_t e__ = (expr);               \
        if (e__ != hipSuccess) {               \
            if (ctx)                           \
                (ctx)->last_hip = (int)e__;    \
            return MI355_ERR_HIP;              \
        }                                      \
    } while (0)

uint64_t now_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

uint32_t fbits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

bool valid_k(int k) { return k >= 1 && k <= MI355_MAX_GAUSS_K && (k & 1) == 1; }
bool valid_sigma(float s) { return std::isfinite(s) && s > 0.0f; }

// Controller::_GenerateGaussianKernelBuffers, RT/src/Controller.cpp:352-372.
// `exp` there binds to ::exp(double); the float argument is widened.
void gen_weights(int k, float sigma, float* out)
{
    const int half = k / 2;
    float sum = 0.0f;
    for (int y = -half; y <= half; y++) {
        for (int x = -half; x <= half; x++) {
            const float arg = -(x * x + y * y) / (2 * sigma * sigma);
            const float value = (float)(std::exp((double)arg) / (2 * M_PI * sigma * sigma));
            out[(y + half) * k + (x + half)] = value;
            sum += value;
        }
    }
    for (int i = 0; i < k * k; i++)
        out[i] /= sum;
}

// Controller::_GenerateGaussianKernelImage2D, RT/src/Controller.cpp:374-403: the image-mode twin.  Its loops run
// x, y < half (one short), so the last row and the last column of the table stay 0, and the normalising sum covers
// only the (k-1) x (k-1) entries that were written; x is the OUTER index.  Same promotion chain as gen_weights.
void gen_weights_image2d(int k, float sigma, float* out)
{
    const int half = k / 2;
    for (int i = 0; i < k * k; i++)
        out[i] = 0.0f;
    float sum = 0.0f;
    for (int x = -half; x < half; x++) {
        for (int y = -half; y < half; y++) {
            const float arg = -((x * x + y * y) / (2 * sigma * sigma));
            const float value = (float)(std::exp((double)arg) / (2 * M_PI * sigma * sigma));
            out[(x + half) * k + (y + half)] = value;
            sum += value;
        }
    }
    for (int i = 0; i < k * k; i++)
        out[i] /= sum;
}

// Separable factor of the table for the FAST arithmetic: rowsum / sqrt(total), in double.  Returns whether the
// factor really reproduces the table: every entry non-negative, total > 0 and |w2d[i][j] - w1d[i] * w1d[j]| within
// float rounding of the largest entry (the reference's own tables deviate by <= 1.8e-7 of it for every odd k <= 63;
// the bound used is 1e-6).  A table that fails — non-separable, asymmetric, negative lobes — must not go through
// the separable kernels: the caller routes it to the tap-by-tap tiled kernel.
bool separable_factor(int k, const float* w2d, float* w1d)
{
    double tot = 0.0, wmax = 0.0;
    bool nonneg = true;
    std::vector<double> rs(k, 0.0);
    for (int i = 0; i < k; i++) {
        for (int j = 0; j < k; j++) {
            const double v = (double)w2d[i * k + j];
            rs[i] += v;
            nonneg = nonneg && v >= 0.0;
            wmax = std::fmax(wmax, std::fabs(v));
        }
        tot += rs[i];
    }
    if (!nonneg || !(tot > 0.0)) {
        for (int i = 0; i < k; i++)
            w1d[i] = 0.0f;
        return false;
    }
    const double s = std::sqrt(tot);
    for (int i = 0; i < k; i++)
        w1d[i] = (float)(rs[i] / s);
    double dev = 0.0;
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++)
            dev = std::fmax(dev, std::fabs((double)w2d[i * k + j] - (double)w1d[i] * (double)w1d[j]));
    return dev <= 1.0e-6 * wmax;
}

// First use of a (k, sigma) key — and a call that evicts — synchronises the context's stream and makes blocking
// allocations / copies; every later call with a cached key does not (include/mi355_imgfilter.h says so).
int install_coef(mi355_ctx* ctx, int k, float sigma, const float* w2d, bool installed, const GaussCoef** out)
{
    CoefEntry* slot = nullptr;
    size_t n_generated = 0, n_installed = 0;
    for (auto& e : ctx->coefs) {
        if (e.k == k && e.sigma_bits == fbits(sigma))
            slot = &e;
        (e.installed ? n_installed : n_generated)++;
    }
    if (!slot) {
        if (installed && n_installed >= kMaxInstalledCoefs)
            return MI355_ERR_BAD_ARG;
        if (!installed && n_generated >= kMaxCoefEntries) {
            // evict the least recently used GENERATED table; a kernel still in flight may be reading it
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            size_t lru = ctx->coefs.size();
            for (size_t i = 0; i < ctx->coefs.size(); i++)
                if (!ctx->coefs[i].installed && (lru == ctx->coefs.size() || ctx->coefs[i].last_use < ctx->coefs[lru].last_use))
                    lru = i;
            (void)hipFree(ctx->coefs[lru].d_buf);
            ctx->coefs.erase(ctx->coefs.begin() + (long)lru);
        }
        CoefEntry e{};
        e.k = k;
        e.sigma_bits = fbits(sigma);
        HIP_TRY(ctx, hipMalloc((void**)&e.d_buf, sizeof(float) * (size_t)(k * k + k + 512)));
        ctx->coefs.push_back(e);
        slot = &ctx->coefs.back();
    }
    slot->last_use = ++ctx->coef_clock;
    slot->installed = slot->installed || installed;
    std::vector<float> host((size_t)k * k + k + 512);
    std::memcpy(host.data(), w2d, sizeof(float) * (size_t)k * k);
    const bool separable = separable_factor(k, w2d, host.data() + (size_t)k * k);
    uint32_t alpha_tab[256];
    for (uint32_t a = 0; a < 256; a++)
        alpha_tab[a] = gauss_const_alpha(host.data() + (size_t)k * k, k, a) << 24;
    std::memcpy(host.data() + (size_t)k * k + k, alpha_tab, sizeof(alpha_tab));
    uint32_t alpha_cpu[256];
    for (uint32_t a = 0; a < 256; a++) {
        // the CPU path's own chain over a window that is `a` everywhere (one float multiply, one float add per tap;
        // this translation unit is built with -ffp-contract=off), clamped and truncated
        float chain = 0.0f;
        for (int i = 0; i < k * k; i++)
            chain += (float)a * w2d[i];
        chain = chain < 0.0f ? 0.0f : (chain > 255.0f ? 255.0f : chain);
        alpha_cpu[a] = (uint32_t)chain << 16;
    }
    std::memcpy(host.data() + (size_t)k * k + k + 256, alpha_cpu, sizeof(alpha_cpu));
    // blocking copy from pageable memory: the table is live on the device when this returns
    const hipError_t ce = hipMemcpy(slot->d_buf, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
    if (ce != hipSuccess) {
        // never leave a half-installed table behind: a later call with this (k, sigma) would find it
        ctx->last_hip = (int)ce;
        (void)hipFree(slot->d_buf);
        ctx->coefs.erase(ctx->coefs.begin() + (slot - ctx->coefs.data()));
        return MI355_ERR_HIP;
    }
    slot->coef.k = k;
    slot->coef.separable = separable;
    slot->coef.d_w2d = slot->d_buf;
    slot->coef.d_w1d = slot->d_buf + (size_t)k * k;
    slot->coef.d_alpha_tab = reinterpret_cast<const uint32_t*>(slot->d_buf + (size_t)k * k + k);
    std::memcpy(slot->coef.h_alpha_tab, alpha_tab, sizeof(alpha_tab));
    slot->coef.d_alpha_cpu = reinterpret_cast<const uint32_t*>(slot->d_buf + (size_t)k * k + k + 256);
    std::memcpy(slot->coef.h_alpha_cpu, alpha_cpu, sizeof(alpha_cpu));
    std::memset(slot->coef.h_w1d, 0, sizeof(slot->coef.h_w1d));
    std::memcpy(slot->coef.h_w1d, host.data() + (size_t)k * k, sizeof(float) * k);
    slot->h_tab = host;
    slot->coef.h_w2d = slot->h_tab.data();
    if (out)
        *out = &slot->coef;
    return MI355_OK;
}

int get_coef(mi355_ctx* ctx, int k, float sigma, const GaussCoef** out)
{
    for (auto& e : ctx->coefs)
        if (e.k == k && e.sigma_bits == fbits(sigma)) {
            e.last_use = ++ctx->coef_clock;
            *out = &e.coef;
            return MI355_OK;
        }
    std::vector<float> w((size_t)k * k);
    gen_weights(k, sigma, w.data());
    return install_coef(ctx, k, sigma, w.data(), false, out);
}

int ensure(mi355_ctx* ctx, DevBuf& b, size_t need)
{
    if (b.cap >= need)
        return MI355_OK;
    if (b.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(b.p));
        b = {};
    }
    // grow geometrically so a stream of slightly different frame sizes does not reallocate each time
    size_t want = need + need / 4;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        e = hipMalloc(&b.p, need);
        want = need;
    }
    if (e != hipSuccess) {
        ctx->last_hip = (int)e;
        b.p = nullptr;
        return MI355_ERR_NOMEM;
    }
    b.cap = want;
    return MI355_OK;
}

// the streamed path's slots: exactly `need` bytes each.  A slot may still be in use on any of the path's three
// streams, so growing them waits for the whole device first.
int ensure_slots(mi355_ctx* ctx, DevBuf (&slots)[mi355_ctx::kSlots], size_t need)
{
    if (slots[0].cap >= need)
        return MI355_OK;
    HIP_TRY(ctx, hipDeviceSynchronize());
    for (DevBuf& b : slots) {
        if (b.p)
            (void)hipFree(b.p);
        b = {};
    }
    for (DevBuf& b : slots)
        if (hipMalloc(&b.p, need) != hipSuccess)
            return MI355_ERR_NOMEM;  // the caps stay 0: the next call starts over
    for (DevBuf& b : slots)
        b.cap = need;
    return MI355_OK;
}

// What a filter call's k and sigma must be: ignored; the Gaussian's odd 1 <= k <= MI355_MAX_GAUSS_K with a finite
// sigma > 0; the median's odd 3 <= k <= MI355_MAX_MEDIAN_K; the morphology's odd 3 <= k <= MI355_MAX_MORPH_K; the box
// mean's odd 3 <= k <= MI355_MAX_BOX_K.
enum class KRule { none, gauss, median, morph, box };

struct FilterInfo {
    int id;
    int in_bpp, out_bpp;  // bytes per pixel the kernel reads / writes
    KRule k;
    bool table;     // needs the (k, sigma) coefficient table
    bool below_2g;  // frames of 2^31 pixels or more are rejected (OpenCV counts a frame's pixels in an int)
};

// every filter id of include/mi355_imgfilter.h; dispatch_dev's switch maps each one to its launcher
constexpr FilterInfo kFilters[] = {
    {MI355_FILTER_GRAY, 4, 4, KRule::none, false, false},
    {MI355_FILTER_GRAY1, 4, 1, KRule::none, false, false},
    {MI355_FILTER_GAUSS, 4, 4, KRule::gauss, true, false},
    {MI355_FILTER_SOBEL, 4, 1, KRule::none, false, false},
    {MI355_FILTER_PIPELINE, 4, 1, KRule::gauss, true, false},
    {MI355_FILTER_GAUSS_GRAY8, 1, 1, KRule::gauss, true, false},
    {MI355_FILTER_SOBEL_GRAY8, 1, 1, KRule::none, false, false},
    {MI355_FILTER_PIPELINE_GRAY8, 1, 1, KRule::gauss, true, false},
    {MI355_FILTER_MEDIAN, 4, 4, KRule::median, false, false},
    {MI355_FILTER_MEDIAN_GRAY8, 1, 1, KRule::median, false, false},
    {MI355_FILTER_ERODE, 4, 4, KRule::morph, false, false},
    {MI355_FILTER_DILATE, 4, 4, KRule::morph, false, false},
    {MI355_FILTER_OPEN, 4, 4, KRule::morph, false, false},
    {MI355_FILTER_CLOSE, 4, 4, KRule::morph, false, false},
    {MI355_FILTER_ERODE_GRAY8, 1, 1, KRule::morph, false, false},
    {MI355_FILTER_DILATE_GRAY8, 1, 1, KRule::morph, false, false},
    {MI355_FILTER_OPEN_GRAY8, 1, 1, KRule::morph, false, false},
    {MI355_FILTER_CLOSE_GRAY8, 1, 1, KRule::morph, false, false},
    {MI355_FILTER_EQUALIZE_GRAY8, 1, 1, KRule::none, false, true},
    {MI355_FILTER_OTSU_GRAY8, 1, 1, KRule::none, false, true},
    {MI355_FILTER_BOX, 4, 4, KRule::box, false, false},
    {MI355_FILTER_BOX_GRAY8, 1, 1, KRule::box, false, false},
};

const FilterInfo* filter_info(int filter)
{
    for (const FilterInfo& f : kFilters)
        if (f.id == filter)
            return &f;
    return nullptr;
}

bool odd_in(int k, int lo, int hi) { return k >= lo && k <= hi && (k & 1) == 1; }

bool valid_sizes(int w, int h, int nframes)
{
    // 2^31 tiles / 2^40 bytes is far beyond 288 GB of HBM; reject before any size_t arithmetic wraps
    return w > 0 && h > 0 && nframes > 0 && (double)w * (double)h * (double)nframes <= 6.0e10;
}

// The value checks of every filter call (the callers check their own context and pointers first): a known id and
// sizes, then the id's k / sigma / frame-size rule.  All of them come before any HIP call.
int check_filter(int filter, int w, int h, int nframes, int k, float sigma, const FilterInfo** row)
{
    const FilterInfo* f = filter_info(filter);
    if (!f || !valid_sizes(w, h, nframes))
        return MI355_ERR_BAD_ARG;
    const bool k_ok = f->k == KRule::gauss    ? valid_k(k) && valid_sigma(sigma)
                      : f->k == KRule::median ? odd_in(k, 3, MI355_MAX_MEDIAN_K)
                      : f->k == KRule::morph  ? odd_in(k, 3, MI355_MAX_MORPH_K)
                      : f->k == KRule::box    ? odd_in(k, 3, MI355_MAX_BOX_K)
                                              : true;
    if (!k_ok || (f->below_2g && (int64_t)w * (int64_t)h >= (1ll << 31)))
        return MI355_ERR_BAD_ARG;
    if (row)
        *row = f;
    return MI355_OK;
}

// [a0, a0 + na) and [b0, b0 + nb) share a byte
constexpr bool overlap(uintptr_t a0, size_t na, uintptr_t b0, size_t nb) { return a0 < b0 + nb && b0 < a0 + na; }

size_t frame_bytes(int w, int h, int nframes, int bpp) { return (size_t)w * h * nframes * (size_t)bpp; }

// One byte range of a device-resident call: where it starts (0: the caller passed no such pointer), its length, the
// power-of-two alignment the kernels need of it, and whether the call writes it.
struct Range {
    uintptr_t at;
    size_t len;
    uintptr_t align;
    bool written;
};

Range rd(const void* p, size_t len, int align) { return {reinterpret_cast<uintptr_t>(p), len, (uintptr_t)align, false}; }
Range wr(const void* p, size_t len, int align) { return {reinterpret_cast<uintptr_t>(p), len, (uintptr_t)align, true}; }

// What every device-resident call refuses of its pointers: a present pointer that misses its alignment (RGBA pixels and
// every 4- or 8-byte output are accessed as such; frames of 1-byte pixels take any address, so a frame's alignment is its
// bytes per pixel), and two present ranges that share a byte unless neither is written.  The stencil and geometric
// kernels read neighbouring rows / halo / source pixels of what another wave may already have overwritten, and the
// (pointwise) grayscale kernels are compiled for non-aliasing pointers (__restrict__, non-temporal accesses): in-place
// and overlapping calls are rejected, not run, for every call (the reference never aliases them either: two
// clCreateBuffer objects per call, RT/src/Controller.cpp:234-244)
template <int N>
constexpr bool bad_ranges(const Range (&r)[N])
{
    for (int i = 0; i < N; i++) {
        if (!r[i].at)
            continue;
        if (r[i].at & (r[i].align - 1))
            return true;
        for (int j = 0; j < i; j++)
            if (r[j].at && (r[i].written || r[j].written) && overlap(r[i].at, r[i].len, r[j].at, r[j].len))
                return true;
    }
    return false;
}

static_assert(!bad_ranges({{64, 16, 4, false}, {80, 16, 4, true}}), "touching ranges pass");
static_assert(bad_ranges({{64, 17, 4, false}, {80, 16, 4, true}}), "one shared byte fails ...");
static_assert(bad_ranges({{80, 16, 4, true}, {64, 17, 1, false}}), "... whichever side is written");
static_assert(!bad_ranges({{64, 32, 4, false}, {80, 32, 2, false}, {128, 8, 8, true}}), "read-only ranges may overlap");
static_assert(!bad_ranges({{64, 32, 1, false}, {0, 1u << 20, 8, true}, {96, 8, 8, true}}), "a null entry is ignored");
static_assert(bad_ranges({{64, 16, 1, false}, {82, 16, 4, true}}), "a misaligned entry fails");
static_assert(!bad_ranges({{65, 15, 1, false}, {80, 16, 4, true}}), "a 1-byte range takes any address");

// The front of a device-resident call with frames of `bpp` bytes per pixel in and out, each side with its own shape: the
// null checks, what the call's value check answered (it is pure, so the caller has evaluated it), the pointer rules, and
// the context's device made current.
int frames_dev(mi355_ctx* ctx, const void* d_in, const void* d_out, int bpp, int src_w, int src_h, int dst_w, int dst_h,
               int nframes, int values_rc)
{
    if (!ctx || !d_in || !d_out)
        return MI355_ERR_BAD_ARG;
    if (values_rc != MI355_OK)
        return values_rc;
    if (bad_ranges({rd(d_in, frame_bytes(src_w, src_h, nframes, bpp), bpp),
                    wr(d_out, frame_bytes(dst_w, dst_h, nframes, bpp), bpp)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return MI355_OK;
}

// EQUALIZE_GRAY8 / OTSU_GRAY8 up to the tables in ctx->d_lut; Otsu's thresholds also to d_thresh if not null (below)
int hist_tables(mi355_ctx* ctx, const uint8_t* in, int32_t* d_thresh, int w, int h, int nframes, bool otsu);

int dispatch_dev(mi355_ctx* ctx, int filter, const void* d_in, void* d_out, int w, int h, int nframes,
                 int k, float sigma)
{
    if (!ctx || !d_in || !d_out)
        return MI355_ERR_BAD_ARG;
    const FilterInfo* f = nullptr;
    int rc = check_filter(filter, w, h, nframes, k, sigma, &f);
    if (rc != MI355_OK)
        return rc;
    if (bad_ranges({rd(d_in, frame_bytes(w, h, nframes, f->in_bpp), f->in_bpp),
                    wr(d_out, frame_bytes(w, h, nframes, f->out_bpp), f->out_bpp)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const GaussCoef* coef = nullptr;
    if (f->table) {
        rc = get_coef(ctx, k, sigma, &coef);
        if (rc != MI355_OK)
            return rc;
    }
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    uint8_t* out = static_cast<uint8_t*>(d_out);
    // a table the separable factor does not reproduce is applied tap by tap, whatever the mode
    const bool exact = ctx->gauss_mode == MI355_GAUSS_EXACT || (coef && !coef->separable);
    hipError_t e;
    switch (filter) {
    case MI355_FILTER_GRAY:
        e = launch_gray(ctx->stream, in, out, w, h, nframes, false);
        break;
    case MI355_FILTER_GRAY1:
        e = launch_gray(ctx->stream, in, out, w, h, nframes, true);
        break;
    case MI355_FILTER_GAUSS: {
        const size_t nflags = gauss_flag_items(in, out, w, h, nframes, *coef, exact, ctx->impl);
        if (nflags) {
            rc = ensure(ctx, ctx->d_flags, nflags * sizeof(uint32_t));
            if (rc != MI355_OK)
                return rc;
        }
        e = launch_gauss(ctx->stream, in, out, w, h, nframes, *coef, exact, ctx->impl,
                         static_cast<uint32_t*>(ctx->d_flags.p));
        break;
    }
    case MI355_FILTER_SOBEL:
        e = launch_sobel(ctx->stream, in, out, w, h, nframes, ctx->impl);
        break;
    case MI355_FILTER_PIPELINE:
        e = launch_pipeline(ctx->stream, in, out, w, h, nframes, *coef, exact, ctx->impl);
        break;
    case MI355_FILTER_GAUSS_GRAY8:
        e = launch_gauss_gray8(ctx->stream, in, out, w, h, nframes, *coef, exact, ctx->impl);
        break;
    case MI355_FILTER_SOBEL_GRAY8:
        e = launch_sobel_gray8(ctx->stream, in, out, w, h, nframes);
        break;
    case MI355_FILTER_PIPELINE_GRAY8:
        e = launch_pipeline_gray8(ctx->stream, in, out, w, h, nframes, *coef, ctx->impl);
        break;
    case MI355_FILTER_MEDIAN:
    case MI355_FILTER_MEDIAN_GRAY8:
        e = launch_median(ctx->stream, in, out, w, h, nframes, k, filter == MI355_FILTER_MEDIAN_GRAY8, ctx->impl);
        break;
    case MI355_FILTER_ERODE:
    case MI355_FILTER_DILATE:
    case MI355_FILTER_OPEN:
    case MI355_FILTER_CLOSE:
        e = launch_morph(ctx->stream, in, out, w, h, nframes, k, filter - MI355_FILTER_ERODE, false);
        break;
    case MI355_FILTER_ERODE_GRAY8:
    case MI355_FILTER_DILATE_GRAY8:
    case MI355_FILTER_OPEN_GRAY8:
    case MI355_FILTER_CLOSE_GRAY8:
        e = launch_morph(ctx->stream, in, out, w, h, nframes, k, filter - MI355_FILTER_ERODE_GRAY8, true);
        break;
    case MI355_FILTER_EQUALIZE_GRAY8:
    case MI355_FILTER_OTSU_GRAY8:
        rc = hist_tables(ctx, in, nullptr, w, h, nframes, filter == MI355_FILTER_OTSU_GRAY8);
        if (rc != MI355_OK)
            return rc;
        e = launch_lut_apply(ctx->stream, in, out, static_cast<const uint8_t*>(ctx->d_lut.p), w, h, nframes);
        break;
    case MI355_FILTER_BOX:
    case MI355_FILTER_BOX_GRAY8:
        e = launch_box(ctx->stream, in, out, w, h, nframes, k, filter == MI355_FILTER_BOX_GRAY8);
        break;
    default:
        return MI355_ERR_BAD_ARG;
    }
    HIP_TRY(ctx, e);
    return MI355_OK;
}

// The six timestamps of a write / kernel / read call from the four events recorded around the three operations on the
// in-order stream (ev[0] before the write, ev[1] between write and kernel, ev[3] between kernel and read, ev[5] after
// the read): write-end IS kernel-start, kernel-end IS read-start.
int fill_prof(mi355_ctx* ctx, uint64_t host0, uint64_t prof_ns[6])
{
    static const int kEv[6] = {0, 1, 1, 3, 3, 5};
    float ms1 = 0.0f, ms3 = 0.0f, ms5 = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms1, ctx->ev[0], ctx->ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms3, ctx->ev[0], ctx->ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms5, ctx->ev[0], ctx->ev[5]));
    prof_ns[0] = host0;
    for (int i = 1; i < 6; i++) {
        const float ms = kEv[i] == 1 ? ms1 : (kEv[i] == 3 ? ms3 : ms5);
        prof_ns[i] = host0 + (uint64_t)((double)ms * 1.0e6);
    }
    return MI355_OK;
}

// The timed part of a host-buffer call: H2D of `in_bytes` from `in` to `d_dst`, launch(), D2H of `out_bytes` from
// ctx->d_out to `out`, synchronised, with the reference's six profiling timestamps (RT/src/Controller.cpp:66-74).
// Four events on the in-order stream give the six timestamps: write-end IS kernel-start and kernel-end IS read-start
// (round 2 recorded six events and made five elapsed-time queries per call; at 75 x 75 the API calls around the three
// operations were a third of the call).  No events at all when the caller wants no timestamps.
// `upload` enqueues whatever else the call sends to the device (the maps of a remap); it counts as H2D time.
template <class Upload, class Launch>
int timed_roundtrip(mi355_ctx* ctx, void* d_dst, const void* in, size_t in_bytes, uint8_t* out, size_t out_bytes,
                    uint64_t prof_ns[6], Upload upload, Launch launch)
{
    hipStream_t s = ctx->stream;
    const uint64_t host0 = now_ns();
    if (prof_ns)
        HIP_TRY(ctx, hipEventRecord(ctx->ev[0], s));
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, in, in_bytes, hipMemcpyHostToDevice, s));
    const int urc = upload();
    if (urc != MI355_OK)
        return urc;
    if (prof_ns)
        HIP_TRY(ctx, hipEventRecord(ctx->ev[1], s));
    const int rc = launch();
    if (rc != MI355_OK)
        return rc;
    if (prof_ns)
        HIP_TRY(ctx, hipEventRecord(ctx->ev[3], s));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    if (prof_ns)
        HIP_TRY(ctx, hipEventRecord(ctx->ev[5], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (prof_ns)
        return fill_prof(ctx, host0, prof_ns);
    return MI355_OK;
}

template <class Launch>
int timed_roundtrip(mi355_ctx* ctx, void* d_dst, const void* in, size_t in_bytes, uint8_t* out, size_t out_bytes,
                    uint64_t prof_ns[6], Launch launch)
{
    return timed_roundtrip(ctx, d_dst, in, in_bytes, out, out_bytes, prof_ns, [] { return (int)MI355_OK; }, launch);
}

// What a host-buffer call has staged for its round trip through the pooled buffers d_in / d_raw / d_out
struct HostIO {
    bool bgr;  // the host sends 3-byte BGR pixels to d_raw; they are expanded to RGBA in d_in on the device
    size_t in_px, in_bytes, out_bytes;
};

// The untimed half of every host-buffer call, after the call's own pointer and value checks: the input-format rule, the
// device, and the pooled buffers for `in_px` pixels of `in_bpp` bytes each as the kernel reads them (4 or 1) and
// `out_bytes` of output.  Whatever may allocate, free or wait happens here (and in what the caller adds after it: its
// coefficient table, its maps), never inside the timed window.
int stage_host(mi355_ctx* ctx, size_t in_px, int in_bpp, size_t out_bytes, HostIO* io)
{
    const bool bgr = ctx->input_format == MI355_INPUT_BGR;
    if (bgr && in_bpp == 1)
        return MI355_ERR_UNSUPPORTED;  // a gray plane has no BGR form; nothing is converted silently
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *io = {bgr, in_px, in_px * (size_t)in_bpp, out_bytes};
    int rc = ensure(ctx, ctx->d_in, io->in_bytes);
    if (rc == MI355_OK && bgr)
        rc = ensure(ctx, ctx->d_raw, in_px * 3);
    if (rc == MI355_OK)
        rc = ensure(ctx, ctx->d_out, out_bytes);
    return rc;
}

// The timed half: the round trip of what stage_host prepared.  launch() runs the call's kernels from ctx->d_in to
// ctx->d_out; under MI355_INPUT_BGR the BGR2RGBA expansion goes in front of it and counts as kernel time.
template <class Upload, class Launch>
int timed_roundtrip(mi355_ctx* ctx, const HostIO& io, const uint8_t* in, uint8_t* out, uint64_t prof_ns[6],
                    Upload upload, Launch launch)
{
    auto kernels = [&]() -> int {
        if (io.bgr)
            HIP_TRY(ctx, launch_bgr_to_rgba(ctx->stream, static_cast<const uint8_t*>(ctx->d_raw.p),
                                            static_cast<uint8_t*>(ctx->d_in.p), io.in_px));
        return launch();
    };
    return timed_roundtrip(ctx, io.bgr ? ctx->d_raw.p : ctx->d_in.p, in, io.bgr ? io.in_px * 3 : io.in_bytes, out,
                           io.out_bytes, prof_ns, upload, kernels);
}

template <class Launch>
int timed_roundtrip(mi355_ctx* ctx, const HostIO& io, const uint8_t* in, uint8_t* out, uint64_t prof_ns[6],
                    Launch launch)
{
    return timed_roundtrip(ctx, io, in, out, prof_ns, [] { return (int)MI355_OK; }, launch);
}

// The whole of a host-buffer call with frames of `bpp` bytes per pixel in and out, each side with its own shape: the null
// checks, what the call's value check answered (it is pure, so the caller has evaluated it), the staging (BGR input
// with 1-byte frames: unsupported), scratch() for what the family pools beside the frames, outside the timed window, and
// the round trip around dev(), the family's device-resident call from ctx->d_in to ctx->d_out.
template <class Scratch, class Dev>
int frames_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h, int dst_w, int dst_h,
                   int nframes, uint64_t prof_ns[6], int values_rc, Scratch scratch, Dev dev)
{
    if (!ctx || !in || !out)
        return MI355_ERR_BAD_ARG;
    if (values_rc != MI355_OK)
        return values_rc;
    HostIO io;
    int rc = stage_host(ctx, (size_t)src_w * src_h * nframes, bpp, frame_bytes(dst_w, dst_h, nframes, bpp), &io);
    if (rc == MI355_OK)
        rc = scratch();
    if (rc != MI355_OK)
        return rc;
    return timed_roundtrip(ctx, io, in, out, prof_ns, dev);
}

int no_scratch() { return MI355_OK; }  // ... of a family that pools nothing

// One of the several outputs of a host-buffer call: where the caller takes it (null: not taken), its bytes and the
// alignment of its place in the pooled output buffer.  An output the caller does not take has no place there, unless the
// kernels write it regardless (`kept`).
struct HostOut {
    void* host;
    size_t bytes, align;
    bool kept;
    size_t at;  // set by outputs_batched
};

// The place of an output on the device, once outputs_batched has staged the call; null for an output without one
template <class T>
T* out_dev(mi355_ctx* ctx, const HostOut& e)
{
    return e.host || e.kept ? reinterpret_cast<T*>(static_cast<uint8_t*>(ctx->d_out.p) + e.at) : nullptr;
}

// What follows the null and value checks of a host-buffer call with `in_bytes` of 1-byte frames in (BGR input:
// unsupported) and several outputs.  They lie side by side in ctx->d_out in their order; scratch() is what the family
// pools beside them, outside the timed window; dev() is its device-resident call from ctx->d_in to the out_dev()s.  The
// first output the caller takes is what the round trip reads back behind the kernels (from 0: nothing `kept` stands in
// front of it).  The others, a few rows or further planes, leave the device ahead of it: enqueued behind dev() and
// before the kernel-end event, so they count as kernel time.
template <int N, class Scratch, class Dev>
int outputs_batched(mi355_ctx* ctx, const uint8_t* in, size_t in_bytes, HostOut (&o)[N], uint64_t prof_ns[6],
                    Scratch scratch, Dev dev)
{
    size_t total = 0;
    int first = N;  // the caller's null checks have seen to it that one is taken
    for (int i = 0; i < N; i++)
        if (o[i].host || o[i].kept) {
            o[i].at = (total + o[i].align - 1) & ~(o[i].align - 1);
            total = o[i].at + o[i].bytes;
            first = o[i].host && i < first ? i : first;
        }
    HostIO io;
    int rc = stage_host(ctx, in_bytes, 1, total, &io);
    if (rc == MI355_OK)
        rc = scratch();
    if (rc != MI355_OK)
        return rc;
    io.out_bytes = o[first].bytes;
    return timed_roundtrip(ctx, io, in, static_cast<uint8_t*>(o[first].host), prof_ns, [&] {
        const int lrc = dev();
        if (lrc != MI355_OK)
            return lrc;
        for (int i = first + 1; i < N; i++)
            if (o[i].host)
                HIP_TRY(ctx, hipMemcpyAsync(o[i].host, out_dev<void>(ctx, o[i]), o[i].bytes, hipMemcpyDeviceToHost,
                                            ctx->stream));
        return (int)MI355_OK;
    });
}

// H2D, kernel, D2H through the context's pooled buffers
int run_host(mi355_ctx* ctx, int filter, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
             int k, float sigma, uint64_t prof_ns[6])
{
    if (!ctx || !in || !out)
        return MI355_ERR_BAD_ARG;
    const FilterInfo* f = nullptr;
    int rc = check_filter(filter, w, h, nframes, k, sigma, &f);
    if (rc != MI355_OK)
        return rc;
    HostIO io;
    rc = stage_host(ctx, (size_t)w * h * nframes, f->in_bpp, frame_bytes(w, h, nframes, f->out_bpp), &io);
    const GaussCoef* coef = nullptr;
    if (rc == MI355_OK && f->table)
        rc = get_coef(ctx, k, sigma, &coef);  // built / uploaded outside the timed write/kernel/read window
    if (rc != MI355_OK)
        return rc;
    return timed_roundtrip(ctx, io, in, out, prof_ns, [&] {
        return dispatch_dev(ctx, filter, ctx->d_in.p, ctx->d_out.p, w, h, nframes, k, sigma);
    });
}

// cv::warpAffine's inverse map: m itself under MI355_WARP_INVERSE_MAP, else OpenCV's inversion, operation by operation
// (fp64, nothing fused: the library is built with -ffp-contract=off).  A singular matrix gives the all-zero map.
void warp_inverse(const double m[6], int flags, double inv[6])
{
    if (flags & MI355_WARP_INVERSE_MAP) {
        for (int i = 0; i < 6; i++)
            inv[i] = m[i];
        return;
    }
    double D = m[0] * m[4] - m[1] * m[3];
    D = (D != 0.0) ? 1.0 / D : 0.0;
    const double A11 = m[4] * D, A22 = m[0] * D;
    inv[0] = A11;
    inv[1] = m[1] * (-D);
    inv[3] = m[3] * (-D);
    inv[4] = A22;
    inv[2] = -inv[0] * m[2] - inv[1] * m[5];
    inv[5] = -inv[3] * m[2] - inv[4] * m[5];
}

bool warp_flags_ok(int flags)
{
    const int interp = flags & ~MI355_WARP_INVERSE_MAP;
    return interp == MI355_INTERP_NEAREST || interp == MI355_INTERP_LINEAR;
}

bool all_finite(const double* m, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(m[i]))
            return false;
    return true;
}

// The argument errors every geometric call with two shapes shares
bool bad_shapes(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int border_mode)
{
    return (bpp != 1 && bpp != 4) || (border_mode != MI355_BORDER_CONSTANT && border_mode != MI355_BORDER_REPLICATE) ||
           src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 || nframes <= 0;
}

// ... and what follows them (and the matrix, where there is one): the size limit, then the number of pixels
int check_shape_limits(int src_w, int src_h, int dst_w, int dst_h, int nframes)
{
    if (src_w > MI355_MAX_WARP_SIZE || src_h > MI355_MAX_WARP_SIZE || dst_w > MI355_MAX_WARP_SIZE ||
        dst_h > MI355_MAX_WARP_SIZE)
        return MI355_ERR_UNSUPPORTED;
    if (!valid_sizes(src_w, src_h, nframes) || !valid_sizes(dst_w, dst_h, nframes))
        return MI355_ERR_BAD_ARG;
    return MI355_OK;
}

// The value checks of the warp calls, before any HIP call: bytes per pixel, flags, border mode, both shapes, the matrix;
// then the sizes and the inverse map the fixed-point arithmetic takes.  inv (may be null) gets the inverse map.
int check_warp(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, const double* m, int flags,
               int border_mode, double* inv)
{
    if (!m || !warp_flags_ok(flags) || bad_shapes(bpp, src_w, src_h, dst_w, dst_h, nframes, border_mode) ||
        !all_finite(m, 6))
        return MI355_ERR_BAD_ARG;
    const int rc = check_shape_limits(src_w, src_h, dst_w, dst_h, nframes);
    if (rc != MI355_OK)
        return rc;
    double i[6];
    warp_inverse(m, flags, i);
    if (warp_work_items(i, dst_w, dst_h, nframes) > 0x7FFFFFF0ull)
        return MI355_ERR_BAD_ARG;
    const double limit = 1048576.0;  // 2^20: below it no int sum of the coordinate arithmetic overflows
    const double rx = std::fabs(i[0]) * (double)(dst_w - 1) + std::fabs(i[1]) * (double)(dst_h - 1) + std::fabs(i[2]);
    const double ry = std::fabs(i[3]) * (double)(dst_w - 1) + std::fabs(i[4]) * (double)(dst_h - 1) + std::fabs(i[5]);
    if (!(rx < limit) || !(ry < limit))  // an inverse that overflowed to inf or nan lands here too
        return MI355_ERR_UNSUPPORTED;
    if (inv)
        for (int k = 0; k < 6; k++)
            inv[k] = i[k];
    return MI355_OK;
}

// The shape checks of the remap and perspective calls: check_warp's, in its order, with the amount of work of remap.hip's
// launches
int check_two_shapes(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int border_mode)
{
    if (bad_shapes(bpp, src_w, src_h, dst_w, dst_h, nframes, border_mode))
        return MI355_ERR_BAD_ARG;
    const int rc = check_shape_limits(src_w, src_h, dst_w, dst_h, nframes);
    if (rc == MI355_OK && remap_work_items(dst_w, dst_h, nframes) > 0x7FFFFFF0ull)
        return MI355_ERR_BAD_ARG;
    return rc;
}

// bytes of the two maps of a remap call; map2 of FIXED + NEAREST is not read
void map_bytes(int dst_w, int dst_h, int map_kind, size_t* n1, size_t* n2)
{
    const size_t entries = (size_t)dst_w * dst_h;
    *n1 = entries * 4;
    *n2 = entries * (map_kind == MI355_MAP_FIXED ? 2 : 4);
}

// cv::warpPerspective's inverse map: m itself under MI355_WARP_INVERSE_MAP, else the adjugate times 1 / det, operation
// by operation (fp64, nothing fused).  A singular matrix gives the all-zero map.
void perspective_inverse(const double m[9], int flags, double inv[9])
{
    if (flags & MI355_WARP_INVERSE_MAP) {
        for (int i = 0; i < 9; i++)
            inv[i] = m[i];
        return;
    }
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                       m[2] * (m[3] * m[7] - m[4] * m[6]);
    const double d = (det != 0.0) ? 1.0 / det : 0.0;
    inv[0] = (m[4] * m[8] - m[5] * m[7]) * d;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) * d;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    inv[3] = (m[5] * m[6] - m[3] * m[8]) * d;
    inv[4] = (m[0] * m[8] - m[2] * m[6]) * d;
    inv[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    inv[6] = (m[3] * m[7] - m[4] * m[6]) * d;
    inv[7] = (m[1] * m[6] - m[0] * m[7]) * d;
    inv[8] = (m[0] * m[4] - m[1] * m[3]) * d;
}

// The value checks of the perspective calls, before any HIP call.  inv (may be null) gets the inverse map.
int check_perspective(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, const double* m, int flags,
                      int border_mode, double* inv)
{
    // a non-finite entry is an argument error even where the size limit would answer UNSUPPORTED (check_warp's order)
    if (!m || !warp_flags_ok(flags) || bad_shapes(bpp, src_w, src_h, dst_w, dst_h, nframes, border_mode) ||
        !all_finite(m, 9))
        return MI355_ERR_BAD_ARG;
    const int rc = check_two_shapes(bpp, src_w, src_h, dst_w, dst_h, nframes, border_mode);
    if (rc == MI355_OK && inv)
        perspective_inverse(m, flags, inv);
    return rc;
}

// cv::adaptiveThreshold's integer delta: ceil for BINARY, floor for BINARY_INV; beyond +-256 the output is constant
int adaptive_idelta(int type, double delta)
{
    const double d = type == MI355_ADAPTIVE_BINARY ? std::ceil(delta) : std::floor(delta);
    return d < -256.0 ? -256 : (d > 256.0 ? 256 : (int)d);
}

int create_common(int device, hipStream_t stream, bool own, mi355_ctx** out)
{
    if (!out)
        return MI355_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return MI355_ERR_NO_DEVICE;
    if (device < 0 || device >= n)
        return MI355_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return MI355_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return MI355_ERR_UNSUPPORTED;  // the code objects in this library are gfx950 only
    mi355_ctx* ctx = new (std::nothrow) mi355_ctx();
    if (!ctx)
        return MI355_ERR_NOMEM;
    ctx->device = device;
    std::snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
    bool ok = hipSetDevice(device) == hipSuccess;
    if (ok && own)
        ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
    ctx->stream = stream;
    ctx->own_stream = own && ok;
    for (int i = 0; ok && i < 6; i++)
        ok = hipEventCreate(&ctx->ev[i]) == hipSuccess;
    ok = ok && hipEventCreate(&ctx->t0) == hipSuccess && hipEventCreate(&ctx->t1) == hipSuccess;
    ok = ok && hipMalloc((void**)&ctx->d_acc, sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        mi355_ctx_destroy(ctx);
        return MI355_ERR_HIP;
    }
    *out = ctx;
    return MI355_OK;
}

}  // namespace

extern "C" {

#define MI355_API __attribute__((visibility("default")))

MI355_API int mi355_device_count(int* count)
{
    if (!count)
        return MI355_ERR_BAD_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        n = 0;
    *count = n;
    return MI355_OK;
}

MI355_API int mi355_ctx_create(int device, mi355_ctx** out)
{
    return create_common(device, nullptr, true, out);
}

MI355_API int mi355_ctx_create_on_stream(int device, void* hip_stream, mi355_ctx** out)
{
    return create_common(device, static_cast<hipStream_t>(hip_stream), false, out);
}

MI355_API int mi355_ctx_destroy(mi355_ctx* ctx)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& e : ctx->coefs)
        (void)hipFree(e.d_buf);
    for (void* p : ctx->pinned)
        (void)hipHostFree(p);
    for (void* p : {(void*)ctx->d_acc, (void*)ctx->d_img_table, ctx->d_in.p, ctx->d_out.p, ctx->d_raw.p, ctx->d_flags.p,
                    ctx->d_hist.p, ctx->d_lut.p, ctx->d_ccl.p, ctx->d_dist.p, ctx->d_parent.p, ctx->d_hough.p, ctx->d_hough_acc.p,
                    (void*)ctx->d_hough_tab, ctx->d_map1.p, ctx->d_map2.p})
        if (p)
            (void)hipFree(p);
    for (int i = 0; i < mi355_ctx::kSlots; i++) {
        for (void* p : {ctx->slot_in[i].p, ctx->slot_out[i].p, ctx->slot_raw[i].p})
            if (p)
                (void)hipFree(p);
        for (hipEvent_t ev : {ctx->ev_h2d[i], ctx->ev_k[i], ctx->ev_d2h[i]})
            if (ev)
                (void)hipEventDestroy(ev);
    }
    for (hipStream_t s : {ctx->s_h2d, ctx->s_d2h})
        if (s)
            (void)hipStreamDestroy(s);
    for (hipEvent_t ev : {ctx->ev[0], ctx->ev[1], ctx->ev[2], ctx->ev[3], ctx->ev[4], ctx->ev[5], ctx->t0, ctx->t1})
        if (ev)
            (void)hipEventDestroy(ev);
    if (ctx->own_stream && ctx->stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MI355_OK;
}

MI355_API int mi355_ctx_device_name(mi355_ctx* ctx, char* buf, size_t buflen)
{
    if (!ctx || !buf || buflen == 0)
        return MI355_ERR_BAD_ARG;
    std::snprintf(buf, buflen, "%s", ctx->name);
    return MI355_OK;
}

MI355_API int mi355_sync(mi355_ctx* ctx)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

MI355_API int mi355_last_hip_error(mi355_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

MI355_API const char* mi355_strerror(int code)
{
    switch (code) {
    case MI355_OK: return "ok";
    case MI355_ERR_BAD_ARG: return "bad argument";
    case MI355_ERR_HIP: return "HIP runtime error";
    case MI355_ERR_NO_DEVICE: return "no such GPU";
    case MI355_ERR_UNSUPPORTED: return "unsupported (library is built for gfx950 only)";
    case MI355_ERR_NOMEM: return "out of memory";
    default: return "unknown error";
    }
}

MI355_API int mi355_ctx_set_gauss_mode(mi355_ctx* ctx, int mode)
{
    if (!ctx || (mode != MI355_GAUSS_FAST && mode != MI355_GAUSS_EXACT))
        return MI355_ERR_BAD_ARG;
    ctx->gauss_mode = mode;
    return MI355_OK;
}

MI355_API int mi355_ctx_set_impl(mi355_ctx* ctx, int impl)
{
    if (!ctx || impl < MI355_IMPL_AUTO || impl > MI355_IMPL_VALU)
        return MI355_ERR_BAD_ARG;
    ctx->impl = impl;
    return MI355_OK;
}

MI355_API int mi355_ctx_set_input_format(mi355_ctx* ctx, int format)
{
    if (!ctx || (format != MI355_INPUT_RGBA && format != MI355_INPUT_BGR))
        return MI355_ERR_BAD_ARG;
    ctx->input_format = format;
    return MI355_OK;
}

MI355_API int mi355_bgr_to_rgba8_dev(mi355_ctx* ctx, const void* d_bgr, void* d_rgba, int w, int h, int nframes)
{
    if (!ctx || !d_bgr || !d_rgba || !valid_sizes(w, h, nframes) || (reinterpret_cast<uintptr_t>(d_rgba) & 3u))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_bgr_to_rgba(ctx->stream, static_cast<const uint8_t*>(d_bgr), static_cast<uint8_t*>(d_rgba),
                                    (size_t)w * h * nframes));
    return MI355_OK;
}

MI355_API int mi355_gauss_weights(int k, float sigma, float* out_k2)
{
    if (!out_k2 || !valid_k(k) || !valid_sigma(sigma))
        return MI355_ERR_BAD_ARG;
    gen_weights(k, sigma, out_k2);
    return MI355_OK;
}

MI355_API int mi355_gauss_weights_image2d(int k, float sigma, float* out_k2)
{
    if (!out_k2 || !valid_k(k) || !valid_sigma(sigma))
        return MI355_ERR_BAD_ARG;
    gen_weights_image2d(k, sigma, out_k2);
    return MI355_OK;
}

MI355_API int mi355_image2d_rgba8(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w, int h, int k,
                                  float sigma, uint64_t prof_ns[6])
{
    if (!ctx || !rgba || !out || !valid_sizes(w, h, 1) ||
        (filter != MI355_FILTER_GRAY && filter != MI355_FILTER_GAUSS && filter != MI355_FILTER_SOBEL))
        return MI355_ERR_BAD_ARG;
    const bool gauss = filter == MI355_FILTER_GAUSS;
    if (gauss && (!valid_k(k) || !valid_sigma(sigma)))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)w * h, in_bytes = npx * 4, out_bytes = npx * (gauss ? 4 : 1);
    int rc = ensure(ctx, ctx->d_in, in_bytes);
    if (rc == MI355_OK)
        rc = ensure(ctx, ctx->d_out, out_bytes);
    if (rc != MI355_OK)
        return rc;
    if (gauss) {
        if (!ctx->d_img_table)
            HIP_TRY(ctx, hipMalloc((void**)&ctx->d_img_table, sizeof(float) * MI355_MAX_GAUSS_K * MI355_MAX_GAUSS_K));
        std::vector<float> table((size_t)k * k);
        gen_weights_image2d(k, sigma, table.data());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a kernel in flight may still read the previous table
        HIP_TRY(ctx, hipMemcpy(ctx->d_img_table, table.data(), sizeof(float) * table.size(), hipMemcpyHostToDevice));
    }
    return timed_roundtrip(ctx, ctx->d_in.p, rgba, in_bytes, out, out_bytes, prof_ns, [&] {
        HIP_TRY(ctx, launch_image2d(ctx->stream, filter, static_cast<const uint8_t*>(ctx->d_in.p),
                                    static_cast<uint8_t*>(ctx->d_out.p), w, h, 1, k, ctx->d_img_table));
        return MI355_OK;
    });
}

MI355_API int mi355_ctx_set_gauss_weights(mi355_ctx* ctx, int k, float sigma, const float* w_k2)
{
    if (!ctx || !w_k2 || !valid_k(k) || !valid_sigma(sigma))
        return MI355_ERR_BAD_ARG;
    for (int i = 0; i < k * k; i++)
        if (!std::isfinite(w_k2[i]))
            return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // a kernel still in flight may be reading the previous table of this key
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return install_coef(ctx, k, sigma, w_k2, true, nullptr);
}

MI355_API int mi355_filter_out_bpp(int filter)
{
    const FilterInfo* f = filter_info(filter);
    return f ? f->out_bpp : MI355_ERR_BAD_ARG;
}

MI355_API int mi355_filter_in_bpp(int filter)
{
    const FilterInfo* f = filter_info(filter);
    return f ? f->in_bpp : MI355_ERR_BAD_ARG;
}

MI355_API int mi355_gray_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out, int w, int h,
                               uint64_t prof_ns[6])
{
    return run_host(ctx, MI355_FILTER_GRAY, rgba, out, w, h, 1, 0, 0.0f, prof_ns);
}

MI355_API int mi355_gray1_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out, int w, int h,
                                uint64_t prof_ns[6])
{
    return run_host(ctx, MI355_FILTER_GRAY1, rgba, out, w, h, 1, 0, 0.0f, prof_ns);
}

MI355_API int mi355_gauss_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out, int w, int h, int k,
                                float sigma, uint64_t prof_ns[6])
{
    return run_host(ctx, MI355_FILTER_GAUSS, rgba, out, w, h, 1, k, sigma, prof_ns);
}

MI355_API int mi355_sobel_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out, int w, int h,
                                uint64_t prof_ns[6])
{
    return run_host(ctx, MI355_FILTER_SOBEL, rgba, out, w, h, 1, 0, 0.0f, prof_ns);
}

MI355_API int mi355_pipeline_rgba8(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* out, int w, int h,
                                   int k, float sigma, uint64_t prof_ns[6])
{
    return run_host(ctx, MI355_FILTER_PIPELINE, rgba, out, w, h, 1, k, sigma, prof_ns);
}

MI355_API int mi355_filter_batched(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w,
                                   int h, int nframes, int k, float sigma, uint64_t prof_ns[6])
{
    return run_host(ctx, filter, rgba, out, w, h, nframes, k, sigma, prof_ns);
}

MI355_API int mi355_host_alloc(mi355_ctx* ctx, size_t nbytes, void** h_ptr)
{
    if (!ctx || !h_ptr || nbytes == 0)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipHostMalloc(h_ptr, nbytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        ctx->last_hip = (int)e;
        *h_ptr = nullptr;
        return MI355_ERR_NOMEM;
    }
    ctx->pinned.push_back(*h_ptr);
    return MI355_OK;
}

MI355_API int mi355_host_free(mi355_ctx* ctx, void* h_ptr)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    if (!h_ptr)
        return MI355_OK;
    for (size_t i = 0; i < ctx->pinned.size(); i++)
        if (ctx->pinned[i] == h_ptr) {
            ctx->pinned.erase(ctx->pinned.begin() + i);
            HIP_TRY(ctx, hipHostFree(h_ptr));
            return MI355_OK;
        }
    return MI355_ERR_BAD_ARG;  // not a block of this context
}

MI355_API int mi355_filter_stream(mi355_ctx* ctx, int filter, const uint8_t* rgba, uint8_t* out, int w, int h,
                                  int nframes, int chunk_frames, int k, float sigma, double* elapsed_ms)
{
    if (!ctx || !rgba || !out || chunk_frames < 0)
        return MI355_ERR_BAD_ARG;
    const FilterInfo* f = nullptr;
    int rc = check_filter(filter, w, h, nframes, k, sigma, &f);
    if (rc != MI355_OK)
        return rc;
    const bool bgr = ctx->input_format == MI355_INPUT_BGR;
    if (bgr && f->in_bpp == 1)
        return MI355_ERR_UNSUPPORTED;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t fpx = (size_t)w * h, bpp = (size_t)f->out_bpp;
    const size_t dev_in_bpp = (size_t)f->in_bpp;  // what the kernel reads: 4 (RGBA) or 1 (gray8)
    if (chunk_frames == 0) {
        // ~64 MB of input per chunk: long enough DMA transfers to run at link rate, short enough to overlap
        chunk_frames = (int)((64u << 20) / (fpx * dev_in_bpp));
        if (chunk_frames < 1)
            chunk_frames = 1;
    }
    if (chunk_frames > nframes)
        chunk_frames = nframes;
    constexpr int NS = mi355_ctx::kSlots;
    if (!ctx->s_h2d) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_h2d, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_d2h, hipStreamNonBlocking));
        for (int i = 0; i < NS; i++) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_h2d[i], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_k[i], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_d2h[i], hipEventDisableTiming));
        }
    }
    const size_t in_bpp = bgr ? 3 : dev_in_bpp;  // what crosses PCIe
    rc = bgr ? ensure_slots(ctx, ctx->slot_raw, fpx * 3 * chunk_frames) : MI355_OK;
    if (rc == MI355_OK)
        rc = ensure_slots(ctx, ctx->slot_in, fpx * dev_in_bpp * chunk_frames);
    if (rc == MI355_OK)
        rc = ensure_slots(ctx, ctx->slot_out, fpx * bpp * chunk_frames);
    const GaussCoef* coef = nullptr;
    if (rc == MI355_OK && f->table)
        rc = get_coef(ctx, k, sigma, &coef);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t t0 = now_ns();
    const int nchunks = (nframes + chunk_frames - 1) / chunk_frames;
    for (int c = 0; c < nchunks; c++) {
        const int slot = c % NS;
        const int f0 = c * chunk_frames;
        const int nf = (nframes - f0 < chunk_frames) ? nframes - f0 : chunk_frames;
        // input slot is free once the kernel of chunk c-NS has read it
        if (c >= NS)
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_h2d, ctx->ev_k[slot], 0));
        HIP_TRY(ctx, hipMemcpyAsync(bgr ? ctx->slot_raw[slot].p : ctx->slot_in[slot].p,
                                    rgba + (size_t)f0 * fpx * in_bpp, fpx * in_bpp * nf, hipMemcpyHostToDevice,
                                    ctx->s_h2d));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_h2d[slot], ctx->s_h2d));
        // kernel: needs its input, and its output slot drained by the D2H of chunk c-NS
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_h2d[slot], 0));
        if (c >= NS)
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_d2h[slot], 0));
        if (bgr)
            HIP_TRY(ctx, launch_bgr_to_rgba(ctx->stream, static_cast<const uint8_t*>(ctx->slot_raw[slot].p),
                                            static_cast<uint8_t*>(ctx->slot_in[slot].p), fpx * nf));
        rc = dispatch_dev(ctx, filter, ctx->slot_in[slot].p, ctx->slot_out[slot].p, w, h, nf, k, sigma);
        if (rc != MI355_OK) {
            (void)hipDeviceSynchronize();
            return rc;
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k[slot], ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->ev_k[slot], 0));
        HIP_TRY(ctx, hipMemcpyAsync(out + (size_t)f0 * fpx * bpp, ctx->slot_out[slot].p, fpx * bpp * nf,
                                    hipMemcpyDeviceToHost, ctx->s_d2h));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_d2h[slot], ctx->s_d2h));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_d2h));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_h2d));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (elapsed_ms)
        *elapsed_ms = (double)(now_ns() - t0) * 1e-6;
    return MI355_OK;
}

MI355_API int mi355_filter_dev(mi355_ctx* ctx, int filter, const void* d_in, void* d_out, int w, int h,
                               int nframes, int k, float sigma)
{
    return dispatch_dev(ctx, filter, d_in, d_out, w, h, nframes, k, sigma);
}

// The value checks of the resize calls, before any HIP call: bytes per pixel, interpolation, both shapes; then AREA's
// integer factors.  LINEAR at exactly half size is AREA 2 x 2, which always has them.
MI355_API int mi355_resize_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int interp)
{
    if ((bpp != 1 && bpp != 4) ||
        (interp != MI355_INTERP_NEAREST && interp != MI355_INTERP_LINEAR && interp != MI355_INTERP_AREA) ||
        !valid_sizes(src_w, src_h, nframes) || !valid_sizes(dst_w, dst_h, nframes))
        return MI355_ERR_BAD_ARG;
    if (src_w >= (1 << 29) || dst_w >= (1 << 29))  // a lane's byte offset inside a row is 32-bit
        return MI355_ERR_BAD_ARG;
    int nx = 0, ny = 0;
    if (interp == MI355_INTERP_AREA && !resize_area_factors(src_w, src_h, dst_w, dst_h, &nx, &ny))
        return MI355_ERR_UNSUPPORTED;
    return MI355_OK;
}

MI355_API int mi355_resize_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h, int dst_w,
                               int dst_h, int nframes, int interp)
{
    const int rc = frames_dev(ctx, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, nframes,
                              mi355_resize_check(bpp, src_w, src_h, dst_w, dst_h, nframes, interp));
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_resize(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out), bpp, src_w,
                               src_h, dst_w, dst_h, nframes, interp));
    return MI355_OK;
}

// The host-buffer form of this and of every later call: H2D, one launch, D2H through the pooled buffers, each side
// sized by its own shape
MI355_API int mi355_resize_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                                   int dst_w, int dst_h, int nframes, int interp, uint64_t prof_ns[6])
{
    const int vrc = mi355_resize_check(bpp, src_w, src_h, dst_w, dst_h, nframes, interp);
    return frames_batched(ctx, in, out, bpp, src_w, src_h, dst_w, dst_h, nframes, prof_ns, vrc, no_scratch, [&] {
        return mi355_resize_dev(ctx, ctx->d_in.p, ctx->d_out.p, bpp, src_w, src_h, dst_w, dst_h, nframes, interp);
    });
}

MI355_API int mi355_rotation_matrix(double cx, double cy, double angle_deg, double scale, double m[6])
{
    if (!m || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(angle_deg) || !std::isfinite(scale) ||
        scale == 0.0)
        return MI355_ERR_BAD_ARG;
    const double rad = angle_deg * 3.14159265358979323846 / 180.0;
    const double a = std::cos(rad) * scale, b = std::sin(rad) * scale;
    m[0] = a;
    m[1] = b;
    m[2] = (1.0 - a) * cx - b * cy;
    m[3] = -b;
    m[4] = a;
    m[5] = b * cx + (1.0 - a) * cy;
    return MI355_OK;
}

MI355_API int mi355_warp_affine_matrix(const double m[6], int flags, double inv[6])
{
    if (!m || !inv || !warp_flags_ok(flags) || !all_finite(m, 6))
        return MI355_ERR_BAD_ARG;
    warp_inverse(m, flags, inv);
    return MI355_OK;
}

MI355_API int mi355_warp_affine_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes,
                                      const double m[6], int flags, int border_mode)
{
    return check_warp(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, nullptr);
}

MI355_API int mi355_warp_affine_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h,
                                    int dst_w, int dst_h, int nframes, const double m[6], int flags, int border_mode,
                                    uint32_t border_value)
{
    double inv[6];
    const int rc = frames_dev(ctx, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, nframes,
                              check_warp(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, inv));
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_warp_affine(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out), bpp,
                                    src_w, src_h, dst_w, dst_h, nframes, inv, flags & ~MI355_WARP_INVERSE_MAP, border_mode,
                                    border_value));
    return MI355_OK;
}

MI355_API int mi355_warp_affine_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                                        int dst_w, int dst_h, int nframes, const double m[6], int flags, int border_mode,
                                        uint32_t border_value, uint64_t prof_ns[6])
{
    const int vrc = check_warp(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, nullptr);
    return frames_batched(ctx, in, out, bpp, src_w, src_h, dst_w, dst_h, nframes, prof_ns, vrc, no_scratch, [&] {
        return mi355_warp_affine_dev(ctx, ctx->d_in.p, ctx->d_out.p, bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags,
                                     border_mode, border_value);
    });
}

MI355_API int mi355_remap_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes, int map_kind,
                                int interp, int border_mode)
{
    if ((map_kind != MI355_MAP_FIXED && map_kind != MI355_MAP_FLOAT) ||
        (interp != MI355_INTERP_NEAREST && interp != MI355_INTERP_LINEAR))
        return MI355_ERR_BAD_ARG;
    return check_two_shapes(bpp, src_w, src_h, dst_w, dst_h, nframes, border_mode);
}

MI355_API int mi355_remap_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h, int dst_w,
                              int dst_h, int nframes, const void* d_map1, const void* d_map2, int map_kind, int interp,
                              int border_mode, uint32_t border_value)
{
    if (!ctx || !d_in || !d_out || !d_map1)
        return MI355_ERR_BAD_ARG;
    const int rc = mi355_remap_check(bpp, src_w, src_h, dst_w, dst_h, nframes, map_kind, interp, border_mode);
    if (rc != MI355_OK)
        return rc;
    if (!d_map2 && !(map_kind == MI355_MAP_FIXED && interp == MI355_INTERP_NEAREST))
        return MI355_ERR_BAD_ARG;
    size_t n1 = 0, n2 = 0;
    map_bytes(dst_w, dst_h, map_kind, &n1, &n2);
    if (bad_ranges({rd(d_in, frame_bytes(src_w, src_h, nframes, bpp), bpp),
                    wr(d_out, frame_bytes(dst_w, dst_h, nframes, bpp), bpp), rd(d_map1, n1, 4),
                    rd(d_map2, n2, map_kind == MI355_MAP_FIXED ? 2 : 4)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_remap(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out), bpp, src_w,
                              src_h, dst_w, dst_h, nframes, d_map1, d_map2, map_kind, interp, border_mode, border_value));
    return MI355_OK;
}

MI355_API int mi355_remap_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w, int src_h,
                                  int dst_w, int dst_h, int nframes, const void* map1, const void* map2, int map_kind,
                                  int interp, int border_mode, uint32_t border_value, uint64_t prof_ns[6])
{
    if (!ctx || !in || !out || !map1)
        return MI355_ERR_BAD_ARG;
    int rc = mi355_remap_check(bpp, src_w, src_h, dst_w, dst_h, nframes, map_kind, interp, border_mode);
    if (rc != MI355_OK)
        return rc;
    if (!map2 && !(map_kind == MI355_MAP_FIXED && interp == MI355_INTERP_NEAREST))
        return MI355_ERR_BAD_ARG;
    HostIO io;
    rc = stage_host(ctx, (size_t)src_w * src_h * nframes, bpp, frame_bytes(dst_w, dst_h, nframes, bpp), &io);
    size_t n1 = 0, n2 = 0;
    map_bytes(dst_w, dst_h, map_kind, &n1, &n2);
    if (rc == MI355_OK)
        rc = ensure(ctx, ctx->d_map1, n1);
    if (rc == MI355_OK && map2)
        rc = ensure(ctx, ctx->d_map2, n2);
    if (rc != MI355_OK)
        return rc;
    auto upload = [&] {  // the maps travel with the frames: H2D time
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_map1.p, map1, n1, hipMemcpyHostToDevice, ctx->stream));
        if (map2)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_map2.p, map2, n2, hipMemcpyHostToDevice, ctx->stream));
        return (int)MI355_OK;
    };
    return timed_roundtrip(ctx, io, in, out, prof_ns, upload, [&] {
        return mi355_remap_dev(ctx, ctx->d_in.p, ctx->d_out.p, bpp, src_w, src_h, dst_w, dst_h, nframes, ctx->d_map1.p,
                               map2 ? ctx->d_map2.p : nullptr, map_kind, interp, border_mode, border_value);
    });
}

MI355_API int mi355_perspective_matrix(const double m[9], int flags, double inv[9])
{
    if (!m || !inv || !warp_flags_ok(flags) || !all_finite(m, 9))
        return MI355_ERR_BAD_ARG;
    perspective_inverse(m, flags, inv);
    return MI355_OK;
}

MI355_API int mi355_warp_perspective_check(int bpp, int src_w, int src_h, int dst_w, int dst_h, int nframes,
                                           const double m[9], int flags, int border_mode)
{
    return check_perspective(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, nullptr);
}

MI355_API int mi355_warp_perspective_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int bpp, int src_w, int src_h,
                                         int dst_w, int dst_h, int nframes, const double m[9], int flags,
                                         int border_mode, uint32_t border_value)
{
    double inv[9];
    const int rc = frames_dev(ctx, d_in, d_out, bpp, src_w, src_h, dst_w, dst_h, nframes,
                              check_perspective(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, inv));
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_warp_perspective(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out),
                                         bpp, src_w, src_h, dst_w, dst_h, nframes, inv, flags & ~MI355_WARP_INVERSE_MAP,
                                         border_mode, border_value));
    return MI355_OK;
}

MI355_API int mi355_warp_perspective_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int bpp, int src_w,
                                             int src_h, int dst_w, int dst_h, int nframes, const double m[9], int flags,
                                             int border_mode, uint32_t border_value, uint64_t prof_ns[6])
{
    const int vrc = check_perspective(bpp, src_w, src_h, dst_w, dst_h, nframes, m, flags, border_mode, nullptr);
    return frames_batched(ctx, in, out, bpp, src_w, src_h, dst_w, dst_h, nframes, prof_ns, vrc, no_scratch, [&] {
        return mi355_warp_perspective_dev(ctx, ctx->d_in.p, ctx->d_out.p, bpp, src_w, src_h, dst_w, dst_h, nframes, m,
                                          flags, border_mode, border_value);
    });
}

MI355_API int mi355_adaptive_threshold_check(int w, int h, int nframes, int max_value, int type, int block,
                                             double delta)
{
    if (!valid_sizes(w, h, nframes) || !odd_in(block, 3, MI355_MAX_BOX_K) || max_value < 0 || max_value > 255 ||
        (type != MI355_ADAPTIVE_BINARY && type != MI355_ADAPTIVE_BINARY_INV) || !std::isfinite(delta))
        return MI355_ERR_BAD_ARG;
    return MI355_OK;
}

MI355_API int mi355_adaptive_threshold_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                                 int nframes, int max_value, int type, int block, double delta)
{
    const int rc = frames_dev(ctx, d_in, d_out, 1, w, h, w, h, nframes,
                              mi355_adaptive_threshold_check(w, h, nframes, max_value, type, block, delta));
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_adaptive_threshold(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out),
                                           w, h, nframes, block, max_value, type == MI355_ADAPTIVE_BINARY_INV,
                                           adaptive_idelta(type, delta)));
    return MI355_OK;
}

MI355_API int mi355_adaptive_threshold_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h,
                                                     int nframes, int max_value, int type, int block, double delta,
                                                     uint64_t prof_ns[6])
{
    const int vrc = mi355_adaptive_threshold_check(w, h, nframes, max_value, type, block, delta);
    return frames_batched(ctx, in, out, 1, w, h, w, h, nframes, prof_ns, vrc, no_scratch, [&] {
        return mi355_adaptive_threshold_gray8_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, max_value, type, block,
                                                  delta);
    });
}

// the pooled scratch of the statistics and CLAHE calls: 1 KiB of histogram and 256 B of table per frame or tile (row)
static int hist_scratch(mi355_ctx* ctx, size_t rows)
{
    const int rc = ensure(ctx, ctx->d_hist, rows * 256 * sizeof(uint32_t));
    return rc == MI355_OK ? ensure(ctx, ctx->d_lut, rows * 256) : rc;
}

// that scratch with the histograms, ctx->d_hist.p, zeroed in-stream
static int zeroed_hists(mi355_ctx* ctx, size_t rows)
{
    const int rc = hist_scratch(ctx, rows);
    if (rc == MI355_OK)
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_hist.p, 0, rows * 256 * sizeof(uint32_t), ctx->stream));
    return rc;
}

namespace {
int hist_tables(mi355_ctx* ctx, const uint8_t* in, int32_t* d_thresh, int w, int h, int nframes, bool otsu)
{
    const int rc = zeroed_hists(ctx, (size_t)nframes);
    if (rc != MI355_OK)
        return rc;
    uint32_t* hist = static_cast<uint32_t*>(ctx->d_hist.p);
    HIP_TRY(ctx, launch_hist(ctx->stream, in, hist, w, h, nframes));
    HIP_TRY(ctx, launch_hist_table(ctx->stream, hist, static_cast<uint8_t*>(ctx->d_lut.p), d_thresh, w, h, nframes,
                                   otsu));
    return MI355_OK;
}
}  // namespace

// the argument checks of the two statistics calls: mi355_filter_dev's, with `nout` bytes of 4-byte aligned output
static int check_stats_call(mi355_ctx* ctx, const void* d_in, const void* d_out, int w, int h, int nframes, size_t nout)
{
    if (!ctx || !d_in || !d_out)
        return MI355_ERR_BAD_ARG;
    const int rc = check_filter(MI355_FILTER_EQUALIZE_GRAY8, w, h, nframes, 0, 0.0f, nullptr);
    if (rc != MI355_OK)
        return rc;
    if (bad_ranges({rd(d_in, frame_bytes(w, h, nframes, 1), 1), wr(d_out, nout, 4)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return MI355_OK;
}

MI355_API int mi355_hist_gray8_dev(mi355_ctx* ctx, const void* d_in, uint32_t* d_hist, int w, int h, int nframes)
{
    const size_t nbytes = (size_t)(nframes > 0 ? nframes : 0) * 256 * sizeof(uint32_t);
    const int rc = check_stats_call(ctx, d_in, d_hist, w, h, nframes, nbytes);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, nbytes, ctx->stream));
    HIP_TRY(ctx, launch_hist(ctx->stream, static_cast<const uint8_t*>(d_in), d_hist, w, h, nframes));
    return MI355_OK;
}

MI355_API int mi355_otsu_thresholds_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_thresh, int w, int h,
                                              int nframes)
{
    const size_t nbytes = (size_t)(nframes > 0 ? nframes : 0) * sizeof(int32_t);
    const int rc = check_stats_call(ctx, d_in, d_thresh, w, h, nframes, nbytes);
    return rc == MI355_OK ? hist_tables(ctx, static_cast<const uint8_t*>(d_in), d_thresh, w, h, nframes, true) : rc;
}

// The value checks of every CLAHE call and, when they pass, the call's geometry: the extended frame's tile size, the
// clip limit in counts and the three fp32 scales the kernels take by value (include/mi355_imgfilter.h, "local contrast")
static int clahe_plan(int w, int h, int nframes, double clip_limit, int tiles_x, int tiles_y, ClaheGeom* g)
{
    static_assert(MI355_MAX_CLAHE_TILES == kClaheMaxTiles, "the header's limit is the kernels' limit");
    if (!valid_sizes(w, h, nframes) || tiles_x < 1 || tiles_x > MI355_MAX_CLAHE_TILES || tiles_y < 1 ||
        tiles_y > MI355_MAX_CLAHE_TILES || !std::isfinite(clip_limit))
        return MI355_ERR_BAD_ARG;
    // OpenCV's quirk: when either dimension fails to divide, both are padded, the dividing one by a whole tiles_x / _y
    const bool divides = w % tiles_x == 0 && h % tiles_y == 0;
    const int64_t ew = divides ? w : (int64_t)w + (tiles_x - w % tiles_x);
    const int64_t eh = divides ? h : (int64_t)h + (tiles_y - h % tiles_y);
    if (ew * eh >= (1ll << 31))
        return MI355_ERR_BAD_ARG;
    if (ew - w > w - 1 || eh - h > h - 1)
        return MI355_ERR_UNSUPPORTED;  // one reflection cannot serve the pad
    const int tw = (int)(ew / tiles_x), th = (int)(eh / tiles_y), tot = tw * th;
    int cl = 0;
    if (clip_limit > 0.0) {
        const double c = clip_limit * (double)tot / 256.0;
        cl = c >= (double)tot ? tot : (int)c;  // capped at tot: no bin exceeds it
        cl = cl < 1 ? 1 : cl;
    }
    if (g)
        *g = {w, h, tiles_x, tiles_y, tw, th, cl, 255.0f / (float)tot, 1.0f / (float)tw, 1.0f / (float)th};
    return MI355_OK;
}

// one histogram and one table per tile of every frame
static size_t clahe_rows(const ClaheGeom& g, int nframes) { return (size_t)nframes * (size_t)(g.tiles_x * g.tiles_y); }

// the pooled scratch of a CLAHE call, device-resident or (before its timed window) host-buffer
static int clahe_scratch(mi355_ctx* ctx, const ClaheGeom& g, int nframes)
{
    return hist_scratch(ctx, clahe_rows(g, nframes));
}

// CLAHE up to the tables: the zeroed tile histograms, the histogram launch and the table launch into d_luts
static int clahe_tables(mi355_ctx* ctx, const uint8_t* in, uint8_t* d_luts, const ClaheGeom& g, int nframes)
{
    const int rc = zeroed_hists(ctx, clahe_rows(g, nframes));
    if (rc != MI355_OK)
        return rc;
    uint32_t* hist = static_cast<uint32_t*>(ctx->d_hist.p);
    HIP_TRY(ctx, launch_clahe_hist(ctx->stream, in, hist, g, nframes));
    HIP_TRY(ctx, launch_clahe_table(ctx->stream, hist, d_luts, g, nframes));
    return MI355_OK;
}

// the one argument check of the device-resident CLAHE calls; d_out takes the frames, or with `luts` the aligned tables
static int clahe_check_dev(mi355_ctx* ctx, const void* d_in, const void* d_out, bool luts, int w, int h, int nframes,
                           double clip_limit, int tiles_x, int tiles_y, ClaheGeom* g)
{
    if (!ctx || !d_in || !d_out)
        return MI355_ERR_BAD_ARG;
    const int rc = clahe_plan(w, h, nframes, clip_limit, tiles_x, tiles_y, g);
    if (rc != MI355_OK)
        return rc;
    const size_t nin = frame_bytes(w, h, nframes, 1);
    if (bad_ranges({rd(d_in, nin, 1), luts ? wr(d_out, clahe_rows(*g, nframes) * 256, 4) : wr(d_out, nin, 1)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return clahe_scratch(ctx, *g, nframes);
}

MI355_API int mi355_clahe_check(int w, int h, int nframes, double clip_limit, int tiles_x, int tiles_y)
{
    return clahe_plan(w, h, nframes, clip_limit, tiles_x, tiles_y, nullptr);
}

MI355_API int mi355_clahe_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes,
                                    double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    int rc = clahe_check_dev(ctx, d_in, d_out, false, w, h, nframes, clip_limit, tiles_x, tiles_y, &g);
    if (rc == MI355_OK)
        rc = clahe_tables(ctx, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(ctx->d_lut.p), g, nframes);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_clahe_apply(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out),
                                    static_cast<const uint8_t*>(ctx->d_lut.p), g, nframes));
    return MI355_OK;
}

MI355_API int mi355_clahe_luts_gray8_dev(mi355_ctx* ctx, const void* d_in, uint8_t* d_luts, int w, int h, int nframes,
                                         double clip_limit, int tiles_x, int tiles_y)
{
    ClaheGeom g;
    const int rc = clahe_check_dev(ctx, d_in, d_luts, true, w, h, nframes, clip_limit, tiles_x, tiles_y, &g);
    return rc == MI355_OK ? clahe_tables(ctx, static_cast<const uint8_t*>(d_in), d_luts, g, nframes) : rc;
}

MI355_API int mi355_clahe_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                                        double clip_limit, int tiles_x, int tiles_y, uint64_t prof_ns[6])
{
    ClaheGeom g;
    const int vrc = clahe_plan(w, h, nframes, clip_limit, tiles_x, tiles_y, &g);
    auto scratch = [&] { return clahe_scratch(ctx, g, nframes); };
    return frames_batched(ctx, in, out, 1, w, h, w, h, nframes, prof_ns, vrc, scratch, [&] {
        return mi355_clahe_gray8_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, clip_limit, tiles_x, tiles_y);
    });
}

// ---- the blobs of a mask ---------------------------------------------------------------------------------------------
// What a labelling call writes: byte counts of the four outputs for values that passed ccl_values
struct CclBytes {
    size_t in, labels, count, stats, sums;
};

// The value checks of every labelling call (include/mi355_imgfilter.h, "the blobs of a mask")
static int ccl_values(int w, int h, int nframes, int connectivity, int stats_rows, CclBytes* nb)
{
    static_assert(MI355_MAX_CCL_STATS_ROWS == kCclMaxStatsRows, "the header's limit is the kernels' limit");
    const int rc = check_filter(MI355_FILTER_EQUALIZE_GRAY8, w, h, nframes, 0, 0.0f, nullptr);
    if (rc != MI355_OK)
        return rc;
    if ((connectivity != 4 && connectivity != 8) || stats_rows < 0 || stats_rows > MI355_MAX_CCL_STATS_ROWS)
        return MI355_ERR_BAD_ARG;
    if (nb) {
        const size_t px = (size_t)w * h * nframes, rows = (size_t)nframes * (size_t)stats_rows;
        *nb = {px, px * sizeof(int32_t), (size_t)nframes * sizeof(int32_t), rows * 5 * sizeof(int32_t),
               rows * 2 * sizeof(uint64_t)};
    }
    return MI355_OK;
}

MI355_API int mi355_ccl_check(int w, int h, int nframes, int connectivity, int stats_rows)
{
    return ccl_values(w, h, nframes, connectivity, stats_rows, nullptr);
}

// the pooled scratch of a labelling call, device-resident or (before its timed window) host-buffer
static int ccl_scratch(mi355_ctx* ctx, int w, int h, int nframes)
{
    return ensure(ctx, ctx->d_ccl, ccl_scratch_bytes(w, h, nframes));
}

MI355_API int mi355_ccl_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_labels, int32_t* d_count,
                                  int32_t* d_stats, uint64_t* d_sums, int w, int h, int nframes, int connectivity,
                                  int stats_rows)
{
    if (!ctx || !d_in || !d_labels || !d_count)
        return MI355_ERR_BAD_ARG;
    CclBytes nb;
    const int rc = ccl_values(w, h, nframes, connectivity, stats_rows, &nb);
    if (rc != MI355_OK)
        return rc;
    if (stats_rows > 0 && (!d_stats || !d_sums))
        return MI355_ERR_BAD_ARG;
    // the ranges in play: the input and the outputs this call writes (without statistics, whatever stands in their place
    // is not looked at)
    const bool with_stats = stats_rows > 0;
    if (bad_ranges({rd(d_in, nb.in, 1), wr(d_labels, nb.labels, 4), wr(d_count, nb.count, 4),
                    wr(with_stats ? d_stats : nullptr, nb.stats, 4), wr(with_stats ? d_sums : nullptr, nb.sums, 8)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int erc = ccl_scratch(ctx, w, h, nframes);
    if (erc != MI355_OK)
        return erc;
    HIP_TRY(ctx, launch_ccl(ctx->stream, static_cast<const uint8_t*>(d_in), d_labels, d_count, d_stats, d_sums,
                            static_cast<uint32_t*>(ctx->d_ccl.p), w, h, nframes, connectivity == 8, stats_rows));
    return MI355_OK;
}

MI355_API int mi355_ccl_gray8_batched(mi355_ctx* ctx, const uint8_t* in, int32_t* labels, int32_t* count,
                                      int32_t* stats, uint64_t* sums, int w, int h, int nframes, int connectivity,
                                      int stats_rows, uint64_t prof_ns[6])
{
    if (!ctx || !in || !labels || !count)
        return MI355_ERR_BAD_ARG;
    CclBytes nb;
    int rc = ccl_values(w, h, nframes, connectivity, stats_rows, &nb);
    if (rc != MI355_OK)
        return rc;
    if (stats_rows > 0 && (!stats || !sums))
        return MI355_ERR_BAD_ARG;
    // the labels, then the few rows that leave the device beside them; the sums on an 8-byte boundary
    HostOut o[4] = {{labels, nb.labels, 4}, {count, nb.count, 4}, {stats_rows ? stats : nullptr, nb.stats, 4},
                    {stats_rows ? sums : nullptr, nb.sums, 8}};
    return outputs_batched(ctx, in, nb.in, o, prof_ns, [&] { return ccl_scratch(ctx, w, h, nframes); }, [&] {
        return mi355_ccl_gray8_dev(ctx, ctx->d_in.p, out_dev<int32_t>(ctx, o[0]), out_dev<int32_t>(ctx, o[1]),
                                   out_dev<int32_t>(ctx, o[2]), out_dev<uint64_t>(ctx, o[3]), w, h, nframes, connectivity,
                                   stats_rows);
    });
}

// ---- how far from the background -------------------------------------------------------------------------------------
// The value checks of every distance call (include/mi355_imgfilter.h, "how far from the background")
static int dist_values(int w, int h, int nframes)
{
    static_assert(MI355_MAX_DIST_DIM == kDistMaxDim, "the header's limit is the kernels' limit");
    const int rc = check_filter(MI355_FILTER_EQUALIZE_GRAY8, w, h, nframes, 0, 0.0f, nullptr);
    if (rc != MI355_OK)
        return rc;
    return w > MI355_MAX_DIST_DIM || h > MI355_MAX_DIST_DIM ? MI355_ERR_BAD_ARG : MI355_OK;
}

MI355_API int mi355_dist_check(int w, int h, int nframes)
{
    return dist_values(w, h, nframes);
}

// the pooled scratch of a distance call, device-resident or (before its timed window) host-buffer
static int dist_scratch(mi355_ctx* ctx, int w, int h, int nframes)
{
    return ensure(ctx, ctx->d_dist, dist_scratch_bytes(w, h, nframes));
}

MI355_API int mi355_dist_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_sq, float* d_dist, int32_t* d_nearest,
                                   int w, int h, int nframes)
{
    if (!ctx || !d_in || (!d_sq && !d_dist && !d_nearest))
        return MI355_ERR_BAD_ARG;
    const int rc = dist_values(w, h, nframes);
    if (rc != MI355_OK)
        return rc;
    // the ranges in play: the input and the outputs this call writes
    const size_t plane = frame_bytes(w, h, nframes, 4);
    if (bad_ranges({rd(d_in, frame_bytes(w, h, nframes, 1), 1), wr(d_sq, plane, 4), wr(d_dist, plane, 4),
                    wr(d_nearest, plane, 4)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int erc = dist_scratch(ctx, w, h, nframes);
    if (erc != MI355_OK)
        return erc;
    HIP_TRY(ctx, launch_dist(ctx->stream, static_cast<const uint8_t*>(d_in), d_sq, d_dist, d_nearest,
                             static_cast<int16_t*>(ctx->d_dist.p), w, h, nframes));
    return MI355_OK;
}

MI355_API int mi355_dist_gray8_batched(mi355_ctx* ctx, const uint8_t* in, int32_t* sq, float* dist, int32_t* nearest,
                                       int w, int h, int nframes, uint64_t prof_ns[6])
{
    if (!ctx || !in || (!sq && !dist && !nearest))
        return MI355_ERR_BAD_ARG;
    int rc = dist_values(w, h, nframes);
    if (rc != MI355_OK)
        return rc;
    // the planes the caller takes, 4 bytes per pixel each
    const size_t plane = frame_bytes(w, h, nframes, 4);
    HostOut o[3] = {{sq, plane, 4}, {dist, plane, 4}, {nearest, plane, 4}};
    auto scratch = [&] { return dist_scratch(ctx, w, h, nframes); };
    return outputs_batched(ctx, in, frame_bytes(w, h, nframes, 1), o, prof_ns, scratch, [&] {
        return mi355_dist_gray8_dev(ctx, ctx->d_in.p, out_dev<int32_t>(ctx, o[0]), out_dev<float>(ctx, o[1]),
                                    out_dev<int32_t>(ctx, o[2]), w, h, nframes);
    });
}

// ---- from gradients to edges -----------------------------------------------------------------------------------------
// The value checks of every hysteresis call (include/mi355_imgfilter.h, "from gradients to edges")
static int hysteresis_values(int w, int h, int nframes, int low, int high, int connectivity)
{
    const int rc = ccl_values(w, h, nframes, connectivity, 0, nullptr);
    if (rc != MI355_OK)
        return rc;
    return low < 0 || high > 255 || low > high ? MI355_ERR_BAD_ARG : MI355_OK;
}

// The value checks of every Canny call and, when they pass, the two integer thresholds on the magnitude
static int canny_values(int w, int h, int nframes, double threshold1, double threshold2, int flags, int* low, int* high)
{
    const int rc = ccl_values(w, h, nframes, 8, 0, nullptr);
    if (rc != MI355_OK)
        return rc;
    if (!std::isfinite(threshold1) || !std::isfinite(threshold2) || threshold1 < 0.0 || threshold2 < 0.0 ||
        threshold1 > 1.0e9 || threshold2 > 1.0e9 || (flags & ~MI355_CANNY_L2GRADIENT))
        return MI355_ERR_BAD_ARG;
    double lo = threshold1 < threshold2 ? threshold1 : threshold2, hi = threshold1 < threshold2 ? threshold2 : threshold1;
    if (flags & MI355_CANNY_L2GRADIENT) {
        lo = lo < 32767.0 ? lo : 32767.0;
        hi = hi < 32767.0 ? hi : 32767.0;
        if (lo > 0.0)
            lo *= lo;
        if (hi > 0.0)
            hi *= hi;
    }
    if (low)
        *low = (int)std::floor(lo);  // at most 32767^2 or 10^9: an int
    if (high)
        *high = (int)std::floor(hi);
    return MI355_OK;
}

// the pooled parent array of a hysteresis or Canny call, device-resident or (before its timed window) host-buffer
static int edges_scratch(mi355_ctx* ctx, int w, int h, int nframes)
{
    return ensure(ctx, ctx->d_parent, frame_bytes(w, h, nframes, sizeof(int32_t)));
}

MI355_API int mi355_hysteresis_check(int w, int h, int nframes, int low, int high, int connectivity)
{
    return hysteresis_values(w, h, nframes, low, high, connectivity);
}

MI355_API int mi355_hysteresis_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes, int low,
                                         int high, int connectivity)
{
    int rc = frames_dev(ctx, d_in, d_out, 1, w, h, w, h, nframes,
                        hysteresis_values(w, h, nframes, low, high, connectivity));
    if (rc == MI355_OK)
        rc = edges_scratch(ctx, w, h, nframes);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_hysteresis(ctx->stream, static_cast<const uint8_t*>(d_in), static_cast<uint8_t*>(d_out),
                                   static_cast<int32_t*>(ctx->d_parent.p), w, h, nframes, low, high, connectivity == 8));
    return MI355_OK;
}

MI355_API int mi355_hysteresis_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                                             int low, int high, int connectivity, uint64_t prof_ns[6])
{
    const int vrc = hysteresis_values(w, h, nframes, low, high, connectivity);
    auto scratch = [&] { return edges_scratch(ctx, w, h, nframes); };
    return frames_batched(ctx, in, out, 1, w, h, w, h, nframes, prof_ns, vrc, scratch, [&] {
        return mi355_hysteresis_gray8_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, low, high, connectivity);
    });
}

MI355_API int mi355_canny_check(int w, int h, int nframes, double threshold1, double threshold2, int flags)
{
    return canny_values(w, h, nframes, threshold1, threshold2, flags, nullptr, nullptr);
}

MI355_API int mi355_canny_gray8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h, int nframes,
                                    double threshold1, double threshold2, int flags)
{
    int low = 0, high = 0;
    int rc = frames_dev(ctx, d_in, d_out, 1, w, h, w, h, nframes,
                        canny_values(w, h, nframes, threshold1, threshold2, flags, &low, &high));
    if (rc == MI355_OK)
        rc = edges_scratch(ctx, w, h, nframes);
    if (rc != MI355_OK)
        return rc;
    uint8_t* out = static_cast<uint8_t*>(d_out);
    HIP_TRY(ctx, launch_canny_nms(ctx->stream, static_cast<const uint8_t*>(d_in), out, w, h, nframes, low, high,
                                  (flags & MI355_CANNY_L2GRADIENT) != 0));
    // the class bytes (0 none, 1 candidate, 2 strong) become the edge map in place: candidate = class > 0, strong = class > 1
    HIP_TRY(ctx, launch_hysteresis(ctx->stream, out, out, static_cast<int32_t*>(ctx->d_parent.p), w, h, nframes, 0, 1,
                                   true));
    return MI355_OK;
}

MI355_API int mi355_canny_gray8_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes,
                                        double threshold1, double threshold2, int flags, uint64_t prof_ns[6])
{
    const int vrc = canny_values(w, h, nframes, threshold1, threshold2, flags, nullptr, nullptr);
    auto scratch = [&] { return edges_scratch(ctx, w, h, nframes); };
    return frames_batched(ctx, in, out, 1, w, h, w, h, nframes, prof_ns, vrc, scratch, [&] {
        return mi355_canny_gray8_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, threshold1, threshold2, flags);
    });
}

// ---- from edges to lines ---------------------------------------------------------------------------------------------
// What the value checks of a Hough call leave behind: the kernels' geometry and the byte counts of a call
struct HoughCall {
    HoughGeom g;
    float irho;
    size_t in, accum_frame, accum, lines, votes, count;
};

// The value checks of every Hough call (include/mi355_imgfilter.h, "from edges to lines"), numangle and numrho as the
// header derives them.  threshold and max_lines are checked only when lines is set (the accumulator calls have neither).
static int hough_values(int w, int h, int nframes, double rho, double theta, double min_theta, double max_theta, bool lines,
                        int threshold, int max_lines, HoughCall* out)
{
    static_assert(MI355_MAX_HOUGH_ANGLES == kHoughMaxAngles && MI355_MAX_HOUGH_LINES == kHoughMaxLines,
                  "the header's limits are the kernels' limits");
    if (!valid_sizes(w, h, nframes) || w > MI355_MAX_WARP_SIZE || h > MI355_MAX_WARP_SIZE)
        return MI355_ERR_BAD_ARG;
    if (!std::isfinite(rho) || !std::isfinite(theta) || rho <= 0.0 || theta <= 0.0 || !std::isfinite(min_theta) ||
        !std::isfinite(max_theta) || min_theta < 0.0 || max_theta > M_PI || max_theta < min_theta)
        return MI355_ERR_BAD_ARG;
    const float rho_f = (float)rho, theta_f = (float)theta;
    if (!(rho_f > 0.0f) || !(theta_f > 0.0f) || !std::isfinite(rho_f))  // a double below the smallest float, or above the largest
        return MI355_ERR_BAD_ARG;
    const double steps = std::floor((max_theta - min_theta) / theta);
    if (!(steps <= (double)MI355_MAX_HOUGH_ANGLES))  // numangle - 1 may pass the limit by one only through the correction below
        return MI355_ERR_BAD_ARG;
    int numangle = (int)steps + 1;
    if (numangle > 1 && std::fabs(M_PI - (numangle - 1) * theta) < theta / 2)
        numangle--;
    const float cells = (float)(2 * (w + h) + 1) / rho_f;  // fp32 division; at most 131 065 / rho_f
    if (!(cells < 1.0e9f))
        return MI355_ERR_BAD_ARG;
    const int numrho = (int)std::nearbyintf(cells);  // cvRound: half to even under the default rounding mode
    if (numangle > MI355_MAX_HOUGH_ANGLES || numrho < 1)
        return MI355_ERR_BAD_ARG;
    const uint64_t accum_frame = (uint64_t)(numangle + 2) * (uint64_t)(numrho + 2) * sizeof(int32_t);
    if (accum_frame >= (1ull << 31) || (double)accum_frame * (double)nframes > 2.4e11)
        return MI355_ERR_BAD_ARG;
    if (lines && (threshold < 0 || max_lines < 1 || max_lines > MI355_MAX_HOUGH_LINES))
        return MI355_ERR_BAD_ARG;
    if (out) {
        out->g = {w, h, nframes, numangle, numrho, rho_f, theta_f, (float)min_theta};
        out->irho = 1.0f / rho_f;
        out->in = frame_bytes(w, h, nframes, 1);
        out->accum_frame = (size_t)accum_frame;
        out->accum = (size_t)accum_frame * (size_t)nframes;
        out->lines = (size_t)nframes * (size_t)(lines ? max_lines : 0) * 2 * sizeof(float);
        out->votes = (size_t)nframes * (size_t)(lines ? max_lines : 0) * sizeof(int32_t);
        out->count = (size_t)nframes * sizeof(int32_t);
    }
    return MI355_OK;
}

// The header's trig table: ang is an fp32 variable that grows by theta_f; the products are taken in double
static void hough_table(const HoughCall& c, float* tab_cos, float* tab_sin)
{
    float ang = c.g.min_theta_f;
    for (int n = 0; n < c.g.numangle; ang += c.g.theta_f, n++) {
        tab_cos[n] = (float)(std::cos((double)ang) * (double)c.irho);
        tab_sin[n] = (float)(std::sin((double)ang) * (double)c.irho);
    }
}

// The table on the device.  It is uploaded only when (rho, theta, min_theta, numangle) differ from the last call's: that
// call waits for the stream (the kernels of the call before may still read the old table) and copies synchronously, like
// the first call with a new Gaussian (k, sigma); every other call touches nothing.
static int hough_table_dev(mi355_ctx* ctx, const HoughCall& c)
{
    const double key[4] = {(double)c.g.rho_f, (double)c.g.theta_f, (double)c.g.min_theta_f, (double)c.g.numangle};
    if (ctx->d_hough_tab && std::memcmp(key, ctx->hough_key, sizeof(key)) == 0)
        return MI355_OK;
    if (!ctx->d_hough_tab)
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_hough_tab), 2 * MI355_MAX_HOUGH_ANGLES * sizeof(float)));
    std::vector<float> tab(2 * (size_t)c.g.numangle);
    hough_table(c, tab.data(), tab.data() + c.g.numangle);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->hough_key[3] = 0.0;
    HIP_TRY(ctx, hipMemcpy(ctx->d_hough_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    std::memcpy(ctx->hough_key, key, sizeof(key));
    return MI355_OK;
}

MI355_API int mi355_hough_check(int w, int h, int nframes, double rho, double theta, int threshold, int max_lines,
                                double min_theta, double max_theta)
{
    return hough_values(w, h, nframes, rho, theta, min_theta, max_theta, true, threshold, max_lines, nullptr);
}

MI355_API int mi355_hough_shape(int w, int h, double rho, double theta, double min_theta, double max_theta, int* numangle,
                                int* numrho)
{
    HoughCall c;
    const int rc = hough_values(w, h, 1, rho, theta, min_theta, max_theta, false, 0, 0, &c);
    if (rc != MI355_OK)
        return rc;
    if (numangle)
        *numangle = c.g.numangle;
    if (numrho)
        *numrho = c.g.numrho;
    return MI355_OK;
}

MI355_API int mi355_hough_plan(int w, int h, double rho, double theta, double min_theta, double max_theta,
                               int* angles_per_block, int* rho_splits, int* lds_cells)
{
    HoughCall c;
    const int rc = hough_values(w, h, 1, rho, theta, min_theta, max_theta, false, 0, 0, &c);
    if (rc != MI355_OK)
        return rc;
    const HoughPlan p = hough_plan(c.g.numangle, c.g.numrho);
    if (angles_per_block)
        *angles_per_block = p.angles_per_block;
    if (rho_splits)
        *rho_splits = p.rho_splits;
    if (lds_cells)
        *lds_cells = p.lds_cells;
    return MI355_OK;
}

MI355_API int mi355_hough_trig_table(int w, int h, double rho, double theta, double min_theta, double max_theta,
                                     float* tab_cos, float* tab_sin)
{
    if (!tab_cos || !tab_sin)
        return MI355_ERR_BAD_ARG;
    HoughCall c;
    const int rc = hough_values(w, h, 1, rho, theta, min_theta, max_theta, false, 0, 0, &c);
    if (rc != MI355_OK)
        return rc;
    hough_table(c, tab_cos, tab_sin);
    return MI355_OK;
}

MI355_API size_t mi355_hough_accum_bytes(int w, int h, int nframes, double rho, double theta, double min_theta,
                                         double max_theta)
{
    HoughCall c;
    return hough_values(w, h, nframes, rho, theta, min_theta, max_theta, false, 0, 0, &c) == MI355_OK ? c.accum : 0;
}

// What a Hough call pools, device-resident or (before its timed window) host-buffer: the scratch, the table and, for a
// caller that brings no accumulator, the pooled one
static int hough_scratch(mi355_ctx* ctx, const HoughCall& c, bool pooled_accum)
{
    int rc = ensure(ctx, ctx->d_hough, hough_scratch_bytes(c.g));
    if (rc == MI355_OK)
        rc = hough_table_dev(ctx, c);
    if (rc == MI355_OK && pooled_accum)
        rc = ensure(ctx, ctx->d_hough_acc, c.accum);
    return rc;
}

MI355_API int mi355_hough_accum_gray8_dev(mi355_ctx* ctx, const void* d_in, int32_t* d_accum, int w, int h, int nframes,
                                          double rho, double theta, double min_theta, double max_theta)
{
    if (!ctx || !d_in || !d_accum)
        return MI355_ERR_BAD_ARG;
    HoughCall c;
    int rc = hough_values(w, h, nframes, rho, theta, min_theta, max_theta, false, 0, 0, &c);
    if (rc != MI355_OK)
        return rc;
    if (bad_ranges({rd(d_in, c.in, 1), wr(d_accum, c.accum, 4)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = hough_scratch(ctx, c, false);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_hough_accum(ctx->stream, static_cast<const uint8_t*>(d_in), d_accum, ctx->d_hough_tab,
                                    ctx->d_hough.p, c.g));
    return MI355_OK;
}

MI355_API int mi355_hough_lines_gray8_dev(mi355_ctx* ctx, const void* d_in, float* d_lines, int32_t* d_votes,
                                          int32_t* d_count, int32_t* d_accum, int w, int h, int nframes, double rho,
                                          double theta, int threshold, int max_lines, double min_theta, double max_theta)
{
    if (!ctx || !d_in || !d_lines || !d_count)
        return MI355_ERR_BAD_ARG;
    HoughCall c;
    int rc = hough_values(w, h, nframes, rho, theta, min_theta, max_theta, true, threshold, max_lines, &c);
    if (rc != MI355_OK)
        return rc;
    if (bad_ranges({rd(d_in, c.in, 1), wr(d_lines, c.lines, 4), wr(d_votes, c.votes, 4), wr(d_count, c.count, 4),
                    wr(d_accum, c.accum, 4)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = hough_scratch(ctx, c, !d_accum);
    if (rc != MI355_OK)
        return rc;
    if (!d_accum)
        d_accum = static_cast<int32_t*>(ctx->d_hough_acc.p);
    HIP_TRY(ctx, launch_hough_accum(ctx->stream, static_cast<const uint8_t*>(d_in), d_accum, ctx->d_hough_tab,
                                    ctx->d_hough.p, c.g));
    HIP_TRY(ctx, launch_hough_lines(ctx->stream, d_accum, d_lines, d_votes, d_count, ctx->d_hough.p, c.g, threshold,
                                    max_lines));
    return MI355_OK;
}

MI355_API int mi355_hough_lines_gray8_batched(mi355_ctx* ctx, const uint8_t* in, float* lines, int32_t* votes,
                                              int32_t* count, int w, int h, int nframes, double rho, double theta,
                                              int threshold, int max_lines, double min_theta, double max_theta,
                                              uint64_t prof_ns[6])
{
    if (!ctx || !in || !lines || !count)
        return MI355_ERR_BAD_ARG;
    HoughCall c;
    int rc = hough_values(w, h, nframes, rho, theta, min_theta, max_theta, true, threshold, max_lines, &c);
    if (rc != MI355_OK)
        return rc;
    // the lines, then their votes (written on the device whether or not the caller takes them) and the counts; the
    // accumulator is the pooled one
    HostOut o[3] = {{lines, c.lines, 4}, {votes, c.votes, 4, true}, {count, c.count, 4}};
    return outputs_batched(ctx, in, c.in, o, prof_ns, [&] { return hough_scratch(ctx, c, true); }, [&] {
        return mi355_hough_lines_gray8_dev(ctx, ctx->d_in.p, out_dev<float>(ctx, o[0]), out_dev<int32_t>(ctx, o[1]),
                                           out_dev<int32_t>(ctx, o[2]), nullptr, w, h, nframes, rho, theta, threshold,
                                           max_lines, min_theta, max_theta);
    });
}

// ---- YUV frames ------------------------------------------------------------------------------------------------------
// The integers of the header's table, one row per MI355_YUV_BT* standard.
static const YuvDecodeCoef kYuvDecode[3] = {
    {16, 1220542, 1673527, -852492, -409993, 2116026},  // BT601: OpenCV's three-decimal constants
    {16, 1220945, 1879825, -558796, -223607, 2215014},  // BT709
    {0, 1048576, 1470104, -748826, -360853, 1858077},   // BT601_FULL
};
static const YuvEncodeCoef kYuvEncode[3] = {
    {269484, 528482, 102760, -155188, -305135, 460324, -385875, -74448, (1 << 19) + (16 << 20)},
    {191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230, (1 << 19) + (16 << 20)},
    {313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262, 1 << 19},
};

// The value checks of every YUV call and, when they pass, the surface with pitch and rows resolved.
static int yuv_plan(int layout, int standard, int w, int h, int nframes, int pitch, int rows, int encode, YuvFrames* out)
{
    if (layout < MI355_YUV_NV12 || layout > MI355_YUV_UYVY || standard < MI355_YUV_BT601 ||
        standard > MI355_YUV_BT601_FULL || !valid_sizes(w, h, nframes) || (w & 1) || pitch < 0 || rows < 0)
        return MI355_ERR_BAD_ARG;
    const bool packed = yuv_layout_packed(layout);
    const bool planar = layout == MI355_YUV_I420 || layout == MI355_YUV_YV12;
    const int64_t tight = packed ? 2 * (int64_t)w : (int64_t)w;
    if (tight > 0x7FFFFFFF)
        return MI355_ERR_BAD_ARG;
    const YuvFrames s = {layout, w, h, nframes, pitch ? pitch : (int)tight, rows ? rows : h};
    if (s.pitch < tight || s.rows < h || (!packed && ((h & 1) || (s.rows & 1))) || (planar && (s.pitch & 1)))
        return MI355_ERR_BAD_ARG;
    // the surfaces of a call, padding included, stay below 2^37 bytes: far beyond the HBM, and no size_t sum wraps
    if ((double)s.pitch * (double)s.rows * (double)nframes > 1.2e11)
        return MI355_ERR_BAD_ARG;
    if (encode && packed)
        return MI355_ERR_UNSUPPORTED;
    if (out)
        *out = s;
    return MI355_OK;
}

// the one argument check of the three device-resident YUV calls; `other_bpp` is 4 (RGBA) or 1 (gray8)
static int yuv_check_dev(mi355_ctx* ctx, const void* d_yuv, const void* d_other, int other_bpp, bool yuv_is_input,
                         int layout, int standard, int w, int h, int nframes, int pitch, int rows, YuvFrames* s)
{
    if (!ctx || !d_yuv || !d_other)
        return MI355_ERR_BAD_ARG;
    const int rc = yuv_plan(layout, standard, w, h, nframes, pitch, rows, yuv_is_input ? 0 : 1, s);
    if (rc != MI355_OK)
        return rc;
    const size_t nyuv = yuv_frame_size(*s) * (size_t)nframes, nother = frame_bytes(w, h, nframes, other_bpp);
    if (bad_ranges({yuv_is_input ? rd(d_yuv, nyuv, 1) : wr(d_yuv, nyuv, 1),
                    yuv_is_input ? wr(d_other, nother, other_bpp) : rd(d_other, nother, other_bpp)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return MI355_OK;
}

MI355_API size_t mi355_yuv_frame_bytes(int layout, int w, int h, int pitch, int rows)
{
    YuvFrames s;
    return yuv_plan(layout, MI355_YUV_BT601, w, h, 1, pitch, rows, 0, &s) == MI355_OK ? yuv_frame_size(s) : 0;
}

MI355_API int mi355_yuv_check(int layout, int standard, int w, int h, int nframes, int pitch, int rows, int encode)
{
    return yuv_plan(layout, standard, w, h, nframes, pitch, rows, encode, nullptr);
}

MI355_API int mi355_yuv_to_rgba8_dev(mi355_ctx* ctx, const void* d_yuv, void* d_rgba, int w, int h, int nframes,
                                     int layout, int standard, int pitch, int rows)
{
    YuvFrames s;
    const int rc = yuv_check_dev(ctx, d_yuv, d_rgba, 4, true, layout, standard, w, h, nframes, pitch, rows, &s);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_yuv_to_rgba(ctx->stream, static_cast<const uint8_t*>(d_yuv), static_cast<uint8_t*>(d_rgba), s,
                                    kYuvDecode[standard]));
    return MI355_OK;
}

MI355_API int mi355_rgba8_to_yuv_dev(mi355_ctx* ctx, const void* d_rgba, void* d_yuv, int w, int h, int nframes,
                                     int layout, int standard, int pitch, int rows)
{
    YuvFrames s;
    const int rc = yuv_check_dev(ctx, d_yuv, d_rgba, 4, false, layout, standard, w, h, nframes, pitch, rows, &s);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_rgba_to_yuv(ctx->stream, static_cast<const uint8_t*>(d_rgba), static_cast<uint8_t*>(d_yuv), s,
                                    kYuvEncode[standard]));
    return MI355_OK;
}

MI355_API int mi355_yuv_to_gray8_dev(mi355_ctx* ctx, const void* d_yuv, void* d_gray, int w, int h, int nframes,
                                     int layout, int pitch, int rows)
{
    YuvFrames s;
    const int rc = yuv_check_dev(ctx, d_yuv, d_gray, 1, true, layout, MI355_YUV_BT601, w, h, nframes, pitch, rows, &s);
    if (rc != MI355_OK)
        return rc;
    HIP_TRY(ctx, launch_yuv_to_gray(ctx->stream, static_cast<const uint8_t*>(d_yuv), static_cast<uint8_t*>(d_gray), s));
    return MI355_OK;
}

// The host-buffer form of both directions: the pooled buffers sized by each side's own bytes, then the round trip.  The
// context's input format describes the frames of the filter calls, not these: under MI355_INPUT_BGR nothing is guessed.
static int yuv_batched(mi355_ctx* ctx, const uint8_t* in, uint8_t* out, int w, int h, int nframes, int layout,
                       int standard, int pitch, int rows, bool encode, uint64_t prof_ns[6])
{
    if (!ctx || !in || !out)
        return MI355_ERR_BAD_ARG;
    YuvFrames s;
    int rc = yuv_plan(layout, standard, w, h, nframes, pitch, rows, encode ? 1 : 0, &s);
    if (rc != MI355_OK)
        return rc;
    const size_t nyuv = yuv_frame_size(s) * (size_t)nframes, nrgba = frame_bytes(w, h, nframes, 4);
    const size_t out_bytes = encode ? nyuv : nrgba;
    HostIO io;
    rc = stage_host(ctx, encode ? nrgba : nyuv, 1, out_bytes, &io);  // either input counted in bytes: BGR is unsupported
    if (rc != MI355_OK)
        return rc;
    const bool padded = encode && (s.pitch != w || s.rows != h);
    return timed_roundtrip(ctx, io, in, out, prof_ns, [&] {
        if (!encode)
            return mi355_yuv_to_rgba8_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, layout, standard, pitch, rows);
        if (padded)  // the kernel never writes padding; the host gets zeros there, not the pool's previous content
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_out.p, 0, out_bytes, ctx->stream));
        return mi355_rgba8_to_yuv_dev(ctx, ctx->d_in.p, ctx->d_out.p, w, h, nframes, layout, standard, pitch, rows);
    });
}

MI355_API int mi355_yuv_to_rgba8_batched(mi355_ctx* ctx, const uint8_t* yuv, uint8_t* rgba, int w, int h, int nframes,
                                         int layout, int standard, int pitch, int rows, uint64_t prof_ns[6])
{
    return yuv_batched(ctx, yuv, rgba, w, h, nframes, layout, standard, pitch, rows, false, prof_ns);
}

MI355_API int mi355_rgba8_to_yuv_batched(mi355_ctx* ctx, const uint8_t* rgba, uint8_t* yuv, int w, int h, int nframes,
                                         int layout, int standard, int pitch, int rows, uint64_t prof_ns[6])
{
    return yuv_batched(ctx, rgba, yuv, w, h, nframes, layout, standard, pitch, rows, true, prof_ns);
}

MI355_API int mi355_gray_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                   int nframes)
{
    return dispatch_dev(ctx, MI355_FILTER_GRAY, d_in, d_out, w, h, nframes, 0, 0.0f);
}

MI355_API int mi355_gray1_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                    int nframes)
{
    return dispatch_dev(ctx, MI355_FILTER_GRAY1, d_in, d_out, w, h, nframes, 0, 0.0f);
}

MI355_API int mi355_gauss_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                    int nframes, int k, float sigma)
{
    return dispatch_dev(ctx, MI355_FILTER_GAUSS, d_in, d_out, w, h, nframes, k, sigma);
}

MI355_API int mi355_sobel_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                    int nframes)
{
    return dispatch_dev(ctx, MI355_FILTER_SOBEL, d_in, d_out, w, h, nframes, 0, 0.0f);
}

MI355_API int mi355_pipeline_rgba8_dev(mi355_ctx* ctx, const void* d_in, void* d_out, int w, int h,
                                       int nframes, int k, float sigma)
{
    return dispatch_dev(ctx, MI355_FILTER_PIPELINE, d_in, d_out, w, h, nframes, k, sigma);
}

MI355_API int mi355_synth_rgba8_dev(mi355_ctx* ctx, void* d_out, int w, int h, int nframes,
                                    int first_frame, uint32_t seed, int mode)
{
    if (!ctx || !d_out || mode < 0 || mode > 3 || !valid_sizes(w, h, nframes) ||
        (reinterpret_cast<uintptr_t>(d_out) & 3u))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_synth(ctx->stream, static_cast<uint8_t*>(d_out), w, h, nframes, first_frame, seed,
                              mode));
    return MI355_OK;
}

MI355_API int mi355_checksum_dev(mi355_ctx* ctx, const void* d_buf, size_t nbytes, uint64_t index_base,
                                 uint64_t* out)
{
    if (!ctx || !d_buf || !out)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_acc, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_checksum(ctx->stream, static_cast<const uint8_t*>(d_buf), nbytes, index_base,
                                 ctx->d_acc));
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&v, ctx->d_acc, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = (uint64_t)v;
    return MI355_OK;
}

MI355_API int mi355_stream_copy_dev(mi355_ctx* ctx, void* d_dst, const void* d_src, size_t nbytes)
{
    if (!ctx || !d_dst || !d_src || bad_ranges({rd(d_src, nbytes, 1), wr(d_dst, nbytes, 1)}))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_stream_copy(ctx->stream, static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst),
                                    nbytes));
    return MI355_OK;
}

MI355_API int mi355_selftest(mi355_ctx* ctx, uint32_t* bad_luma, uint32_t* bad_mag)
{
    if (!ctx || !bad_luma || !bad_mag)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_acc, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_selftest(ctx->stream, ctx->d_acc));
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&v, ctx->d_acc, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *bad_luma = (uint32_t)v;
    *bad_mag = (uint32_t)(v >> 32);
    return MI355_OK;
}

MI355_API int mi355_dev_alloc(mi355_ctx* ctx, size_t nbytes, void** d_ptr)
{
    if (!ctx || !d_ptr || nbytes == 0)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(d_ptr, nbytes);
    if (e != hipSuccess) {
        ctx->last_hip = (int)e;
        *d_ptr = nullptr;
        return MI355_ERR_NOMEM;
    }
    return MI355_OK;
}

MI355_API int mi355_pool_alloc(mi355_ctx* ctx, int filter, int w, int h, int nframes, int k, float sigma, int tries,
                               void** d_in, void** d_out, float* probe_ms)
{
    if (!ctx || !d_in || !d_out)
        return MI355_ERR_BAD_ARG;
    *d_in = *d_out = nullptr;
    const FilterInfo* f = nullptr;
    int rc = check_filter(filter, w, h, nframes, k, sigma, &f);
    if (rc != MI355_OK)
        return rc;
    constexpr int kMaxCand = 16;
    for (int i = 0; probe_ms && i < tries; i++)
        probe_ms[i] = -1.0f;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)w * h * nframes;
    const size_t in_bytes = npx * (size_t)f->in_bpp, out_bytes = npx * (size_t)f->out_bpp;
    void* in = nullptr;
    if (hipMalloc(&in, in_bytes) != hipSuccess)
        return MI355_ERR_NOMEM;
    // defined, opaque input (A = 255): the placement probe then times the path real frames take
    hipError_t e = hipMemsetAsync(in, 0xFF, in_bytes, ctx->stream);
    rc = (e == hipSuccess) ? MI355_OK : MI355_ERR_HIP;
    if (e != hipSuccess)
        ctx->last_hip = (int)e;

    // all candidates alive at once, hence all in different places; stop early when memory runs short
    void* cand[kMaxCand] = {};
    int ncand = 0;
    const int want = tries < 1 ? 1 : (tries > kMaxCand ? kMaxCand : tries);
    while (rc == MI355_OK && ncand < want) {
        size_t free_b = 0, total_b = 0;
        if (ncand > 0 && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < out_bytes + ((size_t)8 << 30)))
            break;
        if (hipMalloc(&cand[ncand], out_bytes) != hipSuccess) {
            cand[ncand] = nullptr;
            break;
        }
        ncand++;
    }
    if (rc == MI355_OK && ncand == 0)
        rc = MI355_ERR_NOMEM;
    int keep = 0;
    float best_ms = 0.0f;
    for (int i = 0; rc == MI355_OK && ncand > 1 && i < ncand; i++) {
        float ms = 0.0f;
        for (int l = 0; rc == MI355_OK && l < 4 + 8; l++) {
            if (l == 4 && (e = hipEventRecord(ctx->t0, ctx->stream)) != hipSuccess) {
                ctx->last_hip = (int)e;
                rc = MI355_ERR_HIP;
                break;
            }
            rc = dispatch_dev(ctx, filter, in, cand[i], w, h, nframes, k, sigma);
        }
        if (rc != MI355_OK)
            break;
        e = hipEventRecord(ctx->t1, ctx->stream);
        if (e == hipSuccess)
            e = hipEventSynchronize(ctx->t1);
        if (e == hipSuccess)
            e = hipEventElapsedTime(&ms, ctx->t0, ctx->t1);
        if (e != hipSuccess) {
            ctx->last_hip = (int)e;
            rc = MI355_ERR_HIP;
            break;
        }
        ms /= 8.0f;
        if (probe_ms)
            probe_ms[i] = ms;
        if (i == 0 || ms < best_ms) {
            best_ms = ms;
            keep = i;
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < ncand; i++)
        if (rc != MI355_OK || i != keep)
            (void)hipFree(cand[i]);
    if (rc != MI355_OK) {
        (void)hipFree(in);
        return rc;
    }
    *d_in = in;
    *d_out = cand[keep];
    return MI355_OK;
}

MI355_API int mi355_pool_free(mi355_ctx* ctx, void* d_in, void* d_out)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (d_in)
        HIP_TRY(ctx, hipFree(d_in));
    if (d_out)
        HIP_TRY(ctx, hipFree(d_out));
    return MI355_OK;
}

MI355_API int mi355_dev_free(mi355_ctx* ctx, void* d_ptr)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    if (!d_ptr)
        return MI355_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(d_ptr));
    return MI355_OK;
}

MI355_API int mi355_copy_h2d(mi355_ctx* ctx, void* d_dst, const void* h_src, size_t nbytes)
{
    if (!ctx || !d_dst || !h_src)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

MI355_API int mi355_copy_d2h(mi355_ctx* ctx, void* h_dst, const void* d_src, size_t nbytes)
{
    if (!ctx || !h_dst || !d_src)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MI355_OK;
}

MI355_API int mi355_timer_begin(mi355_ctx* ctx)
{
    if (!ctx)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->t0, ctx->stream));
    return MI355_OK;
}

MI355_API int mi355_timer_end(mi355_ctx* ctx, float* elapsed_ms)
{
    if (!ctx || !elapsed_ms)
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventRecord(ctx->t1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->t1));
    HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->t0, ctx->t1));
    return MI355_OK;
}

}  // extern "C"

// group.hip installs the table it generated once on every member through this (hidden) hook: same path as a table
// the context generated itself — evictable, outside the cap on caller-installed tables.
int mi355_internal_install_generated(mi355_ctx* ctx, int k, float sigma, const float* w_k2)
{
    if (!ctx || !w_k2 || !valid_k(k) || !valid_sigma(sigma))
        return MI355_ERR_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (auto& e : ctx->coefs)
        if (e.k == k && e.sigma_bits == fbits(sigma))
            return MI355_OK;  // already there (generated or installed by the caller: the caller's table wins)
    return install_coef(ctx, k, sigma, w_k2, false, nullptr);
}

// group.hip checks a call's filter id, frame size, k and sigma through this (hidden) hook before it posts any work:
// check_filter for one frame, and whether the call needs the (k, sigma) table
int mi355_internal_check_filter(int filter, int w, int h, int k, float sigma, bool* needs_table)
{
    const FilterInfo* f = nullptr;
    const int rc = check_filter(filter, w, h, 1, k, sigma, &f);
    if (rc == MI355_OK)
        *needs_table = f->table;
    return rc;
}

extern "C" {

MI355_API const char* mi355_build_info(void) { return "gfx950;" __DATE__ " " __TIME__; }

}  // extern "C"
