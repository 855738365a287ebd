// hough.hip — cv::HoughLines (the standard transform) of single-channel edge maps.  Semantics: include/mi355_imgfilter.h,
// "from edges to lines"; design, the LDS budget and the loop bounds: DESIGN.md section 6l.
//
//   hough_points_kernel  the mask becomes a point list per frame, x | y << 16, in raster order inside a block (16 bytes per
//                        thread, a wave prefix sum of the nonzero counts, one global add per block for the block's place in
//                        the list).  The order of the blocks in the list is whatever the adds decide: votes are integer adds
//                        and commute.
//   hough_vote_kernel    the hot path.  A block of 1024 threads owns up to kHoughBlockAngles angles of one frame (or, for a
//                        row longer than the LDS budget, one rho range of one angle), zeroes its rows in LDS, walks the
//                        frame's whole point list (kHoughUnroll points per thread and trip, their loads in flight together)
//                        and votes with return-less LDS adds, then stores its rows, the zero ring
//                        around them included, with coalesced dword stores: every accumulator cell reaches memory exactly once
//                        and no global atomic is used.  The cell of a vote is three separately rounded fp32 operations
//                        (__fmul_rn, __fmul_rn, __fadd_rn) and a round-to-nearest-even conversion.
//                        Run aggregation: neighbouring lanes hold neighbouring points of an image row, and for a fixed angle
//                        the cell is monotone in x, so where the cell moves by at most kHoughAggStep per pixel equal cells sit
//                        in neighbouring lanes.  There a lane compares its cell with the lane before it (DPP row_shr:1; a row
//                        of 16 lanes always starts a run), the run starts are balloted and the first lane of a run adds the
//                        run length once.  Steeper angles add lane by lane.
//   hough_peaks_kernel   every interior cell against the header's five comparisons; a peak appends the key
//                        votes << 29 | (2^29 - 1 - cell) to the frame's candidate list (one global add per wave on d_count,
//                        which thereby becomes the peak count).  The list's order is arbitrary, the keys are distinct.
//   hough_select_kernel  one block per frame.  More candidates than max_lines: a radix select (five 12-bit digits, an LDS
//                        histogram per digit) finds the max_lines-th largest key exactly, and the keys >= it are gathered.  A
//                        bitonic sort of at most 4096 keys in LDS puts them in the contract's order (votes descending, cell
//                        ascending = key descending), and the (rho, theta) rows, the votes and the zero fill are written.
// Kernel boundaries are the only ordering between workgroups: no flag, no grid barrier, no retry; every loop is bounded by
// a count fixed before it starts.  Grids, prefix sums, compaction and chunk bytes: mask_common.hpp.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"
#include "mask_common.hpp"
#include "tile_common.hpp"

namespace mi355 {

namespace {

constexpr int kHoughThreads = 1024;       // of a voting and of a selecting block
constexpr int kHoughPointThreads = 256;   // of a block that lists points or tests peaks
constexpr int kHoughPointBytes = 16;      // mask bytes per thread of hough_points_kernel
constexpr uint32_t kHoughPointBlock = kHoughPointThreads * kHoughPointBytes;
constexpr int kHoughSmallCells = 8192;    // 32 KiB: two voting blocks fit a CU (2048 threads)
constexpr int kHoughDigitBits = 12, kHoughDigits = 1 << kHoughDigitBits;
constexpr int kHoughKeyBits = 60;         // 31 bits of votes above 29 bits of inverted cell index
constexpr uint32_t kHoughIndexMask = (1u << 29) - 1u;
static_assert(kHoughKeyBits % kHoughDigitBits == 0, "whole digits");
static_assert(kHoughMaxLines <= 4096 && (kHoughMaxLines & (kHoughMaxLines - 1)) == 0, "the LDS sort holds every line");
static_assert(kHoughLdsCells * sizeof(uint32_t) + 1024 <= 160 * 1024, "the rows and the block's small arrays fit a CU's LDS");

constexpr int kHoughUnroll = 4;  // points per thread and trip of the voting loop

// cells the per-pixel step of which is at most this take the run-aggregated add
constexpr float kHoughAggStep = 0.5f;

struct VoteArgs {
    const uint32_t* pts;   // the frames' point lists, pts_stride entries apart
    const uint32_t* npts;  // points per frame
    int32_t* accum;        // (numangle + 2) x (numrho + 2) per frame
    const float* tab;      // numangle cosines * irho, then numangle sines * irho
    size_t pts_stride;
    int numangle, numrho;
    int angles;  // per block
    int splits;  // rho ranges per row (1: the whole row in one block)
    int span;    // cells per rho range
    int groups;  // angle groups per frame
    float agg_step;
};

__global__ __launch_bounds__(kHoughPointThreads) void hough_points_kernel(const uint8_t* __restrict__ in,
                                                                          uint32_t* __restrict__ pts,
                                                                          uint32_t* __restrict__ npts, uint32_t w,
                                                                          uint32_t npx, uint32_t bpf)
{
    __shared__ uint32_t wave_sum[kHoughPointThreads / kWave];
    __shared__ uint32_t block_base;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const auto [f, blk, item] = frame_block(bpf, kHoughPointThreads);
    const uint8_t* fin = in + (size_t)f * npx;
    const uint32_t p0 = item * kHoughPointBytes;  // npx < 2^31: no wrap
    const u32x4 v = p0 + kHoughPointBytes <= npx ? *reinterpret_cast<const u32x4_a1*>(fin + p0)
                                                 : load_chunk_bytes(fin + p0, 0, p0 < npx ? (int)(npx - p0) : 0);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kHoughPointBytes; j++)
        m |= (chunk_byte(v, j) != 0u ? 1u : 0u) << j;
    const uint32_t cnt = (uint32_t)__popc(m);
    const uint32_t inc = wave_scan_inclusive(cnt, lane);
    const BlockOffsets o = block_offsets<kHoughPointThreads / kWave>(inc, wave_sum, lane, wave);
    if (tid == 0)
        block_base = o.total ? __hip_atomic_fetch_add(npts + f, o.total, MI355_RELAXED_AGENT) : 0u;
    __syncthreads();
    if (cnt == 0)
        return;
    // block_base + total <= the nonzero bytes of the frame <= npx: the list cannot overflow its npx entries
    uint32_t* dst = pts + (size_t)f * npx + block_base + o.before + (inc - cnt);
    uint32_t y = p0 / w, x = p0 - y * w;
#pragma unroll
    for (int j = 0; j < kHoughPointBytes; j++) {
        if ((m >> j) & 1u)
            *dst++ = x | (y << 16);
        if (++x == w) {
            x = 0;
            y++;
        }
    }
}

// one vote of every lane with `in` set for cell rr of `row`, lane by lane
__device__ __forceinline__ void vote_plain(uint32_t* row, int rr, bool in)
{
    if (in)
        lds_add(row, (uint32_t)rr, 1u);
}

// the same votes with equal neighbours merged: all 64 lanes of the wave call this together
__device__ __forceinline__ void vote_runs(uint32_t* row, int rr, bool in, int lane)
{
    const int key = in ? rr : -1 - lane;  // a lane without a vote never joins a run
    const int prev = __builtin_amdgcn_update_dpp(0, key, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
    const bool start = (lane & 15) == 0 || key != prev;
    const uint64_t starts = __ballot(start);
    if (start && in) {
        const uint64_t rest = (starts >> lane) >> 1;  // the run starts after this lane
        const uint32_t len = rest ? (uint32_t)__ffsll((unsigned long long)rest) : (uint32_t)(kWave - lane);
        lds_add(row, (uint32_t)rr, len);
    }
}

// U points per thread and trip, kHoughThreads apart (neighbouring lanes keep neighbouring points): U loads in flight
template <int CELLS, int U>
__global__ __launch_bounds__(kHoughThreads) void hough_vote_kernel(const VoteArgs a)
{
    __shared__ uint32_t cells[CELLS];
    __shared__ float tcos[kHoughBlockAngles], tsin[kHoughBlockAngles];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    uint32_t b = blockIdx.x;
    const int s = (int)(b % (uint32_t)a.splits);
    b /= (uint32_t)a.splits;
    const int g = (int)(b % (uint32_t)a.groups);
    const uint32_t f = b / (uint32_t)a.groups;
    const int n0 = g * a.angles, na = min(a.angles, a.numangle - n0);
    const int r_lo = s * a.span, r_hi = min(a.numrho, r_lo + a.span), span = r_hi - r_lo;  // na * span <= CELLS (hough_plan)
    for (int i = tid; i < na * span; i += kHoughThreads)  // bound: CELLS / kHoughThreads trips
        cells[i] = 0u;
    if (tid < na) {
        tcos[tid] = a.tab[n0 + tid];
        tsin[tid] = a.tab[a.numangle + n0 + tid];
    }
    __syncthreads();

    const uint32_t np = min(a.npts[f], (uint32_t)a.pts_stride);
    const uint32_t* pts = a.pts + (size_t)f * a.pts_stride;
    const int half = (a.numrho - 1) / 2;
    for (uint32_t base = 0; base < np; base += kHoughThreads * U) {  // bound: np <= w * h, whole waves walk together
        uint32_t pj[U];
        bool vj[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const uint32_t i = base + (uint32_t)(j * kHoughThreads + tid);
            vj[j] = i < np;
            pj[j] = vj[j] ? pts[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const bool valid = vj[j];
            const float fx = (float)(pj[j] & 0xFFFFu), fy = (float)(pj[j] >> 16);
            for (int k = 0; k < na; k++) {  // bound: kHoughBlockAngles
                // wave-uniform by construction; readfirstlane says so to the compiler, and vote_runs needs whole waves
                const float c = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tcos[k])));
                const float sn = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tsin[k])));
                const int r = __float2int_rn(__fadd_rn(__fmul_rn(fx, c), __fmul_rn(fy, sn))) + half;
                const int rr = r - r_lo;
                const bool in = valid && (uint32_t)rr < (uint32_t)span;  // also drops a cell outside the row (header: votes)
                if (__builtin_fabsf(c) <= a.agg_step)                   // uniform in the block
                    vote_runs(cells + k * span, rr, in, lane);
                else
                    vote_plain(cells + k * span, rr, in);
            }
        }
    }
    __syncthreads();

    // The block's share of the accumulator: for each of its rows the columns [j_lo, j_hi) of the numrho + 2, where cell r
    // is column r + 1; the first range also takes column 0 and the last one column numrho + 1 (the ring).  The first angle
    // group adds row 0 and the last one row numangle + 1, all zero.
    const int rowlen = a.numrho + 2;
    const int j_lo = s == 0 ? 0 : r_lo + 1, j_hi = s == a.splits - 1 ? rowlen : r_hi + 1;
    int32_t* acc = a.accum + (size_t)f * (size_t)(a.numangle + 2) * (size_t)rowlen;
    const int first = g == 0 ? -1 : 0, last = g == a.groups - 1 ? na + 1 : na;
    for (int k = first; k < last; k++) {  // bound: kHoughBlockAngles + 2
        const bool ring = k < 0 || k >= na;
        int32_t* dst = acc + (size_t)(k < 0 ? 0 : n0 + k + 1) * (size_t)rowlen;
        for (int j = j_lo + tid; j < j_hi; j += kHoughThreads) {  // bound: (span + 2) / kHoughThreads trips, rounded up
            const int rr = j - 1 - r_lo;
            dst[j] = (!ring && (uint32_t)rr < (uint32_t)span) ? (int32_t)cells[k * span + rr] : 0;
        }
    }
}

__global__ __launch_bounds__(kHoughPointThreads) void hough_peaks_kernel(const int32_t* __restrict__ accum,
                                                                         uint64_t* __restrict__ cand,
                                                                         uint32_t* __restrict__ count, int numangle,
                                                                         int numrho, int threshold, size_t cand_stride,
                                                                         uint32_t bpf)
{
    const int lane = threadIdx.x & (kWave - 1);
    const auto [f, blk, i] = frame_block(bpf, kHoughPointThreads);  // i: interior cell number: numangle * numrho < 2^29
    const uint32_t ncell = (uint32_t)numangle * (uint32_t)numrho;
    const int S = numrho + 2;
    const int32_t* a = accum + (size_t)f * (size_t)(numangle + 2) * (size_t)S;
    bool peak = false;
    uint32_t cell = 0;
    int v = 0;
    if (i < ncell) {
        const uint32_t n = i / (uint32_t)numrho, r = i - n * (uint32_t)numrho;
        cell = (n + 1u) * (uint32_t)S + r + 1u;
        v = a[cell];
        peak = v > threshold && v > a[cell - 1] && v >= a[cell + 1] && v > a[cell - S] && v >= a[cell + S];
    }
    const uint64_t m = __ballot(peak);
    if (m == 0)
        return;
    const size_t slot = (size_t)wave_add_once(count + f, m, lane) + (size_t)lanes_below(m, lane);
    // two neighbours of a row cannot both be peaks (> to the left, >= to the right), so a frame has at most
    // numangle * ceil(numrho / 2) = cand_stride of them; the test below never fails and guards the store all the same
    if (peak && slot < cand_stride)
        cand[(size_t)f * cand_stride + slot] = ((uint64_t)(uint32_t)v << 29) | (uint64_t)(kHoughIndexMask - cell);
}

__global__ __launch_bounds__(kHoughThreads) void hough_select_kernel(const uint64_t* __restrict__ cand,
                                                                     const uint32_t* __restrict__ count,
                                                                     float* __restrict__ lines, int32_t* __restrict__ votes,
                                                                     size_t cand_stride, int numrho, int max_lines,
                                                                     float rho_f, float theta_f, float min_theta_f)
{
    __shared__ uint64_t keys[kHoughMaxLines];
    __shared__ uint32_t hist[kHoughDigits];
    __shared__ uint32_t sh_digit, sh_need, sh_fill;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t f = blockIdx.x;
    const uint64_t* list = cand + (size_t)f * cand_stride;
    const uint32_t n = (uint32_t)min((size_t)count[f], cand_stride);
    const uint32_t m = min(n, (uint32_t)max_lines);
    uint32_t P = 1;
    while (P < m)  // bound: 12 doublings
        P *= 2;
    for (uint32_t i = tid; i < P; i += kHoughThreads)  // bound: 4 trips
        keys[i] = 0;  // below every key: a peak has at least one vote
    if (tid == 0)
        sh_fill = 0;
    __syncthreads();
    if (n <= (uint32_t)max_lines) {
        for (uint32_t i = tid; i < n; i += kHoughThreads)  // bound: 4 trips
            keys[i] = list[i];
    } else {
        // the max_lines-th largest key, digit by digit from the top; `need` keys are still wanted among those that share
        // the digits found so far
        uint64_t prefix = 0;
        uint32_t need = (uint32_t)max_lines;
        for (int shift = kHoughKeyBits - kHoughDigitBits; shift >= 0; shift -= kHoughDigitBits) {  // bound: 5 digits
            for (int i = tid; i < kHoughDigits; i += kHoughThreads)
                hist[i] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < n; i += kHoughThreads) {  // bound: n / kHoughThreads trips, rounded up
                const uint64_t key = list[i];
                if ((key >> (shift + kHoughDigitBits)) == prefix)
                    lds_add(hist, (uint32_t)(key >> shift) & (kHoughDigits - 1), 1u);
            }
            __syncthreads();
            if (tid < kWave) {
                // lane l owns the 64 bins from the top down, kHoughDigits - 1 - 64 l first
                constexpr int kPer = kHoughDigits / kWave;
                const int top = kHoughDigits - 1 - kPer * lane;
                uint32_t own = 0;
#pragma unroll 4
                for (int k = 0; k < kPer; k++)  // bound: 64 bins
                    own += hist[top - k];
                const uint32_t inc = wave_scan_inclusive(own, lane);
                const uint64_t reached = __ballot(inc >= need);  // never empty: at least `need` keys share the prefix
                if (reached && lane == __ffsll((unsigned long long)reached) - 1) {
                    uint32_t above = inc - own;
                    int d = top;
#pragma unroll 1
                    for (int k = 0; k < kPer; k++) {  // bound: 64 bins
                        d = top - k;
                        if (above + hist[d] >= need)
                            break;
                        above += hist[d];
                    }
                    sh_digit = (uint32_t)d;
                    sh_need = need - above;
                }
            }
            __syncthreads();
            prefix = (prefix << kHoughDigitBits) | sh_digit;
            need = sh_need;
            __syncthreads();
        }
        // prefix is that key; the keys are distinct, so exactly max_lines of them are >= it
        for (uint32_t i = tid; i < n; i += kHoughThreads) {  // bound: as above
            const uint64_t key = list[i];
            if (key >= prefix) {
                const uint32_t at = __hip_atomic_fetch_add(&sh_fill, 1u, MI355_RELAXED_WG);
                if (at < (uint32_t)kHoughMaxLines)
                    keys[at] = key;
            }
        }
    }
    __syncthreads();
    // bitonic sort, descending, of P <= 4096 keys
    for (uint32_t k = 2; k <= P; k *= 2) {          // bound: 12
        for (uint32_t j = k / 2; j > 0; j /= 2) {   // bound: 12
            for (uint32_t i = tid; i < P; i += kHoughThreads) {  // bound: 4 trips
                const uint32_t o = i ^ j;
                if (o > i) {
                    const uint64_t x = keys[i], y = keys[o];
                    const bool desc = (i & k) == 0;
                    if (desc ? x < y : x > y) {
                        keys[i] = y;
                        keys[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    const uint32_t S = (uint32_t)numrho + 2u;
    const float centre = __fmul_rn((float)(numrho - 1), 0.5f);
    float* fl = lines + (size_t)f * (size_t)max_lines * 2;
    int32_t* fv = votes ? votes + (size_t)f * (size_t)max_lines : nullptr;
    for (uint32_t i = tid; i < (uint32_t)max_lines; i += kHoughThreads) {  // bound: 4 trips
        float rho = 0.0f, theta = 0.0f;
        int32_t v = 0;
        if (i < m) {
            const uint64_t key = keys[i];
            const uint32_t cell = kHoughIndexMask - ((uint32_t)key & kHoughIndexMask);
            const uint32_t nn = cell / S - 1u, r = cell - (nn + 1u) * S - 1u;
            v = (int32_t)(key >> 29);
            rho = __fmul_rn(__fsub_rn((float)(int)r, centre), rho_f);
            theta = __fadd_rn(min_theta_f, __fmul_rn((float)(int)nn, theta_f));
        }
        fl[2 * i] = rho;
        fl[2 * i + 1] = theta;
        if (fv)
            fv[i] = v;
    }
}

// peaks a frame can have at most: no two neighbours of a row
size_t cand_stride_of(const HoughGeom& g) { return (size_t)g.numangle * (size_t)((g.numrho + 1) / 2); }

size_t counters_bytes(const HoughGeom& g) { return ((size_t)g.nframes * sizeof(uint32_t) + 15) & ~(size_t)15; }

bool geom_ok(const HoughGeom& g)
{
    return hist_frames_ok(g.w, g.h, g.nframes) && g.w <= kWarpMaxSize && g.h <= kWarpMaxSize && g.numangle >= 1 &&
           g.numangle <= kHoughMaxAngles && g.numrho >= 1 &&
           (uint64_t)(g.numangle + 2) * (uint64_t)(g.numrho + 2) * sizeof(int32_t) < (1ull << 31);
}

}  // namespace

HoughPlan hough_plan(int numangle, int numrho)
{
    HoughPlan p = {};
    if (numangle < 1 || numrho < 1)
        return p;
    p.lds_cells = kHoughLdsCells;
    if (numrho <= kHoughLdsCells) {
        int cap = kHoughBlockAngles;
        if (const char* e = tune_env("MI355_TUNE_HOUGH_ANGLES")) {
            const int v = atoi(e);
            if (v >= 1 && v <= kHoughBlockAngles)
                cap = v;
        }
        p.angles_per_block = std::min(std::min(kHoughLdsCells / numrho, cap), numangle);
        p.rho_splits = 1;
        p.span = numrho;
    } else {
        p.angles_per_block = 1;
        p.rho_splits = (numrho + kHoughLdsCells - 1) / kHoughLdsCells;
        p.span = kHoughLdsCells;
    }
    return p;
}

size_t hough_scratch_bytes(const HoughGeom& g)
{
    if (!geom_ok(g))
        return 0;
    // the point lists and the candidate lists are never alive together: they share the bytes behind the counters
    const size_t pts = (size_t)g.nframes * (size_t)g.w * (size_t)g.h * sizeof(uint32_t);
    const size_t cnd = (size_t)g.nframes * cand_stride_of(g) * sizeof(uint64_t);
    return counters_bytes(g) + std::max(pts, cnd);
}

hipError_t launch_hough_accum(hipStream_t stream, const uint8_t* d_in, int32_t* d_accum, const float* d_tab, void* d_scratch,
                              const HoughGeom& g)
{
    if (!geom_ok(g))
        return hipErrorInvalidValue;
    const HoughPlan p = hough_plan(g.numangle, g.numrho);
    const uint32_t npx = (uint32_t)g.w * (uint32_t)g.h;
    const int groups = (g.numangle + p.angles_per_block - 1) / p.angles_per_block;
    const FrameGrid pg = frame_grid(npx, kHoughPointBlock, g.nframes);
    const FrameGrid vg = frame_grid((uint64_t)groups * (uint64_t)p.rho_splits, 1, g.nframes);
    if (!pg.ok || !vg.ok)
        return hipErrorInvalidValue;
    uint32_t* npts = static_cast<uint32_t*>(d_scratch);
    uint32_t* pts = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_scratch) + counters_bytes(g));
    hipError_t e = hipMemsetAsync(npts, 0, (size_t)g.nframes * sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(hough_points_kernel, dim3(pg.blocks), dim3(kHoughPointThreads), 0, stream, d_in, pts, npts,
                       (uint32_t)g.w, npx, pg.bpf);
    VoteArgs a;
    a.pts = pts;
    a.npts = npts;
    a.accum = d_accum;
    a.tab = d_tab;
    a.pts_stride = npx;
    a.numangle = g.numangle;
    a.numrho = g.numrho;
    a.angles = p.angles_per_block;
    a.splits = p.rho_splits;
    a.span = p.span;
    a.groups = groups;
    a.agg_step = kHoughAggStep;
    if (const char* env = tune_env("MI355_TUNE_HOUGH_AGG"))  // 0: never aggregate, 1: always
        a.agg_step = atoi(env) ? 3.0e38f : -1.0f;
    int unroll = kHoughUnroll;
    if (const char* env = tune_env("MI355_TUNE_HOUGH_UNROLL"))
        unroll = atoi(env) == 1 ? 1 : kHoughUnroll;
    const bool small = p.angles_per_block * p.span <= kHoughSmallCells;
    const dim3 grid(vg.blocks), block(kHoughThreads);
    if (small && unroll == 1)
        hipLaunchKernelGGL((hough_vote_kernel<kHoughSmallCells, 1>), grid, block, 0, stream, a);
    else if (small)
        hipLaunchKernelGGL((hough_vote_kernel<kHoughSmallCells, kHoughUnroll>), grid, block, 0, stream, a);
    else if (unroll == 1)
        hipLaunchKernelGGL((hough_vote_kernel<kHoughLdsCells, 1>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((hough_vote_kernel<kHoughLdsCells, kHoughUnroll>), grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_hough_lines(hipStream_t stream, const int32_t* d_accum, float* d_lines, int32_t* d_votes, int32_t* d_count,
                              void* d_scratch, const HoughGeom& g, int threshold, int max_lines)
{
    if (!geom_ok(g) || threshold < 0 || max_lines < 1 || max_lines > kHoughMaxLines)
        return hipErrorInvalidValue;
    const uint32_t ncell = (uint32_t)g.numangle * (uint32_t)g.numrho;
    const FrameGrid pg = frame_grid(ncell, kHoughPointThreads, g.nframes);
    if (!pg.ok)
        return hipErrorInvalidValue;
    uint64_t* cand = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_scratch) + counters_bytes(g));
    uint32_t* count = reinterpret_cast<uint32_t*>(d_count);
    const hipError_t e = hipMemsetAsync(count, 0, (size_t)g.nframes * sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(hough_peaks_kernel, dim3(pg.blocks), dim3(kHoughPointThreads), 0, stream, d_accum, cand, count,
                       g.numangle, g.numrho, threshold, cand_stride_of(g), pg.bpf);
    hipLaunchKernelGGL(hough_select_kernel, dim3((uint32_t)g.nframes), dim3(kHoughThreads), 0, stream, cand, count, d_lines,
                       d_votes, cand_stride_of(g), g.numrho, max_lines, g.rho_f, g.theta_f, g.min_theta_f);
    return hipGetLastError();
}

}  // namespace mi355
