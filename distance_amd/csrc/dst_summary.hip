// dst_summary.hip — per-record and histogram summaries of the pairwise distances (dst_summary): integer reductions over one
// row slab of DST_OUT_DISTANCE payloads at a time, into O(n + bins) of state that lives on the device for the whole call
// (DESIGN.md 3p).
//
// Definition (include/distance_hip.h).  Per pair, from its payload v:
//   link      dst_clusters' rule against T: nn_key(v) <= nn_key(T) (int64: v <= floor(T), clamped by the host, `any` false
//             when nothing can link; f64: IEEE v <= T, NaN never, -0.0 as +0.0)
//   q         the fixed-point value: int64 payloads q = v; f64 q = rint(v 2^37) when v is summable (not NaN, |v| < 2^25)
//   bin       NaN none; v >= 2^25 the last; v <= -2^25 bin 0; else clamp(floor(q / width_q), 0, bins - 1)
// Per record: the links, the summable partners and the exact sum of their q, kept as hi = sum of (q >> 32) and lo = sum of
// (q & 0xFFFFFFFF): fewer than 2^32 partners and |q| < 2^62, so neither 64-bit word overflows and there is no carry; the
// host forms hi 2^32 + lo in 128 bits.  Every accumulation across workgroups is an integer agent-scope relaxed atomic, so
// the result is exact whatever the order.
//
//   summary_rows_kernel   the geometry of clusters_link_kernel: workgroup (x, row) takes entries 2048 x .. 2048 x + 2047 of
//                         its row, reduces over the wave by shuffles and over its four waves through LDS, and issues one
//                         set of atomics to record `row` (none of a value that is zero)
//   summary_cols_kernel   square only: thread = column record j, workgroup row = a segment of kColSegRows slab rows; the
//                         thread walks the segment's rows i < j (adjacent lanes read adjacent entries of a row) with
//                         register accumulators and issues its atomics to record j once
//   summary_hist_kernel   flat grid-stride over the slab's entries, a bounded number of workgroups, each with a private
//                         histogram of `bins` 32-bit counters in LDS, flushed at the end with 64-bit atomics (non-zero
//                         bins only).  The lanes of a wave that share the first lane's bin are added as one LDS atomic
//                         (__ballot / __popcll), for two rounds, before the rest fall to plain LDS atomics: low-diversity
//                         data puts nearly every pair of a wave into one or two bins.  The kernel also counts the call's
//                         totals (NaN, summable, links, the sum as a 128-bit integer in two words), so a call that wants
//                         no per-record result reads the slab once.
//   summary_stream_kernel a summary stream's batch (dst_stream.cpp): a tile pass over the batch's n_records x
//                         n_loaded matrix that reads every entry once for both sides: thread = column (loaded record) with
//                         register accumulators and one set of atomics per tile, the tile's rows (streamed records) reduced
//                         over the wave eight at a time and over the waves through LDS, the totals from the column
//                         accumulators.  The two sides are template parameters.
#include "dst_device.hpp"
#include "dst_pair_sum.hpp"

namespace dst {
namespace {

constexpr int kSumWaves = 4;                                       // waves per workgroup
constexpr int kSumSteps = 8;                                       // 64-entry steps per wave
constexpr uint32_t kSumWavePairs = 64u * kSumSteps;                // 512 entries: one wave's run
constexpr uint32_t kSumBlockPairs = kSumWavePairs * kSumWaves;     // 2048 entries of one row per workgroup
constexpr uint32_t kColSegRows = 64;                               // slab rows per workgroup row of the column pass
constexpr uint32_t kHistBlocksMax = 1024;                          // four workgroups per CU
constexpr int kHistAggRounds = 2;

struct SummaryState {
    uint32_t *within, *summable;        // [records]
    long long *hi;                      // [records]
    unsigned long long *lo;             // [records]
    unsigned long long *hist;           // [bins]
    unsigned long long *tot;            // kSummaryTotals words (dst_internal.h)
};

__device__ __forceinline__ void add_to_record(const SummaryState &s, uint32_t x, const Acc &a)
{
    if (a.within)
        __hip_atomic_fetch_add(s.within + x, a.within, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.summable)
        __hip_atomic_fetch_add(s.summable + x, a.summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.hi)
        __hip_atomic_fetch_add(s.hi + x, a.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.lo)
        __hip_atomic_fetch_add(s.lo + x, a.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct SumRows {
    uint64_t out_base;   // canonical index of the slab's first pair (square)
    uint32_t n_cols;     // square: n
    uint32_t rb, re;     // the slab's rows
    int square;
};

// Rows [row0 + blockIdx.y] (below re) of one slab.  Square: pairs (i, j > i) at slab entry tri_row_start(n, i) - out_base
// + (j - i - 1); rectangle: pairs (i, 0 .. n_cols-1) at (i - rb) n_cols + j.  Wave w of workgroup x: the 512 entries from
// 2048 x + 512 w, lane l of step t entry 512 w + 64 t + l.
template <bool INT>
__global__ __launch_bounds__(256) void summary_rows_kernel(const uint64_t *__restrict__ slab, SumRows g, uint32_t row0,
                                                           uint64_t t_bits, int any, SummaryState s)
{
    __shared__ Acc wave_acc[kSumWaves];
    __shared__ uint32_t wave_nan[kSumWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t row_pairs = g.square ? (uint64_t)g.n_cols - i - 1 : (uint64_t)g.n_cols;
    const uint64_t b0 = (uint64_t)blockIdx.x * kSumBlockPairs;
    if (b0 >= row_pairs)
        return;   // (whole workgroups)
    const uint64_t base = g.square ? tri_row_start(g.n_cols, i) - g.out_base : (uint64_t)(i - g.rb) * g.n_cols;
    const uint64_t q0 = b0 + (uint32_t)wave * kSumWavePairs;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint64_t v[kSumSteps];
#pragma unroll
    for (int t = 0; t < kSumSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        v[t] = q < row_pairs ? __builtin_nontemporal_load(slab + base + q) : 0;
    }
    Acc a{};
    uint32_t nan = 0;   // of the wave (uniform)
#pragma unroll
    for (int t = 0; t < kSumSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        if (q < row_pairs)
            add_pair<INT>(a, v[t], t_key, any != 0);
        if constexpr (!INT)
            nan += (uint32_t)__popcll(__ballot(q < row_pairs && is_nan<INT>(v[t])));
    }
    wave_sum(a);
    if (lane == 0) {
        wave_acc[wave] = a;
        wave_nan[wave] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc total{};
        unsigned long long nans = 0;
#pragma unroll
        for (int w = 0; w < kSumWaves; ++w) {
            total.within += wave_acc[w].within;
            total.summable += wave_acc[w].summable;
            total.hi += wave_acc[w].hi;
            total.lo += wave_acc[w].lo;
            nans += wave_nan[w];
        }
        add_to_record(s, i, total);
        if (nans)   // (the row pass meets every pair once: the call's NaN pairs, apart from the flat pass' count)
            __hip_atomic_fetch_add(s.tot + 5, nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The column side of the square: thread j = blockIdx.x * 256 + threadIdx.x takes the rows i < j of segment seg0 +
// blockIdx.y (rows rb + kColSegRows seg .. + kColSegRows - 1, below re).
template <bool INT>
__global__ __launch_bounds__(256) void summary_cols_kernel(const uint64_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                           uint32_t rb, uint32_t re, uint32_t seg0, uint64_t t_bits, int any,
                                                           SummaryState s)
{
    const uint64_t first = (uint64_t)rb + (uint64_t)(seg0 + blockIdx.y) * kColSegRows;
    if (first >= re)
        return;   // (whole workgroups)
    const uint32_t i0 = (uint32_t)first, i1 = (uint32_t)min((uint64_t)re, first + kColSegRows);
    const uint64_t j64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j64 >= n || j64 <= i0)
        return;   // (no row of the segment lies before this column)
    const uint32_t j = (uint32_t)j64, iend = min(i1, j);
    const uint64_t t_key = nn_key<INT>(t_bits);
    Acc a{};
#pragma unroll 4
    for (uint32_t i = i0; i < iend; ++i) {
        const uint64_t at = tri_row_start(n, i) - out_base + (j - i - 1);
        add_pair<INT>(a, __builtin_nontemporal_load(slab + at), t_key, any != 0);
    }
    add_to_record(s, j, a);
}

struct HistBins {
    uint32_t bins;             // 0: the totals only
    unsigned long long w;      // width_q >= 1
    long long limit;           // min(bins width_q, 2^63 - 1): q at or above it lies in the last bin
    double inv_w;              // 1 / width_q, rounded
};

// clamp(floor(q / w), 0, bins - 1).  Below `limit` the quotient is less than bins <= 4096, so the f64 estimate
// q (1 / w) is within 2^-39 of it and its integer part is the floor or one beside it: one multiply and two compares settle
// it.  (k + 1) w <= q + w < 2^63: no overflow.
__device__ __forceinline__ uint32_t bin_of(long long q, const HistBins &h)
{
    if (q < 0)
        return 0;
    if (q >= h.limit)
        return h.bins - 1;
    if (h.w == 1)
        return (uint32_t)q;
    uint32_t k = (uint32_t)((double)q * h.inv_w);
    const long long r = q - (long long)((unsigned long long)k * h.w);
    if (r < 0)
        --k;
    else if ((unsigned long long)r >= h.w)
        ++k;
    return k;
}

// Entries [0, pairs) of the slab, entry e by thread e mod (256 gridDim.x): every wave runs the same number of steps, so the
// ballots see whole waves.  lds: h.bins counters.
template <bool INT, bool AGG>
__global__ __launch_bounds__(256) void summary_hist_kernel(const uint64_t *__restrict__ slab, uint64_t pairs, HistBins h,
                                                           uint64_t t_bits, int any, SummaryState s)
{
    extern __shared__ uint32_t lds[];
    __shared__ Acc wave_acc[kSumWaves];
    __shared__ uint32_t wave_nan[kSumWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    for (uint32_t b = threadIdx.x; b < h.bins; b += 256)
        lds[b] = 0;
    __syncthreads();
    const uint64_t t_key = nn_key<INT>(t_bits);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    Acc a{};
    uint32_t nan = 0;
    for (uint64_t e0 = (uint64_t)blockIdx.x * 256 + (uint32_t)(wave * 64); e0 < pairs; e0 += stride) {   // (wave-uniform)
        const uint64_t e = e0 + (uint32_t)lane;
        const bool valid = e < pairs;
        const uint64_t bits = valid ? __builtin_nontemporal_load(slab + e) : 0;
        const bool is_n = valid && is_nan<INT>(bits);
        nan += is_n;
        if (valid)
            add_pair<INT>(a, bits, t_key, any != 0);
        if (h.bins == 0)
            continue;   // (uniform)
        bool todo = valid && !is_n;
        uint32_t bin = 0;
        if (todo) {
            long long q;
            if (!fixed_point<INT>(bits, q))   // +-inf and finite values of 2^25 and more: the end bins
                q = (bits >> 63) ? -1 : 0x7FFFFFFFFFFFFFFFll;
            bin = bin_of(q, h);
        }
        if constexpr (AGG) {
#pragma unroll
            for (int r = 0; r < kHistAggRounds; ++r) {
                const unsigned long long left = __ballot(todo);
                if (!left)
                    break;   // (uniform)
                const int leader = __ffsll(left) - 1;
                const uint32_t b = (uint32_t)__shfl((int)bin, leader, 64);
                const unsigned long long same = __ballot(todo && bin == b);
                if (lane == leader)
                    atomicAdd(&lds[b], (uint32_t)__popcll(same));
                if (bin == b)
                    todo = false;
            }
        }
        if (todo)
            atomicAdd(&lds[bin], 1u);
    }
    wave_sum(a);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        nan += (uint32_t)__shfl_down((int)nan, off, 64);
    if (lane == 0) {
        wave_acc[wave] = a;
        wave_nan[wave] = nan;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < h.bins; b += 256) {
        const uint32_t c = lds[b];
        if (c)
            __hip_atomic_fetch_add(s.hist + b, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (threadIdx.x == 0) {
        Acc total{};
        unsigned long long nans = 0;
#pragma unroll
        for (int w = 0; w < kSumWaves; ++w) {
            total.within += wave_acc[w].within;
            total.summable += wave_acc[w].summable;
            total.hi += wave_acc[w].hi;
            total.lo += wave_acc[w].lo;
            nans += wave_nan[w];
        }
        if (nans)
            __hip_atomic_fetch_add(s.tot + 0, nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (total.summable)
            __hip_atomic_fetch_add(s.tot + 1, (unsigned long long)total.summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (total.within)
            __hip_atomic_fetch_add(s.tot + 2, (unsigned long long)total.within, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // The sum over ALL pairs can have 2^32 addends and more, so the hi / lo split of a record does not bound it: the
        // workgroup's exact sum hi 2^32 + lo (its entries are fewer than 2^32) is added as a 128-bit integer in two words,
        // the carry of the low word's add taken from the value the atomic returns.  Every carry is added once, so the
        // two words hold the exact total when the call's kernels are done, in whatever order they ran.
        const unsigned long long shifted = (unsigned long long)total.hi << 32, low = shifted + total.lo;
        long long high = (total.hi >> 32) + (low < shifted ? 1 : 0);
        if (low) {
            const unsigned long long old = __hip_atomic_fetch_add(s.tot + 4, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            high += old + low < old ? 1 : 0;
        }
        if (high)
            __hip_atomic_fetch_add(s.tot + 3, (unsigned long long)high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A workgroup's share of the totals, tot[0 .. 4] as summary_hist_kernel's: its NaN pairs, and the sums of fewer than 2^32
// entries.  The exact sum hi 2^32 + lo goes in as a 128-bit integer in two words, the carry of the low word's add taken
// from the value the atomic returns (summary_hist_kernel explains why every carry is added once).
__device__ __forceinline__ void add_to_totals(unsigned long long *tot, unsigned long long nans, const Acc &total)
{
    if (nans)
        __hip_atomic_fetch_add(tot + 0, nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (total.summable)
        __hip_atomic_fetch_add(tot + 1, (unsigned long long)total.summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (total.within)
        __hip_atomic_fetch_add(tot + 2, (unsigned long long)total.within, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long shifted = (unsigned long long)total.hi << 32, low = shifted + total.lo;
    long long high = (total.hi >> 32) + (low < shifted ? 1 : 0);
    if (low) {
        const unsigned long long old = __hip_atomic_fetch_add(tot + 4, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        high += old + low < old ? 1 : 0;
    }
    if (high)
        __hip_atomic_fetch_add(tot + 3, (unsigned long long)high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kStreamSumUnroll = 8;   // rows whose loads a thread has in flight at once

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long x, int mask)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, mask, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), mask, 64);
    return (unsigned long long)hi << 32 | lo;
}

// The wave's sums of eight rows at once, v[u] this lane's entry of row u.  Three exchanges halve the rows a lane holds: with
// the partner across lane bit 5 (then 4, then 3) a lane keeps the rows of its own half, sends the others and adds what it
// receives.  One row is left, row 4 b5 + 2 b4 + b3 of the lane's bits, and three plain steps across bits 2, 1, 0 finish it:
// ten 64-bit exchanges for the eight rows, where eight separate reductions take 48.  Lane sum_rows_lane(u) (and the seven
// lanes behind it) returns row u's sum; two's complement, so the signed word adds like the unsigned one.
__device__ __forceinline__ constexpr int sum_rows_lane(int u) { return ((u >> 2) & 1) * 32 + ((u >> 1) & 1) * 16 + (u & 1) * 8; }

__device__ __forceinline__ unsigned long long wave_sum_rows(const unsigned long long (&v)[kStreamSumUnroll], int lane)
{
    static_assert(kStreamSumUnroll == 8, "three halving steps");
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    unsigned long long w[4], x[2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (b5 ? v[k + 4] : v[k]) + shfl_xor64(b5 ? v[k] : v[k + 4], 32);
#pragma unroll
    for (int k = 0; k < 2; ++k)
        x[k] = (b4 ? w[k + 2] : w[k]) + shfl_xor64(b4 ? w[k] : w[k + 2], 16);
    unsigned long long y = (b3 ? x[1] : x[0]) + shfl_xor64(b3 ? x[0] : x[1], 8);
    y += shfl_xor64(y, 4);
    y += shfl_xor64(y, 2);
    y += shfl_xor64(y, 1);
    return y;
}

static_assert(kStreamSummaryCols == 64u * kSumWaves, "a thread of the workgroup per column of the tile");
static_assert(kStreamSummaryRows % kStreamSumUnroll == 0 && kStreamSummaryRows <= kStreamSummaryCols,
              "whole unrolled steps; a thread per row of the tile flushes it");

// A summary stream's batch: the n_rows x n_cols matrix (row = streamed record, column = loaded record), tile
// (tile0 + blockIdx.y, blockIdx.x) of kStreamSummaryRows x kStreamSummaryCols entries.  Thread t owns column blockIdx.x
// kStreamSummaryCols + t and walks the tile's rows, so a wave reads 64 adjacent entries of a row per load.  The column's
// four quantities stay in registers and go to loaded record j with one set of atomics per tile (LOADED).  Per row the
// wave's counts come from ballots and its two sum words from wave_sum_rows, eight rows at a time (skipped when the wave
// has nothing summable in them); one lane per row leaves them in LDS, and behind the barrier thread r adds the four waves'
// to streamed record r (STREAMED).
// The totals are the sum of the column accumulators: every entry of the tile once.
template <bool INT, bool LOADED, bool STREAMED>
__global__ __launch_bounds__(256) void summary_stream_kernel(const uint64_t *__restrict__ matrix, uint32_t n_rows, uint32_t n_cols,
                                                             uint32_t tile0, uint64_t t_bits, int any, SummaryState cols, SummaryState rows,
                                                             unsigned long long *tot)
{
    __shared__ Acc row_acc[STREAMED ? kStreamSummaryRows : 1][kSumWaves];
    __shared__ Acc wave_acc[kSumWaves];
    __shared__ uint32_t wave_nan[kSumWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint64_t j64 = (uint64_t)blockIdx.x * kStreamSummaryCols + threadIdx.x;
    const bool col_ok = j64 < n_cols;
    const uint32_t r0 = (tile0 + blockIdx.y) * kStreamSummaryRows;        // (below n_rows: the grids have no empty tile row)
    const uint32_t rows_here = min(kStreamSummaryRows, n_rows - r0);
    const uint64_t t_key = nn_key<INT>(t_bits);
    const uint64_t *p = matrix + (uint64_t)r0 * n_cols + (col_ok ? j64 : 0);
    Acc col{};
    uint32_t nan = 0;   // of the wave (uniform)
    for (uint32_t r = 0; r < rows_here; r += kStreamSumUnroll) {   // (uniform)
        uint64_t v[kStreamSumUnroll];
        [[maybe_unused]] uint32_t row_within[kStreamSumUnroll], row_summable[kStreamSumUnroll];   // of the wave (uniform)
        [[maybe_unused]] unsigned long long row_hi[kStreamSumUnroll], row_lo[kStreamSumUnroll];   // this lane's entry of each row
#pragma unroll
        for (int u = 0; u < kStreamSumUnroll; ++u)
            v[u] = col_ok && r + u < rows_here ? __builtin_nontemporal_load(p + (uint64_t)(r + u) * n_cols) : 0;
#pragma unroll
        for (int u = 0; u < kStreamSumUnroll; ++u) {
            const bool ok = col_ok && r + u < rows_here;
            Acc a{};
            if (ok)
                add_pair<INT>(a, v[u], t_key, any != 0);
            col.within += a.within;
            col.summable += a.summable;
            col.hi += a.hi;
            col.lo += a.lo;
            if constexpr (!INT)
                nan += (uint32_t)__popcll(__ballot(ok && is_nan<INT>(v[u])));
            if constexpr (STREAMED) {
                row_within[u] = (uint32_t)__popcll(__ballot(a.within != 0));
                row_summable[u] = (uint32_t)__popcll(__ballot(a.summable != 0));
                row_hi[u] = (unsigned long long)a.hi;
                row_lo[u] = a.lo;
            }
        }
        if constexpr (STREAMED) {
            uint32_t summable = 0;
#pragma unroll
            for (int u = 0; u < kStreamSumUnroll; ++u)
                summable |= row_summable[u];
            unsigned long long hi = 0, lo = 0;
            if (summable) {   // (uniform)
                hi = wave_sum_rows(row_hi, lane);
                lo = wave_sum_rows(row_lo, lane);
            }
#pragma unroll
            for (int u = 0; u < kStreamSumUnroll; ++u)
                if (lane == sum_rows_lane(u) && r + u < rows_here)
                    row_acc[r + u][wave] = Acc{row_within[u], row_summable[u], (long long)hi, lo};
        }
    }
    if constexpr (LOADED) {
        if (col_ok)
            add_to_record(cols, (uint32_t)j64, col);
    }
    wave_sum(col);
    if (lane == 0) {
        wave_acc[wave] = col;
        wave_nan[wave] = nan;
    }
    __syncthreads();
    if constexpr (STREAMED) {
        if (threadIdx.x < rows_here) {
            Acc total{};
#pragma unroll
            for (int w = 0; w < kSumWaves; ++w) {
                total.within += row_acc[threadIdx.x][w].within;
                total.summable += row_acc[threadIdx.x][w].summable;
                total.hi += row_acc[threadIdx.x][w].hi;
                total.lo += row_acc[threadIdx.x][w].lo;
            }
            add_to_record(rows, r0 + threadIdx.x, total);
        }
    }
    if (threadIdx.x == 0) {
        Acc total{};
        unsigned long long nans = 0;
#pragma unroll
        for (int w = 0; w < kSumWaves; ++w) {
            total.within += wave_acc[w].within;
            total.summable += wave_acc[w].summable;
            total.hi += wave_acc[w].hi;
            total.lo += wave_acc[w].lo;
            nans += wave_nan[w];
        }
        add_to_totals(tot, nans, total);
    }
}

SummaryState state_of(const SummaryBuffers &b)
{
    return SummaryState{b.within, b.summable, reinterpret_cast<long long *>(b.hi), reinterpret_cast<unsigned long long *>(b.lo),
                        reinterpret_cast<unsigned long long *>(b.hist), reinterpret_cast<unsigned long long *>(b.tot)};
}

}  // namespace

hipError_t launch_summary_rows(int measure, bool square, const uint64_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                               uint64_t re, uint64_t t_bits, bool any, const SummaryBuffers &b, hipStream_t stream)
{
    const uint64_t longest = square ? (n_cols > rb + 1 ? n_cols - rb - 1 : 0) : n_cols;   // of row rb
    if (re <= rb || longest == 0)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const SumRows g{out_base, (uint32_t)n_cols, (uint32_t)rb, (uint32_t)re, square ? 1 : 0};
    const unsigned chunks = (unsigned)((longest + kSumBlockPairs - 1) / kSumBlockPairs);
    const SummaryState s = state_of(b);
    return for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
        const dim3 grid(chunks, rows);
        if (int_payload)
            hipLaunchKernelGGL(summary_rows_kernel<true>, grid, dim3(256), 0, stream, slab, g, (uint32_t)row0, t_bits,
                               any ? 1 : 0, s);
        else
            hipLaunchKernelGGL(summary_rows_kernel<false>, grid, dim3(256), 0, stream, slab, g, (uint32_t)row0, t_bits,
                               any ? 1 : 0, s);
        return hipGetLastError();
    });
}

hipError_t launch_summary_cols(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                               uint64_t t_bits, bool any, const SummaryBuffers &b, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const uint64_t segs = (re - rb + kColSegRows - 1) / kColSegRows;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const SummaryState s = state_of(b);
    for (uint64_t seg0 = 0; seg0 < segs; seg0 += kGridRowsMax) {
        const dim3 grid(blocks, grid_rows(segs - seg0));
        if (int_payload)
            hipLaunchKernelGGL(summary_cols_kernel<true>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n, (uint32_t)rb,
                               (uint32_t)re, (uint32_t)seg0, t_bits, any ? 1 : 0, s);
        else
            hipLaunchKernelGGL(summary_cols_kernel<false>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n, (uint32_t)rb,
                               (uint32_t)re, (uint32_t)seg0, t_bits, any ? 1 : 0, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t launch_summary_hist(int measure, const uint64_t *slab, uint64_t pairs, uint32_t bins, uint64_t width_q,
                               uint64_t t_bits, bool any, bool aggregate, const SummaryBuffers &b, hipStream_t stream)
{
    if (pairs == 0)
        return hipSuccess;
    if (bins > DST_SUMMARY_MAX_BINS || (bins && width_q == 0))
        return hipErrorInvalidValue;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    HistBins h;
    h.bins = bins;
    h.w = bins ? width_q : 1;
    const unsigned __int128 lim = (unsigned __int128)bins * h.w;
    h.limit = lim > (unsigned __int128)INT64_MAX ? INT64_MAX : (long long)lim;
    h.inv_w = 1.0 / (double)h.w;
    const unsigned blocks = (unsigned)std::min<uint64_t>((pairs + 255) / 256, kHistBlocksMax);
    const size_t lds = (size_t)bins * sizeof(uint32_t);
    const SummaryState s = state_of(b);
#define DST_SUMMARY_HIST(INT, AGG)                                                                                             \
    hipLaunchKernelGGL((summary_hist_kernel<INT, AGG>), dim3(blocks), dim3(256), lds, stream, slab, pairs, h, t_bits,          \
                       any ? 1 : 0, s)
    if (int_payload) {
        if (aggregate)
            DST_SUMMARY_HIST(true, true);
        else
            DST_SUMMARY_HIST(true, false);
    } else {
        if (aggregate)
            DST_SUMMARY_HIST(false, true);
        else
            DST_SUMMARY_HIST(false, false);
    }
#undef DST_SUMMARY_HIST
    return hipGetLastError();
}

hipError_t launch_summary_stream(int measure, const uint64_t *matrix, uint64_t n_records, uint64_t n_loaded, uint64_t t_bits,
                                 bool any, const SummaryBuffers *loaded, const SummaryBuffers *streamed, uint64_t *tot,
                                 hipStream_t stream)
{
    if (n_records == 0 || n_loaded == 0)
        return hipSuccess;
    if (n_records > 0xFFFFFFFFull || n_loaded > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const unsigned col_tiles = (unsigned)((n_loaded + kStreamSummaryCols - 1) / kStreamSummaryCols);
    const uint64_t row_tiles = (n_records + kStreamSummaryRows - 1) / kStreamSummaryRows;
    const SummaryState none{};
    const SummaryState c = loaded ? state_of(*loaded) : none, r = streamed ? state_of(*streamed) : none;
    unsigned long long *t = reinterpret_cast<unsigned long long *>(tot);
    return for_row_grids(0, row_tiles, [&](uint64_t tile0, unsigned tiles) {
        const dim3 grid(col_tiles, tiles);
#define DST_SUMMARY_STREAM(INT, L, S)                                                                                          \
    hipLaunchKernelGGL((summary_stream_kernel<INT, L, S>), grid, dim3(256), 0, stream, matrix, (uint32_t)n_records,            \
                       (uint32_t)n_loaded, (uint32_t)tile0, t_bits, any ? 1 : 0, c, r, t)
#define DST_SUMMARY_STREAM_SIDES(INT)                                                                                          \
    do {                                                                                                                       \
        if (loaded && streamed)                                                                                                \
            DST_SUMMARY_STREAM(INT, true, true);                                                                               \
        else if (loaded)                                                                                                       \
            DST_SUMMARY_STREAM(INT, true, false);                                                                              \
        else if (streamed)                                                                                                     \
            DST_SUMMARY_STREAM(INT, false, true);                                                                              \
        else                                                                                                                   \
            DST_SUMMARY_STREAM(INT, false, false);                                                                             \
    } while (0)
        if (int_payload)
            DST_SUMMARY_STREAM_SIDES(true);
        else
            DST_SUMMARY_STREAM_SIDES(false);
#undef DST_SUMMARY_STREAM_SIDES
#undef DST_SUMMARY_STREAM
        return hipGetLastError();
    });
}

}  // namespace dst
