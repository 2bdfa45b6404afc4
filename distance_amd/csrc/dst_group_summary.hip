// dst_group_summary.hip — dst_summary's exact sums keyed by group (dst_group_summary): per (record, group of the partner)
// and per (group, group), from one row slab of DST_OUT_DISTANCE payloads at a time.
//
// Definition (include/distance_hip.h).  Per pair the link rule, q, "summable" and NaN are dst_summary's (dst_pair_sum.hpp).
// Device state for the whole call (GroupBuffers, dst_internal.h):
//   rec      [n_rows x G_c] per (record x, column group g): counts = within << 32 | summable (fewer than 2^32 - 1 partners:
//            no carry between the halves), hi = sum of (q >> 32), lo = sum of (q & 0xFFFFFFFF), as dst_summary's records
//   cell     kGroupCellWords planes of [G_r x G_c] words: NaN pairs, links, summable pairs, the 128-bit sum in two words,
//            the smallest and the largest nn_key of the pairs that are not NaN
// Every accumulation across workgroups is an integer agent-scope relaxed atomic (add; min / max on the key), so the
// result is exact whatever the order.
//
//   group_rows_kernel   the geometry of summary_rows_kernel: workgroup (x, row i) takes entries 2048 x .. 2048 x + 2047 of
//                       its row, wave w the 512 from 512 w, and looks up the column group of every entry.  The workgroup
//                       keeps a private table in LDS, five 64-bit words per column group (the three counts packed into
//                       one, hi, lo, min key, max key): 40 B x G_c, 40 KB at DST_GROUPS_MAX.  AGG: a wave first takes the
//                       group of its first open entry, every lane sums ITS entries of that group in registers, the wave
//                       reduces by shuffles and lane 0 adds once to the table, for kGroupAggRounds rounds; what is left
//                       goes to the table entry by entry.  Two or three large groups put a whole wave on as many table
//                       words, and same-address LDS atomics run one lane at a time.  The non-empty table entries are
//                       flushed to row i's line of `rec`, NaN / min / max to cell (group of i, g).
//   group_cols_kernel   square only, the other record of every pair: thread = column j, workgroup row = a segment of
//                       kGroupSegRows slab rows.  The row's group is uniform over the workgroup, so the segment's rows
//                       are first ranked by group in LDS and walked in that order: a thread keeps register accumulators
//                       while consecutive rows share a group and issues its atomics to rec[j][group] on a change.
//   group_fold_kernel   after the walk: rec into the cells' links, summable and 128-bit sum.  Thread = column group g over
//                       a stretch of kGroupFoldRecs records taken in order of their group (`order`, from the host), again
//                       with register accumulators flushed on a change; the carry of the low word's add comes from the
//                       value the atomic returns, as for dst_summary's totals.
//   group_stream_cols_kernel   a group-summary stream's LOADED side (dst_stream.cpp): group_cols_kernel's
//                       method on the batch's rectangle, without the triangle.  Tile = kStreamGroupRows streamed rows x
//                       kStreamGroupCols loaded columns, thread = loaded column j; the tile's rows are ranked by their
//                       streamed group in LDS and walked in that order, eight loads in flight, register accumulators
//                       flushed to the kept table's entry (group, j) on a change.  The table is group-major, so a wave's
//                       64 flushes of one word are 512 adjacent bytes: one lane per line is the slow shape of a global
//                       atomic.
#include "dst_device.hpp"
#include "dst_pair_sum.hpp"

namespace dst {
namespace {

constexpr int kGrpWaves = 4;                                       // waves per workgroup
constexpr int kGrpSteps = 8;                                       // 64-entry steps per wave
constexpr uint32_t kGrpWavePairs = 64u * kGrpSteps;                // 512 entries: one wave's run
constexpr uint32_t kGrpBlockPairs = kGrpWavePairs * kGrpWaves;     // 2048 entries of one row per workgroup
constexpr uint32_t kGroupSegRows = 64;                             // slab rows per workgroup row of the column pass
constexpr uint32_t kGroupFoldRecs = 256;                           // records per workgroup of the fold
constexpr int kGroupAggRounds = 3;
constexpr int kGrpLdsWords = 5;                                    // per column group: counts, hi, lo, min key, max key

struct GroupState {
    const uint32_t *row_group, *col_group, *order;
    unsigned long long *counts;   // rec
    long long *hi;
    unsigned long long *lo;
    unsigned long long *cell;     // plane p of cell c at cell[p * cells + c]
    uint64_t cells;               // G_r x G_c
    uint32_t g_cols;
};

// what a set of entries of one column group adds
struct GroupAcc {
    Acc a;
    uint32_t nan;
    unsigned long long kmin, kmax;   // over the entries that are not NaN (~0 / 0: none)
};

__device__ __forceinline__ GroupAcc group_acc_zero() { return GroupAcc{Acc{}, 0, ~0ull, 0}; }

template <bool INT>
__device__ __forceinline__ void add_entry(GroupAcc &x, uint64_t bits, uint64_t t_key, bool any)
{
    if (is_nan<INT>(bits)) {
        ++x.nan;
    } else {
        const unsigned long long k = nn_key<INT>(bits);
        x.kmin = min(x.kmin, k);
        x.kmax = max(x.kmax, k);
    }
    add_pair<INT>(x.a, bits, t_key, any);
}

// the workgroup's table: counts word = NaN << 48 | within << 24 | summable (each at most 2048 per workgroup)
__device__ __forceinline__ void table_add(unsigned long long *tab, uint32_t G, uint32_t g, const GroupAcc &x)
{
    const unsigned long long c = (unsigned long long)x.nan << 48 | (unsigned long long)x.a.within << 24 | x.a.summable;
    if (c)
        __hip_atomic_fetch_add(tab + g, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x.a.hi)
        __hip_atomic_fetch_add(tab + G + g, (unsigned long long)x.a.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x.a.lo)
        __hip_atomic_fetch_add(tab + 2 * G + g, x.a.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x.kmin != ~0ull)
        __hip_atomic_fetch_min(tab + 3 * G + g, x.kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (x.kmax != 0)
        __hip_atomic_fetch_max(tab + 4 * G + g, x.kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void add_to_entry(const GroupState &s, uint64_t at, const Acc &a)
{
    const unsigned long long c = (unsigned long long)a.within << 32 | a.summable;
    if (c)
        __hip_atomic_fetch_add(s.counts + at, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.hi)
        __hip_atomic_fetch_add(s.hi + at, a.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.lo)
        __hip_atomic_fetch_add(s.lo + at, a.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct GroupRows {
    uint64_t out_base;   // canonical index of the slab's first pair (square)
    uint32_t n_cols;     // square: n
    uint32_t rb, re;     // the slab's rows
    int square;
};

// Rows [row0 + blockIdx.y] (below re) of one slab, indexed as summary_rows_kernel's.  lds: kGrpLdsWords x g_cols words.
template <bool INT, bool AGG>
__global__ __launch_bounds__(256) void group_rows_kernel(const uint64_t *__restrict__ slab, GroupRows g, uint32_t row0,
                                                         uint64_t t_bits, int any, GroupState s)
{
    extern __shared__ unsigned long long tab[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t row_pairs = g.square ? (uint64_t)g.n_cols - i - 1 : (uint64_t)g.n_cols;
    const uint64_t b0 = (uint64_t)blockIdx.x * kGrpBlockPairs;
    if (b0 >= row_pairs)
        return;   // (whole workgroups)
    const uint32_t G = s.g_cols;
    for (uint32_t k = threadIdx.x; k < G; k += 256) {
        tab[k] = 0;
        tab[G + k] = 0;
        tab[2 * G + k] = 0;
        tab[3 * G + k] = ~0ull;
        tab[4 * G + k] = 0;
    }
    __syncthreads();
    const uint64_t base = g.square ? tri_row_start(g.n_cols, i) - g.out_base : (uint64_t)(i - g.rb) * g.n_cols;
    const uint64_t j0 = g.square ? (uint64_t)i + 1 : 0;   // the column record of the row's entry 0
    const uint64_t q0 = b0 + (uint32_t)wave * kGrpWavePairs;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint64_t v[kGrpSteps];
    uint32_t grp[kGrpSteps];
    uint32_t todo = 0;   // bit t: entry t of this lane has a group and is not yet in the table
#pragma unroll
    for (int t = 0; t < kGrpSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        const bool valid = q < row_pairs;
        v[t] = valid ? __builtin_nontemporal_load(slab + base + q) : 0;
        grp[t] = valid ? s.col_group[j0 + q] : DST_GROUP_NONE;
        todo |= (grp[t] != DST_GROUP_NONE ? 1u : 0u) << t;
    }
    if constexpr (AGG) {
#pragma unroll 1
        for (int r = 0; r < kGroupAggRounds; ++r) {
            const unsigned long long left = __ballot(todo != 0);
            if (!left)
                break;   // (uniform)
            const int leader = __ffsll(left) - 1;
            uint32_t mine = DST_GROUP_NONE;
#pragma unroll
            for (int t = kGrpSteps - 1; t >= 0; --t)
                mine = (todo >> t & 1u) ? grp[t] : mine;
            const uint32_t b = (uint32_t)__shfl((int)mine, leader, 64);
            GroupAcc x = group_acc_zero();
#pragma unroll
            for (int t = 0; t < kGrpSteps; ++t)
                if ((todo >> t & 1u) && grp[t] == b) {
                    add_entry<INT>(x, v[t], t_key, any != 0);
                    todo &= ~(1u << t);
                }
            wave_sum(x.a);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                x.nan += (uint32_t)__shfl_down((int)x.nan, off, 64);
                x.kmin = min(x.kmin, shfl_down64(x.kmin, off));
                x.kmax = max(x.kmax, shfl_down64(x.kmax, off));
            }
            if (lane == 0)
                table_add(tab, G, b, x);
        }
    }
#pragma unroll
    for (int t = 0; t < kGrpSteps; ++t)
        if (todo >> t & 1u) {
            GroupAcc x = group_acc_zero();
            add_entry<INT>(x, v[t], t_key, any != 0);
            table_add(tab, G, grp[t], x);
        }
    __syncthreads();
    const uint32_t a = s.row_group[i];
    for (uint32_t k = threadIdx.x; k < G; k += 256) {
        const unsigned long long c = tab[k], kmin = tab[3 * G + k], kmax = tab[4 * G + k];
        Acc acc;
        acc.summable = (uint32_t)(c & 0xFFFFFFu);
        acc.within = (uint32_t)(c >> 24 & 0xFFFFFFu);
        acc.hi = (long long)tab[G + k];
        acc.lo = tab[2 * G + k];
        add_to_entry(s, (uint64_t)i * G + k, acc);
        if (a == DST_GROUP_NONE)
            continue;
        const uint64_t cell = (uint64_t)a * G + k;
        const unsigned long long nans = c >> 48;
        if (nans)
            __hip_atomic_fetch_add(s.cell + cell, nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (kmin != ~0ull)
            __hip_atomic_fetch_min(s.cell + 5 * s.cells + cell, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (kmax != 0)
            __hip_atomic_fetch_max(s.cell + 6 * s.cells + cell, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The column side of the square: thread j = blockIdx.x * 256 + threadIdx.x takes the rows i < j of segment seg0 +
// blockIdx.y (rows rb + kGroupSegRows seg .. + kGroupSegRows - 1, below re), in order of the rows' groups (rows without a
// group last, and not walked).
template <bool INT>
__global__ __launch_bounds__(256) void group_cols_kernel(const uint64_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                         uint32_t rb, uint32_t re, uint32_t seg0, uint64_t t_bits, int any,
                                                         GroupState s)
{
    __shared__ uint32_t seg_grp[kGroupSegRows], ord_row[kGroupSegRows], ord_grp[kGroupSegRows];
    const uint64_t first = (uint64_t)rb + (uint64_t)(seg0 + blockIdx.y) * kGroupSegRows;
    if (first >= re)
        return;   // (whole workgroups)
    const uint32_t i0 = (uint32_t)first, i1 = (uint32_t)min((uint64_t)re, first + kGroupSegRows);
    if ((uint64_t)blockIdx.x * 256 + 255 <= i0)
        return;   // (whole workgroups: no row of the segment lies before any of these columns)
    const uint32_t rows = i1 - i0;
    if (threadIdx.x < kGroupSegRows)
        seg_grp[threadIdx.x] = threadIdx.x < rows ? s.row_group[i0 + threadIdx.x] : DST_GROUP_NONE;
    __syncthreads();
    if (threadIdx.x < rows) {
        const uint32_t mine = seg_grp[threadIdx.x];
        uint32_t rank = 0;
        for (uint32_t u = 0; u < rows; ++u) {
            const uint32_t other = seg_grp[u];
            rank += (other < mine || (other == mine && u < threadIdx.x)) ? 1u : 0u;
        }
        ord_row[rank] = i0 + threadIdx.x;
        ord_grp[rank] = mine;
    }
    __syncthreads();
    const uint64_t j64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j64 >= n || j64 <= i0)
        return;
    const uint32_t j = (uint32_t)j64, G = s.g_cols;
    const uint64_t t_key = nn_key<INT>(t_bits);
    Acc a{};
    uint32_t cur = DST_GROUP_NONE;
    for (uint32_t k = 0; k < rows; ++k) {
        const uint32_t gi = ord_grp[k];   // (uniform)
        if (gi == DST_GROUP_NONE)
            break;
        if (gi != cur) {
            if (cur != DST_GROUP_NONE)
                add_to_entry(s, (uint64_t)j * G + cur, a);
            a = Acc{};
            cur = gi;
        }
        const uint32_t i = ord_row[k];
        if (i < j) {
            const uint64_t at = tri_row_start(n, i) - out_base + (j - i - 1);
            add_pair<INT>(a, __builtin_nontemporal_load(slab + at), t_key, any != 0);
        }
    }
    if (cur != DST_GROUP_NONE)
        add_to_entry(s, (uint64_t)j * G + cur, a);
}

static_assert(kStreamGroupRows <= kStreamGroupCols && kStreamGroupCols == 256, "a thread per column, and one per row to rank");
constexpr int kStreamGroupUnroll = 8;   // rows whose loads a thread has in flight at once

// A group-summary stream's batch, the loaded side: the n_rows x n_cols matrix (row = streamed record, column = loaded
// record), tile (tile0 + blockIdx.y, blockIdx.x).  s.row_group: the batch's labels; s.counts / hi / lo: the kept table
// [G][n_cols], G = s.g_cols the STREAMED group count.  Rows without a group rank last and are not walked.
template <bool INT>
__global__ __launch_bounds__(256) void group_stream_cols_kernel(const uint64_t *__restrict__ matrix, uint32_t n_rows, uint32_t n_cols,
                                                                uint32_t tile0, uint64_t t_bits, int any, GroupState s)
{
    __shared__ uint32_t seg_grp[kStreamGroupRows], ord_row[kStreamGroupRows], ord_grp[kStreamGroupRows];
    const uint64_t first = (uint64_t)(tile0 + blockIdx.y) * kStreamGroupRows;
    if (first >= n_rows)
        return;   // (whole workgroups)
    const uint32_t r0 = (uint32_t)first, rows = min(kStreamGroupRows, n_rows - r0);
    if (threadIdx.x < kStreamGroupRows)
        seg_grp[threadIdx.x] = threadIdx.x < rows ? s.row_group[r0 + threadIdx.x] : DST_GROUP_NONE;
    __syncthreads();
    if (threadIdx.x < kStreamGroupRows) {   // (every slot of the order is written: the rows past the batch rank last)
        const uint32_t mine = seg_grp[threadIdx.x];
        uint32_t rank = 0;
        for (uint32_t u = 0; u < kStreamGroupRows; ++u) {
            const uint32_t other = seg_grp[u];
            rank += (other < mine || (other == mine && u < threadIdx.x)) ? 1u : 0u;
        }
        ord_row[rank] = threadIdx.x;
        ord_grp[rank] = mine;
    }
    __syncthreads();
    const uint64_t j64 = (uint64_t)blockIdx.x * kStreamGroupCols + threadIdx.x;
    if (j64 >= n_cols)
        return;
    const uint64_t t_key = nn_key<INT>(t_bits);
    const uint64_t *p = matrix + (uint64_t)r0 * n_cols + j64;
    Acc a{};
    uint32_t cur = DST_GROUP_NONE;
    for (uint32_t k = 0; k < kStreamGroupRows; k += kStreamGroupUnroll) {   // (uniform)
        if (ord_grp[k] == DST_GROUP_NONE)
            break;
        uint64_t v[kStreamGroupUnroll];
#pragma unroll
        for (int u = 0; u < kStreamGroupUnroll; ++u)   // (a row with a group lies inside the batch)
            v[u] = ord_grp[k + u] != DST_GROUP_NONE ? __builtin_nontemporal_load(p + (uint64_t)ord_row[k + u] * n_cols) : 0;
#pragma unroll
        for (int u = 0; u < kStreamGroupUnroll; ++u) {
            const uint32_t gi = ord_grp[k + u];   // (uniform)
            if (gi == DST_GROUP_NONE)
                break;
            if (gi != cur) {
                if (cur != DST_GROUP_NONE)
                    add_to_entry(s, (uint64_t)cur * n_cols + j64, a);
                a = Acc{};
                cur = gi;
            }
            add_pair<INT>(a, v[u], t_key, any != 0);
        }
    }
    if (cur != DST_GROUP_NONE)
        add_to_entry(s, (uint64_t)cur * n_cols + j64, a);
}

// one record's entry added to 128-bit running words (high, low) of a thread: S = hi 2^32 + lo as a 128-bit integer
struct Wide {
    unsigned long long links, summable;
    long long high;
    unsigned long long low;
};

__device__ __forceinline__ void wide_flush(const GroupState &s, uint64_t cell, const Wide &w)
{
    if (w.links)
        __hip_atomic_fetch_add(s.cell + 1 * s.cells + cell, w.links, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w.summable)
        __hip_atomic_fetch_add(s.cell + 2 * s.cells + cell, w.summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the two words of the cell's 128-bit sum: the carry of the low word's add from the value the atomic returns, every
    // carry added once (summary_hist_kernel's totals)
    long long high = w.high;
    if (w.low) {
        const unsigned long long old =
            __hip_atomic_fetch_add(s.cell + 4 * s.cells + cell, w.low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        high += old + w.low < old ? 1 : 0;
    }
    if (high)
        __hip_atomic_fetch_add(s.cell + 3 * s.cells + cell, (unsigned long long)high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread g = blockIdx.y * 256 + threadIdx.x (below g_cols) takes records order[kGroupFoldRecs blockIdx.x ..] (below
// `assigned`): the records that have a group, sorted by it.
__global__ __launch_bounds__(256) void group_fold_kernel(GroupState s, uint32_t assigned)
{
    const uint32_t g = blockIdx.y * 256 + threadIdx.x, G = s.g_cols;
    if (g >= G)
        return;
    const uint64_t k0 = (uint64_t)blockIdx.x * kGroupFoldRecs, k1 = min((uint64_t)assigned, k0 + kGroupFoldRecs);
    Wide w{};
    uint32_t cur = DST_GROUP_NONE;
    for (uint64_t k = k0; k < k1; ++k) {
        const uint32_t x = s.order[k], a = s.row_group[x];   // (uniform)
        if (a != cur) {
            if (cur != DST_GROUP_NONE)
                wide_flush(s, (uint64_t)cur * G + g, w);
            w = Wide{};
            cur = a;
        }
        const uint64_t at = (uint64_t)x * G + g;
        const unsigned long long c = s.counts[at], lo = s.lo[at];
        const long long hi = s.hi[at];
        w.links += c >> 32;
        w.summable += c & 0xFFFFFFFFull;
        // + hi 2^32 + lo in 128 bits
        const unsigned long long shifted = (unsigned long long)hi << 32, add = shifted + lo;
        const long long add_high = (hi >> 32) + (add < shifted ? 1 : 0);
        const unsigned long long before = w.low;
        w.low += add;
        w.high += add_high + (w.low < before ? 1 : 0);
    }
    if (cur != DST_GROUP_NONE)
        wide_flush(s, (uint64_t)cur * G + g, w);
}

GroupState state_of(const GroupBuffers &b)
{
    return GroupState{b.row_group,
                      b.col_group,
                      b.order,
                      reinterpret_cast<unsigned long long *>(b.counts),
                      reinterpret_cast<long long *>(b.hi),
                      reinterpret_cast<unsigned long long *>(b.lo),
                      reinterpret_cast<unsigned long long *>(b.cell),
                      (uint64_t)b.g_rows * b.g_cols,
                      b.g_cols};
}

}  // namespace

hipError_t launch_group_rows(int measure, bool square, const uint64_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                             uint64_t re, uint64_t t_bits, bool any, bool aggregate, const GroupBuffers &b, hipStream_t stream)
{
    const uint64_t longest = square ? (n_cols > rb + 1 ? n_cols - rb - 1 : 0) : n_cols;   // of row rb
    if (re <= rb || longest == 0)
        return hipSuccess;
    if (b.g_cols == 0 || b.g_cols > DST_GROUPS_MAX)
        return hipErrorInvalidValue;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const GroupRows g{out_base, (uint32_t)n_cols, (uint32_t)rb, (uint32_t)re, square ? 1 : 0};
    const unsigned chunks = (unsigned)((longest + kGrpBlockPairs - 1) / kGrpBlockPairs);
    const size_t lds = (size_t)b.g_cols * kGrpLdsWords * sizeof(unsigned long long);
    const GroupState s = state_of(b);
    return for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
        const dim3 grid(chunks, rows);
#define DST_GROUP_ROWS(INT, AGG)                                                                                               \
    hipLaunchKernelGGL((group_rows_kernel<INT, AGG>), grid, dim3(256), lds, stream, slab, g, (uint32_t)row0, t_bits,           \
                       any ? 1 : 0, s)
        if (int_payload) {
            if (aggregate)
                DST_GROUP_ROWS(true, true);
            else
                DST_GROUP_ROWS(true, false);
        } else {
            if (aggregate)
                DST_GROUP_ROWS(false, true);
            else
                DST_GROUP_ROWS(false, false);
        }
#undef DST_GROUP_ROWS
        return hipGetLastError();
    });
}

hipError_t launch_group_cols(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             uint64_t t_bits, bool any, const GroupBuffers &b, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const uint64_t segs = (re - rb + kGroupSegRows - 1) / kGroupSegRows;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const GroupState s = state_of(b);
    for (uint64_t seg0 = 0; seg0 < segs; seg0 += kGridRowsMax) {
        const dim3 grid(blocks, grid_rows(segs - seg0));
        if (int_payload)
            hipLaunchKernelGGL(group_cols_kernel<true>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n, (uint32_t)rb,
                               (uint32_t)re, (uint32_t)seg0, t_bits, any ? 1 : 0, s);
        else
            hipLaunchKernelGGL(group_cols_kernel<false>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n, (uint32_t)rb,
                               (uint32_t)re, (uint32_t)seg0, t_bits, any ? 1 : 0, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t launch_group_stream_cols(int measure, const uint64_t *matrix, uint64_t n_records, uint64_t n_loaded, uint64_t t_bits,
                                    bool any, const GroupBuffers &b, hipStream_t stream)
{
    if (n_records == 0 || n_loaded == 0)
        return hipSuccess;
    if (n_records > 0xFFFFFFFFull || n_loaded > 0xFFFFFFFFull || b.g_cols == 0 || b.g_cols > DST_GROUPS_MAX)
        return hipErrorInvalidValue;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const unsigned col_tiles = (unsigned)((n_loaded + kStreamGroupCols - 1) / kStreamGroupCols);
    const uint64_t row_tiles = (n_records + kStreamGroupRows - 1) / kStreamGroupRows;
    const GroupState s = state_of(b);
    return for_row_grids(0, row_tiles, [&](uint64_t tile0, unsigned tiles) {
        const dim3 grid(col_tiles, tiles);
        if (int_payload)
            hipLaunchKernelGGL(group_stream_cols_kernel<true>, grid, dim3(256), 0, stream, matrix, (uint32_t)n_records,
                               (uint32_t)n_loaded, (uint32_t)tile0, t_bits, any ? 1 : 0, s);
        else
            hipLaunchKernelGGL(group_stream_cols_kernel<false>, grid, dim3(256), 0, stream, matrix, (uint32_t)n_records,
                               (uint32_t)n_loaded, (uint32_t)tile0, t_bits, any ? 1 : 0, s);
        return hipGetLastError();
    });
}

hipError_t launch_group_fold(const GroupBuffers &b, uint64_t assigned, hipStream_t stream)
{
    if (assigned == 0)
        return hipSuccess;
    const dim3 grid((unsigned)((assigned + kGroupFoldRecs - 1) / kGroupFoldRecs), (b.g_cols + 255) / 256);
    hipLaunchKernelGGL(group_fold_kernel, grid, dim3(256), 0, stream, state_of(b), (uint32_t)assigned);
    return hipGetLastError();
}

}  // namespace dst
