// dst_window_group_summary.hip — dst_group_summary's cells and per-record tables inside every column window
// (dst_window_group_summary): the window sweep with the by-group reduction fused into its epilogue, so that
// no tally and no payload leaves the chip and the state is n_windows x G_r x G_c cells whatever the record count.
//
// Mapping, sweep and payload (window_group_kernel): window_summary_kernel's, unchanged.  One block = kWinRows row records x
// 256 column records x ONE window; window_sweep<M>, M::tallies, the lane-private LDS stage, then ONE rolled loop over the
// tile's rows calling finalize_pair<OUT> with the per-window counts: the payload is window_pair_kernel's by construction.
//
// Reduction.  The row's group a is uniform over the block and lane j carries g = col_group[j], loaded once.  The column
// groups do not change from row to row, so each wave plans its leader rounds ONCE: up to kWgRounds times the first lane
// not yet placed names its group and every lane of that group joins the round; lanes left over are "single".  A wave
// whose 64 columns share one group has one round and no singles (the common case of a file sorted by lineage).  Per row
//   a round    sums its lanes by shuffles (the three counts ride above the low halves' sum in one word, the high halves are
//              skipped while the wave's are all zero) and lane 0 adds ONCE to the workgroup's table in LDS;
//   a single   adds its own pair to the table entry by entry.
// The smallest and the largest key belong to a cell, not to a record: a lane carries them in registers over consecutive rows
// of one group and they take their shuffles and their table entry once per such run (once per tile for a file sorted by
// lineage).
// The table holds five 64-bit words per (row of the batch, column group): the three counts packed into one, hi, lo, min
// key, max key: kWgSlots = 256 slots, 10 KB beside tn93's 32 KB stage.  A batch is as many rows as fit: all eight up to 32
// column groups, one row at 256.  After a batch the thread of slot (row, g) flushes what is not empty with integer
// agent-scope relaxed atomics: to rec[(w, i, g)] when the per-record arrays are wanted, and, from the first row of each
// group in the batch (which first adds the batch's later rows of that group), to cell (w, a, g): NaN pairs, links,
// summable pairs, the 128-bit sum with the carry rule, atomic min / max of the key.  Every accumulation across blocks is
// an integer atomic: the result is exact whatever the order.
//
// Square.  Cells alone: the triangle, each pair i < j once at (g_i, g_j); the host adds the mirror cell.  With per-record
// arrays: the full square with the row side only (window_summary_kernel's kWinSumFull): row i meets every j != i, so
// rec[(w, i, g)] is complete from the row side, cell (a, b != a) holds each of its pairs once and cell (a, a) each twice
// (the host halves it).  tn93's counts of a pair met as (i, j < i) are swapped, so the payload is the canonical pair's.
#include "dst_ctx.h"
#include "dst_device.hpp"
#include "dst_measures.hpp"
#include "dst_pair_sum.hpp"
#include "dst_window_sweep.hpp"

namespace dst {
namespace {

constexpr int kWgRounds = 3;                  // leader rounds of a wave
constexpr int kWgSingle = kWgRounds;          // a lane whose group took no round
constexpr int kWgIdle = kWgRounds + 1;        // a lane without a column, or whose column has no group
constexpr uint32_t kWgSlots = 256;            // table slots: (row of the batch, column group)
constexpr int kWgWords = 5;                   // counts, hi, lo, min key, max key
// where the NaN, summable and link counts of a wave (at most 64 each) ride above the sum of its low halves (below 2^38)
constexpr int kWgNanAt = 40, kWgSummableAt = 47, kWgWithinAt = 54;
static_assert(DST_WINDOW_GROUPS_MAX <= kWgSlots, "one row of the table holds every column group");

struct WinGroupState {
    const uint32_t *row_group, *col_group;
    unsigned long long *rec_counts;   // [n_windows][n_rows][g_cols]: within << 32 | summable; NULL: no per-record result
    long long *rec_hi;
    unsigned long long *rec_lo;
    unsigned long long *cell;         // [n_windows][g_rows][g_cols][kWindowGroupCellWords]
    uint32_t g_rows, g_cols;
};

// the table's counts word: NaN << 48 | within << 24 | summable (each at most 256 per row and block)
__device__ __forceinline__ void wg_table_add(unsigned long long *tab, uint32_t slot, unsigned long long counts, unsigned long long hi,
                                             unsigned long long lo, unsigned long long kmin, unsigned long long kmax)
{
    if (counts)
        __hip_atomic_fetch_add(tab + slot, counts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (hi)
        __hip_atomic_fetch_add(tab + kWgSlots + slot, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lo)
        __hip_atomic_fetch_add(tab + 2 * kWgSlots + slot, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (kmin != ~0ull)
        __hip_atomic_fetch_min(tab + 3 * kWgSlots + slot, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (kmax != 0)
        __hip_atomic_fetch_max(tab + 4 * kWgSlots + slot, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// OUT: OUT_INT, or the measure id whose f64 payload the epilogue reduces (as window_pair_kernel)
template <class M, int OUT>
__global__ __launch_bounds__(kWinCols) void window_group_kernel(
    const uint4 *__restrict__ qpl, const uint4 *__restrict__ tpl, const uint2 *__restrict__ windows,
    const uint4 *__restrict__ q_counts, const uint4 *__restrict__ t_counts, uint32_t nchunks, uint32_t q_npad, uint32_t t_npad,
    uint32_t q_n, uint32_t n_cols, uint32_t row0, uint32_t win0, uint64_t t_bits, int any, int mode, WinGroupState s)
{
    constexpr int NC = M::NC, NT = M::NT;
    constexpr bool INT = OUT == OUT_INT;
    __shared__ uint32_t stage[kWinRows * NT * kWinCols];
    __shared__ unsigned long long tab[kWgWords * kWgSlots];
    __shared__ uint32_t tile_grp[kWinRows + 1];   // (one more, without a group: the row after the tile's last)

    const uint32_t row_end = q_n;
    const uint32_t i0 = row0 + blockIdx.y * kWinRows;   // (< row_end by the grid)
    const uint32_t j0 = blockIdx.x * kWinCols;
    if (mode == kWinSumTriangle && j0 + (kWinCols - 1) <= i0)
        return;   // every column of the tile is at or below its first row: no pair j > i
    const uint32_t w = win0 + blockIdx.z;
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t jl = j < n_cols ? j : n_cols - 1;   // a lane past the last column reads the last one and counts nothing
    const uint32_t gj = j < n_cols ? s.col_group[j] : DST_GROUP_NONE;
    const bool rec = s.rec_counts != nullptr;
    const uint32_t G = s.g_cols;

    if (threadIdx.x <= kWinRows)
        tile_grp[threadIdx.x] =
            threadIdx.x < kWinRows && i0 + threadIdx.x < row_end ? s.row_group[i0 + threadIdx.x] : DST_GROUP_NONE;
    for (uint32_t k = threadIdx.x; k < kWgSlots; k += kWinCols) {
        tab[k] = 0;
        tab[kWgSlots + k] = 0;
        tab[2 * kWgSlots + k] = 0;
        tab[3 * kWgSlots + k] = ~0ull;
        tab[4 * kWgSlots + k] = 0;
    }
    // whole workgroups leave before the sweep: no column of the tile has a group, or the cells alone are wanted and no
    // row of the tile has one
    if (!__syncthreads_or(gj != DST_GROUP_NONE ? 1 : 0))
        return;
    if (!rec) {
        bool some = false;
#pragma unroll
        for (int r = 0; r < kWinRows; ++r)
            some = some || tile_grp[r] != DST_GROUP_NONE;
        if (!some)
            return;   // (uniform)
    }

    const uint2 win = windows[w];
    const uint32_t wb = win.x, we = win.y;

    uint32_t acc[kWinRows][NC];
#pragma unroll
    for (int r = 0; r < kWinRows; ++r)
#pragma unroll
        for (int k = 0; k < NC; ++k)
            acc[r][k] = 0;

    const size_t q_ps = (size_t)nchunks * q_npad, t_ps = (size_t)nchunks * t_npad;   // plane strides, in uint4
    const uint4 *qbase = qpl + (size_t)M::P0 * q_ps;
    const uint4 *tbase = tpl + (size_t)M::P0 * t_ps + jl;

    window_sweep<M>(acc, qbase, tbase, q_ps, t_ps, q_npad, t_npad, i0, row_end, wb, we);

    // the lane's tallies through its own LDS slots: no barrier
    const uint32_t total = we - wb;
#pragma unroll
    for (int r = 0; r < kWinRows; ++r) {
        uint32_t o[NT];
        M::tallies(acc[r], total, o);
#pragma unroll
        for (int k = 0; k < NT; ++k)
            stage[(r * NT + k) * kWinCols + threadIdx.x] = o[k];
    }

    // the wave's rounds, once for all the rows: my_round = the round this lane's group took, kWgSingle or kWgIdle
    const int lane = (int)(threadIdx.x & 63);
    int my_round = gj == DST_GROUP_NONE ? kWgIdle : kWgSingle;
    int n_rounds = 0;   // (wave-uniform)
#pragma unroll 1
    for (int k = 0; k < kWgRounds; ++k) {
        const unsigned long long left = __ballot(my_round == kWgSingle);
        if (!left)
            break;
        const uint32_t b = (uint32_t)__shfl((int)gj, __ffsll(left) - 1, 64);
        if (my_round == kWgSingle && gj == b)
            my_round = k;
        n_rounds = k + 1;
    }

    const uint32_t batch = G <= kWgSlots / kWinRows ? kWinRows : kWgSlots / G;   // rows per table: 8 up to 32 groups, .. 1
    const uint64_t t_key = nn_key<INT>(t_bits);
    // the smallest and the largest key belong to a cell, not to a record: the lane carries them over consecutive rows of one
    // group and the wave reduces them once per run
    unsigned long long kmin = ~0ull, kmax = 0;
#pragma unroll 1
    for (int r = 0; r < kWinRows; ++r) {
        const uint32_t i = i0 + r;
        const uint32_t in_batch = (uint32_t)r % batch;
        const uint32_t ga_r = tile_grp[r];   // (uniform)
        const bool batch_ends = in_batch + 1 == batch || r + 1 == kWinRows;
        const bool keys_now = ga_r != DST_GROUP_NONE && (batch_ends || tile_grp[r + 1] != ga_r);   // the run of ga_r ends here
        const bool valid = i < row_end && gj != DST_GROUP_NONE && (rec || tile_grp[r] != DST_GROUP_NONE) &&
                           (mode == kWinSumRect || (mode == kWinSumTriangle ? j > i : j != i));
        Acc a{};
        uint32_t nan = 0;
        if (valid) {
            uint32_t o[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k)
                o[k] = stage[(r * NT + k) * kWinCols + threadIdx.x];
            uint64_t bits;
            if constexpr (INT) {
                bits = (uint64_t)(int64_t)o[0];
            } else {
                uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
                if constexpr (OUT == DST_TN93) {
                    qc = q_counts[(uint64_t)w * q_n + i];
                    tc = t_counts[(uint64_t)w * n_cols + j];
                    if (mode == kWinSumFull && j < i) {   // the canonical pair (j, i): the counts in that order
                        const uint4 x = qc;
                        qc = tc;
                        tc = x;
                    }
                }
                bits = (uint64_t)__double_as_longlong(finalize_pair<OUT>(o, qc, tc));
            }
            add_pair<INT>(a, bits, t_key, any != 0);
            if (is_nan<INT>(bits)) {
                nan = 1;
            } else if (ga_r != DST_GROUP_NONE) {
                const unsigned long long key = nn_key<INT>(bits);
                kmin = min(kmin, key);
                kmax = max(kmax, key);
            }
        }
#pragma unroll 1
        for (int k = 0; k < n_rounds; ++k) {
            const bool in = my_round == k;
            unsigned long long low = in ? a.lo | (unsigned long long)nan << kWgNanAt | (unsigned long long)a.summable << kWgSummableAt |
                                              (unsigned long long)a.within << kWgWithinAt
                                        : 0;
            unsigned long long hi = in ? (unsigned long long)a.hi : 0, lo_key = in ? kmin : ~0ull, hi_key = in ? kmax : 0;
            const uint32_t b = (uint32_t)__shfl((int)gj, __ffsll(__ballot(in)) - 1, 64);
            const bool any_hi = __ballot(hi != 0) != 0;   // (wave-uniform)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                low += shfl_down64(low, off);
            if (keys_now) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    lo_key = min(lo_key, shfl_down64(lo_key, off));
                    hi_key = max(hi_key, shfl_down64(hi_key, off));
                }
            }
            if (any_hi) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
                    hi += shfl_down64(hi, off);
            }
            if (lane == 0) {
                const unsigned long long counts = (low >> kWgNanAt & 127ull) << 48 | (low >> kWgWithinAt & 127ull) << 24 |
                                                  (low >> kWgSummableAt & 127ull);
                wg_table_add(tab, in_batch * G + b, counts, hi, low & ((1ull << kWgNanAt) - 1), keys_now ? lo_key : ~0ull,
                             keys_now ? hi_key : 0);
            }
        }
        if (my_round == kWgSingle && (valid || keys_now))
            wg_table_add(tab, in_batch * G + gj, (unsigned long long)nan << 48 | (unsigned long long)a.within << 24 | a.summable,
                         (unsigned long long)a.hi, a.lo, keys_now ? kmin : ~0ull, keys_now ? kmax : 0);
        if (keys_now) {
            kmin = ~0ull;
            kmax = 0;
        }
        if (!batch_ends)
            continue;   // (uniform)
        // the batch's rows r - in_batch .. r: slot (x, g) of the table is this thread's
        __syncthreads();
        const uint32_t slot = threadIdx.x, x = slot / G, g = slot - x * G;
        if (x <= in_batch) {
            const int rr = r - (int)in_batch + (int)x;
            const uint32_t ii = i0 + (uint32_t)rr;
            const unsigned long long c = tab[slot];
            if (rec && ii < row_end) {
                const uint64_t at = ((uint64_t)w * q_n + ii) * G + g;
                const unsigned long long counts = (c >> 24 & 0xFFFFFFull) << 32 | (c & 0xFFFFFFull);
                const unsigned long long hi = tab[kWgSlots + slot], lo = tab[2 * kWgSlots + slot];
                if (counts)
                    __hip_atomic_fetch_add(s.rec_counts + at, counts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (hi)
                    __hip_atomic_fetch_add(s.rec_hi + at, (long long)hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lo)
                    __hip_atomic_fetch_add(s.rec_lo + at, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const uint32_t ga = tile_grp[rr];
            bool first = ga != DST_GROUP_NONE;   // the first row of group ga in the batch speaks for the later ones
            for (int e = rr - (int)x; e < rr; ++e)
                first = first && tile_grp[e] != ga;
            if (first) {
                unsigned long long counts = 0, hi = 0, lo = 0, lo_key = ~0ull, hi_key = 0;
                for (uint32_t y = x; y <= in_batch; ++y) {
                    if (tile_grp[rr + (int)(y - x)] != ga)
                        continue;
                    const uint32_t at = y * G + g;
                    counts += tab[at];   // (three fields of at most 2,048 each)
                    hi += tab[kWgSlots + at];
                    lo += tab[2 * kWgSlots + at];
                    lo_key = min(lo_key, tab[3 * kWgSlots + at]);
                    hi_key = max(hi_key, tab[4 * kWgSlots + at]);
                }
                unsigned long long *cell = s.cell + (((uint64_t)w * s.g_rows + ga) * G + g) * kWindowGroupCellWords;
                const unsigned long long nans = counts >> 48, links = counts >> 24 & 0xFFFFFFull, summable = counts & 0xFFFFFFull;
                if (nans)
                    __hip_atomic_fetch_add(cell + 0, nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (links)
                    __hip_atomic_fetch_add(cell + 1, links, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (summable)
                    __hip_atomic_fetch_add(cell + 2, summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // the exact sum hi 2^32 + lo as a 128-bit integer in two words, the carry of the low word's add taken from
                // the value the atomic returns (summary_hist_kernel's rule: every carry is added once, whatever the order)
                const long long bhi = (long long)hi;
                const unsigned long long shifted = (unsigned long long)bhi << 32, low = shifted + lo;
                long long high = (bhi >> 32) + (low < shifted ? 1 : 0);
                if (low) {
                    const unsigned long long old = __hip_atomic_fetch_add(cell + 4, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    high += old + low < old ? 1 : 0;
                }
                if (high)
                    __hip_atomic_fetch_add(cell + 3, (unsigned long long)high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lo_key != ~0ull)
                    __hip_atomic_fetch_min(cell + 5, lo_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (hi_key != 0)
                    __hip_atomic_fetch_max(cell + 6, hi_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (r + 1 == kWinRows)
            break;   // (uniform: the last batch, nothing reads the table again)
        __syncthreads();
        tab[slot] = 0;
        tab[kWgSlots + slot] = 0;
        tab[2 * kWgSlots + slot] = 0;
        tab[3 * kWgSlots + slot] = ~0ull;
        tab[4 * kWgSlots + slot] = 0;
        __syncthreads();
    }
}

template <class M, int OUT>
hipError_t launch_group_one(const WindowGroupLaunch &wl, hipStream_t stream)
{
    const uint64_t row_tiles = (wl.rows->n + kWinRows - 1) / kWinRows;
    const unsigned col_tiles = (unsigned)((wl.cols->n + kWinCols - 1) / kWinCols);
    const WinGroupState s{wl.row_group,
                          wl.col_group,
                          reinterpret_cast<unsigned long long *>(wl.rec_counts),
                          reinterpret_cast<long long *>(wl.rec_hi),
                          reinterpret_cast<unsigned long long *>(wl.rec_lo),
                          reinterpret_cast<unsigned long long *>(wl.cell),
                          wl.g_rows,
                          wl.g_cols};
    // windows and row tiles each in grids of at most 65,535
    return for_row_grids(0, wl.n_windows, [&](uint64_t win0, unsigned nwin) {
        return for_row_grids(0, row_tiles, [&](uint64_t tile0, unsigned ntiles) {
            hipLaunchKernelGGL((window_group_kernel<M, OUT>), dim3(col_tiles, ntiles, nwin), dim3(kWinCols), 0, stream,
                               wl.rows->planes, wl.cols->planes, wl.d_windows, wl.q_counts, wl.t_counts, (uint32_t)wl.rows->nchunks,
                               (uint32_t)wl.rows->npad, (uint32_t)wl.cols->npad, (uint32_t)wl.rows->n, (uint32_t)wl.cols->n,
                               (uint32_t)(tile0 * kWinRows), (uint32_t)win0, wl.t_bits, wl.any ? 1 : 0, wl.mode, s);
            return hipGetLastError();
        });
    });
}

// the cells' min keys to ~0 ("none yet"): the rest of the state is zero
__global__ __launch_bounds__(256) void window_group_init_kernel(unsigned long long *cell, uint64_t cells)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < cells)
        cell[c * kWindowGroupCellWords + 5] = ~0ull;
}

}  // namespace

hipError_t launch_window_group_init(uint64_t *cell, uint64_t cells, hipStream_t stream)
{
    if (cells == 0)
        return hipSuccess;
    if (!cell || cells > ((uint64_t)1 << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_group_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<unsigned long long *>(cell), cells);
    return hipGetLastError();
}

hipError_t launch_window_groups(int measure, const WindowGroupLaunch &wl, hipStream_t stream)
{
    const uint64_t one = 1;
    if (wl.n_windows == 0 || wl.n_windows > DST_WINDOWS_MAX || wl.rows->n == 0 || wl.cols->n == 0 || wl.rows->n >= 0xFFFFFFFFull ||
        wl.cols->n >= 0xFFFFFFFFull || wl.rows->nchunks != wl.cols->nchunks || wl.rows->len != wl.cols->len ||
        wl.rows->len > 0xFFFFFFFFull || !wl.cell || !wl.row_group || !wl.col_group || wl.mode < kWinSumRect || wl.mode > kWinSumFull ||
        (wl.mode != kWinSumRect && wl.rows != wl.cols) || wl.g_rows == 0 || wl.g_rows > DST_WINDOW_GROUPS_MAX || wl.g_cols == 0 ||
        wl.g_cols > DST_WINDOW_GROUPS_MAX || (wl.rec_counts && (!wl.rec_hi || !wl.rec_lo)) ||
        (uint64_t)wl.n_windows * wl.g_rows * wl.g_cols > (one << 31) ||
        (wl.rec_counts && (unsigned __int128)wl.rows->n * wl.n_windows * wl.g_cols > (one << 31)) ||
        (wl.mode == kWinSumFull && !wl.rec_counts))
        return hipErrorInvalidValue;
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: return launch_group_one<MNHigh, OUT_INT>(wl, stream);
    case DST_RAW: return launch_group_one<MRaw, DST_RAW>(wl, stream);
    case DST_JC69: return launch_group_one<MRaw, DST_JC69>(wl, stream);
    case DST_K80: return launch_group_one<MK80, DST_K80>(wl, stream);
    case DST_TN93: return launch_group_one<MTN93, DST_TN93>(wl, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace dst
