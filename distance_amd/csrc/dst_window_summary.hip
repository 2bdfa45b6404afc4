// dst_window_summary.hip — dst_summary's counts and sums per column window (dst_window_summary): the window
// sweep of dst_windows.hip with the reduction fused into its epilogue, so that no tally and no payload leaves the chip.
//
// Mapping (window_summary_kernel): window_pair_kernel's.  One block = kWinRows row records x 256 column records x ONE
// window; grid.x walks the column tiles, grid.y the row tiles, grid.z the windows (y and z cut by for_row_grids); the
// lanes run along the column records and the row operands are wave-uniform.  The sweep is dst_window_sweep.hpp's.
//
// Epilogue.  The lane's tallies (M::tallies with total = end - begin) go through the lane-private LDS stage, and ONE copy
// of the finalisation runs in a rolled loop over the tile's rows, exactly as window_pair_kernel stores its payloads: the
// payload is that kernel's by construction.  Per pair the loop forms dst_pair_sum.hpp's Acc (link, summable, q in its two
// halves) and a NaN flag, and reduces
//   row side      over the wave with shuffles (the three counts of a wave are at most 64 each and ride above the low
//                 halves' sum in one 64-bit word; the high halves are skipped while the whole wave's are zero: counts of
//                 sites always, f64 distances below 2^-5), over the four waves through LDS, then ONE set of
//                 integer agent-scope relaxed atomics per (row, window, block), none of a value that is zero;
//   column side   (the triangle of a square, when a per-record array is wanted) in the lane's registers over the tile's
//                 rows, then the lane's atomics to (window, j): the state is window-major, so the lanes of a wave add to
//                 adjacent words;
//   totals        the eight row sums of the block over eight lanes, then the window's five words: NaN pairs, summable
//                 pairs, links and the sum as a 128-bit integer in two words, with dst_summary's carry rule.
// Every accumulation across blocks is an integer atomic: the result is exact whatever the order.
//
// mode kWinSumFull sweeps the full square (every row against all j != i, as dst_nearest_windows does) and keeps the row
// side only: every pair is met twice, so the window's links, summable pairs and sum come out doubled (the host halves
// them) and the NaN pairs are counted where j > i.  It is the measured alternative to the column side.
#include "dst_ctx.h"
#include "dst_device.hpp"
#include "dst_measures.hpp"
#include "dst_pair_sum.hpp"
#include "dst_window_sweep.hpp"

namespace dst {
namespace {

constexpr int kWinWaves = kWinCols / 64;
// where a pair's NaN flag, summable flag and link flag ride in the word of its low half (q & 0xFFFFFFFF) through the wave's
// shuffles: seven bits each above the 40 that the sum of 64 low halves cannot reach
constexpr int kNanAt = 40, kSummableAt = 47, kWithinAt = 54;

struct WinSumState {
    uint32_t *within, *summable;   // [n_windows][n_rows], or all four NULL: no per-record result
    long long *hi;
    unsigned long long *lo;
    unsigned long long *tot;       // [n_windows][kWindowSummaryTotals]
};

__device__ __forceinline__ void add_to_entry(const WinSumState &s, uint64_t at, const Acc &a)
{
    if (a.within)
        __hip_atomic_fetch_add(s.within + at, a.within, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.summable)
        __hip_atomic_fetch_add(s.summable + at, a.summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.hi)
        __hip_atomic_fetch_add(s.hi + at, a.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.lo)
        __hip_atomic_fetch_add(s.lo + at, a.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// OUT: OUT_INT, or the measure id whose f64 payload the epilogue reduces (as window_pair_kernel)
template <class M, int OUT>
__global__ __launch_bounds__(kWinCols) void window_summary_kernel(
    const uint4 *__restrict__ qpl, const uint4 *__restrict__ tpl, const uint2 *__restrict__ windows,
    const uint4 *__restrict__ q_counts, const uint4 *__restrict__ t_counts, uint32_t nchunks, uint32_t q_npad, uint32_t t_npad,
    uint32_t q_n, uint32_t n_cols, uint32_t row0, uint32_t win0, uint64_t t_bits, int any, int mode, WinSumState s)
{
    constexpr int NC = M::NC, NT = M::NT;
    constexpr bool INT = OUT == OUT_INT;
    __shared__ uint32_t stage[kWinRows * NT * kWinCols];
    __shared__ unsigned long long red[kWinWaves][kWinRows][2];   // per wave and row: the low halves with the counts, hi

    const uint32_t row_end = q_n;
    const uint32_t i0 = row0 + blockIdx.y * kWinRows;   // (< row_end by the grid)
    const uint32_t j0 = blockIdx.x * kWinCols;
    if (mode == kWinSumTriangle && j0 + (kWinCols - 1) <= i0)
        return;   // every column of the tile is at or below its first row: no pair j > i
    const uint32_t w = win0 + blockIdx.z;
    const uint2 win = windows[w];
    const uint32_t wb = win.x, we = win.y;
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t jl = j < n_cols ? j : n_cols - 1;   // a lane past the last column reads the last one and counts nothing

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

    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const bool rec = s.within != nullptr;
    const uint64_t t_key = nn_key<INT>(t_bits);
    const uint64_t state_row = (uint64_t)w * q_n;   // the window's per-record entries
    Acc col{};
#pragma unroll 1
    for (int r = 0; r < kWinRows; ++r) {
        const uint32_t i = i0 + r;
        const bool valid = i < row_end && j < n_cols && (mode == kWinSumRect || (mode == kWinSumTriangle ? j > i : j != i));
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
            nan = is_nan<INT>(bits) && (mode != kWinSumFull || j > i) ? 1u : 0u;
        }
        col.within += a.within;
        col.summable += a.summable;
        col.hi += a.hi;
        col.lo += a.lo;
        // the row's sums over the wave
        // one word for the low halves and the three counts: a wave's low halves sum below 2^38, its counts are at most 64
        unsigned long long low = a.lo | (unsigned long long)nan << kNanAt | (unsigned long long)a.summable << kSummableAt |
                                 (unsigned long long)a.within << kWithinAt;
        unsigned long long hi = (unsigned long long)a.hi;
        const bool any_hi = __ballot(a.hi != 0) != 0;   // (wave-uniform)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            low += shfl_down64(low, off);
        if (any_hi) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1)
                hi += shfl_down64(hi, off);
        }
        if (lane == 0) {
            red[wave][r][0] = low;
            red[wave][r][1] = hi;
        }
    }
    if (rec && mode == kWinSumTriangle && j < n_cols)
        add_to_entry(s, state_row + j, col);
    __syncthreads();
    if (wave != 0)
        return;
    // lane r < kWinRows: row i0 + r of the block; then the block's sums over those lanes
    Acc row{};
    uint32_t nans = 0;
    if (lane < kWinRows) {
        unsigned long long hi = 0;
#pragma unroll
        for (int v = 0; v < kWinWaves; ++v) {
            const unsigned long long low = red[v][lane][0];
            row.within += (uint32_t)(low >> kWithinAt) & 127u;
            row.summable += (uint32_t)(low >> kSummableAt) & 127u;
            nans += (uint32_t)(low >> kNanAt) & 127u;
            row.lo += low & ((1ull << kNanAt) - 1);
            hi += red[v][lane][1];
        }
        row.hi = (long long)hi;
        if (rec && i0 + (uint32_t)lane < row_end)
            add_to_entry(s, state_row + i0 + (uint32_t)lane, row);
    }
    uint32_t counts_a = row.within << 16 | row.summable;   // (each at most 256 per row: 2,048 per block)
    unsigned long long hi = (unsigned long long)row.hi, lo = row.lo;
#pragma unroll
    for (int off = kWinRows / 2; off > 0; off >>= 1) {
        counts_a += (uint32_t)__shfl_down((int)counts_a, off, 64);
        nans += (uint32_t)__shfl_down((int)nans, off, 64);
        hi += shfl_down64(hi, off);
        lo += shfl_down64(lo, off);
    }
    if (lane != 0)
        return;
    unsigned long long *tot = s.tot + (uint64_t)w * kWindowSummaryTotals;
    const uint32_t links = counts_a >> 16, summable = counts_a & 0xFFFFu;
    if (nans)
        __hip_atomic_fetch_add(tot + 0, (unsigned long long)nans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (summable)
        __hip_atomic_fetch_add(tot + 1, (unsigned long long)summable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (links)
        __hip_atomic_fetch_add(tot + 2, (unsigned long long)links, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the block's exact sum hi 2^32 + lo as a 128-bit integer in two words, the carry of the low word's add taken from the
    // value the atomic returns (summary_hist_kernel's rule: every carry is added once, whatever the order)
    const long long bhi = (long long)hi;
    const unsigned long long shifted = (unsigned long long)bhi << 32, low = shifted + lo;
    long long high = (bhi >> 32) + (low < shifted ? 1 : 0);
    if (low) {
        const unsigned long long old = __hip_atomic_fetch_add(tot + 4, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        high += old + low < old ? 1 : 0;
    }
    if (high)
        __hip_atomic_fetch_add(tot + 3, (unsigned long long)high, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class M, int OUT>
hipError_t launch_summary_one(const WindowSummaryLaunch &wl, hipStream_t stream)
{
    const uint64_t row_tiles = (wl.rows->n + kWinRows - 1) / kWinRows;
    const unsigned col_tiles = (unsigned)((wl.cols->n + kWinCols - 1) / kWinCols);
    const WinSumState s{wl.within, wl.summable, reinterpret_cast<long long *>(wl.hi), reinterpret_cast<unsigned long long *>(wl.lo),
                        reinterpret_cast<unsigned long long *>(wl.tot)};
    // windows and row tiles each in grids of at most 65,535
    return for_row_grids(0, wl.n_windows, [&](uint64_t win0, unsigned nwin) {
        return for_row_grids(0, row_tiles, [&](uint64_t tile0, unsigned ntiles) {
            hipLaunchKernelGGL((window_summary_kernel<M, OUT>), dim3(col_tiles, ntiles, nwin), dim3(kWinCols), 0, stream,
                               wl.rows->planes, wl.cols->planes, wl.d_windows, wl.q_counts, wl.t_counts, (uint32_t)wl.rows->nchunks,
                               (uint32_t)wl.rows->npad, (uint32_t)wl.cols->npad, (uint32_t)wl.rows->n, (uint32_t)wl.cols->n,
                               (uint32_t)(tile0 * kWinRows), (uint32_t)win0, wl.t_bits, wl.any ? 1 : 0, wl.mode, s);
            return hipGetLastError();
        });
    });
}

}  // namespace

hipError_t launch_window_summary(int measure, const WindowSummaryLaunch &wl, hipStream_t stream)
{
    if (wl.n_windows == 0 || wl.n_windows > DST_WINDOWS_MAX || wl.rows->n == 0 || wl.cols->n == 0 || wl.rows->n >= 0xFFFFFFFFull ||
        wl.cols->n >= 0xFFFFFFFFull || wl.rows->nchunks != wl.cols->nchunks || wl.rows->len != wl.cols->len ||
        wl.rows->len > 0xFFFFFFFFull || !wl.tot || wl.mode < kWinSumRect || wl.mode > kWinSumFull ||
        (wl.mode != kWinSumRect && wl.rows != wl.cols) || (wl.within && (!wl.summable || !wl.hi || !wl.lo)) ||
        (wl.within && wl.rows->n * wl.n_windows > ((uint64_t)1 << 31)) || (wl.mode == kWinSumFull && !wl.within))
        return hipErrorInvalidValue;
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: return launch_summary_one<MNHigh, OUT_INT>(wl, stream);
    case DST_RAW: return launch_summary_one<MRaw, DST_RAW>(wl, stream);
    case DST_JC69: return launch_summary_one<MRaw, DST_JC69>(wl, stream);
    case DST_K80: return launch_summary_one<MK80, DST_K80>(wl, stream);
    case DST_TN93: return launch_summary_one<MTN93, DST_TN93>(wl, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace dst
