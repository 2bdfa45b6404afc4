// dst_windows.hip — distances per column window (dst_run_windows, dst_window_base_counts): the dense pair
// kernel's sweep (dst_kernels.hip) restricted to the 128-site chunks a window [begin, end) meets, with a site mask on
// the at most two chunks the window's edges cut.
// dst_nearest_windows is here too: it runs the same sweep slab by slab into the context's slab scratch and
// dst_window_nearest.hip's selection directly behind it.
//
// Mapping (window_pair_kernel): one block = kWinRows row records x 256 column records x ONE window.  grid.x walks the
// column tiles, grid.y the row tiles, grid.z the windows; y and z hold at most 65,535 each, so the launcher cuts both
// (for_row_grids).  The lanes run along the column records: a lane's 16 bytes of a (plane, chunk) are contiguous with its
// neighbours' (1 KiB per wave instruction), and stay in VGPRs for all the rows of the tile.  A row record's 16 bytes are
// the same for the whole block: wave-uniform loads, which reach the kernel as scalar loads and SGPR operands.
// Tallies live in VGPRs for the sweep; the epilogue is the dense kernel's (M::tallies, then the tally words, the int64, or
// finalize_pair).  Every entry has one writer: plain vector stores.
//
// The sweep itself, with its mask rule, is dst_window_sweep.hpp's: window_summary_kernel (dst_window_summary.hip) runs the
// same one.
#include "dst_ctx.h"
#include "dst_device.hpp"
#include "dst_measures.hpp"
#include "dst_window_sweep.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace dst {
namespace {

// OUT: OUT_TALLY, OUT_INT, or the measure id whose f64 the epilogue writes (as pair_kernel)
template <class M, int OUT>
__global__ __launch_bounds__(kWinCols) void window_pair_kernel(
    const uint4 *__restrict__ qpl, const uint4 *__restrict__ tpl, const uint2 *__restrict__ windows, void *__restrict__ out_v,
    const uint4 *__restrict__ q_counts, const uint4 *__restrict__ t_counts, uint32_t nchunks, uint32_t q_npad, uint32_t t_npad,
    uint32_t q_n, uint32_t n_cols, uint32_t row_begin, uint32_t row_end, uint32_t row0, uint32_t win0, uint32_t win_first,
    uint64_t pairs, uint64_t out_base, int square)
{
    constexpr int NC = M::NC, NT = M::NT;
    constexpr int STAGE_WORDS = OUT >= 0 ? kWinRows * NT * kWinCols : 1;
    __shared__ uint32_t stage[STAGE_WORDS];

    const uint32_t i0 = row0 + blockIdx.y * kWinRows;   // (< row_end by the grid)
    const uint32_t j0 = blockIdx.x * kWinCols;
    if (square && j0 + (kWinCols - 1) <= i0)
        return;   // every column of the tile is at or below its first row: no pair j > i
    const uint32_t w = win0 + blockIdx.z;
    const uint2 win = windows[w];
    const uint32_t wb = win.x, we = win.y;
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t jl = j < n_cols ? j : n_cols - 1;   // a lane past the last column reads the last one and stores nothing

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

    const uint32_t total = we - wb;
    const uint64_t win_at = (uint64_t)(w - win_first) * pairs;   // (the launch's first window lies at 0)
    if constexpr (OUT < 0) {
#pragma unroll
        for (int r = 0; r < kWinRows; ++r) {
            const uint32_t i = i0 + r;
            if (i >= row_end)
                break;
            if (j < n_cols && (!square || j > i)) {
                const uint64_t at = win_at + (square ? (tri_row_start(n_cols, i) - out_base) + (j - i - 1)
                                                     : (uint64_t)(i - row_begin) * n_cols + j);
                uint32_t o[NT];
                M::tallies(acc[r], total, o);
                if constexpr (OUT == OUT_INT) {
                    static_cast<int64_t *>(out_v)[at] = (int64_t)o[0];
                } else {
#pragma unroll
                    for (int k = 0; k < NT; ++k)
                        static_cast<uint32_t *>(out_v)[at * NT + k] = o[k];
                }
            }
        }
    } else {
        // the dense kernel's scheme: the lane's tallies go through a lane-private LDS slot, so that ONE copy of the
        // finalisation runs in a rolled loop.  A lane only touches its own column: no barrier.
#pragma unroll
        for (int r = 0; r < kWinRows; ++r) {
            uint32_t o[NT];
            M::tallies(acc[r], total, o);
#pragma unroll
            for (int k = 0; k < NT; ++k)
                stage[(r * NT + k) * kWinCols + threadIdx.x] = o[k];
        }
        double *out = static_cast<double *>(out_v);
#pragma unroll 1
        for (int r = 0; r < kWinRows; ++r) {
            const uint32_t i = i0 + r;
            if (i >= row_end)
                break;
            if (j < n_cols && (!square || j > i)) {
                uint32_t o[NT];
#pragma unroll
                for (int k = 0; k < NT; ++k)
                    o[k] = stage[(r * NT + k) * kWinCols + threadIdx.x];
                uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
                if constexpr (OUT == DST_TN93) {
                    qc = q_counts[(uint64_t)w * q_n + i];
                    tc = t_counts[(uint64_t)w * n_cols + j];
                }
                const uint64_t at = win_at + (square ? (tri_row_start(n_cols, i) - out_base) + (j - i - 1)
                                                     : (uint64_t)(i - row_begin) * n_cols + j);
                out[at] = finalize_pair<OUT>(o, qc, tc);
            }
        }
    }
}

// {A,T,G,C} counted by code (a known base is K & its own plane, K from the four base planes as counts_kernel takes it)
// inside every window: one thread per record (16 contiguous bytes per lane and plane), grid.y = the windows.
__global__ __launch_bounds__(256) void window_counts_kernel(const uint4 *__restrict__ planes, const uint2 *__restrict__ windows,
                                                            uint32_t n, uint32_t nchunks, uint32_t npad, uint32_t win0,
                                                            uint4 *__restrict__ counts)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const uint32_t w = win0 + blockIdx.y;
    if (s >= n)
        return;
    const uint2 win = windows[w];
    const uint32_t wb = win.x, we = win.y;
    const size_t ps = (size_t)nchunks * npad;
    uint32_t cnt[4] = {0, 0, 0, 0};   // A, T, G, C
    if (we > wb) {
        const uint32_t c_first = wb / kChunkSites, c_last = (we - 1u) / kChunkSites;
        for (uint32_t c = c_first; c <= c_last; ++c) {
            const size_t at = (size_t)c * npad + s;
            const uint4 A = planes[PL_A * ps + at], G = planes[PL_G * ps + at], C = planes[PL_C * ps + at], T = planes[PL_T * ps + at];
            uint32_t m[4];
            window_mask(c, wb, we, m);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = word_of(A, k), g = word_of(G, k), cc = word_of(C, k), t = word_of(T, k);
                const uint32_t K = (a ^ g ^ cc ^ t) & ~((a & g) | (cc & t)) & m[k];   // exactly one base, inside the window
                cnt[0] += (uint32_t)__builtin_popcount(K & a);
                cnt[1] += (uint32_t)__builtin_popcount(K & t);
                cnt[2] += (uint32_t)__builtin_popcount(K & g);
                cnt[3] += (uint32_t)__builtin_popcount(K & cc);
            }
        }
    }
    counts[(uint64_t)w * n + s] = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
}

template <class M, int OUT>
hipError_t launch_windows_one(const WindowLaunch &wl, hipStream_t stream)
{
    const uint64_t rows = wl.row_end - wl.row_begin;
    const uint64_t row_tiles = (rows + kWinRows - 1) / kWinRows;
    const unsigned col_tiles = (unsigned)((wl.cols->n + kWinCols - 1) / kWinCols);
    // windows and row tiles each in grids of at most 65,535
    return for_row_grids(wl.win_first, (uint64_t)wl.win_first + wl.n_windows, [&](uint64_t win0, unsigned nwin) {
        return for_row_grids(0, row_tiles, [&](uint64_t tile0, unsigned ntiles) {
            hipLaunchKernelGGL((window_pair_kernel<M, OUT>), dim3(col_tiles, ntiles, nwin), dim3(kWinCols), 0, stream,
                               wl.rows->planes, wl.cols->planes, wl.d_windows, wl.d_out, wl.q_counts, wl.t_counts,
                               (uint32_t)wl.rows->nchunks, (uint32_t)wl.rows->npad, (uint32_t)wl.cols->npad, (uint32_t)wl.rows->n,
                               (uint32_t)wl.cols->n, (uint32_t)wl.row_begin, (uint32_t)wl.row_end,
                               (uint32_t)(wl.row_begin + tile0 * kWinRows), (uint32_t)win0, wl.win_first, wl.pairs,
                               wl.square ? square_row_start(wl.cols->n, wl.row_begin) : (uint64_t)0, wl.square ? 1 : 0);
            return hipGetLastError();
        });
    });
}

}  // namespace

hipError_t launch_window_pairs(int measure, const WindowLaunch &wl, hipStream_t stream)
{
    if (wl.n_windows == 0 || (uint64_t)wl.win_first + wl.n_windows > DST_WINDOWS_MAX || wl.row_end <= wl.row_begin || wl.row_end > wl.rows->n ||
        wl.cols->n == 0 || wl.rows->n > 0xFFFFFFFFull || wl.cols->n > 0xFFFFFFFFull || wl.rows->nchunks != wl.cols->nchunks ||
        wl.rows->len != wl.cols->len || wl.rows->len > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const bool tally = wl.out_kind == DST_OUT_TALLY;
    switch (measure) {
    case DST_N:
    case DST_N_HIGH:
        return tally ? launch_windows_one<MNHigh, OUT_TALLY>(wl, stream) : launch_windows_one<MNHigh, OUT_INT>(wl, stream);
    case DST_RAW:
        return tally ? launch_windows_one<MRaw, OUT_TALLY>(wl, stream) : launch_windows_one<MRaw, DST_RAW>(wl, stream);
    case DST_JC69:
        return tally ? launch_windows_one<MRaw, OUT_TALLY>(wl, stream) : launch_windows_one<MRaw, DST_JC69>(wl, stream);
    case DST_K80:
        return tally ? launch_windows_one<MK80, OUT_TALLY>(wl, stream) : launch_windows_one<MK80, DST_K80>(wl, stream);
    case DST_TN93:
        return tally ? launch_windows_one<MTN93, OUT_TALLY>(wl, stream) : launch_windows_one<MTN93, DST_TN93>(wl, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_window_counts(const DeviceSet &set, const uint2 *d_windows, uint32_t n_windows, uint4 *counts, hipStream_t stream)
{
    if (n_windows == 0 || set.n == 0)
        return hipSuccess;
    if (n_windows > DST_WINDOWS_MAX || set.n > 0xFFFFFFFFull || set.len > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    return for_row_grids(0, n_windows, [&](uint64_t win0, unsigned nwin) {
        hipLaunchKernelGGL(window_counts_kernel, dim3((unsigned)((set.n + 255) / 256), nwin), dim3(256), 0, stream, set.planes,
                           d_windows, (uint32_t)set.n, (uint32_t)set.nchunks, (uint32_t)set.npad, (uint32_t)win0, counts);
        return hipGetLastError();
    });
}

// =============================================================================================
// the calls
// =============================================================================================
namespace {

const char *const kSharedRefusal = "a set uploaded with dst_upload_shared runs on the consensus path only (this rank holds "
                                   "the planes of its own records)";

}  // namespace

int windows_valid(dst_ctx *ctx, const uint64_t *wb, const uint64_t *we, uint32_t n_windows, uint64_t len)
{
    for (uint32_t w = 0; w < n_windows; ++w)
        if (wb[w] > we[w] || we[w] > len) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "window %u [%llu, %llu) is not a column range of an alignment of %llu sites", w,
                          (unsigned long long)wb[w], (unsigned long long)we[w], (unsigned long long)len);
            return fail(ctx, DST_ERR_ARG, msg);
        }
    return DST_OK;
}

namespace {

int grow_or_nomem(dst_ctx *ctx, GrownBase &buf, size_t want, const char *what)
{
    const int rc = buf.grow(ctx, want);
    if (rc == DST_ERR_NOMEM)
        return fail(ctx, DST_ERR_NOMEM, std::string("windows: cannot allocate ") + std::to_string(want) + " bytes for " + what);
    return rc;
}

// the window table on the device, by way of its page-locked copy (the caller has waited for every earlier reader)
int upload_windows(dst_ctx *ctx, const uint64_t *wb, const uint64_t *we, uint32_t n_windows, hipStream_t stream)
{
    const size_t bytes = (size_t)n_windows * sizeof(uint2);
    if (int rc = grow_or_nomem(ctx, ctx->win_table, bytes, "the window table"))
        return rc;
    if (ctx->win_table_host.bytes < bytes) {
        const int rc = ctx->win_table_host.grow(ctx, bytes, "windows");
        if (rc)
            return rc;
    }
    uint2 *h = ctx->win_table_host;
    for (uint32_t w = 0; w < n_windows; ++w)
        h[w] = make_uint2((uint32_t)wb[w], (uint32_t)we[w]);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->win_table, h, bytes, hipMemcpyHostToDevice, stream));
    return DST_OK;
}

// what both forms of dst_run_windows check, in the documented order; *bytes = the output's size (0: nothing to do)
int windows_args(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint64_t rb, uint64_t re, const uint64_t *wb,
                 const uint64_t *we, uint32_t n_windows, int out_kind, const void *out, size_t cap, TwoSets &ts, uint64_t &pairs,
                 size_t &bytes)
{
    bytes = 0;
    pairs = 0;
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (n_windows && (!wb || !we))
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (out_kind == DST_OUT_TALLY16)
        return fail(ctx, DST_ERR_ARG, "dst_run_windows writes DST_OUT_DISTANCE or DST_OUT_TALLY (no DST_OUT_TALLY16)");
    if (out_kind != DST_OUT_DISTANCE && out_kind != DST_OUT_TALLY)
        return fail(ctx, DST_ERR_ARG, "unknown output kind");
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts))
        return rc;
    const DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (rows.partial || cols.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (rows.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_run_windows");
    if (int rc = windows_valid(ctx, wb, we, n_windows, rows.len))
        return rc;
    if (rb > re || re > rows.n)
        return fail(ctx, DST_ERR_ARG, "row range out of bounds");
    if (rows.n >= 0xFFFFFFFFull || cols.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    pairs = pairs_in_rows(square != 0, cols.n, rb, re);
    if (n_windows == 0 || pairs == 0)
        return DST_OK;
    const unsigned __int128 need = (unsigned __int128)n_windows * dst_out_bytes(measure, out_kind, pairs);
    if (need > (unsigned __int128)cap)
        return fail(ctx, DST_ERR_CAPACITY, "output buffer too small for the requested rows and windows");
    if (!out)
        return fail(ctx, DST_ERR_ARG, "null output pointer");
    bytes = (size_t)need;
    return DST_OK;
}

// what a window call queues first: the planes its kernels read and the window table on the device
int windows_prepare(dst_ctx *ctx, const TwoSets &ts, const uint64_t *wb, const uint64_t *we, uint32_t n_windows, hipStream_t stream)
{
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the window and count tables are the context's: nothing queued earlier may still read them
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (stream != ctx->stream)
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (int rc = order_after_prep(ctx, stream))
        return rc;
    int rc = ensure_derived(ctx, cols, stream);
    if (!rc && &rows != &cols)
        rc = ensure_derived(ctx, rows, stream);
    if (!rc)
        rc = upload_windows(ctx, wb, we, n_windows, stream);
    return rc;
}

// tn93's per-window base counts of both sets, [n_windows][rows.n] and [n_windows][cols.n] (one table when they are one set)
int window_count_tables(dst_ctx *ctx, const DeviceSet &rows, const DeviceSet &cols, uint32_t n_windows, hipStream_t stream,
                        const uint4 *&q_counts, const uint4 *&t_counts)
{
    const size_t per_row = (size_t)n_windows * rows.n, per_col = &rows != &cols ? (size_t)n_windows * cols.n : 0;
    if (int rc = grow_or_nomem(ctx, ctx->win_counts, (per_row + per_col) * sizeof(uint4), "tn93's per-window base counts"))
        return rc;
    uint4 *q = ctx->win_counts, *t = per_col ? q + per_row : q;
    HIP_TRY(ctx, launch_window_counts(rows, ctx->win_table, n_windows, q, stream));
    if (per_col)
        HIP_TRY(ctx, launch_window_counts(cols, ctx->win_table, n_windows, t, stream));
    q_counts = q;
    t_counts = t;
    return DST_OK;
}

int windows_run(dst_ctx *ctx, int measure, const TwoSets &ts, bool square, uint64_t rb, uint64_t re, uint64_t pairs,
                const uint64_t *wb, const uint64_t *we, uint32_t n_windows, int out_kind, void *d_out, hipStream_t stream)
{
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (int rc = windows_prepare(ctx, ts, wb, we, n_windows, stream))
        return rc;
    WindowLaunch wl{};
    wl.rows = &rows;
    wl.cols = &cols;
    wl.square = square;
    wl.row_begin = rb;
    wl.row_end = re;
    wl.pairs = pairs;
    wl.out_kind = out_kind;
    wl.d_out = d_out;
    wl.d_windows = ctx->win_table;
    wl.n_windows = n_windows;
    if (measure == DST_TN93 && out_kind == DST_OUT_DISTANCE)
        if (int rc = window_count_tables(ctx, rows, cols, n_windows, stream, wl.q_counts, wl.t_counts))
            return rc;
    HIP_TRY(ctx, launch_window_pairs(measure, wl, stream));
    return DST_OK;
}

}  // namespace

// The (row, window) lists of a dst_nearest_windows call (or of a window-closest stream's batch) cut into slabs of rows x
// windows: whole row ranges of all the windows while a row's windows fit the budget, else a few rows (the sweep's tile
// holds eight) of a range of windows.
WindowSlabs cut_window_slabs(uint64_t n_rows, uint32_t n_windows, uint64_t n_cols, uint64_t max_entries)
{
    // (no more than 2^40 entries, 16 TB of tn93 tallies: a slab's byte count stays far inside 64 bits)
    const uint64_t budget = max_entries ? std::min<uint64_t>(max_entries, (uint64_t)1 << 40) : kWindowNearestPairs;
    const uint64_t lists = std::min<uint64_t>(std::max<uint64_t>(budget / n_cols, 1), kWindowNearestListsMax);
    WindowSlabs s;
    if (lists >= n_windows) {
        s.rows = std::min<uint64_t>(lists / n_windows, n_rows);
        s.wins = n_windows;
    } else {
        s.rows = std::min<uint64_t>(std::min<uint64_t>(lists, 8), n_rows);
        s.wins = (uint32_t)(lists / s.rows);
    }
    return s;
}

}  // namespace dst

extern "C" {

int dst_run_windows(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint64_t row_begin, uint64_t row_end,
                    const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows, int out_kind, void *d_out,
                    size_t out_capacity_bytes, void *stream_v)
{
    if (!ctx)
        return DST_ERR_ARG;
    TwoSets ts;
    uint64_t pairs = 0;
    size_t bytes = 0;
    if (int rc = windows_args(ctx, measure, square, row_slot, col_slot, row_begin, row_end, win_begin, win_end, n_windows, out_kind,
                              d_out, out_capacity_bytes, ts, pairs, bytes))
        return rc;
    if (bytes == 0)
        return DST_OK;
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : ctx->stream;
    if (int rc = windows_run(ctx, measure, ts, square != 0, row_begin, row_end, pairs, win_begin, win_end, n_windows, out_kind,
                             d_out, stream))
        return rc;
    if (!stream_v)
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

int dst_run_windows_host(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint64_t row_begin, uint64_t row_end,
                         const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows, int out_kind, void *h_out,
                         size_t out_capacity_bytes)
{
    if (!ctx)
        return DST_ERR_ARG;
    TwoSets ts;
    uint64_t pairs = 0;
    size_t bytes = 0;
    if (int rc = windows_args(ctx, measure, square, row_slot, col_slot, row_begin, row_end, win_begin, win_end, n_windows, out_kind,
                              h_out, out_capacity_bytes, ts, pairs, bytes))
        return rc;
    if (bytes == 0)
        return DST_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the staging buffer's earlier readers)
    if (int rc = ctx->host_out.grow(ctx, bytes))
        return rc;
    if (int rc = windows_run(ctx, measure, ts, square != 0, row_begin, row_end, pairs, win_begin, win_end, n_windows, out_kind,
                             ctx->host_out, ctx->stream))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_out, ctx->host_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DST_OK;
}

int dst_window_base_counts(dst_ctx *ctx, int slot, const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                           uint32_t *counts, size_t cap_entries)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (n_windows && (!win_begin || !win_end))
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (slot < 0 || slot > 1)
        return fail(ctx, DST_ERR_ARG, "slot must be 0 or 1");
    DeviceSet &s = ctx->set[slot];
    if (!s.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    if (s.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (s.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_window_base_counts");
    if (s.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    if (int rc = windows_valid(ctx, win_begin, win_end, n_windows, s.len))
        return rc;
    const unsigned __int128 entries = (unsigned __int128)n_windows * s.n * 4;
    if (entries == 0)
        return DST_OK;
    if (entries > (unsigned __int128)cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "counts buffer too small: n_windows x n x 4 entries");
    if (!counts)
        return fail(ctx, DST_ERR_ARG, "null pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (int rc = order_after_prep(ctx, stream))
        return rc;
    int rc = ensure_planes(ctx, s, stream);
    if (!rc)
        rc = upload_windows(ctx, win_begin, win_end, n_windows, stream);
    if (!rc)
        rc = grow_or_nomem(ctx, ctx->win_counts, (size_t)entries * sizeof(uint32_t), "the per-window base counts");
    if (rc)
        return rc;
    HIP_TRY(ctx, launch_window_counts(s, ctx->win_table, n_windows, ctx->win_counts, stream));
    HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->win_counts, (size_t)entries * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

int dst_nearest_windows(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint64_t row_begin, uint64_t row_end,
                        const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows, uint32_t k, uint64_t max_entries,
                        uint32_t *index, uint32_t *tallies, void *values, size_t cap_entries, uint32_t *k_used)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (k_used)
        *k_used = 0;
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (n_windows && (!win_begin || !win_end))
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (k < 1 || k > kNearestMaxK)
        return fail(ctx, DST_ERR_ARG, "k must be between 1 and 256");
    if (!index || !k_used)
        return fail(ctx, DST_ERR_ARG, "null index or k_used pointer");
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (rows.partial || cols.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (rows.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_nearest_windows");
    if (int rc = windows_valid(ctx, win_begin, win_end, n_windows, rows.len))
        return rc;
    if (row_begin > row_end || row_end > rows.n)
        return fail(ctx, DST_ERR_ARG, "row range out of bounds");
    if (rows.n >= 0xFFFFFFFFull || cols.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    const uint64_t n_rows = row_end - row_begin, n_cols = cols.n;
    const uint64_t candidates = square ? (n_cols > 0 ? n_cols - 1 : 0) : n_cols;
    const uint32_t ku = (uint32_t)std::min<uint64_t>(k, candidates);
    *k_used = ku;
    const unsigned __int128 entries = (unsigned __int128)n_rows * n_windows * ku;
    if (entries == 0)
        return DST_OK;
    if (entries > (unsigned __int128)cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "cap_entries is below rows x n_windows x k_used");
    hipStream_t stream = ctx->stream;
    if (int rc = windows_prepare(ctx, ts, win_begin, win_end, n_windows, stream))
        return rc;
    const int W = tally_width(measure);
    const WindowSlabs cut = cut_window_slabs(n_rows, n_windows, n_cols, max_entries);
    // the slab's tallies, and its lists: payloads, indices and tallies of rows x wins x k_used entries, each 256-byte aligned
    const uint64_t slab_lists = cut.rows * cut.wins, slab_entries = slab_lists * ku;
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t val_bytes = pad(slab_entries * 8), idx_bytes = pad(slab_entries * 4), tal_bytes = pad(slab_entries * W * 4);
    if (int rc = grow_or_nomem(ctx, ctx->pair_slab, std::max<size_t>(dst_out_bytes(measure, DST_OUT_TALLY, slab_lists * n_cols), 256),
                               "a slab of window tallies"))
        return rc;
    if (int rc = grow_or_nomem(ctx, ctx->nn_lists, val_bytes + idx_bytes + tal_bytes, "a slab's lists"))
        return rc;
    NearestLists nl{};
    char *lists = static_cast<char *>(ctx->nn_lists.ptr);
    nl.val = reinterpret_cast<uint64_t *>(lists);
    nl.idx = reinterpret_cast<uint32_t *>(lists + val_bytes);
    nl.tal = reinterpret_cast<uint32_t *>(lists + val_bytes + idx_bytes);
    nl.k = ku;
    WindowLaunch wl{};
    wl.rows = &rows;
    wl.cols = &cols;
    wl.square = false;   // a square job too: slot 0 against itself, so that a row finds all its j != i in the slab
    wl.out_kind = DST_OUT_TALLY;
    wl.d_out = ctx->pair_slab;
    wl.d_windows = ctx->win_table;
    const uint4 *q_counts = nullptr, *t_counts = nullptr;
    if (measure == DST_TN93)
        if (int rc = window_count_tables(ctx, rows, cols, n_windows, stream, q_counts, t_counts))
            return rc;
    // Slab after slab on the stream: sweep, select, copy the lists back.  A slab of all the windows is one contiguous
    // piece of the result; a slab of some windows is one piece per row.  Nothing waits but the copies into host memory.
    const size_t row_pitch = (size_t)n_windows * ku;   // entries of a row record in the result
    const auto copy_back = [&](void *host, const void *dev, size_t entry_bytes, uint64_t r0, uint64_t nr, uint32_t w0,
                               uint32_t nw) -> hipError_t {
        char *h = static_cast<char *>(host) + ((size_t)(r0 - row_begin) * row_pitch + (size_t)w0 * ku) * entry_bytes;
        const char *d = static_cast<const char *>(dev);
        const size_t piece = (size_t)nw * ku * entry_bytes;
        if (nw == n_windows)
            return hipMemcpyAsync(h, d, piece * nr, hipMemcpyDeviceToHost, stream);
        for (uint64_t r = 0; r < nr; ++r)
            if (const hipError_t e = hipMemcpyAsync(h + r * row_pitch * entry_bytes, d + r * piece, piece, hipMemcpyDeviceToHost, stream))
                return e;
        return hipSuccess;
    };
    for (uint64_t r0 = row_begin; r0 < row_end; r0 += cut.rows) {
        const uint64_t nr = std::min<uint64_t>(cut.rows, row_end - r0);
        for (uint32_t w0 = 0; w0 < n_windows; w0 += cut.wins) {
            const uint32_t nw = std::min<uint32_t>(cut.wins, n_windows - w0);
            wl.row_begin = r0;
            wl.row_end = r0 + nr;
            wl.pairs = nr * n_cols;
            wl.win_first = w0;
            wl.n_windows = nw;
            HIP_TRY(ctx, launch_window_pairs(measure, wl, stream));
            HIP_TRY(ctx, launch_window_nearest(measure, static_cast<const uint32_t *>(ctx->pair_slab.ptr), q_counts, t_counts, rows.n,
                                               n_cols, r0, nr, w0, nw, square != 0, nl, stream));
            HIP_TRY(ctx, copy_back(index, nl.idx, 4, r0, nr, w0, nw));
            if (values)
                HIP_TRY(ctx, copy_back(values, nl.val, 8, r0, nr, w0, nw));
            if (tallies)
                HIP_TRY(ctx, copy_back(tallies, nl.tal, (size_t)W * 4, r0, nr, w0, nw));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

int dst_window_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, const uint64_t *win_begin,
                       const uint64_t *win_end, uint32_t n_windows, double threshold, dst_summary_totals *totals,
                       uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum, size_t rec_cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (n_windows && (!win_begin || !win_end))
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    const bool per_record = rec_within || rec_summable || rec_sum;
    if (!totals && !per_record)
        return fail(ctx, DST_ERR_ARG, "null output pointers: neither the totals nor a per-record array is wanted");
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (rows.partial || cols.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (rows.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_window_summary");
    if (int rc = windows_valid(ctx, win_begin, win_end, n_windows, rows.len))
        return rc;
    if (rows.n >= 0xFFFFFFFFull || cols.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    const uint64_t entries = n_rows * n_windows;   // (below 2^48)
    if (per_record && entries > ((uint64_t)1 << 31))
        return fail(ctx, DST_ERR_ARG, "per-record arrays of more than 2^31 entries (n_windows x the row set's records)");
    if (per_record && (unsigned __int128)rec_cap < entries)
        return fail(ctx, DST_ERR_CAPACITY, "rec_cap is below n_windows x the row set's record count");
    const uint64_t pairs = pairs_in_rows(square != 0, n_cols, 0, n_rows);
    if (n_windows == 0 || pairs == 0) {   // no launch: zero counts and sums
        for (uint32_t w = 0; totals && w < n_windows; ++w)
            totals[w] = dst_summary_totals{pairs, 0, 0, 0, 0.0};
        for (uint64_t e = 0; per_record && e < entries; ++e) {
            if (rec_within)
                rec_within[e] = 0;
            if (rec_summable)
                rec_summable[e] = 0;
            if (rec_sum)
                rec_sum[e] = 0.0;
        }
        return DST_OK;
    }
    const bool int_payload = measure_is_int(measure);
    // the state: the per-record arrays, window-major (the lanes of a column-side add hit adjacent words), then the totals
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t rec_entries = per_record ? (size_t)entries : 0;
    const size_t at_summable = pad(rec_entries * 4), at_hi = at_summable + pad(rec_entries * 4), at_lo = at_hi + pad(rec_entries * 8),
                 at_tot = at_lo + pad(rec_entries * 8), state_bytes = at_tot + pad((size_t)n_windows * kWindowSummaryTotals * 8);
    {
        const int rc = ctx->win_summary_work.grow(ctx, state_bytes);
        if (rc == DST_ERR_NOMEM)
            return fail(ctx, DST_ERR_NOMEM, "window summary: cannot allocate " + std::to_string(state_bytes) + " bytes for the per-window state");
        if (rc)
            return rc;
    }
    if (ctx->win_summary_host.bytes < state_bytes)   // (page-locked: the copy back runs at the link's rate)
        if (int rc = ctx->win_summary_host.grow(ctx, state_bytes, "window summary"))
            return rc;
    hipStream_t stream = ctx->stream;
    if (int rc = windows_prepare(ctx, ts, win_begin, win_end, n_windows, stream))
        return rc;
    char *state = static_cast<char *>(ctx->win_summary_work.ptr);
    // measurement knob: the full square with the row side only, instead of the triangle's column side
    static const bool full_square = std::getenv("DST_WINDOW_SUMMARY_FULL_SQUARE") != nullptr;
    WindowSummaryLaunch wl{};
    wl.rows = &rows;
    wl.cols = &cols;
    wl.mode = !square ? kWinSumRect : full_square && per_record ? kWinSumFull : kWinSumTriangle;    wl.d_windows = ctx->win_table;
    wl.n_windows = n_windows;
    wl.any = threshold_payload(measure, threshold, wl.t_bits);
    if (per_record) {
        wl.within = reinterpret_cast<uint32_t *>(state);
        wl.summable = reinterpret_cast<uint32_t *>(state + at_summable);
        wl.hi = reinterpret_cast<int64_t *>(state + at_hi);
        wl.lo = reinterpret_cast<uint64_t *>(state + at_lo);
    }
    wl.tot = reinterpret_cast<uint64_t *>(state + at_tot);
    HIP_TRY(ctx, hipMemsetAsync(state, 0, state_bytes, stream));
    if (measure == DST_TN93)
        if (int rc = window_count_tables(ctx, rows, cols, n_windows, stream, wl.q_counts, wl.t_counts))
            return rc;
    HIP_TRY(ctx, launch_window_summary(measure, wl, stream));
    // the state back in one copy, then the 128-bit sums here
    const char *host = ctx->win_summary_host;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->win_summary_host, state, state_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    const uint32_t *h_within = reinterpret_cast<const uint32_t *>(host);
    const uint32_t *h_summable = reinterpret_cast<const uint32_t *>(host + at_summable);
    const int64_t *h_hi = reinterpret_cast<const int64_t *>(host + at_hi);
    const uint64_t *h_lo = reinterpret_cast<const uint64_t *>(host + at_lo);
    const uint64_t *h_tot = reinterpret_cast<const uint64_t *>(host + at_tot);
    for (uint64_t e = 0; e < rec_entries; ++e) {
        if (rec_within)
            rec_within[e] = h_within[e];
        if (rec_summable)
            rec_summable[e] = h_summable[e];
        if (rec_sum)
            rec_sum[e] = summary_value((__int128)h_hi[e] * ((__int128)1 << 32) + (__int128)h_lo[e], int_payload);
    }
    const unsigned each = wl.mode == kWinSumFull ? 2 : 1;   // (the full square meets every pair twice)
    for (uint32_t w = 0; w < n_windows; ++w) {
        const uint64_t *t = h_tot + (size_t)w * kWindowSummaryTotals;
        const __int128 all = (__int128)(((unsigned __int128)t[3] << 64) | t[4]);
        if (t[1] % each || t[2] % each || all % each)
            return fail(ctx, DST_ERR_STATE, "window summary: internal error, the two sides of the square disagree");
        if (t[0] > pairs || t[1] / each > pairs - t[0] || t[2] / each > pairs - t[0])
            return fail(ctx, DST_ERR_STATE, "window summary: internal error, a window counts more than its pairs");
        if (totals)
            totals[w] = dst_summary_totals{pairs, t[0], t[1] / each, t[2] / each, summary_value(all / each, int_payload)};
    }
    return DST_OK;
}

int dst_window_group_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, const uint64_t *win_begin,
                             const uint64_t *win_end, uint32_t n_windows, const uint32_t *row_group, uint32_t n_row_groups,
                             const uint32_t *col_group, uint32_t n_col_groups, double threshold, dst_group_cell *cells,
                             size_t cells_cap, uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum, size_t rec_cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (n_windows && (!win_begin || !win_end))
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    const bool per_record = rec_within || rec_summable || rec_sum;
    if (!cells && !per_record)
        return fail(ctx, DST_ERR_ARG, "null cells pointer and no per-record array");
    if (!row_group)
        return fail(ctx, DST_ERR_ARG, "null row_group pointer");
    if (square) {
        col_group = row_group;
        n_col_groups = n_row_groups;
    } else if (!col_group)
        return fail(ctx, DST_ERR_ARG, "null col_group pointer");
    if (n_row_groups == 0 || n_row_groups > DST_WINDOW_GROUPS_MAX || n_col_groups == 0 || n_col_groups > DST_WINDOW_GROUPS_MAX)
        return fail(ctx, DST_ERR_ARG, "a group count must be between 1 and " + std::to_string(DST_WINDOW_GROUPS_MAX));
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (rows.partial || cols.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (rows.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_window_group_summary");
    if (int rc = windows_valid(ctx, win_begin, win_end, n_windows, rows.len))
        return rc;
    if (rows.n >= 0xFFFFFFFFull || cols.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    const uint32_t Gr = n_row_groups, Gc = n_col_groups;
    std::vector<uint64_t> row_size, col_size_own;
    if (int rc = group_labels(ctx, row_group, n_rows, Gr, square ? "set" : "row", row_size))
        return rc;
    if (!square)
        if (int rc = group_labels(ctx, col_group, n_cols, Gc, "column", col_size_own))
            return rc;
    const std::vector<uint64_t> &col_size = square ? row_size : col_size_own;
    const uint64_t per_window = (uint64_t)Gr * Gc;                              // cells of one window (at most 2^16)
    const uint64_t n_cells = per_window * n_windows;                            // (at most 2^32)
    const unsigned __int128 entries = (unsigned __int128)n_rows * n_windows * Gc;   // per-record entries
    if (n_cells > ((uint64_t)1 << 31))
        return fail(ctx, DST_ERR_ARG, "more than 2^31 cells (n_windows x row groups x column groups)");
    if (per_record && entries > ((unsigned __int128)1 << 31))
        return fail(ctx, DST_ERR_ARG, "per-record arrays of more than 2^31 entries (n_windows x the row set's records x column groups)");
    if (cells && (unsigned __int128)cells_cap < n_cells)
        return fail(ctx, DST_ERR_CAPACITY, "cells_cap is below " + std::to_string(n_cells) + " entries (n_windows x row groups x column groups)");
    if (per_record && (unsigned __int128)rec_cap < entries)
        return fail(ctx, DST_ERR_CAPACITY, "rec_cap is below " + std::to_string((uint64_t)entries) +
                                               " entries (n_windows x the row set's records x column groups)");
    const size_t rec_entries = per_record ? (size_t)entries : 0;
    const bool int_payload = measure_is_int(measure);
    // what an empty call returns; `pairs` from the group sizes, the same in every window
    const uint64_t none = int_payload ? 0 : 0x7FF8000000000000ull;
    std::vector<uint64_t> cell_pairs(per_window);
    for (uint32_t a = 0; a < Gr; ++a)
        for (uint32_t b = 0; b < Gc; ++b)
            cell_pairs[(size_t)a * Gc + b] =
                square && a == b ? row_size[a] * (row_size[a] - (row_size[a] ? 1 : 0)) / 2 : row_size[a] * col_size[b];
    if (cells)
        for (uint32_t w = 0; w < n_windows; ++w)
            for (uint64_t c = 0; c < per_window; ++c)
                cells[(size_t)w * per_window + c] = dst_group_cell{cell_pairs[c], 0, 0, 0, 0.0, none, none};
    for (size_t e = 0; e < rec_entries; ++e) {
        if (rec_within)
            rec_within[e] = 0;
        if (rec_summable)
            rec_summable[e] = 0;
        if (rec_sum)
            rec_sum[e] = 0.0;
    }
    if (n_windows == 0 || pairs_in_rows(square != 0, n_cols, 0, n_rows) == 0)
        return DST_OK;   // (no pair: no launch)
    uint64_t rows_assigned = 0, cols_assigned = 0;
    for (uint64_t s : row_size)
        rows_assigned += s;
    for (uint64_t s : col_size)
        cols_assigned += s;
    if (cols_assigned == 0 || (rows_assigned == 0 && !per_record))
        return DST_OK;   // (no partner has a group, or no cell has a pair and only the cells are wanted)
    // the state: the labels, then what comes back: the cells and the per-record arrays behind them
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t at_col = pad((size_t)n_rows * 4), at_cells = square ? at_col : at_col + pad((size_t)n_cols * 4),
                 at_counts = at_cells + pad((size_t)n_cells * kWindowGroupCellWords * 8), at_hi = at_counts + pad(rec_entries * 8),
                 at_lo = at_hi + pad(rec_entries * 8), state_bytes = at_lo + pad(rec_entries * 8);
    {
        const int rc = ctx->win_group_work.grow(ctx, state_bytes);
        if (rc == DST_ERR_NOMEM)
            return fail(ctx, DST_ERR_NOMEM,
                        "window group summary: cannot allocate " + std::to_string(state_bytes) + " bytes for the per-window state");
        if (rc)
            return rc;
    }
    if (ctx->win_group_host.bytes < state_bytes)   // (page-locked: the copy back runs at the link's rate)
        if (int rc = ctx->win_group_host.grow(ctx, state_bytes, "window group summary"))
            return rc;
    hipStream_t stream = ctx->stream;
    if (int rc = windows_prepare(ctx, ts, win_begin, win_end, n_windows, stream))
        return rc;
    char *state = static_cast<char *>(ctx->win_group_work.ptr);
    char *host = ctx->win_group_host;
    std::memcpy(host, row_group, (size_t)n_rows * 4);
    if (!square)
        std::memcpy(host + at_col, col_group, (size_t)n_cols * 4);
    WindowGroupLaunch wl{};
    wl.rows = &rows;
    wl.cols = &cols;
    // the square: the triangle for the cells alone; with per-record arrays the full square, the row side only
    wl.mode = !square ? kWinSumRect : per_record ? kWinSumFull : kWinSumTriangle;
    wl.d_windows = ctx->win_table;
    wl.n_windows = n_windows;
    wl.any = threshold_payload(measure, threshold, wl.t_bits);
    wl.row_group = reinterpret_cast<const uint32_t *>(state);
    wl.col_group = square ? wl.row_group : reinterpret_cast<const uint32_t *>(state + at_col);
    wl.g_rows = Gr;
    wl.g_cols = Gc;
    wl.cell = reinterpret_cast<uint64_t *>(state + at_cells);
    if (per_record) {
        wl.rec_counts = reinterpret_cast<uint64_t *>(state + at_counts);
        wl.rec_hi = reinterpret_cast<int64_t *>(state + at_hi);
        wl.rec_lo = reinterpret_cast<uint64_t *>(state + at_lo);
    }
    HIP_TRY(ctx, hipMemcpyAsync(state, host, at_cells, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemsetAsync(state + at_cells, 0, state_bytes - at_cells, stream));
    HIP_TRY(ctx, launch_window_group_init(wl.cell, n_cells, stream));
    if (measure == DST_TN93)
        if (int rc = window_count_tables(ctx, rows, cols, n_windows, stream, wl.q_counts, wl.t_counts))
            return rc;
    HIP_TRY(ctx, launch_window_groups(measure, wl, stream));
    // the cells and the arrays behind them back in one copy, then the 128-bit sums here
    HIP_TRY(ctx, hipMemcpyAsync(host + at_cells, state + at_cells, state_bytes - at_cells, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    const uint64_t *h_cell = reinterpret_cast<const uint64_t *>(host + at_cells);
    const uint64_t *h_counts = reinterpret_cast<const uint64_t *>(host + at_counts);
    const int64_t *h_hi = reinterpret_cast<const int64_t *>(host + at_hi);
    const uint64_t *h_lo = reinterpret_cast<const uint64_t *>(host + at_lo);
    for (uint32_t w = 0; cells && w < n_windows; ++w)
        for (uint32_t a = 0; a < Gr; ++a)
            for (uint32_t g = 0; g < Gc; ++g) {
                const size_t c = (size_t)w * per_window + (size_t)a * Gc + g;
                const uint64_t *t = h_cell + c * kWindowGroupCellWords;
                uint64_t n_nan = t[0], n_links = t[1], n_summ = t[2], lo_key = t[5], hi_key = t[6];
                __int128 S = (__int128)(((unsigned __int128)t[3] << 64) | t[4]);
                if (wl.mode == kWinSumFull && a == g) {
                    // the full square met every pair of the diagonal cell from both of its records
                    if (n_nan % 2 || n_links % 2 || n_summ % 2 || S % 2)
                        return fail(ctx, DST_ERR_STATE, "window group summary: internal error, the two sides of the square disagree");
                    n_nan /= 2, n_links /= 2, n_summ /= 2, S /= 2;
                } else if (wl.mode == kWinSumTriangle && a != g) {
                    // the triangle met a pair as (group of i, group of j), i < j: either order may hold it
                    const uint64_t *m = h_cell + ((size_t)w * per_window + (size_t)g * Gc + a) * kWindowGroupCellWords;
                    n_nan += m[0], n_links += m[1], n_summ += m[2];
                    S += (__int128)(((unsigned __int128)m[3] << 64) | m[4]);
                    lo_key = std::min(lo_key, m[5]);
                    hi_key = std::max(hi_key, m[6]);
                }
                dst_group_cell &out = cells[c];
                if (n_nan + n_summ > out.pairs || n_links > out.pairs)
                    return fail(ctx, DST_ERR_STATE, "window group summary: internal error, a cell counts more than its pairs");
                out.nan_pairs = n_nan;
                out.summable_pairs = n_summ;
                out.links = n_links;
                out.sum = summary_value(S, int_payload);
                if (out.pairs > n_nan) {
                    out.min_bits = payload_of_key(lo_key, int_payload);
                    out.max_bits = payload_of_key(hi_key, int_payload);
                }
            }
    for (size_t e = 0; e < rec_entries; ++e) {
        if (rec_within)
            rec_within[e] = (uint32_t)(h_counts[e] >> 32);
        if (rec_summable)
            rec_summable[e] = (uint32_t)h_counts[e];
        if (rec_sum)
            rec_sum[e] = summary_value((__int128)h_hi[e] * ((__int128)1 << 32) + (__int128)h_lo[e], int_payload);
    }
    return DST_OK;
}

}  // extern "C"
