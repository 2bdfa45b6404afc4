// dst_nearest.hip — the k nearest records of every record (dst_nearest): selection kernels over one row slab of
// DST_OUT_TALLY tallies, merged into running lists that live on the device for the whole call.
//
//   nearest_init_kernel  every list entry := the sentinel (a key above every real one, index 2^32-1)
//   nearest_rows_kernel  row pass: row i of the slab offers its pairs to record i's list (one wave per row)
//   nearest_cols_kernel  column pass, square only: pairs (i, j) with i in the slab and j > i offer i to record j's list;
//                        a wave owns 64 consecutive j, reads 64 rows of them coalesced into LDS, then walks the columns
//   nearest_stream_cols_kernel  column pass over a rectangle [streamed][loaded]: every row of a streamed batch offers its
//                        ordinal to every loaded record's list, which persists from batch to batch (closest streams)
//
// A list is sorted ascending by (key, index), a strict total order, so the k smallest are unique and the passes may
// meet the candidates in any order.  Inside a kernel a wave holds one list in registers, entry e = 64 s + lane in slot
// s (k <= kNearestMaxK = 256: four slots); a candidate below the list's k-th entry is inserted by a shift across the
// lanes.  The value of a pair is the DST_OUT_DISTANCE payload, from the tallies through finalize_pair<M, false> — the
// arithmetic of the pair kernels' epilogue and of finalize_kernel — so it is bitwise what a distance run returns.
#include "dst_device.hpp"
#include "dst_wavelist.hpp"

namespace dst {
namespace {

__global__ __launch_bounds__(256) void nearest_init_kernel(uint64_t *lval, uint32_t *lidx, uint64_t entries)
{
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * blockDim.x) {
        lval[e] = kSentinelVal;
        lidx[e] = kSentinelIdx;
    }
}

// Row pass.  Row i of the slab: square, pairs (i, j > i) from slab entry tri_row_start(n, i) - out_base; rectangle,
// pairs (i, 0 .. n_cols-1) from (i - rb) n_cols.  One wave per row, 64 consecutive candidates per step.
template <int M, int W>
__global__ __launch_bounds__(256) void nearest_rows_kernel(const uint32_t *__restrict__ slab, uint64_t out_base, uint32_t n_cols,
                                                           uint32_t rb, uint32_t re, int square,
                                                           const uint32_t *__restrict__ q_counts,
                                                           const uint32_t *__restrict__ t_counts, uint64_t *lval,
                                                           uint32_t *lidx, uint32_t *ltal, uint32_t k)
{
    constexpr bool INT = M == DST_N_HIGH;
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t i = rb + (uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (i >= re)
        return;   // (whole waves)
    const uint32_t jstart = square ? i + 1 : 0;
    const uint64_t base = square ? tri_row_start(n_cols, i) - out_base : (uint64_t)(i - rb) * n_cols;
    uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
    if constexpr (M == DST_TN93)
        qc = reinterpret_cast<const uint4 *>(q_counts)[i];
    WaveList<W> L;
    L.template load<INT>(lval, lidx, ltal, (uint64_t)i * k, k, lane);
    for (uint32_t j0 = jstart; j0 < n_cols; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        const bool valid = j < n_cols;
        uint32_t o[W];
        uint64_t v = 0, key = ~0ull;
        if (valid) {
            const uint64_t at = base + (j - jstart);
#pragma unroll
            for (int t = 0; t < W; ++t)
                o[t] = slab[at * W + t];
            if constexpr (M == DST_TN93)
                tc = reinterpret_cast<const uint4 *>(t_counts)[j];
            v = pair_value<M>(o, qc, tc);
            key = nn_key<INT>(v);
        } else {
#pragma unroll
            for (int t = 0; t < W; ++t)
                o[t] = 0;
        }
        const bool pass = valid && nn_less(key, j, L.thr_key, L.thr_idx);
        const uint64_t mask = __ballot(pass);
        if (mask)
            L.template offer<INT>(mask, pass, key, v, j, o, k, lane);
    }
    L.store(lval, lidx, ltal, (uint64_t)i * k, k, lane);
}

// Column pass (square).  Block b: the 64 records j0 .. j0+63, j0 = rb + 1 + 64 b, against the slab's rows i < j.
// Each step reads 64 rows of those 64 columns (lane = column: consecutive addresses within a row) into LDS, then takes
// the columns one by one with lane = row, like a step of the row pass; a column's list is loaded only when one of
// the 64 candidates is below its k-th entry (every lane keeps its own column's threshold in registers).
template <int M, int W>
__global__ __launch_bounds__(64) void nearest_cols_kernel(const uint32_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                          uint32_t rb, uint32_t re, const uint32_t *__restrict__ counts,
                                                          uint64_t *lval, uint32_t *lidx, uint32_t *ltal, uint32_t k)
{
    constexpr bool INT = M == DST_N_HIGH;
    __shared__ uint64_t tile[64][65];
    const int lane = (int)threadIdx.x;
    const uint32_t j0 = rb + 1 + blockIdx.x * 64;
    const uint32_t jl = j0 + (uint32_t)lane;   // this lane's column in the load phase
    const uint32_t iend = min(re, j0 + 63);    // rows below some column of the block
    uint64_t my_thr_key = ~0ull;
    uint32_t my_thr_idx = kSentinelIdx;
    if (jl < n) {
        const uint64_t e = (uint64_t)jl * k + (k - 1);
        my_thr_idx = lidx[e];
        my_thr_key = my_thr_idx == kSentinelIdx ? ~0ull : nn_key<INT>(lval[e]);
    }
    uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
    if constexpr (M == DST_TN93)
        if (jl < n)
            tc = reinterpret_cast<const uint4 *>(counts)[jl];
    for (uint32_t i0 = rb; i0 < iend; i0 += 64) {
        const uint32_t rows = min(64u, iend - i0);
        for (uint32_t r = 0; r < rows; ++r) {
            const uint32_t i = i0 + r;
            uint64_t v = 0;
            if (i < jl && jl < n) {
                const uint64_t at = tri_row_start(n, i) - out_base + (jl - i - 1);
                uint32_t o[W];
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = slab[at * W + t];
                if constexpr (M == DST_TN93)
                    qc = reinterpret_cast<const uint4 *>(counts)[i];
                v = pair_value<M>(o, qc, tc);
            }
            tile[r][lane] = v;
        }
        __syncthreads();
        const uint32_t i = i0 + (uint32_t)lane;   // this lane's row in the selection phase
        for (int c = 0; c < 64; ++c) {
            const uint32_t j = j0 + (uint32_t)c;
            if (j >= n)
                break;
            const bool valid = (uint32_t)lane < rows && i < j;
            const uint64_t v = tile[lane][c];
            const uint64_t key = valid ? nn_key<INT>(v) : ~0ull;
            const uint64_t tk = shfl64(my_thr_key, c);
            const uint32_t ti = shfl32(my_thr_idx, c);
            const bool pass = valid && nn_less(key, i, tk, ti);
            const uint64_t mask = __ballot(pass);
            if (!mask)
                continue;
            uint32_t o[W];
            if (pass) {
                const uint64_t at = tri_row_start(n, i) - out_base + (j - i - 1);
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = slab[at * W + t];
            } else {
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = 0;
            }
            WaveList<W> L;
            L.template load<INT>(lval, lidx, ltal, (uint64_t)j * k, k, lane);
            L.template offer<INT>(mask, pass, key, v, i, o, k, lane);
            L.store(lval, lidx, ltal, (uint64_t)j * k, k, lane);
            if (lane == c) {
                my_thr_key = L.thr_key;
                my_thr_idx = L.thr_idx;
            }
        }
        __syncthreads();
    }
}

// Column pass over a rectangle (a closest stream, DST_CLOSEST_FOR_LOADED).  The slab is one streamed batch's
// tallies laid out [streamed][loaded]: entry (r, j) at (r n_loaded + j) W, its candidate the streamed ordinal
// first_ordinal + r.  Block b: the 64 loaded records j0 .. j0+63, j0 = 64 b, against every row of the batch — the
// geometry of nearest_cols_kernel without the i < j condition; tn93 reads q from the batch's counts, t from the loaded
// set's.  The lists outlive the launch: the next batch's launch (same stream, behind this one) goes on with them.
template <int M, int W>
__global__ __launch_bounds__(64) void nearest_stream_cols_kernel(const uint32_t *__restrict__ slab, uint32_t n_batch,
                                                                 uint32_t n_loaded, uint32_t first_ordinal,
                                                                 const uint32_t *__restrict__ q_counts,
                                                                 const uint32_t *__restrict__ t_counts, uint64_t *lval,
                                                                 uint32_t *lidx, uint32_t *ltal, uint32_t k)
{
    constexpr bool INT = M == DST_N_HIGH;
    __shared__ uint64_t tile[64][65];
    const int lane = (int)threadIdx.x;
    const uint32_t j0 = blockIdx.x * 64;
    const uint32_t jl = j0 + (uint32_t)lane;   // this lane's column in the load phase
    uint64_t my_thr_key = ~0ull;
    uint32_t my_thr_idx = kSentinelIdx;
    if (jl < n_loaded) {
        const uint64_t e = (uint64_t)jl * k + (k - 1);
        my_thr_idx = lidx[e];
        my_thr_key = my_thr_idx == kSentinelIdx ? ~0ull : nn_key<INT>(lval[e]);
    }
    uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
    if constexpr (M == DST_TN93)
        if (jl < n_loaded)
            tc = reinterpret_cast<const uint4 *>(t_counts)[jl];
    for (uint32_t r0 = 0; r0 < n_batch; r0 += 64) {
        const uint32_t rows = min(64u, n_batch - r0);
        for (uint32_t r = 0; r < rows; ++r) {
            uint64_t v = 0;
            if (jl < n_loaded) {
                const uint64_t at = (uint64_t)(r0 + r) * n_loaded + jl;
                uint32_t o[W];
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = slab[at * W + t];
                if constexpr (M == DST_TN93)
                    qc = reinterpret_cast<const uint4 *>(q_counts)[r0 + r];
                v = pair_value<M>(o, qc, tc);
            }
            tile[r][lane] = v;
        }
        __syncthreads();
        const uint32_t row = r0 + (uint32_t)lane;          // this lane's row in the selection phase
        const uint32_t ord = first_ordinal + row;          // (the host keeps first_ordinal + n_batch - 1 <= 2^32-2)
        const bool valid = (uint32_t)lane < rows;
        for (int c = 0; c < 64; ++c) {
            const uint32_t j = j0 + (uint32_t)c;
            if (j >= n_loaded)
                break;
            const uint64_t v = tile[lane][c];
            const uint64_t key = valid ? nn_key<INT>(v) : ~0ull;
            const uint64_t tk = shfl64(my_thr_key, c);
            const uint32_t ti = shfl32(my_thr_idx, c);
            const bool pass = valid && nn_less(key, ord, tk, ti);
            const uint64_t mask = __ballot(pass);
            if (!mask)
                continue;
            uint32_t o[W];
            if (pass) {
                const uint64_t at = (uint64_t)row * n_loaded + j;
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = slab[at * W + t];
            } else {
#pragma unroll
                for (int t = 0; t < W; ++t)
                    o[t] = 0;
            }
            WaveList<W> L;
            L.template load<INT>(lval, lidx, ltal, (uint64_t)j * k, k, lane);
            L.template offer<INT>(mask, pass, key, v, ord, o, k, lane);
            L.store(lval, lidx, ltal, (uint64_t)j * k, k, lane);
            if (lane == c) {
                my_thr_key = L.thr_key;
                my_thr_idx = L.thr_idx;
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_nearest_init(const NearestLists &nl, uint64_t records, hipStream_t stream)
{
    const uint64_t entries = records * nl.k;
    if (entries == 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>((entries + 255) / 256, 4096);
    hipLaunchKernelGGL(nearest_init_kernel, dim3(blocks), dim3(256), 0, stream, nl.val, nl.idx, entries);
    return hipGetLastError();
}

hipError_t launch_nearest_rows(int measure, bool square, const uint32_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                               uint64_t re, const uint32_t *q_counts, const uint32_t *t_counts, const NearestLists &nl,
                               hipStream_t stream)
{
    if (re <= rb)
        return hipSuccess;
    const unsigned blocks = (unsigned)((re - rb + 3) / 4);   // four waves (rows) per workgroup
#define DST_NN_ROWS(MEAS, W)                                                                                            \
    hipLaunchKernelGGL((nearest_rows_kernel<MEAS, W>), dim3(blocks), dim3(256), 0, stream, slab, out_base, (uint32_t)n_cols, \
                       (uint32_t)rb, (uint32_t)re, square ? 1 : 0, q_counts, t_counts, nl.val, nl.idx, nl.tal, nl.k)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_NN_ROWS(DST_N_HIGH, 1); break;
    case DST_RAW: DST_NN_ROWS(DST_RAW, 2); break;
    case DST_JC69: DST_NN_ROWS(DST_JC69, 2); break;
    case DST_K80: DST_NN_ROWS(DST_K80, 3); break;
    case DST_TN93: DST_NN_ROWS(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_NN_ROWS
    return hipGetLastError();
}

hipError_t launch_nearest_cols(int measure, const uint32_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                               const uint32_t *counts, const NearestLists &nl, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const unsigned blocks = (unsigned)((n - rb - 1 + 63) / 64);
#define DST_NN_COLS(MEAS, W)                                                                                            \
    hipLaunchKernelGGL((nearest_cols_kernel<MEAS, W>), dim3(blocks), dim3(64), 0, stream, slab, out_base, (uint32_t)n,      \
                       (uint32_t)rb, (uint32_t)re, counts, nl.val, nl.idx, nl.tal, nl.k)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_NN_COLS(DST_N_HIGH, 1); break;
    case DST_RAW: DST_NN_COLS(DST_RAW, 2); break;
    case DST_JC69: DST_NN_COLS(DST_JC69, 2); break;
    case DST_K80: DST_NN_COLS(DST_K80, 3); break;
    case DST_TN93: DST_NN_COLS(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_NN_COLS
    return hipGetLastError();
}

hipError_t launch_nearest_stream_cols(int measure, const uint32_t *slab, uint64_t n_batch, uint64_t n_loaded, uint32_t first_ordinal,
                                      const uint32_t *q_counts, const uint32_t *t_counts, const NearestLists &nl, hipStream_t stream)
{
    if (n_batch == 0 || n_loaded == 0 || nl.k == 0)
        return hipSuccess;
    if (n_batch > 0xFFFFFFFFull || n_loaded > 0xFFFFFFFFull || (uint64_t)first_ordinal + n_batch - 1 > 0xFFFFFFFEull)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n_loaded + 63) / 64);
#define DST_NN_STREAM(MEAS, W)                                                                                           \
    hipLaunchKernelGGL((nearest_stream_cols_kernel<MEAS, W>), dim3(blocks), dim3(64), 0, stream, slab, (uint32_t)n_batch,    \
                       (uint32_t)n_loaded, first_ordinal, q_counts, t_counts, nl.val, nl.idx, nl.tal, nl.k)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_NN_STREAM(DST_N_HIGH, 1); break;
    case DST_RAW: DST_NN_STREAM(DST_RAW, 2); break;
    case DST_JC69: DST_NN_STREAM(DST_JC69, 2); break;
    case DST_K80: DST_NN_STREAM(DST_K80, 3); break;
    case DST_TN93: DST_NN_STREAM(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_NN_STREAM
    return hipGetLastError();
}

}  // namespace dst
