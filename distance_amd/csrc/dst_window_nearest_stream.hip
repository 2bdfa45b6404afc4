// dst_window_nearest_stream.hip — the k nearest STREAMED records of every (loaded record, window), kept across the batches
// of a window-closest stream (dst_stream_open_window_closest): the merge of one batch's window tallies, which
// window_pair_kernel (dst_windows.hip) swept directly before it, into lists that outlive the batch.
//
// The scratch holds loaded rows [row0, row0 + nr) x windows [win0, win0 + nw) x the n_batch records of the batch as
// DST_OUT_TALLY words, entry (w_local nr + i_local) n_batch + j: the slab layout of dst_window_nearest.hip, with the batch as
// the column set.  The lists are the stream's, list i n_windows + w at entry (i n_windows + w) k.
//
// Mapping (window_nearest_stream_kernel): one wave per (loaded record, window) list of the range, four waves per
// workgroup, the range's lists linearised over grid.x; the list number is wave-uniform (readfirstlane), so the list's
// address, the row's counts and the scratch row are scalars.  The wave loads its list (entry e = 64 s + lane: contiguous
// 8- and 4-byte loads, one 16-byte load per lane for tn93's tallies and counts), runs its lanes along the batch, 64
// candidates per step — an entry is W words, one 4 / 8 / 12 / 16-byte load per lane, contiguous across the wave — and
// offers what passes the list's threshold with the ordinal first_ordinal + j.  A list that took nothing is not stored.
// Every list has one writer per launch; launches that share lists follow one another on one stream.
//
// tn93 carries the streamed record's per-window {A,T,G,C} beside the four tallies (the batch is gone when the result is
// read, and dst_finalize needs them): the wave's list is WaveList<8>, words 0-3 the tallies (lists' tal), 4-7 the counts
// (lists' cnt), two arrays so that either leaves the device by one strided copy (WaveList's load / store with a split).
#include "dst_device.hpp"
#include "dst_wavelist.hpp"

namespace dst {
namespace {

template <int M, int W>
__global__ __launch_bounds__(256) void window_nearest_stream_kernel(
    const uint32_t *__restrict__ slab, const uint4 *__restrict__ q_counts, const uint4 *__restrict__ t_counts, uint32_t q_n,
    uint32_t n_batch, uint32_t row0, uint32_t nr, uint32_t win0, uint32_t nw, uint32_t n_windows, uint32_t first_ordinal,
    uint64_t *lval, uint32_t *lidx, uint32_t *ltal, uint32_t *lcnt, uint32_t k)
{
    constexpr bool INT = M == DST_N_HIGH;
    constexpr int WL = M == DST_TN93 ? W + 4 : W;   // the list's words per entry: the tallies (and tn93's counts)
    const int lane = (int)(threadIdx.x & 63);
    // the wave's list of the range (wave-uniform; the host keeps q_n * n_windows <= 2^31)
    const uint32_t list = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if ((uint64_t)list >= (uint64_t)nr * nw)
        return;   // (whole waves)
    const uint32_t il = list / nw, wl = list % nw;
    const uint32_t i = row0 + il, w = win0 + wl;
    const uint64_t base = ((uint64_t)wl * nr + il) * n_batch;      // the list's candidates in the scratch
    const uint64_t at = ((uint64_t)i * n_windows + w) * k;         // the list itself
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (M == DST_TN93)
        qc = q_counts[(uint64_t)w * q_n + i];
    WaveList<WL> L;
    L.template load<INT, W>(lval, lidx, ltal, at, k, lane, lcnt);   // (tn93: words W .. WL-1 in lcnt)
    bool changed = false;   // (wave-uniform)
    for (uint32_t j0 = 0; j0 < n_batch; j0 += 64) {
        const uint32_t j = j0 + (uint32_t)lane;
        const bool valid = j < n_batch;
        const uint32_t ord = first_ordinal + j;   // (the host keeps first_ordinal + n_batch - 1 <= 2^32-2)
        uint32_t o[WL];
        uint64_t v = 0, key = ~0ull;
        if (valid) {
            load_words<W>(slab + (base + j) * W, o);
            uint4 cc = make_uint4(0, 0, 0, 0);
            if constexpr (M == DST_TN93) {
                cc = t_counts[(uint64_t)w * n_batch + j];
                o[4] = cc.x, o[5] = cc.y, o[6] = cc.z, o[7] = cc.w;
            }
            v = pair_value<M>(o, qc, cc);
            key = nn_key<INT>(v);
        } else {
#pragma unroll
            for (int t = 0; t < WL; ++t)
                o[t] = 0;
        }
        const bool pass = valid && nn_less(key, ord, L.thr_key, L.thr_idx);
        const uint64_t mask = __ballot(pass);
        if (mask) {
            L.template offer<INT>(mask, pass, key, v, ord, o, k, lane);
            changed = true;
        }
    }
    if (!changed)
        return;
    L.template store<W>(lval, lidx, ltal, at, k, lane, lcnt);
}

}  // namespace

hipError_t launch_window_nearest_stream(int measure, const uint32_t *slab, const uint4 *q_counts, const uint4 *t_counts,
                                        uint64_t q_n, uint64_t n_batch, uint64_t row0, uint64_t nr, uint32_t win0, uint32_t nw,
                                        uint32_t n_windows, uint32_t first_ordinal, const NearestLists &nl, uint32_t *cnt,
                                        hipStream_t stream)
{
    const uint64_t lists = nr * nw;
    if (lists == 0 || n_batch == 0)
        return hipSuccess;
    if (q_n * n_windows > kWindowNearestListsMax || nl.k < 1 || nl.k > kNearestMaxK || n_batch > 0xFFFFFFFFull ||
        row0 + nr > q_n || (uint64_t)win0 + nw > n_windows || (uint64_t)first_ordinal + n_batch - 1 > 0xFFFFFFFEull ||
        (measure == DST_TN93 && (!cnt || !q_counts || !t_counts)))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((lists + 3) / 4);   // four waves (lists) per workgroup
#define DST_WNS(MEAS, W)                                                                                                          \
    hipLaunchKernelGGL((window_nearest_stream_kernel<MEAS, W>), dim3(blocks), dim3(256), 0, stream, slab, q_counts, t_counts,     \
                       (uint32_t)q_n, (uint32_t)n_batch, (uint32_t)row0, (uint32_t)nr, win0, nw, n_windows, first_ordinal, nl.val,  \
                       nl.idx, nl.tal, cnt, nl.k)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_WNS(DST_N_HIGH, 1); break;
    case DST_RAW: DST_WNS(DST_RAW, 2); break;
    case DST_JC69: DST_WNS(DST_JC69, 2); break;
    case DST_K80: DST_WNS(DST_K80, 3); break;
    case DST_TN93: DST_WNS(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_WNS
    return hipGetLastError();
}

}  // namespace dst
