// dst_window_nearest.hip — the k nearest records of every (row record, window) (dst_nearest_windows): the
// selection over one slab of window tallies that window_pair_kernel (dst_windows.hip) swept directly before it.
//
// The slab holds rows [row0, row0 + nr) x windows [win0, win0 + nw) x ALL n_cols column records as DST_OUT_TALLY words,
// entry (w_local nr + i_local) n_cols + j.  A square job is swept as the rectangle of slot 0 against itself (the tallies
// are symmetric in the two records), so a row's candidates j != i are all there: no column pass, and the whole
// candidate row of a list lies in the slab.
//
// Mapping (window_nearest_kernel): one wave per (row, window) list, four waves per workgroup, the lists linearised over
// grid.x (n_windows reaches 65,536, beyond a grid's y or z).  The lanes run along j, 64 candidates per step: an entry is
// W = dst_tally_width words, one 4 / 8 / 12 / 16-byte load per lane, contiguous across the wave.  The value comes through
// pair_value<M> (tn93: the per-window base counts of the canonical pair, swapped when square and j < i), the key through
// nn_key, and the list is WaveList's: it starts empty in registers and is stored once.  Every list entry has one writer.
#include "dst_device.hpp"
#include "dst_wavelist.hpp"

namespace dst {
namespace {

template <int M, int W>
__global__ __launch_bounds__(256) void window_nearest_kernel(const uint32_t *__restrict__ slab, const uint4 *__restrict__ q_counts,
                                                             const uint4 *__restrict__ t_counts, uint32_t q_n, uint32_t n_cols,
                                                             uint32_t row0, uint32_t nr, uint32_t win0, uint32_t nw, int square,
                                                             uint64_t *lval, uint32_t *lidx, uint32_t *ltal, uint32_t k)
{
    constexpr bool INT = M == DST_N_HIGH;
    const int lane = (int)(threadIdx.x & 63);
    // the wave's list (wave-uniform; the host keeps nr * nw <= 2^31)
    const uint32_t list = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if ((uint64_t)list >= (uint64_t)nr * nw)
        return;   // (whole waves)
    const uint32_t il = list / nw, wl = list % nw;
    const uint32_t i = row0 + il, w = win0 + wl;
    const uint64_t base = ((uint64_t)wl * nr + il) * n_cols;
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (M == DST_TN93)
        qc = q_counts[(uint64_t)w * q_n + i];
    WaveList<W> L;
    L.clear();
    for (uint64_t j0 = 0; j0 < n_cols; j0 += 64) {
        const uint64_t jw = j0 + (uint64_t)lane;
        const uint32_t j = (uint32_t)jw;
        const bool valid = jw < n_cols && !(square && j == i);
        uint32_t o[W];
        uint64_t v = 0, key = ~0ull;
        if (valid) {
            load_words<W>(slab + (base + j) * W, o);
            uint4 rc = qc, cc = make_uint4(0, 0, 0, 0);
            if constexpr (M == DST_TN93) {
                cc = t_counts[(uint64_t)w * n_cols + j];
                if (square && j < i) {   // the canonical pair (j, i): the counts in that order
                    rc = cc;
                    cc = qc;
                }
            }
            v = pair_value<M>(o, rc, cc);
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
    L.store(lval, lidx, ltal, (uint64_t)list * k, k, lane);
}

}  // namespace

hipError_t launch_window_nearest(int measure, const uint32_t *slab, const uint4 *q_counts, const uint4 *t_counts, uint64_t q_n,
                                 uint64_t n_cols, uint64_t row0, uint64_t nr, uint32_t win0, uint32_t nw, bool square,
                                 const NearestLists &nl, hipStream_t stream)
{
    const uint64_t lists = nr * nw;
    if (lists == 0 || n_cols == 0)
        return hipSuccess;
    if (lists > kWindowNearestListsMax || nl.k < 1 || nl.k > kNearestMaxK || q_n > 0xFFFFFFFFull || n_cols > 0xFFFFFFFFull ||
        row0 + nr > q_n)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((lists + 3) / 4);   // four waves (lists) per workgroup
#define DST_WN(MEAS, W)                                                                                                          \
    hipLaunchKernelGGL((window_nearest_kernel<MEAS, W>), dim3(blocks), dim3(256), 0, stream, slab, q_counts, t_counts, (uint32_t)q_n, \
                       (uint32_t)n_cols, (uint32_t)row0, (uint32_t)nr, win0, nw, square ? 1 : 0, nl.val, nl.idx, nl.tal, nl.k)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_WN(DST_N_HIGH, 1); break;
    case DST_RAW: DST_WN(DST_RAW, 2); break;
    case DST_JC69: DST_WN(DST_JC69, 2); break;
    case DST_K80: DST_WN(DST_K80, 3); break;
    case DST_TN93: DST_WN(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_WN
    return hipGetLastError();
}

}  // namespace dst
