// dst_window_sweep.hpp — the sweep of one window tile, shared by the kernels that run it:
// window_pair_kernel (dst_windows.hip), which stores a tile's tallies or payloads, and window_summary_kernel
// (dst_window_summary.hip), which reduces them on chip.
//
// A tile is kWinRows row records x kWinCols column records x one window [wb, we).  The lanes run along the column
// records: a lane's 16 bytes of a (plane, chunk) are contiguous with its neighbours' and stay in VGPRs for all the rows
// of the tile.  A row record's 16 bytes are the same for the whole block: wave-uniform loads.
//
// The mask rule.  n / n_high / raw count the sites whose base sets SHARE a member and subtract from `total`; so a site
// outside the window is taken out of the counted word, and total = end - begin (never the chunks' span).  Zeroing a
// record's planes instead would make its masked sites certain differences.  k80 / tn93 count known sites only: every
// counted word derives from one that the mask went into.
#pragma once
#include "dst_device.hpp"
#include "dst_measures.hpp"

namespace dst {
namespace {

constexpr int kWinRows = 8;          // row records of one block
constexpr int kWinCols = 256;        // column records of one block: one per thread

__device__ __forceinline__ uint32_t bits_below(uint32_t x) { return x >= 32u ? 0xFFFFFFFFu : (1u << x) - 1u; }

// the sites of chunk c inside [begin, end), one bit per site (wave-uniform: SALU)
__device__ __forceinline__ void window_mask(uint32_t c, uint32_t begin, uint32_t end, uint32_t (&m)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t ws = (uint64_t)c * kChunkSites + 32u * k;   // the word's first site
        const uint32_t lo = begin <= ws ? 0u : begin - ws >= 32u ? 32u : (uint32_t)(begin - ws);
        const uint32_t hi = end <= ws ? 0u : end - ws >= 32u ? 32u : (uint32_t)(end - ws);
        m[k] = bits_below(hi) & ~bits_below(lo);   // (lo >= hi: empty)
    }
}

// M::step with the sites outside m left out of every counted word
template <class M>
struct Masked;
template <>
struct Masked<MNHigh> {
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t, uint32_t m)
    {
        bcnt_acc(a[0], share_bits(q, t) & m);
    }
};
template <>
struct Masked<MRaw> {
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t, uint32_t m)
    {
        const uint32_t share = share_bits(q, t) & m;
        bcnt_acc(a[0], share);
        bcnt_acc(a[1], bitop3<TT_AND3>(share, q[4], t[4]));
    }
};
template <>
struct Masked<MK80> {
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t, uint32_t m)
    {
        const uint32_t e1 = q[1] ^ t[1];
        const uint32_t sc = bitop3<TT_A_AND_B_ANDN_C>(q[0] & m, t[0], e1);   // (q and m are scalars: the AND is SALU)
        const uint32_t ts = bitop3<TT_A_AND_B_NE_C>(sc, q[2], t[2]);
        const uint32_t tv = bitop3<TT_AND3>(q[3] & m, t[3], e1);
        bcnt_acc(a[0], sc);
        bcnt_acc(a[1], ts);
        bcnt_acc(a[2], tv);
    }
};
template <>
struct Masked<MTN93> {
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t, uint32_t m)
    {
        const uint32_t bk = bitop3<TT_AND3>(q[0], t[0], m);
        const uint32_t sc = bitop3<TT_A_AND_B_EQ_C>(bk, q[1], t[1]);
        const uint32_t ts = bitop3<TT_A_AND_B_NE_C>(sc, q[2], t[2]);
        const uint32_t p2 = ts & q[1];
        bcnt_acc(a[0], bk);
        bcnt_acc(a[1], sc);
        bcnt_acc(a[2], ts);
        bcnt_acc(a[3], p2);
    }
};

__device__ __forceinline__ uint32_t word_of(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// acc[r][] += the counts of rows i0 + r (clamped below row_end: a row past the end repeats the last one) against the
// lane's column over the 128-site chunks window [wb, we) meets; qbase: the row set's plane M::P0, tbase: the column
// set's, at the lane's column.  The at most two chunks the window's edges cut are masked.
template <class M>
__device__ __forceinline__ void window_sweep(uint32_t (&acc)[kWinRows][M::NC], const uint4 *__restrict__ qbase,
                                             const uint4 *__restrict__ tbase, size_t q_ps, size_t t_ps, uint32_t q_npad,
                                             uint32_t t_npad, uint32_t i0, uint32_t row_end, uint32_t wb, uint32_t we)
{
    constexpr int NP = M::NP;
    if (we > wb) {
        const uint32_t c_first = wb / kChunkSites, c_last = (we - 1u) / kChunkSites;
#pragma unroll 1
        for (uint32_t c = c_first; c <= c_last; ++c) {
            uint4 tv[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p)
                tv[p] = tbase[(size_t)p * t_ps + (size_t)c * t_npad];
            const bool whole = (uint64_t)c * kChunkSites >= wb && (uint64_t)c * kChunkSites + kChunkSites <= we;
            if (whole) {
#pragma unroll
                for (int r = 0; r < kWinRows; ++r) {
                    const uint32_t i = i0 + r < row_end ? i0 + r : row_end - 1u;   // (wave-uniform)
                    uint4 qv[NP];
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        qv[p] = qbase[(size_t)p * q_ps + (size_t)c * q_npad + i];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t q[NP], t[NP];
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            q[p] = word_of(qv[p], k);
                            t[p] = word_of(tv[p], k);
                        }
                        M::step(acc[r], q, t);
                    }
                }
            } else {
                uint32_t m[4];
                window_mask(c, wb, we, m);
#pragma unroll
                for (int r = 0; r < kWinRows; ++r) {
                    const uint32_t i = i0 + r < row_end ? i0 + r : row_end - 1u;
                    uint4 qv[NP];
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        qv[p] = qbase[(size_t)p * q_ps + (size_t)c * q_npad + i];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t q[NP], t[NP];
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            q[p] = word_of(qv[p], k);
                            t[p] = word_of(tv[p], k);
                        }
                        Masked<M>::step(acc[r], q, t, m[k]);
                    }
                }
            }
        }
    }
}

}  // namespace
}  // namespace dst
