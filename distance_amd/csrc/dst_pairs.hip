// dst_pairs.hip — the distances of a list of pairs the caller names (dst_run_pairs): the kernels of its two
// routes.  The call itself (checks, batching, the route rule) is in dst_analysis.cpp.
//
// Direct route (pairs_direct_kernel): a gather over the planes of the two records of every pair, through the dense pair
// kernel's own steps: M::step per 32 sites, M::tallies, finalize_pair.  Nothing here is a second arithmetic, so an entry is
// bitwise what pair_kernel (dst_kernels.hip) writes for the pair.
//
//   total   M::tallies is handed the number of sites the sweep covered INCLUDING the pack's N padding, nchunks x 128, never
//           len: the padded sites are N on both sides, the steps count them as "sharing a base", and n / n_high / raw
//           subtract the shared sites from it.  This is pair_kernel's `total` of an unsplit launch ((c_end - c_begin) x
//           kChunkSites with c_begin = 0, c_end = nchunks).
//
//   mapping A group of G = 2^lg consecutive lanes serves one pair, G chosen by the launcher from nchunks (pairs_lanes:
//           the smallest power of two that covers the chunks, at most 64), so a 1,000-site alignment (8 chunks) keeps all
//           64 lanes of a wave busy with 8 pairs.  Lane g of the group takes chunks g, g + G, ...; the partial popcounts
//           meet in lane 0 of the group by shuffles (groups are aligned, so a shuffle never leaves the wave); that lane runs
//           the epilogue and writes.  One writer per entry, plain vector stores.  dst_pair_sites' count kernel is the
//           G = 64 case of this mapping with a different step.
//
//   memory  The planes are record-minor, planes[(plane x nchunks + chunk) x npad + record]: a lane's 16 bytes of a
//           (plane, chunk) are alone in their 128-byte line unless another lane wants a record within 8 of it.  An unsorted
//           list moves about 2 x NP x nchunks lines per pair and uses an eighth of each; a list sorted by (row, col) shares
//           the row record's lines between neighbouring groups.
//
// Sweep route (pairs_gather_kernel): behind a row slab's pair kernel, entry k of the batch is slab entry pos[k], copied as
// it is (a DST_OUT_DISTANCE slab) or as its tally words, with the value finalised from them by pair_value (a
// DST_OUT_TALLY slab: when the tallies are wanted, alone or with the values).
#include "dst_device.hpp"
#include "dst_measures.hpp"

namespace dst {
namespace {

constexpr int kPairsThreads = 256;

__device__ __forceinline__ uint32_t word_at(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// VAL: OUT_TALLY (no value is written), OUT_INT, or the measure id whose f64 the epilogue writes (as pair_kernel's OUT);
// tallies may be NULL unless VAL == OUT_TALLY
template <class M, int VAL>
__global__ __launch_bounds__(kPairsThreads) void pairs_direct_kernel(
    const uint4 *__restrict__ qpl, const uint4 *__restrict__ tpl, const uint32_t *__restrict__ row, const uint32_t *__restrict__ col,
    uint32_t pairs, uint32_t lg, uint64_t *__restrict__ values, uint32_t *__restrict__ tallies, const uint4 *__restrict__ q_counts,
    const uint4 *__restrict__ t_counts, uint32_t nchunks, uint32_t q_npad, uint32_t t_npad)
{
    constexpr int NP = M::NP, NC = M::NC, NT = M::NT;
    const uint32_t G = 1u << lg;
    const uint32_t t = blockIdx.x * kPairsThreads + threadIdx.x;   // (pairs x G <= 2^26)
    const uint32_t e = t >> lg, g = t & (G - 1u);
    const uint32_t el = e < pairs ? e : pairs - 1u;   // a group past the last pair sweeps the last one and stores nothing
    const uint32_t i = row[el], j = col[el];

    uint32_t acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k)
        acc[k] = 0;
    const size_t q_ps = (size_t)nchunks * q_npad, t_ps = (size_t)nchunks * t_npad;   // plane strides, in uint4
    const uint4 *qbase = qpl + (size_t)M::P0 * q_ps + i;
    const uint4 *tbase = tpl + (size_t)M::P0 * t_ps + j;
#pragma unroll 1
    for (uint32_t c = g; c < nchunks; c += G) {
        uint4 qv[NP], tv[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            qv[p] = qbase[(size_t)p * q_ps + (size_t)c * q_npad];
            tv[p] = tbase[(size_t)p * t_ps + (size_t)c * t_npad];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t q[NP], w[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                q[p] = word_at(qv[p], k);
                w[p] = word_at(tv[p], k);
            }
            M::step(acc, q, w);
        }
    }
    for (uint32_t off = G >> 1; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < NC; ++k)
            acc[k] += (uint32_t)__shfl_down((int)acc[k], off, 64);
    if (g != 0 || e >= pairs)
        return;
    const uint32_t total = nchunks * kChunkSites;   // pair_kernel's: the padded sites count, see the head of the file
    uint32_t o[NT];
    M::tallies(acc, total, o);
    if (tallies) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            tallies[(size_t)e * NT + k] = o[k];
    }
    if constexpr (VAL == OUT_INT) {
        values[e] = (uint64_t)(int64_t)o[0];
    } else if constexpr (VAL >= 0) {
        uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
        if constexpr (VAL == DST_TN93) {
            qc = q_counts[i];
            tc = t_counts[j];
        }
        values[e] = (uint64_t)__double_as_longlong(finalize_pair<VAL>(o, qc, tc));
    }
}

// MEASURE: DST_N_HIGH for both integer measures.  TALLY: the slab holds W DST_OUT_TALLY words per entry, else payloads.
template <int MEASURE, bool TALLY>
__global__ __launch_bounds__(kPairsThreads) void pairs_gather_kernel(const void *__restrict__ slab, const uint64_t *__restrict__ pos,
                                                                     const uint32_t *__restrict__ row, const uint32_t *__restrict__ col,
                                                                     uint32_t pairs, uint64_t *__restrict__ values,
                                                                     uint32_t *__restrict__ tallies, const uint4 *__restrict__ q_counts,
                                                                     const uint4 *__restrict__ t_counts)
{
    constexpr int W = MEASURE == DST_N_HIGH ? 1 : MEASURE == DST_K80 ? 3 : MEASURE == DST_TN93 ? 4 : 2;
    const uint32_t k = blockIdx.x * kPairsThreads + threadIdx.x;
    if (k >= pairs)
        return;
    const uint64_t at = pos[k];
    if constexpr (!TALLY) {
        values[k] = static_cast<const uint64_t *>(slab)[at];
    } else {
        const uint32_t *p = static_cast<const uint32_t *>(slab) + at * W;
        uint32_t o[W];
#pragma unroll
        for (int t = 0; t < W; ++t)
            o[t] = p[t];
        if (tallies) {
#pragma unroll
            for (int t = 0; t < W; ++t)
                tallies[(size_t)k * W + t] = o[t];
        }
        if (values) {
            uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
            if constexpr (MEASURE == DST_TN93) {
                qc = q_counts[row[k]];
                tc = t_counts[col[k]];
            }
            values[k] = pair_value<MEASURE>(o, qc, tc);
        }
    }
}

template <class M, int VAL>
hipError_t launch_direct_one(const PairsLaunch &pl, uint32_t lg, hipStream_t stream)
{
    const uint64_t threads = (uint64_t)pl.pairs << lg;
    hipLaunchKernelGGL((pairs_direct_kernel<M, VAL>), dim3((unsigned)((threads + kPairsThreads - 1) / kPairsThreads)),
                       dim3(kPairsThreads), 0, stream, pl.rows->planes, pl.cols->planes, pl.row, pl.col, pl.pairs, lg, pl.values,
                       pl.tallies, reinterpret_cast<const uint4 *>(pl.q_counts), reinterpret_cast<const uint4 *>(pl.t_counts),
                       (uint32_t)pl.rows->nchunks, (uint32_t)pl.rows->npad, (uint32_t)pl.cols->npad);
    return hipGetLastError();
}

template <int MEASURE>
hipError_t launch_gather_one(const PairsLaunch &pl, const void *slab, bool tally, hipStream_t stream)
{
    const dim3 grid((pl.pairs + kPairsThreads - 1) / kPairsThreads);
    const uint4 *qc = reinterpret_cast<const uint4 *>(pl.q_counts), *tc = reinterpret_cast<const uint4 *>(pl.t_counts);
    if (tally)
        hipLaunchKernelGGL((pairs_gather_kernel<MEASURE, true>), grid, dim3(kPairsThreads), 0, stream, slab, pl.pos, pl.row, pl.col,
                           pl.pairs, pl.values, pl.tallies, qc, tc);
    else
        hipLaunchKernelGGL((pairs_gather_kernel<MEASURE, false>), grid, dim3(kPairsThreads), 0, stream, slab, pl.pos, pl.row, pl.col,
                           pl.pairs, pl.values, pl.tallies, qc, tc);
    return hipGetLastError();
}

}  // namespace

uint32_t pairs_lanes(uint64_t nchunks)
{
    uint32_t g = 1;
    while (g < 64 && g < nchunks)
        g <<= 1;
    return g;
}

hipError_t launch_pairs_direct(int measure, const PairsLaunch &pl, hipStream_t stream, uint32_t *lanes)
{
    const DeviceSet &rows = *pl.rows, &cols = *pl.cols;
    if (pl.pairs == 0 || pl.pairs > DST_RUN_PAIRS_BATCH || (!pl.values && !pl.tallies) || rows.nchunks != cols.nchunks ||
        rows.nchunks == 0 || rows.len != cols.len || rows.len > 0xFFFFFFFFull || rows.npad > 0xFFFFFFFFull || cols.npad > 0xFFFFFFFFull ||
        (measure == DST_TN93 && pl.values && (!pl.q_counts || !pl.t_counts)))
        return hipErrorInvalidValue;
    const uint32_t G = pairs_lanes(rows.nchunks);
    uint32_t lg = 0;
    while ((1u << lg) < G)
        ++lg;
    if (lanes)
        *lanes = G;
    const bool val = pl.values != nullptr;
    switch (measure) {
    case DST_N:
    case DST_N_HIGH:
        return val ? launch_direct_one<MNHigh, OUT_INT>(pl, lg, stream) : launch_direct_one<MNHigh, OUT_TALLY>(pl, lg, stream);
    case DST_RAW: return val ? launch_direct_one<MRaw, DST_RAW>(pl, lg, stream) : launch_direct_one<MRaw, OUT_TALLY>(pl, lg, stream);
    case DST_JC69: return val ? launch_direct_one<MRaw, DST_JC69>(pl, lg, stream) : launch_direct_one<MRaw, OUT_TALLY>(pl, lg, stream);
    case DST_K80: return val ? launch_direct_one<MK80, DST_K80>(pl, lg, stream) : launch_direct_one<MK80, OUT_TALLY>(pl, lg, stream);
    case DST_TN93: return val ? launch_direct_one<MTN93, DST_TN93>(pl, lg, stream) : launch_direct_one<MTN93, OUT_TALLY>(pl, lg, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pairs_gather(int measure, const PairsLaunch &pl, const void *slab, bool tally, hipStream_t stream)
{
    if (pl.pairs == 0 || pl.pairs > DST_RUN_PAIRS_BATCH || !slab || !pl.pos || (!pl.values && !pl.tallies) ||
        (!tally && (!pl.values || pl.tallies)) || (tally && measure == DST_TN93 && pl.values && (!pl.q_counts || !pl.t_counts)))
        return hipErrorInvalidValue;
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: return launch_gather_one<DST_N_HIGH>(pl, slab, tally, stream);
    case DST_RAW: return launch_gather_one<DST_RAW>(pl, slab, tally, stream);
    case DST_JC69: return launch_gather_one<DST_JC69>(pl, slab, tally, stream);
    case DST_K80: return launch_gather_one<DST_K80>(pl, slab, tally, stream);
    case DST_TN93: return launch_gather_one<DST_TN93>(pl, slab, tally, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace dst
