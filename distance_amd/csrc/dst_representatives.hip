// dst_representatives.hip — greedy representatives of one set (dst_representatives): the lexicographically first maximal
// independent set of the dst_links(T) graph, built in one sweep of the triangle in row slabs.
//
// Definition.  Records i < j are linked by dst_clusters' rule (nn_key(v) <= nn_key(T) on the pair's DST_OUT_DISTANCE
// payload v).  Record j is a representative iff no representative i < j is linked to it; rep[j] = j then, otherwise the
// smallest representative linked to j.
//
// State: rep[n], 2^32-1 = unset.  Slabs arrive in ascending row order, and a slab's rows are cut into sub-blocks of
// kRepBlockRows rows, taken in order.  When sub-block [s0, s1) is entered every representative below s0 has lowered the
// rep of every record it is linked to, so a row whose rep is still unset is linked to no earlier representative, and
// the only dependence left is among the sub-block's own rows.
//
//   rep_bits_kernel      once per slab, wide: a wave per row reads the row's entries inside its own sub-block's diagonal block
//                        (i, j), s0 <= i < j < s1, tests them and writes the row's 16 link words (512 bits, bit j - s0) to
//                        the call's bit table.  The bits do not depend on rep, so every sub-block of the slab is served by
//                        the one launch: n x 256 entries a call on average, read by the whole device.
//   rep_resolve_kernel   per sub-block, ONE workgroup: the sub-block's 32 KiB of link words into LDS (16 independent
//                        coalesced loads per thread) and which of its rows are set already; then wave 0 walks the rows in
//                        order with the covered mask in 16 lanes' registers: a row that is not covered is a representative
//                        and ORs its 16 link words into the mask.  Last, rep[i] = i for the new representatives.  32 KiB
//                        and 512 steps over LDS and registers, whatever the number of representatives; it never touches
//                        the slab.
//   rep_cover_kernel     clusters_link_kernel's geometry over the sub-block's rows, in the slab and beyond the diagonal
//                        block: workgroup (x, row) leaves at once unless rep[row] == row; else it tests entries
//                        2048 x .. 2048 x + 2047 of its row and lowers rep[j] to the row with a 32-bit atomic min for every
//                        link (skipped when rep[j] is seen below the row already: values only ever decrease).
//   rep_values_kernel    the same geometry, behind the cover launch: where rep[j] == row the pair (row, j) is the one whose
//                        value and tallies are record j's.  rep[j] == row implies the link, so nothing is tested, and the
//                        slab is read for the winners only.  A pass of its own: inside the cover launch a larger
//                        representative of the sub-block can win the atomic first and be lowered later.
//   rep_final_kernel     behind the last slab: a record that is still unset is its own representative (the last record
//                        belongs to no slab: it has no row)
//
// The slab is DST_OUT_DISTANCE payloads, or DST_OUT_TALLY words when the caller wants tallies: then the payload is
// entry_value's pair_value<M> of the tallies, bitwise what a distance run returns (as dst_links.hip).
// Every write to rep after the initial fill is an agent-scope atomic (a store in resolve and final, a min in cover) and
// every read a relaxed agent-scope atomic load; launches are ordered by the stream.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr uint32_t kRepUnset = 0xFFFFFFFFu;
constexpr int kRepWords = (int)kRepBlockRows / 32;                // link words per row of the diagonal block
constexpr int kRepResolveWaves = 8;
constexpr int kRepSteps = 8;                                      // 64-entry steps per wave of the wide kernels
constexpr uint32_t kRepWavePairs = 64u * kRepSteps;
constexpr int kRepWaves = 4;
constexpr uint32_t kRepBlockPairs = kRepWavePairs * kRepWaves;    // 2048 entries of one row per workgroup
static_assert(kRepBlockRows == 64u * kRepSteps, "a wave's eight steps span the diagonal block's columns");
static_assert(kRepWords == 2 * kRepSteps, "a step's ballot is two of the row's link words");
static_assert(kRepBlockRows == 64u * kRepResolveWaves, "one resolve thread per row for the masks");
static_assert(kRepBlockRows % 32 == 0, "the serial loop's groups of 32 rows tile the sub-block");
static_assert(kRepWords <= 64, "the covered mask lives in one wave's lanes");

__device__ __forceinline__ uint32_t rep_load(const uint32_t *rep, uint32_t x)
{
    return __hip_atomic_load(rep + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Rows [rb, re) of the slab, wave w of workgroup x row rb + 4 x + w; entry (i, j) at slab index tri_row_start(n, i) - out_base
// + j - i - 1.  The row's sub-block is the run of kRepBlockRows rows from rb that holds it; word k of the row's 16 at
// bits[(i - rb) * 16 + k], bit b of it column s0 + 32 k + b.
template <int M, int W, bool TALLY>
__global__ __launch_bounds__(64 * kRepWaves) void rep_bits_kernel(const void *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                                 uint32_t rb, uint32_t re, uint64_t t_bits,
                                                                 const uint32_t *__restrict__ counts, uint32_t *__restrict__ bits)
{
    constexpr bool INT = M == DST_N_HIGH;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint64_t r = (uint64_t)blockIdx.x * kRepWaves + (uint32_t)wave;
    if (r >= re - rb)
        return;   // (whole waves; no barrier below)
    const uint32_t i = rb + (uint32_t)r;
    const uint32_t s0 = rb + (uint32_t)r / kRepBlockRows * kRepBlockRows, li = i - s0;
    const uint32_t rows = min(kRepBlockRows, re - s0);
    const uint64_t base = tri_row_start(n, i) - out_base;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (TALLY && M == DST_TN93)
        qc = reinterpret_cast<const uint4 *>(counts)[i];
    uint64_t v[kRepSteps];
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        const uint32_t lj = (uint32_t)(t * 64 + lane);
        v[t] = lj > li && lj < rows ? entry_value<M, W, TALLY>(slab, base + (lj - li - 1), qc, counts, s0 + lj) : 0;
    }
    uint32_t word = 0;   // lane k < 16: word k of the row
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        const uint32_t lj = (uint32_t)(t * 64 + lane);
        const uint64_t m = __ballot(lj > li && lj < rows && nn_key<INT>(v[t]) <= t_key);
        if ((lane >> 1) == t)
            word = (lane & 1) ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
    if (lane < kRepWords)
        bits[r * kRepWords + (uint32_t)lane] = word;
}

// Rows [s0, s1) of the slab that begins at row rb, s1 - s0 <= kRepBlockRows; their link words from rep_bits_kernel.
__global__ __launch_bounds__(64 * kRepResolveWaves) void rep_resolve_kernel(const uint32_t *__restrict__ bits_all, uint32_t rb,
                                                                           uint32_t s0, uint32_t s1, uint32_t *rep)
{
    __shared__ uint32_t bits[kRepBlockRows * kRepWords];
    __shared__ uint32_t was_set[kRepWords], fresh[kRepWords];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t rows = s1 - s0;
    {
        const uint32_t li = threadIdx.x;   // (one thread per row)
        const uint64_t m = __ballot(li < rows && rep_load(rep, s0 + li) != kRepUnset);
        if (lane == 0) {
            was_set[2 * wave] = (uint32_t)m;
            was_set[2 * wave + 1] = (uint32_t)(m >> 32);
        }
    }
    const uint32_t *mine_bits = bits_all + (uint64_t)(s0 - rb) * kRepWords;
    // every load before the first store, none under a branch (a short last sub-block reads its last word again): one
    // round trip to memory instead of sixteen
    uint32_t fetched[kRepWords];
#pragma unroll
    for (int q = 0; q < kRepWords; ++q)
        fetched[q] = mine_bits[min((uint32_t)q * kRepBlockRows + threadIdx.x, rows * kRepWords - 1)];
#pragma unroll
    for (int q = 0; q < kRepWords; ++q)
        bits[(uint32_t)q * kRepBlockRows + threadIdx.x] = fetched[q];
    __syncthreads();
    if (wave == 0) {
        // The serial part, 32 rows (one word of the masks) at a time.  Lane w < kRepWords holds word w of the covered mask
        // and of the new representatives, and of each of the group's 32 rows, fetched from LDS one group ahead.  Inside a
        // group only the group's own word of the mask decides, so that word lives in a scalar register: a step is a bit
        // test and an OR of the row's own-group word (a lane read that does not wait for the step before) on the scalar
        // unit; the 16-lane OR into the whole mask follows off the chain.
        const int w = lane < kRepWords ? lane : 0;
        const uint32_t keep = lane < kRepWords ? ~0u : 0u;
        uint32_t covered = was_set[w] & keep, mine = 0;
        uint32_t ahead[32];
#pragma unroll
        for (int u = 0; u < 32; ++u)
            ahead[u] = bits[u * kRepWords + w] & keep;
        for (uint32_t wb = 0; wb * 32 < rows; ++wb) {
            uint32_t row[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                row[u] = ahead[u];
                ahead[u] = bits[min(wb * 32 + 32 + (uint32_t)u, kRepBlockRows - 1) * kRepWords + (uint32_t)w] & keep;
            }
            uint32_t cw = (uint32_t)__builtin_amdgcn_readlane((int)covered, (int)wb), mw = 0;   // (wb is uniform)
#pragma unroll
            for (int u = 0; u < 32; ++u) {
                const uint32_t own = (uint32_t)__builtin_amdgcn_readlane((int)row[u], (int)wb);
                // a row that is covered is linked to an earlier representative: its links cover nothing
                const bool take = wb * 32 + (uint32_t)u < rows && !((cw >> u) & 1u);
                cw |= take ? own : 0u;
                mw |= take ? 1u << u : 0u;
                covered |= take ? row[u] : 0u;
            }
            if (lane == (int)wb)
                mine = mw;
        }
        if (lane < kRepWords)
            fresh[lane] = mine;
    }
    __syncthreads();
    const uint32_t li = threadIdx.x;
    if (li < rows && ((fresh[li >> 5] >> (li & 31)) & 1u))
        __hip_atomic_store(rep + s0 + li, s0 + li, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup (x, y): entries 2048 x .. 2048 x + 2047 of row s0 + y, wave w the 512 from 512 w, lane l of step t entry
// 512 w + 64 t + l: column record row + 1 + entry.
template <int M, int W, bool TALLY>
__global__ __launch_bounds__(64 * kRepWaves) void rep_cover_kernel(const void *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                                  uint32_t s0, uint32_t s1, uint64_t t_bits,
                                                                  const uint32_t *__restrict__ counts, uint32_t *rep)
{
    constexpr bool INT = M == DST_N_HIGH;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = s0 + blockIdx.y;
    if (i >= s1)
        return;   // (whole workgroups)
    const uint64_t row_pairs = n - i - 1;
    if ((uint64_t)blockIdx.x * kRepBlockPairs >= row_pairs)
        return;   // (whole workgroups)
    if (rep_load(rep, i) != i)
        return;   // (whole workgroups) a member's row is not read
    const uint64_t q0 = (uint64_t)blockIdx.x * kRepBlockPairs + (uint32_t)wave * kRepWavePairs;
    const uint64_t base = tri_row_start(n, i) - out_base;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (TALLY && M == DST_TN93)
        qc = reinterpret_cast<const uint4 *>(counts)[i];
    uint64_t v[kRepSteps];
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        v[t] = q < row_pairs ? entry_value<M, W, TALLY>(slab, base + q, qc, counts, i + 1 + (uint32_t)q) : 0;
    }
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        if (q < row_pairs && nn_key<INT>(v[t]) <= t_key) {
            const uint32_t j = i + 1 + (uint32_t)q;
            if (rep_load(rep, j) > i)   // (possibly stale, then larger than the truth: the min below decides)
                __hip_atomic_fetch_min(rep + j, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the geometry of rep_cover_kernel; val, tal: NULL when not wanted (tal: TALLY slabs only)
template <int M, int W, bool TALLY>
__global__ __launch_bounds__(64 * kRepWaves) void rep_values_kernel(const void *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                                   uint32_t s0, uint32_t s1, const uint32_t *__restrict__ counts,
                                                                   const uint32_t *rep, uint64_t *__restrict__ val,
                                                                   uint32_t *__restrict__ tal)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = s0 + blockIdx.y;
    if (i >= s1)
        return;   // (whole workgroups)
    const uint64_t row_pairs = n - i - 1;
    if ((uint64_t)blockIdx.x * kRepBlockPairs >= row_pairs)
        return;   // (whole workgroups)
    if (rep_load(rep, i) != i)
        return;   // (whole workgroups)
    const uint64_t q0 = (uint64_t)blockIdx.x * kRepBlockPairs + (uint32_t)wave * kRepWavePairs;
    const uint64_t base = tri_row_start(n, i) - out_base;
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (TALLY && M == DST_TN93)
        qc = reinterpret_cast<const uint4 *>(counts)[i];
    uint32_t r[kRepSteps];
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        r[t] = q < row_pairs ? rep_load(rep, i + 1 + (uint32_t)q) : kRepUnset;
    }
#pragma unroll
    for (int t = 0; t < kRepSteps; ++t) {
        if (r[t] != i)
            continue;
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        const uint32_t j = i + 1 + (uint32_t)q;
        if (val)
            val[j] = entry_value<M, W, TALLY>(slab, base + q, qc, counts, j);
        if constexpr (TALLY) {
            if (tal) {
                const uint32_t *p = static_cast<const uint32_t *>(slab) + (base + q) * W;
#pragma unroll
                for (int k = 0; k < W; ++k)
                    tal[(uint64_t)j * W + k] = p[k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void rep_final_kernel(uint32_t *rep, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && rep_load(rep, i) == kRepUnset)
        __hip_atomic_store(rep + i, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_rep_slab(int measure, bool tally, const void *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                           uint64_t t_bits, const uint32_t *counts, const RepBuffers &b, hipStream_t stream)
{
    if (re <= rb || re > n || (b.tal && !tally))
        return hipErrorInvalidValue;
    if (rb + 1 >= n)
        return hipSuccess;   // (no pair: rep_final_kernel settles the last record)
    const bool wanted = b.val || b.tal;
    const dim3 bits_grid((unsigned)((re - rb + kRepWaves - 1) / kRepWaves));
    // the slab's link bits, then its sub-blocks in order; `grid`: row s0's chunks (the longest row) x the sub-block's rows
#define DST_REP_SLAB(MEAS, W, TAL)                                                                                                \
    do {                                                                                                                          \
        hipLaunchKernelGGL((rep_bits_kernel<MEAS, W, TAL>), bits_grid, dim3(64 * kRepWaves), 0, stream, slab, out_base,            \
                           (uint32_t)n, (uint32_t)rb, (uint32_t)re, t_bits, counts, b.bits);                                      \
        for (uint64_t s0 = rb; s0 < re && s0 + 1 < n; s0 += kRepBlockRows) {                                                      \
            const uint64_t s1 = std::min<uint64_t>(re, s0 + kRepBlockRows);                                                       \
            const dim3 grid((unsigned)((n - s0 - 1 + kRepBlockPairs - 1) / kRepBlockPairs), (unsigned)(s1 - s0));                 \
            hipLaunchKernelGGL(rep_resolve_kernel, dim3(1), dim3(64 * kRepResolveWaves), 0, stream, b.bits, (uint32_t)rb,         \
                               (uint32_t)s0, (uint32_t)s1, b.rep);                                                                \
            hipLaunchKernelGGL((rep_cover_kernel<MEAS, W, TAL>), grid, dim3(64 * kRepWaves), 0, stream, slab, out_base,           \
                               (uint32_t)n, (uint32_t)s0, (uint32_t)s1, t_bits, counts, b.rep);                                   \
            if (wanted)                                                                                                           \
                hipLaunchKernelGGL((rep_values_kernel<MEAS, W, TAL>), grid, dim3(64 * kRepWaves), 0, stream, slab, out_base,      \
                                   (uint32_t)n, (uint32_t)s0, (uint32_t)s1, counts, b.rep, b.val, b.tal);                         \
        }                                                                                                                         \
    } while (0)
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    if (!tally) {
        if (int_payload)
            DST_REP_SLAB(DST_N_HIGH, 1, false);
        else
            DST_REP_SLAB(DST_RAW, 2, false);   // (any f64 measure: the payload is read, not computed)
    } else {
        switch (measure) {
        case DST_N:
        case DST_N_HIGH: DST_REP_SLAB(DST_N_HIGH, 1, true); break;
        case DST_RAW: DST_REP_SLAB(DST_RAW, 2, true); break;
        case DST_JC69: DST_REP_SLAB(DST_JC69, 2, true); break;
        case DST_K80: DST_REP_SLAB(DST_K80, 3, true); break;
        case DST_TN93: DST_REP_SLAB(DST_TN93, 4, true); break;
        default: return hipErrorInvalidValue;
        }
    }
#undef DST_REP_SLAB
    return hipGetLastError();
}

hipError_t launch_rep_final(uint32_t *rep, uint64_t n, hipStream_t stream)
{
    const unsigned blocks = (unsigned)std::max<uint64_t>((n + 255) / 256, 1);
    hipLaunchKernelGGL(rep_final_kernel, dim3(blocks), dim3(256), 0, stream, rep, (uint32_t)n);
    return hipGetLastError();
}

}  // namespace dst
