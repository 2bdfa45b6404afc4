// dst_links.hip — the pairs within a threshold (dst_links): an order-preserving stream compaction of one row slab at a
// time, so the links come out in canonical pair order without a sort.
//
// Definition.  A pair is a link when its DST_OUT_DISTANCE payload v satisfies dst_clusters' rule against T:
// nn_key(v) <= nn_key(T) (int64: v <= floor(T), clamped by the host; f64: IEEE v <= T, NaN never, -0.0 as +0.0).
//
//   links_count_kernel   the geometry of clusters_link_kernel: workgroup (x, row) takes entries 2048 x .. 2048 x + 2047 of
//                        its row (wave w the 512 from 512 w, lane l of step t entry 512 w + 64 t + l), tests them and
//                        writes ONE count, at block number (row - rb) * chunks + x: the blocks are numbered in canonical
//                        order, row-major, then run within the row.  A block past its row's end counts 0.
//   links_scan_kernel    one workgroup: the exclusive scan of the block counts into 64-bit offsets, offsets[blocks] = the
//                        slab's total, which is also added to the call's running total
//   links_write_kernel   a rank window [lo, hi): a block whose [offset, offset + count) does not meet it leaves after
//                        reading its two offsets; any other repeats the test, ranks its links (per step a __ballot and
//                        the __popcll of the lanes below, the steps of a wave in order, the waves' totals through LDS:
//                        rank order is entry order) and writes row, col and what was asked for at offset + rank - lo.
//                        Plain vector stores; two links never share a place, so the output's order is entry order.
//   links_stream_header_kernel   a links stream's batch: the slab's total beside the bad-code word (one thread)
//
// The slab is DST_OUT_DISTANCE payloads (8 B per pair), or DST_OUT_TALLY words when the caller wants the links' tallies:
// then the payload is pair_value<M> of the tallies, the arithmetic of the pair kernels' epilogue, bitwise what a
// distance run returns (as dst_nearest.hip).
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kLinkWaves = 4;                                          // waves per workgroup
constexpr int kLinkSteps = 8;                                          // 64-entry steps per wave
constexpr uint32_t kLinkWavePairs = 64u * kLinkSteps;                  // 512 entries: one wave's run
constexpr uint32_t kLinkBlockPairs = kLinkWavePairs * kLinkWaves;      // 2048 entries of one row per workgroup
constexpr int kScanThreads = 1024;

struct LinkRows {
    uint64_t out_base;   // canonical index of the slab's first pair (square)
    uint32_t n_cols;     // square: n
    uint32_t rb, re;     // the slab's rows
    uint32_t chunks;     // workgroups per row: those of the slab's longest row
    int square;
};

// entry q of row i: its place in the slab and its column record
__device__ __forceinline__ uint64_t row_pairs_of(const LinkRows &g, uint32_t i)
{
    return g.square ? (uint64_t)g.n_cols - i - 1 : (uint64_t)g.n_cols;
}
__device__ __forceinline__ uint64_t row_base_of(const LinkRows &g, uint32_t i)
{
    return g.square ? tri_row_start(g.n_cols, i) - g.out_base : (uint64_t)(i - g.rb) * g.n_cols;
}

// The test of this thread's kLinkSteps entries: v[t] their payloads, the result bit t = the entry of step t is a link.
template <int M, int W, bool TALLY>
__device__ __forceinline__ uint32_t test_entries(const void *__restrict__ slab, const LinkRows &g, uint32_t i, uint64_t q0, int lane,
                                                 uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                                                 uint64_t (&v)[kLinkSteps])
{
    constexpr bool INT = M == DST_N_HIGH;
    const uint64_t row_pairs = row_pairs_of(g, i), base = row_base_of(g, i);
    const uint32_t j0 = g.square ? i + 1 : 0;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint4 qc = make_uint4(0, 0, 0, 0);
    if constexpr (TALLY && M == DST_TN93)
        qc = reinterpret_cast<const uint4 *>(q_counts)[i];
#pragma unroll
    for (int t = 0; t < kLinkSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        v[t] = q < row_pairs ? entry_value<M, W, TALLY>(slab, base + q, qc, t_counts, j0 + (uint32_t)q) : 0;
    }
    uint32_t linked = 0;
#pragma unroll
    for (int t = 0; t < kLinkSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        if (q < row_pairs && nn_key<INT>(v[t]) <= t_key)
            linked |= 1u << t;
    }
    return linked;
}

template <int M, int W, bool TALLY>
__global__ __launch_bounds__(256) void links_count_kernel(const void *__restrict__ slab, LinkRows g, uint32_t row0, uint64_t t_bits,
                                                          const uint32_t *__restrict__ q_counts,
                                                          const uint32_t *__restrict__ t_counts, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_links[kLinkWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t blk = (uint64_t)(i - g.rb) * g.chunks + blockIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * kLinkBlockPairs;
    if (b0 >= row_pairs_of(g, i)) {   // (whole workgroups) past the row's end: nothing, but the scan reads every count
        if (threadIdx.x == 0)
            counts[blk] = 0;
        return;
    }
    uint64_t v[kLinkSteps];
    const uint32_t linked = test_entries<M, W, TALLY>(slab, g, i, b0 + (uint32_t)wave * kLinkWavePairs, lane, t_bits, q_counts,
                                                      t_counts, v);
    uint32_t count = (uint32_t)__popc(linked);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        count += (uint32_t)__shfl_down((int)count, off, 64);
    if (lane == 0)
        wave_links[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < kLinkWaves; ++w)
            total += wave_links[w];
        counts[blk] = total;
    }
}

// One workgroup.  offsets[b] = counts[0] + .. + counts[b - 1] for b <= blocks; *grand += offsets[blocks] (the kernels of a
// call are ordered by the stream: a plain add).
__global__ __launch_bounds__(kScanThreads) void links_scan_kernel(const uint32_t *__restrict__ counts, uint64_t blocks,
                                                                  uint64_t *__restrict__ offsets, uint64_t *grand)
{
    __shared__ uint64_t wave_sum[kScanThreads / 64];
    __shared__ uint64_t carry_s;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0)
        carry_s = 0;
    __syncthreads();
    for (uint64_t b0 = 0; b0 < blocks; b0 += kScanThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t own = b < blocks ? counts[b] : 0;
        uint64_t incl = own;   // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, off, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), off, 64);
            if (lane >= off)
                incl += (uint64_t)hi << 32 | lo;
        }
        if (lane == 63)
            wave_sum[wave] = incl;
        __syncthreads();
        uint64_t before = carry_s;
        for (int w = 0; w < wave; ++w)
            before += wave_sum[w];
        if (b < blocks)
            offsets[b] = before + incl - own;
        __syncthreads();   // (everybody has read carry_s and wave_sum)
        if (threadIdx.x == kScanThreads - 1)
            carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offsets[blocks] = carry_s;
        *grand += carry_s;
    }
}

struct LinkOut {
    uint32_t *row, *col;
    uint64_t *val;     // or NULL
    uint32_t *tal;     // or NULL (TALLY slabs only)
};

template <int M, int W, bool TALLY>
__global__ __launch_bounds__(256) void links_write_kernel(const void *__restrict__ slab, LinkRows g, uint32_t row0, uint64_t t_bits,
                                                          const uint32_t *__restrict__ q_counts,
                                                          const uint32_t *__restrict__ t_counts,
                                                          const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi, LinkOut out)
{
    __shared__ uint32_t wave_links[kLinkWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t blk = (uint64_t)(i - g.rb) * g.chunks + blockIdx.x;
    const uint64_t first = offsets[blk], next = offsets[blk + 1];
    if (next == first || next <= lo || first >= hi)
        return;   // (whole workgroups) no link of this block inside the window: the slab is not touched
    const uint64_t q0 = (uint64_t)blockIdx.x * kLinkBlockPairs + (uint32_t)wave * kLinkWavePairs;
    uint64_t v[kLinkSteps];
    const uint32_t linked = test_entries<M, W, TALLY>(slab, g, i, q0, lane, t_bits, q_counts, t_counts, v);
    // ranks inside the wave: the steps in order, inside a step the lanes in order
    const uint64_t below = (1ull << lane) - 1;
    uint32_t rank[kLinkSteps], wave_total = 0;
#pragma unroll
    for (int t = 0; t < kLinkSteps; ++t) {
        const uint64_t mask = __ballot((linked >> t) & 1u);
        rank[t] = wave_total + (uint32_t)__popcll(mask & below);
        wave_total += (uint32_t)__popcll(mask);
    }
    if (lane == 0)
        wave_links[wave] = wave_total;
    __syncthreads();
    uint64_t at0 = first;
    for (int w = 0; w < wave; ++w)
        at0 += wave_links[w];
    if (!linked)
        return;
    const uint64_t base = row_base_of(g, i);
    const uint32_t j0 = g.square ? i + 1 : 0;
#pragma unroll
    for (int t = 0; t < kLinkSteps; ++t) {
        if (!((linked >> t) & 1u))
            continue;
        const uint64_t r = at0 + rank[t];
        if (r < lo || r >= hi)
            continue;
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane), e = r - lo;
        out.row[e] = i;
        out.col[e] = j0 + (uint32_t)q;
        if (out.val)
            out.val[e] = v[t];
        if constexpr (TALLY) {
            if (out.tal) {
                const uint32_t *p = static_cast<const uint32_t *>(slab) + (base + q) * W;
#pragma unroll
                for (int k = 0; k < W; ++k)
                    out.tal[e * W + k] = p[k];
            }
        }
    }
}

// A links stream's batch (dst_stream.cpp): the two words its collect needs, side by side, so that one 16-byte copy brings
// the batch's link total (the scan's last offset; NULL when nothing can link) and the pack's bad-code word.
__global__ __launch_bounds__(64) void links_stream_header_kernel(const uint64_t *__restrict__ total,
                                                                 const unsigned long long *__restrict__ bad, uint64_t *__restrict__ hdr)
{
    if (threadIdx.x == 0) {
        hdr[0] = total ? *total : 0;
        hdr[1] = *bad;
    }
}

}  // namespace

hipError_t launch_links_stream_header(const uint64_t *total, const unsigned long long *bad, uint64_t *hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(links_stream_header_kernel, dim3(1), dim3(64), 0, stream, total, bad, hdr);
    return hipGetLastError();
}

hipError_t launch_links_scan(const uint32_t *counts, uint64_t blocks, uint64_t *offsets, uint64_t *grand, hipStream_t stream)
{
    hipLaunchKernelGGL(links_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, counts, blocks, offsets, grand);
    return hipGetLastError();
}

uint64_t links_blocks(bool square, uint64_t n_cols, uint64_t rb, uint64_t re)
{
    if (re <= rb)
        return 0;
    const uint64_t longest = square ? (n_cols > rb + 1 ? n_cols - rb - 1 : 0) : n_cols;
    return (re - rb) * ((longest + kLinkBlockPairs - 1) / kLinkBlockPairs);
}

// count (out == NULL) or write one window of the slab's links
static hipError_t launch_links_pass(int measure, bool tally, bool square, const void *slab, uint64_t out_base, uint64_t n_cols,
                                    uint64_t rb, uint64_t re, uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                                    uint32_t *counts, const uint64_t *offsets, uint64_t lo, uint64_t hi, const LinkOut *out,
                                    hipStream_t stream)
{
    const uint64_t blocks = links_blocks(square, n_cols, rb, re);
    if (blocks == 0)
        return hipSuccess;
    LinkRows g;
    g.out_base = out_base;
    g.n_cols = (uint32_t)n_cols;
    g.rb = (uint32_t)rb;
    g.re = (uint32_t)re;
    g.chunks = (uint32_t)(blocks / (re - rb));
    g.square = square ? 1 : 0;
    return for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
        const dim3 grid(g.chunks, rows);
#define DST_LINKS_PASS(MEAS, W, TAL)                                                                                         \
    do {                                                                                                                     \
        if (out)                                                                                                             \
            hipLaunchKernelGGL((links_write_kernel<MEAS, W, TAL>), grid, dim3(256), 0, stream, slab, g, (uint32_t)row0, t_bits, \
                               q_counts, t_counts, offsets, lo, hi, *out);                                                   \
        else                                                                                                                 \
            hipLaunchKernelGGL((links_count_kernel<MEAS, W, TAL>), grid, dim3(256), 0, stream, slab, g, (uint32_t)row0, t_bits, \
                               q_counts, t_counts, counts);                                                                  \
    } while (0)
        const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
        if (!tally) {
            if (int_payload)
                DST_LINKS_PASS(DST_N_HIGH, 1, false);
            else
                DST_LINKS_PASS(DST_RAW, 2, false);   // (any f64 measure: the payload is read, not computed)
        } else {
            switch (measure) {
            case DST_N:
            case DST_N_HIGH: DST_LINKS_PASS(DST_N_HIGH, 1, true); break;
            case DST_RAW: DST_LINKS_PASS(DST_RAW, 2, true); break;
            case DST_JC69: DST_LINKS_PASS(DST_JC69, 2, true); break;
            case DST_K80: DST_LINKS_PASS(DST_K80, 3, true); break;
            case DST_TN93: DST_LINKS_PASS(DST_TN93, 4, true); break;
            default: return hipErrorInvalidValue;
            }
        }
#undef DST_LINKS_PASS
        return hipGetLastError();
    });
}

hipError_t launch_links_count(int measure, bool tally, bool square, const void *slab, uint64_t out_base, uint64_t n_cols,
                              uint64_t rb, uint64_t re, uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                              const LinksBuffers &b, hipStream_t stream)
{
    const uint64_t blocks = links_blocks(square, n_cols, rb, re);
    const hipError_t e = launch_links_pass(measure, tally, square, slab, out_base, n_cols, rb, re, t_bits, q_counts, t_counts,
                                           b.counts, nullptr, 0, 0, nullptr, stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(links_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, b.counts, blocks, b.offsets, b.grand);
    return hipGetLastError();
}

hipError_t launch_links_write(int measure, bool tally, bool square, const void *slab, uint64_t out_base, uint64_t n_cols,
                              uint64_t rb, uint64_t re, uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                              const LinksBuffers &b, uint64_t lo, uint64_t hi, bool values, bool tallies, hipStream_t stream)
{
    if (hi <= lo || hi - lo > DST_LINKS_CHUNK || (tallies && !tally))
        return hipErrorInvalidValue;
    const LinkOut out{b.row, b.col, values ? b.val : nullptr, tallies ? b.tal : nullptr};
    return launch_links_pass(measure, tally, square, slab, out_base, n_cols, rb, re, t_bits, q_counts, t_counts, nullptr, b.offsets,
                             lo, hi, &out, stream);
}

}  // namespace dst
