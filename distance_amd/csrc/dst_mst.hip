// dst_mst.hip — the minimum spanning forest of one set (dst_mst): Boruvka rounds over row slabs of DST_OUT_DISTANCE
// payloads, the triangle recomputed every round, on O(n) arrays that live on the device for the whole call.
//
// Definition.  Records i < j of slot 0 are joined by an edge when the pair's DST_OUT_DISTANCE payload v is not NaN; edges
// are ordered by (nn_key(v), i, j), a strict total order, so the minimum spanning forest is unique (Kruskal's over that
// order).  The int64 payloads of n / n_high are site counts: their key is never ~0, the key of NaN, which therefore
// serves as "no edge" for every measure.
//
//   mst_reset_kernel   best_key[c] := best_pair[c] := ~0, hook[c] := c, the round's counter := 0 (first round also
//                      comp[c] := c and the edge counter := 0)
//   mst_key_kernel     scan, launch A of a slab: best_key[c] := min over c's outgoing edges of the key, for BOTH ends of
//                      every edge; a lane whose atomic strictly lowered best_key[c] stores ~0 to best_pair[c]
//   mst_pair_kernel    scan, launch B of the same slab: best_pair[c] := min (i << 32 | j) over c's outgoing edges whose
//                      key equals best_key[c]
//   mst_hook_kernel    one lane per component with a best edge: hook under the component of the edge's other end and
//                      emit the edge; of a mutual choice the smaller component stays a root and emits, the larger hooks only
//   mst_flatten_kernel comp[x] := the root of comp[x] along hook
//   mst_gather_kernel  finish: one lane per forest edge picks the pair's DST_OUT_TALLY words out of the slab that holds
//                      its row and finalises them to the DST_OUT_DISTANCE payload (finalize_pair<M, false>: the pair
//                      kernels' epilogue, bitwise what a distance run returns)
//
// Why best_pair ends right.  After launch A of slab s best_key[c] is the smallest key of c's outgoing edges in slabs
// 0 .. s.  Launch B of slab s runs behind it (stream order) and offers the slab's pairs of exactly that key.  Pairs that
// earlier slabs offered at a larger key were wiped by the lane that lowered the key; pairs of earlier slabs at the same
// key stay in the minimum; an earlier slab cannot hold a pair of a smaller key.  So after the last slab best_pair[c] is
// the smallest (i, j) among c's outgoing edges of minimal key: c's minimal outgoing edge in the order.
//
// Memory model (the rules of DESIGN.md 3h).  Per-XCD L2s are not coherent inside a kernel; they are at kernel boundaries.
//   - best_key / best_pair are written by agent-scope atomics only (min, and the wipe's store); each only decreases inside
//     one launch (the wipe happens in launch A, which never reads best_pair, and launch B never writes best_key), so the
//     relaxed loads that pre-check an atomic may be stale only upwards: a stale value can cause an atomic that changes
//     nothing, never skip one that would.
//   - comp is read-only in the scan and the hook; the hook writes hook[c] (its own entry) and reads comp / best_pair /
//     best_key, which no lane of that launch writes.  The flatten kernel walks hook with relaxed atomic loads and shortens
//     it with atomic stores of an ancestor: every value hook[x] ever holds is an ancestor of x, roots never change.
//   - nothing re-reads after a failed compare-and-swap: there is none.
// The order is strict, so along the hooks the chosen edges strictly decrease except at a mutual choice: mutual pairs are
// the only cycles, and they are broken by leaving the smaller component a root.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kMstWaves = 4;                                   // waves per workgroup
constexpr int kMstSteps = 8;                                   // 64-pair steps per wave
constexpr uint32_t kMstWavePairs = 64u * kMstSteps;            // 512 pairs: one wave's run
constexpr uint32_t kMstBlockPairs = kMstWavePairs * kMstWaves; // 2048 pairs of one row per workgroup
constexpr uint64_t kNone = ~0ull;

__device__ __forceinline__ uint64_t ld64(uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st64(uint64_t *p, uint64_t x)
{
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t min64(uint64_t *p, uint64_t x)
{
    return __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t wave_min64(uint64_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off, 64);
        const uint64_t y = (uint64_t)hi << 32 | lo;
        x = y < x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(256) void mst_reset_kernel(uint32_t *comp, uint32_t *hook, uint64_t *best_key, uint64_t *best_pair,
                                                        uint32_t n, uint64_t *counters, int first)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) {
        if (first)
            comp[c] = c;
        hook[c] = c;
        best_key[c] = kNone;
        best_pair[c] = kNone;
    }
    if (c == 0) {
        if (first)
            counters[0] = 0;   // edges of the forest so far
        counters[1] = 0;       // edges of this round
    }
}

// One row slab, as clusters_link_kernel lays it out: workgroup (x, y) takes pairs 2048 x .. 2048 x + 2047 of row
// row0 + y (below re), wave w the 512 of them from 2048 x + 512 w, lane l of step t pair 512 w + 64 t + l; pair (i, j) is
// slab entry tri_row_start(n, i) - out_base + (j - i - 1).  PAIRS = false: launch A (keys); true: launch B (pairs, the
// slab's last reader: nontemporal loads).
template <bool INT, bool PAIRS>
__global__ __launch_bounds__(256) void mst_scan_kernel(const uint64_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                       uint32_t row0, uint32_t re, const uint32_t *__restrict__ comp,
                                                       uint64_t *best_key, uint64_t *best_pair)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= re)
        return;   // (whole workgroups)
    const uint64_t row_pairs = n - i - 1;   // (64-bit positions: a row may hold close to 2^32 pairs)
    const uint64_t q0 = (uint64_t)blockIdx.x * kMstBlockPairs + (uint32_t)wave * kMstWavePairs;
    if (q0 >= row_pairs)
        return;   // (whole waves; the kernel has no barrier)
    const uint64_t base = tri_row_start(n, i) - out_base;
    const uint32_t ci = comp[i];   // wave-uniform
    uint64_t v[kMstSteps];
    uint32_t cj[kMstSteps];
#pragma unroll
    for (int t = 0; t < kMstSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        const bool in = q < row_pairs;
        if constexpr (PAIRS)
            v[t] = in ? __builtin_nontemporal_load(slab + base + q) : 0;
        else
            v[t] = in ? slab[base + q] : 0;
        cj[t] = in ? comp[i + 1 + (uint32_t)q] : ci;   // (out of range: never a candidate)
    }
    // the row side is reduced in registers across the wave (i and comp[i] are wave-uniform): one atomic per wave at most
    const uint64_t row_key = PAIRS ? best_key[ci] : 0;   // (launch B: best_key is not written by this launch)
    uint64_t row_best = kNone;
#pragma unroll
    for (int t = 0; t < kMstSteps; ++t) {
        if (cj[t] == ci)
            continue;
        const uint64_t key = nn_key<INT>(v[t]);
        if (key == kNone)
            continue;   // NaN is never an edge
        if constexpr (!PAIRS) {
            row_best = key < row_best ? key : row_best;
            // the column side: a stale pre-check value is too large at worst (best_key only decreases in this launch)
            if (key < ld64(best_key + cj[t]) && min64(best_key + cj[t], key) > key)
                st64(best_pair + cj[t], kNone);   // the key fell: pairs offered at the old key no longer count
        } else {
            const uint64_t pair = (uint64_t)i << 32 | (i + 1 + (uint32_t)q0 + (uint32_t)(t * 64 + lane));
            if (key == row_key)
                row_best = pair < row_best ? pair : row_best;
            if (key == best_key[cj[t]] && pair < ld64(best_pair + cj[t]))
                min64(best_pair + cj[t], pair);
        }
    }
    row_best = wave_min64(row_best);
    if (lane == 0 && row_best != kNone) {
        if constexpr (!PAIRS) {
            if (row_best < ld64(best_key + ci) && min64(best_key + ci, row_best) > row_best)
                st64(best_pair + ci, kNone);
        } else {
            if (row_best < ld64(best_pair + ci))
                min64(best_pair + ci, row_best);
        }
    }
}

__global__ __launch_bounds__(256) void mst_hook_kernel(const uint32_t *__restrict__ comp, uint32_t *hook,
                                                       const uint64_t *__restrict__ best_key,
                                                       const uint64_t *__restrict__ best_pair, uint32_t n, uint64_t *edges,
                                                       uint64_t *edge_keys, uint64_t *counters)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n)
        return;
    const uint64_t pair = best_pair[c];
    if (pair == kNone)
        return;   // not a component root, or a component without an outgoing edge
    const uint32_t ci = comp[(uint32_t)(pair >> 32)], cj = comp[(uint32_t)pair];
    const uint32_t other = ci == c ? cj : ci;
    const bool mutual = best_pair[other] == pair;
    if (mutual && other < c) {
        hook[c] = other;   // the smaller component emits the edge
        return;
    }
    if (!mutual)
        hook[c] = other;
    const unsigned long long at = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(counters), 1ull,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (at < n) {   // (a forest has fewer than n edges)
        edges[at] = pair;
        edge_keys[at] = best_key[c];
    }
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(counters) + 1, 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void mst_flatten_kernel(uint32_t *comp, uint32_t *hook, uint32_t n)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n)
        return;
    const uint32_t c0 = comp[x];   // (this lane's own entry: nobody else touches it)
    uint32_t r = c0, p = __hip_atomic_load(hook + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t first = p;
    while (p != r) {
        r = p;
        p = __hip_atomic_load(hook + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (first != r)   // the old root's entry straight to the new root: later walks through it are one step
        __hip_atomic_store(hook + c0, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    comp[x] = r;
}

// rows [rb, re) of the square as DST_OUT_TALLY words from slab entry tri_row_start(n, i) - out_base
template <int M, int W>
__global__ __launch_bounds__(256) void mst_gather_kernel(const uint32_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                         uint32_t rb, uint32_t re, const uint32_t *__restrict__ counts,
                                                         const uint64_t *__restrict__ edges, uint32_t n_edges, uint64_t *val,
                                                         uint32_t *tal)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges)
        return;
    const uint64_t pair = edges[e];
    const uint32_t i = (uint32_t)(pair >> 32), j = (uint32_t)pair;
    if (i < rb || i >= re)
        return;
    const uint64_t at = tri_row_start(n, i) - out_base + (j - i - 1);
    uint32_t o[W];
#pragma unroll
    for (int t = 0; t < W; ++t) {
        o[t] = slab[at * W + t];
        tal[(uint64_t)e * W + t] = o[t];
    }
    uint4 qc = make_uint4(0, 0, 0, 0), tc = qc;
    if constexpr (M == DST_TN93) {   // base counts in (i, j) order, as the pair kernels take them
        qc = reinterpret_cast<const uint4 *>(counts)[i];
        tc = reinterpret_cast<const uint4 *>(counts)[j];
    }
    val[e] = pair_value<M>(o, qc, tc);
}

}  // namespace

hipError_t launch_mst_reset(const MstBuffers &b, uint64_t n, bool first, hipStream_t stream)
{
    const unsigned blocks = (unsigned)std::max<uint64_t>((n + 255) / 256, 1);
    hipLaunchKernelGGL(mst_reset_kernel, dim3(blocks), dim3(256), 0, stream, b.comp, b.hook, b.best_key, b.best_pair, (uint32_t)n,
                       b.counters, first ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_mst_scan(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                           const MstBuffers &b, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const unsigned chunks = (unsigned)((n - rb - 1 + kMstBlockPairs - 1) / kMstBlockPairs);   // of row rb, the longest
#define DST_MST_SCAN(INT, PAIRS)                                                                                           \
    hipLaunchKernelGGL((mst_scan_kernel<INT, PAIRS>), grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n, (uint32_t)row0, \
                       (uint32_t)re, b.comp, b.best_key, b.best_pair)
    for (int pass = 0; pass < 2; ++pass) {   // launch A over the whole slab, then launch B
        const hipError_t e = for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
            const dim3 grid(chunks, rows);
            if (int_payload) {
                if (pass == 0)
                    DST_MST_SCAN(true, false);
                else
                    DST_MST_SCAN(true, true);
            } else {
                if (pass == 0)
                    DST_MST_SCAN(false, false);
                else
                    DST_MST_SCAN(false, true);
            }
            return hipGetLastError();
        });
        if (e != hipSuccess)
            return e;
    }
#undef DST_MST_SCAN
    return hipSuccess;
}

hipError_t launch_mst_hook(const MstBuffers &b, uint64_t n, hipStream_t stream)
{
    const unsigned blocks = (unsigned)std::max<uint64_t>((n + 255) / 256, 1);
    hipLaunchKernelGGL(mst_hook_kernel, dim3(blocks), dim3(256), 0, stream, b.comp, b.hook, b.best_key, b.best_pair, (uint32_t)n,
                       b.edges, b.edge_keys, b.counters);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(mst_flatten_kernel, dim3(blocks), dim3(256), 0, stream, b.comp, b.hook, (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_mst_gather(int measure, const uint32_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             const uint32_t *counts, const MstBuffers &b, uint64_t n_edges, hipStream_t stream)
{
    if (re <= rb || n_edges == 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)((n_edges + 255) / 256);
#define DST_MST_GATHER(MEAS, W)                                                                                           \
    hipLaunchKernelGGL((mst_gather_kernel<MEAS, W>), dim3(blocks), dim3(256), 0, stream, slab, out_base, (uint32_t)n,      \
                       (uint32_t)rb, (uint32_t)re, counts, b.edges, (uint32_t)n_edges, b.val, b.tal)
    switch (measure) {
    case DST_N:
    case DST_N_HIGH: DST_MST_GATHER(DST_N_HIGH, 1); break;
    case DST_RAW: DST_MST_GATHER(DST_RAW, 2); break;
    case DST_JC69: DST_MST_GATHER(DST_JC69, 2); break;
    case DST_K80: DST_MST_GATHER(DST_K80, 3); break;
    case DST_TN93: DST_MST_GATHER(DST_TN93, 4); break;
    default: return hipErrorInvalidValue;
    }
#undef DST_MST_GATHER
    return hipGetLastError();
}

}  // namespace dst
