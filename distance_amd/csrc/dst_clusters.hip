// dst_clusters.hip — single-linkage clusters of one set (dst_clusters): lock-free union-find over the links of one row
// slab of DST_OUT_DISTANCE payloads at a time, on a parent array that lives on the device for the whole call
// (DESIGN.md 3h).
//
// Definition.  Records i < j of slot 0 are linked when the pair's DST_OUT_DISTANCE payload v satisfies v <= T:
//   n / n_high (int64 v): as real numbers, v <= floor(T) (the host clamps floor(T) to the int64 range);
//   f64 measures:         IEEE v <= T, i.e. nn_key(v) <= nn_key(T): NaN never links, -0.0 links wherever +0.0 does,
//                         T = +inf links every pair whose value is not NaN.
// A cluster is a connected component of the links; label[i] = the smallest record index in i's cluster.  For jc69 /
// k80 / tn93 the payload is the pair kernels' series form, within 1e-15 of the reference's value and not bitwise equal
// to it: a pair whose value lies within that distance of T can be decided differently from a CPU
// computation.  raw, n and n_high are exact.
//
//   clusters_init_kernel   parent[i] := i, the link counter := 0
//   clusters_link_kernel   one row slab: each wave reads a contiguous run of one row's payloads (coalesced), tests them
//                          against T and unites the endpoints of every link; links are counted per block, one 64-bit
//                          agent-scope atomic add per block
//   clusters_final_kernel  full path compression: parent[i] := root(i), the label
//
// Union-find, lock-free.  A hook always puts the larger root under the smaller, so parent[x] <= x at all times and a
// root is the smallest index of its tree.  Per-XCD L2s are not coherent and a CU's L1 is never refreshed by another
// CU's stores, so the algorithm stands on these rules only:
//   - every write to parent is an agent-scope atomic: a CAS for a hook, an atomic min for compression;
//   - reads are relaxed agent-scope atomic loads, and they may be stale;
//   - after a failed CAS the union continues from the value the CAS returned, never from a re-read.
// Every value parent[x] ever holds is a record of x's component, and the values of one entry only decrease.  A stale
// read therefore still names an ancestor, and two chains walked from stale reads meet only when their records really are
// connected.  A union of roots (lo, hi), lo < hi, CASes parent[hi] from hi to lo; when the CAS fails it returned some
// p < hi, and the next attempt is between find(p) <= p and find(lo) <= lo: the larger of the two roots strictly
// decreases, so the union ends.  The link kernels of one call all run before clusters_final_kernel (stream order), so
// the final kernel walks complete trees.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kClusterWaves = 4;                                   // waves per workgroup
constexpr int kClusterSteps = 8;                                   // 64-pair steps per wave
constexpr uint32_t kClusterWavePairs = 64u * kClusterSteps;        // 512 pairs: one wave's run
constexpr uint32_t kClusterBlockPairs = kClusterWavePairs * kClusterWaves;   // 2048 pairs of one row per workgroup

__device__ __forceinline__ uint32_t uf_load(uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as far as this lane can see; x's own entry is pointed at it when the walk took more than one step
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = uf_load(parent, x);
    if (p == x)
        return x;
    const uint32_t x0 = x, first = p;
    do {
        x = p;
        p = uf_load(parent, x);
    } while (p != x);
    if (first != x)
        __hip_atomic_fetch_min(parent + x0, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return x;
}

// joins the trees of a and b (each a root or a record as seen by this lane)
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    while (a != b) {
        const uint32_t lo = min(a, b);
        uint32_t hi = max(a, b);
        if (__hip_atomic_compare_exchange_strong(parent + hi, &hi, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        // hi now holds what parent[hi] was: below hi, an ancestor of hi — the union goes on from there
        a = uf_find(parent, hi);
        b = uf_find(parent, lo);
    }
}

__global__ __launch_bounds__(256) void clusters_init_kernel(uint32_t *parent, uint32_t n, unsigned long long *links)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        __hip_atomic_store(parent + i, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (i == 0)
        __hip_atomic_store(links, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One row slab of the square: rows [row0 + blockIdx.y] (below re), pairs (i, j > i) at slab entry
// tri_row_start(n, i) - out_base + (j - i - 1).  Workgroup (x, y): pairs 2048 x .. 2048 x + 2047 of its row, wave w the
// 512 of them from 2048 x + 512 w, lane l of step t pair 512 w + 64 t + l.  t_bits: the threshold as a payload (int64 /
// f64 bits), compared through nn_key.
template <bool INT>
__global__ __launch_bounds__(256) void clusters_link_kernel(const uint64_t *__restrict__ slab, uint64_t out_base, uint32_t n,
                                                            uint32_t row0, uint32_t re, uint64_t t_bits, uint32_t *parent,
                                                            unsigned long long *links)
{
    __shared__ uint32_t wave_links[kClusterWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= re)
        return;   // (whole workgroups)
    const uint64_t row_pairs = n - i - 1;   // (64-bit positions: a row may hold close to 2^32 pairs)
    const uint64_t q0 = (uint64_t)blockIdx.x * kClusterBlockPairs + (uint32_t)wave * kClusterWavePairs;
    if ((uint64_t)blockIdx.x * kClusterBlockPairs >= row_pairs)
        return;   // (whole workgroups)
    const uint64_t base = tri_row_start(n, i) - out_base;
    const uint64_t t_key = nn_key<INT>(t_bits);
    uint64_t v[kClusterSteps];
#pragma unroll
    for (int t = 0; t < kClusterSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        v[t] = q < row_pairs ? __builtin_nontemporal_load(slab + base + q) : 0;
    }
    uint32_t count = 0, linked = 0;   // linked: bit t = this lane's pair of step t is a link
#pragma unroll
    for (int t = 0; t < kClusterSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        if (q < row_pairs && nn_key<INT>(v[t]) <= t_key)
            linked |= 1u << t;
    }
    count = (uint32_t)__popc(linked);
    if (__ballot(linked != 0)) {
        // the row's root once per wave (possibly stale: any record of i's tree is a valid start).  A link is settled
        // when j's chain reaches ri; the first two steps of every chain are loaded for all the lane's links at once
        // (two round trips instead of two per link), the rest, and the unions, one link at a time.
        uint32_t ri = uf_find(parent, i);
        uint32_t pj[kClusterSteps], gp[kClusterSteps];
#pragma unroll
        for (int t = 0; t < kClusterSteps; ++t)
            pj[t] = (linked >> t & 1u) ? uf_load(parent, i + 1 + (uint32_t)q0 + (uint32_t)(t * 64 + lane)) : ri;
#pragma unroll
        for (int t = 0; t < kClusterSteps; ++t)
            gp[t] = pj[t] != ri ? uf_load(parent, pj[t]) : ri;
        for (int t = 0; t < kClusterSteps; ++t) {
            if (pj[t] == ri)
                continue;
            const uint32_t j = i + 1 + (uint32_t)q0 + (uint32_t)(t * 64 + lane);
            if (gp[t] != pj[t])   // j's entry straight to its grandparent, an ancestor
                __hip_atomic_fetch_min(parent + j, gp[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gp[t] == ri)
                continue;
            const uint32_t rj = uf_find(parent, gp[t]);
            if (rj != ri) {
                uf_unite(parent, ri, rj);
                ri = min(ri, rj);   // (both are records of i's tree now; the smaller one is nearer its root)
            }
        }
    }
    // exact link count: wave sum, workgroup sum, one 64-bit atomic add
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        count += (uint32_t)__shfl_down((int)count, off, 64);
    if (lane == 0)
        wave_links[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < kClusterWaves; ++w)
            total += wave_links[w];
        if (total)
            __hip_atomic_fetch_add(links, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void clusters_final_kernel(uint32_t *parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t x = i, p = uf_load(parent, i);
    const uint32_t first = p;
    while (p != x) {
        x = p;
        p = uf_load(parent, x);
    }
    if (first != x)
        __hip_atomic_fetch_min(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

hipError_t launch_clusters_init(uint32_t *parent, uint64_t n, unsigned long long *links, hipStream_t stream)
{
    const unsigned blocks = (unsigned)std::max<uint64_t>((n + 255) / 256, 1);
    hipLaunchKernelGGL(clusters_init_kernel, dim3(blocks), dim3(256), 0, stream, parent, (uint32_t)n, links);
    return hipGetLastError();
}

hipError_t launch_clusters_link(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                                uint64_t t_bits, uint32_t *parent, unsigned long long *links, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const unsigned chunks = (unsigned)((n - rb - 1 + kClusterBlockPairs - 1) / kClusterBlockPairs);   // of row rb, the longest
    return for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
        const dim3 grid(chunks, rows);
        if (int_payload)
            hipLaunchKernelGGL(clusters_link_kernel<true>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n,
                               (uint32_t)row0, (uint32_t)re, t_bits, parent, links);
        else
            hipLaunchKernelGGL(clusters_link_kernel<false>, grid, dim3(256), 0, stream, slab, out_base, (uint32_t)n,
                               (uint32_t)row0, (uint32_t)re, t_bits, parent, links);
        return hipGetLastError();
    });
}

hipError_t launch_clusters_final(uint32_t *parent, uint64_t n, hipStream_t stream)
{
    const unsigned blocks = (unsigned)std::max<uint64_t>((n + 255) / 256, 1);
    hipLaunchKernelGGL(clusters_final_kernel, dim3(blocks), dim3(256), 0, stream, parent, (uint32_t)n);
    return hipGetLastError();
}

}  // namespace dst
