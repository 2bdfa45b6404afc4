// dst_dendrogram.hip — UPGMA / WPGMA / complete-linkage dendrograms of one set (dst_dendrogram, dst_dendrogram_matrix):
// the f64 square lives on the device (filled by dst_nj.hip's init / scatter / mirror kernels) and a round needs only the
// global minimum distance, which is kept as one cached minimum per row and repaired after a merge.  The
// arithmetic is the one include/distance_hip.h fixes, in the order written there (-ffp-contract=off).
//
//   dg_init_kernel     node := identity, size := 1, heights := +0.0, every row on the rescan list, block minima := ~0
//   dg_rescan_kernel   a fixed grid; a workgroup takes rows from the list (agent-scope atomic add on the list's head)
//                      until it is empty: the smallest (nn_key, k) of row x over the active k > x into row_key[x] /
//                      row_col[x], and the key into the row's block minimum by an agent-scope atomic min
//   dg_select_kernel   one workgroup: the smallest block minimum (ties: the first block), the first row of that block
//                      that holds it, its cached column: the round's (a, b).  Thread 0 makes the node (parent, length,
//                      height, the slot's node id and size, slot b inactive), hands (a, b, s_a, s_b) to the merge and
//                      empties the list
//   dg_merge_kernel    thread k = slot k: d_uk into (a, k) and (k, a); row k's cache entry is invalidated and the row
//                      listed (k = a; k < b with the cached column a or b, unless (k, a) did not rise above the cached
//                      key), or lowered when the one changed entry (k, a) is smaller (k < a); workgroups that hold a
//                      row <= b recompute their block minimum
//
// Who writes what.  The cache order is (key, column) within a row, (key, row) across rows and blocks, which is the
// definition's (key, a, b).  Select: the only workgroup of its launch.  Merge: thread k writes D[a][k], D[k][a],
// row_key[k], row_col[k] and reads D[a][k], D[b][k] and its own cache entry: no entry is written by one thread and read
// by another (k = a and k = b write no D); blk_key[B] is written by workgroup B alone, from its own threads' keys; the
// list grows by an agent-scope atomic add and is read by the next launch.  Rescan: a row is taken by one workgroup, which
// alone writes its cache entry; D and the active flags are read-only in it; blk_key only by atomic min, and it was
// written (not read) by the merge launch before.  An invalidated row carries the key ~0 until its rescan, which no
// finite value's key equals, so the block minima never see it.  Plain C++ and vector atomics only.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kDgThreads = (int)kDgBlockRows;   // merge, select, init: one thread per row of a block
constexpr int kDgScanThreads = 1024;            // rescan: one workgroup per row, 8 loads in flight per lane
constexpr int kDgScanLoads = 8;
constexpr unsigned kDgRoundGrid = 128;          // rescan workgroups of a round (most rounds list one to three rows)
constexpr unsigned kDgFirstGrid = 2048;         // ... of the first scan of every row

// the smallest (key, idx) of the workgroup, returned in every thread (THREADS a multiple of 64)
template <int THREADS>
__device__ __forceinline__ void dg_block_min(uint64_t &key, uint32_t &idx)
{
    __shared__ uint64_t s_key[THREADS / 64];
    __shared__ uint32_t s_idx[THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_down(key, off, 64);
        const uint32_t oi = __shfl_down(idx, off, 64);
        if (ok < key || (ok == key && oi < idx)) {
            key = ok;
            idx = oi;
        }
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    __syncthreads();   // (the arrays may still be read from an earlier call)
    if (lane == 0) {
        s_key[wave] = key;
        s_idx[wave] = idx;
    }
    __syncthreads();
    key = s_key[0];
    idx = s_idx[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w)
        if (s_key[w] < key || (s_key[w] == key && s_idx[w] < idx)) {
            key = s_key[w];
            idx = s_idx[w];
        }
}

__global__ __launch_bounds__(kDgThreads) void dg_init_kernel(DgBuffers b, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * kDgThreads + threadIdx.x;
    if (i < n) {
        b.node[i] = (uint32_t)i;
        b.size[i] = 1;
        b.height[i] = 0.0;
        b.row_key[i] = ~0ull;
        b.row_col[i] = 0xFFFFFFFFu;
        b.list[i] = (uint32_t)i;
    }
    if (threadIdx.x == 0)
        b.blk_key[blockIdx.x] = ~0ull;
    if (i == 0) {
        b.counters[0] = (uint32_t)n;
        b.counters[1] = 0;
        b.counters[2] = 0;
        *b.scans = 0;
        *b.pair = DgPair{0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};
    }
}

__global__ __launch_bounds__(kDgScanThreads) void dg_rescan_kernel(DgBuffers b, uint64_t n)
{
    __shared__ uint32_t s_take;
    const uint32_t listed = b.counters[0];   // (written by earlier launches only)
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0)
            s_take = __hip_atomic_fetch_add(&b.counters[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint32_t take = s_take;
        if (take >= listed)
            return;
        const uint64_t x = b.list[take];
        if (x >= n)
            continue;
        const double *row = b.D + x * n;
        uint64_t bk = ~0ull;
        uint32_t bj = 0xFFFFFFFFu;
        uint64_t j = x + 1 + threadIdx.x;
        for (; j + (kDgScanLoads - 1) * (uint64_t)kDgScanThreads < n; j += (uint64_t)kDgScanLoads * kDgScanThreads) {
            double d[kDgScanLoads];
            uint8_t a[kDgScanLoads];
#pragma unroll
            for (int u = 0; u < kDgScanLoads; ++u) {
                d[u] = row[j + (uint64_t)u * kDgScanThreads];
                a[u] = b.active[j + (uint64_t)u * kDgScanThreads];
            }
#pragma unroll
            for (int u = 0; u < kDgScanLoads; ++u) {
                const uint64_t key = nn_key<false>((uint64_t)__double_as_longlong(d[u]));
                if (a[u] && key < bk) {   // (a lane's columns ascend: the first of equal keys stays)
                    bk = key;
                    bj = (uint32_t)(j + (uint64_t)u * kDgScanThreads);
                }
            }
        }
        for (; j < n; j += kDgScanThreads) {
            const uint64_t key = nn_key<false>((uint64_t)__double_as_longlong(row[j]));
            if (b.active[j] && key < bk) {
                bk = key;
                bj = (uint32_t)j;
            }
        }
        dg_block_min<kDgScanThreads>(bk, bj);
        if (threadIdx.x == 0) {
            b.row_key[x] = bk;
            b.row_col[x] = bj;
            if (bk != ~0ull)
                __hip_atomic_fetch_min((unsigned long long *)&b.blk_key[x / kDgBlockRows], (unsigned long long)bk,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Round t: u = n + t; last: the root's own entries too.
__global__ __launch_bounds__(kDgThreads) void dg_select_kernel(DgBuffers b, uint64_t n, uint32_t u, int last)
{
    const uint32_t nblk = (uint32_t)((n + kDgBlockRows - 1) / kDgBlockRows);
    uint64_t bk = ~0ull;
    uint32_t bb = 0xFFFFFFFFu;
    for (uint32_t p = threadIdx.x; p < nblk; p += kDgThreads) {
        const uint64_t k = b.blk_key[p];
        if (k < bk) {   // (a thread's blocks ascend)
            bk = k;
            bb = p;
        }
    }
    dg_block_min<kDgThreads>(bk, bb);
    const uint64_t x = (uint64_t)bb * kDgBlockRows + threadIdx.x;
    uint64_t rk = ~0ull;
    uint32_t ra = 0xFFFFFFFFu;
    if (bk != ~0ull && x < n && b.row_key[x] == bk) {
        rk = bk;
        ra = (uint32_t)x;
    }
    dg_block_min<kDgThreads>(rk, ra);
    if (threadIdx.x != 0)
        return;
    *b.scans += b.counters[0];
    b.counters[0] = 0;
    b.counters[1] = 0;
    const uint32_t a = ra, c = ra < n ? b.row_col[ra] : 0xFFFFFFFFu;
    if (a >= n || c >= n || c <= a || !b.active[a] || !b.active[c]) {
        // no pair, or a dead slot: finite values and two active slots rule it out unless the cache went wrong.  The
        // first such round is reported (counters[2] = round + 1: DST_ERR_STATE); the launches after it do nothing.
        // No test reaches this branch (none can without a cache bug to provoke it): it is covered by reading only
        if (b.counters[2] == 0)
            b.counters[2] = u - (uint32_t)n + 1;
        *b.pair = DgPair{0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};
        return;
    }
    const double hu = b.D[(uint64_t)a * n + c] * 0.5;
    const uint32_t na = b.node[a], nb = b.node[c];
    b.parent[na] = u;
    b.parent[nb] = u;
    b.length[na] = hu - b.height[na];
    b.length[nb] = hu - b.height[nb];
    b.height[u] = hu;
    const uint32_t sa = b.size[a], sb = b.size[c];
    b.node[a] = u;
    b.size[a] = sa + sb;
    b.active[c] = 0;
    *b.pair = DgPair{a, c, sa, sb};
    if (last) {
        b.parent[u] = 0xFFFFFFFFu;
        b.length[u] = 0.0;
    }
}

template <int LINKAGE>
__global__ __launch_bounds__(kDgThreads) void dg_merge_kernel(DgBuffers b, uint64_t n)
{
    const DgPair p = *b.pair;
    const uint64_t a = p.a, c = p.b;
    if (a >= n || c >= n)
        return;
    const uint64_t base = (uint64_t)blockIdx.x * kDgThreads;
    const uint64_t k = base + threadIdx.x;
    const bool live = k < n && k != c && b.active[k];
    uint64_t key = ~0ull;   // row k's cache key after this launch (~0: none, inactive, or waiting for its rescan)
    if (live && k != a) {
        const double dak = b.D[a * n + k], dbk = b.D[c * n + k];
        double duk;
        if (LINKAGE == DST_LINK_AVERAGE)
            duk = ((double)p.sa * dak + (double)p.sb * dbk) / (double)(p.sa + p.sb);
        else if (LINKAGE == DST_LINK_WEIGHTED)
            duk = (dak + dbk) * 0.5;
        else
            duk = dak < dbk ? dbk : dak;
        b.D[a * n + k] = duk;
        b.D[k * n + a] = duk;
        if (k < c) {
            key = b.row_key[k];
            const uint32_t col = b.row_col[k];
            const uint64_t nk = nn_key<false>((uint64_t)__double_as_longlong(duk));
            bool relist = false;
            if (key != ~0ull && (col == a || col == c)) {
                // the cached entry changed or left.  Every other entry of the row is as it was and not below (key, col),
                // so (k, a) is the minimum again when it did not rise (a <= col: ties stay in order); else rescan
                if (k < a && nk <= key) {
                    key = nk;
                    b.row_key[k] = nk;
                    b.row_col[k] = (uint32_t)a;
                } else {
                    relist = true;
                }
            } else if (k < a && (nk < key || (nk == key && a < col))) {   // the one changed entry of row k: (k, a)
                key = nk;
                b.row_key[k] = nk;
                b.row_col[k] = (uint32_t)a;
            }
            if (relist) {
                key = ~0ull;
                b.row_key[k] = ~0ull;
                b.list[__hip_atomic_fetch_add(&b.counters[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = (uint32_t)k;
            }
        } else if (base <= c) {
            key = b.row_key[k];   // (a row right of b in b's block: unchanged, and part of the block minimum)
        }
    } else if (live) {   // k == a: every entry right of a changed
        b.row_key[k] = ~0ull;
        b.list[__hip_atomic_fetch_add(&b.counters[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = (uint32_t)k;
    } else if (k == c) {
        b.row_key[k] = ~0ull;
    }
    if (base > c)
        return;   // (the whole workgroup: no row right of b changed)
    uint32_t idx = threadIdx.x;
    dg_block_min<kDgThreads>(key, idx);
    if (threadIdx.x == 0)
        b.blk_key[blockIdx.x] = key;
}

}  // namespace

hipError_t launch_dg_init(const DgBuffers &b, uint64_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(dg_init_kernel, dim3((unsigned)((n + kDgThreads - 1) / kDgThreads)), dim3(kDgThreads), 0, stream, b, n);
    return hipGetLastError();
}

hipError_t launch_dg_rounds(const DgBuffers &b, uint64_t n, int linkage, hipStream_t stream)
{
    const unsigned blocks = (unsigned)((n + kDgThreads - 1) / kDgThreads);
    hipLaunchKernelGGL(dg_rescan_kernel, dim3((unsigned)std::min<uint64_t>(n, kDgFirstGrid)), dim3(kDgScanThreads), 0, stream, b,
                       n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const unsigned round_grid = (unsigned)std::min<uint64_t>(n, kDgRoundGrid);
    for (uint64_t t = 0; t + 1 < n; ++t) {
        const bool last = t + 2 == n;
        hipLaunchKernelGGL(dg_select_kernel, dim3(1), dim3(kDgThreads), 0, stream, b, n, (uint32_t)(n + t), last ? 1 : 0);
        if (last)
            break;   // (one cluster is left: nothing to update)
        if (linkage == DST_LINK_AVERAGE)
            hipLaunchKernelGGL(dg_merge_kernel<DST_LINK_AVERAGE>, dim3(blocks), dim3(kDgThreads), 0, stream, b, n);
        else if (linkage == DST_LINK_WEIGHTED)
            hipLaunchKernelGGL(dg_merge_kernel<DST_LINK_WEIGHTED>, dim3(blocks), dim3(kDgThreads), 0, stream, b, n);
        else
            hipLaunchKernelGGL(dg_merge_kernel<DST_LINK_COMPLETE>, dim3(blocks), dim3(kDgThreads), 0, stream, b, n);
        hipLaunchKernelGGL(dg_rescan_kernel, dim3(round_grid), dim3(kDgScanThreads), 0, stream, b, n);
        if ((e = hipGetLastError()) != hipSuccess)
            return e;
    }
    return hipGetLastError();
}

}  // namespace dst
