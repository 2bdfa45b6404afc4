// dst_nj.hip — neighbour-joining trees of one set (dst_nj, dst_nj_matrix): the whole f64 square lives on the device and
// every round of the join is a scan over the active upper triangle plus one merge launch.  The arithmetic
// is the one include/distance_hip.h fixes, in the order written there (the library is compiled -ffp-contract=off).
//
//   nj_init_kernel          diagonal := +0.0, ids[i] := i, every slot active, the non-finite flag := ~0
//   nj_scatter_kernel       one row slab of DST_OUT_DISTANCE payloads into D, mirrored; the smallest linear index
//                           i * n + j of a non-finite value by an agent-scope atomic min (dst_nj)
//   nj_mirror_kernel        D's strict upper triangle into its lower one (dst_nj_matrix)
//   nj_rowsum_kernel        r[x] := sum of column x, top to bottom from +0.0 (D is symmetric: row x left to right)
//   nj_scan_kernel          per workgroup, the smallest (nn_key(Q), (a << 32) | b) over its rows of the active triangle
//   nj_merge_kernel         every workgroup reduces the partials to the round's pair (redundantly, no grid barrier);
//                           thread k applies steps 2-5 of the round to slot k
//   nj_compact_*_kernel     the active slots, in order, into the other matrix buffer (P := m)
//   nj_final_kernel         the trifurcation of the last three nodes at the root
//
// Storage.  D is P x P row-major (P: the stored dimension), slot x holds the node ids[x]; active[x] says whether slot x
// is in the list.  The list keeps its order, so position order is slot order among active slots and a tie on Q goes to
// the smallest slot pair.  r is double-buffered: the merge reads r_in and writes r_out for every active slot, so no
// workgroup reads a row sum another has already replaced.  The merge writes row a and column a of D, active[b], ids[a]
// and r_out; it reads rows a and b, D[a][b], r_in, ids[a], ids[b] — thread k touches only its own entries of row a and
// column a, and never D[a][b] — so no two threads of one launch race.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kNjThreads = 256;
constexpr int kNjRowsumThreads = 64;   // one column per lane: more workgroups on more CUs for the long columns

__device__ __forceinline__ bool nj_better(uint64_t k1, uint64_t ij1, uint64_t k2, uint64_t ij2)
{
    return k1 < k2 || (k1 == k2 && ij1 < ij2);
}

// the smallest (key, ij) of the workgroup, returned in every thread (256 threads)
__device__ __forceinline__ void nj_block_min(uint64_t &key, uint64_t &ij)
{
    __shared__ uint64_t s_key[kNjThreads / 64], s_ij[kNjThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_down(key, off, 64), oij = __shfl_down(ij, off, 64);
        if (nj_better(ok, oij, key, ij)) {
            key = ok;
            ij = oij;
        }
    }
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) {
        s_key[wave] = key;
        s_ij[wave] = ij;
    }
    __syncthreads();
    key = s_key[0];
    ij = s_ij[0];
#pragma unroll
    for (int w = 1; w < kNjThreads / 64; ++w)
        if (nj_better(s_key[w], s_ij[w], key, ij)) {
            key = s_key[w];
            ij = s_ij[w];
        }
}

__global__ __launch_bounds__(kNjThreads) void nj_init_kernel(double *D, uint64_t n, uint32_t *ids, uint8_t *active,
                                                             unsigned long long *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * kNjThreads + threadIdx.x;
    if (i < n) {
        D[i * n + i] = 0.0;
        ids[i] = (uint32_t)i;
        active[i] = 1;
    }
    if (i == 0)
        *bad = ~0ull;
}

// rows [row0 + blockIdx.y] (below re) of one slab: pair (i, j > i) at slab entry tri_row_start(n, i) - out_base + j - i - 1
template <bool INT>
__global__ __launch_bounds__(kNjThreads) void nj_scatter_kernel(const uint64_t *__restrict__ slab, uint64_t out_base,
                                                                uint64_t n, uint64_t row0, uint64_t re, double *D,
                                                                unsigned long long *bad)
{
    const uint64_t i = row0 + blockIdx.y;
    const uint64_t q = (uint64_t)blockIdx.x * kNjThreads + threadIdx.x;
    if (i >= re || q >= n - i - 1)
        return;
    const uint64_t v = __builtin_nontemporal_load(slab + tri_row_start(n, i) - out_base + q);
    const double d = INT ? (double)(int64_t)v : __longlong_as_double((long long)v);
    const uint64_t j = i + 1 + q;
    D[i * n + j] = d;
    D[j * n + i] = d;
    if (!INT && !isfinite(d))
        __hip_atomic_fetch_min(bad, (unsigned long long)(i * n + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kNjThreads) void nj_mirror_kernel(double *D, uint64_t n, uint64_t row0)
{
    const uint64_t i = row0 + blockIdx.y;
    const uint64_t q = (uint64_t)blockIdx.x * kNjThreads + threadIdx.x;
    if (i >= n || q >= n - i - 1)
        return;
    const uint64_t j = i + 1 + q;
    D[j * n + i] = D[i * n + j];
}

__global__ __launch_bounds__(kNjRowsumThreads) void nj_rowsum_kernel(const double *__restrict__ D, uint64_t P, double *r)
{
    const uint64_t x = (uint64_t)blockIdx.x * kNjRowsumThreads + threadIdx.x;
    if (x >= P)
        return;
    const double *col = D + x;
    double s = 0.0;
    uint64_t k = 0;
    for (; k + 8 <= P; k += 8) {   // eight loads in flight, the adds in order
        double v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
            v[t] = col[(k + t) * P];
#pragma unroll
        for (int t = 0; t < 8; ++t)
            s += v[t];
    }
    for (; k < P; ++k)
        s += col[k * P];
    r[x] = s;
}

// Workgroup w takes rows w, 2G-1-w, 2G+w, 4G-1-w, ... (G workgroups: long and short rows alternate) and the active
// columns j > i of each, 256 lanes across the row (coalesced).  Inactive rows are skipped whole.
__global__ __launch_bounds__(kNjThreads) void nj_scan_kernel(const double *__restrict__ D, uint64_t P, uint32_t m,
                                                             const double *__restrict__ r,
                                                             const uint8_t *__restrict__ active, uint64_t *part_key,
                                                             uint64_t *part_ij)
{
    const double c = (double)(m - 2);
    const uint64_t G = gridDim.x;
    uint64_t bk = ~0ull, bij = ~0ull;
    for (uint64_t t = 0; t * G < P; ++t) {
        const uint64_t i = t * G + ((t & 1) ? G - 1 - blockIdx.x : blockIdx.x);
        if (i >= P || !active[i])
            continue;
        const double ri = r[i];
        const double *row = D + i * P;
        const uint64_t hi = i << 32;
        uint64_t j = i + 1 + threadIdx.x;
        for (; j + 3 * kNjThreads < P; j += 4 * kNjThreads) {
            double d[4], rj[4];
            uint8_t a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                d[u] = row[j + u * kNjThreads];
                rj[u] = r[j + u * kNjThreads];
                a[u] = active[j + u * kNjThreads];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t key = nn_key<false>((uint64_t)__double_as_longlong((c * d[u] - ri) - rj[u]));
                const uint64_t ij = hi | (j + u * kNjThreads);
                if (a[u] && nj_better(key, ij, bk, bij)) {
                    bk = key;
                    bij = ij;
                }
            }
        }
        for (; j < P; j += kNjThreads) {
            if (!active[j])
                continue;
            const uint64_t key = nn_key<false>((uint64_t)__double_as_longlong((c * row[j] - ri) - r[j]));
            if (nj_better(key, hi | j, bk, bij)) {
                bk = key;
                bij = hi | j;
            }
        }
    }
    nj_block_min(bk, bij);
    if (threadIdx.x == 0) {
        part_key[blockIdx.x] = bk;
        part_ij[blockIdx.x] = bij;
    }
}

// Round s with m active nodes; u = n + s is the new node.  Thread k = slot k.
__global__ __launch_bounds__(kNjThreads) void nj_merge_kernel(double *D, uint64_t P, uint32_t m, uint32_t u,
                                                              const uint64_t *__restrict__ part_key,
                                                              const uint64_t *__restrict__ part_ij, uint32_t G,
                                                              const double *__restrict__ r_in, double *r_out,
                                                              uint8_t *active, uint32_t *ids, uint32_t *parent,
                                                              double *length)
{
    uint64_t bk = ~0ull, bij = ~0ull;
    for (uint32_t p = threadIdx.x; p < G; p += kNjThreads)
        if (nj_better(part_key[p], part_ij[p], bk, bij)) {
            bk = part_key[p];
            bij = part_ij[p];
        }
    nj_block_min(bk, bij);
    const uint64_t a = bij >> 32, b = bij & 0xFFFFFFFFull;
    const uint64_t k = (uint64_t)blockIdx.x * kNjThreads + threadIdx.x;
    if (a >= P || b >= P || k >= P || !active[k])
        return;   // (a >= P: no pair was found, which m >= 4 active slots rule out)
    const double dab = D[a * P + b];
    if (k == a) {
        const double ra = r_in[a], rb = r_in[b];
        const double da = dab * 0.5 + (ra - rb) / (double)(2 * (m - 2));
        const double db = dab - da;
        const uint32_t ia = ids[a], ib = ids[b];
        parent[ia] = u;
        length[ia] = da;
        parent[ib] = u;
        length[ib] = db;
        ids[a] = u;
        r_out[a] = ((ra + rb) - (double)m * dab) * 0.5;
        D[a * P + a] = 0.0;
    } else if (k == b) {
        active[b] = 0;
    } else {
        const double dak = D[a * P + k], dbk = D[b * P + k];
        const double duk = ((dak + dbk) - dab) * 0.5;
        D[a * P + k] = duk;
        D[k * P + a] = duk;
        r_out[k] = ((r_in[k] - dak) - dbk) + duk;
    }
}

// pos[x] := the x-th active slot of [0, P), for x < cap.  One workgroup of 1024 threads, each a contiguous chunk.
__global__ __launch_bounds__(1024) void nj_compact_index_kernel(const uint8_t *__restrict__ active, uint64_t P, uint32_t *pos,
                                                                uint32_t cap)
{
    __shared__ uint32_t s_cnt[1024];
    const uint64_t chunk = (P + 1023) / 1024;
    const uint64_t lo = std::min<uint64_t>(threadIdx.x * chunk, P), hi = std::min<uint64_t>(lo + chunk, P);
    uint32_t cnt = 0;
    for (uint64_t x = lo; x < hi; ++x)
        cnt += active[x];
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (unsigned off = 1; off < 1024; off <<= 1) {   // inclusive scan (Hillis-Steele)
        const uint32_t add = threadIdx.x >= off ? s_cnt[threadIdx.x - off] : 0;
        __syncthreads();
        s_cnt[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t o = s_cnt[threadIdx.x] - cnt;
    for (uint64_t x = lo; x < hi; ++x)
        if (active[x] && o < cap)
            pos[o++] = (uint32_t)x;
}

// Dn[x][y] := Do[pos[x]][pos[y]] for x, y < m; ids_n[x] := ids_o[pos[x]]; slots [0, m) active
__global__ __launch_bounds__(kNjThreads) void nj_compact_copy_kernel(const double *__restrict__ Do, uint64_t P, double *Dn,
                                                                     uint64_t m, const uint32_t *__restrict__ pos,
                                                                     const uint32_t *__restrict__ ids_o, uint32_t *ids_n,
                                                                     uint8_t *active)
{
    const uint64_t y = (uint64_t)blockIdx.x * kNjThreads + threadIdx.x;
    if (y >= m)
        return;
    const uint64_t py = pos[y];
    for (uint64_t x = blockIdx.y; x < m; x += gridDim.y) {
        const uint64_t px = pos[x];
        Dn[x * m + y] = Do[px * P + py];
    }
    if (blockIdx.y == 0) {
        ids_n[y] = ids_o[py];
        active[y] = 1;
    }
}

// the last three active slots x < y < z join the root
__global__ void nj_final_kernel(const double *__restrict__ D, uint64_t P, const uint8_t *__restrict__ active,
                                const uint32_t *__restrict__ ids, uint32_t root, uint32_t *parent, double *length)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    uint64_t s[3];
    int found = 0;
    for (uint64_t x = 0; x < P && found < 3; ++x)
        if (active[x])
            s[found++] = x;
    if (found < 3)
        return;
    const double dxy = D[s[0] * P + s[1]], dxz = D[s[0] * P + s[2]], dyz = D[s[1] * P + s[2]];
    const double len[3] = {((dxy + dxz) - dyz) * 0.5, ((dxy + dyz) - dxz) * 0.5, ((dxz + dyz) - dxy) * 0.5};
    for (int t = 0; t < 3; ++t) {
        parent[ids[s[t]]] = root;
        length[ids[s[t]]] = len[t];
    }
    parent[root] = 0xFFFFFFFFu;
    length[root] = 0.0;
}

}  // namespace

hipError_t launch_nj_init(double *D, uint64_t n, uint32_t *ids, uint8_t *active, unsigned long long *bad, hipStream_t stream)
{
    hipLaunchKernelGGL(nj_init_kernel, dim3((unsigned)((n + kNjThreads - 1) / kNjThreads)), dim3(kNjThreads), 0, stream, D, n,
                       ids, active, bad);
    return hipGetLastError();
}

hipError_t launch_nj_scatter(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             double *D, unsigned long long *bad, hipStream_t stream)
{
    if (re <= rb || rb + 1 >= n)
        return hipSuccess;
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    const unsigned chunks = (unsigned)((n - rb - 1 + kNjThreads - 1) / kNjThreads);   // of row rb, the longest
    return for_row_grids(rb, re, [&](uint64_t row0, unsigned rows) {
        const dim3 grid(chunks, rows);
        if (int_payload)
            hipLaunchKernelGGL(nj_scatter_kernel<true>, grid, dim3(kNjThreads), 0, stream, slab, out_base, n, row0, re, D, bad);
        else
            hipLaunchKernelGGL(nj_scatter_kernel<false>, grid, dim3(kNjThreads), 0, stream, slab, out_base, n, row0, re, D, bad);
        return hipGetLastError();
    });
}

hipError_t launch_nj_mirror(double *D, uint64_t n, hipStream_t stream)
{
    if (n < 2)
        return hipSuccess;
    const unsigned chunks = (unsigned)((n + kNjThreads - 1) / kNjThreads);
    // rows 0 .. n - 2 hold the triangle; the grids stay cut from n rows, so the last one carries row n - 1 as well
    return for_row_grids(0, n - 1, [&](uint64_t row0, unsigned) {
        hipLaunchKernelGGL(nj_mirror_kernel, dim3(chunks, grid_rows(n - row0)), dim3(kNjThreads), 0, stream, D, n, row0);
        return hipGetLastError();
    });
}

// Every round of the join on the stream, without a synchronisation: the compaction schedule depends on (n, m) only.
hipError_t launch_nj_rounds(const NjBuffers &b, uint64_t n, hipStream_t stream)
{
    double *Dc = b.D[0], *Do = b.D[1];
    uint32_t *ids_c = b.ids[0], *ids_o = b.ids[1];
    int cr = 0;
    uint64_t P = n;
    hipError_t e;
    auto rowsum = [&]() {
        hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)((P + kNjRowsumThreads - 1) / kNjRowsumThreads)),
                           dim3(kNjRowsumThreads), 0, stream, Dc, P, b.r[cr]);
        return hipGetLastError();
    };
    if ((e = rowsum()) != hipSuccess)
        return e;
    for (uint64_t s = 0; n - s > 3; ++s) {
        const uint64_t m = n - s;
        if (m <= 3 * P / 4) {
            hipLaunchKernelGGL(nj_compact_index_kernel, dim3(1), dim3(1024), 0, stream, b.active, P, b.pos, (uint32_t)m);
            hipLaunchKernelGGL(nj_compact_copy_kernel, dim3((unsigned)((m + kNjThreads - 1) / kNjThreads), grid_rows(m)),
                               dim3(kNjThreads), 0, stream, Dc, P, Do, m, b.pos, ids_c, ids_o, b.active);
            std::swap(Dc, Do);
            std::swap(ids_c, ids_o);
            P = m;
            if ((e = rowsum()) != hipSuccess)
                return e;
        }
        const unsigned G = (unsigned)std::min<uint64_t>(P, kNjScanBlocks);
        hipLaunchKernelGGL(nj_scan_kernel, dim3(G), dim3(kNjThreads), 0, stream, Dc, P, (uint32_t)m, b.r[cr], b.active,
                           b.part_key, b.part_ij);
        hipLaunchKernelGGL(nj_merge_kernel, dim3((unsigned)((P + kNjThreads - 1) / kNjThreads)), dim3(kNjThreads), 0, stream,
                           Dc, P, (uint32_t)m, (uint32_t)(n + s), b.part_key, b.part_ij, G, b.r[cr], b.r[cr ^ 1], b.active,
                           ids_c, b.parent, b.length);
        if ((e = hipGetLastError()) != hipSuccess)
            return e;
        cr ^= 1;
    }
    hipLaunchKernelGGL(nj_final_kernel, dim3(1), dim3(64), 0, stream, Dc, P, b.active, ids_c, (uint32_t)(2 * n - 3), b.parent,
                       b.length);
    return hipGetLastError();
}

}  // namespace dst
