// dst_pair_sites.hip — the difference sites of a list of pairs (dst_pair_sites): a gather over the base planes of the two
// records of every pair, with a variable-length output, compacted by the count / scan / windowed-write pattern of
// dst_links.hip.
//
// Definition.  a, b = the high nibbles of the row and the column record at a site (planes A, G, C, T = bits 8, 4, 2, 1).
// The site is listed for measure M when it adds 1 to M's difference tally (dst_site_tallies):
//   n, n_high, raw, jc69   (a & b) == 0
//   k80                    ... and each of a, b has bases of one class only: purines {A, G} or pyrimidines {C, T}
//   tn93                   ... and each of a, b is exactly one base
// all of it bitwise on 128 sites at a time.  Sites at or beyond len are masked, whatever the padding holds.
//
// Mapping: one wave per pair, four pairs (consecutive in the list) per workgroup, the lanes along the pair's 128-site
// chunks: lane l takes chunks l, l + 64, ...  A record's 16 bytes of a (plane, chunk) lie npad x 16 bytes from the next
// chunk's, so every lane's load is its own cache line whichever way the lanes are laid out; what a sorted pair list gives is
// reuse: the row record's lines are shared by the waves of a workgroup and by its neighbours, and column records within 8
// of each other share lines.
//
//   pair_sites_count_kernel   counts[e] = the listed sites of pair e (at most len < 2^32)
//   pair_sites_scan_kernel    one workgroup: the exclusive scan into 64-bit offsets, offsets[pairs] = the batch's total
//   pair_sites_write_kernel   a rank window [lo, hi): a wave whose pair's [offset, offset + count) does not meet it leaves
//                             after reading its two offsets; any other walks the chunks again, ranks its sites (per step the
//                             lanes' popcounts scanned over the wave: rank order is site order) and writes the site and
//                             a << 4 | b at offset + rank - lo.  Plain vector stores; two entries never share a place.
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kPsWaves = 4;   // pairs per workgroup
constexpr int kPsScanThreads = 1024;

struct PairPlanes {
    const uint4 *row, *col;       // the sets' planes
    uint64_t row_npad, col_npad;
    uint32_t nchunks;
    uint32_t len;
};

__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 not4(uint4 a) { return make_uint4(~a.x, ~a.y, ~a.z, ~a.w); }
__device__ __forceinline__ uint32_t pop4(uint4 a) { return (uint32_t)(__popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w)); }

// the sites of chunk c below len, as a mask
__device__ __forceinline__ uint4 valid_sites(uint32_t c, uint32_t len)
{
    const uint64_t s0 = (uint64_t)c * kChunkSites;
    const uint32_t left = s0 >= len ? 0u : len - s0 >= kChunkSites ? kChunkSites : (uint32_t)(len - s0);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t in = left > 32u * k ? left - 32u * k : 0u;
        w[k] = in >= 32u ? 0xFFFFFFFFu : (1u << in) - 1u;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// planes A, G, C, T of record `rec`, chunk c
__device__ __forceinline__ void load_bases(const uint4 *__restrict__ planes, uint64_t npad, uint32_t nchunks, uint32_t c, uint32_t rec,
                                           uint4 (&x)[4])
{
#pragma unroll
    for (int p = 0; p < 4; ++p)
        x[p] = planes[((uint64_t)p * nchunks + c) * npad + rec];
}

// one base class only: (A | G) ^ (C | T); exactly one base: odd parity and neither class complete
__device__ __forceinline__ uint4 one_class(const uint4 (&x)[4]) { return xor4(or4(x[0], x[1]), or4(x[2], x[3])); }
__device__ __forceinline__ uint4 one_base(const uint4 (&x)[4])
{
    return and4(xor4(xor4(x[0], x[1]), xor4(x[2], x[3])), not4(or4(and4(x[0], x[1]), and4(x[2], x[3]))));
}

template <int FAM>
__device__ __forceinline__ uint4 listed_sites(const uint4 (&q)[4], const uint4 (&t)[4], uint4 valid)
{
    uint4 m = and4(valid, not4(or4(or4(and4(q[0], t[0]), and4(q[1], t[1])), or4(and4(q[2], t[2]), and4(q[3], t[3])))));
    if constexpr (FAM == FAM_K80)
        m = and4(m, and4(one_class(q), one_class(t)));
    if constexpr (FAM == FAM_TN93)
        m = and4(m, and4(one_base(q), one_base(t)));
    return m;
}

template <int FAM>
__global__ __launch_bounds__(64 * kPsWaves) void pair_sites_count_kernel(PairPlanes g, const uint32_t *__restrict__ row,
                                                                          const uint32_t *__restrict__ col, uint32_t pairs,
                                                                          uint32_t *__restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t)blockIdx.x * kPsWaves + (threadIdx.x >> 6);
    if (e >= pairs)
        return;   // (whole waves)
    const uint32_t i = row[e], j = col[e];
    uint32_t count = 0;
    for (uint32_t c = lane; c < g.nchunks; c += 64u) {
        uint4 q[4], t[4];
        load_bases(g.row, g.row_npad, g.nchunks, c, i, q);
        load_bases(g.col, g.col_npad, g.nchunks, c, j, t);
        count += pop4(listed_sites<FAM>(q, t, valid_sites(c, g.len)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        count += (uint32_t)__shfl_down((int)count, off, 64);
    if (lane == 0)
        counts[e] = count;
}

// One workgroup.  offsets[e] = counts[0] + .. + counts[e - 1] for e <= pairs (links_scan_kernel's scheme).
__global__ __launch_bounds__(kPsScanThreads) void pair_sites_scan_kernel(const uint32_t *__restrict__ counts, uint32_t pairs,
                                                                         uint64_t *__restrict__ offsets)
{
    __shared__ uint64_t wave_sum[kPsScanThreads / 64];
    __shared__ uint64_t carry_s;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0)
        carry_s = 0;
    __syncthreads();
    for (uint32_t e0 = 0; e0 < pairs; e0 += kPsScanThreads) {
        const uint32_t e = e0 + threadIdx.x;
        const uint64_t own = e < pairs ? counts[e] : 0;
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
        if (e < pairs)
            offsets[e] = before + incl - own;
        __syncthreads();   // (everybody has read carry_s and wave_sum)
        if (threadIdx.x == kPsScanThreads - 1)
            carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        offsets[pairs] = carry_s;
}

template <int FAM>
__global__ __launch_bounds__(64 * kPsWaves) void pair_sites_write_kernel(PairPlanes g, const uint32_t *__restrict__ row,
                                                                          const uint32_t *__restrict__ col, uint32_t pairs,
                                                                          const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi,
                                                                          uint32_t *__restrict__ sites, uint8_t *__restrict__ bases)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t e = (uint64_t)blockIdx.x * kPsWaves + (threadIdx.x >> 6);
    if (e >= pairs)
        return;   // (whole waves)
    const uint64_t first = offsets[e], next = offsets[e + 1];
    if (next == first || next <= lo || first >= hi)
        return;   // (whole waves) no entry of this pair inside the window: the planes are not touched
    const uint32_t i = row[e], j = col[e];
    uint64_t at = first;   // the rank of the step's first entry
    // every lane of the wave takes every step (a lane past the last chunk with an empty mask): the scan needs them all
    for (uint32_t c0 = 0; c0 < g.nchunks && at < hi; c0 += 64u) {
        const uint32_t c = c0 + lane;
        uint4 q[4] = {}, t[4] = {}, m = make_uint4(0, 0, 0, 0);
        if (c < g.nchunks) {
            load_bases(g.row, g.row_npad, g.nchunks, c, i, q);
            load_bases(g.col, g.col_npad, g.nchunks, c, j, t);
            m = listed_sites<FAM>(q, t, valid_sites(c, g.len));
        }
        const uint32_t own = pop4(m);
        uint32_t incl = own;   // inclusive scan over the wave: a step holds at most 64 x 128 entries
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= (uint32_t)off)
                incl += up;
        }
        const uint32_t step_total = (uint32_t)__shfl((int)incl, 63, 64);
        uint64_t r = at + (incl - own);
        at += step_total;
        if (own == 0 || at <= lo)
            continue;   // (this lane has none, or the step's entries all lie below the window; `at` is the wave's)
        const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
        const uint32_t s0 = c * kChunkSites;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t w = mw[k];
            const uint32_t qa = k == 0 ? q[0].x : k == 1 ? q[0].y : k == 2 ? q[0].z : q[0].w;
            const uint32_t qg = k == 0 ? q[1].x : k == 1 ? q[1].y : k == 2 ? q[1].z : q[1].w;
            const uint32_t qc = k == 0 ? q[2].x : k == 1 ? q[2].y : k == 2 ? q[2].z : q[2].w;
            const uint32_t qt = k == 0 ? q[3].x : k == 1 ? q[3].y : k == 2 ? q[3].z : q[3].w;
            const uint32_t ta = k == 0 ? t[0].x : k == 1 ? t[0].y : k == 2 ? t[0].z : t[0].w;
            const uint32_t tg = k == 0 ? t[1].x : k == 1 ? t[1].y : k == 2 ? t[1].z : t[1].w;
            const uint32_t tc = k == 0 ? t[2].x : k == 1 ? t[2].y : k == 2 ? t[2].z : t[2].w;
            const uint32_t tt = k == 0 ? t[3].x : k == 1 ? t[3].y : k == 2 ? t[3].z : t[3].w;
            while (w) {
                const uint32_t s = (uint32_t)__ffs((int)w) - 1u;
                w &= w - 1u;
                if (r >= lo && r < hi) {
                    const uint32_t a = ((qa >> s) & 1u) << 3 | ((qg >> s) & 1u) << 2 | ((qc >> s) & 1u) << 1 | ((qt >> s) & 1u);
                    const uint32_t b = ((ta >> s) & 1u) << 3 | ((tg >> s) & 1u) << 2 | ((tc >> s) & 1u) << 1 | ((tt >> s) & 1u);
                    sites[r - lo] = s0 + 32u * k + s;
                    bases[r - lo] = (uint8_t)(a << 4 | b);
                }
                ++r;
            }
        }
    }
}

}  // namespace

static PairPlanes pair_planes(const DeviceSet &rows, const DeviceSet &cols)
{
    PairPlanes g;
    g.row = rows.planes;
    g.col = cols.planes;
    g.row_npad = rows.npad;
    g.col_npad = cols.npad;
    g.nchunks = (uint32_t)rows.nchunks;
    g.len = (uint32_t)rows.len;
    return g;
}

#define DST_PAIR_SITES_FAMILY(measure, CALL)                         \
    switch (family_of(measure)) {                                   \
    case FAM_NHIGH:                                                  \
    case FAM_RAW: CALL(FAM_NHIGH); break;                            \
    case FAM_K80: CALL(FAM_K80); break;                              \
    case FAM_TN93: CALL(FAM_TN93); break;                            \
    default: return hipErrorInvalidValue;                            \
    }

hipError_t launch_pair_sites_count(int measure, const DeviceSet &rows, const DeviceSet &cols, uint32_t pairs, const PairSitesBuffers &b,
                                   hipStream_t stream)
{
    if (pairs == 0 || pairs > DST_PAIR_SITES_BATCH || rows.nchunks != cols.nchunks || rows.len != cols.len ||
        rows.len > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const PairPlanes g = pair_planes(rows, cols);
    const dim3 grid((pairs + kPsWaves - 1) / kPsWaves);
#define DST_PS_COUNT(F) \
    hipLaunchKernelGGL((pair_sites_count_kernel<F>), grid, dim3(64 * kPsWaves), 0, stream, g, b.row, b.col, pairs, b.counts)
    DST_PAIR_SITES_FAMILY(measure, DST_PS_COUNT)
#undef DST_PS_COUNT
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(pair_sites_scan_kernel, dim3(1), dim3(kPsScanThreads), 0, stream, b.counts, pairs, b.offsets);
    return hipGetLastError();
}

hipError_t launch_pair_sites_write(int measure, const DeviceSet &rows, const DeviceSet &cols, uint32_t pairs, const PairSitesBuffers &b,
                                   uint64_t lo, uint64_t hi, hipStream_t stream)
{
    if (pairs == 0 || pairs > DST_PAIR_SITES_BATCH || hi <= lo || hi - lo > DST_PAIR_SITES_WINDOW || rows.nchunks != cols.nchunks ||
        rows.len != cols.len || rows.len > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const PairPlanes g = pair_planes(rows, cols);
    const dim3 grid((pairs + kPsWaves - 1) / kPsWaves);
#define DST_PS_WRITE(F)                                                                                                       \
    hipLaunchKernelGGL((pair_sites_write_kernel<F>), grid, dim3(64 * kPsWaves), 0, stream, g, b.row, b.col, pairs, b.offsets, lo, hi, \
                       b.sites, b.bases)
    DST_PAIR_SITES_FAMILY(measure, DST_PS_WRITE)
#undef DST_PS_WRITE
    return hipGetLastError();
}

#undef DST_PAIR_SITES_FAMILY

}  // namespace dst
