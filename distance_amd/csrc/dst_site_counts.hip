// dst_site_counts.hip — per (site, group) allele counts from the four base planes (dst_site_counts): the
// column side of the library, a positional popcount over planes that are read once.
//
// Mapping (site_counts_kernel).  The records are listed in order of their group (a stable counting sort on the host; no
// list when there are no labels) and the list is cut into STRIPS of at most kSiteStrip records of ONE group.  One block
// = one 128-site chunk x one strip; grid.x walks the chunks of the site range, grid.y the strips (cut by for_row_grids).
// The lanes run along the strip's records: thread t takes records t, t + 256, ... of the strip, kSiteFlushPeriod of
// them at most, so a wave reads 1 KiB per plane and step where the group's records are contiguous and 64 x 16 bytes
// where they are interleaved.
//
// Counting.  Per 32-site word the five class masks come from word logic: one base exactly, K = (a^g^c^t) & ~((a&g)|(c&t))
// (window_counts_kernel's), then K&a, K&t, K&g, K&c; missing a&g&c&t; ambiguous what is left of a|g|c|t.  Sites outside
// [site_begin, site_end) leave every mask (window_mask), and a lane without a record adds zeros.  A lane adds its masks
// into kSitePlanes carry-save planes per (class, word): plane p holds bit p of the lane's count of every site of the word,
// so one record costs two word operations per plane whatever it holds.  kSiteFlushPeriod = 2^kSitePlanes - 1 records
// fill the planes exactly: no lane takes more, so no count is ever carried out of them.
//
// Flush, once per block.  The 64 lanes' bit-sliced counts are added with full adders over shuffles: the first step hands
// each half of the wave one word of a pair (lanes 0-31 keep the even word, lanes 32-63 the odd one), five more add the
// halves' lanes, and kSitePlanes + 6 planes hold the wave's count (at most 64 x 15 = 960).  Lane l then reads bit l % 32
// out of the planes: the count of one site.  The four waves meet in LDS, and the block adds what is not zero to the
// counts in device memory, laid out as the caller gets them, with 32-bit integer atomics: the answer does not depend on
// the order of anything.
#include <cstring>

#include "dst_ctx.h"
#include "dst_device.hpp"
#include "dst_window_sweep.hpp"

namespace dst {
namespace {

constexpr int kSitePlanes = 4;                                     // carry-save planes of a lane
constexpr uint32_t kSiteFlushPeriod = DST_SITE_FLUSH_PERIOD;       // records a lane counts before the flush
constexpr uint32_t kSiteThreads = 256;
constexpr uint32_t kSiteStrip = DST_SITE_STRIP_RECORDS;            // records of one block
constexpr int kSiteWavePlanes = kSitePlanes + 6;                   // planes of a wave's count
static_assert(kSiteFlushPeriod == (1u << kSitePlanes) - 1u, "a lane's planes hold exactly the flush period");
static_assert(kSiteStrip == kSiteThreads * kSiteFlushPeriod, "a strip is one flush period of every thread");
static_assert(DST_SITE_CLASSES == 5, "A, T, G, C, ambiguous");

struct SiteStrip {
    uint32_t first;   // the strip's first entry of the record list
    uint32_t count;   // 1 .. kSiteStrip
    uint32_t group;
    uint32_t unused;
};

// c (planes of a count) += m (one bit per site)
__device__ __forceinline__ void add_mask(uint32_t (&c)[kSitePlanes], uint32_t m)
{
#pragma unroll
    for (int p = 0; p < kSitePlanes; ++p) {
        const uint32_t carry = c[p] & m;
        c[p] ^= m;
        m = carry;
    }
}

// the N planes of p plus those of the lane `off` away: N + 1 planes
template <int N>
__device__ __forceinline__ void add_lane(uint32_t (&p)[kSiteWavePlanes], int off)
{
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint32_t y = (uint32_t)__shfl_xor((int)p[i], off, 64);
        const uint32_t x = p[i] ^ y;
        p[i] = x ^ carry;
        carry = (x & carry) | (y & ~x);   // majority(p, y, carry): where p != y the carry decides, else y
    }
    p[N] = carry;
}

__global__ __launch_bounds__(kSiteThreads) void site_counts_kernel(const uint4 *__restrict__ planes, const uint32_t *__restrict__ order,
                                                                   const SiteStrip *__restrict__ strips, uint32_t nchunks,
                                                                   uint32_t npad, uint32_t chunk0, uint32_t strip0,
                                                                   uint32_t site_begin, uint32_t site_end, uint32_t n_groups,
                                                                   uint32_t *__restrict__ counts)
{
    __shared__ uint32_t tot[DST_SITE_CLASSES * kChunkSites];
    const uint32_t c = chunk0 + blockIdx.x;
    const SiteStrip strip = strips[strip0 + blockIdx.y];
    for (uint32_t e = threadIdx.x; e < DST_SITE_CLASSES * kChunkSites; e += kSiteThreads)
        tot[e] = 0;
    uint32_t m[4];
    window_mask(c, site_begin, site_end, m);

    uint32_t cs[DST_SITE_CLASSES][4][kSitePlanes];
#pragma unroll
    for (int k = 0; k < DST_SITE_CLASSES; ++k)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int p = 0; p < kSitePlanes; ++p)
                cs[k][w][p] = 0;

    const size_t ps = (size_t)nchunks * npad;   // plane stride, in uint4
    const uint4 *base = planes + (size_t)c * npad;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // the next record's words are asked for before this one's are counted
    uint4 nA = zero, nG = zero, nC = zero, nT = zero;
    if (threadIdx.x < strip.count) {
        const uint32_t at = strip.first + threadIdx.x;
        const uint32_t r = order ? order[at] : at;
        nA = base[PL_A * ps + r], nG = base[PL_G * ps + r], nC = base[PL_C * ps + r], nT = base[PL_T * ps + r];
    }
#pragma unroll 1
    for (uint32_t step = 0; step < kSiteFlushPeriod; ++step) {
        if (step * kSiteThreads >= strip.count)
            break;   // (block-uniform)
        const uint4 A = nA, G = nG, C = nC, T = nT;
        nA = nG = nC = nT = zero;
        const uint32_t next = (step + 1) * kSiteThreads + threadIdx.x;
        if (step + 1 < kSiteFlushPeriod && next < strip.count) {
            const uint32_t at = strip.first + next;
            const uint32_t r = order ? order[at] : at;
            nA = base[PL_A * ps + r], nG = base[PL_G * ps + r], nC = base[PL_C * ps + r], nT = base[PL_T * ps + r];
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t a = word_of(A, w), g = word_of(G, w), cc = word_of(C, w), t = word_of(T, w);
            const uint32_t K = (a ^ g ^ cc ^ t) & ~((a & g) | (cc & t)) & m[w];   // exactly one base, inside the range
            const uint32_t missing = a & g & cc & t;
            const uint32_t ambiguous = (a | g | cc | t) & ~K & ~missing & m[w];
            add_mask(cs[0][w], K & a);
            add_mask(cs[1][w], K & t);
            add_mask(cs[2][w], K & g);
            add_mask(cs[3][w], K & cc);
            add_mask(cs[4][w], ambiguous);
        }
    }

    __syncthreads();   // (tot is zero)
    const uint32_t lane = threadIdx.x & 63u;
    const bool upper = lane >= 32u;
#pragma unroll
    for (int k = 0; k < DST_SITE_CLASSES; ++k)
#pragma unroll
        for (int wp = 0; wp < 2; ++wp) {
            // lanes 0-31 keep word 2 wp and give word 2 wp + 1 away, lanes 32-63 the other way round
            uint32_t p[kSiteWavePlanes];
            uint32_t carry = 0;
#pragma unroll
            for (int i = 0; i < kSitePlanes; ++i) {
                const uint32_t mine = upper ? cs[k][2 * wp + 1][i] : cs[k][2 * wp][i];
                const uint32_t given = upper ? cs[k][2 * wp][i] : cs[k][2 * wp + 1][i];
                const uint32_t y = (uint32_t)__shfl_xor((int)given, 32, 64);
                const uint32_t x = mine ^ y;
                p[i] = x ^ carry;
                carry = (x & carry) | (y & ~x);
            }
            p[kSitePlanes] = carry;
            add_lane<kSitePlanes + 1>(p, 16);
            add_lane<kSitePlanes + 2>(p, 8);
            add_lane<kSitePlanes + 3>(p, 4);
            add_lane<kSitePlanes + 4>(p, 2);
            add_lane<kSitePlanes + 5>(p, 1);
            const uint32_t bit = lane & 31u;
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < kSiteWavePlanes; ++i)
                v |= ((p[i] >> bit) & 1u) << i;
            if (v)
                atomicAdd(&tot[k * kChunkSites + (2 * wp + (upper ? 1 : 0)) * 32 + bit], v);
        }
    __syncthreads();
    // entry (site, class) of the chunk, site-major: one group's entries of a chunk are 640 adjacent words
    for (uint32_t e = threadIdx.x; e < DST_SITE_CLASSES * kChunkSites; e += kSiteThreads) {
        const uint32_t bit = e / DST_SITE_CLASSES, k = e % DST_SITE_CLASSES;
        const uint32_t v = tot[k * kChunkSites + bit];
        if (v) {   // (so the site is inside the range: nothing else was counted)
            const uint64_t site = (uint64_t)c * kChunkSites + bit - site_begin;
            __hip_atomic_fetch_add(counts + (site * n_groups + strip.group) * DST_SITE_CLASSES + k, v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

const char *const kSharedRefusal = "a set uploaded with dst_upload_shared runs on the consensus path only (this rank holds "
                                   "the planes of its own records)";

}  // namespace
}  // namespace dst

extern "C" int dst_site_counts(dst_ctx *ctx, int slot, const uint32_t *group, uint32_t n_groups, uint64_t site_begin,
                               uint64_t site_end, uint32_t *counts, size_t cap_entries)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (!counts)
        return fail(ctx, DST_ERR_ARG, "null counts pointer");
    if (slot < 0 || slot > 1)
        return fail(ctx, DST_ERR_ARG, "slot must be 0 or 1");
    if (n_groups == 0 || n_groups > DST_GROUPS_MAX)
        return fail(ctx, DST_ERR_ARG, "a group count must be between 1 and " + std::to_string(DST_GROUPS_MAX));
    if (!group && n_groups != 1)
        return fail(ctx, DST_ERR_ARG, "site counts: without labels there is one group (n_groups must be 1)");
    DeviceSet &s = ctx->set[slot];
    if (!s.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    if (s.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    if (site_begin > site_end || site_end > s.len)
        return fail(ctx, DST_ERR_ARG, "site counts: [" + std::to_string(site_begin) + ", " + std::to_string(site_end) +
                                          ") is not a site range of an alignment of " + std::to_string(s.len) + " sites");
    if (s.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_site_counts");
    if (s.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    const uint64_t n = s.n;
    std::vector<uint64_t> size(n_groups, 0);
    if (!group)
        size[0] = n;
    for (uint64_t x = 0; group && x < n; ++x) {
        if (group[x] == DST_GROUP_NONE)
            continue;
        if (group[x] >= n_groups)
            return fail(ctx, DST_ERR_ARG, "site counts: record " + std::to_string(x) + " has label " + std::to_string(group[x]) +
                                              ", which is neither below the group count " + std::to_string(n_groups) +
                                              " nor DST_GROUP_NONE");
        ++size[group[x]];
    }
    const uint64_t span = site_end - site_begin;
    const unsigned __int128 need = (unsigned __int128)span * n_groups * DST_SITE_CLASSES;
    if (need > (unsigned __int128)cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "counts buffer too small: (site_end - site_begin) x n_groups x 5 entries");
    const size_t entries = (size_t)need;
    std::memset(counts, 0, entries * sizeof(uint32_t));
    uint64_t assigned = 0;
    for (uint64_t g : size)
        assigned += g;
    if (entries == 0 || assigned == 0)
        return DST_OK;   // (no launch)

    // the strips: every group's records in order, cut at kSiteStrip
    uint64_t n_strips = 0;
    for (uint64_t g : size)
        n_strips += (g + kSiteStrip - 1) / kSiteStrip;
    const size_t counts_bytes = (entries * sizeof(uint32_t) + 255) / 256 * 256;
    const size_t order_bytes = group ? ((size_t)assigned * sizeof(uint32_t) + 255) / 256 * 256 : 0;
    const size_t strip_bytes = (size_t)n_strips * sizeof(SiteStrip);
    const size_t stage_bytes = order_bytes + strip_bytes, work_bytes = counts_bytes + stage_bytes;

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipStreamSynchronize(stream));   // (the work and staging buffers' earlier readers)
    if (int rc = order_after_prep(ctx, stream))
        return rc;
    if (int rc = ensure_planes(ctx, s, stream))
        return rc;
    if (ctx->site_work.grow(ctx, work_bytes)) {
        (void)hipGetLastError();
        return fail(ctx, DST_ERR_NOMEM, "site counts: cannot allocate " + std::to_string(work_bytes) + " bytes of device memory");
    }
    if (int rc = ctx->site_host.grow(ctx, stage_bytes, "site counts"))
        return rc;
    char *stage = ctx->site_host;
    uint32_t *h_order = reinterpret_cast<uint32_t *>(stage);
    SiteStrip *h_strips = reinterpret_cast<SiteStrip *>(stage + order_bytes);
    {
        std::vector<uint64_t> first(n_groups, 0);
        for (uint32_t g = 1; g < n_groups; ++g)
            first[g] = first[g - 1] + size[g - 1];
        uint64_t k = 0;
        for (uint32_t g = 0; g < n_groups; ++g)
            for (uint64_t at = 0; at < size[g]; at += kSiteStrip)
                h_strips[k++] = SiteStrip{(uint32_t)(first[g] + at), (uint32_t)std::min<uint64_t>(kSiteStrip, size[g] - at), g, 0};
        if (group) {
            std::vector<uint64_t> next = first;
            for (uint64_t x = 0; x < n; ++x)
                if (group[x] != DST_GROUP_NONE)
                    h_order[next[group[x]]++] = (uint32_t)x;
        }
    }
    char *dev = static_cast<char *>(ctx->site_work.ptr);
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(dev);
    const uint32_t *d_order = group ? reinterpret_cast<const uint32_t *>(dev + counts_bytes) : nullptr;
    const SiteStrip *d_strips = reinterpret_cast<const SiteStrip *>(dev + counts_bytes + order_bytes);
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, entries * sizeof(uint32_t), stream));
    HIP_TRY(ctx, hipMemcpyAsync(dev + counts_bytes, stage, stage_bytes, hipMemcpyHostToDevice, stream));
    const uint32_t c_first = (uint32_t)(site_begin / kChunkSites), c_last = (uint32_t)((site_end - 1) / kChunkSites);
    HIP_TRY(ctx, for_row_grids(0, n_strips, [&](uint64_t strip0, unsigned ns) {
                hipLaunchKernelGGL(site_counts_kernel, dim3(c_last - c_first + 1, ns), dim3(kSiteThreads), 0, stream, s.planes, d_order,
                                   d_strips, (uint32_t)s.nchunks, (uint32_t)s.npad, c_first, (uint32_t)strip0, (uint32_t)site_begin,
                                   (uint32_t)site_end, n_groups, d_counts);
                return hipGetLastError();
            }));
    HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, entries * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}
