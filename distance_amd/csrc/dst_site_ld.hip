// dst_site_ld.hip — linkage disequilibrium between listed sites (dst_site_ld, dst_site_ld_links): the
// all-pairs job with the roles of sites and records swapped.  Per pair of listed positions p < q four exact integers
// {m, a, b, c} = {|C_p & C_q|, |M_p & C_q|, |C_p & M_q|, |M_p & M_q|}, C_p the records with a single-base call at the site,
// M_p those of them whose base is not the position's reference allele (include/distance_hip.h).
//
//   ld_vectors_kernel   the planes transposed for the listed sites: vec[C or M][position][word], 64 records per 64-bit
//                       word.  Lanes along the records (as site_counts_kernel): a wave reads 64 records' 16-byte words of
//                       one 128-site chunk, forms K (one base exactly) and K & "not the reference allele" per 32-site word
//                       from the chunk's four reference words, clears the records that do not take part (padding records
//                       and those of other groups), and takes one __ballot per listed bit of the chunk and set.  A
//                       workgroup covers kLdKStep words (512 records) of one listed chunk, through LDS, so a position's
//                       words leave as 64 contiguous bytes.  Chunks without a listed site are never visited.  The words
//                       past the last record, up to a multiple of kLdKStep, are written as zeros here.
//   ld_tile_kernel      a workgroup owns kLdTile x kLdTile positions (tile column >= tile row), thread (tx, ty) the rows
//                       4 ty .. 4 ty + 3 against the columns tx, tx + 16, tx + 32, tx + 48: 16 pairs x 4 tallies in
//                       registers.  The K loop runs over the record words in steps of kLdKStep: the tile's C and M rows
//                       of both sides go to LDS as [word][position] (rows padded to kLdRowPad words: the staging stores
//                       of a 16-lane group then fall on 32 different banks), the next step's 16 bytes per array wait in
//                       registers meanwhile.  Per word a thread reads its four row positions with two 16-byte loads per
//                       set (one address per ty: a broadcast) and its four columns with 8-byte loads (16 lanes = 128
//                       contiguous bytes), then per pair four ANDs and four 64-bit popcounts.  Zero words add nothing:
//                       no record tail.  The epilogue writes one uint4 per pair to tri_row_start(S, p) - base + (q - p -
//                       1), masked to p < q < S and to the slab's rows; 16 lanes write 256 contiguous bytes.
//   ld_count_kernel, ld_write_kernel   dst_links.hip's order-preserving compaction over a slab of tallies: block counts in
//                       canonical order, links_scan_kernel, a windowed write by ballot rank.  The test is dst_ld_finalize's
//                       r2 in f64, the same operations in the same order (the library is compiled -ffp-contract=off).
#include <cmath>
#include <cstring>

#include "dst_ctx.h"
#include "dst_device.hpp"
#include "dst_window_sweep.hpp"

namespace dst {
namespace {

constexpr uint32_t kLdTile = 64;                 // positions of a tile side
constexpr uint32_t kLdKStep = 8;                 // record words (of 64 records) staged per step
constexpr uint32_t kLdRowPad = kLdTile + 2;      // words of an LDS row
constexpr uint32_t kLdThreads = 256;
constexpr uint64_t kLdSlabPairs = (uint64_t)1 << 24;   // 256 MiB of tallies
constexpr int kLdWaves = 4, kLdSteps = 8;        // the compaction's geometry: dst_links.hip's
constexpr uint32_t kLdWavePairs = 64u * kLdSteps;
constexpr uint32_t kLdBlockPairs = kLdWavePairs * kLdWaves;
static_assert(kLdKStep == 2 * (kLdThreads / kLdTile), "a staging thread takes two words of one position");
static_assert(kLdKStep == 2 * (kLdThreads / 64), "a wave of ld_vectors_kernel takes two words");

// one listed chunk: its positions first .. first + count - 1 of the list, and per base (A, T, G, C) the bits of its sites
// whose reference allele is that base
struct LdChunk {
    uint32_t chunk, first, count, unused;
    uint32_t ref[4][4];
};

__global__ __launch_bounds__(kLdThreads) void ld_vectors_kernel(const uint4 *__restrict__ planes, uint32_t nchunks, uint32_t npad,
                                                                uint32_t n, const LdChunk *__restrict__ chunks, uint32_t chunk0,
                                                                const uint32_t *__restrict__ sites,
                                                                const uint32_t *__restrict__ group, uint32_t which, uint32_t wpad,
                                                                uint64_t *__restrict__ vec_c, uint64_t *__restrict__ vec_m)
{
    __shared__ uint64_t out[2][kChunkSites][kLdKStep];
    const LdChunk ch = chunks[chunk0 + blockIdx.y];
    const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)ch.count);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t ps = (size_t)nchunks * npad;
    const uint4 *base = planes + (size_t)ch.chunk * npad;
#pragma unroll 1
    for (uint32_t i = 0; i < 2; ++i) {
        const uint32_t wl = wave * 2 + i;
        const uint64_t r = ((uint64_t)blockIdx.x * kLdKStep + wl) * 64 + lane;
        // a record past the set's last, or of another group, is in no set: its planes are not read
        const bool takes_part = r < n && (!group || group[r] == which);
        uint4 A = make_uint4(0, 0, 0, 0), G = A, C = A, T = A;
        if (takes_part)
            A = base[PL_A * ps + r], G = base[PL_G * ps + r], C = base[PL_C * ps + r], T = base[PL_T * ps + r];
        uint32_t K[4], M[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t a = word_of(A, w), g = word_of(G, w), cc = word_of(C, w), t = word_of(T, w);
            K[w] = (a ^ g ^ cc ^ t) & ~((a & g) | (cc & t));   // exactly one base (site_counts_kernel's K)
            M[w] = K[w] & ~((a & ch.ref[0][w]) | (t & ch.ref[1][w]) | (g & ch.ref[2][w]) | (cc & ch.ref[3][w]));
        }
#pragma unroll 1
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t bit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sites[ch.first + k] % kChunkSites));
            const uint32_t w = bit >> 5, sh = bit & 31u;
            const uint32_t kw = w == 0 ? K[0] : w == 1 ? K[1] : w == 2 ? K[2] : K[3];
            const uint32_t mw = w == 0 ? M[0] : w == 1 ? M[1] : w == 2 ? M[2] : M[3];
            const uint64_t bc = __ballot((kw >> sh) & 1u), bm = __ballot((mw >> sh) & 1u);
            if (lane == 0) {
                out[0][k][wl] = bc;
                out[1][k][wl] = bm;
            }
        }
    }
    __syncthreads();
    const uint32_t each = count * kLdKStep;
    for (uint32_t e = threadIdx.x; e < 2 * each; e += kLdThreads) {
        const uint32_t set = e >= each ? 1u : 0u, rest = e - set * each, k = rest / kLdKStep, wl = rest % kLdKStep;
        uint64_t *vec = set ? vec_m : vec_c;
        vec[(size_t)(ch.first + k) * wpad + (size_t)blockIdx.x * kLdKStep + wl] = out[set][k][wl];
    }
}

// the tile body: the staging, the K loop and the 4 x 4 register tile of tile (ti, tj); what becomes of the 16 pairs x 4
// tallies of thread (tx, ty) is the epilogue's: epi(acc, ti, tj, tx, ty, lds), lds the body's staging block (kLdLdsBytes bytes),
// free once the workgroup has passed a barrier.  Every thread of the workgroup reaches the epilogue.
constexpr uint32_t kLdLdsBytes = 4 * kLdKStep * kLdRowPad * 8;
template <class Epilogue>
__device__ __forceinline__ void ld_tile_body(const uint64_t *__restrict__ vec_c, const uint64_t *__restrict__ vec_m, uint32_t wpad,
                                             uint32_t ti, uint32_t tj, const Epilogue &epi)
{
    __shared__ __attribute__((aligned(16))) uint64_t sh[4][kLdKStep][kLdRowPad];   // the rows' C, M, the columns' C, M
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    // staging: thread = (position sp of the tile, words 2 sj and 2 sj + 1 of the step), four lanes read 64 contiguous bytes
    const uint32_t sp = threadIdx.x >> 2, sj = threadIdx.x & 3u;
    const size_t row_at = (size_t)(ti * kLdTile + sp) * wpad + 2 * sj, col_at = (size_t)(tj * kLdTile + sp) * wpad + 2 * sj;
    const ulonglong2 *g0 = reinterpret_cast<const ulonglong2 *>(vec_c + row_at), *g1 = reinterpret_cast<const ulonglong2 *>(vec_m + row_at);
    const ulonglong2 *g2 = reinterpret_cast<const ulonglong2 *>(vec_c + col_at), *g3 = reinterpret_cast<const ulonglong2 *>(vec_m + col_at);
    ulonglong2 n0 = g0[0], n1 = g1[0], n2 = g2[0], n3 = g3[0];

    uint32_t acc[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                acc[a][b][k] = 0;

#pragma unroll 1
    for (uint32_t k0 = 0; k0 < wpad; k0 += kLdKStep) {
        __syncthreads();   // (the step before has been read)
        sh[0][2 * sj][sp] = n0.x, sh[0][2 * sj + 1][sp] = n0.y;
        sh[1][2 * sj][sp] = n1.x, sh[1][2 * sj + 1][sp] = n1.y;
        sh[2][2 * sj][sp] = n2.x, sh[2][2 * sj + 1][sp] = n2.y;
        sh[3][2 * sj][sp] = n3.x, sh[3][2 * sj + 1][sp] = n3.y;
        __syncthreads();
        if (k0 + kLdKStep < wpad) {   // the next step's words, asked for before this one is counted
            const uint32_t at = (k0 + kLdKStep) / 2;
            n0 = g0[at], n1 = g1[at], n2 = g2[at], n3 = g3[at];
        }
#pragma unroll 1
        for (uint32_t k = 0; k < kLdKStep; ++k) {
            uint64_t rc[4], rm[4], cc[4], cm[4];
            const ulonglong2 c01 = *reinterpret_cast<const ulonglong2 *>(&sh[0][k][4 * ty]);
            const ulonglong2 c23 = *reinterpret_cast<const ulonglong2 *>(&sh[0][k][4 * ty + 2]);
            const ulonglong2 m01 = *reinterpret_cast<const ulonglong2 *>(&sh[1][k][4 * ty]);
            const ulonglong2 m23 = *reinterpret_cast<const ulonglong2 *>(&sh[1][k][4 * ty + 2]);
            rc[0] = c01.x, rc[1] = c01.y, rc[2] = c23.x, rc[3] = c23.y;
            rm[0] = m01.x, rm[1] = m01.y, rm[2] = m23.x, rm[3] = m23.y;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                cc[b] = sh[2][k][tx + 16 * b];
                cm[b] = sh[3][k][tx + 16 * b];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    acc[a][b][0] += (uint32_t)__popcll(rc[a] & cc[b]);
                    acc[a][b][1] += (uint32_t)__popcll(rm[a] & cc[b]);
                    acc[a][b][2] += (uint32_t)__popcll(rc[a] & cm[b]);
                    acc[a][b][3] += (uint32_t)__popcll(rm[a] & cm[b]);
                }
        }
    }

    epi(acc, ti, tj, tx, ty, static_cast<void *>(&sh[0][0][0]));
}

// the triangle's epilogue (dst_site_ld, dst_site_ld_links): one uint4 per pair to tri_row_start(S, p) - out_base + (q - p - 1)
struct LdTriangleOut {
    uint32_t S, rb, re;
    uint64_t out_base;
    uint4 *__restrict__ slab;
    __device__ __forceinline__ void operator()(const uint32_t (&acc)[4][4][4], uint32_t ti, uint32_t tj, uint32_t tx, uint32_t ty, void *) const
    {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const uint32_t p = ti * kLdTile + 4 * ty + a;
            if (p < rb || p >= re)
                continue;   // (re <= S)
            const uint64_t row = tri_row_start(S, p) - out_base;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t q = tj * kLdTile + tx + 16 * b;
                if (q > p && q < S)
                    slab[row + (q - p - 1)] = make_uint4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
            }
        }
    }
};

__global__ __launch_bounds__(kLdThreads, 4) void ld_tile_kernel(const uint64_t *__restrict__ vec_c, const uint64_t *__restrict__ vec_m,
                                                             uint32_t S, uint32_t wpad, uint32_t tile_row0, uint32_t rb, uint32_t re,
                                                             uint64_t out_base, uint4 *__restrict__ slab)
{
    const uint32_t tj = blockIdx.x, ti = tile_row0 + blockIdx.y;
    if (tj < ti)
        return;   // (whole workgroups)
    ld_tile_body(vec_c, vec_m, wpad, ti, tj, LdTriangleOut{S, rb, re, out_base, slab});
}

// ---- the band: the tiles that hold a pair within max_gap, from a table ---------------------------------------------------
// workgroup x of a launch owns tile tiles[tile0 + x] = (tile row, tile column): only tiles with a band pair are listed
template <class Epilogue>
__global__ __launch_bounds__(kLdThreads, 4) void ld_band_tile_kernel(const uint64_t *__restrict__ vec_c, const uint64_t *__restrict__ vec_m,
                                                                  uint32_t wpad, const uint2 *__restrict__ tiles, uint64_t tile0,
                                                                  Epilogue epi)
{
    const uint2 t = tiles[tile0 + blockIdx.x];
    const uint32_t ti = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x), tj = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.y);
    ld_tile_body(vec_c, vec_m, wpad, ti, tj, epi);
}

// epilogue A (dst_site_ld_band, dst_site_ld_links_band): one uint4 per band pair to prefix[p] - out_base + (q - p - 1); row p's
// band pairs are p < q < p + 1 + (prefix[p + 1] - prefix[p]); the slab holds band pairs only
struct LdBandOut {
    const uint64_t *__restrict__ prefix;   // [S + 1] the running sum of the rows' band widths
    uint32_t rb, re;
    uint64_t out_base;
    uint4 *__restrict__ slab;
    __device__ __forceinline__ void operator()(const uint32_t (&acc)[4][4][4], uint32_t ti, uint32_t tj, uint32_t tx, uint32_t ty, void *) const
    {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const uint32_t p = ti * kLdTile + 4 * ty + a;
            if (p < rb || p >= re)
                continue;   // (re <= S)
            const uint64_t at = prefix[p], width = prefix[p + 1] - at, row = at - out_base;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t q = tj * kLdTile + tx + 16 * b;
                if (q > p && (uint64_t)(q - p - 1) < width)
                    slab[row + (q - p - 1)] = make_uint4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]);
            }
        }
    }
};

// dst_ld_finalize's r2 of one entry: the same conversions, products and quotient in the same order; false: r2 is NaN
__device__ __forceinline__ bool ld_r2(const uint4 &t, double &r2)
{
    const int64_t m = t.x, a = t.y, b = t.z, c = t.w;
    const int64_t num = m * c - a * b;
    const int64_t A = a * (m - a), B = b * (m - b);
    if (A == 0 || B == 0)
        return false;
    r2 = ((double)num * (double)num) / ((double)A * (double)B);
    return true;
}

// ... against the threshold
__device__ __forceinline__ bool ld_is_link(const uint4 &t, double min_r2)
{
    double r2;
    return ld_r2(t, r2) && r2 >= min_r2;
}

// ld_r2 behind a call, NaN for an r2 that is not defined: inlined 16 times beside the tile's 64 tallies, the 64-bit products and
// the f64 quotient take the kernel past its 128 registers and the K loop spills; as a function they have registers of their own
__device__ __attribute__((noinline)) double ld_r2_or_nan(uint4 t)
{
    double r2;
    return ld_r2(t, r2) ? r2 : __builtin_nan("");
}

// epilogue B (dst_site_ld_decay): no tally leaves the registers.  Per pair the gap's bin and r2 once; {defined, links, q} go to
// the bin's three 64-bit counters bins[3 bin ..].  A thread first merges its consecutive pairs of one bin.  The tile's bins lie
// in [lo, hi], from the gaps of its corner positions (wave-uniform): a span of at most DST_LD_DECAY_LOCAL_BINS is gathered in
// the staging block's LDS and its non-zero counters flushed once per workgroup; a wider tile adds to memory directly.  Every
// sum is an integer atomic: no order shows.
static_assert(DST_LD_DECAY_LOCAL_BINS * 24 <= kLdLdsBytes, "the local bins live in the staging block");
struct LdDecayOut {
    const uint32_t *__restrict__ sites;
    uint32_t S, bin_width, n_bins;   // (bin_width clamped to 2^32 - 1: no gap reaches it)
    double min_r2;
    unsigned long long *__restrict__ bins;
    __device__ __forceinline__ void operator()(const uint32_t (&acc)[4][4][4], uint32_t ti, uint32_t tj, uint32_t tx, uint32_t ty, void *lds) const
    {
        unsigned long long *local = static_cast<unsigned long long *>(lds);
        const uint32_t tid = 16 * ty + tx;   // (threadIdx.x, from what the K loop keeps anyway)
        const uint32_t last = S - 1, r0 = ti * kLdTile, c0 = tj * kLdTile;   // (a listed tile: r0, c0 <= last)
        const uint32_t r1 = min(r0 + kLdTile - 1, last), c1 = min(c0 + kLdTile - 1, last);
        const uint32_t lo_gap = tj > ti ? sites[c0] - sites[r1] : 1u, hi_gap = sites[c1] - sites[r0];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lo_gap / bin_width));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(hi_gap / bin_width, n_bins - 1));
        const bool in_lds = hi - lo < DST_LD_DECAY_LOCAL_BINS;   // (lo <= hi: the tile holds a band pair)
        if (in_lds) {
            __syncthreads();   // (the last step's words have been read)
            for (uint32_t e = tid; e < 3 * (hi - lo + 1); e += kLdThreads)
                local[e] = 0;
            __syncthreads();
        }
        uint32_t sp[4], sq[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
            sp[a] = sites[min(r0 + 4 * ty + a, last)];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            sq[b] = sites[min(c0 + tx + 16 * b, last)];
        uint32_t cur = 0;
        uint32_t defined = 0, links = 0;   // (16 pairs at most)
        unsigned long long sum = 0;
        auto flush = [&]() {
            if (!defined)
                return;
            auto add = [&](unsigned long long *to) {
                atomicAdd(to, (unsigned long long)defined);
                if (links)
                    atomicAdd(to + 1, (unsigned long long)links);
                if (sum)
                    atomicAdd(to + 2, sum);
            };
            if (in_lds)   // (two calls: an LDS add and a global add are different instructions)
                add(local + 3 * (size_t)(cur - lo));
            else
                add(bins + 3 * (size_t)cur);
        };
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const uint32_t p = r0 + 4 * ty + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t q = c0 + tx + 16 * b;
                if (q <= p || q > last)
                    continue;
                const uint32_t bin = (sq[b] - sp[a]) / bin_width;
                if (bin >= n_bins)
                    continue;
                const double r2 = ld_r2_or_nan(make_uint4(acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]));
                if (r2 != r2)
                    continue;
                if (bin != cur) {
                    flush();
                    cur = bin, defined = 0, links = 0, sum = 0;
                }
                ++defined;
                links += r2 >= min_r2 ? 1u : 0u;
                sum += (unsigned long long)rint(r2 * (double)(1ull << DST_LD_SCALE_BITS));
            }
        }
        flush();
        if (in_lds) {
            __syncthreads();
            for (uint32_t e = tid; e < 3 * (hi - lo + 1); e += kLdThreads)
                if (const unsigned long long v = local[e])
                    atomicAdd(bins + 3 * (size_t)lo + e, v);
        }
    }
};

// ---- the links: dst_links.hip's compaction, the entries uint4 tallies, the test r2 >= min_r2 ----------------------------
struct LdRows {
    uint64_t out_base;   // canonical index of the slab's first pair (the band: band index)
    uint32_t S;          // listed positions
    uint32_t rb, re;     // the slab's rows
    uint32_t chunks;     // workgroups per row: those of the slab's longest row
    const uint64_t *prefix;   // the band: [S + 1] the running sum of the rows' band widths (ragged rows)
};

// row i of the slab: its pairs and its first entry; Band: the row's band pairs
template <bool Band>
__device__ __forceinline__ void ld_row(const LdRows &g, uint32_t i, uint64_t &row_pairs, uint64_t &base)
{
    if (Band) {
        const uint64_t at = g.prefix[i];
        row_pairs = g.prefix[i + 1] - at, base = at - g.out_base;
    } else {
        row_pairs = (uint64_t)g.S - i - 1, base = tri_row_start(g.S, i) - g.out_base;
    }
}

__device__ __forceinline__ uint32_t ld_test_entries(const uint4 *__restrict__ slab, uint64_t row_pairs, uint64_t base, uint64_t q0, int lane,
                                                    double min_r2, uint4 (&v)[kLdSteps])
{
#pragma unroll
    for (int t = 0; t < kLdSteps; ++t) {
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane);
        v[t] = q < row_pairs ? slab[base + q] : make_uint4(0, 0, 0, 0);
    }
    uint32_t linked = 0;
#pragma unroll
    for (int t = 0; t < kLdSteps; ++t)
        if (ld_is_link(v[t], min_r2))   // (an entry past the row's end is zeros: never a link)
            linked |= 1u << t;
    return linked;
}

template <bool Band>
__global__ __launch_bounds__(256) void ld_count_kernel(const uint4 *__restrict__ slab, LdRows g, uint32_t row0, double min_r2,
                                                       uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wave_links[kLdWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t blk = (uint64_t)(i - g.rb) * g.chunks + blockIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * kLdBlockPairs;
    uint64_t row_pairs, base;
    ld_row<Band>(g, i, row_pairs, base);
    if (b0 >= row_pairs) {   // (whole workgroups) past the row's end: nothing, but the scan reads every count
        if (threadIdx.x == 0)
            counts[blk] = 0;
        return;
    }
    uint4 v[kLdSteps];
    const uint32_t linked = ld_test_entries(slab, row_pairs, base, b0 + (uint32_t)wave * kLdWavePairs, lane, min_r2, v);
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
        for (int w = 0; w < kLdWaves; ++w)
            total += wave_links[w];
        counts[blk] = total;
    }
}

template <bool Band>
__global__ __launch_bounds__(256) void ld_write_kernel(const uint4 *__restrict__ slab, LdRows g, uint32_t row0, double min_r2,
                                                       const uint64_t *__restrict__ offsets, uint64_t lo, uint64_t hi,
                                                       uint32_t *__restrict__ pos_i, uint32_t *__restrict__ pos_j,
                                                       uint4 *__restrict__ tal)
{
    __shared__ uint32_t wave_links[kLdWaves];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const uint32_t i = row0 + blockIdx.y;
    if (i >= g.re)
        return;   // (whole workgroups)
    const uint64_t blk = (uint64_t)(i - g.rb) * g.chunks + blockIdx.x;
    const uint64_t first = offsets[blk], next = offsets[blk + 1];
    if (next == first || next <= lo || first >= hi)
        return;   // (whole workgroups) no link of this block inside the window
    const uint64_t q0 = (uint64_t)blockIdx.x * kLdBlockPairs + (uint32_t)wave * kLdWavePairs;
    uint64_t row_pairs, base;
    ld_row<Band>(g, i, row_pairs, base);
    uint4 v[kLdSteps];
    const uint32_t linked = ld_test_entries(slab, row_pairs, base, q0, lane, min_r2, v);
    // ranks inside the wave: the steps in order, inside a step the lanes in order
    const uint64_t below = (1ull << lane) - 1;
    uint32_t rank[kLdSteps], wave_total = 0;
#pragma unroll
    for (int t = 0; t < kLdSteps; ++t) {
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
#pragma unroll
    for (int t = 0; t < kLdSteps; ++t) {
        if (!((linked >> t) & 1u))
            continue;
        const uint64_t r = at0 + rank[t];
        if (r < lo || r >= hi)
            continue;
        const uint64_t q = q0 + (uint32_t)(t * 64 + lane), e = r - lo;
        pos_i[e] = i;
        pos_j[e] = i + 1 + (uint32_t)q;
        tal[e] = v[t];
    }
}

const char *const kSharedRefusal = "a set uploaded with dst_upload_shared runs on the consensus path only (this rank holds "
                                   "the planes of its own records)";

size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the rows [rb, re) of the triangle of S positions in order, in slabs of at most max_pairs pairs (at least one row each);
// slabs without pairs are left out
std::vector<RowSlab> ld_slabs(uint64_t S, uint64_t rb, uint64_t re, uint64_t max_pairs)
{
    std::vector<RowSlab> slabs;
    for (uint64_t r = rb; r < re;) {
        uint64_t e = r, pairs = 0;
        do {
            pairs += S - e - 1;
            ++e;
        } while (e < re && pairs + (S - e - 1) <= max_pairs);
        if (pairs)
            slabs.push_back(RowSlab{r, e, square_row_start(S, r), pairs});
        r = e;
    }
    return slabs;
}

uint64_t ld_blocks(uint64_t S, uint64_t rb, uint64_t re)
{
    return re <= rb ? 0 : (re - rb) * ((S - rb - 1 + kLdBlockPairs - 1) / kLdBlockPairs);
}

// ---- the band on the host -------------------------------------------------------------------------------------------
// row_end[p]: the first position past p whose gap to p is above max_gap (p + 1 at least); the list is strictly ascending
void ld_band_rows(const uint32_t *sites, uint32_t S, uint64_t max_gap, uint32_t *row_end)
{
    uint32_t e = 0;
    for (uint32_t p = 0; p < S; ++p) {
        e = std::max(e, p + 1);
        while (e < S && (uint64_t)(sites[e] - sites[p]) <= max_gap)
            ++e;
        row_end[p] = e;
    }
}

// the tile columns [begin, end) of tile row ti that hold a band pair.  The diagonal tile holds one when a row before the tile
// row's last has a band pair (its first, (p, p + 1), lies inside the tile); the last row's pairs all lie in later tile columns.
// row_end being non-decreasing, every tile column from there to the one of the last row's last band pair holds one.
void ld_band_tile_range(const uint32_t *row_end, uint32_t S, uint32_t ti, uint32_t &begin, uint32_t &end)
{
    const uint32_t p0 = ti * kLdTile, p1 = std::min(p0 + kLdTile, S);
    begin = ti + 1;
    for (uint32_t p = p0; p + 1 < p1; ++p)
        if (row_end[p] > p + 1) {
            begin = ti;
            break;
        }
    end = std::max(begin, (row_end[p1 - 1] - 1) / kLdTile + 1);
}

// a call's band: the rows, their running sum (the ragged slab's row bases) and the table of tiles, tile row by tile row
struct LdBand {
    std::vector<uint32_t> row_end;      // [S]
    std::vector<uint64_t> prefix;       // [S + 1]
    std::vector<uint2> tiles;           // (tile row, tile column)
    std::vector<uint64_t> tile_first;   // [tile rows + 1] into tiles
    uint64_t pairs = 0;
    uint32_t bins = 0;                  // the decay call's counters (3 x 8 bytes each)

    void rows(const uint32_t *sites, uint32_t S, uint64_t max_gap)
    {
        row_end.resize(S);
        prefix.assign((size_t)S + 1, 0);
        ld_band_rows(sites, S, max_gap, row_end.data());
        for (uint32_t p = 0; p < S; ++p)
            prefix[p + 1] = prefix[p] + (row_end[p] - p - 1);
        pairs = prefix[S];
    }
    void list_tiles(uint32_t S)
    {
        const uint32_t tile_rows = (S + kLdTile - 1) / kLdTile;
        tile_first.assign((size_t)tile_rows + 1, 0);
        for (uint32_t ti = 0; ti < tile_rows; ++ti) {
            uint32_t begin, end;
            ld_band_tile_range(row_end.data(), S, ti, begin, end);
            for (uint32_t tj = begin; tj < end; ++tj)
                tiles.push_back(make_uint2(ti, tj));
            tile_first[ti + 1] = tiles.size();
        }
    }
};

// dst_site_ld_decay's `pairs`: bins[gap / width].pairs over the band pairs, without a division per pair and without a walk
// over a long row's pairs.  A row shorter than the bins it spans is walked pair by pair behind a running bin edge; a longer
// one reads its bins off the edges' positions: edge[b] = the first position whose site is >= sites[p] + b x width, which
// only moves forward from row to row (each edge advances n_sites times at most over the whole call).
void ld_decay_pairs(const uint32_t *sites, uint32_t S, const uint32_t *row_end, uint64_t width, uint32_t n_bins, dst_ld_bin *bins)
{
    std::vector<uint32_t> edge((size_t)n_bins + 1, 0);
    for (uint32_t p = 0; p < S; ++p) {
        const uint32_t end = row_end[p], len = end - p - 1;
        if (!len)
            continue;
        const uint64_t at = sites[p], spanned = (sites[end - 1] - at) / width + 1;   // (<= n_bins)
        if (len <= spanned) {
            uint64_t bin = 0, next = at + width;   // the first site of bin + 1
            for (uint32_t q = p + 1; q < end; ++q) {
                if (sites[q] >= next) {
                    if (sites[q] < next + width)
                        ++bin, next += width;
                    else
                        bin = (sites[q] - at) / width, next = at + (bin + 1) * width;
                }
                ++bins[bin].pairs;
            }
            continue;
        }
        for (uint64_t b = 0; b <= spanned; ++b) {
            uint32_t e = std::max(edge[b], p + 1);
            const uint64_t first = at + b * width;
            while (e < end && sites[e] < first)
                ++e;
            edge[b] = e;
        }
        for (uint64_t b = 0; b < spanned; ++b)
            bins[b].pairs += std::min(edge[b + 1], end) - std::min(edge[b], end);
    }
}

// the rows [rb, re) in order, in slabs of at most max_pairs BAND pairs (at least one row each); slabs without pairs are left
// out; first: the band index of the slab's first pair
std::vector<RowSlab> ld_band_slabs(const LdBand &band, uint64_t rb, uint64_t re, uint64_t max_pairs)
{
    std::vector<RowSlab> slabs;
    for (uint64_t r = rb; r < re;) {
        uint64_t e = r + 1;
        while (e < re && band.prefix[e + 1] - band.prefix[r] <= max_pairs)
            ++e;
        if (band.prefix[e] > band.prefix[r])
            slabs.push_back(RowSlab{r, e, band.prefix[r], band.prefix[e] - band.prefix[r]});
        r = e;
    }
    return slabs;
}

// the count / write workgroups of a band slab: per row those of its longest band row
uint64_t ld_band_blocks(const LdBand &band, uint64_t rb, uint64_t re)
{
    uint64_t longest = 1;
    for (uint64_t p = rb; p < re; ++p)
        longest = std::max<uint64_t>(longest, band.row_end[p] - p - 1);
    return (re - rb) * ((longest + kLdBlockPairs - 1) / kLdBlockPairs);
}

// what both calls share: the checks of the list (after the caller's own of its pointers), the vectors on the device
struct LdCall {
    DeviceSet *set = nullptr;
    uint32_t S = 0, s_pad = 0, wpad = 0;
    uint64_t taking_part = 0;
    std::vector<LdChunk> chunks;
};

int ld_check(dst_ctx *ctx, const char *what, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
             const uint32_t *group, uint32_t which, LdCall &call)
{
    if (!sites)
        return fail(ctx, DST_ERR_ARG, "null sites pointer");
    if (!allele)
        return fail(ctx, DST_ERR_ARG, "null allele pointer");
    if (slot < 0 || slot > 1)
        return fail(ctx, DST_ERR_ARG, "slot must be 0 or 1");
    if (!group && which != 0)
        return fail(ctx, DST_ERR_ARG, std::string(what) + ": without labels every record takes part (which must be 0)");
    DeviceSet &s = ctx->set[slot];
    if (!s.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    if (s.partial)
        return fail(ctx, DST_ERR_STATE, kSharedRefusal);
    for (uint32_t p = 0; p < n_sites; ++p) {
        if (sites[p] >= s.len)
            return fail(ctx, DST_ERR_ARG, std::string(what) + ": position " + std::to_string(p) + " names site " + std::to_string(sites[p]) +
                                              ", which is not a site of an alignment of " + std::to_string(s.len) + " sites");
        if (p && sites[p] <= sites[p - 1])
            return fail(ctx, DST_ERR_ARG, std::string(what) + ": position " + std::to_string(p) + " names site " + std::to_string(sites[p]) +
                                              " after site " + std::to_string(sites[p - 1]) + ": the list must be strictly ascending");
    }
    for (uint32_t p = 0; p < n_sites; ++p)
        if (allele[p] > 3)
            return fail(ctx, DST_ERR_ARG, std::string(what) + ": position " + std::to_string(p) + " has allele " + std::to_string(allele[p]) +
                                              ", which is not one of 0 (A), 1 (T), 2 (G), 3 (C)");
    call.set = &s;
    call.S = n_sites;
    return DST_OK;
}

int ld_records(dst_ctx *ctx, const char *what, const uint32_t *group, uint32_t which, LdCall &call)
{
    const uint64_t n = call.set->n;
    if (n >= ((uint64_t)1 << 31))
        return fail(ctx, DST_ERR_ARG, std::string(what) + ": sets of 2^31 records or more");
    call.taking_part = n;
    if (group) {
        call.taking_part = 0;
        for (uint64_t x = 0; x < n; ++x)
            call.taking_part += group[x] == which;
    }
    return DST_OK;
}

// the device side of a call: the vectors (and the tables that make them), one slab, and for the links the counts, offsets
// and one window of outputs
struct LdBuffers {
    uint64_t *vec_c, *vec_m;
    LdChunk *chunks;
    uint32_t *sites, *group;
    uint64_t *band_prefix;   // the band calls: [S + 1]
    uint2 *band_tiles;       // ... and the table of tiles
    uint4 *slab;
    uint32_t *counts;
    uint64_t *offsets, *grand;
    uint32_t *pos_i, *pos_j;
    uint4 *tal;
    unsigned long long *bins;   // the decay call: [bins][3]
};

size_t ld_layout(void *base_v, const LdCall &call, bool labels, uint64_t slab_pairs, uint64_t blocks, uint64_t chunk, const LdBand *band,
                 LdBuffers &b)
{
    char *base = static_cast<char *>(base_v);
    size_t used = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + used : nullptr;
        used += pad256(bytes);
        return p;
    };
    const size_t vec_words = (size_t)call.s_pad * call.wpad;
    b.vec_c = reinterpret_cast<uint64_t *>(take(vec_words * 8));
    b.vec_m = reinterpret_cast<uint64_t *>(take(vec_words * 8));
    // (the tables are one piece of the staging block, in this order: one copy brings them)
    b.chunks = reinterpret_cast<LdChunk *>(take(call.chunks.size() * sizeof(LdChunk)));
    b.sites = reinterpret_cast<uint32_t *>(take((size_t)call.S * 4));
    b.group = reinterpret_cast<uint32_t *>(take(labels ? call.set->n * 4 : 0));
    b.band_prefix = reinterpret_cast<uint64_t *>(take(band ? band->prefix.size() * 8 : 0));
    b.band_tiles = reinterpret_cast<uint2 *>(take(band ? band->tiles.size() * sizeof(uint2) : 0));
    b.slab = reinterpret_cast<uint4 *>(take(slab_pairs * 16));
    b.counts = reinterpret_cast<uint32_t *>(take(blocks * 4));
    b.offsets = reinterpret_cast<uint64_t *>(take(blocks ? (blocks + 1) * 8 : 0));
    b.grand = reinterpret_cast<uint64_t *>(take(blocks ? 8 : 0));
    b.pos_i = reinterpret_cast<uint32_t *>(take(chunk * 4));
    b.pos_j = reinterpret_cast<uint32_t *>(take(chunk * 4));
    b.tal = reinterpret_cast<uint4 *>(take(chunk * 16));
    b.bins = reinterpret_cast<unsigned long long *>(take(band ? (size_t)band->bins * 24 : 0));
    return used;
}

// grow the buffers, build and upload the tables, and queue the vectors; host_extra: page-locked bytes the caller wants
// behind the tables' staging (the links' window)
int ld_prepare(dst_ctx *ctx, const char *what, const uint32_t *sites, const uint8_t *allele, const uint32_t *group, uint32_t which,
               LdCall &call, uint64_t slab_pairs, uint64_t blocks, uint64_t chunk, size_t host_extra, LdBuffers &b, size_t &stage_bytes,
               const LdBand *band = nullptr)
{
    DeviceSet &s = *call.set;
    const uint32_t S = call.S;
    call.s_pad = (S + kLdTile - 1) / kLdTile * kLdTile;
    const uint32_t words = (uint32_t)((s.n + 63) / 64);
    call.wpad = (words + kLdKStep - 1) / kLdKStep * kLdKStep;
    // the listed chunks and their reference words
    for (uint32_t p = 0; p < S; ++p) {
        const uint32_t c = sites[p] / kChunkSites, bit = sites[p] % kChunkSites;
        if (call.chunks.empty() || call.chunks.back().chunk != c) {
            LdChunk ch{};
            ch.chunk = c, ch.first = p;
            call.chunks.push_back(ch);
        }
        LdChunk &ch = call.chunks.back();
        ++ch.count;
        ch.ref[allele[p]][bit / 32] |= 1u << (bit % 32);
    }
    const size_t chunk_bytes = pad256(call.chunks.size() * sizeof(LdChunk)), site_bytes = pad256((size_t)S * 4);
    const size_t label_bytes = pad256(group ? s.n * 4 : 0);
    const size_t prefix_bytes = pad256(band ? band->prefix.size() * 8 : 0), tile_bytes = pad256(band ? band->tiles.size() * sizeof(uint2) : 0);
    stage_bytes = chunk_bytes + site_bytes + label_bytes + prefix_bytes + tile_bytes;
    const size_t work_bytes = ld_layout(nullptr, call, group != nullptr, slab_pairs, blocks, chunk, band, b);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipStreamSynchronize(stream));   // (the work and staging buffers' earlier readers)
    if (int rc = order_after_prep(ctx, stream))
        return rc;
    if (int rc = ensure_planes(ctx, s, stream))
        return rc;
    if (ctx->ld_work.grow(ctx, work_bytes)) {
        (void)hipGetLastError();
        return fail(ctx, DST_ERR_NOMEM, std::string(what) + ": cannot allocate " + std::to_string(work_bytes) + " bytes of device memory");
    }
    if (int rc = ctx->ld_host.grow(ctx, stage_bytes + host_extra, what))
        return rc;
    ld_layout(ctx->ld_work, call, group != nullptr, slab_pairs, blocks, chunk, band, b);
    char *stage = ctx->ld_host;
    std::memcpy(stage, call.chunks.data(), call.chunks.size() * sizeof(LdChunk));
    std::memcpy(stage + chunk_bytes, sites, (size_t)S * 4);
    if (group)
        std::memcpy(stage + chunk_bytes + site_bytes, group, s.n * 4);
    if (band) {
        std::memcpy(stage + chunk_bytes + site_bytes + label_bytes, band->prefix.data(), band->prefix.size() * 8);
        std::memcpy(stage + chunk_bytes + site_bytes + label_bytes + prefix_bytes, band->tiles.data(), band->tiles.size() * sizeof(uint2));
    }
    HIP_TRY(ctx, hipMemcpyAsync(b.chunks, stage, stage_bytes, hipMemcpyHostToDevice, stream));
    // the rows of the positions past the list, up to whole tiles: zeros, written by this call
    if (call.s_pad > S) {
        const size_t tail = (size_t)(call.s_pad - S) * call.wpad * 8;
        HIP_TRY(ctx, hipMemsetAsync(b.vec_c + (size_t)S * call.wpad, 0, tail, stream));
        HIP_TRY(ctx, hipMemsetAsync(b.vec_m + (size_t)S * call.wpad, 0, tail, stream));
    }
    HIP_TRY(ctx, for_row_grids(0, call.chunks.size(), [&](uint64_t chunk0, unsigned nc) {
                hipLaunchKernelGGL(ld_vectors_kernel, dim3(call.wpad / kLdKStep, nc), dim3(kLdThreads), 0, stream, s.planes,
                                   (uint32_t)s.nchunks, (uint32_t)s.npad, (uint32_t)s.n, b.chunks, (uint32_t)chunk0, b.sites,
                                   group ? b.group : nullptr, which, call.wpad, b.vec_c, b.vec_m);
                return hipGetLastError();
            }));
    return DST_OK;
}

// the tallies of the slab's rows into b.slab
hipError_t ld_launch_tiles(const LdCall &call, const RowSlab &sl, const LdBuffers &b, hipStream_t stream)
{
    const uint32_t t0 = (uint32_t)(sl.rb / kLdTile), t1 = (uint32_t)((sl.re - 1) / kLdTile) + 1, tiles = call.s_pad / kLdTile;
    return for_row_grids(t0, t1, [&](uint64_t row0, unsigned rows) {
        hipLaunchKernelGGL(ld_tile_kernel, dim3(tiles, rows), dim3(kLdThreads), 0, stream, b.vec_c, b.vec_m, call.S, call.wpad,
                           (uint32_t)row0, (uint32_t)sl.rb, (uint32_t)sl.re, sl.first, b.slab);
        return hipGetLastError();
    });
}

// the band tiles of the tile rows [t0, t1) under one epilogue
constexpr uint64_t kLdGridTiles = (uint64_t)1 << 30;
template <class Epilogue>
hipError_t ld_launch_band_tiles(const LdCall &call, const LdBand &band, uint32_t t0, uint32_t t1, const LdBuffers &b, const Epilogue &epi,
                                hipStream_t stream)
{
    const uint64_t first = band.tile_first[t0], end = band.tile_first[t1];
    for (uint64_t at = first; at < end; at += kLdGridTiles) {
        hipLaunchKernelGGL(ld_band_tile_kernel<Epilogue>, dim3((unsigned)std::min(kLdGridTiles, end - at)), dim3(kLdThreads), 0, stream,
                           b.vec_c, b.vec_m, call.wpad, b.band_tiles, at, epi);
        if (const hipError_t e = hipGetLastError())
            return e;
    }
    return hipSuccess;
}

// the tallies of the slab's rows into b.slab; band: its band pairs only
hipError_t ld_launch_slab(const LdCall &call, const LdBand *band, const RowSlab &sl, const LdBuffers &b, hipStream_t stream)
{
    if (!band)
        return ld_launch_tiles(call, sl, b, stream);
    return ld_launch_band_tiles(call, *band, (uint32_t)(sl.rb / kLdTile), (uint32_t)((sl.re - 1) / kLdTile) + 1, b,
                                LdBandOut{b.band_prefix, (uint32_t)sl.rb, (uint32_t)sl.re, sl.first, b.slab}, stream);
}

// dst_site_ld_links and, with max_gap, dst_site_ld_links_band: the slabs are the triangle's rows or the band's ragged rows
int ld_links_call(dst_ctx *ctx, const char *what, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                  const uint32_t *group, uint32_t which, double min_r2, const uint64_t *max_gap, uint64_t max_pairs, dst_ld_sink sink,
                  void *user, uint64_t *n_links)
{
    LdCall call;
    if (int rc = ld_check(ctx, what, slot, sites, allele, n_sites, group, which, call))
        return rc;
    if (int rc = ld_records(ctx, what, group, which, call))
        return rc;
    if (std::isnan(min_r2))
        return fail(ctx, DST_ERR_ARG, std::string(what) + ": min_r2 is NaN");
    const uint64_t S = n_sites;
    if (S < 2 || call.taking_part == 0)
        return DST_OK;   // (no launch: no pair, or every r2 is NaN)
    LdBand plan;
    const LdBand *band = nullptr;
    if (max_gap) {
        plan.rows(sites, n_sites, *max_gap);
        if (plan.pairs == 0)
            return DST_OK;   // (no launch: no pair within the gap)
        plan.list_tiles(n_sites);
        band = &plan;
    }
    const uint64_t slab_pairs = max_pairs ? max_pairs : kLdSlabPairs;
    const std::vector<RowSlab> slabs = band ? ld_band_slabs(*band, 0, S, slab_pairs) : ld_slabs(S, 0, S, slab_pairs);
    auto blocks_of = [&](const RowSlab &sl) { return band ? ld_band_blocks(*band, sl.rb, sl.re) : ld_blocks(S, sl.rb, sl.re); };
    uint64_t biggest = 0, blocks = 0;
    for (const RowSlab &sl : slabs) {
        biggest = std::max(biggest, sl.pairs);
        blocks = std::max(blocks, blocks_of(sl));
    }
    // one window of outputs: never more links than the largest slab has pairs
    const uint64_t chunk = sink ? std::min<uint64_t>(DST_LD_CHUNK, biggest) : 0;
    LdBuffers b{};
    size_t stage_bytes = 0;
    if (int rc = ld_prepare(ctx, what, sites, allele, group, which, call, biggest, blocks, chunk, (size_t)chunk * 24, b, stage_bytes, band))
        return rc;
    hipStream_t stream = ctx->stream;
    char *host = static_cast<char *>(ctx->ld_host) + stage_bytes;   // pos_i, pos_j, tallies of one window
    const size_t h_j = (size_t)chunk * 4, h_tal = (size_t)chunk * 8;
    HIP_TRY(ctx, hipMemsetAsync(b.grand, 0, 8, stream));
    uint64_t total = 0;
    int rc = DST_OK;
    // per slab: the tallies, the block counts and their scan; with a sink the slab's total comes back (one wait), then every
    // window of at most `chunk` ranks is written, copied (one wait) and handed over
    for (const RowSlab &sl : slabs) {
        rc = [&]() -> int {
            HIP_TRY(ctx, ld_launch_slab(call, band, sl, b, stream));
            const uint64_t n_blocks = blocks_of(sl);
            LdRows g{sl.first, (uint32_t)S, (uint32_t)sl.rb, (uint32_t)sl.re, (uint32_t)(n_blocks / (sl.re - sl.rb)), b.band_prefix};
            HIP_TRY(ctx, for_row_grids(sl.rb, sl.re, [&](uint64_t row0, unsigned rows) {
                        hipLaunchKernelGGL(band ? ld_count_kernel<true> : ld_count_kernel<false>, dim3(g.chunks, rows), dim3(256), 0, stream, b.slab, g, (uint32_t)row0, min_r2,
                                           b.counts);
                        return hipGetLastError();
                    }));
            HIP_TRY(ctx, launch_links_scan(b.counts, n_blocks, b.offsets, b.grand, stream));
            if (!sink)
                return DST_OK;
            uint64_t in_slab = 0;
            HIP_TRY(ctx, hipMemcpyAsync(&in_slab, b.offsets + n_blocks, 8, hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipStreamSynchronize(stream));
            if (in_slab > sl.pairs)
                return fail(ctx, DST_ERR_STATE, std::string(what) + ": more links than pairs in a slab");
            for (uint64_t lo = 0; lo < in_slab; lo += chunk) {
                const uint64_t hi = std::min(in_slab, lo + chunk), m = hi - lo;
                HIP_TRY(ctx, for_row_grids(sl.rb, sl.re, [&](uint64_t row0, unsigned rows) {
                            hipLaunchKernelGGL(band ? ld_write_kernel<true> : ld_write_kernel<false>, dim3(g.chunks, rows), dim3(256), 0, stream, b.slab, g, (uint32_t)row0,
                                               min_r2, b.offsets, lo, hi, b.pos_i, b.pos_j, b.tal);
                            return hipGetLastError();
                        }));
                HIP_TRY(ctx, hipMemcpyAsync(host, b.pos_i, m * 4, hipMemcpyDeviceToHost, stream));
                HIP_TRY(ctx, hipMemcpyAsync(host + h_j, b.pos_j, m * 4, hipMemcpyDeviceToHost, stream));
                HIP_TRY(ctx, hipMemcpyAsync(host + h_tal, b.tal, m * 16, hipMemcpyDeviceToHost, stream));
                HIP_TRY(ctx, hipStreamSynchronize(stream));
                if (sink(user, total, m, reinterpret_cast<const uint32_t *>(host), reinterpret_cast<const uint32_t *>(host + h_j),
                         reinterpret_cast<const uint32_t *>(host + h_tal)))
                    return fail(ctx, DST_ERR_STATE, "stopped by sink");
                total += m;
                if (n_links)
                    *n_links = total;
            }
            return DST_OK;
        }();
        if (rc)
            break;
    }
    if (rc) {
        (void)hipStreamSynchronize(stream);   // (a stop between two slabs leaves nothing queued on the buffers)
        return rc;
    }
    if (!sink) {
        HIP_TRY(ctx, hipMemcpyAsync(&total, b.grand, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    }
    if (n_links)
        *n_links = total;
    return DST_OK;
}

}  // namespace
}  // namespace dst

extern "C" int dst_site_ld(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites, const uint32_t *group,
                           uint32_t which, uint32_t row_begin, uint32_t row_end, uint32_t *tallies, size_t cap_pairs)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (!tallies)
        return fail(ctx, DST_ERR_ARG, "null tallies pointer");
    LdCall call;
    if (int rc = ld_check(ctx, "site ld", slot, sites, allele, n_sites, group, which, call))
        return rc;
    if (row_begin > row_end || row_end > n_sites)
        return fail(ctx, DST_ERR_ARG, "site ld: [" + std::to_string(row_begin) + ", " + std::to_string(row_end) +
                                          ") is not a range of positions of a list of " + std::to_string(n_sites) + " sites");
    if (int rc = ld_records(ctx, "site ld", group, which, call))
        return rc;
    const uint64_t S = n_sites;
    const uint64_t pairs = S < 2 ? 0 : square_row_start(S, std::min<uint64_t>(row_end, S - 1)) - square_row_start(S, std::min<uint64_t>(row_begin, S - 1));
    if (pairs > (uint64_t)cap_pairs)
        return fail(ctx, DST_ERR_CAPACITY, "tallies buffer too small: 4 entries for every pair of the row range");
    if (pairs == 0)
        return DST_OK;   // (no launch)
    if (call.taking_part == 0) {
        std::memset(tallies, 0, (size_t)pairs * 16);
        return DST_OK;   // (no launch)
    }
    const std::vector<RowSlab> slabs = ld_slabs(S, row_begin, row_end, kLdSlabPairs);
    uint64_t biggest = 0;
    for (const RowSlab &sl : slabs)
        biggest = std::max(biggest, sl.pairs);
    LdBuffers b{};
    size_t stage_bytes = 0;
    if (int rc = ld_prepare(ctx, "site ld", sites, allele, group, which, call, biggest, 0, 0, 0, b, stage_bytes))
        return rc;
    hipStream_t stream = ctx->stream;
    const uint64_t first = slabs.front().first;
    for (const RowSlab &sl : slabs) {
        HIP_TRY(ctx, ld_launch_tiles(call, sl, b, stream));
        HIP_TRY(ctx, hipMemcpyAsync(tallies + (sl.first - first) * 4, b.slab, (size_t)sl.pairs * 16, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

extern "C" int dst_site_ld_links(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                                 const uint32_t *group, uint32_t which, double min_r2, uint64_t max_pairs, dst_ld_sink sink, void *user,
                                 uint64_t *n_links)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_links)
        *n_links = 0;
    return dst::ld_links_call(ctx, "site ld links", slot, sites, allele, n_sites, group, which, min_r2, nullptr, max_pairs, sink, user, n_links);
}

extern "C" int dst_site_ld_links_band(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                                      const uint32_t *group, uint32_t which, double min_r2, uint64_t max_gap, uint64_t max_pairs,
                                      dst_ld_sink sink, void *user, uint64_t *n_links)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_links)
        *n_links = 0;
    return dst::ld_links_call(ctx, "site ld links band", slot, sites, allele, n_sites, group, which, min_r2, &max_gap, max_pairs, sink, user,
                              n_links);
}

extern "C" int dst_ld_band(const uint32_t *sites, uint32_t n_sites, uint64_t max_gap, uint32_t *row_end, uint64_t *pairs, uint64_t *tiles)
{
    if (!sites && n_sites)
        return DST_ERR_ARG;
    for (uint32_t p = 1; p < n_sites; ++p)
        if (sites[p] <= sites[p - 1])
            return DST_ERR_ARG;
    std::vector<uint32_t> own;
    if (!row_end && n_sites) {
        own.resize(n_sites);
        row_end = own.data();
    }
    dst::ld_band_rows(sites, n_sites, max_gap, row_end);
    uint64_t n_pairs = 0, n_tiles = 0;
    for (uint32_t p = 0; p < n_sites; ++p)
        n_pairs += row_end[p] - p - 1;
    for (uint32_t ti = 0; ti < (n_sites + dst::kLdTile - 1) / dst::kLdTile; ++ti) {
        uint32_t begin, end;
        dst::ld_band_tile_range(row_end, n_sites, ti, begin, end);
        n_tiles += end - begin;
    }
    if (pairs)
        *pairs = n_pairs;
    if (tiles)
        *tiles = n_tiles;
    return DST_OK;
}

extern "C" int dst_site_ld_band(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites, const uint32_t *group,
                                uint32_t which, uint64_t max_gap, uint32_t row_begin, uint32_t row_end, uint32_t *tallies, size_t cap_pairs)
{
    using namespace dst;
    if (!ctx)
        return DST_ERR_ARG;
    if (!tallies)
        return fail(ctx, DST_ERR_ARG, "null tallies pointer");
    LdCall call;
    if (int rc = ld_check(ctx, "site ld band", slot, sites, allele, n_sites, group, which, call))
        return rc;
    if (row_begin > row_end || row_end > n_sites)
        return fail(ctx, DST_ERR_ARG, "site ld band: [" + std::to_string(row_begin) + ", " + std::to_string(row_end) +
                                          ") is not a range of positions of a list of " + std::to_string(n_sites) + " sites");
    if (int rc = ld_records(ctx, "site ld band", group, which, call))
        return rc;
    LdBand band;
    band.rows(sites, n_sites, max_gap);
    const uint64_t pairs = band.prefix[row_end] - band.prefix[row_begin];
    if (pairs > (uint64_t)cap_pairs)
        return fail(ctx, DST_ERR_CAPACITY, "tallies buffer too small: 4 entries for every band pair of the row range");
    if (pairs == 0)
        return DST_OK;   // (no launch)
    if (call.taking_part == 0) {
        std::memset(tallies, 0, (size_t)pairs * 16);
        return DST_OK;   // (no launch)
    }
    band.list_tiles(n_sites);
    const std::vector<RowSlab> slabs = ld_band_slabs(band, row_begin, row_end, kLdSlabPairs);
    uint64_t biggest = 0;
    for (const RowSlab &sl : slabs)
        biggest = std::max(biggest, sl.pairs);
    LdBuffers b{};
    size_t stage_bytes = 0;
    if (int rc = ld_prepare(ctx, "site ld band", sites, allele, group, which, call, biggest, 0, 0, 0, b, stage_bytes, &band))
        return rc;
    hipStream_t stream = ctx->stream;
    const uint64_t first = band.prefix[row_begin];
    for (const RowSlab &sl : slabs) {
        HIP_TRY(ctx, ld_launch_slab(call, &band, sl, b, stream));
        HIP_TRY(ctx, hipMemcpyAsync(tallies + (sl.first - first) * 4, b.slab, (size_t)sl.pairs * 16, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

extern "C" int dst_site_ld_decay(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites, const uint32_t *group,
                                 uint32_t which, double min_r2, uint64_t bin_width, uint32_t n_bins, uint64_t max_pairs, dst_ld_bin *bins,
                                 size_t cap)
{
    using namespace dst;
    if (!ctx)
        return DST_ERR_ARG;
    if (!bins)
        return fail(ctx, DST_ERR_ARG, "null bins pointer");
    LdCall call;
    if (int rc = ld_check(ctx, "site ld decay", slot, sites, allele, n_sites, group, which, call))
        return rc;
    if (int rc = ld_records(ctx, "site ld decay", group, which, call))
        return rc;
    if (std::isnan(min_r2))
        return fail(ctx, DST_ERR_ARG, "site ld decay: min_r2 is NaN");
    if (bin_width == 0)
        return fail(ctx, DST_ERR_ARG, "site ld decay: bin_width must be at least 1");
    if (n_bins == 0 || n_bins > DST_LD_DECAY_MAX_BINS)
        return fail(ctx, DST_ERR_ARG, "site ld decay: n_bins must be 1.." + std::to_string(DST_LD_DECAY_MAX_BINS) + ", not " + std::to_string(n_bins));
    // the band of the bins: gaps up to n_bins x bin_width - 1 (no gap reaches 2^32 - 1: a wider bin holds every pair)
    const uint64_t width = std::min<uint64_t>(bin_width, 0xFFFFFFFFull), max_gap = (uint64_t)n_bins * width - 1;
    LdBand band;
    band.rows(sites, n_sites, max_gap);
    if (band.pairs > ((uint64_t)1 << 33))
        return fail(ctx, DST_ERR_ARG, "site ld decay: the bins hold " + std::to_string(band.pairs) + " pairs, more than 2^33 (a bin's sum could overflow)");
    if ((uint64_t)cap < n_bins)
        return fail(ctx, DST_ERR_CAPACITY, "bins buffer too small: one entry for every bin");
    std::memset(bins, 0, (size_t)n_bins * sizeof(dst_ld_bin));
    // the bins' pairs, from the list alone (host work: with a launch it runs while the device counts)
    auto fill_pairs = [&]() { ld_decay_pairs(sites, n_sites, band.row_end.data(), width, n_bins, bins); };
    if (band.pairs == 0 || call.taking_part == 0) {
        fill_pairs();
        return DST_OK;   // (no launch: no pair, or every r2 is NaN)
    }
    band.list_tiles(n_sites);
    band.bins = n_bins;
    LdBuffers b{};
    size_t stage_bytes = 0;
    if (int rc = ld_prepare(ctx, "site ld decay", sites, allele, group, which, call, 0, 0, 0, (size_t)n_bins * 24, b, stage_bytes, &band))
        return rc;
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(b.bins, 0, (size_t)n_bins * 24, stream));
    const LdDecayOut epi{b.sites, n_sites, (uint32_t)width, n_bins, min_r2, b.bins};
    // launches of whole tile rows, at most max_pairs band pairs each (at least one tile row)
    const uint64_t launch_pairs = max_pairs ? max_pairs : kLdSlabPairs;
    const uint32_t tile_rows = (uint32_t)band.tile_first.size() - 1;
    auto row_of = [&](uint32_t t) { return std::min<uint64_t>((uint64_t)t * kLdTile, n_sites); };
    for (uint32_t t0 = 0; t0 < tile_rows;) {
        uint32_t t1 = t0 + 1;
        while (t1 < tile_rows && band.prefix[row_of(t1 + 1)] - band.prefix[row_of(t0)] <= launch_pairs)
            ++t1;
        HIP_TRY(ctx, ld_launch_band_tiles(call, band, t0, t1, b, epi, stream));
        t0 = t1;
    }
    unsigned long long *host = reinterpret_cast<unsigned long long *>(static_cast<char *>(ctx->ld_host) + stage_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host, b.bins, (size_t)n_bins * 24, hipMemcpyDeviceToHost, stream));
    fill_pairs();
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < n_bins; ++k) {
        bins[k].defined = host[3 * k], bins[k].links = host[3 * k + 1];
        bins[k].r2_sum = (double)host[3 * k + 2] * (1.0 / (double)(1ull << DST_LD_SCALE_BITS));
    }
    return DST_OK;
}
