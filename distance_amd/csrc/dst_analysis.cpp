// dst_analysis.cpp — the analyses of the C ABI that consume a set's pairs slab by slab on the device and return an O(n)
// or O(n k) result: dst_nearest, dst_clusters, dst_representatives, dst_mst, dst_nj (+ _matrix, _bootstrap), dst_dendrogram
// (+ _matrix), dst_summary; and dst_links, which hands the pairs that pass a threshold to a sink.
// Each one is the same program: plan the row slabs, grow the context's slab scratch, walk the slabs (the
// pair kernel of a slab into the scratch, the analysis' kernels directly behind it), carve its O(n) state out of one
// allocation, copy the result back.  Everything runs on the context's stream and waits before it returns.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dst_ctx.h"

using namespace dst;

namespace dst {

SlabPlan plan_slabs(bool square, uint64_t n_rows, uint64_t n_cols, uint64_t max_pairs, uint64_t default_pairs)
{
    SlabPlan plan;
    plan.slabs = cut_row_slabs(square, n_rows, n_cols, max_pairs ? max_pairs : default_pairs);
    for (const RowSlab &s : plan.slabs)
        plan.biggest = std::max(plan.biggest, s.pairs);
    return plan;
}

}  // namespace dst

namespace {

// An analysis takes the context's stream over here: whatever an earlier call queued has finished after the wait, so
// nothing reads the grow-only buffers any more and they may be replaced.  Then the slab scratch grows to `bytes` (the
// largest slab in the call's output kind); wanted = false: a call that will run no slab leaves it alone.
int slab_scratch(dst_ctx *ctx, size_t bytes, bool wanted = true)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!wanted)
        return DST_OK;
    return ctx->pair_slab.grow(ctx, std::max<size_t>(bytes, 256));
}

// Every slab in order: its pairs, each once (square: the triangle), as `out_kind` into the slab scratch, then
// consume(slab), whose launches go on the context's stream directly behind the slab's pair kernel.  Nothing waits.
template <typename Consume>
int walk_slabs(dst_ctx *ctx, int measure, bool square, DeviceSet &rows, DeviceSet &cols, const std::vector<RowSlab> &slabs,
               int out_kind, Consume &&consume)
{
    for (const RowSlab &s : slabs) {
        int rc = run_sets(ctx, measure, square, rows, cols, s.rb, s.re, out_kind, ctx->pair_slab, ctx->pair_slab.bytes,
                          (void *)ctx->stream);
        if (!rc)
            rc = consume(s);
        if (rc)
            return rc;
    }
    return DST_OK;
}

// Pieces of one allocation, each 256-byte aligned.  A layout is written once as a function over a Carve: run on a null
// base it only adds up `used` (every pointer null), run on the allocation it sets the pointers.
struct Carve {
    char *base;
    size_t used = 0;
    explicit Carve(void *b) : base(static_cast<char *>(b)) {}
    template <typename T>
    T *take(size_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

int not_finite(dst_ctx *ctx, int status, const std::string &prefix, uint64_t i, uint64_t j)
{
    return fail(ctx, status, prefix + "the distance of records " + std::to_string(i) + " and " + std::to_string(j) +
                                 " is not finite");
}

// a caller's n x n matrix: the first non-finite entry of the upper triangle ends the call
int matrix_finite(dst_ctx *ctx, const std::string &prefix, const double *d, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = i + 1; j < n; ++j)
            if (!std::isfinite(d[i * n + j]))
                return not_finite(ctx, DST_ERR_ARG, prefix, i, j);
    return DST_OK;
}

}  // namespace

// dst_summary's conversion: the exact sum hi 2^32 + lo to double once (round to nearest even), f64 measures scaled by
// 2^-DST_SUMMARY_SCALE_BITS (exact)
double dst::summary_value(__int128 s, bool int_payload)
{
    const double d = (double)s;
    return int_payload ? d : std::ldexp(d, -DST_SUMMARY_SCALE_BITS);
}

// dst_summary's rules for a histogram's bin width, and the width as a fixed-point value (a summary stream shares them)
int dst::summary_width_q(dst_ctx *ctx, int measure, double width, uint64_t &width_q)
{
    const bool int_payload = measure_is_int(measure);
    if (!(width > 0 && width < 0x1p25))   // (NaN fails both)
        return fail(ctx, DST_ERR_ARG, "width must be finite, above 0 and below 2^25");
    if (int_payload && width != std::floor(width))
        return fail(ctx, DST_ERR_ARG, "width must be an integer for n and n_high");
    width_q = int_payload ? (uint64_t)width : (uint64_t)std::llrint(std::ldexp(width, DST_SUMMARY_SCALE_BITS));
    if (width_q < 1)
        return fail(ctx, DST_ERR_ARG, "width is below one unit of the fixed-point scale");
    return DST_OK;
}

// The threshold of dst_clusters / dst_links / a links stream as a payload: int64 payloads link when v <= floor(T) (clamped
// to the int64 range), f64 payloads on their bits through nn_key.  false: floor(T) is below -2^63, nothing links.
bool dst::threshold_payload(int measure, double threshold, uint64_t &t_bits)
{
    if (!measure_is_int(measure)) {
        std::memcpy(&t_bits, &threshold, 8);
        return true;
    }
    const double f = std::floor(threshold);
    bool any = true;
    int64_t t;
    if (f >= 9223372036854775808.0)
        t = INT64_MAX;
    else if (f < -9223372036854775808.0) {
        t = INT64_MIN;
        any = false;
    } else
        t = (int64_t)f;
    t_bits = (uint64_t)t;
    return any;
}

namespace {

size_t links_layout(void *base, uint64_t blocks, uint64_t chunk, bool values, int W, LinksBuffers &b)
{
    Carve c(base);
    b.counts = c.take<uint32_t>(blocks);
    b.offsets = c.take<uint64_t>(blocks + 1);
    b.grand = c.take<uint64_t>(1);
    b.row = c.take<uint32_t>(chunk);
    b.col = c.take<uint32_t>(chunk);
    b.val = c.take<uint64_t>(values ? chunk : 0);
    b.tal = c.take<uint32_t>(chunk * (size_t)W);
    return c.used;
}

size_t summary_layout(void *base, uint64_t records, uint32_t bins, SummaryBuffers &b)
{
    Carve c(base);
    b.within = c.take<uint32_t>(records);
    b.summable = c.take<uint32_t>(records);
    b.hi = c.take<int64_t>(records);
    b.lo = c.take<uint64_t>(records);
    b.hist = c.take<uint64_t>(bins);
    b.tot = c.take<uint64_t>(kSummaryTotals);
    return c.used;
}

size_t nearest_layout(void *base, uint64_t entries, int W, NearestLists &nl)
{
    Carve c(base);
    nl.val = c.take<uint64_t>(entries);
    nl.idx = c.take<uint32_t>(entries);
    nl.tal = c.take<uint32_t>(entries * (size_t)W);
    return c.used;
}

size_t mst_layout(void *base, uint64_t n, int W, MstBuffers &b)
{
    Carve c(base);
    b.comp = c.take<uint32_t>(n);
    b.hook = c.take<uint32_t>(n);
    b.best_key = c.take<uint64_t>(n);
    b.best_pair = c.take<uint64_t>(n);
    b.edges = c.take<uint64_t>(n);
    b.edge_keys = c.take<uint64_t>(n);
    b.val = c.take<uint64_t>(n);
    b.tal = c.take<uint32_t>(n * (size_t)W);
    b.counters = c.take<uint64_t>(2);
    return c.used;
}

// The device memory of one n x n f64 square (dst_nj, dst_dendrogram and their forms): the two matrix buffers and one
// block for the rest.  Per call, not grow-only: the square of 50,000 records is 20 GB.  Freed behind the context's
// stream: the members go after the destructor's wait.  A dendrogram needs no compaction: setup(n, false) leaves the second
// matrix buffer out.
struct SquareAlloc {
    dst_ctx *ctx;
    const char *what;
    Grown<double> D0, D1;
    Grown<> work;
    NjBuffers b{};
    unsigned long long *bad = nullptr;
    explicit SquareAlloc(dst_ctx *c, const char *w = "neighbour joining") : ctx(c), what(w) {}
    ~SquareAlloc() { (void)hipStreamSynchronize(ctx->stream); }
    size_t layout(void *base, uint64_t n)
    {
        const size_t nodes = 2 * n - 2;
        Carve c(base);
        b.r[0] = c.take<double>(n);
        b.r[1] = c.take<double>(n);
        b.ids[0] = c.take<uint32_t>(n);
        b.ids[1] = c.take<uint32_t>(n);
        b.active = c.take<uint8_t>(n);
        b.pos = c.take<uint32_t>(n);
        b.part_key = c.take<uint64_t>(kNjScanBlocks);
        b.part_ij = c.take<uint64_t>(kNjScanBlocks);
        b.parent = c.take<uint32_t>(nodes);
        b.length = c.take<double>(nodes);
        bad = c.take<unsigned long long>(1);
        return c.used;
    }
    int setup(uint64_t n, bool compaction = true)
    {
        const uint64_t n1 = std::max<uint64_t>(3 * n / 4, 1);
        int rc = D0.grow(ctx, n * n * 8, what);
        if (!rc && compaction)
            rc = D1.grow(ctx, n1 * n1 * 8, what);
        if (!rc)
            rc = work.grow(ctx, layout(nullptr, n), what);
        if (rc)
            return rc;
        layout(work, n);
        b.D[0] = D0;
        b.D[1] = D1;
        return DST_OK;
    }
};

// the row slabs of the fill of an n-record square and the slab scratch for them
int square_slabs(dst_ctx *ctx, int measure, uint64_t n, uint64_t max_pairs, SlabPlan &plan)
{
    plan = plan_slabs(true, n, n, max_pairs, kClusterSlabPairs);
    return slab_scratch(ctx, dst_out_bytes(measure, DST_OUT_DISTANCE, plan.biggest));
}

// the square of `set` into al's first matrix buffer and the non-finite flag, queued on the context's stream without a
// wait: the initial state, then per slab its DST_OUT_DISTANCE payloads, scattered
int square_fill(dst_ctx *ctx, int measure, DeviceSet &set, const SlabPlan &plan, SquareAlloc &al)
{
    hipStream_t stream = ctx->stream;
    const uint64_t n = set.n;
    HIP_TRY(ctx, launch_nj_init(al.b.D[0], n, al.b.ids[0], al.b.active, al.bad, stream));
    return walk_slabs(ctx, measure, true, set, set, plan.slabs, DST_OUT_DISTANCE, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_nj_scatter(measure, static_cast<const uint64_t *>(ctx->pair_slab.ptr), s.first, n, s.rb, s.re,
                                       al.b.D[0], al.bad, stream));
        return DST_OK;
    });
}

// the message of a non-finite fill: the first pair in canonical order, from the flag's linear index i * n + j
int square_bad_pair(dst_ctx *ctx, const std::string &prefix, unsigned long long bad, uint64_t n)
{
    return not_finite(ctx, DST_ERR_STATE, prefix, bad / n, bad % n);
}

// one look at the fill before the rounds: a non-finite distance ends the call
int square_check(dst_ctx *ctx, const SquareAlloc &al, uint64_t n)
{
    unsigned long long bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, al.bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return bad == ~0ull ? DST_OK : square_bad_pair(ctx, std::string(al.what) + ": ", bad, n);
}

int nj_check_out(dst_ctx *ctx, uint64_t n, uint32_t *parent, double *length, size_t cap)
{
    if (!parent || !length)
        return fail(ctx, DST_ERR_ARG, "null parent or length pointer");
    if (n < 3)
        return fail(ctx, DST_ERR_ARG, "neighbour joining needs at least 3 records");
    if (n >= ((uint64_t)1 << 31))
        return fail(ctx, DST_ERR_ARG, "neighbour joining of 2^31 records or more");
    if (cap < 2 * n - 2)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below 2n - 2 entries");
    return DST_OK;
}

// the rounds behind the fill on the context's stream, then one copy of the tree to the host
int nj_finish(dst_ctx *ctx, SquareAlloc &al, uint64_t n, uint32_t *parent, double *length)
{
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, launch_nj_rounds(al.b, n, stream));
    HIP_TRY(ctx, hipMemcpyAsync(parent, al.b.parent, (2 * n - 2) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(length, al.b.length, (2 * n - 2) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

// dst_nj_bootstrap's device memory beside SquareAlloc: the original codes, the replicate's codes (both n x pitch) and
// the column map.  Freed behind the context's stream (the members go after the destructor's wait), with the replicate's
// packed set.
struct BootAlloc {
    dst_ctx *ctx;
    Grown<uint8_t> src, rep;
    Grown<uint32_t> map;
    explicit BootAlloc(dst_ctx *c) : ctx(c) {}
    ~BootAlloc()
    {
        (void)hipStreamSynchronize(ctx->stream);
        free_set(ctx->boot);
    }
    int setup(uint64_t n, uint64_t pitch, uint64_t len)
    {
        int rc = src.grow(ctx, std::max<size_t>(n * pitch, 128), "bootstrap");
        if (!rc)
            rc = rep.grow(ctx, std::max<size_t>(n * pitch, 128), "bootstrap");
        if (!rc)
            rc = map.grow(ctx, std::max<size_t>(len * 4, 4), "bootstrap");
        return rc;
    }
};

int dg_check(dst_ctx *ctx, uint64_t n, int linkage, uint32_t *parent, double *length, size_t cap)
{
    if (linkage < DST_LINK_AVERAGE || linkage > DST_LINK_COMPLETE)
        return fail(ctx, DST_ERR_ARG, "unknown linkage");
    if (!parent || !length)
        return fail(ctx, DST_ERR_ARG, "null parent or length pointer");
    if (n < 2)
        return fail(ctx, DST_ERR_ARG, "a dendrogram needs at least 2 records");
    if (n >= ((uint64_t)1 << 31))
        return fail(ctx, DST_ERR_ARG, "a dendrogram of 2^31 records or more");
    if (n > ((uint64_t)1 << 30))   // (8 n^2 must fit 64 bits before it is asked for; 2^30 records are 2^63 bytes)
        return fail(ctx, DST_ERR_NOMEM, "dendrogram: a square of " + std::to_string(n) + " records does not fit device memory");
    if (cap < 2 * n - 1)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below 2n - 1 entries");
    return DST_OK;
}

size_t dg_layout(void *base, uint64_t n, DgBuffers &b)
{
    const size_t nodes = 2 * n - 1, nblk = (n + kDgBlockRows - 1) / kDgBlockRows;
    Carve c(base);
    b.size = c.take<uint32_t>(n);
    b.row_key = c.take<uint64_t>(n);
    b.row_col = c.take<uint32_t>(n);
    b.blk_key = c.take<uint64_t>(nblk);
    b.list = c.take<uint32_t>(n);
    b.counters = c.take<uint32_t>(12);   // one piece for the three: the scan count at +16, the round's pair at +32
    b.parent = c.take<uint32_t>(nodes);
    b.length = c.take<double>(nodes);
    b.height = c.take<double>(nodes);
    return c.used;
}

// the O(n) state of a dendrogram call in the context's grow-only scratch, beside the square (and its flags) of `al`
int dg_buffers(dst_ctx *ctx, SquareAlloc &al, uint64_t n, DgBuffers &b)
{
    const size_t total = dg_layout(nullptr, n, b);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (an earlier call's state goes before it is replaced)
    if (int rc = ctx->dg_work.grow(ctx, total))
        return rc;
    dg_layout(ctx->dg_work, n, b);
    b.scans = reinterpret_cast<unsigned long long *>(b.counters + 4);
    b.pair = reinterpret_cast<DgPair *>(b.counters + 8);
    b.D = al.b.D[0];
    b.active = al.b.active;
    b.node = al.b.ids[0];
    return DST_OK;
}

// the rounds behind the fill on the context's stream, then one copy of the tree to the host
int dg_finish(dst_ctx *ctx, const DgBuffers &b, uint64_t n, int linkage, uint32_t *parent, double *length, double *height,
              uint64_t *row_scans)
{
    hipStream_t stream = ctx->stream;
    unsigned long long scans = 0;
    HIP_TRY(ctx, launch_dg_init(b, n, stream));
    HIP_TRY(ctx, launch_dg_rounds(b, n, linkage, stream));
    HIP_TRY(ctx, hipMemcpyAsync(parent, b.parent, (2 * n - 1) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(length, b.length, (2 * n - 1) * 8, hipMemcpyDeviceToHost, stream));
    if (height)
        HIP_TRY(ctx, hipMemcpyAsync(height, b.height, (2 * n - 1) * 8, hipMemcpyDeviceToHost, stream));
    uint32_t failed = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&scans, b.scans, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(&failed, b.counters + 2, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (row_scans)
        *row_scans = scans;
    if (failed)   // (the row-minimum cache lost the pair: never a tree that is silently wrong)
        return fail(ctx, DST_ERR_STATE, "dendrogram: internal error, round " + std::to_string(failed - 1) +
                                            " found no active pair");
    return DST_OK;
}

// ---- dst_run_pairs -------------------------------------------------------------------------------------
// DST_PAIRS_AUTO compares two estimates, in nanoseconds, over the entries that have a canonical position:
//   direct   entries x (kPairsDirectEntryNs + 2 NP nchunks cache lines (dst_pairs.hip, "memory") x kPairsLineNs)
//   sweep    the pairs of the slabs the list touches x the cost of a swept pair + entries x kPairsSweepEntryNs
// The constants were set from a run of tools/run_pairs_bench.py and are held to the figures of one MI355X session with them
// built in (profiles/run_pairs/), the tools/synth
// alignment at 50,000 x 30,000 and 10,000 x 1,000, -m n and tn93, lists of 1e3 to 1e7 random pairs:
//   kPairsLineNs         0.0197 - 0.0211 ns per line at 30,000 sites on lists of 1e5 and 1e7 pairs
//   kPairsDirectEntryNs  what is left of the 2.2 - 2.3 ns per entry at 1,000 sites: staging and scatter on the host
//   kPairsSweepEntryNs   5.7 - 6.0 ns per entry at 10,000 records, 19.4 - 19.5 at 50,000 (the counting sort, the staging, the
//                        gather from a 268 MB slab, the scatter): the larger, so that AUTO errs towards the direct route
//   kPairsSweepIntNs,    a swept pair on the consensus path, which writes at its output's rate whatever the width, by the
//   kPairsSweepF64Ns     slab's payload: 3.8 ps for -m n and 8.2 ps for tn93 at 50,000 records (7.2 and 15.5 ps at 10,000,
//                        where the direct route wins at every size anyway).  n_high takes n's figure and raw, jc69 and
//                        k80 take tn93's, the dearest finalisation: a supposition, none of the four was measured, and
//                        neither was a slab of tallies (a call that wants the tallies), which takes the same figures.
//                        Taken only where the slabs will run on that path: it is forced, or it is automatic and the
//                        column set's lists exist or were counted by its upload.
//   kPairsDenseNs        else: the dense pair kernel's 1.95e14 sites x pairs per second (kHotPermille's note in
//                        dst_internal.h; not measured again in that session), times len
// What the rule gives at 50,000 x 30,000 on the consensus path: the sweep from 2.5e5 listed pairs on for -m n (4.6 ms over
// 38.6 - 20 ns) and from 1.1e6 on for tn93 (10.4 ms over 29.2 - 20 ns), beside fitted crossovers of 2.6e5 and 1.05e6;
// at 10,000 x 1,000 never (2.3 ns per entry direct), as measured.
constexpr double kPairsLineNs = 0.02;
constexpr double kPairsDirectEntryNs = 1.0;
constexpr double kPairsSweepEntryNs = 20.0;
constexpr double kPairsSweepIntNs = 0.0037;
constexpr double kPairsSweepF64Ns = 0.0083;
constexpr double kPairsDenseNs = 1.0 / 1.95e5;

int pairs_planes(int measure)   // M::NP of the measure's traits (dst_measures.hpp)
{
    return measure == DST_RAW || measure == DST_JC69 ? 5 : measure == DST_TN93 ? 3 : 4;
}

// one batch of m entries on the device (and its page-locked copy): what goes in, then what comes back
struct PairsBatch {
    uint32_t *row, *col;
    uint64_t *pos, *val;
    uint32_t *tal;
    size_t idx_bytes, in_bytes;   // row + col; row + col + pos
};
size_t pairs_layout(void *base, uint64_t m, int W, PairsBatch &b)
{
    Carve c(base);
    b.row = c.take<uint32_t>(m);
    b.col = c.take<uint32_t>(m);
    b.idx_bytes = c.used;
    b.pos = c.take<uint64_t>(m);
    b.in_bytes = c.used;
    b.val = c.take<uint64_t>(m);
    b.tal = c.take<uint32_t>(m * (size_t)W);
    return c.used;
}

struct PairsJob {
    dst_ctx *ctx;
    int measure;
    bool square;
    DeviceSet *rows, *cols;
    const uint32_t *row, *col;   // the caller's list
    uint64_t *values;            // the caller's outputs (either may be NULL)
    uint32_t *tallies;
    int W;
    uint32_t lanes = 0;          // of the direct kernel's last launch

    // m <= DST_RUN_PAIRS_BATCH entries: entry k of the batch is list entry entry_of(k).  slab == NULL: the direct kernel;
    // else the gather from `slab` at pos_of(k).  Waits for the results and puts them where the caller wants them.
    template <typename EntryOf, typename PosOf>
    int batch(uint64_t m, EntryOf entry_of, const void *slab, bool tally_slab, PosOf pos_of)
    {
        hipStream_t stream = ctx->stream;
        PairsBatch d, h;
        pairs_layout(ctx->rp_batch.ptr, m, W, d);
        pairs_layout(ctx->rp_batch_host.ptr, m, W, h);
        for (uint64_t k = 0; k < m; ++k) {
            const uint64_t e = entry_of(k);
            const uint32_t i = row[e], j = col[e];
            const bool swap = square && i > j;   // the canonical pair (min, max): dst_nearest's rule
            h.row[k] = swap ? j : i;
            h.col[k] = swap ? i : j;
            if (slab)
                h.pos[k] = pos_of(k);
        }
        HIP_TRY(ctx, hipMemcpyAsync(d.row, h.row, slab ? d.in_bytes : d.idx_bytes, hipMemcpyHostToDevice, stream));
        PairsLaunch pl{};
        pl.rows = rows;
        pl.cols = cols;
        pl.row = d.row;
        pl.col = d.col;
        pl.pos = slab ? d.pos : nullptr;
        pl.pairs = (uint32_t)m;
        pl.values = values ? d.val : nullptr;
        pl.tallies = tallies ? d.tal : nullptr;
        pl.q_counts = rows->counts;
        pl.t_counts = cols->counts;
        if (slab)
            HIP_TRY(ctx, launch_pairs_gather(measure, pl, slab, tally_slab, stream));
        else
            HIP_TRY(ctx, launch_pairs_direct(measure, pl, stream, &lanes));
        if (values)
            HIP_TRY(ctx, hipMemcpyAsync(h.val, d.val, m * 8, hipMemcpyDeviceToHost, stream));
        if (tallies)
            HIP_TRY(ctx, hipMemcpyAsync(h.tal, d.tal, m * 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        for (uint64_t k = 0; k < m; ++k) {
            const uint64_t e = entry_of(k);
            if (values)
                values[e] = h.val[k];
            if (tallies)
                std::memcpy(tallies + e * (size_t)W, h.tal + k * (size_t)W, 4 * (size_t)W);
        }
        return DST_OK;
    }

    // what the direct kernel reads: the planes of the measure's traits, tn93's base counts for the values
    int prepare_direct()
    {
        hipStream_t stream = ctx->stream;
        if (int rc = order_after_prep(ctx, stream))
            return rc;
        const bool derived = measure != DST_N && measure != DST_N_HIGH;   // MRaw reads K, MK80 / MTN93 K, X1, X0 (, CL)
        for (DeviceSet *s : {rows, cols}) {
            if (int rc = derived ? ensure_derived(ctx, *s, stream) : ensure_planes(ctx, *s, stream))
                return rc;
            if (measure == DST_TN93 && values)
                if (int rc = need_counts(ctx, *s, stream))
                    return rc;
        }
        return DST_OK;
    }
};

}  // namespace

extern "C" {

int dst_nearest(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint32_t k, uint32_t *index,
                uint32_t *tallies, void *values, size_t cap_entries, uint32_t *k_used)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (k_used)
        *k_used = 0;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (k < 1 || k > kNearestMaxK)
        return fail(ctx, DST_ERR_ARG, "k must be between 1 and 256");
    if (!index || !k_used)
        return fail(ctx, DST_ERR_ARG, "null index or k_used pointer");
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts, true, true))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    const uint64_t candidates = square ? (n_rows > 0 ? n_rows - 1 : 0) : n_cols;
    const uint32_t ku = (uint32_t)std::min<uint64_t>(k, candidates);
    if (n_rows * ku > cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "cap_entries is below n_rows x k_used");
    if (ku == 0 || n_rows == 0) {
        *k_used = ku;
        return DST_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    int rc = DST_OK;
    if (measure == DST_TN93) {
        rc = need_counts(ctx, rows, stream);
        if (!rc && &cols != &rows)
            rc = need_counts(ctx, cols, stream);
        if (rc)
            return rc;
    }
    const SlabPlan plan = plan_slabs(square != 0, n_rows, n_cols, 0, kNearestSlabPairs);
    const uint64_t entries = n_rows * ku;
    const int W = tally_width(measure);
    NearestLists nl{};
    rc = slab_scratch(ctx, dst_out_bytes(measure, DST_OUT_TALLY, plan.biggest));
    if (!rc)
        rc = ctx->nn_lists.grow(ctx, nearest_layout(nullptr, entries, W, nl));
    if (rc)
        return rc;
    nearest_layout(ctx->nn_lists, entries, W, nl);
    nl.k = ku;
    HIP_TRY(ctx, launch_nearest_init(nl, n_rows, stream));
    const uint32_t *slab = static_cast<const uint32_t *>(ctx->pair_slab.ptr);
    // the slab's exact tallies, then both passes behind its pair kernel: they touch the same lists
    rc = walk_slabs(ctx, measure, square != 0, rows, cols, plan.slabs, DST_OUT_TALLY, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_nearest_rows(measure, square != 0, slab, s.first, n_cols, s.rb, s.re, rows.counts, cols.counts,
                                         nl, stream));
        if (square)
            HIP_TRY(ctx, launch_nearest_cols(measure, slab, s.first, n_cols, s.rb, s.re, cols.counts, nl, stream));
        return DST_OK;
    });
    if (rc)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(index, nl.idx, entries * 4, hipMemcpyDeviceToHost, stream));
    if (values)
        HIP_TRY(ctx, hipMemcpyAsync(values, nl.val, entries * 8, hipMemcpyDeviceToHost, stream));
    if (tallies)
        HIP_TRY(ctx, hipMemcpyAsync(tallies, nl.tal, entries * W * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    *k_used = ku;
    return DST_OK;
}

int dst_clusters(dst_ctx *ctx, int measure, double threshold, uint64_t max_pairs, uint32_t *label, size_t cap,
                 uint64_t *n_clusters, uint64_t *links)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_clusters)
        *n_clusters = 0;
    if (links)
        *links = 0;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (!label)
        return fail(ctx, DST_ERR_ARG, "null label pointer");
    DeviceSet &set = ctx->set[0];
    if (!set.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    const uint64_t n = set.n;
    if (n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    if (cap < n)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below the set's record count");
    uint64_t t_bits;
    const bool any = threshold_payload(measure, threshold, t_bits);
    if (n < 2) {
        if (n == 1)
            label[0] = 0;
        if (n_clusters)
            *n_clusters = n;
        return DST_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    SlabPlan plan = plan_slabs(true, n, n, max_pairs, kClusterSlabPairs);
    if (!any)
        plan.slabs.clear();   // (nothing can link: no slab is run, and no scratch is kept for one)
    uint32_t *parent = nullptr;
    unsigned long long *d_links = nullptr;
    auto layout = [&](void *base) {   // the parent array and the link counter
        Carve c(base);
        parent = c.take<uint32_t>(n);
        d_links = c.take<unsigned long long>(1);
        return c.used;
    };
    int rc = slab_scratch(ctx, dst_out_bytes(measure, DST_OUT_DISTANCE, plan.biggest), any);
    if (!rc)
        rc = ctx->cl_work.grow(ctx, layout(nullptr));
    if (rc)
        return rc;
    layout(ctx->cl_work);
    HIP_TRY(ctx, launch_clusters_init(parent, n, d_links, stream));
    // the slab's DST_OUT_DISTANCE payloads, then its unions behind the pair kernel (and the previous slab's unions)
    rc = walk_slabs(ctx, measure, true, set, set, plan.slabs, DST_OUT_DISTANCE, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_clusters_link(measure, static_cast<const uint64_t *>(ctx->pair_slab.ptr), s.first, n, s.rb, s.re, t_bits,
                                          parent, d_links, stream));
        return DST_OK;
    });
    if (rc)
        return rc;
    HIP_TRY(ctx, launch_clusters_final(parent, n, stream));
    uint64_t h_links = 0;
    HIP_TRY(ctx, hipMemcpyAsync(label, parent, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(&h_links, d_links, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    uint64_t roots = 0;
    for (uint64_t i = 0; i < n; ++i)
        roots += label[i] == i;
    if (n_clusters)
        *n_clusters = roots;
    if (links)
        *links = h_links;
    return DST_OK;
}

int dst_representatives(dst_ctx *ctx, int measure, double threshold, uint64_t max_pairs, uint32_t *rep, uint32_t *tallies,
                        void *values, size_t cap, uint64_t *n_representatives)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_representatives)
        *n_representatives = 0;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (!rep)
        return fail(ctx, DST_ERR_ARG, "null rep pointer");
    DeviceSet &set = ctx->set[0];
    if (!set.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    const uint64_t n = set.n;
    if (n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    if (cap < n)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below the set's record count");
    uint64_t t_bits;
    const bool any = threshold_payload(measure, threshold, t_bits);
    const int W = tally_width(measure);
    if (n < 2 || !any) {   // (nothing can link: every record its own representative, no slab is run)
        for (uint64_t i = 0; i < n; ++i)
            rep[i] = (uint32_t)i;
        if (values)
            std::memset(values, 0, n * 8);
        if (tallies)
            std::memset(tallies, 0, n * 4 * (size_t)W);
        if (n_representatives)
            *n_representatives = n;
        return DST_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const bool tally = tallies != nullptr;
    if (tally && measure == DST_TN93)
        if (int rc = need_counts(ctx, set, stream))
            return rc;
    const int kind = tally ? DST_OUT_TALLY : DST_OUT_DISTANCE;
    const SlabPlan plan = plan_slabs(true, n, n, max_pairs, kClusterSlabPairs);
    RepBuffers b{};
    auto layout = [&](void *base) {
        Carve c(base);
        b.rep = c.take<uint32_t>(n);
        b.bits = c.take<uint32_t>(n * (size_t)(kRepBlockRows / 32));
        b.val = values ? c.take<uint64_t>(n) : nullptr;
        b.tal = tally ? c.take<uint32_t>(n * (size_t)W) : nullptr;
        return c.used;
    };
    const size_t state_bytes = layout(nullptr);
    int rc = slab_scratch(ctx, dst_out_bytes(measure, kind, plan.biggest));
    if (!rc)
        rc = ctx->rep_work.grow(ctx, state_bytes);
    if (rc)
        return rc;
    layout(ctx->rep_work);
    // rep: unset (2^32-1) everywhere; values and tallies: the representatives' zero bits everywhere
    HIP_TRY(ctx, hipMemsetAsync(ctx->rep_work, 0, state_bytes, stream));
    HIP_TRY(ctx, hipMemsetAsync(b.rep, 0xFF, n * 4, stream));
    // the slab, then behind the pair kernel its link bits and its sub-blocks in order: resolve, cover and (when wanted) values each
    rc = walk_slabs(ctx, measure, true, set, set, plan.slabs, kind, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_rep_slab(measure, tally, ctx->pair_slab.ptr, s.first, n, s.rb, s.re, t_bits, set.counts, b, stream));
        return DST_OK;
    });
    if (rc)
        return rc;
    HIP_TRY(ctx, launch_rep_final(b.rep, n, stream));
    HIP_TRY(ctx, hipMemcpyAsync(rep, b.rep, n * 4, hipMemcpyDeviceToHost, stream));
    if (values)
        HIP_TRY(ctx, hipMemcpyAsync(values, b.val, n * 8, hipMemcpyDeviceToHost, stream));
    if (tally)
        HIP_TRY(ctx, hipMemcpyAsync(tallies, b.tal, n * 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    uint64_t count = 0;
    for (uint64_t i = 0; i < n; ++i)
        count += rep[i] == i;
    if (n_representatives)
        *n_representatives = count;
    return DST_OK;
}

int dst_links(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, double threshold, uint64_t max_pairs,
              int what, dst_links_sink sink, void *user, uint64_t *n_links)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_links)
        *n_links = 0;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (what & ~(DST_LINKS_VALUES | DST_LINKS_TALLIES))
        return fail(ctx, DST_ERR_ARG, "unknown bits in what");
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts, true, true))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    uint64_t t_bits;
    const bool any = threshold_payload(measure, threshold, t_bits);
    if (!any || (square ? n_rows < 2 : (n_rows == 0 || n_cols == 0)))
        return DST_OK;   // (nothing can link: no slab is run)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const bool values = sink && (what & DST_LINKS_VALUES), tallies = sink && (what & DST_LINKS_TALLIES);
    const int W = tally_width(measure);
    int rc = DST_OK;
    if (tallies && measure == DST_TN93) {
        rc = need_counts(ctx, rows, stream);
        if (!rc && &cols != &rows)
            rc = need_counts(ctx, cols, stream);
        if (rc)
            return rc;
    }
    const int kind = tallies ? DST_OUT_TALLY : DST_OUT_DISTANCE;
    const SlabPlan plan = plan_slabs(square != 0, n_rows, n_cols, max_pairs, kClusterSlabPairs);
    uint64_t blocks = 0;
    for (const RowSlab &s : plan.slabs)
        blocks = std::max(blocks, links_blocks(square != 0, n_cols, s.rb, s.re));
    // one window of outputs: never more links than the largest slab has pairs
    const uint64_t chunk = sink ? std::min<uint64_t>(DST_LINKS_CHUNK, plan.biggest) : 0;
    LinksBuffers b{};
    rc = slab_scratch(ctx, dst_out_bytes(measure, kind, plan.biggest));
    if (!rc)
        rc = ctx->links_work.grow(ctx, links_layout(nullptr, blocks, chunk, values, tallies ? W : 0, b));
    // the host copy: row, col, values, tallies, each piece where the window's entries of it start
    const size_t h_col = chunk * 4, h_val = h_col + chunk * 4, h_tal = h_val + (values ? chunk * 8 : 0);
    if (!rc && sink)
        rc = ctx->links_host.grow(ctx, h_tal + (tallies ? chunk * 4 * (size_t)W : 0), "links");
    if (rc)
        return rc;
    links_layout(ctx->links_work, blocks, chunk, values, tallies ? W : 0, b);
    char *host = ctx->links_host;
    HIP_TRY(ctx, hipMemsetAsync(b.grand, 0, 8, stream));
    uint64_t total = 0;
    // the slab, its block counts and their scan behind the pair kernel; with a sink the slab's total comes back (one wait),
    // then every window of at most `chunk` ranks is written, copied (one wait) and handed over
    rc = walk_slabs(ctx, measure, square != 0, rows, cols, plan.slabs, kind, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_links_count(measure, tallies, square != 0, ctx->pair_slab, s.first, n_cols, s.rb, s.re, t_bits,
                                        rows.counts, cols.counts, b, stream));
        if (!sink)
            return DST_OK;
        uint64_t in_slab = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&in_slab, b.offsets + links_blocks(square != 0, n_cols, s.rb, s.re), 8,
                                    hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        if (in_slab > s.pairs)
            return fail(ctx, DST_ERR_STATE, "links: more links than pairs in a slab");
        for (uint64_t lo = 0; lo < in_slab; lo += chunk) {
            const uint64_t hi = std::min(in_slab, lo + chunk), m = hi - lo;
            HIP_TRY(ctx, launch_links_write(measure, tallies, square != 0, ctx->pair_slab, s.first, n_cols, s.rb, s.re, t_bits,
                                            rows.counts, cols.counts, b, lo, hi, values, tallies, stream));
            HIP_TRY(ctx, hipMemcpyAsync(host, b.row, m * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipMemcpyAsync(host + h_col, b.col, m * 4, hipMemcpyDeviceToHost, stream));
            if (values)
                HIP_TRY(ctx, hipMemcpyAsync(host + h_val, b.val, m * 8, hipMemcpyDeviceToHost, stream));
            if (tallies)
                HIP_TRY(ctx, hipMemcpyAsync(host + h_tal, b.tal, m * 4 * (size_t)W, hipMemcpyDeviceToHost, stream));
            HIP_TRY(ctx, hipStreamSynchronize(stream));
            if (sink(user, total, m, reinterpret_cast<const uint32_t *>(host), reinterpret_cast<const uint32_t *>(host + h_col),
                     values ? host + h_val : nullptr, tallies ? reinterpret_cast<const uint32_t *>(host + h_tal) : nullptr))
                return fail(ctx, DST_ERR_STATE, "stopped by sink");
            total += m;
            if (n_links)
                *n_links = total;
        }
        return DST_OK;
    });
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

uint32_t dst_run_pairs_lanes(uint64_t len)
{
    return pairs_lanes(std::max<uint64_t>((len + kChunkSites - 1) / kChunkSites, 1));
}

int dst_run_pairs(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, const uint32_t *row, const uint32_t *col,
                  uint64_t n_pairs, int route, uint64_t max_pairs, void *values, uint32_t *tallies, size_t cap_entries,
                  dst_pairs_info *info)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (info)
        *info = dst_pairs_info{};
    if (!row || !col)
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (route != DST_PAIRS_AUTO && route != DST_PAIRS_DIRECT && route != DST_PAIRS_SWEEP)
        return fail(ctx, DST_ERR_ARG, "unknown route");
    if (!values && !tallies)
        return fail(ctx, DST_ERR_ARG, "values and tallies are both NULL");
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    if (rows.partial || cols.partial)
        return fail(ctx, DST_ERR_STATE, "a set uploaded with dst_upload_shared runs on the consensus path only (this rank holds "
                                        "the planes of its own records)");
    if (rows.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond dst_run_pairs");
    for (uint64_t e = 0; e < n_pairs; ++e)
        if (row[e] >= rows.n || col[e] >= cols.n) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "pair %llu (%u, %u) is out of range: %zu row records, %zu column records",
                          (unsigned long long)e, row[e], col[e], rows.n, cols.n);
            return fail(ctx, DST_ERR_ARG, msg);
        }
    if (n_pairs == 0)
        return DST_OK;
    if (cap_entries < n_pairs)
        return fail(ctx, DST_ERR_CAPACITY, "cap_entries is below n_pairs");
    const bool sq = square != 0;
    const uint64_t n_cols = cols.n;
    const int W = tally_width(measure);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (nothing queued earlier reads the grow-only buffers any more)

    // ---- the route: every entry's canonical position and slab; the square's diagonal has neither and stays direct
    SlabPlan plan;
    std::vector<std::pair<uint64_t, uint64_t>> swept;   // (canonical position, list entry), the entries of a slab together
    std::vector<uint64_t> first_of;                      // per slab of the plan: where its entries start in `swept` (+ the end)
    std::vector<uint64_t> diagonal;
    if (route != DST_PAIRS_DIRECT) {
        plan = plan_slabs(sq, rows.n, n_cols, max_pairs, kClusterSlabPairs);
        const size_t n_slabs = plan.slabs.size();
        std::vector<uint32_t> slab_of_row(rows.n, 0);   // (a row without pairs, the square's last, is never asked for)
        for (size_t s = 0; s < n_slabs; ++s)
            std::fill(slab_of_row.begin() + plan.slabs[s].rb, slab_of_row.begin() + plan.slabs[s].re, (uint32_t)s);
        first_of.assign(n_slabs + 1, 0);
        for (uint64_t e = 0; e < n_pairs; ++e) {
            if (sq && row[e] == col[e])
                diagonal.push_back(e);
            else
                ++first_of[slab_of_row[sq ? std::min(row[e], col[e]) : row[e]] + 1];
        }
        double swept_pairs = 0;
        for (size_t s = 0; s < n_slabs; ++s)
            if (first_of[s + 1])
                swept_pairs += (double)plan.slabs[s].pairs;
        const uint64_t n_swept = n_pairs - diagonal.size();
        if (route == DST_PAIRS_AUTO) {
            const double direct_ns = (double)n_swept * (kPairsDirectEntryNs + 2.0 * pairs_planes(measure) * (double)rows.nchunks * kPairsLineNs);
            const bool lists = ctx->path == DST_PATH_CONSENSUS || ctx->path == DST_PATH_HYBRID ||
                               (ctx->path == DST_PATH_AUTO && (cols.rec.valid || cols.rec.pre_valid));
            const double pair_ns = !lists ? (double)rows.len * kPairsDenseNs
                                   : measure_is_int(measure) ? kPairsSweepIntNs : kPairsSweepF64Ns;
            const double sweep_ns = swept_pairs * pair_ns + (double)n_swept * kPairsSweepEntryNs;
            route = sweep_ns < direct_ns ? DST_PAIRS_SWEEP : DST_PAIRS_DIRECT;
        }
        if (route == DST_PAIRS_SWEEP) {
            // a counting sort by slab: inside a slab the gather takes the entries in the list's order
            for (size_t s = 0; s < n_slabs; ++s)
                first_of[s + 1] += first_of[s];
            std::vector<uint64_t> next(first_of.begin(), first_of.end() - 1);
            swept.resize(n_swept);
            for (uint64_t e = 0; e < n_pairs; ++e) {
                const uint64_t i = sq ? std::min(row[e], col[e]) : row[e], j = sq ? std::max(row[e], col[e]) : col[e];
                if (sq && i == j)
                    continue;
                swept[next[slab_of_row[i]]++] = {sq ? square_row_start(n_cols, i) + (j - i - 1) : i * n_cols + j, e};
            }
        }
    }
    const bool all_direct = route == DST_PAIRS_DIRECT;
    const uint64_t n_direct = all_direct ? n_pairs : diagonal.size();

    PairsJob job{ctx, measure, sq, &rows, &cols, row, col, static_cast<uint64_t *>(values), tallies, W};
    const uint64_t mb = std::min<uint64_t>(n_pairs, DST_RUN_PAIRS_BATCH);
    PairsBatch sizes;
    const size_t batch_bytes = pairs_layout(nullptr, mb, W, sizes);
    if (int rc = ctx->rp_batch.grow(ctx, batch_bytes))
        return rc;
    if (int rc = ctx->rp_batch_host.grow(ctx, batch_bytes, "run pairs"))
        return rc;
    const auto no_pos = [](uint64_t) { return (uint64_t)0; };
    if (n_direct) {
        if (int rc = job.prepare_direct())
            return rc;
        for (uint64_t e0 = 0; e0 < n_direct; e0 += mb) {
            const uint64_t m = std::min(mb, n_direct - e0);
            const int rc = all_direct ? job.batch(m, [&](uint64_t k) { return e0 + k; }, nullptr, false, no_pos)
                                      : job.batch(m, [&](uint64_t k) { return diagonal[e0 + k]; }, nullptr, false, no_pos);
            if (rc)
                return rc;
        }
    }
    uint64_t slabs_run = 0;
    if (!all_direct && !swept.empty()) {
        // the touched slabs, each with its range of `swept`; a request for the tallies runs the slab in tallies and the
        // gather finalises the values from them (pair_value: no second arithmetic)
        const bool tally_slab = tallies != nullptr;
        const int kind = tally_slab ? DST_OUT_TALLY : DST_OUT_DISTANCE;
        std::vector<RowSlab> walk;
        std::vector<std::pair<uint64_t, uint64_t>> range;   // [begin, end) of `swept` per walked slab
        uint64_t biggest = 0;
        for (size_t s = 0; s + 1 < first_of.size(); ++s)
            if (first_of[s + 1] > first_of[s]) {
                walk.push_back(plan.slabs[s]);
                range.emplace_back(first_of[s], first_of[s + 1]);
                biggest = std::max(biggest, plan.slabs[s].pairs);
            }
        if (tally_slab && values && measure == DST_TN93) {
            int rc = need_counts(ctx, rows, ctx->stream);
            if (!rc && &cols != &rows)
                rc = need_counts(ctx, cols, ctx->stream);
            if (rc)
                return rc;
        }
        if (int rc = slab_scratch(ctx, dst_out_bytes(measure, kind, biggest)))
            return rc;
        // the slabs' pair kernels are this call's own business: what the caller's last run left to ask about stays
        const int last_path = ctx->last_path;
        const dst_launch_info last_launch = ctx->last_launch;
        size_t at = 0;
        const int rc = walk_slabs(ctx, measure, sq, rows, cols, walk, kind, [&](const RowSlab &s) -> int {
            const uint64_t a = range[at].first, b = range[at].second;
            ++at;
            for (uint64_t e0 = a; e0 < b; e0 += mb) {
                const uint64_t m = std::min(mb, b - e0);
                if (int rc2 = job.batch(m, [&](uint64_t k) { return swept[e0 + k].second; }, ctx->pair_slab.ptr, tally_slab,
                                        [&](uint64_t k) { return swept[e0 + k].first - s.first; }))
                    return rc2;
            }
            return DST_OK;
        });
        ctx->last_path = last_path;
        ctx->last_launch = last_launch;
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        slabs_run = walk.size();
    }
    if (info) {
        info->route = route;
        info->lanes_per_pair = job.lanes;
        info->direct_pairs = n_direct;
        info->swept_pairs = n_pairs - n_direct;
        info->slabs = slabs_run;
    }
    return DST_OK;
}

int dst_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, double threshold, uint64_t max_pairs,
                uint32_t bins, double width, uint64_t *hist, uint32_t *within, uint32_t *summable, double *sum, size_t cap,
                dst_summary_totals *totals)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (totals)
        *totals = dst_summary_totals{0, 0, 0, 0, 0.0};
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    const bool int_payload = measure_is_int(measure);
    uint64_t width_q = 0;
    if (bins) {
        if (bins > DST_SUMMARY_MAX_BINS)
            return fail(ctx, DST_ERR_ARG, "bins must be between 0 and 4096");
        if (!hist)
            return fail(ctx, DST_ERR_ARG, "null hist pointer");
        if (int rc = summary_width_q(ctx, measure, width, width_q))
            return rc;
    }
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts, true, true))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    const bool per_record = within || summable || sum;
    if (per_record && cap < n_rows)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below the row set's record count");
    for (uint64_t x = 0; x < n_rows; ++x) {   // (also what an empty call returns)
        if (within)
            within[x] = 0;
        if (summable)
            summable[x] = 0;
        if (sum)
            sum[x] = 0.0;
    }
    for (uint32_t k = 0; k < bins; ++k)
        hist[k] = 0;
    if (square ? n_rows < 2 : (n_rows == 0 || n_cols == 0))
        return DST_OK;   // (no pair: no slab is run)
    const uint64_t pairs = square ? n_rows * (n_rows - 1) / 2 : n_rows * n_cols;
    // the flat pass counts the totals as it goes, so it also serves a call that wants the totals and no per-record array
    const bool flat = bins > 0 || (totals && !per_record);
    if (!per_record && !flat)
        return DST_OK;   // (nothing is asked for)
    uint64_t t_bits;
    const bool any = threshold_payload(measure, threshold, t_bits);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const SlabPlan plan = plan_slabs(square != 0, n_rows, n_cols, max_pairs, kClusterSlabPairs);
    SummaryBuffers b{};
    const size_t state_bytes = summary_layout(nullptr, n_rows, bins, b);
    int rc = slab_scratch(ctx, dst_out_bytes(measure, DST_OUT_DISTANCE, plan.biggest));
    if (!rc)
        rc = ctx->summary_work.grow(ctx, state_bytes);
    if (rc)
        return rc;
    summary_layout(ctx->summary_work, n_rows, bins, b);
    static const bool no_aggregation = std::getenv("DST_SUMMARY_NO_AGGREGATION") != nullptr;   // measurement knob
    HIP_TRY(ctx, hipMemsetAsync(ctx->summary_work, 0, state_bytes, stream));
    const uint64_t *slab = static_cast<const uint64_t *>(ctx->pair_slab.ptr);
    // the slab's DST_OUT_DISTANCE payloads, then the wanted passes behind its pair kernel
    rc = walk_slabs(ctx, measure, square != 0, rows, cols, plan.slabs, DST_OUT_DISTANCE, [&](const RowSlab &s) -> int {
        if (per_record) {
            HIP_TRY(ctx, launch_summary_rows(measure, square != 0, slab, s.first, n_cols, s.rb, s.re, t_bits, any, b, stream));
            if (square)
                HIP_TRY(ctx, launch_summary_cols(measure, slab, s.first, n_cols, s.rb, s.re, t_bits, any, b, stream));
        }
        if (flat)
            HIP_TRY(ctx, launch_summary_hist(measure, slab, s.pairs, bins, width_q, t_bits, any, !no_aggregation, b, stream));
        return DST_OK;
    });
    if (rc)
        return rc;
    // the state back in one copy, then the 128-bit sums here
    std::vector<char> host(state_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), ctx->summary_work, state_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    SummaryBuffers h{};
    summary_layout(host.data(), n_rows, bins, h);
    for (uint32_t k = 0; k < bins; ++k)
        hist[k] = h.hist[k];
    dst_summary_totals t{pairs, 0, 0, 0, 0.0};
    __int128 all = 0;
    if (flat) {
        t.nan_pairs = h.tot[0];
        t.summable_pairs = h.tot[1];
        t.links = h.tot[2];
        all = (__int128)(((unsigned __int128)h.tot[3] << 64) | h.tot[4]);   // (the flat pass' 128-bit total: high word, low word)
    }
    if (per_record) {
        // the totals from the records' entries too: every pair once in a rectangle, twice in the square
        uint64_t w2 = 0, s2 = 0;
        __int128 all2 = 0;
        for (uint64_t x = 0; x < n_rows; ++x) {
            const __int128 S = (__int128)h.hi[x] * ((__int128)1 << 32) + (__int128)h.lo[x];
            if (within)
                within[x] = h.within[x];
            if (summable)
                summable[x] = h.summable[x];
            if (sum)
                sum[x] = summary_value(S, int_payload);
            w2 += h.within[x];
            s2 += h.summable[x];
            all2 += S;
        }
        const unsigned each = square ? 2 : 1;
        if (w2 % each || s2 % each || all2 % each)
            return fail(ctx, DST_ERR_STATE, "summary: internal error, the two sides of the square disagree");
        if (flat && (t.links != w2 / each || t.summable_pairs != s2 / each || all != all2 / each || t.nan_pairs != h.tot[5]))
            return fail(ctx, DST_ERR_STATE, "summary: internal error, the passes disagree");
        if (!flat) {
            t.links = w2 / each;
            t.summable_pairs = s2 / each;
            all = all2 / each;
            t.nan_pairs = h.tot[5];
        }
    }
    t.sum = summary_value(all, int_payload);
    if (totals)
        *totals = t;
    return DST_OK;
}

namespace {

// the labels, then what comes back (the cells; behind them the per-record table), as one allocation
size_t group_layout(void *base, bool square, uint64_t n_rows, uint64_t n_cols, uint32_t g_rows, uint32_t g_cols, GroupBuffers &b,
                    size_t &cells_at, size_t &table_at)
{
    Carve c(base);
    b.g_rows = g_rows;
    b.g_cols = g_cols;
    b.row_group = c.take<uint32_t>(n_rows);
    b.col_group = square ? b.row_group : c.take<uint32_t>(n_cols);
    b.order = c.take<uint32_t>(n_rows);
    cells_at = c.used;
    b.cell = c.take<uint64_t>((size_t)kGroupCellWords * g_rows * g_cols);
    table_at = c.used;
    b.counts = c.take<uint64_t>(n_rows * g_cols);
    b.hi = c.take<int64_t>(n_rows * g_cols);
    b.lo = c.take<uint64_t>(n_rows * g_cols);
    return c.used;
}

}  // namespace

// shared with dst_window_group_summary (dst_windows.hip; declared in dst_internal.h)
extern "C++" {
namespace dst {

// the payload of a sort key (nn_key, dst_device.hpp): -0.0 has the key of +0.0 and comes back as +0.0
uint64_t payload_of_key(uint64_t key, bool int_payload)
{
    const uint64_t top = 0x8000000000000000ull;
    if (int_payload)
        return key ^ top;
    return (key & top) ? key & ~top : ~key;
}

int group_labels(dst_ctx *ctx, const uint32_t *group, uint64_t n, uint32_t count, const char *side, std::vector<uint64_t> &size)
{
    size.assign(count, 0);
    for (uint64_t x = 0; x < n; ++x) {
        if (group[x] == DST_GROUP_NONE)
            continue;
        if (group[x] >= count)
            return fail(ctx, DST_ERR_ARG, "group summary: " + std::string(side) + " record " + std::to_string(x) + " has label " +
                                              std::to_string(group[x]) + ", which is neither below the group count " +
                                              std::to_string(count) + " nor DST_GROUP_NONE");
        ++size[group[x]];
    }
    return DST_OK;
}

}  // namespace dst
}  // extern "C++"

int dst_group_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, const uint32_t *row_group,
                      uint32_t n_row_groups, const uint32_t *col_group, uint32_t n_col_groups, double threshold,
                      uint64_t max_pairs, dst_group_cell *cells, size_t cells_cap, uint32_t *rec_within, uint32_t *rec_summable,
                      double *rec_sum, size_t rec_cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (!row_group)
        return fail(ctx, DST_ERR_ARG, "null row_group pointer");
    const bool per_record = rec_within || rec_summable || rec_sum;
    if (!cells && !per_record)
        return fail(ctx, DST_ERR_ARG, "null cells pointer and no per-record array");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (square) {
        col_group = row_group;
        n_col_groups = n_row_groups;
    } else if (!col_group)
        return fail(ctx, DST_ERR_ARG, "null col_group pointer");
    if (n_row_groups == 0 || n_row_groups > DST_GROUPS_MAX || n_col_groups == 0 || n_col_groups > DST_GROUPS_MAX)
        return fail(ctx, DST_ERR_ARG, "a group count must be between 1 and " + std::to_string(DST_GROUPS_MAX));
    const bool int_payload = measure_is_int(measure);
    TwoSets ts;
    if (int rc = two_sets(ctx, square != 0, row_slot, col_slot, ts, true, true))
        return rc;
    DeviceSet &rows = *ts.rows, &cols = *ts.cols;
    const uint64_t n_rows = rows.n, n_cols = cols.n;
    const uint32_t Gr = n_row_groups, Gc = n_col_groups;
    std::vector<uint64_t> row_size, col_size_own;
    if (int rc = group_labels(ctx, row_group, n_rows, Gr, square ? "set" : "row", row_size))
        return rc;
    if (!square)
        if (int rc = group_labels(ctx, col_group, n_cols, Gc, "column", col_size_own))
            return rc;
    const std::vector<uint64_t> &col_size = square ? row_size : col_size_own;
    const size_t n_cells = (size_t)Gr * Gc;
    if (cells && cells_cap < n_cells)
        return fail(ctx, DST_ERR_CAPACITY, "cells_cap is below " + std::to_string(n_cells) + " entries (row groups x column groups)");
    if (per_record && rec_cap < n_rows * Gc)
        return fail(ctx, DST_ERR_CAPACITY, "rec_cap is below " + std::to_string(n_rows * Gc) +
                                               " entries (the row set's records x column groups)");
    // what an empty call returns; `pairs` from the group sizes
    const uint64_t none = int_payload ? 0 : 0x7FF8000000000000ull;
    if (cells)
        for (uint32_t a = 0; a < Gr; ++a)
            for (uint32_t b = 0; b < Gc; ++b) {
                const uint64_t p = square && a == b ? row_size[a] * (row_size[a] - (row_size[a] ? 1 : 0)) / 2 : row_size[a] * col_size[b];
                cells[(size_t)a * Gc + b] = dst_group_cell{p, 0, 0, 0, 0.0, none, none};
            }
    for (uint64_t e = 0; per_record && e < n_rows * Gc; ++e) {
        if (rec_within)
            rec_within[e] = 0;
        if (rec_summable)
            rec_summable[e] = 0;
        if (rec_sum)
            rec_sum[e] = 0.0;
    }
    if (square ? n_rows < 2 : (n_rows == 0 || n_cols == 0))
        return DST_OK;   // (no pair: no slab is run)
    uint64_t rows_assigned = 0, cols_assigned = 0;
    for (uint64_t s : row_size)
        rows_assigned += s;
    for (uint64_t s : col_size)
        cols_assigned += s;
    if (cols_assigned == 0 || (rows_assigned == 0 && !per_record))
        return DST_OK;   // (no partner has a group, or no cell has a pair and only the cells are wanted)
    uint64_t t_bits;
    const bool any = threshold_payload(measure, threshold, t_bits);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const SlabPlan plan = plan_slabs(square != 0, n_rows, n_cols, max_pairs, kClusterSlabPairs);
    GroupBuffers b{};
    size_t cells_at = 0, table_at = 0;
    const size_t state_bytes = group_layout(nullptr, square != 0, n_rows, n_cols, Gr, Gc, b, cells_at, table_at);
    int rc = slab_scratch(ctx, dst_out_bytes(measure, DST_OUT_DISTANCE, plan.biggest));
    if (rc)
        return rc;
    if (ctx->group_work.grow(ctx, state_bytes)) {
        (void)hipGetLastError();
        return fail(ctx, DST_ERR_NOMEM, "group summary: cannot allocate " + std::to_string(state_bytes) + " bytes of device memory");
    }
    // the labels and the row records in order of their group (a counting sort), through page-locked staging
    const size_t label_bytes = cells_at;
    rc = ctx->group_host.grow(ctx, label_bytes, "group summary");
    if (rc)
        return rc;
    GroupBuffers st{};
    size_t unused_a = 0, unused_b = 0;
    group_layout(ctx->group_host, square != 0, n_rows, n_cols, Gr, Gc, st, unused_a, unused_b);
    std::memcpy(st.row_group, row_group, n_rows * 4);
    if (!square)
        std::memcpy(st.col_group, col_group, n_cols * 4);
    {
        std::vector<uint64_t> next(Gr, 0);
        for (uint32_t a = 1; a < Gr; ++a)
            next[a] = next[a - 1] + row_size[a - 1];
        for (uint64_t x = 0; x < n_rows; ++x)
            if (row_group[x] != DST_GROUP_NONE)
                st.order[next[row_group[x]]++] = (uint32_t)x;
    }
    group_layout(ctx->group_work, square != 0, n_rows, n_cols, Gr, Gc, b, cells_at, table_at);
    static const bool no_aggregation = std::getenv("DST_GROUPS_NO_AGGREGATION") != nullptr;   // measurement knob
    char *dev = static_cast<char *>(ctx->group_work.ptr);
    HIP_TRY(ctx, hipMemcpyAsync(dev, ctx->group_host.ptr, label_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemsetAsync(dev + cells_at, 0, state_bytes - cells_at, stream));
    HIP_TRY(ctx, hipMemsetAsync(b.cell + 5 * n_cells, 0xFF, n_cells * 8, stream));   // (the min keys: none yet)
    const uint64_t *slab = static_cast<const uint64_t *>(ctx->pair_slab.ptr);
    rc = walk_slabs(ctx, measure, square != 0, rows, cols, plan.slabs, DST_OUT_DISTANCE, [&](const RowSlab &s) -> int {
        HIP_TRY(ctx, launch_group_rows(measure, square != 0, slab, s.first, n_cols, s.rb, s.re, t_bits, any, !no_aggregation, b, stream));
        if (square)
            HIP_TRY(ctx, launch_group_cols(measure, slab, s.first, n_cols, s.rb, s.re, t_bits, any, b, stream));
        return DST_OK;
    });
    if (rc)
        return rc;
    HIP_TRY(ctx, launch_group_fold(b, rows_assigned, stream));
    // the cells, and the table behind them when it is wanted, back in one copy
    const size_t back = (per_record ? state_bytes : table_at) - cells_at;
    std::vector<char> host(back);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), dev + cells_at, back, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    GroupBuffers h{};   // (the copy starts at the cells: the layout's pieces from there)
    const size_t piece = (n_rows * Gc * 8 + 255) / 256 * 256;
    h.cell = reinterpret_cast<uint64_t *>(host.data());
    if (per_record) {
        h.counts = reinterpret_cast<uint64_t *>(host.data() + (table_at - cells_at));
        h.hi = reinterpret_cast<int64_t *>(host.data() + (table_at - cells_at) + piece);
        h.lo = reinterpret_cast<uint64_t *>(host.data() + (table_at - cells_at) + 2 * piece);
    }
    if (cells) {
        const uint64_t *nan = h.cell, *links = h.cell + n_cells, *summ = h.cell + 2 * n_cells, *high = h.cell + 3 * n_cells,
                       *low = h.cell + 4 * n_cells, *kmin = h.cell + 5 * n_cells, *kmax = h.cell + 6 * n_cells;
        for (uint32_t a = 0; a < Gr; ++a)
            for (uint32_t g = 0; g < Gc; ++g) {
                const size_t c = (size_t)a * Gc + g, m = (size_t)g * Gc + a;   // (m: the mirror cell of the square)
                dst_group_cell &out = cells[c];
                __int128 S = (__int128)(((unsigned __int128)high[c] << 64) | low[c]);
                uint64_t n_links = links[c], n_summ = summ[c], n_nan = nan[c], lo_key = kmin[c], hi_key = kmax[c];
                if (square && a == g) {
                    // the fold met every pair of the diagonal cell from both of its records
                    if (n_links % 2 || n_summ % 2 || S % 2)
                        return fail(ctx, DST_ERR_STATE, "group summary: internal error, the two sides of the square disagree");
                    n_links /= 2, n_summ /= 2, S /= 2;
                } else if (square) {
                    // the row pass met a pair as (group of i, group of j), i < j: either order may hold it
                    n_nan += nan[m];
                    lo_key = std::min(lo_key, kmin[m]);
                    hi_key = std::max(hi_key, kmax[m]);
                }
                if (n_nan + n_summ > out.pairs || n_links > out.pairs)
                    return fail(ctx, DST_ERR_STATE, "group summary: internal error, a cell counts more than its pairs");
                out.nan_pairs = n_nan;
                out.summable_pairs = n_summ;
                out.links = n_links;
                out.sum = summary_value(S, int_payload);
                if (out.pairs > n_nan) {
                    out.min_bits = payload_of_key(lo_key, int_payload);
                    out.max_bits = payload_of_key(hi_key, int_payload);
                }
            }
    }
    for (uint64_t e = 0; per_record && e < n_rows * Gc; ++e) {
        if (rec_within)
            rec_within[e] = (uint32_t)(h.counts[e] >> 32);
        if (rec_summable)
            rec_summable[e] = (uint32_t)h.counts[e];
        if (rec_sum)
            rec_sum[e] = summary_value((__int128)h.hi[e] * ((__int128)1 << 32) + (__int128)h.lo[e], int_payload);
    }
    return DST_OK;
}

int dst_mst(dst_ctx *ctx, int measure, uint64_t max_pairs, uint32_t *edge_i, uint32_t *edge_j, void *values,
            uint32_t *tallies, size_t cap, uint64_t *n_edges, uint32_t *rounds)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (n_edges)
        *n_edges = 0;
    if (rounds)
        *rounds = 0;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (!edge_i || !edge_j)
        return fail(ctx, DST_ERR_ARG, "null edge_i or edge_j pointer");
    DeviceSet &set = ctx->set[0];
    if (!set.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    const uint64_t n = set.n;
    if (n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    if (n < 2)
        return DST_OK;
    if (cap < n - 1)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below n - 1 entries");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const bool finish = values || tallies;
    const int W = tally_width(measure);
    int rc = DST_OK;
    if (finish && measure == DST_TN93) {
        rc = need_counts(ctx, set, stream);
        if (rc)
            return rc;
    }
    const SlabPlan plan = plan_slabs(true, n, n, max_pairs, kClusterSlabPairs);
    MstBuffers b{};
    // the scratch holds a slab of payloads in the rounds and, for the finish, the same slab as tallies
    rc = slab_scratch(ctx, std::max(dst_out_bytes(measure, DST_OUT_DISTANCE, plan.biggest),
                                    finish ? dst_out_bytes(measure, DST_OUT_TALLY, plan.biggest) : (size_t)0));
    if (!rc)
        rc = ctx->mst_work.grow(ctx, mst_layout(nullptr, n, W, b));
    if (rc)
        return rc;
    mst_layout(ctx->mst_work, n, W, b);
    // Boruvka rounds: a round that emits nothing ends the call (the forest of a graph that is not connected); n - 1
    // edges end it without that last sweep.  Every round at least halves the components that still have an edge out.
    uint64_t h_count[2] = {0, 0};
    uint32_t n_rounds = 0;
    for (bool first = true;; first = false) {
        if (n_rounds > 64)
            return fail(ctx, DST_ERR_STATE, "minimum spanning tree: more rounds than any set can need");
        HIP_TRY(ctx, launch_mst_reset(b, n, first, stream));
        // the slab's DST_OUT_DISTANCE payloads, the two scan launches behind it
        rc = walk_slabs(ctx, measure, true, set, set, plan.slabs, DST_OUT_DISTANCE, [&](const RowSlab &s) -> int {
            HIP_TRY(ctx, launch_mst_scan(measure, static_cast<const uint64_t *>(ctx->pair_slab.ptr), s.first, n, s.rb, s.re, b, stream));
            return DST_OK;
        });
        if (rc)
            return rc;
        HIP_TRY(ctx, launch_mst_hook(b, n, stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_count, b.counters, 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        if (h_count[1] == 0)
            break;
        ++n_rounds;
        if (h_count[0] >= n - 1)
            break;
    }
    const uint64_t ne = h_count[0];
    if (ne > n - 1)
        return fail(ctx, DST_ERR_STATE, "minimum spanning tree: more than n - 1 edges");
    if (finish && ne) {
        rc = walk_slabs(ctx, measure, true, set, set, plan.slabs, DST_OUT_TALLY, [&](const RowSlab &s) -> int {
            HIP_TRY(ctx, launch_mst_gather(measure, static_cast<const uint32_t *>(ctx->pair_slab.ptr), s.first, n, s.rb, s.re,
                                           set.counts, b, ne, stream));
            return DST_OK;
        });
        if (rc)
            return rc;
    }
    // the edges back once, sorted here by (key, i, j)
    std::vector<uint64_t> h_edges(ne), h_keys(ne), h_val(finish ? ne : 0);
    std::vector<uint32_t> h_tal(tallies ? ne * W : 0), order(ne);
    if (ne) {
        HIP_TRY(ctx, hipMemcpyAsync(h_edges.data(), b.edges, ne * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_keys.data(), b.edge_keys, ne * 8, hipMemcpyDeviceToHost, stream));
        if (finish)
            HIP_TRY(ctx, hipMemcpyAsync(h_val.data(), b.val, ne * 8, hipMemcpyDeviceToHost, stream));
        if (tallies)
            HIP_TRY(ctx, hipMemcpyAsync(h_tal.data(), b.tal, ne * W * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    }
    for (uint64_t e = 0; e < ne; ++e)
        order[e] = (uint32_t)e;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return h_keys[x] != h_keys[y] ? h_keys[x] < h_keys[y] : h_edges[x] < h_edges[y];
    });
    for (uint64_t e = 0; e < ne; ++e) {
        const uint32_t src = order[e];
        edge_i[e] = (uint32_t)(h_edges[src] >> 32);
        edge_j[e] = (uint32_t)h_edges[src];
        if (values)
            static_cast<uint64_t *>(values)[e] = h_val[src];
        if (tallies)
            std::memcpy(tallies + e * W, h_tal.data() + (size_t)src * W, (size_t)W * 4);
    }
    if (n_edges)
        *n_edges = ne;
    if (rounds)
        *rounds = n_rounds;
    return DST_OK;
}

int dst_nj(dst_ctx *ctx, int measure, uint64_t max_pairs, uint32_t *parent, double *length, size_t cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    DeviceSet &set = ctx->set[0];
    if (!set.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    const uint64_t n = set.n;
    if (int rc = nj_check_out(ctx, n, parent, length, cap))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SlabPlan plan;
    int rc = square_slabs(ctx, measure, n, max_pairs, plan);
    if (rc)
        return rc;
    SquareAlloc al(ctx);
    if ((rc = al.setup(n)) || (rc = square_fill(ctx, measure, set, plan, al)) || (rc = square_check(ctx, al, n)))
        return rc;
    return nj_finish(ctx, al, n, parent, length);
}

int dst_nj_bootstrap(dst_ctx *ctx, int measure, const uint8_t *codes, size_t n, size_t len, size_t row_stride,
                     uint32_t replicates, uint64_t seed, uint64_t max_pairs, const uint32_t *parent, uint32_t *support,
                     uint32_t *rep_parent, size_t cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (!parent || !support)
        return fail(ctx, DST_ERR_ARG, "null parent or support pointer");
    if ((len && !codes) || row_stride < len)
        return fail(ctx, DST_ERR_ARG, "null codes or row_stride < len");
    if (n < 3)
        return fail(ctx, DST_ERR_ARG, "neighbour joining needs at least 3 records");
    if (n >= ((uint64_t)1 << 31) || len >= 0xFFFFFF00ull)
        return fail(ctx, DST_ERR_ARG, "bootstrap: n must be below 2^31 and len must fit 32 bits");
    if (replicates < 1 || replicates > 10000)
        return fail(ctx, DST_ERR_ARG, "bootstrap: replicates must be in 1..=10000");
    const uint64_t N = 2 * n - 2;
    if (cap < N)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below 2n - 2 entries");
    SplitCounter splits;
    if (!splits.init(n, parent))
        return fail(ctx, DST_ERR_ARG, "bootstrap: the main tree is not a dst_nj tree on n leaves");
    std::vector<uint32_t> count(N, 0), rp(N);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    SlabPlan plan;
    int rc = square_slabs(ctx, measure, n, max_pairs, plan);
    if (rc)
        return rc;
    const uint64_t pitch = std::max<uint64_t>((len + 127) / 128 * 128, 128);
    SquareAlloc al(ctx);   // (destroyed after `boot`: the replicate set is freed first, then the square)
    BootAlloc boot(ctx);
    if ((rc = boot.setup(n, pitch, len)) || (rc = al.setup(n)))
        return rc;
    if (len)
        HIP_TRY(ctx, hipMemcpy2DAsync(boot.src, pitch, codes, row_stride, len, n, hipMemcpyHostToDevice, stream));
    // the original once through the pack: every byte is checked, as dst_upload checks it (a replicate draws a subset)
    if ((rc = pack_set(ctx, ctx->boot, boot.src, n, len, pitch, nullptr, stream)))
        return rc;
    for (uint32_t r = 0; r < replicates; ++r) {
        HIP_TRY(ctx, launch_boot_resample(boot.src, pitch, boot.rep, n, len, seed, r, boot.map, stream));
        // tn93: no counts passed, so the pair kernels count the replicate's bases by code (need_counts)
        if ((rc = pack_set(ctx, ctx->boot, boot.rep, n, len, pitch, nullptr, stream)))
            return rc;
        if ((rc = square_fill(ctx, measure, ctx->boot, plan, al)))
            return rc;
        // the rounds run whatever the flag says (their indices stay in range on non-finite values), so the flag comes
        // back with the tree instead of through square_check: one wait per tree
        unsigned long long bad = 0;
        uint32_t *dst = rep_parent ? rep_parent + (uint64_t)r * N : rp.data();
        HIP_TRY(ctx, launch_nj_rounds(al.b, n, stream));
        HIP_TRY(ctx, hipMemcpyAsync(dst, al.b.parent, N * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipMemcpyAsync(&bad, al.bad, 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        if (bad != ~0ull)
            return square_bad_pair(ctx, "bootstrap replicate " + std::to_string(r) + ": ", bad, n);
        if (!splits.count(dst, count.data()))
            return fail(ctx, DST_ERR_STATE, "bootstrap replicate " + std::to_string(r) + ": malformed replicate tree");
    }
    for (uint64_t x = 0; x < N; ++x)
        support[x] = x < n || parent[x] == 0xFFFFFFFFu ? 0xFFFFFFFFu : count[x];
    return DST_OK;
}

int dst_nj_matrix(dst_ctx *ctx, const double *d, uint64_t n, uint32_t *parent, double *length, size_t cap)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (!d)
        return fail(ctx, DST_ERR_ARG, "null matrix pointer");
    int rc;
    if ((rc = nj_check_out(ctx, n, parent, length, cap)) || (rc = matrix_finite(ctx, "neighbour joining: ", d, n)))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    SquareAlloc al(ctx);
    if ((rc = al.setup(n)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(al.b.D[0], d, n * n * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, launch_nj_init(al.b.D[0], n, al.b.ids[0], al.b.active, al.bad, stream));
    HIP_TRY(ctx, launch_nj_mirror(al.b.D[0], n, stream));
    return nj_finish(ctx, al, n, parent, length);
}

int dst_dendrogram(dst_ctx *ctx, int measure, int linkage, uint64_t max_pairs, uint32_t *parent, double *length,
                   double *height, size_t cap, uint64_t *row_scans)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    DeviceSet &set = ctx->set[0];
    if (!set.loaded)
        return fail(ctx, DST_ERR_STATE, "set not uploaded");
    const uint64_t n = set.n;
    if (int rc = dg_check(ctx, n, linkage, parent, length, cap))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SlabPlan plan;
    int rc = square_slabs(ctx, measure, n, max_pairs, plan);
    if (rc)
        return rc;
    SquareAlloc al(ctx, "dendrogram");
    DgBuffers b{};
    if ((rc = al.setup(n, false)) || (rc = dg_buffers(ctx, al, n, b)) || (rc = square_fill(ctx, measure, set, plan, al)) ||
        (rc = square_check(ctx, al, n)))
        return rc;
    return dg_finish(ctx, b, n, linkage, parent, length, height, row_scans);
}

int dst_dendrogram_matrix(dst_ctx *ctx, const double *d, uint64_t n, int linkage, uint32_t *parent, double *length,
                          double *height, size_t cap, uint64_t *row_scans)
{
    if (!ctx)
        return DST_ERR_ARG;
    if (!d)
        return fail(ctx, DST_ERR_ARG, "null matrix pointer");
    int rc;
    if ((rc = dg_check(ctx, n, linkage, parent, length, cap)) || (rc = matrix_finite(ctx, "dendrogram: ", d, n)))
        return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    SquareAlloc al(ctx, "dendrogram");
    DgBuffers b{};
    if ((rc = al.setup(n, false)) || (rc = dg_buffers(ctx, al, n, b)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(b.D, d, n * n * 8, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, launch_nj_init(b.D, n, b.node, b.active, al.bad, stream));
    HIP_TRY(ctx, launch_nj_mirror(b.D, n, stream));
    return dg_finish(ctx, b, n, linkage, parent, length, height, row_scans);
}

}  // extern "C"
