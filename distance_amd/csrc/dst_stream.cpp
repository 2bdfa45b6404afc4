// dst_stream.cpp — stream mode behind the C ABI: batches of streamed records against the loaded set of
// slot 0 (stream(), src/lib.rs:269-365; the batches are stream_fasta()'s, src/fastaio.rs:215-286).
//
// A ring of `depth` slots, each with its own page-locked input buffer, device byte buffer, packed planes,
// device result buffer and page-locked result buffer, and three HIP streams:
//
//     copy-in   H2D of batch k+1                       |  while
//     compute   pack + pair kernel of batch k          |  all three
//     copy-out  D2H of batch k-1's results             |  run
//
// The caller encodes straight into the page-locked buffer (dst_stream_acquire), submits, and collects
// results strictly in submission order.  The byte staging of a slot is reused by the next batch that gets
// the slot; nothing is kept for the life of the context.
//
// A closest stream (dst_stream_open_closest) is the same ring, but the batch's result matrix stays on the
// device as DST_OUT_TALLY words and a selection launch behind the pair kernel keeps the k smallest per record:
//   DST_CLOSEST_FOR_LOADED    one set of lists for the loaded records, alive from open to close; every batch's column
//                             pass (nearest_stream_cols_kernel) runs on the compute stream, so the launches follow one
//                             another; only the bad-code word travels back per batch
//   DST_CLOSEST_FOR_STREAMED  per-slot lists for the batch's records (nearest_init + nearest_rows, rectangle form); their
//                             D2H takes the place of the results' on the copy-out stream
//
// A links stream (dst_stream_open_links) is the third kind: the matrix stays on the device (DST_OUT_TALLY words
// when the links' tallies are asked for, else DST_OUT_DISTANCE payloads) and dst_links' count, scan and write launches
// (rectangle form, the batch as rows) follow the pair kernel on the compute stream.  Every slot has its own block counts,
// offsets and window, two batches being on the device at once.  The write pass stores window 0 straight into the slot's
// page-locked window through its device address, and a one-thread launch puts the batch's total beside the bad-code word,
// so that the copy-out stream carries 16 bytes per batch.  (DST_STREAM_LINKS_COPY, a measurement knob: the window in device
// memory, its present entries copied after collect.)
//
// A window-closest stream (dst_stream_open_window_closest) is the fourth: per (loaded record, window) the k
// nearest streamed records.  No plain pair kernel and no matrix: behind the pack, on the compute stream, come the batch's
// per-window base counts (tn93), then per (rows x windows) range the window sweep of loaded x batch as DST_OUT_TALLY words
// into the stream's one scratch and window_nearest_stream_kernel's merge into the lists.  The window table, the count
// tables, the scratch and the lists are the stream's own, so no other call on the context can disturb them.
//
// A summary stream (dst_stream_open_summary) is the fifth: dst_summary's counts and exact sums of the
// batch's DST_OUT_DISTANCE matrix, which stays in the slot's d_out.  Behind the pair kernel, on the compute stream, one
// tile pass (summary_stream_kernel) reads every entry once for both sides: the loaded records' words and the totals are
// the stream's own kept state, zeroed at open; the batch's records' words are the slot's, zeroed in front of the kernel,
// copied to the slot's page-locked block on the copy-out stream and converted at collect.  With bins, dst_summary's
// histogram pass follows into the kept histogram, with totals of its own that the result compares with the tile pass'.
//
// A group-summary stream (dst_stream_open_group_summary) is the sixth: dst_group_summary on the rectangle
// (every record so far) x (the loaded set).  The batch's labels travel in the slot's page-locked label block, with the
// batch's assigned records in order of their group behind them (a counting sort at submit).  Behind the pair kernel, on the
// compute stream: dst_group_summary's row pass into the slot's table (zeroed in front of it) and the kept cells' NaN / min /
// max, its fold of that table into the kept cells' links / summable / 128-bit sum, and with LOADED group_stream_cols_kernel
// into the kept table of the loaded records (group-major on the device, transposed by the result call).  The kept state is the stream's own, zeroed once at open.
#include <algorithm>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "dst_ctx.h"

using namespace dst;

struct dst_stream {
    dst_ctx *ctx = nullptr;
    int measure = 0, out_kind = 0, wire = DST_WIRE_CODES;
    size_t max_records = 0, len = 0, pitch = 0;
    size_t out_bytes_per_record = 0;
    struct Slot {
        // the slot's buffers (and its set's) go with the slot: dst_stream_close, or an open that fails
        Grown<uint8_t, true> h_in;   // max_records x pitch codes, then max_records x 4 base counts
        Grown<uint8_t> d_in;
        Grown<> d_out;
        Grown<void, true> h_out;
        Grown<> d_lists;             // FOR_STREAMED: max_records x k_streamed entries, device and page-locked
        Grown<void, true> h_lists;
        NearestLists nl{}, h_nl{};
        // a links stream: d_lists = block counts, offsets, header (and the window, copy route), h_lists = header and window
        LinksBuffers lb{}, h_lb{};           // lb: what the kernels write (its window: h_lb's by device address, or d_lists')
        LinksBuffers d_win{};                // copy route: the window in device memory (= lb's)
        uint64_t *d_hdr = nullptr, *h_hdr = nullptr;   // [0] the batch's links, [1] its bad-code word
        uint64_t total = 0;                  // of the collected batch
        uint64_t window_first = ~0ull;       // the first link of the window the page-locked buffer holds (~0: none)
        Grown<unsigned long long> d_bad;
        Grown<unsigned long long, true> h_bad;
        // a group-summary stream: max_records labels, then the batch's assigned records in order of their group;
        // d_lists = the batch's table (counts, hi, lo planes), h_lists = the same and the split counts behind them
        Grown<uint32_t, true> h_labels;
        Grown<uint32_t> d_labels;
        uint64_t assigned = 0;               // of the submitted batch
        DeviceSet set;
        Event h2d, computed, landed;   // (made by their first record, in the slot's first submit)
        size_t n = 0;
        int state = 0;  // 0 free, 1 acquired, 2 submitted, 3 collected (results still readable)
    };
    std::vector<Slot> slots;
    hipStream_t s_in = nullptr, s_compute = nullptr, s_out = nullptr;
    size_t next_acquire = 0, next_collect = 0, in_flight = 0;
    int acquired = -1;
    // closest streams (closest = the dst_closest_side, -1: a plain stream, kLinksStream: a links stream)
    int closest = -1;
    uint32_t k = 0, k_streamed = 0;   // asked for; min(k, n_loaded): what a FOR_STREAMED batch's lists hold
    size_t n_loaded = 0;
    int W = 0;
    Grown<> d_lists;                  // FOR_LOADED: n_loaded x k values, indices and W tallies
    NearestLists nl{};
    uint64_t next_ordinal = 0, submitted = 0;
    bool poisoned = false;            // a batch held an invalid code: the lists are not trustworthy
    int last_collected = -1;          // FOR_STREAMED, links: the slot dst_stream_closest_batch / _links_batch hands out
    // links streams
    uint64_t t_bits = 0;              // the threshold as a payload (threshold_payload)
    bool any_links = false;           // false: nothing can link, no compaction is launched
    int what = 0;
    uint64_t window = 0;              // links of one window
    bool via_copy = false;            // DST_STREAM_LINKS_COPY
    uint64_t links_total = 0, late_windows = 0;   // dst_stream_links_stats
    // window-closest streams: n_loaded x n_windows lists in d_lists (nl, and wc_cnt: tn93's 4 count words per entry)
    uint32_t n_windows = 0;
    Grown<uint2> wc_table;            // [n_windows] {begin, end}
    Grown<uint4> wc_q_counts;         // tn93: [n_windows][n_loaded], built at open
    Grown<uint4> wc_t_counts;         // tn93: [n_windows][the batch's records], rebuilt per batch
    Grown<uint32_t> wc_scratch;       // one range's tallies: wc_cut.rows x wc_cut.wins x max_records entries
    WindowSlabs wc_cut{};
    uint32_t *wc_cnt = nullptr;
    // summary streams (what, t_bits, any_links as a links stream's; submitted: the records so far).  The kept state in
    // d_lists: the loaded records' four words (LOADED), the histogram, the tile kernel's totals and the histogram pass'
    uint32_t bins = 0;
    uint64_t width_q = 0;
    size_t sum_state_bytes = 0;
    SummaryBuffers sum_kept{};        // within / summable / hi / lo: NULL without LOADED; hist; tot: the tile kernel's
    SummaryBuffers sum_hist{};        // hist: sum_kept's; tot: the histogram pass' own
    // group-summary streams (what, t_bits, any_links, submitted as a summary stream's).  The kept state in d_lists: the
    // loaded labels, the cells, the loaded records' table (LOADED)
    uint32_t g_loaded = 0, g_streamed = 0;
    GroupBuffers grp_kept{};          // col_group: the loaded labels; cell; counts / hi / lo: [g_streamed][n_loaded] or NULL
    size_t grp_state_bytes = 0, grp_cells_at = 0;
    std::vector<uint64_t> loaded_size, streamed_size;   // records per group, the streamed side's so far
    uint64_t loaded_assigned = 0;
};

constexpr int kLinksStream = 2;       // dst_stream::closest of a links stream (after the two dst_closest_side values)
constexpr int kWindowClosestStream = 3;   // ... and of a window-closest stream
constexpr int kSummaryStream = 4;     // ... and of a summary stream
constexpr int kGroupSummaryStream = 5;   // ... and of a group-summary stream

namespace {

size_t counts_offset(const dst_stream *s) { return s->max_records * s->pitch; }

// the three arrays of `entries` list entries in one block: values (8 B), indices (4 B), W tally words
size_t lists_layout(void *base, uint64_t entries, int W, NearestLists &nl)
{
    if (base) {
        char *p = static_cast<char *>(base);
        nl.val = reinterpret_cast<uint64_t *>(p);
        nl.idx = reinterpret_cast<uint32_t *>(p + entries * 8);
        nl.tal = reinterpret_cast<uint32_t *>(p + entries * 12);
    }
    return (size_t)(entries * (12 + 4 * (uint64_t)W));   // (the size alone with base == NULL)
}

// one window of links in one block: streamed (row), loaded (col), values when asked, W tally words (0: none) per link
size_t window_layout(void *base, uint64_t window, bool values, int W, LinksBuffers &b)
{
    char *p = static_cast<char *>(base);
    size_t used = 0;
    auto take = [&](size_t bytes) {
        char *at = p ? p + used : nullptr;
        used += (bytes + 255) / 256 * 256;
        return at;
    };
    b.row = reinterpret_cast<uint32_t *>(take(window * 4));
    b.col = reinterpret_cast<uint32_t *>(take(window * 4));
    b.val = reinterpret_cast<uint64_t *>(take(values ? window * 8 : 0));
    b.tal = reinterpret_cast<uint32_t *>(take(window * 4 * (size_t)W));
    return used;   // (the size alone with base == NULL)
}

// a summary stream's four words of `records` records in one block of 24 bytes per record: hi, lo, within, summable
size_t records_layout(void *base, uint64_t records, SummaryBuffers &b)
{
    if (base) {
        char *p = static_cast<char *>(base);
        b.hi = reinterpret_cast<int64_t *>(p);
        b.lo = reinterpret_cast<uint64_t *>(p + records * 8);
        b.within = reinterpret_cast<uint32_t *>(p + records * 16);
        b.summable = reinterpret_cast<uint32_t *>(p + records * 20);
    }
    return (size_t)(records * 24);   // (the size alone with base == NULL)
}

// ... and its kept state: the loaded records' words (LOADED), the histogram, the tile kernel's totals, the histogram pass'
size_t summary_state_layout(void *base, uint64_t n_loaded, bool loaded, uint32_t bins, SummaryBuffers &kept, SummaryBuffers &hist)
{
    const size_t records = loaded ? records_layout(base, n_loaded, kept) : 0;   // (a multiple of 8 bytes)
    if (base) {
        uint64_t *p = reinterpret_cast<uint64_t *>(static_cast<char *>(base) + records);
        kept.hist = hist.hist = p;
        kept.tot = p + bins;
        hist.tot = p + bins + kSummaryTotals;
    }
    return records + ((size_t)bins + 2 * kSummaryTotals) * 8;
}

// a group-summary stream's table of `entries` (record, group) entries in one block of 24 bytes per entry: counts, hi, lo
size_t table_layout(void *base, uint64_t entries, GroupBuffers &b)
{
    if (base) {
        char *p = static_cast<char *>(base);
        b.counts = reinterpret_cast<uint64_t *>(p);
        b.hi = reinterpret_cast<int64_t *>(p + entries * 8);
        b.lo = reinterpret_cast<uint64_t *>(p + entries * 16);
    }
    return (size_t)(entries * 24);   // (the size alone with base == NULL)
}

// ... and its kept state: the loaded labels, the cells' planes from cells_at, the loaded records' table (LOADED)
size_t group_state_layout(void *base, uint64_t n_loaded, uint64_t cells, uint64_t table_entries, GroupBuffers &b, size_t &cells_at)
{
    cells_at = (size_t)((n_loaded * 4 + 255) / 256 * 256);
    const size_t cell_bytes = (size_t)(cells * kGroupCellWords * 8);
    if (base) {
        char *p = static_cast<char *>(base);
        b.col_group = reinterpret_cast<uint32_t *>(p);
        b.cell = reinterpret_cast<uint64_t *>(p + cells_at);
    }
    return cells_at + cell_bytes + table_layout(base ? static_cast<char *>(base) + cells_at + cell_bytes : nullptr, table_entries, b);
}

void destroy(dst_stream *s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->ctx->device);
    for (hipStream_t st : {s->s_in, s->s_compute, s->s_out})
        if (st)
            (void)hipStreamSynchronize(st);
    // The context keeps marks of these streams: events of its own, recorded on them.  The streams are idle now, so those
    // events have completed, and the marks go before the streams do: the runtime must not be asked about an event whose
    // stream is gone (forget_stream).
    for (hipStream_t st : {s->s_in, s->s_compute, s->s_out})
        if (st)
            forget_stream(s->ctx, st);
    s->slots.clear();   // the slots' memory, device and page-locked, their sets' and their events
    (void)s->d_lists.release();
    (void)s->wc_scratch.release();   // (a window-closest stream's)
    (void)s->wc_t_counts.release();
    (void)s->wc_q_counts.release();
    (void)s->wc_table.release();
    for (hipStream_t st : {s->s_in, s->s_compute, s->s_out})
        if (st)
            (void)hipStreamDestroy(st);
    delete s;
}

int open_stream(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, int wire, int closest, uint32_t k,
                dst_stream **out);

// the copy route of a links stream: the first m entries of the slot's device window into its page-locked one; waits
int copy_window(dst_stream *s, dst_stream::Slot &sl, uint64_t m, hipStream_t stream)
{
    dst_ctx *ctx = s->ctx;
    HIP_TRY(ctx, hipMemcpyAsync(sl.h_lb.row, sl.d_win.row, m * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipMemcpyAsync(sl.h_lb.col, sl.d_win.col, m * 4, hipMemcpyDeviceToHost, stream));
    if (s->what & DST_LINKS_VALUES)
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_lb.val, sl.d_win.val, m * 8, hipMemcpyDeviceToHost, stream));
    if (s->what & DST_LINKS_TALLIES)
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_lb.tal, sl.d_win.tal, m * 4 * (size_t)s->W, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return DST_OK;
}

}  // namespace

extern "C" {

int dst_stream_open(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, dst_stream **out)
{
    return dst_stream_open_wire(ctx, measure, out_kind, max_records, depth, DST_WIRE_CODES, out);
}

int dst_stream_open_wire(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, int wire, dst_stream **out)
{
    return open_stream(ctx, measure, out_kind, max_records, depth, wire, -1, 0, out);
}

int dst_stream_open_closest(dst_ctx *ctx, int measure, uint32_t k, int side, size_t max_records, int depth, int wire,
                            dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (side != DST_CLOSEST_FOR_LOADED && side != DST_CLOSEST_FOR_STREAMED)
        return fail(ctx, DST_ERR_ARG, "unknown side: DST_CLOSEST_FOR_LOADED or DST_CLOSEST_FOR_STREAMED");
    if (k < 1 || k > kNearestMaxK)
        return fail(ctx, DST_ERR_ARG, "k must be between 1 and 256");
    return open_stream(ctx, measure, DST_OUT_TALLY, max_records, depth, wire, side, k, out);
}

int dst_stream_open_links(dst_ctx *ctx, int measure, double threshold, int what, uint64_t window_links, size_t max_records,
                          int depth, int wire, dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (what & ~(DST_LINKS_VALUES | DST_LINKS_TALLIES))
        return fail(ctx, DST_ERR_ARG, "unknown bits in what");
    if (window_links > DST_LINKS_CHUNK)
        return fail(ctx, DST_ERR_ARG, "window_links is above DST_LINKS_CHUNK");
    dst_stream *s = nullptr;
    const bool tallies = (what & DST_LINKS_TALLIES) != 0, values = (what & DST_LINKS_VALUES) != 0;
    int rc = open_stream(ctx, measure, tallies ? DST_OUT_TALLY : DST_OUT_DISTANCE, max_records, depth, wire, kLinksStream, 0, &s);
    if (rc)
        return rc;
    s->what = what;
    s->any_links = threshold_payload(measure, threshold, s->t_bits) && s->n_loaded != 0;
    const uint64_t n_loaded = s->n_loaded;
    const uint64_t most = n_loaded && max_records > ~0ull / n_loaded ? ~0ull : (uint64_t)max_records * n_loaded;
    s->window = std::min<uint64_t>(std::max<uint64_t>(std::min<uint64_t>(window_links ? window_links : DST_STREAM_LINKS_WINDOW, most), 1),
                                   DST_LINKS_CHUNK);
    s->via_copy = std::getenv("DST_STREAM_LINKS_COPY") != nullptr;   // measurement knob
    // per slot: the block counts, their offsets, the scan's running total and the header; the window
    const uint64_t blocks = links_blocks(false, n_loaded, 0, max_records);
    const int W = tallies ? s->W : 0;
    LinksBuffers none{};
    const size_t win_bytes = window_layout(nullptr, s->window, values, W, none);
    const size_t counts_bytes = (blocks * 4 + 255) / 256 * 256, offsets_bytes = ((blocks + 1) * 8 + 255) / 256 * 256;
    const size_t work_bytes = counts_bytes + offsets_bytes + 256;
    hipError_t e = hipSuccess;
    for (auto &sl : s->slots) {
        if (e != hipSuccess)
            break;
        rc = sl.d_lists.grow(ctx, work_bytes + (s->via_copy ? win_bytes : 0));
        if (!rc)
            rc = sl.h_lists.grow(ctx, 256 + win_bytes);
        if (rc)
            break;
        char *d = static_cast<char *>(sl.d_lists.ptr), *h = static_cast<char *>(sl.h_lists.ptr);
        sl.lb.counts = reinterpret_cast<uint32_t *>(d);
        sl.lb.offsets = reinterpret_cast<uint64_t *>(d + counts_bytes);
        sl.lb.grand = reinterpret_cast<uint64_t *>(d + counts_bytes + offsets_bytes);
        sl.d_hdr = sl.lb.grand + 2;
        sl.h_hdr = reinterpret_cast<uint64_t *>(h);
        window_layout(h + 256, s->window, values, W, sl.h_lb);
        if (s->via_copy) {
            window_layout(d + work_bytes, s->window, values, W, sl.d_win);
        } else {   // the kernels' view of the page-locked window
            void *h_dev = nullptr;
            e = hipHostGetDevicePointer(&h_dev, sl.h_lists, 0);
            if (e == hipSuccess)
                window_layout(static_cast<char *>(h_dev) + 256, s->window, values, W, sl.d_win);
        }
        sl.lb.row = sl.d_win.row, sl.lb.col = sl.d_win.col, sl.lb.val = sl.d_win.val, sl.lb.tal = sl.d_win.tal;
        if (e == hipSuccess) e = hipMemsetAsync(sl.lb.grand, 0, 8, s->s_compute);
    }
    if (rc || e != hipSuccess) {
        destroy(s);
        return rc ? rc : fail_hip(ctx, e, "dst_stream_open_links");
    }
    *out = s;
    return DST_OK;
}

int dst_stream_open_summary(dst_ctx *ctx, int measure, double threshold, int what, uint32_t bins, double width,
                            size_t max_records, int depth, int wire, dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (wire != DST_WIRE_CODES && wire != DST_WIRE_NIBBLES)
        return fail(ctx, DST_ERR_ARG, "unknown wire format");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (what & ~(DST_STREAM_SUMMARY_LOADED | DST_STREAM_SUMMARY_STREAMED))
        return fail(ctx, DST_ERR_ARG, "unknown bits in what");
    uint64_t width_q = 0;
    if (bins) {
        if (bins > DST_SUMMARY_MAX_BINS)
            return fail(ctx, DST_ERR_ARG, "bins must be between 0 and 4096");
        if (int rc = summary_width_q(ctx, measure, width, width_q))
            return rc;
    }
    dst_stream *s = nullptr;
    int rc = open_stream(ctx, measure, DST_OUT_DISTANCE, max_records, depth, wire, kSummaryStream, 0, &s);
    if (rc)
        return rc;
    s->what = what;
    s->bins = bins;
    s->width_q = width_q;
    s->any_links = threshold_payload(measure, threshold, s->t_bits);
    const bool loaded = (what & DST_STREAM_SUMMARY_LOADED) != 0, streamed = (what & DST_STREAM_SUMMARY_STREAMED) != 0;
    const char *const name = "summary stream";
    // the kept state, zeroed once; per slot the batch's records' words, device and page-locked
    s->sum_state_bytes = summary_state_layout(nullptr, s->n_loaded, loaded, bins, s->sum_kept, s->sum_hist);
    rc = s->d_lists.grow(ctx, s->sum_state_bytes, name);
    SummaryBuffers none{};
    const size_t batch_bytes = records_layout(nullptr, max_records, none);
    for (auto &sl : s->slots) {
        if (!rc && streamed)
            rc = sl.d_lists.grow(ctx, batch_bytes, name);
        if (!rc && streamed)
            rc = sl.h_lists.grow(ctx, batch_bytes, name);
    }
    hipError_t e = hipSuccess;
    if (!rc) {
        summary_state_layout(s->d_lists, s->n_loaded, loaded, bins, s->sum_kept, s->sum_hist);
        e = hipMemsetAsync(s->d_lists, 0, s->sum_state_bytes, s->s_compute);
    }
    if (rc || e != hipSuccess) {
        destroy(s);
        return rc ? rc : fail_hip(ctx, e, "dst_stream_open_summary");
    }
    *out = s;
    return DST_OK;
}

int dst_stream_open_group_summary(dst_ctx *ctx, int measure, double threshold, int what, const uint32_t *loaded_group,
                                  uint32_t n_loaded_groups, uint32_t n_streamed_groups, size_t max_records, int depth, int wire,
                                  dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (wire != DST_WIRE_CODES && wire != DST_WIRE_NIBBLES)
        return fail(ctx, DST_ERR_ARG, "unknown wire format");
    if (std::isnan(threshold))
        return fail(ctx, DST_ERR_ARG, "threshold is NaN");
    if (what & ~(DST_STREAM_GROUPS_LOADED | DST_STREAM_GROUPS_STREAMED))
        return fail(ctx, DST_ERR_ARG, "unknown bits in what");
    if (n_loaded_groups == 0 || n_loaded_groups > DST_GROUPS_MAX || n_streamed_groups == 0 || n_streamed_groups > DST_GROUPS_MAX)
        return fail(ctx, DST_ERR_ARG, "a group count must be between 1 and " + std::to_string(DST_GROUPS_MAX));
    if (!loaded_group && n_loaded_groups != 1)
        return fail(ctx, DST_ERR_ARG, "a null loaded_group puts every loaded record in group 0: n_loaded_groups must be 1");
    dst_stream *s = nullptr;
    int rc = open_stream(ctx, measure, DST_OUT_DISTANCE, max_records, depth, wire, kGroupSummaryStream, 0, &s);
    if (rc)
        return rc;
    const uint64_t n_loaded = s->n_loaded;
    const uint32_t Gl = n_loaded_groups, Gs = n_streamed_groups;
    if (loaded_group) {
        rc = group_labels(ctx, loaded_group, n_loaded, Gl, "loaded", s->loaded_size);
        if (rc) {
            destroy(s);
            return rc;
        }
    } else
        s->loaded_size.assign(1, n_loaded);
    for (uint64_t size : s->loaded_size)
        s->loaded_assigned += size;
    s->streamed_size.assign(Gs, 0);
    s->what = what;
    s->g_loaded = Gl;
    s->g_streamed = Gs;
    s->any_links = threshold_payload(measure, threshold, s->t_bits);
    const bool loaded = (what & DST_STREAM_GROUPS_LOADED) != 0, streamed = (what & DST_STREAM_GROUPS_STREAMED) != 0;
    const char *const name = "group-summary stream";
    // the kept state, zeroed once; per slot the batch's labels and order, its table, and (STREAMED) the table page-locked
    const uint64_t cells = (uint64_t)Gs * Gl, kept_entries = loaded ? n_loaded * Gs : 0;
    s->grp_state_bytes = group_state_layout(nullptr, n_loaded, cells, kept_entries, s->grp_kept, s->grp_cells_at);
    rc = s->d_lists.grow(ctx, s->grp_state_bytes, name);
    const uint64_t batch_entries = (uint64_t)max_records * Gl;
    GroupBuffers none{};
    for (auto &sl : s->slots) {
        if (!rc)
            rc = sl.h_labels.grow(ctx, max_records * 8, name);
        if (!rc)
            rc = sl.d_labels.grow(ctx, max_records * 8, name);
        if (!rc)
            rc = sl.d_lists.grow(ctx, table_layout(nullptr, batch_entries, none), name);
        if (!rc && streamed)
            rc = sl.h_lists.grow(ctx, table_layout(nullptr, batch_entries, none) + (size_t)batch_entries * 8, name);
    }
    hipError_t e = hipSuccess;
    if (!rc) {
        group_state_layout(s->d_lists, n_loaded, cells, kept_entries, s->grp_kept, s->grp_cells_at);
        if (!loaded)
            s->grp_kept.counts = nullptr, s->grp_kept.hi = nullptr, s->grp_kept.lo = nullptr;
        s->grp_kept.g_rows = Gs;
        s->grp_kept.g_cols = Gl;
        e = hipMemsetAsync(s->d_lists, 0, s->grp_state_bytes, s->s_compute);
        if (e == hipSuccess) e = hipMemsetAsync(s->grp_kept.cell + 5 * cells, 0xFF, cells * 8, s->s_compute);   // (the min keys: none yet)
        if (e == hipSuccess && loaded_group && n_loaded)   // (pageable memory: the copy has read it when the call returns)
            e = hipMemcpyAsync(s->grp_kept.col_group, loaded_group, n_loaded * 4, hipMemcpyHostToDevice, s->s_compute);
        if (e == hipSuccess) e = hipStreamSynchronize(s->s_compute);
    }
    if (rc || e != hipSuccess) {
        destroy(s);
        return rc ? rc : fail_hip(ctx, e, "dst_stream_open_group_summary");
    }
    *out = s;
    return DST_OK;
}

int dst_stream_open_window_closest(dst_ctx *ctx, int measure, uint32_t k, const uint64_t *win_begin, const uint64_t *win_end,
                                   uint32_t n_windows, uint64_t max_entries, size_t max_records, int depth, int wire,
                                   dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (wire != DST_WIRE_CODES && wire != DST_WIRE_NIBBLES)
        return fail(ctx, DST_ERR_ARG, "unknown wire format");
    if (k < 1 || k > kNearestMaxK)
        return fail(ctx, DST_ERR_ARG, "k must be between 1 and 256");
    if (n_windows == 0)
        return fail(ctx, DST_ERR_ARG, "a window-closest stream needs at least one window");
    if (n_windows > DST_WINDOWS_MAX)
        return fail(ctx, DST_ERR_ARG, "more than DST_WINDOWS_MAX (65,536) windows");
    if (!win_begin || !win_end)
        return fail(ctx, DST_ERR_ARG, "null pointer");
    if (max_records == 0 || depth < 2 || depth > 16)
        return fail(ctx, DST_ERR_ARG, "max_records must be positive and depth in 2..16");
    DeviceSet &loaded = ctx->set[0];
    if (!loaded.loaded)
        return fail(ctx, DST_ERR_STATE, "upload the loaded set to slot 0 before opening a stream");
    if (loaded.partial)
        return fail(ctx, DST_ERR_STATE, "a set uploaded with dst_upload_shared runs on the consensus path only (this rank holds "
                                        "the planes of its own records)");
    if (int rc = windows_valid(ctx, win_begin, win_end, n_windows, loaded.len))
        return rc;
    if (loaded.len >= ((uint64_t)1 << 32))
        return fail(ctx, DST_ERR_ARG, "alignments of 2^32 sites or more are beyond a window-closest stream");
    if (loaded.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    const uint64_t n_lists = (uint64_t)loaded.n * n_windows;
    if (n_lists > kWindowNearestListsMax)
        return fail(ctx, DST_ERR_ARG, "more than 2^31 (loaded record, window) lists");
    // the loaded set's deferred planes, on the context's stream and waited for: the stream's kernels come later
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = order_after_prep(ctx, ctx->stream))
        return rc;
    if (int rc = ensure_derived(ctx, loaded, ctx->stream))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    dst_stream *s = nullptr;
    int rc = open_stream(ctx, measure, DST_OUT_TALLY, max_records, depth, wire, kWindowClosestStream, k, &s);
    if (rc)
        return rc;
    s->n_windows = n_windows;
    const int W = s->W;
    const bool tn93 = measure == DST_TN93;
    const char *const what = "window-closest stream";
    // the ranges of a batch: cut for a full batch, so that every batch's range fits the one scratch
    if (loaded.n)
        s->wc_cut = cut_window_slabs(loaded.n, n_windows, max_records, max_entries);
    const uint64_t scratch_entries = s->wc_cut.rows * s->wc_cut.wins * (uint64_t)max_records;
    // the lists: payloads, ordinals, tallies and (tn93) the streamed records' counts, each 256-byte aligned
    const uint64_t entries = n_lists * k;
    const auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t val_bytes = pad(entries * 8), idx_bytes = pad(entries * 4), tal_bytes = pad(entries * W * 4);
    const size_t cnt_bytes = tn93 ? pad(entries * 16) : 0;
    rc = s->wc_table.grow(ctx, (size_t)n_windows * sizeof(uint2), what);
    if (!rc)
        rc = s->d_lists.grow(ctx, std::max<size_t>(val_bytes + idx_bytes + tal_bytes + cnt_bytes, 256), what);
    if (!rc)
        rc = s->wc_scratch.grow(ctx, std::max<size_t>((size_t)scratch_entries * W * 4, 256), what);
    if (!rc && tn93)
        rc = s->wc_q_counts.grow(ctx, std::max<size_t>((size_t)n_lists * sizeof(uint4), 256), what);
    if (!rc && tn93)
        rc = s->wc_t_counts.grow(ctx, (size_t)n_windows * max_records * sizeof(uint4), what);
    hipError_t e = hipSuccess;
    if (!rc) {
        char *lists = static_cast<char *>(s->d_lists.ptr);
        s->nl.val = reinterpret_cast<uint64_t *>(lists);
        s->nl.idx = reinterpret_cast<uint32_t *>(lists + val_bytes);
        s->nl.tal = reinterpret_cast<uint32_t *>(lists + val_bytes + idx_bytes);
        s->wc_cnt = tn93 ? reinterpret_cast<uint32_t *>(lists + val_bytes + idx_bytes + tal_bytes) : nullptr;
        s->nl.k = k;
        std::vector<uint2> table(n_windows);
        for (uint32_t w = 0; w < n_windows; ++w)
            table[w] = make_uint2((uint32_t)win_begin[w], (uint32_t)win_end[w]);
        e = hipMemcpyAsync(s->wc_table, table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice, s->s_compute);
        if (e == hipSuccess) e = hipStreamSynchronize(s->s_compute);   // (the table's host copy goes with this scope)
        if (e == hipSuccess && tn93) e = launch_window_counts(loaded, s->wc_table, n_windows, s->wc_q_counts, s->s_compute);
        if (e == hipSuccess) e = launch_nearest_init(s->nl, n_lists, s->s_compute);
    }
    if (rc || e != hipSuccess) {
        destroy(s);
        return rc ? rc : fail_hip(ctx, e, "dst_stream_open_window_closest");
    }
    *out = s;
    return DST_OK;
}

}  // extern "C"

namespace {

// One batch of a window-closest stream, queued on the compute stream behind the batch's pack: the batch's per-window base
// counts (tn93), then range by range the window sweep (rows = loaded, columns = the batch, whose records the sweep's lanes
// run along) into the stream's scratch and the merge into the lists.  One scratch is enough: sweep and merge follow each
// other on the one stream.  Every list has one writer per launch.
int window_closest_batch(dst_stream *s, DeviceSet &batch, size_t n_records)
{
    dst_ctx *ctx = s->ctx;
    DeviceSet &loaded = ctx->set[0];
    hipStream_t stream = s->s_compute;
    if (s->n_loaded == 0)
        return DST_OK;
    if (int rc = order_after_prep(ctx, stream))
        return rc;
    if (int rc = ensure_derived(ctx, loaded, stream))   // (derived at open; a no-op unless the set was packed again)
        return rc;
    const bool tn93 = s->measure == DST_TN93;
    if (tn93)
        HIP_TRY(ctx, launch_window_counts(batch, s->wc_table, s->n_windows, s->wc_t_counts, stream));
    WindowLaunch wl{};
    wl.rows = &loaded;
    wl.cols = &batch;
    wl.square = false;
    wl.out_kind = DST_OUT_TALLY;
    wl.d_out = s->wc_scratch;
    wl.d_windows = s->wc_table;
    const uint64_t n_loaded = s->n_loaded;
    for (uint64_t r0 = 0; r0 < n_loaded; r0 += s->wc_cut.rows) {
        const uint64_t nr = std::min<uint64_t>(s->wc_cut.rows, n_loaded - r0);
        for (uint32_t w0 = 0; w0 < s->n_windows; w0 += s->wc_cut.wins) {
            const uint32_t nw = std::min<uint32_t>(s->wc_cut.wins, s->n_windows - w0);
            wl.row_begin = r0;
            wl.row_end = r0 + nr;
            wl.pairs = nr * n_records;
            wl.win_first = w0;
            wl.n_windows = nw;
            HIP_TRY(ctx, launch_window_pairs(s->measure, wl, stream));
            HIP_TRY(ctx, launch_window_nearest_stream(s->measure, s->wc_scratch, s->wc_q_counts, s->wc_t_counts, n_loaded, n_records,
                                                      r0, nr, w0, nw, s->n_windows, (uint32_t)s->next_ordinal, s->nl, s->wc_cnt,
                                                      stream));
        }
    }
    return note_run(ctx, stream);   // a rebuild of the loaded set's planes on another stream waits for these sweeps
}

// closest: -1 a plain stream, else the dst_closest_side of a closest stream (out_kind DST_OUT_TALLY, on the device only)
int open_stream(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, int wire, int closest, uint32_t k,
                dst_stream **out)
{
    if (!ctx || !out)
        return DST_ERR_ARG;
    *out = nullptr;
    if (wire != DST_WIRE_CODES && wire != DST_WIRE_NIBBLES)
        return fail(ctx, DST_ERR_ARG, "unknown wire format");
    if (measure < DST_N || measure > DST_TN93)
        return fail(ctx, DST_ERR_ARG, "unknown measure");
    if (out_kind != DST_OUT_DISTANCE && out_kind != DST_OUT_TALLY)
        return fail(ctx, DST_ERR_ARG, "a stream delivers DST_OUT_DISTANCE or DST_OUT_TALLY");
    if (max_records == 0 || depth < 2 || depth > 16)
        return fail(ctx, DST_ERR_ARG, "max_records must be positive and depth in 2..16");
    const DeviceSet &loaded = ctx->set[0];
    if (!loaded.loaded)
        return fail(ctx, DST_ERR_STATE, "upload the loaded set to slot 0 before opening a stream");
    if (closest >= 0 && loaded.n >= 0xFFFFFFFFull)
        return fail(ctx, DST_ERR_ARG, "sets of 2^32-1 records or more");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    dst_stream *s = new (std::nothrow) dst_stream;
    if (!s)
        return DST_ERR_NOMEM;
    s->ctx = ctx;
    s->measure = measure;
    s->out_kind = out_kind;
    s->max_records = max_records;
    s->len = loaded.len;
    s->wire = wire;
    s->closest = closest;
    s->k = k;
    s->k_streamed = (uint32_t)std::min<uint64_t>(k, loaded.n);
    s->n_loaded = loaded.n;
    s->W = tally_width(measure);
    // rows 128 bytes apart at least: whole 128-site chunks of input per row (64 bytes of nibbles, 128 of codes)
    s->pitch = wire == DST_WIRE_NIBBLES ? std::max<size_t>(((((loaded.len + 127) / 128) * 64 + 127) / 128) * 128, 128)
                                        : std::max<size_t>(((loaded.len + 127) / 128) * 128, 128);
    s->out_bytes_per_record = dst_out_bytes(measure, out_kind, loaded.n);
    s->slots.resize((size_t)depth);
    hipError_t e = hipStreamCreateWithFlags(&s->s_in, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->s_compute, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->s_out, hipStreamNonBlocking);
    const size_t in_bytes = counts_offset(s) + max_records * 16;
    // (a window-closest stream has no matrix: its tallies go range by range through the stream's one scratch)
    const size_t out_bytes = closest == kWindowClosestStream ? 16 : std::max<size_t>(s->out_bytes_per_record * max_records, 16);
    const char *const what = closest == kWindowClosestStream ? "window-closest stream" : nullptr;   // (NOMEM with the byte count)
    // after the first failure, the runtime's (e) or an allocation's (rc), nothing more is made; destroy() frees the rest
    int rc = DST_OK;
    auto grow = [&](GrownBase &b, size_t bytes) {
        if (e == hipSuccess && !rc)
            rc = b.grow(ctx, bytes, what);
    };
    for (auto &sl : s->slots) {
        grow(sl.h_in, in_bytes);
        grow(sl.d_in, in_bytes);
        grow(sl.d_out, out_bytes);
        if (closest < 0)
            grow(sl.h_out, out_bytes);
        if (closest == DST_CLOSEST_FOR_STREAMED) {
            const uint64_t entries = (uint64_t)max_records * s->k_streamed;
            const size_t bytes = std::max<size_t>(lists_layout(nullptr, entries, s->W, sl.nl), 16);
            grow(sl.d_lists, bytes);
            grow(sl.h_lists, bytes);
            lists_layout(sl.d_lists, entries, s->W, sl.nl);
            lists_layout(sl.h_lists, entries, s->W, sl.h_nl);
            sl.nl.k = sl.h_nl.k = s->k_streamed;
        }
        grow(sl.d_bad, sizeof(unsigned long long));
        grow(sl.h_bad, sizeof(unsigned long long));
    }
    if (closest == DST_CLOSEST_FOR_LOADED) {
        const uint64_t entries = (uint64_t)loaded.n * k;
        grow(s->d_lists, std::max<size_t>(lists_layout(nullptr, entries, s->W, s->nl), 16));
        lists_layout(s->d_lists, entries, s->W, s->nl);
        s->nl.k = k;
        if (e == hipSuccess && !rc) e = launch_nearest_init(s->nl, loaded.n, s->s_compute);
    }
    if (rc || e != hipSuccess) {
        destroy(s);
        return rc ? rc : fail_hip(ctx, e, "dst_stream_open");
    }
    *out = s;
    return DST_OK;
}

}  // namespace

extern "C" {

int dst_stream_acquire(dst_stream *s, uint8_t **codes, size_t *pitch, uint32_t **base_counts)
{
    if (!s || !codes || !pitch)
        return DST_ERR_ARG;
    if (s->acquired >= 0)
        return fail(s->ctx, DST_ERR_STATE, "a buffer is already acquired: submit it first");
    auto &sl = s->slots[s->next_acquire % s->slots.size()];
    if (sl.state == 2)
        return fail(s->ctx, DST_ERR_STATE, "every slot is in flight: collect a batch first");
    // the slot's previous batch: its kernels read the slot's planes, its copies read the slot's buffers
    HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    if (sl.landed && sl.state == 3)
        HIP_TRY(s->ctx, hipEventSynchronize(sl.landed));
    sl.state = 1;
    if (s->closest == kGroupSummaryStream)
        std::memset(sl.h_labels.ptr, 0, s->max_records * 4);   // (every record in streamed group 0 until the caller says otherwise)
    s->acquired = (int)(s->next_acquire % s->slots.size());
    *codes = sl.h_in;
    *pitch = s->pitch;
    if (base_counts)
        *base_counts = reinterpret_cast<uint32_t *>(sl.h_in + counts_offset(s));
    return DST_OK;
}

int dst_stream_submit(dst_stream *s, size_t n_records, int use_base_counts)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->acquired < 0)
        return fail(ctx, DST_ERR_STATE, "no buffer acquired");
    if (n_records == 0 || n_records > s->max_records)
        return fail(ctx, DST_ERR_ARG, "n_records must be in 1..max_records");
    DeviceSet &loaded = ctx->set[0];
    if (!loaded.loaded || loaded.len != s->len || (s->closest >= 0 && loaded.n != s->n_loaded))
        return fail(ctx, DST_ERR_STATE, "the loaded set changed while the stream was open");
    const bool grouped = s->closest == kGroupSummaryStream;
    const bool summary = s->closest == kSummaryStream || grouped;   // (what the two kinds share)
    if (s->poisoned && summary)
        return fail(ctx, DST_ERR_STATE, "a batch of this summary stream held an invalid code: its sums are not trustworthy");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this closest stream held an invalid code: its lists are not trustworthy");
    if (summary && s->submitted + (uint64_t)n_records > 0xFFFFFFFEull)   // (64-bit: the counters are uint32, the hi / lo split
        return fail(ctx, DST_ERR_CAPACITY, "a summary stream ends at 2^32-2 records");   //  needs fewer than 2^32 partners)
    const bool windowed = s->closest == kWindowClosestStream;
    if ((s->closest == DST_CLOSEST_FOR_LOADED || windowed) && s->next_ordinal + n_records - 1 > 0xFFFFFFFEull)
        return fail(ctx, DST_ERR_CAPACITY, "streamed ordinals end at 2^32-2");
    if (windowed)
        use_base_counts = 0;   // per-window counts cannot come from the caller: counted by code on the device
    auto &sl = s->slots[(size_t)s->acquired];
    // a group-summary stream: the labels are checked here, before anything changes; the batch's assigned records in order
    // of their group (a counting sort) go behind them
    std::vector<uint64_t> batch_size;
    if (grouped) {
        const uint32_t *labels = sl.h_labels;
        if (int rc = group_labels(ctx, labels, n_records, s->g_streamed, "streamed", batch_size))
            return rc;
        std::vector<uint64_t> next(s->g_streamed, 0);
        for (uint32_t a = 1; a < s->g_streamed; ++a)
            next[a] = next[a - 1] + batch_size[a - 1];
        uint32_t *order = sl.h_labels + s->max_records;
        for (size_t x = 0; x < n_records; ++x)
            if (labels[x] != DST_GROUP_NONE)
                order[next[labels[x]]++] = (uint32_t)x;
        sl.assigned = next[s->g_streamed - 1];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // copy-in: the batch's bytes (and the caller's base counts)
    if (grouped) {
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_labels, sl.h_labels, n_records * 4, hipMemcpyHostToDevice, s->s_in));
        if (sl.assigned)
            HIP_TRY(ctx, hipMemcpyAsync(sl.d_labels + s->max_records, sl.h_labels + s->max_records, sl.assigned * 4,
                                        hipMemcpyHostToDevice, s->s_in));
    }
    if (s->len)
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_in, sl.h_in, n_records * s->pitch, hipMemcpyHostToDevice, s->s_in));
    if (use_base_counts)
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_in + counts_offset(s), sl.h_in + counts_offset(s), n_records * 16,
                                    hipMemcpyHostToDevice, s->s_in));
    HIP_TRY(ctx, sl.h2d.record(s->s_in));
    // compute: pack, then the batch (rows) against the loaded set (columns): streamed-major order
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_compute, sl.h2d, 0));
    int rc = pack_queue(ctx, sl.set, sl.d_in, n_records, s->len, s->pitch,
                        use_base_counts ? reinterpret_cast<const uint32_t *>(sl.d_in + counts_offset(s)) : nullptr,
                        sl.d_bad, s->s_compute, false, s->wire == DST_WIRE_NIBBLES);
    if (rc)
        return rc;
    sl.set.loaded = true;  // validity is reported by dst_stream_collect
    if (!windowed && s->measure == DST_TN93 && (s->out_kind == DST_OUT_DISTANCE || s->closest >= 0) && !sl.set.have_counts) {
        HIP_TRY(ctx, launch_fill_counts(sl.set, s->s_compute));  // same stream as the kernel that reads them
        sl.set.have_counts = true;
    }
    if (!windowed && s->measure == DST_TN93 && s->closest >= 0) {   // the selection finalises the tallies: the loaded set's counts too
        rc = need_counts(ctx, loaded, s->s_compute);
        if (rc)
            return rc;
    }
    // a window-closest stream: no pair kernel and no matrix, the window sweep and the merge range by range
    const size_t bytes = windowed ? 0 : s->out_bytes_per_record * n_records;
    rc = windowed ? window_closest_batch(s, sl.set, n_records)
                  : run_sets(ctx, s->measure, false, sl.set, loaded, 0, n_records, s->out_kind, sl.d_out, bytes, (void *)s->s_compute);
    if (rc)
        return rc;
    // a closest stream: the selection directly behind the batch's pair kernel, on the one compute stream
    const uint32_t *tallies = static_cast<const uint32_t *>(sl.d_out.ptr);
    if (s->closest == DST_CLOSEST_FOR_LOADED) {
        HIP_TRY(ctx, launch_nearest_stream_cols(s->measure, tallies, n_records, s->n_loaded, (uint32_t)s->next_ordinal,
                                                sl.set.counts, loaded.counts, s->nl, s->s_compute));
    } else if (s->closest == DST_CLOSEST_FOR_STREAMED && s->k_streamed) {
        HIP_TRY(ctx, launch_nearest_init(sl.nl, n_records, s->s_compute));
        HIP_TRY(ctx, launch_nearest_rows(s->measure, false, tallies, 0, s->n_loaded, 0, n_records, sl.set.counts, loaded.counts,
                                         sl.nl, s->s_compute));
    }
    // a links stream: the count, the scan and window 0 behind the pair kernel, then the header for the one copy
    if (s->closest == kLinksStream) {
        const bool tally = (s->what & DST_LINKS_TALLIES) != 0;
        if (s->any_links) {
            HIP_TRY(ctx, launch_links_count(s->measure, tally, false, sl.d_out, 0, s->n_loaded, 0, n_records, s->t_bits,
                                            sl.set.counts, loaded.counts, sl.lb, s->s_compute));
            HIP_TRY(ctx, launch_links_write(s->measure, tally, false, sl.d_out, 0, s->n_loaded, 0, n_records, s->t_bits,
                                            sl.set.counts, loaded.counts, sl.lb, 0, s->window, (s->what & DST_LINKS_VALUES) != 0,
                                            tally, s->s_compute));
        }
        HIP_TRY(ctx, launch_links_stream_header(s->any_links ? sl.lb.offsets + links_blocks(false, s->n_loaded, 0, n_records) : nullptr,
                                                sl.d_bad, sl.d_hdr, s->s_compute));
        sl.window_first = 0;
        s->last_collected = -1;   // the collected batch's links were valid until this submit
    }
    // a summary stream: the tile pass for both sides and the totals, then the histogram pass, behind the pair kernel
    const bool sum_streamed = s->closest == kSummaryStream && (s->what & DST_STREAM_SUMMARY_STREAMED);
    if (s->closest == kSummaryStream) {
        const uint64_t *matrix = static_cast<const uint64_t *>(sl.d_out.ptr);
        SummaryBuffers batch{};
        if (sum_streamed)
            HIP_TRY(ctx, hipMemsetAsync(sl.d_lists, 0, records_layout(sl.d_lists, n_records, batch), s->s_compute));
        HIP_TRY(ctx, launch_summary_stream(s->measure, matrix, n_records, s->n_loaded, s->t_bits, s->any_links,
                                           (s->what & DST_STREAM_SUMMARY_LOADED) ? &s->sum_kept : nullptr,
                                           sum_streamed ? &batch : nullptr, s->sum_kept.tot, s->s_compute));
        if (s->bins)
            HIP_TRY(ctx, launch_summary_hist(s->measure, matrix, (uint64_t)n_records * s->n_loaded, s->bins, s->width_q, s->t_bits,
                                             s->any_links, true, s->sum_hist, s->s_compute));
        s->last_collected = -1;   // the collected batch's results were valid until this submit
    }
    // a group-summary stream: dst_group_summary's row pass and its fold into the kept cells, then the loaded side
    const bool grp_streamed = grouped && (s->what & DST_STREAM_GROUPS_STREAMED);
    const uint64_t batch_entries = grouped ? (uint64_t)n_records * s->g_loaded : 0;
    if (grouped) {
        const uint64_t *matrix = static_cast<const uint64_t *>(sl.d_out.ptr);
        const bool cells_run = s->n_loaded != 0 && s->loaded_assigned != 0;
        GroupBuffers b = s->grp_kept;   // col_group, cell, g_rows, g_cols
        b.row_group = sl.d_labels;
        b.order = sl.d_labels + s->max_records;
        if (grp_streamed || cells_run)
            HIP_TRY(ctx, hipMemsetAsync(sl.d_lists, 0, table_layout(sl.d_lists, batch_entries, b), s->s_compute));
        if (cells_run) {
            static const bool no_aggregation = std::getenv("DST_GROUPS_NO_AGGREGATION") != nullptr;   // 
            HIP_TRY(ctx, launch_group_rows(s->measure, false, matrix, 0, s->n_loaded, 0, n_records, s->t_bits, s->any_links,
                                           !no_aggregation, b, s->s_compute));
            HIP_TRY(ctx, launch_group_fold(b, sl.assigned, s->s_compute));
        }
        if ((s->what & DST_STREAM_GROUPS_LOADED) && sl.assigned) {
            GroupBuffers t = s->grp_kept;   // the kept table, keyed by the streamed group
            t.row_group = sl.d_labels;
            t.g_cols = s->g_streamed;
            HIP_TRY(ctx, launch_group_stream_cols(s->measure, matrix, n_records, s->n_loaded, s->t_bits, s->any_links, t, s->s_compute));
        }
        s->last_collected = -1;   // the collected batch's results were valid until this submit
    }
    HIP_TRY(ctx, sl.computed.record(s->s_compute));
    // copy-out
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_out, sl.computed, 0));
    if (s->closest == kLinksStream)
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_hdr, sl.d_hdr, 16, hipMemcpyDeviceToHost, s->s_out));
    else
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_bad, sl.d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->s_out));
    if (s->closest < 0) {
        if (bytes)
            HIP_TRY(ctx, hipMemcpyAsync(sl.h_out, sl.d_out, bytes, hipMemcpyDeviceToHost, s->s_out));
    } else if (s->closest == DST_CLOSEST_FOR_STREAMED && s->k_streamed) {
        const size_t e = n_records * (size_t)s->k_streamed;
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.idx, sl.nl.idx, e * 4, hipMemcpyDeviceToHost, s->s_out));
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.val, sl.nl.val, e * 8, hipMemcpyDeviceToHost, s->s_out));
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.tal, sl.nl.tal, e * 4 * (size_t)s->W, hipMemcpyDeviceToHost, s->s_out));
    } else if (sum_streamed) {
        SummaryBuffers none{};
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_lists, sl.d_lists, records_layout(nullptr, n_records, none), hipMemcpyDeviceToHost, s->s_out));
    } else if (grp_streamed) {
        GroupBuffers none{};
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_lists, sl.d_lists, table_layout(nullptr, batch_entries, none), hipMemcpyDeviceToHost, s->s_out));
    }
    HIP_TRY(ctx, sl.landed.record(s->s_out));
    if (s->closest == DST_CLOSEST_FOR_LOADED || windowed) {
        s->next_ordinal += n_records;
        s->submitted += n_records;
    }
    if (summary)
        s->submitted += n_records;
    for (uint32_t a = 0; grouped && a < s->g_streamed; ++a)
        s->streamed_size[a] += batch_size[a];
    sl.n = n_records;
    sl.state = 2;
    s->acquired = -1;
    s->next_acquire += 1;
    s->in_flight += 1;
    return DST_OK;
}

int dst_stream_collect(dst_stream *s, size_t *n_records, const void **results)
{
    if (!s || !n_records || !results)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->in_flight == 0)
        return fail(ctx, DST_ERR_STATE, "no submitted batch to collect");
    auto &sl = s->slots[s->next_collect % s->slots.size()];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(sl.landed));
    s->next_collect += 1;
    s->in_flight -= 1;
    sl.state = 3;
    s->last_collected = (int)((s->next_collect - 1) % s->slots.size());
    const bool links = s->closest == kLinksStream;
    const unsigned long long bad = links ? sl.h_hdr[1] : *sl.h_bad;
    if (bad != ~0ull) {
        s->poisoned = s->closest >= 0 && !links;   // (a links stream keeps nothing across batches)
        if (links)
            s->last_collected = -1;
        return invalid_code_error(ctx, bad, s->len);
    }
    if (links) {
        sl.total = sl.h_hdr[0];
        if (sl.total > (uint64_t)sl.n * s->n_loaded) {
            s->last_collected = -1;
            return fail(ctx, DST_ERR_STATE, "links stream: more links than pairs in a batch");
        }
        s->links_total += sl.total;
        if (s->via_copy && sl.total) {   // the copy route: what window 0 holds, now that the total is known
            if (int rc = copy_window(s, sl, std::min(sl.total, s->window), s->s_out))
                return rc;
        }
    }
    if (s->closest == kSummaryStream && (s->what & DST_STREAM_SUMMARY_STREAMED)) {
        // the batch's records: the 128-bit sums here, each converted once into the place of its high word
        SummaryBuffers h{};
        records_layout(sl.h_lists, sl.n, h);
        const bool int_payload = s->measure == DST_N || s->measure == DST_N_HIGH;
        for (size_t x = 0; x < sl.n; ++x) {
            const double v = summary_value((__int128)h.hi[x] * ((__int128)1 << 32) + (__int128)h.lo[x], int_payload);
            std::memcpy(h.hi + x, &v, 8);
        }
    }
    if (s->closest == kGroupSummaryStream && (s->what & DST_STREAM_GROUPS_STREAMED)) {
        // the batch's table: the packed counts split into the two arrays behind the planes, the 128-bit sums converted
        // once into the place of their high words
        const uint64_t entries = (uint64_t)sl.n * s->g_loaded, room = (uint64_t)s->max_records * s->g_loaded;
        uint32_t *within = reinterpret_cast<uint32_t *>(static_cast<char *>(sl.h_lists.ptr) + room * 24);
        uint32_t *summable = within + room;
        GroupBuffers got{};
        table_layout(sl.h_lists, entries, got);   // (as the copy left it: planes of the batch's own entries)
        const bool int_payload = s->measure == DST_N || s->measure == DST_N_HIGH;
        for (uint64_t x = 0; x < entries; ++x) {
            within[x] = (uint32_t)(got.counts[x] >> 32);
            summable[x] = (uint32_t)got.counts[x];
            const double v = summary_value((__int128)got.hi[x] * ((__int128)1 << 32) + (__int128)got.lo[x], int_payload);
            std::memcpy(got.hi + x, &v, 8);
        }
    }
    *n_records = sl.n;
    *results = sl.h_out;   // (NULL for a closest stream: its results never leave the device as a matrix)
    return DST_OK;
}

int dst_stream_summary_batch(dst_stream *s, size_t *n_records, const uint32_t **within, const uint32_t **summable,
                             const double **sum)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->closest != kSummaryStream)
        return fail(ctx, DST_ERR_ARG, "not a summary stream");
    if (!(s->what & DST_STREAM_SUMMARY_STREAMED))
        return fail(ctx, DST_ERR_ARG, "the stream was opened without DST_STREAM_SUMMARY_STREAMED");
    if (!n_records)
        return fail(ctx, DST_ERR_ARG, "null n_records pointer");
    *n_records = 0;
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this summary stream held an invalid code: its sums are not trustworthy");
    if (s->last_collected < 0 || s->slots[(size_t)s->last_collected].state != 3)
        return fail(ctx, DST_ERR_STATE, "no collected batch: its results are valid from dst_stream_collect to the next submit");
    const auto &sl = s->slots[(size_t)s->last_collected];
    SummaryBuffers h{};
    records_layout(sl.h_lists, sl.n, h);
    *n_records = sl.n;
    if (within)
        *within = h.within;
    if (summable)
        *summable = h.summable;
    if (sum)
        *sum = reinterpret_cast<const double *>(h.hi);   // (converted at collect)
    return DST_OK;
}

int dst_stream_summary_result(dst_stream *s, uint64_t *hist, uint32_t *within, uint32_t *summable, double *sum, size_t cap,
                              dst_summary_totals *totals, uint64_t *records)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (totals)
        *totals = dst_summary_totals{0, 0, 0, 0, 0.0};
    if (records)
        *records = 0;
    if (s->closest != kSummaryStream)
        return fail(ctx, DST_ERR_ARG, "not a summary stream");
    const bool loaded = (s->what & DST_STREAM_SUMMARY_LOADED) != 0;
    if (!loaded && (within || summable || sum))
        return fail(ctx, DST_ERR_ARG, "the stream was opened without DST_STREAM_SUMMARY_LOADED: the per-record pointers must be NULL");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this summary stream held an invalid code: its sums are not trustworthy");
    if (s->in_flight != 0)
        return fail(ctx, DST_ERR_STATE, "collect every submitted batch before reading the summary");
    const size_t n = s->n_loaded;
    if ((within || summable || sum) && cap < n)
        return fail(ctx, DST_ERR_CAPACITY, "cap is below the loaded set's record count");
    // every batch is collected, so the compute stream is idle: the kept state back in one copy, the 128-bit sums here
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<char> host(s->sum_state_bytes);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), s->d_lists, s->sum_state_bytes, hipMemcpyDeviceToHost, s->s_compute));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
    SummaryBuffers h{}, hh{};
    summary_state_layout(host.data(), n, loaded, s->bins, h, hh);
    const bool int_payload = s->measure == DST_N || s->measure == DST_N_HIGH;
    dst_summary_totals t{s->submitted * (uint64_t)n, h.tot[0], h.tot[1], h.tot[2], 0.0};
    const __int128 all = (__int128)(((unsigned __int128)h.tot[3] << 64) | h.tot[4]);
    // no total is counted twice: the histogram pass' own totals, and the loaded records' entries, only have to agree
    if (s->bins && (hh.tot[0] != h.tot[0] || hh.tot[1] != h.tot[1] || hh.tot[2] != h.tot[2] || hh.tot[3] != h.tot[3] ||
                    hh.tot[4] != h.tot[4]))
        return fail(ctx, DST_ERR_STATE, "summary stream: internal error, the passes disagree");
    if (loaded) {
        uint64_t w2 = 0, s2 = 0;
        __int128 all2 = 0;
        for (size_t x = 0; x < n; ++x) {
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
        if (w2 != t.links || s2 != t.summable_pairs || all2 != all)
            return fail(ctx, DST_ERR_STATE, "summary stream: internal error, the loaded records and the totals disagree");
    }
    if (hist)
        for (uint32_t b = 0; b < s->bins; ++b)
            hist[b] = h.hist[b];
    t.sum = summary_value(all, int_payload);
    if (totals)
        *totals = t;
    if (records)
        *records = s->submitted;
    return DST_OK;
}

int dst_stream_group_labels(dst_stream *s, uint32_t **labels)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (labels)
        *labels = nullptr;
    if (s->closest != kGroupSummaryStream)
        return fail(ctx, DST_ERR_ARG, "not a group-summary stream");
    if (!labels)
        return fail(ctx, DST_ERR_ARG, "null labels pointer");
    if (s->acquired < 0)
        return fail(ctx, DST_ERR_STATE, "no buffer acquired: the label block is valid between dst_stream_acquire and dst_stream_submit");
    *labels = s->slots[(size_t)s->acquired].h_labels;
    return DST_OK;
}

int dst_stream_group_summary_batch(dst_stream *s, size_t *n_records, const uint32_t **within, const uint32_t **summable,
                                   const double **sum)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->closest != kGroupSummaryStream)
        return fail(ctx, DST_ERR_ARG, "not a group-summary stream");
    if (!(s->what & DST_STREAM_GROUPS_STREAMED))
        return fail(ctx, DST_ERR_ARG, "the stream was opened without DST_STREAM_GROUPS_STREAMED");
    if (!n_records)
        return fail(ctx, DST_ERR_ARG, "null n_records pointer");
    *n_records = 0;
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this summary stream held an invalid code: its sums are not trustworthy");
    if (s->last_collected < 0 || s->slots[(size_t)s->last_collected].state != 3)
        return fail(ctx, DST_ERR_STATE, "no collected batch: its results are valid from dst_stream_collect to the next submit");
    const auto &sl = s->slots[(size_t)s->last_collected];
    const uint64_t entries = (uint64_t)sl.n * s->g_loaded, room = (uint64_t)s->max_records * s->g_loaded;
    GroupBuffers h{};
    table_layout(sl.h_lists, entries, h);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(static_cast<const char *>(sl.h_lists.ptr) + room * 24);
    *n_records = sl.n;
    if (within)
        *within = w;
    if (summable)
        *summable = w + room;
    if (sum)
        *sum = reinterpret_cast<const double *>(h.hi);   // (converted at collect)
    return DST_OK;
}

int dst_stream_group_summary_result(dst_stream *s, dst_group_cell *cells, size_t cells_cap, uint32_t *rec_within,
                                    uint32_t *rec_summable, double *rec_sum, size_t rec_cap, uint64_t *records)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (records)
        *records = 0;
    if (s->closest != kGroupSummaryStream)
        return fail(ctx, DST_ERR_ARG, "not a group-summary stream");
    const bool loaded = (s->what & DST_STREAM_GROUPS_LOADED) != 0, per_record = rec_within || rec_summable || rec_sum;
    if (!loaded && per_record)
        return fail(ctx, DST_ERR_ARG, "the stream was opened without DST_STREAM_GROUPS_LOADED: the per-record pointers must be NULL");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this summary stream held an invalid code: its sums are not trustworthy");
    if (s->in_flight != 0)
        return fail(ctx, DST_ERR_STATE, "collect every submitted batch before reading the summary");
    const uint32_t Gs = s->g_streamed, Gl = s->g_loaded;
    const size_t n_cells = (size_t)Gs * Gl;
    const uint64_t n_rec = (uint64_t)s->n_loaded * Gs;
    if (cells && cells_cap < n_cells)
        return fail(ctx, DST_ERR_CAPACITY, "cells_cap is below " + std::to_string(n_cells) + " entries (streamed groups x loaded groups)");
    if (per_record && rec_cap < n_rec)
        return fail(ctx, DST_ERR_CAPACITY, "rec_cap is below " + std::to_string(n_rec) + " entries (the loaded records x streamed groups)");
    // every batch is collected, so the compute stream is idle: the cells, and the table behind them when it is wanted, back
    // in one copy
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t back = (per_record ? s->grp_state_bytes : s->grp_cells_at + n_cells * kGroupCellWords * 8) - s->grp_cells_at;
    std::vector<char> host(back);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), static_cast<const char *>(s->d_lists.ptr) + s->grp_cells_at, back, hipMemcpyDeviceToHost,
                                s->s_compute));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
    const bool int_payload = s->measure == DST_N || s->measure == DST_N_HIGH;
    const uint64_t *cell = reinterpret_cast<const uint64_t *>(host.data());
    if (cells) {
        const uint64_t none = int_payload ? 0 : 0x7FF8000000000000ull;
        const uint64_t *nan = cell, *links = cell + n_cells, *summ = cell + 2 * n_cells, *high = cell + 3 * n_cells,
                       *low = cell + 4 * n_cells, *kmin = cell + 5 * n_cells, *kmax = cell + 6 * n_cells;
        for (uint32_t a = 0; a < Gs; ++a)
            for (uint32_t g = 0; g < Gl; ++g) {
                const size_t c = (size_t)a * Gl + g;
                dst_group_cell out{s->streamed_size[a] * s->loaded_size[g], nan[c], summ[c], links[c], 0.0, none, none};
                if (out.nan_pairs + out.summable_pairs > out.pairs || out.links > out.pairs)
                    return fail(ctx, DST_ERR_STATE, "group-summary stream: internal error, a cell counts more than its pairs");
                out.sum = summary_value((__int128)(((unsigned __int128)high[c] << 64) | low[c]), int_payload);
                if (out.pairs > out.nan_pairs) {
                    out.min_bits = payload_of_key(kmin[c], int_payload);
                    out.max_bits = payload_of_key(kmax[c], int_payload);
                }
                cells[c] = out;
            }
    }
    if (per_record) {
        GroupBuffers h{};
        table_layout(host.data() + n_cells * kGroupCellWords * 8, n_rec, h);
        for (uint64_t i = 0; i < s->n_loaded; ++i)   // (the kept table is group-major: entry g n_loaded + i)
            for (uint32_t g = 0; g < Gs; ++g) {
                const uint64_t e = i * Gs + g, at = (uint64_t)g * s->n_loaded + i;
                if (rec_within)
                    rec_within[e] = (uint32_t)(h.counts[at] >> 32);
                if (rec_summable)
                    rec_summable[e] = (uint32_t)h.counts[at];
                if (rec_sum)
                    rec_sum[e] = summary_value((__int128)h.hi[at] * ((__int128)1 << 32) + (__int128)h.lo[at], int_payload);
            }
    }
    if (records)
        *records = s->submitted;
    return DST_OK;
}

int dst_stream_closest_next_index(dst_stream *s, uint64_t next)
{
    if (!s)
        return DST_ERR_ARG;
    if (s->closest != DST_CLOSEST_FOR_LOADED && s->closest != kWindowClosestStream)
        return fail(s->ctx, DST_ERR_ARG, "not a DST_CLOSEST_FOR_LOADED or window-closest stream");
    if (s->in_flight != 0)
        return fail(s->ctx, DST_ERR_STATE, "collect every submitted batch before renumbering");
    if (next < s->next_ordinal || next > 0xFFFFFFFFull)
        return fail(s->ctx, DST_ERR_ARG, "the next ordinal must not go backwards, nor past 2^32-1");
    s->next_ordinal = next;
    return DST_OK;
}

int dst_stream_closest_result(dst_stream *s, uint32_t *index, uint32_t *tallies, void *values, size_t cap_entries,
                              uint32_t *k_used)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (k_used)
        *k_used = 0;
    if (s->closest != DST_CLOSEST_FOR_LOADED)
        return fail(ctx, DST_ERR_ARG, "not a DST_CLOSEST_FOR_LOADED stream");
    if (!index || !k_used)
        return fail(ctx, DST_ERR_ARG, "null index or k_used pointer");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this closest stream held an invalid code: its lists are not trustworthy");
    if (s->in_flight != 0)
        return fail(ctx, DST_ERR_STATE, "collect every submitted batch before reading the lists");
    const uint32_t ku = (uint32_t)std::min<uint64_t>(s->k, s->submitted);
    if ((uint64_t)s->n_loaded * ku > cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "cap_entries is below n_loaded x k_used");
    *k_used = ku;
    if (ku == 0 || s->n_loaded == 0)
        return DST_OK;
    // every batch is collected, so the compute stream is idle; the first k_used entries of every row, dense
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t k = s->k, n = s->n_loaded, w4 = 4 * (size_t)s->W;
    HIP_TRY(ctx, hipMemcpy2DAsync(index, ku * 4, s->nl.idx, k * 4, ku * 4, n, hipMemcpyDeviceToHost, s->s_compute));
    if (values)
        HIP_TRY(ctx, hipMemcpy2DAsync(values, ku * 8, s->nl.val, k * 8, ku * 8, n, hipMemcpyDeviceToHost, s->s_compute));
    if (tallies)
        HIP_TRY(ctx, hipMemcpy2DAsync(tallies, ku * w4, s->nl.tal, k * w4, ku * w4, n, hipMemcpyDeviceToHost, s->s_compute));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
    return DST_OK;
}

int dst_stream_window_closest_result(dst_stream *s, uint32_t *index, uint32_t *tallies, void *values, uint32_t *col_counts,
                                     size_t cap_entries, uint32_t *k_used)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (k_used)
        *k_used = 0;
    if (s->closest != kWindowClosestStream)
        return fail(ctx, DST_ERR_ARG, "not a window-closest stream");
    if (!index || !k_used)
        return fail(ctx, DST_ERR_ARG, "null index or k_used pointer");
    if (col_counts && s->measure != DST_TN93)
        return fail(ctx, DST_ERR_ARG, "col_counts are tn93's: the lists of another measure carry no base counts");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this closest stream held an invalid code: its lists are not trustworthy");
    if (s->in_flight != 0)
        return fail(ctx, DST_ERR_STATE, "collect every submitted batch before reading the lists");
    const uint32_t ku = (uint32_t)std::min<uint64_t>(s->k, s->submitted);
    *k_used = ku;
    const uint64_t n_lists = (uint64_t)s->n_loaded * s->n_windows;
    if ((unsigned __int128)n_lists * ku > (unsigned __int128)cap_entries)
        return fail(ctx, DST_ERR_CAPACITY, "cap_entries is below n_loaded x n_windows x k_used");
    if (ku == 0 || n_lists == 0)
        return DST_OK;
    // every batch is collected; the wait is for the merges behind the last one.  The first k_used entries of every list,
    // dense: one strided copy per array (one plain copy when the lists are full).
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
    const size_t k = s->k;
    const auto compact = [&](void *host, const void *dev, size_t entry_bytes) -> hipError_t {
        if (ku == k)
            return hipMemcpyAsync(host, dev, n_lists * k * entry_bytes, hipMemcpyDeviceToHost, s->s_compute);
        return hipMemcpy2DAsync(host, ku * entry_bytes, dev, k * entry_bytes, ku * entry_bytes, n_lists, hipMemcpyDeviceToHost,
                                s->s_compute);
    };
    HIP_TRY(ctx, compact(index, s->nl.idx, 4));
    if (values)
        HIP_TRY(ctx, compact(values, s->nl.val, 8));
    if (tallies)
        HIP_TRY(ctx, compact(tallies, s->nl.tal, 4 * (size_t)s->W));
    if (col_counts)
        HIP_TRY(ctx, compact(col_counts, s->wc_cnt, 16));
    HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
    return DST_OK;
}

int dst_stream_closest_batch(dst_stream *s, const uint32_t **index, const uint32_t **tallies, const void **values,
                             uint32_t *k_used)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->closest != DST_CLOSEST_FOR_STREAMED)
        return fail(ctx, DST_ERR_ARG, "not a DST_CLOSEST_FOR_STREAMED stream");
    if (!index || !k_used)
        return fail(ctx, DST_ERR_ARG, "null index or k_used pointer");
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this closest stream held an invalid code");
    if (s->last_collected < 0 || s->slots[(size_t)s->last_collected].state != 3)
        return fail(ctx, DST_ERR_STATE, "no collected batch: its lists are valid from dst_stream_collect to the next submit");
    const auto &sl = s->slots[(size_t)s->last_collected];
    *index = sl.h_nl.idx;
    if (tallies)
        *tallies = sl.h_nl.tal;
    if (values)
        *values = sl.h_nl.val;
    *k_used = s->k_streamed;
    return DST_OK;
}

int dst_stream_links_batch(dst_stream *s, uint64_t first_link, uint64_t *n_links, uint64_t *batch_links,
                           const uint32_t **streamed, const uint32_t **loaded, const void **values, const uint32_t **tallies)
{
    if (!s)
        return DST_ERR_ARG;
    dst_ctx *ctx = s->ctx;
    if (s->closest != kLinksStream)
        return fail(ctx, DST_ERR_ARG, "not a links stream");
    if (!n_links || !batch_links || !streamed || !loaded)
        return fail(ctx, DST_ERR_ARG, "null n_links, batch_links, streamed or loaded pointer");
    *n_links = *batch_links = 0;
    *streamed = *loaded = nullptr;
    if (values)
        *values = nullptr;
    if (tallies)
        *tallies = nullptr;
    if (s->last_collected < 0 || s->slots[(size_t)s->last_collected].state != 3)
        return fail(ctx, DST_ERR_STATE, "no collected batch: its links are valid from dst_stream_collect to the next submit");
    auto &sl = s->slots[(size_t)s->last_collected];
    *batch_links = sl.total;
    if (first_link > sl.total)
        return fail(ctx, DST_ERR_ARG, "first_link is above the batch's links");
    const uint64_t m = std::min(s->window, sl.total - first_link);
    if (m && sl.window_first != first_link) {
        // a late window: one write pass over the batch's matrix, still in the slot's device buffer; the compute stream orders
        // it behind whatever else reads or writes the slot
        const DeviceSet &set0 = ctx->set[0];
        const bool tally = (s->what & DST_LINKS_TALLIES) != 0;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        sl.window_first = ~0ull;
        HIP_TRY(ctx, launch_links_write(s->measure, tally, false, sl.d_out, 0, s->n_loaded, 0, sl.n, s->t_bits, sl.set.counts,
                                        set0.counts, sl.lb, first_link, first_link + m, (s->what & DST_LINKS_VALUES) != 0, tally,
                                        s->s_compute));
        if (s->via_copy) {
            if (int rc = copy_window(s, sl, m, s->s_compute))
                return rc;
        } else
            HIP_TRY(ctx, hipStreamSynchronize(s->s_compute));
        sl.window_first = first_link;
        s->late_windows += 1;
    }
    *n_links = m;
    *streamed = sl.h_lb.row;
    *loaded = sl.h_lb.col;
    if (values && (s->what & DST_LINKS_VALUES))
        *values = sl.h_lb.val;
    if (tallies && (s->what & DST_LINKS_TALLIES))
        *tallies = sl.h_lb.tal;
    return DST_OK;
}

int dst_stream_links_stats(const dst_stream *s, uint64_t *links, uint64_t *late_windows)
{
    if (!s || s->closest != kLinksStream)
        return DST_ERR_ARG;
    if (links)
        *links = s->links_total;
    if (late_windows)
        *late_windows = s->late_windows;
    return DST_OK;
}

int dst_stream_in_flight(const dst_stream *s) { return s ? (int)s->in_flight : -1; }

int dst_stream_close(dst_stream *s)
{
    destroy(s);
    return DST_OK;
}

}  // extern "C"
