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
#include <algorithm>
#include <cstdio>
#include <new>

#include "dst_ctx.h"

using namespace dst;

struct dst_stream {
    dst_ctx *ctx = nullptr;
    int measure = 0, out_kind = 0, wire = DST_WIRE_CODES;
    size_t max_records = 0, len = 0, pitch = 0;
    size_t out_bytes_per_record = 0;
    struct Slot {
        uint8_t *h_in = nullptr, *d_in = nullptr;  // max_records x pitch codes, then max_records x 4 base counts
        void *d_out = nullptr, *h_out = nullptr;
        void *d_lists = nullptr, *h_lists = nullptr;   // FOR_STREAMED: max_records x k_streamed entries, device and page-locked
        NearestLists nl{}, h_nl{};
        unsigned long long *d_bad = nullptr, *h_bad = nullptr;
        DeviceSet set;
        hipEvent_t h2d = nullptr, computed = nullptr, landed = nullptr;
        size_t n = 0;
        int state = 0;  // 0 free, 1 acquired, 2 submitted, 3 collected (results still readable)
    };
    std::vector<Slot> slots;
    hipStream_t s_in = nullptr, s_compute = nullptr, s_out = nullptr;
    size_t next_acquire = 0, next_collect = 0, in_flight = 0;
    int acquired = -1;
    // closest streams (closest = the dst_closest_side, -1: a plain stream)
    int closest = -1;
    uint32_t k = 0, k_streamed = 0;   // asked for; min(k, n_loaded): what a FOR_STREAMED batch's lists hold
    size_t n_loaded = 0;
    int W = 0;
    void *d_lists = nullptr;          // FOR_LOADED: n_loaded x k values, indices and W tallies
    NearestLists nl{};
    uint64_t next_ordinal = 0, submitted = 0;
    bool poisoned = false;            // a batch held an invalid code: the lists are not trustworthy
    int last_collected = -1;          // FOR_STREAMED: the slot dst_stream_closest_batch hands out
};

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

void destroy(dst_stream *s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->ctx->device);
    for (hipStream_t st : {s->s_in, s->s_compute, s->s_out})
        if (st)
            (void)hipStreamSynchronize(st);
    // (the context keeps marks of these streams, events of its own, and no handle it would hand to the runtime again:
    // dst_ctx::Mark.  They are idle now, so those events have completed.)
    for (auto &sl : s->slots) {
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.h_bad) (void)hipHostFree(sl.h_bad);
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.d_bad) (void)hipFree(sl.d_bad);
        if (sl.h_lists) (void)hipHostFree(sl.h_lists);
        if (sl.d_lists) (void)hipFree(sl.d_lists);
        free_set(sl.set);
        for (hipEvent_t e : {sl.h2d, sl.computed, sl.landed})
            if (e)
                (void)hipEventDestroy(e);
    }
    if (s->d_lists)
        (void)hipFree(s->d_lists);
    for (hipStream_t st : {s->s_in, s->s_compute, s->s_out})
        if (st)
            (void)hipStreamDestroy(st);
    delete s;
}

int open_stream(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, int wire, int closest, uint32_t k,
                dst_stream **out);

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

}  // extern "C"

namespace {

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
    const size_t out_bytes = std::max<size_t>(s->out_bytes_per_record * max_records, 16);
    for (auto &sl : s->slots) {
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_in, in_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_in, in_bytes);
        if (e == hipSuccess) e = hipMalloc(&sl.d_out, out_bytes);
        if (e == hipSuccess && closest < 0) e = hipHostMalloc(&sl.h_out, out_bytes, hipHostMallocDefault);
        if (closest == DST_CLOSEST_FOR_STREAMED) {
            const uint64_t entries = (uint64_t)max_records * s->k_streamed;
            const size_t bytes = std::max<size_t>(lists_layout(nullptr, entries, s->W, sl.nl), 16);
            if (e == hipSuccess) e = hipMalloc(&sl.d_lists, bytes);
            if (e == hipSuccess) e = hipHostMalloc(&sl.h_lists, bytes, hipHostMallocDefault);
            lists_layout(sl.d_lists, entries, s->W, sl.nl);
            lists_layout(sl.h_lists, entries, s->W, sl.h_nl);
            sl.nl.k = sl.h_nl.k = s->k_streamed;
        }
        if (e == hipSuccess) e = hipMalloc((void **)&sl.d_bad, sizeof(unsigned long long));
        if (e == hipSuccess) e = hipHostMalloc((void **)&sl.h_bad, sizeof(unsigned long long), hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.h2d, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.computed, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.landed, hipEventDisableTiming);
    }
    if (closest == DST_CLOSEST_FOR_LOADED) {
        const uint64_t entries = (uint64_t)loaded.n * k;
        if (e == hipSuccess) e = hipMalloc(&s->d_lists, std::max<size_t>(lists_layout(nullptr, entries, s->W, s->nl), 16));
        lists_layout(s->d_lists, entries, s->W, s->nl);
        s->nl.k = k;
        if (e == hipSuccess) e = launch_nearest_init(s->nl, loaded.n, s->s_compute);
    }
    if (e != hipSuccess) {
        destroy(s);
        return fail_hip(ctx, e, "dst_stream_open");
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
    if (s->poisoned)
        return fail(ctx, DST_ERR_STATE, "a batch of this closest stream held an invalid code: its lists are not trustworthy");
    if (s->closest == DST_CLOSEST_FOR_LOADED && s->next_ordinal + n_records - 1 > 0xFFFFFFFEull)
        return fail(ctx, DST_ERR_CAPACITY, "streamed ordinals end at 2^32-2");
    auto &sl = s->slots[(size_t)s->acquired];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // copy-in: the batch's bytes (and the caller's base counts)
    if (s->len)
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_in, sl.h_in, n_records * s->pitch, hipMemcpyHostToDevice, s->s_in));
    if (use_base_counts)
        HIP_TRY(ctx, hipMemcpyAsync(sl.d_in + counts_offset(s), sl.h_in + counts_offset(s), n_records * 16,
                                    hipMemcpyHostToDevice, s->s_in));
    HIP_TRY(ctx, hipEventRecord(sl.h2d, s->s_in));
    // compute: pack, then the batch (rows) against the loaded set (columns): streamed-major order
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_compute, sl.h2d, 0));
    int rc = pack_queue(ctx, sl.set, sl.d_in, n_records, s->len, s->pitch,
                        use_base_counts ? reinterpret_cast<const uint32_t *>(sl.d_in + counts_offset(s)) : nullptr,
                        sl.d_bad, s->s_compute, false, s->wire == DST_WIRE_NIBBLES);
    if (rc)
        return rc;
    sl.set.loaded = true;  // validity is reported by dst_stream_collect
    if (s->measure == DST_TN93 && (s->out_kind == DST_OUT_DISTANCE || s->closest >= 0) && !sl.set.have_counts) {
        HIP_TRY(ctx, launch_fill_counts(sl.set, s->s_compute));  // same stream as the kernel that reads them
        sl.set.have_counts = true;
    }
    if (s->measure == DST_TN93 && s->closest >= 0) {   // the selection finalises the tallies: the loaded set's counts too
        rc = need_counts(ctx, loaded, s->s_compute);
        if (rc)
            return rc;
    }
    const size_t bytes = s->out_bytes_per_record * n_records;
    rc = run_sets(ctx, s->measure, false, sl.set, loaded, 0, n_records, s->out_kind, sl.d_out, bytes, (void *)s->s_compute);
    if (rc)
        return rc;
    // a closest stream: the selection directly behind the batch's pair kernel, on the one compute stream
    const uint32_t *tallies = static_cast<const uint32_t *>(sl.d_out);
    if (s->closest == DST_CLOSEST_FOR_LOADED) {
        HIP_TRY(ctx, launch_nearest_stream_cols(s->measure, tallies, n_records, s->n_loaded, (uint32_t)s->next_ordinal,
                                                sl.set.counts, loaded.counts, s->nl, s->s_compute));
    } else if (s->closest == DST_CLOSEST_FOR_STREAMED && s->k_streamed) {
        HIP_TRY(ctx, launch_nearest_init(sl.nl, n_records, s->s_compute));
        HIP_TRY(ctx, launch_nearest_rows(s->measure, false, tallies, 0, s->n_loaded, 0, n_records, sl.set.counts, loaded.counts,
                                         sl.nl, s->s_compute));
    }
    HIP_TRY(ctx, hipEventRecord(sl.computed, s->s_compute));
    // copy-out
    HIP_TRY(ctx, hipStreamWaitEvent(s->s_out, sl.computed, 0));
    HIP_TRY(ctx, hipMemcpyAsync(sl.h_bad, sl.d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->s_out));
    if (s->closest < 0) {
        if (bytes)
            HIP_TRY(ctx, hipMemcpyAsync(sl.h_out, sl.d_out, bytes, hipMemcpyDeviceToHost, s->s_out));
    } else if (s->closest == DST_CLOSEST_FOR_STREAMED && s->k_streamed) {
        const size_t e = n_records * (size_t)s->k_streamed;
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.idx, sl.nl.idx, e * 4, hipMemcpyDeviceToHost, s->s_out));
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.val, sl.nl.val, e * 8, hipMemcpyDeviceToHost, s->s_out));
        HIP_TRY(ctx, hipMemcpyAsync(sl.h_nl.tal, sl.nl.tal, e * 4 * (size_t)s->W, hipMemcpyDeviceToHost, s->s_out));
    }
    HIP_TRY(ctx, hipEventRecord(sl.landed, s->s_out));
    if (s->closest == DST_CLOSEST_FOR_LOADED) {
        s->next_ordinal += n_records;
        s->submitted += n_records;
    }
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
    if (*sl.h_bad != ~0ull) {
        s->poisoned = s->closest >= 0;
        return invalid_code_error(ctx, *sl.h_bad, s->len);
    }
    *n_records = sl.n;
    *results = sl.h_out;   // (NULL for a closest stream: its results never leave the device as a matrix)
    return DST_OK;
}

int dst_stream_closest_next_index(dst_stream *s, uint64_t next)
{
    if (!s)
        return DST_ERR_ARG;
    if (s->closest != DST_CLOSEST_FOR_LOADED)
        return fail(s->ctx, DST_ERR_ARG, "not a DST_CLOSEST_FOR_LOADED stream");
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

int dst_stream_in_flight(const dst_stream *s) { return s ? (int)s->in_flight : -1; }

int dst_stream_close(dst_stream *s)
{
    destroy(s);
    return DST_OK;
}

}  // extern "C"
