/*
 * distance_hip.h — C ABI of libdistance_hip.so, the MI355X (gfx950) all-pairs genetic-distance
 * engine.  Drop-in for the hot path of benjamincjackson/distance: everything between
 * set_up()'s outputs and gather_write()'s input (src/lib.rs:269-474, 502-596), i.e. the pair
 * generator + worker pools that call `fn(&EncodedFastaRecord, &EncodedFastaRecord) -> FloatInt`
 * (src/lib.rs:477-488, call sites src/lib.rs:325 and :434).
 *
 * The reference has no FFI of its own; INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add.  Everything here is POD: plain pointers and sizes, no C++/torch types.
 *
 * Conventions
 *  - every entry point returns a dst_status (0 = ok) and never throws or aborts;
 *    dst_last_error() gives the message of the last failure on that context.
 *  - a context is bound to ONE GPU and is single-owner (not re-entrant).  One process per GPU.
 *  - the caller owns every pointer it passes; host pointers are not retained after return.
 *  - "codes" are Paradis bytes exactly as src/encoding.rs:4-41 produces them (17 valid values);
 *    any other byte is rejected by dst_upload* with DST_ERR_INVALID_CODE (the reference rejects
 *    the character earlier, in encode(), src/fastaio.rs:111-113).
 *  - canonical pair order = the reference's: square i<j row-major (src/lib.rs:511-512),
 *    rectangle i outer / j inner (src/lib.rs:560-561).  Stream mode (src/lib.rs:322-331:
 *    streamed record outer, loaded record inner) is a rectangle run with the streamed batch as
 *    the row set, because every measure is symmetric in its two records.
 */
#ifndef DISTANCE_HIP_H
#define DISTANCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DST_ABI_VERSION 3

typedef struct dst_ctx dst_ctx;

/* -m values, src/lib.rs:104-109; dispatch table of get_distance_function, src/lib.rs:477-488 */
typedef enum {
    DST_N = 0,      /* snp_consensus, src/measures.rs:28-53 (same integers as n_high, computed densely) */
    DST_N_HIGH = 1, /* snp,           src/measures.rs:14-23  */
    DST_RAW = 2,    /* raw,           src/measures.rs:56-69  */
    DST_JC69 = 3,   /* jc69,          src/measures.rs:72-77  */
    DST_K80 = 4,    /* k80,           src/measures.rs:80-113 */
    DST_TN93 = 5    /* tn93,          src/measures.rs:116-193 */
} dst_measure;

typedef enum {
    DST_OK = 0,
    DST_ERR_ARG = 1,          /* bad argument / null pointer / range */
    DST_ERR_HIP = 2,          /* a HIP runtime call failed (message has hipGetErrorString) */
    DST_ERR_INVALID_CODE = 3, /* a byte that src/encoding.rs never produces */
    DST_ERR_STATE = 4,        /* set not uploaded, widths differ (src/fastaio.rs:93-95), ... */
    DST_ERR_NOMEM = 5,
    DST_ERR_CAPACITY = 6      /* output buffer too small */
} dst_status;

/* What a run writes per pair, in canonical order:
 *  DST_OUT_DISTANCE: 8 bytes — the payload of FloatInt (src/measures.rs:5-9): int64 for n/n_high,
 *                    f64 for raw/jc69/k80/tn93 finalised ON DEVICE in the pair kernel's epilogue: raw is the
 *                    reference's bits (one correctly rounded division); jc69 / k80 / tn93 are within 1e-12 of the
 *                    reference (series logarithms and reciprocal multiplies where every logarithm's argument lies
 *                    within 2^-5 of 1, the reference's operation order with a table logarithm elsewhere), not
 *                    bit-identical: for the reference's bits take DST_OUT_TALLY + dst_finalize, for its TEXT dst_text_*.
 *  DST_OUT_TALLY:    dst_tally_width(measure) x uint32 site tallies, bit-exact integers:
 *                      n, n_high : {d}
 *                      raw, jc69 : {n, d}                        (src/measures.rs:57-66)
 *                      k80       : {count_L, ts, tv}             (src/measures.rs:81-107)
 *                      tn93      : {count_L, count_d, count_P1, count_P2} (src/measures.rs:150-175)
 *                    finalise with dst_finalize() on the host for bit-identical TSV text.
 *  DST_OUT_TALLY16:  the same tallies as uint16 (2 x width bytes per pair) for alignments shorter
 *                    than 65,536 sites: the compact form sent between GPUs; dst_finalize_device()
 *                    turns it into distances on the receiving GPU. */
typedef enum { DST_OUT_DISTANCE = 0, DST_OUT_TALLY = 1, DST_OUT_TALLY16 = 2 } dst_output;
/* OR-ed into dst_finalize_device's tally_kind: finalise in the reference's operation order with the device's table
 * logarithm (within a few ulp of the host's libm: what dst_text_* prints from) instead of the epilogue's arithmetic */
#define DST_FIN_CLOSE 0x100

/* ---- library ------------------------------------------------------------------------- */
int dst_abi_version(void);
int dst_device_count(int *count);
/* name -> dst_measure, or -1 (src/lib.rs:477-488 panics on unknown names; clap rejects first) */
int dst_measure_from_name(const char *name);
int dst_tally_width(int measure);
const char *dst_status_string(int status);
/* The measurement macros (DST_DBG_*: alternative store patterns, wave splits ... of tools/variants.sh) this library was
 * compiled with, space separated; "" for a production build.  bench.py refuses to time anything else. */
const char *dst_build_flags(void);

/* ---- context -------------------------------------------------------------------------- */
int dst_create(int device, dst_ctx **ctx);
int dst_destroy(dst_ctx *ctx);
const char *dst_last_error(const dst_ctx *ctx); /* ctx may be NULL: last dst_create failure */
/* kernel tile variant: 0 = default for the measure; see DESIGN.md "tile variants" */
int dst_set_variant(dst_ctx *ctx, int variant);
int dst_variant_count(int measure);
/* split-L factor: launches with few tiles and a long alignment (small sets, streamed batches) cut
 * the sweep over L into `ksplit` parts whose partial integer tallies are combined with atomics
 * (exact).  0 = automatic (default: launches with fewer than 1,024 tiles), 1 = never split, k > 1 = force. */
int dst_set_ksplit(dst_ctx *ctx, int ksplit);

/* DST_PATH_AUTO leaves small jobs to the dense kernels without sampling them: an upload with fewer than
 * `site_comparisons` (n^2/2 x len) ahead of it skips the consensus path's preparation, and a run below it (with no
 * reference sequence yet) goes dense.  Default 2e10 (what the dense kernels finish in ~0.1 ms); 0 makes every upload
 * prepare the lists (tests drive the small shapes of the parity suite through the fused preparation this way). */
int dst_set_prep_threshold(dst_ctx *ctx, double site_comparisons);
/* Which kernels a run uses.  Both give the same integers (tallies bit-exact, the same finalisation):
 *  DST_PATH_DENSE:     bit-plane tile kernels, work ~ pairs x L whatever the data (src/measures.rs:14-23,
 *                      56-66, 85-107, 156-175 evaluated at every site).
 *  DST_PATH_CONSENSUS: the idea of the reference's `-m n` (snp_consensus, src/measures.rs:28-53, over the
 *                      difference lists of get_differences(), src/fastaio.rs:67-75, against consensus(),
 *                      src/fastaio.rs:289-336) carried to every measure: tallies from each record's
 *                      differences to a per-site plurality sequence; work ~ pairs + the differences two
 *                      records share.  Low-diversity alignments (SARS-CoV-2-like) run output-bound.
 *                      Shapes its lists cannot index (zero-width alignments, 2^28 or more records or sites,
 *                      more than 2^31 differences in a set) run dense even when this is selected.
 *  DST_PATH_HYBRID:    consensus path for the "cold" columns, dense kernels for the hot ones (columns where more than
 *                      5 % of a sample of the records deviate from the plurality: clade-defining mutations), whose
 *                      tallies the consensus kernel adds in.  Alignments with phylogenetic structure stay fast.
 *                      Without hot columns it is the consensus path; with mostly hot columns the dense one.
 *  DST_PATH_AUTO:      (default) per launch, whichever a sampled estimate of the alignment's diversity
 *                      says is fastest. */
typedef enum { DST_PATH_AUTO = 0, DST_PATH_DENSE = 1, DST_PATH_CONSENSUS = 2, DST_PATH_HYBRID = 3 } dst_path;
int dst_set_path(dst_ctx *ctx, int path);
/* Records with long runs of N (failed amplicons, partial genomes; N adds nothing to any tally: src/measures.rs:17, 59-66,
 * 89-107, 160-175) in the set of `slot`: how many the consensus path currently treats as "run records" — their chunks
 * of 128 N sites are left out of the difference lists and every pair with such a record is corrected exactly
 * (DESIGN.md 3b'') — and how many list entries that removed.  0 when the set has none, too many (more than a third of the
 * records), or its lists were not built by the upload's fused preparation.  Diagnostic; the results do not depend on it. */
int dst_run_records(const dst_ctx *ctx, int slot, uint64_t *run_records, uint64_t *entries_removed);
/* *stored = 1 when the bit-planes of every (record, 128-site chunk) of the set are in HBM; 0 while the upload has deferred them: a
 * set prepared for the consensus path keeps, per chunk, its differences from the set's reference sequence (what that path
 * reads), and the planes of a chunk are written only if it does not fit that form — the rest is written, from the
 * reference and the differences, the first time something reads planes (a dense or hybrid run, dst_consensus,
 * dst_differences, a run against another set).  Diagnostic; the results do not depend on it. */
int dst_planes_stored(const dst_ctx *ctx, int slot, int *stored);
/* DST_PATH_DENSE, DST_PATH_CONSENSUS or DST_PATH_HYBRID: what the most recent run on this context used */
int dst_last_path(const dst_ctx *ctx);
/* Which kernel variant the most recent pair launch of this context was.  The consensus pair kernel is a family of
 * instantiations <tally family, wide, output, event waves> and three tile heights, chosen per launch from its size and the
 * sampled statistics of the column set; the dense kernels have tile variants and a split-L factor.  Diagnostic: tests
 * assert with it that a shape reached the variant it was written for; the results do not depend on it. */
typedef struct {
    int path;               /* dst_path of the launch; -1: no pair launch on this context yet */
    int measure;            /* dst_measure */
    int family;             /* the tallies accumulated: 0 {d} (n, n_high), 1 {n, d} (raw, jc69), 2 k80's, 3 tn93's */
    int out_kind;           /* dst_output */
    int wide;               /* consensus / hybrid: 1 = one 32-bit word per tally (65,536 sites or more) */
    int square;             /* 1: square job (dst_run_square), 0: rectangle */
    int event_waves;        /* consensus / hybrid: event waves of a workgroup's 8 as instantiated (8: no roles); 0: dense */
    int heavy_events;       /* consensus / hybrid: 0 the output's default split, 1 four event waves, 2 no roles */
    uint32_t rows_per_tile; /* consensus / hybrid: 8, 16 or 32; dense: rows of the tile variant */
    uint32_t tile_cols;     /* consensus / hybrid: records of a column panel; dense: columns of the tile variant */
    uint64_t tiles;         /* workgroups of the pair launch (dst_plan_consensus_launch: the estimate the tile height is chosen by) */
    int hot;                /* 1: hot-column tallies from the dense kernels were added (hybrid) */
    int run_records;        /* 1: run-record corrections were applied (dst_run_records) */
    int variant;            /* dense: the tile variant used, as its number among the measure's (0 is the default's own) */
    uint32_t ksplit;        /* dense: the split-L factor used, also when dst_set_ksplit(0) leaves it to the library; else 0 */
    uint64_t pairs;         /* pairs of the launch */
    double events_per_pair; /* consensus / hybrid: the sample's estimates the choice was made from: events per pair, */
    double list_length;     /*   mean list entries per record, */
    double run_adds;        /*   and the run records' adds per pair */
} dst_launch_info;
int dst_last_launch(const dst_ctx *ctx, dst_launch_info *info);
/* The choice itself, for any shape (pure host code, no GPU needed): what a consensus-path launch of n_rows_in_launch rows
 * against n_cols column records (total_pairs pairs) with these statistics gets.  hot != 0: a hybrid launch; run_adds > 0:
 * a square launch over a set with run records (2 x run records / records).  dst_run_square / dst_run_rect decide by this
 * function.  DST_ERR_ARG: an unknown measure or output, DST_OUT_TALLY16 with wide, a negative or NaN figure. */
int dst_plan_consensus_launch(int measure, int out_kind, int wide, int square, uint64_t n_rows_in_launch, uint64_t n_cols,
                              uint64_t total_pairs, double events_per_pair, double list_length, double run_adds, int hot,
                              dst_launch_info *info);

/* ---- input: replaces Setup.loaded_fastas[slot] (src/lib.rs:133-144) --------------------- */
/* codes: row-major n x len Paradis bytes, rows row_stride bytes apart (>= len).
 * base_counts: n x 4 {A, T, G, C} per-record counts for tn93 (src/fastaio.rs:53-66, or the
 * streamed variant src/fastaio.rs:136-142), or NULL to have them counted on device by code.
 * slot is 0 or 1.  Both slots must have the same len (src/fastaio.rs:206-208). */
int dst_upload(dst_ctx *ctx, int slot, const uint8_t *codes, size_t n, size_t len,
               size_t row_stride, const uint32_t *base_counts);
/* same with codes / base_counts already in this GPU's memory; `stream` is a hipStream_t (NULL =
 * the context's own stream).  Asynchronous on that stream except for the validity check. */
int dst_upload_device(dst_ctx *ctx, int slot, const void *d_codes, size_t n, size_t len,
                      size_t row_stride, const uint32_t *d_base_counts, void *stream);
int dst_set_info(const dst_ctx *ctx, int slot, size_t *n, size_t *len);
/* per-record {A,T,G,C} counts the device holds for `slot` (n x 4), copied to host */
int dst_get_base_counts(dst_ctx *ctx, int slot, uint32_t *counts);

/* ---- per-alignment precompute of `-m n` (src/lib.rs:223-231) ------------------------------ */
/* consensus(), src/fastaio.rs:289-336, computed on the device: per site the plurality of A, G, C, T over
 * every record of slot 0 (and of slot 1 too when both_slots != 0 and it is loaded — the reference walks every
 * loaded file), every other code counted as A, ties to the first of A, G, C, T.  cons receives len codes
 * (136 / 72 / 40 / 24). */
int dst_consensus(dst_ctx *ctx, int both_slots, uint8_t *cons, size_t cap);
/* get_differences(), src/fastaio.rs:67-75, for every record of `slot` against `other` (len codes, host
 * memory; normally the consensus): ascending sites with seq[i] < 240 && seq[i] != other[i].  CSR output:
 * offsets has n + 1 entries, sites holds offsets[n] entries.  Pass sites == NULL to get offsets / *total only;
 * DST_ERR_CAPACITY when cap_sites < *total. */
int dst_differences(dst_ctx *ctx, int slot, const uint8_t *other, size_t len, uint64_t *offsets, uint32_t *sites,
                    size_t cap_sites, uint64_t *total);

/* ---- canonical order helpers (src/lib.rs:502-596) --------------------------------------- */
uint64_t dst_square_pairs(uint64_t n);                   /* n(n-1)/2 */
uint64_t dst_square_row_start(uint64_t n, uint64_t i);   /* index of pair (i, i+1) */
/* cut rows [0, n) into `parts` contiguous ranges of near-equal PAIR count (square) — the
 * multi-GPU partition.  bounds has parts+1 entries, bounds[0]=0, bounds[parts]=n. */
int dst_partition_square(uint64_t n, int parts, uint64_t *bounds);
int dst_partition_rect(uint64_t n_rows, int parts, uint64_t *bounds);

/* ---- run: replaces generate_pairs_* + the worker pools (src/lib.rs:367-474, 269-365) ----- */
/* All pairs (i, j), row_begin <= i < row_end, i < j < n of slot 0, canonical order, written to
 * d_out (device memory) starting with pair (row_begin, row_begin+1).  Asynchronous on `stream`
 * (hipStream_t; NULL = context stream, then the call synchronises before returning).
 * A stream of the caller's, here and in every other call that takes one, is used only during that call: the
 * context keeps events of its own behind the work it queued, never the handle, so the caller may destroy the
 * stream once the work queued on it has completed (and the context may outlive it). */
int dst_run_square(dst_ctx *ctx, int measure, uint64_t row_begin, uint64_t row_end, int out_kind,
                   void *d_out, size_t out_capacity_bytes, void *stream);
/* All pairs (i, j), i in rows [row_begin,row_end) of row_slot, j over every record of col_slot;
 * out[(i-row_begin) * n_col + j].  Two loaded files: row_slot=0, col_slot=1 (src/lib.rs:432-433).
 * Stream mode: row_slot = the streamed batch, col_slot = the loaded set (src/lib.rs:322-331). */
int dst_run_rect(dst_ctx *ctx, int measure, int row_slot, int col_slot, uint64_t row_begin,
                 uint64_t row_end, int out_kind, void *d_out, size_t out_capacity_bytes,
                 void *stream);
/* Tallies (DST_OUT_TALLY or DST_OUT_TALLY16 layout, canonical order of rows [row_begin,row_end))
 * that are already in this GPU's memory -> the DST_OUT_DISTANCE payload in d_out, with the same
 * device arithmetic as a direct DST_OUT_DISTANCE run (bitwise the same values; tally_kind | DST_FIN_CLOSE: the text
 * path's arithmetic instead).  The two sets must
 * be uploaded on this context (tn93 reads their base counts).  Multi-GPU: rank 0 finalises the
 * compact tallies it gathered from the other ranks. */
int dst_finalize_device(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                        uint64_t row_begin, uint64_t row_end, int tally_kind, const void *d_tallies,
                        void *d_out, size_t out_capacity_bytes, void *stream);
/* host-buffer forms: run + copy back (h_out is ordinary or pinned host memory) */
int dst_run_square_host(dst_ctx *ctx, int measure, uint64_t row_begin, uint64_t row_end,
                        int out_kind, void *h_out, size_t out_capacity_bytes);
int dst_run_rect_host(dst_ctx *ctx, int measure, int row_slot, int col_slot, uint64_t row_begin,
                      uint64_t row_end, int out_kind, void *h_out, size_t out_capacity_bytes);
/* ---- stream mode: replaces stream()'s worker pool (src/lib.rs:269-365) ----------------------- */
/* Batches of streamed records (rows) against the loaded set of slot 0 (columns), results in the reference's
 * streamed-major order [streamed record][loaded record] (src/lib.rs:322-331), through a ring of `depth` slots
 * (2..16) on three HIP streams: while batch k is compared, batch k+1 crosses PCIe from page-locked memory and
 * batch k-1's results travel back.  out_kind: DST_OUT_DISTANCE or DST_OUT_TALLY.  max_records: records per batch
 * (stream_fasta()'s batchsize, src/fastaio.rs:215-286).  The width is slot 0's; slot 0 must stay loaded and
 * unchanged while the stream is open.  One owner thread, like the context. */
typedef struct dst_stream dst_stream;
int dst_stream_open(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, dst_stream **stream);
/* The same with a choice of what crosses the host link (which bounds a streamed job: 64 records of 5 Mbp are 320 MB):
 *  DST_WIRE_CODES    Paradis bytes, one per site (dst_stream_open);
 *  DST_WIRE_NIBBLES  the HIGH NIBBLE of each code — all that any measure reads — two sites per byte, site 2k in the low
 *                    four bits of byte k, site 2k + 1 in the high four; a row's unused trailing nibble is ignored.  The
 *                    host writes encoding_array()[c] >> 4 (src/encoding.rs:4-41) instead of the code; 0 is not a code
 *                    (DST_ERR_INVALID_CODE at collect).  Half the bytes, same results; base counts by code
 *                    (use_base_counts == 0) are counted from the nibbles on the device like from the codes. */
typedef enum { DST_WIRE_CODES = 0, DST_WIRE_NIBBLES = 1 } dst_wire;
int dst_stream_open_wire(dst_ctx *ctx, int measure, int out_kind, size_t max_records, int depth, int wire, dst_stream **stream);
/* The page-locked input buffer of the next batch: rows *pitch bytes apart (>= width — half of it, rounded up, for
 * DST_WIRE_NIBBLES — and a multiple of 128), room for max_records; encode straight into it.  *base_counts (may be NULL): max_records x 4 {A,T,G,C} for tn93
 * (encode_count_bases(), src/fastaio.rs:120-145).  DST_ERR_STATE when every slot is in flight. */
int dst_stream_acquire(dst_stream *stream, uint8_t **codes, size_t *pitch, uint32_t **base_counts);
/* Queue the acquired buffer holding n_records records: H2D, pack, compare, D2H.  Returns without waiting.
 * use_base_counts != 0: tn93 uses the caller's counts (streamed records: upper-case letters only,
 * src/fastaio.rs:136-142), else they are counted on the device by code. */
int dst_stream_submit(dst_stream *stream, size_t n_records, int use_base_counts);
/* Wait for the OLDEST submitted batch and hand out its results (page-locked, library-owned, valid until the next
 * dst_stream_submit): n_records x (records of slot 0) x the per-pair payload of out_kind.
 * DST_ERR_INVALID_CODE when the batch held a byte src/encoding.rs never produces. */
int dst_stream_collect(dst_stream *stream, size_t *n_records, const void **results);
int dst_stream_in_flight(const dst_stream *stream);   /* submitted, not yet collected */
int dst_stream_close(dst_stream *stream);
/* ---- closest records in stream mode ------------------------------------------------------------ */
/* A stream that keeps, instead of the result matrix, the k nearest records per record (1 <= k <= 256): what
 * `gofasta closest` answers for a database that does not fit in memory.  A closest stream IS a dst_stream:
 * dst_stream_acquire / _submit / _collect / _in_flight / _close work on it as on any other, with both wire formats, the
 * caller's base counts and the ring of `depth` slots.  The differences: the result matrix is never copied to the host
 * (dst_stream_collect returns *results = NULL, but still waits for the batch and still reports DST_ERR_INVALID_CODE);
 * after a batch with an invalid code the lists are not trustworthy, and every later dst_stream_submit,
 * dst_stream_closest_result and dst_stream_closest_batch on that stream is DST_ERR_STATE.
 * The value of the pair (streamed s, loaded i) is the payload the same stream would deliver for it as DST_OUT_DISTANCE,
 * bit for bit (tn93: the streamed record's base counts as q, the loaded record's as t; the same use_base_counts); its
 * tallies are the plain stream's DST_OUT_TALLY words; its key is dst_nearest's sort key (below: int64 v ^ 2^63; f64 NaN
 * after +inf, -0.0 as +0.0).
 *  DST_CLOSEST_FOR_LOADED    every loaded record i keeps, over the whole life of the stream, its k smallest entries in the
 *                            order (key, streamed ordinal); a record's ordinal is the number of records submitted before it
 *                            (plus what dst_stream_closest_next_index skipped).  The order is strict, so the answer does not
 *                            depend on how the stream is cut into batches.  Ordinals are uint32 and 2^32-1 is the lists'
 *                            sentinel: a submit whose last ordinal would pass 2^32-2 is DST_ERR_CAPACITY and changes nothing.
 *  DST_CLOSEST_FOR_STREAMED  every streamed record gets its k nearest loaded records, in the order (key, loaded index):
 *                            dst_nearest's rectangle form with the batch as rows.  The lists are per batch.
 * Open: an unknown measure, side or wire, k outside 1..256, max_records == 0, depth outside 2..16: DST_ERR_ARG; slot 0 not
 * loaded: DST_ERR_STATE.  The calls below on a plain stream, or on a closest stream of the other side, are DST_ERR_ARG.
 * Single GPU.  All selection launches of a FOR_LOADED stream write the same lists, so they follow one another on the
 * stream's compute stream, each directly behind its batch's pair kernel. */
typedef enum { DST_CLOSEST_FOR_LOADED = 0, DST_CLOSEST_FOR_STREAMED = 1 } dst_closest_side;
int dst_stream_open_closest(dst_ctx *ctx, int measure, uint32_t k, int side, size_t max_records, int depth, int wire,
                            dst_stream **stream);
/* FOR_LOADED (and window-closest streams, below) only.  Sets the ordinal of the next submitted record (numbering the shards of one database).  Allowed only with
 * nothing in flight (else DST_ERR_STATE) and with the current ordinal <= next <= 2^32-1 (else DST_ERR_ARG). */
int dst_stream_closest_next_index(dst_stream *stream, uint64_t next);
/* FOR_LOADED only.  A snapshot of the lists: n_loaded x k_used entries, row-major by loaded record, dense, ascending;
 * k_used = min(k, records submitted so far) - the records, not the ordinal, when ordinals were skipped.  index: the
 * streamed ordinals (required); values: DST_OUT_DISTANCE payloads, tallies: dst_tally_width(measure) words per entry, either
 * may be NULL (host memory, as dst_nearest's).  Needs dst_stream_in_flight() == 0, else DST_ERR_STATE; cap_entries below
 * n_loaded x k_used: DST_ERR_CAPACITY.  Streaming may go on afterwards, and the call may be repeated. */
int dst_stream_closest_result(dst_stream *stream, uint32_t *index, uint32_t *tallies, void *values, size_t cap_entries,
                              uint32_t *k_used);
/* FOR_STREAMED only.  After dst_stream_collect: the collected batch's lists, n_records x k_used entries, dense,
 * k_used = min(k, n_loaded), in page-locked, library-owned memory that is valid until the next dst_stream_submit.  index is
 * required; tallies and values may be NULL.  DST_ERR_STATE when no batch has been collected. */
int dst_stream_closest_batch(dst_stream *stream, const uint32_t **index, const uint32_t **tallies, const void **values,
                             uint32_t *k_used);
/* ---- thresholded pairs in stream mode ------------------------------------------------------------ */
/* A stream that hands back, instead of the result matrix, the pairs within a threshold: which records of a database that
 * does not fit in memory are within T of mine, and at what distance.  A links stream IS a dst_stream: dst_stream_acquire /
 * _submit / _collect / _in_flight / _close work on it as on a closest stream, with both wire formats, the caller's base
 * counts and the ring of `depth` slots (dst_stream_collect returns *results = NULL, but still waits for the batch and still
 * reports DST_ERR_INVALID_CODE).
 * Definition.  The pair (streamed s, loaded i) is a link when its payload v - what the same stream would deliver for the
 * pair as DST_OUT_DISTANCE, bit for bit (tn93: the streamed record's base counts as q, the loaded record's as t; the same
 * use_base_counts) - satisfies dst_links' rule against `threshold`: n / n_high: v <= floor(threshold), the floor clamped to
 * the int64 range (a floor below -2^63: nothing links, no compaction is launched); f64 measures: key(v) <= key(threshold)
 * with dst_nearest's sort key, i.e. IEEE v <= threshold, except that NaN never links, -0.0 links wherever +0.0 does and
 * threshold = +inf links every non-NaN value.
 * A batch's links come in the stream's own order, streamed record outer, loaded record inner (the rectangle's canonical
 * order with the batch as rows).  streamed[e] is the record's index WITHIN THE BATCH, 0 .. n_records - 1 (the caller numbers
 * its stream); loaded[e] is the record of slot 0; values (DST_LINKS_VALUES) are bitwise the plain stream's DST_OUT_DISTANCE
 * payloads and tallies (DST_LINKS_TALLIES) bitwise its DST_OUT_TALLY words, dst_tally_width(measure) per link.  The result
 * depends neither on the kernel path, nor on window_links, nor - once the batch's first ordinal is added to `streamed` - on
 * how the stream is cut into batches.  A links stream keeps nothing across batches: a batch with an invalid code makes its
 * dst_stream_collect return DST_ERR_INVALID_CODE and its dst_stream_links_batch DST_ERR_STATE; later batches are unaffected.
 * Windows.  window = window_links (0: DST_STREAM_LINKS_WINDOW), capped at max_records x n_loaded, at least 1 and at most
 * DST_LINKS_CHUNK.  Window 0 of a batch is written on the compute stream at submit, directly behind the batch's pair kernel,
 * count and scan, so the usual sparse batch costs no launch after collect; any other window is one write pass over the
 * batch's matrix, which stays on the device until the slot is submitted again.  Per batch the bad-code word, the batch's
 * link total and the links present in the window cross the host link: never the window's capacity, never the matrix.
 * Open: a NULL ctx or stream pointer, an unknown measure or wire, a NaN threshold, bits in `what` other than
 * DST_LINKS_VALUES | DST_LINKS_TALLIES, window_links > DST_LINKS_CHUNK, max_records == 0, depth outside 2..16, a loaded set
 * of 2^32-1 records or more: DST_ERR_ARG; slot 0 not loaded: DST_ERR_STATE.  Submit: DST_ERR_STATE when the loaded set's
 * record count changed while the stream was open.  Single GPU. */
#define DST_STREAM_LINKS_WINDOW (1u << 20)   /* default most links of one window */
int dst_stream_open_links(dst_ctx *ctx, int measure, double threshold, int what, uint64_t window_links,
                          size_t max_records, int depth, int wire, dst_stream **stream);
/* Valid from a successful dst_stream_collect until the next dst_stream_submit: links [first_link, min(first_link + window,
 * *batch_links)) of the collected batch, *n_links of them, in page-locked, library-owned memory that is valid until the
 * next call of this function or of dst_stream_submit.  first_link may be anything <= *batch_links (== gives *n_links = 0;
 * above: DST_ERR_ARG, with *batch_links set).  The window the buffer already holds (first_link 0 after collect) costs
 * nothing; any other is written now and the call waits for it.  values / tallies may be NULL; what was not asked for in
 * `what` comes back NULL; what == 0 still delivers streamed and loaded.  On a plain or closest stream, or with a NULL
 * n_links, batch_links, streamed or loaded: DST_ERR_ARG (as are the closest calls on a links stream); no collected
 * batch: DST_ERR_STATE. */
int dst_stream_links_batch(dst_stream *stream, uint64_t first_link, uint64_t *n_links, uint64_t *batch_links,
                           const uint32_t **streamed, const uint32_t **loaded, const void **values,
                           const uint32_t **tallies);
/* A diagnostic, like dst_text_stats: the links of every batch collected so far, and how many windows were written after
 * collect.  Either pointer may be NULL.  DST_ERR_ARG on a NULL, plain or closest stream. */
int dst_stream_links_stats(const dst_stream *stream, uint64_t *links, uint64_t *late_windows);
/* ---- nearest records per window in stream mode ---------------------------------------------------- */
/* A window-closest stream: for every (loaded record of slot 0, window) the k nearest STREAMED records inside that window,
 * kept over the whole life of the stream - the recombination scan of dst_nearest_windows against a panel that does not fit
 * on the GPU.  Few loaded queries against a long stream; the per-streamed-record side is not offered.
 * Definition, fixed to the bit.  Let S be the set that holds every record submitted so far, in ordinal order; a record's
 * ordinal is the number of records submitted before it, plus whatever dst_stream_closest_next_index skipped.  The result is
 * what dst_nearest_windows(square = 0, rows = slot 0, cols = S, every row, the same windows, the same k) returns, with
 * `index` holding the ordinals: a candidate's value is dst_run_windows' DST_OUT_DISTANCE payload of the pair (loaded i,
 * streamed s) in window w, its tallies are that entry's DST_OUT_TALLY words, tn93 takes per-window base counts COUNTED BY
 * CODE, the loaded record's and the streamed record's in that order, and the order is ascending (dst_nearest's key,
 * ordinal): a strict total order.  So the answer does not depend on how the stream is cut into batches, on depth, on the
 * wire format or on max_entries; an empty window lists the first k_used ordinals; and k_used = min(k, records submitted),
 * the records and not the ordinal.  use_base_counts of dst_stream_submit is IGNORED on this stream: per-window counts cannot
 * come from the caller.
 * It IS a dst_stream: dst_stream_acquire / _submit / _collect / _in_flight / _close work as on a closest stream
 * (dst_stream_collect returns *results = NULL, still waits for the batch and still reports DST_ERR_INVALID_CODE; after a
 * batch with an invalid code every later dst_stream_submit and dst_stream_window_closest_result is DST_ERR_STATE, as for
 * DST_CLOSEST_FOR_LOADED).  Ordinals are uint32 with 2^32-1 as the sentinel: a submit whose last ordinal would pass 2^32-2
 * is DST_ERR_CAPACITY and changes nothing; dst_stream_closest_next_index works on this stream with its rules.  The other
 * closest and links calls on it are DST_ERR_ARG, as is dst_stream_window_closest_result on any other stream.
 * Open.  windows as dst_run_windows' (half-open, may overlap, repeat, be empty, come in any order), 1 <= n_windows <=
 * DST_WINDOWS_MAX.  max_entries: the most (loaded record x window x streamed record) tallies of one device range, 0: 2^25;
 * a batch is cut into (rows x windows) ranges by dst_nearest_windows' rule (at least one (row, window) of max_records
 * records), swept and merged range by range.  Errors, in this order: DST_ERR_ARG for a NULL ctx or stream pointer, an unknown
 * measure or wire, k outside 1..256, n_windows 0 or above DST_WINDOWS_MAX, a NULL window array, max_records == 0, depth
 * outside 2..16; DST_ERR_STATE for slot 0 not loaded or from dst_upload_shared; DST_ERR_ARG for a bad window (the message
 * names the first), len >= 2^32, a loaded set of 2^32-1 records or more, n_loaded x n_windows above 2^31 lists;
 * DST_ERR_NOMEM with the byte count.  Submit: DST_ERR_STATE when the loaded set's record count or width changed.
 * The stream owns its window table, its per-window count tables (tn93: the loaded set's, built once at open, and one
 * batch's), its lists and one tally scratch - not the context's - so dst_run_windows, dst_nearest_windows or any other call
 * on the context between two submits does not disturb it.  The loaded set's deferred planes are written at open.  Per
 * submit, on the compute stream behind the pack: the batch's per-window counts (tn93), then per range the window sweep
 * (rows = loaded, columns = the batch) and the merge, one wave per list.  No pair kernel, no matrix.  Single GPU. */
int dst_stream_open_window_closest(dst_ctx *ctx, int measure, uint32_t k,
                                   const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                                   uint64_t max_entries, size_t max_records, int depth, int wire, dst_stream **stream);
/* A snapshot of the lists (host memory): entry (i * n_windows + w) * k_used + e, e ascending, as dst_nearest_windows lays
 * them out.  index: the streamed ordinals (required); tallies: dst_tally_width(measure) words per entry, values: the 8-byte
 * payloads, col_counts: 4 uint32 {A,T,G,C} per entry, the listed streamed record's counts inside window w, by code - with
 * tallies and dst_window_base_counts(slot 0) what dst_finalize needs for the reference's bits, the batch being gone; any
 * of the three may be NULL.  col_counts is tn93's: non-NULL with another measure is DST_ERR_ARG.  Needs
 * dst_stream_in_flight() == 0, else DST_ERR_STATE; cap_entries below n_loaded * n_windows * k_used: DST_ERR_CAPACITY with
 * *k_used set.  The call may be repeated, and streaming may go on afterwards. */
int dst_stream_window_closest_result(dst_stream *stream, uint32_t *index, uint32_t *tallies, void *values,
                                     uint32_t *col_counts, size_t cap_entries, uint32_t *k_used);

/* ---- multi-GPU: the gather of the result slabs (one process per GPU, RCCL over xGMI) --------- */
/* The pair space shards by contiguous canonical ranges (dst_partition_square / dst_partition_rect): every rank
 * uploads the whole set, runs its own row range, and the only exchange is this gather into ONE rank's buffer
 * — what gather_write consumes (src/lib.rs:612-644).  Grouped ncclSend / ncclRecv straight from each rank's slab
 * into its place in the root's buffer (peer -> root on all xGMI links at once; no ring, no staging).  RCCL is
 * loaded on first use (librccl.so.1); single-GPU hosts never touch it.
 * Bootstrap: rank 0 calls dst_comm_unique_id and hands the DST_COMM_ID_BYTES bytes to the other ranks by whatever
 * its launcher offers (environment, file, MPI ...); then every rank calls dst_comm_create (collective). */
#define DST_COMM_ID_BYTES 128
typedef struct dst_comm dst_comm;
int dst_comm_unique_id(uint8_t *id, size_t cap);
int dst_comm_create(dst_ctx *ctx, const uint8_t *id, int rank, int world, dst_comm **comm);
/* A communicator over the caller's own transport (MPI, a test harness): `allgather` must take `bytes_per_rank` bytes at
 * d_send on every rank and leave rank r's at d_recv + r * bytes_per_rank on every rank (device memory), ordered after
 * the work already queued on `stream` (hipStream_t) and visible to work queued on it afterwards; 0 = ok.  Serves
 * dst_upload_shared; dst_gather_slabs needs an RCCL communicator. */
typedef int (*dst_allgather_fn)(void *user, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
int dst_comm_create_custom(dst_ctx *ctx, int rank, int world, dst_allgather_fn allgather, void *user, dst_comm **comm);
int dst_comm_destroy(dst_comm *comm);
int dst_comm_info(const dst_comm *comm, int *rank, int *world);
/* Collective.  byte_offsets / byte_sizes have `world` entries and are the same on every rank: rank r contributes
 * byte_sizes[r] bytes from its d_local, which land at d_full + byte_offsets[r] on `root` (d_full may be NULL on
 * the other ranks; the root's own slab is copied only if it is not already in place).  Any payload: f64 / int64
 * results, or DST_OUT_TALLY16 tallies that the root then finalises with dst_finalize_device.  A rank's range may
 * be sent in several calls (sub-slabs): the transfer of sub-slab k runs on `stream` behind what is already queued
 * there, so the next dst_run_square on another stream overlaps it.  Asynchronous on `stream` (hipStream_t;
 * NULL = the context's stream, then the call waits). */
int dst_gather_slabs(dst_comm *comm, const void *d_local, void *d_full, const uint64_t *byte_offsets,
                     const uint64_t *byte_sizes, int root, void *stream);

/* ---- multi-GPU: the preparation of a loaded set shared out over the ranks ------------------------------------ */
/* Collective form of dst_upload_device for slot 0 against itself (one file, the square job): instead of every rank
 * packing and indexing the whole set before it computes its row range — the reference's workers all read the ONE
 * prepared copy of loaded_fastas, src/lib.rs:413-458, 219-242 — rank k packs and lists records
 * [begin, end) = dst_shared_range(n, k, world) only, one all-gather brings every rank's difference lists (and base
 * counts, with_counts != 0: needed by tn93) to every rank, and the site tables and per-record constants are built from the
 * lists locally.  d_codes is the WHOLE n x len matrix in this GPU's memory (the call reads the rank's own records and the
 * 512 records every rank samples the reference sequence from).  Afterwards dst_run_square / dst_text_square work for any
 * row range on the consensus path; the dense and hybrid kernels, dst_consensus and dst_differences need every record's
 * planes and refuse such a set (DST_ERR_STATE).  When the lists cannot serve (a context forced dense, a set too
 * diverse, hot columns, lists larger than the exchange blocks — every rank reads that from the same figures) the call
 * IS dst_upload_device on every rank.  Every rank must pass the same n, len, with_counts, the same data and hold the
 * same dst_set_path / dst_set_prep_threshold settings.  Synchronous like dst_upload_device (validity check). */
int dst_upload_shared(dst_comm *comm, int slot, const void *d_codes, size_t n, size_t len, size_t row_stride,
                      int with_counts, void *stream);
/* the records rank `rank` of `world` prepares (pure host code) */
int dst_shared_range(uint64_t n, int rank, int world, uint64_t *begin, uint64_t *end);
/* The exchange block of one rank for blocks of `entries` list entries, in 32-bit words (pure host code; documentation
 * and tests — dst_upload_shared sizes its blocks itself): layout = {records per rank, offset of the list lengths, of the
 * base counts (4 per record), of the entries, entry capacity (rounded up to 4), words per block}.  Words 0..3 of a block:
 * entries in it, 1 if they did not fit, the first invalid byte's index (64 bits, ~0: none). */
int dst_shared_block_layout(uint64_t n, int world, uint32_t entries, uint32_t layout[6]);
/* how dst_upload_shared went on this context so far: uploads that were shared, uploads that fell back to the replicated
 * form, entries of the largest exchange block of the last one (any pointer may be NULL) */
int dst_shared_stats(const dst_ctx *ctx, int slot, uint64_t *shared_uploads, uint64_t *fallbacks, uint64_t *block_entries);

/* In-order sink (the shape of gather_write's input, src/lib.rs:612-644): the run is cut into row
 * slabs of at most max_pairs pairs (>= one row each) and `sink` is called once per slab, strictly
 * in canonical order, on the calling thread, with the slab's results in library-owned pinned host
 * memory that is valid only during the call.  While the sink works on slab k the GPU already computes
 * slab k+1 and its copy back is in flight.  A non-zero return from the sink stops the run
 * (DST_ERR_STATE, message "stopped by sink").  square != 0: slot 0 against itself (row_slot/col_slot
 * ignored). */
typedef int (*dst_slab_sink)(void *user, uint64_t first_pair, uint64_t n_pairs, uint64_t row_begin,
                             uint64_t row_end, const void *data);
int dst_run_slabs(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, int out_kind,
                  uint64_t max_pairs, dst_slab_sink sink, void *user);
/* ---- k nearest records ------------------------------------------------------------------------ */
/* For every record of the row set, the k records with the smallest distance, computed next to the values on the GPU
 * (the full result of a large alignment is tens of GB of text; placement, outbreak context and duplicate searches want a
 * few neighbours per record).
 *  square != 0: one set (slot 0; row_slot / col_slot ignored), record i against every j != i; identical sequences stay
 *               (distance 0 is a neighbour).  Candidates per row: n - 1.
 *  square == 0: every record of row_slot against every record of col_slot, none excluded; row_slot == col_slot is
 *               DST_ERR_ARG (use the square form).  Candidates per row: n of col_slot.
 * Order: ascending (key, column record), key from the pair's DST_OUT_DISTANCE payload v:
 *   n / n_high (int64):  key = (uint64)v ^ 2^63
 *   f64:                 NaN -> key ~0 (after +inf; NaNs equal to each other), -0.0 -> the key of +0.0, any other value
 *                        the order-preserving flip (v >= 0: bits | 2^63, v < 0: ~bits)
 * a strict total order, so the k smallest and their order are unique whatever the slabs.  Square results are those of
 * the canonical pair (min(i, j), max(i, j)): the value and tallies of the line a full run prints for it (tn93: base
 * counts in that order).  *k_used = min(k, candidates per row); 1 <= k <= 256, else DST_ERR_ARG; a square set of fewer
 * than 2 records gives DST_OK with *k_used = 0.  Outputs (host memory, row-major by row record, k_used entries each):
 *   index    n_rows x k_used column-record indices (required)
 *   tallies  n_rows x k_used x dst_tally_width(measure) DST_OUT_TALLY words, or NULL (dst_finalize -> the reference's bits)
 *   values   n_rows x k_used DST_OUT_DISTANCE payloads (the key's source), or NULL
 * cap_entries: room for n_rows x k_used entries in each non-NULL buffer, else DST_ERR_CAPACITY.  DST_ERR_STATE: a set is
 * not uploaded or the widths differ.  Synchronous on the context's stream.  The pairs are computed once (square: the
 * triangle), in row slabs of at most 2^25 pairs whose tallies are merged into device-resident lists n_rows x k.
 * Single GPU, loaded sets only (stream mode: dst_stream_open_closest). */
int dst_nearest(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint32_t k, uint32_t *index,
                uint32_t *tallies, void *values, size_t cap_entries, uint32_t *k_used);
/* ---- single-linkage clusters ------------------------------------------------------------------- */
/* Which records are linked within `threshold` differences (transmission clusters, duplicate groups at 0), computed next
 * to the values on the GPU: one label per record, never a pair list.  One set (slot 0, n records).  Records i < j are
 * linked when the pair's DST_OUT_DISTANCE payload v (the value dst_run_square returns, bit-identical on every path)
 * satisfies v <= threshold:
 *   n / n_high (int64):  as real numbers, v <= floor(threshold) (clamped to the int64 range; below -2^63 nothing links)
 *   f64:                 IEEE v <= threshold, decided on dst_nearest's sort key: NaN never links, -0.0 links wherever
 *                        +0.0 does, +inf links every pair whose value is not NaN
 * A cluster is a connected component of the links; label[i] = the smallest record index in i's cluster, so the result is
 * unique whatever order the pairs are met in.  jc69 / k80 / tn93 payloads are the pair kernels' series form, within 2^-44
 * (jc69, k80) or 2^-42 (tn93) of the exact value relatively (measured <= 3.4e-14), not bitwise the reference's: a pair whose value lies that close to the threshold can be decided
 * differently from a CPU computation.  raw, n and n_high are exact.
 *   threshold   any non-NaN double (NaN: DST_ERR_ARG)
 *   max_pairs   0: the default slab bound (2^25 pairs); else the most pairs of one row slab (at least one row per slab),
 *               as in dst_run_slabs.  The result does not depend on it.
 *   label       n labels (host memory, required); cap: its room in entries, below n DST_ERR_CAPACITY
 *   n_clusters  the number of clusters, or NULL
 *   links       the number of linked pairs i < j, exact, or NULL
 * n < 2: the trivial labels and 0 links; n >= 2^32-1: DST_ERR_ARG.  DST_ERR_STATE: slot 0 is not uploaded; DST_ERR_ARG:
 * an unknown measure or a NULL label.  Synchronous on the context's stream.  The pairs are computed once (the triangle),
 * in row slabs whose payloads a lock-free union-find on the device consumes.  Single GPU, loaded set only (not dst_stream). */
int dst_clusters(dst_ctx *ctx, int measure, double threshold, uint64_t max_pairs, uint32_t *label, size_t cap,
                 uint64_t *n_clusters, uint64_t *links);
/* ---- greedy representatives -------------------------------------------------------------------- */
/* A subset in which no two records are within `threshold` of each other, and for every other record the kept record that
 * stands for it (dereplication, downsampling before a tree; greedy incremental clustering): the only grouping here with
 * a guaranteed radius, where single linkage chains.  One set (slot 0, n records, input order 0..n-1).
 *   link             records i < j are linked when the pair's DST_OUT_DISTANCE payload v satisfies dst_clusters' rule
 *                    against T = threshold: n / n_high v <= floor(T) (clamped to the int64 range; below -2^63 nothing
 *                    links); f64 measures on dst_nearest's sort key: NaN never links, -0.0 links wherever +0.0 does, +inf
 *                    links every pair whose value is not NaN
 *   representatives  record j is a representative iff no representative i < j is linked to j: the lexicographically first
 *                    maximal independent set of the dst_links(T) graph, what a sequential pass over the records in input
 *                    order builds.  It is unique, and depends neither on the kernel path nor on max_pairs.
 *   rep        n entries (host memory, required): rep[j] = j for a representative, otherwise the smallest representative
 *              linked to j, which is always < j
 *   values     n DST_OUT_DISTANCE payloads (int64 for n / n_high, else f64), or NULL: for a member the payload of the pair
 *              (rep[j], j), bitwise what dst_run_square returns for it; for a representative all-zero bits
 *   tallies    n x dst_tally_width(measure) DST_OUT_TALLY words, or NULL: for a member the pair's words (tn93 base counts
 *              in (rep[j], j) order; dst_finalize -> the reference's bits); for a representative all-zero words
 *   cap        the room of every non-NULL array in entries, below n DST_ERR_CAPACITY
 *   n_representatives   the number of representatives, or NULL
 *   threshold, max_pairs   as in dst_clusters
 * Consequences: no two representatives are linked; every member is linked to its rep[j] and to no smaller representative;
 * record 0 is always a representative; every member lies in the dst_clusters(T) cluster of its representative; the
 * smallest record of every dst_clusters(T) cluster is a representative; *n_representatives >= the number of clusters.
 * Distance 0 is not transitive under ambiguity codes, so even T = 0 can keep two representatives in one cluster.
 * n < 2: the trivial answer; a threshold below which nothing links: every record its own representative; neither runs a
 * slab.  The checks and messages are dst_clusters': DST_ERR_ARG for a NULL ctx or rep, an unknown measure, a NaN threshold,
 * n >= 2^32-1; DST_ERR_STATE: slot 0 is not uploaded.  Synchronous on the context's stream.  The pairs are computed once
 * (the triangle), in row slabs; behind each slab's pair kernel its rows are resolved in sub-blocks of 512 (one workgroup
 * settles a sub-block's own dependencies in LDS, a wide launch marks what the new representatives cover) and the host
 * never waits inside the sweep.  Slots, the path choice and later dst_run_square results are untouched.  Single GPU,
 * loaded set only (not dst_stream). */
int dst_representatives(dst_ctx *ctx, int measure, double threshold, uint64_t max_pairs, uint32_t *rep, uint32_t *tallies,
                        void *values, size_t cap, uint64_t *n_representatives);
/* ---- pairs within a threshold ------------------------------------------------------------------ */
/* Which pairs are within `threshold` (the edge list of a transmission network, the sparse output of a thresholded run),
 * selected next to the values on the GPU and handed to a sink in chunks: the full result is never written.  The
 * definition is fixed to the bit:
 *   link    a pair whose DST_OUT_DISTANCE payload v (the value dst_run_square / dst_run_rect returns, bit-identical on
 *           every path) satisfies dst_clusters' rule against T = threshold:
 *             n / n_high (int64):  as real numbers, v <= floor(T) (clamped to the int64 range; below -2^63 nothing links)
 *             f64:                 IEEE v <= T, decided on dst_nearest's sort key: NaN is never a link, -0.0 links
 *                                  wherever +0.0 does, T = +inf links every pair whose value is not NaN
 *           jc69 / k80 / tn93 payloads are the pair kernels' series form, within 2^-44 (jc69, k80) or 2^-42 (tn93) of the
 *           exact value relatively, not bitwise the reference's: a pair whose value lies that close to T can be decided
 *           differently from a CPU computation (as in dst_clusters).  raw, n and n_high are exact.
 *   pairs   square != 0: slot 0 against itself (row_slot / col_slot ignored), the pairs i < j.
 *           square == 0: every record of row_slot against every record of col_slot; row_slot == col_slot is DST_ERR_ARG
 *           (use the square form), as in dst_nearest.
 *   result  the links in canonical pair order (square: i < j row-major; rectangle: i outer, j inner): the entries of the
 *           full result that pass the rule, nothing reordered.  It depends neither on the path nor on max_pairs.
 * Consequences: *n_links of a square call equals dst_clusters' `links` for the same T, and the connected components of the
 * links are dst_clusters' clusters.
 *
 * The sink is called on the calling thread, strictly in canonical order, each time with 1 <= n_links <= DST_LINKS_CHUNK
 * links: a row slab with more links is delivered in several calls, a slab with none in no call.  first_link is the running
 * index of the call's first link; row[e], col[e] are record indices (square: row[e] < col[e]); values (DST_LINKS_VALUES)
 * are the links' DST_OUT_DISTANCE payloads, bitwise what dst_run_square / dst_run_rect gives for the pair; tallies
 * (DST_LINKS_TALLIES) are dst_tally_width(measure) DST_OUT_TALLY words per link, the exact integers (tn93: base counts in
 * (row, col) order), so that dst_finalize gives the reference's bits.  values / tallies are NULL unless asked for in
 * `what`.  The buffers are library-owned page-locked memory, valid only during the call.  A non-zero return stops the run:
 * DST_ERR_STATE, message "stopped by sink", as dst_run_slabs.  sink == NULL counts only: nothing is compacted or copied,
 * and the known bits of `what` mean nothing.
 *   threshold   any non-NaN double (NaN: DST_ERR_ARG)
 *   max_pairs   0: the default slab bound (2^25 pairs); else the most pairs of one row slab, as in dst_clusters
 *   n_links     the total, or NULL; 0 on any error before the first slab, after a stop the links delivered so far
 * A square set of fewer than 2 records, or an empty row or column set: DST_OK, 0 links, no sink call.  A threshold below
 * which nothing can link (n / n_high with floor(T) < -2^63) runs no slab, as dst_clusters.  DST_ERR_ARG: a NULL ctx, an
 * unknown measure, a NaN threshold, a bad slot, equal slots with square == 0, unknown bits in `what`, a set of 2^32-1
 * records or more.  DST_ERR_STATE: a set is not uploaded, or the widths differ (dst_nearest's message).  Synchronous on the
 * context's stream; per row slab a count, a scan and one windowed write per DST_LINKS_CHUNK links, no sort.  Slots, the
 * path choice and later results are untouched.  Single GPU, loaded sets only (stream mode: dst_stream_open_links). */
#define DST_LINKS_VALUES 1  /* hand the sink the links' DST_OUT_DISTANCE payloads */
#define DST_LINKS_TALLIES 2 /* and/or dst_tally_width(measure) DST_OUT_TALLY words per link */
#define DST_LINKS_CHUNK (1u << 22) /* the most links of one sink call */
typedef int (*dst_links_sink)(void *user, uint64_t first_link, uint64_t n_links, const uint32_t *row, const uint32_t *col,
                              const void *values, const uint32_t *tallies);
int dst_links(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, double threshold, uint64_t max_pairs,
              int what, dst_links_sink sink, void *user, uint64_t *n_links);
/* ---- difference sites of a list of pairs ---------------------------------------------------------- */
/* WHICH sites separate two records (the label of a 2-SNP link, of an MST edge: "C241T, A23403G"), for a list of pairs the
 * caller names (dst_links' row / col, dst_mst's edges), gathered from the bit-planes the GPU already holds.  The
 * definition is fixed to the bit.  a and b are the high nibbles of the Paradis codes of the row record and the column
 * record at a site: A = 8, G = 4, C = 2, T = 1, nibble 15 is N / - / ?; a nibble determines everything any measure reads.
 * A site is a difference site of `measure` when it adds 1 to the measure's difference tally, as dst_site_tallies
 * defines it:
 *   n, n_high, raw, jc69   (a & b) == 0
 *   k80                    (a & b) == 0, and each of a, b is purine-class {8, 4, 12} or pyrimidine-class {2, 1, 3} (the site
 *                          counts as ts or tv)
 *   tn93                   (a & b) == 0, and both a and b are one of {8, 4, 2, 1} (the site counts in count_d)
 * Consequences: the number of listed sites of a pair equals the pair's difference tally in DST_OUT_TALLY (word 0 of n /
 * n_high / raw / jc69, ts + tv of k80, count_d of tn93); sites at or beyond len (the pack's N padding) are never listed.
 *   pairs    square != 0: both indices address slot 0 (row_slot / col_slot ignored); any row[e], col[e] below n, in any
 *            order, repeated pairs allowed, and row[e] == col[e], which lists nothing.
 *            square == 0: row[e] indexes row_slot, col[e] indexes col_slot; equal slots are DST_ERR_ARG, as in dst_nearest.
 *   result   CSR in host memory: offsets has n_pairs + 1 entries (required); sites holds the ascending 0-based site
 *            indices of pair e at [offsets[e], offsets[e + 1]); bases[k] = a << 4 | b of that site.
 *            sites == NULL and bases == NULL: offsets and *total only, no write pass runs.  cap_entries below the total:
 *            DST_ERR_CAPACITY with offsets and *total valid, as dst_differences.  total may be NULL.
 * n_pairs == 0: DST_OK, offsets[0] = 0.  DST_ERR_ARG: a NULL ctx, row, col or offsets; an unknown measure; a bad slot;
 * exactly one of sites / bases NULL; an index out of range (the message names the first such pair); len >= 2^32.
 * DST_ERR_STATE: a set is not uploaded, the widths differ (dst_nearest's message), or a set came from dst_upload_shared
 * (it holds no planes: the dense kernels' refusal).  Synchronous on the context's stream.  Slots, the path choice and
 * later results are untouched; a set with deferred planes gets them first, as for any plane reader.  Device memory
 * besides the sets is bounded whatever n_pairs and the total: the pairs go to the device in batches of at most
 * DST_PAIR_SITES_BATCH (per batch a count launch, one wave per pair, and a scan), the entries come back in windows of at
 * most DST_PAIR_SITES_WINDOW (one write launch each) through page-locked staging; a pair's entries may straddle
 * windows.  Work ~ pairs x len whatever the data: 128 bytes of planes per pair and 128-site chunk, read once to count
 * and once more per window that the pair's entries meet.  Single GPU, loaded sets only (not dst_stream). */
#define DST_PAIR_SITES_BATCH  (1u << 20)  /* most pairs of one device batch */
#define DST_PAIR_SITES_WINDOW (1u << 24)  /* most entries of one device output window */
int dst_pair_sites(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                   const uint32_t *row, const uint32_t *col, uint64_t n_pairs,
                   uint64_t *offsets, uint32_t *sites, uint8_t *bases, size_t cap_entries, uint64_t *total);
/* ---- distances of a list of pairs ------------------------------------------------------------------ */
/* The distance of THESE pairs and only these (contact-traced pairs, the edges of a tree or a network another tool built, a
 * k-nearest-neighbour graph that needs exact distances, "tn93 for the 3 million links -m n --max-distance 5 gave me"): the
 * value of dst_run_square / dst_run_rect for a list of pairs the caller names, without the all-pairs result.  The
 * definition is fixed to the bit.
 *   pairs    dst_pair_sites': square != 0: both indices address slot 0 (row_slot / col_slot ignored); any row[e], col[e]
 *            below n, in any order, repeated pairs allowed, and row[e] == col[e].  square == 0: row[e] indexes row_slot,
 *            col[e] indexes col_slot; equal slots are DST_ERR_ARG.  The sets are resolved as in dst_nearest, with its
 *            messages, in its order.
 *   result   (host memory) values[e]: the 8-byte DST_OUT_DISTANCE payload (int64 for n / n_high, else f64) that
 *            dst_run_square / dst_run_rect returns for the pair, bitwise; tallies[e * W ..], W = dst_tally_width(measure):
 *            bitwise its DST_OUT_TALLY words.  Either pointer may be NULL; both NULL is DST_ERR_ARG.
 *            square, row[e] > col[e]: the result of the canonical pair (min, max), tn93 base counts in that order
 *            (dst_nearest's rule), so (j, i) equals (i, j).
 *            square, row[e] == col[e]: the record against itself.  Tallies: the sum over the sites of
 *            dst_site_tallies(code, code); value: the device finalisation of those tallies with the record's base counts on
 *            both sides — bitwise what dst_run_rect returns for (i, i) when the same set is also loaded in the other slot.
 *   route    how the entries are computed; the result does not depend on it, nor on max_pairs, the kernel path, the order
 *            of the list or how it is batched.
 *              DST_PAIRS_DIRECT  every pair from the bit-planes of its two records (a gather; work ~ pairs x len)
 *              DST_PAIRS_SWEEP   the row slabs of the all-pairs result that the list touches are run (at most max_pairs
 *                                pairs each, 0: 2^25, at least one row; a slab no listed pair falls into is skipped) and
 *                                the listed entries are gathered from each slab on the device.  The square's diagonal
 *                                entries have no place in that result: they take the direct route whatever `route` says.
 *              DST_PAIRS_AUTO    the cheaper of the two by a cost estimate
 *   info     (may be NULL) the route taken (DST_PAIRS_DIRECT or DST_PAIRS_SWEEP), the lanes that served one pair in the
 *            direct kernel's last launch (0: none ran; dst_run_pairs_lanes(len)), the pairs that went each way, the slabs
 *            the sweep ran.
 * n_pairs == 0: DST_OK, nothing written.  DST_ERR_ARG: a NULL ctx, row or col; an unknown measure or route; both outputs
 * NULL; a bad slot; an index out of range (the message names the first such pair, as dst_pair_sites does); len >= 2^32.
 * DST_ERR_CAPACITY: cap_entries < n_pairs (nothing written).  DST_ERR_STATE: a set is not uploaded, the widths differ, or a
 * set came from dst_upload_shared (it holds no planes: the dense kernels' refusal, same message).  Synchronous on the
 * context's stream.  A set with deferred planes gets them when the direct route first reads them, and the derived planes
 * where the measure reads them (raw, jc69, k80, tn93); slots, the path choice, dst_last_path, dst_last_launch and later
 * results are untouched.  Device memory besides the sets is bounded whatever n_pairs: the pairs go to the device in batches of
 * at most DST_RUN_PAIRS_BATCH and the results come back the same way, through page-locked staging; the sweep adds one
 * slab.  Single GPU, loaded sets only (not dst_stream). */
typedef struct {
    int route;                /* DST_PAIRS_DIRECT or DST_PAIRS_SWEEP: what the call did */
    uint32_t lanes_per_pair;  /* of the direct kernel's last launch, 0: none ran */
    uint64_t direct_pairs, swept_pairs, slabs;
} dst_pairs_info;
#define DST_PAIRS_AUTO 0
#define DST_PAIRS_DIRECT 1
#define DST_PAIRS_SWEEP 2
#define DST_RUN_PAIRS_BATCH (1u << 20) /* most pairs of one device batch */
int dst_run_pairs(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                  const uint32_t *row, const uint32_t *col, uint64_t n_pairs, int route, uint64_t max_pairs,
                  void *values, uint32_t *tallies, size_t cap_entries, dst_pairs_info *info);
/* Pure host code: the lanes the direct route gives one pair for an alignment of len sites — the smallest power of two that
 * covers its 128-site chunks, at most 64. */
uint32_t dst_run_pairs_lanes(uint64_t len);
/* ---- distances per column window ------------------------------------------------------------------- */
/* Distances ALONG the alignment (recombination scans: a query against a panel in windows of 500-1,000 sites sliding by
 * 100-200; per-gene or per-region distances; the genome without its masked ends), from the bit-planes the GPU already
 * holds: no cut, upload and run per window.  The definition is fixed to the bit.
 *   window   a half-open column range [begin, end), 0 <= begin <= end <= len.  Windows may overlap, repeat, be empty and
 *            come in any order; 1 <= n_windows <= DST_WINDOWS_MAX.
 *   restriction of a set to a window: the set with every record cut to those columns, as dst_upload(..., base_counts =
 *            NULL) would hold it — tn93's {A,T,G,C} counts are counted by code, per window.
 *   result of window w: bitwise what dst_run_square / dst_run_rect returns for the same row range and out_kind on the
 *            restricted sets.  Tallies are the exact integers; DST_OUT_DISTANCE payloads come from the same device
 *            finalisation as the pair kernels' epilogue, and since every path is bit-identical the result does not depend
 *            on the path.  An empty window: all tallies and base counts zero, n / n_high give 0, the f64 measures what that
 *            finalisation gives for zeros (NaN for raw).
 *   layout   out[w * P + p]: P = the pairs of the row range (square: i < j row-major over rows [row_begin, row_end);
 *            rectangle: (row_end - row_begin) x n_col), p = the canonical index exactly as dst_run_square / dst_run_rect
 *            lay the range out, an entry dst_out_bytes(measure, out_kind, 1) bytes.  out_kind is DST_OUT_DISTANCE or
 *            DST_OUT_TALLY (DST_OUT_TALLY16: DST_ERR_ARG).  DST_OUT_TALLY + dst_window_base_counts + dst_finalize gives
 *            the reference's bits for the restricted alignment.
 * The sets are resolved as in dst_nearest (square != 0: slot 0 against itself; else two different slots): a bad slot, equal
 * slots, a set not uploaded, different widths fail with its messages.  DST_ERR_ARG: a NULL ctx, window array or output; an
 * unknown measure or out_kind; n_windows above the maximum; a window with begin > end or end > len (the message names the
 * first); row_begin > row_end or row_end > n; len >= 2^32.  n_windows == 0 or an empty row range: DST_OK, nothing written.
 * DST_ERR_CAPACITY: n_windows x dst_out_bytes(measure, out_kind, P) exceeds the capacity (nothing written).
 * DST_ERR_STATE: a set came from dst_upload_shared (it holds no planes: the dense kernels' refusal).  DST_ERR_NOMEM, with
 * the byte count, when the window table or tn93's count table (n_windows x records x 16 bytes per set) does not fit.
 * A set with deferred planes gets them first, as for any plane reader; slots, the path choice, dst_last_path,
 * dst_last_launch and later results are untouched.  stream == NULL: the context's stream, and the call returns when the
 * results are there; else the work is queued on that stream after a wait for it (the window table is the context's: one
 * call at a time per context).  Work ~ P x the chunks (128 sites) the windows meet.  Single GPU, loaded sets only. */
#define DST_WINDOWS_MAX 65536u
int dst_run_windows(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                    uint64_t row_begin, uint64_t row_end,
                    const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                    int out_kind, void *d_out, size_t out_capacity_bytes, void *stream);
/* the same into host memory (synchronous, through the context's staging buffer) */
int dst_run_windows_host(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                         uint64_t row_begin, uint64_t row_end,
                         const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                         int out_kind, void *h_out, size_t out_capacity_bytes);
/* per (window, record) the {A,T,G,C} counted by code inside the window: counts[(w * n + record) * 4 ..], host memory,
 * cap_entries >= n_windows x n x 4 uint32 (else DST_ERR_CAPACITY).  Errors as above. */
int dst_window_base_counts(dst_ctx *ctx, int slot, const uint64_t *win_begin, const uint64_t *win_end,
                           uint32_t n_windows, uint32_t *counts, size_t cap_entries);
/* ---- k nearest records per column window ------------------------------------------------------------ */
/* For every (row record, window) the k column records with the smallest distance INSIDE that window, selected next to the
 * tallies on the GPU: a recombination scan asks which panel records are nearest to a query in each window, a few
 * neighbours per (query, window), never the matrix dst_run_windows returns.  The definition is fixed to the bit.
 *   sets, windows, row range   exactly dst_run_windows': square != 0 is slot 0 against itself (row_slot / col_slot
 *            ignored), else two different slots; a window is a half-open [begin, end), 0 <= begin <= end <= len, windows
 *            may overlap, repeat, be empty and come in any order; 1 <= n_windows <= DST_WINDOWS_MAX; rows [row_begin,
 *            row_end) of the row set.
 *   candidates of row record i in window w   rectangle: every record j of col_slot, none excluded; square: every j != i
 *            of slot 0 (identical sequences stay in).
 *   value of candidate j   the DST_OUT_DISTANCE payload dst_run_windows writes for window w: rectangle, of the pair
 *            (i, j); square, of the canonical pair (min(i, j), max(i, j)) — tn93 takes the two records' per-window base
 *            counts in that order, as dst_nearest does for the whole width.  Its tallies are that entry's DST_OUT_TALLY
 *            words.
 *   order    ascending (key(value), j) with dst_nearest's key (int64: v ^ 2^63; f64: NaN after +inf, -0.0 as +0.0): a
 *            strict total order, so the answer is unique.  1 <= k <= 256, else DST_ERR_ARG.  *k_used = min(k, candidates
 *            per row).  An empty window makes every candidate equal (0 for n / n_high, NaN for raw, whatever the
 *            finalisation gives for zeros otherwise): it lists the first k_used candidates in index order.
 *   layout   (host memory) entry ((i - row_begin) * n_windows + w) * k_used + e, e ascending:
 *              index    the column record (required)
 *              values   the 8-byte DST_OUT_DISTANCE payloads, or NULL
 *              tallies  dst_tally_width(measure) DST_OUT_TALLY words per entry, or NULL
 *            cap_entries below (row_end - row_begin) * n_windows * k_used: DST_ERR_CAPACITY, nothing written but *k_used.
 *   max_entries   the most pair-windows (rows x windows x column records) of one device slab, 0: 2^25.  A slab is a range
 *            of rows x a range of windows, at least one (row, window).  The result does not depend on it.  Device memory
 *            beside the sets, the window table and tn93's per-window count table (n_windows x records x 16 bytes per set,
 *            as dst_run_windows) is bounded by the slab's tallies and its lists, whatever the job's size.
 * n_windows == 0, an empty row range, or no candidates (a square set of fewer than 2 records, an empty column set): DST_OK
 * with *k_used set and nothing written.  Errors are dst_run_windows', in its order and with its messages: DST_ERR_ARG for a
 * NULL ctx; more than DST_WINDOWS_MAX windows; a NULL window array; an unknown measure; k outside 1..256; a NULL index or
 * k_used; a bad slot or equal slots; then DST_ERR_STATE for a set not uploaded, different widths, or a set from
 * dst_upload_shared (the dense kernels' refusal); DST_ERR_ARG for len >= 2^32, a bad window (the message names the first),
 * row_begin > row_end or row_end > n, sets of 2^32-1 records or more; DST_ERR_CAPACITY; DST_ERR_NOMEM with the byte count.
 * Synchronous on the context's stream: per slab the window sweep of the rectangle rows x ALL column records (a square job
 * sweeps slot 0 against itself: every row needs all its j != i, at twice the triangle's work for a whole square), then one
 * wave per (row, window) list, then the copy of the finished lists.  A set with deferred planes gets them first; slots, the
 * path choice, dst_last_path, dst_last_launch and later results are untouched.  Single GPU, loaded sets only. */
int dst_nearest_windows(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                        uint64_t row_begin, uint64_t row_end,
                        const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                        uint32_t k, uint64_t max_entries,
                        uint32_t *index, uint32_t *tallies, void *values, size_t cap_entries, uint32_t *k_used);
/* Pure host code: the windows of `distance --windows W --step S`.  begin_k = k step, end_k = min(begin_k + width, len), for
 * k = 0, 1, ... up to the first k whose end_k == len (no window is a subset of its predecessor) — with a step above the
 * width, which leaves columns between windows out, also no further than the last k with begin_k < len; len == 0: no window.
 * begin == NULL and end == NULL: *count only.  width == 0, step == 0, a NULL count or exactly one NULL array: DST_ERR_ARG.
 * More than DST_WINDOWS_MAX windows, or more than cap: DST_ERR_CAPACITY with *count set (saturated at 2^32-1). */
int dst_sliding_windows(uint64_t len, uint64_t width, uint64_t step, uint64_t *begin, uint64_t *end,
                        size_t cap, uint32_t *count);
/* ---- per-record and histogram summaries ---------------------------------------------------------- */
/* What the distances of a set look like, computed next to the values on the GPU: the histogram of the pairwise distances
 * (from which a threshold is chosen) and, per record, how many records lie within `threshold` of it (its degree in the
 * dst_links network) and the sum of its distances to the rest (mean distance: outliers, the medoid; averaged over the
 * records with raw, the nucleotide diversity).  O(n + bins) of state, the full result is never written.  The definition
 * is fixed to the bit, and every accumulation is an integer one, so the result depends neither on the path, nor on
 * max_pairs, nor on the order the pairs are met in.
 *   pairs   as in dst_links.  square != 0: slot 0 against itself (row_slot / col_slot ignored), the pairs i < j; a pair
 *           counts for both of its records in the per-record results and once in the histogram and the totals.
 *           square == 0: every record of row_slot against every record of col_slot, per-record results for the row
 *           records only; row_slot == col_slot is DST_ERR_ARG (use the square form), as in dst_nearest.
 * Per pair, from its DST_OUT_DISTANCE payload v (the value dst_run_square / dst_run_rect returns, bit-identical on every
 * path):
 *   link      dst_clusters' rule against T = threshold: n / n_high v <= floor(T) (clamped to the int64 range; below -2^63
 *             nothing links); f64 IEEE v <= T on dst_nearest's sort key: NaN never links, -0.0 links wherever +0.0 does
 *   q         the fixed-point value, a signed 64-bit integer.  n / n_high: q = v, always "summable".  f64 measures:
 *             q = rint(v * 2^DST_SUMMARY_SCALE_BITS), round to nearest even (the product is exact), defined only when v
 *             is summable: not NaN and |v| < 2^25 (no distance reaches 2^25)
 *   bin       (bins > 0) with width_q = rint(width * 2^DST_SUMMARY_SCALE_BITS) for f64 measures, (int64)width for
 *             n / n_high: NaN lies in no bin (it is counted in nan_pairs); v >= 2^25, +inf included, in bin bins - 1;
 *             v <= -2^25 in bin 0; any other value in bin clamp(floor(q / width_q), 0, bins - 1), the integer floor quotient
 * Per record x over its partners (each array may be NULL: not wanted):
 *   within[x]    the partners whose pair is a link
 *   summable[x]  the partners whose pair is summable
 *   sum[x]       S = the sum of q over the summable partners, an exact integer, converted to double once (round to nearest
 *                even) and, for f64 measures, scaled by 2^-DST_SUMMARY_SCALE_BITS (exact).  It misses the real sum of the
 *                payloads by at most summable[x] * 2^-(DST_SUMMARY_SCALE_BITS + 1), plus the one rounding.
 * totals (may be NULL): pairs; nan_pairs (payload NaN); summable_pairs; links; sum, the same conversion of the exact sum
 * over the pairs, each once.  hist[b] (bins entries): the pairs in bin b; their sum is pairs - nan_pairs.
 * Consequences: `links` of a square call equals dst_clusters' `links` and dst_links' count for the same T; within[x] is the
 * number of dst_links entries that name x.
 *   threshold   any non-NaN double (NaN: DST_ERR_ARG)
 *   max_pairs   0: the default slab bound (2^25 pairs); else the most pairs of one row slab, as in dst_clusters
 *   bins        0: no histogram (hist, width ignored); else 1 .. DST_SUMMARY_MAX_BINS with a non-NULL hist and a width
 *               that is finite, > 0 and < 2^25 with width_q >= 1; for n / n_high an integer value >= 1.  Else DST_ERR_ARG.
 *   cap         the room of each non-NULL per-record array in entries; below the row set's record count DST_ERR_CAPACITY
 * A square set of fewer than 2 records, or an empty row or column set: DST_OK, zero totals, a zero histogram, zero
 * per-record entries, no slab run.  DST_ERR_ARG: a NULL ctx, an unknown measure, a NaN threshold, a bad slot, equal slots
 * with square == 0, a set of 2^32-1 records or more; DST_ERR_STATE: a set is not uploaded, or the widths differ
 * (dst_nearest's message) - dst_links' checks and messages.  Synchronous on the context's stream: per row slab a row pass
 * and (square) a column pass when a per-record array is wanted, a histogram pass when bins > 0 or only the totals are
 * wanted; one copy back.  Slots, the path choice and later results are untouched.  Single GPU, loaded sets only (not
 * dst_stream). */
#define DST_SUMMARY_SCALE_BITS 37
#define DST_SUMMARY_MAX_BINS 4096
typedef struct dst_summary_totals {
    uint64_t pairs;
    uint64_t nan_pairs;
    uint64_t summable_pairs;
    uint64_t links;
    double sum;
} dst_summary_totals;
int dst_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, double threshold, uint64_t max_pairs,
                uint32_t bins, double width, uint64_t *hist, uint32_t *within, uint32_t *summable, double *sum, size_t cap,
                dst_summary_totals *totals);
/* ---- summaries in stream mode ---------------------------------------------------------------------- */
/* A stream that keeps dst_summary's counts and exact sums instead of the result matrix: how many records of a database that
 * does not fit in memory lie within T of each of mine, each record's mean distance to the database, the distribution of
 * the distances - and, per database record, how it sits against the loaded set.  A summary stream IS a dst_stream, the
 * fifth kind: dst_stream_acquire / _submit / _collect / _in_flight / _close work on it as on a closest stream, with both
 * wire formats, the caller's base counts and the ring of `depth` slots (2..16); dst_stream_collect returns *results = NULL,
 * but still waits for the batch and still reports DST_ERR_INVALID_CODE.
 * Definition, fixed to the bit.  The payload v of the pair (streamed s, loaded i) is what the same stream would deliver for
 * it as DST_OUT_DISTANCE, bit for bit: the rectangle with the batch as rows (tn93: the streamed record's base counts as q,
 * the loaded record's as t; the same use_base_counts).  link, summable, q, bin, the one conversion of an exact integer sum
 * to double and the scaling by 2^-DST_SUMMARY_SCALE_BITS are dst_summary's (above), word for word, and so are threshold,
 * bins and width with their checks and messages.
 *  DST_STREAM_SUMMARY_STREAMED  per batch: within[s], summable[s], sum[s] of every record s of the batch over all loaded i -
 *                               what dst_summary(square = 0, rows = the batch, cols = slot 0) returns per row record
 *  DST_STREAM_SUMMARY_LOADED    kept over the stream's life: within[i], summable[i], sum[i] of every loaded record i over
 *                               every streamed record of every batch submitted so far
 * hist and the totals run over every pair so far, each once; totals.pairs = records x n_loaded, *records the number of
 * records submitted.  `what` may be 0: the totals and the histogram alone are kept, O(bins) of state.  All accumulation is
 * integer, so the answer does not depend on how the stream is cut into batches, on depth, on the wire format or on the path.
 * Limits.  The per-record counters are uint32 and the hi / lo split of a sum needs fewer than 2^32 partners: a submit that
 * would take the records past 2^32-2 (compared in 64 bits) is DST_ERR_CAPACITY and changes nothing.  A batch's atomics cannot
 * be taken back: after a batch with an invalid code every later dst_stream_submit, dst_stream_summary_batch and
 * dst_stream_summary_result on that stream is DST_ERR_STATE, as for DST_CLOSEST_FOR_LOADED.
 * Open, errors in this order: DST_ERR_ARG for a NULL ctx or stream pointer, an unknown measure or wire, a NaN threshold, bits
 * in `what` other than the two, the bins and width rules of dst_summary (hist is not asked for here), max_records == 0, depth
 * outside 2..16; DST_ERR_STATE for slot 0 not loaded; DST_ERR_ARG for a loaded set of 2^32-1 records or more; DST_ERR_NOMEM.
 * Submit: DST_ERR_STATE when the loaded set's record count or width changed.  An empty loaded set runs no reduction and
 * gives zero results.  The calls below on any other stream are DST_ERR_ARG, as are the closest, links and window-closest
 * calls on this one; a NULL stream is DST_ERR_ARG.
 * The stream owns all of its state - the kept words, zeroed once at open, and per ring slot the batch's records' words - so
 * dst_summary or any other call on the context between two submits does not disturb it.  Per submit, on the compute stream
 * behind the batch's pair kernel: one tile pass over the batch's matrix that reads every entry once for both sides and the
 * totals, and with bins > 0 dst_summary's histogram pass.  Per batch the bad-code word and (STREAMED) 24 bytes per streamed
 * record cross the host link, never the matrix.  Single GPU. */
#define DST_STREAM_SUMMARY_LOADED   1  /* keep the loaded records' per-record state over the stream's life */
#define DST_STREAM_SUMMARY_STREAMED 2  /* hand out every batch's streamed records' per-record results     */
int dst_stream_open_summary(dst_ctx *ctx, int measure, double threshold, int what, uint32_t bins, double width,
                            size_t max_records, int depth, int wire, dst_stream **stream);
/* STREAMED only (else DST_ERR_ARG).  After dst_stream_collect: the collected batch, *n_records entries per array, in
 * page-locked, library-owned memory that is valid until the next dst_stream_submit.  n_records is required; within, summable
 * and sum may be NULL.  DST_ERR_STATE when no batch has been collected since the last submit. */
int dst_stream_summary_batch(dst_stream *stream, size_t *n_records, const uint32_t **within,
                             const uint32_t **summable, const double **sum);
/* A snapshot of everything kept so far (host memory): hist (bins entries), the loaded records' within / summable / sum
 * (n_loaded entries each), the totals and *records; every pointer may be NULL.  Without DST_STREAM_SUMMARY_LOADED the three
 * per-record pointers must be NULL, else DST_ERR_ARG.  Needs dst_stream_in_flight() == 0, else DST_ERR_STATE; cap below
 * n_loaded with a non-NULL per-record array: DST_ERR_CAPACITY.  The call may be repeated, and streaming may go on afterwards. */
int dst_stream_summary_result(dst_stream *stream, uint64_t *hist, uint32_t *within, uint32_t *summable, double *sum,
                              size_t cap, dst_summary_totals *totals, uint64_t *records);
/* ---- summaries per column window ------------------------------------------------------------------- */
/* dst_summary's counts and sums INSIDE every column window, reduced next to the window sweep on the GPU: diversity along
 * the genome (pi per window with raw on one set, d_xy per window between two sets), the mean distance of a query to a
 * panel per window, how many pairs lie within T inside each gene.  The state is O(n_windows), or O(n_windows x n_rows)
 * when a per-record array is wanted; the n_windows x P result of dst_run_windows is never written.  The definition is
 * fixed to the bit, and every accumulation is an integer one: the result does not depend on the order the pairs are met in.
 *   sets, windows   exactly dst_run_windows': square != 0 is slot 0 against itself (row_slot / col_slot ignored), the pairs
 *            i < j; else two different slots, every record of row_slot against every record of col_slot.  A window is a
 *            half-open [begin, end), 0 <= begin <= end <= len; windows may overlap, repeat, be empty and come in any order;
 *            1 <= n_windows <= DST_WINDOWS_MAX.  tn93 takes the per-window {A,T,G,C} counts counted by code.
 *   payload  v of a pair in window w: bitwise the DST_OUT_DISTANCE entry dst_run_windows writes for it.
 *   result of window w: dst_summary's definition applied to that window's payloads — the same link rule against
 *            `threshold`, the same fixed-point q in units of 2^-DST_SUMMARY_SCALE_BITS, the same "summable", the same NaN
 *            count, the same one conversion of the exact integer sum to double.
 *   totals[w]   (n_windows entries, or NULL) pairs = P, the same in every window; nan_pairs; summable_pairs; links; sum.
 *   rec_within, rec_summable, rec_sum   (each n_windows x n_rows entries, or NULL) entry w * n_rows + x, window-major as
 *            dst_run_windows and dst_window_base_counts lay theirs out; n_rows = the row set's record count.  A square pair
 *            counts for both of its records, as in dst_summary; a rectangle gives the row records only.
 *   rec_cap  the room of each non-NULL per-record array in entries.
 * An empty window follows from the definition: n / n_high give v = 0 for every pair (all summable, sum 0, links when
 * threshold >= 0); raw gives NaN for every pair (nan_pairs = P).  Consequence: for a set uploaded without caller base
 * counts, the window [0, len) gives dst_summary's totals and per-record arrays bitwise.
 * Errors are dst_run_windows', in its order and with its messages, with these additions: DST_ERR_ARG for a NULL ctx; more
 * than DST_WINDOWS_MAX windows; a NULL window array; an unknown measure; then a NaN threshold; then `totals` and all three
 * per-record arrays NULL; a bad slot or equal slots; DST_ERR_STATE for a set not uploaded, different widths, or a set from
 * dst_upload_shared (the windows' refusal); DST_ERR_ARG for len >= 2^32, a bad window (the message names the first), sets
 * of 2^32-1 records or more, and a per-record array wanted with n_rows x n_windows above 2^31; DST_ERR_CAPACITY, with
 * nothing written, when rec_cap is below n_windows x n_rows and a per-record array is given; DST_ERR_NOMEM, with the byte
 * count, when the state (24 bytes per (window, record) when a per-record array is wanted, 40 bytes per window), the window
 * table or tn93's count table does not fit.
 * n_windows == 0, an empty row or column set, or a square set of fewer than 2 records: DST_OK with zero counts and sums,
 * `pairs` set, and no launch.  Synchronous on the context's stream: one fused sweep-and-reduce launch family and one copy
 * back.  A set with deferred planes gets them first; slots, the path choice, dst_last_path, dst_last_launch and later
 * results are untouched.  Single GPU, loaded sets only. */
int dst_window_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                       const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                       double threshold,
                       dst_summary_totals *totals,
                       uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum,
                       size_t rec_cap);
/* ---- group summaries ------------------------------------------------------------------------------ */
/* dst_summary's exact sums keyed by a labelling of the records (lineages, sites, sampling months): per pair of groups the
 * number of pairs, of links and of summable pairs, the sum of the distances, the smallest and the largest distance ("within
 * group" and "between group" mean distance, pi and d_xy; the input of silhouettes and medoids); and per record and group
 * the same sums over the record's partners in that group (which places an unlabelled record next to its closest group).
 * O(n G + G^2) of state; the full result is never written.
 *   pairs    dst_summary's.  square != 0: slot 0 against itself (row_slot / col_slot ignored), the pairs i < j;
 *            square == 0: every record of row_slot against every record of col_slot, row_slot == col_slot is DST_ERR_ARG.
 *   labels   row_group[x] for every record x of the row set: a group below n_row_groups, or DST_GROUP_NONE (the record
 *            belongs to no group); col_group / n_col_groups the same for the column set.  In the square form the one label
 *            array is row_group and the one count n_row_groups = G; col_group and n_col_groups are ignored.
 * Per pair the link against `threshold`, the fixed-point value q, "summable" and NaN are dst_summary's, word for word.
 * cells (may be NULL when a rec_* array is given): row-major n_row_groups x n_col_groups (square: G x G).  Cell (a, b)
 * covers the pairs with one record in group a and the other in group b, each pair once: in a rectangle the row record in a
 * and the column record in b; in the square both orders are stored, cells[a][b] == cells[b][a] byte for byte, and cell
 * (a, a) holds the pairs i < j inside a.  A pair with an unassigned record is in no cell.
 *   pairs            from the group sizes alone: |a| |b|, or |a| (|a| - 1) / 2 on the square's diagonal
 *   nan_pairs, summable_pairs, links   counts over the cell's pairs; nan_pairs + summable_pairs <= pairs
 *   sum              dst_summary's conversion of the exact integer sum of q over the cell's summable pairs (kept in 128
 *                    bits: a cell can hold 2^32 pairs and more)
 *   min_bits, max_bits   over the cell's pairs whose payload is not NaN: the payloads with the smallest and the largest
 *                    dst_nearest sort key, decoded back from the key (so a -0.0 is reported as +0.0).  A cell without such
 *                    a pair: the quiet NaN 0x7FF8000000000000 for the f64 measures, 0 for n / n_high (there it means
 *                    pairs == 0).
 * rec_within, rec_summable, rec_sum (each may be NULL: not wanted): row-major n_rows x n_col_groups (square: n x G).  Entry
 * (x, g) is dst_summary's within / summable / sum of record x restricted to its partners in group g.  Every record x has
 * a row, assigned or not; a record is never its own partner; the square form counts a pair for both of its records;
 * partners that are unassigned appear nowhere.
 * Consequences: for a != b cell (a, b) is the sum of rec_*[x][b] over the x in a; cell (a, a) is half of that sum, which
 * is even.  With every record assigned the cells' totals (square: over a <= b; rectangle: over all cells) are
 * dst_summary's totals and the sum over g of rec_*[x][g] is dst_summary's per-record result (the sums before their
 * conversion).  Every accumulation is an integer one: the result depends neither on the path, nor on max_pairs, nor on
 * the order the pairs are met in.
 *   threshold   any non-NaN double
 *   max_pairs   0: the default slab bound (2^25 pairs); else the most pairs of one row slab
 *   cells_cap   the room of cells in entries; rec_cap the room of each non-NULL rec_* array in entries
 * DST_ERR_ARG: a NULL ctx or row_group; NULL cells with all three rec_* NULL; an unknown measure; a NaN threshold; a NULL
 * col_group in the rectangle form; a group count of 0 or above DST_GROUPS_MAX; a bad slot, equal slots with square == 0, a
 * set of 2^32-1 records or more (dst_summary's messages); a label that is neither below its count nor DST_GROUP_NONE (the
 * message names the first such record and its side).  DST_ERR_CAPACITY: cells_cap or rec_cap too small.  DST_ERR_STATE: a
 * set is not uploaded, or the widths differ.  DST_ERR_NOMEM: the state does not fit in device memory (the message gives
 * the byte count).  A square set of fewer than 2 records, an empty row or column set, and a call in which no record of
 * the column side (the square: of the set) is assigned or whose cells alone are wanted while no row record is assigned:
 * DST_OK, zero counts and sums, min / max as for an empty cell, no slab run.  Synchronous on the context's stream; slots,
 * the path choice and later results are untouched.  Single GPU, loaded sets only (stream mode:
 * dst_stream_open_group_summary). */
#define DST_GROUPS_MAX 1024u          /* most groups of one side */
#define DST_GROUP_NONE 0xFFFFFFFFu    /* a record that belongs to no group */
typedef struct dst_group_cell {
    uint64_t pairs, nan_pairs, summable_pairs, links;
    double   sum;                     /* dst_summary's conversion of the exact integer sum of q */
    uint64_t min_bits, max_bits;      /* DST_OUT_DISTANCE payloads (int64 or f64 bits) */
} dst_group_cell;
int dst_group_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                      const uint32_t *row_group, uint32_t n_row_groups,
                      const uint32_t *col_group, uint32_t n_col_groups,
                      double threshold, uint64_t max_pairs,
                      dst_group_cell *cells, size_t cells_cap,
                      uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum, size_t rec_cap);
/* ---- group summaries in stream mode ----------------------------------------------------------------- */
/* dst_group_summary for a labelled database that does not fit on the GPU: the mean distance of each of my records to each
 * lineage of the database, the reference group every database record sits closest to, d_xy between my lineages and the
 * database's.  A group-summary stream IS a dst_stream, the sixth kind: dst_stream_acquire / _submit / _collect /
 * _in_flight / _close work on it as on a summary stream, with both wire formats, the caller's base counts and the ring of
 * `depth` slots (2..16); dst_stream_collect returns *results = NULL, but still waits for the batch and still reports
 * DST_ERR_INVALID_CODE.
 * Definition, fixed to the bit.  S is the set of every record submitted so far, in stream order.  The payload of the pair
 * (streamed s, loaded i) is the summary stream's: what the same stream would deliver for it as DST_OUT_DISTANCE, bit for
 * bit, with the batch as rows (tn93's count order and use_base_counts included).  The answer is dst_group_summary's
 * definition (above), word for word, applied to the rectangle rows = S, cols = slot 0: the link rule, q, "summable", NaN,
 * the 128-bit cell sum and its one conversion to double, min / max decoded from the sort key, the empty cell's quiet NaN
 * or 0.
 *   cells (always kept)          n_streamed_groups x n_loaded_groups entries, entry a G_l + b: streamed group a against
 *                                loaded group b; `pairs` from the group sizes so far
 *   DST_STREAM_GROUPS_STREAMED   per batch: n_records x G_l entries, dst_group_summary's rec_* rows of the batch's records
 *   DST_STREAM_GROUPS_LOADED     kept over the stream's life: n_loaded x G_s entries, entry i G_s + g: loaded record i's
 *                                within / summable / sum over its streamed partners in streamed group g - the rec_* rows
 *                                of the transposed rectangle
 * Every record has a row, assigned or not: a record labelled DST_GROUP_NONE still gets its STREAMED row and its LOADED table
 * row.  All accumulation is by integer atomics (add; min / max on the key), so the answer does not depend on the cut into
 * batches, on depth, on the wire format or on the kernel path.
 * Labels.  loaded_group: n_loaded entries, copied at open, each a group below n_loaded_groups or DST_GROUP_NONE; NULL: every
 * loaded record is in group 0, and then n_loaded_groups must be 1.  The streamed records' labels go into the acquired
 * slot's page-locked label block of max_records entries (dst_stream_group_labels, valid between dst_stream_acquire and
 * dst_stream_submit), which dst_stream_acquire has filled with 0: a stream that never asks for the block puts the whole
 * database in streamed group 0.  dst_stream_submit checks the first n_records labels on the host: one that is neither below
 * n_streamed_groups nor DST_GROUP_NONE is DST_ERR_ARG naming the record, and changes nothing.  Both group counts are
 * 1..DST_GROUPS_MAX.
 * Open, errors in this order: DST_ERR_ARG for a NULL ctx or stream pointer, an unknown measure or wire, a NaN threshold, bits
 * in `what` other than the two, a group count of 0 or above DST_GROUPS_MAX, a NULL loaded_group with n_loaded_groups != 1,
 * max_records == 0, depth outside 2..16; DST_ERR_STATE for slot 0 not loaded; DST_ERR_ARG for a loaded set of 2^32-1 records
 * or more and for a bad loaded label (dst_group_summary's message); DST_ERR_NOMEM with the byte count when 56 bytes per cell,
 * 24 bytes per (loaded record, streamed group) with LOADED, or per ring slot 24 bytes per (record, loaded group) do not fit.
 * Submit: DST_ERR_CAPACITY past 2^32-2 records (compared in 64 bits), changing nothing; DST_ERR_STATE when the loaded set's
 * record count or width changed.  A batch's atomics cannot be taken back: after a batch with an invalid code every later
 * dst_stream_submit, dst_stream_group_summary_batch and dst_stream_group_summary_result on that stream is DST_ERR_STATE.
 * An empty loaded set runs no reduction and gives zero results; when no loaded record is assigned and LOADED is not asked
 * for, nothing is launched.  The calls below on any other stream are DST_ERR_ARG, as are the other kinds' calls on this one;
 * a NULL stream is DST_ERR_ARG.
 * The stream owns all of its state - the loaded labels, the cells and the LOADED table, zeroed once at open, and per ring
 * slot the batch's labels and table - so dst_group_summary or any other call on the context between two submits does not
 * disturb it.  Per submit, on the compute stream behind the batch's pair kernel: dst_group_summary's row pass over the
 * batch's matrix (the STREAMED table, the cells' NaN / min / max), its fold of that table into the cells, and with LOADED
 * a column pass.  Per batch the labels, the bad-code word and (STREAMED) 24 bytes per (record, loaded group) cross the host
 * link, never the matrix.  Single GPU. */
#define DST_STREAM_GROUPS_LOADED   1   /* keep, per loaded record and STREAMED group, the table over the stream's life */
#define DST_STREAM_GROUPS_STREAMED 2   /* hand out, per batch, every streamed record's table over the LOADED groups    */
int dst_stream_open_group_summary(dst_ctx *ctx, int measure, double threshold, int what,
                                  const uint32_t *loaded_group, uint32_t n_loaded_groups, uint32_t n_streamed_groups,
                                  size_t max_records, int depth, int wire, dst_stream **stream);
/* The acquired slot's label block: max_records entries, page-locked, library-owned, filled with 0 by dst_stream_acquire.
 * DST_ERR_STATE when no buffer is acquired. */
int dst_stream_group_labels(dst_stream *stream, uint32_t **labels);
/* STREAMED only (else DST_ERR_ARG).  After dst_stream_collect: the collected batch, *n_records x n_loaded_groups entries per
 * array, in page-locked, library-owned memory that is valid until the next dst_stream_submit.  n_records is required;
 * within, summable and sum may be NULL.  DST_ERR_STATE when no batch has been collected since the last submit. */
int dst_stream_group_summary_batch(dst_stream *stream, size_t *n_records, const uint32_t **within,
                                   const uint32_t **summable, const double **sum);
/* A snapshot of everything kept so far (host memory): the cells (n_streamed_groups x n_loaded_groups), the LOADED table
 * (n_loaded x n_streamed_groups entries per array) and *records; every pointer may be NULL.  Without
 * DST_STREAM_GROUPS_LOADED the three rec_* pointers must be NULL, else DST_ERR_ARG.  Needs dst_stream_in_flight() == 0, else
 * DST_ERR_STATE; cells_cap or rec_cap below the entries of a non-NULL array: DST_ERR_CAPACITY.  The call may be repeated,
 * and streaming may go on afterwards. */
int dst_stream_group_summary_result(dst_stream *stream, dst_group_cell *cells, size_t cells_cap,
                                    uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum, size_t rec_cap,
                                    uint64_t *records);
/* ---- group summaries per column window ------------------------------------------------------------ */
/* dst_group_summary's cells and per-record tables INSIDE every column window, reduced next to the window sweep on the GPU:
 * pi per population and d_xy between populations along the genome (the means F_ST is formed from), a query's mean distance
 * to each group of reference sequences per window.  The state is n_windows x G_r x G_c cells, plus n_windows x n_rows x G_c
 * entries when a per-record array is wanted, whatever the record count; the n_windows x P result of dst_run_windows is
 * never written.  The definition is fixed to the bit and every accumulation is an integer one.
 *   sets, windows   exactly dst_window_summary's: square != 0 is slot 0 against itself (row_slot / col_slot ignored), the
 *            pairs i < j; else two different slots.  Windows are half-open, may overlap, repeat, be empty and come in any
 *            order; 1 <= n_windows <= DST_WINDOWS_MAX.  tn93 takes the per-window {A,T,G,C} counts counted by code.
 *   labels   exactly dst_group_summary's: a group below its count or DST_GROUP_NONE; in the square form row_group /
 *            n_row_groups serve both sides and col_group / n_col_groups are ignored.  Group counts are
 *            1 .. DST_WINDOW_GROUPS_MAX.
 *   payload  v of a pair in window w: bitwise the DST_OUT_DISTANCE entry dst_run_windows writes for it.
 *   result of window w: dst_group_summary's definition, word for word, applied to that window's payloads and the labels:
 *            link, q, "summable" and NaN; `pairs` from the group sizes alone (so the same in every window); `sum` the one
 *            conversion of the exact integer sum; min_bits / max_bits decoded from the sort key, the empty cell's quiet
 *            NaN or 0; both orders stored in the square, cell (a, a) the pairs inside a.
 *   cells    (n_windows x G_r x G_c entries, or NULL when a rec_* array is given) entry (w * G_r + a) * G_c + b.
 *   rec_within, rec_summable, rec_sum   (each n_windows x n_rows x G_c entries, or NULL) entry (w * n_rows + x) * G_c + g:
 *            window-major like every other window result, then dst_group_summary's row.
 *   cells_cap, rec_cap   the room of cells, and of each non-NULL rec_* array, in entries.
 * Consequences: for a set uploaded without caller base counts, the window [0, len) gives dst_group_summary's cells and
 * per-record tables bitwise.  With one group and every record assigned, cell (0, 0) of window w is dst_window_summary's
 * totals[w] and rec_*[w][x][0] its per-record entry, bitwise.  Within one window dst_group_summary's own consequences
 * hold: for a != b cell (a, b) is the sum of rec_* over the records of a, and cell (a, a) is half of that sum.
 * Errors are dst_window_summary's, in its order and with its messages, with these additions: after "unknown measure" a NaN
 * threshold; `cells` and all three rec_* NULL; a NULL row_group, or a NULL col_group in the rectangle; a group count of 0
 * or above DST_WINDOW_GROUPS_MAX (all DST_ERR_ARG).  Then the slots, the sets' state (a dst_upload_shared set is refused
 * as the other window calls refuse it), len >= 2^32, a bad window, sets of 2^32-1 records or more, as they are.  Then
 * DST_ERR_ARG for a label that is neither below its count nor DST_GROUP_NONE (dst_group_summary's message: the first such
 * record and its side); DST_ERR_ARG when n_windows x G_r x G_c exceeds 2^31 (whether or not `cells` is given: the device
 * keeps the cells), or n_windows x n_rows x G_c does and a per-record array is wanted; DST_ERR_CAPACITY, with nothing
 * written, when cells_cap or rec_cap is too small (each looked at only when its array is given); DST_ERR_NOMEM with the
 * byte count when the state (56 bytes per cell, 24 per per-record entry, 4 per label), the window table or tn93's count
 * table does not fit.
 * n_windows == 0, an empty row or column set, a square set of fewer than 2 records, no record of the column side (the
 * square: of the set) assigned, or the cells alone wanted while no row record is assigned: DST_OK, zero counts and sums,
 * min / max as for an empty cell, `pairs` still set from the group sizes, and no launch.  Synchronous on the context's
 * stream: one fused sweep-and-reduce launch family and one copy back.  A set with deferred planes gets them first; slots,
 * the path choice, dst_last_path, dst_last_launch and later results are untouched.  Single GPU, loaded sets only. */
#define DST_WINDOW_GROUPS_MAX 256u   /* most groups of one side in the per-window form */
int dst_window_group_summary(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot,
                             const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                             const uint32_t *row_group, uint32_t n_row_groups,
                             const uint32_t *col_group, uint32_t n_col_groups,
                             double threshold,
                             dst_group_cell *cells, size_t cells_cap,
                             uint32_t *rec_within, uint32_t *rec_summable, double *rec_sum, size_t rec_cap);
/* ---- per-site allele counts ------------------------------------------------------------------------- */
/* The column side of the library: per (site, group) how many records hold each base, counted from the set's base planes on
 * the GPU.  The site-frequency spectrum, minor-allele counts, a per-group consensus, which sites vary at all, and (through
 * dst_site_stats below) the segregating sites, Watterson's theta and the per-site pi of every window come from these
 * counts.  They are exact integers added with integer atomics: the result depends on no order.
 *   labels   group[x] for every record x of `slot`: a group below n_groups, or DST_GROUP_NONE (the record is counted
 *            nowhere).  group == NULL: one group that holds every record; n_groups must then be 1.  1 <= n_groups <=
 *            DST_GROUPS_MAX.
 *   counts   (host memory) entry ((s - site_begin) * n_groups + g) * DST_SITE_CLASSES + k for the sites site_begin <= s <
 *            site_end: k = 0..3 the records of group g whose code at site s is exactly A, T, G, C (the library's {A,T,G,C}
 *            order; the code's high nibble is one-hot), k = 4 those whose code names 2 or 3 bases (R M W S K Y V H D B).
 *            Records whose code is N, - or ? (high nibble 1111) are in no class: missing = the group's size - the five.
 *            cap_entries: the room of counts in entries.
 * Only the A, G, C, T planes are read: a lean set serves as it is, a set with deferred planes gets them first.  Padding
 * records and padding sites are never counted, whatever they hold.
 * Errors, in this order: DST_ERR_ARG for a NULL ctx or counts, a bad slot, a group count of 0 or above DST_GROUPS_MAX, NULL
 * labels with n_groups != 1; DST_ERR_STATE for a set not uploaded or one from dst_upload_shared (the window calls' refusal);
 * DST_ERR_ARG for site_begin > site_end or site_end > len, len >= 2^32, a set of 2^32-1 records or more, or a label that is
 * neither below n_groups nor DST_GROUP_NONE (the message names the first such record); DST_ERR_CAPACITY when cap_entries is
 * below (site_end - site_begin) x n_groups x 5, nothing written; DST_ERR_NOMEM with the byte count (4 bytes per entry and
 * per labelled record).  An empty site range, an empty set or no labelled record: DST_OK, the range's entries zero, no
 * launch.  Synchronous on the context's stream.  Slots, the path choice, dst_last_path, dst_last_launch and later results
 * are untouched.  Single GPU, loaded sets only.
 * DST_SITE_STRIP_RECORDS and DST_SITE_FLUSH_PERIOD describe the kernel, not the result: a workgroup counts
 * at most DST_SITE_STRIP_RECORDS records of one group, DST_SITE_FLUSH_PERIOD per thread, before it adds to the counts. */
#define DST_SITE_CLASSES 5
#define DST_SITE_FLUSH_PERIOD 15u
#define DST_SITE_STRIP_RECORDS 3840u   /* 256 threads x DST_SITE_FLUSH_PERIOD */
int dst_site_counts(dst_ctx *ctx, int slot, const uint32_t *group, uint32_t n_groups,
                    uint64_t site_begin, uint64_t site_end, uint32_t *counts, size_t cap_entries);
/* Pure host code: dst_site_counts' entries of the sites [site_begin, site_end) reduced to windows.  Windows are
 * dst_run_windows': half-open, they may overlap, repeat, be empty and come in any order; each must lie inside [site_begin,
 * site_end), else DST_ERR_ARG (the first such window decides; there is no context to carry a message).  out[w * n_groups + g];
 * cap: the room of out in entries, below n_windows x n_groups DST_ERR_CAPACITY with nothing written.  group_size[g] is
 * copied to `records`.  Per site s of the window and group g, with c_A, c_T, c_G, c_C the four base counts:
 *   m = c_A + c_T + c_G + c_C
 *   D = the sum over the six unordered base pairs of c_a x c_b (exact in uint64: m < 2^32)
 *   sites        the window's length
 *   called       the sites with m >= 2
 *   segregating  the called sites with at least two non-zero base counts
 *   pi_sum       the sum over the called sites, in ascending s from +0.0, of (double)D / (double)(m (m - 1) / 2): each
 *                conversion one rounding, then one division, then one addition
 *   theta_sum    the sum over the segregating sites, in ascending s from +0.0, of 1.0 / H[m - 1], with H[0] = 0 and
 *                H[k] = H[k - 1] + 1.0 / (double)k in double
 * compiled without fused multiply-add, like dst_finalize.  Watterson's theta per site is theta_sum / called and pi is
 * pi_sum / called.  This pi is the per-site estimator over single-base calls: every site weighs the same and a site's
 * pairs are those of its called records.  It is NOT the mean of the pairwise `raw` distances that dst_window_summary and
 * dst_window_group_summary sum, where every pair is divided by its own comparable sites.  Tajima's D is left out on
 * purpose: its variance term has no agreed form when m varies by site, and every variant is a function of these fields.
 * DST_ERR_ARG also for a NULL counts, group_size or out, NULL window arrays with n_windows > 0, n_groups == 0, or
 * site_begin > site_end. */
typedef struct {
    uint64_t records, sites, called, segregating;
    double theta_sum, pi_sum;
} dst_site_window;
int dst_site_stats(const uint32_t *counts, uint64_t site_begin, uint64_t site_end, uint32_t n_groups,
                   const uint64_t *win_begin, const uint64_t *win_end, uint32_t n_windows,
                   const uint64_t *group_size, dst_site_window *out, size_t cap);
/* ---- linkage disequilibrium between sites --------------------------------------------------------- */
/* Which mutations travel together: for a list of sites, four exact integers per pair of sites, from which r^2, D and D' are
 * fixed to the bit (PLINK's --r2, scikit-allel's rogers_huff_r on haploid calls).  The all-pairs job with the roles of
 * sites and records swapped: AND and popcount over bit vectors that run along the records.
 *   sites    sites[0..n_sites): 0-based sites of the set in `slot`, strictly ascending.  A site's place in the list is its
 *            POSITION p; pairs are pairs of positions p < q, numbered in canonical order (row-major, as dst_run_square
 *            numbers record pairs: dst_square_row_start(n_sites, p) + q - p - 1).
 *   allele   allele[p] in {0, 1, 2, 3}: the reference allele of position p in dst_site_counts' order A, T, G, C.
 *   records  group == NULL: every record takes part, and `which` must be 0.  Else group has one label per record and the
 *            records with group[x] == which take part.
 *   sets     for position p (site s) and a participating record x: C_p[x] = 1 iff x's code at s is exactly one base (the
 *            code's high nibble is one-hot: dst_site_counts' classes 0..3); M_p[x] = 1 iff C_p[x] and that base is not
 *            allele[p].  Ambiguity codes, N, - and ? are never called.
 *   tallies  per pair p < q four uint32: m = |C_p & C_q|, a = |M_p & C_q|, b = |C_p & M_q|, c = |M_p & M_q|.  Only the
 *            records with a single-base call at BOTH sites count for a pair (pairwise deletion, as in the distance measures).
 * dst_site_ld, the full form: for the positions row_begin <= p < row_end and every q > p, in canonical order, {m, a, b, c}
 * into `tallies` (host memory, 16 bytes per pair); cap_pairs: its room in pairs.
 * dst_site_ld_links: the pairs whose r^2 (dst_ld_finalize below) is not NaN and >= min_r2, in canonical order, nothing
 * reordered, handed to `sink` in chunks of at most DST_LD_CHUNK links: sink(user, first_link, n_links, pos_i, pos_j,
 * tallies), tallies 16 bytes per link.  dst_links' rules: the sink runs on the calling thread, its arrays are page-locked
 * buffers of the library's, valid during the call; a non-zero return stops the run with "stopped by sink" (DST_ERR_STATE);
 * sink == NULL counts only; *n_links (may be NULL) is the number of links delivered or counted.  max_pairs: the most site
 * pairs of one row slab (0: 2^24; at least one row per slab); the result does not depend on it.  min_r2: any double but
 * NaN; min_r2 <= 0 delivers every pair with a defined r^2.  The device decides r^2 >= min_r2 with dst_ld_finalize's
 * operations in their order, so a link is exactly a pair whose dst_ld_finalize r^2 passes.
 * Errors, in this order: DST_ERR_ARG for a NULL ctx, sites, allele or tallies, a bad slot, or group == NULL with which != 0;
 * DST_ERR_STATE for a set not uploaded or one from dst_upload_shared (the window calls' refusal); DST_ERR_ARG for a site
 * >= len or a list that is not strictly ascending (the message names the first such position), an allele above 3,
 * row_begin > row_end or row_end > n_sites, a set of 2^31 records or more, a NaN min_r2; DST_ERR_CAPACITY when cap_pairs is
 * below the row range's pairs, nothing written; DST_ERR_NOMEM with the byte count.  n_sites < 2, an empty row range or no
 * participating record: DST_OK without a launch (the full form's tallies are zero).  Synchronous on the context's stream.
 * Slots, the path choice, dst_last_path, dst_last_launch and later results are untouched; a set with deferred planes gets
 * them first.  Single GPU, loaded sets only. */
#define DST_LD_CHUNK (1u << 22) /* the most links of one dst_ld_sink call */
typedef int (*dst_ld_sink)(void *user, uint64_t first_link, uint64_t n_links, const uint32_t *pos_i, const uint32_t *pos_j,
                           const uint32_t *tallies);
int dst_site_ld(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                const uint32_t *group, uint32_t which, uint32_t row_begin, uint32_t row_end,
                uint32_t *tallies, size_t cap_pairs);
int dst_site_ld_links(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                      const uint32_t *group, uint32_t which, double min_r2, uint64_t max_pairs,
                      dst_ld_sink sink, void *user, uint64_t *n_links);
/* ---- banded LD and the LD-decay curve ---------------------------------------------------------------
 * The pairs within a distance along the genome (PLINK's --ld-window-kb) and one mean r^2 per distance bin, without walking
 * the whole triangle.  Sites, positions, alleles, records (group / which) and the tallies {m, a, b, c} are dst_site_ld's,
 * word for word.  Definitions, fixed to the bit:
 *   gap    of a pair of positions p < q: sites[q] - sites[p]; >= 1, the list is strictly ascending.
 *   band   of max_gap: the pairs with gap <= max_gap.  The band pairs of row p are the contiguous positions p < q <
 *          row_end[p]; row_end[p] >= p + 1 and row_end is non-decreasing.  The BAND ORDER is the canonical order restricted to
 *          the band.
 * dst_ld_band (pure host code, no context): row_end[0..n_sites) (may be NULL), *pairs = the band's pairs, *tiles = the
 * number of 64 x 64 position tiles (tile row p / 64, tile column q / 64) that hold at least one band pair (either may be
 * NULL).  `tiles` describes the kernels, not the result, like DST_SITE_STRIP_RECORDS: it is exactly the number of tiles the
 * band kernels launch work for in one pass over the band.  DST_ERR_ARG for NULL sites with n_sites > 0 or a list that is
 * not strictly ascending.
 * dst_site_ld_band, the full form: {m, a, b, c} of every band pair with row_begin <= p < row_end, in band order, 16 bytes
 * per pair into `tallies` (host memory); every entry is bitwise dst_site_ld's entry of that pair.  cap_pairs below the row
 * range's band pairs: DST_ERR_CAPACITY, nothing written.
 * dst_site_ld_links_band: dst_site_ld_links' arguments plus max_gap, the same sink contract and DST_LD_CHUNK windows.
 * Delivers exactly those links of dst_site_ld_links(min_r2) whose gap is <= max_gap, in the same order, with the same
 * pos_i, pos_j and tallies.  max_pairs bounds the BAND pairs of one row slab (0: 2^24; at least one row per slab) and never
 * changes the result.  max_gap >= sites[n_sites - 1] - sites[0] gives dst_site_ld_links' answer; max_gap = 0 gives no pair:
 * DST_OK, no launch.
 * dst_site_ld_decay: 1 <= bin_width, 1 <= n_bins <= DST_LD_DECAY_MAX_BINS.  A pair lies in bin gap / bin_width (integer
 * division); pairs whose bin is >= n_bins are left out: the call is banded at max_gap = n_bins x bin_width - 1.  No gap
 * reaches 2^32 - 1 (sites are uint32), so a bin_width above 2^32 - 1 is taken as 2^32 - 1: the same bins, and the product
 * cannot overflow.  bins[0..n_bins), cap: the room of `bins` in entries.  Per bin:
 *   pairs     the bin's pairs: a function of the list alone, filled even when nothing is launched
 *   defined   those whose dst_ld_finalize r^2 is not NaN
 *   links     those of them with r^2 >= min_r2: dst_site_ld_links' rule, the same operations in the same order
 *   r2_sum    with q = rint(r^2 x 2^DST_LD_SCALE_BITS) (round to nearest even; the product by a power of two is exact), the
 *             exact unsigned 64-bit sum of q over the bin's defined pairs, converted once to double and scaled by
 *             2^-DST_LD_SCALE_BITS (exact).  The mean r^2 of a bin is r2_sum / defined.
 * r^2 <= 1 up to a few ulp, so q <= 2^30 + 4 and the sum cannot overflow while the band holds at most 2^33 pairs; a band
 * above that is DST_ERR_ARG (from dst_ld_band's count, on the host).  Every accumulation across workgroups is an integer
 * atomic: the result depends on no order, on no slab size and on no kernel detail.  max_pairs only bounds the band pairs
 * whose tiles one launch covers (0: 2^24; whole tile rows, at least one).  No record takes part, n_sites < 2 or an empty
 * band: DST_OK, no launch, `pairs` filled, the rest zero.  DST_LD_DECAY_LOCAL_BINS describes the kernel, not the result: a tile
 * whose pairs span at most that many bins is gathered in on-chip memory and flushed once.
 * Errors of the three device calls: dst_site_ld's, in its order and with its messages under the calls' own names ("site ld
 * band", "site ld links band", "site ld decay"; the NULL output of the decay call is `bins`); then DST_ERR_ARG for a NaN
 * min_r2, bin_width 0, n_bins 0 or above DST_LD_DECAY_MAX_BINS, a band above 2^33 pairs; DST_ERR_CAPACITY; DST_ERR_NOMEM with
 * the byte count.  Slots, the path choice, dst_last_path, dst_last_launch and later results are untouched; a set with
 * deferred planes gets them first; a set from dst_upload_shared is refused as by dst_site_ld.  Single GPU, loaded sets only. */
#define DST_LD_SCALE_BITS 30        /* r2_sum counts in units of 2^-30 */
#define DST_LD_DECAY_MAX_BINS 4096u /* the most bins of one dst_site_ld_decay call */
#define DST_LD_DECAY_LOCAL_BINS 512u /* a tile spanning at most this many bins accumulates on chip */
typedef struct {
    uint64_t pairs, defined, links;
    double r2_sum;
} dst_ld_bin;
int dst_ld_band(const uint32_t *sites, uint32_t n_sites, uint64_t max_gap, uint32_t *row_end, uint64_t *pairs, uint64_t *tiles);
int dst_site_ld_band(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                     const uint32_t *group, uint32_t which, uint64_t max_gap, uint32_t row_begin, uint32_t row_end,
                     uint32_t *tallies, size_t cap_pairs);
int dst_site_ld_links_band(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                           const uint32_t *group, uint32_t which, double min_r2, uint64_t max_gap, uint64_t max_pairs,
                           dst_ld_sink sink, void *user, uint64_t *n_links);
int dst_site_ld_decay(dst_ctx *ctx, int slot, const uint32_t *sites, const uint8_t *allele, uint32_t n_sites,
                      const uint32_t *group, uint32_t which, double min_r2, uint64_t bin_width, uint32_t n_bins,
                      uint64_t max_pairs, dst_ld_bin *bins, size_t cap);
/* Pure host code, compiled without fused multiply-add: r^2, D and D' of n_pairs tallies {m, a, b, c} as the two calls above
 * produce them (c <= a, b <= m < 2^31).  Any output pointer may be NULL.  Per pair, all integer arithmetic exact in 64 bits
 * (which is why the calls refuse sets of 2^31 records or more):
 *   num    = (int64)m c - (int64)a b          A = a (m - a)          B = b (m - b)
 *   D      = (double)num / (double)(m m), NaN when m = 0
 *   r2     = ((double)num (double)num) / ((double)A (double)B), NaN when A = 0 or B = 0 (a site that is monomorphic among
 *            the pair's called records)
 *   Dprime = (double)num / (double)X, X = min(a (m - b), (m - a) b) when num >= 0 and X = min(a b, (m - a) (m - b)) when
 *            num < 0; NaN when A = 0 or B = 0 (else X is never 0)
 * each conversion one rounding, each product or quotient one rounding, in the order written.  The integer conversions are
 * exact below 94,906,266 records (m^2 < 2^53); beyond that each is the one correctly rounded conversion, and the rule is not
 * tested there.  DST_ERR_ARG for NULL tallies with n_pairs > 0. */
int dst_ld_finalize(const uint32_t *tallies, uint64_t n_pairs, double *r2, double *d, double *dprime);
/* Pure host code: from dst_site_counts' entries (n_sites sites, n_groups groups) of group g, per site: allele = the class
 * with the largest of the four base counts A, T, G, C (ties: the smallest class index), major_count = that count,
 * other_count = the sum of the other three (m - major_count).  major_count and other_count may be NULL.  DST_ERR_ARG for a
 * NULL counts or allele with n_sites > 0, or g >= n_groups. */
int dst_site_major(const uint32_t *counts, uint64_t n_sites, uint32_t n_groups, uint32_t g, uint8_t *allele,
                   uint32_t *major_count, uint32_t *other_count);
/* ---- minimum spanning tree --------------------------------------------------------------------- */
/* The single-linkage picture for every threshold at once: the minimum spanning tree (forest) of one set (slot 0, n
 * records), as GrapeTree- and PHYLOViZ-style viewers draw it, computed next to the values on the GPU by Boruvka rounds
 * that recompute the triangle in row slabs: O(n) device memory beside one slab, so it also serves sets whose square
 * cannot be held.  The definition is fixed to the bit:
 *   graph   an edge {i, j}, i < j, for every pair whose DST_OUT_DISTANCE payload v (the value dst_run_square returns,
 *           bit-identical on every path) is not NaN.  +inf is an edge; -0.0 is +0.0; NaN is never an edge (as in
 *           dst_clusters, where NaN never links).
 *   order   edges are ordered by (key(v), i, j) lexicographically, key = dst_nearest's sort key: n / n_high (int64)
 *           (uint64)v ^ 2^63; f64 -0.0 -> the key of +0.0, any other non-NaN value the order-preserving flip (v >= 0:
 *           bits | 2^63, v < 0: ~bits).  A strict total order, so the minimum spanning forest under it is unique: the
 *           forest Kruskal's algorithm builds when it takes the edges in that order.
 *   result  that forest's edges in ascending order: *n_edges = n - c of them, c the number of connected components of
 *           the non-NaN graph (a connected graph: n - 1).  It depends neither on the path nor on max_pairs.
 * Consequence: for every T, the connected components of the result's edges with v <= T (by dst_clusters' rule) are
 * exactly dst_clusters(T)'s clusters: the edges in order are the single-linkage dendrogram.
 *   max_pairs   0: the default slab bound (2^25 pairs); else the most pairs of one row slab, as in dst_clusters
 *   edge_i, edge_j   the edges, edge_i[e] < edge_j[e] (host memory, required)
 *   values      NULL, or the edges' DST_OUT_DISTANCE payloads: bitwise what dst_run_square returns for the pair
 *   tallies     NULL, or dst_tally_width(measure) DST_OUT_TALLY words per edge (dst_finalize -> the reference's bits;
 *               tn93: base counts in (i, j) order)
 *   cap         the room of every non-NULL output in entries; below n - 1 (n >= 2): DST_ERR_CAPACITY, whatever the
 *               forest turns out to hold
 *   rounds      the Boruvka rounds that added edges (at most ceil(log2 n)), or NULL; n_edges may be NULL too
 * n < 2: DST_OK, 0 edges, 0 rounds.  DST_ERR_ARG: an unknown measure, a NULL edge_i or edge_j, n >= 2^32-1;
 * DST_ERR_STATE: slot 0 is not uploaded.  Synchronous on the context's stream.  Every round computes the triangle once
 * more (row slabs, as dst_clusters); one more sweep as tallies serves values / tallies and is skipped when both are NULL.
 * Slots, the path choice and later dst_run_square results are untouched.  Single GPU, loaded set only (not dst_stream). */
int dst_mst(dst_ctx *ctx, int measure, uint64_t max_pairs, uint32_t *edge_i, uint32_t *edge_j, void *values,
            uint32_t *tallies, size_t cap, uint64_t *n_edges, uint32_t *rounds);
/* ---- neighbour-joining trees ------------------------------------------------------------------- */
/* The neighbour-joining (NJ) tree of n >= 3 records, built on the GPU from the square it holds, with the arithmetic fixed
 * below so that a restatement in any language reproduces it bit for bit.  Every expression is evaluated in the order
 * written (the library is compiled -ffp-contract=off: no fused multiply-add).
 *
 * Input.  dst_nj: slot 0 (n records); D(i, j) is the pair's DST_OUT_DISTANCE payload for `measure` (f64 as is, int64 of
 * n / n_high converted to double), bit-identical on every path, so the tree depends neither on the path nor on
 * max_pairs (the most pairs of one row slab of the fill; 0: the default, as in dst_clusters).  dst_nj_matrix: a host
 * n x n row-major matrix of which only the strict upper triangle is read.  D(i, i) = +0.0.
 *
 * Active list.  The active nodes form a list, initially records 0 .. n-1 in order; m is its length and "position" a place
 * in it.  r_x = sum of d(x, k) over active k != x, summed left to right in position order from +0.0; computed so at the
 * start and at every compaction.  (Adding the +0.0 diagonal gives the same bits: a sum that starts at +0.0 is never
 * -0.0.  Payloads can be -0.0.)
 *
 * One round, while m > 3:
 *   0. compaction: let P be the stored dimension (initially n); when m <= floor(3P/4), the matrix is compacted to the
 *      active nodes in their order, P := m, and every r is recomputed as above.  The schedule depends on (n, m) only.
 *   1. the pair: for positions a < b, Q(a, b) = ((double)(m-2) * d_ab - r_a) - r_b; the smallest Q, compared through
 *      nn_key (the sort key of dst_nearest: -0 equals +0, NaN sorts last), ties to the smallest (a, b) in lexicographic
 *      position order
 *   2. branch lengths: delta_a = d_ab * 0.5 + (r_a - r_b) / (double)(2*(m-2)); delta_b = d_ab - delta_a
 *   3. a new internal node u takes position a; b leaves the list
 *   4. for every other active k: d_uk = ((d_ak + d_bk) - d_ab) * 0.5; d_uu = +0.0
 *   5. for every other active k: r_k = ((r_k - d_ak) - d_bk) + d_uk; r_u = ((r_a + r_b) - (double)m * d_ab) * 0.5 (the
 *      closed form of the sum of d_uk)
 * The last round (m = 3, positions x < y < z) joins the three at the root: delta_x = ((d_xy + d_xz) - d_yz) * 0.5,
 * delta_y = ((d_xy + d_yz) - d_xz) * 0.5, delta_z = ((d_xz + d_yz) - d_xy) * 0.5.  Negative branch lengths are kept as
 * computed (NJ gives them on non-additive data).  With integer measures, or any matrix of small integers, every step
 * above is exact in f64 (sums of integers, halves of them, and a quotient that an additive matrix makes exact).
 *
 * Output.  Leaves are nodes 0 .. n-1, the internal node made in round s is n + s, the root is 2n - 3 (so the ids give the
 * order of the joins).  parent[x] and length[x] (the edge from x to its parent) for 2n - 2 nodes; the root has parent
 * UINT32_MAX and length 0.  cap: the room of both arrays in entries, below 2n - 2 DST_ERR_CAPACITY.
 *
 * Errors: n < 3 or n >= 2^31, a NULL pointer or an unknown measure: DST_ERR_ARG; a non-finite D: DST_ERR_STATE from
 * dst_nj (the context's message names the first pair in canonical order), DST_ERR_ARG from dst_nj_matrix; slot 0 not
 * uploaded: DST_ERR_STATE; device memory for the square (8 n^2 bytes, plus 8 floor(3n/4)^2 for the compaction): DST_ERR_NOMEM
 * with the byte count in the message.  Synchronous on the context's stream; single GPU, loaded set only (not dst_stream). */
int dst_nj(dst_ctx *ctx, int measure, uint64_t max_pairs, uint32_t *parent, double *length, size_t cap);
int dst_nj_matrix(dst_ctx *ctx, const double *d, uint64_t n, uint32_t *parent, double *length, size_t cap);
/* Newick text of a dst_nj tree (host only, no GPU): "(c1,c2,c3);\n" at the root, children in ascending node id, each
 * node written as name:length (internal nodes as (children):length), lengths exactly as dst_format_distance prints an
 * f64 distance ({:.12}).  Leaf r is named chars[offsets[r] .. offsets[r+1]) (offsets: n + 1 entries, as dst_set_ids); a
 * name that is empty or holds whitespace or any of ()[]':;, is single-quoted with every ' doubled.  *len receives the
 * text's length (no NUL is written); cap below it: DST_ERR_CAPACITY, nothing written (out may be NULL with cap 0).
 * DST_ERR_ARG: n < 3, a NULL pointer, decreasing offsets, or a malformed parent array (an index out of range, not exactly
 * one root, a cycle, a leaf with children, an internal node without 2 children or a root without 3). */
int dst_newick(uint64_t n, const uint32_t *parent, const double *length, const char *chars, const uint64_t *offsets,
               char *out, size_t cap, size_t *len);

/* ---- hierarchical-clustering dendrograms ------------------------------------------------------------ */
/* The rooted dendrogram of n >= 2 records under a Lance-Williams linkage (UPGMA, WPGMA, complete linkage), built on the
 * GPU from the square it holds, with the arithmetic fixed below so that a restatement in any language reproduces it bit
 * for bit.  Every expression is evaluated in the order written (the library is compiled -ffp-contract=off).
 *
 * Input.  dst_dendrogram: slot 0 (n records); D(i, j) is the pair's DST_OUT_DISTANCE payload for `measure` (f64 as is,
 * int64 of n / n_high converted to double), bit-identical on every path, so the tree depends neither on the path nor on
 * max_pairs (the most pairs of one row slab of the fill; 0: the default, as in dst_nj).  dst_dendrogram_matrix: a host
 * n x n row-major matrix of which only the strict upper triangle is read.
 *
 * State.  Every active cluster has a slot (the smallest record index it contains), a node id, a size s (an integer)
 * and a height h.  Initially record i is the cluster of slot i, node i, s = 1, h = +0.0.
 *
 * Round t = 0 .. n-2:
 *   1. the pair: over active slots a < b, the smallest (nn_key(d_ab), a, b) lexicographically; nn_key is the sort key
 *      of dst_nearest (-0.0 equals +0.0).  A strict total order: the tree is unique.
 *   2. the node: u = n + t, h_u = d_ab * 0.5; length[node(a)] = h_u - h_a, length[node(b)] = h_u - h_b; the parent of
 *      both is u
 *   3. u takes slot a, slot b leaves; s_u = s_a + s_b
 *   4. for every other active slot k, d_uk (stored for both (a, k) and (k, a)):
 *        DST_LINK_AVERAGE  (UPGMA)  ((double)s_a * d_ak + (double)s_b * d_bk) / (double)(s_a + s_b)
 *        DST_LINK_WEIGHTED (WPGMA)  (d_ak + d_bk) * 0.5
 *        DST_LINK_COMPLETE          d_ak < d_bk ? d_bk : d_ak
 *
 * Output.  Leaves are nodes 0 .. n-1, the node made in round t is n + t, the root is 2n - 2.  parent[x], length[x] (the
 * edge from x to its parent) and height[x] (h_x; leaves +0.0) for 2n - 1 nodes; the root has parent UINT32_MAX and
 * length 0.  height may be NULL.  cap: the room of every non-NULL array in entries, below 2n - 1 DST_ERR_CAPACITY.
 * Lengths are kept as computed: under average and weighted linkage a rounding can make one a few ulps negative.  Complete
 * linkage is pure selection: every value in it is an input value or half of one, and heights never decrease.
 * row_scans: NULL, or the number of whole-row scans of the square the call made (the n that build the row-minimum
 * cache included); a diagnostic, not part of the bit-fixed result.
 *
 * Errors: n < 2 or n >= 2^31, an unknown linkage or measure, a NULL ctx, parent or length: DST_ERR_ARG; a non-finite D:
 * DST_ERR_STATE from dst_dendrogram (the message names the first pair in canonical order, as dst_nj's), DST_ERR_ARG from
 * dst_dendrogram_matrix; slot 0 not uploaded: DST_ERR_STATE; device memory for the square (8 n^2 bytes; there is no
 * compaction buffer): DST_ERR_NOMEM with the byte count in the message.  Synchronous on the context's stream; single
 * GPU, loaded set only (not dst_stream).  Slots, the path choice and later results are untouched. */
typedef enum { DST_LINK_AVERAGE = 0, DST_LINK_WEIGHTED = 1, DST_LINK_COMPLETE = 2 } dst_linkage;
int dst_dendrogram(dst_ctx *ctx, int measure, int linkage, uint64_t max_pairs, uint32_t *parent, double *length,
                   double *height, size_t cap, uint64_t *row_scans);
int dst_dendrogram_matrix(dst_ctx *ctx, const double *d, uint64_t n, int linkage, uint32_t *parent, double *length,
                          double *height, size_t cap, uint64_t *row_scans);
/* Newick text of a dst_dendrogram tree (host only, no GPU): "(c1:l1,c2:l2);\n" with a binary root, n >= 2 leaves and
 * 2n - 1 nodes; everything else as dst_newick (children in ascending node id, {:.12} lengths, the same quoting, *len and
 * cap).  DST_ERR_ARG: n < 2, a NULL pointer, decreasing offsets, or a malformed parent array (an index out of range, not
 * exactly one root, a cycle, a leaf with children, an internal node, the root included, without exactly 2 children). */
int dst_newick_rooted(uint64_t n, const uint32_t *parent, const double *length, const char *chars,
                      const uint64_t *offsets, char *out, size_t cap, size_t *len);

/* ---- bootstrap support of neighbour-joining trees ------------------------------------------------------------------ */
/* Replicate columns.  Replicate r (0-based) of an alignment of len sites has len columns; its column c is source column
 * col(seed, r, c), from SplitMix64 output number k = r * len + c of a generator seeded with `seed` (all mod 2^64):
 *   z = seed + (k + 1) * 0x9E3779B97F4A7C15
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   z =  z ^ (z >> 31)
 *   col = the high 64 bits of the 128-bit product z * len
 * dst_bootstrap_columns (host only, no GPU) writes the len columns of one replicate; the device computes the same
 * function (one definition serves both). */
void dst_bootstrap_columns(uint64_t seed, uint32_t replicate, uint64_t len, uint32_t *cols);
/* Bootstrap support of a main tree.  codes: n x len host Paradis bytes, rows row_stride bytes apart (as for dst_upload),
 * copied to the device once per call.  Replicate tree: exactly the tree dst_nj would return with the replicate alignment
 * uploaded to slot 0 (tn93 base counts counted by code from the replicate), so it depends on neither the path nor
 * max_pairs.  parent: the main tree in dst_nj form on n leaves, validated as dst_newick validates it.  Each internal
 * non-root node x (n <= x < 2n - 3) defines one split, the leaves below x or their complement, whichever side does not
 * hold leaf 0; support[x] = the number of replicates whose tree holds that split as an unrooted bipartition (compared
 * exactly; zero-length edges count).  Leaves and the root get UINT32_MAX.  cap: the room of support in entries (below
 * 2n - 2: DST_ERR_CAPACITY).  rep_parent: NULL, or replicates x (2n - 2) entries that receive every replicate's parent
 * array in order.  replicates in 1..=10000.
 * Per replicate, on the context's stream: resample (on the device, from the call's copy of the codes), pack, fill the
 * square, the NJ rounds; the split count runs on the host.  Slots 0 and 1 are neither read nor changed.
 * Errors: DST_ERR_ARG for a bad argument or tree; DST_ERR_STATE when a replicate has a non-finite distance (raw NaN for a
 * record without a resolved site in the replicate, jc69 inf): the message names the replicate and the first pair in
 * canonical order; DST_ERR_INVALID_CODE as dst_upload; DST_ERR_NOMEM as dst_nj.  Synchronous on the context's stream. */
int dst_nj_bootstrap(dst_ctx *ctx, int measure, const uint8_t *codes, size_t n, size_t len, size_t row_stride,
                     uint32_t replicates, uint64_t seed, uint64_t max_pairs, const uint32_t *parent, uint32_t *support,
                     uint32_t *rep_parent, size_t cap);
/* dst_newick with support labels: an internal non-root node x is written (children)S:length, S = support[x] in decimal;
 * leaves and the root as dst_newick writes them.  support == NULL: byte for byte dst_newick. */
int dst_newick_support(uint64_t n, const uint32_t *parent, const double *length, const char *chars,
                       const uint64_t *offsets, const uint32_t *support, char *out, size_t cap, size_t *len);
/* Page-locked host memory for the *_host forms' output buffers (copy-back by DMA at link speed instead
 * of through a pageable bounce buffer).  Free with dst_host_free. */
int dst_host_alloc(size_t bytes, void **ptr);
int dst_host_free(void *ptr);
/* bytes a run writes */
size_t dst_out_bytes(int measure, int out_kind, uint64_t n_pairs);
/* milliseconds of the pair kernel of the most recent run and of the pack kernel of the most recent
 * upload on this context, from HIP events recorded on the launch stream (bench.py's roofline leg);
 * *finalize_ms is always 0: finalisation is fused into the pair kernel's epilogue */
int dst_last_kernel_ms(dst_ctx *ctx, float *pair_ms, float *finalize_ms, float *pack_ms);

/* The same over many launches without waiting for the device after each: means over the pair-kernel and pack-kernel
 * launches of this context since the last call with reset != 0 (at most the 64 most recent of each; waits for the last
 * one).  bench.py times its steps with one call at the end of the timed region. */
int dst_kernel_ms_mean(dst_ctx *ctx, int reset, float *pair_ms, int *pair_launches, float *pack_ms, int *pack_launches);

/* Diagnostic: the tile schedule one pair-kernel launch would use for rows [row_begin,row_end)
 * against n_cols records — (i0, j0) per workgroup in launch order, idle fillers as i0 = 2^32-1.
 * tile_rows/tile_cols receive the tile shape of (measure, variant).  ij may be NULL to query
 * *count only.  Pure host code (no GPU needed). */
int dst_plan_tiles(int square, uint64_t row_begin, uint64_t row_end, uint64_t n_cols, int measure,
                   int variant, uint32_t *ij, size_t cap_tiles, size_t *count, int *tile_rows,
                   int *tile_cols);

/* What ONE site contributes to each tally of `measure` for the code pair (q, t): the bodies of the site loops
 * of src/measures.rs:14-23, 56-66, 85-107, 156-175 (out has dst_tally_width(measure) entries, each 0 or 1).
 * Pure host code; the consensus path's tables are built from it. */
int dst_site_tallies(int measure, uint8_t q, uint8_t t, int *out);

/* ---- host finalisation in the reference's f64 operation order --------------------------- */
/* tallies: dst_tally_width(measure) uint32 per pair.  q_counts/t_counts: {A,T,G,C} of record_1 /
 * record_2 (tn93 only, else may be NULL).  Writes the FloatInt payload: *as_int for n/n_high,
 * *as_float otherwise (glibc log/sqrt, -ffp-contract=off => bit-identical to src/measures.rs). */
int dst_finalize(int measure, const uint32_t *tallies, const uint32_t *q_counts,
                 const uint32_t *t_counts, double *as_float, int64_t *as_int);
/* One TSV field as gather_write prints it (src/lib.rs:626-633): `{}` / `{:.12}` incl. Rust's
 * "NaN", "inf", "-inf", "-0.000000000000".  snprintf semantics: returns the length of the full text
 * (no NUL counted); if that is >= cap the text was truncated to cap-1 characters. */
int dst_format_distance(int measure, double as_float, int64_t as_int, char *buf, size_t cap);

/* ---- TSV text on the device ---------------------------------------------------------------- */
/* gather_write()'s output (src/lib.rs:612-644) produced by the GPU: "id1\tid2\tvalue\n" per pair of rows
 * [row_begin, row_end) in canonical order, `{}` / `{:.12}` exactly as dst_format_distance prints one value.
 * dst_set_ids gives the record ids of the packed set in `slot` (record r: chars[offsets[r] .. offsets[r+1])); they
 * stay valid across uploads of the same record count.  The text goes to `out` (host memory; page-locked memory
 * from dst_host_alloc copies at link speed), *len receives its length.  At most 2^31 pairs, 65,535 rows and 4 GB of
 * text per call.  DST_ERR_CAPACITY: `capacity` is too small; DST_ERR_STATE: a value has no short text (|v| >= 1.8e7,
 * which no distance reaches): format those rows on the host.  dst_text_rect: swap_ids != 0 prints the column
 * record's id first (the value is the one dst_run_rect gives).
 *
 * The text is byte for byte what the reference prints.  n / n_high / raw: the device's values are the reference's bits.
 * jc69 / k80 / tn93 (f64::ln = the host's libm, src/measures.rs:76, 109-112, 187): the device finalises the pair's
 * integer tallies with its own logarithm (within a few ulp of libm's) and notes every value that lies within 2^-47 |v| of
 * a rounding boundary of the 12th decimal; those pairs (~1e-4 of a low-diversity alignment's lines) are re-finalised on
 * the host by dst_finalize and their digits overwritten before the call returns — any value within the guard of a line
 * that was NOT noted prints the same text.  DST_ERR_STATE also when more than 1/16 of a slab's values are near ties
 * (distances far above 1): format that slab on the host. */
int dst_set_ids(dst_ctx *ctx, int slot, const char *chars, const uint64_t *offsets, uint64_t n);
/* running totals over this context's dst_text_* calls: values noted as near ties, and how many of those the host's
 * finalisation printed differently from the device's (either pointer may be NULL) */
int dst_text_stats(const dst_ctx *ctx, uint64_t *near_ties, uint64_t *rewritten);
int dst_text_square(dst_ctx *ctx, int measure, uint64_t row_begin, uint64_t row_end, char *out, size_t capacity,
                    size_t *len);
int dst_text_rect(dst_ctx *ctx, int measure, int row_slot, int col_slot, uint64_t row_begin, uint64_t row_end,
                  int swap_ids, char *out, size_t capacity, size_t *len);

typedef enum { DST_MATRIX_TSV = 0, DST_MATRIX_PHYLIP = 1 } dst_matrix_style;
/* Rows [row_begin, row_end) of a distance matrix as text, formatted on the GPU: per row "<id>" then "<sep><value>" per
 * column, then '\n' (sep '\t' for TSV, ' ' for PHYLIP); header lines are the caller's.  square != 0: slot 0 against
 * itself, every column incl. the diagonal; square == 0: row_slot x col_slot, row_slot != col_slot.  Ids as for
 * dst_text_* (dst_set_ids).
 *
 * Cell (i, j) is exactly the text dst_text_* prints for that pair (dst_format_distance of dst_finalize): square, both
 * (i, j) and (j, i) are the canonical pair (min(i, j), max(i, j)) — tn93 takes the base counts in that order — so the
 * matrix is symmetric byte for byte; the diagonal (i, i) is the measure of record i against itself (0 / 0.000000000000
 * for a record with a resolved site, NaN for raw of a record without one: not a constant).  square == 0: cell (i, j) is
 * row record i against column record j, as dst_text_rect prints it.  Near ties are handed to the host as for dst_text_*.
 * Limits as for dst_text_*: at most 2^31 cells, 65,535 rows and 4 GB of text per call.  DST_ERR_CAPACITY: `capacity` is
 * too small; DST_ERR_STATE: a set or its ids are missing, a value has no short text (|v| >= 1.8e7) or more than 1/16 of
 * the cells are near ties (format those rows on the host); DST_ERR_ARG: a bad slot, range, style or measure, or
 * square == 0 with equal slots. */
int dst_text_matrix(dst_ctx *ctx, int measure, int square, int row_slot, int col_slot, uint64_t row_begin,
                    uint64_t row_end, int style, char *out, size_t capacity, size_t *len);

#ifdef __cplusplus
}
#endif
#endif /* DISTANCE_HIP_H */
