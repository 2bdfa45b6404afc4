// dst_ctx.h — the context behind the C ABI and the helpers its translation units share
// (dst_api.cpp: uploads and runs, dst_analysis.cpp: the slab-driven analyses, dst_stream.cpp: the stream-mode pipeline,
// dst_gather.cpp: multi-GPU gather).
#pragma once
#include <string>
#include <vector>

#include "dst_internal.h"

using namespace dst;

struct dst_ctx {
    ~dst_ctx();   // (dst_api.cpp; after dst_destroy's wait for the device)
    int device = 0;
    hipStream_t stream = nullptr;   // the context's own: the one stream handle it ever synchronises
    DeviceSet set[2];
    DeviceSet boot;   // dst_nj_bootstrap's replicate: packed like a slot, never one (freed when the call ends)
    // staging for host uploads / unaligned device inputs
    Grown<uint8_t> stage;
    Grown<unsigned long long> d_first_bad;
    // what an upload reports to the host (first invalid byte, the sample's statistics, the list totals): written by the
    // device into this page-locked block, so the upload's one synchronisation needs no device-to-host copy
    Grown<unsigned long long, true> h_report;
    unsigned long long *d_report = nullptr;   // (the device's address of h_report)
    // Streams other than its own the context only ever sees as an argument of the call that brought them (a caller's,
    // a dst_stream's).  What outlives that call is a MARK: an event of the context's, recorded behind the stream's
    // latest pair launch (note_run), and the handle's value as a key that is compared and never handed back to the
    // runtime.  So a stream may be destroyed as soon as the work queued on it has completed.  A new stream that gets a
    // destroyed stream's handle value re-records that stream's mark: a later point of a stream whose earlier work was
    // complete, which is what a waiter wants.  A dst_stream takes the marks of its three streams with it when it closes
    // (forget_stream): the runtime's event remembers the stream it was recorded on, and asking it about an event whose
    // stream is gone reads freed memory.
    struct Mark {
        uint64_t id = 0;
        hipStream_t key = nullptr;
        Event event;
    };
    std::vector<Mark> marks;   // one per distinct stream seen; trimmed of completed ones when a new stream comes (mark_of)
    uint64_t mark_ids = 0;
    // tile schedules already on the device, keyed by the launch geometry (multi-GPU runs cycle
    // through a few sub-slab ranges every step: no host sync or H2D on a hit)
    struct Schedule {
        bool square = false;
        uint64_t rb = 0, re = 0, ncols = 0;
        int bm = 0, bn = 0;  // dense tile shape; consensus-path tile lists: bm = rows per tile, bn = -1
        uint32_t nblocks = 0;
        Grown<> d_blocks;
        uint64_t last_use = 0;
        std::vector<uint64_t> users;   // the marks (by id) of the streams whose launches read it: waited for before its buffer is recycled
    };
    std::vector<Schedule> schedules;
    uint64_t schedule_clock = 0;
    int variant = 0;
    int path = DST_PATH_AUTO;         // dst_set_path
    double prep_min_work = 2.0e10;    // dst_set_prep_threshold: site comparisons below which DST_PATH_AUTO stays dense unasked
    int last_path = DST_PATH_DENSE;   // what the most recent run used
    dst_launch_info last_launch = {-1};   // ... and which kernel variant its pair launch was (dst_last_launch; path -1: none yet)
    // consensus path: tables, counters and scratch shared by the two sets
    Grown<ConsensusLut> d_lut;
    Grown<unsigned long long> d_total;   // [0] list entries, [1] overflow entries (the text path sums its lengths here too)
    Grown<uint32_t> scan_tmp;
    Grown<> hot_tally;   // hybrid path: the dense kernels' tallies of the hot columns
    Event hot_free;      // recorded after the last reader of `hot_tally`
    // cross-stream ordering of derived data (dst_api.cpp: publish_prep / order_after_prep / wait_for_other_runs)
    Event prep_event;
    hipStream_t prep_stream = nullptr;   // where prep_event was last recorded: a key, like Mark::key
    Grown<> host_out;   // device staging of the *_host run forms
    int ksplit = 0;  // 0 = automatic split-L factor, >= 1 forced
    Grown<uint32_t> scratch;   // partial-tally meeting buffer of split-L f64 runs
    Event scratch_free;        // recorded after the last reader of `scratch`
    // TSV text on the device (dst_text.hip): the sets' record ids and scratch
    struct Ids {
        Grown<uint32_t> off;   // [n + 1] into chars
        Grown<char> chars;
        uint64_t n = 0;
    } ids[2];
    Grown<> text_res;             // the slab's results (8 B per pair) or tallies (<= 16 B per pair)
    Grown<> text_num;             // 32-byte number records
    Grown<uint32_t> text_len;     // line lengths -> offsets
    Grown<uint32_t> text_scan;
    Grown<char> text_buf;
    Grown<uint32_t> text_flag;    // [0] a value without a short text, [1] near ties noted, [2] placed (dst_text_matrix)
    Grown<> text_ties;            // the slab's near ties (dst_text.hip: NearTie), device and page-locked host copies
    Grown<void, true> text_ties_host;
    // the sets' {A,T,G,C} counts on the host (tn93 near ties are re-finalised there), valid while the epoch matches
    std::vector<uint32_t> text_counts[2];
    uint64_t text_counts_epoch[2] = {~0ull, ~0ull};
    uint64_t text_near_ties = 0, text_patched = 0;   // running totals (dst_text_stats)
    // dst_upload_shared (dst_shared.cpp): this rank's exchange block, everybody's blocks, and what the last exchange told
    struct Shared {
        Grown<> send, recv;
        Grown<uint32_t> off_local;
        uint64_t last_biggest = 0;   // entries of the largest block of the previous shared upload (sizes the next one)
        uint64_t uploads = 0, fallbacks = 0;
    } shared[2];
    // the analyses (dst_analysis.cpp): the one slab scratch their pair kernels write, DST_OUT_TALLY or DST_OUT_DISTANCE as
    // the call needs (a call owns it until it returns, and every call waits for the stream before it does)
    Grown<> pair_slab;
    Grown<> nn_lists;       // dst_nearest: the running lists; dst_nearest_windows: the lists of one slab
    Grown<> cl_work;        // dst_clusters: the parent array + link counter
    Grown<> rep_work;       // dst_representatives: rep, and the values and tallies when they are wanted
    Grown<> mst_work;       // dst_mst: the component, best-edge and edge-list arrays
    Grown<> dg_work;        // dst_dendrogram: the O(n) state beside the per-call square
    // dst_links: the block counts / offsets and one chunk of outputs on the device, the same chunk in page-locked host memory
    Grown<> links_work;
    Grown<char, true> links_host;
    // dst_pair_sites: one batch of pairs with its counts and offsets, one window of entries, and both again in page-locked
    // host memory
    Grown<char> ps_batch, ps_window;
    Grown<char, true> ps_batch_host, ps_window_host;
    // dst_run_pairs: one batch of list entries (indices, slab positions, values, tallies) on the device and again in
    // page-locked host memory
    Grown<char> rp_batch;
    Grown<char, true> rp_batch_host;
    // dst_run_windows / dst_window_base_counts: the window table on the device and in page-locked memory, and the per
    // (window, record) base counts (tn93)
    Grown<uint2> win_table;
    Grown<uint2, true> win_table_host;
    Grown<uint4> win_counts;
    // dst_window_summary: the per (window, record) accumulators and the windows' totals, and their page-locked copy
    Grown<> win_summary_work;
    Grown<char, true> win_summary_host;
    // dst_window_group_summary: the labels, the per-window cells and the per (window, record, group) accumulators, and
    // their page-locked copy
    Grown<> win_group_work;
    Grown<char, true> win_group_host;
    // dst_site_counts: the counts, the record list and the strips on the device; the list's and strips' page-locked staging
    Grown<> site_work;
    Grown<char, true> site_host;
    // dst_site_ld / dst_site_ld_links: the transposed vectors, the list's tables, one slab of tallies and the links' counts,
    // offsets and one window of outputs on the device; the tables' staging and that window again in page-locked memory
    Grown<> ld_work;
    Grown<char, true> ld_host;
    Grown<> summary_work;   // dst_summary: the per-record counters and accumulators, the histogram and the totals
    // dst_group_summary: the labels, the cells and the per-record table; the labels' page-locked staging
    Grown<> group_work;
    Grown<char, true> group_host;
    // HIP events around the pair kernel ([0]) and the pack kernel ([1]) of the most recent launches, recorded on the launch
    // stream: a ring, so that a caller timing many steps reads them ONCE at the end (dst_kernel_ms_mean) instead of
    // waiting for the device after every step
    static constexpr int kTimerRing = 64;
    struct Timer {
        hipEvent_t begin[kTimerRing] = {}, end[kTimerRing] = {};
        uint64_t seq = 0, mark = 0;   // launches timed so far; where the running mean starts
    } timer[2];
    float pair_ms = 0, pack_ms = 0;
    bool timed_pair = false, timed_pack = false;
    std::string err;
};

struct dst_comm;

namespace dst {

// Lists are only worth counting while the sampled records deviate from the reference at less than this share of the
// sites (unstructured data crosses over to the dense path near 3-4 %; profiles/r02/consensus_calibration.txt)
constexpr double kListsMaxDeviation = 0.08;

int fail(dst_ctx *ctx, int status, const std::string &msg);
// bracket the next pair (which = 0) / pack (1) kernel on `stream` with the timer ring's events
int timer_begin(dst_ctx *ctx, int which, hipStream_t stream);
int timer_end(dst_ctx *ctx, int which, hipStream_t stream);
int fail_hip(dst_ctx *ctx, hipError_t e, const char *what);

#define HIP_TRY(ctx, call)                       \
    do {                                         \
        hipError_t e_ = (call);                  \
        if (e_ != hipSuccess)                    \
            return dst::fail_hip((ctx), e_, #call); \
    } while (0)

// The two sets of a call that takes (square, row_slot, col_slot): square means slot 0 against itself; else two different
// slots in range.  Both must be loaded; same_len: and of one width; count_32: and of fewer than 2^32-1 records each.
struct TwoSets {
    int row_slot = 0, col_slot = 0;
    DeviceSet *rows = nullptr, *cols = nullptr;
};
int two_sets(dst_ctx *ctx, bool square, int row_slot, int col_slot, TwoSets &out, bool same_len = true, bool count_32 = false);
// the base planes a deferred upload left out, written before anything but the consensus path reads planes (dst_api.cpp)
int ensure_planes(dst_ctx *ctx, DeviceSet &s, hipStream_t stream);
// ... and the four derived planes of a set that was packed lean: what the dense kernels' measures read (dst_api.cpp)
int ensure_derived(dst_ctx *ctx, DeviceSet &s, hipStream_t stream);
// data another run's stream derived (lists, constants, counts, planes): `stream` waits for it on the device (dst_api.cpp)
int order_after_prep(dst_ctx *ctx, hipStream_t stream);
// behind a launch on `stream` that reads a set: what a later rebuild of the set's derived data on another stream waits for
int note_run(dst_ctx *ctx, hipStream_t stream);
// every window a column range [begin, end) of an alignment of len sites, else DST_ERR_ARG naming the first (dst_windows.hip)
int windows_valid(dst_ctx *ctx, const uint64_t *wb, const uint64_t *we, uint32_t n_windows, uint64_t len);
void free_set(DeviceSet &s);
// forget the mark of a stream that is idle and about to be destroyed (dst_ctx::Mark; dst_api.cpp)
void forget_stream(dst_ctx *ctx, hipStream_t stream);
// queue the pack of an n x len byte matrix (device memory) into `s`; *d_first_bad receives the index of the first
// byte that is not a Paradis code (or stays ~0).  Nothing here waits for the device.
// nibbles: d_codes holds the 4-bit wire format (two sites per byte) instead of Paradis bytes
int pack_queue(dst_ctx *ctx, DeviceSet &s, const uint8_t *d_codes, size_t n, size_t len, size_t row_stride,
               const uint32_t *d_counts, unsigned long long *d_first_bad, hipStream_t stream, bool want_lists, bool nibbles = false);
int invalid_code_error(dst_ctx *ctx, unsigned long long first_bad, size_t len);
// the upload of device bytes into any set of the context (a slot, or dst_nj_bootstrap's replicate): the pack, the
// report and its one synchronisation
int pack_set(dst_ctx *ctx, DeviceSet &s, const uint8_t *d_codes, size_t n, size_t len, size_t row_stride,
             const uint32_t *d_counts, hipStream_t stream);
// the per-record {A,T,G,C} counts of `s` on the device (counted by code unless the upload brought them)
int need_counts(dst_ctx *ctx, DeviceSet &s, hipStream_t stream);
// rows [rb, re) of `rows` against every (square: later) record of `cols` — any two packed sets of this context
int run_sets(dst_ctx *ctx, int measure, bool square, DeviceSet &rows, DeviceSet &cols, uint64_t rb, uint64_t re,
             int out_kind, void *d_out, size_t cap, void *stream_v);
// the row slabs of a call, cut at max_pairs (0: default_pairs) pairs, and the pair count of the largest one
// (dst_analysis.cpp; dst_run_slabs plans with it too)
struct SlabPlan {
    std::vector<RowSlab> slabs;
    uint64_t biggest = 0;
};
SlabPlan plan_slabs(bool square, uint64_t n_rows, uint64_t n_cols, uint64_t max_pairs, uint64_t default_pairs);
// the threshold of dst_clusters / dst_links / dst_stream_open_links as a payload of `measure`; false: nothing can link
// (dst_analysis.cpp)
bool threshold_payload(int measure, double threshold, uint64_t &t_bits);
// dst_summary's one conversion of an exact integer sum to double (dst_analysis.cpp; dst_window_summary shares it)
double summary_value(__int128 s, bool int_payload);
// dst_summary's checks of a bin width (its messages), and width_q: the width as a fixed-point value (dst_analysis.cpp)
int summary_width_q(dst_ctx *ctx, int measure, double width, uint64_t &width_q);

}  // namespace dst
