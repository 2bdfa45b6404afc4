// dst_internal.h — shared between the HIP kernels (dst_kernels.hip), the C-ABI (dst_api.cpp, dst_analysis.cpp)
// and the host-only logic (dst_host.cpp).  Not installed; the public surface is
// include/distance_hip.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/distance_hip.h"
#include "dst_owner.h"

namespace dst {

// ---- device-resident form of one loaded set -------------------------------------------------
// The Paradis byte matrix (src/encoding.rs) is re-laid on upload into 8 bit-planes, one bit per
// site, 128 sites (one uint4) per (plane, chunk, record):
//     planes[(plane * nchunks + chunk) * npad + record]          (uint4 = sites 128c .. 128c+127)
// so that (a) a wave whose lanes own consecutive records reads 1 KiB contiguous per plane-chunk
// and (b) the 16 bytes of one record are a wave-uniform scalar load.  Only the high nibble and
// bit 3 of a code matter to any measure, so the planes carry all of it:
enum Plane : int {
    PL_A = 0,   // code bit 7: A is a member of the site's base set
    PL_G = 1,   // code bit 6
    PL_C = 2,   // code bit 5
    PL_T = 3,   // code bit 4
    PL_K = 4,   // code bit 3: "known base" (exactly one of A,G,C,T)
    PL_X1 = 5,  // class bit: 1 for {C,T,Y} (pyrimidine class), 0 for {A,G,R}; 0 elsewhere
    PL_X0 = 6,  // within-class bit of a known base: 1 for G and T, 0 for A and C; 0 elsewhere
    PL_CL = 7,  // code is in a k80 class: {A,G,R} or {C,T,Y}
    PL_COUNT = 8
};

constexpr uint32_t kChunkSites = 128;  // sites per uint4
constexpr uint32_t kPadRecords = 512;  // npad granularity (>= every tile's BN)
constexpr uint32_t kBlockThreads = 256;
// The widest alignment of the narrow tally form: every tally of a pair is at most len, so up to here two of them share a
// 32-bit word in the consensus pair kernel (Pack, pack_words), the hot columns' tallies travel as uint16, DST_OUT_TALLY16
// exists and the text kernels read 16-bit tallies.  One site more and everything is one tally per 32-bit word ("wide").
constexpr uint64_t kNarrowMaxLen = 65535;

// ---- consensus-delta path (dst_consensus.hip) -------------------------------------------------
// Every tally of every measure is a sum over sites of a per-site function f_k(q[s], t[s]) of the two
// codes' high nibbles (src/measures.rs:14-23, 56-66, 85-107, 156-175).  Against a reference sequence c
// (a per-site plurality code: the idea of consensus(), src/fastaio.rs:289-336, and of snp_consensus(),
// src/measures.rs:28-53, carried to every measure):
//     T_k(q,t) = F_k + A_k(q) + A_k(t) + sum over sites where BOTH q and t differ from c of h_k
//     F_k    = sum_s f_k(c,c)              A_k(x) = sum over x's difference sites of f_k(x,c) - f_k(c,c)
//     h_k    = f_k(q,t) - f_k(q,c) - f_k(c,t) + f_k(c,c)
// exact integers whatever c is; the work is proportional to the differences from c, not to L.
constexpr uint32_t kPanelCols = 2048;      // column records per site bucket = width of the LDS accumulators
constexpr uint32_t kBucketSites = 1024;    // sites per block of site_bucket_kernel: the lists' range_start marks are this far apart
constexpr int kAccRows = 2;                // rows whose accumulators a workgroup holds at once
constexpr uint32_t kTileRowsMax = 32;      // rows of one consensus-path tile (a multiple of kAccRows)
constexpr uint32_t kEntryShift = 28;       // list entries: nibble in the top four bits
constexpr uint32_t kEntryMask = (1u << kEntryShift) - 1;   // bucket entries: column record | nibble << 28
constexpr uint32_t kSiteBits = 25;         // record-list entries: site | reference class << 25 | nibble << 28
constexpr uint32_t kSiteMask = (1u << kSiteBits) - 1;
constexpr uint32_t kInlineEvents = 15;     // bucket entries held inside the 32-byte lookup-table entry
constexpr uint32_t kInlineOverflowing = 13;  // ... of a larger bucket: its last word is where the rest are
constexpr uint32_t kSlotEntries = 7;        // differences a (record, chunk) slot of the pack holds
constexpr uint32_t kRefSamples = 512;      // records sampled for the reference sequence
constexpr int kRefClasses = 5;             // reference nibbles: A(8) G(4) C(2) T(1) N-class(15)
constexpr int kMaxWords = 4;               // packed accumulator words per pair
constexpr uint32_t kHotPermille = 50;      // hybrid path: a site is "hot" when more than 5 % of the sampled records deviate
                                           // (p^2 x 1.85 ps per event against 1 / 1.95e14 s per dense site and pair; 33 while an event cost 4.5 ps)

// Every buffer of a set is a Grown (dst_owner.h): grown where it is needed, released with the set (free_set), read by the
// launchers through its pointer conversion.  A capacity, where one matters, is the owner's `bytes`.
struct ConsensusRef {             // the reference sequence, sampled from the set that owns it (buffers: alloc_ref, grow-only)
    Grown<uint4> planes;          // [4][nchunks] A,G,C,T planes of it (chunk-packed like the records'); N past len
    Grown<uint4> hot_planes;      // [nchunks] bit = 1: a hot site (kHotPermille), handed to the dense kernels by the hybrid path
    Grown<uint32_t> hot_sites;    // [n_hot] the hot sites, ascending
    Grown<uint32_t> partials;     // [nchunks][2][8] every chunk's two shares of `stats` (summed by hot_list_kernel)
    // device: {known sites, sum of deviants, sum of deviants^2, sample size, hot sites, known hot sites,
    //          sum of deviants over the cold sites, sum of deviants^2 over the cold sites}
    Grown<uint64_t> stats;
    uint64_t h_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool valid = false;
};

struct RecordIndex {              // per record: the sites where it differs from the reference, ascending
    Grown<uint32_t> off;          // [n + 1]
    Grown<uint32_t> ent;          // site | class of the reference there << 25 | the record's nibble << 28
    // list lengths counted by the pack itself against the set's own reference (cold sites / hot sites apart), with
    // their sums {cold, hot} — valid while pre_epoch == the set's epoch
    Grown<uint4> pre_slots;       // [nchunks][npad] the entries themselves, by (record, chunk) (PackLists::slots)
    // the pack's counters, one block cleared per upload (pack_counters, dst_api.cpp, lays it out and sets the views):
    // pre_cold owns it and is its first array, pre_hot, pre_totals and RunIndex's cnt_run / run_cold / run_hot point into it
    Grown<uint32_t> pre_cold;
    uint32_t *pre_hot = nullptr;
    unsigned long long *pre_totals = nullptr;
    uint64_t pre_epoch = 0, pre_total_cold = 0, pre_total_hot = 0;
    bool pre_valid = false;
    // column sets: [ceil(nchunks / 8)][npad] where the record's list crosses every multiple of kBucketSites sites
    Grown<uint32_t> range_start;
    uint64_t total = 0;
    const void *ref_owner = nullptr;  // the DeviceSet whose reference these lists are relative to
    uint64_t ref_epoch = 0;
    bool without_hot = false;         // hybrid path: the hot sites are left out
    bool valid = false;
    bool ranges_valid = false;        // range_start holds the marks of THESE lists (a column set's site buckets can be built from them)
};

// ---- records with long runs of N (failed amplicons, partial genomes) ----------------------------------------------
// Every site of a run is a difference from the reference sequence, and two such records share an event at every site
// where their runs overlap: 5 % of 50,000 records half N cost the consensus path 59 ms instead of 2.  N contributes
// NOTHING to any tally, whatever the other record holds, so a whole 128-site chunk of N in record t ("run chunk": the
// reference has at least one known site there) can leave t's list, if every pair (q, t) is corrected for what the
// identity then counts wrongly on those sites:
//     T(q,t) = F + A'(q) + A'(t) + H(q,t) + X(q,t)          M_x = the run chunks of x (records with fewer than kRunMin keep
//     A'(x)  = A(x: stripped list) - F(M_x)                        their entries: M_x is empty)
//     X(q,t) = F(M_q n M_t) - A_q(M_t) - A_t(M_q)             A_q(M) = sum of a(e) over q's entries in the chunks of M
// exact integers again (dst_consensus.hip: corr_kernel computes X's terms per (run record, record) once per set, the
// pair kernel's event waves add them to the accumulators).  Records with runs: "run records" (hot records in DESIGN.md).
constexpr uint32_t kRunMin = 4;            // run chunks (512 sites of N) that make a record a run record
struct RunIndex {
    uint32_t *cnt_run = nullptr;     // [n] run chunks of every record          } counted by the pack: views into the
    uint32_t *run_cold = nullptr;    // [n] their entries at cold sites         } block RecordIndex::pre_cold owns
    uint32_t *run_hot = nullptr;     // [n] ... at hot sites
    Grown<uint32_t> index;           // [n] run record number of a record, or 0xFFFFFFFF; owns the block `ids` is the other half of
    uint32_t *ids = nullptr;         // [n] the run records, ascending (set by pack_queue, with `index`)
    Grown<uint32_t> mask;            // [n_run][mask_words] bit c: chunk c of the run record is a run chunk (from the slots' flags),
                                     // then the same transposed, [mask_words][n_run]
    Grown<uint32_t> known;           // [nchunks] known reference sites of every chunk (cold sites only: without_hot lists)
    Grown<uint32_t> panel_first;     // [n_panels + 1] first run record of every column panel
    Grown<uint32_t> state;           // device: [0] run records, [1] 1: stripping is on for this upload (grown with `index`)
    Grown<uint32_t> aent;            // [kMaxWords][entries] a-words of every list entry (aconst_kernel), what the tables sum;
                                     // entries = aent.bytes / (kMaxWords words): the launchers' stride
    Grown<uint8_t> s7;               // [words][5][tiles of 32 records][mask_words][1 KB] every record's per-chunk sums of them, in 7-bit pieces
    Grown<uint32_t> corr;            // [words][n_run][n]   X's terms by (run record, record) ...
    Grown<uint32_t> corr_t;          // [words][n][n_run]   ... and transposed
    size_t mask_words = 0;
    uint64_t removed = 0;            // entries the run records' lists lost (host copy: rescales the sample's statistics)
    uint32_t n_run = 0;              // host copy (0: no run records, or stripping off)
    bool active = false;             // this upload's lists are stripped of the run records' run chunks
    int corr_family = -1;            // what corr / corr_t hold (like aconst)
    bool corr_wide = false, corr_without_hot = false;
    uint64_t corr_epoch = 0;
};

// chunk_sums_kernel keeps one row of per-chunk sums per wave and accumulator word in LDS and walks the chunks in slices of
// kSumSliceChunks, so what a workgroup needs does not grow with the alignment: 4 waves x 4 words x 1,024 chunks x 4 bytes
// = 64 KiB at most, what a kernel gets without asking for more.  (One row over all chunks, the first form, passed
// 64 KiB at 131,073 sites of tn93 and the CU's whole 160 KiB at 327,681.)
constexpr uint32_t kSumSliceChunks = 1024;   // a multiple of 32: a slice is whole mask words and whole k-steps of s7
struct SumSlices {
    uint32_t kpad;        // chunks padded to whole mask words: 32 x mask_words
    uint32_t row;         // chunks of one LDS row: min(kpad, kSumSliceChunks)
    uint32_t n_slices;    // slice k covers chunks [k * row, min((k + 1) * row, kpad))
    size_t lds_bytes;     // dynamic LDS of a workgroup: [4 waves][words][row] uint32_t
};
inline SumSlices sum_slices(size_t nchunks, int words)
{
    SumSlices s;
    s.kpad = 32u * (uint32_t)((nchunks + 31) / 32);
    s.row = std::min(s.kpad, kSumSliceChunks);
    s.n_slices = s.row ? (s.kpad + s.row - 1) / s.row : 0u;
    s.lds_bytes = (size_t)4 * (size_t)words * s.row * sizeof(uint32_t);
    return s;
}

struct SiteIndex {                // the same entries of a column set by (site, panel of kPanelCols records)
    // [n_sites * n_panels] 32 bytes per bucket = 16 halfwords: [0] entries in the bucket, then up to kInlineEvents
    // entries as record-in-panel | nibble << 11.  The pair kernel reads THIS: one request per (row entry, panel)
    // brings the whole bucket of a typical site.  A larger bucket keeps kInlineOverflowing entries inline and its
    // last word is the place of the others in `ent`.
    Grown<uint4> inl;
    Grown<uint32_t> ent;          // overflow entries by bucket: record | nibble << 28 (any order inside a bucket)
    uint32_t n_panels = 0;
    bool valid = false;
};

struct DeviceSet {
    Grown<uint4> planes;          // PL_COUNT * nchunks * npad   } kept while big enough for the next upload, else the whole
    Grown<uint32_t> counts;       // npad x 4 {A,T,G,C}          } set is freed first (shape_set)
    size_t n = 0, len = 0, nchunks = 0, npad = 0;
    bool loaded = false;
    bool have_counts = false;
    // dst_upload_shared: only the planes of records [part_begin, part_end) are this rank's own work and valid; the lists
    // of ALL records came by the exchange.  Such a set runs on the consensus path only.
    bool partial = false;
    size_t part_begin = 0, part_end = 0;
    bool lean = false;            // only the four base planes are stored (a low-diversity set headed for the consensus path):
                                  // the dense pair kernels' other planes are derived on demand (ensure_derived)
    // the pack stored the base planes only of chunks that do not fit their slot (PackLists::defer_planes): the rest is the
    // reference plus rec.pre_slots, written by ensure_planes the first time anything but the consensus path reads planes
    bool planes_deferred = false;
    uint64_t epoch = 0;           // bumped by every upload: stale consensus indexes are rebuilt
    // consensus path
    ConsensusRef ref;
    RecordIndex rec;
    SiteIndex site;
    RunIndex runs;
    Grown<uint32_t> aconst;       // [kMaxWords][npad] packed A_k words of one measure family (see the key below)
    int aconst_family = -1;       // what `aconst` currently holds: family, packing, and the lists it was summed from
    bool aconst_wide = false;
    uint64_t aconst_epoch = 0, aconst_ref_epoch = 0;
    const void *aconst_ref_owner = nullptr;
    bool aconst_without_hot = false;
    // hybrid path: the hot columns of this set (by some set's reference) as a packed set of their own
    std::unique_ptr<DeviceSet> hot;
    const void *hot_ref_owner = nullptr;
    uint64_t hot_epoch = 0, hot_ref_epoch = 0;
};

struct BlockDesc {
    uint32_t i0, j0;  // first row / first column of the tile; i0 == 0xFFFFFFFF: idle filler
};

// geometry of one tile variant
struct TileShape {
    int bm;  // rows (scalar side) per block
    int bn;  // columns (vector side) per block = 256 * tn
};

struct PairLaunch {
    const DeviceSet *rows;
    const DeviceSet *cols;
    bool square;
    uint64_t row_begin, row_end;  // rows of `rows` this launch covers
    uint64_t out_base;            // canonical index of the first pair of this launch
    int out_kind;                 // DST_OUT_DISTANCE (f64 / int64 by measure), DST_OUT_TALLY or _TALLY16
    void *d_out;                  // first pair of this launch
    const BlockDesc *d_blocks;
    uint32_t nblocks;
    uint32_t ksplit = 1;          // > 1: split-L launch, partial tallies added atomically
};

struct ConsensusTile {
    uint32_t i0, i1, panel;  // rows [i0, i1) against column panel `panel`
};

// per-measure-family tables of the consensus path, built on the host (dst_host.cpp) from the per-site
// semantics of src/measures.rs and uploaded once per context
struct ConsensusLut {
    // [family][wide][ref class][row nibble][col nibble][word]   h_k packed like the accumulators
    // [family][wide][ref class][nibble][word]                    A-term of one difference site
    // [family][wide][word]                                       f_k(known, same known) = F per known ref site
    uint32_t h[4][2][kRefClasses][16][16][kMaxWords];
    uint32_t a[4][2][kRefClasses][16][kMaxWords];
    uint32_t unit[4][2][kMaxWords];
};
enum Family : int { FAM_NHIGH = 0, FAM_RAW = 1, FAM_K80 = 2, FAM_TN93 = 3 };
int family_of(int measure);
int family_words(int family, bool wide);       // accumulator words per pair
void build_consensus_lut(ConsensusLut &lut);   // dst_host.cpp
void pack_tallies(int family, bool wide, const int64_t tallies[4], uint32_t words[kMaxWords]);
// the per-site tallies of one code pair (bytes as src/encoding.rs produces them): the site loop bodies of
// src/measures.rs:14-23, 56-66, 85-107, 156-175.  out has tally_width(measure) entries.
void site_tallies(int measure, uint8_t q, uint8_t t, int out[4]);
std::vector<ConsensusTile> build_consensus_tiles(bool square, uint64_t row_begin, uint64_t row_end,
                                                 uint64_t n_cols, uint32_t rows_per_tile);

struct ConsensusLaunch {
    const DeviceSet *rows;
    const DeviceSet *cols;
    bool square;
    uint64_t row_begin, row_end, out_base;
    int out_kind;
    void *d_out;
    const ConsensusTile *d_tiles;
    uint32_t ntiles;
    bool wide;                   // one 32-bit word per tally (alignments of 65,536 sites or more)
    const ConsensusLut *d_lut;
    const void *d_hot = nullptr; // hybrid path: the dense kernels' tallies of the hot columns (TALLY16 / TALLY layout)
    int heavy_events = 0;        // 1: many events per pair or long lists — more of the workgroup's waves take the event role;
                                 // 2: more than one event per pair — every wave in both roles (consensus_pair_kernel)
};

// ---- shared preparation (dst_shared.cpp): one rank's exchange block, in 32-bit words ------------------
//   [0] entries of the block's lists   [1] 1: they did not fit ent_cap   [2, 3] first invalid byte (~0: none)   [4..15] 0
//   [cnt_at .. + rmax)        list lengths of the rank's records (record k * rmax + i of the set)
//   [counts_at .. + 4 rmax)   their {A,T,G,C} counts
//   [ent_at .. + ent_cap)     the entries, record after record
struct SharedLayout {
    uint32_t world, rmax, cnt_at, counts_at, ent_at, ent_cap, words;
};
SharedLayout shared_layout(uint64_t n, int world, uint32_t ent_cap);   // dst_host.cpp (pure host)

// ---- consensus-path launchers (dst_consensus.hip) --------------------------------------------
hipError_t launch_shared_block(uint32_t *block, const SharedLayout &lay, const DeviceSet &set, size_t rec_begin, size_t count,
                               const uint32_t *off_local, const unsigned long long *first_bad, hipStream_t stream);
// the gathered blocks -> set.rec.off / ent / range_start (and set.counts), then the report for the host (kReportWords + 1 words)
hipError_t launch_shared_splice(const uint32_t *gathered, const SharedLayout &lay, DeviceSet &set, uint32_t *len_all,
                                uint32_t *scan_tmp, bool with_counts, unsigned long long *report, hipStream_t stream);
hipError_t launch_ref_sample(const DeviceSet &set, hipStream_t stream);
// the same from the row-major code matrix (before the pack)
// ... on its way the kernel clears zero[0..zero_words) and sets *first_bad = ~0: what the pack behind it accumulates into
hipError_t launch_ref_sample_bytes(const uint8_t *d_codes, size_t row_stride, const DeviceSet &set, hipStream_t stream,
                                   uint32_t *zero = nullptr, size_t zero_words = 0, unsigned long long *first_bad = nullptr);
// count pass (fill == false): rec_cnt[n], site_cnt[len * n_panels] (when want_sites), *total
// fill pass: entries behind the scanned offsets.  ref_planes: [4][nchunks] uint4.
hipError_t launch_hot_list(const DeviceSet &set, hipStream_t stream);
hipError_t launch_compact(const DeviceSet &src, const uint32_t *hot_sites, uint32_t n_hot, DeviceSet &dst, hipStream_t stream);
// hot_planes != NULL: sites whose bit is set are left out of the lists
hipError_t launch_index(const DeviceSet &set, const uint4 *ref_planes, const uint4 *hot_planes, bool fill, bool skip_nclass,
                        uint32_t *rec_off_or_cnt, uint32_t *rec_ent, unsigned long long *total,
                        hipStream_t stream, uint32_t *range_start = nullptr);
// the same lists from the pack's slots (set.rec.pre_slots) instead of the planes; without_hot: leave the hot entries out
// rec_begin / rec_end / ent_cap: only those records (rec_off[0] = record rec_begin's offset), entries at or beyond ent_cap
// dropped — one rank's share of a set, written into an exchange block of fixed size (dst_upload_shared)
hipError_t launch_slot_fill(const DeviceSet &set, const uint4 *ref_planes, const uint4 *hot_planes, bool without_hot,
                            uint32_t *rec_off, uint32_t *rec_ent, uint32_t *range_start, hipStream_t stream, size_t rec_begin = 0,
                            size_t rec_end = ~(size_t)0, uint32_t ent_cap = 0xFFFFFFFFu);
// a column set's site buckets from its lists (set.rec -> set.site); *ovf_total (zeroed by the caller) counts the
// overflow entries placed in set.site.ent
hipError_t launch_site_buckets(const DeviceSet &set, uint32_t n_panels, uint32_t *ovf_total, hipStream_t stream);
// in-place exclusive scan of data[0..n) (data[n] receives the total); tmp: scan_tmp_words(n) words
size_t scan_tmp_words(size_t n);
// exclusive scan of data[0..n) in place; src0 (+ src1) given: of src0[i] (+ src1[i]) into data
// zero[0..n_zero) (n_zero <= 1024) is cleared before the scan's results are visible: counters the next kernels add to
hipError_t launch_exclusive_scan(uint32_t *data, size_t n, uint32_t *tmp, hipStream_t stream, const uint32_t *src0 = nullptr,
                                 const uint32_t *src1 = nullptr, uint32_t *zero = nullptr, uint32_t n_zero = 0);
hipError_t launch_aconst(const DeviceSet &set, int family, bool wide, const ConsensusLut *d_lut, hipStream_t stream);
// run records (RunIndex): the known reference sites per chunk (hot_planes != NULL: cold sites only), and the correction
// tables of one (family, packing) — after launch_aconst for the same, which leaves the entries' a-words in runs.aent
hipError_t launch_run_known(const DeviceSet &set, const uint4 *ref_planes, const uint4 *hot_planes, hipStream_t stream);
hipError_t launch_run_masks(const DeviceSet &set, hipStream_t stream);   // runs.mask from the slots' run-chunk flags
// (*failed: the kernel whose launch was refused, for the error's message)
hipError_t launch_run_tables(const DeviceSet &set, int family, bool wide, const ConsensusLut *d_lut, hipStream_t stream,
                             const char **failed);
constexpr int kReportWords = 13;   // [0] first invalid byte, [1..8] the sample's statistics, [9..10] list totals, [11] run records, [12] entries their lists lost
// cnt_cold / cnt_hot (may be NULL): the pack's list lengths, summed into words 9 and 10.  runs: the pack's run-chunk
// counters — records with kRunMin run chunks and more become run records (numbered in runs->index / ids, word 11 = how
// many; 0 when there are more than max_run: stripping off), every other record gets its run chunks' entries back into
// its list length
// totals: four zeroed 64-bit words (the set's pre_totals block: the sample kernel clears it with the counters)
hipError_t launch_report(const unsigned long long *first_bad, const unsigned long long *stats, uint32_t *cnt_cold,
                         uint32_t *cnt_hot, size_t n, unsigned long long *report, hipStream_t stream, const RunIndex *runs = nullptr,
                         uint32_t max_run = 0, unsigned long long *totals = nullptr);
hipError_t launch_sum2_u32(const uint32_t *a0, const uint32_t *a1, size_t n, unsigned long long *totals, hipStream_t stream);
// f_words: F_k (known reference sites x the per-site unit), packed like the accumulators
hipError_t launch_consensus_pairs(int measure, const ConsensusLaunch &cl, const uint32_t f_words[kMaxWords],
                                  hipStream_t stream);
// EW of the consensus_pair_kernel<FAM, WIDE, OUT, EW> that launch_consensus_pairs picks for (measure, out_kind, wide,
// heavy_events), by the launcher's own dispatch; 0 for a combination it refuses.  Pure host code.
int consensus_event_waves(int measure, int out_kind, bool wide, int heavy_events);
// exact per-site counts of known G, C, T over the records of `set`, added into hist[len][3]
hipError_t launch_site_hist(const DeviceSet &set, uint32_t *hist, hipStream_t stream);

const char *consensus_build_flags();   // dst_consensus.hip: the DST_DBG_* measurement macros it was compiled with

// ---- kernel launchers (dst_kernels.hip) -----------------------------------------------------
// lists != NULL: the pack also counts every record's differences from the reference (cold and hot sites apart)
struct PackLists {
    const uint4 *ref_planes, *hot_planes;      // [4][nchunks], [nchunks]
    const unsigned long long *stats;           // the sample's statistics (device): [1] = sum of deviants
    unsigned long long max_dev_sum;            // count only while stats[1] <= this (high-diversity sets go dense anyway)
    uint32_t *cnt_cold, *cnt_hot;              // [n], zeroed
    uint4 *slots;                              // [nchunks][npad] the differences of every (record, chunk), see pack_kernel
    // run chunks (RunIndex; all NULL: not looked for): counted apart and flagged in the slot
    uint32_t *cnt_run, *run_cold, *run_hot;
    // the base planes of a chunk that is inline in its slot are not stored (DeviceSet::planes_deferred)
    int defer_planes;
};
// a slot that holds every difference of its (record, chunk): not a chunk of N (flag 0x100), at most kSlotEntries of them
__host__ __device__ inline bool slot_is_inline(uint32_t word0) { return !(word0 & 0x100u) && (word0 & 0xFFu) <= kSlotEntries; }
// rec_begin / rec_end: only those records are packed (one rank's share of a set: dst_upload_shared)
hipError_t launch_pack(const uint8_t *d_codes, size_t row_stride, const DeviceSet &set,
                       unsigned long long *d_first_bad, const PackLists *lists, hipStream_t stream, size_t rec_begin = 0,
                       size_t rec_end = ~(size_t)0);
// the 4-bit wire format: rows of ceil(len / 2) bytes (row_stride a multiple of 64, base 16-byte aligned), two sites per
// byte, even site in the low nibble, a site = the high nibble of its Paradis code
hipError_t launch_pack_nibbles(const uint8_t *d_nibbles, size_t row_stride, const DeviceSet &set, unsigned long long *d_first_bad,
                               hipStream_t stream);
// lists: the pack's, when the set was packed with them (then a chunk that is inline in its slot is counted from the slot:
// its planes may not be there)
hipError_t launch_fill_counts(const DeviceSet &set, hipStream_t stream, const PackLists *lists = nullptr);
// the counts of records [rec_begin, rec_end) only, out[0..4) = record rec_begin's
hipError_t launch_range_counts(const DeviceSet &set, size_t rec_begin, size_t rec_end, uint32_t *out, hipStream_t stream,
                               const PackLists *lists = nullptr);
bool planes_deferred_by_pack();   // (false under DST_PACK_ALL_PLANES, the measurement knob)
// the base planes the pack deferred, from the slots and the reference (DeviceSet::planes_deferred)
hipError_t launch_planes_from_slots(const DeviceSet &set, hipStream_t stream);
hipError_t launch_derive(const DeviceSet &set, hipStream_t stream);   // planes K, X1, X0, CL of a lean set from its base planes
hipError_t launch_pairs(int measure, int variant, const PairLaunch &pl, hipStream_t stream);
// close: the reference's operation order with the table logarithm (what the text path uses), not the epilogue's arithmetic
hipError_t launch_finalize(int measure, const PairLaunch &pl, const void *d_tallies, bool tallies16,
                           void *d_out, hipStream_t stream, bool close = false);
TileShape tile_shape(int measure, int variant);
int variant_count(int measure);

// ---- the analyses (dst_analysis.cpp drives the launchers below, slab by slab) ------------------------------------------
// A grid's y dimension holds at most 65,535 rows: the rows [rb, re) of a launch that gives every row a grid row, in such
// grids.  launch(row0, rows) queues one of them and returns its status; the first failure ends the walk.
constexpr uint64_t kGridRowsMax = 65535;
inline unsigned grid_rows(uint64_t rows) { return (unsigned)std::min<uint64_t>(rows, kGridRowsMax); }
template <typename Launch>
inline hipError_t for_row_grids(uint64_t rb, uint64_t re, Launch &&launch)
{
    for (uint64_t row0 = rb; row0 < re; row0 += kGridRowsMax) {
        const hipError_t e = launch(row0, grid_rows(re - row0));
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// ---- k nearest records (dst_nearest.hip, driven by dst_nearest in dst_analysis.cpp) ---------------------------------
// A call cuts the rows into slabs of at most kNearestSlabPairs pairs (cut_row_slabs, like dst_run_slabs), runs each slab
// into a DST_OUT_TALLY scratch (square: the triangle, every pair once) and merges it into device-resident lists of
// k entries per record, sorted by (key of the DST_OUT_DISTANCE payload, column record).
constexpr uint64_t kNearestSlabPairs = (uint64_t)1 << 25;   // 33.5 M pairs: 0.5 GB of tn93 tallies
constexpr uint32_t kNearestMaxK = 256;
struct NearestLists {
    uint64_t *val;   // [records][k] DST_OUT_DISTANCE payloads (int64 / f64 bits)
    uint32_t *idx;   // [records][k] column records (2^32-1: an empty entry)
    uint32_t *tal;   // [records][k][tally_width] DST_OUT_TALLY words of the pair
    uint32_t k;
};
hipError_t launch_nearest_init(const NearestLists &nl, uint64_t records, hipStream_t stream);
// row pass: rows [rb, re) of the slab offer their pairs to their own lists (q_counts / t_counts: tn93's base counts of the
// row and the column set)
hipError_t launch_nearest_rows(int measure, bool square, const uint32_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                               uint64_t re, const uint32_t *q_counts, const uint32_t *t_counts, const NearestLists &nl,
                               hipStream_t stream);
// column pass (square): pairs (i, j), i in [rb, re), j > i, offer i to record j's list
hipError_t launch_nearest_cols(int measure, const uint32_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                               const uint32_t *counts, const NearestLists &nl, hipStream_t stream);
// column pass over a rectangle (closest streams): the slab is one batch's tallies [n_batch][n_loaded]; row r offers the
// streamed ordinal first_ordinal + r (<= 2^32-2) to every loaded record's list.  q_counts: the batch's, t_counts: the
// loaded set's (tn93).  Launches that share lists must follow one another on one stream.
hipError_t launch_nearest_stream_cols(int measure, const uint32_t *slab, uint64_t n_batch, uint64_t n_loaded, uint32_t first_ordinal,
                                      const uint32_t *q_counts, const uint32_t *t_counts, const NearestLists &nl, hipStream_t stream);

// ---- single-linkage clusters (dst_clusters.hip, driven by dst_clusters in dst_analysis.cpp) -------------------------
// A call cuts the rows of slot 0 into slabs of at most kClusterSlabPairs pairs (cut_row_slabs), runs each slab's triangle
// into a DST_OUT_DISTANCE scratch and unites the endpoints of its links in a device-resident parent array (lock-free
// union-find, parent[x] <= x).  2^25 pairs (256 MB of payloads): the link launch of a full slab has 2^25 / 2048 = 16384
// workgroups of four waves, 64 per CU, so every CU stays busy to the end of the slab; and a slab is one pair-kernel
// launch, whose fixed cost is paid once per slab (2^24 measured slower at 50,000 records: DESIGN.md 3h).
constexpr uint64_t kClusterSlabPairs = (uint64_t)1 << 25;
hipError_t launch_clusters_init(uint32_t *parent, uint64_t n, unsigned long long *links, hipStream_t stream);
// rows [rb, re) of the square, their payloads from slab entry tri_row_start(n, i) - out_base; t_bits: the threshold as a
// payload (int64 for n / n_high, else f64 bits)
hipError_t launch_clusters_link(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                                uint64_t t_bits, uint32_t *parent, unsigned long long *links, hipStream_t stream);
hipError_t launch_clusters_final(uint32_t *parent, uint64_t n, hipStream_t stream);

// ---- greedy representatives (dst_representatives.hip, driven by dst_representatives in dst_analysis.cpp) -----------------
// Slabs as for dst_clusters (DST_OUT_DISTANCE payloads, or DST_OUT_TALLY words when the tallies are wanted: `tally`).  A slab's
// rows are taken in sub-blocks of kRepBlockRows rows, in order: 512 x 512 link bits are 32 KiB of one workgroup's LDS.
constexpr uint32_t kRepBlockRows = 512;
struct RepBuffers {
    uint32_t *rep;    // [n] 2^32-1: unset
    uint32_t *bits;   // [n][kRepBlockRows / 32] the slab's rows' links inside their own sub-block
    uint64_t *val;    // [n] the DST_OUT_DISTANCE payload of (rep[j], j), or NULL
    uint32_t *tal;    // [n][tally_width] its DST_OUT_TALLY words, or NULL
};
// rows [rb, re) of the slab (every earlier row has been through this): the bits launch, then per sub-block the resolve
// launch, the cover launch, and the values launch when b.val or b.tal is set.  counts: tn93's base counts of the set
// (tally slabs)
hipError_t launch_rep_slab(int measure, bool tally, const void *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                           uint64_t t_bits, const uint32_t *counts, const RepBuffers &b, hipStream_t stream);
hipError_t launch_rep_final(uint32_t *rep, uint64_t n, hipStream_t stream);   // behind the last slab: unset -> itself

// ---- pairs within a threshold (dst_links.hip, driven by dst_links in dst_analysis.cpp) --------------------------------
// Per row slab (cut as for dst_clusters; DST_OUT_DISTANCE payloads, or DST_OUT_TALLY words when the links' tallies are
// wanted: `tally`) a count launch with dst_clusters' geometry, one count per workgroup, the workgroups numbered in canonical
// order; a one-workgroup scan of the counts into 64-bit offsets; and per window of at most DST_LINKS_CHUNK ranks a write
// launch that places every link of the window at its rank.  No sort: rank order is canonical pair order.
struct LinksBuffers {
    uint32_t *counts;     // [blocks] links per workgroup of the slab
    uint64_t *offsets;    // [blocks + 1] their exclusive scan; the last entry: the slab's links
    uint64_t *grand;      // the call's links so far (every scan adds its slab's)
    uint32_t *row, *col;  // one window of links: DST_LINKS_CHUNK entries at most
    uint64_t *val;        // their DST_OUT_DISTANCE payloads
    uint32_t *tal;        // their DST_OUT_TALLY words
};
// workgroups (= counts) of the launches over rows [rb, re): rows x the 2048-entry runs of the longest row, row rb
uint64_t links_blocks(bool square, uint64_t n_cols, uint64_t rb, uint64_t re);
// rows [rb, re) of the slab: square, pairs (i, j > i) of n_cols records from slab entry tri_row_start(n_cols, i) - out_base;
// else pairs (i, 0 .. n_cols-1) from (i - rb) n_cols.  t_bits: the threshold as a payload.  q_counts / t_counts: tn93's base
// counts of the row and the column set (tally slabs only).  The count launch and the scan behind it:
hipError_t launch_links_count(int measure, bool tally, bool square, const void *slab, uint64_t out_base, uint64_t n_cols,
                              uint64_t rb, uint64_t re, uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                              const LinksBuffers &b, hipStream_t stream);
// the links of ranks [lo, hi) of the slab into b.row / b.col (and b.val, b.tal when asked), entry rank - lo
hipError_t launch_links_write(int measure, bool tally, bool square, const void *slab, uint64_t out_base, uint64_t n_cols,
                              uint64_t rb, uint64_t re, uint64_t t_bits, const uint32_t *q_counts, const uint32_t *t_counts,
                              const LinksBuffers &b, uint64_t lo, uint64_t hi, bool values, bool tallies, hipStream_t stream);
// the scan alone (dst_site_ld.hip counts its own blocks): offsets[b] = counts[0] + .. + counts[b - 1] for b <= blocks, *grand
// += offsets[blocks]
hipError_t launch_links_scan(const uint32_t *counts, uint64_t blocks, uint64_t *offsets, uint64_t *grand, hipStream_t stream);
// a links stream's batch (dst_stream.cpp): hdr[0] = *total (NULL: 0), hdr[1] = *bad, side by side for the one copy back
hipError_t launch_links_stream_header(const uint64_t *total, const unsigned long long *bad, uint64_t *hdr, hipStream_t stream);

// ---- difference sites of a pair list (dst_pair_sites.hip, driven by dst_pair_sites in dst_api.cpp) ---------------------
// Per batch of at most DST_PAIR_SITES_BATCH pairs: a count launch (one wave per pair, the lanes along its chunks) and a
// one-workgroup scan into 64-bit offsets; then per window of at most DST_PAIR_SITES_WINDOW ranks a write launch that places
// every listed site of the window, and the two records' nibbles, at its rank.  Reads the sets' four base planes only.
struct PairSitesBuffers {
    uint32_t *row, *col;  // [pairs] the batch's record indices
    uint32_t *counts;     // [pairs] listed sites per pair
    uint64_t *offsets;    // [pairs + 1] their exclusive scan; the last entry: the batch's entries
    uint32_t *sites;      // one window of entries: DST_PAIR_SITES_WINDOW at most
    uint8_t *bases;       // row nibble << 4 | column nibble
};
// b.row / b.col hold `pairs` valid record indices of rows / cols (two packed sets of one width, planes stored)
hipError_t launch_pair_sites_count(int measure, const DeviceSet &rows, const DeviceSet &cols, uint32_t pairs, const PairSitesBuffers &b,
                                   hipStream_t stream);
// the entries of ranks [lo, hi) of the batch into b.sites / b.bases, entry rank - lo
hipError_t launch_pair_sites_write(int measure, const DeviceSet &rows, const DeviceSet &cols, uint32_t pairs, const PairSitesBuffers &b,
                                   uint64_t lo, uint64_t hi, hipStream_t stream);

// ---- distances of a pair list (dst_pairs.hip, driven by dst_run_pairs in dst_analysis.cpp) ----------------------------
// One batch of at most DST_RUN_PAIRS_BATCH list entries on the device.  Direct route: entry k is the pair (row[k], col[k])
// swept over the two records' planes.  Sweep route: entry k is entry pos[k] of a row slab that a pair kernel has just
// written; row / col are read for tn93's base counts only.
struct PairsLaunch {
    const DeviceSet *rows, *cols;
    const uint32_t *row, *col;   // [pairs] valid record indices of rows / cols
    const uint64_t *pos;         // [pairs] positions inside the slab (the sweep route)
    uint32_t pairs;
    uint64_t *values;            // [pairs] DST_OUT_DISTANCE payloads, or NULL
    uint32_t *tallies;           // [pairs][tally_width] DST_OUT_TALLY words, or NULL
    const uint32_t *q_counts, *t_counts;   // tn93 values: the {A,T,G,C} counts of the row and the column set
};
// the lanes that serve one pair of the direct kernel for an alignment of `nchunks` 128-site chunks: a power of two, 1..64
uint32_t pairs_lanes(uint64_t nchunks);
// two packed sets of one width with the planes the measure reads stored; *lanes (may be NULL) = the launch's lanes per pair
hipError_t launch_pairs_direct(int measure, const PairsLaunch &pl, hipStream_t stream, uint32_t *lanes);
// tally: the slab holds DST_OUT_TALLY words (values are finalised from them), else DST_OUT_DISTANCE payloads (values only)
hipError_t launch_pairs_gather(int measure, const PairsLaunch &pl, const void *slab, bool tally, hipStream_t stream);

// ---- per-record and histogram summaries (dst_summary.hip, driven by dst_summary in dst_analysis.cpp) -------------------
// Per row slab of DST_OUT_DISTANCE payloads (cut as for dst_clusters) up to three launches, each wanted or not: the row pass
// (dst_clusters' geometry, one set of atomics per workgroup to its row's record), the column pass (square only: thread =
// column record, the slab's rows in segments) and the flat histogram pass, which also counts the call's totals.  All state is
// integer: per record two 32-bit counters and the exact sum of the fixed-point values as hi = sum of (q >> 32), lo = sum of
// (q & 0xFFFFFFFF), so the result does not depend on the order anything arrives in.
constexpr int kSummaryTotals = 6;   // tot[]: NaN pairs, summable pairs, links, the high and the low word of the 128-bit sum
                                    // over pairs (the histogram pass); [5] NaN pairs again, by the row pass
struct SummaryBuffers {
    uint32_t *within;     // [records] links of the record
    uint32_t *summable;   // [records] its summable partners
    int64_t *hi;          // [records] sum of (q >> 32) over them
    uint64_t *lo;         // [records] sum of (q & 0xFFFFFFFF)
    uint64_t *hist;       // [bins]
    uint64_t *tot;        // [kSummaryTotals]
};
// rows [rb, re) of the slab, indexed as launch_links_count's; t_bits: the threshold as a payload, any: false when nothing
// can link (threshold_payload)
hipError_t launch_summary_rows(int measure, bool square, const uint64_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                               uint64_t re, uint64_t t_bits, bool any, const SummaryBuffers &b, hipStream_t stream);
// the same rows of the square, pairs (i, j > i), added to record j
hipError_t launch_summary_cols(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                               uint64_t t_bits, bool any, const SummaryBuffers &b, hipStream_t stream);
// entries [0, pairs) of the slab into b.hist (bins == 0: none) and b.tot; width_q: the bin width as a fixed-point value;
// aggregate: lanes of a wave that share a bin add once (false: the measurement's other side)
hipError_t launch_summary_hist(int measure, const uint64_t *slab, uint64_t pairs, uint32_t bins, uint64_t width_q,
                               uint64_t t_bits, bool any, bool aggregate, const SummaryBuffers &b, hipStream_t stream);
// A summary stream's batch (dst_stream.cpp): one tile pass over the batch's n_records x n_loaded matrix of
// DST_OUT_DISTANCE payloads, entry s n_loaded + i, every entry read once for both sides.  A workgroup takes a tile of
// kStreamSummaryRows rows x kStreamSummaryCols columns, a thread one column.  loaded / streamed: the per-record state of
// either side (within, summable, hi, lo; NULL: the side is not wanted and its code is not compiled in); tot: the first
// five words of a SummaryBuffers::tot.  Adds only: the state is zeroed by the caller.
constexpr uint32_t kStreamSummaryRows = 64;    // mirrored as STREAM_SUMMARY_ROWS in distance_amd/_lib.py
constexpr uint32_t kStreamSummaryCols = 256;   // ... and STREAM_SUMMARY_COLS
hipError_t launch_summary_stream(int measure, const uint64_t *matrix, uint64_t n_records, uint64_t n_loaded, uint64_t t_bits,
                                 bool any, const SummaryBuffers *loaded, const SummaryBuffers *streamed, uint64_t *tot,
                                 hipStream_t stream);

// ---- group summaries (dst_group_summary.hip, driven by dst_group_summary in dst_analysis.cpp) --------------------------
// dst_summary's per-pair quantities keyed by group.  Per row slab a row pass (the per-record table's entry (row, group of
// the column) and the cell's NaN count, smallest and largest key) and, in the square, a column pass (entry (column, group
// of the row)); after the walk one fold of the table into the cells' links, summable pairs and 128-bit sums.  All integer.
constexpr int kGroupCellWords = 7;   // planes of `cell`: NaN pairs, links, summable pairs, the high and the low word of the
                                     // 128-bit sum, the smallest nn_key (~0: none), the largest (0: none)
struct GroupBuffers {
    uint32_t *row_group;   // [n_rows] labels below g_rows, or DST_GROUP_NONE
    uint32_t *col_group;   // [n_cols] labels below g_cols (the square: row_group again)
    uint32_t *order;       // [n_rows] the row records that have a group, in order of it
    uint64_t *cell;        // [kGroupCellWords][g_rows g_cols]
    uint64_t *counts;      // [n_rows g_cols] within << 32 | summable of (record, column group)
    int64_t *hi;           // [n_rows g_cols] sum of (q >> 32)
    uint64_t *lo;          // [n_rows g_cols] sum of (q & 0xFFFFFFFF)
    uint32_t g_rows, g_cols;
};
// rows [rb, re) of the slab, indexed as launch_summary_rows'; aggregate: a wave adds its entries of one group to the
// workgroup's table once (false: the measurement's other side)
hipError_t launch_group_rows(int measure, bool square, const uint64_t *slab, uint64_t out_base, uint64_t n_cols, uint64_t rb,
                             uint64_t re, uint64_t t_bits, bool any, bool aggregate, const GroupBuffers &b, hipStream_t stream);
// the same rows of the square, pairs (i, j > i), added to entry (j, group of i)
hipError_t launch_group_cols(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             uint64_t t_bits, bool any, const GroupBuffers &b, hipStream_t stream);
// the table of the first `assigned` records of b.order into the cells
hipError_t launch_group_fold(const GroupBuffers &b, uint64_t assigned, hipStream_t stream);
// A group-summary stream's LOADED side (dst_stream.cpp): one tile pass over the batch's n_records x n_loaded
// matrix of DST_OUT_DISTANCE payloads, entry s n_loaded + i.  A workgroup takes a tile of kStreamGroupRows rows x
// kStreamGroupCols columns, a thread one loaded column, the rows in order of their streamed group.  b.row_group: the
// batch's labels; b.counts / hi / lo: the kept table [b.g_cols][n_loaded], group-major (a wave's adds of one word are
// adjacent), b.g_cols the STREAMED group count; nothing else of b is read.  Adds only.
constexpr uint32_t kStreamGroupRows = 64;    // mirrored as STREAM_GROUPS_ROWS in distance_amd/_lib.py
constexpr uint32_t kStreamGroupCols = 256;   // ... and STREAM_GROUPS_COLS
hipError_t launch_group_stream_cols(int measure, const uint64_t *matrix, uint64_t n_records, uint64_t n_loaded, uint64_t t_bits,
                                    bool any, const GroupBuffers &b, hipStream_t stream);

// ---- minimum spanning forest (dst_mst.hip, driven by dst_mst in dst_analysis.cpp) -------------------------------------
// Boruvka rounds: every round runs each row slab of the triangle into the DST_OUT_DISTANCE scratch (as dst_clusters) and
// scans it twice (the minimal key of every component's outgoing edges, then the smallest pair of that key), hooks every
// component along its best edge and flattens the component labels.  O(n) device state beside the slab.
struct MstBuffers {
    uint32_t *comp;        // [n] component of a record: a root r has comp[r] == r (between rounds)
    uint32_t *hook;        // [n] this round's hooks, by component root
    uint64_t *best_key;    // [n] by component root: the smallest nn_key of its outgoing edges (~0: none)
    uint64_t *best_pair;   // [n] ... and the smallest i << 32 | j of that key
    uint64_t *edges;       // [n] the forest's edges i << 32 | j in order of emission
    uint64_t *edge_keys;   // [n] their keys
    uint64_t *val;         // [n] their DST_OUT_DISTANCE payloads (the finish)
    uint32_t *tal;         // [n][tally_width] their DST_OUT_TALLY words
    uint64_t *counters;    // [0] edges so far, [1] edges of the current round
};
hipError_t launch_mst_reset(const MstBuffers &b, uint64_t n, bool first, hipStream_t stream);
// rows [rb, re) of the square, payloads from slab entry tri_row_start(n, i) - out_base: the key launch, then the pair launch
hipError_t launch_mst_scan(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                           const MstBuffers &b, hipStream_t stream);
hipError_t launch_mst_hook(const MstBuffers &b, uint64_t n, hipStream_t stream);   // hook + emit, then flatten
// the same rows as DST_OUT_TALLY words: the tallies and the value of every forest edge whose row lies in them (counts:
// tn93's base counts of the set)
hipError_t launch_mst_gather(int measure, const uint32_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             const uint32_t *counts, const MstBuffers &b, uint64_t n_edges, hipStream_t stream);

// ---- neighbour-joining trees (dst_nj.hip, driven by dst_nj / dst_nj_matrix in dst_analysis.cpp) ---------------------
// The n x n f64 square on the device, filled from row slabs of DST_OUT_DISTANCE payloads (as dst_clusters) or from the
// caller's matrix, then n - 3 rounds of a scan launch (kNjScanBlocks workgroups at most, one partial each) and a merge
// launch, and a compaction into the other matrix buffer whenever m <= floor(3P/4).  D[0]: n x n; D[1]: at least
// floor(3n/4)^2 entries (the first compaction's target; later ones fit either buffer).
constexpr uint64_t kNjScanBlocks = 2048;
struct NjBuffers {
    double *D[2];
    double *r[2];          // row sums by slot, read by one round's merge and written for the next
    uint32_t *ids[2];      // node id by slot (the second: the compaction's target)
    uint8_t *active;       // slot in the list
    uint32_t *pos;         // the compaction's gather map
    uint64_t *part_key, *part_ij;   // kNjScanBlocks scan partials
    uint32_t *parent;      // 2n - 2 entries
    double *length;
};
// diagonal := +0.0, ids := identity, every slot active, *bad := ~0
hipError_t launch_nj_init(double *D, uint64_t n, uint32_t *ids, uint8_t *active, unsigned long long *bad, hipStream_t stream);
// rows [rb, re) of the square from slab entry tri_row_start(n, i) - out_base into D (both halves); *bad := min(*bad,
// i * n + j) for every non-finite payload
hipError_t launch_nj_scatter(int measure, const uint64_t *slab, uint64_t out_base, uint64_t n, uint64_t rb, uint64_t re,
                             double *D, unsigned long long *bad, hipStream_t stream);
// D's strict upper triangle into the lower one
hipError_t launch_nj_mirror(double *D, uint64_t n, hipStream_t stream);
// every round, the root included, into b.parent / b.length; n >= 3, D[0] symmetric with a +0.0 diagonal
hipError_t launch_nj_rounds(const NjBuffers &b, uint64_t n, hipStream_t stream);

// ---- dendrograms (dst_dendrogram.hip, driven by dst_dendrogram / dst_dendrogram_matrix in dst_analysis.cpp) ---------
// The n x n f64 square (filled as for NJ) and a row-minimum cache: for every active slot x the smallest (nn_key, column)
// over the active k > x, and per block of kDgBlockRows rows the smallest cached key.  A round is three launches known
// from n alone: the select (one workgroup: the pair from the block minima, the new node), the merge (thread k: the
// linkage update of (a, k) and (k, a), row k's cache entry lowered or invalidated) and the rescan (a fixed grid that
// takes the invalidated rows from a device list).  All of it is O(n) beside D.
constexpr uint32_t kDgBlockRows = 256;
struct DgPair {
    uint32_t a, b, sa, sb;
};
struct DgBuffers {
    double *D;             // n x n
    uint8_t *active;       // slot holds a cluster
    uint32_t *node;        // node id by slot
    uint32_t *size;        // cluster size by slot
    uint64_t *row_key;     // cached minimum of row x over active k > x (~0: none, or the row waits for its rescan)
    uint32_t *row_col;     // ... and its column
    uint64_t *blk_key;     // ceil(n / kDgBlockRows) block minima of row_key
    uint32_t *list;        // the rows to rescan (n entries)
    uint32_t *counters;    // [0] entries of list, [1] entries taken, [2] 0, or 1 + the first round that found no pair
    unsigned long long *scans;   // whole-row scans so far
    DgPair *pair;          // the round's pair, from the select to the merge
    uint32_t *parent;      // 2n - 1 entries
    double *length, *height;
};
// node := identity, size := 1, heights := +0.0, every row listed for its first scan, the block minima := ~0
hipError_t launch_dg_init(const DgBuffers &b, uint64_t n, hipStream_t stream);
// the first scan of every row, then every round, the root included, into b.parent / b.length / b.height; n >= 2, D
// symmetric and finite
hipError_t launch_dg_rounds(const DgBuffers &b, uint64_t n, int linkage, hipStream_t stream);

// ---- bootstrap replicates (dst_bootstrap.hip, driven by dst_nj_bootstrap in dst_analysis.cpp) ------------------------
// replicate r of the n x len codes at src (rows pitch bytes apart, pitch a multiple of 128 and >= len) into out (the same
// pitch): out[i][c] := src[i][boot_column(seed, r * len + c, len)]; map: len entries of scratch
hipError_t launch_boot_resample(const uint8_t *src, uint64_t pitch, uint8_t *out, uint64_t n, uint64_t len, uint64_t seed,
                                uint32_t replicate, uint32_t *map, hipStream_t stream);

// ---- per-window distances (dst_windows.hip: the kernels and dst_run_windows / dst_window_base_counts) -----------------
struct WindowLaunch {
    const DeviceSet *rows, *cols;
    bool square;
    uint64_t row_begin, row_end;   // rows of `rows`
    uint64_t pairs;                // P: the pairs of the row range (an entry of window w lies at w * P + canonical index)
    int out_kind;                  // DST_OUT_DISTANCE or DST_OUT_TALLY
    void *d_out;
    const uint2 *d_windows;        // [n_windows] {begin, end}
    uint32_t n_windows;            // the launch sweeps windows [win_first, win_first + n_windows) of the table ...
    const uint4 *q_counts, *t_counts;   // tn93 distances: [n_windows][rows.n] / [n_windows][cols.n] {A,T,G,C} inside the window
    uint32_t win_first;            // ... and lays window w out at (w - win_first) * P (dst_run_windows: 0, the whole table)
};
hipError_t launch_window_pairs(int measure, const WindowLaunch &wl, hipStream_t stream);
// counts[w * set.n + record] = the record's {A,T,G,C}, counted by code, inside window w
hipError_t launch_window_counts(const DeviceSet &set, const uint2 *d_windows, uint32_t n_windows, uint4 *counts, hipStream_t stream);

// ---- per-window summaries (dst_window_summary.hip, driven by dst_window_summary in dst_windows.hip) -------------------
// The window sweep of all the rows with dst_summary's reduction in its epilogue.  The state is zeroed by the caller and
// window-major: the per-record arrays [n_windows][rows->n] (all four, or all NULL: the totals only, O(n_windows) of
// state), tot [n_windows][kWindowSummaryTotals]: NaN pairs, summable pairs, links, the high and the low word of the
// 128-bit sum.  rows->n x n_windows <= 2^31 when the per-record arrays are there.
constexpr int kWindowSummaryTotals = 5;
enum {
    kWinSumRect = 0,       // every row record against every column record; per-record entries of the row records
    kWinSumTriangle = 1,   // one set, the pairs i < j; a pair adds to both of its records (row side and column side)
    kWinSumFull = 2,       // one set, every row against all j != i, the row side only: links, summable pairs and the sum
                           // of tot come out doubled; needs the per-record arrays (the measured alternative)
};
struct WindowSummaryLaunch {
    const DeviceSet *rows, *cols;
    int mode;
    const uint2 *d_windows;        // [n_windows] {begin, end}
    uint32_t n_windows;
    const uint4 *q_counts, *t_counts;   // tn93: [n_windows][rows.n] / [n_windows][cols.n] {A,T,G,C} inside the window
    uint64_t t_bits;               // the threshold as a payload; any: false when nothing can link (threshold_payload)
    bool any;
    uint32_t *within, *summable;
    int64_t *hi;
    uint64_t *lo;
    uint64_t *tot;
};
hipError_t launch_window_summary(int measure, const WindowSummaryLaunch &wl, hipStream_t stream);

// ---- per-window group summaries (dst_window_group_summary.hip, driven by dst_window_group_summary in dst_windows.hip) --
// The same sweep with dst_group_summary's reduction in its epilogue.  The state is zeroed by the caller, the cells' min
// keys then set by launch_window_group_init.  cell [n_windows][g_rows][g_cols][kWindowGroupCellWords]: NaN pairs, links,
// summable pairs, the high and the low word of the 128-bit sum, the smallest nn_key (~0: none), the largest (0: none).
// The per-record arrays [n_windows][rows->n][g_cols] (all three, or all NULL): within << 32 | summable, hi, lo.
// mode: kWinSumRect; kWinSumTriangle (cells alone: each pair i < j once at (group of i, group of j)); kWinSumFull (with the
// per-record arrays: every row against all j != i, so cell (a, b != a) holds each pair once and cell (a, a) each twice).
constexpr int kWindowGroupCellWords = 7;
struct WindowGroupLaunch {
    const DeviceSet *rows, *cols;
    int mode;
    const uint2 *d_windows;        // [n_windows] {begin, end}
    uint32_t n_windows;
    const uint4 *q_counts;         // tn93 only: per-window base counts of the row set [n_windows][rows->n] and of the
    const uint4 *t_counts;         // column set [n_windows][cols->n]
    uint64_t t_bits;               // the threshold as a payload; any: false when nothing can link (threshold_payload)
    bool any;
    const uint32_t *row_group;     // [rows->n] labels below g_rows, or DST_GROUP_NONE
    const uint32_t *col_group;     // [cols->n] labels below g_cols (one set: row_group again)
    uint32_t g_rows, g_cols;       // 1 .. DST_WINDOW_GROUPS_MAX
    uint64_t *cell;
    uint64_t *rec_counts;
    int64_t *rec_hi;
    uint64_t *rec_lo;
};
hipError_t launch_window_group_init(uint64_t *cell, uint64_t cells, hipStream_t stream);
hipError_t launch_window_groups(int measure, const WindowGroupLaunch &wl, hipStream_t stream);

// dst_group_summary's label check (dst_analysis.cpp): size[a] = the records of group a; the error names the first record
// whose label is neither below `count` nor DST_GROUP_NONE, and its side
int group_labels(dst_ctx *ctx, const uint32_t *group, uint64_t n, uint32_t count, const char *side, std::vector<uint64_t> &size);
// the payload of a sort key (nn_key): -0.0 has the key of +0.0 and comes back as +0.0
uint64_t payload_of_key(uint64_t key, bool int_payload);

// ---- k nearest records per window (dst_window_nearest.hip, driven by dst_nearest_windows in dst_windows.hip) ----------
// A slab is rows [row0, row0 + nr) x windows [win0, win0 + nw) x all n_cols column records as DST_OUT_TALLY words, entry
// (w_local * nr + i_local) * n_cols + j (launch_window_pairs with win_first = win0 on the rectangle; a square job sweeps
// slot 0 against itself).  One wave per (row, window) list; list i_local * nw + w_local of nl (k entries each) is written
// whole.  q_counts / t_counts: tn93's per-window tables [window][record] of the row and the column set.
constexpr uint64_t kWindowNearestPairs = (uint64_t)1 << 25;      // pair-windows of a slab unless the caller says otherwise
constexpr uint64_t kWindowNearestListsMax = (uint64_t)1 << 31;   // lists of one slab: a list number is 32 bits on the device
hipError_t launch_window_nearest(int measure, const uint32_t *slab, const uint4 *q_counts, const uint4 *t_counts, uint64_t q_n,
                                 uint64_t n_cols, uint64_t row0, uint64_t nr, uint32_t win0, uint32_t nw, bool square,
                                 const NearestLists &nl, hipStream_t stream);
// The rows x windows of a job cut into ranges whose tallies (x n_cols column records) fit max_entries (0: 2^25): whole
// row ranges of all the windows while a row's windows fit the budget, else a few rows (the sweep's tile holds eight) of
// a range of windows; at least one (row, window) (dst_nearest_windows, window-closest streams; dst_windows.hip)
struct WindowSlabs {
    uint64_t rows;   // rows of a slab (the last one of a job may hold fewer)
    uint32_t wins;   // windows of a slab (likewise)
};
WindowSlabs cut_window_slabs(uint64_t n_rows, uint32_t n_windows, uint64_t n_cols, uint64_t max_entries);

// ---- k nearest streamed records per window (dst_window_nearest_stream.hip, driven by dst_stream.cpp) ------------------
// The merge of one batch into the lists of a window-closest stream.  The slab is the one above with the batch as the
// column set: loaded rows [row0, row0 + nr) x windows [win0, win0 + nw) x n_batch records.  List i * n_windows + w of nl
// (k entries each; q_n * n_windows <= 2^31) is loaded, offered the batch's candidates with the ordinals first_ordinal + j
// (<= 2^32-2) and stored.  q_counts: the loaded set's per-window table [n_windows][q_n], t_counts: the batch's
// [n_windows][n_batch], cnt: the listed streamed records' counts, 4 words per entry (all three tn93 only, else unused).
// Launches that share lists must follow one another on one stream.
hipError_t launch_window_nearest_stream(int measure, const uint32_t *slab, const uint4 *q_counts, const uint4 *t_counts,
                                        uint64_t q_n, uint64_t n_batch, uint64_t row0, uint64_t nr, uint32_t win0, uint32_t nw,
                                        uint32_t n_windows, uint32_t first_ordinal, const NearestLists &nl, uint32_t *cnt,
                                        hipStream_t stream);

// ---- host-only logic (dst_host.cpp) ----------------------------------------------------------
int tally_width(int measure);
bool measure_is_int(int measure);
// tiles of a launch, interleaved so that blocks b and b+8 (observed to share an XCD and its L2)
// walk the same column tile
std::vector<BlockDesc> build_blocks(bool square, uint64_t row_begin, uint64_t row_end,
                                    uint64_t n_cols, TileShape ts);
uint64_t square_row_start(uint64_t n, uint64_t i);
uint64_t pairs_in_rows(bool square, uint64_t n_cols, uint64_t row_begin, uint64_t row_end);
// rows [0, n_rows) cut in order into slabs of at most max_pairs pairs (at least one row each); slabs without pairs are
// left out.  first = canonical index of the slab's first pair (dst_run_slabs, dst_nearest)
struct RowSlab {
    uint64_t rb, re, first, pairs;
};
std::vector<RowSlab> cut_row_slabs(bool square, uint64_t n_rows, uint64_t n_cols, uint64_t max_pairs);
// dst_newick's shape checks of a dst_nj tree (2n - 2 nodes): ids in range, exactly one root, three children at the root,
// two at every other internal node, none at a leaf, every node below the root.  The children of x in ascending id are
// child[first[x] .. first[x + 1]).  rooted: a dst_dendrogram tree instead (2n - 1 nodes, two children at the root too).
bool tree_children(uint64_t n, const uint32_t *parent, std::vector<uint64_t> &first, std::vector<uint64_t> &child,
                   uint64_t &root, bool rooted = false);
// Bootstrap support (dst_nj_bootstrap): the main tree's splits, each internal non-root node x's, keyed exactly by an
// interval of leaf numbers; count() adds 1 to support[x] for every main split a replicate tree holds.  O(n) per tree.
class SplitCounter {
public:
    bool init(uint64_t n, const uint32_t *parent);        // false: not a valid tree (tree_children)
    bool count(const uint32_t *rep_parent, uint32_t *support);
private:
    void walk(const uint32_t *parent, std::vector<uint32_t> &order, std::vector<uint32_t> &up);
    uint64_t n_ = 0;
    std::vector<uint32_t> rank_, order_, up_, lo_, hi_, cnt_, adj_, adj_first_;
    std::unordered_map<uint64_t, uint32_t> split_;   // (lo << 32 | hi) -> main node
};

}  // namespace dst
