// The command line: help text, the flags, the scan, and the one table of what may not be combined.
#pragma once
#include <cctype>
#include <cmath>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "base.hpp"

namespace {

void print_help()
{
    std::puts(
        "Calculate genetic distances within/between fasta-format alignments of DNA sequences\n\n"
        "Usage: All sequences across all input files must be the same length.\n\n"
        "       distance alignment.fasta\n"
        "       cat alignment.fasta | distance\n"
        "       distance alignment.fasta -o distances.tsv\n"
        "       distance -t 8 -m jc69 alignment.fasta -o jc69.tsv\n"
        "       distance alignment1.fasta alignment2.fasta > distances2.tsv\n"
        "       distance -i smallAlignment.fasta -s bigAlignment.fasta -o distances3.tsv\n"
        "       cat bigAlignment.fasta | distance smallAlignment.fasta -s - > distances3.tsv\n"
        "       \n\n"
        "Options:\n"
        "  -i, --input [<input>...]     One or two input alignment files in fasta format. Loaded into memory. "
        "This flag can be omitted and the files passed as positional arguments\n"
        "  -s, --stream <stream>        One input alignment file in fasta format. Streamed from disk (or stdin "
        "using \"-s -\"). Requires exactly one file also be loaded\n"
        "  -m, --measure <measure>      Which distance measure to use [default: raw] [possible values: n, n_high, "
        "raw, jc69, k80, tn93]\n"
        "  -o, --output <output>        Output file in tab-separated-value format. Omit this option to print to "
        "stdout\n"
        "  -t, --threads <threads>      How many threads to spin up for pairwise comparisons. Omitting this option "
        "spins up the number of available CPUs\n"
        "  -b, --batchsize <batchsize>  Try setting this >(>) 1 to tune the workload per thread [default: 1]\n"
        "  -l, --licenses               Print licence information and exit\n"
        "      --gpus <n>               MI355X GPUs to use (default 1)\n"
        "      --devices <list>         Explicit device ordinals, e.g. 0,1,2,3 (overrides --gpus)\n"
        "      --nearest <k>            Print only the k (1-256) nearest records of every record: of the same file with one "
        "input, of the second file with two. One GPU, no --stream\n"
        "      --closest <k>            Stream mode only: print only the k (1-256) closest records instead of every pair, "
        "each as the line the full run prints for that pair. Requires --stream, one loaded file, one GPU, no other output mode\n"
        "      --closest-for <side>     Whose closest records --closest prints: loaded (for every loaded record its k closest "
        "streamed records, written when the stream ends) or streamed (for every streamed record its k closest loaded "
        "records, in stream order) [default: loaded]\n"
        "      --within <T>             Stream mode only: print only the pairs within distance T (a number >= 0, or inf): the "
        "lines of the full run whose distance is at most T, in the same order and with the same text. Requires --stream, one "
        "loaded file, one GPU, no other output mode\n"
        "      --stream-summary <T>     Stream mode only: print one line per record instead of one per pair, as --summary "
        "does: how many records of the other file lie within distance T (a number >= 0, or inf) of it, how many it was "
        "compared with and its mean distance to those. Reduced on the GPU: no pair is sent back. Requires --stream, one "
        "loaded file, one GPU, no other output mode\n"
        "      --stream-summary-for <side>  Whose lines --stream-summary prints: loaded (every loaded record against the whole "
        "stream, written when the stream ends) or streamed (every streamed record against the loaded file, in stream "
        "order) [default: loaded]\n"
        "      --stream-histogram <W>   Stream mode only: print the histogram of the distances between the loaded and the "
        "streamed records, as --histogram does, bins of width W. Requires --stream, one loaded file, one GPU, no other "
        "output mode\n"
        "      --stream-bins <B>        Bins of --stream-histogram, 1 to 4096 [default: 256]\n"
        "      --stream-groups <FILE>   Stream mode only: print --groups' lines for the streamed file against the loaded one, "
        "reduced on the GPU batch by batch: FILE as for --groups, an id's group applies to whichever file carries it; the "
        "streamed groups are numbered in order of their first record (at most 1024). Requires --stream, one loaded file, one "
        "GPU, no other output mode\n"
        "      --stream-groups-by <what>  What --stream-groups prints a line for: cell (a streamed group and a loaded group, "
        "written when the stream ends: the lines of '--groups FILE streamed loaded'), streamed (every streamed record and "
        "loaded group, in stream order: the lines '--groups FILE streamed loaded' prints when asked for a line per record; "
        "needs no streamed labels) or loaded (every loaded record and streamed group, written when the stream ends; needs no loaded labels) "
        "[default: cell]\n"
        "      --stream-groups-within <T>  With --stream-groups: a 'within' column, the compared pairs within distance T (a "
        "number >= 0, or inf)\n"
        "      --clusters <T>           Print the single-linkage cluster of every record instead of distances: records "
        "within distance T (a number >= 0) of each other share a cluster, numbered from 1 in order of first record. One "
        "input, one GPU, no --stream or --nearest\n"
        "      --representatives <T>    Print the greedy representative of every record instead of distances: in input order a "
        "record is kept (a representative) unless a record kept before it lies within distance T (a number >= 0, or inf); every "
        "other record is listed with the first kept record within T of it and their distance. No two kept records are within "
        "T of each other. One input, one GPU, no --stream and no other output mode\n"
        "      --max-distance <T>       Print only the pairs within distance T (a number >= 0, or inf): the lines of the full "
        "run whose distance is at most T, in the same order and with the same text. One or two inputs, one GPU, no --stream "
        "and no other output mode\n"
        "      --summary <T>            Print one line per record instead of one per pair: how many records lie within distance "
        "T (a number >= 0, or inf) of it, how many it was compared with (pairs with a distance) and its mean distance to "
        "those. With two inputs: the records of the first against the second. One GPU, no --stream and no other output mode\n"
        "      --histogram <W>          Print the histogram of the pairwise distances instead of the pairs: one line per bin "
        "of width W (a number > 0; an integer with -m n / n_high), its lower edge and its pairs, the last bin open-ended, then "
        "the pairs without a distance (NaN). One GPU, no --stream and no other output mode\n"
        "      --bins <B>               Bins of the histogram, 1 to 4096 [default: 256]. Requires --histogram\n"
        "      --groups <FILE>          Print one line per pair of groups instead of one per pair of records: FILE has one "
        "'id<TAB>group' line per labelled record (no header; at most 1024 groups per input, numbered in order of their first "
        "record); the line gives the pairs between the two groups, how many were compared (pairs with a distance), their "
        "mean, smallest and largest distance. With two inputs: the groups of the first against those of the second. For "
        "jc69 / k80 / tn93 min and max are the device's values and can differ from the long output's text in the 12th "
        "decimal on a rounding boundary. One GPU, no --stream and no other output mode\n"
        "      --groups-within <T>      With --groups: a 'within' column, the compared pairs within distance T (a number >= 0, "
        "or inf)\n"
        "      --per-record             With --groups: one line per record of the first input and group of the other side "
        "instead (the record's compared partners in the group and its mean distance to them), labelled or not\n"
        "      --matrix <format>        Print a distance matrix instead of one line per pair: tsv (one or two inputs, rows "
        "from the first, columns from the last) or phylip (relaxed PHYLIP, one input). Not in stream, nearest or "
        "clusters mode\n"
        "      --tree <method>          Print the tree of the records as one Newick line instead of distances: method nj "
        "(neighbour joining). One input, one GPU, no --stream and no other output mode\n"
        "      --bootstrap <B>          Label each internal edge of the neighbour-joining tree with the number of B "
        "(1-10000) bootstrap replicates (alignments of columns drawn with replacement) whose tree holds its split\n"
        "      --seed <S>               Seed of the bootstrap's column draws, 0 to 2^64-1 [default: 1]\n"
        "      --mst                    Print only the edges of the minimum spanning tree of the records (pairs without a "
        "distance, NaN, are no edges: a forest then), in ascending order of (distance, first record, second record), each "
        "as the line the full run prints for that pair. One input, one GPU, no --stream and no other output mode\n"
        "      --sites                  With one of the pair-list outputs (the pairs within a distance, the minimum spanning "
        "tree, the pairs of --pairs): a fourth field per line, the sites that separate the two "
        "records as a comma-separated list of X<pos>Y (pos 1-based, X the first record's IUPAC letter, Y the second's; '.' "
        "when there are none): the sites the measure counts as differences\n"
        "      --pairs <FILE>           Print only the pairs FILE names: FILE has one 'id1<TAB>id2' line per pair (no header, empty "
        "lines skipped); with one input both ids are looked up in it, with two id1 in the first and id2 in the second. One "
        "line per line of FILE, in its order, the two ids as given and the distance exactly as the long output prints it "
        "for that pair (with the separating sites as a fourth field when those are asked for). One GPU, no --stream and no other output mode\n"
        "      --windows <W>            Print every pair's distance per column window instead of over the whole width: windows "
        "of W sites (an integer >= 1) starting every S sites, the last one cut at the alignment's end; a line per pair and "
        "window, 'id1, id2, window number, start, end (1-based, inclusive), distance', the distance exactly what the long "
        "output prints for the pair on the input cut to those columns. One input, or two (the records of the first "
        "against the second). One GPU, no --stream and no other output mode\n"
        "      --step <S>               The distance between the starts of consecutive windows (an integer >= 1) [default: W]. "
        "Requires --windows\n"
        "      --regions <FILE>         As --windows, for named column ranges: FILE has one 'name<TAB>start<TAB>end' line per "
        "region (no header; positions 1-based and inclusive; at most 65536 regions); the window field of a line is the "
        "region's name\n"
        "      --window-nearest <K>     With --windows or --regions: print only the K (1-256) nearest records of every record "
        "of the first input in every window (of the same file with one input, of the second file with two): per record and "
        "window the K lines of the plain --windows / --regions run with the smallest distance, nearest first, ties in input "
        "order\n"
        "      --window-summary <T>     With --windows or --regions: print one line per window instead of one per pair and window: "
        "the window, its pairs, how many were compared (pairs with a distance inside the window), how many lie within "
        "distance T (a number >= 0, or inf) and their mean distance: diversity along the alignment, reduced on the GPU. "
        "One input, or two (the records of the first against the second). One GPU, no --stream and no other output mode\n"
        "      --window-summary-by <what>  What --window-summary prints a line for: window, or record (for every record of the "
        "first input one line per window: the records within T of it inside the window, how many it was compared with and "
        "its mean distance to those) [default: window]\n"
        "      --window-groups <FILE>   With --windows or --regions: print --groups' lines per window instead of one line per pair "
        "and window: FILE as for --groups (at most 256 groups in one input); per window and pair of groups the pairs, how many "
        "were compared, their mean, smallest and largest distance inside the window, reduced on the GPU. With '-m raw' the "
        "mean of a group with itself is its nucleotide diversity in the window, the mean between two groups their d_xy. One "
        "input, or two (the records of the first against the second). One GPU, no --stream and no other output mode\n"
        "      --window-groups-within <T>  With --window-groups: a 'within' column, the compared pairs within distance T (a "
        "number >= 0, or inf)\n"
        "      --window-groups-by <what>  What --window-groups prints a line for: cell (a pair of groups), or record (for every "
        "record of the first input and every window one line per group of the other side: how many of the group it was "
        "compared with and its mean distance to them) [default: cell]\n"
        "      --window-closest <K>     Stream mode, with --windows or --regions: for every loaded record and every window the K "
        "(1-256) nearest STREAMED records, written when the stream ends: byte for byte what '--window-nearest K loaded.fasta "
        "streamed.fasta' prints, for a streamed file that need not fit on the GPU. Requires --stream, one loaded file, one "
        "GPU, no other output mode\n"
        "      --site-counts            Print the allele counts of every site instead of distances: one line per site (1-based) "
        "and group, 'site, group, records, A, C, G, T, ambiguous, missing': the records of the group whose letter there is "
        "exactly that base, those with an ambiguity code of 2 or 3 bases, and those with N, - or ?. Counted on the GPU. "
        "One input, one GPU; -m is accepted and ignored; no --stream and no other output mode\n"
        "      --window-site-stats      With --windows or --regions: print one line per window and group instead of one per pair "
        "and window, 'window, start, end, group, records, sites, called, segregating, theta_w, pi': the sites with at least "
        "two single-base calls, those of them with more than one base (S), Watterson's theta per called site and the "
        "per-site nucleotide diversity over single-base calls (not the mean of the pairwise raw distances, which counts "
        "each pair's own comparable sites). From the per-site allele counts of the GPU. One input, one GPU; -m is accepted "
        "and ignored\n"
        "      --site-groups <FILE>     With --site-counts or --window-site-stats: count per group. FILE as for --groups (at "
        "most 1024 groups, numbered in order of their first record); without it there is one group, 'all', of every record\n"
        "      --ld <R2>                Print the linkage disequilibrium between the variable sites instead of distances: one line "
        "per pair of sites whose r^2 is at least R2 (a number from 0 to 1), 'site1, site2 (1-based), group, major1, major2 (the "
        "sites' major bases), called (records with a single base at both sites), minor1, minor2 (of those, the records whose base "
        "is not the major one at site1, at site2), both, r2, D, Dprime'. Tallied on the GPU. One input, one GPU; -m is accepted "
        "and ignored; no --stream and no other output mode\n"
        "      --ld-min-count <C>       With --ld: a site is listed when both its major base and all its other bases together "
        "are held by at least C records (an integer >= 1) [default: 1]\n"
        "      --ld-groups <FILE>       With --ld: per group. FILE as for --groups (at most 1024 groups, numbered in order of "
        "their first record); each group chooses its own sites and major bases. Without it there is one group, 'all', of every "
        "record\n"
        "      --ld-max-gap <G>         With --ld: only the pairs of sites at most G sites apart (site2 - site1 <= G, an integer; "
        "PLINK's --ld-window-kb in sites): exactly those lines of the plain --ld output, from the band of the triangle alone\n"
        "      --ld-decay <W>           With --ld: print the LD-decay curve instead of the pairs, one line per group and bin of W "
        "sites (an integer from 1 to 4294967295) of the distance site2 - site1, 'group, gap (the bin's lower edge), pairs, defined (pairs whose "
        "r^2 is defined), linked (those with r^2 >= R2), mean_r2 (over the defined pairs; NaN without one)'. Pairs past the last "
        "bin are left out. Summed on the GPU\n"
        "      --ld-bins <B>            With --ld-decay: the number of bins (1-4096) [default: 256]\n"
        "      --dendrogram <linkage>   Print the rooted hierarchical-clustering tree of the records as one Newick line instead "
        "of distances: linkage average (UPGMA), weighted (WPGMA) or complete. One input, one GPU, no --stream and no other "
        "output mode\n"
        "  -h, --help                   Print help\n"
        "  -V, --version                Print version");
}

const char *kLicences =
    "\nCopyright 2022, Ben Jackson (distance, GNU LIBRARY GENERAL PUBLIC LICENSE, Version 2): this program is an\n"
    "independent MI355X re-implementation of its command-line surface and output format.\n"
    "FASTA tokenisation follows Rust-Bio (MIT licence, Copyright (c) 2016 Johannes Koester, the Rust-Bio team,\n"
    "Google Inc.).  Nucleotide coding scheme: Emmanuel Paradis, as used in ape.\n";

// ---------------------------------------------------------------- arguments -------------------
// Every flag the checks below speak about, by the name the messages print.
enum Flag {
    F_STREAM, F_MEASURE, F_OUTPUT, F_THREADS, F_BATCHSIZE, F_GPUS, F_DEVICES, F_SLAB_PAIRS, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR,
    F_WITHIN, F_CLUSTERS, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS, F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX,
    F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES, F_DENDROGRAM, F_SELFTEST, F_REPRESENTATIVES,
    F_WINDOWS, F_STEP, F_REGIONS, F_WINDOW_NEAREST, F_PAIRS, F_WINDOW_CLOSEST,
    F_WINDOW_SUMMARY, F_WINDOW_SUMMARY_BY, F_WINDOW_GROUPS, F_WINDOW_GROUPS_WITHIN, F_WINDOW_GROUPS_BY,
    F_STREAM_SUMMARY, F_STREAM_SUMMARY_FOR, F_STREAM_HISTOGRAM, F_STREAM_BINS,
    F_STREAM_GROUPS, F_STREAM_GROUPS_BY, F_STREAM_GROUPS_WITHIN,
    F_SITE_COUNTS, F_WINDOW_SITE_STATS, F_SITE_GROUPS, F_LD, F_LD_MIN_COUNT, F_LD_GROUPS, F_LD_MAX_GAP,
    F_LD_DECAY, F_LD_BINS, F_COUNT
};
struct FlagDef {
    const char *shown;   // "--name <value>": its first word is the flag itself
    const char *letter;  // "-s", or null
    bool once;           // a second one is refused (the others keep their last value)
};
const FlagDef kFlags[F_COUNT] = {
    {"--stream <stream>", "-s", false}, {"--measure <measure>", "-m", false}, {"--output <output>", "-o", false},
    {"--threads <threads>", "-t", false}, {"--batchsize <batchsize>", "-b", false}, {"--gpus <n>", nullptr, false},
    {"--devices <list>", nullptr, false}, {"--slab-pairs <p>", nullptr, false}, {"--nearest <k>", nullptr, false},
    {"--closest <k>", nullptr, false}, {"--closest-for <side>", nullptr, false}, {"--within <T>", nullptr, true},
    {"--clusters <T>", nullptr, false}, {"--max-distance <T>", nullptr, true}, {"--summary <T>", nullptr, true},
    {"--groups <FILE>", nullptr, true}, {"--groups-within <T>", nullptr, true}, {"--per-record", nullptr, false},
    {"--histogram <W>", nullptr, true}, {"--bins <B>", nullptr, false}, {"--matrix <format>", nullptr, false},
    {"--tree <method>", nullptr, false}, {"--bootstrap <B>", nullptr, false}, {"--seed <S>", nullptr, false},
    {"--mst", nullptr, false}, {"--sites", nullptr, false}, {"--dendrogram <linkage>", nullptr, false},
    {"--host-selftest <what>", nullptr, false}, {"--representatives <T>", nullptr, true},
    {"--windows <W>", nullptr, true}, {"--step <S>", nullptr, true}, {"--regions <FILE>", nullptr, true},
    {"--window-nearest <K>", nullptr, true}, {"--pairs <FILE>", nullptr, true}, {"--window-closest <K>", nullptr, true},
    {"--window-summary <T>", nullptr, true}, {"--window-summary-by <what>", nullptr, false},
    {"--window-groups <FILE>", nullptr, true}, {"--window-groups-within <T>", nullptr, true},
    {"--window-groups-by <what>", nullptr, false},
    {"--stream-summary <T>", nullptr, true}, {"--stream-summary-for <side>", nullptr, false},
    {"--stream-histogram <W>", nullptr, true}, {"--stream-bins <B>", nullptr, false},
    {"--stream-groups <FILE>", nullptr, true}, {"--stream-groups-by <what>", nullptr, false},
    {"--stream-groups-within <T>", nullptr, true},
    {"--site-counts", nullptr, true}, {"--window-site-stats", nullptr, true}, {"--site-groups <FILE>", nullptr, true},
    {"--ld <R2>", nullptr, true}, {"--ld-min-count <C>", nullptr, true}, {"--ld-groups <FILE>", nullptr, true},
    {"--ld-max-gap <G>", nullptr, true}, {"--ld-decay <W>", nullptr, true}, {"--ld-bins <B>", nullptr, true},
};

// what the run prints, decided once by parse_args
enum class Mode { Pairs, Stream, Closest, Within, Nearest, Clusters, MaxDistance, Summary, Histogram, Groups, Matrix, Tree, Mst,
                  Dendrogram, Representatives, Windows, PairList, WindowClosest, StreamSummary, StreamHistogram, StreamGroups,
                  SiteCounts, Ld };

struct Args {
    bool has[F_COUNT] = {};               // the flag was given
    Mode mode = Mode::Pairs;
    std::vector<std::string> flag_inputs, pos_inputs;
    std::string stream, measure = "raw", output;
    bool licenses = false;
    size_t threads = 0, batchsize = 1;
    int gpus = 1;
    std::vector<int> devices;  // explicit device ordinals (--devices 0,1,..); empty: 0..gpus-1
    size_t slab_pairs = (size_t)1 << 22;  // result slab: 4 Mi pairs pipelines GPU, formatters and writer well
    size_t nearest = 0;                   // --nearest k
    size_t closest = 0;                   // --closest k (stream mode)
    int closest_side = DST_CLOSEST_FOR_LOADED;   // --closest-for loaded|streamed
    double within = 0;                    // --within T (stream mode)
    double clusters = 0;                  // --clusters T
    double representatives = 0;           // --representatives T
    double max_distance = 0;              // --max-distance T
    double summary = 0;                   // --summary T
    double histogram = 0;                 // --histogram W
    std::string groups;                   // --groups FILE
    double groups_within = 0;             // --groups-within T
    size_t bins = 256;                    // --bins B
    int matrix = -1;                      // --matrix: DST_MATRIX_TSV / DST_MATRIX_PHYLIP (-1: the long form)
    size_t bootstrap = 0;                 // --bootstrap B (0: none)
    size_t seed = 1;                      // --seed S
    int dendrogram = -1;                  // --dendrogram: DST_LINK_* (-1: none)
    size_t windows = 0, step = 0;         // --windows W --step S (step 0: W)
    std::string regions;                  // --regions FILE
    size_t window_nearest = 0;            // --window-nearest K (0: every pair)
    size_t window_closest = 0;            // --window-closest K (stream mode)
    std::string pairs;                    // --pairs FILE
    double window_summary = 0;            // --window-summary T
    bool window_summary_by_record = false;   // --window-summary-by window|record
    std::string window_groups;            // --window-groups FILE
    double window_groups_within = 0;      // --window-groups-within T
    bool window_groups_by_record = false;    // --window-groups-by cell|record
    double stream_summary = 0;            // --stream-summary T (stream mode)
    bool stream_summary_streamed = false;    // --stream-summary-for loaded|streamed
    double stream_histogram = 0;          // --stream-histogram W (stream mode)
    size_t stream_bins = 256;             // --stream-bins B
    std::string stream_groups;            // --stream-groups FILE (stream mode)
    int stream_groups_by = 0;             // --stream-groups-by cell|streamed|loaded: 0, 1, 2
    double stream_groups_within = 0;      // --stream-groups-within T
    std::string site_groups;              // --site-groups FILE
    double ld = 0;                        // --ld R2
    size_t ld_min_count = 1;              // --ld-min-count C
    std::string ld_groups;                // --ld-groups FILE
    size_t ld_max_gap = 0;                // --ld-max-gap G (has[F_LD_MAX_GAP])
    size_t ld_decay = 0;                  // --ld-decay W (0: the pairs)
    size_t ld_bins = 256;                 // --ld-bins B
    std::string selftest;
    size_t n_inputs() const { return flag_inputs.size() + pos_inputs.size(); }
    // the slab size an analysis is given: the library's own choice unless --slab-pairs was passed
    uint64_t analysis_slab() const { return has[F_SLAB_PAIRS] ? slab_pairs : 0; }
};

[[noreturn]] void die_value(const std::string &v, const char *shown, const std::string &why)
{
    die_usage("invalid value '" + v + "' for '" + shown + "'" + why);
}

size_t parse_usize(const std::string &v, const char *shown)
{
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos)
        die_value(v, shown, ": invalid digit found in string");
    errno = 0;
    unsigned long long x = std::strtoull(v.c_str(), nullptr, 10);
    if (errno)
        die_value(v, shown, ": number too large to fit in target type");
    return (size_t)x;
}

size_t parse_in_range(const std::string &v, const char *shown, size_t lo, size_t hi)
{
    const size_t x = parse_usize(v, shown);
    if (x < lo || x > hi)
        die_value(v, shown, ": " + v + " is not in " + std::to_string(lo) + "..=" + std::to_string(hi));
    return x;
}

// the whole word is the number (or inf): strtod, nothing left over, not NaN
double parse_number(const std::string &v, const char *shown)
{
    char *end = nullptr;
    const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
    if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
        die_value(v, shown, ": not a number");
    return t;
}

double parse_threshold(const std::string &v, const char *shown)
{
    const double t = parse_number(v, shown);
    if (t < 0)
        die_value(v, shown, ": the threshold must not be negative");
    return t;
}

// one of an enumerated list of words -> its value
int parse_choice(const std::string &v, const char *shown, std::initializer_list<std::pair<const char *, int>> choices,
                 const char *note = "")
{
    std::string words;
    for (const auto &c : choices) {
        if (v == c.first)
            return c.second;
        words += std::string(words.empty() ? "" : ", ") + c.first;
    }
    die_value(v, shown, "\n  [possible values: " + words + "]" + note);
}

// The checks that follow the scan, as one table walked top to bottom.  A row speaks when its flag was given, and says the
// first thing that is wrong, in this order: a flag of `refuses` is present (the first one in the row's order is named); none
// of `needs` is; a second loaded file; more than one GPU.  The rows' order and each row's own order are the order the
// messages have always had: which of two modes names the other, and which of several flags is named, is behaviour.
enum TwoInputs { TWO_OK, ONE_INPUT, ONE_LOADED, ONE_FOR_PHYLIP };
struct Rule {
    Flag flag;
    Mode mode;                  // the output mode the flag selects (Mode::Pairs: it is a modifier)
    std::vector<Flag> refuses;
    std::vector<Flag> needs;    // any one of them will do
    const char *needs_shown;    // how the message names them
    TwoInputs two_inputs;
    bool one_gpu;
};
const std::vector<Flag> kNone;
// everything --windows / --regions cannot go with: stream mode, every other output mode and every modifier of one
const std::vector<Flag> kWindowRefuses = {
    F_STREAM, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_REPRESENTATIVES, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS,
    F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES, F_DENDROGRAM};
std::vector<Flag> after(Flag first, std::vector<Flag> rest)
{
    rest.insert(rest.begin(), first);
    return rest;
}
// everything --stream-summary / --stream-histogram cannot go with: every other output mode and every modifier of one (each
// other and each other's modifier: in their rows)
const std::vector<Flag> kStreamSummaryRefuses = {
    F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_REPRESENTATIVES, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS,
    F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES, F_DENDROGRAM,
    F_WINDOWS, F_STEP, F_REGIONS, F_WINDOW_NEAREST, F_PAIRS, F_WINDOW_CLOSEST, F_WINDOW_SUMMARY, F_WINDOW_SUMMARY_BY,
    F_WINDOW_GROUPS, F_WINDOW_GROUPS_WITHIN, F_WINDOW_GROUPS_BY};
// everything --site-counts / --window-site-stats cannot go with besides --windows / --regions / --step: stream mode, every
// other output mode and every modifier of one (--sites, the pair lists' modifier, among them)
const std::vector<Flag> kSiteRefuses = {
    F_STREAM, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_REPRESENTATIVES, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS,
    F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES, F_DENDROGRAM,
    F_WINDOW_NEAREST, F_PAIRS, F_WINDOW_CLOSEST, F_WINDOW_SUMMARY, F_WINDOW_SUMMARY_BY, F_WINDOW_GROUPS, F_WINDOW_GROUPS_WITHIN,
    F_WINDOW_GROUPS_BY, F_STREAM_SUMMARY, F_STREAM_SUMMARY_FOR, F_STREAM_HISTOGRAM, F_STREAM_BINS, F_STREAM_GROUPS,
    F_STREAM_GROUPS_BY, F_STREAM_GROUPS_WITHIN};
// everything --ld cannot go with: what the site modes refuse, the window flags and the site modes themselves
const std::vector<Flag> kLdRefuses = after(F_WINDOWS, after(F_STEP, after(F_REGIONS, after(F_SITE_COUNTS, after(F_WINDOW_SITE_STATS,
                                           after(F_SITE_GROUPS, kSiteRefuses))))));
const Rule kRules[] = {
    // (before every other row: the band and the decay curve are modifiers of --ld; the curve has its own band, B x W - 1)
    {F_LD_BINS, Mode::Pairs, kNone, {F_LD_DECAY}, "'--ld-decay <W>'", TWO_OK, false},
    {F_LD_MAX_GAP, Mode::Pairs, {F_LD_DECAY}, {F_LD}, "'--ld <R2>'", TWO_OK, false},
    {F_LD_DECAY, Mode::Pairs, kNone, {F_LD}, "'--ld <R2>'", TWO_OK, false},
    // (before every other row: a command line with --ld or one of its two modifiers is judged here first, and no other
    // line's outcome changes)
    {F_LD_MIN_COUNT, Mode::Pairs, kNone, {F_LD}, "'--ld <R2>'", TWO_OK, false},
    {F_LD_GROUPS, Mode::Pairs, kNone, {F_LD}, "'--ld <R2>'", TWO_OK, false},
    {F_LD, Mode::Ld, kLdRefuses, kNone, nullptr, ONE_INPUT, true},
    // (before every other row: a command line with --site-counts, --window-site-stats or --site-groups is judged here first,
    // and no other line's outcome changes.  --window-site-stats leaves the mode to --windows / --regions.)
    {F_SITE_GROUPS, Mode::Pairs, kNone, {F_SITE_COUNTS, F_WINDOW_SITE_STATS}, "'--site-counts' or '--window-site-stats'", TWO_OK,
     false},
    {F_SITE_COUNTS, Mode::SiteCounts, after(F_WINDOW_SITE_STATS, after(F_WINDOWS, after(F_STEP, after(F_REGIONS, kSiteRefuses)))),
     kNone, nullptr, ONE_INPUT, true},
    {F_WINDOW_SITE_STATS, Mode::Pairs, kSiteRefuses, {F_WINDOWS, F_REGIONS}, "'--windows <W>' or '--regions <FILE>'", ONE_INPUT,
     true},
    // (before every other row: a command line with --stream-groups or one of its two modifiers is judged here first, and no
    // other line's outcome changes)
    {F_STREAM_GROUPS_BY, Mode::Pairs, kNone, {F_STREAM_GROUPS}, "'--stream-groups <FILE>'", TWO_OK, false},
    {F_STREAM_GROUPS_WITHIN, Mode::Pairs, kNone, {F_STREAM_GROUPS}, "'--stream-groups <FILE>'", TWO_OK, false},
    {F_STREAM_GROUPS, Mode::StreamGroups,
     after(F_STREAM_SUMMARY, after(F_STREAM_SUMMARY_FOR, after(F_STREAM_HISTOGRAM, after(F_STREAM_BINS, kStreamSummaryRefuses)))),
     {F_STREAM}, "'--stream <stream>'", ONE_LOADED, true},
    // (before every other row: a command line with --stream-summary, --stream-histogram or one of their modifiers is judged
    // here first, and no other line's outcome changes)
    {F_STREAM_SUMMARY_FOR, Mode::Pairs, kNone, {F_STREAM_SUMMARY}, "'--stream-summary <T>'", TWO_OK, false},
    {F_STREAM_BINS, Mode::Pairs, kNone, {F_STREAM_HISTOGRAM}, "'--stream-histogram <W>'", TWO_OK, false},
    {F_STREAM_SUMMARY, Mode::StreamSummary, after(F_STREAM_HISTOGRAM, after(F_STREAM_BINS, kStreamSummaryRefuses)), {F_STREAM},
     "'--stream <stream>'", ONE_LOADED, true},
    {F_STREAM_HISTOGRAM, Mode::StreamHistogram, after(F_STREAM_SUMMARY_FOR, kStreamSummaryRefuses), {F_STREAM},
     "'--stream <stream>'", ONE_LOADED, true},
    // (before every other row: a command line with --window-groups or one of its two modifiers is judged here first, and no
    // other line's outcome changes.  Like --window-summary it leaves the mode to --windows / --regions.)
    {F_WINDOW_GROUPS_WITHIN, Mode::Pairs, kNone, {F_WINDOW_GROUPS}, "'--window-groups <FILE>'", TWO_OK, false},
    {F_WINDOW_GROUPS_BY, Mode::Pairs, kNone, {F_WINDOW_GROUPS}, "'--window-groups <FILE>'", TWO_OK, false},
    {F_WINDOW_GROUPS, Mode::Pairs,
     after(F_WINDOW_NEAREST, after(F_WINDOW_CLOSEST, after(F_WINDOW_SUMMARY, after(F_PAIRS, kWindowRefuses)))),
     {F_WINDOWS, F_REGIONS}, "'--windows <W>' or '--regions <FILE>'", TWO_OK, true},
    // (before every other row: a command line with --window-summary or --window-summary-by is judged here first, and no
    // other line's outcome changes.  Like --window-nearest it leaves the mode to --windows / --regions.)
    {F_WINDOW_SUMMARY_BY, Mode::Pairs, kNone, {F_WINDOW_SUMMARY}, "'--window-summary <T>'", TWO_OK, false},
    {F_WINDOW_SUMMARY, Mode::Pairs, after(F_WINDOW_NEAREST, after(F_WINDOW_CLOSEST, after(F_PAIRS, kWindowRefuses))),
     {F_WINDOWS, F_REGIONS}, "'--windows <W>' or '--regions <FILE>'", TWO_OK, true},
    // (before every other row: a command line with --window-closest is judged here first, and no other line's outcome
    // changes.  It is the one flag that takes --windows / --regions into stream mode: check_rules lets those two rows pass
    // --stream, and keep their hands off the mode, when it is there.  Two rows: what it needs is two things.)
    {F_WINDOW_CLOSEST, Mode::Pairs,
     {F_WINDOW_NEAREST, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_REPRESENTATIVES, F_MAX_DISTANCE, F_SUMMARY,
      F_GROUPS, F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES,
      F_DENDROGRAM, F_PAIRS},
     {F_WINDOWS, F_REGIONS}, "'--windows <W>' or '--regions <FILE>'", ONE_LOADED, true},
    {F_WINDOW_CLOSEST, Mode::WindowClosest, kNone, {F_STREAM}, "'--stream <stream>'", ONE_LOADED, true},
    // (before every other row: a command line with --pairs is judged here first, and no other line's outcome changes; --sites
    // is the one modifier it takes)
    {F_PAIRS, Mode::PairList,
     {F_STREAM, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_REPRESENTATIVES, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS,
      F_GROUPS_WITHIN, F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_DENDROGRAM, F_WINDOWS,
      F_STEP, F_REGIONS, F_WINDOW_NEAREST}, kNone, nullptr, TWO_OK, true},
    // (before every other row: a command line with --window-nearest is judged here first, and no other line's outcome changes)
    {F_WINDOW_NEAREST, Mode::Pairs, kWindowRefuses, {F_WINDOWS, F_REGIONS}, "'--windows <W>' or '--regions <FILE>'", TWO_OK, true},
    // (before every older row: a command line with one of these three flags is judged here, and no other line's outcome
    // changes; --windows names --regions, the one mode flag the list does not hold)
    {F_STEP, Mode::Pairs, kNone, {F_WINDOWS}, "'--windows <W>'", TWO_OK, false},
    {F_WINDOWS, Mode::Windows, after(F_REGIONS, kWindowRefuses), kNone, nullptr, TWO_OK, true},
    {F_REGIONS, Mode::Windows, kWindowRefuses, kNone, nullptr, TWO_OK, true},
    // (first: every combination with it is refused here, so no other row's message changes)
    {F_REPRESENTATIVES, Mode::Representatives,
     {F_STREAM, F_NEAREST, F_CLOSEST, F_CLOSEST_FOR, F_WITHIN, F_CLUSTERS, F_MAX_DISTANCE, F_SUMMARY, F_GROUPS, F_GROUPS_WITHIN,
      F_PER_RECORD, F_HISTOGRAM, F_BINS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_SEED, F_MST, F_SITES, F_DENDROGRAM}, kNone, nullptr,
     ONE_INPUT, true},
    {F_CLOSEST_FOR, Mode::Pairs, kNone, {F_CLOSEST}, "'--closest <k>'", TWO_OK, false},
    {F_GROUPS_WITHIN, Mode::Pairs, kNone, {F_GROUPS}, "'--groups <FILE>'", TWO_OK, false},
    {F_PER_RECORD, Mode::Pairs, kNone, {F_GROUPS}, "'--groups <FILE>'", TWO_OK, false},
    {F_GROUPS, Mode::Groups,
     {F_STREAM, F_NEAREST, F_CLOSEST, F_WITHIN, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM, F_MAX_DISTANCE,
      F_SITES, F_HISTOGRAM, F_SUMMARY}, kNone, nullptr, TWO_OK, true},
    // (the message's first line is the recorded one of tests/cli_usage_outcomes.json; --pairs, the third pair-list
    // output, is named on a line of its own)
    {F_SITES, Mode::Pairs,
     {F_STREAM, F_NEAREST, F_CLOSEST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_DENDROGRAM, F_SUMMARY, F_HISTOGRAM},
     {F_MAX_DISTANCE, F_MST, F_PAIRS}, "'--max-distance <T>' or '--mst'\n       (or '--pairs <FILE>')", TWO_OK, false},
    {F_CLOSEST, Mode::Closest,
     {F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM, F_MAX_DISTANCE, F_HISTOGRAM, F_SUMMARY, F_WITHIN},
     {F_STREAM}, "'--stream <stream>'", ONE_LOADED, true},
    {F_WITHIN, Mode::Within,
     {F_CLOSEST, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM, F_MAX_DISTANCE, F_HISTOGRAM, F_SUMMARY},
     {F_STREAM}, "'--stream <stream>'", ONE_LOADED, true},
    {F_SUMMARY, Mode::Summary,
     {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM, F_MAX_DISTANCE, F_HISTOGRAM}, kNone,
     nullptr, TWO_OK, true},
    {F_HISTOGRAM, Mode::Histogram,
     {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM, F_MAX_DISTANCE}, kNone, nullptr, TWO_OK,
     true},
    {F_BINS, Mode::Pairs, kNone, {F_HISTOGRAM}, "'--histogram <W>'", TWO_OK, false},
    {F_MAX_DISTANCE, Mode::MaxDistance, {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MST, F_DENDROGRAM},
     kNone, nullptr, TWO_OK, true},
    // (--dendrogram with --bootstrap or --seed: their own rows below, which ask for '--tree nj')
    {F_DENDROGRAM, Mode::Dendrogram, {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_MST, F_MAX_DISTANCE}, kNone, nullptr,
     ONE_INPUT, true},
    {F_NEAREST, Mode::Nearest, {F_STREAM}, kNone, nullptr, TWO_OK, true},
    {F_CLUSTERS, Mode::Clusters, {F_STREAM, F_NEAREST}, kNone, nullptr, ONE_INPUT, true},
    {F_MATRIX, Mode::Matrix, {F_STREAM, F_NEAREST, F_CLUSTERS}, kNone, nullptr, ONE_FOR_PHYLIP, false},
    {F_TREE, Mode::Tree, {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX}, kNone, nullptr, ONE_INPUT, true},
    {F_MST, Mode::Mst, {F_STREAM, F_NEAREST, F_CLUSTERS, F_MATRIX, F_TREE, F_BOOTSTRAP, F_MAX_DISTANCE}, kNone, nullptr, ONE_INPUT,
     true},
    {F_BOOTSTRAP, Mode::Pairs, kNone, {F_TREE}, "'--tree nj'", TWO_OK, false},
    {F_SEED, Mode::Pairs, kNone, {F_BOOTSTRAP}, "'--bootstrap <B>'", TWO_OK, false},
};

void check_rules(Args &a)
{
    const bool many_gpus = a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1);
    for (const Rule &r : kRules) {
        if (!a.has[r.flag])
            continue;
        const std::string self = std::string("the argument '") + kFlags[r.flag].shown + "'";
        // (--windows / --regions in stream mode: with --window-closest, whose rows have spoken by now)
        const bool window_stream = a.has[F_WINDOW_CLOSEST] && (r.flag == F_WINDOWS || r.flag == F_REGIONS);
        for (const Flag other : r.refuses)
            if (a.has[other] && !(window_stream && other == F_STREAM))
                die_usage(self + " cannot be used with '" + kFlags[other].shown + "'");
        if (!r.needs.empty() && std::none_of(r.needs.begin(), r.needs.end(), [&](Flag f) { return a.has[f]; }))
            die_usage(self + " requires " + r.needs_shown);
        if (a.n_inputs() > 1 && r.two_inputs == ONE_FOR_PHYLIP && a.matrix == DST_MATRIX_PHYLIP)
            die_usage("the argument '--matrix phylip' takes one input alignment (a square matrix), not two");
        if (a.n_inputs() > 1 && (r.two_inputs == ONE_INPUT || r.two_inputs == ONE_LOADED))
            die_usage(self + " takes one " + (r.two_inputs == ONE_INPUT ? "input" : "loaded") + " alignment, not two");
        if (r.one_gpu && many_gpus)
            die_usage(self + " cannot be used with '" + kFlags[a.devices.size() > 1 ? F_DEVICES : F_GPUS].shown +
                      "' naming more than one GPU");
        if (r.mode != Mode::Pairs && !window_stream)
            a.mode = r.mode;   // the modes refuse each other: at most one row gets here
    }
}

Args parse_args(int argc, char **argv)
{
    Args a;
    int k = 1;
    std::string arg, v;
    // "--name value", "--name=value", "-n value", "-nvalue": true when `arg` is flag f, with its value in v
    auto opt = [&](Flag f) -> bool {
        const FlagDef &d = kFlags[f];
        const std::string name(d.shown, std::strcspn(d.shown, " "));
        const bool is_long = arg == name || arg.rfind(name + "=", 0) == 0;
        if (!is_long && !(d.letter && arg.rfind(d.letter, 0) == 0 && arg.rfind("--", 0) != 0))
            return false;
        const size_t eq = arg.find('=');
        if (is_long && eq != std::string::npos)
            v = arg.substr(eq + 1);
        else if (!is_long && arg.size() > 2)
            v = arg.substr(2);  // -mraw
        else if (k + 1 >= argc)
            die_usage(std::string("a value is required for '") + d.shown + "' but none was supplied");
        else
            v = argv[++k];
        if (d.once && a.has[f])
            die_usage(std::string("the argument '") + d.shown + "' cannot be used multiple times");
        a.has[f] = true;
        return true;
    };
    auto shown = [](Flag f) { return kFlags[f].shown; };
    auto text = [&](Flag f, std::string &into) { return opt(f) && (into = v, true); };
    auto count = [&](Flag f, size_t &into, size_t lo, size_t hi) {
        return opt(f) && (into = parse_in_range(v, shown(f), lo, hi), true);
    };
    auto threshold = [&](Flag f, double &into) { return opt(f) && (into = parse_threshold(v, shown(f)), true); };
    // a histogram's bin width, dst_summary's bounds: as a fixed-point value it is at least one unit (2^-37) and below 2^62
    auto bin_width = [&](Flag f) {
        const double w = parse_number(v, shown(f));
        if (!(w > 0) || !(w < 0x1p25) || std::rint(std::ldexp(w, DST_SUMMARY_SCALE_BITS)) < 1)
            die_value(v, shown(f), ": the bin width must be above 0 and below 2^25");
        return w;
    };
    bool only_pos = false;
    for (; k < argc; ++k) {
        arg = argv[k];
        if (only_pos || arg == "-" || arg.empty() || arg[0] != '-') {
            a.pos_inputs.push_back(arg);
        } else if (arg == "--") {
            only_pos = true;
        } else if (arg == "-h" || arg == "--help") {
            print_help();
            std::exit(0);
        } else if (arg == "-V" || arg == "--version") {
            std::printf("distance %s\n", kVersion);
            std::exit(0);
        } else if (arg == "-l" || arg == "--licenses") {
            a.licenses = true;
        } else if (arg == "--input" || arg.rfind("--input=", 0) == 0 || (arg.rfind("-i", 0) == 0 && arg.rfind("--", 0) != 0)) {
            // num_args(0..=2): takes following non-flag words, at most two
            const size_t eq = arg.find('=');
            if (arg.rfind("--", 0) == 0 && eq != std::string::npos)
                a.flag_inputs.push_back(arg.substr(eq + 1));
            else if (arg.rfind("--", 0) != 0 && arg.size() > 2)
                a.flag_inputs.push_back(arg.substr(2));
            while (a.flag_inputs.size() < 2 && k + 1 < argc && (argv[k + 1][0] != '-' || !std::strcmp(argv[k + 1], "-")))
                a.flag_inputs.push_back(argv[++k]);
        } else if (text(F_STREAM, a.stream) || text(F_MEASURE, a.measure) || text(F_OUTPUT, a.output) ||
                   text(F_GROUPS, a.groups) || text(F_WINDOW_GROUPS, a.window_groups) || text(F_STREAM_GROUPS, a.stream_groups) || text(F_SITE_GROUPS, a.site_groups) || text(F_LD_GROUPS, a.ld_groups) ||
                   count(F_LD_MIN_COUNT, a.ld_min_count, 1, 0xFFFFFFFFull) || text(F_REGIONS, a.regions) || text(F_PAIRS, a.pairs) || count(F_WINDOWS, a.windows, 1, SIZE_MAX) ||
                   count(F_STEP, a.step, 1, SIZE_MAX) || count(F_THREADS, a.threads, 0, SIZE_MAX) ||
                   count(F_BATCHSIZE, a.batchsize, 0, SIZE_MAX) || count(F_SEED, a.seed, 0, SIZE_MAX) ||
                   count(F_NEAREST, a.nearest, 1, 256) || count(F_CLOSEST, a.closest, 1, 256) ||
                   count(F_WINDOW_NEAREST, a.window_nearest, 1, 256) || count(F_WINDOW_CLOSEST, a.window_closest, 1, 256) ||
                   count(F_BINS, a.bins, 1, DST_SUMMARY_MAX_BINS) || count(F_BOOTSTRAP, a.bootstrap, 1, 10000) ||
                   threshold(F_CLUSTERS, a.clusters) || threshold(F_REPRESENTATIVES, a.representatives) || threshold(F_MAX_DISTANCE, a.max_distance) ||
                   threshold(F_WITHIN, a.within) || threshold(F_SUMMARY, a.summary) ||
                   threshold(F_GROUPS_WITHIN, a.groups_within) || threshold(F_WINDOW_GROUPS_WITHIN, a.window_groups_within) ||
                   threshold(F_WINDOW_SUMMARY, a.window_summary) || threshold(F_STREAM_SUMMARY, a.stream_summary) ||
                   threshold(F_STREAM_GROUPS_WITHIN, a.stream_groups_within) ||
                   count(F_STREAM_BINS, a.stream_bins, 1, DST_SUMMARY_MAX_BINS) || count(F_LD_MAX_GAP, a.ld_max_gap, 0, SIZE_MAX) ||
                   count(F_LD_DECAY, a.ld_decay, 1, 0xFFFFFFFFull) || count(F_LD_BINS, a.ld_bins, 1, DST_LD_DECAY_MAX_BINS)) {
            // a word, a count in a range or a threshold: stored
        } else if (opt(F_LD)) {
            a.ld = parse_number(v, shown(F_LD));
            if (!(a.ld >= 0 && a.ld <= 1))
                die_value(v, shown(F_LD), ": r^2 is a number from 0 to 1");
        } else if (opt(F_GPUS)) {
            a.gpus = (int)parse_usize(v, shown(F_GPUS));
        } else if (opt(F_DEVICES)) {
            for (size_t p = 0; p <= v.size();) {
                const size_t q = std::min(v.find(',', p), v.size());
                a.devices.push_back((int)parse_usize(v.substr(p, q - p), shown(F_DEVICES)));
                p = q + 1;
            }
        } else if (opt(F_SLAB_PAIRS)) {
            a.slab_pairs = std::max<size_t>(1, parse_usize(v, shown(F_SLAB_PAIRS)));
        } else if (opt(F_CLOSEST_FOR)) {
            a.closest_side = parse_choice(v, shown(F_CLOSEST_FOR), {{"loaded", DST_CLOSEST_FOR_LOADED},
                                          {"streamed", DST_CLOSEST_FOR_STREAMED}});
        } else if (opt(F_WINDOW_SUMMARY_BY)) {
            a.window_summary_by_record = parse_choice(v, shown(F_WINDOW_SUMMARY_BY), {{"window", 0}, {"record", 1}}) != 0;
        } else if (opt(F_WINDOW_GROUPS_BY)) {
            a.window_groups_by_record = parse_choice(v, shown(F_WINDOW_GROUPS_BY), {{"cell", 0}, {"record", 1}}) != 0;
        } else if (opt(F_HISTOGRAM)) {
            a.histogram = bin_width(F_HISTOGRAM);
        } else if (opt(F_STREAM_HISTOGRAM)) {
            a.stream_histogram = bin_width(F_STREAM_HISTOGRAM);
        } else if (opt(F_STREAM_GROUPS_BY)) {
            a.stream_groups_by = parse_choice(v, shown(F_STREAM_GROUPS_BY), {{"cell", 0}, {"streamed", 1}, {"loaded", 2}});
        } else if (opt(F_STREAM_SUMMARY_FOR)) {
            a.stream_summary_streamed = parse_choice(v, shown(F_STREAM_SUMMARY_FOR), {{"loaded", 0}, {"streamed", 1}}) != 0;
        } else if (opt(F_MATRIX)) {
            a.matrix = parse_choice(v, shown(F_MATRIX), {{"tsv", DST_MATRIX_TSV}, {"phylip", DST_MATRIX_PHYLIP}});
        } else if (opt(F_TREE)) {
            parse_choice(v, shown(F_TREE), {{"nj", 0}},
                         "\n  (UPGMA and the other rooted linkage trees: see '--dendrogram average')");
        } else if (opt(F_DENDROGRAM)) {
            a.dendrogram = parse_choice(v, shown(F_DENDROGRAM), {{"average", DST_LINK_AVERAGE}, {"weighted", DST_LINK_WEIGHTED},
                                        {"complete", DST_LINK_COMPLETE}});
        } else if (opt(F_SELFTEST)) {
            a.selftest = v;
        } else if (arg == "--per-record" || arg == "--mst" || arg == "--sites") {
            a.has[arg == "--per-record" ? F_PER_RECORD : arg == "--mst" ? F_MST : F_SITES] = true;
        } else if (arg == "--site-counts" || arg == "--window-site-stats") {
            const Flag f = arg == "--site-counts" ? F_SITE_COUNTS : F_WINDOW_SITE_STATS;
            if (a.has[f])
                die_usage(std::string("the argument '") + kFlags[f].shown + "' cannot be used multiple times");
            a.has[f] = true;
        } else {
            die_usage("unexpected argument '" + arg + "' found");
        }
    }
    if (a.pos_inputs.size() > 2)
        die_usage("unexpected argument '" + a.pos_inputs[2] + "' found");
    a.mode = a.has[F_STREAM] ? Mode::Stream : Mode::Pairs;
    check_rules(a);
    if (dst_measure_from_name(a.measure.c_str()) < 0)
        die_value(a.measure, shown(F_MEASURE), "\n  [possible values: n, n_high, raw, jc69, k80, tn93]");
    if (a.has[F_HISTOGRAM] && dst_measure_from_name(a.measure.c_str()) <= DST_N_HIGH && a.histogram != std::floor(a.histogram))
        die_usage("invalid value for '--histogram <W>': the bin width must be an integer with '--measure " + a.measure + "'");
    if (a.has[F_STREAM_HISTOGRAM] && dst_measure_from_name(a.measure.c_str()) <= DST_N_HIGH &&
        a.stream_histogram != std::floor(a.stream_histogram))
        die_usage("invalid value for '--stream-histogram <W>': the bin width must be an integer with '--measure " + a.measure + "'");
    return a;
}

}  // namespace
