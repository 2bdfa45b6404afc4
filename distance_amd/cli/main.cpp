// distance — drop-in CLI for benjamincjackson/distance on MI355X.
//
// Keeps the reference's surface (clap definition src/lib.rs:68-131, rules of set_up()
// src/lib.rs:162-267): -i/--input (0..2 files) or positional files, -s/--stream (file or "-"),
// -m/--measure {n,n_high,raw,jc69,k80,tn93} (default raw), -o/--output, -t/--threads,
// -b/--batchsize, -l/--licenses, -h, -V; TSV output identical to gather_write()
// (src/lib.rs:612-644).  The pair generators and worker pools (src/lib.rs:269-474, 502-596) are
// replaced by libdistance_hip.so through its C ABI; -t sizes the host formatting pool and -b is
// accepted — neither changes the output, as in the reference (src/lib.rs:919-1154).
// Extra flags: --gpus N (default 1) / --devices LIST, --slab-pairs P (result slab size), --closest K [--closest-for SIDE]
// (stream mode: the K closest records only, dst_stream_open_closest), --within T (stream mode: only the lines of the pairs
// within T, dst_stream_open_links), --nearest K (the K nearest records
// of every record instead of every pair: dst_nearest), --clusters T (single-linkage clusters at threshold T: dst_clusters),
// --matrix tsv|phylip (a square or rectangular distance matrix instead of the long form: dst_text_matrix), --tree nj (the
// neighbour-joining tree as one Newick line: dst_nj, dst_newick), --bootstrap B / --seed S (the tree's splits labelled
// with their support in B column resamplings: dst_nj_bootstrap, dst_newick_support), --mst (the edges of the minimum
// spanning tree in ascending order, one "id1, id2, value" line each: dst_mst), --dendrogram average|weighted|complete (the
// UPGMA / WPGMA / complete-linkage dendrogram as one Newick line with a binary root: dst_dendrogram, dst_newick_rooted),
// --max-distance T (the long output filtered on the GPU: only the lines of the pairs within T, in the full run's order:
// dst_links), --summary T (one line per record: how many records lie within T of it, how many it was compared with and its
// mean distance to them: dst_summary), --histogram W / --bins B (the histogram of the pairwise distances in B bins of width
// W, one "lower edge, pairs" line per bin and a last line for the pairs without a distance: dst_summary), --groups FILE /
// --groups-within T / --per-record (one line per pair of groups of a label file, or per record and group: the pairs, the
// compared pairs, their mean, smallest and largest distance: dst_group_summary), --sites (with
// --max-distance or --mst: a fourth field per line, the sites that separate the two records: dst_pair_sites).
//
// Exactness: the GPU returns integer site tallies; f64 finalisation is dst_finalize() on the host
// (reference operation order, glibc log/sqrt), so the printed digits do not depend on the device.
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <csignal>
#include <cstdio>
#include <sys/stat.h>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <unistd.h>

#include "../../include/distance_hip.h"
#include "fasta.hpp"
#include "format.hpp"

namespace {

const char *kVersion = "0.3.1";  // Cargo.toml:3 of the reference this CLI mirrors

// ---------------------------------------------------------------- errors ----------------------
// main() of the reference returns Result<(), DistanceError>: Rust prints `Error: {:?}` and exits 1.
// Fatal errors can surface on a reader / worker thread while GPU threads are still running: flush
// what was written (the reference's BufWriter content is flushed on its way out too) and leave
// without running static destructors under those threads.
[[noreturn]] void leave(int code)
{
    std::fflush(nullptr);
    _exit(code);
}

[[noreturn]] void die_message(const std::string &m)
{
    std::fprintf(stderr, "Error: Message(\"%s\")\n", m.c_str());
    leave(1);
}

[[noreturn]] void die_io(const std::string &what, int err)
{
    std::fprintf(stderr, "Error: IOError(Os { code: %d, kind: %s, message: \"%s\" }) [%s]\n", err,
                 err == ENOENT ? "NotFound" : err == EACCES ? "PermissionDenied" : "Other", std::strerror(err),
                 what.c_str());
    leave(1);
}

[[noreturn]] void die_usage(const std::string &m)
{
    std::fprintf(stderr, "error: %s\n\nFor more information, try '--help'.\n", m.c_str());
    std::exit(2);  // clap's usage-error exit code
}

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
        "      --clusters <T>           Print the single-linkage cluster of every record instead of distances: records "
        "within distance T (a number >= 0) of each other share a cluster, numbered from 1 in order of first record. One "
        "input, one GPU, no --stream or --nearest\n"
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
        "      --sites                  With one of the two pair-list outputs (the pairs within a distance, the minimum spanning "
        "tree): a fourth field per line, the sites that separate the two "
        "records as a comma-separated list of X<pos>Y (pos 1-based, X the first record's IUPAC letter, Y the second's; '.' "
        "when there are none): the sites the measure counts as differences\n"
        "      --dendrogram <linkage>   Print the rooted hierarchical-clustering tree of the records as one Newick line instead "
        "of distances: linkage average (UPGMA), weighted (WPGMA) or complete. One input, one GPU, no --stream and no other "
        "output mode\n"
        "  -h, --help                   Print help\n"
        "  -V, --version                Print version");
}

// ---------------------------------------------------------------- arguments -------------------
struct Args {
    std::vector<std::string> flag_inputs, pos_inputs;
    bool has_stream = false;
    std::string stream, measure = "raw", output;
    bool has_output = false, has_threads = false, licenses = false;
    size_t threads = 0, batchsize = 1;
    int gpus = 1;
    std::vector<int> devices;  // explicit device ordinals (--devices 0,1,..); empty: 0..gpus-1
    size_t slab_pairs = (size_t)1 << 22;  // result slab: 4 Mi pairs pipelines GPU, formatters and writer well
    size_t nearest = 0;                   // --nearest k (0: every pair)
    bool has_nearest = false;
    size_t closest = 0;                   // --closest k (stream mode)
    bool has_closest = false, has_closest_for = false;
    int closest_side = DST_CLOSEST_FOR_LOADED;   // --closest-for loaded|streamed
    double within = 0;                    // --within T (stream mode)
    bool has_within = false;
    double clusters = 0;                  // --clusters T
    bool has_clusters = false;
    double max_distance = 0;              // --max-distance T
    bool has_max_distance = false;
    double summary = 0;                   // --summary T
    bool has_summary = false;
    double histogram = 0;                 // --histogram W
    bool has_histogram = false;
    std::string groups;                   // --groups FILE
    bool has_groups = false;
    double groups_within = 0;             // --groups-within T
    bool has_groups_within = false;
    bool per_record = false;              // --per-record
    size_t bins = 256;                    // --bins B
    bool has_bins = false;
    int matrix = -1;                      // --matrix: DST_MATRIX_TSV / DST_MATRIX_PHYLIP (-1: the long form)
    bool has_tree = false;                // --tree nj
    uint32_t bootstrap = 0;               // --bootstrap B (0: none)
    bool has_bootstrap = false;
    uint64_t seed = 1;                    // --seed S
    bool has_seed = false;
    bool has_slab_pairs = false;
    bool has_mst = false;                 // --mst
    bool has_sites = false;               // --sites (a modifier of --max-distance and --mst)
    int dendrogram = -1;                  // --dendrogram: DST_LINK_* (-1: none)
    std::string selftest;
};

size_t parse_usize(const std::string &v, const char *flag)
{
    if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos)
        die_usage("invalid value '" + v + "' for '" + flag + "': invalid digit found in string");
    errno = 0;
    unsigned long long x = std::strtoull(v.c_str(), nullptr, 10);
    if (errno)
        die_usage("invalid value '" + v + "' for '" + flag + "': number too large to fit in target type");
    return (size_t)x;
}

Args parse_args(int argc, char **argv)
{
    Args a;
    auto value_of = [&](int &k, const std::string &arg, const char *flag) -> std::string {
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos)
            return arg.substr(eq + 1);
        if (arg.rfind("--", 0) != 0 && arg.size() > 2)
            return arg.substr(2);  // -mraw
        if (k + 1 >= argc)
            die_usage(std::string("a value is required for '") + flag + "' but none was supplied");
        return argv[++k];
    };
    auto is = [](const std::string &arg, const char *s, const char *l) {
        if (arg == l || arg.rfind(std::string(l) + "=", 0) == 0)
            return true;
        return arg.rfind(s, 0) == 0 && arg.rfind("--", 0) != 0;
    };
    bool only_pos = false;
    for (int k = 1; k < argc; ++k) {
        const std::string arg = argv[k];
        if (only_pos || arg == "-" || arg.empty() || arg[0] != '-') {
            a.pos_inputs.push_back(arg);
            continue;
        }
        if (arg == "--") {
            only_pos = true;
        } else if (arg == "-h" || arg == "--help") {
            print_help();
            std::exit(0);
        } else if (arg == "-V" || arg == "--version") {
            std::printf("distance %s\n", kVersion);
            std::exit(0);
        } else if (arg == "-l" || arg == "--licenses") {
            a.licenses = true;
        } else if (is(arg, "-i", "--input")) {
            // num_args(0..=2): takes following non-flag words, at most two
            const size_t eq = arg.find('=');
            if (arg.rfind("--", 0) == 0 && eq != std::string::npos)
                a.flag_inputs.push_back(arg.substr(eq + 1));
            else if (arg.rfind("--", 0) != 0 && arg.size() > 2)
                a.flag_inputs.push_back(arg.substr(2));
            while (a.flag_inputs.size() < 2 && k + 1 < argc && (argv[k + 1][0] != '-' || !std::strcmp(argv[k + 1], "-")))
                a.flag_inputs.push_back(argv[++k]);
        } else if (is(arg, "-s", "--stream")) {
            a.stream = value_of(k, arg, "--stream <stream>");
            a.has_stream = true;
        } else if (is(arg, "-m", "--measure")) {
            a.measure = value_of(k, arg, "--measure <measure>");
        } else if (is(arg, "-o", "--output")) {
            a.output = value_of(k, arg, "--output <output>");
            a.has_output = true;
        } else if (is(arg, "-t", "--threads")) {
            a.threads = parse_usize(value_of(k, arg, "--threads <threads>"), "--threads <threads>");
            a.has_threads = true;
        } else if (is(arg, "-b", "--batchsize")) {
            a.batchsize = parse_usize(value_of(k, arg, "--batchsize <batchsize>"), "--batchsize <batchsize>");
        } else if (arg == "--gpus" || arg.rfind("--gpus=", 0) == 0) {
            a.gpus = (int)parse_usize(value_of(k, arg, "--gpus <n>"), "--gpus <n>");
        } else if (arg == "--devices" || arg.rfind("--devices=", 0) == 0) {
            std::string v = value_of(k, arg, "--devices <list>");
            for (size_t p = 0; p <= v.size();) {
                const size_t q = std::min(v.find(',', p), v.size());
                a.devices.push_back((int)parse_usize(v.substr(p, q - p), "--devices <list>"));
                p = q + 1;
            }
        } else if (arg == "--slab-pairs" || arg.rfind("--slab-pairs=", 0) == 0) {
            a.slab_pairs = std::max<size_t>(1, parse_usize(value_of(k, arg, "--slab-pairs <p>"), "--slab-pairs <p>"));
            a.has_slab_pairs = true;
        } else if (arg == "--nearest" || arg.rfind("--nearest=", 0) == 0) {
            const std::string v = value_of(k, arg, "--nearest <k>");
            a.nearest = parse_usize(v, "--nearest <k>");
            if (a.nearest < 1 || a.nearest > 256)
                die_usage("invalid value '" + v + "' for '--nearest <k>': " + v + " is not in 1..=256");
            a.has_nearest = true;
        } else if (arg == "--closest" || arg.rfind("--closest=", 0) == 0) {
            const std::string v = value_of(k, arg, "--closest <k>");
            a.closest = parse_usize(v, "--closest <k>");
            if (a.closest < 1 || a.closest > 256)
                die_usage("invalid value '" + v + "' for '--closest <k>': " + v + " is not in 1..=256");
            a.has_closest = true;
        } else if (arg == "--closest-for" || arg.rfind("--closest-for=", 0) == 0) {
            const std::string v = value_of(k, arg, "--closest-for <side>");
            if (v == "loaded")
                a.closest_side = DST_CLOSEST_FOR_LOADED;
            else if (v == "streamed")
                a.closest_side = DST_CLOSEST_FOR_STREAMED;
            else
                die_usage("invalid value '" + v + "' for '--closest-for <side>'\n  [possible values: loaded, streamed]");
            a.has_closest_for = true;
        } else if (arg == "--clusters" || arg.rfind("--clusters=", 0) == 0) {
            const std::string v = value_of(k, arg, "--clusters <T>");
            // the whole word is the number: strtod, nothing left over, not NaN, not negative
            char *end = nullptr;
            errno = 0;
            const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--clusters <T>': not a number");
            if (t < 0)
                die_usage("invalid value '" + v + "' for '--clusters <T>': the threshold must not be negative");
            a.clusters = t;
            a.has_clusters = true;
        } else if (arg == "--max-distance" || arg.rfind("--max-distance=", 0) == 0) {
            const std::string v = value_of(k, arg, "--max-distance <T>");
            if (a.has_max_distance)
                die_usage("the argument '--max-distance <T>' cannot be used multiple times");
            // the whole word is the number (or inf), as for --clusters <T>
            char *end = nullptr;
            errno = 0;
            const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--max-distance <T>': not a number");
            if (t < 0)
                die_usage("invalid value '" + v + "' for '--max-distance <T>': the threshold must not be negative");
            a.max_distance = t;
            a.has_max_distance = true;
        } else if (arg == "--within" || arg.rfind("--within=", 0) == 0) {
            const std::string v = value_of(k, arg, "--within <T>");
            if (a.has_within)
                die_usage("the argument '--within <T>' cannot be used multiple times");
            // the whole word is the number (or inf), as for --max-distance <T>
            char *end = nullptr;
            errno = 0;
            const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--within <T>': not a number");
            if (t < 0)
                die_usage("invalid value '" + v + "' for '--within <T>': the threshold must not be negative");
            a.within = t;
            a.has_within = true;
        } else if (arg == "--summary" || arg.rfind("--summary=", 0) == 0) {
            const std::string v = value_of(k, arg, "--summary <T>");
            if (a.has_summary)
                die_usage("the argument '--summary <T>' cannot be used multiple times");
            // the whole word is the number (or inf), as for --clusters <T>
            char *end = nullptr;
            errno = 0;
            const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--summary <T>': not a number");
            if (t < 0)
                die_usage("invalid value '" + v + "' for '--summary <T>': the threshold must not be negative");
            a.summary = t;
            a.has_summary = true;
        } else if (arg == "--groups" || arg.rfind("--groups=", 0) == 0) {
            const std::string v = value_of(k, arg, "--groups <FILE>");
            if (a.has_groups)
                die_usage("the argument '--groups <FILE>' cannot be used multiple times");
            a.groups = v;
            a.has_groups = true;
        } else if (arg == "--groups-within" || arg.rfind("--groups-within=", 0) == 0) {
            const std::string v = value_of(k, arg, "--groups-within <T>");
            if (a.has_groups_within)
                die_usage("the argument '--groups-within <T>' cannot be used multiple times");
            // the whole word is the number (or inf), as for --summary <T>
            char *end = nullptr;
            errno = 0;
            const double t = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || t != t || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--groups-within <T>': not a number");
            if (t < 0)
                die_usage("invalid value '" + v + "' for '--groups-within <T>': the threshold must not be negative");
            a.groups_within = t;
            a.has_groups_within = true;
        } else if (arg == "--per-record") {
            a.per_record = true;
        } else if (arg == "--histogram" || arg.rfind("--histogram=", 0) == 0) {
            const std::string v = value_of(k, arg, "--histogram <W>");
            if (a.has_histogram)
                die_usage("the argument '--histogram <W>' cannot be used multiple times");
            char *end = nullptr;
            errno = 0;
            const double w = v.empty() ? 0.0 : std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || w != w || std::isspace((unsigned char)v[0]))
                die_usage("invalid value '" + v + "' for '--histogram <W>': not a number");
            // dst_summary's bounds: the width as a fixed-point value is at least one unit (2^-37) and below 2^62
            if (!(w > 0) || !(w < 0x1p25) || std::rint(std::ldexp(w, DST_SUMMARY_SCALE_BITS)) < 1)
                die_usage("invalid value '" + v + "' for '--histogram <W>': the bin width must be above 0 and below 2^25");
            a.histogram = w;
            a.has_histogram = true;
        } else if (arg == "--bins" || arg.rfind("--bins=", 0) == 0) {
            const std::string v = value_of(k, arg, "--bins <B>");
            a.bins = parse_usize(v, "--bins <B>");
            if (a.bins < 1 || a.bins > DST_SUMMARY_MAX_BINS)
                die_usage("invalid value '" + v + "' for '--bins <B>': " + v + " is not in 1..=4096");
            a.has_bins = true;
        } else if (arg == "--matrix" || arg.rfind("--matrix=", 0) == 0) {
            const std::string v = value_of(k, arg, "--matrix <format>");
            if (v == "tsv")
                a.matrix = DST_MATRIX_TSV;
            else if (v == "phylip")
                a.matrix = DST_MATRIX_PHYLIP;
            else
                die_usage("invalid value '" + v + "' for '--matrix <format>'\n  [possible values: tsv, phylip]");
        } else if (arg == "--tree" || arg.rfind("--tree=", 0) == 0) {
            const std::string v = value_of(k, arg, "--tree <method>");
            if (v != "nj")
                die_usage("invalid value '" + v + "' for '--tree <method>'\n  [possible values: nj]\n  (UPGMA and the other "
                          "rooted linkage trees: see '--dendrogram average')");
            a.has_tree = true;
        } else if (arg == "--bootstrap" || arg.rfind("--bootstrap=", 0) == 0) {
            const std::string v = value_of(k, arg, "--bootstrap <B>");
            const size_t b = parse_usize(v, "--bootstrap <B>");
            if (b < 1 || b > 10000)
                die_usage("invalid value '" + v + "' for '--bootstrap <B>': " + v + " is not in 1..=10000");
            a.bootstrap = (uint32_t)b;
            a.has_bootstrap = true;
        } else if (arg == "--seed" || arg.rfind("--seed=", 0) == 0) {
            a.seed = parse_usize(value_of(k, arg, "--seed <S>"), "--seed <S>");
            a.has_seed = true;
        } else if (arg == "--mst") {
            a.has_mst = true;
        } else if (arg == "--sites") {
            a.has_sites = true;
        } else if (arg == "--dendrogram" || arg.rfind("--dendrogram=", 0) == 0) {
            const std::string v = value_of(k, arg, "--dendrogram <linkage>");
            if (v == "average")
                a.dendrogram = DST_LINK_AVERAGE;
            else if (v == "weighted")
                a.dendrogram = DST_LINK_WEIGHTED;
            else if (v == "complete")
                a.dendrogram = DST_LINK_COMPLETE;
            else
                die_usage("invalid value '" + v + "' for '--dendrogram <linkage>'\n  [possible values: average, weighted, "
                          "complete]");
        } else if (arg == "--host-selftest") {
            a.selftest = value_of(k, arg, "--host-selftest <what>");
        } else {
            die_usage("unexpected argument '" + arg + "' found");
        }
    }
    if (a.pos_inputs.size() > 2)
        die_usage("unexpected argument '" + a.pos_inputs[2] + "' found");
    if (a.has_closest_for && !a.has_closest)
        die_usage("the argument '--closest-for <side>' requires '--closest <k>'");
    if (a.has_groups_within && !a.has_groups)
        die_usage("the argument '--groups-within <T>' requires '--groups <FILE>'");
    if (a.per_record && !a.has_groups)
        die_usage("the argument '--per-record' requires '--groups <FILE>'");
    if (a.has_groups) {   // against every other output mode, before their own checks
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_closest ? "--closest <k>"
                            : a.has_within ? "--within <T>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_mst ? "--mst"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : a.has_max_distance ? "--max-distance <T>"
                            : a.has_sites ? "--sites" : a.has_histogram ? "--histogram <W>" : a.has_summary ? "--summary <T>"
                            : nullptr;
        if (other)
            die_usage(std::string("the argument '--groups <FILE>' cannot be used with '") + other + "'");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--groups <FILE>' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.has_sites) {   // a modifier of the two pair-list outputs: no other output mode, and one of the two
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_closest ? "--closest <k>"
                            : a.has_clusters ? "--clusters <T>" : a.matrix >= 0 ? "--matrix <format>"
                            : a.has_tree ? "--tree <method>" : a.has_bootstrap ? "--bootstrap <B>"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : a.has_summary ? "--summary <T>"
                            : a.has_histogram ? "--histogram <W>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--sites' cannot be used with '") + other + "'");
        if (!a.has_max_distance && !a.has_mst)
            die_usage("the argument '--sites' requires '--max-distance <T>' or '--mst'");
    }
    if (a.has_closest) {   // against every other output mode, before their own checks (which name --stream)
        const char *other = a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_mst ? "--mst"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : a.has_max_distance ? "--max-distance <T>"
                            : a.has_histogram ? "--histogram <W>" : a.has_summary ? "--summary <T>"
                            : a.has_within ? "--within <T>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--closest <k>' cannot be used with '") + other + "'");
        if (!a.has_stream)
            die_usage("the argument '--closest <k>' requires '--stream <stream>'");
        if (a.flag_inputs.size() + a.pos_inputs.size() > 1)
            die_usage("the argument '--closest <k>' takes one loaded alignment, not two");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--closest <k>' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.has_within) {   // stream mode's --max-distance: like --closest against every other output mode, before their own checks
        const char *other = a.has_closest ? "--closest <k>" : a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_mst ? "--mst"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : a.has_max_distance ? "--max-distance <T>"
                            : a.has_histogram ? "--histogram <W>" : a.has_summary ? "--summary <T>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--within <T>' cannot be used with '") + other + "'");
        if (!a.has_stream)
            die_usage("the argument '--within <T>' requires '--stream <stream>'");
        if (a.flag_inputs.size() + a.pos_inputs.size() > 1)
            die_usage("the argument '--within <T>' takes one loaded alignment, not two");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--within <T>' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    for (int mode = 0; mode < 2; ++mode) {   // --summary, then --histogram: each against everything else
        if (!(mode == 0 ? a.has_summary : a.has_histogram))
            continue;
        const std::string self = mode == 0 ? "--summary <T>" : "--histogram <W>";
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_mst ? "--mst"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : a.has_max_distance ? "--max-distance <T>"
                            : mode == 0 && a.has_histogram ? "--histogram <W>" : nullptr;
        if (other)
            die_usage("the argument '" + self + "' cannot be used with '" + other + "'");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage("the argument '" + self + "' cannot be used with '" +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.has_bins && !a.has_histogram)
        die_usage("the argument '--bins <B>' requires '--histogram <W>'");
    if (a.has_max_distance) {
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_mst ? "--mst"
                            : a.dendrogram >= 0 ? "--dendrogram <linkage>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--max-distance <T>' cannot be used with '") + other + "'");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--max-distance <T>' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.dendrogram >= 0) {
        // (--bootstrap and --seed: the checks below, which ask for '--tree nj')
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>" : a.has_mst ? "--mst"
                            : a.has_max_distance ? "--max-distance <T>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--dendrogram <linkage>' cannot be used with '") + other + "'");
        if (a.flag_inputs.size() + a.pos_inputs.size() > 1)
            die_usage("the argument '--dendrogram <linkage>' takes one input alignment, not two");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--dendrogram <linkage>' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.has_nearest && a.has_stream)
        die_usage("the argument '--nearest <k>' cannot be used with '--stream <stream>'");
    if (a.has_nearest && (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1)))
        die_usage(std::string("the argument '--nearest <k>' cannot be used with '") +
                  (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    if (a.has_clusters && a.has_stream)
        die_usage("the argument '--clusters <T>' cannot be used with '--stream <stream>'");
    if (a.has_clusters && a.has_nearest)
        die_usage("the argument '--clusters <T>' cannot be used with '--nearest <k>'");
    if (a.has_clusters && a.flag_inputs.size() + a.pos_inputs.size() > 1)
        die_usage("the argument '--clusters <T>' takes one input alignment, not two");
    if (a.has_clusters && (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1)))
        die_usage(std::string("the argument '--clusters <T>' cannot be used with '") +
                  (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    if (a.matrix >= 0 && a.has_stream)
        die_usage("the argument '--matrix <format>' cannot be used with '--stream <stream>'");
    if (a.matrix >= 0 && a.has_nearest)
        die_usage("the argument '--matrix <format>' cannot be used with '--nearest <k>'");
    if (a.matrix >= 0 && a.has_clusters)
        die_usage("the argument '--matrix <format>' cannot be used with '--clusters <T>'");
    if (a.matrix == DST_MATRIX_PHYLIP && a.flag_inputs.size() + a.pos_inputs.size() > 1)
        die_usage("the argument '--matrix phylip' takes one input alignment (a square matrix), not two");
    if (a.has_tree && a.has_stream)
        die_usage("the argument '--tree <method>' cannot be used with '--stream <stream>'");
    if (a.has_tree && a.has_nearest)
        die_usage("the argument '--tree <method>' cannot be used with '--nearest <k>'");
    if (a.has_tree && a.has_clusters)
        die_usage("the argument '--tree <method>' cannot be used with '--clusters <T>'");
    if (a.has_tree && a.matrix >= 0)
        die_usage("the argument '--tree <method>' cannot be used with '--matrix <format>'");
    if (a.has_tree && a.flag_inputs.size() + a.pos_inputs.size() > 1)
        die_usage("the argument '--tree <method>' takes one input alignment, not two");
    if (a.has_tree && (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1)))
        die_usage(std::string("the argument '--tree <method>' cannot be used with '") +
                  (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    if (a.has_mst) {
        const char *other = a.has_stream ? "--stream <stream>" : a.has_nearest ? "--nearest <k>" : a.has_clusters ? "--clusters <T>"
                            : a.matrix >= 0 ? "--matrix <format>" : a.has_tree ? "--tree <method>"
                            : a.has_bootstrap ? "--bootstrap <B>" : a.has_max_distance ? "--max-distance <T>" : nullptr;
        if (other)
            die_usage(std::string("the argument '--mst' cannot be used with '") + other + "'");
        if (a.flag_inputs.size() + a.pos_inputs.size() > 1)
            die_usage("the argument '--mst' takes one input alignment, not two");
        if (a.devices.size() > 1 || (a.devices.empty() && a.gpus > 1))
            die_usage(std::string("the argument '--mst' cannot be used with '") +
                      (a.devices.size() > 1 ? "--devices <list>" : "--gpus <n>") + "' naming more than one GPU");
    }
    if (a.has_bootstrap && !a.has_tree)
        die_usage("the argument '--bootstrap <B>' requires '--tree nj'");
    if (a.has_seed && !a.has_bootstrap)
        die_usage("the argument '--seed <S>' requires '--bootstrap <B>'");
    if (dst_measure_from_name(a.measure.c_str()) < 0)
        die_usage("invalid value '" + a.measure + "' for '--measure <measure>'\n  [possible values: n, n_high, raw, "
                  "jc69, k80, tn93]");
    if (a.has_histogram && dst_measure_from_name(a.measure.c_str()) <= DST_N_HIGH && a.histogram != std::floor(a.histogram))
        die_usage("invalid value for '--histogram <W>': the bin width must be an integer with '--measure " + a.measure + "'");
    return a;
}

const char *kLicences =
    "\nCopyright 2022, Ben Jackson (distance, GNU LIBRARY GENERAL PUBLIC LICENSE, Version 2): this program is an\n"
    "independent MI355X re-implementation of its command-line surface and output format.\n"
    "FASTA tokenisation follows Rust-Bio (MIT licence, Copyright (c) 2016 Johannes Koester, the Rust-Bio team,\n"
    "Google Inc.).  Nucleotide coding scheme: Emmanuel Paradis, as used in ape.\n";

// ---------------------------------------------------------------- loading ---------------------
// src/encoding.rs:4-41
void encoding_array(uint8_t a[256])
{
    std::memset(a, 0, 256);
    const char *letters = "AGCTRMWSKYVHDBN";
    const uint8_t codes[] = {136, 72, 40, 24, 192, 160, 144, 96, 80, 48, 224, 176, 208, 112, 240};
    for (int k = 0; letters[k]; ++k) {
        a[(unsigned char)letters[k]] = codes[k];
        a[(unsigned char)(letters[k] - 'A' + 'a')] = codes[k];
    }
    a[(unsigned char)'-'] = 244;
    a[(unsigned char)'?'] = 242;
}

// std::vector that leaves new bytes uninitialised (resize() before a fill would touch every page twice)
template <class T>
struct NoInit : std::allocator<T> {
    template <class U> struct rebind { using other = NoInit<U>; };
    NoInit() = default;
    template <class U> NoInit(const NoInit<U> &) {}
    template <class U> void construct(U *p) noexcept { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&...a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};
using Bytes = std::vector<uint8_t, NoInit<uint8_t>>;

struct Alignment {
    std::vector<std::string> ids;
    Bytes codes;                     // n x width, row-major
    std::vector<uint32_t> counts;    // n x 4 {A,T,G,C}: only filled for streamed tn93 batches
    size_t n = 0, width = 0;
};

std::string err_invalid_nuc(const std::string &id, unsigned char c)  // src/fastaio.rs:89-91
{
    std::string s = "Invalid nucleotide character in record '" + id + "': '";
    s.push_back((char)c);
    return s + "'";
}

std::string err_lengths(size_t w1, size_t w2)  // src/fastaio.rs:93-95
{
    return "Different length sequences in alignment(s): " + std::to_string(w1) + " vs " + std::to_string(w2);
}

FILE *open_input(const std::string &path)
{
    FILE *fh = std::fopen(path.c_str(), "rb");
    if (!fh)
        die_io(path, errno);
    return fh;
}

// One block of whole records -> encoded records.  Errors are returned, not raised, so that the
// consumer reports the FIRST one in file order, like the reference's sequential reader.
struct ParsedBlock {
    std::unique_ptr<Alignment> al;
    std::string error;  // empty: ok
    bool stop = false;  // an empty record ended bio's Records iterator: nothing after it is read
};

ParsedBlock parse_block(const cli::Block &block, const uint8_t *table, bool count_raw_upper, bool fixed_width,
                        size_t width, bool width_first)
{
    // In place on the block's bytes, with fasta.hpp's tokenisation (FastaReader is the readable statement of it and
    // the sequential reader the host tests compare this with): a record starts at a line beginning with '>';
    // id = header up to the first whitespace, the rest (trailing whitespace trimmed) is the description; every
    // following line up to the next '>' line is sequence, trailing whitespace trimmed.  No per-line copies: the
    // lines are encoded straight from the block into the codes.
    ParsedBlock out;
    out.al = std::make_unique<Alignment>();
    Alignment &al = *out.al;
    al.width = width;
    al.codes.reserve(block.len);   // an upper bound: a code per sequence byte
    const char *data = block.bytes();
    const size_t len = block.len;
    auto is_space = [](unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); };
    bool first = !fixed_width;
    std::vector<std::pair<const char *, size_t>> parts;
    std::string id;
    size_t pos = 0;
    while (pos < len) {
        // header line
        const char *h = data + pos;
        const char *nl = (const char *)std::memchr(h, '\n', len - pos);
        size_t hlen = nl ? (size_t)(nl - h) + 1 : len - pos;
        if (h[0] != '>') {
            out.error = "Expected > at record start.";
            return out;
        }
        pos += hlen;
        size_t end = hlen;
        while (end > 1 && is_space((unsigned char)h[end - 1]))
            --end;
        size_t p = 1;
        while (p < end && !is_space((unsigned char)h[p]))
            ++p;
        id.assign(h + 1, p - 1);
        const bool has_desc = p < end;
        // sequence lines
        parts.clear();
        size_t total = 0;
        while (pos < len && data[pos] != '>') {
            const char *l = data + pos;
            const char *e = (const char *)std::memchr(l, '\n', len - pos);
            const size_t llen = e ? (size_t)(e - l) + 1 : len - pos;
            pos += llen;
            size_t keep = llen;
            while (keep > 0 && is_space((unsigned char)l[keep - 1]))
                --keep;
            if (keep) {
                parts.emplace_back(l, keep);
                total += keep;
            }
        }
        if (id.empty() && !has_desc && total == 0) {
            out.stop = true;  // bio's Records iterator stops at an empty record
            break;
        }
        // stream_fasta() compares widths BEFORE encoding (src/fastaio.rs:246-254); load_fasta() encodes first
        // (src/fastaio.rs:182) and compares afterwards (:186-190), so a loaded record that is both the wrong
        // length and holds an invalid character reports the character.
        if (width_first && total != al.width) {
            out.error = err_lengths(total, al.width);  // src/fastaio.rs:93-95, 246-248
            return out;
        }
        // encode() / encode_count_bases(): src/fastaio.rs:101-145
        const size_t at = al.codes.size();
        al.codes.resize(at + total);
        uint8_t *dst = al.codes.data() + at;
        uint32_t counting[256];
        if (count_raw_upper)
            std::memset(counting, 0, sizeof counting);
        for (const auto &part : parts) {
            const unsigned char *src = (const unsigned char *)part.first;
            const size_t n = part.second;
            uint8_t bad = 0xFF;   // AND of the codes: 0 as soon as one byte has none (every code has bit 7, 6, 5 or 4)
            for (size_t i = 0; i < n; ++i) {
                const uint8_t code = table[src[i]];
                dst[i] = code;
                bad = code ? bad : 0;
            }
            if (!bad) {
                for (size_t i = 0; i < n; ++i)
                    if (table[src[i]] == 0) {
                        out.error = err_invalid_nuc(id, src[i]);
                        return out;
                    }
            }
            if (count_raw_upper)
                for (size_t i = 0; i < n; ++i)
                    counting[src[i]] += 1;
            dst += n;
        }
        if (count_raw_upper) {
            al.counts.push_back(counting['A']);
            al.counts.push_back(counting['T']);
            al.counts.push_back(counting['G']);
            al.counts.push_back(counting['C']);
        }
        if (!width_first) {
            if (first) {
                al.width = total;
                first = false;
            } else if (total != al.width) {
                out.error = err_lengths(total, al.width);  // src/fastaio.rs:93-95, 186-190
                return out;
            }
        }
        al.ids.push_back(id);
        al.n += 1;
    }
    return out;
}

// Reads `fh` block by block and parses up to `lookahead` blocks concurrently; `consume` gets the
// parsed blocks strictly in file order (and is where errors surface).
template <class Consume>
void parse_stream(FILE *fh, size_t block_bytes, size_t lookahead, const uint8_t *table, bool count_raw_upper,
                  bool fixed_width, size_t width, Consume consume)
{
    cli::BlockReader blocks(fh, block_bytes);
    std::deque<std::future<ParsedBlock>> inflight;
    cli::Block block;
    bool more = true, width_known = fixed_width;
    size_t w = width;
    while (more || !inflight.empty()) {
        // the first block runs alone when the width is not known yet (it fixes it for the others)
        while (more && inflight.size() < (width_known ? std::max<size_t>(lookahead, 1) : 1)) {
            if (!blocks.next(block)) {
                more = false;
                break;
            }
            inflight.push_back(std::async(std::launch::async,
                                          [b = std::make_shared<cli::Block>(std::move(block)), table, count_raw_upper,
                                           width_known, w, fixed_width]() {
                                              return parse_block(*b, table, count_raw_upper, width_known, w, fixed_width);
                                          }));
            block = cli::Block();
        }
        if (inflight.empty())
            break;
        ParsedBlock pb = inflight.front().get();
        inflight.pop_front();
        if (!pb.error.empty())
            die_message(pb.error);
        if (!width_known && pb.al->n) {
            width_known = true;
            w = pb.al->width;
        }
        const bool stop = pb.stop;
        consume(std::move(pb.al));
        if (stop) {
            for (auto &f : inflight)
                f.wait();
            return;
        }
    }
}

// load_fasta(): src/fastaio.rs:174-199 (blocks parsed in parallel, assembled in file order)
Alignment load_fasta(FILE *fh, const uint8_t *table, size_t threads)
{
    Alignment al;
    bool first = true;
    // DISTANCE_PARSE_BLOCK_BYTES: test hook (tiny blocks put the records of a small file into different parse blocks)
    const char *bb = std::getenv("DISTANCE_PARSE_BLOCK_BYTES");
    const size_t block_bytes = bb && std::atol(bb) > 0 ? (size_t)std::atol(bb) : (size_t)32 << 20;
    // the codes are fewer than the file's bytes: one allocation, no growth copies of a multi-GB vector
    struct stat st;
    if (fstat(fileno(fh), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0)
        al.codes.reserve((size_t)st.st_size);
    // a part's codes are copied into place off this thread (it reads the next block meanwhile: the copy of 1.5 GB was a
    // third of the time this loop took) — as long as the reserved buffer holds them: a growing buffer moves
    std::deque<std::future<void>> copies;
    parse_stream(fh, block_bytes, threads, table, false, false, 0, [&](std::unique_ptr<Alignment> part) {
        if (part->n == 0)
            return;
        if (first) {
            al.width = part->width;
            first = false;
        }
        const size_t at = al.codes.size(), bytes = part->codes.size();
        const bool in_place = at + bytes <= al.codes.capacity();
        if (!in_place) {   // the buffer is about to move: nothing may still be writing into it
            for (auto &c : copies)
                c.get();
            copies.clear();
        }
        al.codes.resize(at + bytes);
        for (auto &id : part->ids)
            al.ids.push_back(std::move(id));
        al.n += part->n;
        if (in_place) {
            while (copies.size() >= 4) {
                copies.front().get();
                copies.pop_front();
            }
            uint8_t *dst = al.codes.data() + at;
            copies.push_back(std::async(std::launch::async, [dst, bytes, p = std::shared_ptr<Alignment>(std::move(part))] {
                std::memcpy(dst, p->codes.data(), bytes);
            }));
        } else {
            std::memcpy(al.codes.data() + at, part->codes.data(), bytes);
        }
    });
    for (auto &c : copies)
        c.get();
    if (al.n == 0)
        die_message("Empty FASTA file");  // src/fastaio.rs:97-99
    return al;
}

// ---------------------------------------------------------------- ordered output --------------
struct Writer {
    FILE *fh = stdout;
    void write(const char *p, size_t n)
    {
        if (!n)
            return;
        if (std::fwrite(p, 1, n, fh) != n) {
            if (errno == EPIPE)
                _exit(0);  // handle_broken_pipe(): src/lib.rs:598-608
            die_io("write", errno);
        }
    }
    void flush()
    {
        if (std::fflush(fh) != 0) {
            if (errno == EPIPE)
                _exit(0);
            die_io("flush", errno);
        }
    }
};

struct Ctx {
    dst_ctx *h = nullptr;
    void check(int rc, const char *what) const
    {
        if (rc != DST_OK) {
            std::fprintf(stderr, "Error: Gpu(\"%s: %s\")\n", what, dst_last_error(h));
            leave(1);
        }
    }
};

// One slab of results: rows [rb, re) of the row set against the column set (square: j > i).
// Text buffers come from a pool: a fresh multi-megabyte allocation is mmap'ed and page-faulted in on every slab
// (the kernel zeroes each page), which cost a fifth of the formatting time at 1e9 lines.
class TextPool {
public:
    ~TextPool()
    {
        for (auto &b : free_)
            delete[] b.first;
    }
    char *acquire(size_t need, size_t *cap)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            size_t best = free_.size();
            for (size_t k = 0; k < free_.size(); ++k)
                if (free_[k].second >= need && (best == free_.size() || free_[k].second < free_[best].second))
                    best = k;
            if (best != free_.size()) {
                auto b = free_[best];
                free_.erase(free_.begin() + (long)best);
                *cap = b.second;
                return b.first;
            }
        }
        *cap = need;
        return new char[need];
    }
    void release(char *p, size_t cap)
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (free_.size() >= 64) {  // bound what is kept
            delete[] p;
            return;
        }
        free_.emplace_back(p, cap);
    }

private:
    std::mutex mu_;
    std::vector<std::pair<char *, size_t>> free_;
};
TextPool g_text_pool;

// un-initialised growable char buffer (std::string::resize would zero-fill every byte first)
struct TextBuf {
    struct Ptr {  // minimal owner so that the call sites keep reading `out.p.get()`
        char *raw = nullptr;
        char *get() const { return raw; }
    } p;
    size_t len = 0, cap = 0;
    TextBuf() = default;
    TextBuf(const TextBuf &) = delete;
    TextBuf &operator=(const TextBuf &) = delete;
    TextBuf(TextBuf &&o) noexcept : p(o.p), len(o.len), cap(o.cap)
    {
        o.p.raw = nullptr;
        o.len = o.cap = 0;
    }
    TextBuf &operator=(TextBuf &&o) noexcept
    {
        if (this != &o) {
            drop();
            p = o.p;
            len = o.len;
            cap = o.cap;
            o.p.raw = nullptr;
            o.len = o.cap = 0;
        }
        return *this;
    }
    ~TextBuf() { drop(); }
    void drop()
    {
        if (p.raw)
            g_text_pool.release(p.raw, cap);
        p.raw = nullptr;
        len = cap = 0;
    }
    void ensure(size_t need)
    {
        if (len + need <= cap)
            return;
        size_t ncap = 0;
        char *q = g_text_pool.acquire(std::max(cap + cap / 2, len + need + ((size_t)1 << 16)), &ncap);
        if (len)
            std::memcpy(q, p.raw, len);
        if (p.raw)
            g_text_pool.release(p.raw, cap);
        p.raw = q;
        cap = ncap;
    }
};

// page-locked result buffers, recycled between slabs (pinning pages costs more than the copy)
// Page-locking a 200 MB buffer costs ~40 ms and unlocking it ~25: the pool hands out buffers of ONE size (the caller asks
// for its largest slab: slabs of whole rows differ by a row's worth, and a buffer a few bytes short used to mean a new
// one — 0.3 s of a 2 s run at 50,000 x 30,000), a helper thread brings the first ones up while the sets are uploaded
// (prewarm), and nothing is unlocked on the way out: the process ends right after the last slab.
class PinnedPool {
public:
    ~PinnedPool()
    {
        if (warm_.joinable())
            warm_.join();
    }
    void prewarm(size_t count, size_t bytes)
    {
        pending_ = count;
        warm_ = std::thread([this, count, bytes] {
            for (size_t k = 0; k < count; ++k) {
                void *p = nullptr;
                const bool ok = dst_host_alloc(bytes, &p) == DST_OK;
                std::lock_guard<std::mutex> lk(mu_);
                if (ok)
                    free_.emplace_back(p, bytes);
                --pending_;
                cv_.notify_all();
            }
        });
    }
    uint32_t *acquire(size_t bytes, size_t *cap)
    {
        {
            std::unique_lock<std::mutex> lk(mu_);
            for (;;) {
                for (size_t k = 0; k < free_.size(); ++k)
                    if (free_[k].second >= bytes) {
                        auto b = free_[k];
                        free_.erase(free_.begin() + (long)k);
                        *cap = b.second;
                        return static_cast<uint32_t *>(b.first);
                    }
                if (pending_ == 0)
                    break;
                cv_.wait(lk);   // one is on its way
            }
        }
        void *p = nullptr;
        if (dst_host_alloc(bytes, &p) != DST_OK)
            return nullptr;
        *cap = bytes;
        return static_cast<uint32_t *>(p);
    }
    void release(uint32_t *p, size_t cap)
    {
        std::lock_guard<std::mutex> lk(mu_);
        free_.emplace_back(p, cap);
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::pair<void *, size_t>> free_;
    size_t pending_ = 0;
    std::thread warm_;
};

struct Slab {
    uint64_t rb = 0, re = 0;
    uint32_t *tallies = nullptr;  // page-locked (PinnedPool): the copy back runs at link speed
    size_t tallies_cap = 0;
    std::vector<TextBuf> text;            // formatted parts, in canonical order
    char *gtext = nullptr;                // the whole slab's text, formatted on the GPU (page-locked, PinnedPool)
    size_t gtext_len = 0, gtext_cap = 0;
};

struct Job {
    int measure = 0;
    bool square = true;
    bool swap_ids = false;            // stream mode: rows are the streamed batch, id1 is the loaded id
    const Alignment *rows = nullptr;  // row set (ids + per-record counts)
    const Alignment *cols = nullptr;
    const uint32_t *row_counts = nullptr, *col_counts = nullptr;  // tn93 {A,T,G,C}
    size_t fmt_threads = 1;
    bool gpu_text = false;            // the GPU writes the TSV lines itself (dst_text_*); the host only writes them out
    int matrix = -1;                  // >= 0: rows of a distance matrix in this layout (dst_matrix_style), every column
};

// tallies -> TSV text, in canonical order, split over the formatting pool (-t)
void format_slab(const Job &job, Slab &slab)
{
    const int w = dst_tally_width(job.measure);
    const uint64_t ncols = job.cols->n;
    const uint64_t rows = slab.re - slab.rb;
    const size_t T = std::max<size_t>(1, std::min<size_t>(job.fmt_threads, rows));
    slab.text.clear();
    slab.text.resize(T);
    // split rows so that each part has about the same number of pairs
    std::vector<uint64_t> cut(T + 1, slab.re);
    cut[0] = slab.rb;
    {
        auto pairs_before = [&](uint64_t r) -> uint64_t {
            if (!job.square)
                return (r - slab.rb) * ncols;
            return dst_square_row_start(ncols, r) - dst_square_row_start(ncols, slab.rb);
        };
        const uint64_t total = pairs_before(slab.re);
        uint64_t r = slab.rb;
        for (size_t k = 1; k < T; ++k) {
            const uint64_t target = total * k / T;
            while (r < slab.re && pairs_before(r) < target)
                ++r;
            cut[k] = r;
        }
    }
    // hot loop of the host side: one TSV line per pair, written with raw pointer bumps into a
    // buffer that is grown geometrically (std::string::append per field costs ~4x more)
    const bool is_int = job.measure == DST_N || job.measure == DST_N_HIGH;
    auto pairs_between = [&](uint64_t r0, uint64_t r1) -> uint64_t {
        if (!job.square)
            return (r1 - r0) * ncols;
        return dst_square_row_start(ncols, r1) - dst_square_row_start(ncols, r0);
    };
    size_t id_max = 0;
    for (const auto &id : job.cols->ids)
        id_max = std::max(id_max, id.size());
    // raw / jc69 / k80: the distance is a function of the pair's tallies alone, and the same tallies recur all the
    // time (a few hundred distinct (n, d) in a SARS-CoV-2-like alignment): a small direct-mapped memo of
    // tallies -> printed number takes most pairs past dst_finalize and the exact decimal conversion.  A miss
    // computes it the ordinary way, so the text is the same either way.
    const bool memo_ok = job.measure == DST_RAW || job.measure == DST_JC69 || job.measure == DST_K80;
    struct Memo {
        uint64_t key_lo;
        uint32_t key_hi;
        uint8_t len;   // 0: empty
        char text[27];
    };
    constexpr size_t kMemoSize = 1u << 14;
    auto work = [&](size_t k) {
        TextBuf &out = slab.text[k];
        std::vector<Memo> memo(memo_ok ? kMemoSize : 0);
        for (auto &mslot : memo)
            mslot.len = 0;
        // first guess: 16 characters of number per line; grows (rarely) if a line needs more
        out.ensure((size_t)pairs_between(cut[k], cut[k + 1]) * (2 * id_max + 20) + 64);
        for (uint64_t i = cut[k]; i < cut[k + 1]; ++i) {
            const uint64_t j0 = job.square ? i + 1 : 0;
            uint64_t p = job.square ? dst_square_row_start(ncols, i) - dst_square_row_start(ncols, slab.rb)
                                    : (i - slab.rb) * ncols;
            const std::string &row_id = job.rows->ids[i];
            const uint32_t *rc = job.row_counts ? job.row_counts + 4 * i : nullptr;
            for (uint64_t j = j0; j < ncols; ++j, ++p) {
                const uint32_t *tl = &slab.tallies[p * w];
                const std::string &id1 = job.swap_ids ? job.cols->ids[j] : row_id;
                const std::string &id2 = job.swap_ids ? row_id : job.cols->ids[j];
                out.ensure(id1.size() + id2.size() + 3 + cli::kFixed12Max);
                char *o = out.p.get() + out.len;
                std::memcpy(o, id1.data(), id1.size());
                o += id1.size();
                *o++ = '\t';
                std::memcpy(o, id2.data(), id2.size());
                o += id2.size();
                *o++ = '\t';
                Memo *slot = nullptr;
                uint64_t key_lo = 0;
                uint32_t key_hi = 0;
                if (memo_ok) {
                    key_lo = (uint64_t)tl[0] | (uint64_t)tl[1] << 32;
                    key_hi = w > 2 ? tl[2] : 0u;
                    slot = &memo[(size_t)((key_lo * 0x9E3779B97F4A7C15ull ^ (uint64_t)key_hi * 0xC2B2AE3D27D4EB4Full) >> 50)];
                    if (slot->len && slot->key_lo == key_lo && slot->key_hi == key_hi) {
                        std::memcpy(o, slot->text, sizeof slot->text);  // fixed-size copy; only `len` bytes count
                        o += slot->len;
                        *o++ = '\n';
                        out.len = (size_t)(o - out.p.get());
                        continue;
                    }
                }
                double f = 0;
                int64_t iv = 0;
                const uint32_t *cc = job.col_counts ? job.col_counts + 4 * j : nullptr;
                // record_1 = loaded / file-0 record, record_2 = the other (src/lib.rs:325, 432-434)
                if (job.swap_ids)
                    dst_finalize(job.measure, tl, cc, rc, &f, &iv);
                else
                    dst_finalize(job.measure, tl, rc, cc, &f, &iv);
                const int len = is_int ? cli::fmt_i64(iv, o) : cli::fmt_fixed12(f, o);
                if (slot && (size_t)len <= sizeof slot->text) {
                    slot->key_lo = key_lo;
                    slot->key_hi = key_hi;
                    slot->len = (uint8_t)len;
                    std::memcpy(slot->text, o, (size_t)len);
                }
                o += len;
                *o++ = '\n';
                out.len = (size_t)(o - out.p.get());
            }
        }
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 1; k < T; ++k)
            th.emplace_back(work, k);
        work(0);
        for (auto &t : th)
            t.join();
    }
}

// tallies of whole matrix rows (every column, the slab's rectangle) -> "<id>" then "<sep><value>" per column, then '\n':
// each cell the text the long form prints for its canonical pair (square: (min, max), tn93 counts in that order)
void format_matrix_slab(const Job &job, Slab &slab)
{
    const int w = dst_tally_width(job.measure);
    const uint64_t ncols = job.cols->n;
    const uint64_t rows = slab.re - slab.rb;
    const size_t T = std::max<size_t>(1, std::min<size_t>(job.fmt_threads, rows));
    const bool is_int = job.measure == DST_N || job.measure == DST_N_HIGH;
    const char sep = job.matrix == DST_MATRIX_PHYLIP ? ' ' : '\t';
    slab.text.clear();
    slab.text.resize(T);
    auto work = [&](size_t k) {
        TextBuf &out = slab.text[k];
        const uint64_t r0 = slab.rb + rows * k / T, r1 = slab.rb + rows * (k + 1) / T;
        out.ensure((size_t)(r1 - r0) * (ncols * 16 + 64) + 64);
        for (uint64_t i = r0; i < r1; ++i) {
            const std::string &id = job.rows->ids[i];
            out.ensure(id.size() + 1);
            std::memcpy(out.p.get() + out.len, id.data(), id.size());
            out.len += id.size();
            for (uint64_t j = 0; j < ncols; ++j) {
                const uint32_t *tl = &slab.tallies[((i - slab.rb) * ncols + j) * w];
                const uint64_t q = job.square ? std::min(i, j) : i, t = job.square ? std::max(i, j) : j;
                double f = 0;
                int64_t iv = 0;
                dst_finalize(job.measure, tl, job.row_counts ? job.row_counts + 4 * q : nullptr,
                             job.col_counts ? job.col_counts + 4 * t : nullptr, &f, &iv);
                out.ensure(1 + cli::kFixed12Max + 1);
                char *o = out.p.get() + out.len;
                *o++ = sep;
                o += is_int ? cli::fmt_i64(iv, o) : cli::fmt_fixed12(f, o);
                out.len = (size_t)(o - out.p.get());
            }
            out.ensure(1);
            out.p.get()[out.len++] = '\n';
        }
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 1; k < T; ++k)
            th.emplace_back(work, k);
        work(0);
        for (auto &t : th)
            t.join();
    }
}

// rows [0, n_rows) cut into slabs of <= max_pairs pairs (at least one row each)
std::vector<std::pair<uint64_t, uint64_t>> make_slabs(bool square, uint64_t n_rows, uint64_t n_cols, uint64_t max_pairs)
{
    std::vector<std::pair<uint64_t, uint64_t>> out;
    uint64_t rb = 0;
    const uint64_t last = square ? (n_rows ? n_rows - 1 : 0) : n_rows;  // the last square row has no pairs
    while (rb < last) {
        uint64_t re = rb, pairs = 0;
        while (re < last) {
            const uint64_t row_pairs = square ? n_cols - re - 1 : n_cols;
            if (re > rb && pairs + row_pairs > max_pairs)
                break;
            pairs += row_pairs;
            ++re;
        }
        out.emplace_back(rb, re);
        rb = re;
    }
    return out;
}

// Compute every slab on the GPUs (slab k on GPU k mod G), format on the host pool, write in order.
// Three stages, like the reference's generator -> workers -> gather_write (src/lib.rs:377-458):
//   GPU threads (one per context): slab k's tallies into page-locked memory, slab k on context k mod G;
//   formatter threads: tallies -> exact TSV text (each fans out over its share of the -t pool);
//   the calling thread: writes slabs strictly in canonical order (gather_write's idx re-ordering).
void run_slabs(std::vector<Ctx> &gpus, const Job &job, int row_slot, int col_slot, uint64_t max_pairs, Writer &wr)
{
    // a matrix has every column in every row (the square's both triangles and diagonal): slabs of whole rows of cells
    const bool matrix = job.matrix >= 0;
    const bool tri = job.square && !matrix;   // the long form's triangle
    const auto slabs = make_slabs(tri, job.rows->n, job.cols->n, max_pairs);
    const int w = dst_tally_width(job.measure);
    std::mutex mu;
    std::condition_variable cv;
    size_t next_to_write = 0;
    std::atomic<size_t> next_slab{0};
    const size_t n_formatters = 2;
    // bound on slabs in flight (page-locked memory; pinning a 240 MB text buffer costs ~40 ms): with the GPU writing
    // the text a slab is either being copied back or being written out
    const size_t window = job.gpu_text ? gpus.size() * 2 + 1 : gpus.size() * 2 + n_formatters + 1;
    PinnedPool pool;
    std::deque<std::pair<size_t, std::unique_ptr<Slab>>> computed;  // GPU done, waiting for a formatter
    size_t gpu_threads_left = gpus.size();
    std::vector<std::unique_ptr<Slab>> ready(slabs.size());
    Job fjob = job;
    fjob.fmt_threads = std::max<size_t>(1, job.fmt_threads / n_formatters);
    size_t row_id_max = 0, col_id_max = 0;
    for (const auto &id : job.rows->ids)
        row_id_max = std::max(row_id_max, id.size());
    for (const auto &id : job.cols->ids)
        col_id_max = std::max(col_id_max, id.size());
    // every text buffer has the size of the largest slab (ids + number + separators per line)
    uint64_t slab_pairs_max = 0, slab_rows_max = 0;
    for (const auto &sl : slabs) {
        slab_pairs_max = std::max<uint64_t>(slab_pairs_max, tri ? dst_square_row_start(job.cols->n, sl.second) -
                                                                       dst_square_row_start(job.cols->n, sl.first)
                                                                 : (sl.second - sl.first) * job.cols->n);
        slab_rows_max = std::max<uint64_t>(slab_rows_max, sl.second - sl.first);
    }
    // matrix: separator + number per cell, id + '\n' per row
    const size_t text_bytes = matrix ? (size_t)slab_pairs_max * 33 + (size_t)slab_rows_max * (row_id_max + 1) + 64
                                     : (size_t)slab_pairs_max * (row_id_max + col_id_max + 34) + 64;
    if (job.gpu_text && !slabs.empty())
        pool.prewarm(std::min(window, slabs.size()), text_bytes);

    auto gpu_worker = [&](size_t g) {
        for (;;) {
            const size_t k = next_slab.fetch_add(1);
            if (k >= slabs.size())
                break;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return k < next_to_write + window; });
            }
            auto s = std::make_unique<Slab>();
            s->rb = slabs[k].first;
            s->re = slabs[k].second;
            const uint64_t pairs = tri ? dst_square_row_start(job.cols->n, s->re) - dst_square_row_start(job.cols->n, s->rb)
                                       : (s->re - s->rb) * job.cols->n;
            if (job.gpu_text) {
                // ids + number + separators per line; a slab the device formatter declines (a value without a short
                // text, a slab beyond its limits) is formatted on the host like before
                size_t cap = 0, len = 0;
                (void)pairs;
                char *buf = reinterpret_cast<char *>(pool.acquire(text_bytes, &cap));
                if (!buf)
                    gpus[g].check(DST_ERR_NOMEM, "pinned host buffer");
                const int trc = matrix ? dst_text_matrix(gpus[g].h, job.measure, job.square ? 1 : 0, row_slot, col_slot, s->rb,
                                                         s->re, job.matrix, buf, cap, &len)
                                : job.square ? dst_text_square(gpus[g].h, job.measure, s->rb, s->re, buf, cap, &len)
                                             : dst_text_rect(gpus[g].h, job.measure, row_slot, col_slot, s->rb, s->re, 0, buf,
                                                             cap, &len);
                if (trc == DST_OK) {
                    s->gtext = buf;
                    s->gtext_len = len;
                    s->gtext_cap = cap;
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        ready[k] = std::move(s);
                    }
                    cv.notify_all();
                    continue;
                }
                pool.release(reinterpret_cast<uint32_t *>(buf), cap);
                if (trc != DST_ERR_STATE && trc != DST_ERR_ARG && trc != DST_ERR_CAPACITY)
                    gpus[g].check(trc, "text");
            }
            const size_t n_tallies = (size_t)pairs * w;
            s->tallies = pool.acquire(std::max<size_t>(n_tallies, 1) * 4, &s->tallies_cap);
            if (!s->tallies)
                gpus[g].check(DST_ERR_NOMEM, "pinned host buffer");
            // (a square matrix: the set against itself as a rectangle, every column of the rows)
            const int rc = tri ? dst_run_square_host(gpus[g].h, job.measure, s->rb, s->re, DST_OUT_TALLY, s->tallies,
                                                     n_tallies * 4)
                               : dst_run_rect_host(gpus[g].h, job.measure, job.square ? 0 : row_slot, job.square ? 0 : col_slot,
                                                   s->rb, s->re, DST_OUT_TALLY, s->tallies, n_tallies * 4);
            gpus[g].check(rc, "run");
            {
                std::lock_guard<std::mutex> lk(mu);
                computed.emplace_back(k, std::move(s));
            }
            cv.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu);
        --gpu_threads_left;
        cv.notify_all();
    };
    auto formatter = [&]() {
        for (;;) {
            std::pair<size_t, std::unique_ptr<Slab>> item;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !computed.empty() || gpu_threads_left == 0; });
                if (computed.empty())
                    return;
                item = std::move(computed.front());
                computed.pop_front();
            }
            if (matrix)
                format_matrix_slab(fjob, *item.second);
            else
                format_slab(fjob, *item.second);
            pool.release(item.second->tallies, item.second->tallies_cap);
            item.second->tallies = nullptr;
            {
                std::lock_guard<std::mutex> lk(mu);
                ready[item.first] = std::move(item.second);
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> workers;
    for (size_t g = 0; g < gpus.size(); ++g)
        workers.emplace_back(gpu_worker, g);
    for (size_t f = 0; f < n_formatters; ++f)
        workers.emplace_back(formatter);
    // ordered writer (the reference's gather_write re-orders by batch idx: src/lib.rs:616-637)
    while (next_to_write < slabs.size()) {
        std::unique_ptr<Slab> s;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return ready[next_to_write] != nullptr; });
            s = std::move(ready[next_to_write]);
        }
        if (s->gtext) {
            wr.write(s->gtext, s->gtext_len);
            pool.release(reinterpret_cast<uint32_t *>(s->gtext), s->gtext_cap);
        }
        for (const TextBuf &part : s->text)
            wr.write(part.p.get(), part.len);
        {
            std::lock_guard<std::mutex> lk(mu);
            ++next_to_write;
        }
        cv.notify_all();
    }
    for (auto &t : workers)
        t.join();
}

// ---------------------------------------------------------------- host self-tests (no GPU) -----
// --nearest: per record of the first file (in input order) its k_used nearest records — of the same file (one input,
// the square) or of the second — from dst_nearest, each line "own id, neighbour id, value" with the value's text exactly
// as the full run prints that pair: the canonical pair's tallies through dst_finalize, then dst_format_distance.
void write_nearest(const Ctx &gpu, const std::vector<Alignment> &loaded, const std::vector<std::vector<uint32_t>> &counts,
                   int measure, uint32_t k, Writer &wr)
{
    const bool square = loaded.size() == 1;
    const Alignment &rows = loaded[0], &cols = loaded.back();
    const size_t W = (size_t)dst_tally_width(measure);
    const size_t cap = rows.n * std::min<size_t>(k, square ? (rows.n ? rows.n - 1 : 0) : cols.n);
    std::vector<uint32_t> index(std::max<size_t>(cap, 1)), tallies(std::max<size_t>(cap * W, 1));
    uint32_t ku = 0;
    gpu.check(dst_nearest(gpu.h, measure, square ? 1 : 0, 0, 1, k, index.data(), tallies.data(), nullptr, cap, &ku), "nearest");
    const uint32_t *rc = measure == DST_TN93 ? counts[0].data() : nullptr;
    const uint32_t *cc = measure == DST_TN93 ? counts.back().data() : nullptr;
    std::string out;
    char num[64];
    for (size_t i = 0; i < rows.n; ++i)
        for (size_t e = 0; e < ku; ++e) {
            const size_t at = i * ku + e, j = index[at];
            const size_t q = square ? std::min(i, j) : i, t = square ? std::max(i, j) : j;
            double f = 0;
            int64_t v = 0;
            dst_finalize(measure, &tallies[at * W], rc ? rc + 4 * q : nullptr, cc ? cc + 4 * t : nullptr, &f, &v);
            const int len = dst_format_distance(measure, f, v, num, sizeof num);
            out += rows.ids[i];
            out += '\t';
            out += cols.ids[j];
            out += '\t';
            out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
            out += '\n';
            if (out.size() >= ((size_t)1 << 20)) {
                wr.write(out.data(), out.size());
                out.clear();
            }
        }
    wr.write(out.data(), out.size());
}

// --clusters: one line per record in input order, "id, cluster", from dst_clusters' labels (the smallest record of the
// cluster); clusters are numbered from 1 in order of their first record, which is the record its label names.
void write_clusters(const Ctx &gpu, const Alignment &set, int measure, double threshold, Writer &wr)
{
    std::vector<uint32_t> label(std::max<size_t>(set.n, 1)), number(std::max<size_t>(set.n, 1), 0);
    uint64_t n_clusters = 0, links = 0;
    gpu.check(dst_clusters(gpu.h, measure, threshold, 0, label.data(), set.n, &n_clusters, &links), "clusters");
    static const char header[] = "sequence\tcluster\n";
    wr.write(header, sizeof header - 1);
    std::string out;
    uint32_t next = 0;
    for (size_t i = 0; i < set.n; ++i) {
        if (label[i] == i)
            number[i] = ++next;
        out += set.ids[i];
        out += '\t';
        out += std::to_string(number[label[i]]);
        out += '\n';
        if (out.size() >= ((size_t)1 << 20)) {
            wr.write(out.data(), out.size());
            out.clear();
        }
    }
    wr.write(out.data(), out.size());
}

// --mst: the edges of dst_mst in its order, each line "id_i, id_j, value" with the value's text exactly as the full run
// prints that pair: the edge's tallies through dst_finalize, then dst_format_distance (as write_nearest).
// --sites: the fourth field of a --max-distance / --mst line.  The pairs of dst_pair_sites' entries, each "X<pos>Y": pos
// 1-based, X / Y the IUPAC letter of the first / second record's nibble; "." for a pair without listed sites.
// diff_tally: how many entries a pair has, from its DST_OUT_TALLY words (dst_pair_sites' first consequence), which sizes
// the buffers without a counting call.
uint64_t diff_tally(int measure, const uint32_t *t)
{
    return measure == DST_K80 ? (uint64_t)t[1] + t[2] : measure == DST_TN93 ? t[1] : t[0];
}

void append_sites(std::string &out, const uint32_t *sites, const uint8_t *bases, uint64_t begin, uint64_t end)
{
    static const char letter[] = "?TCYGKSBAWMHRDVN";   // by nibble: A 8, G 4, C 2, T 1
    if (begin == end)
        out += '.';
    for (uint64_t k = begin; k < end; ++k) {
        if (k != begin)
            out += ',';
        out += letter[bases[k] >> 4];
        out += std::to_string((uint64_t)sites[k] + 1);
        out += letter[bases[k] & 15];
    }
}

// "id_i, id_j, value": the three fields of every pair line, the value from the pair's tallies (as write_nearest)
void append_pair(std::string &out, const std::string &id_i, const std::string &id_j, int measure, const uint32_t *tallies,
                 const uint32_t *qc, const uint32_t *tc)
{
    char num[64];
    double f = 0;
    int64_t v = 0;
    dst_finalize(measure, tallies, qc, tc, &f, &v);
    const int len = dst_format_distance(measure, f, v, num, sizeof num);
    out += id_i;
    out += '\t';
    out += id_j;
    out += '\t';
    out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
}

// The lines of pairs (row[e], col[e]), e < n, with their sites: dst_pair_sites in batches of DST_PAIR_SITES_BATCH pairs,
// each batch's buffers sized from the pairs' tallies.
void write_pairs_with_sites(const Ctx &gpu, const Alignment &rows, const Alignment &cols, bool square, const uint32_t *row_counts,
                            const uint32_t *col_counts, int measure, const uint32_t *row, const uint32_t *col,
                            const uint32_t *tallies, uint64_t n, Writer &wr)
{
    const size_t W = (size_t)dst_tally_width(measure);
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> sites;
    std::vector<uint8_t> bases;
    std::string out;
    for (uint64_t e0 = 0; e0 < n; e0 += DST_PAIR_SITES_BATCH) {
        const uint64_t m = std::min<uint64_t>(DST_PAIR_SITES_BATCH, n - e0);
        uint64_t cap = 0, total = 0;
        for (uint64_t e = e0; e < e0 + m; ++e)
            cap += diff_tally(measure, tallies + e * W);
        offsets.assign(m + 1, 0);
        sites.resize(std::max<uint64_t>(cap, 1));
        bases.resize(std::max<uint64_t>(cap, 1));
        gpu.check(dst_pair_sites(gpu.h, measure, square ? 1 : 0, 0, 1, row + e0, col + e0, m, offsets.data(), sites.data(),
                                 bases.data(), cap, &total),
                  "pair sites");
        for (uint64_t k = 0; k < m; ++k) {
            const size_t i = row[e0 + k], j = col[e0 + k];
            append_pair(out, rows.ids[i], cols.ids[j], measure, tallies + (e0 + k) * W, row_counts ? row_counts + 4 * i : nullptr,
                        col_counts ? col_counts + 4 * j : nullptr);
            out += '\t';
            append_sites(out, sites.data(), bases.data(), offsets[k], offsets[k + 1]);
            out += '\n';
            if (out.size() >= ((size_t)1 << 20)) {
                wr.write(out.data(), out.size());
                out.clear();
            }
        }
    }
    wr.write(out.data(), out.size());
}

void write_mst(const Ctx &gpu, const Alignment &set, const std::vector<uint32_t> &counts, int measure, uint64_t max_pairs,
               bool with_sites, Writer &wr)
{
    const size_t W = (size_t)dst_tally_width(measure);
    const size_t cap = std::max<size_t>(set.n, 1);
    std::vector<uint32_t> ei(cap), ej(cap), tallies(cap * W);
    uint64_t n_edges = 0;
    gpu.check(dst_mst(gpu.h, measure, max_pairs, ei.data(), ej.data(), nullptr, tallies.data(), cap, &n_edges, nullptr), "mst");
    const uint32_t *cc = measure == DST_TN93 ? counts.data() : nullptr;
    if (with_sites) {
        write_pairs_with_sites(gpu, set, set, true, cc, cc, measure, ei.data(), ej.data(), tallies.data(), n_edges, wr);
        return;
    }
    std::string out;
    char num[64];
    for (size_t e = 0; e < n_edges; ++e) {
        const size_t i = ei[e], j = ej[e];
        double f = 0;
        int64_t v = 0;
        dst_finalize(measure, &tallies[e * W], cc ? cc + 4 * i : nullptr, cc ? cc + 4 * j : nullptr, &f, &v);
        const int len = dst_format_distance(measure, f, v, num, sizeof num);
        out += set.ids[i];
        out += '\t';
        out += set.ids[j];
        out += '\t';
        out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
        out += '\n';
        if (out.size() >= ((size_t)1 << 20)) {
            wr.write(out.data(), out.size());
            out.clear();
        }
    }
    wr.write(out.data(), out.size());
}

// --max-distance: the lines of the full run whose pair is a link of dst_links at T, in its (the full run's) order.  The
// sink formats one chunk of links at a time: "id_row, id_col, value" with the value's text exactly as the full run prints
// that pair, from the link's tallies through dst_finalize, then dst_format_distance (as write_mst).
struct LinksText {
    const Alignment *rows, *cols;
    const uint32_t *row_counts, *col_counts;   // tn93
    int measure;
    size_t W;
    Writer *wr;
    std::string out;
};

int links_text_sink(void *user, uint64_t, uint64_t n_links, const uint32_t *row, const uint32_t *col, const void *,
                    const uint32_t *tallies)
{
    LinksText &lt = *static_cast<LinksText *>(user);
    char num[64];
    for (uint64_t e = 0; e < n_links; ++e) {
        const size_t i = row[e], j = col[e];
        double f = 0;
        int64_t v = 0;
        dst_finalize(lt.measure, tallies + e * lt.W, lt.row_counts ? lt.row_counts + 4 * i : nullptr,
                     lt.col_counts ? lt.col_counts + 4 * j : nullptr, &f, &v);
        const int len = dst_format_distance(lt.measure, f, v, num, sizeof num);
        lt.out += lt.rows->ids[i];
        lt.out += '\t';
        lt.out += lt.cols->ids[j];
        lt.out += '\t';
        lt.out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
        lt.out += '\n';
        if (lt.out.size() >= ((size_t)1 << 20)) {
            lt.wr->write(lt.out.data(), lt.out.size());
            lt.out.clear();
        }
    }
    return 0;
}

void write_links(const Ctx &gpu, const std::vector<Alignment> &loaded, const std::vector<std::vector<uint32_t>> &counts,
                 int measure, double threshold, uint64_t max_pairs, Writer &wr)
{
    LinksText lt{&loaded[0], &loaded.back(), measure == DST_TN93 ? counts[0].data() : nullptr,
                 measure == DST_TN93 ? counts.back().data() : nullptr, measure, (size_t)dst_tally_width(measure), &wr, {}};
    gpu.check(dst_links(gpu.h, measure, loaded.size() == 1 ? 1 : 0, 0, 1, threshold, max_pairs, DST_LINKS_TALLIES,
                        links_text_sink, &lt, nullptr),
              "links");
    wr.write(lt.out.data(), lt.out.size());
}

// --max-distance --sites: the context is not re-entrant, so the sink only keeps the links (row, col, tallies: 12 + 4 W
// bytes each) in host memory; the lines are written, with their sites, after dst_links has returned.
struct LinksKept {
    size_t W;
    std::vector<uint32_t> row, col, tallies;
};

int links_keep_sink(void *user, uint64_t, uint64_t n_links, const uint32_t *row, const uint32_t *col, const void *,
                    const uint32_t *tallies)
{
    LinksKept &lk = *static_cast<LinksKept *>(user);
    lk.row.insert(lk.row.end(), row, row + n_links);
    lk.col.insert(lk.col.end(), col, col + n_links);
    lk.tallies.insert(lk.tallies.end(), tallies, tallies + n_links * lk.W);
    return 0;
}

void write_links_sites(const Ctx &gpu, const std::vector<Alignment> &loaded, const std::vector<std::vector<uint32_t>> &counts,
                       int measure, double threshold, uint64_t max_pairs, Writer &wr)
{
    LinksKept lk{(size_t)dst_tally_width(measure), {}, {}, {}};
    const bool square = loaded.size() == 1;
    gpu.check(dst_links(gpu.h, measure, square ? 1 : 0, 0, 1, threshold, max_pairs, DST_LINKS_TALLIES, links_keep_sink, &lk,
                        nullptr),
              "links");
    write_pairs_with_sites(gpu, loaded[0], loaded.back(), square, measure == DST_TN93 ? counts[0].data() : nullptr,
                           measure == DST_TN93 ? counts.back().data() : nullptr, measure, lk.row.data(), lk.col.data(),
                           lk.tallies.data(), lk.row.size(), wr);
}

// --summary: one line per record of the first input in input order, "id, within, compared, mean" from dst_summary: the
// records within T, the partners with a summable distance, and sum / compared printed as an f64 distance (NaN: none)
void write_summary(const Ctx &gpu, const std::vector<Alignment> &loaded, int measure, double threshold, uint64_t max_pairs,
                   Writer &wr)
{
    const Alignment &set = loaded[0];
    const size_t cap = std::max<size_t>(set.n, 1);
    std::vector<uint32_t> within(cap), summable(cap);
    std::vector<double> sum(cap);
    gpu.check(dst_summary(gpu.h, measure, loaded.size() == 1 ? 1 : 0, 0, 1, threshold, max_pairs, 0, 0.0, nullptr, within.data(),
                          summable.data(), sum.data(), set.n, nullptr),
              "summary");
    static const char header[] = "sequence\twithin\tcompared\tmean\n";
    wr.write(header, sizeof header - 1);
    std::string out;
    char num[64];
    for (size_t i = 0; i < set.n; ++i) {
        const double mean = summable[i] ? sum[i] / (double)summable[i] : std::nan("");
        const int len = dst_format_distance(DST_RAW, mean, 0, num, sizeof num);
        out += set.ids[i];
        out += '\t';
        out += std::to_string(within[i]);
        out += '\t';
        out += std::to_string(summable[i]);
        out += '\t';
        out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
        out += '\n';
        if (out.size() >= ((size_t)1 << 20)) {
            wr.write(out.data(), out.size());
            out.clear();
        }
    }
    wr.write(out.data(), out.size());
}

// --groups: the label file, read before any input is opened.  One "id<TAB>group" per line, empty lines skipped, no header.
struct GroupFile {
    std::string path;
    std::unordered_map<std::string, std::pair<std::string, size_t>> of;   // id -> (group, the line that set it)
};

GroupFile read_group_file(const std::string &path)
{
    GroupFile gf;
    gf.path = path;
    FILE *fh = open_input(path);
    std::string text;
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, fh)) > 0;)
        text.append(buf, got);
    std::fclose(fh);
    size_t line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos)
            end = text.size();
        std::string line = text.substr(at, end - at);
        at = end + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r')
            line.pop_back();
        if (line.empty())
            continue;
        const std::string where = "--groups: line " + std::to_string(line_no) + " of '" + path + "' ";
        const size_t tab = line.find('\t');
        if (tab == std::string::npos)
            die_message(where + "has no tab: expected 'id<TAB>group'");
        const std::string id = line.substr(0, tab), group = line.substr(tab + 1);
        if (group.empty())
            die_message(where + "has an empty group");
        if (group.find('\t') != std::string::npos)
            die_message(where + "has more than two fields");
        const auto ins = gf.of.emplace(id, std::make_pair(group, line_no));
        if (!ins.second && ins.first->second.first != group)
            die_message(where + "gives '" + id + "' the group '" + group + "', line " + std::to_string(ins.first->second.second) +
                        " gave it '" + ins.first->second.first + "'");
    }
    return gf;
}

// the labels of one input: groups numbered in order of their first record, as --clusters numbers its clusters
struct GroupLabels {
    std::vector<uint32_t> label;       // per record, DST_GROUP_NONE: not in the file
    std::vector<std::string> names;    // per group
    size_t assigned = 0;
};

GroupLabels label_records(const GroupFile &gf, const Alignment &set, const char *which, std::unordered_set<std::string> &seen)
{
    GroupLabels gl;
    gl.label.assign(set.n, DST_GROUP_NONE);
    std::unordered_map<std::string, uint32_t> number;
    for (size_t r = 0; r < set.n; ++r) {
        const auto it = gf.of.find(set.ids[r]);
        if (it == gf.of.end())
            continue;
        seen.insert(set.ids[r]);
        const auto ins = number.emplace(it->second.first, (uint32_t)gl.names.size());
        if (ins.second) {
            if (gl.names.size() == DST_GROUPS_MAX)
                die_message("--groups: line " + std::to_string(it->second.second) + " of '" + gf.path + "' starts group " +
                            std::to_string(DST_GROUPS_MAX + 1) + " of the " + which + " input: more than " +
                            std::to_string(DST_GROUPS_MAX) + " groups");
            gl.names.push_back(it->second.first);
        }
        gl.label[r] = ins.first->second;
        ++gl.assigned;
    }
    if (gl.assigned == 0)
        die_message("--groups: no record of the " + std::string(which) + " input has a group in '" + gf.path + "'");
    return gl;
}

void append_distance(std::string &out, int measure, bool known, double v, int64_t iv)
{
    if (!known) {
        out += "NaN";
        return;
    }
    char num[64];
    const int len = dst_format_distance(measure, v, iv, num, sizeof num);
    out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
}

// --groups: one line per cell (one input: a <= b; two: every cell), or with --per-record one line per record of the first
// input and group of the other side, from dst_group_summary.  mean = sum / compared as --summary prints its mean.
void write_groups(const Ctx &gpu, const std::vector<Alignment> &loaded, const std::vector<GroupLabels> &labels, int measure,
                  bool has_within, double threshold, uint64_t max_pairs, bool per_record, Writer &wr)
{
    const bool square = loaded.size() == 1;
    const GroupLabels &rl = labels[0], &cl = labels.back();
    const uint32_t Gr = (uint32_t)rl.names.size(), Gc = (uint32_t)cl.names.size();
    const size_t n_rows = loaded[0].n;
    std::vector<dst_group_cell> cells(per_record ? 0 : (size_t)Gr * Gc);
    std::vector<uint32_t> within(per_record ? n_rows * Gc : 0), summable(per_record ? n_rows * Gc : 0);
    std::vector<double> sum(per_record ? n_rows * Gc : 0);
    gpu.check(dst_group_summary(gpu.h, measure, square ? 1 : 0, 0, 1, rl.label.data(), Gr, cl.label.data(), Gc,
                                has_within ? threshold : HUGE_VAL, max_pairs, per_record ? nullptr : cells.data(), cells.size(),
                                per_record ? within.data() : nullptr, per_record ? summable.data() : nullptr,
                                per_record ? sum.data() : nullptr, sum.size()),
              "group summary");
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    std::string out = per_record ? "sequence\tgroup\tcompared" : "group1\tgroup2\tpairs\tcompared";
    if (has_within)
        out += "\twithin";
    out += per_record ? "\tmean\n" : "\tmean\tmin\tmax\n";
    auto flush = [&](bool all) {
        if (all || out.size() >= ((size_t)1 << 20)) {
            wr.write(out.data(), out.size());
            out.clear();
        }
    };
    if (per_record) {
        for (size_t x = 0; x < n_rows; ++x)
            for (uint32_t g = 0; g < Gc; ++g) {
                const size_t e = x * Gc + g;
                out += loaded[0].ids[x];
                out += '\t';
                out += cl.names[g];
                out += '\t';
                out += std::to_string(summable[e]);
                if (has_within)
                    out += '\t' + std::to_string(within[e]);
                out += '\t';
                append_distance(out, DST_RAW, summable[e] != 0, summable[e] ? sum[e] / (double)summable[e] : 0.0, 0);
                out += '\n';
                flush(false);
            }
    } else {
        for (uint32_t a = 0; a < Gr; ++a)
            for (uint32_t b = square ? a : 0; b < Gc; ++b) {
                const dst_group_cell &c = cells[(size_t)a * Gc + b];
                out += rl.names[a];
                out += '\t';
                out += cl.names[b];
                out += '\t' + std::to_string(c.pairs) + '\t' + std::to_string(c.summable_pairs);
                if (has_within)
                    out += '\t' + std::to_string(c.links);
                out += '\t';
                append_distance(out, DST_RAW, c.summable_pairs != 0, c.summable_pairs ? c.sum / (double)c.summable_pairs : 0.0, 0);
                const bool known = c.pairs > c.nan_pairs;   // a pair whose payload is not NaN
                for (const uint64_t bits : {c.min_bits, c.max_bits}) {
                    double v = 0;
                    std::memcpy(&v, &bits, 8);
                    out += '\t';
                    append_distance(out, measure, known, int_payload ? 0.0 : v, int_payload ? (int64_t)bits : 0);
                }
                out += '\n';
                flush(false);
            }
    }
    flush(true);
}

// --histogram: one line per bin, "lower edge, pairs" (the edge b W as the measure's distances are printed; the last bin is
// open-ended), then "NaN, pairs without a distance"
void write_histogram(const Ctx &gpu, const std::vector<Alignment> &loaded, int measure, double width, uint32_t bins,
                     uint64_t max_pairs, Writer &wr)
{
    std::vector<uint64_t> hist(bins);
    dst_summary_totals totals;
    gpu.check(dst_summary(gpu.h, measure, loaded.size() == 1 ? 1 : 0, 0, 1, 0.0, max_pairs, bins, width, hist.data(), nullptr,
                          nullptr, nullptr, 0, &totals),
              "histogram");
    static const char header[] = "distance\tpairs\n";
    wr.write(header, sizeof header - 1);
    std::string out;
    char num[64];
    for (uint32_t b = 0; b < bins; ++b) {
        const int len = dst_format_distance(measure, (double)b * width, (int64_t)b * (int64_t)width, num, sizeof num);
        out.append(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
        out += '\t';
        out += std::to_string(hist[b]);
        out += '\n';
    }
    out += "NaN\t" + std::to_string(totals.nan_pairs) + "\n";
    wr.write(out.data(), out.size());
}

// a DST_ERR_STATE message "... the distance of records I and J is not finite" of the NJ calls, with the pair named by
// its ids; false when the message names no pair of the set
bool non_finite_pair(const Ctx &gpu, const Alignment &set, const char *prefix, const char *suffix)
{
    const std::string msg = dst_last_error(gpu.h);
    unsigned long long i = 0, j = 0;
    const size_t at = msg.find("records ");
    if (at == std::string::npos || std::sscanf(msg.c_str() + at, "records %llu and %llu", &i, &j) != 2 || i >= set.n ||
        j >= set.n)
        return false;
    std::fprintf(stderr, "error: %sthe distance of '%s' and '%s' is not finite%s\n", prefix, set.ids[i].c_str(),
                 set.ids[j].c_str(), suffix);
    return true;
}

// --tree nj: the neighbour-joining tree of one set as one Newick line (dst_nj on the GPU, dst_newick on the host);
// with --bootstrap B its internal nodes carry their support in B replicates (dst_nj_bootstrap, dst_newick_support),
// and nothing is written unless every replicate succeeded
void write_tree(const Ctx &gpu, const Alignment &set, int measure, uint64_t max_pairs, uint32_t bootstrap, uint64_t seed,
                Writer &wr)
{
    if (set.n < 3) {
        std::fprintf(stderr, "error: a neighbour-joining tree needs at least 3 records, the input has %zu\n", (size_t)set.n);
        leave(1);
    }
    std::vector<uint32_t> parent(2 * set.n - 2);
    std::vector<double> length(2 * set.n - 2);
    int rc = dst_nj(gpu.h, measure, max_pairs, parent.data(), length.data(), parent.size());
    if (rc == DST_ERR_STATE && non_finite_pair(gpu, set, "", ": no neighbour-joining tree"))
        leave(1);
    gpu.check(rc, "neighbour joining");
    std::vector<uint32_t> support;
    if (bootstrap) {
        support.resize(parent.size());
        rc = dst_nj_bootstrap(gpu.h, measure, set.codes.data(), set.n, set.width, set.width, bootstrap, seed, max_pairs,
                              parent.data(), support.data(), nullptr, support.size());
        if (rc == DST_ERR_STATE) {
            // "bootstrap replicate R: the distance of records I and J is not finite"
            unsigned long long r = 0;
            const std::string msg = dst_last_error(gpu.h);
            if (std::sscanf(msg.c_str(), "bootstrap replicate %llu", &r) == 1) {
                const std::string prefix = "bootstrap replicate " + std::to_string(r) + ": ";
                if (non_finite_pair(gpu, set, prefix.c_str(), ""))
                    leave(1);
            }
        }
        if (rc != DST_OK) {
            std::fprintf(stderr, "error: bootstrap: %s\n", dst_last_error(gpu.h));
            leave(1);
        }
    }
    std::string chars;
    std::vector<uint64_t> offsets(set.n + 1, 0);
    for (size_t r = 0; r < set.n; ++r) {
        chars += set.ids[r];
        offsets[r + 1] = chars.size();
    }
    const uint32_t *sup = bootstrap ? support.data() : nullptr;
    size_t len = 0;
    dst_newick_support(set.n, parent.data(), length.data(), chars.data(), offsets.data(), sup, nullptr, 0, &len);
    std::string out(len, '\0');
    if (dst_newick_support(set.n, parent.data(), length.data(), chars.data(), offsets.data(), sup, out.data(), out.size(),
                           &len) != DST_OK) {
        std::fprintf(stderr, "error: the Newick text of the tree could not be written\n");
        leave(1);
    }
    wr.write(out.data(), len);
}

// --dendrogram: the UPGMA / WPGMA / complete-linkage tree of one set as one Newick line with a binary root
// (dst_dendrogram on the GPU, dst_newick_rooted on the host)
void write_dendrogram(const Ctx &gpu, const Alignment &set, int measure, int linkage, uint64_t max_pairs, Writer &wr)
{
    if (set.n < 2) {
        std::fprintf(stderr, "error: a dendrogram needs at least 2 records, the input has %zu\n", (size_t)set.n);
        leave(1);
    }
    std::vector<uint32_t> parent(2 * set.n - 1);
    std::vector<double> length(2 * set.n - 1);
    const int rc = dst_dendrogram(gpu.h, measure, linkage, max_pairs, parent.data(), length.data(), nullptr, parent.size(),
                                  nullptr);
    if (rc == DST_ERR_STATE && non_finite_pair(gpu, set, "", ": no dendrogram"))
        leave(1);
    gpu.check(rc, "dendrogram");
    std::string chars;
    std::vector<uint64_t> offsets(set.n + 1, 0);
    for (size_t r = 0; r < set.n; ++r) {
        chars += set.ids[r];
        offsets[r + 1] = chars.size();
    }
    size_t len = 0;
    dst_newick_rooted(set.n, parent.data(), length.data(), chars.data(), offsets.data(), nullptr, 0, &len);
    std::string out(len, '\0');
    if (dst_newick_rooted(set.n, parent.data(), length.data(), chars.data(), offsets.data(), out.data(), out.size(), &len) !=
        DST_OK) {
        std::fprintf(stderr, "error: the Newick text of the tree could not be written\n");
        leave(1);
    }
    wr.write(out.data(), len);
}

int host_selftest(const Args &a)
{
    if (a.selftest == "fasta") {  // parse stdin, print one line per record
        uint8_t table[256];
        encoding_array(table);
        cli::FastaReader reader(stdin);
        cli::FastaRecord rec;
        for (;;) {
            const int rc = reader.next(rec);
            if (rc < 0) {
                std::printf("ERROR\t%s\n", reader.error().c_str());
                return 0;
            }
            if (rc == 0 || (rec.id.empty() && !rec.has_desc && rec.seq.empty()))
                break;
            std::printf("%s\t%s\t%s\n", rec.id.c_str(), rec.has_desc ? rec.desc.c_str() : "<none>", rec.seq.c_str());
        }
        return 0;
    }
    if (a.selftest == "fasta-blocks") {  // the same through BlockReader + parallel parse, tiny blocks
        uint8_t table[256];
        encoding_array(table);
        std::memset(table, 1, 256);  // accept every byte: this mode checks tokenisation only
        size_t total = 0;
        parse_stream(stdin, a.slab_pairs < 4096 ? a.slab_pairs : 7, 4, table, false, false, 0,
                     [&](std::unique_ptr<Alignment> part) {
                         for (size_t r = 0; r < part->n; ++r)
                             std::printf("%s\t%zu\n", part->ids[r].c_str(), part->width);
                         total += part->n;
                     });
        std::printf("records\t%zu\n", total);
        return 0;
    }
    if (a.selftest == "format") {  // hex floats on stdin -> {:.12}
        char line[256], out[512];
        while (std::fgets(line, sizeof line, stdin)) {
            const double v = std::strtod(line, nullptr);
            const int n = cli::fmt_fixed12(v, out);
            out[n] = 0;
            std::puts(out);
        }
        return 0;
    }
    if (a.selftest == "args") {
        std::printf("measure=%s threads=%zu%s batchsize=%zu stream=%s output=%s gpus=%d inputs=", a.measure.c_str(),
                    a.threads, a.has_threads ? "" : "(default)", a.batchsize, a.has_stream ? a.stream.c_str() : "<none>",
                    a.has_output ? a.output.c_str() : "<stdout>", a.gpus);
        for (auto &s : a.flag_inputs)
            std::printf("[-i %s]", s.c_str());
        for (auto &s : a.pos_inputs)
            std::printf("[pos %s]", s.c_str());
        std::puts("");
        return 0;
    }
    die_usage("unknown --host-selftest");
}

}  // namespace

// DISTANCE_TIMING=1: phase wall times on stderr
struct PhaseTimer {
    bool on = std::getenv("DISTANCE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char *what)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[timing] %-28s %8.1f ms (total %8.1f ms)\n", what,
                     std::chrono::duration<double, std::milli>(now - last).count(),
                     std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// num_cpus::get() (src/lib.rs:262): the CPUs this process may use — its affinity mask, capped by a cgroup CPU
// quota when the container has one (cgroup v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us).
static size_t available_cpus()
{
    size_t n = std::max<unsigned>(1, std::thread::hardware_concurrency());
    auto quota = [](const char *path_quota, const char *path_period) -> double {
        double q = -1, p = 100000;
        if (FILE *fh = std::fopen(path_quota, "r")) {
            char word[64] = {0};
            if (path_period == nullptr) {  // "max 100000" or "1600000 100000"
                double per = 0;
                if (std::fscanf(fh, "%63s %lf", word, &per) == 2 && std::strcmp(word, "max") != 0) {
                    q = std::atof(word);
                    p = per;
                }
            } else if (std::fscanf(fh, "%lf", &q) != 1) {
                q = -1;
            }
            std::fclose(fh);
        }
        if (path_period)
            if (FILE *fh = std::fopen(path_period, "r")) {
                if (std::fscanf(fh, "%lf", &p) != 1)
                    p = 100000;
                std::fclose(fh);
            }
        return (q > 0 && p > 0) ? q / p : -1.0;
    };
    double c = quota("/sys/fs/cgroup/cpu.max", nullptr);
    if (c < 0)
        c = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us");
    if (c > 0)
        n = std::min<size_t>(n, std::max<size_t>(1, (size_t)(c + 0.999)));
    return n;
}

int main(int argc, char **argv)
{
    PhaseTimer timer;
    std::signal(SIGPIPE, SIG_IGN);  // EPIPE is handled at the write (exit 0), like the reference
    Args a = parse_args(argc, argv);
    if (!a.selftest.empty())
        return host_selftest(a);
    if (a.licenses) {  // src/main.rs:7-10
        std::puts(kLicences);
        return 0;
    }
    // ---- set_up(): src/lib.rs:162-267 -------------------------------------------------------
    if (!a.pos_inputs.empty() && !a.flag_inputs.empty())
        die_message("For loading input files, don't use both positional arguments and the -i/--input flag");
    std::vector<std::string> inputs = a.flag_inputs;
    inputs.insert(inputs.end(), a.pos_inputs.begin(), a.pos_inputs.end());
    // --groups: the label file's own errors come before anything else is opened
    GroupFile group_file;
    if (a.has_groups)
        group_file = read_group_file(a.groups);
    std::vector<FILE *> files;
    if (inputs.empty())
        files.push_back(stdin);
    for (auto &p : inputs)
        files.push_back(open_input(p));
    FILE *stream_fh = nullptr;
    if (a.has_stream) {
        if (inputs.size() != 1)
            die_message("If you stream one file, you must also provide exactly one other file to be loaded");
        stream_fh = a.stream == "-" ? stdin : open_input(a.stream);
    }
    // ---- GPUs: the HIP runtime and the contexts come up on a thread of their own while the files are parsed (0.2 s of
    // a 2.3 s run at 50,000 x 30,000); what it finds is looked at after the parse, so a bad input is reported first,
    // as before.  One context (and one worker thread) per listed device; a device may be listed more than once.
    struct GpuInit {
        int ndev = 0;
        bool count_ok = false;
        std::vector<int> devices;
        std::vector<Ctx> gpus;
        std::string error;
    } gi;
    std::thread gpu_init([&gi, &a] {
        gi.count_ok = dst_device_count(&gi.ndev) == DST_OK && gi.ndev > 0;
        if (!gi.count_ok)
            return;
        gi.devices = a.devices;
        if (gi.devices.empty())
            for (int g = 0; g < std::max(1, std::min(a.gpus, gi.ndev)); ++g)
                gi.devices.push_back(g);
        gi.gpus.resize(gi.devices.size());
        for (size_t g = 0; g < gi.devices.size(); ++g)
            if (dst_create(gi.devices[g], &gi.gpus[g].h) != DST_OK) {
                gi.error = dst_last_error(nullptr);
                return;
            }
    });
    uint8_t table[256];
    encoding_array(table);
    const size_t threads = a.has_threads ? std::max<size_t>(a.threads, 1)  // src/lib.rs:253-263
                                         : available_cpus();
    const size_t parse_threads = std::min<size_t>(threads, 16);
    std::vector<Alignment> loaded;
    for (size_t k = 0; k < files.size(); ++k) {  // load_fastas(): src/fastaio.rs:202-212
        loaded.push_back(load_fasta(files[k], table, parse_threads));
        if (k == 1 && loaded[0].width != loaded[1].width)
            die_message(err_lengths(loaded[0].width, loaded[1].width));
    }
    timer.mark("parse + encode loaded files");
    // --groups: the records' labels, and what can be wrong with them, before the device is looked at
    std::vector<GroupLabels> group_labels;
    if (a.has_groups) {
        std::unordered_set<std::string> seen;
        for (size_t k = 0; k < loaded.size(); ++k)
            group_labels.push_back(label_records(group_file, loaded[k], k == 0 ? "first" : "second", seen));
        if (seen.size() < group_file.of.size())
            std::fprintf(stderr, "warning: --groups: %zu ids of '%s' are not in the input and were skipped\n",
                         group_file.of.size() - seen.size(), group_file.path.c_str());
    }
    Writer wr;
    if (a.has_output) {
        wr.fh = std::fopen(a.output.c_str(), "wb");
        if (!wr.fh)
            die_io(a.output, errno);
    }
    static char outbuf[1 << 20];
    std::setvbuf(wr.fh, outbuf, _IOFBF, sizeof outbuf);

    const int measure = dst_measure_from_name(a.measure.c_str());
    gpu_init.join();
    if (!gi.count_ok) {
        std::fprintf(stderr, "Error: Gpu(\"no MI355X / HIP device visible: this build has no CPU path\")\n");
        return 1;
    }
    if (!gi.error.empty()) {
        std::fprintf(stderr, "Error: Gpu(\"%s\")\n", gi.error.c_str());
        return 1;
    }
    std::vector<Ctx> &gpus = gi.gpus;
    const int G = (int)gpus.size();
    timer.mark("HIP init + contexts (what the parse did not hide)");
    for (int g = 0; g < G; ++g)
        for (size_t k = 0; k < loaded.size(); ++k)
            gpus[g].check(dst_upload(gpus[g].h, (int)k, loaded[k].codes.data(), loaded[k].n, loaded[k].width,
                                     loaded[k].width, nullptr),
                          "upload");
    // tn93: per-record base counts by code (count_bases(), src/lib.rs:233-239), from the device
    std::vector<std::vector<uint32_t>> counts(loaded.size());
    if (measure == DST_TN93)
        for (size_t k = 0; k < loaded.size(); ++k) {
            counts[k].resize(loaded[k].n * 4);
            gpus[0].check(dst_get_base_counts(gpus[0].h, (int)k, counts[k].data()), "base counts");
        }

    timer.mark("upload + pack + counts");
    static const char header[] = "sequence1\tsequence2\tdistance\n";  // src/lib.rs:613
    if (a.matrix == DST_MATRIX_TSV) {
        // an empty corner cell, then the column ids (the last input's records)
        std::string h;
        for (const auto &id : loaded.back().ids) {
            h += '\t';
            h += id;
        }
        h += '\n';
        wr.write(h.data(), h.size());
    } else if (a.matrix == DST_MATRIX_PHYLIP) {
        const std::string h = std::to_string(loaded[0].n) + "\n";
        wr.write(h.data(), h.size());
    } else if (a.has_sites) {
        static const char sites_header[] = "sequence1\tsequence2\tdistance\tsites\n";
        wr.write(sites_header, sizeof sites_header - 1);
    } else if (!a.has_clusters && !a.has_tree && a.dendrogram < 0 && !a.has_summary && !a.has_histogram && !a.has_groups) {
        wr.write(header, sizeof header - 1);
    }

    Job job;
    job.measure = measure;
    job.fmt_threads = std::max<size_t>(1, threads / (size_t)G);
    if (a.has_tree) {
        write_tree(gpus[0], loaded[0], measure, a.has_slab_pairs ? a.slab_pairs : 0, a.bootstrap, a.seed, wr);
    } else if (a.dendrogram >= 0) {
        write_dendrogram(gpus[0], loaded[0], measure, a.dendrogram, a.has_slab_pairs ? a.slab_pairs : 0, wr);
    } else if (a.has_clusters) {
        write_clusters(gpus[0], loaded[0], measure, a.clusters, wr);
    } else if (a.has_mst) {
        write_mst(gpus[0], loaded[0], counts[0], measure, a.has_slab_pairs ? a.slab_pairs : 0, a.has_sites, wr);
    } else if (a.has_max_distance) {
        if (a.has_sites)
            write_links_sites(gpus[0], loaded, counts, measure, a.max_distance, a.has_slab_pairs ? a.slab_pairs : 0, wr);
        else
            write_links(gpus[0], loaded, counts, measure, a.max_distance, a.has_slab_pairs ? a.slab_pairs : 0, wr);
    } else if (a.has_summary) {
        write_summary(gpus[0], loaded, measure, a.summary, a.has_slab_pairs ? a.slab_pairs : 0, wr);
    } else if (a.has_groups) {
        write_groups(gpus[0], loaded, group_labels, measure, a.has_groups_within, a.groups_within,
                     a.has_slab_pairs ? a.slab_pairs : 0, a.per_record, wr);
    } else if (a.has_histogram) {
        write_histogram(gpus[0], loaded, measure, a.histogram, (uint32_t)a.bins, a.has_slab_pairs ? a.slab_pairs : 0, wr);
    } else if (a.has_nearest) {
        write_nearest(gpus[0], loaded, counts, measure, (uint32_t)a.nearest, wr);
    } else if (!stream_fh) {
        // ---- load(): src/lib.rs:367-474 -------------------------------------------------------
        job.square = loaded.size() == 1;
        job.matrix = a.matrix;
        job.rows = &loaded[0];
        job.cols = &loaded.back();
        job.row_counts = measure == DST_TN93 ? counts[0].data() : nullptr;
        job.col_counts = measure == DST_TN93 ? counts.back().data() : nullptr;
        // The TSV lines themselves come from the GPU (dst_text_*): it has the distances and the ids, the exact
        // {:.12} conversion is integer arithmetic, and the host's formatter pool was what bounded a large run.
        // For jc69 / k80 / tn93 the device finalises the tallies itself and hands the values that lie near a rounding
        // boundary of the 12th decimal back to dst_finalize (libm) before the text leaves the library, so the bytes are
        // the host formatter's (tests/test_gpu_text_identity.py: 0 of 1.5e8 lines differ; DISTANCE_HOST_FORMAT=1 keeps
        // the host formatter, and tests/test_gpu_cli.py compares the two).
        job.gpu_text = std::getenv("DISTANCE_HOST_FORMAT") == nullptr;
        if (job.gpu_text)
            for (int g = 0; g < G && job.gpu_text; ++g)
                for (size_t k = 0; k < loaded.size(); ++k) {
                    std::string chars;
                    std::vector<uint64_t> offs(loaded[k].n + 1, 0);
                    for (size_t r = 0; r < loaded[k].n; ++r) {
                        chars += loaded[k].ids[r];
                        offs[r + 1] = chars.size();
                    }
                    if (dst_set_ids(gpus[g].h, (int)k, chars.data(), offs.data(), loaded[k].n) != DST_OK)
                        job.gpu_text = false;   // (e.g. 4 GB of ids): the host formatter takes over
                }
        run_slabs(gpus, job, 0, 1, a.slab_pairs, wr);
    } else {
        // ---- stream(): src/lib.rs:269-365; stream_fasta(): src/fastaio.rs:215-286 ---------------
        const Alignment &ref = loaded[0];
        // a streamed batch is bounded by records (4096), by result pairs (--slab-pairs) and by bytes
        // (512 MiB of codes: C4-sized 5 Mbp records come ~100 at a time; split-L launches keep the GPU
        // busy on such short batches)
        const size_t by_bytes = ((size_t)512 << 20) / std::max<size_t>(ref.width, 1);
        const size_t batch_records =
            std::max<size_t>(1, std::min<size_t>({(size_t)4096, a.slab_pairs / std::max<size_t>(ref.n, 1), by_bytes}));
        // reader thread: parse + encode batch k+1 while the GPUs and the formatting pool work on
        // batch k (the reference's stream_fasta thread + bounded channel, src/lib.rs:272, 290-307)
        std::mutex qmu;
        std::condition_variable qcv;
        std::deque<std::unique_ptr<Alignment>> queue;
        bool reader_done = false;
        size_t record_counter = 0;
        // bytes of FASTA per parsed block ~ records per batch
        const size_t block_bytes = std::max<size_t>(batch_records * (ref.width + 64), (size_t)1 << 20);
        std::thread reader_thread([&] {
            parse_stream(stream_fh, block_bytes, parse_threads, table, measure == DST_TN93, true, ref.width,
                         [&](std::unique_ptr<Alignment> batch) {
                             if (batch->n == 0)
                                 return;
                             record_counter += batch->n;
                             std::unique_lock<std::mutex> lk(qmu);
                             qcv.wait(lk, [&] { return queue.size() < 2; });
                             queue.push_back(std::move(batch));
                             qcv.notify_all();
                         });
            std::lock_guard<std::mutex> lk(qmu);
            reader_done = true;
            qcv.notify_all();
        });
        // Batches go round-robin to the GPUs (batch b -> GPU b mod G), each GPU runs them through its own
        // overlapped pipeline (dst_stream_*: page-locked ring slots; H2D of the next batch and D2H of the previous
        // one under the compare of the current one), the worker formats what it collects, and the main thread
        // writes the batches strictly in input order (gather_write's idx re-ordering, src/lib.rs:616-637).
        constexpr int kDepth = 3;
        struct Item {
            size_t idx;
            std::unique_ptr<Alignment> batch;
        };
        std::vector<std::deque<Item>> gq((size_t)G);       // per-GPU input queues (guarded by qmu)
        std::vector<bool> gdone((size_t)G, false);
        std::map<size_t, std::vector<TextBuf>> done_text;   // formatted batches waiting for the writer
        std::mutex wmu;
        std::condition_variable wcv;
        size_t next_to_write = 0, n_batches = 0;
        bool all_dispatched = false;
        const size_t window = (size_t)G * (kDepth + 2);     // bound on batches between dispatch and write
        std::vector<dst_stream *> streams((size_t)G, nullptr);
        // what crosses the host link: the codes' high nibbles, two sites per byte (all a measure reads: half the bytes);
        // DISTANCE_WIRE=codes keeps the Paradis bytes (tests run both)
        const char *wire_env = std::getenv("DISTANCE_WIRE");
        const bool nibbles = !(wire_env && std::strcmp(wire_env, "codes") == 0);
        // --closest: the lists stay on the GPU (dst_stream_open_closest); one GPU, so submission order is stream order
        const bool closest = a.has_closest, closest_loaded = closest && a.closest_side == DST_CLOSEST_FOR_LOADED;
        const size_t TW = (size_t)dst_tally_width(measure);
        // --within: the batch's links come back instead of its matrix (dst_stream_open_links), with their tallies
        const bool within = a.has_within;
        // closest for the loaded records: the streamed ids (one arena + offsets) and, for tn93, base counts until the end
        std::vector<char> kept_ids;
        std::vector<uint64_t> kept_off(1, 0);
        std::vector<uint32_t> kept_counts;
        // "loaded id <tab> streamed id <tab> value": the pair's tallies through dst_finalize with the streamed counts as q
        auto closest_line = [&](TextBuf &out, const std::string &lid, const char *sid, size_t sid_len, const uint32_t *tal,
                                const uint32_t *qc, const uint32_t *tc) {
            double f = 0;
            int64_t v = 0;
            dst_finalize(measure, tal, qc, tc, &f, &v);
            char num[64];
            const int len = std::min<int>(dst_format_distance(measure, f, v, num, sizeof num), (int)sizeof num - 1);
            out.ensure(lid.size() + sid_len + (size_t)len + 3);
            char *w = out.p.get() + out.len;
            std::memcpy(w, lid.data(), lid.size());
            w += lid.size();
            *w++ = '\t';
            std::memcpy(w, sid, sid_len);
            w += sid_len;
            *w++ = '\t';
            std::memcpy(w, num, (size_t)len);
            w += len;
            *w++ = '\n';
            out.len = (size_t)(w - out.p.get());
        };
        for (int g = 0; g < G; ++g)
            gpus[g].check(closest ? dst_stream_open_closest(gpus[g].h, measure, (uint32_t)a.closest, a.closest_side, batch_records,
                                                            kDepth, nibbles ? DST_WIRE_NIBBLES : DST_WIRE_CODES, &streams[g])
                          : within ? dst_stream_open_links(gpus[g].h, measure, a.within, DST_LINKS_TALLIES, 0, batch_records, kDepth,
                                                           nibbles ? DST_WIRE_NIBBLES : DST_WIRE_CODES, &streams[g])
                                  : dst_stream_open_wire(gpus[g].h, measure, DST_OUT_TALLY, batch_records, kDepth,
                                                         nibbles ? DST_WIRE_NIBBLES : DST_WIRE_CODES, &streams[g]), "stream open");
        auto gpu_stream_worker = [&](int g) {
            std::deque<Item> inflight;
            auto collect_one = [&]() {
                size_t n_rec = 0;
                const void *res = nullptr;
                gpus[g].check(dst_stream_collect(streams[g], &n_rec, &res), "stream collect");
                Item it = std::move(inflight.front());
                inflight.pop_front();
                if (within) {   // the batch's links in stream order, window after window, each as the full run's line
                    std::vector<TextBuf> text;
                    text.emplace_back();
                    const Alignment &al = *it.batch;
                    for (uint64_t first = 0;;) {
                        uint64_t m = 0, total = 0;
                        const uint32_t *srec = nullptr, *lrec = nullptr, *tal = nullptr;
                        gpus[g].check(dst_stream_links_batch(streams[g], first, &m, &total, &srec, &lrec, nullptr, &tal),
                                      "stream links batch");
                        for (uint64_t e = 0; e < m; ++e) {
                            const size_t r = srec[e], j = lrec[e];
                            closest_line(text.back(), ref.ids[j], al.ids[r].data(), al.ids[r].size(), tal + e * TW,
                                         measure == DST_TN93 ? al.counts.data() + 4 * r : nullptr,
                                         measure == DST_TN93 ? counts[0].data() + 4 * j : nullptr);
                        }
                        first += m;
                        if (first >= total)
                            break;
                    }
                    {
                        std::lock_guard<std::mutex> lk(wmu);
                        done_text[it.idx] = std::move(text);
                    }
                    wcv.notify_all();
                    return;
                }
                if (closest) {
                    std::vector<TextBuf> text;
                    if (!closest_loaded) {   // the batch's records in stream order, each with its k_used closest loaded records
                        const uint32_t *index = nullptr, *tal = nullptr;
                        uint32_t ku = 0;
                        gpus[g].check(dst_stream_closest_batch(streams[g], &index, &tal, nullptr, &ku), "stream closest batch");
                        text.emplace_back();
                        const Alignment &al = *it.batch;
                        for (size_t r = 0; r < n_rec; ++r)
                            for (size_t e = 0; e < ku; ++e) {
                                const size_t at = r * ku + e, j = index[at];
                                closest_line(text.back(), ref.ids[j], al.ids[r].data(), al.ids[r].size(), tal + at * TW,
                                             measure == DST_TN93 ? al.counts.data() + 4 * r : nullptr,
                                             measure == DST_TN93 ? counts[0].data() + 4 * j : nullptr);
                            }
                    }
                    {
                        std::lock_guard<std::mutex> lk(wmu);
                        done_text[it.idx] = std::move(text);
                    }
                    wcv.notify_all();
                    return;
                }
                Job sj = job;
                sj.square = false;
                sj.swap_ids = true;          // id1 = loaded record, id2 = streamed record (src/lib.rs:327-330)
                sj.rows = it.batch.get();    // streamed record outer ...
                sj.cols = &ref;              // ... loaded record inner (src/lib.rs:323-324)
                sj.row_counts = measure == DST_TN93 ? it.batch->counts.data() : nullptr;
                sj.col_counts = measure == DST_TN93 ? counts[0].data() : nullptr;
                Slab slab;
                slab.rb = 0;
                slab.re = it.batch->n;
                slab.tallies = const_cast<uint32_t *>(static_cast<const uint32_t *>(res));  // library-owned, read only
                format_slab(sj, slab);
                {
                    std::lock_guard<std::mutex> lk(wmu);
                    done_text[it.idx] = std::move(slab.text);
                }
                wcv.notify_all();
            };
            for (;;) {
                Item it;
                bool have = false;
                {
                    std::unique_lock<std::mutex> lk(qmu);
                    qcv.wait(lk, [&] { return !gq[(size_t)g].empty() || gdone[(size_t)g]; });
                    if (!gq[(size_t)g].empty()) {
                        it = std::move(gq[(size_t)g].front());
                        gq[(size_t)g].pop_front();
                        have = true;
                    }
                }
                qcv.notify_all();
                if (!have)
                    break;
                if (inflight.size() == (size_t)kDepth - 1)
                    collect_one();
                uint8_t *buf = nullptr;
                size_t pitch = 0;
                uint32_t *cbuf = nullptr;
                gpus[g].check(dst_stream_acquire(streams[g], &buf, &pitch, &cbuf), "stream acquire");
                const Alignment &al = *it.batch;
                for (size_t r = 0; r < al.n; ++r) {
                    const uint8_t *src = al.codes.data() + r * al.width;
                    uint8_t *dst = buf + r * pitch;
                    if (!nibbles) {
                        std::memcpy(dst, src, al.width);
                        continue;
                    }
                    const size_t half = al.width / 2;
                    for (size_t k = 0; k < half; ++k)   // site 2k in the low nibble, 2k + 1 in the high one
                        dst[k] = (uint8_t)((src[2 * k] >> 4) | (src[2 * k + 1] & 0xF0u));
                    if (al.width & 1)
                        dst[half] = (uint8_t)((src[al.width - 1] >> 4) | 0xF0u);
                }
                if (measure == DST_TN93)
                    std::memcpy(cbuf, al.counts.data(), al.n * 4 * sizeof(uint32_t));
                gpus[g].check(dst_stream_submit(streams[g], al.n, measure == DST_TN93 ? 1 : 0), "stream submit");
                if (closest_loaded) {   // ordinal = position in submission order: keep what the final lines need
                    for (size_t r = 0; r < al.n; ++r) {
                        kept_ids.insert(kept_ids.end(), al.ids[r].begin(), al.ids[r].end());
                        kept_off.push_back(kept_ids.size());
                    }
                    if (measure == DST_TN93)
                        kept_counts.insert(kept_counts.end(), al.counts.begin(), al.counts.end());
                    it.batch.reset();
                }
                inflight.push_back(std::move(it));
            }
            while (!inflight.empty())
                collect_one();
        };
        std::vector<std::thread> workers;
        for (int g = 0; g < G; ++g)
            workers.emplace_back(gpu_stream_worker, g);
        // dispatcher: the reader's batches, in order, to the GPUs
        std::thread dispatcher([&] {
            for (;;) {
                std::unique_ptr<Alignment> batch;
                {
                    std::unique_lock<std::mutex> lk(qmu);
                    qcv.wait(lk, [&] { return !queue.empty() || reader_done; });
                    if (queue.empty())
                        break;
                    batch = std::move(queue.front());
                    queue.pop_front();
                }
                qcv.notify_all();
                // a parsed block may hold more records than one pipeline slot: cut it into batches
                for (size_t r0 = 0; r0 < batch->n; r0 += batch_records) {
                    std::unique_ptr<Alignment> piece;
                    if (r0 == 0 && batch->n <= batch_records) {
                        piece = std::move(batch);
                    } else {
                        const size_t r1 = std::min(batch->n, r0 + batch_records);
                        piece = std::make_unique<Alignment>();
                        piece->n = r1 - r0;
                        piece->width = batch->width;
                        piece->ids.assign(batch->ids.begin() + (long)r0, batch->ids.begin() + (long)r1);
                        piece->codes.assign(batch->codes.begin() + (long)(r0 * batch->width),
                                            batch->codes.begin() + (long)(r1 * batch->width));
                        if (!batch->counts.empty())
                            piece->counts.assign(batch->counts.begin() + (long)(4 * r0), batch->counts.begin() + (long)(4 * r1));
                    }
                    size_t idx;
                    {   // keep the number of batches between dispatch and write bounded (memory)
                        std::unique_lock<std::mutex> lk(wmu);
                        wcv.wait(lk, [&] { return n_batches < next_to_write + window; });
                        idx = n_batches++;
                    }
                    {
                        std::lock_guard<std::mutex> lk(qmu);
                        gq[idx % (size_t)G].push_back(Item{idx, std::move(piece)});
                    }
                    qcv.notify_all();
                    if (!batch)
                        break;
                }
            }
            {
                std::lock_guard<std::mutex> lk(qmu);
                for (int g = 0; g < G; ++g)
                    gdone[(size_t)g] = true;
            }
            qcv.notify_all();
            {
                std::lock_guard<std::mutex> lk(wmu);
                all_dispatched = true;
            }
            wcv.notify_all();
        });
        for (;;) {  // ordered writer
            std::vector<TextBuf> text;
            {
                std::unique_lock<std::mutex> lk(wmu);
                wcv.wait(lk, [&] { return done_text.count(next_to_write) || (all_dispatched && next_to_write >= n_batches); });
                if (!done_text.count(next_to_write))
                    break;
                text = std::move(done_text[next_to_write]);
                done_text.erase(next_to_write);
            }
            for (const TextBuf &part : text)
                wr.write(part.p.get(), part.len);
            {
                std::lock_guard<std::mutex> lk(wmu);
                ++next_to_write;
            }
            wcv.notify_all();
        }
        dispatcher.join();
        for (auto &t : workers)
            t.join();
        if (closest_loaded) {   // every loaded record in input order with its k_used closest streamed records
            const size_t cap = ref.n * std::min<size_t>(a.closest, kept_off.size() - 1);
            std::vector<uint32_t> index(std::max<size_t>(cap, 1)), tal(std::max<size_t>(cap * TW, 1));
            uint32_t ku = 0;
            gpus[0].check(dst_stream_closest_result(streams[0], index.data(), tal.data(), nullptr, cap, &ku), "stream closest result");
            TextBuf out;
            for (size_t i = 0; i < ref.n; ++i) {
                for (size_t e = 0; e < ku; ++e) {
                    const size_t at = i * ku + e, o = index[at];
                    closest_line(out, ref.ids[i], kept_ids.data() + kept_off[o], (size_t)(kept_off[o + 1] - kept_off[o]),
                                 tal.data() + at * TW, measure == DST_TN93 ? kept_counts.data() + 4 * o : nullptr,
                                 measure == DST_TN93 ? counts[0].data() + 4 * i : nullptr);
                }
                if (out.len >= ((size_t)1 << 20)) {
                    wr.write(out.p.get(), out.len);
                    out.len = 0;
                }
            }
            wr.write(out.p.get(), out.len);
        }
        for (int g = 0; g < G; ++g)
            dst_stream_close(streams[g]);
        reader_thread.join();
        if (record_counter == 0)
            die_message("Empty FASTA file");  // src/fastaio.rs:281-283
    }
    timer.mark("compute + format + write");
    wr.flush();
    timer.mark("flush");
    for (auto &g : gpus)
        dst_destroy(g.h);
    timer.mark("destroy contexts");
    if (a.has_output && std::fclose(wr.fh) != 0)
        die_io(a.output, errno);
    // everything is written and closed: leave without the runtime's own teardown (unlocking the page-locked text buffers,
    // unloading the code objects: 0.3 s of a 2 s run that nothing is waiting for)
    leave(0);
}
