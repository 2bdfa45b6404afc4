// The analyses of the loaded sets: one write_* per output mode that is not the long form, and the --groups label file.
#pragma once
#include <cmath>
#include <unordered_map>
#include <unordered_set>

#include "load.hpp"
#include "output.hpp"

namespace {

// what every analysis is given: one GPU with the loaded sets uploaded (slots 0 and 1), the measure, the lines' way out
struct Run {
    const Ctx &gpu;
    const std::vector<Alignment> &loaded;
    Tn93Counts tn93;      // of rows() / cols()
    int measure;
    uint64_t max_pairs;   // Args::analysis_slab()
    Writer &wr;
    bool square() const { return loaded.size() == 1; }
    const Alignment &rows() const { return loaded[0]; }
    const Alignment &cols() const { return loaded.back(); }
    size_t tally_width() const { return (size_t)dst_tally_width(measure); }
    void header(const char *line) const { wr.write(line, std::strlen(line)); }
};

// --nearest: per record of the first file (in input order) its k_used nearest records — of the same file (one input,
// the square) or of the second — from dst_nearest, each line "own id, neighbour id, value" for the canonical pair
void write_nearest(const Run &run, uint32_t k)
{
    const bool square = run.square();
    const Alignment &rows = run.rows(), &cols = run.cols();
    const size_t W = run.tally_width();
    const size_t cap = rows.n * std::min<size_t>(k, square ? (rows.n ? rows.n - 1 : 0) : cols.n);
    std::vector<uint32_t> index(std::max<size_t>(cap, 1)), tallies(std::max<size_t>(cap * W, 1));
    uint32_t ku = 0;
    run.gpu.check(dst_nearest(run.gpu.h, run.measure, square ? 1 : 0, 0, 1, k, index.data(), tallies.data(), nullptr, cap, &ku),
                  "nearest");
    LineWriter out(run.wr);
    for (size_t i = 0; i < rows.n; ++i)
        for (size_t e = 0; e < ku; ++e) {
            const size_t at = i * ku + e, j = index[at];
            const size_t q = square ? std::min(i, j) : i, t = square ? std::max(i, j) : j;
            out.pair_line(rows.ids[i], cols.ids[j], run.measure, &tallies[at * W], run.tn93.row(q), run.tn93.col(t));
            out.end_line();
        }
    out.finish();
}

// --clusters: one line per record in input order, "id, cluster", from dst_clusters' labels (the smallest record of the
// cluster); clusters are numbered from 1 in order of their first record, which is the record its label names.
void write_clusters(const Run &run, double threshold)
{
    const Alignment &set = run.rows();
    std::vector<uint32_t> label(std::max<size_t>(set.n, 1)), number(std::max<size_t>(set.n, 1), 0);
    uint64_t n_clusters = 0, links = 0;
    run.gpu.check(dst_clusters(run.gpu.h, run.measure, threshold, 0, label.data(), set.n, &n_clusters, &links), "clusters");
    run.header("sequence\tcluster\n");
    LineWriter out(run.wr);
    uint32_t next = 0;
    for (size_t i = 0; i < set.n; ++i) {
        if (label[i] == i)
            number[i] = ++next;
        out.put(set.ids[i]);
        out.put('\t');
        out.number(number[label[i]]);
        out.end_line();
    }
    out.finish();
}

// --representatives: one line per record in input order, "id, representative's id, value", from dst_representatives.  A
// member's value is the text the full run prints for the pair (representative, record), from the pair's tallies as
// write_nearest's; a representative names itself and its third field is empty.
void write_representatives(const Run &run, double threshold)
{
    const Alignment &set = run.rows();
    const size_t W = run.tally_width(), cap = std::max<size_t>(set.n, 1);
    std::vector<uint32_t> rep(cap), tallies(cap * W);
    run.gpu.check(dst_representatives(run.gpu.h, run.measure, threshold, run.max_pairs, rep.data(), tallies.data(), nullptr, set.n,
                                      nullptr),
                  "representatives");
    run.header("sequence\trepresentative\tdistance\n");
    LineWriter out(run.wr);
    for (size_t j = 0; j < set.n; ++j) {
        const size_t r = rep[j];
        if (r == j) {
            out.put(set.ids[j]);
            out.put('\t');
            out.put(set.ids[j]);
            out.put('\t');
        } else {
            out.pair_line(set.ids[j], set.ids[r], run.measure, &tallies[j * W], run.tn93.row(r), run.tn93.col(j));
        }
        out.end_line();
    }
    out.finish();
}

// --sites: the fourth field of a --max-distance / --mst line.  The pairs of dst_pair_sites' entries, each "X<pos>Y": pos
// 1-based, X / Y the IUPAC letter of the first / second record's nibble; "." for a pair without listed sites.
// diff_tally: how many entries a pair has, from its DST_OUT_TALLY words (dst_pair_sites' first consequence), which sizes
// the buffers without a counting call.
uint64_t diff_tally(int measure, const uint32_t *t)
{
    return measure == DST_K80 ? (uint64_t)t[1] + t[2] : measure == DST_TN93 ? t[1] : t[0];
}

void put_sites(LineWriter &out, const uint32_t *sites, const uint8_t *bases, uint64_t begin, uint64_t end)
{
    static const char letter[] = "?TCYGKSBAWMHRDVN";   // by nibble: A 8, G 4, C 2, T 1
    if (begin == end)
        out.put('.');
    for (uint64_t k = begin; k < end; ++k) {
        if (k != begin)
            out.put(',');
        out.put(letter[bases[k] >> 4]);
        out.number((uint64_t)sites[k] + 1);
        out.put(letter[bases[k] & 15]);
    }
}

// The lines of pairs (row[e], col[e]), e < n: "id_row, id_col, value" from the pair's tallies, and with --sites their
// sites: dst_pair_sites in batches of DST_PAIR_SITES_BATCH pairs, each batch's buffers sized from the pairs' tallies.
void write_pairs(const Run &run, LineWriter &out, const uint32_t *row, const uint32_t *col, const uint32_t *tallies, uint64_t n,
                 bool with_sites)
{
    const size_t W = run.tally_width();
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> sites;
    std::vector<uint8_t> bases;
    for (uint64_t e0 = 0; e0 < n; e0 += DST_PAIR_SITES_BATCH) {
        const uint64_t m = std::min<uint64_t>(DST_PAIR_SITES_BATCH, n - e0);
        if (with_sites) {
            uint64_t cap = 0, total = 0;
            for (uint64_t e = e0; e < e0 + m; ++e)
                cap += diff_tally(run.measure, tallies + e * W);
            offsets.assign(m + 1, 0);
            sites.resize(std::max<uint64_t>(cap, 1));
            bases.resize(std::max<uint64_t>(cap, 1));
            run.gpu.check(dst_pair_sites(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, row + e0, col + e0, m, offsets.data(),
                                         sites.data(), bases.data(), cap, &total),
                          "pair sites");
        }
        for (uint64_t k = 0; k < m; ++k) {
            const size_t i = row[e0 + k], j = col[e0 + k];
            out.pair_line(run.rows().ids[i], run.cols().ids[j], run.measure, tallies + (e0 + k) * W, run.tn93.row(i),
                          run.tn93.col(j));
            if (with_sites) {
                out.put('\t');
                put_sites(out, sites.data(), bases.data(), offsets[k], offsets[k + 1]);
            }
            out.end_line();
        }
    }
}

// --mst: the edges of dst_mst in its order, each as the line the full run prints for that pair
void write_mst(const Run &run, bool with_sites)
{
    const size_t cap = std::max<size_t>(run.rows().n, 1);
    std::vector<uint32_t> ei(cap), ej(cap), tallies(cap * run.tally_width());
    uint64_t n_edges = 0;
    run.gpu.check(dst_mst(run.gpu.h, run.measure, run.max_pairs, ei.data(), ej.data(), nullptr, tallies.data(), cap, &n_edges,
                          nullptr),
                  "mst");
    LineWriter out(run.wr);
    write_pairs(run, out, ei.data(), ej.data(), tallies.data(), n_edges, with_sites);
    out.finish();
}

// --max-distance: the lines of the full run whose pair is a link of dst_links at T, in its (the full run's) order.  The
// sink formats one chunk of links at a time.  With --sites it only keeps them (row, col, tallies: 12 + 4 W bytes each):
// the context is not re-entrant, so the lines are written, with their sites, after dst_links has returned.
struct LinksSink {
    const Run &run;
    LineWriter out;
    bool keep;
    std::vector<uint32_t> row, col, tallies;
};

int links_sink(void *user, uint64_t, uint64_t n_links, const uint32_t *row, const uint32_t *col, const void *,
               const uint32_t *tallies)
{
    LinksSink &s = *static_cast<LinksSink *>(user);
    if (s.keep) {
        s.row.insert(s.row.end(), row, row + n_links);
        s.col.insert(s.col.end(), col, col + n_links);
        s.tallies.insert(s.tallies.end(), tallies, tallies + n_links * s.run.tally_width());
    } else {
        write_pairs(s.run, s.out, row, col, tallies, n_links, false);
    }
    return 0;
}

void write_links(const Run &run, double threshold, bool with_sites)
{
    LinksSink s{run, LineWriter(run.wr), with_sites, {}, {}, {}};
    run.gpu.check(dst_links(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, threshold, run.max_pairs, DST_LINKS_TALLIES,
                            links_sink, &s, nullptr),
                  "links");
    if (with_sites)
        write_pairs(run, s.out, s.row.data(), s.col.data(), s.tallies.data(), s.row.size(), true);
    s.out.finish();
}

// --pairs: the pair file, read before any input is opened.  One "id1<TAB>id2" per line, empty lines skipped, no header.
struct PairFile {
    std::string path;
    std::vector<std::string> first, second;
    std::vector<size_t> line;   // the line that gave the pair
};

PairFile read_pair_file(const std::string &path)
{
    PairFile pf;
    pf.path = path;
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
        const std::string where = "--pairs: line " + std::to_string(line_no) + " of '" + path + "' ";
        const size_t tab = line.find('\t');
        if (tab == std::string::npos)
            die_message(where + "has no tab: expected 'id1<TAB>id2'");
        if (line.find('\t', tab + 1) != std::string::npos)
            die_message(where + "has more than two fields");
        if (tab == 0 || tab + 1 == line.size())
            die_message(where + "has an empty id");
        pf.first.push_back(line.substr(0, tab));
        pf.second.push_back(line.substr(tab + 1));
        pf.line.push_back(line_no);
    }
    return pf;
}

// ... its ids as records of the inputs (one input: both ids in it; two: id1 in the first, id2 in the second), once the
// inputs are loaded and before the device is looked at
struct PairList {
    std::vector<uint32_t> row, col;
};

PairList resolve_pairs(const PairFile &pf, const std::vector<Alignment> &loaded)
{
    // id -> (its first record, how many records carry it)
    std::vector<std::unordered_map<std::string, std::pair<uint32_t, uint32_t>>> of(loaded.size());
    for (size_t k = 0; k < loaded.size(); ++k)
        for (size_t r = 0; r < loaded[k].n; ++r) {
            const auto ins = of[k].emplace(loaded[k].ids[r], std::make_pair((uint32_t)r, 1u));
            if (!ins.second)
                ++ins.first->second.second;
        }
    const bool two = loaded.size() > 1;
    auto record = [&](const std::string &id, size_t k, size_t line_no) -> uint32_t {
        const std::string where = "--pairs: line " + std::to_string(line_no) + " of '" + pf.path + "' ";
        const char *which = !two ? "" : k == 0 ? "first " : "second ";
        const auto it = of[k].find(id);
        if (it == of[k].end())
            die_message(where + "names '" + id + "', which is not in the " + which + "input");
        if (it->second.second > 1)
            die_message(where + "names '" + id + "', which " + std::to_string(it->second.second) + " records of the " + which +
                        "input carry");
        return it->second.first;
    };
    PairList pl;
    for (size_t e = 0; e < pf.first.size(); ++e) {
        pl.row.push_back(record(pf.first[e], 0, pf.line[e]));
        pl.col.push_back(record(pf.second[e], two ? 1 : 0, pf.line[e]));
    }
    return pl;
}

// --pairs: one line per line of the file, in its order: the two ids as given and the value from the pair's DST_OUT_TALLY
// words (dst_run_pairs), which is the long output's text for that pair; with --sites the fourth field
void write_pair_list(const Run &run, const PairList &pl, bool with_sites)
{
    const uint64_t n = pl.row.size();
    std::vector<uint32_t> tallies(std::max<size_t>(n * run.tally_width(), 1));
    if (n)
        run.gpu.check(dst_run_pairs(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, pl.row.data(), pl.col.data(), n, DST_PAIRS_AUTO,
                                    run.max_pairs, nullptr, tallies.data(), n, nullptr),
                      "run pairs");
    LineWriter out(run.wr);
    write_pairs(run, out, pl.row.data(), pl.col.data(), tallies.data(), n, with_sites);
    out.finish();
}

// a record's "id, within, compared, mean" (without the line's end): --summary's line, and --stream-summary's
void summary_line(LineWriter &out, const std::string &id, uint32_t within, uint32_t summable, double sum)
{
    out.put(id);
    out.put('\t');
    out.number(within);
    out.put('\t');
    out.number(summable);
    out.put('\t');
    out.distance(DST_RAW, summable ? sum / (double)summable : std::nan(""), 0);
}

// --summary: one line per record of the first input in input order, "id, within, compared, mean" from dst_summary: the
// records within T, the partners with a summable distance, and sum / compared printed as an f64 distance (NaN: none)
void write_summary(const Run &run, double threshold)
{
    const Alignment &set = run.rows();
    const size_t cap = std::max<size_t>(set.n, 1);
    std::vector<uint32_t> within(cap), summable(cap);
    std::vector<double> sum(cap);
    run.gpu.check(dst_summary(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, threshold, run.max_pairs, 0, 0.0, nullptr,
                              within.data(), summable.data(), sum.data(), set.n, nullptr),
                  "summary");
    run.header("sequence\twithin\tcompared\tmean\n");
    LineWriter out(run.wr);
    for (size_t i = 0; i < set.n; ++i) {
        summary_line(out, set.ids[i], within[i], summable[i], sum[i]);
        out.end_line();
    }
    out.finish();
}

// --groups: the label file, read before any input is opened.  One "id<TAB>group" per line, empty lines skipped, no header.
struct GroupFile {
    std::string path;
    std::string flag = "--groups";   // the flag the messages name (--window-groups reads the same file)
    std::unordered_map<std::string, std::pair<std::string, size_t>> of;   // id -> (group, the line that set it)
};

GroupFile read_group_file(const std::string &path, const char *flag = "--groups")
{
    GroupFile gf;
    gf.path = path;
    gf.flag = flag;
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
        const std::string where = gf.flag + ": line " + std::to_string(line_no) + " of '" + path + "' ";
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

GroupLabels label_records(const GroupFile &gf, const Alignment &set, const char *which, std::unordered_set<std::string> &seen,
                          size_t max_groups)
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
            if (gl.names.size() == max_groups)
                die_message(gf.flag + ": line " + std::to_string(it->second.second) + " of '" + gf.path + "' starts group " +
                            std::to_string(max_groups + 1) + " of the " + which + " input: more than " +
                            std::to_string(max_groups) + " groups");
            gl.names.push_back(it->second.first);
        }
        gl.label[r] = ins.first->second;
        ++gl.assigned;
    }
    if (gl.assigned == 0)
        die_message(gf.flag + ": no record of the " + std::string(which) + " input has a group in '" + gf.path + "'");
    return gl;
}

// the records' labels, and what can be wrong with them: every input against the one label file
std::vector<GroupLabels> label_inputs(const GroupFile &gf, const std::vector<Alignment> &loaded, size_t max_groups = DST_GROUPS_MAX)
{
    std::vector<GroupLabels> labels;
    std::unordered_set<std::string> seen;
    for (size_t k = 0; k < loaded.size(); ++k)
        labels.push_back(label_records(gf, loaded[k], k == 0 ? "first" : "second", seen, max_groups));
    if (seen.size() < gf.of.size())
        std::fprintf(stderr, "warning: %s: %zu ids of '%s' are not in the input and were skipped\n", gf.flag.c_str(),
                     gf.of.size() - seen.size(), gf.path.c_str());
    return labels;
}

// --stream-groups: the label file against the loaded set, before the device is looked at.  The streamed records meet the
// file batch by batch (stream.hpp); `seen` collects the ids of the file that either side carries.
struct StreamGroups {
    const GroupFile *file = nullptr;
    GroupLabels loaded;                        // by loaded: no labels, one group
    std::unordered_set<std::string> seen;
};

StreamGroups label_loaded_for_stream(const GroupFile &gf, const Alignment &set, int by)
{
    StreamGroups sg;
    sg.file = &gf;
    if (by != 2) {
        sg.loaded = label_records(gf, set, "loaded", sg.seen, DST_GROUPS_MAX);
        return sg;
    }
    for (size_t r = 0; r < set.n; ++r)
        if (gf.of.count(set.ids[r]))
            sg.seen.insert(set.ids[r]);
    return sg;
}

// The fields --groups and --window-groups print behind the names of a line, each with its tab in front.
// a cell: pairs, compared, [within,] mean, min, max
void put_group_cell(LineWriter &out, int measure, const dst_group_cell &c, bool has_within)
{
    const bool int_payload = measure == DST_N || measure == DST_N_HIGH;
    auto tab_number = [&](uint64_t v) {
        out.put('\t');
        out.number(v);
    };
    auto tab_distance = [&](int m, bool known, double v, int64_t iv) {
        out.put('\t');
        if (known)
            out.distance(m, v, iv);
        else
            out.put("NaN");
    };
    tab_number(c.pairs);
    tab_number(c.summable_pairs);
    if (has_within)
        tab_number(c.links);
    tab_distance(DST_RAW, c.summable_pairs != 0, c.summable_pairs ? c.sum / (double)c.summable_pairs : 0.0, 0);
    const bool known = c.pairs > c.nan_pairs;   // a pair whose payload is not NaN
    for (const uint64_t bits : {c.min_bits, c.max_bits}) {
        double v = 0;
        std::memcpy(&v, &bits, 8);
        tab_distance(measure, known, int_payload ? 0.0 : v, int_payload ? (int64_t)bits : 0);
    }
}

// a record's entry for one group: compared, [within,] mean
void put_group_record(LineWriter &out, uint32_t summable, uint32_t within, double sum, bool has_within)
{
    out.put('\t');
    out.number(summable);
    if (has_within) {
        out.put('\t');
        out.number(within);
    }
    out.put('\t');
    if (summable)
        out.distance(DST_RAW, sum / (double)summable, 0);
    else
        out.put("NaN");
}

// --groups: one line per cell (one input: a <= b; two: every cell), or with --per-record one line per record of the first
// input and group of the other side, from dst_group_summary.  mean = sum / compared as --summary prints its mean.
void write_groups(const Run &run, const std::vector<GroupLabels> &labels, bool has_within, double threshold, bool per_record)
{
    const bool square = run.square();
    const GroupLabels &rl = labels[0], &cl = labels.back();
    const uint32_t Gr = (uint32_t)rl.names.size(), Gc = (uint32_t)cl.names.size();
    const size_t n_rows = run.rows().n;
    std::vector<dst_group_cell> cells(per_record ? 0 : (size_t)Gr * Gc);
    std::vector<uint32_t> within(per_record ? n_rows * Gc : 0), summable(per_record ? n_rows * Gc : 0);
    std::vector<double> sum(per_record ? n_rows * Gc : 0);
    run.gpu.check(dst_group_summary(run.gpu.h, run.measure, square ? 1 : 0, 0, 1, rl.label.data(), Gr, cl.label.data(), Gc,
                                    has_within ? threshold : HUGE_VAL, run.max_pairs, per_record ? nullptr : cells.data(),
                                    cells.size(), per_record ? within.data() : nullptr, per_record ? summable.data() : nullptr,
                                    per_record ? sum.data() : nullptr, sum.size()),
                  "group summary");
    LineWriter out(run.wr);
    out.put(per_record ? "sequence\tgroup\tcompared" : "group1\tgroup2\tpairs\tcompared");
    if (has_within)
        out.put("\twithin");
    out.put(per_record ? "\tmean" : "\tmean\tmin\tmax");
    out.end_line();
    if (per_record) {
        for (size_t x = 0; x < n_rows; ++x)
            for (uint32_t g = 0; g < Gc; ++g) {
                const size_t e = x * Gc + g;
                out.put(run.rows().ids[x]);
                out.put('\t');
                out.put(cl.names[g]);
                put_group_record(out, summable[e], within[e], sum[e], has_within);
                out.end_line();
            }
    } else {
        for (uint32_t a = 0; a < Gr; ++a)
            for (uint32_t b = square ? a : 0; b < Gc; ++b) {
                const dst_group_cell &c = cells[(size_t)a * Gc + b];
                out.put(rl.names[a]);
                out.put('\t');
                out.put(cl.names[b]);
                put_group_cell(out, run.measure, c, has_within);
                out.end_line();
            }
    }
    out.finish();
}

// a histogram's lines behind the header: --histogram's, and --stream-histogram's
void histogram_lines(Writer &wr, int measure, double width, const std::vector<uint64_t> &hist, uint64_t nan_pairs)
{
    LineWriter out(wr);
    for (size_t b = 0; b < hist.size(); ++b) {
        out.distance(measure, (double)b * width, (int64_t)b * (int64_t)width);
        out.put('\t');
        out.number(hist[b]);
        out.end_line();
    }
    out.put("NaN\t");
    out.number(nan_pairs);
    out.end_line();
    out.finish();
}

// --histogram: one line per bin, "lower edge, pairs" (the edge b W as the measure's distances are printed; the last bin is
// open-ended), then "NaN, pairs without a distance"
void write_histogram(const Run &run, double width, uint32_t bins)
{
    std::vector<uint64_t> hist(bins);
    dst_summary_totals totals;
    run.gpu.check(dst_summary(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, 0.0, run.max_pairs, bins, width, hist.data(),
                              nullptr, nullptr, nullptr, 0, &totals),
                  "histogram");
    run.header("distance\tpairs\n");
    histogram_lines(run.wr, run.measure, width, hist, totals.nan_pairs);
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

// every id of a set in one arena with its offsets, as the library's id and Newick calls take them
struct IdArena {
    std::string chars;
    std::vector<uint64_t> offsets;
    explicit IdArena(const Alignment &set) : offsets(set.n + 1, 0)
    {
        for (size_t r = 0; r < set.n; ++r) {
            chars += set.ids[r];
            offsets[r + 1] = chars.size();
        }
    }
};

// one Newick line: `newick(buffer, capacity, &length)` is asked for the length first, then for the text
template <class Newick>
void write_newick(Writer &wr, Newick newick)
{
    size_t len = 0;
    newick(nullptr, 0, &len);
    std::string out(len, '\0');
    if (newick(out.data(), out.size(), &len) != DST_OK) {
        std::fprintf(stderr, "error: the Newick text of the tree could not be written\n");
        leave(1);
    }
    wr.write(out.data(), len);
}

// --tree nj: the neighbour-joining tree of one set as one Newick line (dst_nj on the GPU, dst_newick on the host);
// with --bootstrap B its internal nodes carry their support in B replicates (dst_nj_bootstrap, dst_newick_support),
// and nothing is written unless every replicate succeeded
void write_tree(const Run &run, uint32_t bootstrap, uint64_t seed)
{
    const Ctx &gpu = run.gpu;
    const Alignment &set = run.rows();
    if (set.n < 3) {
        std::fprintf(stderr, "error: a neighbour-joining tree needs at least 3 records, the input has %zu\n", (size_t)set.n);
        leave(1);
    }
    std::vector<uint32_t> parent(2 * set.n - 2);
    std::vector<double> length(2 * set.n - 2);
    int rc = dst_nj(gpu.h, run.measure, run.max_pairs, parent.data(), length.data(), parent.size());
    if (rc == DST_ERR_STATE && non_finite_pair(gpu, set, "", ": no neighbour-joining tree"))
        leave(1);
    gpu.check(rc, "neighbour joining");
    std::vector<uint32_t> support;
    if (bootstrap) {
        support.resize(parent.size());
        rc = dst_nj_bootstrap(gpu.h, run.measure, set.codes.data(), set.n, set.width, set.width, bootstrap, seed, run.max_pairs,
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
    const IdArena ids(set);
    const uint32_t *sup = bootstrap ? support.data() : nullptr;
    write_newick(run.wr, [&](char *buf, size_t cap, size_t *len) {
        return dst_newick_support(set.n, parent.data(), length.data(), ids.chars.data(), ids.offsets.data(), sup, buf, cap, len);
    });
}

// --dendrogram: the UPGMA / WPGMA / complete-linkage tree of one set as one Newick line with a binary root
// (dst_dendrogram on the GPU, dst_newick_rooted on the host)
void write_dendrogram(const Run &run, int linkage)
{
    const Alignment &set = run.rows();
    if (set.n < 2) {
        std::fprintf(stderr, "error: a dendrogram needs at least 2 records, the input has %zu\n", (size_t)set.n);
        leave(1);
    }
    std::vector<uint32_t> parent(2 * set.n - 1);
    std::vector<double> length(2 * set.n - 1);
    const int rc = dst_dendrogram(run.gpu.h, run.measure, linkage, run.max_pairs, parent.data(), length.data(), nullptr,
                                  parent.size(), nullptr);
    if (rc == DST_ERR_STATE && non_finite_pair(run.gpu, set, "", ": no dendrogram"))
        leave(1);
    run.gpu.check(rc, "dendrogram");
    const IdArena ids(set);
    write_newick(run.wr, [&](char *buf, size_t cap, size_t *len) {
        return dst_newick_rooted(set.n, parent.data(), length.data(), ids.chars.data(), ids.offsets.data(), buf, cap, len);
    });
}

// --windows / --regions: the column windows [begin, end) of the run, 0-based and half-open as dst_run_windows takes them,
// and the name each line carries (--windows: the window's 1-based ordinal)
struct WindowList {
    std::string path;   // --regions FILE
    std::vector<uint64_t> begin, end;
    std::vector<std::string> names;
    std::vector<size_t> line;   // --regions: the line that gave the region
};

// --regions: the file, read before any input is opened.  One "name<TAB>start<TAB>end" per line (1-based, inclusive), empty
// lines skipped, no header.
WindowList read_region_file(const std::string &path)
{
    WindowList wl;
    wl.path = path;
    FILE *fh = open_input(path);
    std::string text;
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, fh)) > 0;)
        text.append(buf, got);
    std::fclose(fh);
    auto position = [](const std::string &v, uint64_t &out) {
        if (v.empty() || v.size() > 19 || v.find_first_not_of("0123456789") != std::string::npos)
            return false;
        out = std::strtoull(v.c_str(), nullptr, 10);
        return true;
    };
    size_t line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t stop = text.find('\n', at);
        if (stop == std::string::npos)
            stop = text.size();
        std::string line = text.substr(at, stop - at);
        at = stop + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r')
            line.pop_back();
        if (line.empty())
            continue;
        const std::string where = "--regions: line " + std::to_string(line_no) + " of '" + path + "' ";
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos)
            die_message(where + "has fewer than three fields: expected 'name<TAB>start<TAB>end'");
        if (line.find('\t', t2 + 1) != std::string::npos)
            die_message(where + "has more than three fields");
        if (t1 == 0)
            die_message(where + "has an empty name");
        uint64_t first = 0, last = 0;
        if (!position(line.substr(t1 + 1, t2 - t1 - 1), first) || !position(line.substr(t2 + 1), last))
            die_message(where + "has a start or an end that is not a whole number");
        if (first < 1 || first > last)
            die_message(where + "must have 1 <= start <= end");
        if (wl.begin.size() == DST_WINDOWS_MAX)
            die_message(where + "starts region " + std::to_string(DST_WINDOWS_MAX + 1) + ": more than " +
                        std::to_string(DST_WINDOWS_MAX) + " regions");
        wl.names.push_back(line.substr(0, t1));
        wl.begin.push_back(first - 1);
        wl.end.push_back(last);
        wl.line.push_back(line_no);
    }
    if (wl.begin.empty())
        die_message("--regions: '" + path + "' names no region");
    return wl;
}

// ... against the alignment's width, once the inputs are loaded and before the device is looked at
void check_regions(const WindowList &wl, size_t width)
{
    for (size_t w = 0; w < wl.begin.size(); ++w)
        if (wl.end[w] > width)
            die_message("--regions: line " + std::to_string(wl.line[w]) + " of '" + wl.path + "' ends at " +
                        std::to_string(wl.end[w]) + ", past the alignment's " + std::to_string(width) + " sites");
}

// --windows W --step S over an alignment of `width` sites (dst_sliding_windows)
WindowList sliding_windows(size_t width, size_t window, size_t step)
{
    WindowList wl;
    uint32_t count = 0;
    if (dst_sliding_windows(width, window, step, nullptr, nullptr, 0, &count) != DST_OK)
        die_message("--windows: " + std::to_string(count) + (count == 0xFFFFFFFFu ? " or more" : "") + " windows, more than " +
                    std::to_string(DST_WINDOWS_MAX));
    wl.begin.resize(count);
    wl.end.resize(count);
    if (count)
        dst_sliding_windows(width, window, step, wl.begin.data(), wl.end.data(), count, &count);
    for (uint32_t w = 0; w < count; ++w)
        wl.names.push_back(std::to_string(w + 1));
    return wl;
}

// --windows / --regions: per pair in canonical order and per window in the given order one line "id1, id2, window, start,
// end, value": the value from the pair's DST_OUT_TALLY words in the window (dst_run_windows) and, for tn93, the two
// records' base counts inside it (dst_window_base_counts), through dst_finalize and the long output's formatter.  Rows are
// walked in ranges whose pair-windows stay within max_entries (at least one row each).
void write_windows(const Run &run, const WindowList &wl, uint64_t max_entries)
{
    const bool square = run.square();
    const Alignment &rows = run.rows(), &cols = run.cols();
    const size_t W = run.tally_width(), nw = wl.begin.size();
    run.header("sequence1\tsequence2\twindow\tstart\tend\tdistance\n");
    if (nw == 0)
        return;
    std::vector<uint32_t> row_counts, col_counts;
    if (run.measure == DST_TN93) {
        row_counts.resize(nw * rows.n * 4);
        run.gpu.check(dst_window_base_counts(run.gpu.h, 0, wl.begin.data(), wl.end.data(), (uint32_t)nw, row_counts.data(),
                                             row_counts.size()),
                      "window base counts");
        if (!square) {
            col_counts.resize(nw * cols.n * 4);
            run.gpu.check(dst_window_base_counts(run.gpu.h, 1, wl.begin.data(), wl.end.data(), (uint32_t)nw, col_counts.data(),
                                                 col_counts.size()),
                          "window base counts");
        }
    }
    const std::vector<uint32_t> &ccounts = square ? row_counts : col_counts;
    auto pairs_of_row = [&](size_t i) -> uint64_t { return square ? rows.n - 1 - i : cols.n; };
    std::vector<uint32_t> tallies;
    LineWriter out(run.wr);
    for (size_t rb = 0; rb < rows.n;) {
        uint64_t P = pairs_of_row(rb);
        size_t re = rb + 1;
        while (re < rows.n && (P + pairs_of_row(re)) * nw <= max_entries)
            P += pairs_of_row(re++);
        if (P) {
            tallies.resize((size_t)P * nw * W);
            run.gpu.check(dst_run_windows_host(run.gpu.h, run.measure, square ? 1 : 0, 0, 1, rb, re, wl.begin.data(), wl.end.data(),
                                               (uint32_t)nw, DST_OUT_TALLY, tallies.data(), tallies.size() * sizeof(uint32_t)),
                          "windows");
        }
        uint64_t p = 0;
        for (size_t i = rb; i < re; ++i)
            for (size_t j = square ? i + 1 : 0; j < cols.n; ++j, ++p)
                for (size_t w = 0; w < nw; ++w) {
                    double f = 0;
                    int64_t iv = 0;
                    dst_finalize(run.measure, &tallies[((size_t)w * P + p) * W],
                                 row_counts.empty() ? nullptr : &row_counts[(w * rows.n + i) * 4],
                                 ccounts.empty() ? nullptr : &ccounts[(w * cols.n + j) * 4], &f, &iv);
                    out.put(rows.ids[i]);
                    out.put('\t');
                    out.put(cols.ids[j]);
                    out.put('\t');
                    out.put(wl.names[w]);
                    out.put('\t');
                    out.number(wl.begin[w] + 1);
                    out.put('\t');
                    out.number(wl.end[w]);
                    out.put('\t');
                    out.distance(run.measure, f, iv);
                    out.end_line();
                }
        rb = re;
    }
    out.finish();
}

// --window-nearest K: per record of the first input in input order and per window in the given order the K nearest
// records of the other side (dst_nearest_windows), each as the line the plain --windows / --regions run prints for that pair
// and window: the value from the entry's DST_OUT_TALLY words and, for tn93, the two records' base counts inside the window,
// through dst_finalize and the long output's formatter.  A square run's neighbour j < i is the canonical pair (j, i): the
// two ids and the two records' counts change places.  Rows are walked in ranges of at most 2^24 result entries (at least
// one row each); max_entries is the library's device slab.
void write_window_nearest(const Run &run, const WindowList &wl, uint32_t k, uint64_t max_entries)
{
    const bool square = run.square();
    const Alignment &rows = run.rows(), &cols = run.cols();
    const size_t W = run.tally_width(), nw = wl.begin.size();
    run.header("sequence1\tsequence2\twindow\tstart\tend\tdistance\n");
    if (nw == 0 || rows.n == 0)
        return;
    std::vector<uint32_t> row_counts, col_counts;
    if (run.measure == DST_TN93) {
        row_counts.resize(nw * rows.n * 4);
        run.gpu.check(dst_window_base_counts(run.gpu.h, 0, wl.begin.data(), wl.end.data(), (uint32_t)nw, row_counts.data(),
                                             row_counts.size()),
                      "window base counts");
        if (!square) {
            col_counts.resize(nw * cols.n * 4);
            run.gpu.check(dst_window_base_counts(run.gpu.h, 1, wl.begin.data(), wl.end.data(), (uint32_t)nw, col_counts.data(),
                                                 col_counts.size()),
                          "window base counts");
        }
    }
    const std::vector<uint32_t> &ccounts = square ? row_counts : col_counts;
    const size_t candidates = square ? cols.n - 1 : cols.n;
    const size_t ku = std::min<size_t>(k, candidates);
    if (ku == 0)
        return;
    const size_t rows_per_call = std::max<size_t>(((size_t)1 << 24) / (nw * ku), 1);
    std::vector<uint32_t> index, tallies;
    LineWriter out(run.wr);
    for (size_t rb = 0; rb < rows.n; rb += rows_per_call) {
        const size_t re = std::min(rows.n, rb + rows_per_call), entries = (re - rb) * nw * ku;
        index.resize(entries);
        tallies.resize(entries * W);
        uint32_t k_used = 0;
        run.gpu.check(dst_nearest_windows(run.gpu.h, run.measure, square ? 1 : 0, 0, 1, rb, re, wl.begin.data(), wl.end.data(),
                                          (uint32_t)nw, k, max_entries, index.data(), tallies.data(), nullptr, entries, &k_used),
                      "window nearest");
        size_t e = 0;
        for (size_t i = rb; i < re; ++i)
            for (size_t w = 0; w < nw; ++w)
                for (size_t r = 0; r < ku; ++r, ++e) {
                    const size_t j = index[e];
                    const bool swapped = square && j < i;   // the canonical pair comes first record first
                    const uint32_t *ic = row_counts.empty() ? nullptr : &row_counts[(w * rows.n + i) * 4];
                    const uint32_t *jc = ccounts.empty() ? nullptr : &ccounts[(w * cols.n + j) * 4];
                    double f = 0;
                    int64_t iv = 0;
                    dst_finalize(run.measure, &tallies[e * W], swapped ? jc : ic, swapped ? ic : jc, &f, &iv);
                    out.put(swapped ? cols.ids[j] : rows.ids[i]);
                    out.put('\t');
                    out.put(swapped ? rows.ids[i] : cols.ids[j]);
                    out.put('\t');
                    out.put(wl.names[w]);
                    out.put('\t');
                    out.number(wl.begin[w] + 1);
                    out.put('\t');
                    out.number(wl.end[w]);
                    out.put('\t');
                    out.distance(run.measure, f, iv);
                    out.end_line();
                }
    }
    out.finish();
}

// --window-summary T: dst_window_summary's counts and means, the mean (sum / compared) printed as --summary prints its own
// (NaN: nothing compared).  By window: one line per window in the given order, "window, start, end, pairs, compared,
// within, mean" from the windows' totals alone.  By record: for every record of the first input in input order one line per
// window, "sequence, window, start, end, within, compared, mean".  The first three window fields are the plain --windows /
// --regions run's.
void write_window_summary(const Run &run, const WindowList &wl, double threshold, bool by_record)
{
    const Alignment &rows = run.rows();
    const size_t nw = wl.begin.size();
    run.header(by_record ? "sequence\twindow\tstart\tend\twithin\tcompared\tmean\n"
                         : "window\tstart\tend\tpairs\tcompared\twithin\tmean\n");
    if (nw == 0)
        return;
    const size_t entries = by_record ? nw * rows.n : 0, cap = std::max<size_t>(entries, 1);
    std::vector<dst_summary_totals> totals(by_record ? 0 : nw);
    std::vector<uint32_t> within(by_record ? cap : 0), summable(by_record ? cap : 0);
    std::vector<double> sum(by_record ? cap : 0);
    run.gpu.check(dst_window_summary(run.gpu.h, run.measure, run.square() ? 1 : 0, 0, 1, wl.begin.data(), wl.end.data(), (uint32_t)nw,
                                     threshold, by_record ? nullptr : totals.data(), by_record ? within.data() : nullptr,
                                     by_record ? summable.data() : nullptr, by_record ? sum.data() : nullptr, entries),
                  "window summary");
    LineWriter out(run.wr);
    auto window_fields = [&](size_t w) {
        out.put(wl.names[w]);
        out.put('\t');
        out.number(wl.begin[w] + 1);
        out.put('\t');
        out.number(wl.end[w]);
        out.put('\t');
    };
    auto mean = [&](double s, uint64_t compared) {
        out.distance(DST_RAW, compared ? s / (double)compared : std::nan(""), 0);
        out.end_line();
    };
    if (!by_record) {
        for (size_t w = 0; w < nw; ++w) {
            window_fields(w);
            out.number(totals[w].pairs);
            out.put('\t');
            out.number(totals[w].summable_pairs);
            out.put('\t');
            out.number(totals[w].links);
            out.put('\t');
            mean(totals[w].sum, totals[w].summable_pairs);
        }
    } else {
        for (size_t i = 0; i < rows.n; ++i)
            for (size_t w = 0; w < nw; ++w) {
                const size_t e = w * rows.n + i;
                out.put(rows.ids[i]);
                out.put('\t');
                window_fields(w);
                out.number(within[e]);
                out.put('\t');
                out.number(summable[e]);
                out.put('\t');
                mean(sum[e], summable[e]);
            }
    }
    out.finish();
}

// --window-groups FILE: --groups' lines per window, from dst_window_group_summary.  By cell: per window in the given order
// "window, start, end" and then what --groups prints for the cell (one input: a <= b; two: every cell).  By record: for
// every record of the first input and every window one line per group of the other side, "sequence, window, start, end"
// and then what --groups --per-record prints.  The window fields are the plain --windows / --regions run's.
void write_window_groups(const Run &run, const WindowList &wl, const std::vector<GroupLabels> &labels, bool has_within,
                         double threshold, bool by_record)
{
    const bool square = run.square();
    const GroupLabels &rl = labels[0], &cl = labels.back();
    const uint32_t Gr = (uint32_t)rl.names.size(), Gc = (uint32_t)cl.names.size();
    const Alignment &rows = run.rows();
    const size_t nw = wl.begin.size();
    LineWriter out(run.wr);
    out.put(by_record ? "sequence\twindow\tstart\tend\tgroup\tcompared" : "window\tstart\tend\tgroup1\tgroup2\tpairs\tcompared");
    if (has_within)
        out.put("\twithin");
    out.put(by_record ? "\tmean" : "\tmean\tmin\tmax");
    out.end_line();
    if (nw == 0) {
        out.finish();
        return;
    }
    const size_t entries = by_record ? nw * rows.n * Gc : 0, cap = std::max<size_t>(entries, 1);
    std::vector<dst_group_cell> cells(by_record ? 0 : nw * Gr * Gc);
    std::vector<uint32_t> within(by_record ? cap : 0), summable(by_record ? cap : 0);
    std::vector<double> sum(by_record ? cap : 0);
    run.gpu.check(dst_window_group_summary(run.gpu.h, run.measure, square ? 1 : 0, 0, 1, wl.begin.data(), wl.end.data(),
                                           (uint32_t)nw, rl.label.data(), Gr, cl.label.data(), Gc,
                                           has_within ? threshold : HUGE_VAL, by_record ? nullptr : cells.data(), cells.size(),
                                           by_record ? within.data() : nullptr, by_record ? summable.data() : nullptr,
                                           by_record ? sum.data() : nullptr, entries),
                  "window group summary");
    auto window_fields = [&](size_t w) {
        out.put(wl.names[w]);
        out.put('\t');
        out.number(wl.begin[w] + 1);
        out.put('\t');
        out.number(wl.end[w]);
        out.put('\t');
    };
    if (by_record) {
        for (size_t x = 0; x < rows.n; ++x)
            for (size_t w = 0; w < nw; ++w)
                for (uint32_t g = 0; g < Gc; ++g) {
                    const size_t e = (w * rows.n + x) * Gc + g;
                    out.put(rows.ids[x]);
                    out.put('\t');
                    window_fields(w);
                    out.put(cl.names[g]);
                    put_group_record(out, summable[e], within[e], sum[e], has_within);
                    out.end_line();
                }
    } else {
        for (size_t w = 0; w < nw; ++w)
            for (uint32_t a = 0; a < Gr; ++a)
                for (uint32_t b = square ? a : 0; b < Gc; ++b) {
                    window_fields(w);
                    out.put(rl.names[a]);
                    out.put('\t');
                    out.put(cl.names[b]);
                    put_group_cell(out, run.measure, cells[(w * Gr + a) * Gc + b], has_within);
                    out.end_line();
                }
    }
    out.finish();
}

// --site-counts / --window-site-stats: the per-site allele counts of the one input (dst_site_counts), walked in ranges of
// sites of at most 2^26 entries.  `labels` is empty without --site-groups: one group, "all", of every record.
struct SiteGroups {
    const uint32_t *label = nullptr;
    uint32_t count = 1;
    std::vector<std::string> names{"all"};
    std::vector<uint64_t> size;
};

SiteGroups site_groups(const Run &run, const std::vector<GroupLabels> &labels)
{
    SiteGroups sg;
    if (labels.empty()) {
        sg.size.assign(1, run.rows().n);
        return sg;
    }
    const GroupLabels &gl = labels[0];
    sg.label = gl.label.data();
    sg.count = (uint32_t)gl.names.size();
    sg.names = gl.names;
    sg.size.assign(sg.count, 0);
    for (const uint32_t g : gl.label)
        if (g != DST_GROUP_NONE)
            ++sg.size[g];
    return sg;
}

constexpr size_t kSiteRangeEntries = (size_t)1 << 26;

// the most entries of one range; DISTANCE_SITE_RANGE_ENTRIES makes it smaller (the tests walk a small input in many ranges)
size_t site_range_entries()
{
    const char *env = std::getenv("DISTANCE_SITE_RANGE_ENTRIES");
    const size_t asked = env ? (size_t)std::strtoull(env, nullptr, 10) : 0;
    return asked ? std::min(asked, kSiteRangeEntries) : kSiteRangeEntries;
}

// the counts of sites [begin, end), in ranges: sink(first site of the range, sites, the range's entries)
template <typename Sink>
void walk_site_counts(const Run &run, const SiteGroups &sg, uint64_t begin, uint64_t end, Sink &&sink)
{
    const size_t per_site = (size_t)sg.count * DST_SITE_CLASSES;
    const uint64_t sites_per_range = std::max<uint64_t>(1, site_range_entries() / per_site);
    std::vector<uint32_t> counts((size_t)std::min<uint64_t>(sites_per_range, end - begin) * per_site);
    for (uint64_t s = begin; s < end; s += sites_per_range) {
        const uint64_t e = std::min(end, s + sites_per_range);
        run.gpu.check(dst_site_counts(run.gpu.h, 0, sg.label, sg.count, s, e, counts.data(), counts.size()), "site counts");
        sink(s, e - s, counts.data());
    }
}

// --site-counts: "site, group, records, A, C, G, T, ambiguous, missing", one line per site (1-based) and group in group order
void write_site_counts(const Run &run, const std::vector<GroupLabels> &labels)
{
    const SiteGroups sg = site_groups(run, labels);
    run.header("site\tgroup\trecords\tA\tC\tG\tT\tambiguous\tmissing\n");
    LineWriter out(run.wr);
    walk_site_counts(run, sg, 0, run.rows().width, [&](uint64_t first, uint64_t sites, const uint32_t *counts) {
        for (uint64_t s = 0; s < sites; ++s)
            for (uint32_t g = 0; g < sg.count; ++g) {
                const uint32_t *c = counts + (s * sg.count + g) * DST_SITE_CLASSES;   // A, T, G, C, ambiguous
                out.number(first + s + 1);
                out.put('\t');
                out.put(sg.names[g]);
                for (const uint64_t v : {sg.size[g], (uint64_t)c[0], (uint64_t)c[3], (uint64_t)c[2], (uint64_t)c[1], (uint64_t)c[4],
                                         sg.size[g] - c[0] - c[1] - c[2] - c[3] - c[4]}) {
                    out.put('\t');
                    out.number(v);
                }
                out.end_line();
            }
    });
    out.finish();
}

// --window-site-stats: per window and group "window, start, end, group, records, sites, called, segregating, theta_w, pi" from
// dst_site_stats; the two means (over the called sites) printed as --summary prints its mean, NaN when no site is called.
// The window fields are the plain --windows / --regions run's.  The counts are walked in ranges of sites; a range's counts
// serve the windows that lie inside it, and a window that crosses a range's end is counted on its own.
void write_window_site_stats(const Run &run, const WindowList &wl, const std::vector<GroupLabels> &labels)
{
    const SiteGroups sg = site_groups(run, labels);
    const size_t nw = wl.begin.size(), G = sg.count;
    run.header("window\tstart\tend\tgroup\trecords\tsites\tcalled\tsegregating\ttheta_w\tpi\n");
    if (nw == 0)
        return;
    std::vector<dst_site_window> stats(nw * G);
    std::vector<char> done(nw, 0);
    auto reduce = [&](size_t w, uint64_t first, uint64_t sites, const uint32_t *counts) {
        if (dst_site_stats(counts, first, first + sites, sg.count, &wl.begin[w], &wl.end[w], 1, sg.size.data(), &stats[w * G], G) != DST_OK)
            die_message("site stats: window " + wl.names[w] + " does not lie inside the counted sites");
        done[w] = 1;
    };
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t w = 0; w < nw; ++w) {
        lo = std::min<uint64_t>(lo, wl.begin[w]);
        hi = std::max<uint64_t>(hi, wl.end[w]);
    }
    walk_site_counts(run, sg, lo, std::max(lo, hi), [&](uint64_t first, uint64_t sites, const uint32_t *counts) {
        for (size_t w = 0; w < nw; ++w)
            if (!done[w] && wl.begin[w] >= first && wl.end[w] <= first + sites)
                reduce(w, first, sites, counts);
    });
    for (size_t w = 0; w < nw; ++w) {
        if (done[w])
            continue;
        if (wl.begin[w] == wl.end[w]) {   // (an empty window outside every range: nothing to count)
            uint32_t none = 0;
            reduce(w, wl.begin[w], 0, &none);
            continue;
        }
        // a window across a range's end: its own sites, counted in ranges again and reduced as one piece (the sums are
        // taken in site order over the whole window)
        std::vector<uint32_t> whole;
        walk_site_counts(run, sg, wl.begin[w], wl.end[w], [&](uint64_t, uint64_t sites, const uint32_t *counts) {
            whole.insert(whole.end(), counts, counts + sites * G * DST_SITE_CLASSES);
        });
        reduce(w, wl.begin[w], wl.end[w] - wl.begin[w], whole.data());
    }
    LineWriter out(run.wr);
    for (size_t w = 0; w < nw; ++w)
        for (size_t g = 0; g < G; ++g) {
            const dst_site_window &r = stats[w * G + g];
            out.put(wl.names[w]);
            out.put('\t');
            out.number(wl.begin[w] + 1);
            out.put('\t');
            out.number(wl.end[w]);
            out.put('\t');
            out.put(sg.names[g]);
            for (const uint64_t v : {r.records, r.sites, r.called, r.segregating}) {
                out.put('\t');
                out.number(v);
            }
            for (const double s : {r.theta_sum, r.pi_sum}) {
                out.put('\t');
                out.distance(DST_RAW, r.called ? s / (double)r.called : std::nan(""), 0);
            }
            out.end_line();
        }
    out.finish();
}

// --ld: "site1, site2, group, major1, major2, called, minor1, minor2, both, r2, D, Dprime", one line per link of
// dst_site_ld_links at R2, per group in canonical order.  A group lists the sites whose major base and whose other bases
// together are each held by at least min_count of its records (walk_site_counts + dst_site_major), with the major base as
// the reference allele.  The three doubles come from dst_ld_finalize, printed as --summary prints its mean.
struct LdSink {
    LineWriter &out;
    const std::string &group;
    const std::vector<uint32_t> &sites;
    const std::vector<uint8_t> &allele;
    std::vector<double> r2, d, dprime;
};

int ld_sink(void *user, uint64_t, uint64_t n_links, const uint32_t *pos_i, const uint32_t *pos_j, const uint32_t *tallies)
{
    LdSink &s = *static_cast<LdSink *>(user);
    s.r2.resize(n_links), s.d.resize(n_links), s.dprime.resize(n_links);
    if (dst_ld_finalize(tallies, n_links, s.r2.data(), s.d.data(), s.dprime.data()) != DST_OK)
        return 1;
    for (uint64_t e = 0; e < n_links; ++e) {
        s.out.number((uint64_t)s.sites[pos_i[e]] + 1);
        s.out.put('\t');
        s.out.number((uint64_t)s.sites[pos_j[e]] + 1);
        s.out.put('\t');
        s.out.put(s.group);
        for (const uint32_t p : {pos_i[e], pos_j[e]}) {
            s.out.put('\t');
            s.out.put("ATGC"[s.allele[p]]);   // (the library's class order)
        }
        for (int k = 0; k < 4; ++k) {
            s.out.put('\t');
            s.out.number(tallies[4 * e + k]);
        }
        for (const double v : {s.r2[e], s.d[e], s.dprime[e]}) {
            s.out.put('\t');
            s.out.distance(DST_RAW, v, 0);
        }
        s.out.end_line();
    }
    return 0;
}

// --ld-max-gap G: the same lines from dst_site_ld_links_band.  --ld-decay W --ld-bins B: "group, gap, pairs, defined, linked,
// mean_r2", one line per group and bin of dst_site_ld_decay in group and then bin order; gap = the bin's lower edge b x W;
// mean_r2 = r2_sum / defined, printed as --summary prints its mean (NaN without a defined pair).
void write_ld(const Run &run, const std::vector<GroupLabels> &labels, double min_r2, uint32_t min_count, const size_t *max_gap,
              size_t decay_width, uint32_t decay_bins)
{
    const SiteGroups sg = site_groups(run, labels);
    run.header(decay_width ? "group\tgap\tpairs\tdefined\tlinked\tmean_r2\n"
                           : "site1\tsite2\tgroup\tmajor1\tmajor2\tcalled\tminor1\tminor2\tboth\tr2\tD\tDprime\n");
    std::vector<std::vector<uint32_t>> sites(sg.count);
    std::vector<std::vector<uint8_t>> allele(sg.count);
    std::vector<uint8_t> al;
    std::vector<uint32_t> major, other;
    walk_site_counts(run, sg, 0, run.rows().width, [&](uint64_t first, uint64_t n_sites, const uint32_t *counts) {
        al.resize(n_sites), major.resize(n_sites), other.resize(n_sites);
        for (uint32_t g = 0; g < sg.count; ++g) {
            if (dst_site_major(counts, n_sites, sg.count, g, al.data(), major.data(), other.data()) != DST_OK)
                die_message("ld: the major alleles of group " + sg.names[g]);
            for (uint64_t s = 0; s < n_sites; ++s)
                if (major[s] >= min_count && other[s] >= min_count) {
                    sites[g].push_back((uint32_t)(first + s));
                    allele[g].push_back(al[s]);
                }
        }
    });
    LineWriter out(run.wr);
    for (uint32_t g = 0; g < sg.count; ++g) {
        if (sites[g].size() < 2)
            continue;
        if (decay_width) {
            std::vector<dst_ld_bin> bins(decay_bins);
            run.gpu.check(dst_site_ld_decay(run.gpu.h, 0, sites[g].data(), allele[g].data(), (uint32_t)sites[g].size(), sg.label, g, min_r2,
                                            decay_width, decay_bins, run.max_pairs, bins.data(), bins.size()),
                          "site ld decay");
            for (uint32_t b = 0; b < decay_bins; ++b) {
                out.put(sg.names[g]);
                for (const uint64_t v : {(uint64_t)b * decay_width, bins[b].pairs, bins[b].defined, bins[b].links}) {
                    out.put('\t');
                    out.number(v);
                }
                out.put('\t');
                out.distance(DST_RAW, bins[b].defined ? bins[b].r2_sum / (double)bins[b].defined : NAN, 0);
                out.end_line();
            }
            continue;
        }
        LdSink s{out, sg.names[g], sites[g], allele[g], {}, {}, {}};
        if (max_gap)
            run.gpu.check(dst_site_ld_links_band(run.gpu.h, 0, sites[g].data(), allele[g].data(), (uint32_t)sites[g].size(), sg.label, g,
                                                 min_r2, *max_gap, run.max_pairs, ld_sink, &s, nullptr),
                          "site ld links band");
        else
            run.gpu.check(dst_site_ld_links(run.gpu.h, 0, sites[g].data(), allele[g].data(), (uint32_t)sites[g].size(), sg.label, g, min_r2,
                                            run.max_pairs, ld_sink, &s, nullptr),
                          "site ld links");
    }
    out.finish();
}

}  // namespace
