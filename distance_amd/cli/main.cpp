// distance — drop-in CLI for benjamincjackson/distance on MI355X.
//
// Keeps the reference's surface (clap definition src/lib.rs:68-131, rules of set_up() src/lib.rs:162-267) and its TSV
// output, identical to gather_write() (src/lib.rs:612-644); the flags, the reference's and this program's own output
// modes, are listed by --help (args.hpp).  The pair generators and worker pools (src/lib.rs:269-474, 502-596) are
// replaced by libdistance_hip.so through its C ABI; -t sizes the host formatting pool and -b is accepted — neither
// changes the output, as in the reference (src/lib.rs:919-1154).
//
// One translation unit: args.hpp (the command line), load.hpp (FASTA -> encoded records), output.hpp (writer, buffers,
// the pair-line writer), slabs.hpp (load mode), analyses.hpp (the other output modes), stream.hpp (stream mode).
//
// Exactness: the GPU returns integer site tallies; f64 finalisation is dst_finalize() on the host
// (reference operation order, glibc log/sqrt), so the printed digits do not depend on the device.
#include <csignal>

#include "analyses.hpp"
#include "args.hpp"
#include "stream.hpp"

namespace {

// ---------------------------------------------------------------- host self-tests (no GPU) -----
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
                    a.threads, a.has[F_THREADS] ? "" : "(default)", a.batchsize, a.has[F_STREAM] ? a.stream.c_str() : "<none>",
                    a.has[F_OUTPUT] ? a.output.c_str() : "<stdout>", a.gpus);
        for (auto &s : a.flag_inputs)
            std::printf("[-i %s]", s.c_str());
        for (auto &s : a.pos_inputs)
            std::printf("[pos %s]", s.c_str());
        std::puts("");
        return 0;
    }
    die_usage("unknown --host-selftest");
}

// The HIP runtime and the contexts come up on a thread of their own while the files are parsed (0.2 s of a 2.3 s run at
// 50,000 x 30,000); what it finds is looked at after the parse, so a bad input is reported first.  One context (and one
// worker thread) per listed device; a device may be listed more than once.
struct GpuInit {
    int ndev = 0;
    bool count_ok = false;
    std::vector<int> devices;
    std::vector<Ctx> gpus;
    std::string error;
    std::thread thread;
    explicit GpuInit(const Args &a)
    {
        thread = std::thread([this, &a] {
            count_ok = dst_device_count(&ndev) == DST_OK && ndev > 0;
            if (!count_ok)
                return;
            devices = a.devices;
            if (devices.empty())
                for (int g = 0; g < std::max(1, std::min(a.gpus, ndev)); ++g)
                    devices.push_back(g);
            gpus.resize(devices.size());
            for (size_t g = 0; g < devices.size(); ++g)
                if (dst_create(devices[g], &gpus[g].h) != DST_OK) {
                    error = dst_last_error(nullptr);
                    return;
                }
        });
    }
};

// ---- load(): src/lib.rs:367-474: the long form, or a matrix, of the loaded sets ----
void run_load_mode(std::vector<Ctx> &gpus, Job &job, const std::vector<Alignment> &loaded, const Tn93Counts &tn93, const Args &a,
                   Writer &wr)
{
    job.square = loaded.size() == 1;
    job.matrix = a.matrix;
    job.rows = &loaded[0];
    job.cols = &loaded.back();
    job.row_counts = tn93.rows;
    job.col_counts = tn93.cols;
    // The TSV lines themselves come from the GPU (dst_text_*): it has the distances and the ids, the exact
    // {:.12} conversion is integer arithmetic, and the host's formatter pool was what bounded a large run.
    // For jc69 / k80 / tn93 the device finalises the tallies itself and hands the values that lie near a rounding
    // boundary of the 12th decimal back to dst_finalize (libm) before the text leaves the library, so the bytes are
    // the host formatter's (tests/test_gpu_text_identity.py: 0 of 1.5e8 lines differ; DISTANCE_HOST_FORMAT=1 keeps
    // the host formatter, and tests/test_gpu_cli.py compares the two).
    job.gpu_text = std::getenv("DISTANCE_HOST_FORMAT") == nullptr;
    for (size_t g = 0; g < gpus.size() && job.gpu_text; ++g)
        for (size_t k = 0; k < loaded.size(); ++k) {
            const IdArena ids(loaded[k]);
            if (dst_set_ids(gpus[g].h, (int)k, ids.chars.data(), ids.offsets.data(), loaded[k].n) != DST_OK)
                job.gpu_text = false;   // (e.g. 4 GB of ids): the host formatter takes over
        }
    run_slabs(gpus, job, 0, 1, a.slab_pairs, wr);
}

}  // namespace

int main(int argc, char **argv)
{
    PhaseTimer timer;
    std::signal(SIGPIPE, SIG_IGN);  // EPIPE is handled at the write (exit 0), like the reference
    const Args a = parse_args(argc, argv);
    if (!a.selftest.empty())
        return host_selftest(a);
    if (a.licenses) {  // src/main.rs:7-10
        std::puts(kLicences);
        return 0;
    }
    // ---- inputs: set_up(), src/lib.rs:162-267 ------------------------------------------------
    if (!a.pos_inputs.empty() && !a.flag_inputs.empty())
        die_message("For loading input files, don't use both positional arguments and the -i/--input flag");
    std::vector<std::string> inputs = a.flag_inputs;
    inputs.insert(inputs.end(), a.pos_inputs.begin(), a.pos_inputs.end());
    // --groups: the label file's own errors come before anything else is opened
    GroupFile group_file;
    if (a.mode == Mode::Groups)
        group_file = read_group_file(a.groups);
    else if (a.has[F_WINDOW_GROUPS])
        group_file = read_group_file(a.window_groups, "--window-groups");
    else if (a.mode == Mode::StreamGroups)
        group_file = read_group_file(a.stream_groups, "--stream-groups");
    else if (a.has[F_SITE_GROUPS])
        group_file = read_group_file(a.site_groups, "--site-groups");
    else if (a.has[F_LD_GROUPS])
        group_file = read_group_file(a.ld_groups, "--ld-groups");
    // --pairs: likewise
    PairFile pair_file;
    if (a.mode == Mode::PairList)
        pair_file = read_pair_file(a.pairs);
    // --regions: likewise
    WindowList windows;
    if (a.has[F_REGIONS])
        windows = read_region_file(a.regions);
    std::vector<FILE *> files;
    if (inputs.empty())
        files.push_back(stdin);
    for (auto &p : inputs)
        files.push_back(open_input(p));
    FILE *stream_fh = nullptr;
    if (a.has[F_STREAM]) {
        if (inputs.size() != 1)
            die_message("If you stream one file, you must also provide exactly one other file to be loaded");
        stream_fh = a.stream == "-" ? stdin : open_input(a.stream);
    }
    // ---- GPU bring-up under the parse ---------------------------------------------------------
    GpuInit gi(a);
    uint8_t table[256];
    encoding_array(table);
    const size_t threads = a.has[F_THREADS] ? std::max<size_t>(a.threads, 1)  // src/lib.rs:253-263
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
    if (a.mode == Mode::Groups)
        group_labels = label_inputs(group_file, loaded);
    else if (a.has[F_WINDOW_GROUPS])
        group_labels = label_inputs(group_file, loaded, DST_WINDOW_GROUPS_MAX);
    else if (a.has[F_SITE_GROUPS] || a.has[F_LD_GROUPS])
        group_labels = label_inputs(group_file, loaded);
    // --stream-groups: the loaded records' labels (cell, streamed), and the ids of the file that the loaded side carries
    StreamGroups stream_groups;
    if (a.mode == Mode::StreamGroups)
        stream_groups = label_loaded_for_stream(group_file, loaded[0], a.stream_groups_by);
    // --pairs: the records its ids name
    PairList pair_list;
    if (a.mode == Mode::PairList)
        pair_list = resolve_pairs(pair_file, loaded);
    // --windows / --regions: the windows over the width the inputs turned out to have
    if (a.has[F_REGIONS])
        check_regions(windows, loaded[0].width);
    else if (a.mode == Mode::Windows || a.mode == Mode::WindowClosest)
        windows = sliding_windows(loaded[0].width, a.windows, a.has[F_STEP] ? a.step : a.windows);
    Writer wr;
    if (a.has[F_OUTPUT]) {
        wr.fh = std::fopen(a.output.c_str(), "wb");
        if (!wr.fh)
            die_io(a.output, errno);
    }
    static char outbuf[1 << 20];
    std::setvbuf(wr.fh, outbuf, _IOFBF, sizeof outbuf);

    const int measure = dst_measure_from_name(a.measure.c_str());
    gi.thread.join();
    if (!gi.count_ok) {
        std::fprintf(stderr, "Error: Gpu(\"no MI355X / HIP device visible: this build has no CPU path\")\n");
        return 1;
    }
    if (!gi.error.empty()) {
        std::fprintf(stderr, "Error: Gpu(\"%s\")\n", gi.error.c_str());
        return 1;
    }
    std::vector<Ctx> &gpus = gi.gpus;
    timer.mark("HIP init + contexts (what the parse did not hide)");
    // ---- upload ---------------------------------------------------------------------------------
    for (Ctx &gpu : gpus)
        for (size_t k = 0; k < loaded.size(); ++k)
            gpu.check(dst_upload(gpu.h, (int)k, loaded[k].codes.data(), loaded[k].n, loaded[k].width, loaded[k].width, nullptr),
                      "upload");
    // tn93: per-record base counts by code (count_bases(), src/lib.rs:233-239), from the device
    std::vector<std::vector<uint32_t>> counts(loaded.size());
    if (measure == DST_TN93)
        for (size_t k = 0; k < loaded.size(); ++k) {
            counts[k].resize(loaded[k].n * 4);
            gpus[0].check(dst_get_base_counts(gpus[0].h, (int)k, counts[k].data()), "base counts");
        }
    timer.mark("upload + pack + counts");

    // ---- the header line (the analyses with columns of their own write theirs), then the mode ----
    const Run run{gpus[0], loaded, tn93_counts(measure, counts[0], counts.back()), measure, a.analysis_slab(), wr};
    Job job;
    job.measure = measure;
    job.fmt_threads = std::max<size_t>(1, threads / gpus.size());
    const bool pair_lines = a.mode == Mode::Pairs || a.mode == Mode::Stream || a.mode == Mode::Closest ||
                            a.mode == Mode::Within || a.mode == Mode::Nearest || a.mode == Mode::MaxDistance || a.mode == Mode::Mst ||
                            a.mode == Mode::PairList;
    if (pair_lines)   // src/lib.rs:613
        run.header(a.has[F_SITES] ? "sequence1\tsequence2\tdistance\tsites\n" : "sequence1\tsequence2\tdistance\n");
    switch (a.mode) {
    case Mode::Tree: write_tree(run, (uint32_t)a.bootstrap, a.seed); break;
    case Mode::Dendrogram: write_dendrogram(run, a.dendrogram); break;
    case Mode::Clusters: write_clusters(run, a.clusters); break;
    case Mode::Representatives: write_representatives(run, a.representatives); break;
    case Mode::Mst: write_mst(run, a.has[F_SITES]); break;
    case Mode::MaxDistance: write_links(run, a.max_distance, a.has[F_SITES]); break;
    case Mode::PairList: write_pair_list(run, pair_list, a.has[F_SITES]); break;
    case Mode::Summary: write_summary(run, a.summary); break;
    case Mode::Groups: write_groups(run, group_labels, a.has[F_GROUPS_WITHIN], a.groups_within, a.has[F_PER_RECORD]); break;
    case Mode::Histogram: write_histogram(run, a.histogram, (uint32_t)a.bins); break;
    case Mode::Nearest: write_nearest(run, (uint32_t)a.nearest); break;
    case Mode::SiteCounts: write_site_counts(run, group_labels); break;
    case Mode::Ld: write_ld(run, group_labels, a.ld, (uint32_t)a.ld_min_count, a.has[F_LD_MAX_GAP] ? &a.ld_max_gap : nullptr, a.ld_decay, (uint32_t)a.ld_bins); break;
    case Mode::Windows:
        if (a.has[F_WINDOW_SITE_STATS])
            write_window_site_stats(run, windows, group_labels);
        else if (a.has[F_WINDOW_GROUPS])
            write_window_groups(run, windows, group_labels, a.has[F_WINDOW_GROUPS_WITHIN], a.window_groups_within,
                                a.window_groups_by_record);
        else if (a.has[F_WINDOW_SUMMARY])
            write_window_summary(run, windows, a.window_summary, a.window_summary_by_record);
        else if (a.has[F_WINDOW_NEAREST])
            write_window_nearest(run, windows, (uint32_t)a.window_nearest, a.analysis_slab());
        else
            write_windows(run, windows, a.slab_pairs);
        break;
    case Mode::Matrix: {
        // tsv: an empty corner cell, then the column ids (the last input's records); phylip: the number of records
        std::string h = a.matrix == DST_MATRIX_PHYLIP ? std::to_string(loaded[0].n) : "";
        for (size_t j = 0; a.matrix == DST_MATRIX_TSV && j < loaded.back().n; ++j)
            h += '\t' + loaded.back().ids[j];
        h += '\n';
        wr.write(h.data(), h.size());
        [[fallthrough]];
    }
    case Mode::Pairs: run_load_mode(gpus, job, loaded, run.tn93, a, wr); break;
    case Mode::Stream:
    case Mode::Closest:
    case Mode::WindowClosest:
    case Mode::StreamSummary:
    case Mode::StreamHistogram:
    case Mode::StreamGroups:
    case Mode::Within:
        StreamRun(a, gpus, loaded[0], counts[0], job, stream_fh, table, parse_threads, wr, &windows, &stream_groups).run();
        break;
    }
    timer.mark("compute + format + write");
    wr.flush();
    timer.mark("flush");
    for (auto &g : gpus)
        dst_destroy(g.h);
    timer.mark("destroy contexts");
    if (a.has[F_OUTPUT] && std::fclose(wr.fh) != 0)
        die_io(a.output, errno);
    // everything is written and closed: leave without the runtime's own teardown (unlocking the page-locked text buffers,
    // unloading the code objects: 0.3 s of a 2 s run that nothing is waiting for)
    leave(0);
}
