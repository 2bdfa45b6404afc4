// Stream mode: one loaded set against a FASTA read batch by batch.  stream(): src/lib.rs:269-365; stream_fasta():
// src/fastaio.rs:215-286.
#pragma once
#include <map>

#include "analyses.hpp"
#include "args.hpp"
#include "slabs.hpp"

namespace {

// A reader thread parses + encodes batch k+1 while the GPUs and the formatting pool work on batch k (the reference's
// stream_fasta thread + bounded channel, src/lib.rs:272, 290-307).  A dispatcher hands the batches round-robin to the
// GPUs (batch b -> GPU b mod G), each GPU's worker runs them through its own overlapped pipeline (dst_stream_*:
// page-locked ring slots; H2D of the next batch and D2H of the previous one under the compare of the current one) and
// formats what it collects, and the calling thread writes the batches strictly in input order (gather_write's idx
// re-ordering, src/lib.rs:616-637).
struct StreamRun {
    static constexpr int kDepth = 3;
    struct Item {
        size_t idx;
        std::unique_ptr<Alignment> batch;
    };

    const Args &a;
    std::vector<Ctx> &gpus;
    const Alignment &ref;                  // the loaded set
    Tn93Counts ref_counts;                 // its tn93 counts (rows and cols both)
    const Job &job;
    const int measure;
    const bool tn93;
    FILE *fh;
    const uint8_t *table;
    const size_t parse_threads;
    Writer &wr;
    const size_t G, TW;
    // a streamed batch is bounded by records (4096), by result pairs (--slab-pairs) and by bytes
    // (512 MiB of codes: C4-sized 5 Mbp records come ~100 at a time; split-L launches keep the GPU
    // busy on such short batches)
    const size_t batch_records;
    // what crosses the host link: the codes' high nibbles, two sites per byte (all a measure reads: half the bytes);
    // DISTANCE_WIRE=codes keeps the Paradis bytes (tests run both)
    const bool nibbles;
    // --closest for the loaded records: the lists stay on the GPU until the stream ends (one GPU, so submission order is
    // stream order)
    const bool closest_loaded;
    // --window-closest: likewise, one list per (loaded record, window) of `windows`
    const WindowList *const windows;
    const bool window_closest;
    const bool keep_ids;                   // the final lines name streamed records: their ids stay, in one arena
    // --stream-summary / --stream-histogram: the sums stay on the GPU; only --stream-summary-for streamed has lines per batch
    const bool summary, summary_streamed;
    // --stream-groups: the cells and the tables stay on the GPU; only --stream-groups-by streamed has lines per batch.  The
    // streamed groups are numbered as their first record is submitted (one GPU, so submission order is stream order).
    StreamGroups *const groups;
    const bool grouped, groups_streamed, groups_within;
    const uint32_t groups_open;            // the streamed group count the stream was opened with
    std::unordered_map<std::string, uint32_t> group_number;
    std::vector<std::string> group_names;

    std::mutex qmu;                        // reader -> dispatcher -> per-GPU input queues
    std::condition_variable qcv;
    std::deque<std::unique_ptr<Alignment>> queue;
    bool reader_done = false;
    size_t record_counter = 0;
    std::vector<std::deque<Item>> gq;
    std::vector<bool> gdone;
    std::mutex wmu;                        // workers -> ordered writer
    std::condition_variable wcv;
    std::map<size_t, std::vector<TextBuf>> done_text;   // formatted batches waiting for the writer
    size_t next_to_write = 0, n_batches = 0;
    bool all_dispatched = false;
    const size_t window;                   // bound on batches between dispatch and write
    std::vector<dst_stream *> streams;
    // closest for the loaded records: the streamed ids (one arena + offsets) and, for tn93, base counts until the end
    std::vector<char> kept_ids;
    std::vector<uint64_t> kept_off{0};
    std::vector<uint32_t> kept_counts;

    StreamRun(const Args &args, std::vector<Ctx> &g, const Alignment &loaded, const std::vector<uint32_t> &counts, const Job &j,
              FILE *stream_fh, const uint8_t *tab, size_t threads, Writer &w, const WindowList *wl = nullptr, StreamGroups *sg = nullptr)
        : a(args), gpus(g), ref(loaded), ref_counts(tn93_counts(j.measure, counts, counts)), job(j), measure(j.measure),
          tn93(j.measure == DST_TN93), fh(stream_fh), table(tab), parse_threads(threads), wr(w), G(g.size()),
          TW((size_t)dst_tally_width(j.measure)),
          batch_records(std::max<size_t>(1, std::min<size_t>({(size_t)4096, args.slab_pairs / std::max<size_t>(loaded.n, 1),
                                                              ((size_t)512 << 20) / std::max<size_t>(loaded.width, 1)}))),
          nibbles(!(std::getenv("DISTANCE_WIRE") && std::strcmp(std::getenv("DISTANCE_WIRE"), "codes") == 0)),
          closest_loaded(args.mode == Mode::Closest && args.closest_side == DST_CLOSEST_FOR_LOADED), windows(wl),
          window_closest(args.mode == Mode::WindowClosest),
          keep_ids(closest_loaded || window_closest),
          summary(args.mode == Mode::StreamSummary || args.mode == Mode::StreamHistogram),
          summary_streamed(args.mode == Mode::StreamSummary && args.stream_summary_streamed), groups(sg),
          grouped(args.mode == Mode::StreamGroups), groups_streamed(grouped && args.stream_groups_by == 1),
          groups_within(args.has[F_STREAM_GROUPS_WITHIN]),
          groups_open(grouped && !groups_streamed ? (uint32_t)std::min<size_t>(std::max<size_t>(distinct_groups(sg), 1), DST_GROUPS_MAX) : 1),
          gq(G), gdone(G, false),
          window(G * (kDepth + 2)), streams(G, nullptr)
    {
    }

    static size_t distinct_groups(const StreamGroups *sg)
    {
        std::unordered_set<std::string> names;
        for (const auto &entry : sg->file->of)
            names.insert(entry.second.first);
        return names.size();
    }

    void read()
    {
        // bytes of FASTA per parsed block ~ records per batch
        const size_t block_bytes = std::max<size_t>(batch_records * (ref.width + 64), (size_t)1 << 20);
        parse_stream(fh, block_bytes, parse_threads, table, tn93, true, ref.width, [&](std::unique_ptr<Alignment> batch) {
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
    }

    // the reader's batches, in order, to the GPUs
    void dispatch()
    {
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
                    gq[idx % G].push_back(Item{idx, std::move(piece)});
                }
                qcv.notify_all();
                if (!batch)
                    break;
            }
        }
        {
            std::lock_guard<std::mutex> lk(qmu);
            for (size_t g = 0; g < G; ++g)
                gdone[g] = true;
        }
        qcv.notify_all();
        {
            std::lock_guard<std::mutex> lk(wmu);
            all_dispatched = true;
        }
        wcv.notify_all();
    }

    // a batch's records into a pipeline slot: the code bytes, or their high nibbles (site 2k in the low nibble, 2k + 1 in
    // the high one)
    void pack(const Alignment &al, uint8_t *buf, size_t pitch) const
    {
        for (size_t r = 0; r < al.n; ++r) {
            const uint8_t *src = al.codes.data() + r * al.width;
            uint8_t *dst = buf + r * pitch;
            if (!nibbles) {
                std::memcpy(dst, src, al.width);
                continue;
            }
            const size_t half = al.width / 2;
            for (size_t k = 0; k < half; ++k)
                dst[k] = (uint8_t)((src[2 * k] >> 4) | (src[2 * k + 1] & 0xF0u));
            if (al.width & 1)
                dst[half] = (uint8_t)((src[al.width - 1] >> 4) | 0xF0u);
        }
    }

    void hand_over(size_t idx, std::vector<TextBuf> text)
    {
        {
            std::lock_guard<std::mutex> lk(wmu);
            done_text[idx] = std::move(text);
        }
        wcv.notify_all();
    }

    // a batch's lines as one text: "loaded id <tab> streamed id <tab> value", the streamed record's counts as q
    void streamed_pair(LineWriter &out, const Alignment &al, size_t r, size_t j, const uint32_t *tal) const
    {
        out.pair_line(ref.ids[j], al.ids[r], measure, tal, tn93 ? al.counts.data() + 4 * r : nullptr, ref_counts.col(j));
        out.put('\n');   // (not end_line: the text goes to the ordered writer, not out now)
    }

    // every pair of the batch, formatted like a slab of the long form
    std::vector<TextBuf> collect_matrix(const Item &it, const void *res) const
    {
        Job sj = job;
        sj.square = false;
        sj.swap_ids = true;          // id1 = loaded record, id2 = streamed record (src/lib.rs:327-330)
        sj.rows = it.batch.get();    // streamed record outer ...
        sj.cols = &ref;              // ... loaded record inner (src/lib.rs:323-324)
        sj.row_counts = tn93 ? it.batch->counts.data() : nullptr;
        sj.col_counts = ref_counts.cols;
        Slab slab;
        slab.rb = 0;
        slab.re = it.batch->n;
        slab.tallies = const_cast<uint32_t *>(static_cast<const uint32_t *>(res));  // library-owned, read only
        format_slab(sj, slab);
        return std::move(slab.text);
    }

    // --closest-for streamed: the batch's records in stream order, each with its k_used closest loaded records
    // (--closest-for loaded: nothing per batch, the lines follow the stream's end)
    std::vector<TextBuf> collect_closest(size_t g, const Item &it, size_t n_rec)
    {
        std::vector<TextBuf> text;
        if (closest_loaded)
            return text;
        const uint32_t *index = nullptr, *tal = nullptr;
        uint32_t ku = 0;
        gpus[g].check(dst_stream_closest_batch(streams[g], &index, &tal, nullptr, &ku), "stream closest batch");
        LineWriter out(wr);
        for (size_t r = 0; r < n_rec; ++r)
            for (size_t e = 0; e < ku; ++e)
                streamed_pair(out, *it.batch, r, index[r * ku + e], tal + (r * ku + e) * TW);
        text.push_back(std::move(out.buf));
        return text;
    }

    // --within: the batch's links in stream order, window after window, each as the full run's line
    std::vector<TextBuf> collect_within(size_t g, const Item &it)
    {
        LineWriter out(wr);
        for (uint64_t first = 0;;) {
            uint64_t m = 0, total = 0;
            const uint32_t *srec = nullptr, *lrec = nullptr, *tal = nullptr;
            gpus[g].check(dst_stream_links_batch(streams[g], first, &m, &total, &srec, &lrec, nullptr, &tal), "stream links batch");
            for (uint64_t e = 0; e < m; ++e)
                streamed_pair(out, *it.batch, srec[e], lrec[e], tal + e * TW);
            first += m;
            if (first >= total)
                break;
        }
        std::vector<TextBuf> text;
        text.push_back(std::move(out.buf));
        return text;
    }

    // --stream-summary-for streamed: the batch's records in stream order, each with --summary's line against the loaded set
    // (--stream-summary-for loaded and --stream-histogram: nothing per batch, the lines follow the stream's end)
    std::vector<TextBuf> collect_summary(size_t g, const Item &it)
    {
        std::vector<TextBuf> text;
        if (!summary_streamed)
            return text;
        size_t n_rec = 0;
        const uint32_t *within = nullptr, *summable = nullptr;
        const double *sum = nullptr;
        gpus[g].check(dst_stream_summary_batch(streams[g], &n_rec, &within, &summable, &sum), "stream summary batch");
        LineWriter out(wr);
        for (size_t r = 0; r < n_rec; ++r) {
            summary_line(out, it.batch->ids[r], within[r], summable[r], sum[r]);
            out.put('\n');   // (not end_line: the text goes to the ordered writer, not out now)
        }
        text.push_back(std::move(out.buf));
        return text;
    }

    // --stream-groups: the batch's labels into the acquired slot's block (by streamed: none, every record in group 0), the
    // ids of the file that the batch carries into `seen`
    void label_batch(size_t g, const Alignment &al)
    {
        uint32_t *labels = nullptr;
        gpus[g].check(dst_stream_group_labels(streams[g], &labels), "stream group labels");
        const GroupFile &gf = *groups->file;
        for (size_t r = 0; r < al.n; ++r) {
            const auto it = gf.of.find(al.ids[r]);
            if (it == gf.of.end()) {
                if (!groups_streamed)
                    labels[r] = DST_GROUP_NONE;
                continue;
            }
            groups->seen.insert(al.ids[r]);
            if (groups_streamed)
                continue;
            const auto ins = group_number.emplace(it->second.first, (uint32_t)group_names.size());
            if (ins.second) {
                if (group_names.size() == groups_open)
                    die_message(gf.flag + ": the streamed record '" + al.ids[r] + "' starts group " + std::to_string(groups_open + 1) +
                                " of the stream: more than " + std::to_string(groups_open) + " groups");
                group_names.push_back(it->second.first);
            }
            labels[r] = ins.first->second;
        }
    }

    // --stream-groups-by streamed: the batch's records in stream order, each with --groups --per-record's lines against the
    // loaded groups (cell, loaded: nothing per batch, the lines follow the stream's end)
    std::vector<TextBuf> collect_groups(size_t g, const Item &it)
    {
        std::vector<TextBuf> text;
        if (!groups_streamed)
            return text;
        size_t n_rec = 0;
        const uint32_t *within = nullptr, *summable = nullptr;
        const double *sum = nullptr;
        gpus[g].check(dst_stream_group_summary_batch(streams[g], &n_rec, &within, &summable, &sum), "stream group summary batch");
        const std::vector<std::string> &names = groups->loaded.names;
        LineWriter out(wr);
        for (size_t r = 0; r < n_rec; ++r)
            for (size_t b = 0; b < names.size(); ++b) {
                const size_t e = r * names.size() + b;
                out.put(it.batch->ids[r]);
                out.put('\t');
                out.put(names[b]);
                put_group_record(out, summable[e], within[e], sum[e], groups_within);
                out.put('\n');   // (not end_line: the text goes to the ordered writer, not out now)
            }
        text.push_back(std::move(out.buf));
        return text;
    }

    void collect_one(size_t g, std::deque<Item> &inflight)
    {
        size_t n_rec = 0;
        const void *res = nullptr;
        gpus[g].check(dst_stream_collect(streams[g], &n_rec, &res), "stream collect");
        Item it = std::move(inflight.front());
        inflight.pop_front();
        hand_over(it.idx, a.mode == Mode::Within          ? collect_within(g, it)
                          : a.mode == Mode::Closest       ? collect_closest(g, it, n_rec)
                          : summary                       ? collect_summary(g, it)
                          : grouped                       ? collect_groups(g, it)
                          : a.mode == Mode::WindowClosest ? std::vector<TextBuf>()   // (the lines follow the stream's end)
                                                          : collect_matrix(it, res));
    }

    // one GPU's worker: its queue's batches through its pipeline, kDepth - 1 in flight
    void work(size_t g)
    {
        std::deque<Item> inflight;
        for (;;) {
            Item it;
            bool have = false;
            {
                std::unique_lock<std::mutex> lk(qmu);
                qcv.wait(lk, [&] { return !gq[g].empty() || gdone[g]; });
                if (!gq[g].empty()) {
                    it = std::move(gq[g].front());
                    gq[g].pop_front();
                    have = true;
                }
            }
            qcv.notify_all();
            if (!have)
                break;
            if (inflight.size() == (size_t)kDepth - 1)
                collect_one(g, inflight);
            uint8_t *buf = nullptr;
            size_t pitch = 0;
            uint32_t *cbuf = nullptr;
            gpus[g].check(dst_stream_acquire(streams[g], &buf, &pitch, &cbuf), "stream acquire");
            const Alignment &al = *it.batch;
            pack(al, buf, pitch);
            // (a window-closest stream counts per window on the device: the caller's counts are not read)
            const bool send_counts = tn93 && !window_closest;
            if (send_counts)
                std::memcpy(cbuf, al.counts.data(), al.n * 4 * sizeof(uint32_t));
            if (grouped)
                label_batch(g, al);
            gpus[g].check(dst_stream_submit(streams[g], al.n, send_counts ? 1 : 0), "stream submit");
            if (keep_ids) {   // ordinal = position in submission order: keep what the final lines need
                for (size_t r = 0; r < al.n; ++r) {
                    kept_ids.insert(kept_ids.end(), al.ids[r].begin(), al.ids[r].end());
                    kept_off.push_back(kept_ids.size());
                }
                if (send_counts)
                    kept_counts.insert(kept_counts.end(), al.counts.begin(), al.counts.end());
                it.batch.reset();
            }
            if ((summary && !summary_streamed) || (grouped && !groups_streamed))
                it.batch.reset();   // no line names a streamed record: host memory does not grow with the stream
            inflight.push_back(std::move(it));
        }
        while (!inflight.empty())
            collect_one(g, inflight);
    }

    void write_in_order()
    {
        for (;;) {
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
    }

    // --closest-for loaded: every loaded record in input order with its k_used closest streamed records
    void write_closest_loaded()
    {
        const size_t cap = ref.n * std::min<size_t>(a.closest, kept_off.size() - 1);
        std::vector<uint32_t> index(std::max<size_t>(cap, 1)), tal(std::max<size_t>(cap * TW, 1));
        uint32_t ku = 0;
        gpus[0].check(dst_stream_closest_result(streams[0], index.data(), tal.data(), nullptr, cap, &ku), "stream closest result");
        LineWriter out(wr);
        for (size_t i = 0; i < ref.n; ++i)
            for (size_t e = 0; e < ku; ++e) {
                const size_t at = i * ku + e, o = index[at];
                out.pair_line(ref.ids[i].data(), ref.ids[i].size(), kept_ids.data() + kept_off[o],
                              (size_t)(kept_off[o + 1] - kept_off[o]), measure, tal.data() + at * TW,
                              tn93 ? kept_counts.data() + 4 * o : nullptr, ref_counts.col(i));
                out.end_line();
            }
        out.finish();
    }

    // --window-closest K: every loaded record in input order and every window in the given order with its k_used nearest
    // streamed records, each as the line '--window-nearest K loaded streamed' prints for it: the value from the entry's
    // DST_OUT_TALLY words and, for tn93, the loaded record's base counts inside the window (dst_window_base_counts) and the
    // streamed record's, which the lists carry (the batch is gone), through dst_finalize and the long output's formatter
    void write_window_closest()
    {
        static const char header[] = "sequence1\tsequence2\twindow\tstart\tend\tdistance\n";
        wr.write(header, sizeof header - 1);
        if (ref.n == 0 || kept_off.size() < 2)
            return;
        const WindowList &wl = *windows;
        const size_t nw = wl.begin.size();
        const size_t cap = ref.n * nw * std::min<size_t>(a.window_closest, kept_off.size() - 1);
        std::vector<uint32_t> index(cap), tal(cap * TW), counts(tn93 ? cap * 4 : 0), row_counts(tn93 ? nw * ref.n * 4 : 0);
        uint32_t ku = 0;
        gpus[0].check(dst_stream_window_closest_result(streams[0], index.data(), tal.data(), nullptr,
                                                       tn93 ? counts.data() : nullptr, cap, &ku),
                      "stream window closest result");
        if (tn93)
            gpus[0].check(dst_window_base_counts(gpus[0].h, 0, wl.begin.data(), wl.end.data(), (uint32_t)nw, row_counts.data(),
                                                 row_counts.size()),
                          "window base counts");
        LineWriter out(wr);
        size_t e = 0;
        for (size_t i = 0; i < ref.n; ++i)
            for (size_t w = 0; w < nw; ++w)
                for (size_t r = 0; r < ku; ++r, ++e) {
                    const size_t o = index[e];
                    double f = 0;
                    int64_t iv = 0;
                    dst_finalize(measure, &tal[e * TW], tn93 ? &row_counts[(w * ref.n + i) * 4] : nullptr,
                                 tn93 ? &counts[e * 4] : nullptr, &f, &iv);
                    out.put(ref.ids[i]);
                    out.put('\t');
                    out.put(kept_ids.data() + kept_off[o], (size_t)(kept_off[o + 1] - kept_off[o]));
                    out.put('\t');
                    out.put(wl.names[w]);
                    out.put('\t');
                    out.number(wl.begin[w] + 1);
                    out.put('\t');
                    out.number(wl.end[w]);
                    out.put('\t');
                    out.distance(measure, f, iv);
                    out.end_line();
                }
        out.finish();
    }

    // --stream-summary (loaded): every loaded record in input order with --summary's line against the whole stream
    void write_summary_loaded()
    {
        const size_t cap = std::max<size_t>(ref.n, 1);
        std::vector<uint32_t> within(cap), summable(cap);
        std::vector<double> sum(cap);
        gpus[0].check(dst_stream_summary_result(streams[0], nullptr, within.data(), summable.data(), sum.data(), ref.n, nullptr,
                                                nullptr),
                      "stream summary result");
        LineWriter out(wr);
        for (size_t i = 0; i < ref.n; ++i) {
            summary_line(out, ref.ids[i], within[i], summable[i], sum[i]);
            out.end_line();
        }
        out.finish();
    }

    // --stream-histogram: --histogram's lines over every loaded x streamed pair
    void write_stream_histogram()
    {
        std::vector<uint64_t> hist(a.stream_bins);
        dst_summary_totals totals;
        gpus[0].check(dst_stream_summary_result(streams[0], hist.data(), nullptr, nullptr, nullptr, 0, &totals, nullptr),
                      "stream summary result");
        histogram_lines(wr, measure, a.stream_histogram, hist, totals.nan_pairs);
    }

    // --stream-groups (cell): --groups' line per (streamed group, loaded group); (loaded): --per-record's line per loaded
    // record in input order and streamed group, the groups in order of their first record
    void write_groups_end()
    {
        const size_t Gs = groups_open, Gl = std::max<size_t>(groups->loaded.names.size(), 1), seen_groups = group_names.size();
        LineWriter out(wr);
        if (a.stream_groups_by == 0) {
            std::vector<dst_group_cell> cells(Gs * Gl);
            gpus[0].check(dst_stream_group_summary_result(streams[0], cells.data(), cells.size(), nullptr, nullptr, nullptr, 0, nullptr),
                          "stream group summary result");
            for (size_t s = 0; s < seen_groups; ++s)
                for (size_t b = 0; b < Gl; ++b) {
                    out.put(group_names[s]);
                    out.put('\t');
                    out.put(groups->loaded.names[b]);
                    put_group_cell(out, measure, cells[s * Gl + b], groups_within);
                    out.end_line();
                }
        } else {
            const size_t cap = std::max<size_t>(ref.n * Gs, 1);
            std::vector<uint32_t> within(cap), summable(cap);
            std::vector<double> sum(cap);
            gpus[0].check(dst_stream_group_summary_result(streams[0], nullptr, 0, within.data(), summable.data(), sum.data(), ref.n * Gs,
                                                          nullptr),
                          "stream group summary result");
            for (size_t i = 0; i < ref.n; ++i)
                for (size_t s = 0; s < seen_groups; ++s) {
                    const size_t e = i * Gs + s;
                    out.put(ref.ids[i]);
                    out.put('\t');
                    out.put(group_names[s]);
                    put_group_record(out, summable[e], within[e], sum[e], groups_within);
                    out.end_line();
                }
        }
        out.finish();
    }

    void run()
    {
        if (grouped) {
            std::string header = a.stream_groups_by == 0 ? "group1\tgroup2\tpairs\tcompared" : "sequence\tgroup\tcompared";
            if (groups_within)
                header += "\twithin";
            header += a.stream_groups_by == 0 ? "\tmean\tmin\tmax\n" : "\tmean\n";
            wr.write(header.data(), header.size());
        }
        if (summary) {
            const char *header = a.mode == Mode::StreamSummary ? "sequence\twithin\tcompared\tmean\n" : "distance\tpairs\n";
            wr.write(header, std::strlen(header));
        }
        std::thread reader([this] { read(); });
        const int wire = nibbles ? DST_WIRE_NIBBLES : DST_WIRE_CODES;
        for (size_t g = 0; g < G; ++g)
            gpus[g].check(grouped
                              ? dst_stream_open_group_summary(
                                    gpus[g].h, measure, groups_within ? a.stream_groups_within : HUGE_VAL,
                                    groups_streamed ? DST_STREAM_GROUPS_STREAMED : a.stream_groups_by == 2 ? DST_STREAM_GROUPS_LOADED : 0,
                                    a.stream_groups_by == 2 ? nullptr : groups->loaded.label.data(),
                                    a.stream_groups_by == 2 ? 1 : (uint32_t)groups->loaded.names.size(), groups_open, batch_records,
                                    kDepth, wire, &streams[g])
                          : a.mode == Mode::StreamSummary
                              ? dst_stream_open_summary(gpus[g].h, measure, a.stream_summary,
                                                        summary_streamed ? DST_STREAM_SUMMARY_STREAMED : DST_STREAM_SUMMARY_LOADED, 0,
                                                        0.0, batch_records, kDepth, wire, &streams[g])
                          : a.mode == Mode::StreamHistogram
                              ? dst_stream_open_summary(gpus[g].h, measure, 0.0, 0, (uint32_t)a.stream_bins, a.stream_histogram,
                                                        batch_records, kDepth, wire, &streams[g])
                          : a.mode == Mode::Closest
                              ? dst_stream_open_closest(gpus[g].h, measure, (uint32_t)a.closest, a.closest_side, batch_records,
                                                        kDepth, wire, &streams[g])
                          : window_closest
                              ? dst_stream_open_window_closest(gpus[g].h, measure, (uint32_t)a.window_closest, windows->begin.data(),
                                                               windows->end.data(), (uint32_t)windows->begin.size(),
                                                               a.analysis_slab(), batch_records, kDepth, wire, &streams[g])
                          : a.mode == Mode::Within
                              ? dst_stream_open_links(gpus[g].h, measure, a.within, DST_LINKS_TALLIES, 0, batch_records, kDepth,
                                                      wire, &streams[g])
                              : dst_stream_open_wire(gpus[g].h, measure, DST_OUT_TALLY, batch_records, kDepth, wire, &streams[g]),
                          "stream open");
        std::vector<std::thread> workers;
        for (size_t g = 0; g < G; ++g)
            workers.emplace_back([this, g] { work(g); });
        std::thread dispatcher([this] { dispatch(); });
        write_in_order();
        dispatcher.join();
        for (auto &t : workers)
            t.join();
        if (closest_loaded)
            write_closest_loaded();
        if (a.mode == Mode::WindowClosest)
            write_window_closest();
        if (a.mode == Mode::StreamSummary && !summary_streamed)
            write_summary_loaded();
        if (a.mode == Mode::StreamHistogram)
            write_stream_histogram();
        if (grouped && !groups_streamed)
            write_groups_end();
        if (grouped && groups->seen.size() < groups->file->of.size())
            std::fprintf(stderr, "warning: %s: %zu ids of '%s' are not in the input and were skipped\n", groups->file->flag.c_str(),
                         groups->file->of.size() - groups->seen.size(), groups->file->path.c_str());
        for (size_t g = 0; g < G; ++g)
            dst_stream_close(streams[g]);
        reader.join();
        if (record_counter == 0)
            die_message("Empty FASTA file");  // src/fastaio.rs:281-283
    }
};

}  // namespace
