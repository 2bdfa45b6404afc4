// Load mode: result slabs computed on the GPUs, formatted on the host pool (or by the GPU), written in order.
#pragma once
#include <atomic>
#include <deque>

#include "format.hpp"
#include "load.hpp"
#include "output.hpp"

namespace {

// One slab of results: rows [rb, re) of the row set against the column set (square: j > i).
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

}  // namespace
