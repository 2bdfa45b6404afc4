// Output: the writer, recycled text and page-locked buffers, and the one writer of "id <tab> id <tab> value" lines.
#pragma once
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "base.hpp"

namespace {

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

// tn93's per-record base counts {A,T,G,C} of the row set and the column set; null for every other measure
struct Tn93Counts {
    const uint32_t *rows = nullptr, *cols = nullptr;
    const uint32_t *row(size_t i) const { return rows ? rows + 4 * i : nullptr; }
    const uint32_t *col(size_t j) const { return cols ? cols + 4 * j : nullptr; }
};

Tn93Counts tn93_counts(int measure, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &cols)
{
    return measure == DST_TN93 ? Tn93Counts{rows.data(), cols.data()} : Tn93Counts{};
}

// The lines of every output but the long form's slabs: text appended to a recycled buffer that goes to the writer
// whenever a finished line leaves 1 MiB in it, and when the lines are finished.
struct LineWriter {
    Writer &wr;
    TextBuf buf;
    explicit LineWriter(Writer &w) : wr(w) {}
    void put(const char *s, size_t n)
    {
        buf.ensure(n);
        std::memcpy(buf.p.get() + buf.len, s, n);
        buf.len += n;
    }
    void put(const std::string &s) { put(s.data(), s.size()); }
    void put(char c) { put(&c, 1); }
    void number(uint64_t v) { put(std::to_string(v)); }
    // a distance as the full run prints it (dst_format_distance)
    void distance(int measure, double f, int64_t iv)
    {
        char num[64];
        const int len = dst_format_distance(measure, f, iv, num, sizeof num);
        put(num, (size_t)std::min<int>(len, (int)sizeof num - 1));
    }
    // "id1 <tab> id2 <tab> value", the value's text exactly as the full run prints that pair: its tallies through
    // dst_finalize (q / t: the tn93 counts of record_1 / record_2), then dst_format_distance.  No newline: --sites adds a field.
    void pair_line(const char *id1, size_t len1, const char *id2, size_t len2, int measure, const uint32_t *tallies,
                   const uint32_t *qcounts, const uint32_t *tcounts)
    {
        double f = 0;
        int64_t iv = 0;
        dst_finalize(measure, tallies, qcounts, tcounts, &f, &iv);
        put(id1, len1);
        put('\t');
        put(id2, len2);
        put('\t');
        distance(measure, f, iv);
    }
    void pair_line(const std::string &id1, const std::string &id2, int measure, const uint32_t *tallies, const uint32_t *qcounts,
                   const uint32_t *tcounts)
    {
        pair_line(id1.data(), id1.size(), id2.data(), id2.size(), measure, tallies, qcounts, tcounts);
    }
    void end_line()
    {
        put('\n');
        if (buf.len >= ((size_t)1 << 20))
            finish();
    }
    void finish()
    {
        wr.write(buf.p.get(), buf.len);
        buf.len = 0;
    }
};

}  // namespace
