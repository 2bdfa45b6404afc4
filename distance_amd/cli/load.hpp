// Loading: the nucleotide coding, FASTA blocks parsed in parallel into encoded records, in file order.
#pragma once
#include <cstdint>
#include <deque>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "base.hpp"
#include "fasta.hpp"

namespace {

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

}  // namespace
