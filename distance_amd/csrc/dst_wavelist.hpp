// dst_wavelist.hpp — one sorted list of at most kNearestMaxK = 256 (key, index) entries held in the registers of a wave
// (dst_nearest.hip's passes, dst_window_nearest.hip's selection).  Entry e = 64 s + lane lives in slot s of that lane; the
// order is ascending (key, index), a strict total order, so the k smallest are unique and candidates may come in any
// order.  A candidate below the list's k-th entry is inserted by a shift across the lanes.
#pragma once
#include "dst_device.hpp"

namespace dst {
namespace {

constexpr int kSlots = (int)(kNearestMaxK / 64);
constexpr uint64_t kSentinelVal = 0x7FFFFFFFFFFFFFFFull;   // key ~0 for both the int64 and the f64 payloads
constexpr uint32_t kSentinelIdx = 0xFFFFFFFFu;

__device__ __forceinline__ bool nn_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib)
{
    return ka < kb || (ka == kb && ia < ib);
}

__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint32_t shfl32(uint32_t x, int src) { return (uint32_t)__shfl((int)x, src, 64); }

// W consecutive 32-bit words as one 4 / 8 / 16-byte access where W allows it (p aligned to it), else word by word
template <int W>
__device__ __forceinline__ void load_words(const uint32_t *__restrict__ p, uint32_t *o)
{
    if constexpr (W == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else if constexpr (W == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        o[0] = v.x, o[1] = v.y;
    } else {
#pragma unroll
        for (int t = 0; t < W; ++t)
            o[t] = p[t];
    }
}
template <int W>
__device__ __forceinline__ void store_words(uint32_t *p, const uint32_t *o)
{
    if constexpr (W == 4) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (W == 2) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(o[0], o[1]);
    } else {
#pragma unroll
        for (int t = 0; t < W; ++t)
            p[t] = o[t];
    }
}

// one record's list, spread over the wave
template <int W>
struct WaveList {
    uint64_t key[kSlots], val[kSlots];
    uint32_t idx[kSlots], tal[kSlots][W];
    uint64_t thr_key;   // entry k-1
    uint32_t thr_idx;

    // the empty list: every entry the sentinel (a key above every real one, index 2^32-1)
    __device__ void clear()
    {
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            val[s] = kSentinelVal;
            idx[s] = kSentinelIdx;
            key[s] = ~0ull;
#pragma unroll
            for (int t = 0; t < W; ++t)
                tal[s][t] = 0;
        }
        thr_key = ~0ull;
        thr_idx = kSentinelIdx;
    }

    // WA < W: the entry's words in two arrays, [0, WA) in ltal (WA per entry) and [WA, W) in lext (W - WA per entry)
    template <bool INT, int WA = W>
    __device__ void load(const uint64_t *lval, const uint32_t *lidx, const uint32_t *ltal, uint64_t base, uint32_t k, int lane,
                         const uint32_t *lext = nullptr)
    {
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const uint32_t e = (uint32_t)(s * 64 + lane);
            if (e < k) {
                val[s] = lval[base + e];
                idx[s] = lidx[base + e];
                if constexpr (WA == W) {
#pragma unroll
                    for (int t = 0; t < W; ++t)
                        tal[s][t] = ltal[(base + e) * W + t];
                } else {
                    load_words<WA>(ltal + (base + e) * WA, tal[s]);
                    load_words<W - WA>(lext + (base + e) * (W - WA), tal[s] + WA);
                }
                key[s] = idx[s] == kSentinelIdx ? ~0ull : nn_key<INT>(val[s]);
            } else {
                val[s] = kSentinelVal;
                idx[s] = kSentinelIdx;
                key[s] = ~0ull;
#pragma unroll
                for (int t = 0; t < W; ++t)
                    tal[s][t] = 0;
            }
        }
        threshold(k);
    }

    template <int WA = W>
    __device__ void store(uint64_t *lval, uint32_t *lidx, uint32_t *ltal, uint64_t base, uint32_t k, int lane,
                          uint32_t *lext = nullptr) const
    {
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const uint32_t e = (uint32_t)(s * 64 + lane);
            if (e < k) {
                lval[base + e] = val[s];
                lidx[base + e] = idx[s];
                if constexpr (WA == W) {
#pragma unroll
                    for (int t = 0; t < W; ++t)
                        ltal[(base + e) * W + t] = tal[s][t];
                } else {
                    store_words<WA>(ltal + (base + e) * WA, tal[s]);
                    store_words<W - WA>(lext + (base + e) * (W - WA), tal[s] + WA);
                }
            }
        }
    }

    __device__ void threshold(uint32_t k)
    {
        const int s_t = (int)((k - 1) / 64), l_t = (int)((k - 1) % 64);
        uint64_t kk = 0;
        uint32_t ii = 0;
#pragma unroll
        for (int s = 0; s < kSlots; ++s)
            if (s == s_t) {   // (wave-uniform)
                kk = key[s];
                ii = idx[s];
            }
        thr_key = shfl64(kk, l_t);
        thr_idx = shfl32(ii, l_t);
    }

    // the candidate (wave-uniform) is below entry k-1: it goes where it belongs, the entries behind it move up one
    __device__ void insert(uint64_t ck, uint64_t cv, uint32_t ci, const uint32_t *ct, uint32_t k, int lane)
    {
        uint32_t pos = 0;
#pragma unroll
        for (int s = 0; s < kSlots; ++s)
            pos += (uint32_t)__popcll(__ballot(nn_less(key[s], idx[s], ck, ci)));
        const int from = lane == 0 ? 63 : lane - 1;
#pragma unroll
        for (int s = kSlots - 1; s >= 0; --s) {
            // entry e - 1: the lane below in this slot, or lane 63 of the slot before for lane 0
            uint64_t pk = shfl64(key[s], from), pv = shfl64(val[s], from);
            uint32_t pi = shfl32(idx[s], from), pt[W];
#pragma unroll
            for (int t = 0; t < W; ++t)
                pt[t] = shfl32(tal[s][t], from);
            if (s > 0) {
                const uint64_t qk = shfl64(key[s - 1], 63), qv = shfl64(val[s - 1], 63);
                const uint32_t qi = shfl32(idx[s - 1], 63);
                uint32_t qt[W];
#pragma unroll
                for (int t = 0; t < W; ++t)
                    qt[t] = shfl32(tal[s - 1][t], 63);
                if (lane == 0) {
                    pk = qk;
                    pv = qv;
                    pi = qi;
#pragma unroll
                    for (int t = 0; t < W; ++t)
                        pt[t] = qt[t];
                }
            }
            const uint32_t e = (uint32_t)(s * 64 + lane);
            if (e > pos) {
                key[s] = pk;
                val[s] = pv;
                idx[s] = pi;
#pragma unroll
                for (int t = 0; t < W; ++t)
                    tal[s][t] = pt[t];
            } else if (e == pos) {
                key[s] = ck;
                val[s] = cv;
                idx[s] = ci;
#pragma unroll
                for (int t = 0; t < W; ++t)
                    tal[s][t] = ct[t];
            }
        }
        threshold(k);
    }

    // every lane of `mask` offers its candidate, lowest lane first (the order does not matter: a total order)
    template <bool INT>
    __device__ void offer(uint64_t mask, bool pass, uint64_t ck, uint64_t cv, uint32_t ci, const uint32_t *ct, uint32_t k, int lane)
    {
        while (mask) {
            const int src = __ffsll((unsigned long long)mask) - 1;
            const uint64_t bk = shfl64(ck, src), bv = shfl64(cv, src);
            const uint32_t bi = shfl32(ci, src);
            uint32_t bt[W];
#pragma unroll
            for (int t = 0; t < W; ++t)
                bt[t] = shfl32(ct[t], src);
            insert(bk, bv, bi, bt, k, lane);
            mask &= ~(1ull << src);
            mask &= __ballot(pass && nn_less(ck, ci, thr_key, thr_idx));
        }
    }
};

}  // namespace
}  // namespace dst
