// dst_pair_sum.hpp — what one DST_OUT_DISTANCE payload adds to an exact sum (dst_summary's per-pair definition,
// include/distance_hip.h), shared by the kernels that accumulate it: dst_summary.hip and dst_group_summary.hip.
#pragma once
#include "dst_device.hpp"

namespace dst {
namespace {

// what one pair adds: links and summable partners as counts, q in its two halves
struct Acc {
    uint32_t within, summable;
    long long hi;
    unsigned long long lo;
};

template <bool INT>
__device__ __forceinline__ bool is_nan(uint64_t bits)
{
    if constexpr (INT)
        return false;
    else
        return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

// summable: q is defined (int64 payloads always; f64: |v| < 2^25, false for NaN)
template <bool INT>
__device__ __forceinline__ bool fixed_point(uint64_t bits, long long &q)
{
    if constexpr (INT) {
        q = (long long)bits;
        return true;
    } else {
        const double v = __longlong_as_double((long long)bits);
        const bool ok = fabs(v) < 0x1p25;
        q = ok ? __double2ll_rn(v * 0x1p37) : 0;   // (the product is exact: a power of two, far from overflow)
        return ok;
    }
}

template <bool INT>
__device__ __forceinline__ void add_pair(Acc &a, uint64_t bits, uint64_t t_key, bool any)
{
    long long q;
    if (fixed_point<INT>(bits, q)) {
        ++a.summable;
        a.hi += q >> 32;
        a.lo += (unsigned long long)q & 0xFFFFFFFFull;
    }
    if (any && nn_key<INT>(bits) <= t_key)
        ++a.within;
}

__device__ __forceinline__ unsigned long long shfl_down64(unsigned long long x, int off)
{
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)x, off, 64), hi = (uint32_t)__shfl_down((int)(uint32_t)(x >> 32), off, 64);
    return (unsigned long long)hi << 32 | lo;
}

// lane 0 of the wave receives the wave's sums (two's complement: the signed word adds like the unsigned ones)
__device__ __forceinline__ void wave_sum(Acc &a)
{
    unsigned long long counts = (unsigned long long)a.within << 32 | a.summable;   // (each at most 2^31 per workgroup)
    unsigned long long hi = (unsigned long long)a.hi, lo = a.lo;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        counts += shfl_down64(counts, off);
        hi += shfl_down64(hi, off);
        lo += shfl_down64(lo, off);
    }
    a.within = (uint32_t)(counts >> 32);
    a.summable = (uint32_t)counts;
    a.hi = (long long)hi;
    a.lo = lo;
}

}  // namespace
}  // namespace dst
