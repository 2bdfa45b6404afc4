// dst_measures.hpp — the measures of the bit-plane kernels (dst_kernels.hip: the dense pair kernel over the whole width,
// dst_windows.hip: the same steps over column windows): per-32-site step on plane words + conversion of the raw
// popcounts to the reference's tallies.  q = row record (SGPR operands), t = column record (VGPR operands).
#pragma once
#include "dst_internal.h"

namespace dst {
namespace {

// The inner ops are pinned.  Left to itself hipcc rebalances the OR-of-ANDs into 5 ops instead
// of 4 and splits chained popcount-accumulates into v_bcnt(x,0) + v_add3 (1.5 issue slots per
// tally instead of 1).  Boolean steps use the gfx950 v_bitop3_b32 builtin (any function of three
// inputs, TT = f(0xF0, 0xCC, 0xAA)); the accumulate is a one-instruction asm.  Only the bcnt is
// asm: hipcc pads back-to-back dependent asm statements with s_nop (dst-forwarding hazard it
// cannot rule out), and with ordinary VALU in between the scheduler never needs to.
template <int TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t b, uint32_t c)  // (a & b) | c
{
    return bitop3<((0xF0 & 0xCC) | 0xAA)>(a, b, c);
}
__device__ __forceinline__ void bcnt_acc(uint32_t &acc, uint32_t x)  // acc += popcount(x)
{
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
}
constexpr int TT_AND3 = 0xF0 & 0xCC & 0xAA;          // a & b & c
constexpr int TT_A_AND_B_EQ_C = 0xF0 & ~(0xCC ^ 0xAA) & 0xFF;  // a & ~(b ^ c)
constexpr int TT_A_AND_B_NE_C = 0xF0 & (0xCC ^ 0xAA);          // a & (b ^ c)
constexpr int TT_A_AND_B_ANDN_C = 0xF0 & 0xCC & 0x55;          // a & b & ~c

// share = the two base sets intersect  <=>  NOT "certainly different" ((q & t) < 16 on bytes)
__device__ __forceinline__ uint32_t share_bits(const uint32_t *q, const uint32_t *t)
{
    return and_or(q[3], t[3], and_or(q[2], t[2], and_or(q[1], t[1], q[0] & t[0])));
}

struct MNHigh {  // src/measures.rs:14-23  d = #{(q&t) < 16}                       5 ops / 32 sites
    static constexpr int NP = 4, NC = 1, NT = 1, P0 = PL_A;  // planes A,G,C,T
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t)
    {
        bcnt_acc(a[0], share_bits(q, t));
    }
    static __device__ __forceinline__ void tallies(const uint32_t *a, uint32_t total, uint32_t *o)
    {
        o[0] = total - a[0];
    }
};

struct MRaw {  // src/measures.rs:56-66  same: known & equal; else different      7 ops / 32 sites
    static constexpr int NP = 5, NC = 2, NT = 2, P0 = PL_A;  // planes A,G,C,T,K
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t)
    {
        const uint32_t share = share_bits(q, t);
        bcnt_acc(a[0], share);
        bcnt_acc(a[1], bitop3<TT_AND3>(share, q[4], t[4]));  // both known and intersecting = equal
    }
    static __device__ __forceinline__ void tallies(const uint32_t *a, uint32_t total, uint32_t *o)
    {
        const uint32_t n = total - a[0];
        o[0] = n;         // n
        o[1] = n + a[1];  // d
    }
};

struct MK80 {  // src/measures.rs:85-107                                          7 ops / 32 sites
    static constexpr int NP = 4, NC = 3, NT = 3, P0 = PL_K;  // planes K,X1,X0,CL
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t)
    {
        const uint32_t e1 = q[1] ^ t[1];                                 // classes differ
        const uint32_t sc = bitop3<TT_A_AND_B_ANDN_C>(q[0], t[0], e1);   // both known, same class
        const uint32_t ts = bitop3<TT_A_AND_B_NE_C>(sc, q[2], t[2]);     // A<->G or C<->T
        const uint32_t tv = bitop3<TT_AND3>(q[3], t[3], e1);             // purine vs pyrimidine class
        bcnt_acc(a[0], sc);
        bcnt_acc(a[1], ts);
        bcnt_acc(a[2], tv);
    }
    static __device__ __forceinline__ void tallies(const uint32_t *a, uint32_t, uint32_t *o)
    {
        o[0] = a[0] + a[2];  // count_L = same + ts + tv   (sc = same + ts)
        o[1] = a[1];         // ts
        o[2] = a[2];         // tv
    }
};

struct MTN93 {  // src/measures.rs:156-175                                        8 ops / 32 sites
    static constexpr int NP = 3, NC = 4, NT = 4, P0 = PL_K;  // planes K,X1,X0
    static __device__ __forceinline__ void step(uint32_t *a, const uint32_t *q, const uint32_t *t)
    {
        const uint32_t bk = q[0] & t[0];                                 // both known
        const uint32_t sc = bitop3<TT_A_AND_B_EQ_C>(bk, q[1], t[1]);     // same class
        const uint32_t ts = bitop3<TT_A_AND_B_NE_C>(sc, q[2], t[2]);     // transition
        const uint32_t p2 = ts & q[1];                                   // ... between pyrimidines
        bcnt_acc(a[0], bk);
        bcnt_acc(a[1], sc);
        bcnt_acc(a[2], ts);
        bcnt_acc(a[3], p2);
    }
    static __device__ __forceinline__ void tallies(const uint32_t *a, uint32_t, uint32_t *o)
    {
        o[0] = a[0];                  // count_L  (same + different, both known)
        o[1] = a[0] - (a[1] - a[2]);  // count_d  = L - same
        o[2] = a[2] - a[3];           // count_P1 (A<->G)
        o[3] = a[3];                  // count_P2 (C<->T)
    }
};

}  // namespace
}  // namespace dst
