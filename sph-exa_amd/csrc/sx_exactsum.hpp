/*! @file sx_exactsum.hpp
 * @brief The number format of the exact, order-independent sums (sx_profile.hip, sx_twopoint.hip), shared by the host
 *        helpers and the kernels: windows and keys, the 128-bit fixed point, its atomic add and the one rounding back.
 *
 * The exact sum.  A series' window E is the smallest integer with max |term| < 2^E.  A finite double is m 2^e with an
 * integer m < 2^53; its window key is the bit length of m plus e + 1074, so E = key - 1074 and key 0 means a zero.  The
 * key is a u32 that grows with |t|: the window of many terms, blocks and ranks is an integer maximum.
 * fixed(t) = sign(t) floor(|t| 2^(96 - E)) is m shifted by e + 96 - E bits (below 2^96 in magnitude), negated in 128-bit
 * two's complement for a negative term.  Sums are 128-bit integer additions modulo 2^128 (two u64 words, the carry of
 * the low word added to the high one), so any grouping gives the same integer; 2^31 terms stay below 2^127.
 * The result is the integer times 2^(E - 96) rounded once to the nearest double, ties to even, built bit by bit.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sx::exact
{

struct U128
{
    uint64_t lo, hi;
};

#define SX_EXACT_HD __host__ __device__ __forceinline__

SX_EXACT_HD uint64_t doubleBits(double t)
{
    union
    {
        double   d;
        uint64_t u;
    } c;
    c.d = t;
    return c.u;
}

SX_EXACT_HD double bitsDouble(uint64_t u)
{
    union
    {
        double   d;
        uint64_t u;
    } c;
    c.u = u;
    return c.d;
}

SX_EXACT_HD int bitLength(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

SX_EXACT_HD bool finiteBits(uint64_t bits) { return ((bits >> 52) & 0x7ff) != 0x7ff; }

//! the window key of a finite t: 0 for a zero, else E + 1074 with E the smallest integer with |t| < 2^E
SX_EXACT_HD uint32_t windowKey(double t)
{
    const uint64_t bits = doubleBits(t) & 0x7fffffffffffffffull;
    const uint32_t be   = (uint32_t)(bits >> 52);
    return be ? be + 52 : (uint32_t)bitLength(bits);
}

SX_EXACT_HD int32_t windowOfKey(uint32_t key) { return (int32_t)key - 1074; }

//! sign(t) floor(|t| 2^(shift - E)); |t| < 2^(E + 128 - shift - 1) (a larger term would lose its top bits: the callers rule it out)
SX_EXACT_HD U128 toFixedShift(double t, int32_t E, int shift)
{
    const uint64_t bits = doubleBits(t);
    const uint32_t be   = (uint32_t)((bits >> 52) & 0x7ff);
    const uint64_t frac = bits & 0xfffffffffffffull;
    const uint64_t m    = be ? (frac | (1ull << 52)) : frac;
    const int      e    = be ? (int)be - 1075 : -1074;
    const int      s    = e + shift - E;
    U128           v{0, 0};
    if (m == 0 || s <= -64) return v;
    if (s < 0) v.lo = m >> (-s);
    else if (s == 0) v.lo = m;
    else if (s < 64) v.lo = m << s, v.hi = m >> (64 - s);
    else if (s < 128) v.hi = m << (s - 64);
    if (bits >> 63)
    {
        v.lo = ~v.lo + 1;
        v.hi = ~v.hi + (v.lo == 0 ? 1 : 0);
    }
    return v;
}

SX_EXACT_HD void addFixed(U128& acc, U128 v)
{
    const uint64_t lo = acc.lo + v.lo;
    acc.hi += v.hi + (lo < acc.lo ? 1 : 0);
    acc.lo = lo;
}

#ifdef __HIPCC__
//! p[0], p[1] += v as one 128-bit integer (LDS or global)
template<class P>
__device__ __forceinline__ void add128(P p, U128 v)
{
    if ((v.lo | v.hi) == 0) return;
    uint64_t hi = v.hi;
    if (v.lo)
    {
        const unsigned long long old = atomicAdd(p, (unsigned long long)v.lo);
        if (old + v.lo < old) ++hi;
    }
    if (hi) atomicAdd(p + 1, (unsigned long long)hi);
}
#endif

//! the double nearest (ties to even) to acc 2^(E - shift), acc a 128-bit two's-complement integer
SX_EXACT_HD double fromFixedShift(U128 acc, int32_t E, int shift)
{
    const uint64_t sign = acc.hi >> 63;
    if (sign)
    {
        acc.lo = ~acc.lo + 1;
        acc.hi = ~acc.hi + (acc.lo == 0 ? 1 : 0);
    }
    if ((acc.lo | acc.hi) == 0) return 0.0;
    const int len = acc.hi ? 64 + bitLength(acc.hi) : bitLength(acc.lo);
    // bits to drop: down to 53 significant ones, and nothing below 2^-1074
    int drop = len - 53;
    if (shift - 1074 - E > drop) drop = shift - 1074 - E;
    if (drop > 127) return bitsDouble(sign << 63); // below half of 2^-1074 whatever the 127 bits hold
    uint64_t q;
    int      exp2 = E - shift; // the value is q 2^exp2
    if (drop <= 0) q = acc.lo;
    else
    {
        // q = acc >> drop, rem = the dropped bits against half = 2^(drop - 1); drop <= 127
        uint64_t remHi, remLo, halfHi, halfLo;
        if (drop < 64)
        {
            q      = (acc.lo >> drop) | (acc.hi << (64 - drop));
            remHi  = 0;
            remLo  = acc.lo & ((1ull << drop) - 1);
            halfHi = 0;
            halfLo = 1ull << (drop - 1);
        }
        else if (drop == 64)
        {
            q      = acc.hi;
            remHi  = 0;
            remLo  = acc.lo;
            halfHi = 0;
            halfLo = 1ull << 63;
        }
        else
        {
            const int d = drop - 64; // 1 .. 63
            q      = acc.hi >> d;
            remHi  = acc.hi & ((1ull << d) - 1);
            remLo  = acc.lo;
            halfHi = 1ull << (d - 1);
            halfLo = 0;
        }
        const bool above = remHi > halfHi || (remHi == halfHi && remLo > halfLo);
        const bool tie   = remHi == halfHi && remLo == halfLo;
        if (above || (tie && (q & 1))) ++q;
        exp2 += drop;
    }
    if (q == 0) return bitsDouble(sign << 63);
    // q <= 2^53 and exp2 >= -1074: normalise towards 53 bits without going below the subnormal scale
    int lq = bitLength(q);
    if (lq < 53 && exp2 > -1074)
    {
        int sh = 53 - lq;
        if (exp2 + 1074 < sh) sh = exp2 + 1074;
        q <<= sh;
        exp2 -= sh;
        lq += sh;
    }
    if (lq == 54) q >>= 1, ++exp2;
    uint64_t out;
    if (exp2 == -1074 && lq <= 53) out = q; // subnormal, or the lowest binade, whose scale is the same
    else
    {
        const int be = exp2 + 1075;
        out          = be >= 2047 ? 0x7ffull << 52 : ((uint64_t)be << 52) | (q & 0xfffffffffffffull);
    }
    return bitsDouble(out | (sign << 63));
}

} // namespace sx::exact
