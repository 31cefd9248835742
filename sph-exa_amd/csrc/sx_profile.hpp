/*! @file sx_profile.hpp
 * @brief Binned profiles of the particles with exact, order-independent sums (sx_profile.hip, sx_sim_profile.cpp).  The
 *        definitions -- displacement, coordinate, bins, quantities, solutions, series -- are the header comment of the
 *        section in include/sphexa_hip.h; this file holds the number format, shared by the host helpers and the kernels.
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

#include <functional>
#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_tree.hpp"

namespace sx::profile
{

constexpr int      kMaxQ      = SX_PROF_MAX_Q;
constexpr int      kMaxSeries = 1 + 3 * kMaxQ;
constexpr uint32_t kMaxBins   = 4096;
constexpr uint32_t kMaxTable  = 1u << 20;
constexpr uint32_t kLdsBytes  = 65536 - 128; //!< a workgroup's share of the CU's 160 KB: two workgroups stay resident
constexpr int      kBlock     = 256;
constexpr int      kNumCodes  = 11;    //!< quantity codes
constexpr int      kKeyWords  = 1 + kMaxSeries; //!< [refusals | window key per series]
constexpr int32_t  kZeroWindow = -1074;
constexpr uint64_t kMaxParticles = 0x7fffffffull;

struct U128
{
    uint64_t lo, hi;
};

#define SX_PROF_HD __host__ __device__ __forceinline__

SX_PROF_HD uint64_t doubleBits(double t)
{
    union
    {
        double   d;
        uint64_t u;
    } c;
    c.d = t;
    return c.u;
}

SX_PROF_HD double bitsDouble(uint64_t u)
{
    union
    {
        double   d;
        uint64_t u;
    } c;
    c.u = u;
    return c.d;
}

SX_PROF_HD int bitLength(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

SX_PROF_HD bool finiteBits(uint64_t bits) { return ((bits >> 52) & 0x7ff) != 0x7ff; }

//! the window key of a finite t: 0 for a zero, else E + 1074 with E the smallest integer with |t| < 2^E
SX_PROF_HD uint32_t windowKey(double t)
{
    const uint64_t bits = doubleBits(t) & 0x7fffffffffffffffull;
    const uint32_t be   = (uint32_t)(bits >> 52);
    return be ? be + 52 : (uint32_t)bitLength(bits);
}

SX_PROF_HD int32_t windowOfKey(uint32_t key) { return (int32_t)key - 1074; }

constexpr int kShift = 96; //!< the profile's fixed point: fixed(t) = sign(t) floor(|t| 2^(kShift - E))

//! sign(t) floor(|t| 2^(shift - E)); |t| < 2^(E + 128 - shift - 1) (a larger term would lose its top bits: the callers rule it out)
SX_PROF_HD U128 toFixedShift(double t, int32_t E, int shift)
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

//! fixed(t) of window E; |t| < 2^E
SX_PROF_HD U128 toFixed(double t, int32_t E) { return toFixedShift(t, E, kShift); }

SX_PROF_HD void addFixed(U128& acc, U128 v)
{
    const uint64_t lo = acc.lo + v.lo;
    acc.hi += v.hi + (lo < acc.lo ? 1 : 0);
    acc.lo = lo;
}

//! the double nearest (ties to even) to acc 2^(E - shift), acc a 128-bit two's-complement integer
SX_PROF_HD double fromFixedShift(U128 acc, int32_t E, int shift)
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

SX_PROF_HD double fromFixed(U128 acc, int32_t E) { return fromFixedShift(acc, E, kShift); }

//! finite doubles as u64 whose order is the doubles' (min and max per bin through integer atomics)
SX_PROF_HD uint64_t orderKey(double d)
{
    const uint64_t b = doubleBits(d);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
SX_PROF_HD double fromOrderKey(uint64_t k) { return bitsDouble((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }

//! bytes of accumulators per internal bin: the 128-bit sums, min and max as order keys, the count
constexpr uint32_t bytesPerBin(int nq) { return 16u * (1 + 3 * nq) + 16u * nq + 8u; }
//! the largest nbins the block-private path takes
constexpr uint32_t ldsBins(int nq)
{
    const uint32_t b = kLdsBytes / bytesPerBin(nq);
    return b > 2 ? (b - 2 < kMaxBins ? b - 2 : kMaxBins) : 0;
}

//! the reason sx_profile_check refuses, or nullptr
const char* checkSpec(const sx_profile* p, const sx_box* box);
//! the reason the quantity `code` cannot be read from f (a NULL column), or nullptr
const char* missingColumns(int code, const sx_fields& f, int std);

//! the reason a call on n particles of f is refused, or nullptr: checkSpec, the coordinates, the columns, the count
const char* whyRefused(const sx_profile* p, const sx_box* box, const sx_fields& f, int std, size_t n);

//! the collectives of sx_sim_profile; all unset on one rank
struct Reduce
{
    std::function<bool(uint32_t*, size_t)> maxU32, sumU32;
    std::function<bool(double*, size_t)>   minF64;
};

/*! the typed owner of the accumulators, uploaded edges and tables, and the last call's figures.  Every "prof.*" arena
 *  tag is requested at one site in sx_profile.hip, which stores the pointer here. */
struct ProfBuffers
{
    uint32_t* keys{nullptr};     // kKeyWords: refusals, window key per series
    uint32_t* keysHost{nullptr}; // pinned
    uint64_t* acc{nullptr};      // [nonfinite | sums 2 x series x bins | count bins | min nq x bins | max nq x bins]
    uint32_t* limbs{nullptr};    // the integer part of acc as 16-bit limbs, for the u32-sum reduction
    double*   minmax{nullptr};   // [min | -max] as doubles, for the f64-min reduction
    double*   edges{nullptr};
    double*   table{nullptr};
    uint64_t* out{nullptr};      // [count bins | nonfinite | W bins | S1, S2, D, min, max: nq x bins each]
    uint64_t* outHost{nullptr};  // pinned
    bool      useLds{true};
    uint32_t  numCus{0};         // compute units of the device (the fixed grids), read by the first call
    bool      timing{false}, done{false};
    float     ms[3]{};
    double    passBytes{0};
    uint64_t  stats[4]{};
    hipEvent_t ev[4]{};
};

//! words of the packed result for nbins bins and nq quantities
inline size_t outWords(uint32_t nbins, uint32_t nq) { return 1 + (size_t)(nbins + 2) * (2 + 5 * nq); }

/*! all stages over [first, last) of f into b.out (device).  refused (nullable): this rank's reason not to take part; with
 *  collectives it still joins the first one, then returns SX_ERR_ARG with that reason.  Synchronises once when
 *  collectives are set (the refusal word) and once at the end when timing. */
int compute(Arena& arena, ProfBuffers& b, const sx_profile& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, float muiConst, double gamma, int std, const char* refused, const Reduce& reduce,
            hipStream_t s, std::string& err);
//! where the arrays of a result lie in the packed one (words of 8 bytes)
struct Piece
{
    void*  dst;
    size_t off, words;
};
//! the non-null arrays of res as pieces of the packed result; returns their number
inline int pieces(uint32_t nbins, uint32_t nq, const sx_profile_result& res, Piece out[8])
{
    const size_t nb = nbins + 2;
    const Piece  all[8] = {{res.count, 0, nb},
                           {res.nonfinite, nb, 1},
                           {res.W, nb + 1, nb},
                           {res.S1, 2 * nb + 1, nq * nb},
                           {res.S2, (2 + nq) * nb + 1, nq * nb},
                           {res.D, (2 + 2 * nq) * nb + 1, nq * nb},
                           {res.min, (2 + 3 * nq) * nb + 1, nq * nb},
                           {res.max, (2 + 4 * nq) * nb + 1, nq * nb}};
    int k = 0;
    for (const Piece& p : all)
        if (p.dst && p.words) out[k++] = p;
    return k;
}
void release(ProfBuffers& b);

} // namespace sx::profile
