/*! @file sx_profile.hpp
 * @brief Binned profiles of the particles with exact, order-independent sums (sx_profile.hip, sx_sim_profile.cpp).  The
 *        definitions -- displacement, coordinate, bins, quantities, solutions, series -- are the header comment of the
 *        section in include/sphexa_hip.h; this file holds the fixed point of the sums, the spec check and the typed
 *        owner of the scratch.
 *
 * The number format of the sums is sx_exactsum.hpp, shared with the two-point statistics; the shift of the fixed point
 * is this file's.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_exactsum.hpp"
#include "sx_step_timer.hpp"
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

using namespace exact; // U128, doubleBits, windowKey, toFixedShift, addFixed, add128, fromFixedShift, ... (sx_exactsum.hpp)

constexpr int kShift = 96; //!< the profile's fixed point: fixed(t) = sign(t) floor(|t| 2^(kShift - E))

//! fixed(t) of window E; |t| < 2^E
SX_EXACT_HD U128 toFixed(double t, int32_t E) { return toFixedShift(t, E, kShift); }

SX_EXACT_HD double fromFixed(U128 acc, int32_t E) { return fromFixedShift(acc, E, kShift); }

//! finite doubles as u64 whose order is the doubles' (min and max per bin through integer atomics)
SX_EXACT_HD uint64_t orderKey(double d)
{
    const uint64_t b = doubleBits(d);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
SX_EXACT_HD double fromOrderKey(uint64_t k) { return bitsDouble((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }

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
    bool          done{false};
    StageClock<3> clock;         // pass 1, pass 2 (with their collectives), conversion
    double        passBytes{0};
    uint64_t      stats[4]{};
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
inline void release(ProfBuffers& b) { b.clock.release(); }

} // namespace sx::profile
