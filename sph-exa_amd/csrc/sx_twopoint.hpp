/*! @file sx_twopoint.hpp
 * @brief Two-point statistics of the particles: pair counts and longitudinal velocity structure functions binned by
 *        separation, with exact, order-independent sums (sx_twopoint.hip, sx_sim_twopoint.cpp).  The definitions --
 *        particles, targets, pairs, separation, bins, terms, series, windows -- are the header comment of the section in
 *        include/sphexa_hip.h; this file holds the spec check, the grid decision and the typed owner of the scratch.
 *
 * The grid and the index of the particles by cell are those of the group finder (sx_cellgrid.hpp) with r_max =
 * edges[nbins] in the place of the linking length.
 * The number format is the profiles' (sx_exactsum.hpp) with shift 64 and windows that follow from the largest velocity
 * component and mass alone, so one cheap pass over the particles fixes them and the pairs are walked once.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_cellgrid.hpp"
#include "sx_exactsum.hpp"
#include "sx_step_timer.hpp"

namespace sx::twopoint
{

constexpr int      kShift        = 64;
constexpr int      kSeries       = 6; //!< U1 U2 U3 A3 T2 WW, in the order of their flags
constexpr uint32_t kMaxBins      = SX_TP_MAX_BINS;
constexpr uint64_t kMaxParticles = 0x7fffffffull;
constexpr int      kBlock        = 256;
//! the particle flags of the window pass
constexpr uint8_t kFinite = 1, kTarget = 2;

//! the reason sx_twopoint_check refuses, with its figures; empty: accepted
std::string checkSpec(const sx_twopoint* p, const sx_box* box);
//! the cell grid of sx_twopoint_grid; p and box have passed checkSpec
void chooseGrid(const sx_twopoint& p, const sx_box& box, uint64_t n, uint32_t dims[3]);
//! the reason a call on [first, last) of f is refused, or empty: checkSpec, the columns, the range
std::string whyRefused(const sx_twopoint* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_twopoint_result* res);

/*! the typed owner of the scratch and the last call's figures.  Every "twopoint.*" arena tag is requested at one site,
 *  the cell index's seven (cellgrid::Index) in cellgrid::build, the others in sx_twopoint.hip, which stores them here. */
struct TwoPointBuffers
{
    cellgrid::Index grid;
    // the window pass: per particle of the range its flags; [vmax key, mmax key]
    uint8_t*  flags{nullptr};
    uint32_t* winKeys{nullptr};
    // the sorted columns of the pair kernel
    double * xs{nullptr}, *ys{nullptr}, *zs{nullptr};
    float *  vxs{nullptr}, *vys{nullptr}, *vzs{nullptr}, *ms{nullptr};
    uint8_t* flagsSorted{nullptr};
    double*  edges{nullptr}; // nbins + 1, uploaded
    // [pairs tested, coincident, targets, nonfinite | count nbins | sums (low, high) x kSeries x nbins]
    uint64_t* acc{nullptr};
    // [count nbins | U1 .. WW: nbins each | targets, nonfinite, coincident, pairs tested]
    uint64_t *out{nullptr}, *outHost{nullptr};
    bool          done{false};
    StageClock<4> clock; // grid, windows and gather, pairs, conversion
    uint64_t      stats[5]{};
};

constexpr size_t kHead = 4; //!< the counters in front of acc
inline size_t accWords(uint32_t nbins) { return kHead + (size_t)nbins * (1 + 2 * kSeries); }
inline size_t outWords(uint32_t nbins) { return (size_t)nbins * (1 + kSeries) + 4; }

/*! all stages over [first, last) of f; the results go to the non-null arrays of res, device pointers (toHost false) or
 *  host pointers (true, through the pinned copy of the packed result).  Synchronises at the end. */
int compute(Arena& arena, TwoPointBuffers& b, const sx_twopoint& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, const uint64_t* id, const sx_twopoint_result& res, bool toHost, hipStream_t s,
            std::string& err);
inline void release(TwoPointBuffers& b) { b.clock.release(); }

} // namespace sx::twopoint
