/*! @file sx_halo.hpp
 * @brief Properties of the friends-of-friends groups (sx_halo.hip, sx_sim_halos.cpp): a density cut in front of the
 *        linker, the central moments of every catalogue group and its gravitational self-energy.  The definitions are
 *        the header comment of the section in include/sphexa_hip.h; this file holds the host decisions and the typed
 *        owner of the scratch.
 *
 * The search itself is sx_fof.hip's, with its buffers (FofBuffers): the catalogue stage leaves the members of every
 * catalogue group contiguous and in ascending id (memSorted, segStart, outCount) and mass, centre and velocity in
 * outReal.  The two passes here read those.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_fof.hpp"
#include "sx_step_timer.hpp"

namespace sx::halo
{

constexpr int      kBlock          = 256;
constexpr uint32_t kTile           = 256;      //!< members per tile of the pair kernel: one per lane
constexpr uint32_t kDefaultPairCap = 1u << 20; //!< maxPairMembers == 0
constexpr uint32_t kAllFlags       = SX_HALO_MOMENTS | SX_HALO_THERMAL | SX_HALO_POTENTIAL;
//! doubles per catalogue entry of HaloBuffers::out: sigma 6, shape 6, angmom 3, rmax, eint, epot
constexpr int kOutPerGroup = 18;

//! the sx_fof a specification searches with
inline sx_fof fofOf(const sx_halo& p) { return sx_fof{p.linking, p.minMembers, p.maxGroups}; }
//! the seven arrays a result shares with sx_fof_result
inline sx_fof_result fofOf(const sx_halo_result& r)
{
    return sx_fof_result{r.label, r.groupLabel, r.groupCount, r.groupMass, r.groupCom, r.groupVel, r.numGroups};
}

//! the reason sx_halo_check refuses, with its figures; empty: accepted
std::string checkSpec(const sx_halo* p, const sx_box* box);
//! the reason a call on [first, last) of f is refused, or empty: checkSpec, sx_fof's reasons, the columns
std::string whyRefused(const sx_halo* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_halo_result* res);

/*! the typed owner of the scratch beyond FofBuffers and the last call's figures.  Every "halo.*" arena tag is requested
 *  at one site, in sx_halo.hip, which stores the pointer here. */
struct HaloBuffers
{
    double*   out{nullptr};     // [sigma 6 G | shape 6 G | angmom 3 G | rmax G | eint G | epot G]
    double*   outHost{nullptr}; // pinned: the same, for host results
    uint64_t *items{nullptr}, *itemStart{nullptr}; // work items per catalogue group (G + 1) and their exclusive sum
    void*     scanTmp{nullptr};
    double*   partial{nullptr}; // one per work item
    uint64_t *counters{nullptr}, *countersHost{nullptr}; // pair terms, work items, groups with epot, over the cap; total
    bool          done{false};
    StageClock<4> clock; // group search, moments, pair kernel, combination and copies
    uint64_t      stats[4]{};
};

/*! the search (fof::compute on fb) and the passes the flags ask for over [first, last) of f; the results go to the
 *  non-null arrays of res, device pointers (toHost false) or host pointers (true).  Synchronises. */
int compute(Arena& arena, fof::FofBuffers& fb, HaloBuffers& b, const sx_halo& p, const sx_fields& f, const sx_box& box,
            uint32_t first, uint32_t last, const uint64_t* id, const sx_halo_result& res, bool toHost, hipStream_t s,
            std::string& err);
inline void release(HaloBuffers& b) { b.clock.release(); }

} // namespace sx::halo
