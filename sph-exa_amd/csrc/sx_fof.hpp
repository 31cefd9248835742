/*! @file sx_fof.hpp
 * @brief Friends-of-friends groups of the particles (sx_fof.hip, sx_sim_fof.cpp).  The definitions -- link criterion,
 *        groups, labels, catalogue, order of the sums -- are the header comment of the section in include/sphexa_hip.h;
 *        this file holds the grid decision, shared by the host entry points and the launcher, and the typed owner of
 *        the scratch.
 *
 * The grid and the index of the particles by cell are sx_cellgrid.hpp's, shared with the two-point statistics, with the
 * linking length as the search length.
 *
 * Union-find.  parent[] over the sorted indices, parent[i] <= i always.  A link hooks the larger root under the smaller
 * with a compare-and-swap that expects the larger to be a root still; a loser starts again from what it found there.
 * Every store to parent[] lowers it to an ancestor, so there is no cycle, a walk to the root ends, and nobody waits for
 * another wave.  The root of a component is its smallest sorted index; the label is found afterwards.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_cellgrid.hpp"
#include "sx_step_timer.hpp"

namespace sx::fof
{

constexpr uint64_t kMaxParticles = 0x7fffffffull; //!< sorted indices and hipcub's item counts are ints
constexpr int      kBlock        = 256;
constexpr uint32_t kNoGroup      = 0xffffffffu;

//! the reason sx_fof_check refuses, with its figures; empty: accepted
std::string checkSpec(const sx_fof* p, const sx_box* box);
//! the cell grid of sx_fof_grid; p and box have passed checkSpec
void chooseGrid(const sx_fof& p, const sx_box& box, uint64_t n, uint32_t dims[3]);

/*! the typed owner of the scratch and the last call's figures.  Every "fof.*" arena tag is requested at one site, the
 *  cell index's seven (cellgrid::Index) in cellgrid::build, the others in sx_fof.hip, which stores the pointer here. */
struct FofBuffers
{
    cellgrid::Index grid; // its sortTmp serves the catalogue's sorts and scan as well
    double *        xs{nullptr}, *ys{nullptr}, *zs{nullptr}; // sorted coordinates
    // union-find and labels, by sorted index; count, minId and rankOf are read at the roots
    uint32_t *parent{nullptr}, *root{nullptr}, *count{nullptr}, *rankOf{nullptr};
    uint64_t *minId{nullptr}, *label{nullptr};
    // catalogue: the selected roots, and the members by (group, id)
    uint64_t *selLabel{nullptr}, *selLabelSorted{nullptr}, *idKeys{nullptr}, *idKeysSorted{nullptr};
    uint32_t *selRoot{nullptr}, *selRootSorted{nullptr}, *selKey{nullptr}, *selKeySorted{nullptr}, *selPos{nullptr},
        *selPosSorted{nullptr};
    uint32_t *mem{nullptr}, *memById{nullptr}, *memKey{nullptr}, *memKeySorted{nullptr}, *memSorted{nullptr};
    uint32_t *segCount{nullptr}, *segStart{nullptr};
    uint64_t* outLabel{nullptr};
    uint32_t* outCount{nullptr};
    double*   outReal{nullptr}; // [mass G | com 3 G | vel 3 G]
    uint64_t *counters{nullptr}, *countersHost{nullptr}; // pair tests, union retries, all groups, selected groups
    uint32_t      catGroups{0};   // catalogue groups of the last call: entries of segStart, segCount, outCount, outReal
    bool          members{false}; // the last call sorted the members and reduced them (memSorted, outReal)
    bool          done{false};
    StageClock<4> clock; // grid, link, compress and labels, catalogue
    uint64_t      stats[4]{};
};

/*! what the group properties (sx_halo.hip) ask of the search beyond sx_fof, which passes none.  A particle is selected
 *  iff rhoMin <= 0 or its density (the rule of SX_PROF_RHO) is >= rhoMin; an unselected one gets a NaN sorted coordinate,
 *  so every link test on it fails, and is kept out of the labels and counts.  members: sort the members and reduce the
 *  catalogue whether or not res asks for mass, centre or velocity. */
struct Extra
{
    double       rhoMin{0.0};
    int          std{0};
    const float *kx{nullptr}, *xm{nullptr}, *rho{nullptr}; // m is f.m
    bool         members{false};
};

/*! all stages over [first, last) of f; the results go to the non-null arrays of res, device pointers (toHost false) or
 *  host pointers (true).  Synchronises after the compress stage (the number of groups sizes the catalogue's sorts) and
 *  at the end. */
int compute(Arena& arena, FofBuffers& b, const sx_fof& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, const uint64_t* id, const sx_fof_result& res, bool toHost, hipStream_t s, std::string& err,
            const Extra* extra = nullptr);
//! the reason a call on [first, last) of f is refused, or empty: checkSpec, the columns, the range, the capacity
std::string whyRefused(const sx_fof* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_fof_result* res);
inline void release(FofBuffers& b) { b.clock.release(); }

} // namespace sx::fof
