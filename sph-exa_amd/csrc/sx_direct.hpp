/*! @file sx_direct.hpp
 * @brief direct-sum gravity (sx_direct.hip): arguments and launchers behind sx_gravity_direct.
 *
 * Replaces ryoanji::directSum (ryoanji/src/ryoanji/nbody/direct.cuh:52-123; the CPU form
 * nbody/traversal_cpu.hpp:234-270).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace sx::direct
{

constexpr uint32_t kThreads = 256; //!< threads of a workgroup; targets of a block per target-per-lane
constexpr uint32_t kTile    = 256; //!< sources staged in LDS at a time, one per thread
//! targets a lane of the fast kernel carries.  Two halve the LDS reads per interaction and change nothing beyond the
//! spread between runs: the loop is bound by its vector instructions (A/B in DESIGN.md 7f: 524k x 524k in 89.3 and
//! 89.9 ms with one, 87.1 and 90.8 ms with two)
constexpr uint32_t kDefaultTargetsPerLane = 1;

/*! The targets are slots 0 .. numTargets-1: slot t is particle first + t ([first, last) views) or targets[t] (explicit
 *  groups, flattened in group order by the caller).  Workgroup (bx, by) takes the slots [bx, bx + 1) * kThreads *
 *  targetsPerLane and the source tiles [by, by + 1) * tilesPerSplit and writes its sums {phi, ax, ay, az} to
 *  partial[(by * numTargets + slot) * 4]. */
struct DirectArgs
{
    uint32_t        numTargets, first;
    const uint32_t* targets;
    uint32_t        n; // sources [0, n)
    const double *  x, *y, *z;
    const float *   m, *h;
    float *         ax, *ay, *az; // nullable (all three)
    double*         out4;         // nullable, 4 n
    float           G;
    int             numShells;
    double          boxL[3];
    uint32_t        splits, tilesPerSplit, targetsPerLane;
    double*         partial; // splits x numTargets x 4
    double*         blockE;  // combineBlocks(numTargets) sums of G m_i phi_i
    double*         egrav;   // device scalar: 0.5 sum of blockE in order
};

inline uint32_t sourceTiles(uint32_t n) { return (n + kTile - 1) / kTile; }
inline uint32_t targetBlocks(uint32_t numTargets, uint32_t targetsPerLane)
{
    return (numTargets + kThreads * targetsPerLane - 1) / (kThreads * targetsPerLane);
}
inline uint32_t combineBlocks(uint32_t numTargets) { return (numTargets + kThreads - 1) / kThreads; }

/*! splits and tiles per split of a.numTargets x a.n: requested == 0 is the automatic rule
 *  clamp(ceil(16 * 256 / targetBlocks), 1, sourceTiles) -- sixteen workgroups for each of the 256 CUs: with four (about
 *  as many workgroups as the chip holds at once) some CUs run five where others run four, and 4096 targets against
 *  14M sources took 27.1 ms instead of 21.8; a request beyond sourceTiles is clamped.  The tiles are
 *  dealt ceil(tiles / splits) per split and splits without a tile are dropped. */
inline void planSplits(DirectArgs& a, uint32_t requested)
{
    const uint32_t tiles = std::max(1u, sourceTiles(a.n));
    const uint32_t tb    = std::max(1u, targetBlocks(a.numTargets, a.targetsPerLane));
    uint32_t       k     = requested ? requested : (16u * 256u + tb - 1) / tb;
    k                    = std::min(std::min(std::max(k, 1u), tiles), 65535u); // gridDim.y
    a.tilesPerSplit      = (tiles + k - 1) / k;
    a.splits             = (tiles + a.tilesPerSplit - 1) / a.tilesPerSplit;
}

//! the reference's loop in double (images outermost, sources ascending)
hipError_t directExact(const DirectArgs& a, hipStream_t s);
//! packed float on LDS tiles (tiles outermost, images inside)
hipError_t directFast(const DirectArgs& a, hipStream_t s);
//! splits added in ascending order, the output stage, *egrav
hipError_t directCombine(const DirectArgs& a, hipStream_t s);

} // namespace sx::direct
