/*! @file sx_map.hpp
 * @brief Column-density and slice maps of the particles (sx_map.hip): the reduction of the state to an image.
 *
 * Each particle's footprint is binned into tiles of 16 x 16 pixels (64-bit pairs tile << 32 | particle), the pairs are
 * radix-sorted, and one workgroup per tile gathers its list in ascending particle index: fixed order, no float atomics,
 * so the image does not depend on scheduling.  Pairs are produced and consumed in bands of whole tile rows that stay
 * under a cap; a tile's list is the same whatever the banding, so the image is bit-identical for every cap.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sphexa_hip.h"
#include "sx_tree.hpp"

namespace sx::map
{

constexpr int      kTile           = 16;          //!< pixels per tile edge: 256 pixels, one per lane of the workgroup
constexpr uint32_t kChunk          = 256;         //!< records staged through LDS at a time (one per lane, 8 KB)
constexpr uint32_t kMaxPix         = 4096;        //!< largest npix per direction
constexpr uint64_t kDefaultPairCap = 1ull << 27;  //!< pairs per band (24 B each with the sort's storage)
constexpr uint64_t kMaxBandPairs   = 0x7fffffffu; //!< the sort counts its items in an int

//! the reason sx_map_check refuses a specification, or nullptr
const char* checkSpec(const sx_map* m, const sx_box* box);

//! what one render needs (device pointers; a nullable)
struct Args
{
    sx_map        spec;
    sx_box        box;
    const double *x, *y, *z;
    const float * h, *m;
    const void*   a;
    int           aIsDouble;
    uint32_t      first, last;
    double        K;
    double *      sum0, *sum1;
};

/*! the typed owner of the pair scratch and of the last render's figures.  Every "map.*" arena tag is requested at one
 *  site, in render(), which stores the pointer here. */
struct MapBuffers
{
    uint64_t            pairCap{0};       // sx_set_map_pair_cap: 0 = kDefaultPairCap
    unsigned long long* counts{nullptr};  // device: footprints, longest list, pairs per tile row
    unsigned long long* countsHost{nullptr};
    uint64_t *          pairsIn{nullptr}, *pairsOut{nullptr};
    uint32_t *          offsets{nullptr}, *cursor{nullptr};
    void*               sortTmp{nullptr};
    double *            img{nullptr}, *imgHost{nullptr}; // sx_sim_render: the two device images and their pinned copy
                                                         // (requested there; unused by a context)
    // the last render
    bool       rendered{false};
    uint64_t   pairs{0}, bands{0}, scratchBytes{0};
    bool       timing{false}; // HIP events around the stages (synchronises after every band)
    float      ms[3]{};       // binning (count + emit), sort (+ list offsets), render
    hipEvent_t ev[4]{};
};

/*! renders a.spec over [first, last) into a.sum0 (and a.sum1 when a.a is set) on stream s.  Synchronises the stream once,
 *  after the counting pass: the band plan is made on the host.  Returns an SX_* code; err receives the reason. */
int render(Arena& arena, MapBuffers& b, const Args& a, hipStream_t s, std::string& err);
//! stats(): in some band of the last render the emit pass wrote another number of pairs than the count pass had found
//! (the image then lacks contributions; the callers report SX_ERR_HIP with kStatsMismatchText)
constexpr int         kStatsMismatch     = -1;
constexpr const char* kStatsMismatchText = "the last render's emit pass disagreed with its count pass: the image is incomplete";
//! {pairs, bands, longest tile list, particles with a footprint in the window} of the last render; synchronises
int stats(MapBuffers& b, hipStream_t s, uint64_t out[4]);
void release(MapBuffers& b);

} // namespace sx::map
