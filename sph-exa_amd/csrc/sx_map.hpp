/*! @file sx_map.hpp
 * @brief Column-density and slice maps of the particles (sx_map.hip): the reduction of the state to an image.
 *
 * Each particle's footprint is binned into tiles of 16 x 16 pixels and one workgroup per tile gathers its list in
 * ascending particle index: fixed order, no float atomics, so the image does not depend on scheduling.  The pairs
 * tile << 32 | particle, their bands of whole tile rows under a cap and their sort are the pair-binning engine's
 * (sx_pairbin.hpp); a tile's list is the same whatever the banding, so the image is bit-identical for every cap.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sphexa_hip.h"
#include "sx_pairbin.hpp"
#include "sx_tree.hpp"

namespace sx::map
{

constexpr int      kTile   = 16;   //!< pixels per tile edge: 256 pixels, one per lane of the workgroup
constexpr uint32_t kChunk  = 256;  //!< records staged through LDS at a time (one per lane, 8 KB)
constexpr uint32_t kMaxPix = 4096; //!< largest npix per direction

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

/*! the pair scratch and the last render's figures (bin: every "map.*" tag of the engine), and the driver's images */
struct MapBuffers
{
    pairbin::Buffers bin; // counts[0]: particles with a footprint in the window; rows: tile rows
    double *         img{nullptr}, *imgHost{nullptr}; // sx_sim_render: the two device images and their pinned copy
                                                      // (requested there; unused by a context)
};

/*! renders a.spec over [first, last) into a.sum0 (and a.sum1 when a.a is set) on stream s.  Synchronises the stream once,
 *  after the counting pass: the band plan is made on the host.  Returns an SX_* code; err receives the reason. */
int render(Arena& arena, MapBuffers& b, const Args& a, hipStream_t s, std::string& err);
//! the engine's words for the maps; stats: {pairs, bands, longest tile list, particles with a footprint in the window}
//! (after a count / emit disagreement the image lacks contributions: SX_ERR_HIP with the last text)
constexpr pairbin::Names kNames{"sx_map_render",
                                "sx_map_render",
                                "tile row",
                                "(render a smaller window or fewer particles at a time)",
                                "sx_set_map_pair_cap",
                                "map.",
                                "nothing has been rendered",
                                "the last render's emit pass disagreed with its count pass: the image is incomplete"};

} // namespace sx::map
