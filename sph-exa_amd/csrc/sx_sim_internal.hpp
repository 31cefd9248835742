/*! @file sx_sim_internal.hpp
 * @brief what the translation units of the step driver share beyond sx_sim.hpp: sx_sim.cpp (C API, step orchestrator),
 *        sx_sim_domain.cpp (SFC domain), sx_sim_gravity.cpp (self-gravity), sx_sim_skin.cpp (skin-list driver),
 *        sx_sim_nbody.cpp (gravity-only step)
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sphexa_hip.h"
#include "sx_comm.hpp"
#include "sx_gravity.hpp"
#include "sx_hydro.hpp"
#include "sx_nbody.hpp"
#include "sx_observables.hpp"
#include "sx_sim.hpp"
#include "sx_skin.hpp"
#include "sx_traverse.hpp"
#include "sx_tree.hpp"
#include "sx_turb.hpp"

extern "C" void*          sx_ctx_stream_internal(sx_ctx* c);
extern "C" int            sx_ctx_exact_internal(sx_ctx* c);
extern "C" uint32_t       sx_ctx_pack12_max_internal(sx_ctx* c);
extern "C" const float2*  sx_ctx_table_internal(sx_ctx* c, int which);
extern "C" const float*   sx_ctx_powtab_internal(sx_ctx* c, uint32_t ng0);
extern "C" sx::Transport* sx_comm_transport_internal(sx_comm* c);
extern "C" void           sx_ctx_set_error_internal(sx_ctx* c, const char* msg);

#define SIM_HIP(call)                                                                                                  \
    do {                                                                                                               \
        if ((call) != hipSuccess) return SX_ERR_HIP;                                                                   \
    } while (0)
#define SIM_COMM(call)                                                                                                 \
    do {                                                                                                               \
        if (!(call)) return SX_ERR_HIP;                                                                                \
    } while (0)

namespace sx::sim
{

constexpr int      kHistBits = 18;   // global key histogram resolution (level 6)
constexpr uint32_t kChunk    = 2048; // particles per halo request box

//! halo request box: AABB grown by the search radius
struct __attribute__((aligned(16))) ReqBox
{
    double c[3], s[3];
    double hmax;
    int32_t owner, pad;
};

static inline unsigned grid(size_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// ---- sx_sim.cpp ---------------------------------------------------------------------------------------------------

PairArgs simPairArgs(sx_sim* s);

// ---- sx_sim_domain.cpp --------------------------------------------------------------------------------------------

//! the sync's small per-rank buffers (DomBuffers but mybox) for P ranks, requested by sx_sim_set_comm so that no rank
//! fails alone between two collectives of a step; false: out of memory
bool domReserveComm(sx_sim* s, size_t P);
void packXHalos(sx_sim* s, hipStream_t st);
bool overlapping(const sx_sim* s, const HydroLaunch& H);
//! interior / boundary cluster lists of this step's search (clsList, clsCount), the counts on their way to clsHost
int classifyClusters(sx_sim* s, hipStream_t st);
int deviceCountsOrAbort(sx_sim* s, bool fail, hipStream_t st, std::vector<uint64_t>& send,
                        std::vector<uint64_t>& sendOff, std::vector<uint64_t>& recv);
//! out[q] = difference of consecutive segment boundaries (u64 or u32), q < P
void diffCounts(const uint64_t* b64, const uint32_t* b32, int P, uint64_t* out, hipStream_t st);
//! request boxes of every kChunk consecutive particles of [0, n) (one workgroup per chunk; nChunks > 0)
void chunkBoxes(const double* x, const double* y, const double* z, const float* h, size_t n, size_t nChunks,
                double margin, double qmargin, int owner, ReqBox* out, hipStream_t st);
//! flag |= 1 if some local's h exceeds its chunk's request radius (margin) after the h iteration
void chunkCheck(sx_sim* s, double margin, unsigned* flag, hipStream_t st);
int  syncErrEnqueue(sx_sim* s, hipStream_t st);
bool syncErrFailed(sx_sim* s);

// ---- sx_sim_gravity.cpp -------------------------------------------------------------------------------------------

//! the P2P / M2P counters (sx_sim_set_gravity_counting), requested where counting is switched on and by a counting step
unsigned long long* gravReserveInteractions(sx_sim* s);
//! self-gravity of the step on one rank or several, then max |a|^2; reuse: a skin-list reuse step (no sync)
int gravityStage(sx_sim* s, hipStream_t st, bool dist, bool reuse);

// ---- sx_sim_skin.cpp ----------------------------------------------------------------------------------------------

constexpr int kSkinResync = 1000; //!< skinSearch: redo this step's search from a full sync (not an error code)

//! a step's skin search on this rank: clusters, stale ones (rebuilt at once or sent to the exact search directly),
//! those rebuilt, and those that took the exact search
struct SkinCounts
{
    uint32_t clusters{0}, stale{0}, rebuilt{0}, exact{0};
};

bool skinUsable(const sx_sim* s);
void skinTooThin(SkinState& K);
bool skinParticleBuffers(sx_sim* s, PosArgs& q, hipStream_t st);
int  skinSearch(sx_sim* s, const NsArgs& na, bool reuse, hipStream_t st, float* xmOut, RecT* rtXm, SkinCounts& out);
void skinDecide(SkinState& K, bool reuse, const SkinCounts& c, uint64_t staleAll, uint64_t clustersAll);
int  skinHaloRefresh(sx_sim* s, hipStream_t st);
//! a build with several ranks: the drift bounds of coverListKernel zeroed, the locals' positions kept (x0, y0, z0)
int  skinBuildSnapshot(sx_sim* s, hipStream_t st);
//! a reuse step with several ranks: flag |= 1 when the sphere of some target of a cluster searched again this step
//! (c.rebuilt skins, c.exact exact searches) may reach particles that were no halos of the last build
int  skinCoverCheck(sx_sim* s, const SkinCounts& c, unsigned* flag, hipStream_t st);
void xmassRest(sx_sim* s, const HydroLaunch& H, PairArgs a, hipStream_t st);

} // namespace sx::sim
