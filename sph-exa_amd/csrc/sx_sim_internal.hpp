/*! @file sx_sim_internal.hpp
 * @brief what the translation units of the step driver share beyond sx_sim.hpp: sx_sim.cpp (C API, step orchestrator),
 *        sx_sim_domain.cpp (SFC domain), sx_sim_gravity.cpp (self-gravity), sx_sim_skin.cpp (skin-list driver),
 *        sx_sim_nbody.cpp (gravity-only step), sx_bdt.cpp (ve-bdt substeps), and the analysis passes over the current
 *        state (sx_sim_map.cpp, sx_sim_spectrum.cpp, sx_sim_profile.cpp).  simFields is the one place that lists
 *        the sim's arrays as a field view; kernel arguments are built from that view (sx_args.hpp).  Step times go
 *        through s->timer (sx_step_timer.hpp): marks by stage and kernel name, one collect() at the end of the step.
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
#include "sx_args.hpp"
#include "sx_comm.hpp"
#include "sx_cool.hpp"
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

/*! sphexa::ParticlesData fields of the simulation from particle `offset` on (0: every particle, halos included).  A
 *  field the propagator does not keep stays NULL under an offset (the gravity-only propagator: every thermal and hydro
 *  field).  n is the caller's to set. */
inline sx_fields simFields(const sx_sim* s, size_t offset = 0)
{
    auto at = [offset](auto* p) { return p ? p + offset : nullptr; };
    sx_fields f{};
    f.x = at(s->x), f.y = at(s->y), f.z = at(s->z);
    f.x_m1 = at(s->xm1), f.y_m1 = at(s->ym1), f.z_m1 = at(s->zm1);
    f.vx = at(s->vx), f.vy = at(s->vy), f.vz = at(s->vz);
    f.rho = at(s->rho), f.p = at(s->pres), f.prho = at(s->prho);
    f.h = at(s->h), f.m = at(s->m), f.c = at(s->c);
    f.ax = at(s->ax), f.ay = at(s->ay), f.az = at(s->az);
    f.du = at(s->du), f.du_m1 = at(s->dum1), f.temp = at(s->temp);
    f.c11 = at(s->c11), f.c12 = at(s->c12), f.c13 = at(s->c13);
    f.c22 = at(s->c22), f.c23 = at(s->c23), f.c33 = at(s->c33);
    f.xm = at(s->xm), f.kx = at(s->kx), f.gradh = at(s->gradh);
    f.divv = at(s->divv), f.curlv = at(s->curlv), f.alpha = at(s->alpha);
    f.keys = at(s->keys), f.nc = at(s->nc), f.rung = at(s->rung);
    f.dV11 = at(s->dV[0]), f.dV12 = at(s->dV[1]), f.dV13 = at(s->dV[2]);
    f.dV22 = at(s->dV[3]), f.dV23 = at(s->dV[4]), f.dV33 = at(s->dV[5]);
    return f;
}

//! an SX_MAP_FIELD_* column of the sim (a null for SX_MAP_FIELD_NONE)
struct MapField
{
    const void* a{nullptr};
    int         isDouble{0};
    const char* name{nullptr};
};

/*! the column `field` for sx_sim_render and sx_sim_spectrum.  False, with the refusal in `why` behind the caller's name
 *  fn, for an unknown value and for a field the propagator's layout does not keep (a null pointer). */
inline bool mapField(const sx_sim* s, int field, const char* fn, MapField& f, std::string& why)
{
    switch (field)
    {
        case SX_MAP_FIELD_NONE: return true;
        case SX_MAP_FIELD_TEMP: f = {s->temp, 1, "temp"}; break;
        case SX_MAP_FIELD_P: f = {s->pres, 0, "p"}; break;
        case SX_MAP_FIELD_C: f = {s->c, 0, "c"}; break;
        case SX_MAP_FIELD_VX: f = {s->vx, 0, "vx"}; break;
        case SX_MAP_FIELD_VY: f = {s->vy, 0, "vy"}; break;
        case SX_MAP_FIELD_VZ: f = {s->vz, 0, "vz"}; break;
        case SX_MAP_FIELD_DIVV: f = {s->divv, 0, "divv"}; break;
        case SX_MAP_FIELD_CURLV: f = {s->curlv, 0, "curlv"}; break;
        case SX_MAP_FIELD_ALPHA: f = {s->alpha, 0, "alpha"}; break;
        case SX_MAP_FIELD_H: f = {s->h, 0, "h"}; break;
        default: why = std::string(fn) + ": unknown field"; return false;
    }
    if (f.a) return true;
    why = std::string(fn) + ": the field " + f.name + " is not kept by " +
          (s->p.propagator == 3 ? "the gravity-only propagator (none, vx, vy, vz and h are supported)"
                                : "this propagator (p exists under the std propagator only: VE keeps p / rho)");
    return false;
}

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
void skinBookkeeping(SkinState& K, bool reuse, const SkinCounts& c, uint64_t staleAll, uint64_t clustersAll);
int  skinHaloRefresh(sx_sim* s, hipStream_t st);
//! a build with several ranks: the drift bounds of coverListKernel zeroed, the locals' positions kept (x0, y0, z0)
int  skinBuildSnapshot(sx_sim* s, hipStream_t st);
//! a reuse step with several ranks: flag |= 1 when the sphere of some target of a cluster searched again this step
//! (c.rebuilt skins, c.exact exact searches) may reach particles that were no halos of the last build
int  skinCoverCheck(sx_sim* s, const SkinCounts& c, unsigned* flag, hipStream_t st);
void xmassRest(sx_sim* s, const HydroLaunch& H, PairArgs a, hipStream_t st);

} // namespace sx::sim
