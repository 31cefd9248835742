/*! @file sx_args.hpp
 * @brief kernel argument structs from a field view (sx_fields), parameters and the box: the one mapping behind the
 *        stateless C API (sx_capi.cpp) and the step drivers of sx_sim (sx_sim_internal.hpp)
 *
 * The builders request nothing from an arena and set only what both callers set alike; what differs between them
 * (packed records, kernel tables, the time-step source, scratch) stays at the call site.  [first, last) indexes into
 * the view's arrays.
 */
#pragma once

#include "../../include/sphexa_hip.h"
#include "sx_hydro.hpp"
#include "sx_nbody.hpp"
#include "sx_observables.hpp"
#include "sx_tree.hpp"

namespace sx
{

//! the part of PairArgs that depends on the fields, the neighbor lists, the parameters and the box alone
inline PairArgs pairArgsCommon(uint32_t first, uint32_t last, const sx_fields& f, const NbLists& nb, const sx_params& p,
                               const DevBox& box)
{
    PairArgs a{};
    a.first = first, a.last = last;
    a.numGroups  = (uint32_t)((size_t(last - first) + kGroupSize - 1) / kGroupSize);
    a.ngmax      = p.ngmax;
    a.localLists = nb.local;
    a.nidx = nb.nidx, a.nloc = nb.nloc, a.uni = nb.uni, a.ucount = nb.ucount, a.ucap = nb.ucap;
    a.packMax = nb.packMax;
    a.nc      = f.nc;
    a.box     = box;
    a.K       = p.K;
    a.xm = f.xm, a.kx = f.kx, a.gradh = f.gradh;
    a.c11 = f.c11, a.c12 = f.c12, a.c13 = f.c13, a.c22 = f.c22, a.c23 = f.c23, a.c33 = f.c33;
    a.divv = f.divv, a.curlv = f.curlv, a.alpha = f.alpha;
    a.ax = f.ax, a.ay = f.ay, a.az = f.az, a.du = f.du;
    a.alphamin = p.alphamin, a.alphamax = p.alphamax, a.decay_constant = p.decay_constant;
    a.Atmin = p.Atmin, a.Atmax = p.Atmax, a.ramp = p.ramp, a.Kcour = (float)p.Kcour;
    a.dV11 = f.dV11, a.dV12 = f.dV12, a.dV13 = f.dV13, a.dV22 = f.dV22, a.dV23 = f.dV23, a.dV33 = f.dV33;
    return a;
}

//! computePositions of [first, last); the caller sets the time-step (dt and dt_m1, or dtPtr) and the optional outputs
inline PosArgs posArgs(uint32_t first, uint32_t last, const sx_fields& f, const DevBox& box, float muiConst, double gamma)
{
    PosArgs a{};
    a.first = first, a.last = last;
    a.box = box;
    a.x = f.x, a.y = f.y, a.z = f.z;
    a.x_m1 = f.x_m1, a.y_m1 = f.y_m1, a.z_m1 = f.z_m1;
    a.vx = f.vx, a.vy = f.vy, a.vz = f.vz;
    a.ax = f.ax, a.ay = f.ay, a.az = f.az;
    a.temp = f.temp, a.du = f.du, a.du_m1 = f.du_m1;
    a.h       = f.h;
    a.constCv = idealGasCv(muiConst, gamma);
    return a;
}

//! the gravity-only position update of [first, last); the caller sets the time-step (dt and dt_m1, or dtPtr) and keys
inline NbodyPosArgs nbodyPosArgs(uint32_t first, uint32_t last, const sx_fields& f, const DevBox& box)
{
    NbodyPosArgs a{};
    a.first = first, a.last = last;
    a.box = box;
    a.x = f.x, a.y = f.y, a.z = f.z;
    a.x_m1 = f.x_m1, a.y_m1 = f.y_m1, a.z_m1 = f.z_m1;
    a.vx = f.vx, a.vy = f.vy, a.vz = f.vz;
    a.ax = f.ax, a.ay = f.ay, a.az = f.az;
    a.h = f.h;
    return a;
}

//! the conserved sums over [first, last): the internal energy from u where the view has it, else from cv * temp
inline ConservedArgs conservedArgs(size_t first, size_t last, const sx_fields& f, float muiConst, double gamma)
{
    return ConservedArgs{first, last, f.x,    f.y, f.z,  f.vx, f.vy,
                         f.vz,  f.m,  f.temp, f.u, f.nc, (double)idealGasCv(muiConst, gamma)};
}

} // namespace sx
