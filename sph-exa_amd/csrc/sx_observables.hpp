/*! @file sx_observables.hpp
 * @brief Conserved-quantity reduction and the fused observables pass (sx_observables.hip).
 */
#pragma once

#include "sx_device.hpp"

#include <algorithm>

namespace sx
{

struct ConservedArgs
{
    size_t          first, last;
    const double *  x, *y, *z;
    const float *   vx, *vy, *vz, *m;
    const double*   temp; // used with cv when u is null
    const double*   u;    // nullable
    const uint32_t* nc;   // nullable
    double          cv;
};

//! doubles of scratch for n particles
size_t conservedScratch(size_t n);
//! out[0..8]: 0.5 sum m v^2, sum u m (or cv T m), linear momentum (3), angular momentum (3), sum nc
hipError_t conservedQuantities(const ConservedArgs& a, double* scratch, double* out, hipStream_t s);

//! the observables of main/src/observables/factory.hpp:46-69 (SX_OBS_* of sphexa_hip.h, same values)
enum ObsKind : int
{
    kObsTimeEnergy = 0,
    kObsMachRms    = 1,
    kObsKhGrowth   = 2,
    kObsWindBubble = 3,
    kObsGravWaves  = 4,
    kObsKinds      = 5
};

constexpr int kObsConserved = 9;  // the sums of conservedQuantities, in its order
constexpr int kObsMaxSums   = 15; // + the six d2Q sums of the gravitational waves

//! extra sums of a kind: 0, 1 (sum |v|^2/c^2), 3 (si, ci, di), 1 (cloud particles), 6 (d2Q xx yy zz xy xz yz)
constexpr int obsExtraSums(int kind)
{
    return kind == kObsMachRms ? 1 : kind == kObsKhGrowth ? 3 : kind == kObsWindBubble ? 1 : kind == kObsGravWaves ? 6 : 0;
}

struct ObsArgs
{
    ConservedArgs c;         // [first, last) and the fields of the conserved sums
    bool          conserved; // false: the nine conserved sums are not formed (they read as zero) and only the kind's
                             // fields are touched
    const float*  cs;        // speed of sound (Mach RMS)
    const float * kx, *xm;   // VE normalisation and definition (KH growth, wind bubble)
    const float * ax, *ay, *az; // gravitational waves
    double        ybox;      // box.ly() (KH growth)
    double        rhoMin;    // 0.64 rhoBubble (wind bubble)
    double        tempMax;   // 0.9 tempWind
};

//! doubles of scratch of the fused pass: one partial per workgroup and sum, the grid is a function of n alone
size_t observablesScratch();
/*! one pass over [first, last): out[0..8] as conservedQuantities, out[9..9 + obsExtraSums(kind)) the kind's sums
 *  (the gravitational-wave diagonal already times 2/3), then out[9 + extra] = last - first as a double */
hipError_t observables(int kind, const ObsArgs& a, double* scratch, double* out, hipStream_t s);

} // namespace sx
