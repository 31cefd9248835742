/*! @file sx_nbody.hpp
 * @brief device code of the gravity-only propagator (NbodyProp, main/src/propagator/nbody.hpp:52-171): the position
 *        update without thermal fields.  The force path is the walk of sx_gravity.hpp as it is.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sx_device.hpp"

namespace sx
{

//! computePositions with neither temp nor u (positions.hpp:77-110 + putInBox): x, v and x_m1 of [first, last)
struct NbodyPosArgs
{
    uint32_t      first, last;
    double        dt, dt_m1;
    const double* dtPtr; // if non-null: dt = dtPtr[0], dt_m1 = dtPtr[1] (the device scalars minDt, minDt_m1)
    DevBox        box;
    double *      x, *y, *z;
    float *       x_m1, *y_m1, *z_m1, *vx, *vy, *vz;
    const float * ax, *ay, *az;
    const float*  h; // read only when an axis of box is fixed
    // nullable: the next sync's SFC keys of the updated coordinates (sfcKey, box `box`), written in the same pass
    uint64_t*     keys;
};

//! one streaming pass; two particles per lane (16-byte double, 8-byte float accesses) when every array is aligned for
//! it, one per lane otherwise.  The results do not depend on which.
hipError_t nbodyIntegrate(const NbodyPosArgs& a, hipStream_t s);

} // namespace sx
