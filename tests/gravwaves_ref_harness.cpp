/*! @file gravwaves_ref_harness.cpp
 * @brief C entry points over the reference's own gravitational-wave arithmetic, for tests/test_observables_ref.py.
 *
 * Includes the reference's main/src/observables/grav_waves_calculations.hpp (compiled from where it lies, with
 * -I<reference>/main/src) and calls d2QuadpoleMomentum and computeHtt with the types sph::SphTypes gives them:
 * Tc = double, Tv = Ta = Tm = float.  Built without OpenMP, so the header's reduction loops run sequentially.
 */
#include <array>
#include <cstddef>

#include "observables/grav_waves_calculations.hpp"

extern "C"
{
    //! the six sums of gravRad (gravitational_waves.hpp:72-77): xx, yy, zz, xy, xz, yz
    void ref_d2q(size_t first, size_t last, const double* x, const double* y, const double* z, const float* vx,
                 const float* vy, const float* vz, const float* ax, const float* ay, const float* az, const float* m,
                 double out[6])
    {
        const int dims[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
        for (int k = 0; k < 6; ++k)
            out[k] = sphexa::d2QuadpoleMomentum(first, last, dims[k][0], dims[k][1], x, y, z, vx, vy, vz, ax, ay, az, m);
    }

    void ref_htt(const double q[6], double theta, double phi, double out[2])
    {
        std::array<double, 6> a{q[0], q[1], q[2], q[3], q[4], q[5]};
        sphexa::computeHtt(a, theta, phi, &out[0], &out[1]);
    }
}
