/*! @file direct_ref_harness.cpp
 * @brief a C entry point over the reference's CPU direct sum, for tests/test_direct_ref.py.
 *
 * Includes the reference's ryoanji/nbody/traversal_cpu.hpp (compiled from where it lies, with
 * -I<reference>/ryoanji/src -I<reference>/domain/include) and calls ryoanji::directSum (traversal_cpu.hpp:234-270).
 * That function instantiates only with Th == Tc (target_h is a Tc and P2P deduces one Th), so h is taken as double:
 * Tc = Th = double, Tm = float.  Built without OpenMP and without FMA contraction: the loops run sequentially and
 * every operation rounds on its own.
 */
#include <cstddef>

#include "ryoanji/nbody/traversal_cpu.hpp"

extern "C"
{
    //! ax, ay, az, ugrav: the reference accumulates into them; the caller zeroes them
    void ref_direct_sum(size_t n, const double* x, const double* y, const double* z, const double* h, const float* m,
                        float G, double lx, double ly, double lz, int numShells, double* ax, double* ay, double* az,
                        double* ugrav)
    {
        ryoanji::directSum(x, y, z, h, m, (cstone::LocalIndex)n, G, cstone::Vec3<double>{lx, ly, lz}, numShells, ax, ay,
                           az, ugrav);
    }
}
