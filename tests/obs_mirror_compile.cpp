/*! Compile (and link) check of the drop-in sph-exa_amd/host/observables/gpu_reductions.h against the reference's own
 *  cstone::Box: the three templates of main/src/observables/gpu_reductions.h:52-89 in namespace sphexa, instantiated
 *  with the type combinations sph::SphTypes yields and called as time_energy_growth.hpp:95-97,
 *  turbulence_mach_rms.hpp:74-75 and wind_bubble_fraction.hpp:83-84 call them (template arguments deduced).  Built by
 *  tests/test_obs_mirror_compile.py with g++ -I<reference include dirs>; never run (no GPU is touched). */
#include <cstddef>
#include <tuple>

#include "observables/gpu_reductions.h"

template std::tuple<double, double, double>
sphexa::gpuGrowthRate<double, float, float>(const double*, const double*, const float*, const float*, const float*,
                                            const cstone::Box<double>&, size_t, size_t);
template double sphexa::machSquareSumGpu<float, float>(const float*, const float*, const float*, const float*, size_t,
                                                       size_t);
template size_t sphexa::survivorsGpu<float, double, float>(const double*, const float*, const float*, const float*,
                                                           double, double, size_t, size_t);

double callLikeTheObservables(const double* x, const double* y, const double* temp, const float* vx, const float* vy,
                              const float* vz, const float* c, const float* xm, const float* kx, const float* m,
                              const cstone::Box<double>& box, size_t first, size_t last)
{
    double s[3];
    std::tie(s[0], s[1], s[2]) = sphexa::gpuGrowthRate(x, y, vy, xm, kx, box, first, last);
    double mach                = sphexa::machSquareSumGpu(vx, vy, vz, c, first, last);
    size_t cloud               = sphexa::survivorsGpu(temp, kx, xm, m, 1.0, 2.0, first, last);
    return s[0] + s[1] + s[2] + mach + double(cloud);
}

int main(int argc, char**)
{
    if (argc > 1000) // never: the calls need a GPU; the check is that they compile and link
    {
        cstone::Box<double> box(0, 1);
        return (int)callLikeTheObservables(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, nullptr, box, 0, 0);
    }
    return 0;
}
