/*! Compile (and link) check of sph::computeStirringGpu of the C++ mirror (sph-exa_amd/host/sphexa_amd/sph_gpu.hpp)
 *  against the declaration a turb_ve.hpp build sees: sph/hydro_turb/stirring.hpp declares the template `extern`
 *  (stirring.hpp:123-126) and driveTurbulence calls it with a cstone::GroupView and raw device pointers
 *  (driver.hpp:116-119).  The mirror's definition must be that template, so the explicit instantiation below and the
 *  deduced call both resolve to it and the only undefined symbols are sx_* functions.  Built by
 *  tests/test_turb_mirror_compile.py with g++ -I<reference include dirs>; never run (no GPU is touched). */
#include <cstddef>

#include "sph/hydro_turb/stirring.hpp"

#include "sphexa_amd/sph_gpu.hpp"

void stirLikeDriveTurbulence(cstone::GroupView grp, const double* x, const double* y, const double* z, float* ax,
                             float* ay, float* az, size_t numModes, const double* modes, const double* phasesReal,
                             const double* phasesImag, const double* amplitudes, double solWeightNorm)
{
    size_t numDim = 3;
    sph::computeStirringGpu<double, float, double>(grp, numDim, x, y, z, ax, ay, az, numModes, modes, phasesReal,
                                                   phasesImag, amplitudes, solWeightNorm);
    // as driveTurbulence writes it: template arguments deduced
    sph::computeStirringGpu(grp, numDim, x, y, z, ax, ay, az, numModes, modes, phasesReal, phasesImag, amplitudes,
                            solWeightNorm);
}

int main(int argc, char**)
{
    if (argc > 1000) // never: the call needs a GPU; the check is that it compiles and links
    {
        cstone::GroupView grp{};
        stirLikeDriveTurbulence(grp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                nullptr, 1.0);
    }
    return 0;
}
