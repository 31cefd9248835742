/*! @file gpu_reductions.h
 * @brief Drop-in for the reference's main/src/observables/gpu_reductions.h (:52-89): gpuGrowthRate, machSquareSumGpu
 *        and survivorsGpu in namespace sphexa, defined over sx_observables of libsphexa_hip.so.
 *
 * The reference declares the three templates `extern` and instantiates them in gpu_reductions.cu with thrust; put this
 * directory before main/src/observables on the include path and leave gpu_reductions.cu out of the build
 * (INTEGRATION.md).  The context is the process-wide one of sphexa_amd/sph_gpu.hpp.  The pointers are the only fields
 * handed over, so sx_observables forms no conserved sums on this path and reads nothing else.  Type combinations:
 * those sph::SphTypes yields (coordinates and temperature double, everything else float).
 */
#pragma once

#include <cstddef>
#include <tuple>
#include <type_traits>

#include "cstone/sfc/box.hpp"

#include "sphexa_amd/sph_gpu.hpp"

namespace sphexa
{

namespace amd_detail
{
inline void observe(const sx_fields& f, const sx_box* box, size_t first, size_t last, int kind,
                    const sx_obs_settings* set, double* out, const char* what)
{
    namespace sa = sphexa_amd;
    sa::check(sx_observables(sa::context(), &f, box, (uint32_t)first, (uint32_t)last, kind, set, 10.0f, 5.0 / 3.0, out,
                             SX_OBS_MAX_SUMS),
              what);
}
} // namespace amd_detail

//! gpu_reductions.h:52-55: the local sums si, ci, di of the Kelvin-Helmholtz growth rate
template<class Tc, class Tv, class T>
std::tuple<double, double, double> gpuGrowthRate(const Tc* x, const Tc* y, const Tv* vy, const T* xm, const T* kx,
                                                 const cstone::Box<Tc>& box, size_t startIndex, size_t endIndex)
{
    static_assert(std::is_same_v<Tc, double> && std::is_same_v<Tv, float> && std::is_same_v<T, float>,
                  "gpuGrowthRate: double coordinates, float velocities and volume elements (SphTypes)");
    sx_fields f{};
    f.n = endIndex;
    f.x = const_cast<Tc*>(x), f.y = const_cast<Tc*>(y), f.vy = const_cast<Tv*>(vy);
    f.xm = const_cast<T*>(xm), f.kx = const_cast<T*>(kx);
    const sx_box b = sphexa_amd::toBox(box);
    double       out[SX_OBS_MAX_SUMS];
    amd_detail::observe(f, &b, startIndex, endIndex, SX_OBS_KH_GROWTH, nullptr, out, "gpuGrowthRate");
    return {out[9], out[10], out[11]};
}

//! gpu_reductions.h:69-70: the local sum of |v|^2 / c^2
template<class Tv, class T>
double machSquareSumGpu(const Tv* vx, const Tv* vy, const Tv* vz, const T* c, size_t first, size_t last)
{
    static_assert(std::is_same_v<Tv, float> && std::is_same_v<T, float>,
                  "machSquareSumGpu: float velocities and speed of sound (SphTypes)");
    sx_fields f{};
    f.n  = last;
    f.vx = const_cast<Tv*>(vx), f.vy = const_cast<Tv*>(vy), f.vz = const_cast<Tv*>(vz), f.c = const_cast<T*>(c);
    double out[SX_OBS_MAX_SUMS];
    amd_detail::observe(f, nullptr, first, last, SX_OBS_MACH_RMS, nullptr, out, "machSquareSumGpu");
    return out[9];
}

//! gpu_reductions.h:87-89: the local number of particles that still belong to the cloud
template<class T, class Tt, class Tm>
size_t survivorsGpu(const Tt* temp, const T* kx, const T* xmass, const Tm* m, double rhoBubble, double tempWind,
                    size_t first, size_t last)
{
    static_assert(std::is_same_v<T, float> && std::is_same_v<Tt, double> && std::is_same_v<Tm, float>,
                  "survivorsGpu: double temperature, float volume elements and masses (SphTypes)");
    sx_fields f{};
    f.n    = last;
    f.temp = const_cast<Tt*>(temp), f.kx = const_cast<T*>(kx), f.xm = const_cast<T*>(xmass), f.m = const_cast<Tm*>(m);
    sx_obs_settings set{};
    set.rhoBubble = rhoBubble, set.tempWind = tempWind;
    double out[SX_OBS_MAX_SUMS];
    amd_detail::observe(f, nullptr, first, last, SX_OBS_WIND_BUBBLE, &set, out, "survivorsGpu");
    return (size_t)out[9];
}

} // namespace sphexa
