/*! @file sx_turb.hpp
 * @brief turbulence stirring: the host state behind sx_turb_* (sx_turb.cpp), the launchers of the stirring and
 *        noise-advance kernels (sx_turb.hip) and the per-sim device state of a stirred sx_sim.
 *
 * Replaces sph/include/sph/hydro_turb/ (turbulence_data.hpp, create_modes.hpp, driver.hpp, phases.hpp, stirring.hpp,
 * stirring_gpu.cu).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <random>
#include <string>
#include <vector>

#include "../../include/sphexa_hip.h"

//! sph::TurbulenceData<double, ...> (turbulence_data.hpp:46-184) without the device vectors
struct sx_turb
{
    sx_turb_settings    set{};
    double              variance{0}, decayTime{0}, solWeight{0}, solWeightNorm{0};
    uint64_t            numModes{0};
    std::vector<double> modes, amplitudes, phases;
    std::mt19937        gen;
};

namespace sx::turb
{

/*! largest lattice index of the fast stirring kernel.  It unrolls the (kMaxHarmonic + 1)^3 lattice points i, j, k >= 0
 *  at compile time, so the harmonics e^{i n theta}, n <= kMaxHarmonic, of the three axes stay in registers
 *  (6 kMaxHarmonic VGPRs) and the presence of each point is one bit of a 64-bit mask.  3 covers every table
 *  createStirringModes can produce with epsilon < 1 (its band is [1 - eps, 3 + eps] 2 pi / L); 4 would take 125
 *  points, twice the code (beyond the 64 KB instruction cache) and a second mask word. */
constexpr int kMaxHarmonic = 3;
constexpr int kAxis        = kMaxHarmonic + 1;
constexpr int kPoints      = kAxis * kAxis * kAxis; //!< lattice points (i, j, k), i, j, k in [0, kMaxHarmonic]
constexpr int kSlots       = 4 * kPoints;           //!< per point the sign variants (+j +k), (-j +k), (+j -k), (-j -k)
constexpr int kSlotCoefs   = 6;                     //!< per slot {Re, Im} of x, y, z, times amplitude solWeightNorm
static_assert(kPoints <= 64, "the presence mask is one 64-bit word");

/*! a mode table on an integer lattice k = w0 (a, b, c), |a|, |b|, |c| <= kMaxHarmonic.  A mode with a < 0 is taken
 *  as the conjugate of (-a, -b, -c): cos is even, sin odd, so its {Re, Im} enter the slot of (-a, -b, -c) as {Re, -Im}.
 *  slot[m] = slot index | 256 for a conjugated mode. */
struct Lattice
{
    bool                 ok{false};
    double               w0{0};
    uint64_t             present{0};
    std::vector<int32_t> slot;
};
Lattice latticeOf(uint64_t numModes, const double* modes);

//! computePhases (phases.hpp:47-72)
void computePhases(uint64_t numModes, const double* phases, double solWeight, const double* modes, double* phasesReal,
                   double* phasesImag);
//! the fast kernel's coefficients, kSlots x kSlotCoefs: per slot the sum over its modes, in mode order and in double,
//! rounded to float
void denseTable(const Lattice& lat, uint64_t numModes, const double* amplitudes, double solWeightNorm,
                const double* phasesReal, const double* phasesImag, float* table);
//! n draws of std::normal_distribution<double>(0, 1) from a fresh distribution object (updateNoise, driver.hpp:85-89)
void drawNormals(std::mt19937& gen, double* out, size_t n);

//! a GroupView (traversal/groups.hpp:19-55): explicit [start[g], end[g]) or, with start == nullptr, the 64-particle
//! blocks of [first, last)
struct StirArgs
{
    uint32_t        first, last, numGroups;
    const uint32_t* start;
    const uint32_t* end;
    const double *  x, *y, *z;
    float *         ax, *ay, *az;
    // exact: the reference's arrays
    uint64_t        numModes;
    const double *  modes, *phasesReal, *phasesImag, *amplitudes;
    double          solWeightNorm;
    // fast: the dense coefficient table
    const float*    table;
    uint64_t        present;
    double          w0;
};
hipError_t stirExact(const StirArgs& a, hipStream_t s);
hipError_t stirFast(const StirArgs& a, hipStream_t s);

//! one OU step on the device (updateNoise + computePhases + the dense table), dt read from the device scalars
struct NoiseArgs
{
    const double*  dt;
    double         variance, decayTime, solWeight, solWeightNorm;
    uint64_t       numModes;
    const double*  normals; // 6 numModes draws of N(0, 1)
    double*        phases;  // 6 numModes, updated in place
    const double * modes, *amplitudes;
    double *       phasesReal, *phasesImag; // 3 numModes each
    const int32_t* slot;                    // Lattice::slot, nullptr when the table is not on the lattice
    float*         table;
};
hipError_t advanceNoise(const NoiseArgs& a, hipStream_t s);

//! the turbulence state of a stirred sx_sim
struct SimTurb
{
    sx_turb* host{nullptr};
    Lattice  lat;
    double * phases{nullptr}, *modes{nullptr}, *amplitudes{nullptr}, *phasesReal{nullptr}, *phasesImag{nullptr};
    double*  normals{nullptr};
    float*   table{nullptr};
    int32_t* slot{nullptr};
    /*! the step's normals travel host -> device through a ring of pinned buffers: a slot is rewritten only after the
     *  copy queued from it has completed (its event) */
    static constexpr int kRing = 4;
    double*              ring[kRing]{};
    hipEvent_t           ringEv[kRing]{};
    bool                 ringBusy[kRing]{};
    int                  next{0};
    hipEvent_t           ev[3]{};
    float                ms[2]{0.f, 0.f};
};

} // namespace sx::turb
