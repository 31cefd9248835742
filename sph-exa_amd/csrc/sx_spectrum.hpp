/*! @file sx_spectrum.hpp
 * @brief Power spectra of the particles (sx_spectrum.hip, sx_fft.hip): the state reduced to a few hundred numbers.
 *
 * Box and mesh.  The box must be periodic on all three axes and cubic, with edge L.  The mesh has n^3 cells,
 * n in {16, 32, 64, 128, 256}; cell size D = L / n; cell (ix, iy, iz) has its centre at lim_lo + (i + 1/2) D per axis;
 * cells are stored [iz][iy][ix], x fastest.
 *
 * Deposit.  S0(c) = sum_j m_j K W(r_jc / he_j) / he_j^3 with W = sinc^6 (kernelWt), r the minimum-image distance to the
 * cell centre and he_j = max(h_j, D / 2): with this clamp every particle reaches at least one centre.  Up to three
 * further sums S1_a(c) = sum_j w_jc a_j use the same weights, for three device columns a (float or double).  Neither rho
 * nor a volume element is read.  Each cell sums in float, FMA, in ascending particle index, and stores a double; a cell
 * is exactly 0 where no support contains its centre; there are no float atomics: the result is bit-identical from run to
 * run and for every pair cap.  One workgroup per block of 8 x 8 x 4 cells gathers the block's list; the pairs
 * block << 32 | particle, their bands of whole block layers along z under a pair cap and their sort are the pair-binning
 * engine's (sx_pairbin.hpp), as for the maps.
 *
 * Field.  SX_SPEC_VELOCITY: W_a = S0^p S1_a / S0 for a = vx, vy, vz; weight 0: p = 0, 1: p = 1/2, 2: p = 1/3; prefactor
 * 1/2.  SX_SPEC_SCALAR: one column (W = S1 / S0), or the mesh density S0 itself; weight 0; prefactor 1.  W = 0 where
 * S0 = 0.  W is computed in double from the stored sums.
 *
 * Transform and shells.  What(n) = n^-3 sum_c W(c) exp(-2 pi i n.c / n), complex to complex in double; integer wave
 * vectors n_i in [-n/2, n/2); shell s = floor(|n| + 1/2); numShells = floor(sqrt(3) n / 2 + 1/2) + 1;
 * power[s] = prefactor sum_a sum_{n in s} |What_a(n)|^2; modes[s] = the wave vectors in shell s.  It follows that
 * sum_s power[s] = prefactor <sum_a W_a^2> over the cells (Parseval).  The wave number of shell s is 2 pi s / L.
 * The shell sums are a fixed tree over a mode permutation grouped by shell: the same bits every run.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/sphexa_hip.h"
#include "sx_pairbin.hpp"
#include "sx_tree.hpp"

namespace sx::spectrum
{

constexpr int      kBx = 8, kBy = 8, kBz = 4;   //!< cells per block: 256, one per lane; wave w owns the layer z = w
constexpr uint32_t kChunk      = 256;         //!< records staged through LDS at a time (one per lane, 12 KB)
constexpr uint32_t kMaxN       = 256;
constexpr int      kMaxLayers  = kMaxN / kBz; //!< block layers along z: the unit of a band
constexpr uint32_t kShellChunk = 2048;        //!< modes per leaf of the shell sums' fixed tree

//! the reason sx_spectrum_check refuses, or nullptr
const char* checkSpec(const sx_spectrum* sp, const sx_box* box);
bool        validN(uint32_t n);
uint32_t    numShells(uint32_t n);
//! shell of the integer wave vector with squared length k2: the s with s (s - 1) < k2 <= s (s + 1)
uint32_t shellOf(uint32_t k2);
//! modes per shell, numShells(n) entries
void shellModes(uint32_t n, uint64_t* modes);

//! one deposit (device pointers)
struct DepositArgs
{
    sx_box        box;
    const double *x, *y, *z;
    const float * h, *m;
    const void*   a[3];
    int           numA, aIsDouble;
    uint32_t      first, last;
    double        K;
    uint32_t      n;
    double *      sum0, *sum1; // n^3 and numA n^3 doubles
};

/*! the typed owner of the scratch, the cached tables and the last call's figures.  Every "spec.*" arena tag is requested
 *  at one site, the deposit's pair scratch by the engine (bin), the others in sx_spectrum.hip, which stores the pointer here. */
struct SpecBuffers
{
    pairbin::Buffers bin; // counts[0]: particles clamped to D / 2; rows: block layers.  Its events time fft and shells too
    // per-n tables, built by the first call that needs them
    double2* twiddle{nullptr}; // exp(-2 pi i k / n), k < n
    uint32_t twiddleN{0};
    uint32_t* perm{nullptr};   // the cells of the transformed mesh grouped by shell, ascending cell index within one
    uint32_t* leafBeg{nullptr}; // numLeaves + 1: leaves of at most kShellChunk modes, none across a shell boundary
    uint32_t* shellLeaf{nullptr}; // numShells + 1: first leaf of each shell
    uint32_t* shellBeg{nullptr};  // numShells + 1: first mode of each shell in perm
    double*   leafSum{nullptr};
    uint32_t  permN{0}, numLeaves{0};
    // sx_spectrum_compute / sx_sim_spectrum: [2 leading doubles | S0 | S1 x 3], one complex mesh, power and modes
    double *sums{nullptr}, *cplx{nullptr}, *out{nullptr}, *outHost{nullptr};
    float msFft{0.0f}, msShells{0.0f}; // since the last deposit (bin.timing)
};

int deposit(Arena& arena, SpecBuffers& b, const DepositArgs& a, hipStream_t s, std::string& err);
//! in place, forward, scaled by n^-3 (sx_fft.hip)
int fft3d(Arena& arena, SpecBuffers& b, double* complexMesh, uint32_t n, hipStream_t s, std::string& err);
int shellSums(Arena& arena, SpecBuffers& b, const double* complexMesh, uint32_t n, double prefactor, int accumulate,
              double* power, uint64_t* modes, hipStream_t s, std::string& err);

/*! all stages: deposit over [first, last) (a.sum0, a.sum1 and a.n are set here), `reduce` (if set) over the leading
 *  doubles and the meshes -- called also where this rank's deposit was refused, with zeroed meshes and a refusal count of
 *  1 in front, so nobody waits in a collective for a rank that left early --, then field, transform and shell sums into
 *  the device arrays power and modes (either nullable: then b.out holds [power | modes]).  Synchronises. */
int compute(Arena& arena, SpecBuffers& b, const sx_spectrum& sp, DepositArgs a, double* power, uint64_t* modes,
            const std::function<bool(double*, size_t)>& reduce, hipStream_t s, std::string& err);

//! the engine's words for the deposit; stats: {pairs, bands, longest block list, particles clamped to D / 2}
//! (after a count / emit disagreement the mesh lacks contributions: SX_ERR_HIP with the last text)
constexpr pairbin::Names kNames{"sx_mesh_deposit",
                                "sx_spectrum",
                                "block layer",
                                "(deposit fewer particles at a time)",
                                "sx_set_spectrum_pair_cap",
                                "spec.",
                                "nothing has been deposited",
                                "the last deposit's emit pass disagreed with its count pass: the mesh is incomplete"};

//! the twiddle table of n on the host: exp(-2 pi i k / n) from the first octant, each entry within 1 ulp
void twiddleTable(uint32_t n, std::vector<double2>& t);
//! the line transforms (sx_fft.hip): x, then y, then z; tw: device table of n entries
hipError_t fftLaunch(double2* mesh, uint32_t n, const double2* tw, hipStream_t s);

} // namespace sx::spectrum
