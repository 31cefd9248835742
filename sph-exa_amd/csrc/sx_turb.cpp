/*! @file sx_turb.cpp
 * @brief host state of the turbulence stirring (sx_turb_*): what sph::TurbulenceData holds, with the mode table of
 *        createStirringModes, the OU step of updateNoise and the projection of computePhases restated in double and in
 *        the reference's order of operations (compiled -ffp-contract=off), so that seeds give its numbers.
 *
 * Replaces sph/include/sph/hydro_turb/turbulence_data.hpp:46-184, create_modes.hpp:59-244, driver.hpp:80-92 and
 * phases.hpp:47-72.  Plain C++: nothing here touches the GPU.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <sstream>

#include "sx_turb.hpp"

namespace
{

constexpr size_t kDim = 3; // TurbulenceData::numDim

/*! The mode table of createStirringModes (create_modes.hpp:59-244) for three dimensions and a cubic box of side
 *  boxLen, restated: the arithmetic of every stored value is the reference's, operation by operation.
 *  Forms 0 (band) and 1 (parabola): every lattice point 2 pi (i, j, l) / boxLen, i, j, l >= 0, inside the band
 *  [kLow, kHigh], in i-major order, each as the four sign variants (+j +l), (-j +l), (+j -l), (-j -l).
 *  Form 2 (power law): per shell of integer radius a number of random directions, rounded to the lattice.
 *  The cap: a point is refused once the stored modes + 4 exceed maxModes (also in form 2, which stores one). */
void buildModeTable(sx_turb& d, double boxLen, size_t maxModes, double kHigh, double kLow, size_t form, double slope,
                    double anglesExp)
{
    const double twoPi = 2.0 * M_PI;
    // the wavenumber the amplitudes are scaled to: the lower band edge, for the parabola the band centre
    const double kRef = form == 1 ? 0.5 * (kLow + kHigh) : kLow;

    d.modes.clear();
    d.amplitudes.clear();
    uint64_t stored    = 0;
    auto     tableFull = [&] { return double(stored) + 4.0 > double(maxModes); };
    auto     add       = [&](double amp, double kx, double ky, double kz)
    {
        d.amplitudes.push_back(amp);
        d.modes.insert(d.modes.end(), {kx, ky, kz});
        stored++;
    };
    auto inBand = [&](double k) { return k >= kLow && k <= kHigh; };

    if (form != 2)
    {
        const double curvature = -4.0 / ((kHigh - kLow) * (kHigh - kLow));
        // the reference scans indices 0 .. 256 on every axis; an index whose own wavenumber exceeds kHigh cannot pass
        const size_t top = std::min<double>(256.0, std::floor(kHigh * boxLen / twoPi) + 1.0);
        for (size_t i = 0; i <= top; i++)
            for (size_t j = 0; j <= top; j++)
                for (size_t l = 0; l <= top; l++)
                {
                    const double kx = twoPi * i / boxLen, ky = twoPi * j / boxLen, kz = twoPi * l / boxLen;
                    const double kAbs = std::sqrt(kx * kx + ky * ky + kz * kz);
                    if (!inBand(kAbs)) continue;
                    // the reference leaves its innermost loop here and refuses every later point likewise
                    if (tableFull()) break;
                    const double shape = form == 1 ? std::abs(curvature * (kAbs - kRef) * (kAbs - kRef) + 1.0) : 1.0;
                    const double amp   = 2.0 * std::sqrt(shape) * std::pow(kRef / kAbs, 0.5 * (kDim - 1));
                    for (int v = 0; v < 4; ++v)
                        add(amp, kx, (v & 1) ? -ky : ky, (v & 2) ? -kz : kz);
                }
    }
    else
    {
        std::uniform_real_distribution<double> unit(0, 1);
        const int shellLo = std::max(1, int(kLow * boxLen / twoPi + 0.5));
        const int shellHi = int(kHigh * boxLen / twoPi + 0.5);
        for (int shell = shellLo; shell <= shellHi; shell++)
        {
            const size_t directions = 8.0 * std::ceil(std::pow(double(shell), anglesExp));
            for (size_t n = 1; n <= directions; n++)
            {
                // three draws per direction, in this order: azimuth, polar angle (uniform on the sphere), radius
                const double azimuth = twoPi * unit(d.gen);
                const double polar   = std::acos(1.0 - 2.0 * unit(d.gen));
                const double radius  = shell + unit(d.gen) - 0.5;
                const double kx      = twoPi * std::round(radius * std::sin(polar) * std::cos(azimuth)) / boxLen;
                const double ky      = twoPi * std::round(radius * std::sin(polar) * std::sin(azimuth)) / boxLen;
                const double kz      = twoPi * std::round(radius * std::cos(polar)) / boxLen;
                const double kAbs    = std::sqrt(kx * kx + ky * ky + kz * kz);
                if (!inBand(kAbs)) continue;
                // ends this shell's draws; the next shell draws again
                if (tableFull()) break;
                const double law = std::pow(kAbs / kRef, slope);
                // corrected for the directions sampled relative to the full shell (shell^2 points)
                const double amp =
                    std::sqrt(law * (std::pow(double(shell), double(kDim - 1)) * 4.0 * std::sqrt(3.0) / directions)) *
                    std::pow(kRef / kAbs, (kDim - 1) / 2.0);
                add(amp, kx, ky, kz);
            }
        }
    }
    d.numModes = stored;
}

//! the constants TurbulenceData::initModes derives (turbulence_data.hpp:150-183), the table and the first phases
void initState(sx_turb& d)
{
    const sx_turb_settings& c = d.set;
    const double twoPi = 2.0 * M_PI, L = c.Lbox, v = c.stMachVelocity, w = c.solWeight;

    const double power = c.stEnergyPrefac * std::pow(v, 3) / L;
    const double kLow  = (1.0 - c.epsilon) * twoPi / L;
    const double kHigh = (3.0 + c.epsilon) * twoPi / L;

    d.solWeight = w;
    d.decayTime = L / (2.0 * v);
    d.variance  = std::sqrt(power / d.decayTime);
    // keeps the rms force independent of the solenoidal weight
    d.solWeightNorm =
        std::sqrt(3.0) * std::sqrt(3.0 / double(kDim)) / std::sqrt(1.0 - 2.0 * w + double(kDim) * w * w);

    buildModeTable(d, L, size_t(c.stMaxModes), kHigh, kLow, size_t(c.stSpectForm), c.powerLawExp, c.anglesExp);

    // Gaussian phases of standard deviation `variance`, from ONE distribution object (its saved second value is used)
    std::normal_distribution<double> gauss(0, d.variance);
    d.phases.resize(2 * kDim * d.numModes);
    for (double& p : d.phases)
        p = gauss(d.gen);
}

//! the largest spacing w0 = (smallest nonzero |component|) / n, n <= maxDivisor, of which every mode component is an
//! integer multiple (within 1e-9); 0 when there is none.  maxIndex receives the largest multiple.
double latticeSpacing(uint64_t numModes, const double* modes, int maxDivisor, int& maxIndex)
{
    double wmin = 0.0;
    for (uint64_t c = 0; c < 3 * numModes; ++c)
    {
        const double a = std::fabs(modes[c]);
        if (a > 0.0 && (wmin == 0.0 || a < wmin)) wmin = a;
    }
    if (!(wmin > 0.0) || !std::isfinite(wmin)) return 0.0;
    for (int n = 1; n <= maxDivisor; ++n)
    {
        const double w0   = wmin / n;
        bool         good = true;
        maxIndex          = 0;
        for (uint64_t c = 0; c < 3 * numModes && good; ++c)
        {
            const double r = modes[c] / w0, q = std::nearbyint(r);
            good           = std::fabs(r - q) <= 1e-9 && std::fabs(q) < 1e6;
            if (good) maxIndex = std::max(maxIndex, std::abs(int(q)));
        }
        if (good) return w0;
    }
    return 0.0;
}

} // namespace

namespace sx::turb
{

/*! The projection of computePhases (phases.hpp:47-72), restated: per mode the six OU phases are three complex
 *  numbers z_j = (re_j, im_j); their component along k is k (k . z) / k^2, the rest is solenoidal; the result mixes
 *  the two with the solenoidal weight.  Sums run over j = 0, 1, 2 in order, as the reference's. */
void computePhases(uint64_t numModes, const double* ou, double solWeight, const double* modes, double* phasesReal,
                   double* phasesImag)
{
    for (size_t m = 0; m < numModes; m++)
    {
        const double* k = modes + 3 * m;
        const double* z = ou + 6 * m;
        double k2 = 0.0, dotIm = 0.0, dotRe = 0.0;
        for (size_t j = 0; j < kDim; j++)
        {
            k2    = k2 + k[j] * k[j];
            dotIm = dotIm + k[j] * z[2 * j + 1];
            dotRe = dotRe + k[j] * z[2 * j];
        }
        for (size_t j = 0; j < kDim; j++)
        {
            const double alongIm = k[j] * dotIm / k2, alongRe = k[j] * dotRe / k2;
            const double restRe = z[2 * j] - alongRe, restIm = z[2 * j + 1] - alongIm;
            phasesReal[3 * m + j] = solWeight * restRe + (1.0 - solWeight) * alongRe;
            phasesImag[3 * m + j] = solWeight * restIm + (1.0 - solWeight) * alongIm;
        }
    }
}

void drawNormals(std::mt19937& gen, double* out, size_t n)
{
    std::normal_distribution<double> dist(0, 1);
    for (size_t i = 0; i < n; ++i)
        out[i] = dist(gen);
}

Lattice latticeOf(uint64_t numModes, const double* modes)
{
    Lattice      lat;
    int          maxIndex = 0;
    // the smallest nonzero component is n w0 with n <= kMaxHarmonic; a finer spacing only makes the indices larger
    const double w0 = latticeSpacing(numModes, modes, kMaxHarmonic, maxIndex);
    if (w0 == 0.0 || maxIndex > kMaxHarmonic) return lat;
    lat.ok = true, lat.w0 = w0;
    lat.slot.assign(numModes, 0);
    for (uint64_t m = 0; m < numModes; ++m)
    {
        int idx[3];
        for (int e = 0; e < 3; ++e)
            idx[e] = int(std::nearbyint(modes[3 * m + e] / w0));
        const bool conj = idx[0] < 0;
        if (conj) idx[0] = -idx[0], idx[1] = -idx[1], idx[2] = -idx[2];
        const int point   = (idx[0] * kAxis + std::abs(idx[1])) * kAxis + std::abs(idx[2]);
        const int variant = (idx[1] < 0 ? 1 : 0) + (idx[2] < 0 ? 2 : 0);
        lat.slot[m]       = (point * 4 + variant) | (conj ? 256 : 0);
        lat.present |= uint64_t(1) << point;
    }
    return lat;
}

void denseTable(const Lattice& lat, uint64_t numModes, const double* amplitudes, double solWeightNorm,
                const double* phasesReal, const double* phasesImag, float* out)
{
    double table[kSlots * kSlotCoefs];
    std::fill(table, table + kSlots * kSlotCoefs, 0.0);
    for (uint64_t m = 0; m < numModes; ++m)
    {
        const int    t = lat.slot[m] & 255;
        const double w = amplitudes[m] * solWeightNorm, sgn = (lat.slot[m] & 256) ? -1.0 : 1.0;
        for (int e = 0; e < 3; ++e)
        {
            table[t * kSlotCoefs + 2 * e] += w * phasesReal[3 * m + e];
            table[t * kSlotCoefs + 2 * e + 1] += sgn * (w * phasesImag[3 * m + e]);
        }
    }
    for (int q = 0; q < kSlots * kSlotCoefs; ++q)
        out[q] = (float)table[q];
}

} // namespace sx::turb

extern "C"
{

    int sx_turb_default_settings(sx_turb_settings* s)
    {
        if (!s) return SX_ERR_ARG;
        *s = sx_turb_settings{0.5, 100000, 1.0, 5.0e-3, 0.3e0, 1e-15, 251299, 1, 5. / 3, 2.0};
        return SX_OK;
    }

    int sx_turb_create(sx_turb** out, const sx_turb_settings* s)
    {
        if (!out || !s || s->stSpectForm > 2 || s->stMaxModes == 0 || !(s->Lbox > 0.0) || !(s->stMachVelocity > 0.0))
            return SX_ERR_ARG;
        auto* d = new sx_turb;
        d->set  = *s;
        d->gen.seed(size_t(s->rngSeed));
        initState(*d);
        *out = d;
        return SX_OK;
    }

    void sx_turb_destroy(sx_turb* t) { delete t; }

    uint64_t sx_turb_num_modes(const sx_turb* t) { return t ? t->numModes : 0; }

    int sx_turb_get_scalars(const sx_turb* t, double out[4])
    {
        if (!t || !out) return SX_ERR_ARG;
        out[0] = t->variance, out[1] = t->decayTime, out[2] = t->solWeight, out[3] = t->solWeightNorm;
        return SX_OK;
    }

    int sx_turb_get_arrays(const sx_turb* t, double* modes, double* amplitudes, double* phases)
    {
        if (!t) return SX_ERR_ARG;
        if (modes) std::copy(t->modes.begin(), t->modes.end(), modes);
        if (amplitudes) std::copy(t->amplitudes.begin(), t->amplitudes.end(), amplitudes);
        if (phases) std::copy(t->phases.begin(), t->phases.end(), phases);
        return SX_OK;
    }

    int64_t sx_turb_get_rng(const sx_turb* t, char* buf, size_t cap)
    {
        if (!t) return -1;
        std::stringstream s;
        s << t->gen;
        const std::string txt = s.str();
        if (buf && cap)
        {
            const size_t k = std::min(cap - 1, txt.size());
            std::memcpy(buf, txt.data(), k);
            buf[k] = 0;
        }
        return int64_t(txt.size());
    }

    int sx_turb_set_state(sx_turb* t, const double scalars[4], uint64_t numModes, const double* modes,
                          const double* amplitudes, const double* phases, const char* rng)
    {
        if (!t || !scalars || (numModes && (!modes || !amplitudes || !phases))) return SX_ERR_ARG;
        if (rng)
        {
            std::mt19937      g;
            std::stringstream s;
            s << rng;
            s >> g;
            if (s.fail()) return SX_ERR_ARG;
            t->gen = g;
        }
        t->variance = scalars[0], t->decayTime = scalars[1], t->solWeight = scalars[2], t->solWeightNorm = scalars[3];
        t->numModes = numModes;
        t->modes.assign(modes, modes + 3 * numModes);
        t->amplitudes.assign(amplitudes, amplitudes + numModes);
        t->phases.assign(phases, phases + 6 * numModes);
        return SX_OK;
    }

    int sx_turb_max_index(const sx_turb* t)
    {
        if (!t) return -1;
        if (t->numModes == 0) return 0;
        int maxIndex = 0;
        return latticeSpacing(t->numModes, t->modes.data(), 16, maxIndex) > 0.0 ? maxIndex : -1;
    }

    int sx_turb_fast_limit(void) { return sx::turb::kMaxHarmonic; }

    int sx_turb_update_noise(sx_turb* t, double dt)
    {
        if (!t) return SX_ERR_ARG;
        // the OU step of updateNoise (driver.hpp:80-92): x <- x f + sigma sqrt(1 - f^2) z, f = exp(-dt / decayTime), z
        // drawn from a distribution object of this call
        const double keep = std::exp(-dt / t->decayTime);
        const double kick = std::sqrt(1.0 - keep * keep);
        std::normal_distribution<double> gauss(0, 1);
        for (double& x : t->phases)
        {
            const double z = gauss(t->gen);
            x              = x * keep + t->variance * kick * z;
        }
        return SX_OK;
    }

    int sx_turb_compute_phases(const sx_turb* t, double* phasesReal, double* phasesImag)
    {
        if (!t || !phasesReal || !phasesImag) return SX_ERR_ARG;
        sx::turb::computePhases(t->numModes, t->phases.data(), t->solWeight, t->modes.data(), phasesReal, phasesImag);
        return SX_OK;
    }

} // extern "C"
