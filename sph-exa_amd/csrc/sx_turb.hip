/*! @file sx_turb.hip
 * @brief turbulence stirring on gfx950: the stirring kernel in its two variants and the device-side noise advance.
 *
 * Replaces sph/include/sph/hydro_turb/stirring_gpu.cu (computeStirringGpu; stirParticle, stirring.hpp:44-79) and the
 * per-step host work of driveTurbulence (driver.hpp:102-114: updateNoise, computePhases, the phase upload).
 *
 * Compiled twice (Makefile):
 *   -DSX_TURB_EXACT -ffp-contract=off   stirExact: the reference's sum, operation by operation, and advanceNoise (the OU
 *                                       recursion and the projection round like the host's)
 *   -DSX_TURB_FAST  -ffp-contract=fast  stirFast: every mode lies on the lattice k = w0 (a, b, c), so a particle needs
 *                                       sincos of w0 x, w0 y, w0 z once (the angle reduced in double, the rest in
 *                                       float: DESIGN.md 7d), the harmonics up to kMaxHarmonic by recurrence
 *                                       and per lattice point (i, j, k >= 0) two complex products for e^{i(ix +- jy)}
 *                                       and four for the sign variants (+-j, +-k), which share them.  The lattice is
 *                                       unrolled at compile time (harmonics in registers, no indexed access), a point
 *                                       without modes is skipped by a wave-uniform branch on one bit, and the
 *                                       coefficients (amplitude solWeightNorm {Re, Im}, summed per slot) are read at
 *                                       compile-time offsets from a wave-uniform pointer: scalar loads, no gathers.
 *
 * One wavefront per group of the view (explicit groups, or the 64-particle blocks of [first, last)), lanes striding
 * the group's particles.
 */
#include "sx_device.hpp"
#include "sx_turb.hpp"

namespace sx::turb
{

__device__ __forceinline__ bool groupBounds(const StirArgs& g, uint32_t w, uint32_t& s, uint32_t& e)
{
    if (w >= g.numGroups) return false;
    if (g.start)
    {
        s = g.start[w];
        e = g.end[w];
    }
    else
    {
        s = g.first + w * 64u;
        e = min(s + 64u, g.last);
    }
    return true;
}

static unsigned waveGrid(uint32_t numGroups) { return (numGroups + 3) / 4; }

#ifdef SX_TURB_EXACT

/*! The reference's stirring sum (stirParticle<double, float, double> and the update of computeStirring,
 *  stirring.hpp:44-79, :116-118), restated with its arithmetic kept operation by operation: per mode cos and sin of
 *  each k component times the coordinate in double, e^{i k.x} from their products, the three components accumulated in
 *  float, and solWeightNorm times the float sum added to the float acceleration in double. */
__global__ __launch_bounds__(256) void stirExactKernel(StirArgs a)
{
    const uint32_t w    = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t       s, e;
    if (!groupBounds(a, w, s, e)) return;
    float* const out[3] = {a.ax, a.ay, a.az};
    for (uint32_t i = s + lane; i < e; i += 64)
    {
        const double px = a.x[i], py = a.y[i], pz = a.z[i];
        float        sum[3] = {0.0f, 0.0f, 0.0f};
        for (uint64_t m = 0; m < a.numModes; ++m)
        {
            const double* k = a.modes + 3 * m;
            const double  cz = cos(k[2] * pz), sz = sin(k[2] * pz);
            const double  cy = cos(k[1] * py), sy = sin(k[1] * py);
            const double  cx = cos(k[0] * px), sx = sin(k[0] * px);
            // e^{i k.x} = (cx + i sx)(cy + i sy)(cz + i sz)
            const double eRe = (cx * cy - sx * sy) * cz - (sx * cy + cx * sy) * sz;
            const double eIm = cx * (cy * sz + sy * cz) + sx * (cy * cz - sy * sz);
            const double amp = a.amplitudes[m];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                sum[c] = (float)((double)sum[c] +
                                 amp * (a.phasesReal[3 * m + c] * eRe - a.phasesImag[3 * m + c] * eIm));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[c][i] = (float)((double)out[c][i] + a.solWeightNorm * (double)sum[c]);
    }
}

hipError_t stirExact(const StirArgs& a, hipStream_t s)
{
    if (a.numGroups) stirExactKernel<<<waveGrid(a.numGroups), 256, 0, s>>>(a);
    return hipGetLastError();
}

/*! updateNoise (driver.hpp:80-92) with the host's normals, computePhases (phases.hpp:47-72) and, for a table on the
 *  lattice, the fast kernel's coefficients (denseTable: per slot the sum over its modes in mode order).  One
 *  workgroup: the tables are a few hundred entries. */
__global__ __launch_bounds__(256) void advanceNoiseKernel(NoiseArgs a)
{
    const double dt       = *a.dt;
    const double dampingA = exp(-dt / a.decayTime);
    const double dampingB = sqrt(1.0 - dampingA * dampingA);
    for (uint64_t m = threadIdx.x; m < a.numModes; m += blockDim.x)
    {
        double ph[6];
        for (int q = 0; q < 6; ++q)
        {
            ph[q]               = a.phases[6 * m + q] * dampingA + a.variance * dampingB * a.normals[6 * m + q];
            a.phases[6 * m + q] = ph[q];
        }
        double ka = 0.0, kb = 0.0, kk = 0.0;
        for (int j = 0; j < 3; ++j)
        {
            const double k = a.modes[3 * m + j];
            kk             = kk + k * k;
            ka             = ka + k * ph[2 * j + 1];
            kb             = kb + k * ph[2 * j];
        }
        for (int j = 0; j < 3; ++j)
        {
            const double k     = a.modes[3 * m + j];
            const double diva  = k * ka / kk;
            const double divb  = k * kb / kk;
            const double curla = ph[2 * j] - divb;
            const double curlb = ph[2 * j + 1] - diva;
            a.phasesReal[3 * m + j] = a.solWeight * curla + (1.0 - a.solWeight) * divb;
            a.phasesImag[3 * m + j] = a.solWeight * curlb + (1.0 - a.solWeight) * diva;
        }
    }
    if (!a.slot) return;
    __threadfence_block();
    __syncthreads();
    for (int t = threadIdx.x; t < kSlots; t += blockDim.x)
    {
        double c[kSlotCoefs] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint64_t m = 0; m < a.numModes; ++m)
        {
            const int sl = a.slot[m];
            if ((sl & 255) != t) continue;
            const double w = a.amplitudes[m] * a.solWeightNorm, sgn = (sl & 256) ? -1.0 : 1.0;
            for (int e = 0; e < 3; ++e)
            {
                c[2 * e] += w * a.phasesReal[3 * m + e];
                c[2 * e + 1] += sgn * (w * a.phasesImag[3 * m + e]);
            }
        }
        for (int q = 0; q < kSlotCoefs; ++q)
            a.table[t * kSlotCoefs + q] = (float)c[q];
    }
}

hipError_t advanceNoise(const NoiseArgs& a, hipStream_t s)
{
    advanceNoiseKernel<<<1, 256, 0, s>>>(a);
    return hipGetLastError();
}

#endif // SX_TURB_EXACT

#ifdef SX_TURB_FAST

//! harmonics e^{i n t}, n = 0 .. kMaxHarmonic, of one axis
struct Harm
{
    float c[kAxis], s[kAxis];
};

__device__ __forceinline__ Harm harmonics(double t)
{
    Harm h;
    h.c[0] = 1.0f, h.s[0] = 0.0f;
    // the angle is reduced in double and split into a float and its remainder: sin, cos of the float, corrected to
    // first order by the remainder (second order: 2^-49)
    t -= 6.283185307179586 * rint(t * 0.15915494309189535);
    const float th = (float)t, tl = (float)(t - (double)th);
    float       sn, cs;
    sincosf(th, &sn, &cs);
    h.s[1] = sn + tl * cs;
    h.c[1] = cs - tl * sn;
#pragma unroll
    for (int n = 2; n < kAxis; ++n)
    {
        h.c[n] = h.c[n - 1] * h.c[1] - h.s[n - 1] * h.s[1];
        h.s[n] = h.s[n - 1] * h.c[1] + h.c[n - 1] * h.s[1];
    }
    return h;
}

//! acc += Re(coef) Re(E) - Im(coef) Im(E) for x, y, z; coef: one slot of the table (wave-uniform address)
__device__ __forceinline__ void addSlot(const float* __restrict__ coef, float er, float ei, float acc[3])
{
#pragma unroll
    for (int e = 0; e < 3; ++e)
        acc[e] += coef[2 * e] * er - coef[2 * e + 1] * ei;
}

template<int I, int J>
__device__ __forceinline__ void addRow(const float* __restrict__ table, uint64_t present, const Harm& hx,
                                       const Harm& hy, const Harm& hz, float acc[3])
{
    constexpr int      row     = (I * kAxis + J) * kAxis;
    constexpr uint64_t rowMask = ((uint64_t(1) << kAxis) - 1) << row;
    if (!(present & rowMask)) return;
    // P = e^{i(I x + J y)}, Q = e^{i(I x - J y)}
    const float cc = hx.c[I] * hy.c[J], ss = hx.s[I] * hy.s[J], sc = hx.s[I] * hy.c[J], cs = hx.c[I] * hy.s[J];
    const float pr = cc - ss, pi = sc + cs, qr = cc + ss, qi = sc - cs;
#pragma unroll
    for (int K = 0; K < kAxis; ++K)
    {
        if (!((present >> (row + K)) & 1)) continue;
        const float* __restrict__ coef = table + (row + K) * 4 * kSlotCoefs;
        const float cz = hz.c[K], sz = hz.s[K];
        const float prc = pr * cz, pis = pi * sz, pic = pi * cz, prs = pr * sz;
        const float qrc = qr * cz, qis = qi * sz, qic = qi * cz, qrs = qr * sz;
        addSlot(coef, prc - pis, pic + prs, acc);                  // (+J, +K)
        addSlot(coef + kSlotCoefs, qrc - qis, qic + qrs, acc);     // (-J, +K)
        addSlot(coef + 2 * kSlotCoefs, prc + pis, pic - prs, acc); // (+J, -K)
        addSlot(coef + 3 * kSlotCoefs, qrc + qis, qic - qrs, acc); // (-J, -K)
    }
}

template<int I>
__device__ __forceinline__ void addPlane(const float* __restrict__ table, uint64_t present, const Harm& hx,
                                         const Harm& hy, const Harm& hz, float acc[3])
{
    addRow<I, 0>(table, present, hx, hy, hz, acc);
    addRow<I, 1>(table, present, hx, hy, hz, acc);
    addRow<I, 2>(table, present, hx, hy, hz, acc);
    addRow<I, 3>(table, present, hx, hy, hz, acc);
}
static_assert(kAxis == 4, "addPlane / stirFastKernel list the lattice rows and planes");

//! table: the coefficients as a kernel argument of its own -- only a noalias argument lets the compiler prove the
//! table is not written through ax, ay, az and read it with scalar loads (as a member of `a`: 392 per-lane loads)
__global__ __launch_bounds__(256) void stirFastKernel(StirArgs a, const float* __restrict__ table)
{
    const uint32_t w    = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t       s, e;
    if (!groupBounds(a, w, s, e)) return;
    const uint64_t present = a.present;
    for (uint32_t i = s + lane; i < e; i += 64)
    {
        const Harm hx = harmonics(a.w0 * a.x[i]), hy = harmonics(a.w0 * a.y[i]), hz = harmonics(a.w0 * a.z[i]);
        float      acc[3] = {0.0f, 0.0f, 0.0f};
        addPlane<0>(table, present, hx, hy, hz, acc);
        addPlane<1>(table, present, hx, hy, hz, acc);
        addPlane<2>(table, present, hx, hy, hz, acc);
        addPlane<3>(table, present, hx, hy, hz, acc);
        a.ax[i] = (float)((double)a.ax[i] + (double)acc[0]);
        a.ay[i] = (float)((double)a.ay[i] + (double)acc[1]);
        a.az[i] = (float)((double)a.az[i] + (double)acc[2]);
    }
}

hipError_t stirFast(const StirArgs& a, hipStream_t s)
{
    if (a.numGroups) stirFastKernel<<<waveGrid(a.numGroups), 256, 0, s>>>(a, a.table);
    return hipGetLastError();
}

#endif // SX_TURB_FAST

} // namespace sx::turb
