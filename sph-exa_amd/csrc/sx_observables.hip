/*! @file sx_observables.hip
 * @brief Conserved quantities of the locally owned particles on the GPU (replaces conservedQuantitiesGpu,
 *        main/src/observables/conserved_gpu.cu:71-94, and the nc reduction of computeConservedQuantities,
 *        conserved_quantities.hpp:118-131).
 *
 * One pass over [first, last): kinetic energy sum m |v|^2 (halved at the end), internal energy sum u m (or
 * cv T m), linear momentum sum m v, angular momentum sum m (x cross v) and sum nc, all in double.  Each workgroup
 * reduces its 256 particles with wave shuffles and writes one partial per quantity; a second one-workgroup pass sums
 * the partials in a fixed order, so the result is deterministic (independent of scheduling).
 *
 * observablesKernel<Kind> fuses those sums with the ones of the reference's other observables (turbulence Mach RMS,
 * Kelvin-Helmholtz growth rate, wind-shock cloud survival: gpu_reductions.cu:47-151; gravitational-wave quadrupole:
 * grav_waves_calculations.hpp:87-121, host-only in the reference) in one persistent grid-stride pass.
 */
#include "sx_observables.hpp"

namespace sx
{

namespace
{

constexpr int kQ = 10; // eKin, eInt, linmom xyz, angmom xyz, ncsum, (spare)

template<class T>
__device__ __forceinline__ T blockSum(T v, T* s)
{
    v = waveSum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
            r += s[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void conservedPartialKernel(ConservedArgs a, double* partial)
{
    __shared__ double s[4];
    const size_t i = a.first + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    double q[kQ] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < a.last)
    {
        const double m  = a.m[i];
        const double X0 = a.x[i], X1 = a.y[i], X2 = a.z[i];
        const double V0 = a.vx[i], V1 = a.vy[i], V2 = a.vz[i];
        q[0]            = m * (V0 * V0 + V1 * V1 + V2 * V2);
        q[1]            = a.u ? a.u[i] * m : (a.temp ? a.cv * a.temp[i] * m : 0.0);
        q[2] = m * V0, q[3] = m * V1, q[4] = m * V2;
        q[5] = m * (X1 * V2 - X2 * V1);
        q[6] = m * (X2 * V0 - X0 * V2);
        q[7] = m * (X0 * V1 - X1 * V0);
        q[8] = a.nc ? (double)a.nc[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k)
    {
        const double v = blockSum(q[k], s);
        if (threadIdx.x == 0) partial[(size_t)k * gridDim.x + blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void conservedFinalKernel(const double* partial, int nb, double* out)
{
    __shared__ double s[4];
    for (int k = 0; k < kQ; ++k)
    {
        double acc = 0;
        for (int b = threadIdx.x; b < nb; b += blockDim.x)
            acc += partial[(size_t)k * nb + b];
        acc = blockSum(acc, s);
        if (threadIdx.x == 0) out[k] = k == 0 ? 0.5 * acc : acc;
    }
}

// ---- the fused observables pass --------------------------------------------------------------------------------
//
// A fixed grid of at most kObsGrid workgroups; workgroup b takes the chunks b, b + grid, b + 2 grid, ... of
// kObsChunk consecutive particles, in that order, each thread kObsUnroll particles of a chunk a block width apart
// (coalesced).  The grid (min(kObsGrid, chunks of n)) and the partition depend on n alone, the lanes add their terms
// in a fixed order, the wave, the block and the final pass sum in fixed trees: the result is the same from run to
// run and on any device.  Per workgroup and sum one waveSum, then all sums cross LDS behind ONE barrier.

// the results depend on kObsUnroll and kObsGrid (the partition)
constexpr int kObsBlock  = 256;
constexpr int kObsUnroll = 2;
constexpr int kObsChunk  = kObsBlock * kObsUnroll;
constexpr int kObsGrid   = 1024; // 4 workgroups per CU of an MI355X, 2 loads of every field in flight per lane
// register budget (128 VGPRs) at which the whole grid is resident at once there; the KH growth's double exp, sin and
// cos would spill under it and take one wave less (that kind is bound by their arithmetic, not by residency)
constexpr int kObsWavesPerSimd = 4;

/*! the terms of particle i added to q: q[0..8] as conservedPartialKernel, then the kind's.  Types and operation order
 *  are the reference's with sph::SphTypes (x, y, z, temp double; v, a, m, c, kx, xm float); every float step is
 *  written as one, everything else is double.  This file is compiled without contraction. */
template<int Kind, bool Cons>
__device__ __forceinline__ void obsTerms(const ObsArgs& a, size_t i, double* q)
{
    constexpr bool needX = Cons || Kind == kObsKhGrowth || Kind == kObsGravWaves;
    constexpr bool needV = Cons || Kind == kObsMachRms || Kind == kObsKhGrowth || Kind == kObsGravWaves;
    constexpr bool needM = Cons || Kind == kObsWindBubble || Kind == kObsGravWaves;
    double X0 = 0, X1 = 0, X2 = 0, T = 0;
    float  v0 = 0, v1 = 0, v2 = 0, mf = 0;
    if constexpr (needX) X0 = a.c.x[i], X1 = a.c.y[i];
    if constexpr (Cons || Kind == kObsGravWaves) X2 = a.c.z[i];
    if constexpr (needV) v1 = a.c.vy[i];
    if constexpr (Cons || Kind == kObsMachRms || Kind == kObsGravWaves) v0 = a.c.vx[i], v2 = a.c.vz[i];
    if constexpr (needM) mf = a.c.m[i];
    // temp is read where it is used: the internal energy without u, and the wind bubble's criterion (uniform branch)
    if constexpr (Cons || Kind == kObsWindBubble)
        if (a.c.temp && (Kind == kObsWindBubble || !a.c.u)) T = a.c.temp[i];
    if constexpr (Cons)
    {
        const double m  = mf;
        const double V0 = v0, V1 = v1, V2 = v2;
        q[0] += m * (V0 * V0 + V1 * V1 + V2 * V2);
        q[1] += a.c.u ? a.c.u[i] * m : (a.c.temp ? a.c.cv * T * m : 0.0);
        q[2] += m * V0, q[3] += m * V1, q[4] += m * V2;
        q[5] += m * (X1 * V2 - X2 * V1);
        q[6] += m * (X2 * V0 - X0 * V2);
        q[7] += m * (X0 * V1 - X1 * V0);
        q[8] += a.c.nc ? (double)a.c.nc[i] : 0.0;
    }
    if constexpr (Kind == kObsMachRms)
    {
        // MachSquareSum (gpu_reductions.cu:98-107): norm2(V) / (c * c) in Tv = T = float, returned as double
        // A particle at rest has Mach number 0 whatever c holds: before an sx_sim's first step c is not computed yet
        // and the quotient would be 0/0 (the one deviation from the reference's term).
        const float c  = a.cs[i];
        const float vsq = v0 * v0 + v1 * v1 + v2 * v2;
        q[9] += vsq == 0.0f ? 0.0 : (double)(vsq / (c * c));
    }
    if constexpr (Kind == kObsKhGrowth)
    {
        // localGrowthRate (time_energy_growth.hpp:57-63): Tc voli = xm / kx divides in float, the rest is double
        const float  volf = a.xm[i] / a.kx[i];
        const double voli = volf;
        const double aux  = X1 < a.ybox * 0.5 ? exp(-4.0 * M_PI * fabs(X1 - 0.25))
                                              : exp(-4.0 * M_PI * fabs(a.ybox - X1 - 0.25));
        const double vyv = (double)v1 * voli;
        q[9] += vyv * sin(4.0 * M_PI * X0) * aux;
        q[10] += vyv * cos(4.0 * M_PI * X0) * aux;
        q[11] += voli * aux;
    }
    if constexpr (Kind == kObsWindBubble)
    {
        // Survivors (gpu_reductions.cu:132-151): rhoi = kx / xm * m in float against 0.64 rhoBubble in double
        const float rhoi = a.kx[i] / a.xm[i] * mf;
        q[9] += ((double)rhoi >= a.rhoMin && T <= a.tempMax) ? 1.0 : 0.0;
    }
    if constexpr (Kind == kObsGravWaves)
    {
        // d2QuadpoleMomentum (grav_waves_calculations.hpp:87-121), Tc double, Tv = Ta = Tm float
        const float  a0 = a.ax[i], a1 = a.ay[i], a2 = a.az[i];
        const double m      = mf;
        const float  scalv2 = v0 * v0 + v1 * v1 + v2 * v2;                            // :102, Tv
        const double cda    = X0 * (double)a0 + X1 * (double)a1 + X2 * (double)a2;    // :103, Tc
        q[9] += (3.0 * ((double)(v0 * v0) + X0 * (double)a0) - (double)scalv2 - cda) * m; // :106
        q[10] += (3.0 * ((double)(v1 * v1) + X1 * (double)a1) - (double)scalv2 - cda) * m;
        q[11] += (3.0 * ((double)(v2 * v2) + X2 * (double)a2) - (double)scalv2 - cda) * m;
        q[12] += (2.0 * (double)v0 * (double)v1 + (double)a0 * X1 + X0 * (double)a1) * m; // :116
        q[13] += (2.0 * (double)v0 * (double)v2 + (double)a0 * X2 + X0 * (double)a2) * m;
        q[14] += (2.0 * (double)v1 * (double)v2 + (double)a1 * X2 + X1 * (double)a2) * m;
    }
}

template<int Kind, bool Cons>
__global__ __launch_bounds__(kObsBlock, Kind == kObsKhGrowth ? kObsWavesPerSimd - 1 : kObsWavesPerSimd) void
observablesKernel(ObsArgs a, double* partial)
{
    constexpr int NQ = kObsConserved + obsExtraSums(Kind);
    __shared__ double s[NQ][kObsBlock / kWave];
    double q[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k)
        q[k] = 0.0;

    const size_t n         = a.c.last - a.c.first;
    const size_t numChunks = (n + kObsChunk - 1) / kObsChunk;
    for (size_t c = blockIdx.x; c < numChunks; c += gridDim.x)
    {
        const size_t i0 = a.c.first + c * kObsChunk + threadIdx.x;
        if ((c + 1) * kObsChunk <= n) // a whole chunk: no bound checks, the unrolled loads issue together
        {
#pragma unroll
            for (int u = 0; u < kObsUnroll; ++u)
                obsTerms<Kind, Cons>(a, i0 + (size_t)u * kObsBlock, q);
        }
        else
        {
#pragma unroll
            for (int u = 0; u < kObsUnroll; ++u)
                if (i0 + (size_t)u * kObsBlock < a.c.last) obsTerms<Kind, Cons>(a, i0 + (size_t)u * kObsBlock, q);
        }
    }

#pragma unroll
    for (int k = 0; k < NQ; ++k)
    {
        const double v = waveSum(q[k]);
        if ((threadIdx.x & (kWave - 1)) == 0) s[k][threadIdx.x / kWave] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ)
    {
        double r = 0;
        for (int w = 0; w < kObsBlock / kWave; ++w)
            r += s[threadIdx.x][w];
        partial[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
    }
}

//! sums the nb partials of each of the nq sums in a fixed order; out[nq] = the number of particles
__global__ __launch_bounds__(256) void observablesFinalKernel(const double* partial, int nb, int nq, int kind,
                                                              double count, double* out)
{
    __shared__ double s[4];
    for (int k = 0; k < nq; ++k)
    {
        double acc = 0;
        for (int b = threadIdx.x; b < nb; b += blockDim.x)
            acc += partial[(size_t)k * nb + b];
        acc = blockSum(acc, s);
        if (threadIdx.x == 0)
        {
            if (k == 0) acc = 0.5 * acc;
            // the diagonal's 2/3 after the sum, as `return out * 2.0 / 3.0` (grav_waves_calculations.hpp:108)
            if (kind == kObsGravWaves && k >= kObsConserved && k < kObsConserved + 3) acc = acc * 2.0 / 3.0;
            out[k] = acc;
        }
    }
    if (threadIdx.x == 0) out[nq] = count;
}

template<int Kind>
void launchObservables(const ObsArgs& a, int nb, double* scratch, hipStream_t s)
{
    if (a.conserved) observablesKernel<Kind, true><<<nb, kObsBlock, 0, s>>>(a, scratch);
    else observablesKernel<Kind, false><<<nb, kObsBlock, 0, s>>>(a, scratch);
}

} // namespace

size_t observablesScratch() { return (size_t)kObsMaxSums * kObsGrid; }

hipError_t observables(int kind, const ObsArgs& a, double* scratch, double* out, hipStream_t s)
{
    if (kind < 0 || kind >= kObsKinds) return hipErrorInvalidValue;
    const size_t n      = a.c.last > a.c.first ? a.c.last - a.c.first : 0;
    const size_t chunks = (n + kObsChunk - 1) / kObsChunk;
    const int    nb     = (int)std::min<size_t>(kObsGrid, std::max<size_t>(1, chunks));
    ObsArgs      b      = a;
    if (n == 0) b.c.last = b.c.first;
    switch (kind)
    {
        case kObsTimeEnergy: launchObservables<kObsTimeEnergy>(b, nb, scratch, s); break;
        case kObsMachRms: launchObservables<kObsMachRms>(b, nb, scratch, s); break;
        case kObsKhGrowth: launchObservables<kObsKhGrowth>(b, nb, scratch, s); break;
        case kObsWindBubble: launchObservables<kObsWindBubble>(b, nb, scratch, s); break;
        default: launchObservables<kObsGravWaves>(b, nb, scratch, s); break;
    }
    observablesFinalKernel<<<1, 256, 0, s>>>(scratch, nb, kObsConserved + obsExtraSums(kind), kind, (double)n, out);
    return hipGetLastError();
}

size_t conservedScratch(size_t n) { return (size_t)kQ * std::max<size_t>(1, (n + 255) / 256); }

hipError_t conservedQuantities(const ConservedArgs& a, double* scratch, double* out, hipStream_t s)
{
    const size_t n  = a.last > a.first ? a.last - a.first : 0;
    const int    nb = (int)std::max<size_t>(1, (n + 255) / 256);
    conservedPartialKernel<<<nb, 256, 0, s>>>(a, scratch);
    conservedFinalKernel<<<1, 256, 0, s>>>(scratch, nb, out);
    return hipGetLastError();
}

} // namespace sx
