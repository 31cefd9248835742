/*! @file sx_cool.hip
 * @brief the two kernels of the radiative cooling (sx_cool.hpp): the exact integration of every particle's
 *        temperature over the step, with a deterministic sum of the energy radiated, and the shortest cooling time.
 *
 * Both stage the table (T, L, alpha, Y: at most 8 KB) in LDS once per block and walk the particles in tiles of one
 * block; the grid is a function of n alone (partialBlocks), so a block's particles, and with them every partial sum,
 * are the same on every run.  The searches take a fixed number of iterations (sx_cool.hpp), so the lanes of a wave
 * stay together up to the alpha == 1 select.  A particle costs 24 bytes (temp read and written, rho and m read) and two
 * logarithm / exponential pairs in double.
 */
#include "sx_cool.hpp"

namespace sx::cool
{

namespace
{

constexpr int      kBlock     = 256;
constexpr int      kWaves     = kBlock / 64;
constexpr uint32_t kMaxBlocks = 1024; // four blocks on each of the 256 CUs

//! the block's LDS copy of the table
__device__ inline Table stageTable(double* sh, const double* table, uint32_t numNodes)
{
    for (uint32_t i = threadIdx.x; i < 4 * numNodes; i += kBlock)
        sh[i] = table[i];
    __syncthreads();
    return Table{sh, sh + numNodes, sh + 2 * numNodes, sh + 3 * numNodes, numNodes};
}

__device__ inline double densityOf(const Density& d, uint64_t i)
{
    return d.rho ? (double)d.rho[i] : (double)((d.kx[i] * d.m[i]) / d.xm[i]);
}

//! the sum over the block in a fixed order (shuffle tree per wave, then the waves in index order), valid in thread 0
template<class T>
__device__ inline T blockSum(T v, T* shw)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) shw[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = shw[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
        r += shw[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void coolKernel(CoolArgs a)
{
    __shared__ double   sh[4 * kMaxNodes];
    __shared__ double   shE[kWaves];
    __shared__ uint32_t shC[kWaves];
    const Table  t  = stageTable(sh, a.table, a.numNodes);
    const double dt = a.dtPtr ? *a.dtPtr : a.dt;
    const double T1 = t.T[0];
    double       e  = 0.0;
    uint32_t     onFloor = 0, cooled = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * kBlock)
    {
        const double T0 = a.temp[i];
        const double s  = (densityOf(a.d, i) * dt) / a.cv;
        const double Tn = integrate(t, T0, s);
        if (T0 >= T1) // below the floor (or NaN): untouched, no term
        {
            if (Tn != T0) a.temp[i] = Tn;
            e += ((double)a.m[i] * a.cv) * (T0 - Tn);
            ++cooled;
            if (Tn == T1) ++onFloor;
        }
    }
    e       = blockSum(e, shE);
    onFloor = blockSum(onFloor, shC);
    cooled  = blockSum(cooled, shC);
    if (threadIdx.x == 0)
    {
        a.ePart[blockIdx.x]         = e;
        a.cPart[2 * blockIdx.x]     = onFloor;
        a.cPart[2 * blockIdx.x + 1] = cooled;
    }
}

//! one block: every thread its run of consecutive partials in index order, then the block's fixed order
__global__ __launch_bounds__(kBlock) void coolFoldKernel(uint32_t blocks, const double* ePart, const uint32_t* cPart,
                                                         double* stats, double* total)
{
    __shared__ double   shE[kWaves];
    __shared__ uint32_t shC[kWaves];
    const uint32_t per = (blocks + kBlock - 1) / kBlock;
    double         e   = 0.0;
    uint32_t       onFloor = 0, cooled = 0;
    for (uint32_t b = threadIdx.x * per; b < blocks && b < (threadIdx.x + 1) * per; ++b)
    {
        e += ePart[b];
        onFloor += cPart[2 * b];
        cooled += cPart[2 * b + 1];
    }
    e       = blockSum(e, shE);
    onFloor = blockSum(onFloor, shC);
    cooled  = blockSum(cooled, shC);
    if (threadIdx.x == 0)
    {
        stats[0] = e;
        stats[1] = (double)onFloor;
        stats[2] = (double)cooled;
        if (total) *total += e;
    }
}

__global__ void initMinKernel(unsigned long long* minBits) { *minBits = (unsigned long long)__double_as_longlong(INFINITY); }

__global__ __launch_bounds__(kBlock) void coolingTimeKernel(CoolTimeArgs a)
{
    __shared__ double sh[4 * kMaxNodes];
    __shared__ double shM[kWaves];
    const Table t  = stageTable(sh, a.table, a.numNodes);
    double      tc = INFINITY;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * kBlock)
    {
        const double ti = coolingTime(t, a.temp[i], densityOf(a.d, i), a.cv);
        tc              = ti < tc ? ti : tc;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        const double o = __shfl_xor(tc, off, 64);
        tc             = o < tc ? o : tc;
    }
    if ((threadIdx.x & 63) == 0) shM[threadIdx.x >> 6] = tc;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < kWaves; ++w)
            tc = shM[w] < tc ? shM[w] : tc;
        // cooling times are positive: their order is the order of their bit images (as Scalars::maxAccSqBits)
        if (tc >= 0.0) atomicMin(a.minBits, (unsigned long long)__double_as_longlong(tc));
    }
}

__global__ void scaledMinKernel(const unsigned long long* minBits, double factor, double* out)
{
    *out = factor * __longlong_as_double((long long)*minBits);
}

} // namespace

uint32_t partialBlocks(uint32_t n)
{
    const uint64_t b = ((uint64_t)n + kBlock - 1) / kBlock;
    return (uint32_t)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

hipError_t coolLaunch(const CoolArgs& a, hipStream_t s)
{
    const uint32_t blocks = partialBlocks(a.n);
    coolKernel<<<blocks, kBlock, 0, s>>>(a);
    coolFoldKernel<<<1, kBlock, 0, s>>>(blocks, a.ePart, a.cPart, a.stats, a.total);
    return hipGetLastError();
}

hipError_t coolingTimeLaunch(const CoolTimeArgs& a, hipStream_t s)
{
    initMinKernel<<<1, 1, 0, s>>>(a.minBits);
    if (a.n) coolingTimeKernel<<<partialBlocks(a.n), kBlock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t scaledMin(const unsigned long long* minBits, double factor, double* out, hipStream_t s)
{
    scaledMinKernel<<<1, 1, 0, s>>>(minBits, factor, out);
    return hipGetLastError();
}

} // namespace sx::cool
