/*! @file sx_fft.hip
 * @brief The 3-D transform of the spectra (sx_spectrum.hpp): complex to complex, double, in place, n in {16 .. 256}.
 *
 * One kernel transforms kLines lines of n points in LDS and is applied along x, then y, then z.  A line transform is a
 * Stockham autosort: radix-4 stages, preceded by one radix-2 stage where log2 n is odd (its twiddles are all 1).  Stage
 * Ns (the length of the sub-transforms done so far) has thread j of a line read the points j + q n / 4, multiply them by
 * exp(-2 pi i q k / (4 Ns)), k = j mod Ns, from the table, and write the butterfly's outputs to (j - k) 4 + k + q Ns: the
 * result is in natural order, no bit reversal.  The points pass through registers between two barriers, so one LDS
 * buffer serves (a second one would not fit beside it at n = 256).
 *
 * Global access.  Along x a workgroup takes kLines consecutive rows (contiguous).  Along y and z it takes a tile of
 * kLines = 16 adjacent x: 16 x 16 B = 256 B contiguous per row of the tile, so the loads and stores stay coalesced.
 * A line in LDS has n + 1 elements: with a stride that is a multiple of 256 B every line would start on the same banks,
 * and the 16 lanes that fill one row of the tile would collide 16-fold.
 * 16 lines x 257 x 16 B + the table's 4 KB = 68 KB of the 160 KB of LDS at n = 256: two workgroups of 1024 per CU.
 */
#include "sx_spectrum.hpp"

namespace sx::spectrum
{

namespace
{

constexpr int kLines = 16;

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

//! element i of line l of tile b
template<int N, int Pass>
__device__ __forceinline__ size_t address(uint32_t b, int l, int i)
{
    if (Pass == 0) return ((size_t)b * kLines + l) * N + i;
    if (Pass == 1) return (size_t)(b / (N / kLines)) * N * N + (size_t)i * N + (b % (N / kLines)) * kLines + l;
    return (size_t)i * N * N + (size_t)b * kLines + l;
}

template<int N, int Pass>
__global__ __launch_bounds__(kLines* N / 4) void lineKernel(double2* __restrict__ mesh, const double2* __restrict__ table,
                                                            double scale)
{
    constexpr int T      = N / 4; // threads per line
    constexpr int NT     = kLines * T;
    constexpr int stride = N + 1;
    constexpr bool odd   = N == 32 || N == 128;
    __shared__ double2 buf[kLines * stride];
    __shared__ double2 tw[N];
    const int      tid = threadIdx.x;
    const uint32_t b   = blockIdx.x;

    for (int k = tid; k < N; k += NT)
        tw[k] = table[k];
    for (int idx = tid; idx < kLines * N; idx += NT)
    {
        const int l = Pass == 0 ? idx / N : idx % kLines, i = Pass == 0 ? idx % N : idx / kLines;
        buf[l * stride + i] = mesh[address<N, Pass>(b, l, i)];
    }
    __syncthreads();

    double2*  line = buf + (tid / T) * stride;
    const int j    = tid % T;
    int       Ns   = 1;
    if (odd)
    {
        const double2 a0 = line[j], a1 = line[j + N / 2], b0 = line[j + T], b1 = line[j + T + N / 2];
        __syncthreads();
        line[2 * j]           = cadd(a0, a1);
        line[2 * j + 1]       = csub(a0, a1);
        line[2 * (j + T)]     = cadd(b0, b1);
        line[2 * (j + T) + 1] = csub(b0, b1);
        __syncthreads();
        Ns = 2;
    }
    for (; Ns < N; Ns *= 4)
    {
        const int k = j & (Ns - 1), step = N / (4 * Ns);
        double2   v0 = line[j], v1 = line[j + T], v2 = line[j + 2 * T], v3 = line[j + 3 * T];
        if (Ns > 1)
        {
            v1 = cmul(v1, tw[k * step]);
            v2 = cmul(v2, tw[2 * k * step]);
            v3 = cmul(v3, tw[3 * k * step]);
        }
        const double2 t0 = cadd(v0, v2), t1 = csub(v0, v2), t2 = cadd(v1, v3), d = csub(v1, v3);
        const double2 t3 = make_double2(d.y, -d.x); // -i (v1 - v3)
        __syncthreads();
        const int j0      = ((j - k) << 2) + k;
        line[j0]          = cadd(t0, t2);
        line[j0 + Ns]     = cadd(t1, t3);
        line[j0 + 2 * Ns] = csub(t0, t2);
        line[j0 + 3 * Ns] = csub(t1, t3);
        __syncthreads();
    }

    for (int idx = tid; idx < kLines * N; idx += NT)
    {
        const int     l = Pass == 0 ? idx / N : idx % kLines, i = Pass == 0 ? idx % N : idx / kLines;
        const double2 v = buf[l * stride + i];
        mesh[address<N, Pass>(b, l, i)] = make_double2(v.x * scale, v.y * scale);
    }
}

template<int N>
hipError_t launch(double2* mesh, const double2* tw, hipStream_t s)
{
    constexpr unsigned tiles = N * N / kLines, threads = kLines * N / 4;
    lineKernel<N, 0><<<tiles, threads, 0, s>>>(mesh, tw, 1.0);
    lineKernel<N, 1><<<tiles, threads, 0, s>>>(mesh, tw, 1.0);
    lineKernel<N, 2><<<tiles, threads, 0, s>>>(mesh, tw, 1.0 / ((double)N * N * N)); // a power of two: exact
    return hipGetLastError();
}

} // namespace

hipError_t fftLaunch(double2* mesh, uint32_t n, const double2* tw, hipStream_t s)
{
    switch (n)
    {
        case 16: return launch<16>(mesh, tw, s);
        case 32: return launch<32>(mesh, tw, s);
        case 64: return launch<64>(mesh, tw, s);
        case 128: return launch<128>(mesh, tw, s);
        case 256: return launch<256>(mesh, tw, s);
        default: return hipErrorInvalidValue;
    }
}

} // namespace sx::spectrum
