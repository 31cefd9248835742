/*! @file sx_spectrum.hip
 * @brief Power spectra (sx_spectrum.hpp): the mesh deposit (binning into blocks of 8 x 8 x 4 cells and a radix sort of
 *        the (block, particle) pairs, both the pair-binning engine's (sx_pairbin.hpp), then one workgroup per block that
 *        gathers its list through LDS in list order), the field
 *        that is transformed, and the deterministic shell sums.  The transform itself is in sx_fft.hip.
 *
 * Geometry of the deposit, in cell units from the box corner: cell i has its centre at i + 0.5 and a particle at f with
 * reach r = 2 he / D >= 1 touches the cells whose centres lie within r of one of its images, i in
 * [ceil(f - r - 0.5), floor(f + r - 0.5)] modulo n; 2 r >= n reaches every cell of the axis.  The gather places a record
 * by the minimum image about its BLOCK centre, relative to the block origin (small numbers: float keeps them to 2^-24 of
 * the block's extent plus the reach), and every lane folds its own distances by whole periods (d - n rint(d / n)), as
 * does the per-wave cull: a support may be wider than half the box when n is small against h, and a cell sees the
 * minimum-image distance then too.  The kernel value is exactly 0 beyond the support (kernelWt), so the binning and the
 * cull may be conservative without changing a bit of the mesh.
 */
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sx_device.hpp"
#include "sx_kernel_poly.hpp"
#include "sx_spectrum.hpp"

namespace sx::spectrum
{

bool validN(uint32_t n) { return n == 16 || n == 32 || n == 64 || n == 128 || n == 256; }

uint32_t shellOf(uint32_t k2)
{
    uint32_t s = (uint32_t)std::floor(std::sqrt((double)k2) + 0.5);
    // the integer criterion decides: s (s - 1) < k2 <= s (s + 1)
    while (s > 0 && !(s * (s - 1) < k2)) --s;
    while (k2 > s * (s + 1)) ++s;
    return s;
}

uint32_t numShells(uint32_t n) { return validN(n) ? shellOf(3 * (n / 2) * (n / 2)) + 1 : 0; }

void shellModes(uint32_t n, uint64_t* modes)
{
    const uint32_t ns = numShells(n);
    std::fill(modes, modes + ns, uint64_t(0));
    const int h = (int)n / 2;
    // squared lengths of one axis occur in pairs but for -n/2 and 0: count over two axes first
    std::vector<uint64_t> two(2 * h * h + 1, 0);
    for (int a = -h; a < h; ++a)
        for (int b = -h; b < h; ++b)
            ++two[a * a + b * b];
    for (uint32_t q = 0; q < two.size(); ++q)
        if (two[q])
            for (int c = -h; c < h; ++c)
                modes[shellOf(q + c * c)] += two[q];
}

const char* checkSpec(const sx_spectrum* sp, const sx_box* box)
{
    if (!sp || !box) return "sx_spectrum_check: null spectrum or box";
    if (sp->kind != SX_SPEC_VELOCITY && sp->kind != SX_SPEC_SCALAR)
        return "sx_spectrum_check: unknown kind (SX_SPEC_VELOCITY or SX_SPEC_SCALAR)";
    if (sp->weight < 0 || sp->weight > 2) return "sx_spectrum_check: unknown weight (0: p = 0, 1: p = 1/2, 2: p = 1/3)";
    if (sp->kind == SX_SPEC_SCALAR && sp->weight != 0) return "sx_spectrum_check: SX_SPEC_SCALAR takes weight 0 only";
    if (!validN(sp->n)) return "sx_spectrum_check: n must be 16, 32, 64, 128 or 256";
    for (int k = 0; k < 3; ++k)
        if (box->bnd[k] != 1) return "sx_spectrum_check: the box must be periodic on all three axes";
    const double L = box->lim[1] - box->lim[0];
    if (!(L > 0.0) || !std::isfinite(L)) return "sx_spectrum_check: the box must be cubic (its x edge is not positive)";
    for (int k = 1; k < 3; ++k)
        if (std::fabs((box->lim[2 * k + 1] - box->lim[2 * k]) - L) > 1e-12 * L) return "sx_spectrum_check: the box must be cubic";
    return nullptr;
}

void twiddleTable(uint32_t n, std::vector<double2>& t)
{
    t.resize(n);
    // exp(-2 pi i k / n) = (c, -s) with (c, s) of the angle 2 pi k / n, reduced to [0, pi / 4]: libm's sin and cos are
    // within 1 ulp there and the reflections are exact
    for (uint32_t k = 0; k < n; ++k)
    {
        const uint32_t oct = (8 * k) / n;          // octant of the angle
        const uint32_t q   = (oct + 1) / 2;        // nearest multiple of pi / 2
        const int      r   = (int)k - (int)(q * n / 4); // angle - q pi / 2 in units of 2 pi / n, |r| <= n / 8
        const double   a   = 2.0 * M_PI * (double)std::abs(r) / (double)n;
        const double   c0 = std::cos(a), s0 = r < 0 ? -std::sin(a) : std::sin(a);
        double         c, s;
        switch (q & 3)
        {
            case 0: c = c0, s = s0; break;
            case 1: c = -s0, s = c0; break;
            case 2: c = -c0, s = -s0; break;
            default: c = s0, s = -c0; break;
        }
        t[k] = make_double2(c, -s);
    }
}

namespace
{

//! the mesh in the units the kernels use
struct Plan
{
    int    n, nbx, nby, nbz;
    double lo[3], L, D, iD, hmin, K;
    float  nf, inf; // the period in cells and its inverse
};

struct Particles
{
    const double *x, *y, *z;
    const float * h, *m;
    const void*   a[3];
    int           numA, aIsDouble;
};

//! blocks of extent B touched along one axis: count of them from block `start` on (modulo nb)
struct Span
{
    int start, count;
};

__device__ inline Span blockSpan(double f, double r, int n, int B, int nb)
{
    if (2.0 * r >= (double)n) return Span{0, nb};
    const double lo = ceil(f - r - 0.5 - 1e-6), hi = floor(f + r - 0.5 + 1e-6);
    if (!(lo <= hi)) return Span{0, 0}; // not with r >= 1
    const int blo = (int)floor(lo / B), bhi = (int)floor(hi / B);
    const int cnt = std::min(bhi - blo + 1, nb);
    return Span{((blo % nb) + nb) % nb, cnt};
}

//! position in cell units from the box corner, in [0, n), and the reach in cells
__device__ inline void place(const Plan& p, const Particles& q, uint32_t i, double f[3], double& r, bool& clamped)
{
    const double pos[3] = {q.x[i], q.y[i], q.z[i]};
    for (int k = 0; k < 3; ++k)
    {
        double d = (pos[k] - p.lo[k]) * p.iD;
        d -= (double)p.n * floor(d / (double)p.n);
        f[k] = d;
    }
    const double h = (double)q.h[i];
    clamped        = h < p.hmin;
    r              = 2.0 * fmax(h, p.hmin) * p.iD;
}

/*! the engine's geometry (sx_pairbin.hpp): rows are block layers along z, units the blocks of one; counts[0] tallies the
 *  particles clamped to D / 2, whatever they touch */
struct Geom
{
    static constexpr int kMaxRows = kMaxLayers;
    struct Foot
    {
        Span sx{0, 0}, sy{0, 0}, sz{0, 0};
        bool clamped{false};
    };
    Plan      p;
    Particles q;

    __host__ __device__ int      rows() const { return p.nbz; }
    __host__ __device__ uint32_t unitsPerRow() const { return (uint32_t)(p.nbx * p.nby); }

    __device__ void foot(uint32_t i, Foot& ft) const
    {
        double f[3], r;
        place(p, q, i, f, r, ft.clamped);
        ft.sx = blockSpan(f[0], r, p.n, kBx, p.nbx), ft.sy = blockSpan(f[1], r, p.n, kBy, p.nby);
        ft.sz = blockSpan(f[2], r, p.n, kBz, p.nbz);
    }
    __device__ bool counted(const Foot& ft) const { return ft.clamped; }
    template<class F>
    __device__ void forRows(const Foot& ft, F&& f) const
    {
        const uint32_t per = (uint32_t)(ft.sx.count * ft.sy.count);
        if (!per) return;
        for (int k = 0; k < ft.sz.count; ++k)
            f((ft.sz.start + k) % p.nbz, per);
    }
    template<class F>
    __device__ void forUnits(const Foot& ft, int, F&& f) const
    {
        for (int ky = 0; ky < ft.sy.count; ++ky)
        {
            const int by = (ft.sy.start + ky) % p.nby;
            for (int kx = 0; kx < ft.sx.count; ++kx)
                f((uint32_t)(by * p.nbx + (ft.sx.start + kx) % p.nbx));
        }
    }
};

/*! one workgroup per block, one cell per lane (lane t: cell (t & 7, (t >> 3) & 7, t >> 6) of the block, so wave w owns
 *  the 8 x 8 layer z = w).  The block's list is staged through LDS kChunk records at a time, each lane building one
 *  record in double from the particle's fields; then every lane walks the chunk in list order.  The record address is
 *  the same in all lanes (an LDS broadcast read), and the test of the record's box against the wave's layer is
 *  wave-uniform, so a wave skips the records that cannot reach it without divergence.
 *  Record: {x, y, z relative to the block origin in cells, D^2 / he^2} {w, w a0, w a1, w a2} {reach in cells}.
 *  NA is the number of columns: the velocity spectrum's four accumulators need one pass over the lists.
 */
template<int NA>
__global__ __launch_bounds__(256) void gatherKernel(Plan p, Particles q, const uint64_t* __restrict__ pairs,
                                                    const uint32_t* __restrict__ offsets, int r0, uint32_t last,
                                                    double* __restrict__ sum0, double* __restrict__ sum1,
                                                    unsigned long long* counts)
{
    __shared__ float4 rec[2 * kChunk];
    __shared__ float  reach[kChunk];
    const int      t     = threadIdx.x;
    const uint32_t block = blockIdx.x;
    const int      bx = block % p.nbx, by = (block / p.nbx) % p.nby, bz = r0 + block / (p.nbx * p.nby);
    const uint32_t beg = offsets[block], end = offsets[block + 1];
    if (t == 0 && end > beg) atomicMax(&counts[1], (unsigned long long)(end - beg));

    const int   lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
    const float fx = (float)lx + 0.5f, fy = (float)ly + 0.5f, fz = (float)lz + 0.5f;
    // block centre in cells from the box corner
    const double cx = bx * kBx + kBx / 2, cy = by * kBy + kBy / 2, cz = bz * kBz + kBz / 2;

    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (uint32_t c0 = beg; c0 < end; c0 += kChunk)
    {
        const uint32_t cnt = std::min(kChunk, end - c0);
        __syncthreads(); // the previous chunk has been walked
        if ((uint32_t)t < cnt)
        {
            // every sorted key was written by emitKernel; the clamp keeps the gathers in bounds if one was not
            const uint32_t i  = std::min((uint32_t)pairs[c0 + t], last - 1);
            double         dx = (q.x[i] - p.lo[0]) * p.iD - cx, dy = (q.y[i] - p.lo[1]) * p.iD - cy,
                           dz = (q.z[i] - p.lo[2]) * p.iD - cz;
            dx -= (double)p.n * rint(dx / (double)p.n);
            dy -= (double)p.n * rint(dy / (double)p.n);
            dz -= (double)p.n * rint(dz / (double)p.n);
            const double he  = fmax((double)q.h[i], p.hmin);
            const double ih2 = 1.0 / (he * he);
            const float  wf  = (float)((double)q.m[i] * p.K * ih2 / he);
            float        af[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < NA; ++k)
                af[k] = q.aIsDouble ? (float)((const double*)q.a[k])[i] : ((const float*)q.a[k])[i];
            rec[2 * t]     = make_float4((float)(dx + kBx / 2), (float)(dy + kBy / 2), (float)(dz + kBz / 2),
                                         (float)(p.D * p.D * ih2));
            rec[2 * t + 1] = make_float4(wf, wf * af[0], wf * af[1], wf * af[2]);
            // the reach with a margin that covers the rounding of the float distances it is compared with
            reach[t] = (float)(2.0 * he * p.iD) * 1.0001f + 1e-3f;
        }
        __syncthreads();
        for (uint32_t k = 0; k < cnt; ++k)
        {
            const float4 a = rec[2 * k], b = rec[2 * k + 1];
            const float  R = reach[k];
            // wave-uniform: the record's box against the layer z = lz, centre (4, 4, lz + 0.5), half extents 3.5, 3.5, 0
            float gx = a.x - 4.0f, gy = a.y - 4.0f, gz = a.z - fz;
            gx       = fmaf(-p.nf, rintf(gx * p.inf), gx);
            gy       = fmaf(-p.nf, rintf(gy * p.inf), gy);
            gz       = fmaf(-p.nf, rintf(gz * p.inf), gz);
            if (fabsf(gx) > R + 3.5f || fabsf(gy) > R + 3.5f || fabsf(gz) > R) continue;
            // the minimum image of this cell's own distances: any number of periods
            float dx = a.x - fx, dy = a.y - fy;
            dx       = fmaf(-p.nf, rintf(dx * p.inf), dx);
            dy       = fmaf(-p.nf, rintf(dy * p.inf), dy);
            const float r2 = fmaf(dx, dx, fmaf(dy, dy, gz * gz));
            const float kv = kernelWt(r2 * a.w);
            s0             = fmaf(b.x, kv, s0);
            if (NA > 0) s1 = fmaf(b.y, kv, s1);
            if (NA > 1) s2 = fmaf(b.z, kv, s2);
            if (NA > 2) s3 = fmaf(b.w, kv, s3);
        }
    }
    const size_t n3 = (size_t)p.n * p.n * p.n;
    const size_t o  = ((size_t)(bz * kBz + lz) * p.n + (by * kBy + ly)) * p.n + (bx * kBx + lx);
    sum0[o]         = (double)s0;
    if (NA > 0) sum1[o] = (double)s1;
    if (NA > 1) sum1[n3 + o] = (double)s2;
    if (NA > 2) sum1[2 * n3 + o] = (double)s3;
}

/*! W = S0^p Sa / S0 and Sb likewise (imaginary part; Sb null: 0) in double; mode 0: p = 0, 1: p = 1/2, 2: p = 1/3,
 *  3: W = Sa itself (the mesh density).  W = 0 where S0 = 0. */
__global__ __launch_bounds__(256) void fieldKernel(const double* __restrict__ S0, const double* __restrict__ Sa,
                                                   const double* __restrict__ Sb, int mode, size_t n3,
                                                   double2* __restrict__ out)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n3) return;
    const double s = S0[c];
    double       f = 0.0;
    if (mode == 3) f = 1.0;
    else if (s > 0.0) f = mode == 0 ? 1.0 / s : mode == 1 ? 1.0 / sqrt(s) : cbrt(s) / s;
    out[c] = make_double2(Sa[c] * f, Sb ? Sb[c] * f : 0.0);
}

/*! one leaf of the fixed tree: the modes perm[leafBeg[l] .. leafBeg[l + 1]) of one shell.  Lane t adds the squares of
 *  the modes beg + t, beg + t + 256, ... in that order, then the 256 lanes fold pairwise at strides 128 .. 1. */
__global__ __launch_bounds__(256) void leafKernel(const double2* __restrict__ mesh, const uint32_t* __restrict__ perm,
                                                  const uint32_t* __restrict__ leafBeg, double* __restrict__ leafSum)
{
    __shared__ double part[256];
    const uint32_t beg = leafBeg[blockIdx.x], end = leafBeg[blockIdx.x + 1];
    double         s = 0.0;
    for (uint32_t k = beg + threadIdx.x; k < end; k += 256)
    {
        const double2 v = mesh[perm[k]];
        s += fma(v.x, v.x, v.y * v.y);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1)
    {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) leafSum[blockIdx.x] = part[0];
}

//! the leaves of shell s added in ascending order
__global__ void shellKernel(const double* __restrict__ leafSum, const uint32_t* __restrict__ shellLeaf,
                            const uint32_t* __restrict__ shellBeg, uint32_t numShells, double prefactor, int accumulate,
                            double* __restrict__ power, uint64_t* __restrict__ modes)
{
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= numShells) return;
    double sum = 0.0;
    for (uint32_t l = shellLeaf[s]; l < shellLeaf[s + 1]; ++l)
        sum += leafSum[l];
    const double v = prefactor * sum;
    power[s]       = accumulate ? power[s] + v : v;
    if (modes) modes[s] = (uint64_t)(shellBeg[s + 1] - shellBeg[s]);
}

Plan makePlan(const DepositArgs& a)
{
    Plan p{};
    p.n   = (int)a.n;
    p.nbx = p.n / kBx, p.nby = p.n / kBy, p.nbz = p.n / kBz;
    for (int k = 0; k < 3; ++k)
        p.lo[k] = a.box.lim[2 * k];
    p.L    = a.box.lim[1] - a.box.lim[0];
    p.D    = p.L / p.n;
    p.iD   = 1.0 / p.D;
    p.hmin = 0.5 * p.D;
    p.K    = a.K;
    p.nf   = (float)p.n;
    p.inf  = 1.0f / p.nf;
    return p;
}

//! [power | modes] of the largest n, on the device and pinned
bool reserveOut(Arena& arena, SpecBuffers& b)
{
    const uint32_t ns = numShells(kMaxN);
    b.out             = arena.get<double>("spec.out", 2 * ns);
    b.outHost         = arena.pinned<double>("spec.outHost", 2 * ns);
    return b.out && b.outHost;
}

} // namespace

int deposit(Arena& arena, SpecBuffers& b, const DepositArgs& a, hipStream_t s, std::string& err)
{
    if (!validN(a.n))
    {
        err = "sx_mesh_deposit: n must be 16, 32, 64, 128 or 256";
        return SX_ERR_ARG;
    }
    const sx_spectrum probe{SX_SPEC_SCALAR, 0, a.n};
    if (const char* why = checkSpec(&probe, &a.box))
    {
        err = why;
        return SX_ERR_ARG;
    }
    if (a.numA < 0 || a.numA > 3)
    {
        err = "sx_mesh_deposit: numA must be 0 .. 3";
        return SX_ERR_ARG;
    }
    const Plan      p = makePlan(a);
    const Particles q{a.x, a.y, a.z, a.h, a.m, {a.a[0], a.a[1], a.a[2]}, a.numA, a.aIsDouble};
    b.msFft = b.msShells = 0.0f;
    auto gather = [&](const pairbin::Band& bd, const uint64_t* pairs, const uint32_t* offsets, unsigned long long* counts) {
        const uint32_t blocks = (uint32_t)(bd.r1 - bd.r0) * p.nbx * p.nby;
        // a block without pairs reads no particle: last - 1 is never formed for an empty range
        switch (a.numA)
        {
            case 0: gatherKernel<0><<<blocks, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.sum1, counts); break;
            case 1: gatherKernel<1><<<blocks, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.sum1, counts); break;
            case 2: gatherKernel<2><<<blocks, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.sum1, counts); break;
            default: gatherKernel<3><<<blocks, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.sum1, counts); break;
        }
    };
    return pairbin::run(arena, b.bin, kNames, Geom{p, q}, a.first, a.last, gather, s, err);
}

int fft3d(Arena& arena, SpecBuffers& b, double* complexMesh, uint32_t n, hipStream_t s, std::string& err)
{
    if (!validN(n) || !complexMesh)
    {
        err = "sx_fft3d: a mesh and n of 16, 32, 64, 128 or 256";
        return SX_ERR_ARG;
    }
    if ((uintptr_t)complexMesh % 16)
    {
        err = "sx_fft3d: the mesh must be 16-byte aligned";
        return SX_ERR_ARG;
    }
    if (b.twiddleN != n)
    {
        b.twiddle = arena.get<double2>("spec.twiddle", kMaxN);
        if (!b.twiddle)
        {
            err = "sx_fft3d: twiddle table";
            return SX_ERR_NOMEM;
        }
        std::vector<double2> t;
        twiddleTable(n, t);
        SX_TRY_HIP("sx_spectrum", hipStreamSynchronize(s)); // a transform of another n may still read the table
        SX_TRY_HIP("sx_spectrum", hipMemcpy(b.twiddle, t.data(), n * sizeof(double2), hipMemcpyHostToDevice));
        b.twiddleN = n;
    }
    SX_TRY_HIP("sx_spectrum", pairbin::ensureEvents(b.bin));
    if (b.bin.timing) SX_TRY_HIP("sx_spectrum", hipEventRecord(b.bin.ev[0], s));
    SX_TRY_HIP("sx_spectrum", fftLaunch(reinterpret_cast<double2*>(complexMesh), n, b.twiddle, s));
    if (b.bin.timing)
    {
        float ms = 0.0f;
        SX_TRY_HIP("sx_spectrum", hipEventRecord(b.bin.ev[1], s));
        SX_TRY_HIP("sx_spectrum", hipEventSynchronize(b.bin.ev[1]));
        if (hipEventElapsedTime(&ms, b.bin.ev[0], b.bin.ev[1]) == hipSuccess) b.msFft += ms;
    }
    return SX_OK;
}

//! the mode permutation of n, its leaves and the shells' first leaves, on the host, then to the device
static int ensurePerm(Arena& arena, SpecBuffers& b, uint32_t n, hipStream_t s, std::string& err)
{
    if (b.permN == n) return SX_OK;
    const uint32_t ns = numShells(n);
    const size_t   n3 = (size_t)n * n * n;
    const int      h  = (int)n / 2;
    // shell of every cell of the transformed mesh: index i along an axis is the wave number i for i < n / 2, i - n else
    std::vector<uint32_t> sq(n);
    for (uint32_t i = 0; i < n; ++i)
    {
        const int k = (int)i < h ? (int)i : (int)i - (int)n;
        sq[i]       = (uint32_t)(k * k);
    }
    std::vector<uint16_t> shell(n3);
    std::vector<uint32_t> beg(ns + 1, 0);
    for (uint32_t z = 0; z < n; ++z)
        for (uint32_t y = 0; y < n; ++y)
            for (uint32_t x = 0; x < n; ++x)
            {
                const uint32_t sh                    = shellOf(sq[x] + sq[y] + sq[z]);
                shell[((size_t)z * n + y) * n + x] = (uint16_t)sh;
                ++beg[sh + 1];
            }
    for (uint32_t k = 0; k < ns; ++k)
        beg[k + 1] += beg[k];
    // a counting sort by shell: stable, so ascending cell index within a shell
    std::vector<uint32_t> perm(n3), at(beg.begin(), beg.end() - 1);
    for (size_t c = 0; c < n3; ++c)
        perm[at[shell[c]]++] = (uint32_t)c;
    std::vector<uint32_t> leafBeg, shellLeaf(ns + 1);
    for (uint32_t k = 0; k < ns; ++k)
    {
        shellLeaf[k] = (uint32_t)leafBeg.size();
        for (uint32_t m = beg[k]; m < beg[k + 1]; m += kShellChunk)
            leafBeg.push_back(m);
    }
    shellLeaf[ns] = (uint32_t)leafBeg.size();
    leafBeg.push_back((uint32_t)n3);
    // a leaf ends where the next begins; the last leaf of a shell ends at the next shell's first mode (shells are not
    // empty for these n, and an empty one would own no leaf)
    const uint32_t nl = (uint32_t)leafBeg.size() - 1;

    // an arena buffer grows and never shrinks: a smaller n after a larger one keeps the larger buffers
    b.perm      = arena.get<uint32_t>("spec.perm", n3);
    b.leafBeg   = arena.get<uint32_t>("spec.leafBeg", nl + 1);
    b.shellLeaf = arena.get<uint32_t>("spec.shellLeaf", ns + 1);
    b.shellBeg  = arena.get<uint32_t>("spec.shellBeg", ns + 1);
    b.leafSum   = arena.get<double>("spec.leafSum", nl);
    if (!b.perm || !b.leafBeg || !b.shellLeaf || !b.shellBeg || !b.leafSum)
    {
        err = "sx_shell_sums: mode permutation (" + std::to_string(n3 * 4) + " bytes)";
        b.permN = 0;
        return SX_ERR_NOMEM;
    }
    b.permN = 0;
    SX_TRY_HIP("sx_spectrum", hipStreamSynchronize(s));
    SX_TRY_HIP("sx_spectrum", hipMemcpy(b.perm, perm.data(), n3 * 4, hipMemcpyHostToDevice));
    SX_TRY_HIP("sx_spectrum", hipMemcpy(b.leafBeg, leafBeg.data(), leafBeg.size() * 4, hipMemcpyHostToDevice));
    SX_TRY_HIP("sx_spectrum", hipMemcpy(b.shellLeaf, shellLeaf.data(), shellLeaf.size() * 4, hipMemcpyHostToDevice));
    SX_TRY_HIP("sx_spectrum", hipMemcpy(b.shellBeg, beg.data(), beg.size() * 4, hipMemcpyHostToDevice));
    b.numLeaves = nl;
    b.permN     = n;
    return SX_OK;
}

int shellSums(Arena& arena, SpecBuffers& b, const double* complexMesh, uint32_t n, double prefactor, int accumulate,
              double* power, uint64_t* modes, hipStream_t s, std::string& err)
{
    if (!validN(n) || !complexMesh || !power)
    {
        err = "sx_shell_sums: a mesh, power and n of 16, 32, 64, 128 or 256";
        return SX_ERR_ARG;
    }
    if (int rc = ensurePerm(arena, b, n, s, err)) return rc;
    SX_TRY_HIP("sx_spectrum", pairbin::ensureEvents(b.bin));
    const uint32_t ns = numShells(n);
    if (b.bin.timing) SX_TRY_HIP("sx_spectrum", hipEventRecord(b.bin.ev[0], s));
    leafKernel<<<b.numLeaves, 256, 0, s>>>(reinterpret_cast<const double2*>(complexMesh), b.perm, b.leafBeg, b.leafSum);
    shellKernel<<<(ns + 63) / 64, 64, 0, s>>>(b.leafSum, b.shellLeaf, b.shellBeg, ns, prefactor, accumulate, power, modes);
    SX_TRY_HIP("sx_spectrum", hipGetLastError());
    if (b.bin.timing)
    {
        float ms = 0.0f;
        SX_TRY_HIP("sx_spectrum", hipEventRecord(b.bin.ev[1], s));
        SX_TRY_HIP("sx_spectrum", hipEventSynchronize(b.bin.ev[1]));
        if (hipEventElapsedTime(&ms, b.bin.ev[0], b.bin.ev[1]) == hipSuccess) b.msShells += ms;
    }
    return SX_OK;
}

int compute(Arena& arena, SpecBuffers& b, const sx_spectrum& sp, DepositArgs a, double* power, uint64_t* modes,
            const std::function<bool(double*, size_t)>& reduce, hipStream_t s, std::string& err)
{
    if (const char* why = checkSpec(&sp, &a.box))
    {
        err = why;
        return SX_ERR_ARG;
    }
    const uint32_t n  = sp.n;
    const size_t   n3 = (size_t)n * n * n;
    const uint32_t ns = numShells(n);
    // [refusals, 0 | S0 | S1 x 3]: the word in front travels with the meshes through the one reduction
    b.sums = arena.get<double>("spec.sums", 2 + 4 * n3);
    b.cplx = arena.get<double>("spec.cplx", 2 * n3);
    if (!b.sums || !b.cplx || !reserveOut(arena, b))
    {
        err = "sx_spectrum_compute: mesh buffers (" + std::to_string((6 * n3 + 2) * 8) + " bytes)";
        return SX_ERR_NOMEM;
    }
    a.n    = n;
    a.sum0 = b.sums + 2;
    a.sum1 = a.sum0 + n3;
    int rc = deposit(arena, b, a, s, err);
    const size_t count = 2 + (size_t)(1 + a.numA) * n3;
    if (reduce)
    {
        const double lead[2] = {rc != SX_OK ? 1.0 : 0.0, 0.0};
        if (rc != SX_OK) SX_TRY_HIP("sx_spectrum", hipMemsetAsync(b.sums, 0, count * sizeof(double), s));
        SX_TRY_HIP("sx_spectrum", hipMemcpyAsync(b.sums, lead, sizeof(lead), hipMemcpyHostToDevice, s));
        SX_TRY_HIP("sx_spectrum", hipStreamSynchronize(s)); // lead is on this frame
        if (!reduce(b.sums, count))
        {
            if (rc == SX_OK) err = "sx_spectrum_compute: the reduction over the ranks failed";
            return rc != SX_OK ? rc : SX_ERR_HIP;
        }
        SX_TRY_HIP("sx_spectrum", hipMemcpyAsync(b.outHost, b.sums, sizeof(double), hipMemcpyDeviceToHost, s));
        SX_TRY_HIP("sx_spectrum", hipStreamSynchronize(s));
        if (rc == SX_OK && b.outHost[0] != 0.0)
        {
            err = "sx_spectrum_compute: refused on another rank (its sx_last_error has the reason)";
            return SX_ERR_ARG;
        }
    }
    if (rc != SX_OK) return rc;

    double*      pw = power ? power : b.out;
    uint64_t*    md = modes ? modes : reinterpret_cast<uint64_t*>(b.out + ns);
    double2*     cm = reinterpret_cast<double2*>(b.cplx);
    const double *S0 = a.sum0, *S1 = a.sum1;
    const unsigned fblocks = (unsigned)((n3 + 255) / 256);
    if (sp.kind == SX_SPEC_VELOCITY)
    {
        fieldKernel<<<fblocks, 256, 0, s>>>(S0, S1, S1 + n3, sp.weight, n3, cm);
        SX_TRY_HIP("sx_spectrum", hipGetLastError());
        if ((rc = fft3d(arena, b, b.cplx, n, s, err))) return rc;
        if ((rc = shellSums(arena, b, b.cplx, n, 0.5, 0, pw, md, s, err))) return rc;
        fieldKernel<<<fblocks, 256, 0, s>>>(S0, S1 + 2 * n3, nullptr, sp.weight, n3, cm);
        SX_TRY_HIP("sx_spectrum", hipGetLastError());
        if ((rc = fft3d(arena, b, b.cplx, n, s, err))) return rc;
        if ((rc = shellSums(arena, b, b.cplx, n, 0.5, 1, pw, md, s, err))) return rc;
    }
    else
    {
        fieldKernel<<<fblocks, 256, 0, s>>>(S0, a.numA ? S1 : S0, nullptr, a.numA ? 0 : 3, n3, cm);
        SX_TRY_HIP("sx_spectrum", hipGetLastError());
        if ((rc = fft3d(arena, b, b.cplx, n, s, err))) return rc;
        if ((rc = shellSums(arena, b, b.cplx, n, 1.0, 0, pw, md, s, err))) return rc;
    }
    SX_TRY_HIP("sx_spectrum", hipStreamSynchronize(s));
    return SX_OK;
}

} // namespace sx::spectrum
