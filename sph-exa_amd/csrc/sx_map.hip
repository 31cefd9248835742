/*! @file sx_map.hip
 * @brief Column-density and slice maps (sx_map.hpp): footprint binning into 16 x 16-pixel tiles, a radix sort of the
 *        (tile, particle) pairs (both the pair-binning engine's, sx_pairbin.hpp), and one workgroup per tile that
 *        gathers its list through LDS in list order.
 *
 * Geometry.  Pixel (i, j) has its centre at window coordinates (i + 0.5, j + 0.5) in pixel units.  A particle with
 * in-plane reach R (2 he for a column, sqrt(4 h^2 - dn^2) for a slice) touches the pixels whose centres lie within R
 * of one of its images; on a periodic axis the images -L, 0, +L of the minimum-image position about the window centre
 * are looked at, and tiles reached by two of them are emitted once.  The render kernel places a record by the minimum
 * image about its TILE centre, in pixel units relative to the tile origin (small numbers: float keeps them to 2^-24 of
 * the tile's extent plus the reach), and every lane folds its own distance by whole periods (d - L rint(d / L)), as does
 * the per-wave cull, so a pixel sees the minimum-image distance also where the period is shorter than a tile (an image
 * of a few pixels, or of one, along a periodic axis).
 * The kernel value is exactly 0 beyond the support (mapKernelY, kernelWt), so the binning and the per-wave cull may be
 * conservative without changing a bit of the image.
 */
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sx_device.hpp"
#include "sx_kernel_poly.hpp"
#include "sx_map.hpp"

namespace sx::map
{

const char* checkSpec(const sx_map* m, const sx_box* box)
{
    if (!m || !box) return "sx_map_check: null map or box";
    if (m->kind != SX_MAP_COLUMN && m->kind != SX_MAP_SLICE) return "sx_map_check: unknown kind (SX_MAP_COLUMN or SX_MAP_SLICE)";
    if (m->axis < 0 || m->axis > 2) return "sx_map_check: unknown axis (0 x, 1 y, 2 z)";
    for (int k = 0; k < 2; ++k)
    {
        if (m->npix[k] == 0 || m->npix[k] > kMaxPix) return "sx_map_check: npix must be 1..4096";
        if (!(m->width[k] > 0.0) || !std::isfinite(m->width[k])) return "sx_map_check: width must be positive";
        const int    ax = (m->axis + 1 + k) % 3;
        const double L  = box->lim[2 * ax + 1] - box->lim[2 * ax];
        if (box->bnd[ax] == 1 && m->width[k] > L) return "sx_map_check: width exceeds the box length on a periodic axis";
    }
    if (!(m->depth >= 0.0)) return "sx_map_check: depth must not be negative";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(m->center[k])) return "sx_map_check: center must be finite";
    return nullptr;
}

namespace
{

//! the window in the units the kernels use
struct Plan
{
    int    kind, nx, ny, ntx, nty;
    double cu, cv, cn;     // window centre
    double wu, wv;         // half widths
    double du, dv, idu, idv;
    double Lu, Lv, Ln;     // period, 0 on an axis that is not periodic
    double halfDepth;      // column slab, 0 = unbounded
    double hmin;           // column: half the larger pixel size; slice: 0
    double K;
    float  du2, dv2;       // squared pixel sizes
    float  LuPix, LvPix;   // period in pixels (0: none)
    float  iLuPix, iLvPix; // its inverse (0: none, so the fold below is the identity)
};

struct Particles
{
    const double *u, *v, *n; // coordinates along the in-plane axes and the normal
    const float * h, *m;
    const void*   a;
    int           aIsDouble;
};

/*! tile intervals [lo, hi] along one axis, one slot per image -L, 0, +L of f: the pixels whose centres lie within r of
 *  that image (pixel units), less the tiles of an earlier slot; an unused slot is empty (lo > hi).  The slots are walked
 *  by unrolled loops, so a Span lives in registers. */
struct Span
{
    int lo[3]{0, 0, 0}, hi[3]{-1, -1, -1};
};

__device__ inline void tileSpan(double f, double r, double Lpix, int npix, Span& s)
{
    int prev = -1;
#pragma unroll
    for (int k = -1; k <= 1; ++k)
    {
        if (k != 0 && !(Lpix > 0.0)) continue;
        const double c  = f + k * Lpix;
        const double lo = fmax(ceil(c - r - 0.5 - 1e-6), 0.0), hi = fmin(floor(c + r - 0.5 + 1e-6), (double)(npix - 1));
        if (!(lo <= hi)) continue;
        const int tlo = std::max((int)lo / kTile, prev + 1), thi = (int)hi / kTile;
        if (tlo > thi) continue;
        s.lo[k + 1] = tlo, s.hi[k + 1] = thi;
        prev = thi;
    }
}

//! reach of particle i in the window: false when it has none; fu, fv = position in pixel units from the window's corner
__device__ inline bool reach(const Plan& p, const Particles& q, uint32_t i, double& fu, double& fv, double& R)
{
    double dn = q.n[i] - p.cn;
    if (p.Ln > 0.0) dn -= p.Ln * rint(dn / p.Ln);
    const double h = (double)q.h[i];
    if (p.kind == SX_MAP_COLUMN)
    {
        if (p.halfDepth > 0.0 && fabs(dn) > p.halfDepth) return false;
        R = 2.0 * fmax(h, p.hmin);
    }
    else
    {
        const double r2 = 4.0 * h * h - dn * dn;
        if (!(r2 > 0.0)) return false;
        R = sqrt(r2);
    }
    double d = q.u[i] - p.cu, e = q.v[i] - p.cv;
    if (p.Lu > 0.0) d -= p.Lu * rint(d / p.Lu);
    if (p.Lv > 0.0) e -= p.Lv * rint(e / p.Lv);
    fu = (d + p.wu) * p.idu;
    fv = (e + p.wv) * p.idv;
    return true;
}

__device__ inline int spanTiles(const Span& s)
{
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        n += std::max(s.hi[k] - s.lo[k] + 1, 0);
    return n;
}

/*! the engine's geometry (sx_pairbin.hpp): rows are tile rows, units the tiles of one; counts[0] tallies the particles
 *  with a footprint in the window */
struct Geom
{
    static constexpr int kMaxRows = kMaxPix / kTile;
    struct Foot
    {
        Span su, sv;
    };
    Plan      p;
    Particles q;

    __host__ __device__ int      rows() const { return p.nty; }
    __host__ __device__ uint32_t unitsPerRow() const { return (uint32_t)p.ntx; }

    __device__ void foot(uint32_t i, Foot& ft) const
    {
        double fu, fv, R;
        if (!reach(p, q, i, fu, fv, R)) return;
        tileSpan(fu, R * p.idu, p.Lu * p.idu, p.nx, ft.su);
        tileSpan(fv, R * p.idv, p.Lv * p.idv, p.ny, ft.sv);
    }
    __device__ bool counted(const Foot& ft) const { return spanTiles(ft.su) && spanTiles(ft.sv); }
    template<class F>
    __device__ void forRows(const Foot& ft, F&& f) const
    {
        const uint32_t nu = (uint32_t)spanTiles(ft.su);
        if (!nu) return;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int ty = ft.sv.lo[k]; ty <= ft.sv.hi[k]; ++ty)
                f(ty, nu);
    }
    template<class F>
    __device__ void forUnits(const Foot& ft, int, F&& f) const
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int tx = ft.su.lo[k]; tx <= ft.su.hi[k]; ++tx)
                f((uint32_t)tx);
    }
};

/*! one workgroup per tile, one pixel per lane (lane t: pixel (t & 15, t >> 4) of the tile, so wave w owns the 16 x 4
 *  block of rows 4w .. 4w + 3).  The tile's list is staged through LDS kChunk records at a time, each lane building one
 *  record in double from the particle's fields; then every lane walks the chunk in list order.  The record address is
 *  the same in all lanes (an LDS broadcast read of 2 x 16 bytes), and the test of the record's box against the wave's
 *  block is wave-uniform, so a wave skips the records that cannot reach it without divergence.
 *  Record: {u, v relative to the tile origin in pixels, 1 / he^2, w} {w a, dn^2 / h^2 (slice), reach in pixels along u, v}.
 */
template<bool Slice>
__global__ __launch_bounds__(256) void renderKernel(Plan p, Particles q, const uint64_t* __restrict__ pairs,
                                                    const uint32_t* __restrict__ offsets, int r0, uint32_t last,
                                                    double* __restrict__ sum0, double* __restrict__ sum1,
                                                    unsigned long long* counts)
{
    __shared__ float4 rec[2 * kChunk];
    const int      t    = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int      tx = tile % p.ntx, ty = r0 + tile / p.ntx;
    const uint32_t beg = offsets[tile], end = offsets[tile + 1];
    if (t == 0 && end > beg) atomicMax(&counts[1], (unsigned long long)(end - beg));

    const float fx = (float)(t & 15) + 0.5f, fy = (float)(t >> 4) + 0.5f;
    const float cy = (float)(4 * (t >> 6)) + 2.0f; // centre of the wave's block along v (along u: the tile's, 8)
    // tile centre relative to the window centre
    const double tcu = (tx * kTile + kTile / 2) * p.du - p.wu, tcv = (ty * kTile + kTile / 2) * p.dv - p.wv;

    float s0 = 0.0f, s1 = 0.0f;
    for (uint32_t c0 = beg; c0 < end; c0 += kChunk)
    {
        const uint32_t cnt = std::min(kChunk, end - c0);
        __syncthreads(); // the previous chunk has been walked
        if ((uint32_t)t < cnt)
        {
            // every sorted key was written by emitKernel; the clamp keeps the gathers in bounds if one was not
            const uint32_t i  = std::min((uint32_t)pairs[c0 + t], last - 1);
            double         d  = q.u[i] - p.cu - tcu, e = q.v[i] - p.cv - tcv, dn = q.n[i] - p.cn;
            if (p.Lu > 0.0) d -= p.Lu * rint(d / p.Lu);
            if (p.Lv > 0.0) e -= p.Lv * rint(e / p.Lv);
            if (p.Ln > 0.0) dn -= p.Ln * rint(dn / p.Ln);
            const double h  = (double)q.h[i];
            const double he = Slice ? h : fmax(h, p.hmin);
            const double ih2 = 1.0 / (he * he);
            const double w   = Slice ? (double)q.m[i] * p.K * ih2 / he : (double)q.m[i] * p.K * ih2;
            const double R   = Slice ? sqrt(fmax(4.0 * h * h - dn * dn, 0.0)) : 2.0 * he;
            const float  wf  = (float)w;
            float        af  = 0.0f;
            if (q.a) af = q.aIsDouble ? (float)((const double*)q.a)[i] : ((const float*)q.a)[i];
            rec[2 * t]     = make_float4((float)(d * p.idu + kTile / 2), (float)(e * p.idv + kTile / 2), (float)ih2, wf);
            // the reach with a margin that covers the rounding of the float distances it is compared with
            rec[2 * t + 1] = make_float4(wf * af, Slice ? (float)(dn * dn * ih2) : 0.0f,
                                         (float)(R * p.idu) * 1.0001f + 1e-3f, (float)(R * p.idv) * 1.0001f + 1e-3f);
        }
        __syncthreads();
        for (uint32_t k = 0; k < cnt; ++k)
        {
            const float4 a = rec[2 * k], b = rec[2 * k + 1];
            float        gy = a.y - cy;
            gy              = fmaf(-p.LvPix, rintf(gy * p.iLvPix), gy);
            if (fabsf(a.x - 8.0f) > b.z + 7.5f || fabsf(gy) > b.w + 1.5f) continue; // wave-uniform
            float dx = a.x - fx, dy = a.y - fy;
            // the minimum image of this pixel's own distance: any number of periods, an image may be narrower than a tile
            dx       = fmaf(-p.LuPix, rintf(dx * p.iLuPix), dx);
            dy       = fmaf(-p.LvPix, rintf(dy * p.iLvPix), dy);
            const float r2 = fmaf(dx * dx, p.du2, dy * dy * p.dv2);
            const float kv = Slice ? kernelWt(fmaf(r2, a.z, b.y)) : mapKernelY(r2 * a.z);
            s0             = fmaf(a.w, kv, s0);
            s1             = fmaf(b.x, kv, s1);
        }
    }
    const int i = tx * kTile + (t & 15), j = ty * kTile + (t >> 4);
    if (i < p.nx && j < p.ny)
    {
        const size_t o = (size_t)j * p.nx + i;
        sum0[o]        = (double)s0;
        if (sum1) sum1[o] = (double)s1;
    }
}

Plan makePlan(const Args& a)
{
    const sx_map& m  = a.spec;
    const int     au = (m.axis + 1) % 3, av = (m.axis + 2) % 3, an = m.axis;
    auto          L  = [&](int ax) { return a.box.bnd[ax] == 1 ? a.box.lim[2 * ax + 1] - a.box.lim[2 * ax] : 0.0; };
    Plan          p{};
    p.kind = m.kind, p.nx = (int)m.npix[0], p.ny = (int)m.npix[1];
    p.ntx = (p.nx + kTile - 1) / kTile, p.nty = (p.ny + kTile - 1) / kTile;
    p.cu = m.center[au], p.cv = m.center[av], p.cn = m.center[an];
    p.wu = 0.5 * m.width[0], p.wv = 0.5 * m.width[1];
    p.du = m.width[0] / p.nx, p.dv = m.width[1] / p.ny;
    p.idu = 1.0 / p.du, p.idv = 1.0 / p.dv;
    p.Lu = L(au), p.Lv = L(av), p.Ln = L(an);
    p.halfDepth = m.kind == SX_MAP_COLUMN ? 0.5 * m.depth : 0.0;
    p.hmin      = m.kind == SX_MAP_COLUMN ? 0.5 * std::max(p.du, p.dv) : 0.0;
    p.K         = a.K;
    p.du2 = (float)(p.du * p.du), p.dv2 = (float)(p.dv * p.dv);
    p.LuPix = (float)(p.Lu * p.idu), p.LvPix = (float)(p.Lv * p.idv);
    p.iLuPix = p.Lu > 0.0 ? 1.0f / p.LuPix : 0.0f;
    p.iLvPix = p.Lv > 0.0 ? 1.0f / p.LvPix : 0.0f;
    return p;
}

} // namespace

int render(Arena& arena, MapBuffers& b, const Args& a, hipStream_t s, std::string& err)
{
    if (const char* why = checkSpec(&a.spec, &a.box))
    {
        err = why;
        return SX_ERR_ARG;
    }
    const Plan      p = makePlan(a);
    const double*   xyz[3] = {a.x, a.y, a.z};
    const Particles q{xyz[(a.spec.axis + 1) % 3], xyz[(a.spec.axis + 2) % 3], xyz[a.spec.axis], a.h, a.m, a.a, a.aIsDouble};
    auto gather = [&](const pairbin::Band& bd, const uint64_t* pairs, const uint32_t* offsets, unsigned long long* counts) {
        const uint32_t tiles = (uint32_t)(bd.r1 - bd.r0) * p.ntx;
        if (p.kind == SX_MAP_SLICE)
            renderKernel<true><<<tiles, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.a ? a.sum1 : nullptr, counts);
        else
            renderKernel<false><<<tiles, 256, 0, s>>>(p, q, pairs, offsets, bd.r0, a.last, a.sum0, a.a ? a.sum1 : nullptr, counts);
    };
    return pairbin::run(arena, b.bin, kNames, Geom{p, q}, a.first, a.last, gather, s, err);
}

} // namespace sx::map
