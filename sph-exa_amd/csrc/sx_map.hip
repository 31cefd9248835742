/*! @file sx_map.hip
 * @brief Column-density and slice maps (sx_map.hpp): footprint binning into 16 x 16-pixel tiles, a radix sort of the
 *        (tile, particle) pairs, and one workgroup per tile that gathers its list through LDS in list order.
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
#include <hipcub/hipcub.hpp>

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

//! tile intervals [lo, hi] along one axis: the pixels whose centres lie within r of an image of f (pixel units)
struct Span
{
    int lo[3], hi[3], n;
};

__device__ inline void tileSpan(double f, double r, double Lpix, int npix, Span& s)
{
    s.n            = 0;
    int       prev = -1;
    const int k0 = Lpix > 0.0 ? -1 : 0, k1 = Lpix > 0.0 ? 1 : 0;
    for (int k = k0; k <= k1; ++k)
    {
        const double c  = f + k * Lpix;
        const double lo = fmax(ceil(c - r - 0.5 - 1e-6), 0.0), hi = fmin(floor(c + r - 0.5 + 1e-6), (double)(npix - 1));
        if (!(lo <= hi)) continue;
        const int tlo = std::max((int)lo / kTile, prev + 1), thi = (int)hi / kTile;
        if (tlo > thi) continue;
        s.lo[s.n] = tlo, s.hi[s.n] = thi, ++s.n;
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
    for (int k = 0; k < s.n; ++k)
        n += s.hi[k] - s.lo[k] + 1;
    return n;
}

/*! counts[0] += particles with a footprint, counts[2 + ty] += pairs of tile row ty.  Integer atomics: the same totals
 *  on every run. */
__global__ __launch_bounds__(256) void countKernel(Plan p, Particles q, uint32_t first, uint32_t last,
                                                   unsigned long long* counts)
{
    __shared__ uint32_t rows[kMaxPix / kTile];
    __shared__ uint32_t feet;
    for (int k = threadIdx.x; k < p.nty; k += 256)
        rows[k] = 0;
    if (threadIdx.x == 0) feet = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < last)
    {
        double fu, fv, R;
        if (reach(p, q, (uint32_t)i, fu, fv, R))
        {
            Span su, sv;
            tileSpan(fu, R * p.idu, p.Lu * p.idu, p.nx, su);
            tileSpan(fv, R * p.idv, p.Lv * p.idv, p.ny, sv);
            const uint32_t nu = (uint32_t)spanTiles(su);
            if (nu && sv.n)
            {
                atomicAdd(&feet, 1u);
                for (int k = 0; k < sv.n; ++k)
                    for (int ty = sv.lo[k]; ty <= sv.hi[k]; ++ty)
                        atomicAdd(&rows[ty], nu);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < p.nty; k += 256)
        if (rows[k]) atomicAdd(&counts[2 + k], (unsigned long long)rows[k]);
    if (threadIdx.x == 0 && feet) atomicAdd(&counts[0], (unsigned long long)feet);
}

/*! the pairs of tile rows [r0, r1): (band-local tile) << 32 | particle, at positions taken from a cursor (one atomic
 *  per wave).  The positions differ from run to run, the set of keys does not, and the keys are distinct. */
__global__ __launch_bounds__(256) void emitKernel(Plan p, Particles q, uint32_t first, uint32_t last, int r0, int r1,
                                                  uint32_t* cursor, uint64_t* pairs, uint32_t capacity)
{
    const uint64_t i    = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int      lane = threadIdx.x & 63;
    Span           su, sv;
    su.n = sv.n = 0;
    uint32_t n  = 0;
    if (i < last)
    {
        double fu, fv, R;
        if (reach(p, q, (uint32_t)i, fu, fv, R))
        {
            tileSpan(fu, R * p.idu, p.Lu * p.idu, p.nx, su);
            tileSpan(fv, R * p.idv, p.Lv * p.idv, p.ny, sv);
            uint32_t rowsIn = 0;
            for (int k = 0; k < sv.n; ++k)
            {
                sv.lo[k] = std::max(sv.lo[k], r0);
                sv.hi[k] = std::min(sv.hi[k], r1 - 1);
                if (sv.lo[k] <= sv.hi[k]) rowsIn += sv.hi[k] - sv.lo[k] + 1;
            }
            n = rowsIn * (uint32_t)spanTiles(su);
        }
    }
    // exclusive scan of n over the wave, one atomic for its total (every lane takes part)
    uint32_t incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    if (total == 0) return; // wave-uniform
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(cursor, total);
    base         = __shfl(base, 63, 64);
    uint32_t pos = base + incl - n;
    if (n == 0) return;
    for (int kv = 0; kv < sv.n; ++kv)
        for (int ty = sv.lo[kv]; ty <= sv.hi[kv]; ++ty)
            for (int ku = 0; ku < su.n; ++ku)
                for (int tx = su.lo[ku]; tx <= su.hi[ku]; ++tx)
                {
                    // the count pass sized the buffer from the same arithmetic; the guard keeps a disagreement in bounds
                    if (pos < capacity) pairs[pos] = ((uint64_t)((ty - r0) * p.ntx + tx) << 32) | (uint64_t)i;
                    ++pos;
                }
}

//! offsets[t] = first sorted pair of band-local tile t, t in [0, tiles]; *mismatch counts the bands in which the emit
//! pass wrote another number of pairs than the count pass announced (the buffer was filled with keys beyond every tile
//! before, so such a band loses pairs but reads no stale one; sx_map_stats reports it)
__global__ void offsetsKernel(const uint64_t* sorted, uint32_t num, uint32_t tiles, uint32_t* offsets,
                              const uint32_t* cursor, unsigned long long* mismatch)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0 && *cursor != num) atomicAdd(mismatch, 1ull);
    if (t > tiles) return;
    const uint64_t key = (uint64_t)t << 32;
    uint32_t       lo = 0, hi = num;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    offsets[t] = lo;
}

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

#define MAP_HIP(call)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
        {                                                                                                              \
            err = std::string("sx_map_render: " #call ": ") + hipGetErrorString(e_);                                   \
            return SX_ERR_HIP;                                                                                         \
        }                                                                                                              \
    } while (0)

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
    const uint32_t  np = a.last - a.first;
    const unsigned  pblocks = (np + 255) / 256;
    constexpr int   kRows = kMaxPix / kTile;

    b.counts     = arena.get<unsigned long long>("map.counts", 3 + kRows);
    b.countsHost = arena.pinned<unsigned long long>("map.countsHost", 3 + kRows);
    if (!b.counts || !b.countsHost)
    {
        err = "sx_map_render: counters";
        return SX_ERR_NOMEM;
    }
    if (b.timing)
        for (auto& e : b.ev)
            if (!e) MAP_HIP(hipEventCreate(&e));
    b.ms[0] = b.ms[1] = b.ms[2] = 0.0f;
    float ms = 0.0f;

    // pairs per tile row
    if (b.timing) MAP_HIP(hipEventRecord(b.ev[0], s));
    MAP_HIP(hipMemsetAsync(b.counts, 0, (3 + kRows) * sizeof(unsigned long long), s));
    if (np) countKernel<<<pblocks, 256, 0, s>>>(p, q, a.first, a.last, b.counts);
    MAP_HIP(hipGetLastError());
    if (b.timing) MAP_HIP(hipEventRecord(b.ev[1], s));
    MAP_HIP(hipMemcpyAsync(b.countsHost, b.counts, (2 + p.nty) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    MAP_HIP(hipStreamSynchronize(s));
    if (b.timing && hipEventElapsedTime(&ms, b.ev[0], b.ev[1]) == hipSuccess) b.ms[0] += ms;

    // bands of whole tile rows within the cap
    const uint64_t cap = std::min(b.pairCap ? b.pairCap : kDefaultPairCap, kMaxBandPairs);
    struct Band
    {
        int      r0, r1;
        uint64_t pairs;
    };
    std::vector<Band> bands;
    uint64_t          total = 0, largest = 0;
    for (int r = 0; r < p.nty; ++r)
    {
        const uint64_t c = b.countsHost[2 + r];
        if (c > kMaxBandPairs)
        {
            err = "sx_map_render: one tile row holds more than 2^31 - 1 pairs (render a smaller window or fewer particles at a time)";
            return SX_ERR_ARG;
        }
        if (c > cap)
        {
            err = "sx_map_render: one tile row holds " + std::to_string(c) + " pairs, more than the pair cap of " +
                  std::to_string(cap) + " (sx_set_map_pair_cap)";
            return SX_ERR_ARG;
        }
        if (bands.empty() || bands.back().pairs + c > cap) bands.push_back(Band{r, r + 1, c});
        else bands.back().r1 = r + 1, bands.back().pairs += c;
        total += c;
    }
    for (const Band& bd : bands)
        largest = std::max(largest, bd.pairs);

    int tileBits = 1;
    while ((1u << tileBits) < (unsigned)(p.ntx * p.nty) + 1u)
        ++tileBits;
    size_t tmpBytes = 0;
    if (largest)
        MAP_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmpBytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)largest,
                                                  0, 32 + tileBits, s));
    b.pairsIn  = arena.get<uint64_t>("map.pairsIn", largest);
    b.pairsOut = arena.get<uint64_t>("map.pairsOut", largest);
    b.sortTmp  = arena.get<char>("map.sortTmp", tmpBytes);
    b.offsets  = arena.get<uint32_t>("map.offsets", (size_t)p.ntx * p.nty + 1);
    b.cursor   = arena.get<uint32_t>("map.cursor", 1);
    if (!b.pairsIn || !b.pairsOut || !b.sortTmp || !b.offsets || !b.cursor)
    {
        err = "sx_map_render: pair scratch (" + std::to_string(2 * largest * 8 + tmpBytes) + " bytes)";
        return SX_ERR_NOMEM;
    }
    b.scratchBytes = 2 * largest * 8 + tmpBytes + ((size_t)p.ntx * p.nty + 2) * 4 + (2 + kRows) * 8;

    for (const Band& bd : bands)
    {
        const uint32_t tiles = (uint32_t)(bd.r1 - bd.r0) * p.ntx;
        const uint32_t num   = (uint32_t)bd.pairs;
        if (b.timing) MAP_HIP(hipEventRecord(b.ev[0], s));
        MAP_HIP(hipMemsetAsync(b.cursor, 0, 4, s));
        if (num)
        {
            // keys beyond every tile: a slot the emit pass should leave unwritten sorts behind the last list
            MAP_HIP(hipMemsetAsync(b.pairsIn, 0xff, (size_t)num * sizeof(uint64_t), s));
            emitKernel<<<pblocks, 256, 0, s>>>(p, q, a.first, a.last, bd.r0, bd.r1, b.cursor, b.pairsIn, num);
            MAP_HIP(hipGetLastError());
        }
        if (b.timing) MAP_HIP(hipEventRecord(b.ev[1], s));
        if (num)
            MAP_HIP(hipcub::DeviceRadixSort::SortKeys(b.sortTmp, tmpBytes, (const uint64_t*)b.pairsIn, b.pairsOut, (int)num, 0,
                                                      32 + tileBits, s));
        offsetsKernel<<<(tiles + 1 + 255) / 256, 256, 0, s>>>(b.pairsOut, num, tiles, b.offsets, b.cursor, b.counts + 2 + kRows);
        MAP_HIP(hipGetLastError());
        if (b.timing) MAP_HIP(hipEventRecord(b.ev[2], s));
        if (p.kind == SX_MAP_SLICE)
            renderKernel<true><<<tiles, 256, 0, s>>>(p, q, b.pairsOut, b.offsets, bd.r0, a.last, a.sum0, a.a ? a.sum1 : nullptr, b.counts);
        else
            renderKernel<false><<<tiles, 256, 0, s>>>(p, q, b.pairsOut, b.offsets, bd.r0, a.last, a.sum0, a.a ? a.sum1 : nullptr, b.counts);
        MAP_HIP(hipGetLastError());
        if (b.timing)
        {
            MAP_HIP(hipEventRecord(b.ev[3], s));
            MAP_HIP(hipEventSynchronize(b.ev[3]));
            for (int k = 0; k < 3; ++k)
                if (hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]) == hipSuccess) b.ms[k] += ms;
        }
    }
    b.pairs    = total;
    b.bands    = bands.size();
    b.rendered = true;
    return SX_OK;
}

int stats(MapBuffers& b, hipStream_t s, uint64_t out[4])
{
    if (!b.rendered) return SX_ERR_ARG;
    constexpr int kRows = kMaxPix / kTile;
    if (hipMemcpyAsync(b.countsHost, b.counts, (3 + kRows) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SX_ERR_HIP;
    if (b.countsHost[2 + kRows]) return kStatsMismatch;
    out[0] = b.pairs, out[1] = b.bands, out[2] = b.countsHost[1], out[3] = b.countsHost[0];
    return SX_OK;
}

void release(MapBuffers& b)
{
    for (auto& e : b.ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
}

} // namespace sx::map
