/*! @file sx_halo.hip
 * @brief Group properties: the central moments of every catalogue group and its gravitational self-energy by a
 *        segmented all-pairs kernel over the members (sx_halo.hpp).  The search and the density cut are sx_fof.hip's.
 */
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sx_device.hpp"
#include "sx_halo.hpp"

namespace sx::halo
{

// ---- host decisions ---------------------------------------------------------------------------------------------

std::string checkSpec(const sx_halo* p, const sx_box* box)
{
    if (!p || !box) return "sx_halo_check: null specification or box";
    const sx_fof fs = fofOf(*p);
    if (std::string why = fof::checkSpec(&fs, box); !why.empty()) return why;
    char buf[256];
    if (!std::isfinite(p->rhoMin))
    {
        std::snprintf(buf, sizeof buf, "sx_halo_check: rhoMin must be finite (got %g); <= 0 means no cut", p->rhoMin);
        return buf;
    }
    if (!std::isfinite(p->G))
    {
        std::snprintf(buf, sizeof buf, "sx_halo_check: G must be finite (got %g)", (double)p->G);
        return buf;
    }
    if (p->flags & ~kAllFlags)
    {
        std::snprintf(buf, sizeof buf, "sx_halo_check: unknown flags 0x%x (known: 0x%x)", p->flags & ~kAllFlags, kAllFlags);
        return buf;
    }
    if (p->flags & SX_HALO_THERMAL)
    {
        if (!std::isfinite(p->gamma) || !(p->gamma > 1.0))
        {
            std::snprintf(buf, sizeof buf, "sx_halo_check: the thermal energy needs a finite gamma > 1 (got %g)", p->gamma);
            return buf;
        }
        if (!std::isfinite(p->muiConst) || !(p->muiConst > 0.0f))
        {
            std::snprintf(buf, sizeof buf, "sx_halo_check: the thermal energy needs a finite muiConst > 0 (got %g)",
                          (double)p->muiConst);
            return buf;
        }
    }
    return {};
}

std::string whyRefused(const sx_halo* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_halo_result* res)
{
    if (std::string why = checkSpec(p, box); !why.empty()) return why;
    if (!f || !res) return "sx_halo: null fields or result";
    const sx_fof        fs = fofOf(*p);
    const sx_fof_result fr = fofOf(*res);
    if (std::string why = fof::whyRefused(&fs, box, f, first, last, &fr); !why.empty()) return why;
    if (p->rhoMin > 0.0)
    {
        if (p->std && !f->rho) return "sx_halo: the density cut needs the rho column";
        if (!p->std && (!f->kx || !f->xm || !f->m))
            return "sx_halo: the density cut needs kx, xm and m, which this layout does not keep";
    }
    const bool mom = (p->flags & SX_HALO_MOMENTS) && (res->groupSigma || res->groupShape || res->groupAngmom || res->groupRmax);
    const bool thm = (p->flags & SX_HALO_THERMAL) && res->groupEint;
    const bool pot = (p->flags & SX_HALO_POTENTIAL) && res->groupEpot;
    if ((mom || thm || pot) && p->maxGroups == 0)
        return "sx_halo: maxGroups is 0 with a catalogue array set (capacity 0 for a catalogue that was asked for)";
    if ((mom || thm || pot) && (!f->m || !f->vx || !f->vy || !f->vz))
        return "sx_halo: the group properties need m, vx, vy and vz";
    if (thm && !f->temp) return "sx_halo: the thermal energy needs temp, which this layout does not keep";
    if (pot && !f->h) return "sx_halo: the potential needs h";
    return {};
}

// ---- kernels -----------------------------------------------------------------------------------------------------

namespace
{

using cellgrid::Grid;
using cellgrid::minImage;

constexpr const char* kWho = "sx_halo";

//! sum of part[0 .. 255] by the catalogue's pairwise tree, in part[0]; every thread of the workgroup arrives
__device__ __forceinline__ void treeSum(double* part, uint32_t t)
{
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1)
    {
        if (t < (uint32_t)w) part[t] += part[t + w];
        __syncthreads();
    }
}

struct MomentArgs
{
    const uint32_t *memSorted, *segStart, *outCount, *order;
    const double *  xs, *ys, *zs;
    const float *   m, *vx, *vy, *vz;
    const double*   temp;
    uint32_t        first, G;
    Grid            g;
    const double*   outReal; // [mass G | com 3 G | vel 3 G]
    double          cv;
    int             moments, thermal;
    double*         out; // HaloBuffers::out
};

/*! one workgroup per catalogue group.  Thread t adds the terms of the members t, t + 256, ... of the (id-ordered)
 *  segment in turn, then each of the 16 series is added by the pairwise tree: the catalogue's order. */
__global__ __launch_bounds__(kBlock) void momentKernel(MomentArgs a)
{
    __shared__ double part[kBlock];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const size_t   G = a.G;
    const uint32_t start = a.segStart[g], cnt = a.outCount[g];
    const double   M = a.outReal[g];
    const double   X[3] = {a.outReal[G + 3 * (size_t)g], a.outReal[G + 3 * (size_t)g + 1], a.outReal[G + 3 * (size_t)g + 2]};
    const double   V[3] = {a.outReal[4 * G + 3 * (size_t)g], a.outReal[4 * G + 3 * (size_t)g + 1],
                           a.outReal[4 * G + 3 * (size_t)g + 2]};
    double sum[16], r2max = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q)
        sum[q] = 0.0;
    for (uint32_t k = t; k < cnt; k += kBlock)
    {
        const uint32_t s  = a.memSorted[start + k];
        const size_t   p  = (size_t)a.first + a.order[s];
        const double   mk = (double)a.m[p];
        if (a.moments)
        {
            const double dx = minImage(a.xs[s] - X[0], a.g.pbc[0], a.g.half[0], a.g.len[0]);
            const double dy = minImage(a.ys[s] - X[1], a.g.pbc[1], a.g.half[1], a.g.len[1]);
            const double dz = minImage(a.zs[s] - X[2], a.g.pbc[2], a.g.half[2], a.g.len[2]);
            const double wx = (double)a.vx[p] - V[0], wy = (double)a.vy[p] - V[1], wz = (double)a.vz[p] - V[2];
            const double mwx = mk * wx, mwy = mk * wy, mwz = mk * wz;
            const double mdx = mk * dx, mdy = mk * dy, mdz = mk * dz;
            sum[0] += mwx * wx, sum[1] += mwx * wy, sum[2] += mwx * wz;
            sum[3] += mwy * wy, sum[4] += mwy * wz, sum[5] += mwz * wz;
            sum[6] += mdx * dx, sum[7] += mdx * dy, sum[8] += mdx * dz;
            sum[9] += mdy * dy, sum[10] += mdy * dz, sum[11] += mdz * dz;
            sum[12] += mk * ((dy * wz) - (dz * wy));
            sum[13] += mk * ((dz * wx) - (dx * wz));
            sum[14] += mk * ((dx * wy) - (dy * wx));
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            r2max           = r2 > r2max ? r2 : r2max;
        }
        if (a.thermal) sum[15] += mk * (a.cv * a.temp[p]);
    }
    double* sigma = a.out + 6 * (size_t)g;
    double* shape = a.out + 6 * G + 6 * (size_t)g;
    double* ang   = a.out + 12 * G + 3 * (size_t)g;
#pragma unroll
    for (int q = 0; q < 16; ++q)
    {
        if (q < 15 ? !a.moments : !a.thermal) continue; // uniform
        part[t] = sum[q];
        treeSum(part, t);
        if (t == 0)
        {
            const double v = part[0];
            if (q < 6) sigma[q] = v / M;
            else if (q < 12) shape[q - 6] = v / M;
            else if (q < 15) ang[q - 12] = v;
            else a.out[16 * G + g] = v;
        }
        __syncthreads();
    }
    if (a.moments)
    {
        part[t] = r2max;
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1)
        {
            if (t < (uint32_t)w) part[t] = part[t + w] > part[t] ? part[t + w] : part[t];
            __syncthreads();
        }
        if (t == 0) a.out[15 * G + g] = sqrt(part[0]);
    }
}

//! tiles of a group of c members and the work items of its tile pairs a <= b
__host__ __device__ __forceinline__ uint64_t tilesOf(uint32_t c) { return ((uint64_t)c + kTile - 1) / kTile; }

//! items[g] for g < G (0 for a group over the cap) and items[G] = 0, so that the exclusive sum ends with the total
__global__ __launch_bounds__(kBlock) void itemKernel(const uint32_t* __restrict__ outCount, uint32_t G, uint32_t cap,
                                                     uint64_t* __restrict__ items)
{
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g > G) return;
    uint64_t v = 0;
    if (g < G && outCount[g] <= cap)
    {
        const uint64_t T = tilesOf(outCount[g]);
        v                = T * (T + 1) / 2;
    }
    items[g] = v;
}

struct __attribute__((aligned(16))) Src
{
    double x, y, z;
    float  m, h;
};

struct PairArgs
{
    const uint32_t *memSorted, *segStart, *outCount, *order;
    const double *  xs, *ys, *zs;
    const float *   m, *h;
    uint32_t        first, G;
    double          half[3], len[3]; // of the box; half = +inf on an axis that is not periodic
    const uint64_t* itemStart; // G + 1
    uint64_t        itemBase;  // of this launch
    double*         partial;
    unsigned long long* counters;
};

/*! one workgroup of 256 lanes per work item.  The item's group is found by bisection in the exclusive sum of the item
 *  counts, its tile pair a <= b by the triangular root of its index in the group.  A lane holds one target of tile a;
 *  tile b's {x, y, z, m, h} are staged once in LDS (8 KB) and read at one address by the whole wave.  The diagonal item
 *  takes the sources behind the target only.  A term: the differences in double (minimum image), rounded to float once;
 *  r^2, h_i + h_j, r_eff^2, the hardware's reciprocal square root and m_j r^2 / r_eff^3 in float; source s is added to
 *  the lane's accumulator s % 4 (at most 64 terms each).  The four go on in double: times m_i, then the pairwise tree
 *  over the lanes.  One partial per item, no atomics on floating-point data. */
template<bool Pbc>
__device__ __forceinline__ double image(double d, double half, double len)
{
    if constexpr (Pbc)
    {
        // cellgrid::minImage without a branch: d - len < -half would need d < half
        d = d > half ? d - len : d;
        d = d < -half ? d + len : d;
    }
    return d;
}

//! Pbc false: no axis is periodic and the loop carries no minimum image at all
template<bool Pbc>
__global__ __launch_bounds__(kBlock) void pairKernel(PairArgs a)
{
    __shared__ Src    src[kTile];
    __shared__ double part[kBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t w = a.itemBase + blockIdx.x;
    // the last g with itemStart[g] <= w: groups without items (over the cap) have itemStart[g] == itemStart[g + 1]
    uint32_t lo = 0, hi = a.G; // itemStart[lo] <= w < itemStart[hi]
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.itemStart[mid] <= w) lo = mid;
        else hi = mid;
    }
    const uint32_t g     = lo;
    const uint64_t local = w - a.itemStart[g];
    uint64_t       tb    = (uint64_t)((sqrt(8.0 * (double)local + 1.0) - 1.0) * 0.5);
    while (tb * (tb + 1) / 2 > local)
        --tb;
    while ((tb + 1) * (tb + 2) / 2 <= local)
        ++tb;
    const uint32_t ta    = (uint32_t)(local - tb * (tb + 1) / 2);
    const uint32_t start = a.segStart[g], c = a.outCount[g];
    const uint32_t i0 = ta * kTile, j0 = (uint32_t)tb * kTile;
    const uint32_t cntA = min(kTile, c - i0), cntB = min(kTile, c - j0);
    const bool     diag = ta == (uint32_t)tb;

    // stage tile b; the entries behind cntB up to the next multiple of 4 have no mass
    {
        Src v{0.0, 0.0, 0.0, 0.0f, 1.0f};
        if (t < cntB)
        {
            const uint32_t s = a.memSorted[start + j0 + t];
            const size_t   p = (size_t)a.first + a.order[s];
            v                = Src{a.xs[s], a.ys[s], a.zs[s], a.m[p], a.h[p]};
        }
        src[t] = v;
    }
    double xi = 0.0, yi = 0.0, zi = 0.0, mi = 0.0;
    float  hi_ = 1.0f;
    const bool valid = t < cntA;
    if (valid)
    {
        const uint32_t s = a.memSorted[start + i0 + t];
        const size_t   p = (size_t)a.first + a.order[s];
        xi = a.xs[s], yi = a.ys[s], zi = a.zs[s], mi = (double)a.m[p], hi_ = a.h[p];
    }
    __syncthreads();

    // the diagonal item: a wave starts at its first lane (sources at or before the target are masked below)
    const uint32_t sBegin = diag ? (t & ~63u) : 0u;
    const uint32_t sEnd   = (cntB + 3u) & ~3u;
    const uint32_t after  = diag ? t : 0xffffffffu; // sources s > after count; all of them off the diagonal
    float          acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t s0 = sBegin; s0 < sEnd; s0 += 4)
    {
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
        {
            const uint32_t s  = s0 + u;
            const Src      q  = src[s];
            const float    fx = (float)image<Pbc>(q.x - xi, a.half[0], a.len[0]);
            const float    fy = (float)image<Pbc>(q.y - yi, a.half[1], a.len[1]);
            const float    fz = (float)image<Pbc>(q.z - zi, a.half[2], a.len[2]);
            const float    r2 = (fx * fx + fy * fy) + fz * fz;
            const float    hij = hi_ + q.h;
            const float    h2  = hij * hij;
            const float    re2 = r2 < h2 ? h2 : r2;
            // r_eff = 0 happens with r = 0 only, where the term is 0 whatever the root: no branch in the loop
            const float    ri   = __builtin_amdgcn_rsqf(re2 > 0.0f ? re2 : 1.0f);
            const float    term = (q.m * r2) * ((ri * ri) * ri);
            acc[u] += (s > after || !diag) ? term : 0.0f;
        }
    }
    const double lane = valid ? mi * (((double)acc[0] + (double)acc[1]) + ((double)acc[2] + (double)acc[3])) : 0.0;
    part[t]           = lane;
    treeSum(part, t);
    if (t == 0)
    {
        a.partial[w] = part[0];
        const unsigned long long pairs =
            diag ? (unsigned long long)cntA * (cntA - 1) / 2 : (unsigned long long)cntA * cntB;
        atomicAdd(a.counters + 0, pairs);
        atomicAdd(a.counters + 1, 1ull);
    }
}

/*! one workgroup per catalogue group: its items k, k + 256, ... per thread in turn, then the pairwise tree; epot =
 *  -(G sum).  A group over the cap has no items and gets NaN. */
__global__ __launch_bounds__(kBlock) void combineKernel(const double* __restrict__ partial,
                                                        const uint64_t* __restrict__ itemStart,
                                                        const uint32_t* __restrict__ outCount, uint32_t cap, float G,
                                                        double* __restrict__ epot, unsigned long long* counters)
{
    __shared__ double part[kBlock];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const uint64_t k0 = itemStart[g], k1 = itemStart[g + 1];
    double         sum = 0.0;
    for (uint64_t k = k0 + t; k < k1; k += kBlock)
        sum += partial[k];
    part[t] = sum;
    treeSum(part, t);
    if (t == 0)
    {
        const bool over = outCount[g] > cap;
        epot[g]         = over ? __builtin_nan("") : -((double)G * part[0]);
        atomicAdd(counters + (over ? 3 : 2), 1ull);
    }
}

} // namespace

// ---- the launcher ------------------------------------------------------------------------------------------------

int compute(Arena& arena, fof::FofBuffers& fb, HaloBuffers& b, const sx_halo& p, const sx_fields& f, const sx_box& box,
            uint32_t first, uint32_t last, const uint64_t* id, const sx_halo_result& res, bool toHost, hipStream_t s,
            std::string& err)
{
    const uint32_t n    = last - first;
    const bool     mom  = (p.flags & SX_HALO_MOMENTS) && (res.groupSigma || res.groupShape || res.groupAngmom || res.groupRmax);
    const bool     thm  = (p.flags & SX_HALO_THERMAL) && res.groupEint;
    const bool     pot  = (p.flags & SX_HALO_POTENTIAL) && res.groupEpot;
    const uint32_t pcap = p.maxPairMembers ? p.maxPairMembers : kDefaultPairCap;
    const auto     kind = toHost ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;

    b.counters     = arena.get<uint64_t>("halo.counters", 5);
    b.countersHost = arena.pinned<uint64_t>("halo.countersHost", 5);
    if (!b.counters || !b.countersHost)
    {
        err = "sx_halo: counter buffers";
        return SX_ERR_NOMEM;
    }
    SX_TRY_HIP(kWho, b.clock.begin());
    SX_TRY_HIP(kWho, b.clock.mark(0, s));
    SX_TRY_HIP(kWho, hipMemsetAsync(b.counters, 0, 5 * sizeof(uint64_t), s));

    // ---- the search, behind the density cut
    fof::Extra extra;
    extra.rhoMin = p.rhoMin, extra.std = p.std, extra.kx = f.kx, extra.xm = f.xm, extra.rho = f.rho;
    extra.members = mom || thm || pot;
    if (int rc = fof::compute(arena, fb, fofOf(p), f, box, first, last, id, fofOf(res), toHost, s, err, &extra)) return rc;
    SX_TRY_HIP(kWho, b.clock.mark(1, s));

    const uint32_t G     = fb.catGroups;
    uint64_t       total = 0;
    if (G && extra.members)
    {
        if (!fb.members)
        {
            err = "sx_halo: the search left no member lists";
            return SX_ERR_ARG;
        }
        const size_t cap = std::min<size_t>(p.maxGroups, std::max(n, 1u));
        b.out            = arena.get<double>("halo.out", kOutPerGroup * cap);
        if (!b.out)
        {
            err = "sx_halo: result buffers";
            return SX_ERR_NOMEM;
        }
        const uint32_t oneCell[3] = {1, 1, 1};
        const Grid     g          = cellgrid::makeGrid(box, oneCell, p.linking); // read for the minimum image only
        // ---- moments and the thermal energy
        if (mom || thm)
        {
            MomentArgs ma{fb.memSorted, fb.segStart, fb.outCount, fb.grid.order, fb.xs, fb.ys, fb.zs, f.m, f.vx, f.vy, f.vz,
                          f.temp, first, G, g, fb.outReal, thm ? (double)idealGasCv(p.muiConst, p.gamma) : 0.0, mom, thm, b.out};
            momentKernel<<<G, kBlock, 0, s>>>(ma);
        }
        SX_TRY_HIP(kWho, b.clock.mark(2, s));
        // ---- the potential
        if (pot)
        {
            size_t scanBytes = 0;
            SX_TRY_HIP(kWho, hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, b.items, b.itemStart, (int)(cap + 1), s));
            b.items     = arena.get<uint64_t>("halo.items", cap + 1);
            b.itemStart = arena.get<uint64_t>("halo.itemStart", cap + 1);
            b.scanTmp   = arena.get<char>("halo.scanTmp", scanBytes);
            if (!b.items || !b.itemStart || !b.scanTmp)
            {
                err = "sx_halo: work item buffers";
                return SX_ERR_NOMEM;
            }
            itemKernel<<<blocks((size_t)G + 1), kBlock, 0, s>>>(fb.outCount, G, pcap, b.items);
            SX_TRY_HIP(kWho, hipcub::DeviceScan::ExclusiveSum(b.scanTmp, scanBytes, b.items, b.itemStart, (int)(G + 1), s));
            SX_TRY_HIP(kWho, hipMemcpyAsync(b.countersHost + 4, b.itemStart + G, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            SX_TRY_HIP(kWho, hipStreamSynchronize(s));
            total = b.countersHost[4];
            if (total)
            {
                b.partial = arena.get<double>("halo.partial", total);
                if (!b.partial)
                {
                    err = "sx_halo: " + std::to_string(total) + " work items need " + std::to_string(8 * total) +
                          " bytes of partial sums; lower maxPairMembers";
                    return SX_ERR_NOMEM;
                }
                PairArgs pa{fb.memSorted, fb.segStart, fb.outCount, fb.grid.order, fb.xs, fb.ys, fb.zs, f.m, f.h, first, G,
                            {},           {},          b.itemStart, 0,             b.partial,
                            reinterpret_cast<unsigned long long*>(b.counters)};
                bool pbc = false;
                for (int k = 0; k < 3; ++k)
                {
                    pa.half[k] = g.pbc[k] ? g.half[k] : HUGE_VAL;
                    pa.len[k]  = g.len[k];
                    pbc        = pbc || g.pbc[k];
                }
                constexpr uint64_t kMaxLaunch = 1ull << 30;
                for (uint64_t base = 0; base < total; base += kMaxLaunch)
                {
                    pa.itemBase        = base;
                    const unsigned grd = (unsigned)std::min(kMaxLaunch, total - base);
                    if (pbc) pairKernel<true><<<grd, kBlock, 0, s>>>(pa);
                    else pairKernel<false><<<grd, kBlock, 0, s>>>(pa);
                }
            }
            SX_TRY_HIP(kWho, b.clock.mark(3, s));
            combineKernel<<<G, kBlock, 0, s>>>(b.partial, b.itemStart, fb.outCount, pcap, p.G, b.out + 17 * (size_t)G,
                                               reinterpret_cast<unsigned long long*>(b.counters));
        }
        else SX_TRY_HIP(kWho, b.clock.mark(3, s));
        SX_TRY_HIP(kWho, hipGetLastError());

        // ---- results: device to device, or through the pinned buffer
        struct Piece
        {
            double* dst;
            size_t  off, per;
            bool    on;
        };
        const Piece pieces[6] = {{res.groupSigma, 0, 6, mom},   {res.groupShape, 6, 6, mom}, {res.groupAngmom, 12, 3, mom},
                                 {res.groupRmax, 15, 1, mom},   {res.groupEint, 16, 1, thm}, {res.groupEpot, 17, 1, pot}};
        if (toHost)
        {
            b.outHost = arena.pinned<double>("halo.outHost", kOutPerGroup * cap);
            if (!b.outHost)
            {
                err = "sx_halo: pinned result buffer";
                return SX_ERR_NOMEM;
            }
            SX_TRY_HIP(kWho, hipMemcpyAsync(b.outHost, b.out, kOutPerGroup * (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        else
            for (const Piece& pc : pieces)
                if (pc.on && pc.dst)
                    SX_TRY_HIP(kWho, hipMemcpyAsync(pc.dst, b.out + pc.off * G, pc.per * (size_t)G * sizeof(double), kind, s));
        SX_TRY_HIP(kWho, hipMemcpyAsync(b.countersHost, b.counters, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        SX_TRY_HIP(kWho, b.clock.mark(4, s));
        SX_TRY_HIP(kWho, hipStreamSynchronize(s));
        if (toHost)
            for (const Piece& pc : pieces)
                if (pc.on && pc.dst) std::memcpy(pc.dst, b.outHost + pc.off * G, pc.per * (size_t)G * sizeof(double));
        std::copy(b.countersHost, b.countersHost + 4, b.stats);
    }
    else
    {
        for (int k = 2; k <= 4; ++k)
            SX_TRY_HIP(kWho, b.clock.mark(k, s));
        SX_TRY_HIP(kWho, hipStreamSynchronize(s));
        std::fill(b.stats, b.stats + 4, 0ull);
    }
    b.clock.finish();
    b.done = true;
    return SX_OK;
}

} // namespace sx::halo
