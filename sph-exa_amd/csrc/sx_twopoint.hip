/*! @file sx_twopoint.hip
 * @brief Two-point statistics (sx_twopoint.hpp): the cell grid, the window pass, the gather, the pair kernel and the
 *        conversion.
 *
 * The pair kernel.  One lane per sorted particle i, 256 per workgroup.  The lane walks the particles j > i of the 27 cells
 * round its own (sx_cellgrid.hpp: nine x-runs), so every unordered pair is visited once, from its earlier member, and
 * with stride > 1 dropped unless one member is a target (a lane per target instead lost: DESIGN.md 7m).  A
 * non-finite particle carries a NaN x in the sorted columns: every r2 with it is a NaN and fails each comparison.  A pair
 * beyond r_max is dropped on r2 before the square root.  An accepted pair adds 1 to its bin's count and fixed(term) to
 * the bin's 128-bit sum of every enabled series, all in block-private LDS: an add to the low word whose returned old
 * value tells this lane whether it carried, then an add of (high word + carry) to the high word, skipped where that is
 * zero (always, for the non-negative series, until a bin's low word wraps).  The pair is not consistent mid-flight and
 * need not be: only the totals are read, after the kernel.  A workgroup's non-zero words go to the global accumulators
 * with 64-bit integer atomics once, at its end.  No floating-point atomic anywhere.
 * Built with -ffp-contract=off: the arithmetic rule of include/sphexa_hip.h.
 */
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sx_twopoint.hpp"

namespace sx::twopoint
{

// ---- host decisions ---------------------------------------------------------------------------------------------

std::string checkSpec(const sx_twopoint* p, const sx_box* box)
{
    if (!p || !box) return "sx_twopoint_check: null specification or box";
    if (!p->edges) return "sx_twopoint_check: null edges";
    char buf[320];
    if (p->nbins == 0 || p->nbins > kMaxBins)
    {
        std::snprintf(buf, sizeof buf, "sx_twopoint_check: nbins must be 1 .. %u (got %u)", kMaxBins, p->nbins);
        return buf;
    }
    for (uint32_t k = 0; k <= p->nbins; ++k)
        if (!std::isfinite(p->edges[k]))
        {
            std::snprintf(buf, sizeof buf, "sx_twopoint_check: edge %u is not finite (%g)", k, p->edges[k]);
            return buf;
        }
    if (p->edges[0] < 0.0)
    {
        std::snprintf(buf, sizeof buf, "sx_twopoint_check: the first edge is negative (%g)", p->edges[0]);
        return buf;
    }
    for (uint32_t k = 0; k < p->nbins; ++k)
        if (!(p->edges[k] < p->edges[k + 1]))
        {
            std::snprintf(buf, sizeof buf, "sx_twopoint_check: the edges do not ascend strictly at %u (%g, then %g)", k,
                          p->edges[k], p->edges[k + 1]);
            return buf;
        }
    if (p->stride == 0) return "sx_twopoint_check: stride is 0 (1 takes every particle as a target)";
    if (p->phase >= p->stride)
    {
        std::snprintf(buf, sizeof buf, "sx_twopoint_check: phase %u is not below stride %u", p->phase, p->stride);
        return buf;
    }
    if (p->series & ~SX_TP_ALL)
    {
        std::snprintf(buf, sizeof buf, "sx_twopoint_check: unknown series flags 0x%x (known: 0x%x)", p->series & ~SX_TP_ALL,
                      SX_TP_ALL);
        return buf;
    }
    const double rmax = p->edges[p->nbins];
    for (int a = 0; a < 3; ++a)
    {
        const double L = box->lim[2 * a + 1] - box->lim[2 * a];
        if (box->bnd[a] == 1 && !(rmax <= L / 3.0))
        {
            std::snprintf(buf, sizeof buf,
                          "sx_twopoint_check: r_max %g exceeds a third of the periodic %c extent %g (%g): three distinct "
                          "cells and an unambiguous minimum image need it",
                          rmax, "xyz"[a], L, L / 3.0);
            return buf;
        }
    }
    return {};
}

void chooseGrid(const sx_twopoint& p, const sx_box& box, uint64_t n, uint32_t dims[3])
{
    cellgrid::chooseDims(p.edges[p.nbins], box, n, dims);
}

std::string whyRefused(const sx_twopoint* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_twopoint_result* res)
{
    if (std::string why = checkSpec(p, box); !why.empty()) return why;
    if (!f || !res) return "sx_twopoint: null fields or result";
    if (first > last || last > f->n) return "sx_twopoint: [first, last) is not a range of f";
    if (!f->x || !f->y || !f->z || !f->vx || !f->vy || !f->vz) return "sx_twopoint: x, y, z, vx, vy and vz are required";
    if ((p->series & SX_TP_WW) && !f->m) return "sx_twopoint: the series WW needs m";
    if ((uint64_t)last - first > kMaxParticles) return "sx_twopoint: more than 2^31 - 1 particles";
    return {};
}

// ---- kernels -----------------------------------------------------------------------------------------------------

namespace
{

using cellgrid::Grid;
using cellgrid::minImage;
using exact::add128;
using exact::U128;

__device__ __forceinline__ bool finite(double v) { return exact::finiteBits(exact::doubleBits(v)); }

/*! the windows, nonfinite, targets and the flags of the particles of the range, in the order of the columns.  Integer
 *  maxima on the exponent keys: any order gives the same key. */
__global__ __launch_bounds__(kBlock) void windowKernel(const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ z, const float* __restrict__ vx,
                                                       const float* __restrict__ vy, const float* __restrict__ vz,
                                                       const float* __restrict__ m, const uint64_t* __restrict__ id,
                                                       uint32_t first, uint32_t n, uint32_t stride, uint32_t phase,
                                                       uint8_t* __restrict__ flags, uint32_t* __restrict__ winKeys,
                                                       unsigned long long* __restrict__ acc)
{
    __shared__ uint32_t sKey[2], sCnt[2];
    if (threadIdx.x < 2) sKey[threadIdx.x] = 0, sCnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n)
    {
        const size_t p  = (size_t)first + i;
        const double dvx = (double)vx[p], dvy = (double)vy[p], dvz = (double)vz[p];
        const double dm  = m ? (double)m[p] : 0.0;
        const bool   fin = finite(x[p]) && finite(y[p]) && finite(z[p]) && finite(dvx) && finite(dvy) && finite(dvz) &&
                         finite(dm);
        const uint64_t key = id ? id[p] : (uint64_t)p;
        const bool     tgt = key % stride == phase;
        flags[i]           = (uint8_t)((fin ? kFinite : 0) | (tgt ? kTarget : 0));
        if (fin)
        {
            const uint32_t kv = max(max(exact::windowKey(dvx), exact::windowKey(dvy)), exact::windowKey(dvz));
            if (kv) atomicMax(&sKey[0], kv);
            if (m)
            {
                const uint32_t km = exact::windowKey(dm);
                if (km) atomicMax(&sKey[1], km);
            }
            if (tgt) atomicAdd(&sCnt[0], 1u);
        }
        else atomicAdd(&sCnt[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2)
    {
        if (sKey[threadIdx.x]) atomicMax(&winKeys[threadIdx.x], sKey[threadIdx.x]);
        if (sCnt[threadIdx.x]) atomicAdd(&acc[2 + threadIdx.x], (unsigned long long)sCnt[threadIdx.x]);
    }
}

//! the columns in the sorted order; a non-finite particle gets a NaN x, which keeps it out of every pair
__global__ __launch_bounds__(kBlock) void gatherKernel(const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ z, const float* __restrict__ vx,
                                                       const float* __restrict__ vy, const float* __restrict__ vz,
                                                       const float* __restrict__ m, uint32_t first, uint32_t n,
                                                       const uint32_t* __restrict__ order,
                                                       const uint8_t* __restrict__ flags, double* __restrict__ xs,
                                                       double* __restrict__ ys, double* __restrict__ zs,
                                                       float* __restrict__ vxs, float* __restrict__ vys,
                                                       float* __restrict__ vzs, float* __restrict__ ms,
                                                       uint8_t* __restrict__ flagsSorted)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t o  = order[s];
    const size_t   p  = (size_t)first + o;
    const uint8_t  fl = flags[o];
    xs[s] = (fl & kFinite) ? x[p] : NAN, ys[s] = y[p], zs[s] = z[p];
    vxs[s] = vx[p], vys[s] = vy[p], vzs[s] = vz[p];
    if (m) ms[s] = m[p];
    flagsSorted[s] = fl;
}

struct PairArgs
{
    const double *  xs, *ys, *zs;
    const float *   vxs, *vys, *vzs, *ms;
    const uint8_t*  flags;
    const uint32_t *keys, *cellStart, *winKeys;
    const double*   edges;
    uint32_t        n, nbins, series;
    int             allTargets;
    double          cut; // a pair with r2 >= cut has r >= r_max
    Grid            g;
    unsigned long long* acc;
};

//! the windows of the six series from the two keys of the window pass
__device__ __host__ __forceinline__ void windows(uint32_t vkey, uint32_t mkey, int32_t E[kSeries])
{
    const int32_t Eu = exact::windowOfKey(vkey) + 2, em = exact::windowOfKey(mkey);
    E[0] = Eu, E[1] = 2 * Eu, E[2] = 3 * Eu, E[3] = 3 * Eu, E[4] = 2 * Eu, E[5] = 2 * em;
}

extern __shared__ unsigned long long sMem[];

/*! LDS: [edges nbins + 1 | count nbins | (low, high) x nbins per enabled series, in the order of the flags].  Vel: some
 *  velocity series is on; Mass: WW is on. */
template<bool Vel, bool Mass>
__global__ __launch_bounds__(kBlock) void pairKernel(PairArgs a)
{
    const uint32_t nb     = a.nbins;
    double* const  sEdges = reinterpret_cast<double*>(sMem);
    unsigned long long* const sBins = sMem + nb + 1;
    // the slot of series k among the enabled ones
    int slot[kSeries], nslot = 0;
#pragma unroll
    for (int k = 0; k < kSeries; ++k)
        slot[k] = (a.series >> k) & 1u ? nslot++ : -1;
    const uint32_t words = nb * (1 + 2 * (uint32_t)nslot);
    for (uint32_t w = threadIdx.x; w <= nb; w += kBlock)
        sEdges[w] = a.edges[w];
    for (uint32_t w = threadIdx.x; w < words; w += kBlock)
        sBins[w] = 0ull;
    __syncthreads();
    int32_t E[kSeries];
    windows(a.winKeys[0], a.winKeys[1], E);

    const uint32_t     i     = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long tests = 0, same = 0;
    const uint8_t      fi    = i < a.n ? a.flags[i] : 0;
    if (fi & kFinite)
    {
        const Grid&  g  = a.g;
        const double xi = a.xs[i], yi = a.ys[i], zi = a.zs[i];
        double       vxi = 0, vyi = 0, vzi = 0, mi = 0;
        if constexpr (Vel) vxi = (double)a.vxs[i], vyi = (double)a.vys[i], vzi = (double)a.vzs[i];
        if constexpr (Mass) mi = (double)a.ms[i];
        const bool   ti = a.allTargets || (fi & kTarget);
        const double e0 = sEdges[0], eN = sEdges[nb];
        auto scan = [&](uint32_t begin, uint32_t end)
        {
            for (uint32_t j = begin > i ? begin : i + 1; j < end; ++j)
            {
                if (!ti && !(a.flags[j] & kTarget)) continue;
                const double dx = minImage(a.xs[j] - xi, g.pbc[0], g.half[0], g.len[0]);
                const double dy = minImage(a.ys[j] - yi, g.pbc[1], g.half[1], g.len[1]);
                const double dz = minImage(a.zs[j] - zi, g.pbc[2], g.half[2], g.len[2]);
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                if (!(r2 == r2)) continue; // j is not finite
                ++tests;
                if (r2 == 0.0)
                {
                    ++same;
                    continue;
                }
                if (r2 >= a.cut) continue;
                const double r = sqrt(r2);
                if (!(r >= e0 && r < eN)) continue;
                uint32_t lo = 0, hi = nb;
                while (hi - lo > 1)
                {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sEdges[mid] <= r) lo = mid;
                    else hi = mid;
                }
                atomicAdd(&sBins[lo], 1ull);
                if constexpr (Vel)
                {
                    const double dvx = (double)a.vxs[j] - vxi, dvy = (double)a.vys[j] - vyi, dvz = (double)a.vzs[j] - vzi;
                    const double u  = ((dvx * dx + dvy * dy) + dvz * dz) / r;
                    const double u2 = u * u, u3 = u2 * u;
                    if (slot[0] >= 0) add128(&sBins[nb + 2 * (slot[0] * nb + lo)], exact::toFixedShift(u, E[0], kShift));
                    if (slot[1] >= 0) add128(&sBins[nb + 2 * (slot[1] * nb + lo)], exact::toFixedShift(u2, E[1], kShift));
                    if (slot[2] >= 0) add128(&sBins[nb + 2 * (slot[2] * nb + lo)], exact::toFixedShift(u3, E[2], kShift));
                    if (slot[3] >= 0)
                        add128(&sBins[nb + 2 * (slot[3] * nb + lo)], exact::toFixedShift(fabs(u3), E[3], kShift));
                    if (slot[4] >= 0)
                        add128(&sBins[nb + 2 * (slot[4] * nb + lo)],
                               exact::toFixedShift((dvx * dvx + dvy * dvy) + dvz * dvz, E[4], kShift));
                }
                if constexpr (Mass)
                    add128(&sBins[nb + 2 * (slot[5] * nb + lo)], exact::toFixedShift(mi * (double)a.ms[j], E[5], kShift));
            }
        };
        cellgrid::forEachRun(g, a.keys[i], a.cellStart, scan);
    }
    // the wave's counts in one add each; every lane of the wave arrives here
    for (int o = 32; o > 0; o >>= 1)
    {
        tests += __shfl_xor(tests, o);
        same += __shfl_xor(same, o);
    }
    if ((threadIdx.x & 63) == 0)
    {
        if (tests) atomicAdd(a.acc + 0, tests);
        if (same) atomicAdd(a.acc + 1, same);
    }
    __syncthreads();
    // the block's totals into the global array [count | (low, high) x kSeries x nbins]; empty bins cost nothing
    unsigned long long* const global = a.acc + kHead;
    for (uint32_t b = threadIdx.x; b < nb; b += kBlock)
        if (sBins[b]) atomicAdd(&global[b], sBins[b]);
#pragma unroll
    for (int k = 0; k < kSeries; ++k)
        if (slot[k] >= 0)
            for (uint32_t b = threadIdx.x; b < nb; b += kBlock)
            {
                const uint32_t w = nb + 2 * (slot[k] * nb + b);
                add128(&global[nb + 2 * ((uint32_t)k * nb + b)], U128{sBins[w], sBins[w + 1]});
            }
}

//! [count nbins | U1 .. WW nbins each | targets, nonfinite, coincident, pairs tested] from the accumulators
__global__ void convertKernel(const uint64_t* __restrict__ acc, const uint32_t* __restrict__ winKeys, uint32_t nb,
                              uint64_t* __restrict__ out)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nb) out[w] = acc[kHead + w];
    else if (w < nb * (1 + kSeries))
    {
        int32_t E[kSeries];
        windows(winKeys[0], winKeys[1], E);
        const uint32_t  k = (w - nb) / nb, b = (w - nb) % nb;
        const uint64_t* p = acc + kHead + nb + 2 * ((size_t)k * nb + b);
        out[w]            = exact::doubleBits(exact::fromFixedShift(U128{p[0], p[1]}, E[k], kShift));
    }
    else if (w < nb * (1 + kSeries) + 4)
    {
        const uint32_t t = w - nb * (1 + kSeries);
        out[w]           = acc[t == 0 ? 2 : t == 1 ? 3 : t == 2 ? 1 : 0];
    }
}

constexpr const char* kWho = "sx_twopoint"; // in front of the messages of SX_TRY_HIP and the cell index

} // namespace

// ---- the launcher ------------------------------------------------------------------------------------------------

int compute(Arena& arena, TwoPointBuffers& b, const sx_twopoint& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, const uint64_t* id, const sx_twopoint_result& res, bool toHost, hipStream_t s,
            std::string& err)
{
    const uint32_t n = last - first, nb = p.nbins;
    uint32_t       dims[3];
    chooseGrid(p, box, n, dims);
    const bool     wantM  = (p.series & SX_TP_WW) != 0;
    const size_t   nAcc   = accWords(nb), nOut = outWords(nb);

    b.flags       = arena.get<uint8_t>("twopoint.flags", n);
    b.winKeys     = arena.get<uint32_t>("twopoint.winKeys", 2);
    b.xs          = arena.get<double>("twopoint.xs", n);
    b.ys          = arena.get<double>("twopoint.ys", n);
    b.zs          = arena.get<double>("twopoint.zs", n);
    b.vxs         = arena.get<float>("twopoint.vxs", n);
    b.vys         = arena.get<float>("twopoint.vys", n);
    b.vzs         = arena.get<float>("twopoint.vzs", n);
    b.ms          = arena.get<float>("twopoint.ms", n);
    b.flagsSorted = arena.get<uint8_t>("twopoint.flagsSorted", n);
    b.edges       = arena.get<double>("twopoint.edges", kMaxBins + 1);
    b.acc         = arena.get<uint64_t>("twopoint.acc", accWords(kMaxBins));
    b.out         = arena.get<uint64_t>("twopoint.out", outWords(kMaxBins));
    b.outHost     = arena.pinned<uint64_t>("twopoint.outHost", outWords(kMaxBins));
    if (!b.flags || !b.winKeys || !b.xs || !b.ys || !b.zs || !b.vxs || !b.vys || !b.vzs || !b.ms || !b.flagsSorted ||
        !b.edges || !b.acc || !b.out || !b.outHost)
    {
        err = "sx_twopoint: scratch buffers";
        return SX_ERR_NOMEM;
    }
    SX_TRY_HIP(kWho, b.clock.begin());

    const Grid       g   = cellgrid::makeGrid(box, dims, p.edges[nb]);
    cellgrid::Index& ix  = b.grid;
    auto*            acc = reinterpret_cast<unsigned long long*>(b.acc);
    SX_TRY_HIP(kWho, hipMemsetAsync(b.acc, 0, nAcc * sizeof(uint64_t), s));
    SX_TRY_HIP(kWho, hipMemsetAsync(b.winKeys, 0, 2 * sizeof(uint32_t), s));
    SX_TRY_HIP(kWho, hipMemcpyAsync(b.edges, p.edges, ((size_t)nb + 1) * sizeof(double), hipMemcpyHostToDevice, s));

    // ---- grid
    SX_TRY_HIP(kWho, b.clock.mark(0, s));
    if (int rc = cellgrid::build(arena, "twopoint.", ix, g, f.x, f.y, f.z, first, n, 0, s, kWho, err)) return rc;
    SX_TRY_HIP(kWho, b.clock.mark(1, s));
    // ---- windows, gather
    if (n)
    {
        windowKernel<<<blocks(n), kBlock, 0, s>>>(f.x, f.y, f.z, f.vx, f.vy, f.vz, wantM ? f.m : nullptr, id, first, n,
                                                  p.stride, p.phase, b.flags, b.winKeys, acc);
        gatherKernel<<<blocks(n), kBlock, 0, s>>>(f.x, f.y, f.z, f.vx, f.vy, f.vz, wantM ? f.m : nullptr, first, n,
                                                  ix.order, b.flags, b.xs, b.ys, b.zs, b.vxs, b.vys, b.vzs, b.ms,
                                                  b.flagsSorted);
    }
    SX_TRY_HIP(kWho, b.clock.mark(2, s));
    // ---- pairs
    if (n)
    {
        const double rmax = p.edges[nb];
        PairArgs     a{b.xs, b.ys, b.zs, b.vxs, b.vys, b.vzs, b.ms, b.flagsSorted, ix.keysSorted, ix.cellStart, b.winKeys,
                   b.edges, n, nb, p.series, p.stride == 1, (rmax * rmax) * (1.0 + 0x1p-50), g, acc};
        const int    nslot = __builtin_popcount(p.series & SX_TP_ALL);
        const size_t lds   = ((size_t)nb + 1 + (size_t)nb * (1 + 2 * nslot)) * sizeof(uint64_t);
        const bool   vel   = (p.series & SX_TP_VEL) != 0;
        if (vel && wantM) pairKernel<true, true><<<blocks(n), kBlock, lds, s>>>(a);
        else if (vel) pairKernel<true, false><<<blocks(n), kBlock, lds, s>>>(a);
        else if (wantM) pairKernel<false, true><<<blocks(n), kBlock, lds, s>>>(a);
        else pairKernel<false, false><<<blocks(n), kBlock, lds, s>>>(a);
    }
    SX_TRY_HIP(kWho, b.clock.mark(3, s));
    // ---- conversion
    convertKernel<<<(unsigned)((nOut + 255) / 256), 256, 0, s>>>(b.acc, b.winKeys, nb, b.out);
    SX_TRY_HIP(kWho, b.clock.mark(4, s));
    SX_TRY_HIP(kWho, hipGetLastError());
    SX_TRY_HIP(kWho, hipMemcpyAsync(b.outHost, b.out, nOut * sizeof(uint64_t), hipMemcpyDeviceToHost, s));

    void* const dst[1 + kSeries] = {res.count, res.U1, res.U2, res.U3, res.A3, res.T2, res.WW};
    const size_t tot = (size_t)nb * (1 + kSeries);
    if (!toHost)
    {
        for (int k = 0; k <= kSeries; ++k)
            if (dst[k] && (k == 0 || ((p.series >> (k - 1)) & 1u)))
                SX_TRY_HIP(kWho, hipMemcpyAsync(dst[k], b.out + (size_t)k * nb, (size_t)nb * sizeof(uint64_t),
                                      hipMemcpyDeviceToDevice, s));
        if (res.totals)
            SX_TRY_HIP(kWho, hipMemcpyAsync(res.totals, b.out + tot, 3 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    }
    SX_TRY_HIP(kWho, hipStreamSynchronize(s));
    if (toHost)
    {
        for (int k = 0; k <= kSeries; ++k)
            if (dst[k] && (k == 0 || ((p.series >> (k - 1)) & 1u)))
                std::memcpy(dst[k], b.outHost + (size_t)k * nb, (size_t)nb * sizeof(uint64_t));
        if (res.totals) std::memcpy(res.totals, b.outHost + tot, 3 * sizeof(uint64_t));
    }
    b.clock.finish();
    uint64_t binned = 0;
    for (uint32_t k = 0; k < nb; ++k)
        binned += b.outHost[k];
    b.stats[0] = b.outHost[tot + 3], b.stats[1] = binned;
    b.stats[2] = b.outHost[tot], b.stats[3] = b.outHost[tot + 1], b.stats[4] = b.outHost[tot + 2];
    b.done     = true;
    return SX_OK;
}

} // namespace sx::twopoint
