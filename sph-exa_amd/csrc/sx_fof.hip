/*! @file sx_fof.hip
 * @brief Friends-of-friends groups: cell grid, lock-free union-find, labels and the catalogue (sx_fof.hpp).
 */
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "sx_exactsum.hpp"
#include "sx_fof.hpp"

namespace sx::fof
{

// ---- host decisions ---------------------------------------------------------------------------------------------

std::string checkSpec(const sx_fof* p, const sx_box* box)
{
    if (!p || !box) return "sx_fof_check: null specification or box";
    char buf[256];
    if (!std::isfinite(p->linking) || !(p->linking > 0.0))
    {
        std::snprintf(buf, sizeof buf, "sx_fof_check: the linking length must be finite and positive (got %g)", p->linking);
        return buf;
    }
    for (int a = 0; a < 3; ++a)
    {
        const double L = box->lim[2 * a + 1] - box->lim[2 * a];
        if (box->bnd[a] == 1 && !(p->linking <= L / 3.0))
        {
            std::snprintf(buf, sizeof buf,
                          "sx_fof_check: the linking length %g exceeds a third of the periodic %c extent %g (%g): three "
                          "distinct cells and an unambiguous minimum image need it",
                          p->linking, "xyz"[a], L, L / 3.0);
            return buf;
        }
    }
    return {};
}

void chooseGrid(const sx_fof& p, const sx_box& box, uint64_t n, uint32_t dims[3])
{
    cellgrid::chooseDims(p.linking, box, n, dims);
}

std::string whyRefused(const sx_fof* p, const sx_box* box, const sx_fields* f, uint32_t first, uint32_t last,
                       const sx_fof_result* res)
{
    if (std::string why = checkSpec(p, box); !why.empty()) return why;
    if (!f || !res) return "sx_fof: null fields or result";
    if (first > last || last > f->n) return "sx_fof: [first, last) is not a range of f";
    if (!f->x || !f->y || !f->z) return "sx_fof: x, y and z are required";
    if ((uint64_t)last - first > kMaxParticles) return "sx_fof: more than 2^31 - 1 particles";
    const bool real = res->groupMass || res->groupCom || res->groupVel;
    const bool cat  = real || res->groupLabel || res->groupCount;
    if (cat && p->maxGroups == 0) return "sx_fof: maxGroups is 0 with a catalogue array set (capacity 0 for a catalogue that was asked for)";
    if (real && (!f->m || !f->vx || !f->vy || !f->vz)) return "sx_fof: the catalogue's mass, centre and velocity need m, vx, vy and vz";
    return {};
}

// ---- kernels -----------------------------------------------------------------------------------------------------

namespace
{

using cellgrid::Grid;
using cellgrid::minImage;

__global__ __launch_bounds__(kBlock) void gatherKernel(const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ z, uint32_t first, uint32_t n,
                                                       const uint32_t* __restrict__ order, double* __restrict__ xs,
                                                       double* __restrict__ ys, double* __restrict__ zs,
                                                       uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                       unsigned long long* __restrict__ minId, uint32_t* __restrict__ rankOf)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const size_t p = (size_t)first + order[s];
    xs[s] = x[p], ys[s] = y[p], zs[s] = z[p];
    parent[s] = s, count[s] = 0, minId[s] = ~0ull, rankOf[s] = kNoGroup;
}

//! the density cut of the group properties: an unselected particle (a NaN density included) gets a NaN sorted x
__global__ __launch_bounds__(kBlock) void maskKernel(const float* __restrict__ kx, const float* __restrict__ m,
                                                     const float* __restrict__ xm, const float* __restrict__ rho,
                                                     int std, double rhoMin, uint32_t first, uint32_t n,
                                                     const uint32_t* __restrict__ order, double* __restrict__ xs)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const size_t p = (size_t)first + order[s];
    const float  r = std ? rho[p] : (kx[p] * m[p]) / xm[p];
    if (!((double)r >= rhoMin)) xs[s] = __builtin_nan("");
}

//! a load that another compute unit's store reaches: the first-level cache is per compute unit and not coherent
__device__ __forceinline__ uint32_t loadShared(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

//! the root above x as seen now; on the way every visited node is lowered to its grandparent (an ancestor: no cycle)
__device__ __forceinline__ uint32_t findRoot(uint32_t* parent, uint32_t x)
{
    uint32_t p = loadShared(parent + x);
    while (p != x)
    {
        const uint32_t gp = loadShared(parent + p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

//! joins the components of a and b; returns the root both are under now.  retries: compare-and-swaps lost
__device__ __forceinline__ uint32_t unite(uint32_t* parent, uint32_t a, uint32_t b, unsigned long long& retries)
{
    for (;;)
    {
        a = findRoot(parent, a);
        b = findRoot(parent, b);
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        ++retries; // hi was hooked under old < hi meanwhile: go on from there
        a = old, b = lo;
    }
}

struct LinkArgs
{
    const double *  xs, *ys, *zs;
    const uint32_t *keys, *cellStart;
    uint32_t*       parent;
    uint32_t        n;
    Grid            g;
    unsigned long long* counters;
};

/*! one wave per 64 consecutive sorted targets, a lane per target.  A target tests the particles behind it in the sorted
 *  order that lie in the 27 cells around its own, so every unordered pair is tested once. */
__global__ __launch_bounds__(kBlock) void linkKernel(LinkArgs a)
{
    const uint32_t     i     = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long tests = 0, retries = 0;
    if (i < a.n)
    {
        const Grid&    g  = a.g;
        const double   xi = a.xs[i], yi = a.ys[i], zi = a.zs[i];
        const uint32_t key = a.keys[i];
        uint32_t       ri = i;
        auto scan = [&](uint32_t begin, uint32_t end)
        {
            for (uint32_t j = begin > i ? begin : i + 1; j < end; ++j)
            {
                const double ddx = minImage(xi - a.xs[j], g.pbc[0], g.half[0], g.len[0]);
                const double ddy = minImage(yi - a.ys[j], g.pbc[1], g.half[1], g.len[1]);
                const double ddz = minImage(zi - a.zs[j], g.pbc[2], g.half[2], g.len[2]);
                ++tests;
                if (ddx * ddx + ddy * ddy + ddz * ddz < g.l2) ri = unite(a.parent, ri, j, retries);
            }
        };
        cellgrid::forEachRun(g, key, a.cellStart, scan);
    }
    // the wave's counts in one add each; every lane of the wave arrives here
    for (int o = 32; o > 0; o >>= 1)
    {
        tests += __shfl_xor(tests, o);
        retries += __shfl_xor(retries, o);
    }
    if ((threadIdx.x & 63) == 0)
    {
        if (tests) atomicAdd(a.counters + 0, tests);
        if (retries) atomicAdd(a.counters + 1, retries);
    }
}

/*! pointer jumping to the end: root[s] is the root above s (nothing stores to parent[] here).  The label is the minimum
 *  id per root, the member count an integer add: the same totals whatever the order. */
template<bool Masked>
__global__ __launch_bounds__(kBlock) void compressKernel(const uint32_t* __restrict__ parent, uint32_t n, uint32_t first,
                                                         const uint32_t* __restrict__ order,
                                                         const double* __restrict__ xs,
                                                         const uint64_t* __restrict__ id, uint32_t* __restrict__ root,
                                                         unsigned long long* __restrict__ minId,
                                                         uint32_t* __restrict__ count, uint64_t* __restrict__ idKeys,
                                                         uint32_t* __restrict__ mem)
{
    const uint32_t     s  = blockIdx.x * kBlock + threadIdx.x;
    const bool         in = s < n;
    uint32_t           r  = kNoGroup;
    unsigned long long v  = ~0ull;
    if (in)
    {
        uint32_t p = parent[s];
        r          = s;
        while (p != r)
        {
            r = p;
            p = parent[r];
        }
        root[s]        = r;
        const size_t q = (size_t)first + order[s];
        v              = id ? id[q] : (uint64_t)q;
        idKeys[s]      = v;
        mem[s]         = s;
    }
    // neighbours in the sorted order mostly share their root: a wave that is of one root sends one minimum and one add
    // (a halo of 10^5 members would otherwise queue that many atomics on two addresses)
    const uint32_t r0 = __shfl(r, 0);
    if (__all(in && r == r0))
    {
        for (int o = 32; o > 0; o >>= 1)
        {
            const unsigned long long w = __shfl_xor(v, o);
            v                          = w < v ? w : v;
        }
        if ((threadIdx.x & 63) == 0)
        {
            atomicMin(minId + r0, v);
            atomicAdd(count + r0, 64u);
        }
    }
    else if (in && !(Masked && xs[s] != xs[s])) // an unselected particle is its own root: no label, no count
    {
        atomicMin(minId + r, v);
        atomicAdd(count + r, 1u);
    }
}

//! the labels in the order of the columns; the roots counted, those with minMembers members or more appended
template<bool Masked>
__global__ __launch_bounds__(kBlock) void labelKernel(const uint32_t* __restrict__ root, uint32_t n,
                                                      const uint32_t* __restrict__ order,
                                                      const double* __restrict__ xs,
                                                      const unsigned long long* __restrict__ minId,
                                                      const uint32_t* __restrict__ count, uint32_t minMembers,
                                                      uint64_t* __restrict__ label, uint64_t* __restrict__ selLabel,
                                                      uint32_t* __restrict__ selRoot, unsigned long long* counters)
{
    const uint32_t s      = blockIdx.x * kBlock + threadIdx.x;
    const bool     in     = s < n;
    const uint32_t r      = in ? root[s] : 0;
    const bool     isRoot = in && r == s && !(Masked && xs[s] != xs[s]);
    if (in) label[order[s]] = minId[r]; // of an unselected particle: still ~0
    const unsigned long long roots = __popcll(__ballot(isRoot));
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(counters + 2, roots);
    if (isRoot && count[s] >= minMembers)
    {
        const unsigned long long slot = atomicAdd(counters + 3, 1ull);
        selLabel[slot] = minId[s];
        selRoot[slot]  = s;
    }
}

__global__ __launch_bounds__(kBlock) void selKeyKernel(const uint32_t* __restrict__ selRootSorted,
                                                       const uint32_t* __restrict__ count, uint32_t G,
                                                       uint32_t* __restrict__ selKey, uint32_t* __restrict__ selPos)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= G) return;
    selKey[k] = ~count[selRootSorted[k]]; // ascending in ~count: descending in count
    selPos[k] = k;
}

//! the first Gc groups of the order (count descending, label ascending): their rank at the root, label and count out
__global__ __launch_bounds__(kBlock) void rankKernel(const uint32_t* __restrict__ selPosSorted,
                                                     const uint32_t* __restrict__ selRootSorted,
                                                     const uint64_t* __restrict__ selLabelSorted,
                                                     const uint32_t* __restrict__ count, uint32_t Gc,
                                                     uint32_t* __restrict__ rankOf, uint64_t* __restrict__ outLabel,
                                                     uint32_t* __restrict__ outCount, uint32_t* __restrict__ segCount)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= Gc) return;
    const uint32_t pos = selPosSorted[k], r = selRootSorted[pos];
    rankOf[r]   = k;
    outLabel[k] = selLabelSorted[pos];
    outCount[k] = segCount[k] = count[r];
}

__global__ __launch_bounds__(kBlock) void memKeyKernel(const uint32_t* __restrict__ memById,
                                                       const uint32_t* __restrict__ root,
                                                       const uint32_t* __restrict__ rankOf, uint32_t n, uint32_t Gc,
                                                       uint32_t* __restrict__ memKey)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t g = rankOf[root[memById[k]]];
    memKey[k]        = g < Gc ? g : Gc; // no catalogue group: behind them all
}

struct ReduceArgs
{
    const uint32_t *memSorted, *segStart, *outCount, *order;
    const double *  xs, *ys, *zs;
    const float *   m, *vx, *vy, *vz;
    uint32_t        first, G;
    Grid            g;
    double*         outReal; // [mass G | com 3 G | vel 3 G]
};

/*! one workgroup per catalogue group.  Thread t sums the members t, t + 256, ... of the (id-ordered) segment in turn,
 *  then the 256 partials are added pairwise in LDS: a fixed order, so the same bits on every run. */
__global__ __launch_bounds__(kBlock) void reduceKernel(ReduceArgs a)
{
    __shared__ double part[7][kBlock];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const uint32_t start = a.segStart[g], cnt = a.outCount[g];
    const uint32_t sRef  = a.memSorted[start];
    const double   ref[3] = {a.xs[sRef], a.ys[sRef], a.zs[sRef]};
    double         sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = t; k < cnt; k += kBlock)
    {
        const uint32_t s  = a.memSorted[start + k];
        const size_t   p  = (size_t)a.first + a.order[s];
        const double   mk = (double)a.m[p];
        sum[0] += mk;
        sum[1] += mk * minImage(a.xs[s] - ref[0], a.g.pbc[0], a.g.half[0], a.g.len[0]);
        sum[2] += mk * minImage(a.ys[s] - ref[1], a.g.pbc[1], a.g.half[1], a.g.len[1]);
        sum[3] += mk * minImage(a.zs[s] - ref[2], a.g.pbc[2], a.g.half[2], a.g.len[2]);
        sum[4] += mk * (double)a.vx[p];
        sum[5] += mk * (double)a.vy[p];
        sum[6] += mk * (double)a.vz[p];
    }
    for (int q = 0; q < 7; ++q)
        part[q][t] = sum[q];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1)
    {
        if (t < (uint32_t)w)
            for (int q = 0; q < 7; ++q)
                part[q][t] += part[q][t + w];
        __syncthreads();
    }
    if (t == 0)
    {
        const double M = part[0][0];
        a.outReal[g]   = M;
        for (int k = 0; k < 3; ++k)
        {
            double c = ref[k] + part[1 + k][0] / M;
            if (a.g.pbc[k])
            {
                if (c < a.g.lo[k]) c += a.g.len[k];
                else if (c >= a.g.hi[k]) c -= a.g.len[k];
            }
            a.outReal[(size_t)a.G + 3 * (size_t)g + k]     = c;
            a.outReal[4 * (size_t)a.G + 3 * (size_t)g + k] = part[4 + k][0] / M;
        }
    }
}

constexpr const char* kWho = "sx_fof"; // in front of the messages of SX_TRY_HIP and the cell index

} // namespace

// ---- the launcher ------------------------------------------------------------------------------------------------

int compute(Arena& arena, FofBuffers& b, const sx_fof& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, const uint64_t* id, const sx_fof_result& res, bool toHost, hipStream_t s, std::string& err,
            const Extra* extra)
{
    const uint32_t n = last - first;
    uint32_t       dims[3];
    chooseGrid(p, box, n, dims);
    const uint32_t minMembers = std::max(1u, p.minMembers);
    const bool     masked     = extra && extra->rhoMin > 0.0;
    const bool     wantReal   = res.groupMass || res.groupCom || res.groupVel || (extra && extra->members);
    const bool     wantCat    = wantReal || res.groupLabel || res.groupCount;
    const uint32_t cap        = wantCat ? std::min(p.maxGroups, std::max(n, 1u)) : 0;
    const auto     kind       = toHost ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;

    b.counters     = arena.get<uint64_t>("fof.counters", 4);
    b.countersHost = arena.pinned<uint64_t>("fof.countersHost", 4);
    if (!b.counters || !b.countersHost)
    {
        err = "sx_fof: counter buffers";
        return SX_ERR_NOMEM;
    }
    b.catGroups = 0, b.members = false;
    SX_TRY_HIP(kWho, b.clock.begin());
    SX_TRY_HIP(kWho, hipMemsetAsync(b.counters, 0, 4 * sizeof(uint64_t), s));
    if (n == 0)
    {
        if (res.numGroups) SX_TRY_HIP(kWho, hipMemcpyAsync(res.numGroups, b.counters, 2 * sizeof(uint64_t), kind, s));
        SX_TRY_HIP(kWho, hipStreamSynchronize(s));
        std::fill(b.stats, b.stats + 4, 0ull);
        b.done = true;
        return SX_OK;
    }

    // the catalogue's largest sort and its scan run in the cell index's temporary storage (a size query reads no pointer)
    size_t sortTmp = 0, scanTmp = 0;
    SX_TRY_HIP(kWho, hipcub::DeviceRadixSort::SortPairs(nullptr, sortTmp, b.idKeys, b.idKeysSorted, b.mem, b.memById,
                                                        (int)n, 0, 64, s));
    SX_TRY_HIP(kWho, hipcub::DeviceScan::ExclusiveSum(nullptr, scanTmp, b.segCount, b.segStart, (int)n, s));
    b.xs       = arena.get<double>("fof.xs", n);
    b.ys       = arena.get<double>("fof.ys", n);
    b.zs       = arena.get<double>("fof.zs", n);
    b.parent   = arena.get<uint32_t>("fof.parent", n);
    b.root     = arena.get<uint32_t>("fof.root", n);
    b.count    = arena.get<uint32_t>("fof.count", n);
    b.rankOf   = arena.get<uint32_t>("fof.rankOf", n);
    b.minId    = arena.get<uint64_t>("fof.minId", n);
    b.label    = arena.get<uint64_t>("fof.label", n);
    b.selLabel = arena.get<uint64_t>("fof.selLabel", n);
    b.selRoot  = arena.get<uint32_t>("fof.selRoot", n);
    b.idKeys   = arena.get<uint64_t>("fof.idKeys", n);
    b.mem      = arena.get<uint32_t>("fof.mem", n);
    if (!b.xs || !b.ys || !b.zs || !b.parent || !b.root || !b.count || !b.rankOf || !b.minId || !b.label ||
        !b.selLabel || !b.selRoot || !b.idKeys || !b.mem)
    {
        err = "sx_fof: scratch buffers";
        return SX_ERR_NOMEM;
    }

    const Grid      g        = cellgrid::makeGrid(box, dims, p.linking);
    cellgrid::Index& ix      = b.grid;
    auto*           counters = reinterpret_cast<unsigned long long*>(b.counters);
    auto*           minId    = reinterpret_cast<unsigned long long*>(b.minId);

    // ---- grid
    SX_TRY_HIP(kWho, b.clock.mark(0, s));
    if (int rc = cellgrid::build(arena, "fof.", ix, g, f.x, f.y, f.z, first, n, std::max(sortTmp, scanTmp), s, kWho, err))
        return rc;
    gatherKernel<<<blocks(n), kBlock, 0, s>>>(f.x, f.y, f.z, first, n, ix.order, b.xs, b.ys, b.zs, b.parent, b.count,
                                              minId, b.rankOf);
    if (masked)
        maskKernel<<<blocks(n), kBlock, 0, s>>>(extra->kx, f.m, extra->xm, extra->rho, extra->std, extra->rhoMin, first, n,
                                                ix.order, b.xs);
    SX_TRY_HIP(kWho, b.clock.mark(1, s));
    // ---- link
    LinkArgs la{b.xs, b.ys, b.zs, ix.keysSorted, ix.cellStart, b.parent, n, g, counters};
    linkKernel<<<blocks(n), kBlock, 0, s>>>(la);
    SX_TRY_HIP(kWho, b.clock.mark(2, s));
    // ---- compress, labels, counts
    if (masked)
    {
        compressKernel<true><<<blocks(n), kBlock, 0, s>>>(b.parent, n, first, ix.order, b.xs, id, b.root, minId, b.count,
                                                          b.idKeys, b.mem);
        labelKernel<true><<<blocks(n), kBlock, 0, s>>>(b.root, n, ix.order, b.xs, minId, b.count, minMembers, b.label,
                                                       b.selLabel, b.selRoot, counters);
    }
    else
    {
        compressKernel<false><<<blocks(n), kBlock, 0, s>>>(b.parent, n, first, ix.order, b.xs, id, b.root, minId, b.count,
                                                           b.idKeys, b.mem);
        labelKernel<false><<<blocks(n), kBlock, 0, s>>>(b.root, n, ix.order, b.xs, minId, b.count, minMembers, b.label,
                                                        b.selLabel, b.selRoot, counters);
    }
    SX_TRY_HIP(kWho, b.clock.mark(3, s));
    SX_TRY_HIP(kWho, hipGetLastError());
    SX_TRY_HIP(kWho, hipMemcpyAsync(b.countersHost, b.counters, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SX_TRY_HIP(kWho, hipStreamSynchronize(s));
    const uint64_t numAll = b.countersHost[2], G = b.countersHost[3];
    const uint32_t Gc     = (uint32_t)std::min<uint64_t>(G, cap);
    if (res.label) SX_TRY_HIP(kWho, hipMemcpyAsync(res.label, b.label, (size_t)n * sizeof(uint64_t), kind, s));
    if (res.numGroups)
    {
        // [selected, all]: the counters hold them the other way round
        SX_TRY_HIP(kWho, hipMemcpyAsync(res.numGroups, b.counters + 3, sizeof(uint64_t), kind, s));
        SX_TRY_HIP(kWho, hipMemcpyAsync(res.numGroups + 1, b.counters + 2, sizeof(uint64_t), kind, s));
    }

    // ---- catalogue
    b.catGroups = Gc;
    if (Gc)
    {
        b.selLabelSorted = arena.get<uint64_t>("fof.selLabelSorted", n);
        b.selRootSorted  = arena.get<uint32_t>("fof.selRootSorted", n);
        b.selKey         = arena.get<uint32_t>("fof.selKey", n);
        b.selKeySorted   = arena.get<uint32_t>("fof.selKeySorted", n);
        b.selPos         = arena.get<uint32_t>("fof.selPos", n);
        b.selPosSorted   = arena.get<uint32_t>("fof.selPosSorted", n);
        b.segCount       = arena.get<uint32_t>("fof.segCount", n);
        b.segStart       = arena.get<uint32_t>("fof.segStart", n);
        b.outLabel       = arena.get<uint64_t>("fof.outLabel", n);
        b.outCount       = arena.get<uint32_t>("fof.outCount", n);
        if (!b.selLabelSorted || !b.selRootSorted || !b.selKey || !b.selKeySorted || !b.selPos || !b.selPosSorted ||
            !b.segCount || !b.segStart || !b.outLabel || !b.outCount)
        {
            err = "sx_fof: catalogue buffers";
            return SX_ERR_NOMEM;
        }
        // by label ascending, then (stable) by count descending
        SX_TRY_HIP(kWho, hipcub::DeviceRadixSort::SortPairs(ix.sortTmp, ix.tmpBytes, b.selLabel, b.selLabelSorted,
                                                            b.selRoot, b.selRootSorted, (int)G, 0, 64, s));
        selKeyKernel<<<blocks(G), kBlock, 0, s>>>(b.selRootSorted, b.count, (uint32_t)G, b.selKey, b.selPos);
        SX_TRY_HIP(kWho, hipcub::DeviceRadixSort::SortPairs(ix.sortTmp, ix.tmpBytes, b.selKey, b.selKeySorted, b.selPos,
                                                            b.selPosSorted, (int)G, 0, 32, s));
        rankKernel<<<blocks(Gc), kBlock, 0, s>>>(b.selPosSorted, b.selRootSorted, b.selLabelSorted, b.count, Gc, b.rankOf,
                                                 b.outLabel, b.outCount, b.segCount);
        if (res.groupLabel)
            SX_TRY_HIP(kWho, hipMemcpyAsync(res.groupLabel, b.outLabel, (size_t)Gc * sizeof(uint64_t), kind, s));
        if (res.groupCount)
            SX_TRY_HIP(kWho, hipMemcpyAsync(res.groupCount, b.outCount, (size_t)Gc * sizeof(uint32_t), kind, s));
        if (wantReal)
        {
            b.idKeysSorted = arena.get<uint64_t>("fof.idKeysSorted", n);
            b.memById      = arena.get<uint32_t>("fof.memById", n);
            b.memKey       = arena.get<uint32_t>("fof.memKey", n);
            b.memKeySorted = arena.get<uint32_t>("fof.memKeySorted", n);
            b.memSorted    = arena.get<uint32_t>("fof.memSorted", n);
            b.outReal      = arena.get<double>("fof.outReal", 7 * (size_t)n);
            if (!b.idKeysSorted || !b.memById || !b.memKey || !b.memKeySorted || !b.memSorted || !b.outReal)
            {
                err = "sx_fof: member buffers";
                return SX_ERR_NOMEM;
            }
            SX_TRY_HIP(kWho, hipcub::DeviceScan::ExclusiveSum(ix.sortTmp, ix.tmpBytes, b.segCount, b.segStart,
                                                              (int)Gc, s));
            // the members by id ascending, then (stable) by group: the catalogue groups' segments lead
            SX_TRY_HIP(kWho, hipcub::DeviceRadixSort::SortPairs(ix.sortTmp, ix.tmpBytes, b.idKeys, b.idKeysSorted,
                                                                b.mem, b.memById, (int)n, 0, 64, s));
            memKeyKernel<<<blocks(n), kBlock, 0, s>>>(b.memById, b.root, b.rankOf, n, Gc, b.memKey);
            SX_TRY_HIP(kWho, hipcub::DeviceRadixSort::SortPairs(ix.sortTmp, ix.tmpBytes, b.memKey, b.memKeySorted,
                                                                b.memById, b.memSorted, (int)n, 0,
                                                                std::max(1, exact::bitLength(Gc)), s));
            ReduceArgs ra{b.memSorted, b.segStart, b.outCount, ix.order, b.xs, b.ys, b.zs, f.m, f.vx, f.vy, f.vz, first, Gc, g,
                          b.outReal};
            reduceKernel<<<Gc, kBlock, 0, s>>>(ra);
            b.members = true;
            if (res.groupMass)
                SX_TRY_HIP(kWho, hipMemcpyAsync(res.groupMass, b.outReal, (size_t)Gc * sizeof(double), kind, s));
            if (res.groupCom)
                SX_TRY_HIP(kWho, hipMemcpyAsync(res.groupCom, b.outReal + Gc, 3 * (size_t)Gc * sizeof(double), kind,
                                                s));
            if (res.groupVel)
                SX_TRY_HIP(kWho, hipMemcpyAsync(res.groupVel, b.outReal + 4 * (size_t)Gc,
                                                3 * (size_t)Gc * sizeof(double), kind, s));
        }
    }
    SX_TRY_HIP(kWho, b.clock.mark(4, s));
    SX_TRY_HIP(kWho, hipGetLastError());
    SX_TRY_HIP(kWho, hipStreamSynchronize(s));
    b.clock.finish();
    b.stats[0] = b.countersHost[0], b.stats[1] = b.countersHost[1], b.stats[2] = numAll, b.stats[3] = G;
    b.done     = true;
    return SX_OK;
}

} // namespace sx::fof
