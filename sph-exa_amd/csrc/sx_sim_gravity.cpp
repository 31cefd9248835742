/*! @file sx_sim_gravity.cpp
 * @brief Self-gravity of sx_sim: the single-rank stage, the multi-rank near / far decomposition, the Ewald step of
 *        periodic boxes and the force-error check of the walk.
 */
#include "sx_sim_internal.hpp"

using namespace sx;
using namespace sx::sim;

namespace
{

//! max |a|^2 over [first, last) for accelerationTimestep (ts_global.hpp:47-67)
__global__ void maxAccSqKernel(const float* ax, const float* ay, const float* az, size_t first, size_t last,
                               unsigned long long* out)
{
    double v = 0.0;
    for (size_t i = first + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < last; i += (size_t)gridDim.x * blockDim.x)
    {
        double x = ax[i], y = ay[i], z = az[i], q = x * x + (y * y + z * z);
        v        = q > v ? q : v;
    }
    // wave max -> block max -> one atomic per block (a per-wave atomic on one address serialises: 0.74 ms at 4M)
    __shared__ double s[4];
    v = waveMax(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        double m = s[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            m = s[w] > m ? s[w] : m;
        atomicMax(out, (unsigned long long)__double_as_longlong(m));
    }
}

// ---- multi-rank gravity helpers (distributedGravity) ----------------------------------------------------------

constexpr int kCellShift = 63 - kHistBits; // level-6 cell of a key: the global histogram bins, one owner each

//! source record of a gravity halo: coordinates, mass, smoothing length and the SFC key of the owner's last sync
//! (inside a ve-bdt hierarchy the particles drift while the key order of the sync stays the tree's order)
struct __attribute__((aligned(8))) GPart
{
    double   x, y, z;
    float    m, h;
    uint64_t key;
};

__global__ void farKeysKernel(uint64_t* keys, size_t n)
{
    size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (c < n) keys[c] = (uint64_t)c << kCellShift;
}

__global__ void cellFlagKernel(const uint64_t* keys, size_t n, uint32_t* flag)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i > n) return;
    flag[i] = (i < n && (i == 0 || (keys[i] >> kCellShift) != (keys[i - 1] >> kCellShift))) ? 1u : 0u;
}

__global__ void cellCountCheckKernel(const uint32_t* total, uint32_t expected, unsigned* err)
{
    if (*total != expected) *err = 1u;
}

//! the buffers hold nCells (+1) entries, sized from the sync's histogram; a scan that disagrees (cellCountCheckKernel
//! reports it) writes nothing out of range
__global__ void cellScatterKernel(const uint64_t* keys, const uint32_t* flag, const uint32_t* scan, size_t n,
                                  uint32_t nCells, uint32_t* cellBeg, uint32_t* cellIds)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n && flag[i] && scan[i] < nCells)
    {
        cellBeg[scan[i]] = (uint32_t)i;
        cellIds[scan[i]] = (uint32_t)(keys[i] >> kCellShift);
    }
    if (i == n && scan[n] <= nCells) cellBeg[scan[n]] = (uint32_t)n;
}

__global__ void nearToFarKernel(const uint32_t* nearFlag, size_t n, uint32_t* farFlag, uint32_t* reqFlag)
{
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k > n) return;
    const uint32_t v = k < n ? nearFlag[k] : 0u;
    if (k < n) farFlag[k] = 1u - v;
    reqFlag[k] = v;
}

__global__ void reqScatterKernel(const GCell* cells, const uint32_t* reqFlag, const uint32_t* scan, size_t n,
                                 uint32_t* reqIds)
{
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k < n && reqFlag[k]) reqIds[scan[k]] = cells[k].cell;
}

//! v[q] = scan[off[q]] for the P+1 segment boundaries
__global__ void segmentAtKernel(const uint32_t* scan, const uint64_t* off, int P, uint32_t* out)
{
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= P) out[q] = scan[off[q]];
}

//! owner side: requested cell -> particle range of the local cell (binary search over the sorted local cell ids)
__global__ void reqLookupKernel(const uint32_t* req, size_t nReq, const uint32_t* cellIds, const uint32_t* cellBeg,
                                int nCells, uint32_t* size, uint32_t* beg)
{
    size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k > nReq) return;
    if (k == nReq)
    {
        size[k] = 0;
        return;
    }
    const uint32_t id = req[k];
    int            lo = 0, hi = nCells;
    while (lo < hi)
    {
        int mid = (lo + hi) >> 1;
        if (cellIds[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    const bool found = lo < nCells && cellIds[lo] == id;
    beg[k]           = found ? cellBeg[lo] : 0u;
    size[k]          = found ? cellBeg[lo + 1] - cellBeg[lo] : 0u;
}

//! one wave per request: the cell's particles into the send buffer at its scanned offset
__global__ void gatherCellsKernel(const uint32_t* beg, const uint32_t* size, const uint32_t* off, size_t nReq,
                                  const double* x, const double* y, const double* z, const float* m, const float* h,
                                  const uint64_t* keys, GPart* out)
{
    const size_t k    = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const int    lane = threadIdx.x & 63;
    if (k >= nReq) return;
    const uint32_t b = beg[k], c = size[k], o = off[k];
    for (uint32_t t = lane; t < c; t += 64)
    {
        const uint32_t i = b + t;
        out[o + t]       = GPart{x[i], y[i], z[i], m[i], h[i], keys[i]};
    }
}

__global__ void unpackGPartKernel(const GPart* in, size_t n, double* x, double* y, double* z, float* m, float* h,
                                  uint64_t* keys)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GPart p = in[i];
    x[i] = p.x, y[i] = p.y, z[i] = p.z, m[i] = p.m, h[i] = p.h, keys[i] = p.key;
}

} // namespace

namespace sx::sim
{

unsigned long long* gravReserveInteractions(sx_sim* s)
{
    return s->grav.inter = s->work.get<unsigned long long>("grav.inter", 2);
}

//! per-wavefront potential-energy sums of a traversal over nTargets targets (GravArgs::waveE)
static double* gravWaveE(sx_sim* s, uint32_t nTargets)
{
    return s->work.get<double>("grav.waveE", (nTargets + kWave - 1) / kWave + 1);
}

//! the part of a walk's arguments that the sim fixes: G, the opening angle, the step's accumulators, the kernel variant,
//! the interaction counters (on request) and, in a periodic box, the one image shell (then nothing is counted)
static void gravSimConstants(const sx_sim* s, GravArgs& a)
{
    const bool pbc = periodicGravity(s);
    a.G            = (float)s->p.g;
    a.invTheta     = 1.0f / s->p.theta;
    a.egrav        = &s->sc->egrav;
    a.err          = &s->sc->gravErr;
    a.fast         = sx_ctx_exact_internal(s->ctx) ? 0 : 1;
    a.interactions = s->gravCount && !pbc ? s->grav.inter : nullptr;
    if (pbc)
    {
        a.numShells = 1;
        for (int d = 0; d < 3; ++d)
            a.boxL[d] = s->box.lim[2 * d + 1] - s->box.lim[2 * d];
    }
}

/*! the Ewald correction of periodic self-gravity (gravity_wrapper.hpp:135-157) for the locals [first, last), from the
 *  global root expansion (c4: mass center, m8: quadrupole) with the reference's EwaldSettings defaults (ewald.h:17-21)
 *  and the walk's one image shell; the box is a cube (checked by sx_sim_create) */
int ewaldStep(sx_sim* s, const double c4[4], const float m8[8], const uint8_t* active, hipStream_t st)
{
    EwaldArgs           ea{};
    std::vector<double> hs;
    const double        L = s->box.lim[1] - s->box.lim[0];
    if (ewaldInit(ea.p, hs, c4, m8, L, 1, 2.6, 2.8, 2.0, 3.0e-3)) return SX_ERR_ARG;
    double* hd = s->work.get<double>("ewald.hsum", std::max<size_t>(hs.size(), 5));
    if (!hd) return SX_ERR_NOMEM;
    SIM_HIP(hipMemcpyAsync(hd, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ea.first = (uint32_t)s->first, ea.last = (uint32_t)s->last;
    ea.x = s->x, ea.y = s->y, ea.z = s->z, ea.m = s->m;
    ea.ax = s->ax, ea.ay = s->ay, ea.az = s->az;
    ea.active = active;
    ea.G = (float)s->p.g, ea.hsum = hd, ea.usum = &s->sc->egrav, ea.uscale = 0.5 * (double)ea.G;
    SIM_HIP(ewaldCorrection(ea, st));
    // the host table must outlive the copy
    SIM_HIP(hipStreamSynchronize(st));
    return SX_OK;
}

/*! Self-gravity with several ranks (replaces syncGrav + MultipoleHolder::upsweep/traverse of the reference,
 *  domain.hpp:246-372, multipole_holder.cuh:40-66, and the global multipole exchange of
 *  ryoanji/interface/global_multipole.hpp).  Sources are split by level-6 SFC cells, each owned by one rank (the
 *  splitters are histogram-bin boundaries):
 *   1. every rank forms mass center, MAC radius and quadrupole of its own cells; all cells are all-gathered;
 *   2. a remote cell that satisfies the vector MAC against every request box of this rank (each box contains 2048
 *      SFC-consecutive locals) is "far": its multipole is a leaf of the uniform level-6 far tree, whose upsweep and
 *      Barnes-Hut traversal give the far field (all other leaves massless);
 *   3. the particles of the remaining ("near") remote cells are fetched from their owners as gravity halos, merged
 *      with the locals in key order ([lower ranks | locals | higher ranks]) and traversed with the single-rank
 *      upsweep + traversal on their own tree.
 *  Each source is counted once (locals and near cells in the near tree, far cells in the far tree); every far-cell
 *  multipole is accepted by the same MAC the reference applies, so the result matches the single-rank
 *  Barnes-Hut field within its opening-angle error. */
int distributedGravity(sx_sim* s, hipStream_t st, const uint8_t* active, bool drift)
{
    sx::Transport* T  = s->comm;
    const int      P  = T->size(), r = T->rank();
    const size_t   nl = s->last - s->first;
    const float    invTheta = 1.0f / s->p.theta;
    const size_t   nCellsAll = size_t(1) << kHistBits;
    // periodic self-gravity: both walks over the one image shell of the single-rank path (gravity_wrapper.hpp:135-157)
    const bool     pbc = periodicGravity(s);
    const double   boxL[3] = {s->box.lim[1] - s->box.lim[0], s->box.lim[3] - s->box.lim[2], s->box.lim[5] - s->box.lim[4]};

    // --- far tree: uniform level-6 octree (one synthetic key per cell, bucket 1), built once
    if (s->farTree.numLeaves != (int)nCellsAll)
    {
        uint64_t* fk = s->gravWork.get<uint64_t>("far.keys", nCellsAll);
        farKeysKernel<<<grid(nCellsAll), 256, 0, st>>>(fk, nCellsAll);
        SIM_HIP(buildTree(s->farMem, fk, nCellsAll, 1, s->dbox, s->farTree, st));
        if (s->farTree.numLeaves != (int)nCellsAll) return SX_ERR_HIP;
        GravArgs fa   = gravArgs(s->farTree); // (the leaf map reads the links alone)
        fa.leafToNode = s->grav.farL2N = s->farMem.get<int32_t>("far.leafToNode", nCellsAll);
        SIM_HIP(farTreeLeafMap(fa, st));
        s->grav.farLay = s->farMem.get<uint32_t>("far.emptyLayout", nCellsAll + 1);
        SIM_HIP(hipMemsetAsync(s->grav.farLay, 0, 4 * (nCellsAll + 1), st));
    }
    int32_t*  farL2N = s->grav.farL2N;
    uint32_t* farLay = s->grav.farLay;
    Arena&    W      = s->gravWork;

    // --- 1. local cells: ranges of the key-sorted locals, moments
    const uint64_t* lkeys = s->keys + s->first;
    uint32_t*       flag  = W.get<uint32_t>("g.flag", nl + 1);
    uint32_t*       scan  = W.get<uint32_t>("g.scan", nl + 1);
    cellFlagKernel<<<grid(nl + 1), 256, 0, st>>>(lkeys, nl, flag);
    size_t tmpB = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmpB, flag, scan, (int)nl + 1, st);
    SIM_HIP(hipcub::DeviceScan::ExclusiveSum(W.get<char>("g.scantmp", tmpB), tmpB, flag, scan, (int)nl + 1, st));
    // the cell count is known from the sync's histogram (cellsOf); the device checks the scan agrees
    if (s->cellsOf.size() != (size_t)P) return SX_ERR_ARG;
    const int nCells = (int)s->cellsOf[r];
    cellCountCheckKernel<<<1, 1, 0, st>>>(scan + nl, (uint32_t)nCells, &s->sc->gravErr);
    uint32_t* cellBeg = W.get<uint32_t>("g.cellBeg", nCells + 1);
    uint32_t* cellIds = W.get<uint32_t>("g.cellIds", nCells);
    cellScatterKernel<<<grid(nl + 1), 256, 0, st>>>(lkeys, flag, scan, nl, (uint32_t)nCells, cellBeg, cellIds);
    GCell* mine = W.get<GCell>("g.mine", nCells);
    SIM_HIP(cellMoments(s->x + s->first, s->y + s->first, s->z + s->first, s->m + s->first, cellBeg, cellIds, nCells,
                        farL2N, s->farTree.centers, s->farTree.sizes, invTheta, mine, st, drift));

    // --- 2. all-gather the cells (rank order = key order)
    std::vector<uint64_t> cnt(P, (uint64_t)nCells), rcnt(s->cellsOf);
    cnt[r]  = 0;
    rcnt[r] = 0;
    std::vector<uint64_t> aOff(P + 1, 0);
    for (int q = 0; q < P; ++q)
        aOff[q + 1] = aOff[q] + rcnt[q];
    const size_t nAll = aOff[P];
    GCell*       all  = W.get<GCell>("g.all", nAll);
    {
        std::vector<uint64_t> sb(P), so(P, 0), rb(P), ro(P);
        for (int q = 0; q < P; ++q)
        {
            sb[q] = cnt[q] * sizeof(GCell);
            rb[q] = rcnt[q] * sizeof(GCell);
            ro[q] = aOff[q] * sizeof(GCell);
        }
        SIM_COMM(T->alltoallv(mine, sb.data(), so.data(), all, rb.data(), ro.data(), st));
    }

    // --- 3. near / far classification against this rank's request boxes (distributedSync step 4)
    const size_t  nChunks = (nl + kChunk - 1) / kChunk;
    const ReqBox* boxes   = s->dom.mybox;
    if (drift)
    {
        // the locals have moved since the sync's request boxes: boxes of their current positions (the same chunks)
        ReqBox* cur = W.get<ReqBox>("g.curbox", nChunks);
        if (!cur) return SX_ERR_NOMEM;
        if (nChunks)
            chunkBoxes(s->x + s->first, s->y + s->first, s->z + s->first, s->h + s->first, nl, nChunks, kHaloMargin,
                       quantMargin(s->dbox), r, cur, st);
        boxes = cur;
    }
    uint32_t*     nearF   = W.get<uint32_t>("g.near", nAll + 1);
    uint32_t*     farF    = W.get<uint32_t>("g.far", nAll + 1);
    uint32_t*     reqF    = W.get<uint32_t>("g.reqFlag", nAll + 1);
    uint32_t*     reqS    = W.get<uint32_t>("g.reqScan", nAll + 1);
    SIM_HIP(cellNearFlags(all, (int)nAll, reinterpret_cast<const double*>(boxes), (int)nChunks, nearF, st,
                          pbc ? boxL : nullptr));
    nearToFarKernel<<<grid(nAll + 1), 256, 0, st>>>(nearF, nAll, farF, reqF);
    tmpB = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmpB, reqF, reqS, (int)nAll + 1, st);
    SIM_HIP(hipcub::DeviceScan::ExclusiveSum(W.get<char>("g.scantmp2", tmpB), tmpB, reqF, reqS, (int)nAll + 1, st));
    uint32_t* reqIds = W.get<uint32_t>("g.reqIds", nAll);
    reqScatterKernel<<<grid(nAll), 256, 0, st>>>(all, reqF, reqS, nAll, reqIds);
    uint64_t* dOff = W.get<uint64_t>("g.aOff", P + 1);
    uint32_t* dAt  = W.get<uint32_t>("g.at", P + 1);
    SIM_HIP(hipMemcpyAsync(dOff, aOff.data(), 8 * (P + 1), hipMemcpyHostToDevice, st));
    segmentAtKernel<<<grid(P + 1, 64), 64, 0, st>>>(reqS, dOff, P, dAt);
    // --- 4. requests to the owners (counts from the device, exchanged and read back in one synchronisation), owners
    //        send the cells' particles
    diffCounts(nullptr, dAt, P, s->cntBuf, st);
    std::vector<uint64_t> reqCnt, reqOff, reqRecv;
    if (int e = deviceCountsOrAbort(s, false, st, reqCnt, reqOff, reqRecv)) return e;
    const uint64_t hwReq = reqOff[P]; // near (requested) remote cells
    std::vector<uint64_t> rrOff(P + 1, 0);
    for (int q = 0; q < P; ++q)
        rrOff[q + 1] = rrOff[q] + reqRecv[q];
    const size_t nReq = rrOff[P];
    uint32_t*    req  = W.get<uint32_t>("g.req", nReq);
    {
        std::vector<uint64_t> sb(P), so(P), rb(P), ro(P);
        for (int q = 0; q < P; ++q)
            sb[q] = reqCnt[q] * 4, so[q] = reqOff[q] * 4, rb[q] = reqRecv[q] * 4, ro[q] = rrOff[q] * 4;
        SIM_COMM(T->alltoallv(reqIds, sb.data(), so.data(), req, rb.data(), ro.data(), st));
    }
    uint32_t* rsize = W.get<uint32_t>("g.rsize", nReq + 1);
    uint32_t* rbeg  = W.get<uint32_t>("g.rbeg", nReq + 1);
    uint32_t* roff  = W.get<uint32_t>("g.roff", nReq + 1);
    reqLookupKernel<<<grid(nReq + 1), 256, 0, st>>>(req, nReq, cellIds, cellBeg, nCells, rsize, rbeg);
    tmpB = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmpB, rsize, roff, (int)nReq + 1, st);
    SIM_HIP(hipcub::DeviceScan::ExclusiveSum(W.get<char>("g.scantmp3", tmpB), tmpB, rsize, roff, (int)nReq + 1, st));
    SIM_HIP(hipMemcpyAsync(dOff, rrOff.data(), 8 * (P + 1), hipMemcpyHostToDevice, st));
    segmentAtKernel<<<grid(P + 1, 64), 64, 0, st>>>(roff, dOff, P, dAt);
    diffCounts(nullptr, dAt, P, s->cntBuf, st);
    std::vector<uint64_t> pCnt, pOff, pRecv;
    if (int e = deviceCountsOrAbort(s, false, st, pCnt, pOff, pRecv)) return e;
    const size_t nSend = pOff[P];
    GPart*       psend = W.get<GPart>("g.psend", nSend);
    if (nReq)
        gatherCellsKernel<<<grid(nReq * 64), 256, 0, st>>>(rbeg, rsize, roff, nReq, s->x + s->first, s->y + s->first,
                                                           s->z + s->first, s->m + s->first, s->h + s->first,
                                                           s->keys + s->first, psend);
    uint64_t nLow = 0, nHigh = 0;
    for (int q = 0; q < P; ++q)
        (q < r ? nLow : nHigh) += (q == r ? 0 : pRecv[q]);
    const size_t nG    = nLow + nl + nHigh;
    GPart*       precv = W.get<GPart>("g.precv", nLow + nHigh);
    {
        std::vector<uint64_t> sb(P), so(P), rb(P), ro(P);
        uint64_t              acc = 0;
        for (int q = 0; q < P; ++q)
        {
            sb[q] = pCnt[q] * sizeof(GPart), so[q] = pOff[q] * sizeof(GPart);
            rb[q] = (q == r ? 0 : pRecv[q]) * sizeof(GPart), ro[q] = acc * sizeof(GPart);
            acc += (q == r ? 0 : pRecv[q]);
        }
        SIM_COMM(T->alltoallv(psend, sb.data(), so.data(), precv, rb.data(), ro.data(), st));
    }

    // --- 5. near sources: [lower-rank halos | locals | higher-rank halos], key sorted by construction
    double*   gx = W.get<double>("g.x", nG);
    double*   gy = W.get<double>("g.y", nG);
    double*   gz = W.get<double>("g.z", nG);
    float*    gm = W.get<float>("g.m", nG);
    float*    gh = W.get<float>("g.h", nG);
    uint64_t* gk = W.get<uint64_t>("g.keys", nG);
    if (nLow) unpackGPartKernel<<<grid(nLow), 256, 0, st>>>(precv, nLow, gx, gy, gz, gm, gh, gk);
    if (nHigh)
        unpackGPartKernel<<<grid(nHigh), 256, 0, st>>>(precv + nLow, nHigh, gx + nLow + nl, gy + nLow + nl,
                                                       gz + nLow + nl, gm + nLow + nl, gh + nLow + nl, gk + nLow + nl);
    SIM_HIP(hipMemcpyAsync(gx + nLow, s->x + s->first, 8 * nl, hipMemcpyDeviceToDevice, st));
    SIM_HIP(hipMemcpyAsync(gy + nLow, s->y + s->first, 8 * nl, hipMemcpyDeviceToDevice, st));
    SIM_HIP(hipMemcpyAsync(gz + nLow, s->z + s->first, 8 * nl, hipMemcpyDeviceToDevice, st));
    SIM_HIP(hipMemcpyAsync(gm + nLow, s->m + s->first, 4 * nl, hipMemcpyDeviceToDevice, st));
    SIM_HIP(hipMemcpyAsync(gh + nLow, s->h + s->first, 4 * nl, hipMemcpyDeviceToDevice, st));
    // the keys of the last sync, not of the current positions: the sources stay in the sync's key order (inside a
    // ve-bdt hierarchy particles drift out of their cells, as in the reference's fixed focus tree)
    SIM_HIP(hipMemcpyAsync(gk + nLow, s->keys + s->first, 8 * nl, hipMemcpyDeviceToDevice, st));
    SIM_HIP(buildTree(W, gk, nG, s->bucket, s->dbox, s->nearTree, st));

    GravArgs ga = gravArgs(s->nearTree);
    gravSimConstants(s, ga);
    ga.first      = (uint32_t)nLow;
    ga.last       = (uint32_t)(nLow + nl);
    ga.leafToNode = W.get<int32_t>("g.leafToNode", (size_t)s->nearTree.numLeaves);
    if (drift)
    {
        // the near tree's cells come from the sync's keys: boxes holding each node's cell and its current particles
        double* c3 = W.get<double>("g.geoC", 3 * (size_t)s->nearTree.numNodes);
        double* s3 = W.get<double>("g.geoS", 3 * (size_t)s->nearTree.numNodes);
        if (!c3 || !s3) return SX_ERR_NOMEM;
        SIM_HIP(skinRefreshBoxes(s->nearTree, gx, gy, gz, s->dbox, c3, s3, st, true));
        ga.geoCenters = c3;
        ga.geoSizes   = s3;
    }
    ga.x = gx, ga.y = gy, ga.z = gz, ga.m = gm, ga.h = gh;
    ga.centers4   = W.get<double>("g.centers", 4 * (size_t)s->nearTree.numNodes);
    ga.multipoles = W.get<float>("g.multipoles", 8 * (size_t)s->nearTree.numNodes);
    // target i of the near arrays is local particle s->first + (i - nLow)
    const ptrdiff_t shift = (ptrdiff_t)s->first - (ptrdiff_t)nLow;
    ga.ax    = s->ax + shift;
    ga.ay    = s->ay + shift;
    ga.az    = s->az + shift;
    ga.active = active ? active + shift : nullptr;
    SIM_HIP(gravityUpsweep(ga, s->nearTree.levelRangeHost.data(), st));
    ga.waveE = gravWaveE(s, ga.last - ga.first);
    SIM_HIP(gravityTraverse(ga, st));

    // --- 6. far field: far cells as leaves of the level-6 tree, traversed by the locals
    GravArgs fa = gravArgs(s->farTree);
    gravSimConstants(s, fa);
    fa.first      = (uint32_t)s->first;
    fa.last       = (uint32_t)s->last;
    fa.layout     = farLay; // no particles: a far leaf is always accepted (MAC holds for every request box)
    fa.leafToNode = farL2N;
    fa.x = s->x, fa.y = s->y, fa.z = s->z, fa.m = s->m, fa.h = s->h;
    fa.centers4   = s->farMem.get<double>("far.centers", 4 * (size_t)s->farTree.numNodes);
    fa.multipoles = s->farMem.get<float>("far.multipoles", 8 * (size_t)s->farTree.numNodes);
    fa.ax = s->ax, fa.ay = s->ay, fa.az = s->az;
    fa.active = active;
    if (drift)
    {
        double* c3 = s->farMem.get<double>("far.geoC", 3 * (size_t)s->farTree.numNodes);
        double* s3 = s->farMem.get<double>("far.geoS", 3 * (size_t)s->farTree.numNodes);
        if (!c3 || !s3) return SX_ERR_NOMEM;
        SIM_HIP(farRefreshBoxes(fa, all, farF, (int)nAll, s->farTree.levelRangeHost.data(), c3, s3, st));
        fa.geoCenters = c3;
        fa.geoSizes   = s3;
    }
    SIM_HIP(farUpsweep(fa, all, farF, (int)nAll, s->farTree.levelRangeHost.data(), st));
    fa.waveE = gravWaveE(s, fa.last - fa.first);
    SIM_HIP(gravityTraverse(fa, st));
    if (pbc)
    {
        // the Ewald correction from the global root: the near tree (locals + near cells) and the far tree (far cells)
        // together hold every source once
        double cN[4], cF[4], c4[4];
        float  mN[8], mF[8], m8[8];
        SIM_HIP(hipMemcpyAsync(cN, ga.centers4, sizeof(cN), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(mN, ga.multipoles, sizeof(mN), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(cF, fa.centers4, sizeof(cF), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(mF, fa.multipoles, sizeof(mF), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        combineRoots(cN, mN, cF, mF, c4, m8);
        if (int e = ewaldStep(s, c4, m8, active, st)) return e;
    }
    s->gravHalos       = nLow + nHigh;
    s->gravRemoteCells = nAll;
    s->gravFarCells    = nAll - (reqOff.empty() ? 0 : hwReq);
    return SX_OK;
}

void maxAccSq(sx_sim* s, hipStream_t st)
{
    const size_t nl = s->last - s->first;
    if (nl)
        maxAccSqKernel<<<std::min<unsigned>(grid(nl), 2048), 256, 0, st>>>(s->ax, s->ay, s->az, s->first, s->last,
                                                                          &s->sc->maxAccSqBits);
}

//! self-gravity with periodic images (the reference's test, gravity_wrapper.hpp:77,135: boundaryX; sx_sim_create
//! admits only boxes periodic along all three axes with self-gravity)
bool periodicGravity(const sx_sim* s) { return s->p.g != 0.0 && s->box.bnd[0] == 1; }

/*! the armed step's force-error sample (sx_sim_set_gravity_check): every stride-th 64-particle target block of the walk
 *  that has just run (step: its arguments), walked once more into zeroed scratch accelerations and summed directly
 *  (sx_gravity_direct) into a second scratch, both read back and compared on the host.  Writes scratch only. */
int gravityCheck(sx_sim* s, const GravArgs& step, hipStream_t st)
{
    s->gravCheckValid = false;
    const uint32_t first = step.first, last = step.last;
    if (last <= first) return SX_OK;
    const uint32_t blocks = (last - first + kWave - 1) / kWave;
    const uint32_t want   = std::max(1u, (s->gravCheckTargets + kWave - 1) / kWave);
    const uint32_t stride = std::max(1u, (blocks + want / 2) / want);
    std::vector<uint32_t> grp; // starts, then ends
    for (uint32_t b = 0; b < blocks; b += stride)
        grp.push_back(first + b * kWave);
    const size_t ng = grp.size();
    for (size_t k = 0; k < ng; ++k)
        grp.push_back(std::min(grp[k] + (uint32_t)kWave, last));
    size_t T = 0;
    for (size_t k = 0; k < ng; ++k)
        T += grp[ng + k] - grp[k];

    const size_t n    = s->n;
    float*       acc  = s->work.get<float>("gravcheck.acc", 6 * n);
    uint8_t*     mask = s->work.get<uint8_t>("gravcheck.mask", n);
    uint32_t*    dg   = s->work.get<uint32_t>("gravcheck.groups", 2 * ng);
    double*      eg   = s->work.get<double>("gravcheck.egrav", 1);
    uint32_t*    er   = s->work.get<uint32_t>("gravcheck.err", 1);
    if (!acc || !mask || !dg || !eg || !er) return SX_ERR_NOMEM;
    SIM_HIP(hipMemsetAsync(acc, 0, 6 * n * sizeof(float), st));
    SIM_HIP(hipMemsetAsync(mask, 0, n, st));
    for (size_t k = 0; k < ng; ++k)
        SIM_HIP(hipMemsetAsync(mask + grp[k], 1, grp[ng + k] - grp[k], st));
    SIM_HIP(hipMemsetAsync(eg, 0, sizeof(double), st));
    SIM_HIP(hipMemsetAsync(er, 0, sizeof(uint32_t), st));
    SIM_HIP(hipMemcpyAsync(dg, grp.data(), grp.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));

    GravArgs ga     = step;
    ga.ax           = acc;
    ga.ay           = acc + n;
    ga.az           = acc + 2 * n;
    ga.active       = mask;
    ga.egrav        = eg;
    ga.waveE        = nullptr;
    ga.err          = er;
    ga.interactions = nullptr;
    SIM_HIP(gravityTraverse(ga, st));

    sx_fields f{};
    f.n = n;
    f.x = s->x, f.y = s->y, f.z = s->z, f.m = s->m, f.h = s->h;
    f.ax = acc + 3 * n, f.ay = acc + 4 * n, f.az = acc + 5 * n;
    const sx_groups g{0u, 0u, (uint32_t)ng, dg, dg + ng};
    if (int rc = sx_gravity_direct(s->ctx, &g, &f, &s->box, step.numShells, step.G, nullptr, nullptr)) return rc;

    std::vector<float> hw(3 * T), hd(3 * T);
    uint32_t           eb = 0;
    size_t             o  = 0;
    for (size_t k = 0; k < ng; ++k)
    {
        const size_t len = grp[ng + k] - grp[k];
        for (int c = 0; c < 3; ++c)
        {
            SIM_HIP(hipMemcpyAsync(hw.data() + c * T + o, acc + c * n + grp[k], len * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
            SIM_HIP(hipMemcpyAsync(hd.data() + c * T + o, acc + (3 + c) * n + grp[k], len * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
        }
        o += len;
    }
    SIM_HIP(hipMemcpyAsync(&eb, er, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SIM_HIP(hipStreamSynchronize(st));
    if (eb)
    {
        sx_ctx_set_error_internal(s->ctx, "GPU traversal stack exhausted in Barnes-Hut (gravity check)");
        return SX_ERR_TRAVERSAL;
    }
    std::vector<double> rel(T);
    double              sum = 0.0, d2 = 0.0, a2 = 0.0;
    for (size_t t = 0; t < T; ++t)
    {
        double dd = 0.0, aa = 0.0;
        for (int c = 0; c < 3; ++c)
        {
            const double w = hw[c * T + t], d = hd[c * T + t];
            dd += (w - d) * (w - d);
            aa += d * d;
        }
        rel[t] = std::sqrt(dd) / std::sqrt(aa);
        sum += rel[t];
        d2 += dd;
        a2 += aa;
    }
    std::sort(rel.begin(), rel.end());
    s->gravCheck[0]   = (double)T;
    s->gravCheck[1]   = sum / (double)T;
    s->gravCheck[2]   = rel[T / 2];
    s->gravCheck[3]   = rel[std::min(T - 1, (size_t)(0.99 * (double)T))];
    s->gravCheck[4]   = rel[T - 1];
    s->gravCheck[5]   = std::sqrt(d2 / a2);
    s->gravCheckValid = true;
    return SX_OK;
}

//! one rank: upsweep + traversal on the step's tree, added to ax, ay, az; the armed force-error check; in a periodic
//! box the walk over one image shell, then the Ewald correction (gravity_wrapper.hpp:135-157)
static int singleRankGravity(sx_sim* s, hipStream_t st, bool reuse)
{
    GravArgs ga = gravArgs(s->tree);
    gravSimConstants(s, ga);
    ga.first = (uint32_t)s->first;
    ga.last  = (uint32_t)s->last;
    if (reuse)
    {
        // no sync this step: particles may have left their cells; the MAC takes boxes that hold both
        double* gc3 = s->work.get<double>("grav.geoC", 3 * (size_t)s->tree.numNodes);
        double* gs3 = s->work.get<double>("grav.geoS", 3 * (size_t)s->tree.numNodes);
        if (!gc3 || !gs3) return SX_ERR_NOMEM;
        SIM_HIP(skinRefreshBoxes(s->tree, s->x, s->y, s->z, s->dbox, gc3, gs3, st, true));
        ga.geoCenters = gc3;
        ga.geoSizes   = gs3;
    }
    ga.leafToNode = s->work.get<int32_t>("grav.leafToNode", (size_t)s->tree.numLeaves);
    ga.x = s->x, ga.y = s->y, ga.z = s->z, ga.m = s->m, ga.h = s->h;
    ga.centers4   = s->work.get<double>("grav.centers", 4 * (size_t)s->tree.numNodes);
    ga.multipoles = s->work.get<float>("grav.multipoles", 8 * (size_t)s->tree.numNodes);
    ga.ax = s->ax, ga.ay = s->ay, ga.az = s->az;
    SIM_HIP(gravityUpsweep(ga, s->tree.levelRangeHost.data(), st));
    ga.waveE = gravWaveE(s, ga.last - ga.first);
    SIM_HIP(gravityTraverse(ga, st));
    if (s->gravCheckTargets)
    {
        if (int e = gravityCheck(s, ga, st)) return e;
        s->gravCheckTargets = 0; // armed for one step
    }
    if (periodicGravity(s))
    {
        double c4[4];
        float  m8[8];
        SIM_HIP(hipMemcpyAsync(c4, ga.centers4, sizeof(c4), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(m8, ga.multipoles, sizeof(m8), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        if (int e = ewaldStep(s, c4, m8, nullptr, st)) return e;
    }
    return SX_OK;
}

int gravityStage(sx_sim* s, hipStream_t st, bool dist, bool reuse)
{
    // P2P, M2P of this step (BhStats), counted only on request (sx_sim_set_gravity_counting)
    auto* inter = s->gravCount ? gravReserveInteractions(s) : nullptr;
    if (inter) SIM_HIP(hipMemsetAsync(inter, 0, 2 * sizeof(unsigned long long), st));
    if (int e = dist ? distributedGravity(s, st, nullptr, reuse) : singleRankGravity(s, st, reuse)) return e;
    maxAccSq(s, st);
    return SX_OK;
}

} // namespace sx::sim
