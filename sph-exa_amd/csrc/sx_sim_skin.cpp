/*! @file sx_sim_skin.cpp
 * @brief The skin-list driver of sx_sim (sx_skin.hpp): the step's search through skin lists, the build decisions,
 *        the halo refresh and cover test of reuse steps on several ranks.
 */
#include "sx_sim_internal.hpp"

using namespace sx;
using namespace sx::sim;

namespace
{

/*! several ranks, a reuse step: the clusters list[1 .. list[0]] were searched again this step (a skin rebuilt from the
 *  current positions, or the exact search), over the locals and the halos of the last build only.  That search saw
 *  every particle within a target's radius only if the target's sphere lies inside its chunk's request box of that
 *  build: radius 2 r_i scale, r = hb (rebuilt skins: the h of their build, scale 1 + s) or h (exact search, scale 1).
 *  The halos are the particles that were inside the box AT THE BUILD, at their current positions.  A peer's particle p
 *  that was outside the box then and is within R of the target i now is no halo, though it is inside the box now: the
 *  sphere inside the box is not enough.  Let d_q(t) be the move of particle q in reuse step t since the build, and
 *  w(t) any vector per step.  p_build - (x_i - sum_t w(t)) = (p_now - x_i) - sum_t (d_p(t) - w(t)), so with
 *  |p_now - x_i| <= R the particle was, at the build, within R + sum_t max_q |d_q(t) - w(t)| of the centre
 *  x_i - sum_t w(t): if that sphere lies inside the box, p was inside the box at the build, hence a halo.  Every
 *  particle of every rank is in the all-reduced displacement grid, so its component ranges bound max_q.  Two choices:
 *    w = 0:      centre x_i (now), radius R + D, D = sum_t max_q |d_q(t)| (drift[0]);
 *    w = d_i(t): centre the target's position at the build, radius R + relg_i, relg_i = sum_t max_q |d_q(t) - d_i(t)|
 *                (Galilean-invariant: nothing under a uniform translation of everything; a target moving through
 *                resting peers pays for the motion once, not twice as with w = 0).
 *  A target is covered when either sphere lies inside its box.  (The filter's own relative bound, d_i + A_C, does not
 *  serve here: A_C only counts the grid cells within the largest skin radius of the cluster, and a particle coming
 *  from beyond the box starts outside them -- its first steps would be missing from the sum.  The ranges of the whole
 *  grid have no such region.)
 *  One workgroup per listed cluster; flag |= 1 when some sphere leaves its box (then every rank redoes the step from
 *  a full sync) */
__global__ void coverListKernel(const uint32_t* list, uint32_t maxList, uint32_t first, uint32_t last, const double* x,
                                const double* y, const double* z, const float* r, float scale, const ReqBox* boxes,
                                DevBox box, double qmargin, const double* drift, const double* x0, const double* y0,
                                const double* z0, const double* relg, unsigned* flag)
{
    const uint32_t k = blockIdx.x;
    if (k >= min(list[0], maxList)) return;
    const uint32_t i = first + list[1 + k] * kCluster + threadIdx.x;
    if (i >= last) return;
    const ReqBox& b  = boxes[(i - first) / kChunk];
    const double  R  = 2.0 * (double)r[i] * (double)scale * (1.0 + 1e-6) + qmargin;
    const double  Ra = R + drift[0], Rr = R + relg[i];
    const bool    outNow = fabs(foldPbc(x[i] - b.c[0], box, 0)) + Ra > b.s[0] ||
                        fabs(foldPbc(y[i] - b.c[1], box, 1)) + Ra > b.s[1] ||
                        fabs(foldPbc(z[i] - b.c[2], box, 2)) + Ra > b.s[2];
    const bool    outBuild = fabs(foldPbc(x0[i] - b.c[0], box, 0)) + Rr > b.s[0] ||
                          fabs(foldPbc(y0[i] - b.c[1], box, 1)) + Rr > b.s[1] ||
                          fabs(foldPbc(z0[i] - b.c[2], box, 2)) + Rr > b.s[2];
    if (outNow && outBuild) atomicOr(flag, 1u);
}

/*! the last position update's displacements over the all-reduced grid (every particle of every rank lies in some
 *  cell), reduced to red[0]: the largest length (per cell the length of the largest components, rounded upwards; float
 *  bits -- non-negative floats order like their bits), red[1..3]: the smallest, red[4..6]: the largest x, y, z
 *  component (ordered bits; initialised like a cell: 0xffffffff, 0 -- an empty cell changes nothing) */
__global__ void skinGridMaxKernel(const uint32_t* cells, uint32_t nc, uint32_t* red)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float          m = 0.0f;
    uint32_t       lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (i < nc && cells[i] != 0xffffffffu) // a cell without particles has no range
    {
        for (int d = 0; d < 3; ++d)
            lo[d] = cells[d * nc + i], hi[d] = cells[(3 + d) * nc + i];
        const float ex = fmaxf(fabsf(orderedFloat(lo[0])), fabsf(orderedFloat(hi[0])));
        const float ey = fmaxf(fabsf(orderedFloat(lo[1])), fabsf(orderedFloat(hi[1])));
        const float ez = fmaxf(fabsf(orderedFloat(lo[2])), fabsf(orderedFloat(hi[2])));
        m              = sqrtf(fmaf(ex, ex, fmaf(ey, ey, ez * ez))) * (1.0f + 0x1p-18f) + 1e-30f;
    }
    m = waveMax(m);
    for (int d = 0; d < 3; ++d)
        lo[d] = waveMin(lo[d]), hi[d] = waveMax(hi[d]);
    if ((threadIdx.x & 63) == 0 && m > 0.0f)
    {
        atomicMax(&red[0], __float_as_uint(m));
        for (int d = 0; d < 3; ++d)
            atomicMin(&red[1 + d], lo[d]), atomicMax(&red[4 + d], hi[d]);
    }
}

/*! the drift bounds of coverListKernel after a reuse step's grid reduction: drift[0] += the step's largest displacement;
 *  per local i, relg[i] += the largest |d_q - d_i| over the grid's component ranges, rounded upwards.  The float
 *  displacements are within 2^-24 (relative) of the moves themselves: 2^-22 of the largest covers both ends */
__global__ void skinDriftKernel(const uint32_t* red, uint32_t first, uint32_t last, const float* dx, const float* dy,
                                const float* dz, double* drift, double* relg)
{
    const uint32_t t  = blockIdx.x * blockDim.x + threadIdx.x;
    const float    mx = __uint_as_float(red[0]);
    if (t == 0) drift[0] += (double)mx * (1.0 + 1e-6);
    const uint32_t i = first + t;
    if (i >= last || red[1] == 0xffffffffu) return;
    const float ex = fmaxf(fabsf(orderedFloat(red[1]) - dx[i]), fabsf(orderedFloat(red[4]) - dx[i]));
    const float ey = fmaxf(fabsf(orderedFloat(red[2]) - dy[i]), fabsf(orderedFloat(red[5]) - dy[i]));
    const float ez = fmaxf(fabsf(orderedFloat(red[3]) - dz[i]), fabsf(orderedFloat(red[6]) - dz[i]));
    const float e  = sqrtf(fmaf(ex, ex, fmaf(ey, ey, ez * ez))) * (1.0f + 0x1p-18f) + 0x1p-22f * mx + 1e-30f;
    relg[i] += (double)e * (1.0 + 1e-6);
}

} // namespace

namespace sx::sim
{

//! skin lists serve this sim: one rank, not ve-bdt, cluster lists.  With self-gravity a reuse step traverses the last
//! sync's tree, its multipoles formed from the current positions and its MAC geometry refreshed (cells + particles).
//! Not with periodic self-gravity: between syncs a particle that crossed a periodic face is wrapped to the far side of
//! the box while it stays in its old leaf, so the leaf's multipole (raw coordinates) would spread across the box
//! while its refreshed MAC box (minimum image) covers only the old cell -- every step syncs there
//! Several ranks: the halo set of a full build is requested with the skin radius, a reuse step refreshes the halos'
//! x, y, z, h, m over the build's send lists and reduces the displacement grid over all ranks, and every decision
//! about builds is taken on all ranks together (skinHaloRefresh, the decision exchange in sx_sim_step); self-gravity
//! on a reuse step splits near and far cells against boxes of the current positions and takes MAC boxes that hold
//! each cell (node) and its drifted particles (distributedGravity with drift)
bool skinUsable(const sx_sim* s)
{
    return s->skin.factor > 0.0f && s->p.propagator != 2 && NbLists::localPossible(s->p.ngmax) &&
           !periodicGravity(s);
}

//! widest skin the adaptation goes to: skin lists (1.16)^3 = 1.56x the neighbors; wider unions outgrow the filter's LDS
//! staging (kSkinCap) in dense regions (Noh at s = 0.25: 37% of the clusters)
constexpr float kMaxSkin = 0.16f;
//! reuse steps after which a skin has paid for its build several times over: a stale-forced build before them widens it
constexpr int kShortSkin = 10;

//! a skin that did not outlast two steps: the next build takes a twice wider one; at the widest, the next steps
//! search without skin (backoff, doubling up to 32 steps)
void skinTooThin(SkinState& K)
{
    K.forceBuild = true;
    if (K.cur < kMaxSkin) K.cur = std::min(2.0f * K.cur, kMaxSkin);
    else
    {
        K.backoff    = K.backoffLen;
        K.backoffLen = std::min(2 * K.backoffLen, 32);
    }
}

//! the displacement grid over the box: kSkinGridN cells per axis
SkinGrid skinGrid(const DevBox& b)
{
    SkinGrid g{};
    g.n = kSkinGridN;
    for (int d = 0; d < 3; ++d)
    {
        g.lo[d]  = b.lim[2 * d];
        g.inv[d] = (double)kSkinGridN / b.l[d];
        g.pbc[d] = b.pbc[d];
    }
    return g;
}

//! skin-list capacity per target: the neighbor capacity scaled by the skin volume, with room for density variation
uint32_t skinCapacity(uint32_t ngmax, float factor)
{
    const double f = std::pow(1.0 + factor, 3.0) * 1.15;
    const uint32_t c = (uint32_t)std::ceil(ngmax * f);
    return std::min<uint32_t>(256u, (c + 1u) & ~1u);
}

//! per particle this step's displacement vector, per cell of the displacement grid the component ranges: written by the
//! position update, read by the next step's filter and (several ranks) reduced by skinHaloRefresh
static bool skinReserveDisp(sx_sim* s)
{
    auto& B = s->skinBuf;
    B.dx    = s->mem.get<float>("skin.dx", s->cap);
    B.dy    = s->mem.get<float>("skin.dy", s->cap);
    B.dz    = s->mem.get<float>("skin.dz", s->cap);
    B.cells = s->mem.get<uint32_t>("skin.cells", kGridWords * (size_t)kSkinGridN * kSkinGridN * kSkinGridN);
    return B.dx && B.dy && B.dz && B.cells;
}

//! several ranks: how far any particle can have moved since the build (drift[0], per local relg) and the locals'
//! positions at the build -- coverListKernel's bounds, zeroed / kept by a build, advanced by every reuse step
static bool skinReserveDrift(sx_sim* s)
{
    auto& B = s->skinBuf;
    B.drift = s->mem.get<double>("skin.drift", 8);
    B.relg  = s->mem.get<double>("skin.relg", s->cap);
    B.x0    = s->mem.get<double>("skin.x0", s->cap);
    B.y0    = s->mem.get<double>("skin.y0", s->cap);
    B.z0    = s->mem.get<double>("skin.z0", s->cap);
    return B.drift && B.relg && B.x0 && B.y0 && B.z0;
}

//! the skin arrays the position update feeds: per particle this step's displacement vector, and per cell of the grid
//! the component ranges (initialised here: the update scatters into them)
bool skinParticleBuffers(sx_sim* s, PosArgs& q, hipStream_t st)
{
    const size_t nc = (size_t)kSkinGridN * kSkinGridN * kSkinGridN;
    const bool   ok = skinReserveDisp(s);
    const auto&  B  = s->skinBuf;
    q.dispX = B.dx, q.dispY = B.dy, q.dispZ = B.dz, q.cells = B.cells;
    q.grid  = skinGrid(s->dbox);
    if (!ok) return false;
    return hipMemsetAsync(q.cells, 0xff, 3 * nc * sizeof(uint32_t), st) == hipSuccess &&
           hipMemsetAsync(q.cells + 3 * nc, 0, 3 * nc * sizeof(uint32_t), st) == hipSuccess;
}

//! the scratch of one skin search over ncl clusters (sloc is sized by K.ngmaxS, which changes at a build)
static bool skinReserveSearch(sx_sim* s, const NsArgs& na, uint32_t ncl, bool twoSets)
{
    auto&      B    = s->skinBuf;
    auto&      M    = s->mem;
    const bool disp = skinReserveDisp(s);
    B.rel     = M.get<float>("skin.rel", s->cap);
    B.sloc    = M.get<uint32_t>("skin.sloc", na.numGroups * (size_t)nlocWords(s->skin.ngmaxS) * kWave);
    B.scnt    = M.get<uint32_t>("skin.scnt", s->cap);
    B.hb      = M.get<float>("skin.hb", s->cap);
    B.acc     = M.get<float>("skin.acc", ncl);
    B.ucountS = M.get<uint32_t>("skin.ucount", ncl);
    B.l1      = M.get<uint32_t>("skin.l1", ncl + 1);
    B.l2      = M.get<uint32_t>("skin.l2", ncl + 1);
    B.l3      = M.get<uint32_t>("skin.l3", ncl + 1);
    B.dec     = M.get<uint8_t>("skin.dec", ncl);
    B.host    = M.pinned<uint32_t>("skin.host", 4);
    B.streak  = M.get<uint8_t>("skin.streak", ncl);
    B.hitmask = M.get<uint32_t>("skin.hitmask", na.numGroups * (size_t)kSkinMaskWords * kWave);
    B.same    = M.get<uint8_t>("skin.same", ncl);
    B.frz     = M.get<float2>("skin.frz", ncl);
    // the second set of exact lists (SkinArgs::nlocB): its union in the slot's second quarter, below the skin union
    B.nlocB    = twoSets ? M.get<uint32_t>("skin.nlocB", na.numGroups * (size_t)nlocWords(na.ngmax) * kWave) : nullptr;
    B.ucountB  = twoSets ? M.get<uint32_t>("skin.ucountB", ncl) : nullptr;
    B.hitmaskB = twoSets ? M.get<uint32_t>("skin.hitmaskB", na.numGroups * (size_t)kSkinMaskWords * kWave) : nullptr;
    return disp && B.rel && B.sloc && B.scnt && B.hb && B.acc && B.ucountS && B.l1 && B.l2 && B.l3 && B.dec && B.host &&
           B.streak && B.hitmask && B.same && B.frz && (!twoSets || (B.nlocB && B.ucountB && B.hitmaskB));
}

/*! The step's neighbor search through skin lists (sx_skin.hpp).  A full build (after a full sync) builds every
 *  cluster's skin and filters it; a reuse step only filters.  Stale clusters are rebuilt at once on node boxes refreshed
 *  from the current positions (reuse steps) and filtered; clusters stale again take the exact search (on a reuse step
 *  over the refreshed boxes: should it outgrow a capacity there, kSkinResync makes the caller restore h and redo the
 *  step's search from a full sync).  na: the step's search arguments (exact lists, h, nc, tree).  One host read of the
 *  stale count, two or three when some cluster is stale. */
int skinSearch(sx_sim* s, const NsArgs& na, bool reuse, hipStream_t st, float* xmOut, RecT* rtXm, SkinCounts& out)
{
    auto&          K   = s->skin;
    const uint32_t ncl = (na.numGroups + kClusterWaves - 1) / kClusterWaves;
    out                = SkinCounts{};
    out.clusters       = ncl;
    if (!reuse) K.built = K.cur; // (also with no local cluster: every rank's skin state stays the same)
    if (!ncl) return SX_OK;
    if (!reuse) K.ngmaxS = skinCapacity(s->p.ngmax, K.built);
    const bool twoSets = na.ucap / 4 >= (uint32_t)kSkinCap;
    if (!skinReserveSearch(s, na, ncl, twoSets)) return SX_ERR_NOMEM;
    const SkinBuffers& B = s->skinBuf;
    uint32_t *const l1 = B.l1, *const l2 = B.l2, *const l3 = B.l3, *const hl = B.host;
    uint32_t* const hmask = B.hitmask, *const nlocB = B.nlocB;
    uint8_t* const  same  = B.same;
    float2* const   frz   = B.frz;

    const SkinGrid g = skinGrid(s->dbox);
    SkinArgs fa{};
    fa.first = na.first, fa.last = na.last, fa.numGroups = na.numGroups, fa.ngmax = na.ngmax, fa.ng0 = na.ng0;
    fa.ngmaxS = K.ngmaxS, fa.iterateH = na.iterateH, fa.skin1 = 1.0f + K.built;
    fa.x = na.x, fa.y = na.y, fa.z = na.z, fa.h = na.h, fa.m = na.m, fa.nc = na.nc, fa.rxOut = na.rxOut;
    // the skin union lives in the upper half of each cluster's union slot, the exact union (the pair kernels') at its
    // start
    const uint32_t uoff = na.ucap / 2;
    fa.nloc = na.nloc, fa.uni = na.uni, fa.ucount = na.ucount, fa.ucap = na.ucap, fa.uoff = uoff, fa.ucountS = B.ucountS;
    fa.packMax = na.packMax;
    fa.sloc = B.sloc, fa.scnt = B.scnt, fa.hb = B.hb, fa.rel = B.rel, fa.acc = B.acc, fa.cells = B.cells, fa.grid = g;
    fa.dispX = B.dx, fa.dispY = B.dy, fa.dispZ = B.dz;
    fa.xmOut = xmOut, fa.rtXm = rtXm, fa.K = s->p.K;
    K.xmFused   = xmOut != nullptr;
    K.exactList = l2;
    fa.box = na.box, fa.powTab = na.powTab, fa.stats = na.stats, fa.clStats = na.clStats;
    // exact lists kept where no target's hits changed: only over the lists, masks and flags the last skin search of
    // this simulation left (no other search or allocation since)
    fa.hitMask   = hmask;
    fa.same      = same;
    fa.nlocB = nlocB, fa.ucountB = B.ucountB, fa.hitMaskB = B.hitmaskB, fa.uoffB = na.ucap / 4;
    fa.frz       = frz;
    fa.keepLists = reuse && K.listsKept && K.keptNloc == na.nloc && K.keptUni == na.uni && K.keptMask == hmask &&
                   K.keptSame == same && K.keptFrz == frz && K.keptNlocB == nlocB;
    K.listsKept  = false; // until this search completes

    // the skin build: the search with radii 2 h (1 + s), no h iteration, skin lists and counts as its outputs
    NsArgs b   = na;
    b.skin1    = 1.0f + K.built;
    b.iterateH = 0;
    b.nloc     = B.sloc;
    b.packMax  = 0; // the skin lists stay u16
    b.ngmax    = K.ngmaxS;
    b.nc       = B.scnt;
    b.rxOut    = nullptr;
    b.uoff     = uoff;
    b.ucount   = B.ucountS;

    SIM_HIP(hipMemsetAsync(l1, 0, 4, st));
    SIM_HIP(hipMemsetAsync(l2, 0, 4, st));
    if (!reuse)
    {
        SIM_HIP(hipMemsetAsync(B.streak, 0, ncl, st));
        SIM_HIP(findNeighbors(b, st));
        fa.fresh = 1;
    }
    else fa.fresh = 0; // the grid of this step's displacements came from the last position update
    fa.list  = nullptr;
    fa.stale = l1;
    // reuse steps: a cluster stale again on the step after its rebuild goes straight to the exact search (l2)
    fa.streak = reuse ? B.streak : nullptr;
    fa.direct = reuse ? l2 : nullptr;
    if (reuse)
    {
        // decide first (every cluster: stale, frozen or walk), then the frozen clusters' XMass over their exact lists
        // and the walk of the others; a consumer's workgroup leaves at once when its cluster is not marked for it
        fa.dec = B.dec;
        fa.frozenStage = K.frozenStage ? K.frozenStage : (uint32_t)kSkinFrozenCap;
        SIM_HIP(skinDecide(fa, ncl, st));
        SIM_HIP(skinFrozen(fa, ncl, st));
    }
    SIM_HIP(skinFilter(fa, ncl, st));
    SIM_HIP(hipMemcpyAsync(hl, l1, 4, hipMemcpyDeviceToHost, st));
    SIM_HIP(hipMemcpyAsync(hl + 1, l2, 4, hipMemcpyDeviceToHost, st));
    SIM_HIP(hipStreamSynchronize(st));
    const uint32_t n1 = hl[0], nd = hl[1];
    uint32_t       n2 = nd;
    out.rebuilt = n1, out.stale = n1 + nd, out.exact = nd;
    NsArgs         x  = na; // the exact search, for clusters whose h iteration outgrows even a fresh skin
    // subset searches of a reuse step run the large build directly: on the refreshed (overlapping) boxes many of the
    // few clusters overflow the compact one, whose launch then only adds a tail (Noh -n 300: 20.4 -> 20.1 ms/step)
    NsPolicy large;
    large.mode = 1;
    if (reuse) b.policy = x.policy = &large;
    if ((n1 || nd) && reuse)
    {
        // particles have left the cells of the last full sync's tree: the walk takes boxes of the current positions
        double* c3 = s->mem.get<double>("skin.centers", 3 * (size_t)s->tree.numNodes);
        double* s3 = s->mem.get<double>("skin.sizes", 3 * (size_t)s->tree.numNodes);
        if (!c3 || !s3) return SX_ERR_NOMEM;
        SIM_HIP(skinRefreshBoxes(s->tree, na.x, na.y, na.z, na.box, c3, s3, st));
        b.centers = x.centers = c3;
        b.sizes = x.sizes = s3;
    }
    // the directly stale clusters' exact search does not depend on the rebuild of the others (disjoint clusters: their
    // lists, unions, h, nc and records; only the statistics words are shared, reduced again below): with both, it runs
    // on the auxiliary stream with its own search scratch while the rebuild and its filter run here
    const bool early = n1 && nd && reuse && s->auxStream && s->evAuxIn && s->evAuxOut;
    if (early)
    {
        NsArgs xd   = x;
        xd.subset   = l2;
        xd.work     = s->mem.get<uint32_t>("skin.aux.work", 16);
        xd.hSave    = s->mem.get<float>("skin.aux.over", ncl + 1);
        xd.hitMasks = s->mem.get<uint64_t>("skin.aux.masks", searchScratchBytes() / sizeof(uint64_t));
        // one workgroup per cluster here, the rest of the resident grid for the rebuild: a persistent rebuild grid
        // holding every slot would leave this search waiting for it
        const unsigned G = searchGrid();
        xd.maxGrid       = std::min(nd, G / 2);
        b.maxGrid        = G - xd.maxGrid;
        if (!xd.work || !xd.hSave || !xd.hitMasks) return SX_ERR_NOMEM;
        SIM_HIP(hipEventRecord(s->evAuxIn, st));
        SIM_HIP(hipStreamWaitEvent(s->auxStream, s->evAuxIn, 0));
        SIM_HIP(findNeighbors(xd, s->auxStream));
        SIM_HIP(hipEventRecord(s->evAuxOut, s->auxStream));
    }
    uint32_t* lx = l2; // the exact search's list below: l2 (the direct clusters, then those stale after the rebuild)
    if (n1)
    {
        b.subset  = l1;
        SIM_HIP(findNeighbors(b, st));
        fa.fresh  = 1;
        fa.list   = l1;
        // appended after the direct ones, or (their search already running) a list of their own
        if (early) SIM_HIP(hipMemsetAsync(l3, 0, 4, st));
        fa.stale  = early ? l3 : l2;
        fa.streak = nullptr;
        fa.direct = nullptr;
        fa.dec    = nullptr;
        SIM_HIP(skinFilter(fa, ncl, st));
        SIM_HIP(hipMemcpyAsync(hl + 2, fa.stale, 4, hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        n2 = hl[2];
    }
    uint32_t n3 = 0; // early: the clusters stale after the rebuild (l3), searched below
    if (early)
    {
        n3 = n2, n2 = nd + n3, lx = l3;
        K.earlyExact += nd;
        SIM_HIP(hipStreamWaitEvent(st, s->evAuxOut, 0));
    }
    out.exact = n2;
    {
        if (early ? n3 : n2)
        {
            x.subset = lx;
            SIM_HIP(findNeighbors(x, st));
        }
        if (early)
        {
            // one list of every exact-search cluster (XMass, skinMarkStale): l3's entries after the direct ones
            if (n3) SIM_HIP(hipMemcpyAsync(l2 + 1 + nd, l3 + 1, 4 * (size_t)n3, hipMemcpyDeviceToDevice, st));
            hl[3] = n2;
            SIM_HIP(hipMemcpyAsync(l2, hl + 3, 4, hipMemcpyHostToDevice, st)); // read by the synchronisation below
        }
        if (n2)
        {
            if (reuse)
            {
                // on a reuse step the walk takes the drifted tree's refreshed boxes, which overlap: should the exact
                // search outgrow its capacities there, the step's search is redone from a full sync
                SIM_HIP(hipMemcpyAsync(hl, na.stats + kStatFlags, 4, hipMemcpyDeviceToHost, st));
                SIM_HIP(hipStreamSynchronize(st));
                if (hl[0] & kFlagError)
                {
                    SIM_HIP(hipMemsetAsync(na.stats + kStatFlags, 0, 4, st));
                    return kSkinResync;
                }
            }
            SIM_HIP(skinMarkStale(l2, ncl, B.acc, st)); // their skins are rebuilt next step
        }
    }
    SIM_HIP(reduceClusterStats(na.clStats, ncl, na.stats, st));
    K.listsKept = true, K.keptNloc = na.nloc, K.keptUni = na.uni, K.keptMask = hmask, K.keptSame = same, K.keptFrz = frz;
    K.keptNlocB = nlocB;
    // the pair kernels read each cluster's current set
    K.lb = twoSets ? ListsB{same, nlocB, B.ucountB, na.ucap / 4} : ListsB{};
    return SX_OK;
}

/*! the skin's bookkeeping after a step's search: statistics of this rank, and the build decisions from the stale share
 *  of all ranks (staleAll of clustersAll: with several ranks the sums over every rank, so that every rank takes the
 *  same decisions and the next step is a full sync + build on all of them or on none) */
void skinBookkeeping(SkinState& K, bool reuse, const SkinCounts& c, uint64_t staleAll, uint64_t clustersAll)
{
    K.lastStale = c.stale, K.lastExact = c.exact;
    K.staleClusters += c.stale, K.exactClusters += c.exact;
    if (reuse)
    {
        K.reuseSteps++;
        K.sinceBuild++;
    }
    else
    {
        K.builds++;
        K.valid      = true;
        K.forceBuild = false;
        K.sinceBuild = 0;
    }
    // many clusters rebuilt one by one: the next step syncs (SFC order restored) and builds them all at once.  A
    // stale-heavy step costs about a build; a skin with fewer than two clean reuse steps since its build saved
    // nothing, so the next steps search without it (backoff, doubling up to 32 steps with every such skin)
    const bool clean = (double)staleAll <= K.staleLimit * (double)clustersAll;
    if (!reuse) K.cleanSinceBuild = 0;
    else if (clean) K.cleanSinceBuild++;
    if (!clean)
    {
        K.forceBuild = true;
        if (!reuse || K.cleanSinceBuild < 2) skinTooThin(K);
        // a skin used up by the flow in fewer than kShortSkin steps (Noh's shock at s = 0.05: a full build every ~6
        // steps) is widened a little for the next build; one that lasts until maxReuse (Sedov) stays as it is
        else if (K.sinceBuild < kShortSkin) K.cur = std::min(1.25f * K.cur, kMaxSkin);
    }
    if (clean && K.cleanSinceBuild >= 2) K.backoffLen = 4;
}

//! a reuse step with several ranks: the halos of the last build get their owners' current x, y, z, h, m over the
//! build's send lists (the particles stay where they are: no exchange to the SFC owners until the next build), and
//! the displacement grid of the last position update becomes the grid of every rank's particles (u32 min / max of the
//! ordered-float component ranges): a particle that was no halo at the build can only reach a target's 2h sphere
//! through the region around its cluster, where its steps now count in the filter's drift bound (sx_skin.hpp)
int skinHaloRefresh(sx_sim* s, hipStream_t st)
{
    if (int e = haloExchange(s, {{s->x, 8}, {s->y, 8}, {s->z, 8}, {s->h, 4}, {s->m, 4}}, st)) return e;
    const size_t nc = (size_t)kSkinGridN * kSkinGridN * kSkinGridN;
    const auto&  B  = s->skinBuf;
    if (!skinReserveDisp(s)) return SX_ERR_NOMEM;
    SIM_COMM(s->comm->allreduceMinU32(B.cells, 3 * nc, st));
    SIM_COMM(s->comm->allreduceMaxU32(B.cells + 3 * nc, 3 * nc, st));
    // how far any particle of any rank can have moved since the build (coverListKernel's D)
    if (!skinReserveDrift(s)) return SX_ERR_NOMEM;
    uint32_t* red = reinterpret_cast<uint32_t*>(B.drift + 2); // 7 words
    SIM_HIP(hipMemsetAsync(red, 0, 7 * 4, st));
    SIM_HIP(hipMemsetAsync(red + 1, 0xff, 3 * 4, st));
    skinGridMaxKernel<<<grid(nc), 256, 0, st>>>(B.cells, (uint32_t)nc, red);
    const size_t nl = s->last - s->first;
    skinDriftKernel<<<std::max(1u, grid(nl)), 256, 0, st>>>(red, (uint32_t)s->first, (uint32_t)s->last, B.dx, B.dy, B.dz,
                                                           B.drift, B.relg);
    SIM_HIP(hipGetLastError());
    return SX_OK;
}

int skinBuildSnapshot(sx_sim* s, hipStream_t st)
{
    // the halo set is this sync's: no particle has moved since
    if (!skinReserveDrift(s)) return SX_ERR_NOMEM;
    const auto&  B  = s->skinBuf;
    const size_t f0 = s->first, nl0 = s->last - s->first;
    SIM_HIP(hipMemsetAsync(B.drift, 0, 8 * sizeof(double), st));
    SIM_HIP(hipMemsetAsync(B.relg + f0, 0, nl0 * sizeof(double), st));
    double*       p0[3] = {B.x0, B.y0, B.z0};
    const double* pc[3] = {s->x, s->y, s->z};
    for (int d = 0; d < 3; ++d)
        SIM_HIP(hipMemcpyAsync(p0[d] + f0, pc[d] + f0, nl0 * sizeof(double), hipMemcpyDeviceToDevice, st));
    return SX_OK;
}

int skinCoverCheck(sx_sim* s, const SkinCounts& c, unsigned* flag, hipStream_t st)
{
    // (skinHaloRefresh: this step's drift bounds; skinBuildSnapshot: the build's positions)
    const auto& B = s->skinBuf;
    if (!B.drift || !B.relg || !B.x0 || !B.y0 || !B.z0) return SX_ERR_NOMEM;
    const double   qm    = quantMargin(s->dbox);
    const uint32_t first = (uint32_t)s->first, last = (uint32_t)s->last;
    if (c.rebuilt)
        coverListKernel<<<c.rebuilt, kCluster, 0, st>>>(B.l1, c.rebuilt, first, last, s->x, s->y, s->z, B.hb,
                                                        1.0f + s->skin.built, s->dom.mybox, s->dbox, qm, B.drift, B.x0,
                                                        B.y0, B.z0, B.relg, flag);
    if (c.exact)
        coverListKernel<<<c.exact, kCluster, 0, st>>>(B.l2, c.exact, first, last, s->x, s->y, s->z, s->h, 1.0f,
                                                      s->dom.mybox, s->dbox, qm, B.drift, B.x0, B.y0, B.z0, B.relg, flag);
    return SX_OK;
}

//! XMass of the step: all clusters, or after a filter that computed it only the exact-search clusters
void xmassRest(sx_sim* s, const HydroLaunch& H, PairArgs a, hipStream_t st)
{
    if (!s->skin.xmFused) return H.xmass(a, st);
    if (!s->skin.lastExact) return;
    a.clusterList = s->skin.exactList + 1;
    a.listCount   = s->skin.lastExact;
    H.xmass(a, st);
}

} // namespace sx::sim
