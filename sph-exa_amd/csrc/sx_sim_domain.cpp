/*! @file sx_sim_domain.cpp
 * @brief The SFC domain of sx_sim: local sort, the distributed sync (particle exchange, halo discovery), halo
 *        exchanges and the decisions the ranks take together.  The design is described at the top of sx_sim.cpp.
 */
#include "sx_sim_internal.hpp"

using namespace sx;
using namespace sx::sim;

namespace
{

//! particle record of the SFC exchange (conserved fields of the VE propagator, ve_hydro.hpp:74)
struct __attribute__((aligned(16))) PRec
{
    double   x, y, z, temp;
    float    h, m, vx, vy, vz, xm1, ym1, zm1, dum1, alpha;
    uint64_t id;
};
static_assert(sizeof(PRec) == 80, "PRec layout");

// ---- domain decomposition kernels -------------------------------------------------------------------------

__global__ void histKernel(const uint64_t* keys, size_t n, uint32_t* bins)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&bins[keys[i] >> (63 - kHistBits)], 1u);
}

//! out[q] = first local key >= split[q] (out[0] = 0, out[P] = n: the whole range is assigned)
__global__ void lowerBoundsKernel(const uint64_t* keys, size_t n, const uint64_t* split, int P, uint64_t* out)
{
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > P) return;
    uint64_t v  = split[q];
    size_t   lo = 0, hi = n;
    while (lo < hi)
    {
        size_t mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    out[q] = q == 0 ? 0 : (q == P ? n : lo);
}

//! per peer count = difference of consecutive segment boundaries (u64 or u32), into the count-exchange buffer
__global__ void diffCountsKernel(const uint64_t* b64, const uint32_t* b32, int P, uint64_t* out)
{
    int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    out[q] = b64 ? b64[q + 1] - b64[q] : (uint64_t)(b32[q + 1] - b32[q]);
}

__global__ void packPRecKernel(Fields f, size_t n, PRec* out)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    // ve-bdt: the rung rides in the top byte of the id slot (particle ids < 2^56)
    const uint64_t id = f.rung ? (f.id[i] | (uint64_t)f.rung[i] << 56) : f.id[i];
    // the gravity-only propagator has no temp, du_m1, alpha (null members): their slots travel as zeros
    const double temp = f.temp ? f.temp[i] : 0.0;
    const float  dum1 = f.dum1 ? f.dum1[i] : 0.0f, alpha = f.alpha ? f.alpha[i] : 0.0f;
    out[i] = PRec{f.x[i],   f.y[i],   f.z[i],   temp,     f.h[i], f.m[i], f.vx[i], f.vy[i],
                  f.vz[i],  f.xm1[i], f.ym1[i], f.zm1[i], dum1,   alpha,  id};
}

__global__ void unpackPRecKernel(const PRec* in, size_t n, Fields f)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    PRec r    = in[i];
    f.x[i]    = r.x;
    f.y[i]    = r.y;
    f.z[i]    = r.z;
    if (f.temp) f.temp[i] = r.temp;
    f.h[i]    = r.h;
    f.m[i]    = r.m;
    f.vx[i]   = r.vx;
    f.vy[i]   = r.vy;
    f.vz[i]   = r.vz;
    f.xm1[i]  = r.xm1;
    f.ym1[i]  = r.ym1;
    f.zm1[i]  = r.zm1;
    if (f.dum1) f.dum1[i] = r.dum1;
    if (f.alpha) f.alpha[i] = r.alpha;
    f.id[i]   = f.rung ? r.id & ((1ull << 56) - 1) : r.id;
    if (f.rung) f.rung[i] = (uint8_t)(r.id >> 56);
}

//! request box of every kChunk SFC-consecutive local particles: AABB grown by 2*hmax*margin + quantisation margin
__global__ void chunkBoxKernel(const double* x, const double* y, const double* z, const float* h, size_t n,
                               double margin, double qmargin, int owner, ReqBox* out)
{
    const size_t c0   = (size_t)blockIdx.x * kChunk;
    const size_t c1   = min(n, c0 + kChunk);
    double       lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float        hm   = 0;
    for (size_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
    {
        lo[0] = fmin(lo[0], x[i]), hi[0] = fmax(hi[0], x[i]);
        lo[1] = fmin(lo[1], y[i]), hi[1] = fmax(hi[1], y[i]);
        lo[2] = fmin(lo[2], z[i]), hi[2] = fmax(hi[2], z[i]);
        hm    = fmaxf(hm, h[i]);
    }
    __shared__ double s[6][4];
    __shared__ float  sh[4];
    for (int k = 0; k < 3; ++k)
    {
        lo[k] = waveMin(lo[k]);
        hi[k] = waveMax(hi[k]);
    }
    hm = waveMax(hm);
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
    {
        for (int k = 0; k < 3; ++k)
            s[k][w] = lo[k], s[3 + k][w] = hi[k];
        sh[w] = hm;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        int nw = blockDim.x >> 6;
        for (int v = 1; v < nw; ++v)
            for (int k = 0; k < 3; ++k)
                s[k][0] = fmin(s[k][0], s[k][v]), s[3 + k][0] = fmax(s[3 + k][0], s[3 + k][v]), sh[0] = fmaxf(sh[0], sh[v]);
        ReqBox b;
        double R = 2.0 * (double)sh[0] * margin + qmargin;
        for (int k = 0; k < 3; ++k)
        {
            b.c[k] = 0.5 * (s[k][0] + s[3 + k][0]);
            b.s[k] = 0.5 * (s[3 + k][0] - s[k][0]) + R;
        }
        b.hmax  = sh[0];
        b.owner = owner;
        b.pad   = 0;
        out[blockIdx.x] = b;
    }
}

//! 1 if some particle of the chunk grew beyond the chunk's request radius during the h iteration
__global__ void chunkCheckKernel(const float* h, size_t n, const ReqBox* boxes, double margin, unsigned* flag)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ReqBox& b = boxes[i / kChunk];
    if ((double)h[i] > b.hmax * margin) atomicOr(flag, 1u);
}

/*! 1 if some local's search sphere (2h around its current position) leaves its chunk's request box (minimum image):
 *  the peers sent every particle inside that box, so a sphere inside it sees all of them.  Unlike chunkCheckKernel
 *  this also covers the drift of the locals inside a ve-bdt hierarchy. */
__global__ void chunkCoverKernel(const double* x, const double* y, const double* z, const float* h, size_t n,
                                 const ReqBox* boxes, DevBox box, double qmargin, unsigned* flag)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ReqBox& b = boxes[i / kChunk];
    const double  r = 2.0 * (double)h[i] * (1.0 + 1e-6) + qmargin;
    const bool    out = fabs(foldPbc(x[i] - b.c[0], box, 0)) + r > b.s[0] || fabs(foldPbc(y[i] - b.c[1], box, 1)) + r > b.s[1] ||
                     fabs(foldPbc(z[i] - b.c[2], box, 2)) + r > b.s[2];
    if (out) atomicOr(flag, 1u);
}

/*! one wave per peer request box: traverse the local tree, mark local particles inside the box (minimum image)
 *  for the box owner.  mark: one bit per rank (<= 64 ranks). */
__global__ __launch_bounds__(256) void markHalosKernel(const ReqBox* boxes, int numBoxes, const int32_t* childOffsets,
                                                       const int32_t* internalToLeaf, const uint32_t* layout,
                                                       const double* centers, const double* sizes, const double* x,
                                                       const double* y, const double* z, DevBox box, double qmargin,
                                                       unsigned long long* mark, uint32_t* err)
{
    __shared__ int s_queue[4][kQCap];
    constexpr int  kCCap = 2048; // candidate leaves per wave of the halo discovery
    __shared__ int s_cand[4][kCCap];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bi   = blockIdx.x * 4 + wave;
    if (bi >= numBoxes) return;
    const ReqBox b = boxes[bi];
    bool         overflow;
    const int    numCand = waveCollectLeaves<kCCap>(
        childOffsets,
        [&](int node) {
            return boxDist2(centers + 3 * (size_t)node, sizes + 3 * (size_t)node, b.c[0], b.c[1], b.c[2],
                            b.s[0] + qmargin, b.s[1] + qmargin, b.s[2] + qmargin, box) <= 0.0;
        },
        s_queue[wave], s_cand[wave], lane, overflow);
    if (overflow && lane == 0) atomicOr(err, 1u);
    const unsigned long long bit = 1ull << b.owner;
    for (int c = 0; c < numCand; ++c)
    {
        const int      node = __builtin_amdgcn_readfirstlane(s_cand[wave][c]);
        const int      leaf = internalToLeaf[node];
        const uint32_t p0 = layout[leaf], p1 = layout[leaf + 1];
        for (uint32_t p = p0 + lane; p < p1; p += 64)
        {
            double d0 = fabs(foldPbc(x[p] - b.c[0], box, 0));
            double d1 = fabs(foldPbc(y[p] - b.c[1], box, 1));
            double d2 = fabs(foldPbc(z[p] - b.c[2], box, 2));
            if (d0 <= b.s[0] && d1 <= b.s[1] && d2 <= b.s[2]) atomicOr(&mark[p], bit);
        }
    }
}

//! send flags of every peer at once: segment q of (n + 1) entries holds bit q of each particle's mark (0 for q == r
//! and for the segment's closing entry), so one exclusive scan numbers the send lists of all peers in peer order
//! send flags of peers [q0, q0 + Pb): one segment of n + 1 flags per peer (the extra 0 makes the scan's last entry
//! the batch total)
__global__ void maskFlagsKernel(const unsigned long long* mark, size_t n, int q0, int Pb, int r, uint32_t* flag)
{
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= (size_t)Pb * (n + 1)) return;
    const size_t j = k / (n + 1), i = k - j * (n + 1);
    const int    q = q0 + (int)j;
    flag[k]        = (i < n && q != r) ? (uint32_t)((mark[i] >> q) & 1ull) : 0u;
}

__global__ void scatterIdxKernel(const uint32_t* flag, const uint32_t* scan, size_t n, int Pb, uint64_t base,
                                 uint32_t* out)
{
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k < (size_t)Pb * (n + 1) && flag[k]) out[base + scan[k]] = (uint32_t)(k % (n + 1));
}

//! start of every peer's send list in the scan (P entries) and the total (entry P)
__global__ void segStartsKernel(const uint32_t* scan, size_t n, int P, uint32_t* out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= P) out[q] = scan[q < P ? (size_t)q * (n + 1) : (size_t)P * (n + 1) - 1];
}

//! interior / boundary clusters: a cluster is interior when no entry of its neighbor union is a halo (outside
//! [first, last)).  One wave per cluster; the lists are compacted with one atomic per cluster (order is free: every
//! cluster is computed independently)
__global__ void classifyClustersKernel(const uint32_t* uni, const uint32_t* ucount, uint32_t ucap, ListsB lb,
                                       uint32_t first, uint32_t last, uint32_t numClusters, uint32_t* lists,
                                       uint32_t* counts)
{
    const uint32_t c    = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63;
    if (c >= numClusters) return;
    // an overflowed union (ucount > ucap, stats bit 8, reported as an error after the step) is only partly stored:
    // read what is there and treat the cluster as boundary
    const bool      lB = listsB(lb, c);
    const uint32_t  uc = lB ? lb.ucount[c] : ucount[c];
    const uint32_t  U  = min(uc, ucap);
    const uint32_t* u  = uni + (size_t)c * ucap + (lB ? lb.uoff : 0u);
    bool            halo = uc > ucap;
    for (uint32_t k = lane; k < U; k += 64)
    {
        const uint32_t j = u[k];
        halo |= j < first || j >= last;
    }
    const bool any = __ballot(halo) != 0ull;
    if (lane == 0)
    {
        const uint32_t pos = atomicAdd(&counts[any ? 1 : 0], 1u);
        lists[(any ? numClusters : 0u) + pos] = c;
    }
}

} // namespace

namespace sx::sim
{

double quantMargin(const DevBox& b)
{
    return 4.0 * std::max(b.l[0], std::max(b.l[1], b.l[2])) / double(1u << kMaxLevel);
}

bool domReserveComm(sx_sim* s, size_t P)
{
    auto& D     = s->dom;
    D.bins      = s->work.get<uint32_t>("dom.bins", size_t(1) << kHistBits);
    D.split     = s->work.get<uint64_t>("dom.split", P + 1);
    D.seg       = s->work.get<uint64_t>("dom.seg", P + 1);
    s->cntBuf   = s->work.get<uint64_t>("dom.cnt", 2 * P);
    D.cnth      = s->work.pinned<uint64_t>("dom.cnth", 2 * P);
    D.agree     = s->work.get<uint32_t>("dom.agree", 1);
    D.agreeh    = s->work.pinned<uint32_t>("dom.agreeh", 1);
    D.hflag     = s->work.get<unsigned>("dom.hflag", 5);
    D.hflagh    = s->work.pinned<unsigned>("dom.hflagh", 1);
    D.errh      = s->work.pinned<uint32_t>("dom.errh", 1);
    return D.bins && D.split && D.seg && s->cntBuf && D.cnth && D.agree && D.agreeh && D.hflag && D.hflagh && D.errh;
}

void diffCounts(const uint64_t* b64, const uint32_t* b32, int P, uint64_t* out, hipStream_t st)
{
    diffCountsKernel<<<grid(P, 64), 64, 0, st>>>(b64, b32, P, out);
}

void chunkBoxes(const double* x, const double* y, const double* z, const float* h, size_t n, size_t nChunks,
                double margin, double qmargin, int owner, ReqBox* out, hipStream_t st)
{
    chunkBoxKernel<<<(unsigned)nChunks, 256, 0, st>>>(x, y, z, h, n, margin, qmargin, owner, out);
}

void chunkCheck(sx_sim* s, double margin, unsigned* flag, hipStream_t st)
{
    const size_t nl = s->last - s->first;
    if (nl) chunkCheckKernel<<<grid(nl), 256, 0, st>>>(s->h + s->first, nl, s->dom.mybox, margin, flag);
}

int classifyClusters(sx_sim* s, hipStream_t st)
{
    const uint32_t ncl = (uint32_t)((s->last - s->first + kCluster - 1) / kCluster);
    s->clsList         = s->work.get<uint32_t>("ovl.list", 2 * (size_t)std::max(1u, ncl));
    s->clsCount        = s->work.get<uint32_t>("ovl.count", 2);
    SIM_HIP(hipMemsetAsync(s->clsCount, 0, 8, st));
    if (ncl)
        classifyClustersKernel<<<(ncl + 3) / 4, 256, 0, st>>>(s->nb.uni, s->nb.ucount, s->nb.ucap, s->skin.lb,
                                                             (uint32_t)s->first, (uint32_t)s->last, ncl, s->clsList,
                                                             s->clsCount);
    SIM_HIP(hipMemcpyAsync(s->clsHost, s->clsCount, 8, hipMemcpyDeviceToHost, st));
    return SX_OK;
}

//! sort the local particles [0,nl) of the primary arrays by key (keys[0..nl) computed) via the spare buffers
/*! SFC order of the locals, identical to the reference's stable sort of the full keys (Domain::sync):
 *  - keys already ascending (no descent): the stable sort is the identity, nothing moves;
 *  - else a stable radix sort of the top sortBits key bits, accepted when the result is ascending in the full keys
 *    (then keys equal in the sorted bits kept their input order AND that order is ascending in the lower bits, which
 *    is what the full stable sort gives); otherwise the full sort, and more bits from the next step on.
 *  Lattice-like states separate every particle within the top 10 levels (30 bits), so 4 of the 8 radix passes.
 *  Up to 32 bits the sort moves 32-bit keys (the top bits, extracted by the descent count) and an implicit identity
 *  permutation: 8 instead of 12 bytes per element and pass; the full keys are then reordered with the other fields
 *  (only the moved positions), instead of being copied back from the sort's output. */
int sortLocals(sx_sim* s, size_t nl, hipStream_t st)
{
    uint32_t* cnt  = s->work.get<uint32_t>("sort.desc", 2);
    uint32_t* cntH = s->work.pinned<uint32_t>("sort.desch", 2);
    auto      read = [&]() -> int {
        SIM_HIP(hipMemcpyAsync(cntH, cnt, 8, hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        return SX_OK;
    };
    const int bits = std::clamp(s->sortBits, 1, 63);
    uint32_t* top  = bits <= 32 ? s->work.get<uint32_t>("sort.top", nl) : nullptr;
    SIM_HIP(hipMemsetAsync(cnt, 0, 8, st));
    if (top) SIM_HIP(countDescentsTop(s->keys, nl, 63 - bits, top, cnt, st));
    else SIM_HIP(countDescents(s->keys, nl, cnt, st));
    if (int e = read()) return e;
    s->sortStats[0]++;
    if (cntH[0] == 0) return SX_OK;
    hipError_t he          = hipSuccess;
    bool       permuteKeys = false; // the order is final and the keys are reordered with the fields
    uint32_t   moved       = 0;
    if (top)
    {
        SIM_HIP(sortTopBits(s->work, top, s->order, nl, bits, st));
        SIM_HIP(hipMemsetAsync(cnt, 0, 8, st));
        SIM_HIP(checkSorted(s->keys, s->order, nl, cnt, st));
        if (int e = read()) return e;
        permuteKeys = cntH[0] == 0;
        moved       = cntH[1];
    }
    if (!permuteKeys)
    {
        uint64_t* kOut = nullptr;
        if (!top && bits < 63)
        {
            kOut = sortKeysBits(s->work, s->keys, s->order, nl, 63 - bits, st, he);
            SIM_HIP(he);
            SIM_HIP(hipMemsetAsync(cnt, 0, 8, st));
            SIM_HIP(countDescents(kOut, nl, cnt, st));
            if (int e = read()) return e;
            if (cntH[0]) kOut = nullptr;
        }
        if (!kOut)
        {
            kOut = sortKeysBits(s->work, s->keys, s->order, nl, 0, st, he);
            SIM_HIP(he);
            if (bits < 63)
            {
                s->sortBits = std::min(63, bits + 9);
                s->sortStats[2]++;
            }
        }
        SIM_HIP(hipMemcpyAsync(s->keys, kOut, nl * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        SIM_HIP(hipMemsetAsync(cnt, 0, 8, st));
        SIM_HIP(movedCount(s->order, nl, cnt, st));
        if (int e = read()) return e;
        moved = cntH[0];
    }
    s->sortStats[1]++;
    // a nearly stationary state moves few positions per step (Sedov 64M: ~10 %): then only those are rewritten, in
    // place (read into a scratch copy, then written back), instead of gathering every field into its spare buffer
    if (moved <= nl / 4)
    {
        size_t colBytes = permuteKeys ? ((size_t)nl * sizeof(uint64_t) + 255) & ~size_t(255) : 0;
        for (auto& sp : s->spares)
            colBytes += ((size_t)nl * sp.elemBytes + 255) & ~size_t(255);
        char*     tmp = s->work.get<char>("sort.movedtmp", colBytes);
        GatherSet set{};
        auto      add = [&](void* field, int bytes) -> int {
            if (set.count == kMaxGatherFields)
            {
                SIM_HIP(permuteMoved(s->order, nl, set, tmp, st));
                set.count = 0;
            }
            set.src[set.count] = field, set.dst[set.count] = field, set.bytes[set.count] = bytes;
            ++set.count;
            return SX_OK;
        };
        if (permuteKeys)
            if (int e = add(s->keys, sizeof(uint64_t))) return e;
        for (auto& sp : s->spares)
            if (int e = add(*sp.field, sp.elemBytes)) return e;
        SIM_HIP(permuteMoved(s->order, nl, set, tmp, st));
        s->sortStats[3]++;
        return SX_OK;
    }
    GatherSet set{};
    auto      add = [&](const void* src, void* dst, int bytes) -> int {
        if (set.count == kMaxGatherFields)
        {
            SIM_HIP(gatherMany(s->order, nl, set, st));
            set.count = 0;
        }
        set.src[set.count] = src, set.dst[set.count] = dst, set.bytes[set.count] = bytes;
        ++set.count;
        return SX_OK;
    };
    uint64_t* kOut = permuteKeys ? s->work.get<uint64_t>("sort.kout", nl) : nullptr;
    if (kOut)
        if (int e = add(s->keys, kOut, sizeof(uint64_t))) return e;
    for (auto& sp : s->spares)
    {
        if (int e = add(*sp.field, sp.alt, sp.elemBytes)) return e;
        std::swap(*sp.field, sp.alt);
    }
    SIM_HIP(gatherMany(s->order, nl, set, st));
    if (kOut) SIM_HIP(hipMemcpyAsync(s->keys, kOut, nl * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    return SX_OK;
}

//! RecX of the halos [0, first) and [last, n): the search wrote the locals' records (NsArgs::rxOut)
void packXHalos(sx_sim* s, hipStream_t st)
{
    if (s->first) packX(s->first, s->x, s->y, s->z, s->h, s->m, s->rx, st);
    if (s->n > s->last)
        packX(s->n - s->last, s->x + s->last, s->y + s->last, s->z + s->last, s->h + s->last, s->m + s->last,
              s->rx + s->last, st);
}

//! exchange one set of fields for the halos of this step (send lists built by discoverHalos)
int haloExchange(sx_sim* s, std::initializer_list<std::pair<void*, int>> fields, hipStream_t st)
{
    if (!s->comm || s->comm->size() == 1) return SX_OK;
    const int P = s->comm->size();
    for (auto [ptr, es] : fields)
    {
        char* f   = static_cast<char*>(ptr);
        char* buf = s->work.get<char>("halo.send", std::max<uint64_t>(1, s->numSend) * 8);
        if (s->numSend) SIM_HIP(gather(s->sendIdx, s->numSend, f + s->first * es, buf, es, st));
        std::vector<uint64_t> sb(P), so(P), rb(P), ro(P);
        for (int q = 0; q < P; ++q)
        {
            sb[q] = s->haloSend[q] * es;
            so[q] = s->haloSendOff[q] * es;
            rb[q] = s->haloRecv[q] * es;
            ro[q] = s->haloRecvOff[q] * es;
        }
        SIM_COMM(s->comm->alltoallv(buf, sb.data(), so.data(), f, rb.data(), ro.data(), st));
    }
    return SX_OK;
}

//! whether this step's exchanges overlap with interior clusters (several ranks, cluster lists, not disabled)
bool overlapping(const sx_sim* s, const HydroLaunch& H)
{
    return s->comm && s->comm->size() > 1 && s->overlap && s->nb.local && s->commStream && H.clusterLists;
}

/*! distributed sync: SFC assignment, particle exchange, halo discovery + setup exchange, combined tree.
 *  On entry the local particles are [first,last); on exit [first,last) again with halos around them. */
int anyRank(sx_sim* s, bool bad, hipStream_t st, bool& out);

//! a count exchange that doubles as a collective abort: a rank that cannot go on (capacity, scratch) sends
//! kAbortCount to every peer, so all ranks leave the sync at the same exchange (SX_ERR_NOMEM) instead of the others
//! waiting in the next collective; no extra host round trip
constexpr uint64_t kAbortCount = ~0ull;
int countsOrAbort(sx_sim* s, std::vector<uint64_t>& send, std::vector<uint64_t>& recv, bool fail, hipStream_t st)
{
    if (fail) send.assign(send.size(), kAbortCount);
    SIM_COMM(s->comm->exchangeCounts(send, recv, st, s->cntBuf));
    bool abort = fail;
    for (uint64_t c : recv)
        abort |= c == kAbortCount;
    return abort ? SX_ERR_NOMEM : SX_OK;
}

//! the same exchange for counts the device computed (cntBuf[0, P), e.g. diffCountsKernel): sent as they are (or the
//! abort marker), and the sent and received counts read back in one synchronisation; sendOff = prefix sums of send
int deviceCountsOrAbort(sx_sim* s, bool fail, hipStream_t st, std::vector<uint64_t>& send,
                        std::vector<uint64_t>& sendOff, std::vector<uint64_t>& recv)
{
    const int P = s->comm->size();
    uint64_t* h = s->dom.cnth;
    if (!h || !s->cntBuf) return SX_ERR_NOMEM;
    if (fail)
    {
        for (int q = 0; q < P; ++q)
            h[q] = kAbortCount;
        SIM_HIP(hipMemcpyAsync(s->cntBuf, h, 8 * (size_t)P, hipMemcpyHostToDevice, st));
    }
    std::vector<uint64_t> bytes(P, 8), off(P);
    for (int q = 0; q < P; ++q)
        off[q] = 8 * (uint64_t)q;
    SIM_COMM(s->comm->alltoallv(s->cntBuf, bytes.data(), off.data(), s->cntBuf + P, bytes.data(), off.data(), st));
    SIM_HIP(hipMemcpyAsync(h, s->cntBuf, 16 * (size_t)P, hipMemcpyDeviceToHost, st));
    SIM_HIP(hipStreamSynchronize(st));
    send.assign(h, h + P);
    recv.assign(h + P, h + 2 * P);
    sendOff.assign(P + 1, 0);
    bool abort = fail;
    for (int q = 0; q < P; ++q)
    {
        abort |= recv[q] == kAbortCount;
        sendOff[q + 1] = sendOff[q] + (fail ? 0 : send[q]);
    }
    return abort ? SX_ERR_NOMEM : SX_OK;
}

int distributedSync(sx_sim* s, hipStream_t st, double margin)
{
    sx::Transport* T  = s->comm;
    const int      P  = T->size(), r = T->rank();
    size_t         nl = s->last - s->first;
    const double   qm = quantMargin(s->dbox);

    // --- 1. local keys + sort (compacts locals to [0, nl))
    SIM_HIP(launchSfcKeys(s->x + s->first, s->y + s->first, s->z + s->first, s->keys, nl, s->dbox, st));
    if (s->first != 0)
    {
        for (auto& sp : s->spares)
        {
            SIM_HIP(hipMemcpyAsync(sp.alt, static_cast<char*>(*sp.field) + s->first * sp.elemBytes, nl * sp.elemBytes,
                                   hipMemcpyDeviceToDevice, st));
            std::swap(*sp.field, sp.alt);
        }
    }
    if (int e = sortLocals(s, nl, st)) return e;

    // --- 2. global histogram -> splitters (the small per-rank buffers of the sync were allocated by sx_sim_set_comm,
    //        so nothing here fails on one rank alone between two collectives)
    const size_t nb   = size_t(1) << kHistBits;
    uint32_t*    bins = s->dom.bins;
    if (!bins) return SX_ERR_NOMEM; // allocated by set_comm: cannot fail here
    SIM_HIP(hipMemsetAsync(bins, 0, nb * 4, st));
    if (nl) histKernel<<<grid(nl), 256, 0, st>>>(s->keys, nl, bins);
    SIM_COMM(T->allreduceSumU32(bins, nb, st));
    std::vector<uint32_t> hb(nb);
    SIM_HIP(hipMemcpyAsync(hb.data(), bins, nb * 4, hipMemcpyDeviceToHost, st));
    SIM_HIP(hipStreamSynchronize(st));
    std::vector<uint64_t> split(P + 1, 0);
    if (int e = sx_domain_splitters(hb.data(), kHistBits, P, split.data())) return e;
    // every rank's particle count after the exchange: the histogram bins of its range (splitters are bin
    // boundaries), so the request-box counts of step 4 need no exchange
    std::vector<uint64_t> nlOf(P, 0);
    s->cellsOf.assign(P, 0);
    for (int q = 0; q < P; ++q)
        for (uint64_t b = split[q] >> (63 - kHistBits); b < (split[q + 1] >> (63 - kHistBits)) && b < nb; ++b)
        {
            nlOf[q] += hb[b];
            s->cellsOf[q] += hb[b] != 0;
        }

    // --- 3. particle exchange
    uint64_t* dsplit = s->dom.split;
    uint64_t* dseg   = s->dom.seg;
    if (!dsplit || !dseg || !s->cntBuf) return SX_ERR_NOMEM; // set by set_comm (domReserveComm)
    // the send counts stay on the device: segments of the sorted keys -> counts -> the count exchange, read back
    // together with the receive counts (one synchronisation)
    SIM_HIP(hipMemcpyAsync(dsplit, split.data(), 8 * (P + 1), hipMemcpyHostToDevice, st));
    lowerBoundsKernel<<<grid(P + 1, 64), 64, 0, st>>>(s->keys, nl, dsplit, P, dseg);
    diffCountsKernel<<<grid(P, 64), 64, 0, st>>>(dseg, nullptr, P, s->cntBuf);
    std::vector<uint64_t> sendCnt, seg, recvCnt;
    // the new local count is this rank's histogram bins (nlOf[r], the sum of the receive counts); the exchange
    // buffers are sized by it before the count exchange, so a failure is decided there on every rank
    auto  recvBuf = [&](size_t count) { return s->work.get<PRec>("dom.precv", count); };
    PRec* sbuf = nullptr;
    PRec* rbuf = nullptr;
    bool  noRoom = nlOf[r] > s->cap;
    if (!noRoom)
    {
        sbuf   = s->work.get<PRec>("dom.psend", nl);
        rbuf   = recvBuf(nlOf[r]);
        noRoom = !sbuf || !rbuf;
    }
    if (int e = deviceCountsOrAbort(s, noRoom, st, sendCnt, seg, recvCnt)) return e;
    bool moved = false;
    for (int q = 0; q < P; ++q)
        moved |= (q != r) && (sendCnt[q] || recvCnt[q]);
    // a local count that disagrees with the histogram cannot happen (the splitters are bin boundaries of the histogram
    // of these same keys); should it, this rank still takes part in every collective up to the halo count exchange,
    // sized by the histogram as its peers expect, and aborts all ranks there together (countsOrAbort)
    bool broken = false;
    if (moved)
    {
        uint64_t nNew = 0;
        for (int q = 0; q < P; ++q)
            nNew += recvCnt[q];
        broken = nNew != nlOf[r];
        if (broken) rbuf = recvBuf(nNew); // the peers send nNew records
        if (nl) packPRecKernel<<<grid(nl), 256, 0, st>>>(s->fields(), nl, sbuf);
        std::vector<uint64_t> sb(P), so(P), rb(P), ro(P);
        uint64_t              acc = 0;
        for (int q = 0; q < P; ++q)
        {
            sb[q] = sendCnt[q] * sizeof(PRec);
            so[q] = seg[q] * sizeof(PRec);
            rb[q] = recvCnt[q] * sizeof(PRec);
            ro[q] = acc * sizeof(PRec);
            acc += recvCnt[q];
        }
        if (!rbuf) // only on the broken path: receive nothing (the peers abort with this rank below)
            for (int q = 0; q < P; ++q)
                rb[q] = 0;
        SIM_COMM(T->alltoallv(sbuf, sb.data(), so.data(), rbuf, rb.data(), ro.data(), st));
        if (!broken)
        {
            nl = nNew;
            if (nl) unpackPRecKernel<<<grid(nl), 256, 0, st>>>(rbuf, nl, s->fields());
            SIM_HIP(launchSfcKeys(s->x, s->y, s->z, s->keys, nl, s->dbox, st));
            if (int e = sortLocals(s, nl, st)) return e;
        }
    }

    // --- 4. halo discovery: request boxes, exchange, mark, send lists
    // the exchange delivers exactly this rank's bins (the peers size their box receives from nlOf): the splitters
    // are bin boundaries of the histogram of these same keys, so this holds on every rank by construction; a rank
    // where it does not (`broken`) sends boxes of the size its peers expect and aborts them at the count exchange below
    broken |= nl != nlOf[r];
    if (broken) nl = std::min<size_t>(nl, nlOf[r]);
    const size_t nChunks = (nlOf[r] + kChunk - 1) / kChunk;
    ReqBox*      myBoxes = s->dom.mybox = s->work.get<ReqBox>("dom.mybox", nChunks);
    if (!myBoxes) return SX_ERR_NOMEM;
    if (broken) SIM_HIP(hipMemsetAsync(myBoxes, 0, nChunks * sizeof(ReqBox), st));
    else if (nChunks)
        chunkBoxKernel<<<(unsigned)nChunks, 256, 0, st>>>(s->x, s->y, s->z, s->h, nl, margin, qm, r, myBoxes);
    std::vector<uint64_t> boxCnt(P, nChunks), boxRecv(P);
    boxCnt[r] = 0;
    for (int q = 0; q < P; ++q)
        boxRecv[q] = q == r ? 0 : (nlOf[q] + kChunk - 1) / kChunk;
    uint64_t nRemote = 0;
    for (int q = 0; q < P; ++q)
        nRemote += boxRecv[q];
    ReqBox* remote = s->work.get<ReqBox>("dom.rbox", nRemote);
    {
        std::vector<uint64_t> sb(P), so(P, 0), rb(P), ro(P);
        uint64_t              acc = 0;
        for (int q = 0; q < P; ++q)
        {
            sb[q] = boxCnt[q] * sizeof(ReqBox);
            rb[q] = boxRecv[q] * sizeof(ReqBox);
            ro[q] = acc * sizeof(ReqBox);
            acc += boxRecv[q];
        }
        SIM_COMM(T->alltoallv(myBoxes, sb.data(), so.data(), remote, rb.data(), ro.data(), st));
    }
    SIM_HIP(buildTree(s->work, s->keys, nl, s->bucket, s->dbox, s->localTree, st));
    auto* mark = s->work.get<unsigned long long>("dom.mark", nl);
    auto* err  = s->work.get<uint32_t>("dom.err", 1);
    SIM_HIP(hipMemsetAsync(mark, 0, nl * 8, st));
    SIM_HIP(hipMemsetAsync(err, 0, 4, st));
    if (nRemote && nl)
        markHalosKernel<<<grid(nRemote, 4), 256, 0, st>>>(
            remote, (int)nRemote, s->localTree.childOffsets, s->localTree.internalToLeaf, s->localTree.layout,
            s->localTree.centers, s->localTree.sizes, s->x, s->y, s->z, s->dbox, qm, mark, err);
    // send lists of the peers from one flag array and one scan per batch of peers (peer order), one host read of the
    // batch's offsets; a batch holds as many peers as keep its flags within kFlagCap entries (and the scan's int
    // count), so the scratch does not grow with the rank count
    constexpr size_t kFlagCap = size_t(1) << 27;
    const int        Pb       = (int)std::max<size_t>(1, std::min<size_t>(P, kFlagCap / (nl + 1)));
    const size_t     nf       = (size_t)Pb * (nl + 1);
    // scratch failures are not returned here (the peers would wait in the count exchange below): they skip the
    // send-list work and abort every rank at that exchange (countsOrAbort)
    bool      fail = broken || nf > (size_t)INT32_MAX; // one peer's segment alone beyond the scan's range
    uint32_t* flag = fail ? nullptr : s->work.get<uint32_t>("dom.flag", nf);
    uint32_t* scan = fail ? nullptr : s->work.get<uint32_t>("dom.scan", nf);
    uint32_t* segs = s->work.get<uint32_t>("dom.segs", Pb + 1);
    uint32_t* hseg = s->work.pinned<uint32_t>("dom.hseg", Pb + 1);
    fail |= !flag || !scan || !segs || !hseg;
    s->haloSend.assign(P, 0);
    s->haloSendOff.assign(P, 0);
    size_t tmpB = 0;
    void*  tmp  = nullptr;
    if (!fail)
    {
        hipcub::DeviceScan::ExclusiveSum(nullptr, tmpB, flag, scan, (int)nf, st);
        tmp  = s->work.get<char>("dom.scantmp", tmpB);
        fail = !tmp;
    }
    // flags + scan of one batch; with scatter, the batch's send indices go to sendIdx[base, ...)
    auto batch = [&](int q0, int nb, bool scatter, uint64_t base) -> int
    {
        const size_t nfb = (size_t)nb * (nl + 1);
        maskFlagsKernel<<<grid(nfb), 256, 0, st>>>(mark, nl, q0, nb, r, flag);
        SIM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmpB, flag, scan, (int)nfb, st));
        if (scatter) scatterIdxKernel<<<grid(nfb), 256, 0, st>>>(flag, scan, nl, nb, base, s->sendIdx);
        segStartsKernel<<<grid(nb + 1, 64), 64, 0, st>>>(scan, nl, nb, segs);
        SIM_HIP(hipMemcpyAsync(hseg, segs, 4 * (nb + 1), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        for (int j = 0; j < nb; ++j)
        {
            s->haloSendOff[q0 + j] = base + hseg[j];
            s->haloSend[q0 + j]    = (j < nb - 1 ? hseg[j + 1] : hseg[nb]) - hseg[j];
        }
        return SX_OK;
    };
    // the send list is sized by what the peers request (a local may go to several peers): with one batch the scan
    // is read before the scatter; with several, a counting pass first (the arena's growth does not keep contents)
    auto     sendList = [&](uint64_t count) { return s->work.get<uint32_t>("dom.sendIdx", std::max<uint64_t>(1, count)); };
    uint64_t total   = 0;
    bool     idxFail = false; // the send list could not be sized (one batch: decided after the count exchange)
    if (!fail && Pb >= P)
    {
        // one batch (the common case): the send counts stay on the device -- segment starts of the scan -> counts ->
        // the count exchange, read back with the halo receive counts in one synchronisation; the send list is sized
        // and scattered after it (flags and scan are kept)
        const size_t nfb = (size_t)P * (nl + 1);
        maskFlagsKernel<<<grid(nfb), 256, 0, st>>>(mark, nl, 0, P, r, flag);
        SIM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmpB, flag, scan, (int)nfb, st));
        segStartsKernel<<<grid(P + 1, 64), 64, 0, st>>>(scan, nl, P, segs);
        diffCountsKernel<<<grid(P, 64), 64, 0, st>>>(nullptr, segs, P, s->cntBuf);
        std::vector<uint64_t> off;
        if (int e = deviceCountsOrAbort(s, false, st, s->haloSend, off, s->haloRecv)) return e;
        for (int q = 0; q < P; ++q)
            s->haloSendOff[q] = off[q];
        total      = off[P];
        s->sendIdx = sendList(total);
        idxFail    = !s->sendIdx;
        if (!idxFail) scatterIdxKernel<<<grid(nfb), 256, 0, st>>>(flag, scan, nl, P, 0, s->sendIdx);
    }
    else
    {
        // several batches (the flags of all peers beyond kFlagCap): a counting pass, then the scatter pass, the
        // counts exchanged on the host's copy
        for (int q0 = 0; q0 < P && !fail; q0 += Pb)
        {
            const int nb = std::min(Pb, P - q0);
            if (int e = batch(q0, nb, false, total)) return e;
            total += hseg[nb];
        }
        s->sendIdx = fail ? nullptr : sendList(total);
        fail |= !s->sendIdx;
        if (!fail)
        {
            uint64_t base = 0;
            for (int q0 = 0; q0 < P; q0 += Pb)
            {
                const int nb = std::min(Pb, P - q0);
                if (int e = batch(q0, nb, true, base)) return e;
                base += hseg[nb];
            }
        }
        if (int e = countsOrAbort(s, s->haloSend, s->haloRecv, fail, st)) return e;
    }
    s->numSend     = total;
    s->haloRecv[r] = 0;
    uint64_t nLow = 0, nHigh = 0;
    for (int q = 0; q < P; ++q)
        (q < r ? nLow : nHigh) += s->haloRecv[q];
    {
        // the halo capacity (known once the receive counts are) and the send list, decided on every rank together
        bool full = false;
        if (int e = anyRank(s, nLow + nl + nHigh > s->cap || idxFail, st, full)) return e;
        if (full) return SX_ERR_NOMEM;
    }
    s->haloRecvOff.assign(P, 0);
    {
        uint64_t lay[3];
        if (int e = sx_domain_halo_layout(s->haloRecv.data(), P, r, nl, s->haloRecvOff.data(), lay)) return e;
    }
    s->numHalos = nLow + nHigh;

    // --- 5. move locals to [nLow, nLow + nl), exchange x,y,z,h,m, keys + tree over everything
    if (nLow)
    {
        for (auto& sp : s->spares)
        {
            SIM_HIP(hipMemcpyAsync(static_cast<char*>(sp.alt) + nLow * sp.elemBytes, *sp.field, nl * sp.elemBytes,
                                   hipMemcpyDeviceToDevice, st));
            std::swap(*sp.field, sp.alt);
        }
    }
    s->first = nLow;
    s->last  = nLow + nl;
    s->n     = nLow + nl + nHigh;
    // the halos' keys come from their owners (8 B each; the owners computed them from the same coordinates), so the
    // combined tree is built while x,y,z,h,m (28 B per halo) are still in flight on the communication stream
    SIM_HIP(launchSfcKeys(s->x + s->first, s->y + s->first, s->z + s->first, s->keys + s->first, nl, s->dbox, st));
    if (int e = haloExchange(s, {{s->keys, 8}}, st)) return e;
    const bool ovl = s->overlap && s->commStream;
    hipStream_t cs = ovl ? s->commStream : st;
    if (ovl)
    {
        SIM_HIP(hipEventRecord(s->evProd, st));
        SIM_HIP(hipStreamWaitEvent(cs, s->evProd, 0));
    }
    if (int e = haloExchange(s, {{s->x, 8}, {s->y, 8}, {s->z, 8}, {s->h, 4}, {s->m, 4}}, cs)) return e;
    if (ovl) SIM_HIP(hipEventRecord(s->evComm, cs));
    SIM_HIP(buildTree(s->work, s->keys, s->n, s->bucket, s->dbox, s->tree, st));
    if (ovl) SIM_HIP(hipStreamWaitEvent(st, s->evComm, 0));
    s->syncErr = err; // read after the search, with its statistics (syncErrEnqueue / syncErrFailed)
    return SX_OK;
}

//! the last sync's halo-marking flag -> host, ordered on st before the caller's next synchronisation
int syncErrEnqueue(sx_sim* s, hipStream_t st)
{
    uint32_t* h = s->dom.errh;
    if (!h) return SX_ERR_NOMEM;
    *h = 0;
    if (s->syncErr) SIM_HIP(hipMemcpyAsync(h, s->syncErr, 4, hipMemcpyDeviceToHost, st));
    return SX_OK;
}

//! after that synchronisation: the halo marking of the last sync overflowed its traversal stack
bool syncErrFailed(sx_sim* s)
{
    const uint32_t* h = s->dom.errh;
    return h && *h != 0;
}

/*! a decision every rank must take together: true on all ranks if `bad` holds on any (one allreduce).  A rank that
 *  returned alone from the middle of distributedSync would leave its peers waiting in the next collective. */
int anyRank(sx_sim* s, bool bad, hipStream_t st, bool& out)
{
    uint32_t* flg  = s->dom.agree;
    uint32_t* hflg = s->dom.agreeh;
    if (!flg || !hflg) return SX_ERR_NOMEM;
    *hflg = bad ? 1u : 0u;
    SIM_HIP(hipMemcpyAsync(flg, hflg, 4, hipMemcpyHostToDevice, st));
    SIM_COMM(s->comm->allreduceSumU32(flg, 1, st));
    SIM_HIP(hipMemcpyAsync(hflg, flg, 4, hipMemcpyDeviceToHost, st));
    SIM_HIP(hipStreamSynchronize(st));
    out = *hflg != 0;
    return SX_OK;
}

int halosOutgrown(sx_sim* s, hipStream_t st, unsigned& hf)
{
    const size_t nl  = s->last - s->first;
    unsigned*    flg = s->dom.hflag;
    SIM_HIP(hipMemsetAsync(flg, 0, 4, st));
    if (nl)
        chunkCoverKernel<<<grid(nl), 256, 0, st>>>(s->x + s->first, s->y + s->first, s->z + s->first, s->h + s->first,
                                                 nl, s->dom.mybox, s->dbox,
                                                 quantMargin(s->dbox), flg);
    // the retry decision must be global: a rank redoing the sync alone would deadlock the collectives
    SIM_COMM(s->comm->allreduceSumU32(flg, 1, st));
    unsigned* hflg = s->dom.hflagh;
    SIM_HIP(hipMemcpyAsync(hflg, flg, 4, hipMemcpyDeviceToHost, st));
    if (int e = syncErrEnqueue(s, st)) return e;
    SIM_HIP(hipStreamSynchronize(st));
    if (syncErrFailed(s)) return SX_ERR_TRAVERSAL;
    hf = *hflg;
    return SX_OK;
}

int localSync(sx_sim* s, hipStream_t st)
{
    const size_t n = s->n;
    // keys written by the last position update (PosArgs::keys) are those of the current coordinates
    if (!s->keysFresh) SIM_HIP(launchSfcKeys(s->x, s->y, s->z, s->keys, n, s->dbox, st));
    s->keysFresh = false;
    if (int e = sortLocals(s, n, st)) return e;
    SIM_HIP(buildTree(s->work, s->keys, n, s->bucket, s->dbox, s->tree, st));
    s->first = 0;
    s->last  = n;
    return SX_OK;
}

} // namespace sx::sim
