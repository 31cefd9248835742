/*! @file sx_profile.hip
 * @brief Binned profiles with exact sums (sx_profile.hpp): two streaming passes over the particles and a conversion.
 *
 * Pass 1 evaluates coordinate, quantities and terms and reduces, per series, the largest window key (an integer maximum)
 * and the number of non-finite particles.  Pass 2 evaluates the same expressions again (the same instructions: the same
 * bits), shifts every term into its series' window and adds the 128-bit integers per bin in block-private LDS with
 * 64-bit integer atomics, flushed once per block with 64-bit global integer atomics.  Where (nbins + 2) x bytesPerBin
 * exceeds the block's share the bins are tiled: one launch of pass 2 per tile, which skips the particles of the other
 * tiles.  (A variant that adds straight into the global array is kept behind sx_set_profile_lds for measurement and
 * as a second route to the same bits: at 8M particles and 50 bins it takes 67 ms against 0.6.)  A 128-bit add is an add to the low word whose
 * returned old value tells this thread whether it carried, plus an add of (high word + carry) to the high word; the
 * pair is not consistent mid-flight and need not be: only the totals are read, after the kernel.
 * Built with -ffp-contract=off: the arithmetic rule of include/sphexa_hip.h.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sx_device.hpp"
#include "sx_profile.hpp"

namespace sx::profile
{

namespace
{

struct SolDev
{
    int           kind;
    uint32_t      nt;
    const double *r, *y;
    double        rscale, r2, behind, rho0, vt;
    int           xgeom;
};

struct KArgs
{
    const double *x, *y, *z, *temp;
    const float * vx, *vy, *vz, *m, *kx, *xm, *rho, *c, *h, *divv, *curlv, *alpha;
    uint32_t      first, last;
    double        center[3], len[3];
    int           pbc[3];
    int           coord, coordQ, weight, std;
    uint32_t      nbins;
    const double* edges;
    int           uniform;
    double        e0, invWidth;
    int           nq;
    int           q[kMaxQ];
    SolDev        sol[kMaxQ];
    double        cv, gm1;
    uint32_t*     keys;
    uint64_t*     acc;
    uint32_t      tileLo, tileBins; // pass 2 in LDS: the internal bins of this launch
};

struct Eval
{
    double c;
    double q[kMaxQ];
    double t[kMaxSeries];
    bool   ok;
};

__device__ __forceinline__ bool finite(double v) { return finiteBits(doubleBits(v)); }

__device__ __forceinline__ double quantity(const KArgs& a, int code, uint32_t i, double dx, double dy, double dz, double r)
{
    switch (code)
    {
        case SX_PROF_RHO:
        case SX_PROF_P:
        {
            const float rho = a.std ? a.rho[i] : (a.kx[i] * a.m[i]) / a.xm[i];
            if (code == SX_PROF_RHO) return (double)rho;
            return (double)(float)((double)rho * ((a.cv * a.temp[i]) * a.gm1));
        }
        case SX_PROF_U: return a.cv * a.temp[i];
        case SX_PROF_TEMP: return a.temp[i];
        case SX_PROF_VEL:
        {
            const double vx = a.vx[i], vy = a.vy[i], vz = a.vz[i];
            return sqrt((vx * vx + vy * vy) + vz * vz);
        }
        case SX_PROF_VRAD:
        {
            if (r == 0.0) return 0.0;
            const double vx = a.vx[i], vy = a.vy[i], vz = a.vz[i];
            return ((dx * vx + dy * vy) + dz * vz) / r;
        }
        case SX_PROF_C: return (double)a.c[i];
        case SX_PROF_H: return (double)a.h[i];
        case SX_PROF_DIVV: return (double)a.divv[i];
        case SX_PROF_CURLV: return (double)a.curlv[i];
        default: return (double)a.alpha[i];
    }
}

__device__ __forceinline__ double solution(const SolDev& s, double c)
{
    const double xi = c * s.rscale;
    if (s.kind == SX_PROF_SOL_TABLE)
    {
        const uint32_t last = s.nt - 1;
        if (xi < s.r[0]) return s.y[0];
        if (xi >= s.r[last]) return s.y[last];
        uint32_t lo = 0, hi = last; // r[lo] <= xi < r[hi]
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (s.r[mid] <= xi) lo = mid;
            else hi = mid;
        }
        const double rj = s.r[lo], yj = s.y[lo];
        if (xi == rj) return yj;
        return ((s.y[lo + 1] - yj) / (s.r[lo + 1] - rj)) * (xi - rj) + yj;
    }
    // SX_PROF_SOL_NOH_RHO
    if (xi > s.r2)
    {
        const double b  = 1.0 - s.vt / (xi > 1e-300 ? xi : 1e-300);
        const double pw = s.xgeom == 1 ? 1.0 : (s.xgeom == 2 ? b : b * b);
        return s.rho0 * pw;
    }
    return s.behind;
}

__device__ __forceinline__ Eval evaluate(const KArgs& a, uint32_t i)
{
    Eval   e;
    double d[3] = {a.x[i] - a.center[0], a.y[i] - a.center[1], a.z[i] - a.center[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (a.pbc[k]) d[k] = d[k] - a.len[k] * rint(d[k] / a.len[k]);
    const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    switch (a.coord)
    {
        case SX_PROF_RADIUS: e.c = r; break;
        case SX_PROF_X: e.c = d[0]; break;
        case SX_PROF_Y: e.c = d[1]; break;
        case SX_PROF_Z: e.c = d[2]; break;
        default: e.c = quantity(a, a.coordQ, i, d[0], d[1], d[2], r);
    }
    const double w = a.weight == SX_PROF_MASS ? (double)a.m[i] : 1.0;
    e.ok           = finite(e.c) && finite(w);
    e.t[0]         = w;
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k)
    {
        if (k < a.nq)
        {
            const double q  = quantity(a, a.q[k], i, d[0], d[1], d[2], r);
            const double wq = w * q;
            e.q[k]          = q;
            e.t[1 + 3 * k]  = wq;
            e.t[2 + 3 * k]  = wq * q;
            double dev      = 0.0;
            if (a.sol[k].kind != SX_PROF_SOL_NONE && e.ok)
            {
                const double s = solution(a.sol[k], e.c);
                dev            = w * fabs(q - s);
                e.ok           = e.ok && finite(s);
            }
            e.t[3 + 3 * k] = dev;
            e.ok           = e.ok && finite(q) && finite(wq) && finite(e.t[2 + 3 * k]) && finite(dev);
        }
    }
    return e;
}

//! the internal bin of a finite c: np.searchsorted(edges, c, side="right") - 1, underflow nbins, overflow nbins + 1
__device__ __forceinline__ uint32_t binOf(const KArgs& a, double c)
{
    const double*  e  = a.edges;
    const uint32_t nb = a.nbins;
    if (c < e[0]) return nb;
    if (c >= e[nb]) return nb + 1;
    if (a.uniform)
    {
        // a guess from the spacing, then corrected against the edges: e[0] <= c < e[nb] bounds both walks
        const double g = (c - a.e0) * a.invWidth;
        uint32_t     b = g >= (double)nb ? nb - 1 : (g > 0.0 ? (uint32_t)g : 0u);
        while (c < e[b])
            --b;
        while (c >= e[b + 1])
            ++b;
        return b;
    }
    uint32_t lo = 0, hi = nb; // e[lo] <= c < e[hi]
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (e[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void pass1Kernel(KArgs a)
{
    __shared__ uint32_t     sKey[kMaxSeries];
    __shared__ unsigned int sBad;
    if (threadIdx.x < kMaxSeries) sKey[threadIdx.x] = 0;
    if (threadIdx.x == 0) sBad = 0;
    __syncthreads();
    const int nser = 1 + 3 * a.nq;
    uint32_t  key[kMaxSeries];
#pragma unroll
    for (int j = 0; j < kMaxSeries; ++j)
        key[j] = 0;
    unsigned int bad = 0;
    for (uint64_t i = (uint64_t)a.first + blockIdx.x * kBlock + threadIdx.x; i < a.last; i += (uint64_t)gridDim.x * kBlock)
    {
        const Eval e = evaluate(a, (uint32_t)i);
        if (!e.ok)
        {
            ++bad;
            continue;
        }
#pragma unroll
        for (int j = 0; j < kMaxSeries; ++j)
            if (j < nser) key[j] = max(key[j], windowKey(e.t[j]));
    }
#pragma unroll
    for (int j = 0; j < kMaxSeries; ++j)
        if (j < nser && key[j]) atomicMax(&sKey[j], key[j]);
    if (bad) atomicAdd(&sBad, bad);
    __syncthreads();
    if ((int)threadIdx.x < nser && sKey[threadIdx.x]) atomicMax(&a.keys[1 + threadIdx.x], sKey[threadIdx.x]);
    if (threadIdx.x == 0 && sBad) atomicAdd((unsigned long long*)a.acc, (unsigned long long)sBad);
}

extern __shared__ unsigned long long sBins[];

template<bool Lds>
__global__ __launch_bounds__(kBlock) void pass2Kernel(KArgs a)
{
    const int      nser = 1 + 3 * a.nq;
    const uint32_t nb2  = a.nbins + 2;
    // [sums 2 x series x bins | count bins | min nq x bins | max nq x bins]: the global array over all nb2 internal
    // bins, the LDS copy over the tb bins of this launch's tile [tileLo, tileLo + tb)
    const uint32_t offCnt = 2 * nser * nb2, offMin = offCnt + nb2, offMax = offMin + a.nq * nb2;
    const uint32_t tb = a.tileBins, lo = a.tileLo;
    const uint32_t lCnt = 2 * nser * tb, lMin = lCnt + tb, lMax = lMin + a.nq * tb, lWords = lMax + a.nq * tb;
    unsigned long long* const global = (unsigned long long*)a.acc + 1;
    if constexpr (Lds)
    {
        const unsigned long long minInit = orderKey(INFINITY), maxInit = orderKey(-INFINITY);
        for (uint32_t w = threadIdx.x; w < lWords; w += kBlock)
            sBins[w] = w < lMin ? 0ull : (w < lMax ? minInit : maxInit);
        __syncthreads();
    }
    int32_t E[kMaxSeries];
#pragma unroll
    for (int j = 0; j < kMaxSeries; ++j)
        E[j] = j < nser ? windowOfKey(a.keys[1 + j]) : kZeroWindow;

    for (uint64_t i = (uint64_t)a.first + blockIdx.x * kBlock + threadIdx.x; i < a.last; i += (uint64_t)gridDim.x * kBlock)
    {
        const Eval e = evaluate(a, (uint32_t)i);
        if (!e.ok) continue;
        const uint32_t b = binOf(a, e.c);
        if constexpr (Lds)
        {
            if (b < lo || b >= lo + tb) continue; // another launch's tile
            const uint32_t lb = b - lo;
#pragma unroll
            for (int j = 0; j < kMaxSeries; ++j)
                if (j < nser) add128(&sBins[2 * (j * tb + lb)], toFixed(e.t[j], E[j]));
            atomicAdd(&sBins[lCnt + lb], 1ull);
#pragma unroll
            for (int k = 0; k < kMaxQ; ++k)
                if (k < a.nq)
                {
                    const unsigned long long ok = orderKey(e.q[k]);
                    atomicMin(&sBins[lMin + k * tb + lb], ok);
                    atomicMax(&sBins[lMax + k * tb + lb], ok);
                }
        }
        else
        {
#pragma unroll
            for (int j = 0; j < kMaxSeries; ++j)
                if (j < nser) add128(&global[2 * (j * nb2 + b)], toFixed(e.t[j], E[j]));
            atomicAdd(&global[offCnt + b], 1ull);
#pragma unroll
            for (int k = 0; k < kMaxQ; ++k)
                if (k < a.nq)
                {
                    const unsigned long long ok = orderKey(e.q[k]);
                    atomicMin(&global[offMin + k * nb2 + b], ok);
                    atomicMax(&global[offMax + k * nb2 + b], ok);
                }
        }
    }
    if constexpr (Lds)
    {
        __syncthreads();
        // the block's totals, each a 128-bit integer modulo 2^128, into the global array; empty bins cost nothing
        for (uint32_t s = threadIdx.x; s < (uint32_t)nser * tb; s += kBlock)
            add128(&global[2 * ((s / tb) * nb2 + lo + s % tb)], U128{sBins[2 * s], sBins[2 * s + 1]});
        for (uint32_t w = lCnt + threadIdx.x; w < lWords; w += kBlock)
        {
            const unsigned long long v = sBins[w];
            if (w < lMin)
            {
                if (v) atomicAdd(&global[offCnt + lo + (w - lCnt)], v);
            }
            else if (w < lMax)
            {
                if (v != orderKey(INFINITY)) atomicMin(&global[offMin + ((w - lMin) / tb) * nb2 + lo + (w - lMin) % tb], v);
            }
            else if (v != orderKey(-INFINITY)) atomicMax(&global[offMax + ((w - lMax) / tb) * nb2 + lo + (w - lMax) % tb], v);
        }
    }
}

__global__ void initKernel(uint64_t* acc, uint32_t offMin, uint32_t offMax, uint32_t words)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    // word 0: nonfinite; then as pass2Kernel's layout, shifted by one
    acc[w] = (w == 0 || w - 1 < offMin) ? 0ull : (w - 1 < offMax ? orderKey(INFINITY) : orderKey(-INFINITY));
}

//! the integer words of acc (nonfinite, sums, counts) as 16-bit limbs in u32, four per word
__global__ void toLimbsKernel(const uint64_t* acc, uint32_t words, uint32_t* limbs)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    const uint64_t v = acc[w];
#pragma unroll
    for (int l = 0; l < 4; ++l)
        limbs[4 * w + l] = (uint32_t)((v >> (16 * l)) & 0xffffu);
}

//! the summed limbs back into integers, the carries propagated through each integer: one word for nonfinite and the
//! counts, two for a sum
__global__ void fromLimbsKernel(const uint32_t* limbs, uint32_t numSums, uint32_t numCounts, uint64_t* acc)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 1 + numSums + numCounts) return;
    // entity t: word 0 | sums, two words each | counts
    const bool     wide  = t >= 1 && t < 1 + numSums;
    const uint32_t first = t == 0 ? 0 : (wide ? 1 + 2 * (t - 1) : 1 + 2 * numSums + (t - 1 - numSums));
    uint64_t       carry = 0, out[2] = {0, 0};
    for (int l = 0; l < (wide ? 8 : 4); ++l)
    {
        const uint64_t v = (uint64_t)limbs[4 * first + l] + carry;
        out[l / 4] |= (v & 0xffffu) << (16 * (l % 4));
        carry = v >> 16;
    }
    acc[first] = out[0];
    if (wide) acc[first + 1] = out[1];
}

__global__ void minMaxOutKernel(const uint64_t* keysMin, uint32_t count, double* mm)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    const double v = fromOrderKey(keysMin[t]);
    mm[t]          = t < count ? v : -v;
}

__global__ void minMaxInKernel(const double* mm, uint32_t count, uint64_t* keysMin)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * count) return;
    keysMin[t] = orderKey(t < count ? mm[t] : -mm[t]);
}

//! 128-bit integers to doubles, the counts and the decoded extrema into the packed result
__global__ void finalKernel(const uint64_t* acc, const uint32_t* keys, uint32_t nb2, int nq, uint64_t* out)
{
    const uint32_t nser = 1 + 3 * nq;
    const uint32_t t    = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nSum = nser * nb2, offCnt = 1 + 2 * nSum, offMin = offCnt + nb2;
    if (t < nSum)
    {
        const uint32_t j = t / nb2, b = t % nb2;
        const double   v = fromFixed(U128{acc[1 + 2 * t], acc[2 + 2 * t]}, windowOfKey(keys[1 + j]));
        // W, then S1, S2, D: nq rows each
        const uint32_t row = j == 0 ? 1 : 2 + ((j - 1) % 3) * nq + (j - 1) / 3;
        out[row * nb2 + 1 + b] = doubleBits(v);
    }
    else if (t < nSum + nb2) out[t - nSum] = acc[offCnt + (t - nSum)];
    else if (t < nSum + nb2 + 2 * nq * nb2)
    {
        const uint32_t k = t - nSum - nb2; // min rows, then max rows
        out[(2 + 3 * nq) * nb2 + 1 + k] = doubleBits(fromOrderKey(acc[offMin + k]));
    }
    else if (t == nSum + nb2 + 2 * nq * nb2) out[nb2] = acc[0];
}

constexpr const char* kWho = "sx_profile"; // in front of the messages of SX_TRY_HIP

} // namespace

const char* checkSpec(const sx_profile* p, const sx_box* box)
{
    if (!p || !box) return "sx_profile: null profile or box";
    if (p->coord < SX_PROF_RADIUS || p->coord > SX_PROF_QUANTITY) return "sx_profile: unknown coord";
    if (p->coord == SX_PROF_QUANTITY && (p->coordQ < 0 || p->coordQ >= kNumCodes))
        return "sx_profile: unknown quantity for the coordinate";
    if (p->weight != SX_PROF_NUMBER && p->weight != SX_PROF_MASS) return "sx_profile: unknown weight";
    if (p->nbins < 1 || p->nbins > kMaxBins) return "sx_profile: nbins must be in 1 .. 4096";
    if (!p->edges) return "sx_profile: null edges";
    for (uint32_t b = 0; b <= p->nbins; ++b)
        if (!std::isfinite(p->edges[b])) return "sx_profile: edges must be finite";
    for (uint32_t b = 0; b < p->nbins; ++b)
        if (!(p->edges[b] < p->edges[b + 1])) return "sx_profile: edges must be strictly ascending";
    if (p->nq > (uint32_t)kMaxQ) return "sx_profile: at most 4 quantities per call";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->center[k])) return "sx_profile: center must be finite";
    for (uint32_t k = 0; k < p->nq; ++k)
        if (p->q[k] < 0 || p->q[k] >= kNumCodes) return "sx_profile: unknown quantity";
    for (uint32_t k = 0; k < (uint32_t)kMaxQ; ++k)
    {
        const sx_profile_solution& s = p->sol[k];
        if (s.kind < SX_PROF_SOL_NONE || s.kind > SX_PROF_SOL_NOH_RHO) return "sx_profile: unknown solution kind";
        if (s.kind == SX_PROF_SOL_NONE) continue;
        if (k >= p->nq) return "sx_profile: a solution on a slot that holds no quantity";
        if (!std::isfinite(s.rscale)) return "sx_profile: rscale must be finite";
        if (s.kind == SX_PROF_SOL_TABLE)
        {
            if (s.nt < 2 || s.nt > kMaxTable) return "sx_profile: a table needs 2 .. 2^20 entries";
            if (!s.r || !s.y) return "sx_profile: a table needs r and y";
            for (uint32_t j = 0; j < s.nt; ++j)
                if (!std::isfinite(s.r[j]) || (j && s.r[j] < s.r[j - 1])) return "sx_profile: a table's r must be finite and ascending";
        }
        else
        {
            if (s.xgeom < 1 || s.xgeom > 3) return "sx_profile: xgeom must be 1, 2 or 3";
            if (!std::isfinite(s.gamma) || !std::isfinite(s.rho0) || !std::isfinite(s.vel0) || !std::isfinite(s.time) || s.gamma == 1.0)
                return "sx_profile: the Noh parameters must be finite and gamma not 1";
        }
    }
    return nullptr;
}

const char* missingColumns(int code, const sx_fields& f, int std)
{
    switch (code)
    {
        case SX_PROF_RHO:
            if (std) return f.rho ? nullptr : "sx_profile: rho needs the rho column";
            return f.kx && f.xm && f.m ? nullptr : "sx_profile: rho needs kx, xm and m, which this layout does not keep";
        case SX_PROF_P:
            if (!f.temp) return "sx_profile: p needs temp, which this layout does not keep";
            if (std) return f.rho ? nullptr : "sx_profile: p needs the rho column";
            return f.kx && f.xm && f.m ? nullptr : "sx_profile: p needs kx, xm and m, which this layout does not keep";
        case SX_PROF_U: return f.temp ? nullptr : "sx_profile: u needs temp, which this layout does not keep";
        case SX_PROF_TEMP: return f.temp ? nullptr : "sx_profile: temp is not kept by this layout";
        case SX_PROF_VEL:
        case SX_PROF_VRAD: return f.vx && f.vy && f.vz ? nullptr : "sx_profile: vel and vrad need vx, vy and vz";
        case SX_PROF_C: return f.c ? nullptr : "sx_profile: c is not kept by this layout";
        case SX_PROF_H: return f.h ? nullptr : "sx_profile: h is not kept by this layout";
        case SX_PROF_DIVV: return f.divv ? nullptr : "sx_profile: divv is not kept by this layout";
        case SX_PROF_CURLV: return f.curlv ? nullptr : "sx_profile: curlv is not kept by this layout";
        case SX_PROF_ALPHA: return f.alpha ? nullptr : "sx_profile: alpha is not kept by this layout";
        default: return "sx_profile: unknown quantity";
    }
}

const char* whyRefused(const sx_profile* p, const sx_box* box, const sx_fields& f, int std, size_t n)
{
    if (const char* why = checkSpec(p, box)) return why;
    if (!f.x || !f.y || !f.z) return "sx_profile: x, y and z are required";
    if (p->weight == SX_PROF_MASS && !f.m) return "sx_profile: the mass weight needs m";
    if (n > kMaxParticles) return "sx_profile: more than 2^31 - 1 particles: the 128-bit sums are not guaranteed";
    if (p->coord == SX_PROF_QUANTITY)
        if (const char* why = missingColumns(p->coordQ, f, std)) return why;
    for (uint32_t k = 0; k < p->nq; ++k)
        if (const char* why = missingColumns(p->q[k], f, std)) return why;
    return nullptr;
}

//! bytes per particle one pass reads: the coordinates and every distinct column of the quantities and the weight
static double bytesPerParticle(const sx_profile& p, int std)
{
    bool vel = false, rho = false, temp = false, mass = p.weight == SX_PROF_MASS;
    int  other = 0;
    auto use   = [&](int code)
    {
        switch (code)
        {
            case SX_PROF_RHO: rho = true; break;
            case SX_PROF_P: rho = temp = true; break;
            case SX_PROF_U:
            case SX_PROF_TEMP: temp = true; break;
            case SX_PROF_VEL:
            case SX_PROF_VRAD: vel = true; break;
            default: other |= 1 << code;
        }
    };
    for (uint32_t k = 0; k < p.nq; ++k)
        use(p.q[k]);
    if (p.coord == SX_PROF_QUANTITY) use(p.coordQ);
    double bytes = 24;
    if (vel) bytes += 12;
    if (temp) bytes += 8;
    if (rho && std) bytes += 4;
    if (rho && !std) bytes += 8, mass = true;
    if (mass) bytes += 4;
    return bytes + 4 * __builtin_popcount(other);
}

int compute(Arena& arena, ProfBuffers& b, const sx_profile& p, const sx_fields& f, const sx_box& box, uint32_t first,
            uint32_t last, float muiConst, double gamma, int std, const char* refused, const Reduce& reduce,
            hipStream_t s, std::string& err)
{
    const bool dist = (bool)reduce.maxU32;
    b.keys          = arena.get<uint32_t>("prof.keys", kKeyWords);
    b.keysHost      = arena.pinned<uint32_t>("prof.keysHost", kKeyWords);
    if (!b.keys || !b.keysHost)
    {
        err = "sx_profile: window buffers";
        return SX_ERR_NOMEM;
    }
    SX_TRY_HIP(kWho, hipMemsetAsync(b.keys, 0, kKeyWords * sizeof(uint32_t), s));
    if (refused)
    {
        err = refused;
        if (dist)
        {
            // take part in the one collective every rank reaches whatever its specification, then leave
            const uint32_t one = 1;
            SX_TRY_HIP(kWho, hipMemcpyAsync(b.keys, &one, sizeof(one), hipMemcpyHostToDevice, s));
            if (!reduce.maxU32(b.keys, kKeyWords)) return SX_ERR_HIP;
            SX_TRY_HIP(kWho, hipStreamSynchronize(s));
        }
        return SX_ERR_ARG;
    }

    const uint32_t nq = p.nq, nser = 1 + 3 * nq, nb2 = p.nbins + 2;
    const uint32_t offMin = 2 * nser * nb2 + nb2, offMax = offMin + nq * nb2; // pass2Kernel's layout
    const uint32_t accWords = 1 + offMax + nq * nb2;
    const size_t   nOut     = outWords(p.nbins, nq);
    size_t         tableWords = 0;
    for (uint32_t k = 0; k < nq; ++k)
        if (p.sol[k].kind == SX_PROF_SOL_TABLE) tableWords += 2 * (size_t)p.sol[k].nt;
    b.acc     = arena.get<uint64_t>("prof.acc", accWords);
    b.edges   = arena.get<double>("prof.edges", p.nbins + 1);
    b.table   = arena.get<double>("prof.table", tableWords);
    b.out     = arena.get<uint64_t>("prof.out", nOut);
    b.outHost = arena.pinned<uint64_t>("prof.outHost", nOut);
    if (dist)
    {
        b.limbs  = arena.get<uint32_t>("prof.limbs", 4 * (size_t)offMin + 4);
        b.minmax = arena.get<double>("prof.minmax", 2 * (size_t)nq * nb2);
    }
    if (!b.acc || !b.edges || !b.table || !b.out || !b.outHost || (dist && (!b.limbs || !b.minmax)))
    {
        err = "sx_profile: accumulator buffers";
        return SX_ERR_NOMEM;
    }
    SX_TRY_HIP(kWho, b.clock.begin());

    KArgs a{};
    a.x = f.x, a.y = f.y, a.z = f.z, a.temp = f.temp;
    a.vx = f.vx, a.vy = f.vy, a.vz = f.vz, a.m = f.m, a.kx = f.kx, a.xm = f.xm, a.rho = f.rho;
    a.c = f.c, a.h = f.h, a.divv = f.divv, a.curlv = f.curlv, a.alpha = f.alpha;
    a.first = first, a.last = last;
    for (int k = 0; k < 3; ++k)
    {
        a.center[k] = p.center[k];
        a.len[k]    = box.lim[2 * k + 1] - box.lim[2 * k];
        a.pbc[k]    = box.bnd[k] == 1 && a.len[k] > 0.0;
    }
    a.coord = p.coord, a.coordQ = p.coordQ, a.weight = p.weight, a.std = std;
    a.nbins = p.nbins, a.edges = b.edges;
    // equal spacing (to a hundredth of a bin) lets binOf start from a computed guess; the edges decide either way
    const double width = (p.edges[p.nbins] - p.edges[0]) / p.nbins;
    a.uniform          = std::isfinite(width) && width > 0.0;
    for (uint32_t k = 0; a.uniform && k <= p.nbins; ++k)
        a.uniform = std::fabs(p.edges[k] - (p.edges[0] + k * width)) <= 0.01 * width;
    a.e0 = p.edges[0], a.invWidth = a.uniform ? 1.0 / width : 0.0;
    if (!std::isfinite(a.invWidth)) a.uniform = 0;
    a.nq = (int)nq;
    a.cv = (double)idealGasCv(muiConst, gamma), a.gm1 = gamma - 1.0;
    a.keys = b.keys, a.acc = b.acc;
    SX_TRY_HIP(kWho, hipMemcpyAsync(b.edges, p.edges, (p.nbins + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    double* tab = b.table;
    for (uint32_t k = 0; k < nq; ++k)
    {
        const sx_profile_solution& h = p.sol[k];
        SolDev&                    d = a.sol[k];
        a.q[k]   = p.q[k];
        d.kind   = h.kind;
        d.rscale = h.rscale;
        if (h.kind == SX_PROF_SOL_TABLE)
        {
            d.nt = h.nt, d.r = tab, d.y = tab + h.nt;
            SX_TRY_HIP(kWho, hipMemcpyAsync(tab, h.r, h.nt * sizeof(double), hipMemcpyHostToDevice, s));
            SX_TRY_HIP(kWho, hipMemcpyAsync(tab + h.nt, h.y, h.nt * sizeof(double), hipMemcpyHostToDevice, s));
            tab += 2 * (size_t)h.nt;
        }
        else if (h.kind == SX_PROF_SOL_NOH_RHO)
        {
            d.xgeom  = h.xgeom;
            d.rho0   = h.rho0;
            d.vt     = h.vel0 * h.time;
            d.r2     = 0.5 * (h.gamma - 1) * std::fabs(h.vel0) * h.time;
            d.behind = h.rho0 * std::pow((h.gamma + 1) / (h.gamma - 1), (double)h.xgeom);
        }
    }

    const size_t n   = last - first;
    const bool   lds = b.useLds;
    // the internal bins in tiles that fit the block's LDS share, of equal size but the last; one launch per tile
    const uint32_t tileCap  = ldsBins((int)nq) + 2;
    const uint32_t tiles    = (nb2 + tileCap - 1) / tileCap;
    const uint32_t tileBins = (nb2 + tiles - 1) / tiles;
    // fixed grids: as many workgroups per CU as stay resident (pass 2: as its LDS share allows, two at the least)
    if (!b.numCus)
    {
        int dev = 0, cus = 0;
        SX_TRY_HIP(kWho, hipGetDevice(&dev));
        SX_TRY_HIP(kWho, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        b.numCus = cus > 0 ? cus : 256;
    }
    const uint32_t ldsBytes = tileBins * bytesPerBin((int)nq);
    const unsigned perCu    = lds ? std::clamp(160u * 1024u / ldsBytes, 2u, 8u) : 8u;
    const unsigned grid1    = (unsigned)std::min<size_t>(blocks(n, kBlock), 8u * b.numCus);
    const unsigned grid     = (unsigned)std::min<size_t>(blocks(n, kBlock), perCu * b.numCus);
    initKernel<<<blocks(accWords), 256, 0, s>>>(b.acc, offMin, offMax, accWords);
    SX_TRY_HIP(kWho, b.clock.mark(0, s));
    if (n) pass1Kernel<<<grid1, kBlock, 0, s>>>(a);
    SX_TRY_HIP(kWho, b.clock.mark(1, s));
    if (dist)
    {
        if (!reduce.maxU32(b.keys, kKeyWords)) return SX_ERR_HIP;
        SX_TRY_HIP(kWho, hipMemcpyAsync(b.keysHost, b.keys, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SX_TRY_HIP(kWho, hipStreamSynchronize(s));
        if (b.keysHost[0])
        {
            err = "sx_profile: refused on another rank (its sx_last_error has the reason)";
            return SX_ERR_ARG;
        }
    }
    SX_TRY_HIP(kWho, b.clock.mark(1, s));
    if (n)
    {
        if (lds)
            for (uint32_t lo = 0; lo < nb2; lo += tileBins)
            {
                a.tileLo = lo, a.tileBins = std::min(tileBins, nb2 - lo);
                pass2Kernel<true><<<grid, kBlock, ldsBytes, s>>>(a);
            }
        else pass2Kernel<false><<<grid, kBlock, 0, s>>>(a);
    }
    SX_TRY_HIP(kWho, b.clock.mark(2, s));
    if (dist)
    {
        // nonfinite, the sums and the counts are the first offMin + 1 words of acc: as limbs through the u32 sum
        const uint32_t intWords = 1 + offMin;
        toLimbsKernel<<<blocks(intWords), 256, 0, s>>>(b.acc, intWords, b.limbs);
        if (!reduce.sumU32(b.limbs, 4 * (size_t)intWords)) return SX_ERR_HIP;
        fromLimbsKernel<<<blocks(1 + nser * nb2 + nb2), 256, 0, s>>>(b.limbs, nser * nb2, nb2, b.acc);
        if (nq)
        {
            minMaxOutKernel<<<blocks(2 * nq * nb2), 256, 0, s>>>(b.acc + 1 + offMin, nq * nb2, b.minmax);
            if (!reduce.minF64(b.minmax, 2 * (size_t)nq * nb2)) return SX_ERR_HIP;
            minMaxInKernel<<<blocks(2 * nq * nb2), 256, 0, s>>>(b.minmax, nq * nb2, b.acc + 1 + offMin);
        }
        SX_TRY_HIP(kWho, b.clock.mark(2, s));
    }
    finalKernel<<<blocks(nser * nb2 + nb2 + 2 * nq * nb2 + 1), 256, 0, s>>>(b.acc, b.keys, nb2, (int)nq, b.out);
    SX_TRY_HIP(kWho, b.clock.mark(3, s));
    SX_TRY_HIP(kWho, hipGetLastError());
    SX_TRY_HIP(kWho, hipMemcpyAsync(b.outHost, b.out, nOut * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    SX_TRY_HIP(kWho, hipStreamSynchronize(s));
    b.clock.finish();
    b.passBytes = bytesPerParticle(p, std) * (double)n;
    uint64_t total = b.outHost[nb2];
    for (uint32_t k = 0; k < nb2; ++k)
        total += b.outHost[k];
    b.stats[0] = n, b.stats[1] = lds && n ? 1 : 0, b.stats[2] = n ? 1 + (lds ? tiles : 1) : 0, b.stats[3] = b.outHost[nb2];
    b.done     = true;
    if (total > kMaxParticles)
    {
        err = "sx_profile: more than 2^31 - 1 particles: the 128-bit sums are not guaranteed";
        return SX_ERR_ARG;
    }
    return SX_OK;
}

} // namespace sx::profile
