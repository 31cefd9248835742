/*! @file sx_cool.hpp
 * @brief optically thin radiative cooling: the host table behind sx_cooling_* (sx_cooling.cpp), the one statement of
 *        the per-particle arithmetic that the host evaluators and the kernels share, and the launchers of the two
 *        kernels (sx_cool.hip).
 *
 * Model: dT/dt = -rho L(T) / cv at fixed rho over the step, L a power law on each segment of a table
 * T_1 < ... < T_N, L(T) = L_k (T / T_k)^alpha_k on [T_k, T_k+1]; the last segment's law continues above T_N and
 * L = 0 below T_1, the temperature floor.  Integrated exactly (Townsend 2009, ApJS 181, 391): with the temporal
 * evolution function
 *     Y(T) = (L_N / T_N) int_T^T_N dT' / L(T')        (dimensionless, Y(T_N) = 0, growing as T falls)
 * the solution after s = rho dt / cv is Y(T_new) = Y(T_old) + (L_N / T_N) s, unconditionally stable for any s.  On
 * segment k, with x = T / T_k,
 *     Y(T) = Y_k - c_k g_k(x),  c_k = (L_N / T_N)(T_k / L_k),
 *     g_k(x) = expm1((1 - alpha_k) ln x) / (1 - alpha_k)   and its inverse  exp(log1p((1 - alpha_k) z) / (1 - alpha_k)),
 * ln x and exp z where alpha_k == 1 exactly: one code path, no threshold on |1 - alpha|.
 *
 * Everything is double and is written one operation at a time; the translation units that include this compile with
 * -ffp-contract=off, so tests/cooling_ref.py repeats it operation by operation.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/sphexa_hip.h"

//! the table of sx_cooling_create: nodes, values, and what create derives from them
struct sx_cooling
{
    std::vector<double> T, lambda, alpha, Y; // N each; alpha[N-1] = alpha[N-2] (the law that continues above T_N)
};

namespace sx::cool
{

//! the table as the kernels read it: [T | lambda | alpha | Y], N each
inline std::vector<double> packedTable(const sx_cooling& c)
{
    std::vector<double> p;
    for (const auto* v : {&c.T, &c.lambda, &c.alpha, &c.Y})
        p.insert(p.end(), v->begin(), v->end());
    return p;
}

constexpr uint32_t kMaxNodes   = 256; //!< SX_COOLING_MAX_NODES
constexpr int      kSearchSteps = 8;   //!< binary search over at most 256 nodes, the same count for every lane

//! the table as the arithmetic reads it (host vectors, or the block's LDS copy)
struct Table
{
    const double *T, *L, *alpha, *Y;
    uint32_t      n;
};

//! largest k <= n - 2 with key(k) true, key true on a prefix of the nodes and at 0; a fixed number of iterations
template<class Key>
__host__ __device__ inline uint32_t searchPrefix(uint32_t n, Key&& key)
{
    uint32_t lo = 0;
#pragma unroll
    for (int b = kSearchSteps - 1; b >= 0; --b)
    {
        const uint32_t cand = lo + (1u << b);
        if (cand + 2 <= n && key(cand)) lo = cand;
    }
    return lo;
}

//! g_k(x) of the file comment
__host__ __device__ inline double segIntegral(double alpha, double lnx)
{
    const double om = 1.0 - alpha;
    return alpha == 1.0 ? lnx : expm1(om * lnx) / om;
}

//! its inverse, as a factor on T_k
__host__ __device__ inline double segInverse(double alpha, double z)
{
    const double om = 1.0 - alpha;
    return alpha == 1.0 ? exp(z) : exp(log1p(om * z) / om);
}

//! L(T): 0 below the floor (and for a NaN), the segment's power law from there on
__host__ __device__ inline double rate(const Table& t, double T)
{
    if (!(T >= t.T[0])) return 0.0;
    const uint32_t k = searchPrefix(t.n, [&](uint32_t c) { return t.T[c] <= T; });
    return t.L[k] * exp(t.alpha[k] * log(T / t.T[k]));
}

//! cv T / (rho L(T)), +inf where L = 0
__host__ __device__ inline double coolingTime(const Table& t, double T, double rho, double cv)
{
    const double L = rate(t, T);
    if (L == 0.0) return INFINITY;
    return (cv * T) / (rho * L);
}

/*! T after s = rho dt / cv.  The source segment k is found by T, the target segment j by a search on Y, so the
 *  inverse's argument lies inside its segment; a particle that stays on its segment advances z itself (no Y_k to
 *  cancel against: a step that cools by 1e-12 T keeps its digits).  Exact whatever rounding does: the result is never
 *  above T0, never below the floor for T0 on or above it, T0 itself for s == 0 and for T0 below the floor (or NaN). */
__host__ __device__ inline double integrate(const Table& t, double T0, double s)
{
    const double T1 = t.T[0];
    if (!(T0 >= T1) || s == 0.0) return T0;
    const uint32_t N    = t.n;
    const double   norm = t.L[N - 1] / t.T[N - 1];
    const uint32_t k    = searchPrefix(N, [&](uint32_t c) { return t.T[c] <= T0; });
    const double   ak   = t.alpha[k];
    const double   ck   = norm * (t.T[k] / t.L[k]);
    const double   z0   = segIntegral(ak, log(T0 / t.T[k]));
    const double   Y0   = t.Y[k] - ck * z0;
    const double   d    = norm * s;
    const double   Yn   = Y0 + d;
    double         Tn;
    if (Yn >= t.Y[0]) Tn = T1;
    else
    {
        const uint32_t j  = searchPrefix(N, [&](uint32_t c) { return t.Y[c] >= Yn; });
        const double   cj = norm * (t.T[j] / t.L[j]);
        const double   z  = j == k ? z0 - d / ck : (t.Y[j] - Yn) / cj;
        Tn                = t.T[j] * segInverse(t.alpha[j], z);
    }
    if (!(Tn <= T0)) Tn = T0;
    if (Tn < T1) Tn = T1;
    return Tn;
}

//! rho of a particle: the std propagator's column, or (kx m) / xm of the VE propagator in float (rho == nullptr)
struct Density
{
    const float *rho, *kx, *xm, *m;
};

struct CoolArgs
{
    uint32_t      n;
    Density       d;
    const float*  m;
    double*       temp; // updated in place
    double        cv;
    double        dt;    // used when dtPtr == nullptr
    const double* dtPtr; // the step's minDt on the device
    // table on the device: T, L, alpha, Y, numNodes each
    const double* table;
    uint32_t      numNodes;
    // block partials (partialBlocks(n) each) and the result {energy radiated, on the floor, cooled}
    double*   ePart;
    uint32_t* cPart; // 2 per block: on the floor, cooled
    double*   stats;
    double*   total; // nullable: += energy radiated (the sim's running total)
};

struct CoolTimeArgs
{
    uint32_t            n;
    Density             d;
    const double*       temp;
    double              cv;
    const double*       table;
    uint32_t            numNodes;
    unsigned long long* minBits; // bit image of the minimum, a non-negative double; set to +inf by the launcher
};

//! the number of block partials of sx_cool for n particles: a function of n alone
uint32_t partialBlocks(uint32_t n);
hipError_t coolLaunch(const CoolArgs& a, hipStream_t s);
hipError_t coolingTimeLaunch(const CoolTimeArgs& a, hipStream_t s);
//! *out = factor * (the double behind *minBits), on the stream (the step's minDtCool)
hipError_t scaledMin(const unsigned long long* minBits, double factor, double* out, hipStream_t s);

} // namespace sx::cool
