/*! @file sx_nbody.hip
 * @brief nbodyIntegrateKernel: the position update of the gravity-only propagator (NbodyProp::integrate,
 *        main/src/propagator/nbody.hpp:152-163: computePositions without temp and u).
 *
 * positionUpdate (positions.hpp:77-88) in the reference's operation order, the fixed-boundary skip (:102-110) and
 * putInBox, as positionsKernel (sx_hydro.hip) does them, without the energy update: no thermal field is touched.
 * Per particle the pass reads x y z (24 B), x_m1 y_m1 z_m1 (12 B) and ax ay az (12 B) and writes x y z (24 B),
 * vx vy vz (12 B), x_m1 y_m1 z_m1 (12 B) and the SFC key of the new coordinates (8 B): 104 B.  v and h are read only
 * in a box with a fixed axis (the skip's test).  Compiled without contraction: x is bit-equal to the CPU reference.
 */
#include "sx_nbody.hpp"
#include "sx_sfc.hpp"

namespace sx
{

namespace
{

constexpr int kNbBlock = 256;

//! one particle in registers
struct Body
{
    double X[3];
    float  dX[3], A[3], V[3], h;
};

//! positionUpdate + putInBox of one particle; fixed: some axis of b is fixed (then p.V and p.h are loaded)
__device__ __forceinline__ void pressUpdate(Body& p, const DevBox& b, bool fixed, double dt, double dt_m1)
{
    if (fixed && p.V[0] == 0.0f && p.V[1] == 0.0f && p.V[2] == 0.0f)
    {
        bool skip = false;
#pragma unroll
        for (int d = 0; d < 3; ++d)
        {
            const double top = b.lim[2 * d + 1], bot = b.lim[2 * d];
            if (b.fbc[d] && (fabs(top - p.X[d]) < 2.0f * p.h || fabs(bot - p.X[d]) < 2.0f * p.h)) skip = true;
        }
        if (skip) return; // a resting particle inside 2h of a fixed wall stays (positions.hpp:102-110)
    }
    const double inv = 1.0 / dt_m1, hdm1 = 0.5 * dt_m1, adt = fabs(dt);
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const double A       = p.A[k];
        const double Vnmhalf = (double)p.dX[k] * inv;
        const double Vn      = Vnmhalf + A * hdm1;
        const double Vn1     = Vn + A * dt;
        const double dXn1    = (Vn + (A * 0.5) * adt) * dt;
        double       Xn      = p.X[k] + dXn1;
        if (b.pbc[k] && Xn > b.lim[2 * k + 1]) Xn -= b.l[k];
        else if (b.pbc[k] && Xn < b.lim[2 * k]) Xn += b.l[k];
        p.X[k]  = Xn;
        p.dX[k] = (float)dXn1;
        p.V[k]  = (float)Vn1;
    }
}

__device__ __forceinline__ void loadOne(const NbodyPosArgs& a, uint32_t i, bool fixed, Body& p)
{
    p.X[0] = a.x[i], p.X[1] = a.y[i], p.X[2] = a.z[i];
    p.dX[0] = a.x_m1[i], p.dX[1] = a.y_m1[i], p.dX[2] = a.z_m1[i];
    p.A[0] = a.ax[i], p.A[1] = a.ay[i], p.A[2] = a.az[i];
    p.V[0] = p.V[1] = p.V[2] = 0.0f, p.h = 0.0f;
    if (fixed) p.V[0] = a.vx[i], p.V[1] = a.vy[i], p.V[2] = a.vz[i], p.h = a.h[i];
}

__device__ __forceinline__ void storeOne(const NbodyPosArgs& a, uint32_t i, const Body& p)
{
    a.x[i] = p.X[0], a.y[i] = p.X[1], a.z[i] = p.X[2];
    a.x_m1[i] = p.dX[0], a.y_m1[i] = p.dX[1], a.z_m1[i] = p.dX[2];
    a.vx[i] = p.V[0], a.vy[i] = p.V[1], a.vz[i] = p.V[2];
    if (a.keys) a.keys[i] = sfcKey(p.X[0], p.X[1], p.X[2], a.box);
}

/*! W = 1: lane t takes particle first + t.  W = 2: lane t takes the aligned pair {2q, 2q + 1}, q = first / 2 + t, with
 *  one 16-byte access per double field and one 8-byte access per float field; a pair that straddles first or last
 *  goes through the one-particle path for its member inside the range. */
template<int W>
__global__ __launch_bounds__(kNbBlock) void nbodyIntegrateKernel(NbodyPosArgs a)
{
    const DevBox& b     = a.box;
    const bool    fixed = b.fbc[0] || b.fbc[1] || b.fbc[2];
    const double  dt = a.dtPtr ? a.dtPtr[0] : a.dt, dt_m1 = a.dtPtr ? a.dtPtr[1] : a.dt_m1;
    const uint32_t t = blockIdx.x * kNbBlock + threadIdx.x;
    if constexpr (W == 1)
    {
        // (t < last - first: no wrap of first + t)
        if (t >= a.last - a.first) return;
        Body p;
        loadOne(a, a.first + t, fixed, p);
        pressUpdate(p, b, fixed, dt, dt_m1);
        storeOne(a, a.first + t, p);
    }
    else
    {
        const uint32_t q0 = a.first >> 1, q1 = (a.last + 1u) >> 1; // pairs [q0, q1) cover [first, last)
        if (t >= q1 - q0) return;
        const uint32_t i0 = 2u * (q0 + t);
        if (i0 >= a.first && i0 + 1u < a.last)
        {
            Body p[2];
            const double2 X = *reinterpret_cast<const double2*>(a.x + i0), Y = *reinterpret_cast<const double2*>(a.y + i0),
                          Z = *reinterpret_cast<const double2*>(a.z + i0);
            const float2 dx = *reinterpret_cast<const float2*>(a.x_m1 + i0),
                         dy = *reinterpret_cast<const float2*>(a.y_m1 + i0),
                         dz = *reinterpret_cast<const float2*>(a.z_m1 + i0);
            const float2 ax = *reinterpret_cast<const float2*>(a.ax + i0), ay = *reinterpret_cast<const float2*>(a.ay + i0),
                         az = *reinterpret_cast<const float2*>(a.az + i0);
            p[0].X[0] = X.x, p[0].X[1] = Y.x, p[0].X[2] = Z.x, p[1].X[0] = X.y, p[1].X[1] = Y.y, p[1].X[2] = Z.y;
            p[0].dX[0] = dx.x, p[0].dX[1] = dy.x, p[0].dX[2] = dz.x, p[1].dX[0] = dx.y, p[1].dX[1] = dy.y, p[1].dX[2] = dz.y;
            p[0].A[0] = ax.x, p[0].A[1] = ay.x, p[0].A[2] = az.x, p[1].A[0] = ax.y, p[1].A[1] = ay.y, p[1].A[2] = az.y;
#pragma unroll
            for (int e = 0; e < 2; ++e)
                p[e].V[0] = p[e].V[1] = p[e].V[2] = 0.0f, p[e].h = 0.0f;
            if (fixed)
            {
                const float2 vx = *reinterpret_cast<const float2*>(a.vx + i0), vy = *reinterpret_cast<const float2*>(a.vy + i0),
                             vz = *reinterpret_cast<const float2*>(a.vz + i0), hh = *reinterpret_cast<const float2*>(a.h + i0);
                p[0].V[0] = vx.x, p[0].V[1] = vy.x, p[0].V[2] = vz.x, p[0].h = hh.x;
                p[1].V[0] = vx.y, p[1].V[1] = vy.y, p[1].V[2] = vz.y, p[1].h = hh.y;
            }
            pressUpdate(p[0], b, fixed, dt, dt_m1);
            pressUpdate(p[1], b, fixed, dt, dt_m1);
            *reinterpret_cast<double2*>(a.x + i0)   = make_double2(p[0].X[0], p[1].X[0]);
            *reinterpret_cast<double2*>(a.y + i0)   = make_double2(p[0].X[1], p[1].X[1]);
            *reinterpret_cast<double2*>(a.z + i0)   = make_double2(p[0].X[2], p[1].X[2]);
            *reinterpret_cast<float2*>(a.x_m1 + i0) = make_float2(p[0].dX[0], p[1].dX[0]);
            *reinterpret_cast<float2*>(a.y_m1 + i0) = make_float2(p[0].dX[1], p[1].dX[1]);
            *reinterpret_cast<float2*>(a.z_m1 + i0) = make_float2(p[0].dX[2], p[1].dX[2]);
            *reinterpret_cast<float2*>(a.vx + i0)   = make_float2(p[0].V[0], p[1].V[0]);
            *reinterpret_cast<float2*>(a.vy + i0)   = make_float2(p[0].V[1], p[1].V[1]);
            *reinterpret_cast<float2*>(a.vz + i0)   = make_float2(p[0].V[2], p[1].V[2]);
            if (a.keys)
                *reinterpret_cast<ulonglong2*>(a.keys + i0) =
                    make_ulonglong2(sfcKey(p[0].X[0], p[0].X[1], p[0].X[2], b), sfcKey(p[1].X[0], p[1].X[1], p[1].X[2], b));
        }
        else
        {
#pragma unroll
            for (uint32_t e = 0; e < 2; ++e)
            {
                const uint32_t i = i0 + e;
                if (i < a.first || i >= a.last) continue;
                Body p;
                loadOne(a, i, fixed, p);
                pressUpdate(p, b, fixed, dt, dt_m1);
                storeOne(a, i, p);
            }
        }
    }
}

bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

} // namespace

hipError_t nbodyIntegrate(const NbodyPosArgs& a, hipStream_t s)
{
    if (a.last <= a.first) return hipSuccess;
    const bool fixed = a.box.fbc[0] || a.box.fbc[1] || a.box.fbc[2];
    bool       wide  = aligned(a.x, 16) && aligned(a.y, 16) && aligned(a.z, 16) && (!a.keys || aligned(a.keys, 16));
    for (const void* f : {(const void*)a.x_m1, (const void*)a.y_m1, (const void*)a.z_m1, (const void*)a.vx,
                          (const void*)a.vy, (const void*)a.vz, (const void*)a.ax, (const void*)a.ay, (const void*)a.az})
        wide = wide && aligned(f, 8);
    if (fixed) wide = wide && aligned(a.h, 8);
    if (wide)
    {
        const uint32_t pairs = ((a.last + 1u) >> 1) - (a.first >> 1);
        nbodyIntegrateKernel<2><<<(pairs + kNbBlock - 1) / kNbBlock, kNbBlock, 0, s>>>(a);
    }
    else
    {
        const uint32_t n = a.last - a.first;
        nbodyIntegrateKernel<1><<<(n + kNbBlock - 1) / kNbBlock, kNbBlock, 0, s>>>(a);
    }
    return hipGetLastError();
}

} // namespace sx
