/*! @file sx_kernel_poly.hpp
 * @brief The SPH kernel W(v) = sinc(pi v / 2)^6 and dW/dv evaluated in registers (fast variant's LDS-staged pair
 *        kernels, sx_hydro_cluster.hip) instead of the reference's 20000-point lookup tables
 *        (sph/sph_kernel_tables.hpp:27-101, table_lookup.hpp:14-26).
 *
 * sinc(pi v / 2) and (d/dv sinc(pi v / 2)) / v are least-squares polynomials of degree 6 in t = v^2 on [0, 2]
 * (coefficients fitted in double, stored as float).  Evaluated in float with FMA, |W - sinc6| < 3.1e-7 and
 * |dW - sinc6d| < 8e-7 over [0, 2) (the float-interpolated tables: 1.1e-7 and 2.2e-7) -- a few float ulps of W(0) = 1
 * (tests/test_capi_cpu.py::test_kernel_poly_matches_sinc6_and_tables checks this against the exact function and the tables, through
 * sx_kernel_poly()).  Both are 0 for v >= 2, like lt::lookup's last interval.
 *
 * mapKernelY(t) is W integrated along a line of sight at impact parameter q, t = q^2 (the column maps of sx_map.hip):
 * Y(q) = 2 int_0^sqrt(4 - q^2) W(sqrt(q^2 + s^2)) ds, Y(0) = 1.09986220787, K int Y 2 pi q dq = 1.  Towards the edge
 * of the support W ~ ((2 - r) / 2)^6, so Y ~ u^6.5 with u = 1 - t / 4: a polynomial in t alone keeps an absolute error
 * floor there (degree 12 in t: 3.3e-7 Y(0) everywhere, a relative error without bound over the outer third of the disc),
 * and the maps' per-pixel relative check needs the relative error.  So Y = u^6 sqrt(u) R(u) with R = Y / u^6.5, a smooth
 * function between 0.0213 and Y(0): a least-squares polynomial of degree 10 in u on [0, 1], fitted to relative error in
 * double on 6000 Chebyshev nodes against a 200-node Gauss-Legendre quadrature, stored as float, Horner in u (which is
 * exact at the edge).  Fit error in double 1.8e-8 relative; evaluated in float with FMA on 400001 points of [0, 4]
 * (through sx_map_kernel): max |Y_poly - Y| = 5.5e-7 Y(0) -- of the order of kernelW's -- and max |Y_poly / Y - 1| =
 * 8.8e-7 for u > 1e-3; most of both is the rounding of u and of the five products behind u^6.5, not the fit (degree 9
 * fits to 1.2e-7).  Nearer the edge Y < 1e-19 Y(0) and u^6 runs into the float denormals.  u is clamped at 0: t >= 4
 * gives exactly 0 and no value is negative (tests/test_map_capi_cpu.py checks all of this through
 * sx_map_kernel()).
 */
#pragma once

#include <hip/hip_runtime.h>

namespace sx
{

//! sinc(pi v / 2) as a polynomial in t = v^2 on [0, 2] (least squares, see the file header)
__host__ __device__ __forceinline__ float sincPoly(float t)
{
    float s = 3.08339593857454e-08f;
    s       = fmaf(s, t, -2.262898533444968e-06f);
    s       = fmaf(s, t, 0.00010206655861111358f);
    s       = fmaf(s, t, -0.0029803994111716747f);
    s       = fmaf(s, t, 0.050733841955661774f);
    s       = fmaf(s, t, -0.411233514547348f);
    return fmaf(s, t, 1.0f);
}
//! (d/dv sinc(pi v / 2)) / v as a polynomial in t = v^2
__host__ __device__ __forceinline__ float dsincPolyOverV(float t)
{
    float s = 5.004272196629245e-08f;
    s       = fmaf(s, t, -2.7139270741827204e-07f);
    s       = fmaf(s, t, -1.9479362890706398e-05f);
    s       = fmaf(s, t, 0.0008091478957794607f);
    s       = fmaf(s, t, -0.01787404529750347f);
    s       = fmaf(s, t, 0.20293137431144714f);
    return fmaf(s, t, -0.8224664926528931f);
}
//! W(v) = sinc6 (sph_kernel_tables.hpp:27-40); 0 beyond the support like lt::lookup's last interval: t = v^2 is
//! clamped to 4, where sincPoly evaluates to exactly 0.0f (with or without FMA), so no compare/select is needed
__host__ __device__ __forceinline__ float kernelW(float v)
{
    float s  = sincPoly(fminf(v * v, 4.0f));
    float s2 = s * s;
    return s2 * s2 * s2;
}
//! W as a function of t = v^2 = r^2 / h^2: the pair kernels that need no |r| skip the square root
__host__ __device__ __forceinline__ float kernelWt(float t)
{
    float s  = sincPoly(fminf(t, 4.0f));
    float s2 = s * s;
    return s2 * s2 * s2;
}
//! W and v dW/dv = 6 sinc^5 t sinc'/v as functions of t = v^2
__host__ __device__ __forceinline__ void kernelWvdWt(float t, float& w, float& vdw)
{
    t        = fminf(t, 4.0f);
    float s  = sincPoly(t);
    float s2 = s * s;
    float s4 = s2 * s2;
    w        = s4 * s2;
    vdw      = 6.0f * s4 * s * t * dsincPolyOverV(t);
}
//! W and dW/dv = 6 sinc^5 sinc' (sinc6d); both exactly 0 for v >= 2 through the same clamp (s = 0)
__host__ __device__ __forceinline__ void kernelWdW(float v, float& w, float& dw)
{
    float t  = fminf(v * v, 4.0f);
    float s  = sincPoly(t);
    float s2 = s * s;
    float s4 = s2 * s2;
    w        = s4 * s2;
    dw       = 6.0f * s4 * s * v * dsincPolyOverV(t);
}

//! Y(t), t = q^2: the kernel integrated along the line of sight (see the file header); exactly 0 for t >= 4
__host__ __device__ __forceinline__ float mapKernelY(float t)
{
    const float u = fmaxf(fmaf(t, -0.25f, 1.0f), 0.0f);
    float       s = 0.0087612435387116779f;
    s             = fmaf(s, u, -0.010187234241781817f);
    s             = fmaf(s, u, 0.042689993427930437f);
    s             = fmaf(s, u, 0.030267166061782289f);
    s             = fmaf(s, u, 0.10669873237637979f);
    s             = fmaf(s, u, 0.16356153873887344f);
    s             = fmaf(s, u, 0.22687781410082566f);
    s             = fmaf(s, u, 0.23839661608874291f);
    s             = fmaf(s, u, 0.18197386561421483f);
    s             = fmaf(s, u, 0.089510442574192911f);
    s             = fmaf(s, u, 0.021312021455030951f);
    const float u2 = u * u, u4 = u2 * u2;
    return u4 * u2 * sqrtf(u) * s;
}

} // namespace sx
