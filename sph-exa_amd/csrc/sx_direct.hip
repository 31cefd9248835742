/*! @file sx_direct.hip
 * @brief direct-sum gravity on gfx950: every target of a view against all sources [0, n), over the periodic images.
 *
 * Replaces ryoanji::directSum (nbody/direct.cuh:52-123, the CPU form traversal_cpu.hpp:234-270) with the softened P2P
 * of kernel.hpp:514-535.
 *
 * Compiled twice (Makefile):
 *   -DSX_DIRECT_EXACT -ffp-contract=off   directExact: the reference's CPU loop in double, operation by operation (the
 *                                         norm2 fold a0 b0 + (a1 b1 + a2 b2), 1 / sqrt, h_i + h_j in float), images
 *                                         outermost and the sources of the split ascending inside; directCombine: the
 *                                         splits added in ascending order, the walk's output stage, egrav.
 *   -DSX_DIRECT_FAST  -ffp-contract=fast  directFast: a tile of 256 sources is loaded coalesced, converted once to
 *                                         float relative to the tile's first source (formed in double) and staged in
 *                                         LDS as pairs; the inner loop reads a pair at one address for the whole wave
 *                                         (broadcast) and evaluates it in packed FP32 with v_rsq_f32; a target is
 *                                         converted per tile and image ((x_i + shift) - origin in double, rounded
 *                                         once).  The float sums of one tile and image are folded into double
 *                                         accumulators, so the rounding of the sum does not grow with n.  The origin
 *                                         belongs to the tile, not to the target block: what a target gets does not
 *                                         depend on the view it is part of.  Rounding both coordinates relative to
 *                                         the origin leaves a pair's displacement with an absolute error of up to
 *                                         2^-24 (|s - o| + |t - o|) <= 2^-24 (2 |t - o| + R), so its force with a
 *                                         relative error of up to 6.2 * 2^-24 (2 |t - o| / R_eff + 2) (1 for dX,
 *                                         3 sqrt 3 for R_eff^-3).  Every target
 *                                         keeps the smallest R_eff it met in the tile; where that is below
 *                                         |t - o| / kOriginGuard it takes the tile again with displacements formed in
 *                                         double and rounded once (same float arithmetic).  What stays on the packed
 *                                         path is within 6.2 * 2^-23 * 17 = 1.3e-5 per pair if all three roundings
 *                                         align and a third of that in the root mean square (measured: 5.0e-6 of a
 *                                         target's sum of absolute terms at worst).  The decision belongs to
 *                                         the target and the tile alone, so views keep their bits.
 *
 * Grid: (blocks of 256 targets per target-per-lane) x (source splits).  Every (block, split) writes its sums to a
 * slab; no atomics, no communication between workgroups.
 */
#include "sx_device.hpp"
#include "sx_direct.hpp"

namespace sx::direct
{

__device__ __forceinline__ uint32_t particleOf(const DirectArgs& a, uint32_t slot)
{
    return a.targets ? a.targets[slot] : a.first + slot;
}

#ifdef SX_DIRECT_EXACT

struct __attribute__((aligned(16))) Src
{
    double x, y, z;
    float  m, h;
};

//! P2P<double, double, float, float> (kernel.hpp:514-535)
__device__ __forceinline__ void p2p(double (&acc)[4], double xi, double yi, double zi, const Src& s, float hi)
{
    const double dx = s.x - xi, dy = s.y - yi, dz = s.z - zi;
    const double R2     = dx * dx + (dy * dy + dz * dz);
    const float  h_ij   = hi + s.h;
    const float  h_ij2  = h_ij * h_ij;
    const double R2eff  = (R2 < (double)h_ij2) ? (double)h_ij2 : R2;
    const double invR   = 1.0 / sqrt(R2eff);
    const double invR2  = invR * invR;
    const double invR3m = (double)s.m * invR * invR2;
    acc[0] -= invR3m * R2;
    acc[1] += dx * invR3m;
    acc[2] += dy * invR3m;
    acc[3] += dz * invR3m;
}

__global__ __launch_bounds__(256) void directExactKernel(DirectArgs a)
{
    __shared__ Src s_src[kTile];
    const uint32_t tid   = threadIdx.x;
    const uint32_t slot  = blockIdx.x * kThreads + tid;
    const bool     valid = slot < a.numTargets;
    const uint32_t i     = particleOf(a, valid ? slot : a.numTargets - 1);
    const double   xi = a.x[i], yi = a.y[i], zi = a.z[i];
    const float    hi = a.h[i];
    const uint32_t tiles = (a.n + kTile - 1) / kTile;
    const uint32_t t0 = blockIdx.y * a.tilesPerSplit, t1 = min(t0 + a.tilesPerSplit, tiles);
    double         acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int iz = -a.numShells; iz <= a.numShells; ++iz)
        for (int iy = -a.numShells; iy <= a.numShells; ++iy)
            for (int ix = -a.numShells; ix <= a.numShells; ++ix)
            {
                const double tx = xi + ix * a.boxL[0], ty = yi + iy * a.boxL[1], tz = zi + iz * a.boxL[2];
                for (uint32_t t = t0; t < t1; ++t)
                {
                    const uint32_t j0 = t * kTile, cnt = min(kTile, a.n - j0);
                    __syncthreads();
                    if (tid < cnt) s_src[tid] = Src{a.x[j0 + tid], a.y[j0 + tid], a.z[j0 + tid], a.m[j0 + tid], a.h[j0 + tid]};
                    __syncthreads();
                    for (uint32_t s = 0; s < cnt; ++s)
                        p2p(acc, tx, ty, tz, s_src[s], hi);
                }
            }
    if (valid)
    {
        double* p = a.partial + ((size_t)blockIdx.y * a.numTargets + slot) * 4;
        p[0] = acc[0], p[1] = acc[1], p[2] = acc[2], p[3] = acc[3];
    }
}

hipError_t directExact(const DirectArgs& a, hipStream_t s)
{
    if (!a.numTargets) return hipSuccess;
    directExactKernel<<<dim3(targetBlocks(a.numTargets, 1), a.splits), kThreads, 0, s>>>(a);
    return hipGetLastError();
}

//! sum of s_u[0 .. 255] in a fixed order, in s_u[0]
__device__ __forceinline__ void blockSum(double* s_u, uint32_t tid)
{
    __syncthreads();
    for (uint32_t o = kThreads / 2; o > 0; o >>= 1)
    {
        if (tid < o) s_u[tid] += s_u[tid + o];
        __syncthreads();
    }
}

/*! the splits of a target in ascending order, then the output stage of the walk (computeGravity,
 *  traversal_cpu.hpp:218-228; directSum :265-268): u = G m_i phi_i, a += G acc */
__global__ __launch_bounds__(256) void directCombineKernel(DirectArgs a)
{
    __shared__ double s_u[kThreads];
    const uint32_t tid = threadIdx.x, slot = blockIdx.x * kThreads + tid;
    double         u = 0.0;
    if (slot < a.numTargets)
    {
        const double* p = a.partial + (size_t)slot * 4;
        double        acc[4] = {p[0], p[1], p[2], p[3]};
        for (uint32_t k = 1; k < a.splits; ++k)
        {
            const double* q = p + (size_t)k * a.numTargets * 4;
            acc[0] += q[0], acc[1] += q[1], acc[2] += q[2], acc[3] += q[3];
        }
        const uint32_t i = particleOf(a, slot);
        const double   G = (double)a.G;
        u                = (double)(a.G * a.m[i]) * acc[0];
        if (a.ax)
        {
            a.ax[i] = (float)((double)a.ax[i] + G * acc[1]);
            a.ay[i] = (float)((double)a.ay[i] + G * acc[2]);
            a.az[i] = (float)((double)a.az[i] + G * acc[3]);
        }
        if (a.out4)
        {
            double* o = a.out4 + (size_t)i * 4;
            o[0] = u, o[1] = G * acc[1], o[2] = G * acc[2], o[3] = G * acc[3];
        }
    }
    s_u[tid] = u;
    blockSum(s_u, tid);
    if (tid == 0) a.blockE[blockIdx.x] = s_u[0];
}

__global__ __launch_bounds__(256) void directEnergyKernel(const double* blockE, uint32_t nb, double* egrav)
{
    __shared__ double s_u[kThreads];
    const uint32_t tid = threadIdx.x;
    double         u = 0.0;
    for (uint32_t b = tid; b < nb; b += kThreads)
        u += blockE[b];
    s_u[tid] = u;
    blockSum(s_u, tid);
    if (tid == 0) *egrav = 0.5 * s_u[0];
}

hipError_t directCombine(const DirectArgs& a, hipStream_t s)
{
    if (!a.numTargets) return hipSuccess;
    const uint32_t nb = combineBlocks(a.numTargets);
    directCombineKernel<<<nb, kThreads, 0, s>>>(a);
    directEnergyKernel<<<1, kThreads, 0, s>>>(a.blockE, nb, a.egrav);
    return hipGetLastError();
}

#endif // SX_DIRECT_EXACT

#ifdef SX_DIRECT_FAST

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr float kOriginGuard = 16.0f; //!< |t - o| / R_eff beyond which a target takes a tile in double (file comment)

/*! NT targets per lane.  LDS per pair of sources P: s_A[P] = {x0, x1, y0, y1}, s_B[P] = {z0, z1, m0, m1},
 *  s_H[P] = {h0, h1}, coordinates relative to the tile's origin.  The padding of the last tile sits at the origin with
 *  m = 0, h = 1 and adds exact zeros. */
template<int NT>
__global__ __launch_bounds__(256) void directFastKernel(DirectArgs a)
{
    __shared__ float4 s_A[kTile / 2], s_B[kTile / 2];
    __shared__ float2 s_H[kTile / 2];
    const uint32_t tid  = threadIdx.x;
    const uint32_t base = blockIdx.x * kThreads * NT;
    bool           valid[NT];
    uint32_t       slot[NT];
    double         xi[NT], yi[NT], zi[NT];
    v2f            th[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
    {
        slot[t]          = base + t * kThreads + tid;
        valid[t]         = slot[t] < a.numTargets;
        const uint32_t i = particleOf(a, valid[t] ? slot[t] : a.numTargets - 1);
        xi[t] = a.x[i], yi[t] = a.y[i], zi[t] = a.z[i];
        const float hi = a.h[i];
        th[t]          = v2f{hi, hi};
    }
    const uint32_t tiles = (a.n + kTile - 1) / kTile;
    const uint32_t t0 = blockIdx.y * a.tilesPerSplit, t1 = min(t0 + a.tilesPerSplit, tiles);
    double         acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.0;

    for (uint32_t tile = t0; tile < t1; ++tile)
    {
        const uint32_t j0 = tile * kTile, cnt = min(kTile, a.n - j0);
        const double   ox = a.x[j0], oy = a.y[j0], oz = a.z[j0]; // the tile's origin: its first source
        const uint32_t j  = j0 + tid;
        const bool     in = tid < cnt;
        const float    rx = in ? (float)(a.x[j] - ox) : 0.0f, ry = in ? (float)(a.y[j] - oy) : 0.0f;
        const float    rz = in ? (float)(a.z[j] - oz) : 0.0f;
        const float    mj = in ? a.m[j] : 0.0f, hj = in ? a.h[j] : 1.0f;
        __syncthreads(); // the previous tile has been read
        {
            const uint32_t P = tid >> 1, hf = tid & 1;
            float*         A = reinterpret_cast<float*>(&s_A[P]);
            float*         B = reinterpret_cast<float*>(&s_B[P]);
            A[hf] = rx, A[2 + hf] = ry, B[hf] = rz, B[2 + hf] = mj;
            reinterpret_cast<float*>(&s_H[P])[hf] = hj;
        }
        __syncthreads();
        const uint32_t pairs = (cnt + 1) >> 1;
        for (int iz = -a.numShells; iz <= a.numShells; ++iz)
            for (int iy = -a.numShells; iy <= a.numShells; ++iy)
                for (int ix = -a.numShells; ix <= a.numShells; ++ix)
                {
                    v2f   tx[NT], ty[NT], tz[NT], f2[NT][4];
                    float rmin[NT], far2[NT]; // smallest R_eff^2 met, (|t - o| / kOriginGuard)^2
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                    {
                        // the image shifts the target in double; one rounding, of the difference to the origin
                        const float x = (float)((xi[t] + ix * a.boxL[0]) - ox);
                        const float y = (float)((yi[t] + iy * a.boxL[1]) - oy);
                        const float z = (float)((zi[t] + iz * a.boxL[2]) - oz);
                        tx[t] = v2f{x, x}, ty[t] = v2f{y, y}, tz[t] = v2f{z, z};
                        f2[t][0] = f2[t][1] = f2[t][2] = f2[t][3] = v2f{0.0f, 0.0f};
                        rmin[t] = INFINITY;
                        far2[t] = (x * x + y * y + z * z) * (1.0f / (kOriginGuard * kOriginGuard));
                    }
#pragma unroll 4
                    for (uint32_t P = 0; P < pairs; ++P)
                    {
                        // one address for the whole wave: broadcast reads
                        const float4 A = s_A[P], B = s_B[P];
                        const float2 H = s_H[P];
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                        {
                            const v2f dx = v2f{A.x, A.y} - tx[t], dy = v2f{A.z, A.w} - ty[t], dz = v2f{B.x, B.y} - tz[t];
                            const v2f R2 =
                                __builtin_elementwise_fma(dx, dx, __builtin_elementwise_fma(dy, dy, dz * dz));
                            const v2f h_ij = th[t] + v2f{H.x, H.y};
                            const v2f hh   = h_ij * h_ij;
                            const v2f Re2  = {fmaxf(R2.x, hh.x), fmaxf(R2.y, hh.y)};
                            const v2f invR = {__builtin_amdgcn_rsqf(Re2.x), __builtin_amdgcn_rsqf(Re2.y)};
                            rmin[t]        = fminf(fminf(rmin[t], Re2.x), Re2.y); // one v_min3_f32
                            const v2f invR3m = v2f{B.z, B.w} * invR * invR * invR;
                            f2[t][0] = __builtin_elementwise_fma(-invR3m, R2, f2[t][0]);
                            f2[t][1] = __builtin_elementwise_fma(dx, invR3m, f2[t][1]);
                            f2[t][2] = __builtin_elementwise_fma(dy, invR3m, f2[t][2]);
                            f2[t][3] = __builtin_elementwise_fma(dz, invR3m, f2[t][3]);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                    {
                        if (rmin[t] < far2[t])
                        {
                            // a source this close to a target this far from the origin: the tile again, displacements
                            // formed in double and rounded once (the padding of the last tile is not visited)
                            const double xt = xi[t] + ix * a.boxL[0], yt = yi[t] + iy * a.boxL[1];
                            const double zt = zi[t] + iz * a.boxL[2];
                            float        g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                            for (uint32_t s = 0; s < cnt; ++s)
                            {
                                const float dx = (float)(a.x[j0 + s] - xt), dy = (float)(a.y[j0 + s] - yt);
                                const float dz = (float)(a.z[j0 + s] - zt);
                                const float R2   = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                                const float h_ij = th[t].x + a.h[j0 + s];
                                const float invR = __builtin_amdgcn_rsqf(fmaxf(R2, h_ij * h_ij));
                                const float invR3m = a.m[j0 + s] * invR * invR * invR;
                                g[0] = fmaf(-invR3m, R2, g[0]);
                                g[1] = fmaf(dx, invR3m, g[1]);
                                g[2] = fmaf(dy, invR3m, g[2]);
                                g[3] = fmaf(dz, invR3m, g[3]);
                            }
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                acc[t][c] += (double)g[c];
                        }
                        else
                        {
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                acc[t][c] += (double)f2[t][c].x + (double)f2[t][c].y;
                        }
                    }
                }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (valid[t])
        {
            double* p = a.partial + ((size_t)blockIdx.y * a.numTargets + slot[t]) * 4;
            p[0] = acc[t][0], p[1] = acc[t][1], p[2] = acc[t][2], p[3] = acc[t][3];
        }
}

hipError_t directFast(const DirectArgs& a, hipStream_t s)
{
    if (!a.numTargets) return hipSuccess;
    const dim3 grid(targetBlocks(a.numTargets, a.targetsPerLane), a.splits);
    if (a.targetsPerLane == 2) directFastKernel<2><<<grid, kThreads, 0, s>>>(a);
    else directFastKernel<1><<<grid, kThreads, 0, s>>>(a);
    return hipGetLastError();
}

#endif // SX_DIRECT_FAST

} // namespace sx::direct
