/*! @file sx_cellgrid.hpp
 * @brief The cell grid under the pair searches within a fixed length (sx_fof.hip: the linking length, sx_twopoint.hip:
 *        r_max): the rule for the cells per axis, the index of the particles by cell and its build (sx_cellgrid.hip),
 *        the cell of a coordinate, the minimum image and the walk over the 27 cells round one.
 *
 * Cells of edge > length, x-fastest key cx + dx (cy + dy cz), particles sorted by key: the 27 cells around a particle are
 * nine x-runs of up to three cells, each one contiguous range of the sorted particles (a run that wraps round a periodic
 * x axis adds the cell at the far end as a range of its own).  The cell count is capped at max(27, 2 n), so a sparse set
 * gets cells wider than the length instead of a start array larger than its columns.  hipcub stays in sx_cellgrid.hip:
 * this header is reached from every file of the step driver.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/sphexa_hip.h"
#include "sx_tree.hpp"

namespace sx::cellgrid
{

constexpr uint32_t kMaxDim = 1024; //!< cells per axis: keys stay below 2^30
constexpr int      kBlock  = 256;

/*! per axis floor(L / length (1 - 2^-20)) cells, at least 1 (3 on a periodic axis) and at most kMaxDim; then, while the
 *  cells number more than max(27, 2 n), the axis with the most cells (the first of equals) takes ceil(dims / 2) */
inline void chooseDims(double length, const sx_box& box, uint64_t n, uint32_t dims[3])
{
    uint32_t lowest[3];
    for (int a = 0; a < 3; ++a)
    {
        const double L = box.lim[2 * a + 1] - box.lim[2 * a];
        const double q = std::floor(L / length * (1.0 - 0x1p-20));
        lowest[a]      = box.bnd[a] == 1 ? 3 : 1;
        dims[a]        = q >= (double)kMaxDim ? kMaxDim : q >= (double)lowest[a] ? (uint32_t)q : lowest[a];
    }
    const uint64_t limit = std::max<uint64_t>(27, 2 * n);
    while ((uint64_t)dims[0] * dims[1] * dims[2] > limit)
    {
        int a = 0;
        for (int k = 1; k < 3; ++k)
            if (dims[k] > dims[a]) a = k;
        dims[a] = std::max(lowest[a], (dims[a] + 1) / 2);
    }
}

struct Grid
{
    double   lo[3], hi[3], len[3], half[3], inv[3]; // inv: cells per unit length (0 on an axis without extent)
    uint32_t dims[3];
    int      pbc[3];
    double   l2;
};

//! the grid of dims cells over box; l2 = length^2
inline Grid makeGrid(const sx_box& box, const uint32_t dims[3], double length)
{
    Grid g{};
    for (int a = 0; a < 3; ++a)
    {
        g.lo[a] = box.lim[2 * a], g.hi[a] = box.lim[2 * a + 1];
        g.len[a]  = g.hi[a] - g.lo[a];
        g.half[a] = 0.5 * g.len[a];
        g.dims[a] = dims[a];
        g.inv[a]  = g.len[a] > 0.0 && std::isfinite(g.len[a]) ? dims[a] / g.len[a] : 0.0;
        g.pbc[a]  = box.bnd[a] == 1;
    }
    g.l2 = length * length;
    return g;
}

/*! the particles of a range by cell: the typed owner of <prefix>keys, keysSorted, idx, order, cellCount, cellStart and
 *  sortTmp (prefix "fof." or "twopoint."), requested at one site, in build, which stores the pointers here */
struct Index
{
    uint32_t *keys{nullptr}, *keysSorted{nullptr}, *idx{nullptr}, *order{nullptr}; // order[s]: column index - first
    uint32_t *cellCount{nullptr}, *cellStart{nullptr};                              // cells + 1
    void*     sortTmp{nullptr}; // tmpBytes: hipcub's temporary storage, the client's further sorts and scans included
    uint32_t  cells{0};
    int       keyBits{1}; // of the largest key, at least 1: the bits the sort looks at
    size_t    tmpBytes{0};
};

/*! the index of the particles [first, first + n) in the cells of g: keys and cell counts, the particles sorted by
 *  key, the exclusive sum of the counts over cells + 1.  sortTmp is sized once, for the sort, the scan and the
 *  minTmpBytes of the client's own hipcub calls.  n == 0: the buffers and no launch; n < 2^31.  who: for the messages */
int build(Arena& arena, const std::string& tagPrefix, Index& ix, const Grid& g, const double* x, const double* y,
          const double* z, uint32_t first, uint32_t n, size_t minTmpBytes, hipStream_t s, const char* who,
          std::string& err);

__device__ __forceinline__ uint32_t cellOf(double v, const Grid& g, int a)
{
    const double t = (v - g.lo[a]) * g.inv[a];
    if (!(fabs(t) < 1e15)) return 0; // not a number, or far outside: any cell will do, it has no friends
    long long       c = (long long)floor(t);
    const long long d = g.dims[a];
    if (g.pbc[a])
    {
        c %= d;
        if (c < 0) c += d;
    }
    else c = c < 0 ? 0 : c > d - 1 ? d - 1 : c;
    return (uint32_t)c;
}

__device__ __forceinline__ double minImage(double d, int pbc, double half, double len)
{
    if (pbc)
    {
        if (d > half) d -= len;
        else if (d < -half) d += len;
    }
    return d;
}

/*! the ranges of the sorted particles in the 27 cells around the cell `key`: visit(begin, end) per range, nine x-runs
 *  and, round a periodic x axis, the cell at the far end */
template<class Visit>
__device__ __forceinline__ void forEachRun(const Grid& g, uint32_t key, const uint32_t* __restrict__ cellStart,
                                           Visit&& visit)
{
    const int dx = (int)g.dims[0], dy = (int)g.dims[1], dz = (int)g.dims[2];
    const int cx = (int)(key % g.dims[0]), cy = (int)((key / g.dims[0]) % g.dims[1]);
    const int cz = (int)(key / (g.dims[0] * g.dims[1]));
    for (int oz = -1; oz <= 1; ++oz)
    {
        int zc = cz + oz;
        if (zc < 0 || zc >= dz)
        {
            if (!g.pbc[2]) continue;
            zc += zc < 0 ? dz : -dz;
        }
        for (int oy = -1; oy <= 1; ++oy)
        {
            int yc = cy + oy;
            if (yc < 0 || yc >= dy)
            {
                if (!g.pbc[1]) continue;
                yc += yc < 0 ? dy : -dy;
            }
            const uint32_t row = (uint32_t)dx * ((uint32_t)yc + (uint32_t)dy * (uint32_t)zc);
            const int      xl = cx > 0 ? cx - 1 : 0, xh = cx < dx - 1 ? cx + 1 : dx - 1;
            visit(cellStart[row + xl], cellStart[row + xh + 1]);
            if (g.pbc[0]) // three cells or more: the far end is not in the run above
            {
                if (cx == 0) visit(cellStart[row + dx - 1], cellStart[row + dx]);
                else if (cx == dx - 1) visit(cellStart[row], cellStart[row + 1]);
            }
        }
    }
}

} // namespace sx::cellgrid
