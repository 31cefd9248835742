/*! @file sx_cellgrid.hip
 * @brief The build of the cell index (sx_cellgrid.hpp): the key kernel, the sort by key and the scan of the cell counts.
 *        Built with -ffp-contract=off, as its clients are. */
#include <hipcub/hipcub.hpp>

#include "sx_cellgrid.hpp"
#include "sx_exactsum.hpp"

namespace sx::cellgrid
{

namespace
{

//! key, identity index and cell count of the particles [first, first + n)
__global__ __launch_bounds__(kBlock) void keyKernel(const double* __restrict__ x, const double* __restrict__ y,
                                                    const double* __restrict__ z, uint32_t first, uint32_t n, Grid g,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                    uint32_t* __restrict__ cellCount)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t   p   = (size_t)first + i;
    const uint32_t key = cellOf(x[p], g, 0) + g.dims[0] * (cellOf(y[p], g, 1) + g.dims[1] * cellOf(z[p], g, 2));
    keys[i]            = key;
    idx[i]             = i;
    atomicAdd(cellCount + key, 1u);
}

} // namespace

int build(Arena& arena, const std::string& tagPrefix, Index& ix, const Grid& g, const double* x, const double* y,
          const double* z, uint32_t first, uint32_t n, size_t minTmpBytes, hipStream_t s, const char* who,
          std::string& err)
{
    ix.cells    = g.dims[0] * g.dims[1] * g.dims[2];
    ix.keyBits  = std::max(1, exact::bitLength(ix.cells - 1));
    const size_t starts = (size_t)ix.cells + 1;
    size_t       sortTmp = 0, scanTmp = 0; // a size query reads no pointer
    if (n)
    {
        SX_TRY_HIP(who, hipcub::DeviceRadixSort::SortPairs(nullptr, sortTmp, ix.keys, ix.keysSorted, ix.idx, ix.order,
                                                           (int)n, 0, 32, s));
        SX_TRY_HIP(who, hipcub::DeviceScan::ExclusiveSum(nullptr, scanTmp, ix.cellCount, ix.cellStart, (int)starts, s));
    }
    ix.tmpBytes = std::max({minTmpBytes, sortTmp, scanTmp});
    ix.keys       = arena.get<uint32_t>(tagPrefix + "keys", n);
    ix.keysSorted = arena.get<uint32_t>(tagPrefix + "keysSorted", n);
    ix.idx        = arena.get<uint32_t>(tagPrefix + "idx", n);
    ix.order      = arena.get<uint32_t>(tagPrefix + "order", n);
    ix.cellCount  = arena.get<uint32_t>(tagPrefix + "cellCount", starts);
    ix.cellStart  = arena.get<uint32_t>(tagPrefix + "cellStart", starts);
    ix.sortTmp    = arena.get<char>(tagPrefix + "sortTmp", ix.tmpBytes);
    if (!ix.keys || !ix.keysSorted || !ix.idx || !ix.order || !ix.cellCount || !ix.cellStart || !ix.sortTmp)
    {
        err = std::string(who) + ": scratch buffers";
        return SX_ERR_NOMEM;
    }
    if (n == 0) return SX_OK;
    SX_TRY_HIP(who, hipMemsetAsync(ix.cellCount, 0, starts * sizeof(uint32_t), s));
    keyKernel<<<blocks(n, kBlock), kBlock, 0, s>>>(x, y, z, first, n, g, ix.keys, ix.idx, ix.cellCount);
    SX_TRY_HIP(who, hipcub::DeviceRadixSort::SortPairs(ix.sortTmp, ix.tmpBytes, ix.keys, ix.keysSorted, ix.idx,
                                                       ix.order, (int)n, 0, ix.keyBits, s));
    SX_TRY_HIP(who, hipcub::DeviceScan::ExclusiveSum(ix.sortTmp, ix.tmpBytes, ix.cellCount, ix.cellStart,
                                                     (int)starts, s));
    return SX_OK;
}

} // namespace sx::cellgrid
