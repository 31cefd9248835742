/*! @file sx_pairbin.hip
 * @brief The pair-binning engine's host side (sx_pairbin.hpp): the band plan, the driver of one run, the list offsets,
 *        and the figures of the last run.
 */
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "sx_pairbin.hpp"

namespace sx::pairbin
{

int planBands(const uint64_t* rowCounts, int rows, uint64_t cap, const Names& nm, BandPlan& plan, std::string& err)
{
    cap  = std::min(cap ? cap : kDefaultPairCap, kMaxBandPairs);
    plan = BandPlan{};
    for (int r = 0; r < rows; ++r)
    {
        const uint64_t c = rowCounts[r];
        if (c > kMaxBandPairs)
        {
            err = std::string(nm.fn) + ": one " + nm.row + " holds more than 2^31 - 1 pairs " + nm.tooMany;
            return SX_ERR_ARG;
        }
        if (c > cap)
        {
            err = std::string(nm.fn) + ": one " + nm.row + " holds " + std::to_string(c) + " pairs, more than the pair cap of " +
                  std::to_string(cap) + " (" + nm.setter + ")";
            return SX_ERR_ARG;
        }
        if (plan.bands.empty() || plan.bands.back().pairs + c > cap) plan.bands.push_back(Band{r, r + 1, c});
        else plan.bands.back().r1 = r + 1, plan.bands.back().pairs += c;
        plan.total += c;
    }
    for (const Band& bd : plan.bands)
        plan.largest = std::max(plan.largest, bd.pairs);
    return SX_OK;
}

namespace
{

//! offsets[t] = first sorted pair of band-local unit t, t in [0, units]; *mismatch counts the bands in which the emit
//! pass wrote another number of pairs than the count pass announced (the buffer was filled with keys beyond every unit
//! before, so such a band loses pairs but reads no stale one; stats() reports it)
__global__ void offsetsKernel(const uint64_t* sorted, uint32_t num, uint32_t units, uint32_t* offsets,
                              const uint32_t* cursor, unsigned long long* mismatch)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t == 0 && *cursor != num) atomicAdd(mismatch, 1ull);
    if (t > units) return;
    const uint64_t key = (uint64_t)t << 32;
    uint32_t       lo = 0, hi = num;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    offsets[t] = lo;
}

} // namespace

hipError_t ensureEvents(Buffers& b)
{
    if (b.timing)
        for (auto& e : b.ev)
            if (!e)
                if (hipError_t rc = hipEventCreate(&e); rc != hipSuccess) return rc;
    return hipSuccess;
}

int drive(Arena& arena, Buffers& b, const Names& nm, int maxRows, int rows, uint32_t unitsPerRow, const Launches& l,
          hipStream_t s, std::string& err)
{
    const std::string tag      = nm.tag;
    const size_t      numCount = 3 + (size_t)maxRows;
    b.counts     = arena.get<unsigned long long>(tag + "counts", numCount);
    b.countsHost = arena.pinned<unsigned long long>(tag + "countsHost", numCount);
    if (!b.counts || !b.countsHost)
    {
        err = std::string(nm.fn) + ": counters";
        return SX_ERR_NOMEM;
    }
    b.maxRows = maxRows;
    SX_TRY_HIP(nm.hipFn, ensureEvents(b));
    b.ms[0] = b.ms[1] = b.ms[2] = 0.0f;
    float ms = 0.0f;

    // pairs per row
    if (b.timing) SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[0], s));
    SX_TRY_HIP(nm.hipFn, hipMemsetAsync(b.counts, 0, numCount * sizeof(unsigned long long), s));
    l.count(b.counts);
    SX_TRY_HIP(nm.hipFn, hipGetLastError());
    if (b.timing) SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[1], s));
    SX_TRY_HIP(nm.hipFn, hipMemcpyAsync(b.countsHost, b.counts, (2 + rows) * sizeof(unsigned long long),
                                        hipMemcpyDeviceToHost, s));
    SX_TRY_HIP(nm.hipFn, hipStreamSynchronize(s));
    if (b.timing && hipEventElapsedTime(&ms, b.ev[0], b.ev[1]) == hipSuccess) b.ms[0] += ms;

    BandPlan plan;
    if (int rc = planBands(reinterpret_cast<const uint64_t*>(b.countsHost + 2), rows, b.pairCap, nm, plan, err)) return rc;

    const size_t   largest  = plan.largest;
    const uint32_t allUnits = unitsPerRow * (uint32_t)rows;
    int            unitBits = 1;
    while ((1u << unitBits) < allUnits + 1u)
        ++unitBits;
    size_t tmpBytes = 0;
    if (largest)
        SX_TRY_HIP(nm.hipFn, hipcub::DeviceRadixSort::SortKeys(nullptr, tmpBytes, (const uint64_t*)nullptr,
                                                               (uint64_t*)nullptr, (int)largest, 0, 32 + unitBits, s));
    b.pairsIn  = arena.get<uint64_t>(tag + "pairsIn", largest);
    b.pairsOut = arena.get<uint64_t>(tag + "pairsOut", largest);
    b.sortTmp  = arena.get<char>(tag + "sortTmp", tmpBytes);
    b.offsets  = arena.get<uint32_t>(tag + "offsets", (size_t)allUnits + 1);
    b.cursor   = arena.get<uint32_t>(tag + "cursor", 1);
    if (!b.pairsIn || !b.pairsOut || !b.sortTmp || !b.offsets || !b.cursor)
    {
        err = std::string(nm.fn) + ": pair scratch (" + std::to_string(2 * largest * 8 + tmpBytes) + " bytes)";
        return SX_ERR_NOMEM;
    }
    b.scratchBytes = 2 * largest * 8 + tmpBytes + ((size_t)allUnits + 2) * 4 + numCount * 8;

    for (const Band& bd : plan.bands)
    {
        const uint32_t units = (uint32_t)(bd.r1 - bd.r0) * unitsPerRow;
        const uint32_t num   = (uint32_t)bd.pairs;
        if (b.timing) SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[0], s));
        SX_TRY_HIP(nm.hipFn, hipMemsetAsync(b.cursor, 0, 4, s));
        if (num)
        {
            // keys beyond every unit: a slot the emit pass should leave unwritten sorts behind the last list
            SX_TRY_HIP(nm.hipFn, hipMemsetAsync(b.pairsIn, 0xff, (size_t)num * sizeof(uint64_t), s));
            l.emit(bd, b.cursor, b.pairsIn);
            SX_TRY_HIP(nm.hipFn, hipGetLastError());
        }
        if (b.timing) SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[1], s));
        if (num)
            SX_TRY_HIP(nm.hipFn, hipcub::DeviceRadixSort::SortKeys(b.sortTmp, tmpBytes, (const uint64_t*)b.pairsIn,
                                                                   b.pairsOut, (int)num, 0, 32 + unitBits, s));
        offsetsKernel<<<(units + 1 + 255) / 256, 256, 0, s>>>(b.pairsOut, num, units, b.offsets, b.cursor,
                                                              b.counts + 2 + maxRows);
        SX_TRY_HIP(nm.hipFn, hipGetLastError());
        if (b.timing) SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[2], s));
        // a unit without pairs reads no particle
        l.gather(bd, b.pairsOut, b.offsets, b.counts);
        SX_TRY_HIP(nm.hipFn, hipGetLastError());
        if (b.timing)
        {
            SX_TRY_HIP(nm.hipFn, hipEventRecord(b.ev[3], s));
            SX_TRY_HIP(nm.hipFn, hipEventSynchronize(b.ev[3]));
            for (int k = 0; k < 3; ++k)
                if (hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]) == hipSuccess) b.ms[k] += ms;
        }
    }
    b.pairs = plan.total;
    b.bands = plan.bands.size();
    b.done  = true;
    return SX_OK;
}

int stats(Buffers& b, hipStream_t s, uint64_t out[4])
{
    if (!b.done) return SX_ERR_ARG;
    if (hipMemcpyAsync(b.countsHost, b.counts, (3 + b.maxRows) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SX_ERR_HIP;
    if (b.countsHost[2 + b.maxRows]) return kStatsMismatch;
    out[0] = b.pairs, out[1] = b.bands, out[2] = b.countsHost[1], out[3] = b.countsHost[0];
    return SX_OK;
}

int statsCode(int rc, const char* fn, const Names& nm, std::string& why)
{
    if (rc == SX_OK) return SX_OK;
    why = std::string(fn) + ": " + (rc == kStatsMismatch ? nm.mismatch : rc == SX_ERR_ARG ? nm.nothing : "copy failed");
    return rc == kStatsMismatch ? SX_ERR_HIP : rc;
}

void release(Buffers& b)
{
    for (auto& e : b.ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
}

} // namespace sx::pairbin
