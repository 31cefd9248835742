/*! @file sx_pairbin.hpp
 * @brief The banded pair-binning engine under the maps (sx_map.hip) and the mesh deposit (sx_spectrum.hip): 64-bit
 *        pairs unit << 32 | particle, produced in bands of whole rows of units that stay under a cap, radix-sorted, with
 *        the offsets of every unit's list.  A client brings a geometry (which units a particle touches) and a gather
 *        launch (what a unit does with its list); everything between the two is here, once.
 *
 * A geometry G is passed to the kernels by value and provides
 *     static constexpr int kMaxRows                    the size of the count pass's LDS row array
 *     int rows() const, uint32_t unitsPerRow() const   the rows in use; a band is a range of them
 *     struct Foot (empty as constructed)               a particle's footprint
 *     __device__ void foot(uint32_t i, Foot&)          ... of particle i, computed once
 *     __device__ bool counted(const Foot&)             whether the particle adds to counts[0], the client's own tally
 *     __device__ void forRows(const Foot&, f)          f(row, units touched in that row): THE enumeration
 *     __device__ void forUnits(const Foot&, row, f)    f(unit in [0, unitsPerRow())), as many calls as forRows announced
 * The count pass sums forRows per row; the emit pass sums the same forRows over the band's rows for its position and
 * walks forUnits to fill it.  The pass that sizes the buffer and the pass that fills it share one enumeration.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/sphexa_hip.h"
#include "sx_tree.hpp"

namespace sx::pairbin
{

constexpr uint64_t kDefaultPairCap = 1ull << 27;  //!< pairs per band (24 B each with the sort's storage)
constexpr uint64_t kMaxBandPairs   = 0x7fffffffu; //!< the sort counts its items in an int

//! the words of a client's messages and its arena tags
struct Names
{
    const char* fn;       //!< "sx_map_render": in front of every refusal
    const char* hipFn;    //!< in front of a failed HIP call
    const char* row;      //!< "tile row"
    const char* tooMany;  //!< the advice after the 2^31 - 1 refusal
    const char* setter;   //!< "sx_set_map_pair_cap"
    const char* tag;      //!< arena tag prefix, "map."
    const char* nothing;  //!< stats before the first run: "nothing has been rendered"
    const char* mismatch; //!< stats after a count / emit disagreement
};

//! rows [r0, r1) and their pairs
struct Band
{
    int      r0, r1;
    uint64_t pairs;
};

struct BandPlan
{
    std::vector<Band> bands;
    uint64_t          total{0}, largest{0};
};

/*! whole rows packed greedily into bands of at most min(cap ? cap : kDefaultPairCap, kMaxBandPairs) pairs.  SX_ERR_ARG
 *  and the reason for a row above 2^31 - 1 pairs or above the cap.  Plain host code: sx_pair_bands_internal tests it. */
int planBands(const uint64_t* rowCounts, int rows, uint64_t cap, const Names& nm, BandPlan& plan, std::string& err);

/*! the typed owner of the pair scratch and of the last run's figures.  Every tag of a client's prefix that the engine
 *  needs is requested at one site, in run(), which stores the pointer here. */
struct Buffers
{
    uint64_t            pairCap{0};      // 0 = kDefaultPairCap
    unsigned long long* counts{nullptr}; // device: [client's tally, longest list, pairs per row x maxRows, mismatches]
    unsigned long long* countsHost{nullptr};
    uint64_t *          pairsIn{nullptr}, *pairsOut{nullptr};
    uint32_t *          offsets{nullptr}, *cursor{nullptr};
    void*               sortTmp{nullptr};
    // the last run
    bool       done{false};
    int        maxRows{0};
    uint64_t   pairs{0}, bands{0}, scratchBytes{0};
    bool       timing{false}; // HIP events around the stages (synchronises after every band)
    float      ms[3]{};       // binning (count + emit), sort (+ list offsets), gather
    hipEvent_t ev[4]{};
};

//! the three launches of a run; count and emit come from run<G>, gather from the client
struct Launches
{
    std::function<void(unsigned long long* counts)>                     count;
    std::function<void(const Band&, uint32_t* cursor, uint64_t* pairs)> emit;
    std::function<void(const Band&, const uint64_t* sorted, const uint32_t* offsets, unsigned long long* counts)> gather;
};

/*! counters, count pass, one synchronisation, band plan, scratch, then per band: emit, sort, list offsets, gather.
 *  Returns an SX_* code; err receives the reason. */
int drive(Arena& arena, Buffers& b, const Names& nm, int maxRows, int rows, uint32_t unitsPerRow, const Launches& l,
          hipStream_t s, std::string& err);

//! the events of a timed run, created on first use
hipError_t ensureEvents(Buffers& b);

//! stats(): in some band of the last run the emit pass wrote another number of pairs than the count pass had found
constexpr int kStatsMismatch = -1;
//! {pairs, bands, longest list, the client's tally} of the last run; synchronises
int stats(Buffers& b, hipStream_t s, uint64_t out[4]);
//! stats()'s result as an SX_* code, with the text for sx_last_error where it is not SX_OK (fn: the caller's name)
int  statsCode(int rc, const char* fn, const Names& nm, std::string& why);
void release(Buffers& b);

/*! the calling lane's first position among its wave's n's: an exclusive scan over the wave, and one atomic on the cursor
 *  for the wave's total.  Every lane of the wave calls it; meaningless (0) where the whole wave has n = 0. */
__device__ inline uint32_t waveTake(uint32_t n, uint32_t* cursor)
{
    const int lane = threadIdx.x & 63;
    uint32_t  incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    if (total == 0) return 0; // wave-uniform
    uint32_t base = 0;
    if (lane == 63) base = atomicAdd(cursor, total);
    base = __shfl(base, 63, 64);
    return base + incl - n;
}

/*! counts[0] += particles the geometry counts, counts[2 + r] += pairs of row r.  Integer atomics: the same totals on
 *  every run. */
template<class G>
__global__ __launch_bounds__(256) void countKernel(G g, uint32_t first, uint32_t last, unsigned long long* counts)
{
    __shared__ uint32_t rows[G::kMaxRows];
    __shared__ uint32_t tally;
    for (int k = threadIdx.x; k < g.rows(); k += 256)
        rows[k] = 0;
    if (threadIdx.x == 0) tally = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < last)
    {
        typename G::Foot ft;
        g.foot((uint32_t)i, ft);
        if (g.counted(ft)) atomicAdd(&tally, 1u);
        g.forRows(ft, [&](int r, uint32_t n) { atomicAdd(&rows[r], n); });
    }
    __syncthreads();
    for (int k = threadIdx.x; k < g.rows(); k += 256)
        if (rows[k]) atomicAdd(&counts[2 + k], (unsigned long long)rows[k]);
    if (threadIdx.x == 0 && tally) atomicAdd(&counts[0], (unsigned long long)tally);
}

/*! the pairs of rows [r0, r1): (band-local unit) << 32 | particle, at positions taken from a cursor.  The positions
 *  differ from run to run, the set of keys does not, and the keys are distinct. */
template<class G>
__global__ __launch_bounds__(256) void emitKernel(G g, uint32_t first, uint32_t last, int r0, int r1, uint32_t* cursor,
                                                  uint64_t* pairs, uint32_t capacity)
{
    const uint64_t   i = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    typename G::Foot ft;
    uint32_t         n = 0;
    if (i < last)
    {
        g.foot((uint32_t)i, ft);
        g.forRows(ft, [&](int r, uint32_t k) { n += (r >= r0 && r < r1) ? k : 0u; });
    }
    uint32_t pos = waveTake(n, cursor);
    if (n == 0) return;
    g.forRows(ft, [&](int r, uint32_t) {
        if (r < r0 || r >= r1) return;
        g.forUnits(ft, r, [&](uint32_t u) {
            // the count pass sized the buffer from the same enumeration; the guard keeps a disagreement in bounds
            if (pos < capacity) pairs[pos] = ((uint64_t)((uint32_t)(r - r0) * g.unitsPerRow() + u) << 32) | (uint64_t)i;
            ++pos;
        });
    });
}

/*! one run of the engine for geometry g over the particles [first, last); gather(band, sorted pairs, offsets, counts)
 *  launches the client's kernel with one workgroup per unit of the band. */
template<class G, class Gather>
int run(Arena& arena, Buffers& b, const Names& nm, const G& g, uint32_t first, uint32_t last, Gather&& gather,
        hipStream_t s, std::string& err)
{
    const unsigned blocks = (last - first + 255) / 256;
    Launches       l;
    l.count = [&](unsigned long long* counts) {
        if (blocks) countKernel<G><<<blocks, 256, 0, s>>>(g, first, last, counts);
    };
    l.emit = [&](const Band& bd, uint32_t* cursor, uint64_t* pairs) {
        emitKernel<G><<<blocks, 256, 0, s>>>(g, first, last, bd.r0, bd.r1, cursor, pairs, (uint32_t)bd.pairs);
    };
    l.gather = gather;
    return drive(arena, b, nm, G::kMaxRows, g.rows(), g.unitsPerRow(), l, s, err);
}

} // namespace sx::pairbin
