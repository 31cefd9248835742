/*! @file sx_pack12.hpp
 * @brief "packed12" cluster neighbor lists: 12-bit union positions, eight per three 32-bit words.
 *
 * A target's cnt stored entries stay in ascending union position.  Entries 8g .. 8g+7 form group g; entry e of the
 * group sits at bits [12e, 12e+12) of the group's 96-bit little-endian value (three consecutive words).  Unused tail
 * entries of the last group repeat the last valid position (a valid slot that is never computed).  The three words of
 * a lane's group are contiguous: word t of group g of lane l is at (g * kWave + l) * 3 + t inside the 64-target
 * group's row, so a group is one 12-byte load per lane and 768 contiguous bytes per wave.
 *
 * Positions must be below 4096: a cluster's lists are packed12 when its union count is at most a threshold
 * (kPack12Max by default), else they keep the u16 format (two per word, nlocWords).
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sx
{
namespace p12
{

constexpr uint32_t kBits      = 12;
constexpr uint32_t kGroup     = 8;    //!< entries per group
constexpr uint32_t kWords     = 3;    //!< words per group
constexpr uint32_t kPack12Max = 4095; //!< largest union count whose positions fit

//! groups of a list of cnt entries
__host__ __device__ constexpr uint32_t groups(uint32_t cnt) { return (cnt + kGroup - 1) / kGroup; }
//! words per lane of a row that holds up to ngmax entries per target
__host__ __device__ constexpr uint32_t rowWords(uint32_t ngmax) { return kWords * groups(ngmax); }

//! entry E (0 .. 7) of the group w0, w1, w2
template<int E>
__host__ __device__ inline uint32_t get(uint32_t w0, uint32_t w1, uint32_t w2)
{
    static_assert(E >= 0 && E < 8);
    if constexpr (E == 0) return w0 & 0xfffu;
    else if constexpr (E == 1) return (w0 >> 12) & 0xfffu;
    else if constexpr (E == 2) return ((w0 >> 24) | (w1 << 8)) & 0xfffu;
    else if constexpr (E == 3) return (w1 >> 4) & 0xfffu;
    else if constexpr (E == 4) return (w1 >> 16) & 0xfffu;
    else if constexpr (E == 5) return ((w1 >> 28) | (w2 << 4)) & 0xfffu;
    else if constexpr (E == 6) return (w2 >> 8) & 0xfffu;
    else return w2 >> 20;
}

//! entry e (0 .. 7, a runtime value) of the group w[0 .. 2]
__host__ __device__ inline uint32_t get(const uint32_t* w, uint32_t e)
{
    const uint32_t b = kBits * e, t = b >> 5, s = b & 31u;
    const uint64_t v = (uint64_t)w[t] | ((uint64_t)w[t < 2 ? t + 1 : 2] << 32);
    return (uint32_t)(v >> s) & 0xfffu;
}

//! packs the entries p[0 .. n), 1 <= n <= 8, of one group into w[0 .. 2]; the tail repeats p[n - 1]
__host__ __device__ inline void packGroup(const uint32_t* p, uint32_t n, uint32_t* w)
{
    uint32_t q[kGroup];
    for (uint32_t e = 0; e < kGroup; ++e)
        q[e] = p[e < n ? e : n - 1] & 0xfffu;
    w[0] = q[0] | (q[1] << 12) | (q[2] << 24);
    w[1] = (q[2] >> 8) | (q[3] << 4) | (q[4] << 16) | (q[5] << 28);
    w[2] = (q[5] >> 4) | (q[6] << 8) | (q[7] << 20);
}

} // namespace p12
} // namespace sx
