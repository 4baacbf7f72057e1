// The TOTAL ORDER of the neighbour extremes, stated once: the image of a value under it, the 64-bit word a lane keeps per column
// (image << 32 | ~j: greater = wins) carried across lanes, and one compare of a candidate against the best so far.  include/wdg.h, at
// wdg_neighbor_max_batched_f32, DEFINES the order; this header only implements it.  Users: neighbor_max.hip, neighbor_moments.hip.
//
// Integer work only: no floating-point operation, no LDS, no atomics - the header means the same in any unit.
#pragma once
#include <cstdint>

#include "wdg_common.h"

namespace wdg {

// the image of a value under the order: greater = wins.  A NaN: 0xffffffff; -0 and +0 share an image; every other image lies in
// [0x007fffff, 0xff800000], for the maximum and (complemented) for the minimum alike - never 0, the word of "no entry yet"
__device__ __forceinline__ uint32_t nm_key(uint32_t b, const bool minimum) {
    const uint32_t a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return 0xffffffffu;
    if (a == 0) b = 0;
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return minimum ? ~m : m;
}
__device__ __forceinline__ uint64_t nm_shfl_xor64(const uint64_t w, const int off) {
    const uint32_t lo = __shfl_xor(static_cast<int>(static_cast<uint32_t>(w)), off), hi = __shfl_xor(static_cast<int>(static_cast<uint32_t>(w >> 32)), off);
    return static_cast<uint64_t>(hi) << 32 | lo;
}

}  // namespace wdg
