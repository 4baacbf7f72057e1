// What the wave-per-row kernels share, stated once: a row's extent, the 16-byte decision, four adjacent words of a row, and the THINNED
// ROW - the layout that drop_edge.hip and neighbor_sample.hip write and that drop_edge.hip's aggregation and neighbor_max.hip read
// (include/wdg.h, at wdg_drop_edge_thin_batched, DEFINES it; this header only implements it).  Users: drop_edge.hip,
// neighbor_sample.hip, neighbor_max.hip, neighbor_moments.hip, gcnii.hip, gat_scores.hip and gat_lanes.h (gat.hip, signed_att.hip).
//
// No LDS, no atomics, no fused multiply-add, and no floating-point expression that could contract - only the ONE division (or 1 / sqrtf)
// of a row's scale: the header means the same in a unit compiled with contraction off and in one compiled without.
#pragma once
#include <cmath>
#include <cstdint>

#include "wdg_common.h"

namespace wdg {

// the extent of row `row` of a CSR, wave-uniform: false = it lies outside [0, nnz] (the row is left untouched)
__device__ __forceinline__ bool row_extent(const global_ptr<const int32_t> rowptr, const int row, const int nnz, int &beg, int &end) {
    beg = __builtin_amdgcn_readfirstlane(rowptr[row]);
    end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    return beg >= 0 && beg <= end && end <= nnz;
}

// rows of 32-bit words at p, `ld` words apart, start on 16-byte boundaries.  With a width that is a multiple of 4 this is the WAVE's
// (or the job's) decision for VEC below: every lane that has columns has four, and no per-lane branch sits between a load and its use.
__device__ __forceinline__ bool aligned16(const void *p, const int64_t ld) {
    return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(ld * 4)) & 15) == 0;
}

typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void load_x4(const global_ptr<const float> p, float (&x)[4]) {
    const float4 in = load_f32x4(p);
    x[0] = in.x, x[1] = in.y, x[2] = in.z, x[3] = in.w;
}
__device__ __forceinline__ void load_x4(const global_ptr<const uint32_t> p, uint32_t (&x)[4]) {
    const i32x4_t in = *(global_ptr<const i32x4_t>)p;
    x[0] = in.x, x[1] = in.y, x[2] = in.z, x[3] = in.w;
}
__device__ __forceinline__ void store_x4(const global_ptr<float> p, const float (&x)[4]) { store_f32x4(p, make_float4(x[0], x[1], x[2], x[3])); }
__device__ __forceinline__ void store_x4(const global_ptr<uint32_t> p, const uint32_t (&x)[4]) {
    *(global_ptr<i32x4_t>)p = i32x4_t{static_cast<int>(x[0]), static_cast<int>(x[1]), static_cast<int>(x[2]), static_cast<int>(x[3])};
}
// Four adjacent words (float or uint32_t) of a row, of which `live` (1 .. 4) exist.  VEC: one 16-byte access.  Without VEC the words go
// one by one: a load's address of a word the lane does not have is clamped to its last one (that value is never stored), a store
// writes the live words only.
template <bool VEC, typename T>
__device__ __forceinline__ void load4(const global_ptr<const T> p, const int live, T (&x)[4]) {
    if (VEC) {
        load_x4(p, x);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = p[min(k, live - 1)];
    }
}
template <bool VEC, typename T>
__device__ __forceinline__ void store4(const global_ptr<T> p, const int live, const T (&x)[4]) {
    if (VEC) {
        store_x4(p, x);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < live) p[k] = x[k];
    }
}

// ---- the thinned row, producer side.  A wave owns the row and walks its extent [beg, end) in chunks of 64 entries, one per lane.
// One chunk: the vote, the lane's prefix count, the kept column j stored behind the `kept` (wave-uniform) kept entries so far.
// EVERY lane of the wave is active here.
__device__ __forceinline__ void thinned_row_keep(const global_ptr<int32_t> kept_col, const int beg, int &kept, const bool keep, const int j) {
    const unsigned long long votes = __ballot(keep);
    const int before = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(votes >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(votes), 0u));
    if (keep) kept_col[beg + kept + before] = j;  // (beg + kept + before <= the entry's own position: inside the row's extent)
    kept += __popcll(votes);
}
// The row's tail: -1 up to `end`, then lane 0 writes kept_len[row] and, where the job has one, scale[row] - the F32 path of
// wdg_degree_norm on the count: 1 / sqrtf(c) where `norm_sym` is not 0, else 1 / c; inf -> 0.  J: a job with kept_len and scale.
template <typename J>
__device__ __forceinline__ void thinned_row_finish(const desc_ptr<J> job, const global_ptr<int32_t> kept_col, const int row, const int beg, const int end,
                                                   const int kept, const int lane, const int norm_sym) {
    for (int q = beg + kept + lane; q < end; q += 64) kept_col[q] = -1;
    if (lane == 0) {
        to_global(job->kept_len)[row] = kept;
        if (job->scale) {
            const float c = static_cast<float>(kept);
            float d = norm_sym ? 1.0f / sqrtf(c) : 1.0f / c;
            if (isinf(d)) d = 0.f;
            to_global(job->scale)[row] = d;
        }
    }
}
// ---- consumer side: the entries to walk behind `beg` (wave-uniform).  kept_len == NULL: a plain CSR pattern, the whole extent.
__device__ __forceinline__ int thinned_row_len(const int32_t *kept_len, const int row, const int beg, const int end) {
    int len = end - beg;
    if (kept_len) len = min(__builtin_amdgcn_readfirstlane(to_global(kept_len)[row]), len);
    return len;
}

}  // namespace wdg
