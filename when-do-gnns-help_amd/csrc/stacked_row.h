// One (row, replica) pair of STACKED logits, once, for csrc/xent_eval.hip, csrc/xent_curve.hip and csrc/confusion.hip.
//
// The layout: the logits of R models (all splits of one graph) lie side by side in one [n, R cs] matrix with leading dimension ld;
// replica r's C classes are columns r cs .. r cs + C - 1 of a row, columns r cs + C .. (r + 1) cs - 1 are padding and are never
// read.  split [n, R] uint8 holds a pair's part (0 unused, 1 train, 2 validation, 3 test), labels [n] its true class.
// The ownership: one thread owns one pair and holds its C <= SR_MAX_C logits in registers; adjacent lanes own adjacent replicas of a
// row, so a wave reads the split codes as consecutive bytes and the logits as one contiguous piece of a row.
// The rule: a pair's prediction is its FIRST maximum; a pair with a NaN among its C logits has no prediction.
// Which rows a workgroup owns, what it counts and where it writes are each kernel's own.
#pragma once
#include "wdg_common.h"

namespace wdg {

constexpr int SR_MAX_C = 16;

// the part of every kernel's "skip this job" test that is about a thread's registers (a job that lies about its own C must still not
// be indexed out of bounds); what a kernel asks of n, R, ld and its pointers is its own
__host__ __device__ __forceinline__ bool sr_bad_classes(const int C, const int cs) { return C < 1 || C > SR_MAX_C || cs < C; }

// (uniform) whether every pair of a matrix at p with leading dimension ld (floats) and replica stride cs starts at a 16-byte boundary
__device__ __forceinline__ bool sr_rows16(const void *p, const int64_t ld, const int cs) {
    return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(ld * 4)) & 15) == 0 && (cs & 3) == 0;
}

// z[0 .. C - 1] = the pair's logits at p: 16-byte loads of whole groups of four where vec (sr_rows16) allows, else scalar loads; the
// rest of a partially filled group is 0, the groups beyond C stay untouched
__device__ __forceinline__ void sr_load(float (&z)[SR_MAX_C], const global_ptr<const float> p, const int C, const bool vec) {
#pragma unroll
    for (int g = 0; g < SR_MAX_C / 4; ++g) {
        if (4 * g >= C) continue;
        if (vec && 4 * g + 3 < C) {
            const float4 v = load_f32x4(p + 4 * g);
            z[4 * g] = v.x, z[4 * g + 1] = v.y, z[4 * g + 2] = v.z, z[4 * g + 3] = v.w;
        } else {
#pragma unroll
            for (int k = 4 * g; k < 4 * g + 4; ++k) z[k] = k < C ? p[k] : 0.f;
        }
    }
}

// the first maximum of z[0 .. C - 1] and its index, and whether any of the C values is a NaN.  m is the maximum the comparisons
// leave: a NaN survives below whatever they made of it - it makes its own exponential a NaN, and with it sr_exp_sum's result
struct sr_max {
    float m;
    int pred;
    bool nan;
};
__device__ __forceinline__ sr_max sr_first_max(const float (&z)[SR_MAX_C], const int C) {
    sr_max r{z[0], 0, z[0] != z[0]};
#pragma unroll
    for (int k = 1; k < SR_MAX_C; ++k) {
        if (k < C) {
            r.nan = r.nan || z[k] != z[k];
            if (z[k] > r.m) r.m = z[k], r.pred = k;
        }
    }
    return r;
}

// z[k] <- expf(z[k] - m) for k < C -> their sum in ascending k (tests/_xent_ref.py and tests/_curve_ref.py restate this order)
__device__ __forceinline__ float sr_exp_sum(float (&z)[SR_MAX_C], const int C, const float m) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < SR_MAX_C; ++k) {
        if (k < C) {
            z[k] = expf(z[k] - m);
            s = k == 0 ? z[0] : s + z[k];
        }
    }
    return s;
}

}  // namespace wdg
