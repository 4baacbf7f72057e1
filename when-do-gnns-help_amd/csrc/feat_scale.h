// The row scaling of a compact feature matrix, stated once: features.hip applies it while it expands a row, sparse_dense.hip
// (wdg_feat_scaled_values_f32) applies it to the stored values themselves.  Both include this file, so an entry's scaled value
// has the same bits on either route.
#pragma once
#include "wdg_common.h"

namespace wdg {

// the row's scale from its fp64 sum, exactly as row_l1_kernel: sum -> y = r * x, r = 1 / s (inf -> 0); abs -> y = x / max(s, 1e-12)
struct RowScale {
    int mode;
    float f;
    __device__ __forceinline__ RowScale(int mode_, double sum) : mode(mode_), f(1.f) {
        const float s = static_cast<float>(sum);
        if (mode == WDG_FEAT_NORM_SUM) {
            f = 1.0f / s;
            if (isinf(f)) f = 0.f;
        } else if (mode == WDG_FEAT_NORM_ABS) {
            f = fmaxf(s, 1e-12f);
        }
    }
    __device__ __forceinline__ float operator()(float x) const {
        return mode == WDG_FEAT_NORM_SUM ? f * x : mode == WDG_FEAT_NORM_ABS ? x / f : x;
    }
};

// the fp64 sum of a CSR row's entries [beg, end) as ONE WAVE forms it (every lane calls this with its own lane index): a lane at a
// time over the entries lane, lane + 64, ..., then across the wave; an entry whose column lies outside [0, F) is left out
__device__ __forceinline__ double feat_csr_row_sum(global_ptr<const int32_t> col, global_ptr<const float> val, const int beg, const int end,
                                                   const int F, const int mode, const int lane) {
    double sum = 0.0;
    if (mode != WDG_FEAT_NORM_NONE) {
        for (int e = beg + lane; e < end; e += 64) {
            if (static_cast<unsigned>(col[e]) >= static_cast<unsigned>(F)) continue;
            const float x = val ? val[e] : 1.f;
            sum += static_cast<double>(mode == WDG_FEAT_NORM_ABS ? fabsf(x) : x);
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    }
    return sum;
}

}  // namespace wdg
