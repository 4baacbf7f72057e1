// The per-row arithmetic of the ACM channel mix (include/wdg.h states it; tests/_acm_ref.py restates it in numpy), once, for
// csrc/acm_mix.hip and csrc/acm_mix_packed.hip: a replica of the packed kernel has the bits of a one-job launch of acm_mix.hip
//  because both call the functions below.  Everything here starts AFTER the row sums: which lanes own a row, the
// loads, the stores and the reductions are each kernel's own.  Device code only.
#pragma once
#include <cstdint>

#pragma clang fp contract(off)  // every multiply-add below is written out (fmaf or two operations): the same bits in every caller

namespace wdg::acm {

// what the two kernels share by contract: a workgroup of THREADS owns TILE rows, thread (row slot t >> 4, lane t & 15) works on rows
// slot, slot + SLOTS, ... (ROWS_PER_THREAD of them); a job per gridDim.z; a row of aux is AUX_WORDS floats:
// alpha_L alpha_H alpha_I s_L s_H s_I 0 0
constexpr int TILE = 64, THREADS = 256, SLOTS = 16, ROWS_PER_THREAD = 4;
constexpr int MAX_JOBS = 65535;
constexpr int AUX_WORDS = 8, AUX_ALPHA = 0, AUX_S = 3;
constexpr float INV_T = 1.0f / 3.0f;

// whether every row of a matrix at p with leading dimension ld (floats) starts at a 16-byte boundary
__host__ __device__ inline bool rows_aligned16(const void *p, const int64_t ld) {
    return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(ld * 4)) & 15) == 0;
}

__device__ __forceinline__ float relu(const float p) { return p <= 0.f ? 0.f : p; }  // (a NaN fails the comparison and stays)

// dot[c] = the row sum of H_c . att_c  ->  s = sigmoid(dot), al = softmax((s / 3) wmix)
__device__ __forceinline__ void alpha(const float (&dot)[3], const float (&wm)[9], float (&s)[3], float (&al)[3]) {
    float z[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = 1.0f / (1.0f + expf(-dot[c]));
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = fmaf(s[2] * INV_T, wm[6 + c], fmaf(s[1] * INV_T, wm[3 + c], (s[0] * INV_T) * wm[c]));
    const float zmax = fmaxf(fmaxf(z[0], z[1]), z[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) al[c] = expf(z[c] - zmax);
    const float den = (al[0] + al[1]) + al[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) al[c] = al[c] / den;
}

// one element of out = 3 sum_c alpha_c H_c
__device__ __forceinline__ float mix(const float (&al)[3], const float l, const float h, const float i) {
    return 3.0f * fmaf(al[2], i, fmaf(al[1], h, al[0] * l));
}

// dal[c] = 3 x the row sum of d_out . H_c  ->  du[c] = the gradient of the row's score dot[c]; dw += the row's term of d_wmix
__device__ __forceinline__ void scores_backward(const float (&al)[3], const float (&s)[3], const float (&dal)[3], const float (&wm)[9],
                                                float (&du)[3], float (&dw)[9]) {
    float dz[3];
    const float mean = fmaf(al[2], dal[2], fmaf(al[1], dal[1], al[0] * dal[0]));
#pragma unroll
    for (int c = 0; c < 3; ++c) dz[c] = al[c] * (dal[c] - mean);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float ds = INV_T * fmaf(wm[3 * j + 2], dz[2], fmaf(wm[3 * j + 1], dz[1], wm[3 * j] * dz[0]));
        du[j] = (ds * s[j]) * (1.0f - s[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) dw[3 * j + c] = fmaf(s[j] * INV_T, dz[c], dw[3 * j + c]);
    }
}

// one element of a channel: da += its term of d_att; -> the gradient of the channel's input (a3 = 3 alpha_c, g = d_out, h = the
// activated unit, act = the job's ReLU flag)
__device__ __forceinline__ float input_gradient(const float a3, const float g, const float du, const float att, const float h, const bool act,
                                                float &da) {
    da = fmaf(du, h, da);
    float dp = fmaf(a3, g, du * att);
    if (act && !(h > 0.f) && h == h) dp = 0.f;  // (a NaN unit keeps its NaN gradient)
    return dp;
}

}  // namespace wdg::acm
