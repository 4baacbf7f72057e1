// The 32 x 32 block routines that the two kernel-regression solvers share (csrc/kernel_reg.hip: the register-resident solver of up
// to 320 train rows; csrc/kernel_reg_large.hip: the solver of up to 1024 rows whose factor lives in device memory): the column
// deal of the MFMA accumulator layout, a block's registers <-> its row-major image, and the one-wave routine that factors and
// inverts a diagonal block.
#pragma once
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int K2_PS = 36;  // row stride (floats) of a block's image in LDS: conflict-free for the four ds_read_b128 of a lane

__device__ __forceinline__ int k2_jmap(int h, int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ float k2_bcast(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// a block's registers <-> its row-major image in LDS (lane (i, h): row i, columns 4 h + 8 q .. + 3)
__device__ __forceinline__ void k2_store_block(const f32x16 &t, float *img, int li, int h) {
    float *row = img + li * K2_PS + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(row + 8 * q) = make_float4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
}
__device__ __forceinline__ void k2_load_block(f32x16 &t, const float *img, int li, int h) {
    const float *row = img + li * K2_PS + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(row + 8 * q);
        t[4 * q] = v.x, t[4 * q + 1] = v.y, t[4 * q + 2] = v.z, t[4 * q + 3] = v.w;
    }
}

// The diagonal block: factored AND inverted by one wave, right-looking, in one instruction stream.  Lane i of the LOWER half
// holds row i of the 32 x 32 block A, lane i of the UPPER half row i of the identity - 32 registers each.  Step j:
//     pivot = a[j][j] (v_readlane from lane j), inv = 1 / sqrt(pivot), res = x[j] inv, x[c] -= res l[c][j] for c > j,
// which for the lower half is column j of the Cholesky factor (res = l[i][j]) and the right-looking update of the trailing
// rows, and for the upper half - the SAME instructions - the substitution X L^T = I by columns (res = X[i][j], the entries c > j
// of the right-hand side reduced by it): the upper half ends with row i of L^-T, i.e. column i of M = L_kk^-1, and writes it
// row-major over the image of the block in `ld`.  Column j of L reaches all lanes through LDS (`lt[j][.]`, written by the lower
// half, read back as broadcast float4s); the ONE product the next pivot waits for - entry j + 1 - takes l[j + 1][j] from lane
// j + 1's register (v_readlane), so the step's dependent chain is pivot -> rsq -> scale -> readlane -> fma, no LDS access in it.
// History: a left-looking recurrence (a 16-term dot product per lane half in front of every pivot, ~100
// instructions and ~480 cycles per step) for the factor, the same code run by a second wave two rows behind for the inverse
// (polling a step counter in LDS); then both right-looking on two waves (~460 cycles per step: the chain still carried the
// half-select / permlane swap of the split-row layout and the follower's polls).
__device__ __forceinline__ bool k2_factor_invert(float *ld, float *lt, int li, int h, int rows_real, float drop_below, float ridge) {
    float x[32];
    const bool hi = h != 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 v = *reinterpret_cast<const float4 *>(ld + li * K2_PS + 4 * q);
        x[4 * q] = hi ? (4 * q == li ? 1.f : 0.f) : v.x, x[4 * q + 1] = hi ? (4 * q + 1 == li ? 1.f : 0.f) : v.y;
        x[4 * q + 2] = hi ? (4 * q + 2 == li ? 1.f : 0.f) : v.z, x[4 * q + 3] = hi ? (4 * q + 3 == li ? 1.f : 0.f) : v.w;
    }
    // Software-pipelined by one step: the column read back from LDS in step j - 1 is applied (to the entries c > j) in step j,
    // in the shadow of step j's own chain; the entry that chain needs, x[j], got column j - 1 through the v_readlane shortcut.
    bool low_any = false;
    float4 cp[8];  // column j - 1 of L, as read back (cp[q] = l[4 q .. 4 q + 3][j - 1])
    float res_p = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) cp[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        // column j - 1 on the entries c > j, dealt into six slots that are placed BETWEEN the later links of the step's dependent chain
        // (the column was requested from LDS at the end of the step before: the first links run while it arrives)
        // (a scheduling barrier after every link pins the order: left to itself the scheduler issues the chain first and the
        // products after it - a wave issues in order, so the chain's latencies then stay empty)
        auto bulk = [&](int slot) {
            if (j == 0) return;
#pragma unroll
            for (int c = j + 1; c < 32; ++c) {
                if ((c - j - 1) % 6 != slot) continue;  // (compile-time)
                const float4 &cq = cp[c >> 2];
                x[c] = fmaf(-res_p, (c & 3) == 0 ? cq.x : (c & 3) == 1 ? cq.y : (c & 3) == 2 ? cq.z : cq.w, x[c]);
                // (pinned: left alone, the compiler sinks these products down to the step that reads the entry - a left-looking
                // factorisation again, with every earlier column held in registers: 430 spilled registers)
                asm volatile("" : "+v"(x[c]));
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        float piv = k2_bcast(x[j], j);
        const bool low = !(piv > drop_below) && j < rows_real;  // (uniform; also catches NaN)
        low_any |= low;
        piv = low ? fmaxf(ridge, drop_below) : piv;
        const float xj = (!hi && li == j) ? piv : x[j];  // (the diagonal entry follows a replaced pivot)
        float inv = __builtin_amdgcn_rsqf(piv);
        float nt_ = -0.5f * piv * inv;
        __builtin_amdgcn_sched_barrier(0);
        bulk(0);
        nt_ = fmaf(nt_, inv, 1.5f);  // one Newton step: 1 / sqrt(piv) to within an ulp
        bulk(1);
        inv = inv * nt_;
        bulk(2);
        const float res = xj * inv;
        x[j] = res;
        bulk(3);
        if (j + 1 == 32) break;
        if (!hi) lt[j * K2_PS + li] = res;  // column j of L (rows < j: never read)
        const float ln = k2_bcast(res, j + 1);
        bulk(4);
        x[j + 1] = fmaf(-res, ln, x[j + 1]);  // the entry the next pivot waits for
        bulk(5);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (4 * q + 3 > j + 1) cp[q] = *reinterpret_cast<const float4 *>(lt + j * K2_PS + 4 * q);  // (for the next step)
        res_p = res;
        __builtin_amdgcn_sched_barrier(0);
    }
    if (hi) {  // x = row li of L_kk^-T = column li of M
#pragma unroll
        for (int c = 0; c < 32; ++c) ld[c * K2_PS + li] = x[c];
    }
    return low_any;
}

}  // namespace
