// What the per-edge kernels of gat.hip (a softmax weight per stored entry) and signed_att.hip (a signed tanh weight) share: a wave per
// row, the lanes' column groups, the batches of row loads in flight, the wave's sums in their stated order, and the pass over the
// transposed pattern, which is the same arithmetic for both layers (include/wdg.h: d_H and d_S[j, heads + h]).  Both units are
// compiled with contraction off; every fused multiply-add here is written as fmaf.
#pragma once
#include <cmath>
#include <cstdint>

#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // every fused multiply-add of the definitions is written as fmaf; nothing else may be fused

namespace wdg_gt {

using namespace wdg;

constexpr int GT_WAVES = 4;                  // rows per workgroup
constexpr int GT_HEADS = WDG_GAT_MAX_HEADS;  // the unrolled head loops and the LDS stage's row
#ifndef WDG_GAT_DEPTH
#define WDG_GAT_DEPTH 8
#endif
constexpr int GT_DEPTH = WDG_GAT_DEPTH;      // row loads in flight before the first fmaf of a batch (a divisor of 64; DESIGN 4.25 has the A/B)

// the wave's sum in the STATED order: partner lanes 32, 16, 8, 4, 2, 1 apart, each step adding a pair both ways (every lane ends with
// the same bits)
__device__ __forceinline__ float gt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
// what one lane of a wave wrote to the wave's LDS region is read by another: LDS operations of a wave execute in order, so only the
// compiler has to keep them in place
__device__ __forceinline__ void gt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the lane's four columns c0 .. c0 + 3 of the job's heads * w, and the head of each
struct gt_lane_cols {
    int c0, live;  // live: how many of the four exist (0 .. 4)
    int hk[4];
};
__device__ __forceinline__ gt_lane_cols gt_columns(const int lane, const int heads, const int w) {
    gt_lane_cols lc;
    lc.c0 = 4 * lane;
    lc.live = max(0, min(4, heads * w - lc.c0));
#pragma unroll
    for (int k = 0; k < 4; ++k) lc.hk[k] = min((lc.c0 + k) / w, heads - 1);
    return lc;
}
// VEC of load4 (wave_rows.h) is the WAVE's decision here - gt_wave_vec: pointer and leading dimension 16-byte aligned, heads w a
// multiple of 4 -, so the loads of a batch stay in flight together.  The store takes the decision at RUN time and stays written out:
// as a dispatch to store4<true / false> the compiler inverts the callers' branch on it.
__device__ __forceinline__ void gt_store4(const global_ptr<float> p, const bool vec, const int live, const float (&x)[4]) {
    if (vec) {
        store_f32x4(p, make_float4(x[0], x[1], x[2], x[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < live) p[k] = x[k];
    }
}
__device__ __forceinline__ bool gt_wave_vec(const float *p, const int64_t ld, const int cols) { return aligned16(p, ld) && (cols & 3) == 0; }

// D consecutive entries d0 .. d0 + D - 1 of the chunk the wave holds: all D row loads, then the D x 4 fmafs in entry order -
// acc[k] = fmaf(weight of the entry for the column's head, X[source row][c0 + k], acc[k]).  src: lane d holds the source row of entry
// d, or -1 for an entry that is skipped (its load goes to row 0 and its fmaf is not applied); stage: the wave's [64][GT_HEADS]
// weights.  EVERY lane is active at the readlanes; a lane without columns only skips the loads and the fmafs.
template <int D, bool VEC>
__device__ __forceinline__ void gt_batch(const global_ptr<const float> x_base, const int64_t ld, const gt_lane_cols &lc, const bool one_head, const int src,
                                         const int d0, const float *stage, float (&acc)[4]) {
    int r[D];
#pragma unroll
    for (int d = 0; d < D; ++d) r[d] = __builtin_amdgcn_readlane(src, d0 + d);
    if (lc.live > 0) {
        float x[D][4];
#pragma unroll
        for (int d = 0; d < D; ++d) load4<VEC>(x_base + static_cast<int64_t>(max(r[d], 0)) * ld + lc.c0, lc.live, x[d]);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool ok = r[d] >= 0;  // (uniform)
            const float *a = stage + (d0 + d) * GT_HEADS;
            if (one_head) {
                const float a0 = a[lc.hk[0]];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = ok ? fmaf(a0, x[d][k], acc[k]) : acc[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = ok ? fmaf(a[lc.hk[k]], x[d][k], acc[k]) : acc[k];
            }
        }
    }
}
// the chains of the lane's four columns over the `cnt` entries of a chunk, in entry order: batches of GT_DEPTH, a shorter tail in
// batches of 8, 4, 2, 1
template <bool VEC>
__device__ __forceinline__ void gt_chains(const global_ptr<const float> x_base, const int64_t ld, const gt_lane_cols &lc, const bool one_head, const int src,
                                          const int cnt, const float *stage, float (&acc)[4]) {
    int d0 = 0;
    for (; d0 + GT_DEPTH <= cnt; d0 += GT_DEPTH) gt_batch<GT_DEPTH, VEC>(x_base, ld, lc, one_head, src, d0, stage, acc);
    if (GT_DEPTH > 8 && d0 + 8 <= cnt) gt_batch<8, VEC>(x_base, ld, lc, one_head, src, d0, stage, acc), d0 += 8;
    if (GT_DEPTH > 4 && d0 + 4 <= cnt) gt_batch<4, VEC>(x_base, ld, lc, one_head, src, d0, stage, acc), d0 += 4;
    if (GT_DEPTH > 2 && d0 + 2 <= cnt) gt_batch<2, VEC>(x_base, ld, lc, one_head, src, d0, stage, acc), d0 += 2;
    if (d0 + 1 <= cnt) gt_batch<1, VEC>(x_base, ld, lc, one_head, src, d0, stage, acc);
}

// what every kernel reads of a job first (wave-uniform): false = the job is outside the limits and is left untouched.  J: wdg_gat_job
// or wdg_signed_att_job (the fields the two share carry the same names)
struct gt_shape {
    int n, heads, w, cols, nnz;
};
template <typename J>
__device__ __forceinline__ bool gt_job_shape(const desc_ptr<J> job, const int max_rows, gt_shape &s) {
    s.n = min(job->n, max_rows), s.heads = job->heads, s.w = job->w, s.nnz = job->nnz;
    s.cols = s.heads * s.w;
    return s.heads >= 1 && s.heads <= GT_HEADS && s.w >= 1 && s.cols <= WDG_GAT_MAX_COLS && s.nnz >= 0 && job->n >= 0;
}

template <typename J>
__device__ __forceinline__ bool gt_has_backward(const desc_ptr<J> job, const int nnz) {
    return job->rowptr && job->t_rowptr && job->H && job->S && job->d_out && job->d_H && job->d_S &&
           (nnz == 0 || (job->col && job->t_col && job->t_pos && job->alpha && job->d_pre));
}

// g = d_out[i, :] into the wave's LDS row, +0 past the job's columns (the row pass of either layer reads it against a neighbour's row)
template <typename J>
__device__ __forceinline__ void gt_stage_d_out(const desc_ptr<J> job, const gt_shape &s, const int i, const int lane, float *g) {
    const gt_lane_cols lc = gt_columns(lane, s.heads, s.w);
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    const global_ptr<const float> gi = to_global(job->d_out) + static_cast<int64_t>(i) * job->ld_d_out + lc.c0;
    if (lc.live > 0) {
        if (gt_wave_vec(job->d_out, job->ld_d_out, s.cols))
            load4<true>(gi, lc.live, x);
        else
            load4<false>(gi, lc.live, x);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) g[4 * lane + k] = k < lc.live ? x[k] : 0.f;
}

// The pass over the transposed pattern, a wave's row j with the extent [beg, end) of its transposed row (the kernel has checked the job's
// shape, its backward pointers and the extent): d_H[j, :] - the forward's chains with the applied weight alpha
// gathered through t_pos and d_out in the place of H - and d_S[j, heads + h] = sum_q d_pre[t_pos[q], h].  stage: the wave's
// [64 * GT_HEADS] floats of LDS.  gat.hip keeps this pass written out in its own kernel (the comment there says why): the two are ONE
// statement of include/wdg.h and change together.
template <typename J>
__device__ __forceinline__ void gt_transposed_row(const desc_ptr<J> job, const gt_shape &s, const int j, const int beg, const int end, const int lane,
                                                  float *stage) {
    const int heads = s.heads, n = job->n;
    const global_ptr<const int32_t> t_col = to_global(job->t_col), t_pos = to_global(job->t_pos);
    const global_ptr<const float> alpha = to_global(const_cast<const float *>(job->alpha)), d_pre = to_global(const_cast<const float *>(job->d_pre));
    const gt_lane_cols lc = gt_columns(lane, heads, s.w);
    const bool one_head = (s.w & 3) == 0, vec_g = gt_wave_vec(job->d_out, job->ld_d_out, s.cols);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, ds[GT_HEADS];
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h) ds[h] = 0.f;
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);  // (wave-uniform)
        const bool mine = lane < cnt;
        int src = mine ? t_col[e0 + lane] : -1;
        const int p = mine ? t_pos[e0 + lane] : -1;
        if (static_cast<unsigned>(src) >= static_cast<unsigned>(n) || static_cast<unsigned>(p) >= static_cast<unsigned>(s.nnz)) src = -1;
        const bool valid = src >= 0;
        const int64_t at = static_cast<int64_t>(valid ? p : 0) * heads;  // (a lane without an entry reads entry 0: no branch between a load and its use)
        float av[GT_HEADS], dv[GT_HEADS];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) {
            av[h] = alpha[at + min(h, heads - 1)];
            dv[h] = d_pre[at + min(h, heads - 1)];
        }
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h)
            if (h < heads) {
                ds[h] = valid ? ds[h] + dv[h] : ds[h];  // (a lane's entries in ascending order)
                stage[lane * GT_HEADS + h] = valid ? av[h] : 0.f;
            }
        gt_wave_sync();
        if (vec_g)
            gt_chains<true>(to_global(job->d_out), job->ld_d_out, lc, one_head, src, cnt, stage, acc);
        else
            gt_chains<false>(to_global(job->d_out), job->ld_d_out, lc, one_head, src, cnt, stage, acc);
        gt_wave_sync();
    }
    if (lc.live > 0)
        gt_store4(to_global(job->d_H) + static_cast<int64_t>(j) * job->ld_d_h + lc.c0, gt_wave_vec(job->d_H, job->ld_d_h, s.cols), lc.live, acc);
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) {
            const float total = gt_wave_sum(ds[h]);
            if (lane == 0) to_global(job->d_S)[static_cast<int64_t>(j) * job->ld_d_s + heads + h] = total;
        }
}

// the table-level refusals of the launch entries and of the host predicates (what = the entry's name in the message)
inline int gt_check_table(const char *what, const void *jobs, int32_t n_jobs, int32_t max_rows) {
    WDG_REQUIRE(max_rows >= 0, "%s: negative count", what);
    return check_job_table(what, jobs, n_jobs);
}

}  // namespace wdg_gt
