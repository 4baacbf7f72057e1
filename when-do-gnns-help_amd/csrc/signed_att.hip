// Signed attention for many graphs in one launch (the FAGCN layer of Bo et al., "Beyond Low-frequency Information in Graph Convolutional
// Networks"): per stored entry a weight tanh(score) * row_scale[i] * col_scale[j] that may be NEGATIVE - an edge can subtract a
// neighbour -, the weighted sum of the neighbours' rows, an optional residual eps * res, and the backward pass.  include/wdg.h states
// the arithmetic and every sum's order; tests/_signed_att_ref.py restates both passes in numpy fp64.
//
// replaces: the FIXED weights of the aggregation - normalize_tensor, utils/util_funcs.py:365-381 - by a signed weight learnt per edge,
//           beside the GCN / SGC tables of gnns_on_syn.py:1-154; the reference ships no model code, so the layer is defined by this
//           project.
//
// Shape: gat.hip's - a WAVE per row, four rows per workgroup, a job per grid z - on the lane helpers of gat_lanes.h.
//   forward   ONE walk over the row in chunks of 64 (there is no maximum and no Z to wait for): a lane forms a_p for its entry, stores
//             it to alpha[] and to the wave's LDS stage; then the lanes switch to the heads * w columns and run gt_chains over the chunk.
//   backward  rows: a lane per entry reads its neighbour's row against d_out[i, :] (in LDS) - dalpha is one fmaf chain over k per head,
//             kept in registers -, recomputes t by the forward's expression and writes d_pre; d_S[i, h] in gat.hip's lane order.
//             transposed rows: gt_transposed_row, the arithmetic of gat.hip's second pass.
// Nothing is added across rows: no atomic.  As in gat.hip every step issues ALL its loads first - through addresses clamped into range,
// not predicated - and only then computes and stores (the job's pointers come out of a table and may alias for all the compiler knows);
// the 16-byte path is the WAVE's decision.
// Guards: an entry whose column (or whose t_pos) lies outside the job is skipped - never read through; its alpha and d_pre are +0 -, a
// row whose extent lies outside [0, nnz] and a job outside the limits are left untouched.
#include "gat_lanes.h"

namespace {

using namespace wdg_gt;

static_assert(WDG_SIGNED_ATT_MAX_HEADS == WDG_GAT_MAX_HEADS && WDG_SIGNED_ATT_MAX_COLS == WDG_GAT_MAX_COLS, "gat_lanes.h is sized by the attention layer's limits");

// t_p of the definition, the ONE expression both passes evaluate (the backward pass recomputes the forward's bits)
__device__ __forceinline__ float sa_tanh_pre(const float si, const float sj) { return tanhf(si + sj); }

__global__ __launch_bounds__(64 * GT_WAVES) void signed_att_forward_kernel(const wdg_signed_att_job *__restrict__ jobs, const int max_rows) {
    __shared__ float stage_all[GT_WAVES][64 * GT_HEADS];
    const desc_ptr<wdg_signed_att_job> job = (desc_ptr<wdg_signed_att_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int i = blockIdx.x * GT_WAVES + wave;
    if (i >= s.n || !job->rowptr || !job->H || !job->S || !job->out || (s.nnz > 0 && (!job->col || !job->alpha))) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->rowptr), i, s.nnz, beg, end)) return;
    const int heads = s.heads, n = job->n;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<const float> S = to_global(job->S), H = to_global(job->H), col_scale = to_global(job->col_scale);
    const global_ptr<float> alpha = to_global(job->alpha);
    const int64_t ld_s = job->ld_s;
    const bool has_cs = job->col_scale != nullptr;  // (wave-uniform)
    float *stage = stage_all[wave];

    float si[GT_HEADS];
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h) si[h] = S[static_cast<int64_t>(i) * ld_s + min(h, heads - 1)];  // (a head the job does not have reads its last one: no branch)
    const float rs = job->row_scale ? to_global(job->row_scale)[i] : 1.f;  // (a factor that is not given is 1: the product with it is exact)
    const gt_lane_cols lc = gt_columns(lane, heads, s.w);
    const bool one_head = (s.w & 3) == 0, vec_h = gt_wave_vec(job->H, job->ld_h, s.cols);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);  // (wave-uniform)
        const bool mine = lane < cnt;
        int j = mine ? col[e0 + lane] : -1;
        if (static_cast<unsigned>(j) >= static_cast<unsigned>(n)) j = -1;
        const bool ok = j >= 0;
        const int jj = ok ? j : 0;  // (a lane without an entry reads row 0: no branch between a load and its use)
        const global_ptr<const float> sj = S + static_cast<int64_t>(jj) * ld_s + heads;
        float sv[GT_HEADS];  // every load before the first store: the compiler cannot know that alpha[] aliases none of them
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) sv[h] = sj[min(h, heads - 1)];
        const float cs = has_cs ? col_scale[jj] : 1.f;
        const float coef = rs * cs;
        const int64_t at = static_cast<int64_t>(e0 + lane) * heads;
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h)
            if (h < heads) {
                const float a = ok ? sa_tanh_pre(si[h], sv[h]) * coef : 0.f;
                if (mine) alpha[at + h] = a;
                stage[lane * GT_HEADS + h] = a;
            }
        gt_wave_sync();
        if (vec_h)
            gt_chains<true>(H, job->ld_h, lc, one_head, j, cnt, stage, acc);
        else
            gt_chains<false>(H, job->ld_h, lc, one_head, j, cnt, stage, acc);
        gt_wave_sync();  // (the next chunk overwrites the stage)
    }
    if (lc.live > 0) {
        if (job->res) {  // out = fmaf(eps, res, chain): the residual's row is loaded whole before the store
            const float eps = job->eps;
            const global_ptr<const float> ri = to_global(job->res) + static_cast<int64_t>(i) * job->ld_res + lc.c0;
            float r[4];
            if (gt_wave_vec(job->res, job->ld_res, s.cols))
                load4<true>(ri, lc.live, r);
            else
                load4<false>(ri, lc.live, r);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(eps, r[k], acc[k]);
        }
        gt_store4(to_global(job->out) + static_cast<int64_t>(i) * job->ld_out + lc.c0, gt_wave_vec(job->out, job->ld_out, s.cols), lc.live, acc);
    }
}

// the row pass: d_pre[p, h] and d_S[i, h]
__global__ __launch_bounds__(64 * GT_WAVES) void signed_att_backward_rows_kernel(const wdg_signed_att_job *__restrict__ jobs, const int max_rows) {
    __shared__ __attribute__((aligned(16))) float g_all[GT_WAVES][WDG_GAT_MAX_COLS];
    const desc_ptr<wdg_signed_att_job> job = (desc_ptr<wdg_signed_att_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int i = blockIdx.x * GT_WAVES + wave;
    if (i >= s.n || !gt_has_backward(job, s.nnz)) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->rowptr), i, s.nnz, beg, end)) return;
    const int heads = s.heads, w = s.w, cols = s.cols, n = job->n;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<const float> S = to_global(job->S), H = to_global(job->H), col_scale = to_global(job->col_scale);
    const global_ptr<float> d_pre = to_global(job->d_pre);
    const int64_t ld_s = job->ld_s, ld_h = job->ld_h;
    const bool has_cs = job->col_scale != nullptr;  // (wave-uniform)
    float *g = g_all[wave];
    gt_stage_d_out(job, s, i, lane, g);  // g = d_out[i, :] into LDS, +0 past the job's columns
    gt_wave_sync();
    float si[GT_HEADS], ds[GT_HEADS];
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h) {
        si[h] = S[static_cast<int64_t>(i) * ld_s + min(h, heads - 1)];  // (a head the job does not have reads its last one: no branch)
        ds[h] = 0.f;
    }
    const float rs = job->row_scale ? to_global(job->row_scale)[i] : 1.f;
    const bool vec_h = gt_wave_vec(job->H, ld_h, cols);
    // a lane per entry: dalpha[p, h] = one fmaf chain over k ascending from +0 against the neighbour's row, then d_pre and the lane's part
    // of d_S[i, h] (its entries lane, lane + 64, ... in ascending order)
    for (int e = beg + lane; e < end; e += 64) {
        const int j = col[e];
        const bool ok = static_cast<unsigned>(j) < static_cast<unsigned>(n);
        const int jj = ok ? j : 0;
        const global_ptr<const float> row = H + static_cast<int64_t>(jj) * ld_h, sj = S + static_cast<int64_t>(jj) * ld_s + heads;
        float sv[GT_HEADS], da[GT_HEADS];  // the entry's scores and scale: loaded before its first store
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) sv[h] = sj[min(h, heads - 1)], da[h] = 0.f;
        const float coef = rs * (has_cs ? col_scale[jj] : 1.f);
        float acc = 0.f;
        int kk = 0, h = 0;
        for (int c = 0; c < cols; c += 16) {  // (the same trip for every lane: cols, w are the job's)
            // 16 columns' loads first - an address past the row is clamped into it, its value never used -, then their fmafs in order
            float x[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (vec_h) {
                    load4<true>(row + min(c + 4 * u, cols - 4), 4, x[u]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) x[u][k] = row[min(c + 4 * u + k, cols - 1)];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 g4 = *reinterpret_cast<const float4 *>(g + c + 4 * u);
                const float gk[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (c + 4 * u + k < cols) {  // (uniform)
                        acc = fmaf(gk[k], x[u][k], acc);
                        if (++kk == w) {  // (uniform) the head's chain is complete: it goes to the head's register, selected without an indexed array
#pragma unroll
                            for (int hh = 0; hh < GT_HEADS; ++hh) da[hh] = hh == h ? acc : da[hh];
                            ++h, kk = 0, acc = 0.f;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int hh = 0; hh < GT_HEADS; ++hh)
            if (hh < heads) {
                const float t = sa_tanh_pre(si[hh], sv[hh]);
                const float u = fmaf(-t, t, 1.0f);
                const float v = ok ? (da[hh] * coef) * u : 0.f;
                d_pre[static_cast<int64_t>(e) * heads + hh] = v;
                ds[hh] = ds[hh] + v;
            }
    }
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) {
            const float total = gt_wave_sum(ds[h]);
            if (lane == 0) to_global(job->d_S)[static_cast<int64_t>(i) * job->ld_d_s + h] = total;
        }
}

// the pass over the transposed pattern: d_H[j, :] and d_S[j, heads + h]
__global__ __launch_bounds__(64 * GT_WAVES) void signed_att_backward_cols_kernel(const wdg_signed_att_job *__restrict__ jobs, const int max_rows) {
    __shared__ float stage_all[GT_WAVES][64 * GT_HEADS];
    const desc_ptr<wdg_signed_att_job> job = (desc_ptr<wdg_signed_att_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int j = blockIdx.x * GT_WAVES + wave;
    if (j >= s.n || !gt_has_backward(job, s.nnz)) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->t_rowptr), j, s.nnz, beg, end)) return;
    gt_transposed_row(job, s, j, beg, end, lane, stage_all[wave]);
}

}  // namespace

extern "C" int wdg_signed_att_forward_batched_f32(const wdg_signed_att_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = gt_check_table("signed_att_forward_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GT_WAVES)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(signed_att_forward_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("signed_att_forward_kernel");
}

extern "C" int wdg_signed_att_backward_batched_f32(const wdg_signed_att_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = gt_check_table("signed_att_backward_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GT_WAVES)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(signed_att_backward_rows_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    if (const int rc = wdg::check_launch("signed_att_backward_rows_kernel")) return rc;
    hipLaunchKernelGGL(signed_att_backward_cols_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);  // (reads the row pass's d_pre)
    return wdg::check_launch("signed_att_backward_cols_kernel");
}

// The per-job part of the contract, on the table the caller still holds on the host (train.SignedAttBatch calls this before it uploads).
extern "C" int wdg_signed_att_check_jobs(const wdg_signed_att_job *jobs_host, int32_t n_jobs) {
    if (const int rc = gt_check_table("signed_att_check_jobs", jobs_host, n_jobs, 0)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_signed_att_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0 && j.nnz >= 0, "signed_att_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.heads >= 1 && j.heads <= WDG_SIGNED_ATT_MAX_HEADS, "signed_att_check_jobs: job %d has %d heads; the kernel holds 1..%d", i, j.heads,
                    WDG_SIGNED_ATT_MAX_HEADS);
        WDG_REQUIRE(j.w >= 1 && static_cast<int64_t>(j.heads) * j.w <= WDG_SIGNED_ATT_MAX_COLS,
                    "signed_att_check_jobs: job %d has %d heads of %d columns; the kernel holds heads * w <= %d", i, j.heads, j.w, WDG_SIGNED_ATT_MAX_COLS);
        WDG_REQUIRE(std::isfinite(j.eps), "signed_att_check_jobs: job %d has an eps that is infinite or not a number", i);
        WDG_REQUIRE(j.flags == 0, "signed_att_check_jobs: job %d has flags %d; none is defined", i, j.flags);
        if (j.n == 0) continue;
        const int64_t cols = static_cast<int64_t>(j.heads) * j.w;
        WDG_REQUIRE(j.rowptr && j.H && j.S && j.out, "signed_att_check_jobs: job %d has a null rowptr, H, S or out", i);
        WDG_REQUIRE(j.nnz == 0 || (j.col && j.alpha), "signed_att_check_jobs: job %d has a null col or alpha", i);
        WDG_REQUIRE(j.ld_h >= cols && j.ld_out >= cols && j.ld_s >= 2 * j.heads, "signed_att_check_jobs: job %d has a leading dimension below its row", i);
        WDG_REQUIRE(!j.res || j.ld_res >= cols, "signed_att_check_jobs: job %d has a residual whose leading dimension lies below its row", i);
        const bool any = j.d_out || j.d_H || j.d_S || j.d_pre || j.t_rowptr || j.t_col || j.t_pos;
        if (!any) continue;
        WDG_REQUIRE(j.d_out && j.d_H && j.d_S && j.t_rowptr, "signed_att_check_jobs: job %d has some of d_out, d_H, d_S, t_rowptr and not others", i);
        WDG_REQUIRE(j.nnz == 0 || (j.d_pre && j.t_col && j.t_pos), "signed_att_check_jobs: job %d has a null d_pre, t_col or t_pos", i);
        WDG_REQUIRE(j.ld_d_out >= cols && j.ld_d_h >= cols && j.ld_d_s >= 2 * j.heads, "signed_att_check_jobs: job %d has a gradient's leading dimension below its row",
                    i);
    }
    return WDG_OK;
}
