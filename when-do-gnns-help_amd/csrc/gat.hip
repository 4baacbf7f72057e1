// Graph attention for many graphs in one launch: per stored entry a score, per row a softmax over its entries, and the weighted sum
// of the neighbours' rows - out_i = sum_j alpha_ij H_j - with its backward pass, and the positions that tie a transposed CSR to its
// forward pattern (wdg_csr_transpose_positions).  include/wdg.h states the arithmetic and every sum's order; tests/_gat_ref.py
// restates both passes in numpy fp64.
//
// replaces: the FIXED weights of the aggregation - normalize_tensor, utils/util_funcs.py:365-381 - by a weight learnt per edge, in the
//           baseline that stands beside the GCN / SGC tables of gnns_on_syn.py:1-154; the reference ships no model code, so the layer
//           is defined by this project.
//
// Shape: a WAVE per row (the band kernel's shape: the gathered rows come from L2), four rows per workgroup, a job per grid z.
//   forward   the lanes run over the row's entries, 64 at a time: pre, the maximum, exp and Z per head (the un-normalised q is parked
//             in alpha[] by the lane that reads it back); then, chunk by chunk, alpha goes to global memory and to the wave's LDS stage
//             and the lanes switch to the heads * w columns - four per lane, one 16-byte load where pointer and leading dimension
//             allow - and walk the chunk's entries in order: one fmaf chain per column.
//   backward  rows: the lanes run over entries again; a lane reads its neighbour's whole row against d_out[i, :] (in LDS) - dalpha is
//             one fmaf chain over k per head -, parks it in d_pre[], then c, d_pre and d_S[i, h].
//             transposed rows: the forward's second half with alpha gathered through t_pos and d_out in the place of H.
// Nothing is added across rows, so there is no atomic; every cross-lane sum is the butterfly of gt_wave_sum.
// Loads in flight: the job's pointers come out of a table, so the compiler must assume that a store to alpha[] or d_pre[] aliases any
// later load, and a value loaded under a per-lane branch is waited for at the branch's end.  Every pass therefore issues ALL the loads
// of a step first - the heads of an entry, the GT_DEPTH rows of a batch, 16 columns of a neighbour's row - into registers, through
// addresses that are clamped into range instead of predicated, and only then computes and stores; the 16-byte path is the WAVE's
// decision.  The first form of this file left one wait behind every load and ran at 1.5 - 1.8 times these times.
// Guards: an entry whose column (or whose t_pos) lies outside the job is skipped - never read through -, a row whose extent lies outside
// [0, nnz] and a job outside the limits are left untouched.
#include "gat_lanes.h"

namespace {

using namespace wdg_gt;

// the wave's maximum; fmaxf skips a NaN, and the value of a maximum does not depend on the order
__device__ __forceinline__ float gt_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float gt_leaky(const float pre, const float slope) { return pre > 0.f ? pre : slope * pre; }

__global__ __launch_bounds__(64 * GT_WAVES) void gat_forward_kernel(const wdg_gat_job *__restrict__ jobs, const int max_rows) {
    __shared__ float stage_all[GT_WAVES][64 * GT_HEADS];
    const desc_ptr<wdg_gat_job> job = (desc_ptr<wdg_gat_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int i = blockIdx.x * GT_WAVES + wave;
    if (i >= s.n || !job->rowptr || !job->H || !job->S || !job->out || (s.nnz > 0 && (!job->col || !job->alpha))) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->rowptr), i, s.nnz, beg, end)) return;
    const int heads = s.heads, n = job->n;
    const float slope = job->slope;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<const float> S = to_global(job->S), H = to_global(job->H);
    const global_ptr<float> alpha = to_global(job->alpha);
    const int64_t ld_s = job->ld_s;
    float *stage = stage_all[wave];

    float si[GT_HEADS], m[GT_HEADS], z[GT_HEADS];
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h) {
        si[h] = S[static_cast<int64_t>(i) * ld_s + min(h, heads - 1)];  // (a head the job does not have reads its last one: no branch)
        m[h] = -INFINITY, z[h] = 0.f;
    }
    // the maximum of e over the row, per head
    for (int e = beg + lane; e < end; e += 64) {
        const int j = col[e];
        if (static_cast<unsigned>(j) >= static_cast<unsigned>(n)) continue;
        const global_ptr<const float> sj = S + static_cast<int64_t>(j) * ld_s + heads;
        float sv[GT_HEADS];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) sv[h] = sj[min(h, heads - 1)];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) m[h] = fmaxf(m[h], gt_leaky(si[h] + sv[h], slope));
    }
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) m[h] = gt_wave_max(m[h]);
    // q = exp(e - m), parked in alpha[]; Z: a lane adds its entries (lane, lane + 64, ...) in ascending order, then the butterfly
    for (int e = beg + lane; e < end; e += 64) {
        const int j = col[e];
        const bool ok = static_cast<unsigned>(j) < static_cast<unsigned>(n);
        const global_ptr<const float> sj = S + static_cast<int64_t>(ok ? j : 0) * ld_s + heads;
        float sv[GT_HEADS];  // every load before the first store: the compiler cannot know that alpha[] aliases none of them
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) sv[h] = sj[min(h, heads - 1)];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h)
            if (h < heads) {
                const float q = ok ? expf(gt_leaky(si[h] + sv[h], slope) - m[h]) : 0.f;
                alpha[static_cast<int64_t>(e) * heads + h] = q;
                z[h] = z[h] + q;
            }
    }
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) z[h] = gt_wave_sum(z[h]);
    // alpha = q / Z to global memory and to the stage, then the columns' chains over the chunk
    const gt_lane_cols lc = gt_columns(lane, heads, s.w);
    const bool one_head = (s.w & 3) == 0, vec_h = gt_wave_vec(job->H, job->ld_h, s.cols);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);  // (wave-uniform)
        const bool mine = lane < cnt;
        int j = mine ? col[e0 + lane] : -1;
        if (static_cast<unsigned>(j) >= static_cast<unsigned>(n)) j = -1;
        const int64_t at = static_cast<int64_t>(mine ? e0 + lane : end - 1) * heads;  // (a lane without an entry reads the row's last: no branch between a load and its use)
        float qv[GT_HEADS];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) qv[h] = alpha[at + min(h, heads - 1)];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h)
            if (h < heads) {
                const float a = mine ? qv[h] / z[h] : 0.f;
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
    if (lc.live > 0)
        gt_store4(to_global(job->out) + static_cast<int64_t>(i) * job->ld_out + lc.c0, gt_wave_vec(job->out, job->ld_out, s.cols), lc.live, acc);
}

// the row pass: d_pre[p, h] and d_S[i, h]
__global__ __launch_bounds__(64 * GT_WAVES) void gat_backward_rows_kernel(const wdg_gat_job *__restrict__ jobs, const int max_rows) {
    __shared__ __attribute__((aligned(16))) float g_all[GT_WAVES][WDG_GAT_MAX_COLS];
    const desc_ptr<wdg_gat_job> job = (desc_ptr<wdg_gat_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int i = blockIdx.x * GT_WAVES + wave;
    if (i >= s.n || !gt_has_backward(job, s.nnz)) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->rowptr), i, s.nnz, beg, end)) return;
    const int heads = s.heads, w = s.w, cols = s.cols, n = job->n;
    const float slope = job->slope;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<const float> S = to_global(job->S), H = to_global(job->H), alpha = to_global(const_cast<const float *>(job->alpha));
    const global_ptr<float> d_pre = to_global(job->d_pre);
    const int64_t ld_s = job->ld_s, ld_h = job->ld_h;
    float *g = g_all[wave];
    gt_stage_d_out(job, s, i, lane, g);  // g = d_out[i, :] into LDS, +0 past the job's columns
    gt_wave_sync();
    // dalpha[p, h] = one fmaf chain over k ascending from +0, parked in d_pre[]: a lane per entry reads its neighbour's row
    const bool vec_h = gt_wave_vec(job->H, ld_h, cols);
    for (int e = beg + lane; e < end; e += 64) {
        const int j = col[e];
        const bool ok = static_cast<unsigned>(j) < static_cast<unsigned>(n);
        const global_ptr<const float> row = H + static_cast<int64_t>(ok ? j : 0) * ld_h;
        const global_ptr<float> park = d_pre + static_cast<int64_t>(e) * heads;
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
                        if (++kk == w) {
                            park[h] = ok ? acc : 0.f;
                            ++h, kk = 0, acc = 0.f;
                        }
                    }
                }
            }
        }
    }
    // c = sum_p alpha dalpha: a lane's fmaf chain over its entries in ascending order, then the butterfly
    float si[GT_HEADS], cs[GT_HEADS], ds[GT_HEADS];
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h) {
        si[h] = S[static_cast<int64_t>(i) * ld_s + min(h, heads - 1)];  // (a head the job does not have reads its last one: no branch)
        cs[h] = 0.f, ds[h] = 0.f;
    }
    for (int e = beg + lane; e < end; e += 64) {
        float av[GT_HEADS], dv[GT_HEADS];
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) {
            av[h] = alpha[static_cast<int64_t>(e) * heads + min(h, heads - 1)];
            dv[h] = d_pre[static_cast<int64_t>(e) * heads + min(h, heads - 1)];
        }
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) cs[h] = fmaf(av[h], dv[h], cs[h]);
    }
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) cs[h] = gt_wave_sum(cs[h]);
    // d_pre = (alpha (dalpha - c)) gate, and d_S[i, h]: the order of Z
    for (int e = beg + lane; e < end; e += 64) {
        const int j = col[e];
        const bool ok = static_cast<unsigned>(j) < static_cast<unsigned>(n);
        const global_ptr<const float> sj = S + static_cast<int64_t>(ok ? j : 0) * ld_s + heads;
        float sv[GT_HEADS], dv[GT_HEADS], av[GT_HEADS];  // every load before the first store
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h) {
            const int hh = min(h, heads - 1);
            sv[h] = sj[hh], dv[h] = d_pre[static_cast<int64_t>(e) * heads + hh], av[h] = alpha[static_cast<int64_t>(e) * heads + hh];
        }
#pragma unroll
        for (int h = 0; h < GT_HEADS; ++h)
            if (h < heads) {
                const float gate = si[h] + sv[h] > 0.f ? 1.f : slope;
                const float t = dv[h] - cs[h];
                const float u = av[h] * t;
                const float v = ok ? u * gate : 0.f;
                d_pre[static_cast<int64_t>(e) * heads + h] = v;
                ds[h] = ds[h] + v;
            }
    }
#pragma unroll
    for (int h = 0; h < GT_HEADS; ++h)
        if (h < heads) {
            const float total = gt_wave_sum(ds[h]);
            if (lane == 0) to_global(job->d_S)[static_cast<int64_t>(i) * job->ld_d_s + h] = total;
        }
}

// the pass over the transposed pattern: d_H[j, :] and d_S[j, heads + h].  signed_att.hip runs the same pass as gt_transposed_row of
// gat_lanes.h; here it stays written out: called through that function the compiler ends at 82 registers instead of 80 - five waves
// per SIMD instead of six - and this kernel is to compile to the code it had.  A change to one is a change to the other.
__global__ __launch_bounds__(64 * GT_WAVES) void gat_backward_cols_kernel(const wdg_gat_job *__restrict__ jobs, const int max_rows) {
    __shared__ float stage_all[GT_WAVES][64 * GT_HEADS];
    const desc_ptr<wdg_gat_job> job = (desc_ptr<wdg_gat_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    gt_shape s;
    if (!gt_job_shape(job, max_rows, s)) return;
    const int j = blockIdx.x * GT_WAVES + wave;
    if (j >= s.n || !gt_has_backward(job, s.nnz)) return;  // (wave-uniform)
    int beg, end;
    if (!row_extent(to_global(job->t_rowptr), j, s.nnz, beg, end)) return;
    const int heads = s.heads, n = job->n;
    const global_ptr<const int32_t> t_col = to_global(job->t_col), t_pos = to_global(job->t_pos);
    const global_ptr<const float> alpha = to_global(const_cast<const float *>(job->alpha)), d_pre = to_global(const_cast<const float *>(job->d_pre));
    float *stage = stage_all[wave];
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

// a thread per row r: whether row r of either pattern is not strictly ascending (or holds a column outside [0, n)), and, for every entry
// q of transposed row r - the forward entry (t_col[q], r) -, its position in the forward row by binary search
__global__ __launch_bounds__(256) void csr_transpose_positions_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                      const int32_t *__restrict__ t_rowptr, const int32_t *__restrict__ t_col, const int n,
                                                                      int32_t *__restrict__ t_pos, int32_t *__restrict__ bad) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int nnz = rowptr[n], t_nnz = t_rowptr[n];
    int count = 0;
    {
        const int b = rowptr[r], e = rowptr[r + 1];
        bool fine = b >= 0 && b <= e && e <= nnz;
        for (int p = b; fine && p < e; ++p) fine = static_cast<unsigned>(col[p]) < static_cast<unsigned>(n) && (p == b || col[p - 1] < col[p]);
        count += fine ? 0 : 1;
    }
    const int tb = t_rowptr[r], te = t_rowptr[r + 1];
    if (tb < 0 || tb > te || te > t_nnz) {
        count += 1;
    } else {
        bool fine = true;
        for (int q = tb; q < te; ++q) {
            const int i = t_col[q];
            if (q > tb && t_col[q - 1] >= i) fine = false;
            int found = -1;
            if (static_cast<unsigned>(i) < static_cast<unsigned>(n)) {
                int lo = rowptr[i], hi = rowptr[i + 1];
                if (lo >= 0 && lo <= hi && hi <= nnz) {
                    const int last = hi;
                    while (lo < hi) {  // the first position whose column is not below r
                        const int mid = lo + (hi - lo) / 2;
                        if (col[mid] < r)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    if (lo < last && col[lo] == r) found = lo;
                }
            }
            t_pos[q] = found;
            count += found < 0 ? 1 : 0;
        }
        count += fine ? 0 : 1;
    }
    if (count) atomicAdd(bad, count);
}

int gt_check(const char *what, const wdg_gat_job *jobs, int32_t n_jobs, int32_t max_rows) { return gt_check_table(what, jobs, n_jobs, max_rows); }

}  // namespace

extern "C" int wdg_gat_forward_batched_f32(const wdg_gat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = gt_check("gat_forward_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GT_WAVES)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gat_forward_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("gat_forward_kernel");
}

extern "C" int wdg_gat_backward_batched_f32(const wdg_gat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = gt_check("gat_backward_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GT_WAVES)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gat_backward_rows_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    if (const int rc = wdg::check_launch("gat_backward_rows_kernel")) return rc;
    hipLaunchKernelGGL(gat_backward_cols_kernel, grid, dim3(64 * GT_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);  // (reads the row pass's d_pre)
    return wdg::check_launch("gat_backward_cols_kernel");
}

// The per-job part of the contract, on the table the caller still holds on the host (train.GatBatch calls this before it uploads).
extern "C" int wdg_gat_check_jobs(const wdg_gat_job *jobs_host, int32_t n_jobs) {
    if (const int rc = gt_check("gat_check_jobs", jobs_host, n_jobs, 0)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_gat_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0 && j.nnz >= 0, "gat_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.heads >= 1 && j.heads <= WDG_GAT_MAX_HEADS, "gat_check_jobs: job %d has %d heads; the kernel holds 1..%d", i, j.heads, WDG_GAT_MAX_HEADS);
        WDG_REQUIRE(j.w >= 1 && static_cast<int64_t>(j.heads) * j.w <= WDG_GAT_MAX_COLS, "gat_check_jobs: job %d has %d heads of %d columns; the kernel holds heads * w <= %d",
                    i, j.heads, j.w, WDG_GAT_MAX_COLS);
        WDG_REQUIRE(j.slope >= 0.f, "gat_check_jobs: job %d has a slope that is negative or not a number", i);  // (a NaN fails the comparison)
        WDG_REQUIRE(j.flags == 0, "gat_check_jobs: job %d has flags %d; none is defined", i, j.flags);
        if (j.n == 0) continue;
        const int64_t cols = static_cast<int64_t>(j.heads) * j.w;
        WDG_REQUIRE(j.rowptr && j.H && j.S && j.out, "gat_check_jobs: job %d has a null rowptr, H, S or out", i);
        WDG_REQUIRE(j.nnz == 0 || (j.col && j.alpha), "gat_check_jobs: job %d has a null col or alpha", i);
        WDG_REQUIRE(j.ld_h >= cols && j.ld_out >= cols && j.ld_s >= 2 * j.heads, "gat_check_jobs: job %d has a leading dimension below its row", i);
        const bool any = j.d_out || j.d_H || j.d_S || j.d_pre || j.t_rowptr || j.t_col || j.t_pos;
        if (!any) continue;
        WDG_REQUIRE(j.d_out && j.d_H && j.d_S && j.t_rowptr, "gat_check_jobs: job %d has some of d_out, d_H, d_S, t_rowptr and not others", i);
        WDG_REQUIRE(j.nnz == 0 || (j.d_pre && j.t_col && j.t_pos), "gat_check_jobs: job %d has a null d_pre, t_col or t_pos", i);
        WDG_REQUIRE(j.ld_d_out >= cols && j.ld_d_h >= cols && j.ld_d_s >= 2 * j.heads, "gat_check_jobs: job %d has a gradient's leading dimension below its row", i);
    }
    return WDG_OK;
}

extern "C" int wdg_csr_transpose_positions(const int32_t *rowptr, const int32_t *col, const int32_t *t_rowptr, const int32_t *t_col, int32_t n,
                                           int32_t *t_pos, int32_t *bad_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n >= 0, "csr_transpose_positions: negative count");
    WDG_REQUIRE(bad_dev != nullptr, "csr_transpose_positions: null count word");
    WDG_REQUIRE(rowptr && t_rowptr, "csr_transpose_positions: null row pointers");
    hipStream_t st = wdg::as_stream(stream);
    if (hipMemsetAsync(bad_dev, 0, sizeof(int32_t), st) != hipSuccess) return wdg::fail(WDG_ERR_LAUNCH, "csr_transpose_positions: the count word could not be cleared");
    if (n == 0) return WDG_OK;
    hipLaunchKernelGGL(csr_transpose_positions_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(n, 256))), dim3(256), 0, st, rowptr, col, t_rowptr, t_col, n,
                       t_pos, bad_dev);
    return wdg::check_launch("csr_transpose_positions_kernel");
}
