// The channel mix of an ACM layer for many models in one launch, and its backward pass: per node a low-pass, a high-pass and an
// identity channel are scored (a row dot product and a sigmoid each), the scores go through a 3 x 3 matrix and a softmax, and the
// output is the weighted sum of the channels.  include/wdg.h states the arithmetic; tests/_acm_ref.py restates it in numpy.
//
// replaces: the use of the high-pass operator g_high = I - A_hat that the reference's loader returns (utils/util_funcs.py:198-204)
//           in the model family behind its "mf-GCN" / "mf-SGC" accuracy tables (gnns_on_syn.py:58-104, gnns_on_syn.py:159-206); the
//           models live upstream of the reference, which has no model code, so the layer is defined by this project.
//
// Ownership as in dropout.hip: a workgroup of 256 threads owns 64 rows of one job, thread (row slot t >> 4, column group t & 15)
// works on rows slot, slot + 16, slot + 32, slot + 48, and the 16 lanes of a row cover 256 contiguous bytes of it per 64-column
// chunk (one 16-byte access per lane where a matrix's pointer and leading dimension allow).  A row's channels stay in registers
// (3 x 4 x CH floats, CH = 64-column chunks of the table's widest job: 1, 2 or 4), row sums go over the 16 lanes in a fixed
// butterfly (every lane ends with the same bits), and nothing but the results is written.  Columns past a job's width are zeros
// in registers: they add exact zeros, so a job computes the same bits in a wider table's instantiation.
// The parameter gradients are sums over rows and must repeat bit for bit: no atomics.  A thread adds its four rows in order, the
// 16 row slots are added in order through LDS, the workgroup stores one vector per 64-row block, and acm_mix_reduce_kernel adds
// the blocks in block order (the store-and-sum form).
#include "wdg_common.h"
#include "acm_mix_row.h"  // the arithmetic of a row after its row sums, shared with acm_mix_packed.hip

#pragma clang fp contract(off)  // every multiply-add below is written out (fmaf or two operations): the same bits in every instantiation

namespace {

using namespace wdg;

constexpr int AM_TILE = acm::TILE, AM_THREADS = acm::THREADS, AM_SLOTS = acm::SLOTS, AM_ROWS_PER_THREAD = acm::ROWS_PER_THREAD;
constexpr int AM_MAX_JOBS = acm::MAX_JOBS;  // gridDim.z: a job per z

struct am_mat {  // one [rows, cols] operand of a job
    global_ptr<const float> p;
    int64_t ld;
    bool vec;  // 16-byte rows: pointer and leading dimension
};
__device__ __forceinline__ am_mat am_operand(const float *p, const int64_t ld) {
    return am_mat{to_global(p), ld, acm::rows_aligned16(p, ld)};
}
// four adjacent columns c .. c + 3 of row r; columns at or past `cols` read as +0
__device__ __forceinline__ void am_load4(const am_mat &m, const int r, const int c, const int cols, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (c >= cols) return;
    const global_ptr<const float> p = m.p + static_cast<int64_t>(r) * m.ld + c;
    if (m.vec && c + 3 < cols) {
        const float4 in = load_f32x4(p);
        v[0] = in.x, v[1] = in.y, v[2] = in.z, v[3] = in.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < cols) v[k] = p[k];
    }
}
__device__ __forceinline__ void am_store4(float *base, const int64_t ld, const int r, const int c, const int cols, const float (&v)[4]) {
    if (c >= cols) return;
    const global_ptr<float> p = to_global(base) + static_cast<int64_t>(r) * ld + c;
    if (acm::rows_aligned16(base, ld) && c + 3 < cols) {
        store_f32x4(p, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < cols) p[k] = v[k];
    }
}
// sum over the 16 lanes of a row, fixed order; every lane receives the same bits (each step adds a pair both ways)
__device__ __forceinline__ float am_row_sum(float v) {
    v = v + __shfl_xor(v, 1, 16);
    v = v + __shfl_xor(v, 2, 16);
    v = v + __shfl_xor(v, 4, 16);
    v = v + __shfl_xor(v, 8, 16);
    return v;
}

// the three channels of row r, columns 4 gq + 64 q .. + 3, activation applied: h[c][q][k]
template <int CH>
__device__ __forceinline__ void am_channels(const am_mat &low, const am_mat &high, const am_mat &agg, const bool has_agg, const am_mat &ident,
                                            const int r, const int gq, const int cols, const bool relu, float (&h)[3][CH][4]) {
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        const int c = 64 * q + 4 * gq;
        float a[4];
        am_load4(low, r, c, cols, h[0][q]);
        am_load4(high, r, c, cols, h[1][q]);
        am_load4(ident, r, c, cols, h[2][q]);
        if (has_agg) {
            am_load4(agg, r, c, cols, a);
#pragma unroll
            for (int k = 0; k < 4; ++k) h[1][q][k] = h[1][q][k] - a[k];
        }
        if (relu) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int k = 0; k < 4; ++k) h[ch][q][k] = acm::relu(h[ch][q][k]);
        }
    }
}
template <int CH>
__device__ __forceinline__ void am_load_att(const float *att_p, const int gq, const int cols, float (&att)[3][CH][4]) {
    const global_ptr<const float> p = to_global(att_p);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int q = 0; q < CH; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 64 * q + 4 * gq + k;
                att[ch][q][k] = c < cols ? p[static_cast<int64_t>(ch) * cols + c] : 0.f;
            }
}
// this lane's share of sum_k x[k] y[k]: chunk by chunk, column by column
template <int CH>
__device__ __forceinline__ float am_dot(const float (&x)[CH][4], const float (&y)[CH][4]) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < CH; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc = fmaf(x[q][k], y[q][k], acc);
    return acc;
}

template <int CH>
__global__ __launch_bounds__(AM_THREADS) void acm_mix_kernel(const wdg_acm_mix_job *__restrict__ jobs, const int max_rows, const int max_cols) {
    __shared__ float tile[AM_TILE][AM_TILE + 1];
    const desc_ptr<wdg_acm_mix_job> job = (desc_ptr<wdg_acm_mix_job>)(jobs + blockIdx.z);
    const int rows = min(job->rows, max_rows), cols = job->cols;
    const int r0 = blockIdx.x * AM_TILE;
    if (r0 >= rows || cols < 1 || cols > max_cols) return;  // (uniform: before any barrier)
    const am_mat low = am_operand(job->low, job->ld_low), high = am_operand(job->high, job->ld_high),
                 agg = am_operand(job->high_agg, job->ld_high_agg), ident = am_operand(job->ident, job->ld_ident);
    const bool has_agg = job->high_agg != nullptr, relu = (job->flags & WDG_ACM_RELU) != 0, transposed = job->out_t != nullptr;
    const int t = threadIdx.x, gq = t & 15, slot = t >> 4;
    float att[3][CH][4], wm[9], o[AM_ROWS_PER_THREAD][CH][4];
    am_load_att<CH>(job->att, gq, cols, att);
#pragma unroll
    for (int i = 0; i < 9; ++i) wm[i] = to_global(job->wmix)[i];
    const global_ptr<float> aux = to_global(job->aux);
#pragma unroll
    for (int m = 0; m < AM_ROWS_PER_THREAD; ++m) {
        const int r = r0 + slot + AM_SLOTS * m;
#pragma unroll
        for (int q = 0; q < CH; ++q) o[m][q][0] = o[m][q][1] = o[m][q][2] = o[m][q][3] = 0.f;
        if (r >= rows) continue;  // (the 16 lanes of a row together)
        float h[3][CH][4], dot[3], s[3], al[3];
        am_channels<CH>(low, high, agg, has_agg, ident, r, gq, cols, relu, h);
#pragma unroll
        for (int c = 0; c < 3; ++c) dot[c] = am_row_sum(am_dot<CH>(h[c], att[c]));
        acm::alpha(dot, wm, s, al);
#pragma unroll
        for (int q = 0; q < CH; ++q) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[m][q][k] = acm::mix(al, h[0][q][k], h[1][q][k], h[2][q][k]);
            am_store4(job->out, job->ld_out, r, 64 * q + 4 * gq, cols, o[m][q]);
        }
        if (gq < acm::AUX_WORDS) {  // aux[r] = alpha_L alpha_H alpha_I s_L s_H s_I 0 0: a lane per word
            const float w = gq == 0 ? al[0] : gq == 1 ? al[1] : gq == 2 ? al[2] : gq == 3 ? s[0] : gq == 4 ? s[1] : gq == 5 ? s[2] : 0.f;
            aux[static_cast<int64_t>(r) * acm::AUX_WORDS + gq] = w;
        }
    }
    if (!transposed) return;  // (uniform)
    const global_ptr<float> ot = to_global(job->out_t);
    const int64_t ld_t = job->ld_out_t;
    const int rl = t & 63, rt = r0 + rl;
#pragma unroll
    for (int q = 0; q < CH; ++q) {
        if (64 * q >= cols) break;  // (uniform)
        if (q) __syncthreads();  // the previous chunk's columns have been read
#pragma unroll
        for (int m = 0; m < AM_ROWS_PER_THREAD; ++m)
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[slot + AM_SLOTS * m][4 * gq + k] = o[m][q][k];
        __syncthreads();
        if (rt < rows) {
#pragma unroll
            for (int m = 0; m < AM_TILE / 4; ++m) {
                const int cl = (t >> 6) + 4 * m, c = 64 * q + cl;
                if (c < cols) ot[static_cast<int64_t>(c) * ld_t + rt] = tile[rl][cl];
            }
        }
    }
}

// floats of a block's partial vector: d_att [3, cols] then d_wmix [9]
__host__ __device__ constexpr int am_partial_len(const int cols) { return 3 * cols + 9; }

template <int CH>
__global__ __launch_bounds__(AM_THREADS) void acm_mix_backward_kernel(const wdg_acm_mix_job *__restrict__ jobs, const int max_rows, const int max_cols) {
    constexpr int RED = 3 * 64 * CH + 12;  // a row slot's sums: d_att by (channel, column), then d_wmix
    __shared__ float red[AM_SLOTS][RED];
    const desc_ptr<wdg_acm_mix_job> job = (desc_ptr<wdg_acm_mix_job>)(jobs + blockIdx.z);
    const int rows = min(job->rows, max_rows), cols = job->cols;
    const int r0 = blockIdx.x * AM_TILE;
    if (r0 >= rows || cols < 1 || cols > max_cols) return;  // (uniform: before any barrier)
    const am_mat low = am_operand(job->low, job->ld_low), high = am_operand(job->high, job->ld_high),
                 agg = am_operand(job->high_agg, job->ld_high_agg), ident = am_operand(job->ident, job->ld_ident),
                 dout = am_operand(job->d_out, job->ld_d_out);
    const bool has_agg = job->high_agg != nullptr, relu = (job->flags & WDG_ACM_RELU) != 0;
    const int t = threadIdx.x, gq = t & 15, slot = t >> 4;
    float att[3][CH][4], wm[9], da[3][CH][4], dw[9];
    am_load_att<CH>(job->att, gq, cols, att);
#pragma unroll
    for (int i = 0; i < 9; ++i) wm[i] = to_global(job->wmix)[i], dw[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < CH; ++q) da[c][q][0] = da[c][q][1] = da[c][q][2] = da[c][q][3] = 0.f;
    const global_ptr<const float> aux = to_global(const_cast<const float *>(job->aux));
    float *const d_mat[3] = {job->d_low, job->d_high, job->d_ident};
    const int64_t d_ld[3] = {job->ld_d_low, job->ld_d_high, job->ld_d_ident};
#pragma unroll
    for (int m = 0; m < AM_ROWS_PER_THREAD; ++m) {
        const int r = r0 + slot + AM_SLOTS * m;
        if (r >= rows) continue;  // (the 16 lanes of a row together)
        float h[3][CH][4], g[CH][4], al[3], s[3], dal[3], du[3];
        am_channels<CH>(low, high, agg, has_agg, ident, r, gq, cols, relu, h);
#pragma unroll
        for (int q = 0; q < CH; ++q) am_load4(dout, r, 64 * q + 4 * gq, cols, g[q]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            al[c] = aux[static_cast<int64_t>(r) * acm::AUX_WORDS + acm::AUX_ALPHA + c];
            s[c] = aux[static_cast<int64_t>(r) * acm::AUX_WORDS + acm::AUX_S + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dal[c] = 3.0f * am_row_sum(am_dot<CH>(g, h[c]));
        acm::scores_backward(al, s, dal, wm, du, dw);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a3 = 3.0f * al[c];
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                float dp[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) dp[k] = acm::input_gradient(a3, g[q][k], du[c], att[c][q][k], h[c][q][k], relu, da[c][q][k]);
                am_store4(d_mat[c], d_ld[c], r, 64 * q + 4 * gq, cols, dp);
            }
        }
    }
    // the 16 row slots' sums, added in slot order
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < CH; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[slot][c * 64 * CH + 64 * q + 4 * gq + k] = da[c][q][k];
    if (gq == 0) {  // (every lane of a row holds the same d_wmix terms: lane 0 speaks for the slot)
#pragma unroll
        for (int i = 0; i < 9; ++i) red[slot][3 * 64 * CH + i] = dw[i];
    }
    __syncthreads();
    const global_ptr<float> part = to_global(job->partials) + static_cast<int64_t>(blockIdx.x) * am_partial_len(cols);
    for (int i = t; i < am_partial_len(cols); i += AM_THREADS) {
        const int c = i / cols, k = i - c * cols;
        const int at = i < 3 * cols ? c * 64 * CH + k : 3 * 64 * CH + (i - 3 * cols);
        float acc = 0.f;
#pragma unroll
        for (int sl = 0; sl < AM_SLOTS; ++sl) acc = acc + red[sl][at];
        part[i] = acc;
    }
}

// d_att / d_wmix of a job = its blocks' partial vectors added in block order
__global__ __launch_bounds__(AM_THREADS) void acm_mix_reduce_kernel(const wdg_acm_mix_job *__restrict__ jobs, const int max_rows, const int max_cols) {
    const desc_ptr<wdg_acm_mix_job> job = (desc_ptr<wdg_acm_mix_job>)(jobs + blockIdx.y);
    const int rows = min(job->rows, max_rows), cols = job->cols;
    if (cols < 1 || cols > max_cols) return;
    const int len = am_partial_len(cols), i = blockIdx.x * AM_THREADS + threadIdx.x;
    if (i >= len) return;
    const int blocks = (rows + AM_TILE - 1) / AM_TILE;
    const global_ptr<const float> part = to_global(const_cast<const float *>(job->partials));
    float acc = 0.f;
    for (int b = 0; b < blocks; ++b) acc = acc + part[static_cast<int64_t>(b) * len + i];
    if (i < 3 * cols)
        to_global(job->d_att)[i] = acc;
    else
        to_global(job->d_wmix)[i - 3 * cols] = acc;
}

int am_check(const char *what, const wdg_acm_mix_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "%s: negative count", what);
    WDG_REQUIRE(n_jobs <= AM_MAX_JOBS, "%s: %d jobs; one launch takes %d", what, n_jobs, AM_MAX_JOBS);
    WDG_REQUIRE(max_cols <= WDG_ACM_MAX_COLS, "%s: %d columns; the kernel holds a row of at most %d", what, max_cols, WDG_ACM_MAX_COLS);
    WDG_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "%s: null job table", what);
    return WDG_OK;
}

}  // namespace

extern "C" int wdg_acm_mix_batched_f32(const wdg_acm_mix_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream) {
    if (const int rc = am_check("acm_mix_batched", jobs_dev, n_jobs, max_rows, max_cols)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_cols == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, AM_TILE)), 1, static_cast<unsigned>(n_jobs));
    if (max_cols <= 64)
        hipLaunchKernelGGL(acm_mix_kernel<1>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
    else if (max_cols <= 128)
        hipLaunchKernelGGL(acm_mix_kernel<2>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
    else
        hipLaunchKernelGGL(acm_mix_kernel<4>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
    return wdg::check_launch("acm_mix_kernel");
}

extern "C" int wdg_acm_mix_backward_batched_f32(const wdg_acm_mix_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                                wdg_stream_t stream) {
    if (const int rc = am_check("acm_mix_backward_batched", jobs_dev, n_jobs, max_rows, max_cols)) return rc;
    if (n_jobs == 0 || max_cols == 0) return WDG_OK;
    if (max_rows > 0) {
        const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, AM_TILE)), 1, static_cast<unsigned>(n_jobs));
        if (max_cols <= 64)
            hipLaunchKernelGGL(acm_mix_backward_kernel<1>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
        else if (max_cols <= 128)
            hipLaunchKernelGGL(acm_mix_backward_kernel<2>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
        else
            hipLaunchKernelGGL(acm_mix_backward_kernel<4>, grid, dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
        if (const int rc = wdg::check_launch("acm_mix_backward_kernel")) return rc;
    }
    hipLaunchKernelGGL(acm_mix_reduce_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(am_partial_len(max_cols), AM_THREADS)), static_cast<unsigned>(n_jobs)),
                       dim3(AM_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols);
    return wdg::check_launch("acm_mix_reduce_kernel");
}
