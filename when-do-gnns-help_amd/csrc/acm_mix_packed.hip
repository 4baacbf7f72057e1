// The channel mix of an ACM layer (csrc/acm_mix.hip; include/wdg.h states the arithmetic) for STACKED narrow layers: a job is one
// [rows, reps * stride] layer of `reps` replicas - the splits of one graph trained as one run - of `cols` <= stride real columns
// each, stride 4, 8 or 16 floats.  acm_mix.hip gives a row of one job to 16 lanes; a class-width replica would use 1, 2 or 4 of
// them and the rows would be walked once per replica.  Here 1, 2 or 4 adjacent lanes are one replica and 16, 8 or 4 replicas share
// the 256 contiguous bytes that the 16 lanes of a row cover: one pass over the rows for all replicas.
//
// replaces: the use of the high-pass operator g_high = I - A_hat that the reference's loader returns (utils/util_funcs.py:198-204)
//           in the model family behind its "mf-GCN" / "mf-SGC" accuracy tables (gnns_on_syn.py:58-104, gnns_on_syn.py:159-206); the
//           models live upstream of the reference, which has no model code, so the layer is defined by this project.
//
// Ownership is acm_mix.hip's, so that a replica's bits are the bits of a one-job launch of acm_mix.hip on its column slices: a
// workgroup of 256 threads owns 64 rows x 64 columns (grid: row blocks, column blocks, jobs), thread (row slot t >> 4, lane t & 15)
// works on rows slot, slot + 16, slot + 32, slot + 48 and holds 4 adjacent columns.  A lane's share of a row dot product is the
// same fmaf chain over its 4 columns (padding columns are +0 in registers), the row sum is am_row_sum's butterfly cut to the
// replica's lanes (xor 1, then xor 2: no step across a replica boundary) and the steps that acm_mix.hip takes over lanes that hold
// zeros are one addition of +0 (which turns a -0 sum into the +0 it is there).  The parameter gradients take the store-and-sum
// form: a thread adds its four rows in order, the 16 row slots are added in slot order through LDS, the workgroup stores one
// vector per (64-row block, replica), and acm_packed_reduce_kernel adds the blocks in block order.  No floating-point atomics.
// Every access to a matrix, to att / d_att, aux and the partial sums is a 16-byte one (the preconditions: 16-byte aligned pointers,
// leading dimensions that are multiples of 4); wmix / d_wmix are [reps, 9] and are read and written word by word.
#include "wdg_common.h"
#include "acm_mix_row.h"  // the arithmetic of a row after its row sums, shared with acm_mix.hip: one text, so one set of bits

#pragma clang fp contract(off)  // every multiply-add below is written out (fmaf or two operations): acm_mix.hip's bits

namespace {

using namespace wdg;

constexpr int AP_TILE = acm::TILE, AP_THREADS = acm::THREADS, AP_SLOTS = acm::SLOTS, AP_ROWS_PER_THREAD = acm::ROWS_PER_THREAD;
constexpr int AP_MAX_JOBS = acm::MAX_JOBS;       // gridDim.z: a job per z
constexpr int64_t AP_MAX_WIDTH = 64LL * 65535;   // gridDim.y: a 64-column block per y
constexpr int AP_RED_DW = 3 * AP_TILE;           // a row slot's sums in LDS: d_att [3][64], then 12 words of d_wmix per replica

__host__ __device__ constexpr int ap_partial_len(const int stride) { return 3 * stride + 12; }  // d_att [3, stride], d_wmix [9], 3 unused

// what makes a job malformed (the kernels skip such a job; wdg_acm_mix_packed_check_jobs says which rule it breaks)
template <typename J>
__host__ __device__ inline const char *ap_defect(const J job, const bool backward) {
    const int stride = job->stride, cols = job->cols, reps = job->reps;
    if (stride != 4 && stride != 8 && stride != 16) return "a stride outside {4, 8, 16}";
    if (cols < 1 || cols > stride) return "a column count outside 1 .. stride";
    if (reps < 1) return "fewer than one replica";
    if (job->rows < 0) return "a negative row count";
    const int64_t width = static_cast<int64_t>(reps) * stride;
    if (width > AP_MAX_WIDTH) return "more columns than one launch takes";
    const bool empty = job->rows == 0;  // (a matrix without rows has no memory: its pointer may be null)
    if (!job->att || !job->wmix || (!empty && (!job->low || !job->high || !job->ident || !job->out || !job->aux))) return "a null required pointer";
    if (job->ld_low < width || job->ld_high < width || job->ld_ident < width || job->ld_out < width || (job->high_agg && job->ld_high_agg < width))
        return "a leading dimension below reps * stride";
    if (!acm::rows_aligned16(job->low, job->ld_low) || !acm::rows_aligned16(job->high, job->ld_high) || !acm::rows_aligned16(job->ident, job->ld_ident) ||
        !acm::rows_aligned16(job->out, job->ld_out) || (job->high_agg && !acm::rows_aligned16(job->high_agg, job->ld_high_agg)) || !acm::rows_aligned16(job->att, 0) || !acm::rows_aligned16(job->aux, 0))
        return "a pointer that is not 16-byte aligned or a leading dimension that is no multiple of 4";
    const bool any = job->d_out || job->d_low || job->d_high || job->d_ident || job->d_att || job->d_wmix || job->partials;
    if (!backward && !any) return nullptr;
    if (!job->d_att || !job->d_wmix || (!empty && (!job->d_out || !job->d_low || !job->d_high || !job->d_ident || !job->partials)))
        return "a null required pointer (the gradient arrays come together)";
    if (job->ld_d_out < width || job->ld_d_low < width || job->ld_d_high < width || job->ld_d_ident < width)
        return "a leading dimension below reps * stride";
    if (!acm::rows_aligned16(job->d_out, job->ld_d_out) || !acm::rows_aligned16(job->d_low, job->ld_d_low) || !acm::rows_aligned16(job->d_high, job->ld_d_high) ||
        !acm::rows_aligned16(job->d_ident, job->ld_d_ident) || !acm::rows_aligned16(job->d_att, 0) || !acm::rows_aligned16(job->partials, 0))
        return "a pointer that is not 16-byte aligned or a leading dimension that is no multiple of 4";
    return nullptr;
}

// this lane's four columns of a row; the padding columns (k >= real) count as +0 whatever memory holds
__device__ __forceinline__ void ap_load4(const global_ptr<const float> base, const int64_t at, const int real, float (&v)[4]) {
    const float4 in = load_f32x4(base + at);
    v[0] = real > 0 ? in.x : 0.f, v[1] = real > 1 ? in.y : 0.f, v[2] = real > 2 ? in.z : 0.f, v[3] = real > 3 ? in.w : 0.f;
}
// sum over the lanes of a replica, am_row_sum's order; every lane of the replica receives the same bits
__device__ __forceinline__ float ap_seg_sum(float v, const int stride) {
    if (stride >= 8) v = v + __shfl_xor(v, 1, 16);   // (uniform: a job has one stride)
    if (stride >= 16) v = v + __shfl_xor(v, 2, 16);
    return v + 0.f;  // am_row_sum's remaining steps add lanes that hold +0
}
__device__ __forceinline__ float ap_dot(const float (&x)[4], const float (&y)[4]) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(x[k], y[k], acc);
    return acc;
}

struct ap_operands {
    global_ptr<const float> low, high, agg, ident;
    int64_t ld_low, ld_high, ld_agg, ld_ident;
    bool has_agg, relu;
};
__device__ __forceinline__ ap_operands ap_read_operands(const desc_ptr<wdg_acm_packed_job> job) {
    return ap_operands{to_global(job->low), to_global(job->high), to_global(job->high_agg), to_global(job->ident),
                       job->ld_low, job->ld_high, job->ld_high_agg, job->ld_ident, job->high_agg != nullptr, (job->flags & WDG_ACM_RELU) != 0};
}
// the three channels of row r at this lane's columns, activation applied
__device__ __forceinline__ void ap_channels(const ap_operands &o, const int r, const int64_t c0, const int real, float (&h)[3][4]) {
    ap_load4(o.low, static_cast<int64_t>(r) * o.ld_low + c0, real, h[0]);
    ap_load4(o.high, static_cast<int64_t>(r) * o.ld_high + c0, real, h[1]);
    ap_load4(o.ident, static_cast<int64_t>(r) * o.ld_ident + c0, real, h[2]);
    if (o.has_agg) {
        float a[4];
        ap_load4(o.agg, static_cast<int64_t>(r) * o.ld_agg + c0, real, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) h[1][k] = h[1][k] - a[k];
    }
    if (o.relu) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int k = 0; k < 4; ++k) h[ch][k] = acm::relu(h[ch][k]);
    }
}

__global__ __launch_bounds__(AP_THREADS) void acm_packed_kernel(const wdg_acm_packed_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_acm_packed_job> job = (desc_ptr<wdg_acm_packed_job>)(jobs + blockIdx.z);
    if (ap_defect(job, false)) return;  // (uniform)
    const int rows = min(job->rows, max_rows), cols = job->cols, stride = job->stride, reps = job->reps;
    const int r0 = blockIdx.x * AP_TILE;
    const int t = threadIdx.x, gq = t & 15, slot = t >> 4;
    const int64_t c0 = static_cast<int64_t>(blockIdx.y) * AP_TILE + 4 * gq;  // this lane's first column of the stacked row
    const int64_t rep = c0 / stride;
    // (no barrier in this kernel, and the lanes a shuffle pairs belong to one replica: a whole replica leaves together)
    if (r0 >= rows || rep >= reps) return;
    const int cr = static_cast<int>(c0 - rep * stride), real = min(max(cols - cr, 0), 4);
    const ap_operands ops = ap_read_operands(job);
    float att[3][4], wm[9];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) ap_load4(to_global(job->att), (rep * 3 + ch) * stride + cr, real, att[ch]);
#pragma unroll
    for (int i = 0; i < 9; ++i) wm[i] = to_global(job->wmix)[rep * 9 + i];
    const global_ptr<float> aux = to_global(job->aux), out = to_global(job->out);
    const int64_t ld_out = job->ld_out;
#pragma unroll
    for (int m = 0; m < AP_ROWS_PER_THREAD; ++m) {
        const int r = r0 + slot + AP_SLOTS * m;
        if (r >= rows) continue;  // (the 16 lanes of a row together)
        float h[3][4], dot[3], s[3], al[3], o[4];
        ap_channels(ops, r, c0, real, h);
#pragma unroll
        for (int c = 0; c < 3; ++c) dot[c] = ap_seg_sum(ap_dot(h[c], att[c]), stride);
        acm::alpha(dot, wm, s, al);
#pragma unroll
        for (int k = 0; k < 4; ++k)  // (a padding column is WRITTEN +0: a NaN alpha does not reach it)
            o[k] = k < real ? acm::mix(al, h[0][k], h[1][k], h[2][k]) : 0.f;
        store_f32x4(out + (static_cast<int64_t>(r) * ld_out + c0), make_float4(o[0], o[1], o[2], o[3]));
        if (cr == 0) {  // aux[r][rep] = alpha_L alpha_H alpha_I s_L s_H s_I 0 0: the replica's first lane
            const global_ptr<float> a = aux + (static_cast<int64_t>(r) * reps + rep) * acm::AUX_WORDS;
            store_f32x4(a, make_float4(al[0], al[1], al[2], s[0]));
            store_f32x4(a + 4, make_float4(s[1], s[2], 0.f, 0.f));
        }
    }
}

__global__ __launch_bounds__(AP_THREADS) void acm_packed_backward_kernel(const wdg_acm_packed_job *__restrict__ jobs, const int max_rows) {
    constexpr int RED = AP_RED_DW + 12 * (AP_TILE / 4);  // (at most 16 replicas in a column block)
    __shared__ __attribute__((aligned(16))) float red[AP_SLOTS][RED];
    const desc_ptr<wdg_acm_packed_job> job = (desc_ptr<wdg_acm_packed_job>)(jobs + blockIdx.z);
    if (ap_defect(job, true)) return;  // (uniform: before any barrier)
    const int rows = min(job->rows, max_rows), cols = job->cols, stride = job->stride, reps = job->reps;
    const int r0 = blockIdx.x * AP_TILE;
    const int64_t cb = static_cast<int64_t>(blockIdx.y) * AP_TILE, width = static_cast<int64_t>(reps) * stride;
    if (r0 >= rows || cb >= width) return;  // (uniform: before any barrier)
    const int t = threadIdx.x, gq = t & 15, slot = t >> 4;
    const int64_t c0 = cb + 4 * gq, rep = c0 / stride;
    const bool live = rep < reps;  // (lanes past the last replica compute on zeros, touch no memory and stay for the barrier)
    const int cr = static_cast<int>(c0 - rep * stride), real = live ? min(max(cols - cr, 0), 4) : 0;
    const ap_operands ops = ap_read_operands(job);
    const global_ptr<const float> dout = to_global(job->d_out), aux = to_global(const_cast<const float *>(job->aux));
    const int64_t ld_dout = job->ld_d_out;
    float att[3][4], wm[9], da[3][4], dw[9];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        att[ch][0] = att[ch][1] = att[ch][2] = att[ch][3] = 0.f;
        da[ch][0] = da[ch][1] = da[ch][2] = da[ch][3] = 0.f;
        if (live) ap_load4(to_global(job->att), (rep * 3 + ch) * stride + cr, real, att[ch]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) wm[i] = live ? to_global(job->wmix)[rep * 9 + i] : 0.f, dw[i] = 0.f;
    const global_ptr<float> d_mat[3] = {to_global(job->d_low), to_global(job->d_high), to_global(job->d_ident)};
    const int64_t d_ld[3] = {job->ld_d_low, job->ld_d_high, job->ld_d_ident};
    if (live) {
#pragma unroll
        for (int m = 0; m < AP_ROWS_PER_THREAD; ++m) {
            const int r = r0 + slot + AP_SLOTS * m;
            if (r >= rows) continue;  // (the 16 lanes of a row together)
            float h[3][4], g[4], al[3], s[3], dal[3], du[3];
            ap_channels(ops, r, c0, real, h);
            ap_load4(dout, static_cast<int64_t>(r) * ld_dout + c0, real, g);
            const global_ptr<const float> a = aux + (static_cast<int64_t>(r) * reps + rep) * acm::AUX_WORDS;
            const float4 a0 = load_f32x4(a), a1 = load_f32x4(a + 4);
            al[0] = a0.x, al[1] = a0.y, al[2] = a0.z, s[0] = a0.w, s[1] = a1.x, s[2] = a1.y;
#pragma unroll
            for (int c = 0; c < 3; ++c) dal[c] = 3.0f * ap_seg_sum(ap_dot(g, h[c]), stride);
            acm::scores_backward(al, s, dal, wm, du, dw);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a3 = 3.0f * al[c];
                float dp[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    dp[k] = acm::input_gradient(a3, g[k], du[c], att[c][k], h[c][k], ops.relu, da[c][k]);
                    if (k >= real) dp[k] = 0.f;  // (a padding column is WRITTEN +0)
                }
                store_f32x4(d_mat[c] + (static_cast<int64_t>(r) * d_ld[c] + c0), make_float4(dp[0], dp[1], dp[2], dp[3]));
            }
        }
    }
    // the 16 row slots' sums, added in slot order
    const int seg = (4 * gq) / stride;  // this lane's replica inside the column block
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[slot][c * AP_TILE + 4 * gq + k] = da[c][k];
    if (cr == 0 || !live) {  // (every lane of a replica holds the same d_wmix terms: its first lane speaks for the slot)
#pragma unroll
        for (int i = 0; i < 12; ++i) red[slot][AP_RED_DW + 12 * seg + i] = i < 9 ? dw[i] : 0.f;
    }
    __syncthreads();
    // one vector of 3 stride + 12 floats per (row block, replica), four floats of it per thread
    const int plen = ap_partial_len(stride), quads = plen / 4, segs = AP_TILE / stride;
    const global_ptr<float> part = to_global(job->partials);
    for (int i = t; i < segs * quads; i += AP_THREADS) {
        const int sg = i / quads, e = 4 * (i - sg * quads);
        const int64_t rp = cb / stride + sg;
        if (rp >= reps) continue;
        const int at = e < 3 * stride ? (e / stride) * AP_TILE + sg * stride + (e % stride) : AP_RED_DW + 12 * sg + (e - 3 * stride);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < AP_SLOTS; ++sl)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] + red[sl][at + k];
        store_f32x4(part + ((static_cast<int64_t>(blockIdx.x) * reps + rp) * plen + e), make_float4(acc[0], acc[1], acc[2], acc[3]));
    }
}

// d_att / d_wmix of a replica = its blocks' partial vectors added in block order; the padding columns of d_att are WRITTEN +0
__global__ __launch_bounds__(AP_THREADS) void acm_packed_reduce_kernel(const wdg_acm_packed_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_acm_packed_job> job = (desc_ptr<wdg_acm_packed_job>)(jobs + blockIdx.y);
    if (ap_defect(job, true)) return;
    const int rows = min(job->rows, max_rows), cols = job->cols, stride = job->stride, reps = job->reps;
    const int plen = ap_partial_len(stride), quads = plen / 4;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * AP_THREADS + threadIdx.x;
    if (i >= static_cast<int64_t>(reps) * quads) return;
    const int64_t rep = i / quads;
    const int e = 4 * static_cast<int>(i - rep * quads);
    const int blocks = (rows + AP_TILE - 1) / AP_TILE;
    const global_ptr<const float> part = to_global(const_cast<const float *>(job->partials));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < blocks; ++b) {
        const float4 p = load_f32x4(part + ((static_cast<int64_t>(b) * reps + rep) * plen + e));
        acc[0] = acc[0] + p.x, acc[1] = acc[1] + p.y, acc[2] = acc[2] + p.z, acc[3] = acc[3] + p.w;
    }
    if (e < 3 * stride) {
        const int cr = e % stride;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cr + k >= cols) acc[k] = 0.f;
        store_f32x4(to_global(job->d_att) + (rep * 3 * stride + e), make_float4(acc[0], acc[1], acc[2], acc[3]));
    } else {
        const global_ptr<float> dw = to_global(job->d_wmix) + rep * 9;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e - 3 * stride + k < 9) dw[e - 3 * stride + k] = acc[k];
    }
}

int ap_check(const char *what, const wdg_acm_packed_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int64_t max_width) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_width >= 0, "%s: negative count", what);
    WDG_REQUIRE(n_jobs <= AP_MAX_JOBS, "%s: %d jobs; one launch takes %d", what, n_jobs, AP_MAX_JOBS);
    WDG_REQUIRE(max_width <= AP_MAX_WIDTH, "%s: %lld columns; one launch takes %lld", what, static_cast<long long>(max_width),
                static_cast<long long>(AP_MAX_WIDTH));
    WDG_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "%s: null job table", what);
    return WDG_OK;
}

}  // namespace

extern "C" int wdg_acm_mix_packed_f32(const wdg_acm_packed_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int64_t max_width, wdg_stream_t stream) {
    if (const int rc = ap_check("acm_mix_packed", jobs_dev, n_jobs, max_rows, max_width)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_width == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, AP_TILE)), static_cast<unsigned>(wdg::ceil_div(max_width, AP_TILE)),
                    static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(acm_packed_kernel, grid, dim3(AP_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("acm_packed_kernel");
}

extern "C" int wdg_acm_mix_packed_backward_f32(const wdg_acm_packed_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int64_t max_width,
                                               wdg_stream_t stream) {
    if (const int rc = ap_check("acm_mix_packed_backward", jobs_dev, n_jobs, max_rows, max_width)) return rc;
    if (n_jobs == 0 || max_width == 0) return WDG_OK;
    if (max_rows > 0) {
        const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, AP_TILE)), static_cast<unsigned>(wdg::ceil_div(max_width, AP_TILE)),
                        static_cast<unsigned>(n_jobs));
        hipLaunchKernelGGL(acm_packed_backward_kernel, grid, dim3(AP_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows);
        if (const int rc = wdg::check_launch("acm_packed_backward_kernel")) return rc;
    }
    // (a replica has 3 stride / 4 + 3 quads of sums: at most 6 per 4 columns of the widest job, at stride 4)
    const int64_t max_quads = wdg::ceil_div(3 * max_width, 2);
    hipLaunchKernelGGL(acm_packed_reduce_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_quads, AP_THREADS)), static_cast<unsigned>(n_jobs)),
                       dim3(AP_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("acm_packed_reduce_kernel");
}

extern "C" int wdg_acm_mix_packed_check_jobs(const wdg_acm_packed_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "acm_mix_packed_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "acm_mix_packed_check_jobs: null job table");
    WDG_REQUIRE(n_jobs <= AP_MAX_JOBS, "acm_mix_packed_check_jobs: %d jobs; one launch takes %d", n_jobs, AP_MAX_JOBS);
    for (int32_t i = 0; i < n_jobs; ++i) {
        const char *defect = ap_defect(jobs_host + i, false);
        WDG_REQUIRE(defect == nullptr, "acm_mix_packed_check_jobs: job %d has %s", i, defect);
    }
    return WDG_OK;
}
