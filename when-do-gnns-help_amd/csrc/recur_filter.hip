// A graph filter in a basis of orthogonal polynomials, of many graphs in one launch (the propagation of ChebNet / ChebNetII - He, Wei,
// Wen, "Convolutional Neural Networks on Graphs with Chebyshev Approximation, Revisited" - and of JacobiConv - Wang, Zhang, "How
// Powerful are Spectral Graph Neural Networks"): out = sum_k gamma_k T_k with T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1}, the
// three-term recurrence every such basis obeys, and optionally the K + 1 dot products <T_k, u> - which, on the transposed pattern, are
// the gradient of the coefficients.  include/wdg.h states the arithmetic and every sum's order; tests/_recur_filter_ref.py restates it.
//
// replaces: the ONE fixed aggregation of normalize_tensor, utils/util_funcs.py:365-381, behind the SGC / GCN tables of
//           gnns_on_syn.py:1-154, by K of them combined through a three-term recurrence with a learnt weight per basis polynomial; the
//           reference ships no model code, so the filter is defined by this project.
//
// Shape: csrc/poly_filter.hip's - a workgroup of 1024 threads owns up to group_cols columns of ONE segment of one job and runs ALL
// hops over two [n, W] images in LDS that swap after every hop's barrier; rows are owned for the whole launch by a team of 4 lanes or,
// past PF_LONG entries, by a wave; csrc/filter_rows.h holds what the two units share.  What differs is one row's hop: during hop k the
// image that is about to take T_{k+1} still holds T_{k-1}, and row i of it is read and written by the row's owner alone - so the
// owner reads T_k[i, :] and T_{k-1}[i, :] with the row's other loads, before its first store, and writes T_{k+1}[i, :] over
// T_{k-1}[i, :]: the recurrence costs no LDS beyond the monomial filter's and the row limits are the same.
// No floating-point atomic; contraction is off for the unit and every fmaf is written out.
#include "filter_rows.h"

namespace {

template <typename J>
__host__ __device__ __forceinline__ bool rf_malformed(const J job) {
    return pf_malformed(job) || (job->order > 0 && (job->recur == nullptr || job->ld_recur < 3));
}

// one hop of row i by its L lanes: include/wdg.h states the row sum, the two products and the recurrence's fmafs
template <int W>
struct rf_hop {
    const pf_ctx &c;
    const float *cur;
    float *nxt;
    float gk, a, b, cc;
    bool first;  // hop 0: T_1 = fmaf(a_0, P, b_0 * T_0) - the image behind nxt holds nothing yet and c_0 is not read
    template <int L>
    __device__ __forceinline__ void row(const int i, const int beg, const int end, const int l) const {
        const float rs = c.has_rs ? c.row_scale[i] : 1.f;
        const bool keeps = l < c.live;
        const global_ptr<float> mine = c.out + static_cast<int64_t>(i) * c.ld_out + c.c0 + (keeps ? l : 0);
        const float old = keeps ? *mine : 0.f;
        float tk[W], tp[W];  // T_k[i, :] and T_{k-1}[i, :]: every lane of the owner reads them (one address: a broadcast)
        pf_lds_load<W>(cur + i * W, tk);
        pf_lds_load<W>(nxt + i * W, tp);
        float acc[W];
        pf_row_sum<W, L>(c, cur, beg, end, l, acc);
        float t[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float tail = first ? b * tk[k] : fmaf(b, tk[k], cc * tp[k]);  // (a select on values: what hop 0 finds behind nxt is dropped)
            t[k] = fmaf(a, rs * acc[k], tail);
        }
        if (l == 0) pf_lds_store<W>(nxt + i * W, t);
        if (keeps) {
            float own = t[0];  // t[l], by compile-time indices
#pragma unroll
            for (int k = 1; k < W; ++k) own = l == k ? t[k] : own;
            *mine = fmaf(gk, own, old);
        }
    }
};

template <int W>
__device__ __forceinline__ void rf_run(const desc_ptr<wdg_recur_filter_job> job, const pf_ctx &c, const int seg, float *lds) {
    const int order = job->order, cols = job->cols;
    const global_ptr<const float> gamma = to_global(job->gamma) + seg, recur = to_global(job->recur);
    const int64_t ld_gamma = job->ld_gamma, ld_recur = job->ld_recur;
    const global_ptr<double> partials = to_global(job->partials);
    const bool dots = job->dots != nullptr;  // (uniform)
    float *cur = lds, *nxt = lds + static_cast<size_t>(c.n) * W;
    pf_walk<W, true>(c, cur, gamma[0], pf_no_hop{});
    __syncthreads();
    for (int k = 0; k < order; ++k) {
        const global_ptr<const float> abc = recur + k * ld_recur;
        if (dots) pf_dot_blocks<W>(c, cur, partials, cols, k);
        pf_walk<W, false>(c, cur, 0.f, rf_hop<W>{c, cur, nxt, gamma[(k + 1) * ld_gamma], abc[0], abc[1], k == 0 ? 0.f : abc[2], k == 0});
        __syncthreads();
        float *const swap = cur;
        cur = nxt, nxt = swap;
    }
    if (dots) pf_dot_blocks<W>(c, cur, partials, cols, order);
}

__global__ __launch_bounds__(PF_THREADS) void recur_filter_kernel(const wdg_recur_filter_job *__restrict__ jobs, const int max_floats) {
    extern __shared__ __attribute__((aligned(16))) float rf_lds[];
    const desc_ptr<wdg_recur_filter_job> job = (desc_ptr<wdg_recur_filter_job>)(jobs + blockIdx.y);
    // (uniform: before any barrier)
    if (rf_malformed(job) || job->n == 0 || job->cols == 0) return;
    pf_ctx c;
    int seg;
    if (!pf_bind(job, max_floats, c, seg)) return;
    if (c.live == 1)
        rf_run<1>(job, c, seg, rf_lds);
    else if (c.live == 2)
        rf_run<2>(job, c, seg, rf_lds);
    else
        rf_run<4>(job, c, seg, rf_lds);
}

__global__ __launch_bounds__(PF_FIN_THREADS) void recur_filter_dots_kernel(const wdg_recur_filter_job *__restrict__ jobs) {
    const desc_ptr<wdg_recur_filter_job> job = (desc_ptr<wdg_recur_filter_job>)(jobs + blockIdx.y);
    if (rf_malformed(job)) return;  // (uniform: a job the filter's launch skipped has no partials to add)
    pf_finish_dots(job);
}

}  // namespace

// The per-job part of the contract, on the table the caller still holds on the host (train.RecurFilterBatch calls this before it uploads).
extern "C" int wdg_recur_filter_check_jobs(const wdg_recur_filter_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("recur_filter_check_jobs", jobs_host, n_jobs, PF_MAX_JOBS)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_recur_filter_job &j = jobs_host[i];
        if (const int rc = pf_check_job("recur_filter_check_jobs", j, i)) return rc;
        WDG_REQUIRE(j.order == 0 || j.recur != nullptr, "recur_filter_check_jobs: job %d has order %d and a null recurrence table", i, j.order);
        WDG_REQUIRE(j.order == 0 || j.ld_recur >= 3, "recur_filter_check_jobs: job %d has a recurrence table of leading dimension %lld; rows of (a, b, c) expected", i,
                    static_cast<long long>(j.ld_recur));
    }
    return WDG_OK;
}

extern "C" int wdg_recur_filter_batched_f32(const wdg_recur_filter_job *jobs_dev, int32_t n_jobs, int32_t max_groups, int32_t max_floats, int32_t max_dot_rows,
                                            wdg_stream_t stream) {
    return pf_launch("recur_filter_batched", recur_filter_kernel, recur_filter_dots_kernel, jobs_dev, n_jobs, max_groups, max_floats, max_dot_rows, stream);
}
