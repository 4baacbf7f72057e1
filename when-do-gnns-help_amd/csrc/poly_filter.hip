// A polynomial graph filter of many graphs in one launch (the propagation of GPR-GNN, Chien et al., "Adaptive Universal Generalized
// PageRank Graph Neural Network"; APPNP with frozen coefficients): out = sum_k gamma_k A_hat^k v at class width, and optionally the
// K + 1 dot products <A_hat^k v, u> - which, on the transposed pattern, are the gradient of the coefficients.  include/wdg.h states
// the arithmetic and every sum's order; tests/_poly_filter_ref.py restates it in numpy.
//
// replaces: the ONE fixed aggregation of normalize_tensor, utils/util_funcs.py:365-381, behind the SGC / GCN tables of
//           gnns_on_syn.py:1-154, by K of them with a learnt weight per hop; the reference ships no model code, so the filter is
//           defined by this project.
//
// Shape: a workgroup of 1024 threads owns up to group_cols columns of ONE segment of one job and runs ALL hops: T_k and T_{k+1} of its
// columns are two [n, W] images in LDS that swap after every hop's barrier; there is no grid-wide synchronisation.  Rows are owned for
// the whole launch: row i of at most PF_LONG entries by the team of 4 lanes i mod 256 - a row is a chain of dependent loads, so the rows in
// flight, not the lanes, set the pace of a graph of short rows -, a longer row by the wave (i / 64) mod 16 - so a hub row of squirrel's
// ~1 900 entries costs its wave 30 steps and no team 475.  The owner's lane c keeps out[i, c0 + c] where it lives:
// one thread reads and writes an element on every hop, no other touches it.  The dot products' row blocks are walked by one thread per
// (block, column) in the same barrier interval as the hop that reads the same T_k; their fp64 partials go to the job's workspace and a
// second small launch adds them in order.  No floating-point atomic; contraction is off for the unit and every fmaf is written out.
// Every row's loads - the next row's extent, the scale, the old out, four entries' indices, scales and LDS gathers - are issued before
// the row's first store (the job's pointers come out of a table and may alias for all the compiler knows).
#include "filter_rows.h"  // the launch's constants, the predicate, the context, the row sum, the walk, the dot blocks, the launches: shared with recur_filter.hip

namespace {

// one hop of row i by its L lanes: include/wdg.h states the chain, the butterfly and the two products
template <int W>
struct pf_hop {
    const pf_ctx &c;
    const float *cur;
    float *nxt;
    float gk;
    template <int L>
    __device__ __forceinline__ void row(const int i, const int beg, const int end, const int l) const {
        const float rs = c.has_rs ? c.row_scale[i] : 1.f;
        const bool keeps = l < c.live;
        const global_ptr<float> mine = c.out + static_cast<int64_t>(i) * c.ld_out + c.c0 + (keeps ? l : 0);
        const float old = keeps ? *mine : 0.f;
        float acc[W];
        pf_row_sum<W, L>(c, cur, beg, end, l, acc);
        float t[W];
#pragma unroll
        for (int k = 0; k < W; ++k) t[k] = rs * acc[k];
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
__device__ __forceinline__ void pf_run(const desc_ptr<wdg_poly_filter_job> job, const pf_ctx &c, const int seg, float *lds) {
    const int order = job->order, cols = job->cols;
    const global_ptr<const float> gamma = to_global(job->gamma) + seg;
    const int64_t ld_gamma = job->ld_gamma;
    const global_ptr<double> partials = to_global(job->partials);
    const bool dots = job->dots != nullptr;  // (uniform)
    float *cur = lds, *nxt = lds + static_cast<size_t>(c.n) * W;
    pf_walk<W, true>(c, cur, gamma[0], pf_no_hop{});
    __syncthreads();
    for (int k = 0; k < order; ++k) {
        if (dots) pf_dot_blocks<W>(c, cur, partials, cols, k);
        pf_walk<W, false>(c, cur, 0.f, pf_hop<W>{c, cur, nxt, gamma[(k + 1) * ld_gamma]});
        __syncthreads();
        float *const swap = cur;
        cur = nxt, nxt = swap;
    }
    if (dots) pf_dot_blocks<W>(c, cur, partials, cols, order);
}

__global__ __launch_bounds__(PF_THREADS) void poly_filter_kernel(const wdg_poly_filter_job *__restrict__ jobs, const int max_floats) {
    extern __shared__ __attribute__((aligned(16))) float pf_lds[];
    const desc_ptr<wdg_poly_filter_job> job = (desc_ptr<wdg_poly_filter_job>)(jobs + blockIdx.y);
    // (uniform: before any barrier)
    if (pf_malformed(job) || job->n == 0 || job->cols == 0) return;
    pf_ctx c;
    int seg;
    if (!pf_bind(job, max_floats, c, seg)) return;
    if (c.live == 1)
        pf_run<1>(job, c, seg, pf_lds);
    else if (c.live == 2)
        pf_run<2>(job, c, seg, pf_lds);
    else
        pf_run<4>(job, c, seg, pf_lds);
}

__global__ __launch_bounds__(PF_FIN_THREADS) void poly_filter_dots_kernel(const wdg_poly_filter_job *__restrict__ jobs) {
    pf_finish_dots((desc_ptr<wdg_poly_filter_job>)(jobs + blockIdx.y));
}

}  // namespace

extern "C" int32_t wdg_poly_filter_max_rows(int32_t group_cols) { return pf_max_rows(group_cols); }

extern "C" int64_t wdg_poly_filter_partials_len(int32_t n, int32_t cols, int32_t order) {
    if (n < 0 || cols < 0 || order < 0) return 0;
    return static_cast<int64_t>(order + 1) * cols * (wdg::ceil_div(n, PF_DOT_ROWS) + 1);
}

// The per-job part of the contract, on the table the caller still holds on the host (train.PolyFilterBatch calls this before it uploads).
extern "C" int wdg_poly_filter_check_jobs(const wdg_poly_filter_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("poly_filter_check_jobs", jobs_host, n_jobs, PF_MAX_JOBS)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i)
        if (const int rc = pf_check_job("poly_filter_check_jobs", jobs_host[i], i)) return rc;
    return WDG_OK;
}

extern "C" int wdg_poly_filter_batched_f32(const wdg_poly_filter_job *jobs_dev, int32_t n_jobs, int32_t max_groups, int32_t max_floats, int32_t max_dot_rows,
                                           wdg_stream_t stream) {
    return pf_launch("poly_filter_batched", poly_filter_kernel, poly_filter_dots_kernel, jobs_dev, n_jobs, max_groups, max_floats, max_dot_rows, stream);
}
