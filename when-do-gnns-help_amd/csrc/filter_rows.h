// What the K-hop filter kernels share (csrc/poly_filter.hip: the monomial basis; csrc/recur_filter.hip: a three-term recurrence): the
// launch's constants, the malformed-job predicate over the members both job records have, a workgroup's view of its job, the extent
// rule, the LDS loads and stores, the load of T_0, the row sum P - the lane chains and the butterfly that include/wdg.h states -, the
// walk that gives every row its owner, the dot products' row blocks, their finishing pass, the host predicate and the two launches.
// A unit states what differs: the hop of one row (its `row<L>` below) and the loop over the hops.  Every unit that includes this is
// compiled with contraction off; every fmaf is written out.
#pragma once
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int PF_THREADS = 1024, PF_TEAM = WDG_POLY_FILTER_TEAM, PF_TEAMS = PF_THREADS / PF_TEAM, PF_AHEAD = 4;
constexpr int PF_LONG = WDG_POLY_FILTER_LONG_ROW, PF_DOT_ROWS = WDG_POLY_FILTER_DOT_ROWS;
constexpr int PF_FIN_THREADS = 256, PF_FIN_AHEAD = 16;
constexpr int PF_MAX_JOBS = 65535;  // gridDim.y: a job per y
static_assert(PF_TEAM >= 4 && 64 % PF_TEAM == 0, "a team has a lane per column of the widest group and lies inside one wave");

__host__ __device__ __forceinline__ int pf_max_rows(const int group_cols) {
    return group_cols == 1 || group_cols == 2 || group_cols == 4 ? WDG_POLY_FILTER_LDS_BYTES / (8 * group_cols) : 0;
}

// what both launches skip and the check_jobs entries refuse (one predicate, over the members every filter job has)
template <typename J>
__host__ __device__ __forceinline__ bool pf_malformed(const J job) {
    const bool has_u = job->u != nullptr, has_dots = job->dots != nullptr;
    if (job->n < 0 || job->nnz < 0 || job->cols < 0 || job->order < 0 || job->order > WDG_POLY_FILTER_MAX_ORDER || job->seg_cols < 1 ||
        job->cols % job->seg_cols != 0 || (has_u != has_dots && job->n > 0 && job->cols > 0) || (has_dots && job->partials == nullptr) || pf_max_rows(job->group_cols) == 0 ||
        job->n > pf_max_rows(job->group_cols))
        return true;
    if (job->cols > 0 && (job->gamma == nullptr || job->ld_gamma < job->cols / job->seg_cols || (has_dots && job->ld_dots < job->cols / job->seg_cols))) return true;
    if (job->n == 0 || job->cols == 0) return false;
    return job->rowptr == nullptr || job->v == nullptr || job->out == nullptr || (job->nnz > 0 && job->col == nullptr) ||
           (job->n > 1 && (job->ld_v < job->cols || job->ld_out < job->cols || (has_u && job->ld_u < job->cols)));
}

// one workgroup's view of its job
struct pf_ctx {
    global_ptr<const int32_t> rowptr, col;
    global_ptr<const float> val, row_scale, col_scale, v, u;
    global_ptr<float> out;
    int64_t ld_v, ld_out, ld_u;
    int n, nnz, c0, live;
    bool has_val, has_rs, has_cs;
};

// the group blockIdx.x of a well-formed job with rows and columns: false where the launch has no such group or its LDS does not hold
// the job (uniform: before any barrier); else the view, and the group's segment
template <typename J>
__device__ __forceinline__ bool pf_bind(const J job, const int max_floats, pf_ctx &c, int &seg) {
    const int gc = job->group_cols, seg_cols = job->seg_cols;
    const int per_seg = (seg_cols + gc - 1) / gc;
    const int64_t groups = static_cast<int64_t>(job->cols / seg_cols) * per_seg;
    if (blockIdx.x >= groups || static_cast<int64_t>(job->n) * gc > max_floats) return false;  // (the LDS of the launch holds 2 * max_floats floats)
    seg = blockIdx.x / per_seg;
    const int gi = blockIdx.x - seg * per_seg;
    c.rowptr = to_global(job->rowptr), c.col = to_global(job->col);
    c.val = to_global(job->val), c.row_scale = to_global(job->row_scale), c.col_scale = to_global(job->col_scale), c.v = to_global(job->v), c.u = to_global(job->u);
    c.out = to_global(job->out);
    c.ld_v = job->ld_v, c.ld_out = job->ld_out, c.ld_u = job->ld_u;
    c.n = job->n, c.nnz = job->nnz, c.c0 = seg * seg_cols + gi * gc, c.live = min(gc, seg_cols - gi * gc);
    c.has_val = job->val != nullptr, c.has_rs = job->row_scale != nullptr, c.has_cs = job->col_scale != nullptr;
    return true;
}

__device__ __forceinline__ void pf_extent(const pf_ctx &c, const int i, int &beg, int &end) {
    beg = c.rowptr[i], end = c.rowptr[i + 1];
    if (beg < 0 || end < beg || end > c.nnz) beg = end = 0;  // (an extent outside the pattern counts as an empty row)
}

template <int W>
__device__ __forceinline__ void pf_lds_load(const float *p, float (&x)[W]) {
    if constexpr (W == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        x[0] = t.x, x[1] = t.y, x[2] = t.z, x[3] = t.w;
    } else if constexpr (W == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        x[0] = t.x, x[1] = t.y;
    } else {
        x[0] = *p;
    }
}

template <int W>
__device__ __forceinline__ void pf_lds_store(float *p, const float (&x)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
    } else if constexpr (W == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(x[0], x[1]);
    } else {
        *p = x[0];
    }
}

// T_0[i, :] = v[i, :] and out[i, :] = gamma_0 * v[i, :], by the lanes that own the row's columns for the rest of the launch
template <int W>
__device__ __forceinline__ void pf_first_row(const pf_ctx &c, float *cur, const int i, const int l, const float g0) {
    if (l < W) {
        float x = 0.f;  // (a column of the image past the group's last one holds +0 and is never stored)
        if (l < c.live) {
            x = c.v[static_cast<int64_t>(i) * c.ld_v + c.c0 + l];
            c.out[static_cast<int64_t>(i) * c.ld_out + c.c0 + l] = g0 * x;
        }
        cur[i * W + l] = x;
    }
}

// the sum of row i over its L lanes, before the product with row_scale[i]: lane l's fmaf chain from +0 over the entries beg + l,
// beg + l + L, ..., then the butterfly over the distances L/2 .. 1 - every lane ends with the same bits (include/wdg.h)
template <int W, int L>
__device__ __forceinline__ void pf_row_sum(const pf_ctx &c, const float *cur, const int beg, const int end, const int l, float (&acc)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.f;
    for (int p = beg + l; p < end; p += PF_AHEAD * L) {
        int jj[PF_AHEAD];
        bool ok[PF_AHEAD];
        float wv[PF_AHEAD], cs[PF_AHEAD], x[PF_AHEAD][W];
#pragma unroll
        for (int a = 0; a < PF_AHEAD; ++a) {  // (an entry past the row's end reads the lane's first one: no branch; it is not used)
            const bool in = p + a * L < end;
            const int at = in ? p + a * L : p;
            const int j = c.col[at];
            wv[a] = c.has_val ? c.val[at] : 1.f;
            ok[a] = in && static_cast<unsigned>(j) < static_cast<unsigned>(c.n);
            jj[a] = ok[a] ? j : 0;
        }
#pragma unroll
        for (int a = 0; a < PF_AHEAD; ++a) cs[a] = wv[a] * (c.has_cs ? c.col_scale[jj[a]] : 1.f);  // (a factor that is not given is 1: the product is exact)
#pragma unroll
        for (int a = 0; a < PF_AHEAD; ++a) pf_lds_load<W>(cur + jj[a] * W, x[a]);
#pragma unroll
        for (int a = 0; a < PF_AHEAD; ++a)
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] = ok[a] ? fmaf(cs[a], x[a][k], acc[k]) : acc[k];
    }
#pragma unroll
    for (int d = L / 2; d >= 1; d >>= 1)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], d);
}

// every row of the job by its owner: FIRST - the load of T_0 -, or one hop, hop.row<L>(i, beg, end, l) by the row's L lanes
template <int W, bool FIRST, typename HOP>
__device__ __forceinline__ void pf_walk(const pf_ctx &c, float *cur, const float g0, const HOP &hop) {
    const int t = threadIdx.x, team = t / PF_TEAM, l = t % PF_TEAM, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    {  // rows of at most PF_LONG entries: team i mod PF_TEAMS; the next row's extent is requested before this row's work
        int i = team, beg = 0, end = 0;
        if (i < c.n) beg = c.rowptr[i], end = c.rowptr[i + 1];
        while (i < c.n) {
            const int i_next = i + PF_TEAMS;
            int beg_next = 0, end_next = 0;
            if (i_next < c.n) beg_next = c.rowptr[i_next], end_next = c.rowptr[i_next + 1];  // (looked at one row later: the loads stay in flight)
            if (beg < 0 || end < beg || end > c.nnz) beg = end = 0;  // (pf_extent's rule)
            if (end - beg <= PF_LONG) {  // (uniform in the team)
                if constexpr (FIRST)
                    pf_first_row<W>(c, cur, i, l, g0);
                else
                    hop.template row<PF_TEAM>(i, beg, end, l);
            }
            i = i_next, beg = beg_next, end = end_next;
        }
    }
    // longer rows: the wave (i / 64) mod 16 - every wave looks at the lengths of its blocks of 64 rows, a lane per row
    for (int base = wave * 64; base < c.n; base += PF_THREADS) {
        int beg = 0, end = 0;
        if (base + lane < c.n) pf_extent(c, base + lane, beg, end);
        unsigned long long todo = __ballot(end - beg > PF_LONG);
        while (todo) {  // (wave-uniform)
            const int i = base + __builtin_ctzll(todo);
            todo &= todo - 1;
            if constexpr (FIRST) {
                pf_first_row<W>(c, cur, i, lane, g0);
            } else {
                int b, e;
                pf_extent(c, i, b, e);
                hop.template row<64>(i, b, e, lane);
            }
        }
    }
}

struct pf_no_hop {};  // (the FIRST walk calls no hop)

// the partials of dots[k, .]: one thread per (block of PF_DOT_ROWS rows, column of the group) walks the block's rows in ascending order
template <int W>
__device__ __forceinline__ void pf_dot_blocks(const pf_ctx &c, const float *cur, const global_ptr<double> partials, const int cols, const int k) {
    const int blocks = (c.n + PF_DOT_ROWS - 1) / PF_DOT_ROWS;
    for (int q = threadIdx.x; q < blocks * c.live; q += PF_THREADS) {
        const int b = q / c.live, k_col = q - b * c.live;
        const int r0 = b * PF_DOT_ROWS, r1 = min(c.n, r0 + PF_DOT_ROWS);
        const global_ptr<const float> u = c.u + c.c0 + k_col;
        double s = 0.0;
        for (int r = r0; r < r1; ++r) s = s + static_cast<double>(cur[r * W + k_col]) * static_cast<double>(u[static_cast<int64_t>(r) * c.ld_u]);
        partials[(static_cast<int64_t>(k) * cols + c.c0 + k_col) * blocks + b] = s;
    }
}

// after every group has left its partials: a workgroup per (k, job).  A thread per column adds the column's blocks in ascending order
// - the loads of PF_FIN_AHEAD blocks are in flight together, the adds stay in order - and leaves the column's total behind the block
// partials; then a thread per segment adds the segment's columns in ascending order and rounds once.
template <typename J>
__device__ __forceinline__ void pf_finish_dots(const J job) {
    const int k = blockIdx.x;
    if (pf_malformed(job) || job->dots == nullptr || k > job->order || job->cols == 0) return;  // (uniform: before the barrier)
    const int n = job->n, cols = job->cols, seg_cols = job->seg_cols;
    const int blocks = (n + PF_DOT_ROWS - 1) / PF_DOT_ROWS;
    const global_ptr<double> partials = to_global(job->partials);
    const global_ptr<double> totals = partials + static_cast<int64_t>(job->order + 1) * cols * blocks + static_cast<int64_t>(k) * cols;
    for (int col = threadIdx.x; col < cols; col += PF_FIN_THREADS) {
        const global_ptr<const double> mine = partials + (static_cast<int64_t>(k) * cols + col) * blocks;
        double s = 0.0;
        for (int b0 = 0; b0 < blocks; b0 += PF_FIN_AHEAD) {
            double x[PF_FIN_AHEAD];
#pragma unroll
            for (int a = 0; a < PF_FIN_AHEAD; ++a) x[a] = b0 + a < blocks ? mine[b0 + a] : 0.0;
#pragma unroll
            for (int a = 0; a < PF_FIN_AHEAD; ++a)
                if (b0 + a < blocks) s = s + x[a];
        }
        __hip_atomic_store(totals + col, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (read back by another thread of the workgroup: past its L1)
    }
    __threadfence();
    __syncthreads();
    const global_ptr<float> dots = to_global(job->dots) + static_cast<int64_t>(k) * job->ld_dots;
    for (int seg = threadIdx.x; seg < cols / seg_cols; seg += PF_FIN_THREADS) {
        double s = 0.0;
        for (int col = seg * seg_cols; col < (seg + 1) * seg_cols; ++col) s = s + __hip_atomic_load(totals + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dots[seg] = static_cast<float>(s);
    }
}

// The per-job part of the contract over the members every filter job has, on the table the caller still holds on the host; `what`
// names the entry in the messages.  WDG_OK: the unit goes on with what its own record adds.
template <typename J>
inline int pf_check_job(const char *what, const J &j, const int32_t i) {
    WDG_REQUIRE(j.n >= 0 && j.nnz >= 0 && j.cols >= 0, "%s: job %d has a negative shape", what, i);
    WDG_REQUIRE(j.order >= 0 && j.order <= WDG_POLY_FILTER_MAX_ORDER, "%s: job %d has order %d; the kernel runs 0..%d hops", what, i, j.order, WDG_POLY_FILTER_MAX_ORDER);
    WDG_REQUIRE(j.seg_cols >= 1 && j.cols % j.seg_cols == 0, "%s: job %d has %d columns in segments of %d; a multiple expected", what, i, j.cols, j.seg_cols);
    // (an empty u has no address: a job of no rows or no columns is asked for neither)
    WDG_REQUIRE((j.u != nullptr) == (j.dots != nullptr) || j.n == 0 || j.cols == 0, "%s: job %d has u without dots or dots without u", what, i);
    WDG_REQUIRE(j.dots == nullptr || j.partials != nullptr, "%s: job %d has dots without the workspace of their partial sums", what, i);
    WDG_REQUIRE(pf_max_rows(j.group_cols) > 0, "%s: job %d has group_cols %d; 1, 2 or 4 expected", what, i, j.group_cols);
    if (j.n > pf_max_rows(j.group_cols))
        return wdg::fail(WDG_ERR_UNSUPPORTED, "%s: job %d has %d rows; %d columns of at most %d rows fit twice in a workgroup's LDS", what, i, j.n, j.group_cols,
                         pf_max_rows(j.group_cols));
    WDG_REQUIRE(j.cols == 0 || j.gamma != nullptr, "%s: job %d has a null gamma", what, i);
    WDG_REQUIRE(j.cols == 0 || (j.ld_gamma >= j.cols / j.seg_cols && (j.dots == nullptr || j.ld_dots >= j.cols / j.seg_cols)),
                "%s: job %d has a gamma or dots whose leading dimension lies below its %d segments", what, i, j.cols / j.seg_cols);
    if (j.n == 0 || j.cols == 0) return WDG_OK;
    WDG_REQUIRE(j.rowptr && j.v && j.out, "%s: job %d has a null rowptr, v or out", what, i);
    WDG_REQUIRE(j.nnz == 0 || j.col, "%s: job %d has a null col", what, i);
    WDG_REQUIRE(j.n == 1 || (j.ld_v >= j.cols && j.ld_out >= j.cols && (j.u == nullptr || j.ld_u >= j.cols)), "%s: job %d has a leading dimension below its row", what, i);
    WDG_REQUIRE(!pf_malformed(&j), "%s: job %d is malformed", what, i);
    return WDG_OK;
}

// the filter's launch and, with max_dot_rows != 0, the finishing one (include/wdg.h lists the refusals)
template <typename J>
inline int pf_launch(const char *what, void (*filter)(const J *, int), void (*finish)(const J *), const J *jobs_dev, const int32_t n_jobs, const int32_t max_groups,
                     const int32_t max_floats, const int32_t max_dot_rows, wdg_stream_t stream) {
    WDG_REQUIRE(max_groups >= 0 && max_floats >= 0 && max_dot_rows >= 0, "%s: negative count", what);
    if (const int rc = wdg::check_job_table(what, jobs_dev, n_jobs, PF_MAX_JOBS)) return rc;
    WDG_REQUIRE(max_dot_rows <= WDG_POLY_FILTER_MAX_ORDER + 1, "%s: %d rows of dots; an order has at most %d", what, max_dot_rows, WDG_POLY_FILTER_MAX_ORDER + 1);
    WDG_REQUIRE(static_cast<int64_t>(max_floats) * 8 <= WDG_POLY_FILTER_LDS_BYTES, "%s: %d floats per image; two of them must fit in %d bytes of LDS", what, max_floats,
                WDG_POLY_FILTER_LDS_BYTES);
    if (n_jobs == 0) return WDG_OK;
    const hipStream_t st = wdg::as_stream(stream);
    if (max_groups > 0 && max_floats > 0) {
        static thread_local int configured_dev = -1;  // (per J: a unit's own kernel)
        if (configured_dev != wdg::current_device()) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(filter), hipFuncAttributeMaxDynamicSharedMemorySize, WDG_POLY_FILTER_LDS_BYTES) != hipSuccess)
                return wdg::fail(WDG_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", what);
            configured_dev = wdg::current_device();
        }
        const size_t lds = (static_cast<size_t>(max_floats) * 8 + 15) / 16 * 16;
        const dim3 grid(static_cast<unsigned>(max_groups), static_cast<unsigned>(n_jobs));
        hipLaunchKernelGGL(filter, grid, dim3(PF_THREADS), lds, st, jobs_dev, max_floats);
        if (const int rc = wdg::check_launch(what)) return rc;
    }
    if (max_dot_rows > 0) {
        hipLaunchKernelGGL(finish, dim3(static_cast<unsigned>(max_dot_rows), static_cast<unsigned>(n_jobs)), dim3(PF_FIN_THREADS), 0, st, jobs_dev);
        return wdg::check_launch(what);
    }
    return WDG_OK;
}

}  // namespace
