// The attention scores of many stacked layers in one launch - S = H blockdiag(a_dst, a_src) without the operand - and their backward
// pass: d_H += d_S blockdiag^T, d_att = the block-diagonal part of H^T d_S, summed in a stated order.  include/wdg.h states the column
// layout, the arithmetic and every sum's order; tests/_gat_scores_ref.py restates both passes in numpy.
//
// replaces: the product that forms the scores of the attention layer (csrc/gat.hip; normalize_tensor, utils/util_funcs.py:365-381, is
//           what that layer stands in for) for all replicas of a stacked run: of the operand [R heads w, 2 R heads] one part in R
//           is not zero, and its gradient on the GEMM needs a transposed copy of H.
//
// Shape: both passes read H once and are bound by that read.
//   forward   a THREAD per (row, group): the chain over the group's w columns is the thread's own.  Neighbouring lanes hold neighbouring
//             groups of one row - their w-float pieces of H are contiguous -, a workgroup of 256 threads is [256 / lg rows] x [lg groups]
//             (lg = 64, or the power of two that holds a smaller G) and walks its WDG_GAT_SCORES_ROW_BLOCK rows in passes.  A thread keeps
//             its group for all its rows: for w <= 16 both attention vectors of the group are loaded ONCE, into registers; a wider
//             group reads them with H, four columns at a time (they stay in the CU's cache: every row of the workgroup reads the same).
//   backward  a thread per FOUR consecutive columns of H and a block of WDG_GAT_SCORES_ROW_BLOCK rows: it walks the rows in order, four
//             rows' loads (H, d_H, the two scores) in flight before the first fmaf, adds into d_H and carries the two partial sums of
//             its columns, which go to the workspace; a second launch adds the blocks' sums in order.  No atomics.
// 16-byte accesses are the JOB's decision (every pointer and leading dimension of the pass and w: multiples of 16 bytes / 4), so no
// per-lane branch sits between a load and its use.
#include <cstdint>

#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // every fused multiply-add of the definition is written as fmaf; nothing else may be fused

namespace {

using namespace wdg;

constexpr int GS_THREADS = 256;
constexpr int GS_ROWS = WDG_GAT_SCORES_ROW_BLOCK;  // rows per workgroup of either pass; the backward pass's block of partial sums
constexpr int GS_REG_W = 16;                       // the widest group whose attention vectors a forward thread keeps in registers
constexpr int GS_DEPTH = 4;                        // backward: rows whose loads are in flight together (a divisor of GS_ROWS)
static_assert(GS_ROWS % GS_DEPTH == 0, "a block of rows is a whole number of batches");

__device__ __forceinline__ bool gs_in_limits(const int n, const int G, const int w, const int heads) {
    return n > 0 && G > 0 && heads >= 1 && heads <= WDG_GAT_SCORES_MAX_HEADS && w >= 1 && w <= WDG_GAT_SCORES_MAX_W &&
           static_cast<int64_t>(G) * w <= INT32_MAX;
}
// the score column of group g's dst score; *hb = the groups of its block (the src score is *hb columns further)
__device__ __forceinline__ int gs_dst_column(const int g, const int G, const int heads, int *hb) {
    const int b = g / heads;
    *hb = min(heads, G - b * heads);
    return 2 * heads * b + (g - b * heads);
}

// ---------------------------------------------------------------------------------------------------------------- forward
// One (row, group) of a narrow group: a_d, a_s are the thread's registers (elements >= w are never used).
template <bool VEC>
__device__ __forceinline__ void gs_forward_narrow(const global_ptr<const float> h, const int w, const float (&a_d)[GS_REG_W],
                                                  const float (&a_s)[GS_REG_W], float &s_d, float &s_s) {
    float x[GS_REG_W];
    if (VEC) {
#pragma unroll
        for (int q = 0; q < GS_REG_W / 4; ++q)
            if (4 * q < w) {  // (uniform: w is the job's, and a multiple of 4 here)
                const float4 v = load_f32x4(h + 4 * q);
                x[4 * q] = v.x, x[4 * q + 1] = v.y, x[4 * q + 2] = v.z, x[4 * q + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int k = 0; k < GS_REG_W; ++k)
            if (k < w) x[k] = h[k];
    }
    float d = 0.f, s = 0.f;
#pragma unroll
    for (int k = 0; k < GS_REG_W; ++k)
        if (k < w) {
            d = fmaf(x[k], a_d[k], d);
            s = fmaf(x[k], a_s[k], s);
        }
    s_d = d, s_s = s;
}

template <bool VEC>
__device__ __forceinline__ void gs_forward_job(const desc_ptr<wdg_gat_scores_job> j, const int n, const int G, const int w, const int heads) {
    // the workgroup's tile: lg groups x (256 / lg) rows per pass
    int lg = 64;
    while (lg > 1 && (lg >> 1) >= G) lg >>= 1;
    const int t = static_cast<int>(threadIdx.x);
    const int g = static_cast<int>(blockIdx.y) * lg + (t & (lg - 1));
    const int r_local = t / lg, rows_per_pass = GS_THREADS / lg;
    const int r0 = static_cast<int>(blockIdx.x) * GS_ROWS, r1 = min(n, r0 + GS_ROWS);
    if (g >= G || r0 + r_local >= r1) return;
    const global_ptr<const float> H = to_global(j->H) + static_cast<int64_t>(g) * w;
    const global_ptr<const float> a_dst = to_global(j->att) + static_cast<int64_t>(g) * w, a_src = a_dst + j->ld_att;
    const global_ptr<float> S = to_global(j->S);
    const int64_t ld_h = j->ld_h, ld_s = j->ld_s;
    int hb;
    const int c_dst = gs_dst_column(g, G, heads, &hb), c_src = c_dst + hb;
    if (w <= GS_REG_W) {
        float a_d[GS_REG_W], a_s[GS_REG_W];
#pragma unroll
        for (int k = 0; k < GS_REG_W; ++k) {
            a_d[k] = a_dst[min(k, w - 1)];
            a_s[k] = a_src[min(k, w - 1)];
        }
        for (int r = r0 + r_local; r < r1; r += rows_per_pass) {
            float s_d, s_s;
            gs_forward_narrow<VEC>(H + r * ld_h, w, a_d, a_s, s_d, s_s);
            S[r * ld_s + c_dst] = s_d;
            S[r * ld_s + c_src] = s_s;
        }
        return;
    }
    for (int r = r0 + r_local; r < r1; r += rows_per_pass) {
        const global_ptr<const float> h = H + r * ld_h;
        float d = 0.f, s = 0.f;
        if (VEC) {
#pragma unroll 4
            for (int k = 0; k < w; k += 4) {
                const float4 x = load_f32x4(h + k), ad = load_f32x4(a_dst + k), as = load_f32x4(a_src + k);
                d = fmaf(x.w, ad.w, fmaf(x.z, ad.z, fmaf(x.y, ad.y, fmaf(x.x, ad.x, d))));
                s = fmaf(x.w, as.w, fmaf(x.z, as.z, fmaf(x.y, as.y, fmaf(x.x, as.x, s))));
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < w; ++k) {
                const float x = h[k];
                d = fmaf(x, a_dst[k], d);
                s = fmaf(x, a_src[k], s);
            }
        }
        S[r * ld_s + c_dst] = d;
        S[r * ld_s + c_src] = s;
    }
}

__global__ __launch_bounds__(GS_THREADS) void gat_scores_forward_kernel(const wdg_gat_scores_job *__restrict__ jobs) {
    const desc_ptr<wdg_gat_scores_job> j = (desc_ptr<wdg_gat_scores_job>)(jobs + blockIdx.z);
    const int n = j->n, G = j->G, w = j->w, heads = j->heads;
    if (!gs_in_limits(n, G, w, heads) || !j->H || !j->S || !j->att) return;
    if (static_cast<int64_t>(blockIdx.x) * GS_ROWS >= n) return;
    const bool vec = (w & 3) == 0 && aligned16(j->H, j->ld_h) && aligned16(j->att, j->ld_att);
    if (vec)
        gs_forward_job<true>(j, n, G, w, heads);
    else
        gs_forward_job<false>(j, n, G, w, heads);
}

// --------------------------------------------------------------------------------------------------------------- backward
// VEC: w is a multiple of 4, so the thread's four columns lie in ONE group and read one pair of scores per row; else every column has
// its own pair.
template <bool VEC>
__device__ __forceinline__ void gs_backward_job(const desc_ptr<wdg_gat_scores_job> j, const int n, const int G, const int w, const int heads) {
    constexpr int NS = VEC ? 1 : 4;  // the pairs of scores a thread reads per row
    const int64_t cols = static_cast<int64_t>(G) * w;
    const int64_t c0 = (static_cast<int64_t>(blockIdx.y) * GS_THREADS + threadIdx.x) * 4;
    if (c0 >= cols) return;
    const int live = static_cast<int>(min(static_cast<int64_t>(4), cols - c0));
    const int r0 = static_cast<int>(blockIdx.x) * GS_ROWS, r1 = min(n, r0 + GS_ROWS);
    int c_dst[NS], c_src[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        int hb;
        c_dst[k] = gs_dst_column(static_cast<int>((c0 + min(k, live - 1)) / w), G, heads, &hb);
        c_src[k] = c_dst[k] + hb;
    }
    const global_ptr<const float> H = to_global(j->H) + c0, d_S = to_global(j->d_S), att = to_global(j->att) + c0;
    const global_ptr<float> d_H = to_global(j->d_H) + c0;
    const int64_t ld_h = j->ld_h, ld_d_h = j->ld_d_h, ld_d_s = j->ld_d_s;
    float a_d[4], a_s[4], acc_d[4] = {0.f, 0.f, 0.f, 0.f}, acc_s[4] = {0.f, 0.f, 0.f, 0.f};
    load4<VEC>(att, live, a_d);
    load4<VEC>(att + j->ld_att, live, a_s);
    for (int r = r0; r < r1; r += GS_DEPTH) {
        float x[GS_DEPTH][4], dh[GS_DEPTH][4], sd[GS_DEPTH][NS], ss[GS_DEPTH][NS];
#pragma unroll
        for (int u = 0; u < GS_DEPTH; ++u) {  // all the loads of the batch (a row past the block's end: the last one again, not used)
            const int64_t row = min(r + u, r1 - 1);
            load4<VEC>(H + row * ld_h, live, x[u]);
            load4<VEC>(d_H + row * ld_d_h, live, dh[u]);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                sd[u][k] = d_S[row * ld_d_s + c_dst[k]];
                ss[u][k] = d_S[row * ld_d_s + c_src[k]];
            }
        }
#pragma unroll
        for (int u = 0; u < GS_DEPTH; ++u) {
            if (r + u >= r1) break;
            float out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = sd[u][VEC ? 0 : k], s = ss[u][VEC ? 0 : k];
                acc_d[k] = fmaf(d, x[u][k], acc_d[k]);
                acc_s[k] = fmaf(s, x[u][k], acc_s[k]);
                out[k] = fmaf(s, a_s[k], fmaf(d, a_d[k], dh[u][k]));
            }
            store4<VEC>(d_H + (r + u) * ld_d_h, live, out);
        }
    }
    const global_ptr<float> part = to_global(j->partial) + static_cast<int64_t>(blockIdx.x) * 2 * cols + c0;
    store4<VEC>(part, live, acc_d);
    store4<VEC>(part + cols, live, acc_s);
}

__device__ __forceinline__ bool gs_has_backward(const desc_ptr<wdg_gat_scores_job> j) {
    return j->H && j->att && j->d_S && j->d_H && j->d_att && j->partial;
}

__global__ __launch_bounds__(GS_THREADS) void gat_scores_backward_kernel(const wdg_gat_scores_job *__restrict__ jobs) {
    const desc_ptr<wdg_gat_scores_job> j = (desc_ptr<wdg_gat_scores_job>)(jobs + blockIdx.z);
    const int n = j->n, G = j->G, w = j->w, heads = j->heads;
    if (!gs_in_limits(n, G, w, heads) || !gs_has_backward(j)) return;
    if (static_cast<int64_t>(blockIdx.x) * GS_ROWS >= n) return;
    const bool vec = (w & 3) == 0 && aligned16(j->H, j->ld_h) && aligned16(j->d_H, j->ld_d_h) && aligned16(j->att, j->ld_att) &&
                     aligned16(j->partial, 0);
    if (vec)
        gs_backward_job<true>(j, n, G, w, heads);
    else
        gs_backward_job<false>(j, n, G, w, heads);
}

// d_att[p, c] = the blocks' partial sums in ascending order from +0: a thread per element
__global__ __launch_bounds__(GS_THREADS) void gat_scores_sum_blocks_kernel(const wdg_gat_scores_job *__restrict__ jobs) {
    const desc_ptr<wdg_gat_scores_job> j = (desc_ptr<wdg_gat_scores_job>)(jobs + blockIdx.z);
    const int n = j->n, G = j->G, w = j->w;
    if (!gs_in_limits(n, G, w, j->heads) || !gs_has_backward(j)) return;
    const int64_t cols = static_cast<int64_t>(G) * w;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * GS_THREADS + threadIdx.x;
    if (e >= 2 * cols) return;
    const int p = e >= cols ? 1 : 0;
    const int64_t c = e - p * cols;
    const global_ptr<const float> part = to_global(static_cast<const float *>(j->partial)) + e;  // element (b, p, c) = part[b * 2 cols]
    const int blocks = (n + GS_ROWS - 1) / GS_ROWS;
    float acc = 0.f;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) acc = acc + part[static_cast<int64_t>(b) * 2 * cols];
    to_global(j->d_att)[p * j->ld_d_att + c] = acc;
}

int gs_check(const char *what, const wdg_gat_scores_job *jobs, int32_t n_jobs, int32_t max_rows, int32_t max_other) {
    WDG_REQUIRE(max_rows >= 0 && max_other >= 0, "%s: negative count", what);
    return wdg::check_job_table(what, jobs, n_jobs);
}

}  // namespace

extern "C" int64_t wdg_gat_scores_partial_len(int32_t n, int32_t G, int32_t w) {
    if (n < 0 || G < 0 || w < 0) return 0;
    return wdg::ceil_div(n, GS_ROWS) * 2 * G * w;
}

extern "C" int wdg_gat_scores_forward_batched_f32(const wdg_gat_scores_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_groups,
                                                  wdg_stream_t stream) {
    if (const int rc = gs_check("gat_scores_forward_batched", jobs_dev, n_jobs, max_rows, max_groups)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_groups == 0) return WDG_OK;
    const int64_t tiles = wdg::ceil_div(max_groups, 64);
    WDG_REQUIRE(tiles <= 65535, "gat_scores_forward_batched: %d groups; one launch takes %d", max_groups, 65535 * 64);
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GS_ROWS)), static_cast<unsigned>(tiles), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gat_scores_forward_kernel, grid, dim3(GS_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("gat_scores_forward_kernel");
}

extern "C" int wdg_gat_scores_backward_batched_f32(const wdg_gat_scores_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                                   wdg_stream_t stream) {
    if (const int rc = gs_check("gat_scores_backward_batched", jobs_dev, n_jobs, max_rows, max_cols)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_cols == 0) return WDG_OK;
    const int64_t tiles = wdg::ceil_div(max_cols, 4 * GS_THREADS);
    WDG_REQUIRE(tiles <= 65535, "gat_scores_backward_batched: %d columns; one launch takes %d", max_cols, 65535 * 4 * GS_THREADS);
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, GS_ROWS)), static_cast<unsigned>(tiles), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gat_scores_backward_kernel, grid, dim3(GS_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    if (const int rc = wdg::check_launch("gat_scores_backward_kernel")) return rc;
    const dim3 sums(static_cast<unsigned>(wdg::ceil_div(2 * static_cast<int64_t>(max_cols), GS_THREADS)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gat_scores_sum_blocks_kernel, sums, dim3(GS_THREADS), 0, wdg::as_stream(stream), jobs_dev);  // (reads the first launch's partial sums)
    return wdg::check_launch("gat_scores_sum_blocks_kernel");
}

// The per-job part of the contract, on the table the caller still holds on the host (train.GatScoresBatch calls this before it uploads).
extern "C" int wdg_gat_scores_check_jobs(const wdg_gat_scores_job *jobs_host, int32_t n_jobs) {
    if (const int rc = gs_check("gat_scores_check_jobs", jobs_host, n_jobs, 0, 0)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_gat_scores_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0 && j.G >= 0, "gat_scores_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.heads >= 1 && j.heads <= WDG_GAT_SCORES_MAX_HEADS, "gat_scores_check_jobs: job %d has a block of %d heads; the kernel holds 1..%d", i,
                    j.heads, WDG_GAT_SCORES_MAX_HEADS);
        WDG_REQUIRE(j.w >= 1 && j.w <= WDG_GAT_SCORES_MAX_W, "gat_scores_check_jobs: job %d has groups of %d columns; the kernel holds 1..%d", i, j.w,
                    WDG_GAT_SCORES_MAX_W);
        const int64_t cols = static_cast<int64_t>(j.G) * j.w;
        WDG_REQUIRE(cols <= INT32_MAX, "gat_scores_check_jobs: job %d has %lld columns; the kernel holds fewer than 2^31", i, static_cast<long long>(cols));
        if (j.n == 0 || j.G == 0) continue;
        WDG_REQUIRE(j.H && j.S && j.att, "gat_scores_check_jobs: job %d has a null H, S or att", i);
        WDG_REQUIRE(j.ld_h >= cols && j.ld_s >= 2 * static_cast<int64_t>(j.G) && j.ld_att >= cols, "gat_scores_check_jobs: job %d has a leading dimension below its row", i);
        const bool any = j.d_S || j.d_H || j.d_att || j.partial;
        if (!any) continue;
        WDG_REQUIRE(j.d_S && j.d_H && j.d_att && j.partial, "gat_scores_check_jobs: job %d has some of d_S, d_H, d_att, partial and not others", i);
        WDG_REQUIRE(j.ld_d_h >= cols && j.ld_d_s >= 2 * static_cast<int64_t>(j.G) && j.ld_d_att >= cols,
                    "gat_scores_check_jobs: job %d has a gradient's leading dimension below its row", i);
        WDG_REQUIRE((reinterpret_cast<uintptr_t>(j.partial) & 15) == 0, "gat_scores_check_jobs: job %d has a workspace that is not 16-byte aligned", i);
    }
    return WDG_OK;
}
