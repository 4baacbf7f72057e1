// One GCNII layer behind its aggregation for many layers / graphs in one launch - S = (1 - alpha) P + alpha H0, Z = (1 - beta) S + beta S W,
// out = relu_dropout(Z) - and its backward pass: d_P, d_H0 +=, the blocks' partial sums of d_W, and (an entry of its own, called once
// for all the layers of a model) d_W.  include/wdg.h states the arithmetic operation by operation and every sum's order;
// tests/_gcnii_ref.py restates both passes in numpy.
//
// replaces: nothing of the reference, which ships no model code - the layer stands behind the aggregation with the fixed weights of
//           normalize_tensor, utils/util_funcs.py:365-381, whose result is its P.
//
// Shape: a workgroup of 256 threads owns a block of WDG_GCNII_ROW_BLOCK rows of one job and keeps the block's S (backward: S and dZ)
// in LDS; the w x w product runs on plain fmaf chains - on gfx950 the exact-fp32 matrix instructions run at the vector rate, and a
// chain written out has bits that can be stated.  The job's width picks the thread shape: CW = 16, 32, 64 or 128, the power of two
// that holds w.
//   forward   a thread owns FOUR adjacent columns of 1, 1, 2 or 4 rows: per k it reads W[k, c .. c + 3] (one 16-byte load, coalesced
//             over the lanes), S[i, k] from LDS (a broadcast), and advances its chains; the epilogue - Z, one Philox block per four
//             columns, the store - is the thread's own.
//   backward  the same threads own four adjacent k of their rows: U's chains walk c, reading W[k .. k + 3, c .. c + 3] (the lane's own
//             four rows: cache lines it uses up over the next steps) and dZ[i, c] from LDS; d_P and d_H0 are the thread's own.  Then a
//             thread owns four adjacent c of 1, 1, 4 or 16 rows k of the block's partial sum and walks the block's rows in order.
//   weight    a thread per element of d_W adds the blocks' sums in order.  No atomics.
// 16-byte accesses are the JOB's decision per pass (every pointer and leading dimension of the pass and w: multiples of 16 bytes / 4),
// so no per-lane branch sits between a load and its use.
#include <cstdint>

#include "philox.h"
#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // every fused multiply-add of the definition is written as fmaf; nothing else may be fused

namespace {

using namespace wdg;

constexpr int GC_THREADS = 256;
constexpr int GC_ROWS = WDG_GCNII_ROW_BLOCK;  // rows per workgroup of either pass; the backward pass's block of partial sums
constexpr int GC_LD = WDG_GCNII_MAX_W + 4;    // the LDS tiles' row pitch in floats: a multiple of 4 (16-byte reads), not of 32
constexpr int GC_MAX_JOBS = 65535;            // gridDim.z

__device__ __forceinline__ bool gc_in_limits(const int n, const int w) { return n > 0 && w >= 1 && w <= WDG_GCNII_MAX_W; }

// the contract of wdg_relu_dropout_batched_f32 for one element (csrc/dropout.hip's dr_value, word for word)
__device__ __forceinline__ float gc_relu_dropout(const float h, const unsigned word, const unsigned drop_threshold, const float scale) {
    if (h != h) return h;
    return (word >= drop_threshold && h > 0.f) ? h * scale : 0.f;
}

// S of the block's rows into the LDS tile (columns w .. 4 ceil(w / 4) - 1 of a row: zeros, so that a group of four reads numbers) and,
// where the job has one, into S: a thread per (row, four columns), in passes
template <bool VEC>
__device__ __forceinline__ void gc_stage_s(const desc_ptr<wdg_gcnii_job> j, const int w, const int r0, const int r1, float (*tile)[GC_LD]) {
    const float alpha = j->alpha, a1 = 1.0f - alpha;
    const global_ptr<const float> P = to_global(j->P), H0 = to_global(j->H0);
    const global_ptr<float> S = to_global(j->S);
    const int64_t ld_p = j->ld_p, ld_h0 = j->ld_h0, ld_s = j->ld_s;
    const int quads = (w + 3) >> 2;
    for (int e = static_cast<int>(threadIdx.x); e < (r1 - r0) * quads; e += GC_THREADS) {
        const int rl = e / quads, c = 4 * (e - rl * quads), live = min(4, w - c);
        const int64_t r = r0 + rl;
        float p[4], h[4], s[4];
        load4<VEC>(P + r * ld_p + c, live, p);
        load4<VEC>(H0 + r * ld_h0 + c, live, h);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = fmaf(alpha, h[k], a1 * p[k]);
        if (j->S) store4<VEC>(S + r * ld_s + c, live, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[rl][c + k] = k < live ? s[k] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int CW, bool VEC>
__device__ __forceinline__ void gc_forward_job(const desc_ptr<wdg_gcnii_job> j, const int n, const int w, const int act, const unsigned drop_threshold,
                                               const float scale, const unsigned seed, const unsigned *__restrict__ step_dev, float (*tile)[GC_LD]) {
    constexpr int Q = CW / 4, GROUPS = GC_THREADS / Q, RPT = GROUPS >= GC_ROWS ? 1 : GC_ROWS / GROUPS;  // a thread's rows: rg, rg + GROUPS, ...
    const int r0 = static_cast<int>(blockIdx.x) * GC_ROWS, r1 = min(n, r0 + GC_ROWS);
    gc_stage_s<VEC>(j, w, r0, r1, tile);
    __syncthreads();
    const int t = static_cast<int>(threadIdx.x), c = 4 * (t % Q), rg = t / Q;
    if (c >= w || r0 + rg >= r1) return;  // (after the only barrier)
    const int live = min(4, w - c);
    const float beta = j->beta, b1 = 1.0f - beta;
    const global_ptr<const float> W = to_global(j->W) + c;
    const int64_t ld_w = j->ld_w;
    float acc[RPT][4];
#pragma unroll
    for (int u = 0; u < RPT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[u][q] = 0.f;
#pragma unroll 4
    for (int k = 0; k < w; ++k) {
        float wk[4];
        load4<VEC>(W + k * ld_w, live, wk);
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const float s = tile[min(rg + u * GROUPS, GC_ROWS - 1)][k];  // (a row past the block's end: never stored)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[u][q] = fmaf(s, wk[q], acc[u][q]);
        }
    }
    const global_ptr<float> out = to_global(j->out);
    const int64_t ld_out = j->ld_out;
    const unsigned groups_per_row = (static_cast<unsigned>(w) + 3u) >> 2, stream = j->stream;
    const bool draws = act != 0 && drop_threshold != 0u;  // (no word is below a threshold of 0: a plain ReLU draws none)
    const unsigned step = draws ? *step_dev : 0u;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const int rl = rg + u * GROUPS, r = r0 + rl;
        if (r >= r1) break;
        float z[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) z[q] = fmaf(beta, acc[u][q], b1 * tile[rl][c + q]);
        if (act != 0) {
            philox_words pw = {{0u, 0u, 0u, 0u}};
            if (draws) pw = philox4x32_10_words(static_cast<unsigned>(r) * groups_per_row + (static_cast<unsigned>(c) >> 2), step, seed, stream);
#pragma unroll
            for (int q = 0; q < 4; ++q) z[q] = gc_relu_dropout(z[q], pw.w[q], drop_threshold, scale);
        }
        store4<VEC>(out + static_cast<int64_t>(r) * ld_out + c, live, z);
    }
}

template <bool VEC>
__device__ __forceinline__ void gc_forward_width(const desc_ptr<wdg_gcnii_job> j, const int n, const int w, const int act, const unsigned drop_threshold,
                                                 const float scale, const unsigned seed, const unsigned *__restrict__ step_dev, float (*tile)[GC_LD]) {
    if (w <= 16)
        gc_forward_job<16, VEC>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
    else if (w <= 32)
        gc_forward_job<32, VEC>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
    else if (w <= 64)
        gc_forward_job<64, VEC>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
    else
        gc_forward_job<128, VEC>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
}

__global__ __launch_bounds__(GC_THREADS) void gcnii_forward_kernel(const wdg_gcnii_job *__restrict__ jobs, const int act, const unsigned drop_threshold,
                                                                   const float scale, const unsigned seed, const unsigned *__restrict__ step_dev) {
    __shared__ __attribute__((aligned(16))) float tile[GC_ROWS][GC_LD];
    const desc_ptr<wdg_gcnii_job> j = (desc_ptr<wdg_gcnii_job>)(jobs + blockIdx.z);
    const int n = j->n, w = j->w;
    if (!gc_in_limits(n, w) || !j->P || !j->H0 || !j->W || !j->out) return;  // (uniform: before the barrier)
    if (static_cast<int64_t>(blockIdx.x) * GC_ROWS >= n) return;
    const bool vec = (w & 3) == 0 && aligned16(j->P, j->ld_p) && aligned16(j->H0, j->ld_h0) && aligned16(j->W, j->ld_w) &&
                     aligned16(j->out, j->ld_out) && aligned16(j->S, j->ld_s);
    if (vec)
        gc_forward_width<true>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
    else
        gc_forward_width<false>(j, n, w, act, drop_threshold, scale, seed, step_dev, tile);
}

// --------------------------------------------------------------------------------------------------------------- backward
template <int CW, bool VEC>
__device__ __forceinline__ void gc_backward_job(const desc_ptr<wdg_gcnii_job> j, const int n, const int w, const int act, const float scale,
                                                float (*s_tile)[GC_LD], float (*dz_tile)[GC_LD]) {
    constexpr int Q = CW / 4, GROUPS = GC_THREADS / Q, RPT = GROUPS >= GC_ROWS ? 1 : GC_ROWS / GROUPS;
    constexpr int KPT = CW >= GROUPS ? CW / GROUPS : 1;  // partial sums: a thread's rows k (kg KPT .. kg KPT + KPT - 1) of its four columns
    const int r0 = static_cast<int>(blockIdx.x) * GC_ROWS, r1 = min(n, r0 + GC_ROWS);
    const int quads = (w + 3) >> 2;
    {  // S and dZ of the block's rows into the tiles (columns w .. 4 ceil(w / 4) - 1: zeros)
        const global_ptr<const float> S = to_global(static_cast<const float *>(j->S)), out = to_global(static_cast<const float *>(j->out)),
                                      d_out = to_global(j->d_out);
        const int64_t ld_s = j->ld_s, ld_out = j->ld_out, ld_d_out = j->ld_d_out;
        for (int e = static_cast<int>(threadIdx.x); e < (r1 - r0) * quads; e += GC_THREADS) {
            const int rl = e / quads, c = 4 * (e - rl * quads), live = min(4, w - c);
            const int64_t r = r0 + rl;
            float s[4], g[4], o[4] = {1.f, 1.f, 1.f, 1.f};
            load4<VEC>(S + r * ld_s + c, live, s);
            load4<VEC>(d_out + r * ld_d_out + c, live, g);
            if (act != 0) load4<VEC>(out + r * ld_out + c, live, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dz = act != 0 ? (o[k] > 0.f ? g[k] * scale : 0.f) : g[k];
                s_tile[rl][c + k] = k < live ? s[k] : 0.f;
                dz_tile[rl][c + k] = k < live ? dz : 0.f;
            }
        }
    }
    __syncthreads();
    const int t = static_cast<int>(threadIdx.x), q4 = 4 * (t % Q), rg = t / Q;
    const float alpha = j->alpha, a1 = 1.0f - alpha, beta = j->beta, b1 = 1.0f - beta;
    if (q4 < w && r0 + rg < r1) {  // U, dS, d_P, d_H0 of the thread's rows at k = q4 .. q4 + 3
        const int live = min(4, w - q4);
        const int64_t ld_w = j->ld_w;
        global_ptr<const float> Wk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) Wk[q] = to_global(j->W) + min(q4 + q, w - 1) * ld_w;  // (a row the thread does not have: its last one, never stored)
        float acc[RPT][4];
#pragma unroll
        for (int u = 0; u < RPT; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[u][q] = 0.f;
        for (int c = 0; c < 4 * quads; c += 4) {
            const int lc = min(4, w - c);
            float wk[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) load4<VEC>(Wk[q] + c, lc, wk[q]);
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const float *dz = dz_tile[min(rg + u * GROUPS, GC_ROWS - 1)] + c;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    if (cc >= lc) break;  // (uniform: w is the job's)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[u][q] = fmaf(dz[cc], wk[q][cc], acc[u][q]);
                }
            }
        }
        const global_ptr<float> d_P = to_global(j->d_P), d_H0 = to_global(j->d_H0);
        const int64_t ld_d_p = j->ld_d_p, ld_d_h0 = j->ld_d_h0;
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int rl = rg + u * GROUPS;
            const int64_t r = r0 + rl;
            if (r >= r1) break;
            float h[4], dp[4];
            load4<VEC>(d_H0 + r * ld_d_h0 + q4, live, h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float ds = fmaf(beta, acc[u][q], b1 * dz_tile[rl][q4 + q]);
                dp[q] = a1 * ds;
                h[q] = fmaf(alpha, ds, h[q]);
            }
            store4<VEC>(d_P + r * ld_d_p + q4, live, dp);
            store4<VEC>(d_H0 + r * ld_d_h0 + q4, live, h);
        }
    }
    // the block's partial sums: columns q4 .. q4 + 3 of rows k = kg KPT .. of partial[b]
    const int kg = rg, k0 = kg * KPT;
    if (q4 >= w || k0 >= w) return;
    const int live = min(4, w - q4);
    float acc[KPT][4];
#pragma unroll
    for (int u = 0; u < KPT; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[u][q] = 0.f;
    for (int rl = 0; rl < r1 - r0; ++rl) {
        float dz[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dz[q] = dz_tile[rl][q4 + q];
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const float s = s_tile[rl][min(k0 + u, WDG_GCNII_MAX_W - 1)];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[u][q] = fmaf(s, dz[q], acc[u][q]);
        }
    }
    const global_ptr<float> part = to_global(j->partial) + static_cast<int64_t>(blockIdx.x) * w * w + q4;
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        if (k0 + u >= w) break;
        store4<VEC>(part + static_cast<int64_t>(k0 + u) * w, live, acc[u]);
    }
}

template <bool VEC>
__device__ __forceinline__ void gc_backward_width(const desc_ptr<wdg_gcnii_job> j, const int n, const int w, const int act, const float scale,
                                                  float (*s_tile)[GC_LD], float (*dz_tile)[GC_LD]) {
    if (w <= 16)
        gc_backward_job<16, VEC>(j, n, w, act, scale, s_tile, dz_tile);
    else if (w <= 32)
        gc_backward_job<32, VEC>(j, n, w, act, scale, s_tile, dz_tile);
    else if (w <= 64)
        gc_backward_job<64, VEC>(j, n, w, act, scale, s_tile, dz_tile);
    else
        gc_backward_job<128, VEC>(j, n, w, act, scale, s_tile, dz_tile);
}

__device__ __forceinline__ bool gc_has_backward(const desc_ptr<wdg_gcnii_job> j) {
    return j->W && j->out && j->S && j->d_out && j->d_P && j->d_H0 && j->d_W && j->partial;
}

__global__ __launch_bounds__(GC_THREADS) void gcnii_backward_kernel(const wdg_gcnii_job *__restrict__ jobs, const int act, const float scale) {
    __shared__ __attribute__((aligned(16))) float s_tile[GC_ROWS][GC_LD];
    __shared__ __attribute__((aligned(16))) float dz_tile[GC_ROWS][GC_LD];
    const desc_ptr<wdg_gcnii_job> j = (desc_ptr<wdg_gcnii_job>)(jobs + blockIdx.z);
    const int n = j->n, w = j->w;
    if (!gc_in_limits(n, w) || !gc_has_backward(j)) return;  // (uniform: before the barrier)
    if (static_cast<int64_t>(blockIdx.x) * GC_ROWS >= n) return;
    const bool vec = (w & 3) == 0 && aligned16(j->S, j->ld_s) && aligned16(j->W, j->ld_w) && aligned16(j->out, j->ld_out) &&
                     aligned16(j->d_out, j->ld_d_out) && aligned16(j->d_P, j->ld_d_p) && aligned16(j->d_H0, j->ld_d_h0) &&
                     aligned16(j->partial, 0);
    if (vec)
        gc_backward_width<true>(j, n, w, act, scale, s_tile, dz_tile);
    else
        gc_backward_width<false>(j, n, w, act, scale, s_tile, dz_tile);
}

// d_W[k, c] = beta * (the blocks' partial sums in ascending order from +0): a thread per element
__global__ __launch_bounds__(GC_THREADS) void gcnii_weight_grad_kernel(const wdg_gcnii_job *__restrict__ jobs) {
    const desc_ptr<wdg_gcnii_job> j = (desc_ptr<wdg_gcnii_job>)(jobs + blockIdx.z);
    const int n = j->n, w = j->w;
    if (!gc_in_limits(n, w) || !gc_has_backward(j)) return;
    const int e = static_cast<int>(blockIdx.x) * GC_THREADS + static_cast<int>(threadIdx.x);
    if (e >= w * w) return;
    const int k = e / w, c = e - k * w;
    const global_ptr<const float> part = to_global(static_cast<const float *>(j->partial)) + e;  // element (b, k, c) = part[b w w]
    const int blocks = (n + GC_ROWS - 1) / GC_ROWS;
    float acc = 0.f;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) acc = acc + part[static_cast<int64_t>(b) * w * w];
    to_global(j->d_W)[k * j->ld_d_w + c] = j->beta * acc;
}

int gc_check(const char *what, const wdg_gcnii_job *jobs, int32_t n_jobs, int32_t max_rows, int32_t max_w) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_w >= 0, "%s: negative count", what);
    WDG_REQUIRE(n_jobs <= GC_MAX_JOBS, "%s: %d jobs; one launch takes %d", what, n_jobs, GC_MAX_JOBS);
    WDG_REQUIRE(max_w <= WDG_GCNII_MAX_W, "%s: %d columns; the kernel holds 1..%d", what, max_w, WDG_GCNII_MAX_W);
    WDG_REQUIRE(n_jobs == 0 || jobs != nullptr, "%s: null job table", what);
    WDG_REQUIRE(static_cast<int64_t>(max_rows) * wdg::ceil_div(max_w, 4) < (int64_t{1} << 32),
                "%s: %d rows of %d columns hold 2^32 or more groups of four columns", what, max_rows, max_w);
    return WDG_OK;
}

int gc_check_act(const char *what, int32_t act, float scale) {
    WDG_REQUIRE(act == 0 || act == 1, "%s: act is %d; 0 (none) or 1 (ReLU + dropout) expected", what, act);
    WDG_REQUIRE(scale == scale, "%s: the scale is not a number", what);
    return WDG_OK;
}

dim3 gc_grid(int32_t n_jobs, int32_t max_rows) {
    return dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, GC_ROWS)), 1, static_cast<unsigned>(n_jobs));
}

}  // namespace

extern "C" int64_t wdg_gcnii_partial_len(int32_t n, int32_t w) {
    if (n < 0 || w < 0) return 0;
    return wdg::ceil_div(n, GC_ROWS) * w * w;
}

extern "C" int wdg_gcnii_forward_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, int32_t act,
                                             uint32_t drop_threshold, float scale, uint32_t seed, const uint32_t *step_dev, wdg_stream_t stream) {
    if (const int rc = gc_check("gcnii_forward_batched", jobs_dev, n_jobs, max_rows, max_w)) return rc;
    if (const int rc = gc_check_act("gcnii_forward_batched", act, scale)) return rc;
    WDG_REQUIRE(act == 0 || step_dev != nullptr, "gcnii_forward_batched: null step word");
    if (n_jobs == 0 || max_rows == 0 || max_w == 0) return WDG_OK;
    hipLaunchKernelGGL(gcnii_forward_kernel, gc_grid(n_jobs, max_rows), dim3(GC_THREADS), 0, wdg::as_stream(stream), jobs_dev, act, drop_threshold, scale,
                       seed, step_dev);
    return wdg::check_launch("gcnii_forward_kernel");
}

extern "C" int wdg_gcnii_backward_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, int32_t act, float scale,
                                              wdg_stream_t stream) {
    if (const int rc = gc_check("gcnii_backward_batched", jobs_dev, n_jobs, max_rows, max_w)) return rc;
    if (const int rc = gc_check_act("gcnii_backward_batched", act, scale)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_w == 0) return WDG_OK;
    hipLaunchKernelGGL(gcnii_backward_kernel, gc_grid(n_jobs, max_rows), dim3(GC_THREADS), 0, wdg::as_stream(stream), jobs_dev, act, scale);
    return wdg::check_launch("gcnii_backward_kernel");
}

extern "C" int wdg_gcnii_weight_grad_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, wdg_stream_t stream) {
    if (const int rc = gc_check("gcnii_weight_grad_batched", jobs_dev, n_jobs, max_rows, max_w)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_w == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(static_cast<int64_t>(max_w) * max_w, GC_THREADS)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gcnii_weight_grad_kernel, grid, dim3(GC_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("gcnii_weight_grad_kernel");
}

// The per-job part of the contract, on the table the caller still holds on the host (train.GcniiBatch calls this before it uploads).
extern "C" int wdg_gcnii_check_jobs(const wdg_gcnii_job *jobs_host, int32_t n_jobs) {
    if (const int rc = gc_check("gcnii_check_jobs", jobs_host, n_jobs, 0, 0)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_gcnii_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0, "gcnii_check_jobs: job %d has a negative row count", i);
        WDG_REQUIRE(j.w >= 1 && j.w <= WDG_GCNII_MAX_W, "gcnii_check_jobs: job %d has %d columns; the kernel holds 1..%d", i, j.w, WDG_GCNII_MAX_W);
        WDG_REQUIRE(static_cast<int64_t>(j.n) * wdg::ceil_div(j.w, 4) < (int64_t{1} << 32), "gcnii_check_jobs: job %d holds 2^32 or more groups of four columns", i);
        if (j.n == 0) continue;
        WDG_REQUIRE(j.P && j.H0 && j.W && j.out, "gcnii_check_jobs: job %d has a null P, H0, W or out", i);
        WDG_REQUIRE(j.ld_p >= j.w && j.ld_h0 >= j.w && j.ld_w >= j.w && j.ld_out >= j.w && (!j.S || j.ld_s >= j.w),
                    "gcnii_check_jobs: job %d has a leading dimension below its row", i);
        const bool any = j.d_out || j.d_P || j.d_H0 || j.d_W || j.partial;
        if (!any) continue;
        WDG_REQUIRE(j.d_out && j.d_P && j.d_H0 && j.d_W && j.partial, "gcnii_check_jobs: job %d has some of d_out, d_P, d_H0, d_W, partial and not others", i);
        WDG_REQUIRE(j.S, "gcnii_check_jobs: job %d has a backward pass and no S", i);
        WDG_REQUIRE(j.ld_d_out >= j.w && j.ld_d_p >= j.w && j.ld_d_h0 >= j.w && j.ld_d_w >= j.w,
                    "gcnii_check_jobs: job %d has a gradient's leading dimension below its row", i);
        WDG_REQUIRE((reinterpret_cast<uintptr_t>(j.partial) & 15) == 0, "gcnii_check_jobs: job %d has a workspace that is not 16-byte aligned", i);
    }
    return WDG_OK;
}
