// Y = S W for a sparse feature matrix S (CSR) and a dense W, a table of products per launch (wdg_sparse_dense_batched_f32), and the
// one-time scaling of a feature matrix's stored values in CSR and in transposed order (wdg_feat_scaled_values_f32).
//
// why:      the stacked trainers open with X [W0_1 | ... | W0_R] and close with X^T dP.  X is a bag-of-words table - cora 1.3 % dense,
//           citeseer 0.9 % - and both products were dense MFMA launches over its zeros (2708 x 1433 x 7680 at 120 replicas).
// replaces: th.FloatTensor(features) / .todense() utils/util_funcs.py:339 - the densification in front of the first layer - and
//           preprocess_features utils/util_funcs.py:39-46 for the scaled values.
//
// THE CONTRACT (include/wdg.h states it in full): element (i, j) of Y is ONE fp32 fma chain over row i's stored entries in ascending
// entry order from +0 - acc = fmaf(val[e], W[col[e]][j], acc) - whatever the row's length: no row is split, nothing is added
// across lanes or waves, there is no atomic.  wdg_gemm_f32 is the same chain over ALL k, and fma(0, w, acc) = acc, so with sorted
// columns the bits are the dense product's.  The unit is compiled with contraction off and the fma is written out.
//
// Schedule: a WAVE owns one row and one BAND of 256 columns of Y: lane l holds the four columns 256 band + 4 l .. + 3 in registers, so
// an entry costs the wave one 1-KiB row piece of W (a 16-byte load per lane where W's pointer and leading dimension allow, scalar
// loads elsewhere and at a ragged right edge - the same values, the same fma).  The row's indices and values are read 64 at a time,
// one per lane, and handed out with v_readlane: the addresses of an entry's loads are wave-uniform plus the lane's offset.  Entries
// go in batches of SD_DEPTH = 16 (32 was measured and lost: DESIGN 4.23): sixteen loads are in flight before the first fma, and the
// fmas then run in entry order (a shorter tail goes in batches of 8, 4, 2, 1).  The readlanes run with every lane active; only the
// loads and the fmas are predicated on the lane having columns.  The chain of a long row is SEQUENTIAL by contract: a row of k entries costs k / 16 load
// round trips, so the launch is bounded below by its longest row; rows are therefore dealt longest first (`order`), so that the
// long chains start at once and the short rows fill in behind them.
// Placement: four waves = four consecutive positions of `order` per workgroup, items = (band, row block) band-major, and block b
// works on item xcd_contiguous_item(b): the workgroups b = x (mod 8), which share an XCD's L2, walk one contiguous range of items,
// i.e. a few bands at a time, whose slice of W (n_cols x 1 KiB per band) then stays in that L2 (dealing the items in launch order
// was measured and lost: DESIGN 4.23).  Speed only.
//
// Guards: an entry whose column is outside [0, n_cols) is skipped - its load is redirected to row 0 of W and its fma is not applied -
// and never read through; a position of `order` outside [0, n_rows) is skipped; a job outside the contract is left untouched.
#include <cstdint>

#include "feat_scale.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // the chain's fma is written out; nothing else may be fused

namespace {

using namespace wdg;

constexpr int SD_WAVES = 4;          // rows per workgroup
constexpr int SD_BAND = 256;         // columns of Y per wave: four per lane
constexpr int SD_DEPTH = 16;         // loads in flight before the first fma
constexpr int SD_MAX_JOBS = 65535;   // gridDim.y

struct sd_operand {  // the lane's four columns of one matrix
    global_ptr<float> p;  // column j0 of row 0
    int64_t ld;
    bool vec;  // 16-byte accesses: pointer, leading dimension, and all four columns inside the matrix
    int live;  // how many of the four columns exist (0 .. 4)
};

__device__ __forceinline__ sd_operand sd_columns(const float *base, const int64_t ld, const int j0, const int m) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(base) | static_cast<uintptr_t>(ld * 4)) & 15) == 0;
    const int live = max(0, min(4, m - j0));
    return sd_operand{to_global(const_cast<float *>(base)) + j0, ld, aligned && live == 4, live};
}

// VEC: the WAVE's decision (W 16-byte aligned, m a multiple of 4: every lane that has columns has four) - no per-lane branch
template <bool VEC>
__device__ __forceinline__ void sd_load(const sd_operand &w, const int row, float (&x)[4]) {
    const global_ptr<float> p = w.p + static_cast<int64_t>(row) * w.ld;
    if (VEC) {
        const float4 in = load_f32x4(p);
        x[0] = in.x, x[1] = in.y, x[2] = in.z, x[3] = in.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = t < w.live ? p[t] : 0.f;
    }
}

__device__ __forceinline__ void sd_store(const sd_operand &y, const int row, const float (&x)[4]) {
    const global_ptr<float> p = y.p + static_cast<int64_t>(row) * y.ld;
    if (y.vec) {
        store_f32x4(p, make_float4(x[0], x[1], x[2], x[3]));
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < y.live) p[t] = x[t];
    }
}

// D consecutive entries k0 .. k0 + D - 1 of the 64 the wave holds (c, v: one per lane): all D loads, then the D x 4 fmas in order.
// EVERY lane of the wave is active here: the readlanes give wave-uniform values; a lane without columns only skips the loads and fmas
template <int D, bool VEC>
__device__ __forceinline__ void sd_batch(const sd_operand &w, const int c, const float v, const int k0, const int n_cols, float (&acc)[4]) {
    int ck[D];
    float vk[D];
    bool ok[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        ck[d] = __builtin_amdgcn_readlane(c, k0 + d);
        vk[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k0 + d));
        ok[d] = static_cast<unsigned>(ck[d]) < static_cast<unsigned>(n_cols);
    }
    if (w.live > 0) {
        float x[D][4];
#pragma unroll
        for (int d = 0; d < D; ++d) sd_load<VEC>(w, ok[d] ? ck[d] : 0, x[d]);  // (n_cols >= 1 here: row 0 exists)
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = ok[d] ? __builtin_fmaf(vk[d], x[d][t], acc[t]) : acc[t];
        }
    }
}

// one row's chain for the lane's four columns: the row's indices and values 64 at a time, one per lane, handed out by sd_batch
template <bool VEC>
__device__ __forceinline__ void sd_row(const sd_operand &w, const global_ptr<const int32_t> col, const global_ptr<const float> val, const int beg,
                                       const int end, const int n_cols, const int lane, float (&acc)[4]) {
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);  // wave-uniform
        const bool mine = lane < cnt;
        const int c = mine ? col[e0 + lane] : -1;
        const float v = mine ? (val ? val[e0 + lane] : 1.f) : 0.f;
        int k0 = 0;
        for (; k0 + SD_DEPTH <= cnt; k0 += SD_DEPTH) sd_batch<SD_DEPTH, VEC>(w, c, v, k0, n_cols, acc);
        if (k0 + 8 <= cnt) sd_batch<8, VEC>(w, c, v, k0, n_cols, acc), k0 += 8;
        if (k0 + 4 <= cnt) sd_batch<4, VEC>(w, c, v, k0, n_cols, acc), k0 += 4;
        if (k0 + 2 <= cnt) sd_batch<2, VEC>(w, c, v, k0, n_cols, acc), k0 += 2;
        if (k0 + 1 <= cnt) sd_batch<1, VEC>(w, c, v, k0, n_cols, acc);
    }
}

__global__ __launch_bounds__(64 * SD_WAVES) void sparse_dense_kernel(const wdg_sparse_dense_job *__restrict__ jobs, const int row_blocks,
                                                                     const int n_bands) {
    const desc_ptr<wdg_sparse_dense_job> job = (desc_ptr<wdg_sparse_dense_job>)(jobs + blockIdx.y);
    const int64_t n_items = static_cast<int64_t>(row_blocks) * n_bands;
    const int64_t item = xcd_contiguous_item(blockIdx.x, n_items);
    if (item >= n_items) return;
    const int band = static_cast<int>(item / row_blocks), block = static_cast<int>(item % row_blocks);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_rows = job->n_rows, n_cols = job->n_cols, m = job->m;
    const int pos = block * SD_WAVES + wave;
    if (pos >= n_rows || band * SD_BAND >= m) return;                                  // (wave-uniform, like everything above)
    if (n_cols < 0 || job->ldw < m || job->ldy < m || !job->rowptr || !job->Y) return;  // a job outside the contract: untouched
    const global_ptr<const int32_t> order = to_global(job->order);
    const int row = __builtin_amdgcn_readfirstlane(order ? order[pos] : pos);
    if (static_cast<unsigned>(row) >= static_cast<unsigned>(n_rows)) return;
    const global_ptr<const int32_t> rowptr = to_global(job->rowptr), col = to_global(job->col);
    const global_ptr<const float> val = to_global(job->val);
    const int beg = __builtin_amdgcn_readfirstlane(rowptr[row]);
    const int end = (n_cols > 0 && job->W && job->col) ? __builtin_amdgcn_readfirstlane(rowptr[row + 1]) : beg;  // (nothing to gather from: every entry is skipped)

    const int j0 = band * SD_BAND + 4 * lane;
    const sd_operand w = sd_columns(job->W, job->ldw, j0, m), y = sd_columns(job->Y, job->ldy, j0, m);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if ((m & 3) == 0 && ((reinterpret_cast<uintptr_t>(job->W) | static_cast<uintptr_t>(job->ldw * 4)) & 15) == 0)
        sd_row<true>(w, col, val, beg, end, n_cols, lane, acc);
    else
        sd_row<false>(w, col, val, beg, end, n_cols, lane, acc);
    if (y.live > 0) sd_store(y, row, acc);
}

// val_scaled[e] = scale_row(e)(val[e]) in CSR order: a wave per row, features.hip's sum and RowScale (csrc/feat_scale.h)
__global__ __launch_bounds__(256) void feat_scale_rows_kernel(const int32_t *__restrict__ rowptr_, const int32_t *__restrict__ col_,
                                                              const float *__restrict__ val_, const int n_rows, const int n_feat, const int mode,
                                                              float *__restrict__ out_) {
    const int row = blockIdx.x * 4 + static_cast<int>(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const global_ptr<const int32_t> rowptr = to_global(rowptr_), col = to_global(col_);
    const global_ptr<const float> val = to_global(val_);
    const global_ptr<float> out = to_global(out_);
    const int beg = rowptr[row], end = rowptr[row + 1];
    const RowScale scale(mode, feat_csr_row_sum(col, val, beg, end, n_feat, mode, lane));
    for (int e = beg + lane; e < end; e += 64) out[e] = scale(val ? val[e] : 1.f);
}

// t_val_scaled[e] = val_scaled[t_src[e]]: the same numbers in the transposed layout's order (a source outside [0, nnz): +0)
__global__ __launch_bounds__(256) void feat_scale_permute_kernel(const float *__restrict__ scaled, const int32_t *__restrict__ t_src, const int nnz,
                                                                 float *__restrict__ out) {
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int s = t_src[e];
    out[e] = static_cast<unsigned>(s) < static_cast<unsigned>(nnz) ? scaled[s] : 0.f;
}

}  // namespace

extern "C" int wdg_sparse_dense_batched_f32(const wdg_sparse_dense_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_m,
                                            wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_m >= 0, "sparse_dense_batched: negative count");
    WDG_REQUIRE(n_jobs <= SD_MAX_JOBS, "sparse_dense_batched: %d jobs; one launch takes %d", n_jobs, SD_MAX_JOBS);
    if (n_jobs == 0 || max_rows == 0 || max_m == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "sparse_dense_batched: null job table");
    const int64_t row_blocks = wdg::ceil_div(max_rows, SD_WAVES), n_bands = wdg::ceil_div(max_m, SD_BAND);
    const int64_t blocks = wdg::xcd_grid_size(row_blocks * n_bands);
    WDG_REQUIRE(blocks <= INT32_MAX, "sparse_dense_batched: %d rows x %d columns are more workgroups than one launch takes", max_rows, max_m);
    hipLaunchKernelGGL(sparse_dense_kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(n_jobs)), dim3(64 * SD_WAVES), 0,
                       wdg::as_stream(stream), jobs_dev, static_cast<int>(row_blocks), static_cast<int>(n_bands));
    return wdg::check_launch("sparse_dense_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host (sparse_features.SparseDenseBatch calls this on
// the table it is about to upload).
extern "C" int wdg_sparse_dense_check_jobs(const wdg_sparse_dense_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "sparse_dense_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "sparse_dense_check_jobs: null job table");
    WDG_REQUIRE(n_jobs <= SD_MAX_JOBS, "sparse_dense_check_jobs: %d jobs; one launch takes %d", n_jobs, SD_MAX_JOBS);
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_sparse_dense_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_cols >= 0 && j.m >= 0, "sparse_dense_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.reserved == 0, "sparse_dense_check_jobs: job %d has a reserved word of %d", i, j.reserved);
        if (j.n_rows == 0 || j.m == 0) continue;
        WDG_REQUIRE(j.ldw >= j.m && j.ldy >= j.m, "sparse_dense_check_jobs: job %d has a leading dimension below its %d columns", i, j.m);
        WDG_REQUIRE(j.rowptr && j.Y, "sparse_dense_check_jobs: job %d has a null rowptr or Y", i);
        WDG_REQUIRE(j.n_cols == 0 || (j.col && j.W), "sparse_dense_check_jobs: job %d has a null col or W", i);  // (a matrix without entries passes any non-null col: it is never read)
    }
    return WDG_OK;
}

extern "C" int wdg_feat_scaled_values_f32(const int32_t *rowptr, const int32_t *col, const float *val, int32_t n_rows, int32_t n_feat,
                                          int normalise, const int32_t *t_src, int32_t nnz, float *val_scaled, float *t_val_scaled,
                                          wdg_stream_t stream) {
    WDG_REQUIRE(n_rows >= 0 && n_feat >= 0 && nnz >= 0, "feat_scaled_values: negative count");
    WDG_REQUIRE(normalise == WDG_FEAT_NORM_NONE || normalise == WDG_FEAT_NORM_SUM || normalise == WDG_FEAT_NORM_ABS,
                "feat_scaled_values: normalise %d is none of WDG_FEAT_NORM_*", normalise);
    if (n_rows == 0 || nnz == 0) return WDG_OK;
    WDG_REQUIRE(rowptr && col && val_scaled, "feat_scaled_values: null rowptr, col or val_scaled");
    WDG_REQUIRE((t_src == nullptr) == (t_val_scaled == nullptr), "feat_scaled_values: t_src and t_val_scaled go together");
    hipStream_t st = wdg::as_stream(stream);
    hipLaunchKernelGGL(feat_scale_rows_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(n_rows, 4))), dim3(256), 0, st, rowptr, col, val, n_rows,
                       n_feat, normalise, val_scaled);
    if (t_src)
        hipLaunchKernelGGL(feat_scale_permute_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(nnz, 256))), dim3(256), 0, st, val_scaled, t_src, nnz,
                           t_val_scaled);
    return wdg::check_launch("feat_scale_rows_kernel");
}
