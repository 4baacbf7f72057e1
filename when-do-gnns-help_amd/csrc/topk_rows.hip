// The k best columns of every row of many dense fp32 matrices in one launch: the selection of a k-nearest-neighbour feature graph
// (AM-GCN, SimP-GCN, kNN-GCN) over similarity matrices that ops.gemm(transb) / GramBatch leave on the device, and the reciprocal row
// norms that turn dot products into a cosine ranking.  include/wdg.h DEFINES the result - a total order, so the output is a pure
// function of the input - and lists every refusal; tests/_topk_ref.py restates it in numpy.
//
// stands next to: the dense cosine matrix of `generalized_edge_homophily` (utils/homophily_metrics.py:167) - its rows are what
//           wdg_topk_rows_batched_f32 ranks; wdg_row_rnorm_f32's 0 for an all-zero row is that function's sim[isnan] = 0
//           (utils/homophily_metrics.py:168).  The reference selects nothing: the kNN graph is defined by this project.
//
// Shape: grid (row groups, jobs), TK_WAVES waves per workgroup, ONE wave owns one row at a time.  Lane l holds the current rank-l
// candidate as a 64-bit word: the monotone uint32 image of the key (auc.hip's) above the complemented column, so "ranks before" is
// "is the larger word" and 0 - the image of no eligible key - is "nothing".  The row is streamed in coalesced chunks of 64 columns,
// four chunks requested at once; a chunk is looked at only when a __ballot finds a word above the current k-th.  Up to TK_INSERT_MAX
// such words are inserted one by one (a scalar lane read, a ballot for the rank, one lane shift of the held set); more than that and
// the chunk is sorted (bitonic, 21 compare-exchange steps) and merged with the held 64 (one reversed maximum + 6 steps), every step
// a cross-lane move of the two halves of the word - __shfl_xor, which this compiler lowers to ds_bpermute_b32 throughout (the LDS
// crossbar, no LDS allocation; it emits no DPP form for them).  Both routes keep the held set in the one order the definition fixes, so which one ran cannot show.  No LDS allocation, no per-thread array indexed at run time, no atomic.  The keys written out are read again at the
// chosen columns (k loads per row), so a -0 product stays -0.
// #pragma clang fp contract(off): the key is ONE rounded product, and wdg_row_rnorm_f32's fmaf chain is written out (the Makefile
// passes -ffp-contract=off as well).
#include <algorithm>

#include "wdg_common.h"

#pragma clang fp contract(off)

namespace {

using namespace wdg;

constexpr int TK_WAVES = 4, TK_THREADS = TK_WAVES * kWave;
constexpr int TK_MAX_JOBS = 65535;      // gridDim.y: a job per y
constexpr int TK_MAX_GROUPS = 1 << 20;  // gridDim.x: the waves stride over a job's rows
constexpr int TK_FLAGS = WDG_TOPK_EXCLUDE_SELF | WDG_TOPK_SORT_COLUMNS;
constexpr int TK_AHEAD = 4;             // chunks of 64 columns requested together
constexpr int TK_INSERT_MAX = 8;        // up to this many entrants of a chunk are inserted one by one; more: sort + merge
static_assert(WDG_TOPK_MAX_K == kWave, "a lane per held candidate");

// what the kernel skips and wdg_topk_rows_check_jobs refuses (one predicate)
template <typename J>
__host__ __device__ __forceinline__ bool tk_malformed(const J job) {
    return job->k < 1 || job->k > WDG_TOPK_MAX_K || job->rows < 0 || job->cols < 0 || job->ld < job->cols || job->ld_out < job->k ||
           (job->flags & ~TK_FLAGS) != 0 || job->out_col == nullptr || job->out_len == nullptr ||
           (job->scores == nullptr && job->rows > 0 && job->cols > 0);
}

// the word of (key, column): 0 for a NaN; larger = ranks earlier.  -0 and +0 share an image; the image of any other key is > 0
// (the image 0 belongs to a NaN's bit pattern), so a word of an eligible column is never 0.
__device__ __forceinline__ uint64_t tk_word(float key, const int col) {
    if (key != key) return 0ull;
    uint32_t bits = __float_as_uint(key);
    if ((bits & 0x7fffffffu) == 0u) bits = 0u;  // -0 -> +0
    const uint32_t image = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return (static_cast<uint64_t>(image) << 32) | static_cast<uint32_t>(~col);
}

// lane `src`'s word in every lane (src is wave-uniform)
__device__ __forceinline__ uint64_t tk_readlane(const uint64_t w, const int src) {
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(w)), src);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(w >> 32)), src);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t tk_max(const uint64_t a, const uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t tk_min(const uint64_t a, const uint64_t b) { return a < b ? a : b; }

// the wave's 64 words in descending order over the lanes (bitonic sorting network; zeros end up last)
__device__ __forceinline__ uint64_t tk_sort_desc(uint64_t w, const int lane) {
#pragma unroll
    for (int size = 2; size <= kWave; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            const uint64_t p = __shfl_xor(w, j);
            const bool keep_max = ((lane & j) == 0) == ((lane & size) == 0);
            w = keep_max ? tk_max(w, p) : tk_min(w, p);
        }
    }
    return w;
}

// held and chunk both descending -> the 64 largest of the 128, descending
__device__ __forceinline__ uint64_t tk_merge_desc(const uint64_t held, const uint64_t chunk, const int lane) {
    uint64_t w = tk_max(held, __shfl(chunk, kWave - 1 - lane));  // bitonic, and it holds the 64 largest
#pragma unroll
    for (int j = kWave >> 1; j > 0; j >>= 1) {
        const uint64_t p = __shfl_xor(w, j);
        w = (lane & j) == 0 ? tk_max(w, p) : tk_min(w, p);
    }
    return w;
}

// the wave's 64 unsigned values in ascending order over the lanes
__device__ __forceinline__ uint32_t tk_sort_asc_u32(uint32_t w, const int lane) {
#pragma unroll
    for (int size = 2; size <= kWave; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            const uint32_t p = __shfl_xor(w, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & size) == 0);
            w = keep_min ? min(w, p) : max(w, p);
        }
    }
    return w;
}

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const wdg_topk_job *__restrict__ jobs) {
    const desc_ptr<wdg_topk_job> job = (desc_ptr<wdg_topk_job>)(jobs + blockIdx.y);
    if (tk_malformed(job)) return;
    const int rows = job->rows, cols = job->cols, k = job->k, flags = job->flags;
    const int64_t ld = job->ld, ld_out = job->ld_out, row0 = job->row0;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const global_ptr<const float> scores = to_global(job->scores), scale = to_global(job->col_scale);
    const global_ptr<int32_t> out_col = to_global(job->out_col), out_len = to_global(job->out_len);
    const global_ptr<float> out_key = to_global(job->out_key);
    const bool has_scale = job->col_scale != nullptr, has_key = job->out_key != nullptr;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * TK_WAVES + wave; r < rows; r += static_cast<int64_t>(gridDim.x) * TK_WAVES) {
        const global_ptr<const float> row = scores + r * ld;
        const int64_t self = (flags & WDG_TOPK_EXCLUDE_SELF) ? row0 + r : int64_t{-1};  // (no column is -1)
        uint64_t held = 0ull, kth = 0ull;  // kth: the word of rank k - 1, wave-uniform
        for (int64_t c0 = 0; c0 < cols; c0 += TK_AHEAD * kWave) {
            float v[TK_AHEAD], s[TK_AHEAD];
#pragma unroll
            for (int u = 0; u < TK_AHEAD; ++u) {  // (columns are counted in 64 bits: c0 + 255 may pass 2^31)
                const int64_t c = c0 + u * kWave + lane;
                v[u] = c < cols ? row[c] : 0.0f;
                s[u] = (has_scale && c < cols) ? scale[c] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < TK_AHEAD; ++u) {
                const int64_t c = c0 + u * kWave + lane;
                const float key = has_scale ? v[u] * s[u] : v[u];
                const uint64_t w = (c < cols && c != self) ? tk_word(key, static_cast<int>(c)) : 0ull;
                uint64_t cand = __ballot(w > kth);
                if (cand == 0ull) continue;  // (wave-uniform: nothing of this chunk enters the first k)
                if (__popcll(cand) <= TK_INSERT_MAX) {
                    // a few entrants - the usual chunk once the held set has settled: each is inserted where it ranks, the rest of
                    // the held set moves up a lane and the last falls off (a word that no longer beats the k-th after an earlier
                    // insertion still lands where it ranks: harmless)
                    do {
                        const int src = __builtin_ctzll(cand);
                        cand &= cand - 1ull;
                        const uint64_t c = tk_readlane(w, src);
                        const int pos = __popcll(__ballot(held > c));  // held is descending: lanes 0 .. pos - 1 rank before c
                        const uint64_t up = __shfl_up(held, 1);
                        held = lane < pos ? held : (lane == pos ? c : up);
                    } while (cand != 0ull);
                } else {
                    held = tk_merge_desc(held, tk_sort_desc(w, lane), lane);
                }
                kth = tk_readlane(held, k - 1);
            }
        }
        const int len = __popcll(__ballot(lane < k && held != 0ull));  // the eligible columns come first: lanes 0 .. len - 1
        uint32_t c = lane < len ? ~static_cast<uint32_t>(held) : 0xffffffffu;
        if (flags & WDG_TOPK_SORT_COLUMNS) c = tk_sort_asc_u32(c, lane);  // (the padding sorts last)
        if (lane < k) {
            const bool live = lane < len;
            out_col[r * ld_out + lane] = live ? static_cast<int32_t>(c) : -1;
            if (has_key) {
                float key = 0.0f;
                if (live) key = has_scale ? row[c] * scale[c] : row[c];
                out_key[r * ld_out + lane] = key;
            }
        }
        if (lane == 0) out_len[r] = len;
    }
}

// out[i] = 1 / ||x_i||, 0 for an all-zero row; the arithmetic is written out in include/wdg.h
__global__ __launch_bounds__(TK_THREADS) void row_rnorm_kernel(const float *__restrict__ x, const int64_t ld, const int n, const int F, float *__restrict__ out) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * TK_WAVES + wave; i < n; i += static_cast<int64_t>(gridDim.x) * TK_WAVES) {
        const float *row = x + i * ld;
        float s = 0.0f;
        for (int f = lane; f < F; f += kWave) {
            const float v = row[f];
            s = fmaf(v, v, s);
        }
#pragma unroll
        for (int o = kWave >> 1; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
        if (lane == 0) out[i] = s == 0.0f ? 0.0f : __fdiv_rn(1.0f, __fsqrt_rn(s));
    }
}

unsigned tk_groups(const int64_t rows) { return static_cast<unsigned>(std::min<int64_t>(wdg::ceil_div(rows, TK_WAVES), TK_MAX_GROUPS)); }

}  // namespace

// The per-job part of the contract, on the table the caller still holds on the host (graphs.TopkRowsBatch calls this before it uploads).
extern "C" int wdg_topk_rows_check_jobs(const wdg_topk_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("topk_rows_check_jobs", jobs_host, n_jobs, TK_MAX_JOBS)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_topk_job &j = jobs_host[i];
        WDG_REQUIRE(j.k >= 1 && j.k <= WDG_TOPK_MAX_K, "topk_rows_check_jobs: job %d has k = %d; 1 .. %d are supported", i, j.k, WDG_TOPK_MAX_K);
        WDG_REQUIRE(j.rows >= 0 && j.cols >= 0, "topk_rows_check_jobs: job %d has a negative rows or cols", i);
        WDG_REQUIRE(j.ld >= j.cols, "topk_rows_check_jobs: job %d has ld = %lld below its %d cols", i, static_cast<long long>(j.ld), j.cols);
        WDG_REQUIRE(j.ld_out >= j.k, "topk_rows_check_jobs: job %d has ld_out = %lld below its k = %d", i, static_cast<long long>(j.ld_out), j.k);
        WDG_REQUIRE((j.flags & ~TK_FLAGS) == 0, "topk_rows_check_jobs: job %d has flags %d; WDG_TOPK_EXCLUDE_SELF (1) and WDG_TOPK_SORT_COLUMNS (2) are defined", i,
                    j.flags);
        WDG_REQUIRE(j.out_col && j.out_len, "topk_rows_check_jobs: job %d has a null out_col or out_len", i);
        WDG_REQUIRE(j.scores || j.rows == 0 || j.cols == 0, "topk_rows_check_jobs: job %d has null scores", i);
        WDG_REQUIRE(!tk_malformed(&j), "topk_rows_check_jobs: job %d is malformed", i);
    }
    return WDG_OK;
}

extern "C" int wdg_topk_rows_batched_f32(const wdg_topk_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = wdg::check_job_table("topk_rows_batched_f32", jobs_dev, n_jobs, TK_MAX_JOBS)) return rc;
    WDG_REQUIRE(max_rows >= 0, "topk_rows_batched_f32: negative max_rows");
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    hipLaunchKernelGGL(topk_rows_kernel, dim3(tk_groups(max_rows), static_cast<unsigned>(n_jobs)), dim3(TK_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("topk_rows_batched_f32");
}

extern "C" int wdg_row_rnorm_f32(const float *x, int64_t ld, int32_t n, int32_t F, float *out, wdg_stream_t stream) {
    WDG_REQUIRE(n >= 0 && F >= 0, "row_rnorm_f32: negative n or F");
    WDG_REQUIRE(ld >= F, "row_rnorm_f32: ld = %lld below F = %d", static_cast<long long>(ld), F);
    WDG_REQUIRE(x != nullptr || n == 0 || F == 0, "row_rnorm_f32: null x");
    WDG_REQUIRE(out != nullptr || n == 0, "row_rnorm_f32: null out");
    if (n == 0) return WDG_OK;
    hipLaunchKernelGGL(row_rnorm_kernel, dim3(tk_groups(n)), dim3(TK_THREADS), 0, wdg::as_stream(stream), x, ld, n, F, out);
    return wdg::check_launch("row_rnorm_f32");
}
