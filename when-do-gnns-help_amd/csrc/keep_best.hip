// Keep the selected model of a stacked run: of every tensor of a table, the segments of the replicas whose best epoch is the current
// step are copied from src to dst, in one launch (include/wdg.h states the rule; tests/_keep_ref.py restates it in numpy).  The
// selection (wdg_xent_job.best) and the step word are read from device memory: a captured epoch keeps its best model with no host in it.
//
// replaces: the bookkeeping of the training loops behind the accuracy tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the
//           loop itself lives upstream of the reference, where it keeps the selected model): what xent_eval.hip cites.  It stands in
//           for a read-back of `best` and a torch.where over every stacked parameter, which would put the host into the epoch.
//
// Ownership as in adam.hip: a workgroup of 256 threads owns a 64 x 64 tile of one job; thread (row slot t >> 4, column group t & 15)
// works on four adjacent columns of the rows slot, slot + 16, slot + 32, slot + 48.  A job whose pointers are 16-byte aligned and
// whose seg_cols and leading dimensions are multiples of 4 moves a selected group as one 16-byte load and one 16-byte store (the four
// columns share a segment then); any other job, and a ragged right edge, goes word by word.  The words are moved as integers:
// nothing can quieten a NaN or lose the sign of a zero.  No LDS, no atomics: 8 bytes move per selected element, none for the others.
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int KB_TILE = 64, KB_THREADS = 256;
constexpr int KB_MAX_JOBS = 65535;       // gridDim.z: a job per z
constexpr int KB_MAX_COL_TILES = 65535;  // gridDim.y

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// whether two [rows, cols] views may share a byte: their byte ranges intersect, unless both have one leading dimension and their
// column ranges are disjoint inside it (column ranges of one wider matrix)
__host__ __device__ inline bool kb_overlap(const uintptr_t a, const int64_t lda, const uintptr_t b, const int64_t ldb, const int64_t rows,
                                           const int64_t cols) {
    const uintptr_t na = static_cast<uintptr_t>(((rows - 1) * lda + cols) * 4), nb = static_cast<uintptr_t>(((rows - 1) * ldb + cols) * 4);
    if (a + na <= b || b + nb <= a) return false;
    if (rows > 1 && lda == ldb) {
        const uintptr_t pitch = static_cast<uintptr_t>(lda) * 4, w = static_cast<uintptr_t>(cols) * 4;
        const uintptr_t delta = b >= a ? (b - a) % pitch : (pitch - (a - b) % pitch) % pitch;
        return delta < w || delta + w > pitch;
    }
    return true;
}

// the per-job part of the contract: what the kernel skips and wdg_keep_best_check_jobs refuses (a job of 0 rows or 0 columns is
// well-formed and empty)
template <typename Job>
__host__ __device__ inline bool kb_malformed(const Job &j) {
    if (j.rows <= 0 || j.cols <= 0) return j.rows < 0 || j.cols < 0;
    if (j.seg_rows < 1 || j.seg_cols < 1 || j.reps < 1 || j.ld_src < j.cols || j.ld_dst < j.cols) return true;
    if (j.src == nullptr || j.dst == nullptr || j.best == nullptr) return true;
    return kb_overlap(reinterpret_cast<uintptr_t>(j.src), j.ld_src, reinterpret_cast<uintptr_t>(j.dst), j.ld_dst, j.rows, j.cols);
}

__global__ __launch_bounds__(KB_THREADS) void keep_best_kernel(const wdg_keep_job *__restrict__ jobs, const int max_rows, const int max_cols,
                                                               const int32_t *__restrict__ step_dev) {
    const desc_ptr<wdg_keep_job> jp = (desc_ptr<wdg_keep_job>)(jobs + blockIdx.z);
    wdg_keep_job job;  // (uniform: the fields arrive by scalar loads)
    job.src = jp->src, job.dst = jp->dst, job.best = jp->best, job.ld_src = jp->ld_src, job.ld_dst = jp->ld_dst;
    job.rows = jp->rows, job.cols = jp->cols, job.seg_rows = jp->seg_rows, job.seg_cols = jp->seg_cols, job.reps = jp->reps, job.reserved = 0;
    const int rows = min(job.rows, max_rows), cols = job.cols;
    const int r0 = blockIdx.x * KB_TILE, c0 = blockIdx.y * KB_TILE;
    if (r0 >= rows || c0 >= cols || cols > max_cols) return;
    if (kb_malformed(job)) return;  // (a job outside the contract is left untouched)
    const int seg_rows = job.seg_rows, seg_cols = job.seg_cols, reps = job.reps;
    const int64_t ld_src = job.ld_src, ld_dst = job.ld_dst;
    const global_ptr<const uint32_t> src = (global_ptr<const uint32_t>)job.src;
    const global_ptr<uint32_t> dst = (global_ptr<uint32_t>)job.dst;
    const global_ptr<const int32_t> best = to_global(job.best);
    // (uniform) 16-byte accesses: both pointers, both leading dimensions, and four adjacent columns in one segment
    const bool vec = ((reinterpret_cast<uintptr_t>(job.src) | reinterpret_cast<uintptr_t>(job.dst) | static_cast<uintptr_t>(ld_src * 4) |
                       static_cast<uintptr_t>(ld_dst * 4)) & 15) == 0 && (seg_cols & 3) == 0;
    const int t = threadIdx.x, gq = t & 15, rr = t >> 4;
    const int c = c0 + 4 * gq;
    if (c >= cols) return;
    const int32_t step = *step_dev;
    const int64_t segs_per_row = (cols + seg_cols - 1) / seg_cols;
    int cseg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cseg[k] = min(c + k, cols - 1) / seg_cols;
    int64_t cur = -1;  // the segment whose answer is in `selected`
    bool selected = false;
#pragma unroll
    for (int i = 0; i < KB_TILE / 16; ++i) {
        const int r = r0 + rr + 16 * i;
        if (r >= rows) continue;
        const int64_t rseg = static_cast<int64_t>(r / seg_rows) * segs_per_row;
        const global_ptr<const uint32_t> s = src + static_cast<int64_t>(r) * ld_src + c;
        const global_ptr<uint32_t> d = dst + static_cast<int64_t>(r) * ld_dst + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c + k >= cols) continue;
            const int64_t seg = rseg + cseg[k];
            if (seg != cur) {
                cur = seg;
                const int64_t rep = seg % reps;
                selected = best[3 * rep] >= 0 && best[3 * rep + 2] == step;
            }
            if (!selected) continue;
            if (k == 0 && vec && c + 3 < cols) {  // (cseg[0 .. 3] are one segment: seg_cols and c are multiples of 4)
                *(global_ptr<u32x4_t>)d = *(global_ptr<const u32x4_t>)s;
                break;
            }
            d[k] = s[k];
        }
    }
}

}  // namespace

extern "C" int wdg_keep_best_batched_f32(const wdg_keep_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                         const int32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "keep_best_batched: negative count");
    WDG_REQUIRE(step_dev != nullptr, "keep_best_batched: null step word");
    WDG_REQUIRE(n_jobs <= KB_MAX_JOBS, "keep_best_batched: %d jobs; one launch takes %d", n_jobs, KB_MAX_JOBS);
    WDG_REQUIRE(wdg::ceil_div(max_cols, KB_TILE) <= KB_MAX_COL_TILES, "keep_best_batched: %d columns; one launch takes %d", max_cols,
                KB_TILE * KB_MAX_COL_TILES);
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "keep_best_batched: null job table");
    if (max_rows == 0 || max_cols == 0) return WDG_OK;
    hipLaunchKernelGGL(keep_best_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, KB_TILE)), static_cast<unsigned>(wdg::ceil_div(max_cols, KB_TILE)),
                                              static_cast<unsigned>(n_jobs)),
                       dim3(KB_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols, step_dev);
    return wdg::check_launch("keep_best_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host: the predicate the kernel skips a job by
// (ops.KeepBestBatch calls this on the table it is about to upload).
extern "C" int wdg_keep_best_check_jobs(const wdg_keep_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "keep_best_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "keep_best_check_jobs: null job table");
    WDG_REQUIRE(n_jobs <= KB_MAX_JOBS, "keep_best_check_jobs: %d jobs; one launch takes %d", n_jobs, KB_MAX_JOBS);
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_keep_job &j = jobs_host[i];
        WDG_REQUIRE(j.rows >= 0 && j.cols >= 0, "keep_best_check_jobs: job %d has a negative shape", i);
        if (j.rows == 0 || j.cols == 0) continue;
        WDG_REQUIRE(j.seg_rows >= 1 && j.seg_cols >= 1 && j.reps >= 1, "keep_best_check_jobs: job %d has segments of %d x %d and %d replicas", i,
                    j.seg_rows, j.seg_cols, j.reps);
        WDG_REQUIRE(j.ld_src >= j.cols && j.ld_dst >= j.cols, "keep_best_check_jobs: job %d has a leading dimension below its %d columns", i, j.cols);
        WDG_REQUIRE(j.src && j.dst && j.best, "keep_best_check_jobs: job %d has a null pointer", i);
        WDG_REQUIRE(!kb_malformed(j), "keep_best_check_jobs: src and dst of job %d overlap", i);
    }
    return WDG_OK;
}
