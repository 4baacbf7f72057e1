// Predictions and confusion counts of many models whose logits are STACKED along the feature axis (replica r's classes are columns
// r cs .. r cs + C - 1 of one [n, R cs] matrix): per replica and per part of its split (train, validation, test) a
// [C, C + 1] table of (true class, predicted class or "none"), and the prediction of every row.  include/wdg.h states the rule;
// tests/_confusion_ref.py restates it in numpy.
//
// replaces: the accuracy of utils/util_funcs.py:393 taken apart by class, for the models the accuracy tables gnns_on_syn.py:109-154 and
//           gnns_on_syn.py:213-249 train (the loop itself lives upstream of the reference).  It stands in for an argmax, a mask per
//           split part and a bincount per replica.
//
// csrc/stacked_row.h states the layout, the ownership of a (row, replica) pair, its loads and the prediction rule.  A workgroup owns
// CF_ROWS rows of a job and walks the replicas in chunks.  A chunk is as many replicas as CF_LDS_INTS counters hold (3 C (C + 1) per
// replica: 10 replicas of 16 classes, 91 of 5): the workgroup counts in LDS (integer adds) and adds one integer per non-zero counter to
// the job's `counts`.  No floating-point atomics: a sum of integers does not depend on its order.
#include "stacked_row.h"

namespace {

using namespace wdg;

constexpr int CF_ROWS = 64, CF_THREADS = 256, CF_MAX_C = SR_MAX_C, CF_LDS_INTS = 8192;
constexpr int CF_MAX_JOBS = 65535;  // gridDim.z: a job per z
static_assert(3 * CF_MAX_C * (CF_MAX_C + 1) <= CF_LDS_INTS, "a chunk holds at least one replica");

// what the kernel skips: nothing to do, a shape the registers of a thread do not hold, a row narrower than its replicas, a NULL pointer
__host__ __device__ inline bool cf_skipped(const void *logits, const void *labels, const void *split, const void *counts, const int64_t ld,
                                           const int n, const int R, const int C, const int cs) {
    return n <= 0 || R <= 0 || sr_bad_classes(C, cs) || ld < static_cast<int64_t>(R) * cs || !logits || !labels || !split || !counts;
}

__global__ __launch_bounds__(CF_THREADS) void confusion_kernel(const wdg_confusion_job *__restrict__ jobs, const int max_rows) {
    __shared__ int lds[CF_LDS_INTS];  // [replica of the chunk][part][true class][predicted class | none]
    const desc_ptr<wdg_confusion_job> job = (desc_ptr<wdg_confusion_job>)(jobs + blockIdx.z);
    const int R = job->R, C = job->C, cs = job->cs;
    const int64_t ld = job->ld_logits;
    const int i0 = blockIdx.x * CF_ROWS;
    if (cf_skipped(job->logits, job->labels, job->split, job->counts, ld, job->n, R, C, cs)) return;  // (uniform: before any barrier)
    const int n = min(job->n, max_rows);
    if (i0 >= n) return;
    const int rows_here = min(CF_ROWS, n - i0);
    const global_ptr<const float> logits = to_global(job->logits);
    const global_ptr<const int32_t> labels = to_global(job->labels);
    const global_ptr<const uint8_t> split = to_global(job->split);
    const global_ptr<uint8_t> pred_out = to_global(job->pred);
    int32_t *const counts = job->counts;
    const bool has_pred = job->pred != nullptr;
    const bool vec_in = sr_rows16(job->logits, ld, cs);
    const int per = 3 * C * (C + 1);  // counters of a replica
    const int chunk = min(CF_LDS_INTS / per, R);
    const int t = threadIdx.x;
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int rc = min(chunk, R - r0);
        for (int q = t; q < rc * per; q += CF_THREADS) lds[q] = 0;
        __syncthreads();
        for (int q = t; q < rows_here * rc; q += CF_THREADS) {
            const int il = q / rc, rl = q - il * rc;
            const int i = i0 + il, r = r0 + rl;
            const int code = split[static_cast<int64_t>(i) * R + r];
            const int lab = labels[i];
            float z[CF_MAX_C];
            sr_load(z, logits + static_cast<int64_t>(i) * ld + static_cast<int64_t>(r) * cs, C, vec_in);
            const sr_max top = sr_first_max(z, C);
            const int pred = top.nan ? C : top.pred;  // (C: none)
            if (has_pred) pred_out[static_cast<int64_t>(i) * R + r] = static_cast<uint8_t>(top.nan ? 255 : pred);
            if (code >= 1 && code <= 3 && lab >= 0 && lab < C) atomicAdd(&lds[rl * per + ((code - 1) * C + lab) * (C + 1) + pred], 1);
        }
        __syncthreads();
        for (int q = t; q < rc * per; q += CF_THREADS) {  // (the counters of consecutive replicas are consecutive in `counts` as well)
            const int v = lds[q];
            if (v) atomicAdd(counts + static_cast<int64_t>(r0) * per + q, v);
        }
        __syncthreads();  // (the next chunk zeroes the counters)
    }
}

}  // namespace

extern "C" int wdg_confusion_batched_i32(const wdg_confusion_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream) {
    WDG_REQUIRE(max_rows >= 0 && max_cols >= 0, "confusion_batched: negative count");
    if (const int rc = wdg::check_job_table("confusion_batched", jobs_dev, n_jobs, CF_MAX_JOBS)) return rc;
    if (max_cols > CF_MAX_C) return wdg::fail(WDG_ERR_UNSUPPORTED, "confusion_batched: %d classes; the kernel holds %d", max_cols, CF_MAX_C);
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    hipLaunchKernelGGL(confusion_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, CF_ROWS)), 1, static_cast<unsigned>(n_jobs)), dim3(CF_THREADS), 0,
                       wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("confusion_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host: what the kernel would skip, other than an empty job
// (ops.ConfusionBatch calls this on the table it is about to upload).
extern "C" int wdg_confusion_check_jobs(const wdg_confusion_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "confusion_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "confusion_check_jobs: null job table");
    WDG_REQUIRE(n_jobs <= CF_MAX_JOBS, "confusion_check_jobs: %d jobs; one launch takes %d", n_jobs, CF_MAX_JOBS);
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_confusion_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0 && j.R >= 0, "confusion_check_jobs: job %d has a negative shape", i);
        if (j.C > CF_MAX_C) return wdg::fail(WDG_ERR_UNSUPPORTED, "confusion_check_jobs: job %d has %d classes; the kernel holds %d", i, j.C, CF_MAX_C);
        WDG_REQUIRE(j.C >= 1 && j.cs >= j.C, "confusion_check_jobs: job %d has %d classes in a replica stride of %d", i, j.C, j.cs);
        if (j.n == 0 || j.R == 0) continue;
        WDG_REQUIRE(!cf_skipped(j.logits, j.labels, j.split, j.counts, j.ld_logits, j.n, j.R, j.C, j.cs),
                    "confusion_check_jobs: job %d has a null pointer or a leading dimension below its %d x %d columns", i, j.R, j.cs);
    }
    return WDG_OK;
}
