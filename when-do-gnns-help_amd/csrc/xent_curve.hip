// The evaluation of a training epoch for many models whose logits are STACKED along the feature axis (wdg_xent_eval_batched_f32's
// layout: replica r's classes are columns r cs .. r cs + C - 1 of one [n, R cs] matrix) WITH the losses: per replica the mean
// cross-entropy and the hits of its train, validation and test rows, a row of its learning curve, its model selection by one of
// three rules and its patience counter - on the device, so that a captured epoch needs no host.
//
// replaces: the accuracy of utils/util_funcs.py:393 and the loss / accuracy / early-stopping bookkeeping of the training loops behind
//           the accuracy tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the loop itself lives upstream of the reference).
//           It stands in for wdg_xent_eval_batched_f32's WDG_XENT_EVAL call where a run asks for losses, another selection rule, a
//           patience or a learning curve.
//
// csrc/stacked_row.h states the layout, the ownership of a (row, replica) pair, its loads and the prediction rule.  A workgroup
// owns XC_ROWS rows of a job and walks the replicas in chunks of XC_RCHUNK: every pair leaves its fp32 loss term and a mark (its
// part, whether it counts, whether it is a hit) in LDS; then one thread per replica walks the chunk's rows in ASCENDING order and adds
// the widened terms of each part in fp64 - one partial per (row block, replica, part), stored, not added.  The finishing launch adds
// a replica's partials in ascending block order, divides, writes the curve row, selects and counts patience.  No floating-point
// atomic anywhere: the order of the sum is a function of the job's own n; the hits are integers.
#include "stacked_row.h"

#include <cmath>

namespace {

using namespace wdg;

constexpr int XC_ROWS = 32, XC_THREADS = 256, XC_RCHUNK = 256, XC_MAX_C = SR_MAX_C;
constexpr int XC_MAX_JOBS = 65535;  // gridDim.z: a job per z
constexpr unsigned XC_COUNTS = 4, XC_HIT = 8;  // a pair's mark: its split code (1 .. 3) | the term counts | the row is a hit

// what both launches skip and wdg_xent_curve_check_jobs refuses (one predicate): nothing to do, a shape the registers of a thread do
// not hold, a row narrower than its replicas, a rule or a patience outside the definition, a curve without its buffers, a NULL pointer
template <typename J>
__host__ __device__ __forceinline__ bool xc_empty(const J job) {
    return job->n <= 0 || job->R <= 0;
}
template <typename J>
__host__ __device__ __forceinline__ bool xc_malformed(const J job) {
    return job->n < 0 || job->R < 0 || sr_bad_classes(job->C, job->cs) ||
           (job->n > 1 && job->ld_logits < static_cast<int64_t>(job->R) * job->cs) || job->rule < 0 || job->rule > 2 || job->patience < 0 ||
           job->curve_rows < 0 || (job->curve_rows > 0 && (job->curve_loss == nullptr || job->curve_hits == nullptr)) ||
           (job->n > 0 && job->R > 0 && (job->logits == nullptr || job->labels == nullptr || job->split == nullptr || job->n_part == nullptr ||
                                         job->best == nullptr || job->best_loss == nullptr || job->state == nullptr || job->hits == nullptr ||
                                         job->partials == nullptr));
}

__global__ __launch_bounds__(XC_THREADS) void xent_curve_kernel(const wdg_xent_curve_job *__restrict__ jobs) {
    __shared__ float terms[XC_ROWS * XC_RCHUNK];
    __shared__ uint8_t marks[XC_ROWS * XC_RCHUNK];
    const desc_ptr<wdg_xent_curve_job> job = (desc_ptr<wdg_xent_curve_job>)(jobs + blockIdx.z);
    const int n = job->n, R = job->R, C = job->C, cs = job->cs;
    const int i0 = blockIdx.x * XC_ROWS;
    if (xc_malformed(job) || xc_empty(job) || i0 >= n) return;  // (uniform: before any barrier)
    const int rows_here = min(XC_ROWS, n - i0);
    const global_ptr<const float> logits = to_global(job->logits);
    const global_ptr<const int32_t> labels = to_global(job->labels);
    const global_ptr<const uint8_t> split = to_global(job->split);
    const global_ptr<double> partials = to_global(job->partials);
    const int64_t ld = job->ld_logits;
    const bool vec_in = sr_rows16(job->logits, ld, cs);
    const int t = threadIdx.x;
    for (int r0 = 0; r0 < R; r0 += XC_RCHUNK) {
        const int rc = min(XC_RCHUNK, R - r0);
        for (int q = t; q < rows_here * rc; q += XC_THREADS) {  // (q = il * rc + rl: the pair's place in LDS as well)
            const int il = q / rc, rl = q - il * rc;
            const int i = i0 + il, r = r0 + rl;
            const unsigned code = split[static_cast<int64_t>(i) * R + r];
            const int lab = labels[i];
            float term = 0.f;
            unsigned mark = 0;
            if (code >= 1 && code <= 3) {  // (the padding columns C .. cs - 1 are never read)
                float z[XC_MAX_C];
                sr_load(z, logits + static_cast<int64_t>(i) * ld + static_cast<int64_t>(r) * cs, C, vec_in);
                const sr_max top = sr_first_max(z, C);
                mark = code;
                if (!top.nan && top.pred == lab) mark |= XC_HIT;
                if (lab >= 0 && lab < C) {  // (a label outside 0 .. C - 1 adds nothing)
                    float zl = z[0];  // z[lab], by compile-time indices: the array stays in registers
#pragma unroll
                    for (int k = 1; k < XC_MAX_C; ++k)
                        if (k == lab) zl = z[k];
                    term = logf(sr_exp_sum(z, C, top.m)) - (zl - top.m);
                    mark |= XC_COUNTS;
                }
            }
            terms[q] = term;
            marks[q] = static_cast<uint8_t>(mark);
        }
        __syncthreads();
        if (t < rc) {
            // replica r0 + t: the rows of this block in ascending order, a part's terms widened and added in fp64
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            int h0 = 0, h1 = 0, h2 = 0;
            for (int il = 0; il < rows_here; ++il) {
                const unsigned mk = marks[il * rc + t];
                const double v = static_cast<double>(terms[il * rc + t]);
                const unsigned part = mk & 3u;
                const bool counts = (mk & XC_COUNTS) != 0;
                const int hit = (mk & XC_HIT) ? 1 : 0;
                if (part == 1) {
                    if (counts) s0 += v;
                    h0 += hit;
                } else if (part == 2) {
                    if (counts) s1 += v;
                    h1 += hit;
                } else if (part == 3) {
                    if (counts) s2 += v;
                    h2 += hit;
                }
            }
            const int r = r0 + t;
            const global_ptr<double> out = partials + (static_cast<int64_t>(blockIdx.x) * R + r) * 3;
            out[0] = s0, out[1] = s1, out[2] = s2;  // (all three, every call: the finishing launch reads every block of the job)
            if (h0) atomicAdd(job->hits + 3 * r, h0);
            if (h1) atomicAdd(job->hits + 3 * r + 1, h1);
            if (h2) atomicAdd(job->hits + 3 * r + 2, h2);
        }
        __syncthreads();  // (the next chunk overwrites the terms)
    }
}

// after every row block has left its partials: a replica's sums in ascending block order, its means, its curve row, its selection and
// its patience; the hit counters go back to zero for the next call.  A workgroup owns a job and walks its replicas XC_FIN_REPS at a
// time: one thread per (replica, part) adds that pair's partials - the loads of XC_FIN_AHEAD blocks are in flight together, the adds
// stay in block order - and leaves the mean and the hits in LDS; then one thread per replica selects.
constexpr int XC_FIN_REPS = 85, XC_FIN_AHEAD = 16;  // 85 replicas x 3 parts = 255 of the 256 threads
__global__ __launch_bounds__(XC_THREADS) void xent_curve_finish_kernel(const wdg_xent_curve_job *__restrict__ jobs, const int32_t *__restrict__ step_dev) {
    __shared__ float mean[3 * XC_FIN_REPS];
    __shared__ int32_t count[3 * XC_FIN_REPS];
    const desc_ptr<wdg_xent_curve_job> job = (desc_ptr<wdg_xent_curve_job>)(jobs + blockIdx.x);
    if (xc_malformed(job) || xc_empty(job)) return;  // (uniform: before any barrier)
    const int n = job->n, R = job->R, rule = job->rule, patience = job->patience, curve_rows = job->curve_rows;
    const int blocks = (n + XC_ROWS - 1) / XC_ROWS;
    const global_ptr<const double> partials = to_global(job->partials);
    const global_ptr<const int32_t> n_part = to_global(job->n_part);
    const global_ptr<int32_t> hits = to_global(job->hits), best = to_global(job->best), state = to_global(job->state);
    const global_ptr<float> best_loss = to_global(job->best_loss), curve_loss = to_global(job->curve_loss);
    const global_ptr<int32_t> curve_hits = to_global(job->curve_hits);
    const int32_t step = *step_dev;
    const bool curve = step >= 0 && step < curve_rows;
    const int t = threadIdx.x;
    const int64_t pairs = static_cast<int64_t>(R) * 3;  // (a block's partials: [R, 3], pair e = 3 r + p)
    for (int r0 = 0; r0 < R; r0 += XC_FIN_REPS) {
        const int rc = min(XC_FIN_REPS, R - r0);
        if (t < 3 * rc) {
            const int64_t e = static_cast<int64_t>(r0) * 3 + t;
            double s = 0.0;
            for (int b0 = 0; b0 < blocks; b0 += XC_FIN_AHEAD) {
                double v[XC_FIN_AHEAD];
#pragma unroll
                for (int u = 0; u < XC_FIN_AHEAD; ++u) v[u] = b0 + u < blocks ? partials[(b0 + u) * pairs + e] : 0.0;
#pragma unroll
                for (int u = 0; u < XC_FIN_AHEAD; ++u)
                    if (b0 + u < blocks) s += v[u];
            }
            const int32_t rows = n_part[e];
            const float loss = rows > 0 ? static_cast<float>(s / static_cast<double>(rows)) : __builtin_nanf("");
            const int32_t h = hits[e];
            hits[e] = 0;
            if (curve) {
                const int64_t at = static_cast<int64_t>(step) * pairs + e;
                curve_loss[at] = loss, curve_hits[at] = h;
            }
            mean[t] = loss, count[t] = h;
        }
        __syncthreads();
        const int r = r0 + t;
        if (t < rc && state[2 * r + 1] < 0) {  // (a stopped replica's best, best_loss and state never change again)
            const int32_t hv = count[3 * t + 1], best_hits = best[3 * r];
            const float lv = mean[3 * t + 1], best_val = best_loss[3 * r + 1];
            // (a NaN makes every comparison false)
            const bool more = hv > best_hits, lower = lv < best_val;
            const bool improved = rule == 0 ? more : rule == 1 ? lower : (more || (hv == best_hits && lower));
            int32_t bad = state[2 * r];
            if (improved) {
                best[3 * r] = hv, best[3 * r + 1] = count[3 * t + 2], best[3 * r + 2] = step;
#pragma unroll
                for (int p = 0; p < 3; ++p) best_loss[3 * r + p] = mean[3 * t + p];
                bad = 0;
            } else {
                bad += 1;
            }
            state[2 * r] = bad;
            if (patience > 0 && bad >= patience) state[2 * r + 1] = step;
        }
        __syncthreads();  // (the next replicas overwrite the means)
    }
}

}  // namespace

extern "C" int64_t wdg_xent_curve_partials_len(int32_t n, int32_t R) {
    if (n <= 0 || R <= 0) return 0;
    return wdg::ceil_div(n, XC_ROWS) * R * 3;
}

extern "C" int wdg_xent_curve_check_jobs(const wdg_xent_curve_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "xent_curve_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "xent_curve_check_jobs: null job table");
    for (int32_t j = 0; j < n_jobs; ++j) {
        const wdg_xent_curve_job *job = jobs_host + j;
        WDG_REQUIRE(job->rule >= 0 && job->rule <= 2, "xent_curve_check_jobs: job %d: rule %d; 0 (val_hits), 1 (val_loss) or 2 (val_hits_then_loss)", j, job->rule);
        WDG_REQUIRE(job->patience >= 0, "xent_curve_check_jobs: job %d: a patience of %d", j, job->patience);
        WDG_REQUIRE(job->curve_rows >= 0, "xent_curve_check_jobs: job %d: %d curve rows", j, job->curve_rows);
        WDG_REQUIRE(!xc_malformed(job), "xent_curve_check_jobs: job %d: n %d, R %d, C %d, cs %d, ld_logits %lld: C in 1..%d, cs >= C, a row of R cs columns, "
                    "no NULL pointer and both curve buffers with curve_rows > 0 expected", j, job->n, job->R, job->C, job->cs,
                    static_cast<long long>(job->ld_logits), XC_MAX_C);
    }
    return WDG_OK;
}

extern "C" int wdg_xent_curve_batched_f32(const wdg_xent_curve_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                          const int32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "xent_curve_batched: negative count");
    WDG_REQUIRE(step_dev != nullptr, "xent_curve_batched: null step word");
    WDG_REQUIRE(n_jobs <= XC_MAX_JOBS, "xent_curve_batched: %d jobs; one launch takes %d", n_jobs, XC_MAX_JOBS);
    WDG_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "xent_curve_batched: null job table");
    if (max_cols > XC_MAX_C) return wdg::fail(WDG_ERR_UNSUPPORTED, "xent_curve_batched: %d classes; the kernel holds %d", max_cols, XC_MAX_C);
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const hipStream_t st = wdg::as_stream(stream);
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, XC_ROWS)), 1, static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(xent_curve_kernel, grid, dim3(XC_THREADS), 0, st, jobs_dev);
    const int rc = wdg::check_launch("xent_curve_kernel");
    if (rc != WDG_OK) return rc;
    hipLaunchKernelGGL(xent_curve_finish_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(XC_THREADS), 0, st, jobs_dev, step_dev);
    return wdg::check_launch("xent_curve_finish_kernel");
}
