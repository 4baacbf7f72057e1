// The tail of a training epoch for many models whose logits are STACKED along the feature axis (all splits of one graph: replica r's
// classes are columns r cs .. r cs + C - 1 of one [n, R cs] matrix): the cross-entropy gradient of the train rows, the validation
// and test hits, and the model selection of every replica, in one pass over the logits.
//
// replaces: the accuracy of utils/util_funcs.py:393 and the loss / accuracy bookkeeping of the training loops behind the accuracy
//           tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the loop itself lives upstream of the reference).  It stands in
//           for the softmax / scatter / argmax / gather / where launches of sweep.TrainBatch.train_step and eval_step, which need
//           a [J, n, c] layout and splits of equal length.
//
// csrc/stacked_row.h states the layout, the ownership of a (row, replica) pair, its loads and the prediction rule.  A workgroup owns
// XE_ROWS rows of a job and walks the replicas in chunks of XE_RCHUNK: the hits of a chunk are counted in LDS (integer adds) and one
// integer per workgroup and non-zero counter is added to the job's `hits`.  A second launch of the same call compares, records and
// zeroes them.  No floating-point atomics: a pair's gradient depends on its own C logits alone, and a sum of integers does not depend
// on its order.
#include "stacked_row.h"

namespace {

using namespace wdg;

constexpr int XE_ROWS = 64, XE_THREADS = 256, XE_RCHUNK = 256, XE_MAX_C = SR_MAX_C;
constexpr int XE_MAX_JOBS = 65535;  // gridDim.z: a job per z

// what both launches skip: nothing to do, or a shape the registers of a thread do not hold (the entry refuses max_cols > 16; a job
// that lies about its own C must still not be indexed out of bounds)
__device__ __forceinline__ bool xe_skipped(const int n, const int R, const int C, const int cs) {
    return n <= 0 || R <= 0 || sr_bad_classes(C, cs);
}

template <bool GRAD, bool EVAL>
__global__ __launch_bounds__(XE_THREADS) void xent_eval_kernel(const wdg_xent_job *__restrict__ jobs) {
    __shared__ int counts[2 * XE_RCHUNK];  // [validation | test] hits of the replicas of the current chunk
    const desc_ptr<wdg_xent_job> job = (desc_ptr<wdg_xent_job>)(jobs + blockIdx.z);
    const int n = job->n, R = job->R, C = job->C, cs = job->cs;
    const int i0 = blockIdx.x * XE_ROWS;
    if (xe_skipped(n, R, C, cs) || i0 >= n) return;  // (uniform: before any barrier)
    const int rows_here = min(XE_ROWS, n - i0);
    const global_ptr<const float> logits = to_global(job->logits);
    const global_ptr<float> dlogits = to_global(job->dlogits);
    const global_ptr<const int32_t> labels = to_global(job->labels);
    const global_ptr<const uint8_t> split = to_global(job->split);
    const global_ptr<const float> inv_n_train = to_global(job->inv_n_train);
    const int64_t ld = job->ld_logits, ldd = job->ld_dlogits;
    // (uniform) 16-byte accesses where the job's pointers, leading dimensions and replica stride allow
    const bool vec_in = sr_rows16(job->logits, ld, cs), vec_out = GRAD && sr_rows16(job->dlogits, ldd, cs);
    const int t = threadIdx.x;
    for (int r0 = 0; r0 < R; r0 += XE_RCHUNK) {
        const int rc = min(XE_RCHUNK, R - r0);
        if (EVAL) {
            counts[t] = 0;
            counts[XE_RCHUNK + t] = 0;
            __syncthreads();
        }
        for (int q = t; q < rows_here * rc; q += XE_THREADS) {
            const int il = q / rc, rl = q - il * rc;
            const int i = i0 + il, r = r0 + rl;
            const int code = split[static_cast<int64_t>(i) * R + r];
            const bool train = GRAD && code == 1, scored = EVAL && (code == 2 || code == 3);
            const int lab = labels[i];
            float z[XE_MAX_C];
            if (train || scored) sr_load(z, logits + static_cast<int64_t>(i) * ld + static_cast<int64_t>(r) * cs, C, vec_in);
            if (scored) {
                const sr_max top = sr_first_max(z, C);
                if (!top.nan && top.pred == lab) atomicAdd(&counts[(code == 3 ? XE_RCHUNK : 0) + rl], 1);
            }
            if (GRAD) {
                float o[XE_MAX_C];
#pragma unroll
                for (int k = 0; k < XE_MAX_C; ++k) o[k] = 0.f;
                if (train) {
                    const float s = sr_exp_sum(z, C, sr_first_max(z, C).m);  // (a NaN among the logits makes s a NaN)
                    const float inv = inv_n_train[r];
#pragma unroll
                    for (int k = 0; k < XE_MAX_C; ++k)
                        if (k < C) o[k] = (z[k] / s - (k == lab ? 1.f : 0.f)) * inv;
                }
                // all cs columns of the replica: the gradient (or +0) and +0 in the padding - the backward aggregation reads whole rows
                const global_ptr<float> d = dlogits + static_cast<int64_t>(i) * ldd + static_cast<int64_t>(r) * cs;
#pragma unroll
                for (int g = 0; g < XE_MAX_C / 4; ++g) {
                    if (4 * g >= cs) continue;
                    if (vec_out) {
                        store_f32x4(d + 4 * g, make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]));
                    } else {
#pragma unroll
                        for (int k = 4 * g; k < 4 * g + 4; ++k)
                            if (k < cs) d[k] = o[k];
                    }
                }
                for (int k = XE_MAX_C; k < cs; ++k) d[k] = 0.f;
            }
        }
        if (EVAL) {
            __syncthreads();
            if (t < rc) {
                const int hv = counts[t], ht = counts[XE_RCHUNK + t];
                if (hv) atomicAdd(job->hits + 2 * (r0 + t), hv);
                if (ht) atomicAdd(job->hits + 2 * (r0 + t) + 1, ht);
            }
            __syncthreads();  // (the next chunk zeroes the counters)
        }
    }
}

// after every row is counted: a replica whose validation hits beat its best (strictly) records them, its test hits and the step
// word; the counters go back to zero for the next call
__global__ __launch_bounds__(XE_THREADS) void xent_select_kernel(const wdg_xent_job *__restrict__ jobs, const int32_t *__restrict__ step_dev) {
    const desc_ptr<wdg_xent_job> job = (desc_ptr<wdg_xent_job>)(jobs + blockIdx.x);
    const int R = job->R;
    if (xe_skipped(job->n, R, job->C, job->cs)) return;
    const global_ptr<int32_t> hits = to_global(job->hits), best = to_global(job->best);
    const int32_t step = *step_dev;
    for (int r = threadIdx.x; r < R; r += XE_THREADS) {
        const int32_t hv = hits[2 * r], ht = hits[2 * r + 1];
        if (hv > best[3 * r]) {
            best[3 * r] = hv;
            best[3 * r + 1] = ht;
            best[3 * r + 2] = step;
        }
        hits[2 * r] = 0;
        hits[2 * r + 1] = 0;
    }
}

}  // namespace

extern "C" int wdg_xent_eval_batched_f32(const wdg_xent_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, int32_t flags,
                                         const int32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "xent_eval_batched: negative count");
    WDG_REQUIRE(flags >= 1 && flags <= (WDG_XENT_GRAD | WDG_XENT_EVAL), "xent_eval_batched: flags %d; WDG_XENT_GRAD, WDG_XENT_EVAL or both", flags);
    WDG_REQUIRE(!(flags & WDG_XENT_EVAL) || step_dev != nullptr, "xent_eval_batched: null step word");
    WDG_REQUIRE(n_jobs <= XE_MAX_JOBS, "xent_eval_batched: %d jobs; one launch takes %d", n_jobs, XE_MAX_JOBS);
    WDG_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "xent_eval_batched: null job table");
    if (max_cols > XE_MAX_C) return wdg::fail(WDG_ERR_UNSUPPORTED, "xent_eval_batched: %d classes; the kernel holds %d", max_cols, XE_MAX_C);
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, XE_ROWS)), 1, static_cast<unsigned>(n_jobs));
    const hipStream_t st = wdg::as_stream(stream);
    if (flags == WDG_XENT_GRAD)
        hipLaunchKernelGGL((xent_eval_kernel<true, false>), grid, dim3(XE_THREADS), 0, st, jobs_dev);
    else if (flags == WDG_XENT_EVAL)
        hipLaunchKernelGGL((xent_eval_kernel<false, true>), grid, dim3(XE_THREADS), 0, st, jobs_dev);
    else
        hipLaunchKernelGGL((xent_eval_kernel<true, true>), grid, dim3(XE_THREADS), 0, st, jobs_dev);
    int rc = wdg::check_launch("xent_eval_kernel");
    if (rc != WDG_OK || !(flags & WDG_XENT_EVAL)) return rc;
    hipLaunchKernelGGL(xent_select_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(XE_THREADS), 0, st, jobs_dev, step_dev);
    return wdg::check_launch("xent_select_kernel");
}
