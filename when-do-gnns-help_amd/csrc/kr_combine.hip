// Kernel-regression metric on the device, problems of 9 .. 16 classes: the COMBINE pass over the class windows of a problem
// (include/wdg.h: class windows).  The solvers (csrc/kernel_reg.hip, csrc/kernel_reg_large.hip) carry 8 right-hand sides per job, so
// such a problem is solved as two window jobs, each of which leaves per validation row the first maximum over ITS classes
// (wdg_kr_row_best: value, absolute class id).  Here: the first maximum over the windows in window order - with the windows'
// classes ascending that is the first maximum over all classes, torch.argmax's -, compared with the row's label and counted.
//
// replaces: `.argmax(1).eq(labels[idx_val])` and the accuracy of utils/homophily_metrics.py:283-297 (utils/homophily_plot.py:296-310)
//           over class columns that the window jobs hold apart.
//
//   * kr_combine_kernel  one workgroup of 256 threads per problem, one thread per validation row at a time; integer counts only:
//                        the result does not depend on the order in which the rows are taken.
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int KC_THREADS = 256, KC_MAX_WINDOWS = 2;

__global__ __launch_bounds__(KC_THREADS) void kr_combine_kernel(const wdg_kr_combine_job *__restrict__ jobs) {
    __shared__ int hits;
    const desc_ptr<wdg_kr_combine_job> job = (desc_ptr<wdg_kr_combine_job>)(jobs + blockIdx.x);
    const int tid = threadIdx.x, nv = job->n_val, nw = job->n_windows;
    if (job->correct_out == nullptr) return;  // (uniform)
    const global_ptr<const int32_t> win_correct = to_global(job->win_correct), win_flags = to_global(job->win_flags);
    bool refused = nw < 1 || nw > KC_MAX_WINDOWS || nv < 0 || job->win_correct == nullptr || job->rows == nullptr;
    int flags = 0;
    if (!refused)
        for (int w = 0; w < nw; ++w) {  // (uniform: every thread reads the same few words)
            refused |= win_correct[w] < 0;
            if (job->win_flags != nullptr) flags |= win_flags[w];
        }
    if (refused) {
        if (tid == 0) *to_global(job->correct_out) = -1;
        if (tid == 0 && job->flags_out) *to_global(job->flags_out) = 0;
        return;
    }
    if (tid == 0) hits = 0;
    __syncthreads();
    const global_ptr<const float> rows = to_global(reinterpret_cast<const float *>(job->rows));  // (value, class) pairs: 2 words a row
    const global_ptr<const int32_t> val = to_global(job->val), labels = to_global(job->labels);
    const int64_t stride = job->row_stride;
    int mine = 0;
    for (int v = tid; v < nv; v += KC_THREADS) {
        int best = 0;
        float bv = -3.4e38f;
        for (int w = 0; w < nw; ++w) {
            const int64_t at = 2 * (w * stride + v);
            const float value = rows[at];
            if (value > bv) {  // first maximum: a strictly greater value replaces, NaN never wins
                bv = value;
                best = __builtin_bit_cast(int, rows[at + 1]);
            }
        }
        mine += best == labels[val[v]] ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((tid & 63) == 0 && mine) atomicAdd(&hits, mine);
    __syncthreads();
    if (tid == 0) {
        *to_global(job->correct_out) = hits;
        if (job->flags_out) *to_global(job->flags_out) = flags;
    }
}

}  // namespace

extern "C" {

int wdg_kr_combine_windows_batched(const wdg_kr_combine_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "kr_combine_windows_batched: negative size");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "kr_combine_windows_batched: null job table");
    hipLaunchKernelGGL(kr_combine_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(KC_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("kr_combine_kernel");
}

}  // extern "C"
