// The Adam step of every parameter tensor of a stacked run in one launch, with the learning rate and the weight decay of each
// SEGMENT of a tensor (a replica's column block of w0 / w, a replica's row block of w1) read from device memory, and the step count
// read from the run's step word.  include/wdg.h states the arithmetic; tests/_adam_ref.py restates it in numpy, bit for bit.
//
// replaces: the optimiser step of the training loops behind the accuracy tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the
//           loop itself lives upstream of the reference, which has no model code): torch.optim.Adam with the L2 term in the gradient.
//           In split_train.SplitTrainBatch(optimizer="device") it stands in for the fused torch Adam over the stacked parameters,
//           which has one lr and one weight_decay per tensor.
//
// Ownership as in dropout.hip: a workgroup of 256 threads owns a 64 x 64 tile of one job; thread (row slot t >> 4, column group
// t & 15) works on four adjacent columns of the rows slot, slot + 16, slot + 32, slot + 48, so the 16 lanes of a row cover 256
// contiguous bytes of it: one 16-byte access per lane and operand where the operand's pointer and leading dimension allow, scalar
// accesses elsewhere and at a ragged right edge.  Both paths run ad_element() on the same values: the same bits.
// 28 bytes move per element (p, g, m, v in; p, m, v out) against some twenty operations: the launch is bound by memory bandwidth.
// The fp64 work is per LAUNCH (the two powers beta^t, every thread for itself: a few dozen multiplies) and per SEGMENT RUN (the
// division behind step_size): a thread's column group lies in one segment whenever seg_cols is a multiple of 4 - every trainer
// layout - and then the division happens once per row-segment change, at most four times per thread.
// No atomics, no sums: an element depends on its own four inputs, its segment's two numbers and t.
#include "ipow.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // every multiply and add below is its own correctly rounded operation: numpy restates the bits

namespace {

using namespace wdg;

constexpr int AD_TILE = 64, AD_THREADS = 256;
constexpr int AD_MAX_JOBS = 65535;       // gridDim.z: a job per z
constexpr int AD_MAX_COL_TILES = 65535;  // gridDim.y

struct ad_mat {  // one [rows, cols] operand of a job
    global_ptr<float> p;
    int64_t ld;
    bool vec;  // 16-byte rows: pointer and leading dimension
};
__device__ __forceinline__ ad_mat ad_operand(const float *p, const int64_t ld) {
    return ad_mat{to_global(const_cast<float *>(p)), ld, ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(ld * 4)) & 15) == 0};
}
// columns c .. c + 3 of row r (c < cols); columns at or past `cols` read as +0 and are never written
__device__ __forceinline__ void ad_load4(const ad_mat &a, const int r, const int c, const int cols, float (&x)[4]) {
    const global_ptr<float> p = a.p + static_cast<int64_t>(r) * a.ld + c;
    if (a.vec && c + 3 < cols) {
        const float4 in = load_f32x4(p);
        x[0] = in.x, x[1] = in.y, x[2] = in.z, x[3] = in.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = c + k < cols ? p[k] : 0.f;
    }
}
__device__ __forceinline__ void ad_store4(const ad_mat &a, const int r, const int c, const int cols, const float (&x)[4]) {
    const global_ptr<float> p = a.p + static_cast<int64_t>(r) * a.ld + c;
    if (a.vec && c + 3 < cols) {
        store_f32x4(p, make_float4(x[0], x[1], x[2], x[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c + k < cols) p[k] = x[k];
    }
}

// the contract of include/wdg.h for one element, one rounded operation per line
__device__ __forceinline__ void ad_element(float &p, const float g, float &m, float &v, const float weight_decay, const float step_size,
                                           const float beta1, const float beta2, const float one_minus_beta1, const float one_minus_beta2,
                                           const float bc2_sqrt, const float eps) {
    const float decay = weight_decay * p;
    const float g1 = g + decay;
    const float m_old = beta1 * m;
    const float m_new = one_minus_beta1 * g1;
    m = m_old + m_new;
    const float v_old = beta2 * v;
    float v_new = one_minus_beta2 * g1;
    v_new = v_new * g1;
    v = v_old + v_new;
    float den = sqrtf(v);
    den = den / bc2_sqrt;
    den = den + eps;
    const float ratio = m / den;
    const float delta = step_size * ratio;
    p = p - delta;
}

__global__ __launch_bounds__(AD_THREADS) void adam_kernel(const wdg_adam_job *__restrict__ jobs, const int max_rows, const int max_cols,
                                                          const float beta1, const float beta2, const float eps,
                                                          const int32_t *__restrict__ step_dev) {
    const desc_ptr<wdg_adam_job> job = (desc_ptr<wdg_adam_job>)(jobs + blockIdx.z);
    const int rows = min(job->rows, max_rows), cols = job->cols;
    const int seg_rows = job->seg_rows, seg_cols = job->seg_cols;
    const int r0 = blockIdx.x * AD_TILE, c0 = blockIdx.y * AD_TILE;
    if (r0 >= rows || c0 >= cols || cols > max_cols) return;
    if (seg_rows < 1 || seg_cols < 1 || job->ld < cols || job->ld_s < cols) return;  // (a job outside the contract is left untouched)
    const ad_mat P = ad_operand(job->p, job->ld), G = ad_operand(job->g, job->ld), M = ad_operand(job->m, job->ld_s),
                 V = ad_operand(job->v, job->ld_s);
    const global_ptr<const float> hyper = to_global(job->hyper);
    const int t = threadIdx.x, gq = t & 15, rr = t >> 4;
    const int c = c0 + 4 * gq;
    if (c >= cols) return;
    // per launch: the bias corrections of step *step_dev + 1, in double
    const int step = *step_dev + 1;
    const double bc1 = 1.0 - ipow_f64(static_cast<double>(beta1), step);
    const float bc2_sqrt = static_cast<float>(sqrt(1.0 - ipow_f64(static_cast<double>(beta2), step)));
    const float one_minus_beta1 = 1.f - beta1, one_minus_beta2 = 1.f - beta2;
    // the column part of the segment index of the thread's four columns (one division when they share a segment)
    const int64_t segs_per_row = (cols + seg_cols - 1) / seg_cols;
    int cseg[4];
    cseg[0] = c / seg_cols;
    cseg[3] = min(c + 3, cols - 1) / seg_cols;
    cseg[1] = cseg[0] == cseg[3] ? cseg[0] : min(c + 1, cols - 1) / seg_cols;
    cseg[2] = cseg[0] == cseg[3] ? cseg[0] : min(c + 2, cols - 1) / seg_cols;
    int64_t cur = -1;  // the segment whose numbers are in step_size / weight_decay
    float step_size = 0.f, weight_decay = 0.f;
#pragma unroll
    for (int i = 0; i < AD_TILE / 16; ++i) {
        const int r = r0 + rr + 16 * i;
        if (r >= rows) continue;
        const int64_t rseg = static_cast<int64_t>(r / seg_rows) * segs_per_row;
        float p[4], g[4], m[4], v[4];
        ad_load4(P, r, c, cols, p);
        ad_load4(G, r, c, cols, g);
        ad_load4(M, r, c, cols, m);
        ad_load4(V, r, c, cols, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c + k >= cols) continue;
            const int64_t seg = rseg + cseg[k];
            if (seg != cur) {
                cur = seg;
                const float lr = hyper[2 * seg];
                weight_decay = hyper[2 * seg + 1];
                step_size = static_cast<float>(static_cast<double>(lr) / bc1);
            }
            ad_element(p[k], g[k], m[k], v[k], weight_decay, step_size, beta1, beta2, one_minus_beta1, one_minus_beta2, bc2_sqrt, eps);
        }
        ad_store4(P, r, c, cols, p);
        ad_store4(M, r, c, cols, m);
        ad_store4(V, r, c, cols, v);
    }
}

}  // namespace

extern "C" int wdg_adam_batched_f32(const wdg_adam_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, float beta1, float beta2,
                                    float eps, const int32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "adam_batched: negative count");
    WDG_REQUIRE(step_dev != nullptr, "adam_batched: null step word");
    WDG_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_batched: Adam needs 0 <= beta < 1");  // (a NaN fails)
    WDG_REQUIRE(eps == eps, "adam_batched: eps is not a number");
    WDG_REQUIRE(n_jobs <= AD_MAX_JOBS, "adam_batched: %d jobs; one launch takes %d", n_jobs, AD_MAX_JOBS);
    WDG_REQUIRE(wdg::ceil_div(max_cols, AD_TILE) <= AD_MAX_COL_TILES, "adam_batched: %d columns; one launch takes %d", max_cols,
                AD_TILE * AD_MAX_COL_TILES);
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "adam_batched: null job table");
    if (max_rows == 0 || max_cols == 0) return WDG_OK;
    hipLaunchKernelGGL(adam_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, AD_TILE)), static_cast<unsigned>(wdg::ceil_div(max_cols, AD_TILE)),
                                         static_cast<unsigned>(n_jobs)),
                       dim3(AD_THREADS), 0, wdg::as_stream(stream), jobs_dev, max_rows, max_cols, beta1, beta2, eps, step_dev);
    return wdg::check_launch("adam_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host: what wdg_adam_batched_f32 cannot see in device
// memory before it launches (ops.AdamBatch calls this on the table it is about to upload).
extern "C" int wdg_adam_check_jobs(const wdg_adam_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "adam_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "adam_check_jobs: null job table");
    WDG_REQUIRE(n_jobs <= AD_MAX_JOBS, "adam_check_jobs: %d jobs; one launch takes %d", n_jobs, AD_MAX_JOBS);
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_adam_job &j = jobs_host[i];
        WDG_REQUIRE(j.rows >= 0 && j.cols >= 0, "adam_check_jobs: job %d has a negative shape", i);
        if (j.rows == 0 || j.cols == 0) continue;
        WDG_REQUIRE(j.seg_rows >= 1 && j.seg_cols >= 1, "adam_check_jobs: job %d has segments of %d x %d", i, j.seg_rows, j.seg_cols);
        WDG_REQUIRE(j.ld >= j.cols && j.ld_s >= j.cols, "adam_check_jobs: job %d has a leading dimension below its %d columns", i, j.cols);
        WDG_REQUIRE(j.p && j.g && j.m && j.v && j.hyper, "adam_check_jobs: job %d has a null pointer", i);
    }
    return WDG_OK;
}
