// The errors the Bayes rule of two isotropic Gaussian classes makes on a graph's features x, on its aggregated features h and on
// the high-pass features x - h (wdg_qda_errors_batched_i32): per job a [3, 2, 2] table of integer counts, [set][true][predicted].
// include/wdg.h states the arithmetic; tests/_csbmh_ref.py restates it in numpy, and the counts are compared for equality.
//
// replaces: nothing the reference measures - it has the rule's error in closed form only (chi2comb_error, csbm-h.py:9-37; PBE,
//           csbm-h.py:40-60); this is the same rule (the constant of csbm-h.py:13-14 is its two-feature case) applied to sampled rows.
//
// A workgroup per job, a thread per row in strides of the workgroup.  The discriminants are fp64 sums over at most 16 features in
// ascending order; the class means, 1 / (2 v) and the bias sit in the job descriptor and arrive by scalar loads.  A thread counts its
// rows in twelve registers; a wave sums them with a butterfly, the four waves meet in LDS, and twelve threads store the table: integer
// adds only, no atomic, and nothing has to be cleared before the launch.
#include "wdg_common.h"

#pragma clang fp contract(off)  // every multiply and add below is its own correctly rounded operation: numpy restates the bits

namespace {

using namespace wdg;

constexpr int QD_THREADS = 256;

__global__ __launch_bounds__(QD_THREADS) void qda_errors_kernel(const wdg_qda_job *__restrict__ jobs) {
    __shared__ int part[QD_THREADS / 64][12];
    const desc_ptr<wdg_qda_job> j = (desc_ptr<wdg_qda_job>)(jobs + blockIdx.x);
    const int n = j->n, F = j->F, tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63;
    const global_ptr<const float> x = to_global(j->x), h = to_global(j->h);
    const global_ptr<const int32_t> labels = to_global(j->labels);
    const int64_t ldx = j->ldx, ldh = j->ldh;
    int cnt[12];
#pragma unroll
    for (int b = 0; b < 12; ++b) cnt[b] = 0;
    for (int i = tid; i < n; i += QD_THREADS) {
        const int y = labels[i];
        double s[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        for (int f = 0; f < F; ++f) {
            const float xf = x[i * ldx + f], hf = h[i * ldh + f];
            const double z[3] = {static_cast<double>(xf), static_cast<double>(hf), static_cast<double>(xf - hf)};
#pragma unroll
            for (int t = 0; t < 3; ++t) {
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double e = z[t] - j->mean[t][c][f];
                    s[t][c] = s[t][c] + e * e;
                }
            }
        }
        if (y == 0 || y == 1) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const double g0 = j->bias[t][0] - j->inv2v[t][0] * s[t][0], g1 = j->bias[t][1] - j->inv2v[t][1] * s[t][1];
                const int pred = g0 > g1 ? 0 : 1;  // (a NaN on either side: 1)
#pragma unroll
                for (int b = 0; b < 4; ++b) cnt[4 * t + b] += (2 * y + pred == b) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 12; ++b) {
        int v = cnt[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) part[wave][b] = v;
    }
    __syncthreads();
    if (tid < 12) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < QD_THREADS / 64; ++w) v += part[w][tid];
        to_global(j->counts)[tid] = v;
    }
}

}  // namespace

extern "C" {

int wdg_qda_errors_batched_i32(const wdg_qda_job *jobs_host, const wdg_qda_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "qda_errors_batched: negative job count");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_host != nullptr && jobs_dev != nullptr, "qda_errors_batched: null job table");
    WDG_REQUIRE(n_jobs <= 65535, "qda_errors_batched: more than 65535 jobs in one launch");
    for (int g = 0; g < n_jobs; ++g) {
        const wdg_qda_job &j = jobs_host[g];
        WDG_REQUIRE(j.n >= 0, "qda_errors_batched: job %d: negative row count", g);
        WDG_REQUIRE(j.F >= 1 && j.F <= WDG_QDA_MAX_F, "qda_errors_batched: job %d: F = %d outside 1 .. %d", g, j.F, WDG_QDA_MAX_F);
        WDG_REQUIRE(j.ldx >= j.F && j.ldh >= j.F, "qda_errors_batched: job %d: a leading dimension below F = %d", g, j.F);
        WDG_REQUIRE(j.counts != nullptr, "qda_errors_batched: job %d: null counts", g);
        WDG_REQUIRE(j.n == 0 || (j.x && j.h && j.labels), "qda_errors_batched: job %d: null x, h or labels", g);
    }
    hipLaunchKernelGGL(qda_errors_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(QD_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("qda_errors_kernel");
}

}  // extern "C"
