// The graphs and features of the CSBM-H model, drawn on the device (wdg_synth_classes_batched, wdg_gauss_features_batched_f32): classes
// of any sizes with a degree and a same-class count of their own - the regular generator's keys and its row routine (synth_row.h) -
// and Gaussian class features, Box-Muller on Philox words.  include/wdg.h defines both; tests/_csbmh_ref.py restates them in numpy.
//
// replaces: the i.i.d. draws of csbm-h.py:174-175,187-191 (which sample the aggregated features' closed-form law, not a graph).
// No fast-math in this unit: the features use the accurate logf / sqrtf / cospif / sinpif.
#include "synth_row.h"

namespace {

using namespace wdg;

// Classes of any sizes, each with a k and a d of its own (wdg_synth_classes_batched): the same wave per row and the same row routine,
// with the row's class block and counts looked up in the job's inline arrays (at most 16 classes: a scalar walk).
__global__ __launch_bounds__(SY_THREADS) void synth_classes_kernel(const wdg_synth_classes_job *__restrict__ jobs, int per) {
    extern __shared__ unsigned sy_lds[];
    const int waves = static_cast<int>(blockDim.x) >> 6, wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const desc_ptr<wdg_synth_classes_job> j = (desc_ptr<wdg_synth_classes_job>)(jobs + blockIdx.y);
    const int C = j->n_classes, row = static_cast<int>(blockIdx.x) * waves + wave, loops = (j->flags & WDG_SYNTH_SELF_LOOPS) ? 1 : 0;
    int n = 0, nnz = 0, cls = -1, cs = 0, ce = 0, first = 0;  // first: rowptr of the class's first row
    for (int c = 0; c < C; ++c) {
        const int m = j->class_size[c], Dc = j->d[c] + loops;
        if (row >= n && row < n + m) cls = c, cs = n, ce = n + m, first = nnz;
        n += m;
        nnz += m * Dc;
    }
    if (cls < 0) return;  // row >= n (wave-uniform; the kernel has no workgroup barrier)
    const int k = j->k[cls], d = j->d[cls], D = d + loops, at = first + (row - cs) * D;
    const unsigned k0 = static_cast<unsigned>(j->seed), k1 = static_cast<unsigned>(j->seed >> 32);
    sy_row(sy_lds, wave, lane, per, n, row, cs, ce, k, d - k, loops, D, k0, k1, to_global(j->col) + at, to_global(j->val) + at);
    if (lane == 0) {
        const global_ptr<int32_t> rowptr = to_global(j->rowptr), labels = to_global(j->labels);
        rowptr[row] = at;
        labels[row] = cls;
        if (row == n - 1) rowptr[n] = nnz;
    }
}

// Gaussian class features (wdg_gauss_features_batched_f32): a thread per (node, Philox block); a block gives two Box-Muller pairs =
// four consecutive features.  The accurate library functions: this unit is compiled without fast-math.
constexpr int GF_THREADS = 256;
__global__ __launch_bounds__(GF_THREADS) void gauss_features_kernel(const wdg_gauss_job *__restrict__ jobs) {
    const desc_ptr<wdg_gauss_job> j = (desc_ptr<wdg_gauss_job>)(jobs + blockIdx.y);
    const int n = j->n, F = j->F, Q = (F + 3) >> 2;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * GF_THREADS + threadIdx.x;
    if (t >= static_cast<int64_t>(n) * Q) return;
    const int i = static_cast<int>(t / Q), q = static_cast<int>(t % Q);
    const int c = to_global(j->labels)[i];
    const bool known = c >= 0 && c < j->n_classes;
    const philox_words w = philox4x32_10_words(static_cast<unsigned>(i), static_cast<unsigned>(q), static_cast<unsigned>(j->seed),
                                               static_cast<unsigned>(j->seed >> 32));
    float z[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = static_cast<float>((w.w[2 * p] >> 8) + 1u) * 0x1p-24f;  // (0, 1], exact
        const float u2 = static_cast<float>(w.w[2 * p + 1] >> 8) * 0x1p-24f;     // [0, 1), exact
        const float r = sqrtf(-2.0f * logf(u1));
        z[2 * p] = r * cospif(2.0f * u2);
        z[2 * p + 1] = r * sinpif(2.0f * u2);
    }
    const float sd = known ? to_global(j->sd)[c] : 0.0f;
    const global_ptr<const float> mean = to_global(j->mean) + static_cast<int64_t>(known ? c : 0) * F;
    const global_ptr<float> out = to_global(j->x) + static_cast<int64_t>(i) * j->ldx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int f = 4 * q + e;
        if (f < F) out[f] = known ? fmaf(sd, z[e], mean[f]) : __builtin_nanf("");  // (a label outside the classes: NaN, nothing is read)
    }
}

}  // namespace

extern "C" {

int wdg_synth_classes_batched(const wdg_synth_classes_job *jobs_host, const wdg_synth_classes_job *jobs_dev, int32_t n_jobs,
                              wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "synth_classes_batched: negative job count");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_host != nullptr && jobs_dev != nullptr, "synth_classes_batched: null job table");
    WDG_REQUIRE(n_jobs <= 65535, "synth_classes_batched: more than 65535 graphs in one launch");
    int max_n = 0;
    for (int g = 0; g < n_jobs; ++g) {
        const wdg_synth_classes_job &j = jobs_host[g];
        WDG_REQUIRE(j.n_classes >= 1 && j.n_classes <= WDG_SYNTH_MAX_CLASSES, "synth_classes_batched: graph %d has %d classes (1 .. %d)", g,
                    j.n_classes, WDG_SYNTH_MAX_CLASSES);
        WDG_REQUIRE((j.flags & ~WDG_SYNTH_SELF_LOOPS) == 0, "synth_classes_batched: graph %d: unknown flags %d", g, j.flags);
        int64_t n = 0;
        for (int c = 0; c < j.n_classes; ++c) {
            WDG_REQUIRE(j.class_size[c] >= 1 && j.class_size[c] <= SY_MAX_N, "synth_classes_batched: graph %d: class %d has %d nodes (1 .. %d)", g,
                        c, j.class_size[c], SY_MAX_N);
            n += j.class_size[c];
        }
        WDG_REQUIRE(n >= 1 && n <= SY_MAX_N, "synth_classes_batched: graph %d has %lld nodes (1 .. %d)", g, static_cast<long long>(n), SY_MAX_N);
        for (int c = 0; c < j.n_classes; ++c) {
            const int m = j.class_size[c];
            WDG_REQUIRE(j.k[c] >= 0 && j.k[c] <= m - 1, "synth_classes_batched: graph %d: class %d: k = %d outside 0 .. %d", g, c, j.k[c], m - 1);
            WDG_REQUIRE(j.d[c] >= j.k[c], "synth_classes_batched: graph %d: class %d: d = %d below k = %d", g, c, j.d[c], j.k[c]);
            WDG_REQUIRE(j.d[c] - j.k[c] <= n - m, "synth_classes_batched: graph %d: class %d: %d other-class neighbours of %d nodes", g, c,
                        j.d[c] - j.k[c], static_cast<int>(n - m));
        }
        WDG_REQUIRE(j.rowptr && j.col && j.val && j.labels, "synth_classes_batched: graph %d: null output", g);
        max_n = n > max_n ? static_cast<int>(n) : max_n;  // (n <= 16384 rows of <= 16384 entries: a graph's entries fit 31 bits)
    }
    const int per = static_cast<int>(ceil_div(ceil_div(max_n, 4), 64));     // Philox blocks per lane
    const int wave_bytes = per * 4 * 64 * 4;                                // <= 64 KB at n = 16384
    const int waves = wave_bytes * 4 <= SY_LDS_BYTES ? 4 : (wave_bytes * 2 <= SY_LDS_BYTES ? 2 : 1);
    static thread_local int dev = -1;
    if (dev != wdg::current_device()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(synth_classes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SY_LDS_BYTES) != hipSuccess)
            return wdg::fail(WDG_ERR_LAUNCH, "synth_classes_batched: cannot raise the dynamic LDS limit");
        dev = wdg::current_device();
    }
    const dim3 grid(static_cast<unsigned>(ceil_div(max_n, waves)), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(synth_classes_kernel, grid, dim3(64 * waves), static_cast<size_t>(wave_bytes) * waves, wdg::as_stream(stream),
                       jobs_dev, per);
    return wdg::check_launch("synth_classes_kernel");
}

int wdg_gauss_features_batched_f32(const wdg_gauss_job *jobs_host, const wdg_gauss_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "gauss_features_batched: negative job count");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_host != nullptr && jobs_dev != nullptr, "gauss_features_batched: null job table");
    WDG_REQUIRE(n_jobs <= 65535, "gauss_features_batched: more than 65535 jobs in one launch");
    int64_t max_threads = 0;
    for (int g = 0; g < n_jobs; ++g) {
        const wdg_gauss_job &j = jobs_host[g];
        WDG_REQUIRE(j.n >= 0, "gauss_features_batched: job %d: negative row count", g);
        WDG_REQUIRE(j.F >= 1 && j.F <= WDG_GAUSS_MAX_F, "gauss_features_batched: job %d: F = %d outside 1 .. %d", g, j.F, WDG_GAUSS_MAX_F);
        WDG_REQUIRE(j.n_classes >= 1 && j.n_classes <= WDG_SYNTH_MAX_CLASSES, "gauss_features_batched: job %d: %d classes (1 .. %d)", g,
                    j.n_classes, WDG_SYNTH_MAX_CLASSES);
        WDG_REQUIRE(j.ldx >= j.F, "gauss_features_batched: job %d: leading dimension %lld below F = %d", g, static_cast<long long>(j.ldx), j.F);
        WDG_REQUIRE(j.n == 0 || (j.x && j.labels && j.mean && j.sd), "gauss_features_batched: job %d: null pointer", g);
        const int64_t threads = static_cast<int64_t>(j.n) * ((j.F + 3) / 4);
        max_threads = threads > max_threads ? threads : max_threads;
    }
    if (max_threads == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(ceil_div(max_threads, GF_THREADS)), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(gauss_features_kernel, grid, dim3(GF_THREADS), 0, wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("gauss_features_kernel");
}

}  // extern "C"
