// The sweep's synthetic inputs, drawn on the device: the homophily-varied regular graphs of a shard written straight into sorted
// CSR arrays (one launch, nothing uploaded, nothing sorted), and the per-class draw of base-dataset rows behind their features.
//
// replaces: the loads of the pre-generated adjacency / label / degree files (synthetic_plot.py:84-90) and, for the feature rows,
//           of the pre-sampled feature files (synthetic_plot.py:81-82) - the generator that wrote those files is not part of the
//           reference; its rule is restated in include/wdg.h (same distribution, a documented stream of its own).
#include "synth_row.h"

namespace {

using namespace wdg;

__global__ __launch_bounds__(SY_THREADS) void synth_regular_kernel(const wdg_synth_job *__restrict__ jobs, int per) {
    extern __shared__ unsigned sy_lds[];
    const int waves = static_cast<int>(blockDim.x) >> 6, wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const desc_ptr<wdg_synth_job> j = (desc_ptr<wdg_synth_job>)(jobs + blockIdx.y);
    const int n = j->n, row = static_cast<int>(blockIdx.x) * waves + wave;
    if (row >= n) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const int C = j->n_classes, k = j->k, d = j->d, n_other = d - k, loops = (j->flags & WDG_SYNTH_SELF_LOOPS) ? 1 : 0;
    const int m = n / C, cls = row / m, cs = cls * m, ce = cs + m, D = d + loops;
    const unsigned k0 = static_cast<unsigned>(j->seed), k1 = static_cast<unsigned>(j->seed >> 32);
    sy_row(sy_lds, wave, lane, per, n, row, cs, ce, k, n_other, loops, D, k0, k1, to_global(j->col) + static_cast<int64_t>(row) * D,
           to_global(j->val) + static_cast<int64_t>(row) * D);
    if (lane == 0) {
        const global_ptr<int32_t> rowptr = to_global(j->rowptr), uni = to_global(j->rowptr_union), labels = to_global(j->labels);
        rowptr[row] = row * D;
        labels[row] = cls;
        if (uni) uni[row] = j->nnz_base + row * D;
        if (row == n - 1) {
            rowptr[n] = n * D;
            if (uni) uni[n] = j->nnz_base + n * D;
        }
    }
}

// Feature rows: a workgroup per class lists the base rows of its label ascending (an ordered compaction over chunks of 256
// rows) and then draws, for every node of the class, a member of that list.
constexpr int SF_THREADS = 256;
__global__ __launch_bounds__(SF_THREADS) void synth_feature_rows_kernel(const int32_t *__restrict__ base_labels, int n_base, int n, int C,
                                                                        unsigned k0, unsigned k1, int32_t *__restrict__ out,
                                                                        int32_t *__restrict__ members, int32_t *__restrict__ counts) {
    __shared__ int wave_n[SF_THREADS / 64];
    const int c = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63;
    int32_t *list = members + static_cast<int64_t>(c) * n_base;
    int total = 0;
    for (int first = 0; first < n_base; first += SF_THREADS) {
        const int r = first + tid;
        const bool is = r < n_base && base_labels[r] == c;
        const unsigned long long mask = __ballot(is);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int at = total + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < SF_THREADS / 64; ++w) {
            if (w < wave) at += wave_n[w];
            total += wave_n[w];
        }
        if (is) list[at] = r;
        __syncthreads();
    }
    if (tid == 0) counts[c] = total;
    if (total == 0) return;  // (the caller reads the counts and raises)
    const int m = n / C;
    for (int i = c * m + tid; i < (c + 1) * m; i += SF_THREADS) {
        const unsigned u = philox4x32_10(static_cast<unsigned>(i), 0u, k0, k1);
        const int pick = static_cast<int>((static_cast<unsigned long long>(u) * static_cast<unsigned long long>(total)) >> 32);
        out[i] = list[pick];
    }
}

}  // namespace

extern "C" {

int wdg_synth_regular_batched(const wdg_synth_job *jobs_host, const wdg_synth_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "synth_regular_batched: negative job count");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_host != nullptr && jobs_dev != nullptr, "synth_regular_batched: null job table");
    WDG_REQUIRE(n_jobs <= 65535, "synth_regular_batched: more than 65535 graphs in one launch");
    int max_n = 0;
    for (int g = 0; g < n_jobs; ++g) {
        const wdg_synth_job &j = jobs_host[g];
        WDG_REQUIRE(j.n >= 1 && j.n <= SY_MAX_N, "synth_regular_batched: graph %d has %d nodes (1 .. %d)", g, j.n, SY_MAX_N);
        WDG_REQUIRE(j.n_classes >= 1 && j.n % j.n_classes == 0, "synth_regular_batched: graph %d: %d classes do not divide %d nodes", g,
                    j.n_classes, j.n);
        const int m = j.n / j.n_classes;
        WDG_REQUIRE(j.k >= 1 && j.k <= m - 1, "synth_regular_batched: graph %d: k = %d outside 1 .. %d", g, j.k, m - 1);
        WDG_REQUIRE(j.d >= j.k, "synth_regular_batched: graph %d: d = %d below k = %d", g, j.d, j.k);
        WDG_REQUIRE(j.d - j.k <= j.n - m, "synth_regular_batched: graph %d: %d other-class neighbours of %d nodes", g, j.d - j.k, j.n - m);
        WDG_REQUIRE((j.flags & ~WDG_SYNTH_SELF_LOOPS) == 0, "synth_regular_batched: graph %d: unknown flags %d", g, j.flags);
        WDG_REQUIRE(j.rowptr && j.col && j.val && j.labels, "synth_regular_batched: graph %d: null output", g);
        WDG_REQUIRE(static_cast<int64_t>(j.nnz_base) + static_cast<int64_t>(j.n) * (j.d + 1) < (1ll << 31),
                    "synth_regular_batched: graph %d: more than 2^31 entries in the shard", g);
        max_n = j.n > max_n ? j.n : max_n;
    }
    const int per = static_cast<int>(ceil_div(ceil_div(max_n, 4), 64));     // Philox blocks per lane
    const int wave_bytes = per * 4 * 64 * 4;                                // <= 64 KB at n = 16384
    const int waves = wave_bytes * 4 <= SY_LDS_BYTES ? 4 : (wave_bytes * 2 <= SY_LDS_BYTES ? 2 : 1);
    static thread_local int dev = -1;
    if (dev != wdg::current_device()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(synth_regular_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SY_LDS_BYTES) != hipSuccess)
            return wdg::fail(WDG_ERR_LAUNCH, "synth_regular_batched: cannot raise the dynamic LDS limit");
        dev = wdg::current_device();
    }
    const dim3 grid(static_cast<unsigned>(ceil_div(max_n, waves)), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(synth_regular_kernel, grid, dim3(64 * waves), static_cast<size_t>(wave_bytes) * waves, wdg::as_stream(stream),
                       jobs_dev, per);
    return wdg::check_launch("synth_regular_kernel");
}

size_t wdg_synth_feature_rows_workspace_bytes(int32_t n_base, int32_t n_classes) {
    if (n_base < 0 || n_classes < 0) return 0;
    return (static_cast<size_t>(n_base) * n_classes + n_classes) * sizeof(int32_t);
}

int wdg_synth_feature_rows(const int32_t *base_labels, int32_t n_base, int32_t n, int32_t n_classes, uint64_t seed, int32_t *rows_out,
                           void *workspace, size_t workspace_bytes, wdg_stream_t stream) {
    WDG_REQUIRE(n_base >= 0 && n >= 0 && n_classes >= 0, "synth_feature_rows: negative size");
    if (n == 0 || n_classes == 0) return WDG_OK;
    WDG_REQUIRE(n % n_classes == 0, "synth_feature_rows: %d classes do not divide %d nodes", n_classes, n);
    WDG_REQUIRE(n_classes <= 65535, "synth_feature_rows: more than 65535 classes");
    WDG_REQUIRE(base_labels != nullptr && rows_out != nullptr && workspace != nullptr, "synth_feature_rows: null pointer");
    if (workspace_bytes < wdg_synth_feature_rows_workspace_bytes(n_base, n_classes))
        return wdg::fail(WDG_ERR_WORKSPACE, "synth_feature_rows: workspace of %zu bytes, %zu needed", workspace_bytes,
                         wdg_synth_feature_rows_workspace_bytes(n_base, n_classes));
    int32_t *members = static_cast<int32_t *>(workspace), *counts = members + static_cast<size_t>(n_base) * n_classes;
    hipLaunchKernelGGL(synth_feature_rows_kernel, dim3(static_cast<unsigned>(n_classes)), dim3(SF_THREADS), 0, wdg::as_stream(stream),
                       base_labels, n_base, n, n_classes, static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32), rows_out, members,
                       counts);
    return wdg::check_launch("synth_feature_rows_kernel");
}

}  // extern "C"
