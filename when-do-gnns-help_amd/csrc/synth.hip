// The sweep's synthetic inputs, drawn on the device: the homophily-varied regular graphs of a shard written straight into sorted
// CSR arrays (one launch, nothing uploaded, nothing sorted), and the per-class draw of base-dataset rows behind their features.
//
// replaces: the loads of the pre-generated adjacency / label / degree files (synthetic_plot.py:84-90) and, for the feature rows,
//           of the pre-sampled feature files (synthetic_plot.py:81-82) - the generator that wrote those files is not part of the
//           reference; its rule is restated in include/wdg.h (same distribution, a documented stream of its own).
#include "philox.h"
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int SY_MAX_N = 16384;          // GraphBatch's cap for a SELL-16 copy
constexpr int SY_THREADS = 256;          // up to four rows (waves) per workgroup
constexpr int SY_LDS_BYTES = 64 * 1024;  // of keys per workgroup: n <= 4096 -> 4 rows, n <= 8192 -> 2, else 1

__device__ __forceinline__ unsigned sy_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned sy_wave_inclusive(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// A wave per row.  Lane l owns the `cpl` = 4 x `per` consecutive candidate columns from l x cpl on (whole Philox blocks: a block
// serves four columns) and keeps their keys in LDS, column q of its range at word q x 64 + l of the wave's region: lane-private
// and conflict-free.  The k-th smallest key of the row's class block and the (d - k)-th smallest of the rest are found TOGETHER by
// a search over the 32 key bits, most significant first: T becomes the largest value with fewer than k keys below it, i.e. the
// k-th smallest key; a pass counts both groups in one walk over the lane's keys and sums the two counts packed in one word (each
// < 2^15 resp. <= 2^14).  Keys equal to the threshold are taken in column order until the group is full.  Lanes own ascending
// column ranges, so a prefix sum of the lanes' counts gives every chosen column its sorted position: no sort.
__global__ __launch_bounds__(SY_THREADS) void synth_regular_kernel(const wdg_synth_job *__restrict__ jobs, int per) {
    extern __shared__ unsigned sy_lds[];
    const int waves = static_cast<int>(blockDim.x) >> 6, wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const desc_ptr<wdg_synth_job> j = (desc_ptr<wdg_synth_job>)(jobs + blockIdx.y);
    const int n = j->n, row = static_cast<int>(blockIdx.x) * waves + wave;
    if (row >= n) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const int C = j->n_classes, k = j->k, d = j->d, n_other = d - k, loops = (j->flags & WDG_SYNTH_SELF_LOOPS) ? 1 : 0;
    const int m = n / C, cls = row / m, cs = cls * m, ce = cs + m, D = d + loops;
    const unsigned k0 = static_cast<unsigned>(j->seed), k1 = static_cast<unsigned>(j->seed >> 32);
    const int cpl = 4 * per, base = lane * cpl;
    unsigned *keys = sy_lds + static_cast<size_t>(wave) * cpl * 64 + lane;  // keys[q * 64]: column base + q
    const int cnt = max(0, min(n - base, cpl));                              // columns this lane owns
    for (int t = 0; 4 * t < cnt; ++t) {
        const philox_words w = philox4x32_10_words(static_cast<unsigned>(row), static_cast<unsigned>((base >> 2) + t), k0, k1);
#pragma unroll
        for (int x = 0; x < 4; ++x) keys[(4 * t + x) * 64] = w.w[x];  // (inside the lane's cpl slots, also past column n - 1)
    }
    // the lane's columns: [0, qa) and [qb, cnt) lie outside the row's class block, [qa, qb) inside; qi = the row itself
    const int qa = min(max(cs - base, 0), cnt), qb = min(max(ce - base, 0), cnt), qi = row - base;
    const bool self_here = qi >= 0 && qi < cnt;
    const unsigned key_i = self_here ? keys[qi * 64] : 0u;
    unsigned Ts = 0, To = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand_s = Ts | (1u << bit), cand_o = To | (1u << bit);
        unsigned a = 0, b = 0;
        for (int q = 0; q < qa; ++q) b += keys[q * 64] < cand_o ? 1u : 0u;
        for (int q = qa; q < qb; ++q) a += keys[q * 64] < cand_s ? 1u : 0u;
        for (int q = qb; q < cnt; ++q) b += keys[q * 64] < cand_o ? 1u : 0u;
        if (self_here && key_i < cand_s) --a;  // the row is no candidate of its own class
        const unsigned both = sy_wave_sum(b | (a << 16));
        if (static_cast<int>(both >> 16) < k) Ts = cand_s;
        if (static_cast<int>(both & 0xffffu) < n_other) To = cand_o;
    }
    // keys below the thresholds are in; of the keys equal to them, the first need_s / need_o in column order
    unsigned less_s = 0, less_o = 0, eq_s = 0, eq_o = 0;
    for (int q = 0; q < cnt; ++q) {
        const unsigned key = keys[q * 64];
        if (q >= qa && q < qb) {
            if (q != qi) less_s += key < Ts ? 1u : 0u, eq_s += key == Ts ? 1u : 0u;
        } else {
            less_o += key < To ? 1u : 0u, eq_o += key == To ? 1u : 0u;
        }
    }
    const unsigned less = sy_wave_sum(less_o | (less_s << 16));
    const int need_s = k - static_cast<int>(less >> 16), need_o = n_other - static_cast<int>(less & 0xffffu);
    const unsigned eq_mine = eq_o | (eq_s << 16), eq_before = sy_wave_inclusive(eq_mine, lane) - eq_mine;
    const int rank_s0 = static_cast<int>(eq_before >> 16), rank_o0 = static_cast<int>(eq_before & 0xffffu);
    const global_ptr<int32_t> col_out = to_global(j->col) + static_cast<int64_t>(row) * D;
    const global_ptr<float> val_out = to_global(j->val) + static_cast<int64_t>(row) * D;
    auto walk = [&](bool write, int pos) {
        int rank_s = rank_s0, rank_o = rank_o0;
        for (int q = 0; q < cnt; ++q) {
            const unsigned key = keys[q * 64];
            bool in;
            if (q == qi) in = loops != 0;
            else if (q >= qa && q < qb) in = key < Ts || (key == Ts && rank_s++ < need_s);
            else in = key < To || (key == To && rank_o++ < need_o);
            if (in) {
                if (write && pos < D) col_out[pos] = base + q, val_out[pos] = 1.0f;
                ++pos;
            }
        }
        return pos;
    };
    const unsigned mine = static_cast<unsigned>(walk(false, 0));
    const unsigned before = sy_wave_inclusive(mine, lane) - mine;
    walk(true, static_cast<int>(before));
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
