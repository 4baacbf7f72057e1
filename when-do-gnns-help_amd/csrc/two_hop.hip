// The strict two-hop neighbourhood of many graphs in two launches (the second aggregation pattern of H2GCN: Zhu et al., "Beyond
// Homophily in Graph Neural Networks"): T = (A . A > 0) \ (A u I) as a CSR pattern, for a table of square CSR patterns.
// include/wdg.h DEFINES the result set and lists every refusal; tests/_two_hop_ref.py restates it with Python sets.
//
// replaces: nothing the reference computes - its aggregations (normalize_tensor, utils/util_funcs.py:365-381) run on the pattern they
//           are handed; the pattern product is defined by this project.
//
// Shape: grid (row groups, jobs), TH_WAVES waves per workgroup.  ONE wave owns one row i at a time and keeps a bitmap of n bits in LDS
// (its own slice of the workgroup's: no workgroup barrier anywhere).  It zeroes the words, reads 64 stored k of row i with their
// extents at once (a lane each), then walks row k - all 64 lanes over its entries - and ORs the bit of every j with LDS atomics; then
// it clears (or, with WDG_TWO_HOP_KEEP_ONE_HOP, sets) the bits of row i's own entries and clears i's (unless WDG_TWO_HOP_KEEP_SELF).
// The set is a bitmap, so the input rows may be unsorted and hold duplicates, and the output is strictly ascending by construction.
// The count pass adds the popcounts; a second kernel of the same entry (a workgroup per job) turns the counts into row pointers and
// writes the total.  The fill pass REBUILDS the bitmap - there is no n^2 / 8-byte workspace - and emits the set bits: 64 words per
// round, a word per lane, a wave prefix sum of the popcounts for the offsets.
// An index outside [0, n) never addresses LDS: it is skipped, and the row that stores it marks its count (every stored entry is seen
// by its own row's walk), which the second kernel turns into total = -1.  Integer only; no global atomic; results do not depend on
// the table or on the launch geometry.
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int TH_WAVES = WDG_TWO_HOP_WAVES, TH_THREADS = TH_WAVES * kWave;
constexpr int TH_MAX_JOBS = 65535;   // gridDim.y: a job per y
constexpr int TH_MAX_GROUPS = 4096;  // gridDim.x: the waves stride over a job's rows
constexpr int TH_SCAN_THREADS = 1024;
constexpr int TH_FLAGS = WDG_TWO_HOP_KEEP_ONE_HOP | WDG_TWO_HOP_KEEP_SELF;
static_assert(TH_WAVES * 4 * ((WDG_TWO_HOP_MAX_ROWS + 31) / 32) <= WDG_TWO_HOP_LDS_BYTES, "every wave's bitmap of the largest job fits in the workgroup's LDS");
static_assert(WDG_TWO_HOP_MAX_ROWS >= 32768, "the limit the front end promises at least");

__host__ __device__ __forceinline__ int th_words(const int n) { return (n + 31) / 32; }

// what both launches skip and wdg_csr_two_hop_check_jobs refuses (one predicate; the kernels add n > max_rows, which sizes their LDS)
template <typename J>
__host__ __device__ __forceinline__ bool th_malformed(const J job) {
    return job->n < 0 || job->n > WDG_TWO_HOP_MAX_ROWS || (job->flags & ~TH_FLAGS) != 0 || job->out_rowptr == nullptr || job->total == nullptr ||
           (job->n > 0 && job->rowptr == nullptr);
}

__device__ __forceinline__ void th_wave_sync() {  // the wave's LDS operations so far, before the ones that follow (gat_lanes.h's idiom)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int th_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Row i's bitmap into bm[0 .. words); -> whether the row stores an index outside [0, n) (wave-uniform).  has_col: col != NULL.
__device__ __forceinline__ bool th_build_row(uint32_t *bm, const global_ptr<const int32_t> rowptr, const global_ptr<const int32_t> col, const bool has_col,
                                             const int n, const int words, const int flags, const int i, const int lane) {
    for (int w = lane; w < words; w += kWave) bm[w] = 0u;
    th_wave_sync();
    const int beg = has_col ? rowptr[i] : 0, end = has_col ? rowptr[i + 1] : 0;
    bool bad = false;
    for (int p0 = beg; p0 < end; p0 += kWave) {
        // 64 stored k of row i and their extents, a lane each: the dependent loads of the walk below are in flight together
        const int p = p0 + lane;
        int k = -1, kb = 0, ke = 0;
        if (p < end) {
            k = col[p];
            if (k < 0 || k >= n) {
                bad = true;
                k = -1;
            } else if (k != i) {
                kb = rowptr[k];
                ke = rowptr[k + 1];
            }
        }
        const int live = min(end - p0, kWave);
        for (int t = 0; t < live; ++t) {
            const int qb = __shfl(kb, t), qe = __shfl(ke, t);  // (k == i, or out of range: an empty extent)
            for (int q = qb + lane; q < qe; q += kWave) {
                const int j = col[q];
                if (j >= 0 && j < n) __hip_atomic_fetch_or(bm + (j >> 5), 1u << (j & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // (an index out of range in row k is marked by row k's own walk)
            }
        }
    }
    th_wave_sync();
    // the row's own entries leave the set - or, with KEEP_ONE_HOP, join it; the diagonal of A counts as not stored either way
    for (int p = beg + lane; p < end; p += kWave) {
        const int j = col[p];
        if (j < 0 || j >= n || j == i) continue;
        if (flags & WDG_TWO_HOP_KEEP_ONE_HOP)
            __hip_atomic_fetch_or(bm + (j >> 5), 1u << (j & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            __hip_atomic_fetch_and(bm + (j >> 5), ~(1u << (j & 31)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    th_wave_sync();
    if (!(flags & WDG_TWO_HOP_KEEP_SELF) && lane == 0) bm[i >> 5] &= ~(1u << (i & 31));
    th_wave_sync();
    return __ballot(bad) != 0ull;
}

// out_rowptr[i] = the count of row i, or ~count when the row stores an index out of range (the scan below reads the mark)
__global__ __launch_bounds__(TH_THREADS) void two_hop_count_kernel(const wdg_two_hop_job *__restrict__ jobs, const int max_rows) {
    extern __shared__ uint32_t th_lds[];
    const desc_ptr<wdg_two_hop_job> job = (desc_ptr<wdg_two_hop_job>)(jobs + blockIdx.y);
    const int n = job->n;
    if (th_malformed(job) || n > max_rows) return;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, words = th_words(n), flags = job->flags;
    uint32_t *bm = th_lds + static_cast<size_t>(wave) * th_words(max_rows);
    const global_ptr<const int32_t> rowptr = to_global(job->rowptr), col = to_global(job->col);
    const global_ptr<int32_t> out_rowptr = to_global(job->out_rowptr);
    const bool has_col = job->col != nullptr;
    for (int i = blockIdx.x * TH_WAVES + wave; i < n; i += gridDim.x * TH_WAVES) {
        const bool bad = th_build_row(bm, rowptr, col, has_col, n, words, flags, i, lane);
        int cnt = 0;
        for (int w = lane; w < words; w += kWave) cnt += __popc(bm[w]);
        cnt = th_wave_sum(cnt);
        if (lane == 0) out_rowptr[i] = bad ? ~cnt : cnt;
        th_wave_sync();  // (the next row zeroes the words this one has just read)
    }
}

// counts -> exclusive row pointers in place, out_rowptr[n] and total; a workgroup per job, thread t owns the rows t * chunk ..
__global__ __launch_bounds__(TH_SCAN_THREADS) void two_hop_scan_kernel(const wdg_two_hop_job *__restrict__ jobs, const int max_rows) {
    __shared__ int64_t part[2][TH_SCAN_THREADS];
    __shared__ int any_bad;
    const desc_ptr<wdg_two_hop_job> job = (desc_ptr<wdg_two_hop_job>)(jobs + blockIdx.x);
    const int n = job->n;
    if (th_malformed(job) || n > max_rows) return;
    const global_ptr<int32_t> out_rowptr = to_global(job->out_rowptr);
    const int t = threadIdx.x, chunk = (n + TH_SCAN_THREADS - 1) / TH_SCAN_THREADS;
    const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
    if (t == 0) any_bad = 0;
    __syncthreads();
    int64_t sum = 0;
    bool bad = false;
    for (int i = lo; i < hi; ++i) {
        const int c = out_rowptr[i];
        bad |= c < 0;
        sum += c < 0 ? ~c : c;
    }
    if (bad) any_bad = 1;  // (every writer stores the same value)
    part[0][t] = sum;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < TH_SCAN_THREADS; o <<= 1) {  // inclusive scan of the chunks' sums
        part[cur ^ 1][t] = part[cur][t] + (t >= o ? part[cur][t - o] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int64_t run = part[cur][t] - sum;
    for (int i = lo; i < hi; ++i) {
        const int c = out_rowptr[i];
        out_rowptr[i] = static_cast<int32_t>(run);  // (a total beyond 2^31 - 1 wraps here: the caller reads `total` first)
        run += c < 0 ? ~c : c;
    }
    if (t == TH_SCAN_THREADS - 1) {
        const int64_t total = part[cur][t];
        out_rowptr[n] = static_cast<int32_t>(total);
        *to_global(job->total) = any_bad ? int64_t{-1} : total;
    }
}

__global__ __launch_bounds__(TH_THREADS) void two_hop_fill_kernel(const wdg_two_hop_job *__restrict__ jobs, const int max_rows) {
    extern __shared__ uint32_t th_lds[];
    const desc_ptr<wdg_two_hop_job> job = (desc_ptr<wdg_two_hop_job>)(jobs + blockIdx.y);
    const int n = job->n;
    if (th_malformed(job) || n > max_rows || job->out_col == nullptr) return;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, words = th_words(n), flags = job->flags;
    uint32_t *bm = th_lds + static_cast<size_t>(wave) * th_words(max_rows);
    const global_ptr<const int32_t> rowptr = to_global(job->rowptr), col = to_global(job->col);
    const global_ptr<const int32_t> out_rowptr = to_global((const int32_t *)job->out_rowptr);
    const global_ptr<int32_t> out_col = to_global(job->out_col);
    const bool has_col = job->col != nullptr;
    for (int i = blockIdx.x * TH_WAVES + wave; i < n; i += gridDim.x * TH_WAVES) {
        (void)th_build_row(bm, rowptr, col, has_col, n, words, flags, i, lane);
        int base = out_rowptr[i];
        const int row_end = out_rowptr[i + 1];  // (nothing is written past the row the count pass sized)
        for (int w0 = 0; w0 < words && base < row_end; w0 += kWave) {
            uint32_t word = w0 + lane < words ? bm[w0 + lane] : 0u;
            const int c = __popc(word);
            int incl = c;
            for (int o = 1; o < kWave; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            int off = base + incl - c;
            const int j0 = (w0 + lane) << 5;
            while (word) {
                if (off >= 0 && off < row_end) out_col[off] = j0 + __builtin_ctz(word);
                ++off;
                word &= word - 1u;
            }
            base += __shfl(incl, kWave - 1);
        }
        th_wave_sync();
    }
}

int th_launch_checks(const char *what, const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows) {
    WDG_REQUIRE(max_rows >= 0, "%s: negative count", what);
    if (const int rc = wdg::check_job_table(what, jobs_dev, n_jobs, TH_MAX_JOBS)) return rc;
    if (max_rows > WDG_TWO_HOP_MAX_ROWS)
        return wdg::fail(WDG_ERR_UNSUPPORTED, "%s: %d rows; a wave's bitmap holds at most %d columns in LDS", what, max_rows, WDG_TWO_HOP_MAX_ROWS);
    return WDG_OK;
}

template <typename K>
int th_launch_rows(K kernel, const char *what, const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows, hipStream_t st, int &configured_dev) {
    if (configured_dev != wdg::current_device()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WDG_TWO_HOP_LDS_BYTES) != hipSuccess)
            return wdg::fail(WDG_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", what);
        configured_dev = wdg::current_device();
    }
    const size_t lds = static_cast<size_t>(TH_WAVES) * 4 * th_words(max_rows);
    const dim3 grid(static_cast<unsigned>(min(static_cast<int>(wdg::ceil_div(max_rows, TH_WAVES)), TH_MAX_GROUPS)), static_cast<unsigned>(n_jobs));
    hipLaunchKernelGGL(kernel, grid, dim3(TH_THREADS), lds, st, jobs_dev, max_rows);
    return wdg::check_launch(what);
}

}  // namespace

extern "C" int32_t wdg_csr_two_hop_max_rows(void) { return WDG_TWO_HOP_MAX_ROWS; }

// The per-job part of the contract, on the table the caller still holds on the host (graphs.TwoHopBatch calls this before it uploads).
extern "C" int wdg_csr_two_hop_check_jobs(const wdg_two_hop_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("csr_two_hop_check_jobs", jobs_host, n_jobs, TH_MAX_JOBS)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_two_hop_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0, "csr_two_hop_check_jobs: job %d has a negative n", i);
        if (j.n > WDG_TWO_HOP_MAX_ROWS)
            return wdg::fail(WDG_ERR_UNSUPPORTED, "csr_two_hop_check_jobs: job %d has %d rows; a wave's bitmap holds at most %d columns in LDS", i, j.n,
                             WDG_TWO_HOP_MAX_ROWS);
        WDG_REQUIRE((j.flags & ~TH_FLAGS) == 0, "csr_two_hop_check_jobs: job %d has flags %d; WDG_TWO_HOP_KEEP_ONE_HOP (1) and WDG_TWO_HOP_KEEP_SELF (2) are defined", i,
                    j.flags);
        WDG_REQUIRE(j.out_rowptr && j.total, "csr_two_hop_check_jobs: job %d has a null out_rowptr or total", i);
        WDG_REQUIRE(j.n == 0 || j.rowptr, "csr_two_hop_check_jobs: job %d has a null rowptr", i);
        WDG_REQUIRE(!th_malformed(&j), "csr_two_hop_check_jobs: job %d is malformed", i);
    }
    return WDG_OK;
}

extern "C" int wdg_csr_two_hop_count_batched(const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = th_launch_checks("csr_two_hop_count_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const hipStream_t st = wdg::as_stream(stream);
    static thread_local int configured_dev = -1;
    if (const int rc = th_launch_rows(two_hop_count_kernel, "csr_two_hop_count_batched", jobs_dev, n_jobs, max_rows, st, configured_dev)) return rc;
    hipLaunchKernelGGL(two_hop_scan_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(TH_SCAN_THREADS), 0, st, jobs_dev, max_rows);
    return wdg::check_launch("csr_two_hop_count_batched (row pointers)");
}

extern "C" int wdg_csr_two_hop_fill_batched(const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream) {
    if (const int rc = th_launch_checks("csr_two_hop_fill_batched", jobs_dev, n_jobs, max_rows)) return rc;
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    static thread_local int configured_dev = -1;
    return th_launch_rows(two_hop_fill_kernel, "csr_two_hop_fill_batched", jobs_dev, n_jobs, max_rows, wdg::as_stream(stream), configured_dev);
}
