// The exact ROC-AUC of many BINARY models whose logits are STACKED along the feature axis (replica r owns columns r cs and r cs + 1 of
// one [n, R cs] matrix), per replica and part of its split, as two int64 (u2, pairs) - with the selection on the validation AUC, the
// patience counter and the curve row on the device.  include/wdg.h states the definition; tests/_auc_ref.py restates it in numpy.
//
// replaces: nothing the reference computes - its only score is the accuracy of utils/util_funcs.py:393, while five of the seven large
//           data sets of homophily_tests.py:30 are binary and load_yelpchi_dataset (utils/datasets.py:82) and load_genius
//           (utils/datasets.py:197) give unbalanced labels that upstream scores by ROC-AUC.  It stands in for a copy of the logits to
//           the host and a rank statistic per replica and epoch.
//
// csrc/stacked_row.h states the layout and the ownership of a (row, replica) pair: one thread owns one pair, adjacent lanes own
// adjacent replicas of a row.  Nothing is sorted.  Five launches:
//   count    a pair's key = the monotone uint32 image of d = z_1 - z_0; one integer add to the counter of (replica, part, bin, class)
//            (adjacent lanes own adjacent replicas: the adds of a wave go to different counters); NaN rows are counted on their own
//   scan     a workgroup per replica walks its 3 B (bin: negatives, positives) counters once: the pairs ACROSS bins,
//            2 pos[b] (negatives below b), and the offsets - a bin's negatives, then its positives, bins ascending, parts ascending
//   scatter  the keys again, each to its bin's piece of the replica's key array through the bin's integer cursor
//   in-bin   per (replica, part, bin) with both classes: the negatives' keys in LDS tiles of AU_TILE, a positive key per thread,
//            2 lt + eq counted in integers, one 64-bit integer add per workgroup; the bin's counters go back to zero here
//   finish   validity, pairs, the curve row, selection and patience; the NaN counters go back to zero
// Every sum is a sum of integers: no floating-point atomic, and no result depends on the order inside a bin, on bins_log2 or on the
// table a job is in.  All scores equal puts a part into one bin: |pos| |neg| comparisons by one workgroup (include/wdg.h says so).
#include "stacked_row.h"

namespace {

using namespace wdg;

constexpr int AU_ROWS = 64, AU_THREADS = 256, AU_TILE = 1024;
constexpr int AU_MAX_JOBS = 65535;                 // gridDim.z: a job per z
constexpr int AU_SCAN_WGS = 64, AU_BIN_WGS = 512;  // workgroups per job of the scan (a replica each, strided) and of the in-bin count
constexpr int AU_SCAN_BINS = 4;                    // consecutive bins of a thread in one step of the scan
constexpr int AU_WAVES = AU_THREADS / kWave;

// the work space of a job (include/wdg.h: wdg_auc_workspace_bytes), B = 1 << bins_log2, G = 3 R groups g = 3 r + p:
//   acc   int64 [G]        the pairs across bins (stored by the scan), then + the pairs inside bins (integer adds)
//   tot   int32 [G][2]     the keyed negatives and positives of a group (stored by the scan)
//   nan   int32 [G][2]     the NaN rows of a group by class: zero between calls
//   cnt   int32 [G][B][2]  count: the rows of (bin, class); scan: where the next key of (bin, class) goes; zero between calls
//   start int32 [G][B]     where a bin's negatives start (stored by the scan); its positives start where its negatives end
//   keys  uint32 [R][n]    replica r's keys, bin-contiguous; every offset above is relative to r n
struct au_work {
    global_ptr<unsigned long long> acc;
    global_ptr<int32_t> tot, nan, cnt, start;
    global_ptr<uint32_t> keys;
};
__device__ __forceinline__ au_work au_carve(void *work, const int n, const int R, const int bins_log2) {
    const int64_t G = static_cast<int64_t>(R) * 3, B = int64_t{1} << bins_log2;
    au_work w;
    char *p = static_cast<char *>(work);
    w.acc = (global_ptr<unsigned long long>)p, p += 8 * G;
    w.tot = (global_ptr<int32_t>)p, p += 8 * G;
    w.nan = (global_ptr<int32_t>)p, p += 8 * G;
    w.cnt = (global_ptr<int32_t>)p, p += 8 * G * B;
    w.start = (global_ptr<int32_t>)p, p += 4 * G * B;
    w.keys = (global_ptr<uint32_t>)p;
    return w;
}

// what every launch skips and wdg_auc_check_jobs refuses (one predicate)
template <typename J>
__host__ __device__ __forceinline__ bool au_empty(const J job) {
    return job->n <= 0 || job->R <= 0;
}
template <typename J>
__host__ __device__ __forceinline__ bool au_malformed(const J job) {
    return job->n < 0 || job->R < 0 || job->cs < 2 || (job->n > 1 && job->ld_logits < static_cast<int64_t>(job->R) * job->cs) ||
           job->bins_log2 < 1 || job->bins_log2 > 16 || job->select < 0 || job->select > 1 || job->patience < 0 || job->curve_rows < 0 ||
           (job->curve_rows > 0 && job->curve_u2 == nullptr) ||
           (job->n > 0 && job->R > 0 && (job->logits == nullptr || job->labels == nullptr || job->split == nullptr || job->u2 == nullptr ||
                                         job->pairs == nullptr || job->best_u2 == nullptr || job->best == nullptr || job->state == nullptr ||
                                         job->work == nullptr || (reinterpret_cast<uintptr_t>(job->work) & 7) != 0));
}

// a pair's class (0 negative, 1 positive; -1: not counted), part and key
struct au_pair {
    int cls, part;
    uint32_t key;
    bool nan;
};
__device__ __forceinline__ au_pair au_read(const global_ptr<const float> logits, const global_ptr<const int32_t> labels,
                                           const global_ptr<const uint8_t> split, const int64_t ld, const int R, const int cs, const int i, const int r) {
    au_pair a{-1, 0, 0u, false};
    const unsigned code = split[static_cast<int64_t>(i) * R + r];
    const int lab = labels[i];
    if (code < 1 || code > 3 || lab < 0 || lab > 1) return a;
    const global_ptr<const float> z = logits + static_cast<int64_t>(i) * ld + static_cast<int64_t>(r) * cs;
    const float d = z[1] - z[0];
    a.cls = lab, a.part = static_cast<int>(code) - 1;
    a.nan = d != d;
    const uint32_t bits = d == 0.f ? 0u : __float_as_uint(d);  // (-0 -> +0)
    a.key = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return a;
}

// launches 1 and 3: count == true adds to the counters, count == false moves the keys through the cursors
template <bool count>
__global__ __launch_bounds__(AU_THREADS) void auc_rows_kernel(const wdg_auc_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_auc_job> job = (desc_ptr<wdg_auc_job>)(jobs + blockIdx.z);
    if (au_malformed(job) || au_empty(job)) return;
    const int n_all = job->n, R = job->R, cs = job->cs, bins_log2 = job->bins_log2;
    const int n = min(n_all, max_rows);
    const int i0 = blockIdx.x * AU_ROWS;
    if (i0 >= n) return;
    const int rows_here = min(AU_ROWS, n - i0);
    const global_ptr<const float> logits = to_global(job->logits);
    const global_ptr<const int32_t> labels = to_global(job->labels);
    const global_ptr<const uint8_t> split = to_global(job->split);
    const int64_t ld = job->ld_logits;
    const au_work w = au_carve(job->work, n_all, R, bins_log2);
    const int64_t B = int64_t{1} << bins_log2;
    const int64_t todo = static_cast<int64_t>(rows_here) * R;
    for (int64_t q = threadIdx.x; q < todo; q += AU_THREADS) {
        const int il = static_cast<int>(q / R), r = static_cast<int>(q - static_cast<int64_t>(il) * R);
        const au_pair a = au_read(logits, labels, split, ld, R, cs, i0 + il, r);
        if (a.cls < 0) continue;
        const int64_t g = static_cast<int64_t>(r) * 3 + a.part;
        if (a.nan) {
            if (count) atomicAdd((int32_t *)(w.nan + g * 2 + a.cls), 1);
            continue;
        }
        const int64_t at = (g * B + (a.key >> (32 - bins_log2))) * 2 + a.cls;
        int32_t *const counter = (int32_t *)(w.cnt + at);
        if (count) {
            atomicAdd(counter, 1);
        } else {
            const int32_t to = atomicAdd(counter, 1);
            if (to >= 0 && to < n_all) w.keys[static_cast<int64_t>(r) * n_all + to] = a.key;  // (the offsets are the scan's: inside the replica's n keys)
        }
    }
}

// the exclusive scan of one 64-bit value per thread over the workgroup (two int32 sums side by side: no carry crosses, both stay
// below 2^31) -> the sum of the threads before this one; total: the workgroup's sum.  lds: AU_WAVES words.  Two barriers.
__device__ __forceinline__ unsigned long long au_scan(const unsigned long long v, unsigned long long *lds, unsigned long long &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long up = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += up;
    }
    __syncthreads();  // (the previous step's readers are done with lds)
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < AU_WAVES; ++k) {
        const unsigned long long s = lds[k];
        if (k < wave) before += s;
        all += s;
    }
    total = all;
    return before + inc - v;
}

// launch 2: a workgroup per replica (strided).  The counters of a part in steps of AU_THREADS * AU_SCAN_BINS bins.
__global__ __launch_bounds__(AU_THREADS) void auc_scan_kernel(const wdg_auc_job *__restrict__ jobs) {
    __shared__ unsigned long long sums[AU_WAVES];
    __shared__ unsigned long long cross_of[AU_WAVES];
    const desc_ptr<wdg_auc_job> job = (desc_ptr<wdg_auc_job>)(jobs + blockIdx.z);
    if (au_malformed(job) || au_empty(job)) return;  // (uniform: before any barrier)
    const int n = job->n, R = job->R, bins_log2 = job->bins_log2;
    const au_work w = au_carve(job->work, n, R, bins_log2);
    const int B = 1 << bins_log2;
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {  // (uniform)
        unsigned int placed = 0;  // keys of this replica before the current step
        for (int p = 0; p < 3; ++p) {
            const int64_t g = static_cast<int64_t>(r) * 3 + p;
            unsigned int neg_below = 0, pos_below = 0;
            unsigned long long cross = 0;
            for (int b0 = 0; b0 < B; b0 += AU_THREADS * AU_SCAN_BINS) {
                const int mine = b0 + t * AU_SCAN_BINS;
                unsigned int nn[AU_SCAN_BINS], np[AU_SCAN_BINS], my_neg = 0, my_pos = 0;
#pragma unroll
                for (int k = 0; k < AU_SCAN_BINS; ++k) {
                    const bool in = mine + k < B;
                    nn[k] = in ? static_cast<unsigned int>(w.cnt[(g * B + mine + k) * 2]) : 0u;
                    np[k] = in ? static_cast<unsigned int>(w.cnt[(g * B + mine + k) * 2 + 1]) : 0u;
                    my_neg += nn[k], my_pos += np[k];
                }
                unsigned long long total;
                const unsigned long long before = au_scan((static_cast<unsigned long long>(my_pos) << 32) | my_neg, sums, total);
                unsigned int negs = neg_below + static_cast<unsigned int>(before & 0xFFFFFFFFull);
                unsigned int at = placed + negs + pos_below + static_cast<unsigned int>(before >> 32);
#pragma unroll
                for (int k = 0; k < AU_SCAN_BINS; ++k) {
                    if (mine + k < B) {
                        cross += 2ull * np[k] * negs;
                        w.start[g * B + mine + k] = static_cast<int32_t>(at);
                        w.cnt[(g * B + mine + k) * 2] = static_cast<int32_t>(at);
                        w.cnt[(g * B + mine + k) * 2 + 1] = static_cast<int32_t>(at + nn[k]);
                        negs += nn[k], at += nn[k] + np[k];
                    }
                }
                neg_below += static_cast<unsigned int>(total & 0xFFFFFFFFull), pos_below += static_cast<unsigned int>(total >> 32);
            }
            placed += neg_below + pos_below;
            // the workgroup's sum of cross
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) cross += __shfl_down(cross, d, kWave);
            __syncthreads();  // (cross_of's readers of the previous part are done)
            if (lane == 0) cross_of[wave] = cross;
            __syncthreads();
            if (t == 0) {
                unsigned long long s = 0;
#pragma unroll
                for (int k = 0; k < AU_WAVES; ++k) s += cross_of[k];
                w.acc[g] = s;
                w.tot[g * 2] = static_cast<int32_t>(neg_below), w.tot[g * 2 + 1] = static_cast<int32_t>(pos_below);
            }
        }
    }
}

// launch 4: the workgroups of a job walk the (group, bin) items in pieces of AU_THREADS; a thread reads its item's three offsets
// and puts the counters back to zero, the items with both classes are listed in LDS, and the workgroup counts them one after the other
__global__ __launch_bounds__(AU_THREADS) void auc_bins_kernel(const wdg_auc_job *__restrict__ jobs) {
    __shared__ uint32_t tile[AU_TILE];
    __shared__ int32_t list[AU_THREADS][4];  // replica, group, start of the negatives, of the positives | their end: below
    __shared__ int32_t ends[AU_THREADS];
    __shared__ int listed;
    __shared__ unsigned long long part_sum[AU_WAVES];
    const desc_ptr<wdg_auc_job> job = (desc_ptr<wdg_auc_job>)(jobs + blockIdx.z);
    if (au_malformed(job) || au_empty(job)) return;  // (uniform: before any barrier)
    const int n = job->n, R = job->R, bins_log2 = job->bins_log2;
    const au_work w = au_carve(job->work, n, R, bins_log2);
    const int64_t B = int64_t{1} << bins_log2, items = static_cast<int64_t>(R) * 3 * B;
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    for (int64_t m0 = static_cast<int64_t>(blockIdx.x) * AU_THREADS; m0 < items; m0 += static_cast<int64_t>(gridDim.x) * AU_THREADS) {  // (uniform)
        if (t == 0) listed = 0;
        __syncthreads();
        const int64_t m = m0 + t;  // = g B + b
        if (m < items) {
            const int32_t s = w.start[m], e0 = w.cnt[2 * m], e1 = w.cnt[2 * m + 1];
            w.cnt[2 * m] = 0, w.cnt[2 * m + 1] = 0;
            if (s >= 0 && s < e0 && e0 < e1 && e1 <= n) {  // (both classes; inside the replica's n keys)
                const int slot = atomicAdd(&listed, 1);
                const int g = static_cast<int>(m >> bins_log2);
                list[slot][0] = g / 3, list[slot][1] = g, list[slot][2] = s, list[slot][3] = e0, ends[slot] = e1;
            }
        }
        __syncthreads();
        const int n_listed = listed;
        for (int it = 0; it < n_listed; ++it) {  // (uniform)
            const int r = list[it][0], g = list[it][1], s = list[it][2], e0 = list[it][3], e1 = ends[it];
            const global_ptr<const uint32_t> keys = (global_ptr<const uint32_t>)(w.keys + static_cast<int64_t>(r) * n);
            unsigned long long mine = 0;
            for (int j0 = s; j0 < e0; j0 += AU_TILE) {  // a tile of the negatives
                const int tn = min(AU_TILE, e0 - j0);
                __syncthreads();  // (the previous tile's readers are done)
                for (int j = t; j < tn; j += AU_THREADS) tile[j] = keys[j0 + j];
                __syncthreads();
                for (int i = e0 + t; i < e1; i += AU_THREADS) {  // a positive per thread
                    const uint32_t pk = keys[i];
                    unsigned int c = 0;  // (at most 2 AU_TILE)
                    for (int j = 0; j < tn; ++j) {
                        const uint32_t nk = tile[j];
                        c += (nk < pk ? 1u : 0u) + (nk <= pk ? 1u : 0u);
                    }
                    mine += c;
                }
            }
#pragma unroll
            for (int d = kWave / 2; d >= 1; d >>= 1) mine += __shfl_down(mine, d, kWave);
            __syncthreads();  // (part_sum's reader of the previous item is done)
            if (lane == 0) part_sum[wave] = mine;
            __syncthreads();
            if (t == 0) {
                unsigned long long sum = 0;
#pragma unroll
                for (int k = 0; k < AU_WAVES; ++k) sum += part_sum[k];
                if (sum) atomicAdd((unsigned long long *)(w.acc + g), sum);
            }
        }
        __syncthreads();  // (the next piece rewrites the list)
    }
}

// launch 5: a workgroup per job, a thread per replica (strided)
__global__ __launch_bounds__(AU_THREADS) void auc_finish_kernel(const wdg_auc_job *__restrict__ jobs, const int32_t *__restrict__ step_dev) {
    const desc_ptr<wdg_auc_job> job = (desc_ptr<wdg_auc_job>)(jobs + blockIdx.x);
    if (au_malformed(job) || au_empty(job)) return;
    const int n = job->n, R = job->R, select = job->select, patience = job->patience, curve_rows = job->curve_rows;
    const au_work w = au_carve(job->work, n, R, job->bins_log2);
    const global_ptr<int64_t> u2 = to_global(job->u2), pairs = to_global(job->pairs), best_u2 = to_global(job->best_u2),
                              curve_u2 = to_global(job->curve_u2);
    const global_ptr<int32_t> best = to_global(job->best), state = to_global(job->state);
    const int32_t step = *step_dev;
    const bool curve = step >= 0 && step < curve_rows;
    for (int r = threadIdx.x; r < R; r += AU_THREADS) {
        int64_t v[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const int64_t g = static_cast<int64_t>(r) * 3 + p;
            const int64_t nan_neg = w.nan[2 * g], nan_pos = w.nan[2 * g + 1];
            w.nan[2 * g] = 0, w.nan[2 * g + 1] = 0;
            v[p] = nan_neg + nan_pos > 0 ? int64_t{-1} : static_cast<int64_t>(w.acc[g]);
            u2[g] = v[p];
            pairs[g] = (w.tot[2 * g] + nan_neg) * (w.tot[2 * g + 1] + nan_pos);
            if (curve) curve_u2[(static_cast<int64_t>(step) * R + r) * 3 + p] = v[p];
        }
        if (select == 1 && state[2 * r + 1] < 0) {  // (a stopped replica's best, best_u2 and state never change again)
            int32_t bad = state[2 * r];
            if (v[1] >= 0 && v[1] > best_u2[3 * r + 1]) {
#pragma unroll
                for (int p = 0; p < 3; ++p) best_u2[3 * r + p] = v[p];
                best[3 * r] = 0, best[3 * r + 1] = 0, best[3 * r + 2] = step;
                bad = 0;
            } else {
                bad += 1;
            }
            state[2 * r] = bad;
            if (patience > 0 && bad >= patience) state[2 * r + 1] = step;
        }
    }
}

}  // namespace

extern "C" int64_t wdg_auc_workspace_bytes(int32_t n, int32_t R, int32_t bins_log2) {
    if (bins_log2 < 1 || bins_log2 > 16) return -1;
    if (n <= 0 || R <= 0) return 0;
    const int64_t B = int64_t{1} << bins_log2;
    return 72 * static_cast<int64_t>(R) + 36 * static_cast<int64_t>(R) * B + 4 * static_cast<int64_t>(n) * R;
}

extern "C" int wdg_auc_check_jobs(const wdg_auc_job *jobs_host, int32_t n_jobs) {
    WDG_REQUIRE(n_jobs >= 0, "auc_check_jobs: negative count");
    WDG_REQUIRE(n_jobs == 0 || jobs_host != nullptr, "auc_check_jobs: null job table");
    for (int32_t j = 0; j < n_jobs; ++j) {
        const wdg_auc_job *job = jobs_host + j;
        WDG_REQUIRE(job->cs >= 2, "auc_check_jobs: job %d: a replica stride of %d columns; a binary model has 2", j, job->cs);
        WDG_REQUIRE(job->bins_log2 >= 1 && job->bins_log2 <= 16, "auc_check_jobs: job %d: bins_log2 %d; 1 .. 16", j, job->bins_log2);
        WDG_REQUIRE(job->select >= 0 && job->select <= 1, "auc_check_jobs: job %d: select %d; 0 or 1", j, job->select);
        WDG_REQUIRE(job->patience >= 0, "auc_check_jobs: job %d: a patience of %d", j, job->patience);
        WDG_REQUIRE(job->curve_rows >= 0, "auc_check_jobs: job %d: %d curve rows", j, job->curve_rows);
        WDG_REQUIRE(!au_malformed(job), "auc_check_jobs: job %d: n %d, R %d, cs %d, ld_logits %lld: a row of R cs columns, no NULL pointer, an 8-byte "
                    "aligned work space and the curve buffer with curve_rows > 0 expected", j, job->n, job->R, job->cs, static_cast<long long>(job->ld_logits));
    }
    return WDG_OK;
}

extern "C" int wdg_auc_batched_i64(const wdg_auc_job *jobs_dev, int32_t n_jobs, int32_t max_rows, const int32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0, "auc_batched: negative count");
    WDG_REQUIRE(step_dev != nullptr, "auc_batched: null step word");
    WDG_REQUIRE(n_jobs <= AU_MAX_JOBS, "auc_batched: %d jobs; one launch takes %d", n_jobs, AU_MAX_JOBS);
    WDG_REQUIRE(n_jobs == 0 || jobs_dev != nullptr, "auc_batched: null job table");
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const hipStream_t st = wdg::as_stream(stream);
    const unsigned z = static_cast<unsigned>(n_jobs);
    const dim3 rows(static_cast<unsigned>(wdg::ceil_div(max_rows, AU_ROWS)), 1, z);
    hipLaunchKernelGGL(auc_rows_kernel<true>, rows, dim3(AU_THREADS), 0, st, jobs_dev, max_rows);
    int rc = wdg::check_launch("auc_rows_kernel (count)");
    if (rc != WDG_OK) return rc;
    hipLaunchKernelGGL(auc_scan_kernel, dim3(AU_SCAN_WGS, 1, z), dim3(AU_THREADS), 0, st, jobs_dev);
    rc = wdg::check_launch("auc_scan_kernel");
    if (rc != WDG_OK) return rc;
    hipLaunchKernelGGL(auc_rows_kernel<false>, rows, dim3(AU_THREADS), 0, st, jobs_dev, max_rows);
    rc = wdg::check_launch("auc_rows_kernel (scatter)");
    if (rc != WDG_OK) return rc;
    hipLaunchKernelGGL(auc_bins_kernel, dim3(AU_BIN_WGS, 1, z), dim3(AU_THREADS), 0, st, jobs_dev);
    rc = wdg::check_launch("auc_bins_kernel");
    if (rc != WDG_OK) return rc;
    hipLaunchKernelGGL(auc_finish_kernel, dim3(z), dim3(AU_THREADS), 0, st, jobs_dev, step_dev);
    return wdg::check_launch("auc_finish_kernel");
}
