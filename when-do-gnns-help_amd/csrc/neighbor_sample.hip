// GraphSAGE's neighbour sampling (Hamilton, Ying, Leskovec: "Inductive Representation Learning on Large Graphs", NeurIPS 2017) on the
// device: per training step, EXACTLY `fanout` of every row's eligible entries, uniformly and without replacement, written as the thinned
// PATTERN that csrc/drop_edge.hip's aggregation (wdg_spmm_thinned_batched_f32) walks - and the same edges on the transposed pattern, for
// the backward pass, without a position map.
//
// why:      DropEdge's draw is a pure function of the entry; "s of this row's entries" is an order statistic of the ROW.  Composed by
//           hand - random keys per entry, a per-row sort or top-k, a mask gathered through transpose_positions - it stores a mask, cannot
//           redraw inside a captured epoch and pays a segmented sort per step.
// replaces: nothing of the reference, which ships no model code (its loaders only carry the switch: `sage_data`,
//           utils/util_funcs.py:207, 342): the pass restates the degree part of its normalisation on the KEPT entries - normalize,
//           utils/util_funcs.py:29-36, and normalize_tensor, utils/util_funcs.py:365-380 - for the models that stand beside the tables
//           of gnns_on_syn.py:9-53.
//
// THE CONTRACT (include/wdg.h states it in full; tests/_neighbor_sample_ref.py restates it in numpy): an entry's 64-bit KEY is a Philox
// word of its FORWARD coordinates above its column - a total order within a row -, tau[i] is the fanout-th smallest key of row i's eligible
// entries (2^64 - 1 where there are fewer), and an entry is kept when its key is <= tau of its FORWARD row.  So the transposed job needs
// tau and nothing else: phase 0 selects and writes tau, phase 1 reads tau[j] at each stored column.  Integer arithmetic plus one scale per
// row; no LDS, no atomics, no scratch, no per-thread array.
//
// Phase 0: a WAVE owns a row, four rows per workgroup, a job per grid y.  A row of fewer than `fanout` stored entries keeps every valid
// one: nothing is drawn for it.  A longer row goes in chunks of 64 entries, one per lane; lane l holds the rank-l smallest key seen so
// far as a 64-bit word (2^64 - 1 = nothing; the candidate set of csrc/topk_rows.hip, restated ascending).  A chunk is looked at only
// when a ballot finds a key below the current fanout-th; up to NS_INSERT_MAX entrants are inserted one by one (a scalar lane read, a
// ballot for the rank, one lane shift), more are sorted (bitonic) and merged.  Both routes leave ranks 0 .. fanout - 1 exact, so which
// one ran cannot show.  A second pass over the chunks recomputes each key, compares with tau and compacts (ballot + mbcnt:
// csrc/wave_rows.h's thinned row, the one drop_edge_thin_kernel writes).  There is NO multi-wave path for a hub row.
// Phase 1: the same compaction pass over the transposed pattern with tau read per entry.
#include <cmath>
#include <cstdint>

#include "philox.h"
#include "wave_rows.h"
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int NS_WAVES = 4;         // rows per workgroup
constexpr int NS_INSERT_MAX = 8;    // up to this many entrants of a chunk are inserted one by one; more: sort + merge
constexpr unsigned NS_KEY_TAG = 0x53414745u;  // "SAGE": the second key word of the step key
constexpr int NS_KNOWN_FLAGS = WDG_NEIGHBOR_SAMPLE_TRANSPOSED | WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL | WDG_NEIGHBOR_SAMPLE_NORM_SYM;
constexpr uint64_t NS_NOTHING = ~0ull;  // no key of an entry with a column inside the pattern is 2^64 - 1 (its low word is < 2^31)
static_assert(WDG_NEIGHBOR_SAMPLE_MAX_FANOUT == kWave, "a lane per held key");

// what the kernels skip and wdg_neighbor_sample_check_jobs refuses (the part that reads no address arithmetic)
template <typename J>
__host__ __device__ __forceinline__ bool ns_malformed(const J job) {
    const bool forward = !(job->flags & WDG_NEIGHBOR_SAMPLE_TRANSPOSED);
    return job->n < 0 || job->n_cols < 0 || job->nnz < 0 || (job->flags & ~NS_KNOWN_FLAGS) != 0 ||
           (forward && (job->fanout < 1 || job->fanout > WDG_NEIGHBOR_SAMPLE_MAX_FANOUT)) ||
           (job->n > 0 && (!job->rowptr || !job->kept_len || (forward && !job->tau))) ||
           (job->n > 0 && job->nnz > 0 && (!job->col || !job->kept_col || job->kept_col == job->col || !job->tau));
}

// the key of the entry with FORWARD coordinates (i, j)
__device__ __forceinline__ uint64_t ns_key(const unsigned i, const unsigned j, const unsigned k0, const unsigned k1) {
    return (static_cast<uint64_t>(philox4x32_10(i, j, k0, k1)) << 32) | j;
}

// lane `src`'s word in every lane (src is wave-uniform)
__device__ __forceinline__ uint64_t ns_readlane(const uint64_t w, const int src) {
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(w)), src);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(w >> 32)), src);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t ns_max(const uint64_t a, const uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t ns_min(const uint64_t a, const uint64_t b) { return a < b ? a : b; }

// the wave's 64 words in ascending order over the lanes (bitonic sorting network; NS_NOTHING ends up last)
__device__ __forceinline__ uint64_t ns_sort_asc(uint64_t w, const int lane) {
#pragma unroll
    for (int size = 2; size <= kWave; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            const uint64_t p = __shfl_xor(w, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & size) == 0);
            w = keep_min ? ns_min(w, p) : ns_max(w, p);
        }
    }
    return w;
}

// held and chunk both ascending -> the 64 smallest of the 128, ascending
__device__ __forceinline__ uint64_t ns_merge_asc(const uint64_t held, const uint64_t chunk, const int lane) {
    uint64_t w = ns_min(held, __shfl(chunk, kWave - 1 - lane));  // bitonic, and it holds the 64 smallest
#pragma unroll
    for (int j = kWave >> 1; j > 0; j >>= 1) {
        const uint64_t p = __shfl_xor(w, j);
        w = (lane & j) == 0 ? ns_min(w, p) : ns_max(w, p);
    }
    return w;
}

// The compaction pass both phases share.  FORWARD: the row is forward row `row`, every entry compares with the one `tau_row`
// (NS_NOTHING: every valid entry is kept and nothing is drawn).  Transposed: the entry (row, j) is forward (j, row) and compares with
// tau[j], read only where j is a valid column.
template <bool FORWARD>
__device__ __forceinline__ void ns_compact(const desc_ptr<wdg_neighbor_sample_job> job, const int row, const int beg, const int end, const int lane,
                                           const unsigned k0, const unsigned k1, const uint64_t tau_row) {
    const int n_cols = job->n_cols, flags = job->flags;
    const bool diagonal = flags & WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<int32_t> kept_col = to_global(job->kept_col);
    const global_ptr<const uint64_t> tau = to_global(static_cast<const uint64_t *>(job->tau));
    int kept = 0;  // (wave-uniform) kept entries of the chunks so far
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);
        const int j = lane < cnt ? col[e0 + lane] : -1;
        const bool valid = static_cast<unsigned>(j) < static_cast<unsigned>(n_cols);
        bool keep = valid;
        if (FORWARD) {
            if (tau_row != NS_NOTHING)  // (wave-uniform)
                keep = valid && ((diagonal && j == row) || ns_key(static_cast<unsigned>(row), static_cast<unsigned>(j), k0, k1) <= tau_row);
        } else {
            const uint64_t t = valid ? tau[j] : 0ull;
            keep = valid && ((diagonal && j == row) || ns_key(static_cast<unsigned>(j), static_cast<unsigned>(row), k0, k1) <= t);
        }
        thinned_row_keep(kept_col, beg, kept, keep, j);
    }
    thinned_row_finish(job, kept_col, row, beg, end, kept, lane, flags & WDG_NEIGHBOR_SAMPLE_NORM_SYM);
}

template <bool FORWARD>
__global__ __launch_bounds__(64 * NS_WAVES) void neighbor_sample_kernel(const wdg_neighbor_sample_job *__restrict__ jobs, const int max_rows,
                                                                        const unsigned seed, const unsigned *__restrict__ step_dev) {
    const desc_ptr<wdg_neighbor_sample_job> job = (desc_ptr<wdg_neighbor_sample_job>)(jobs + blockIdx.y);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int flags = job->flags, nnz = job->nnz;
    const int row = blockIdx.x * NS_WAVES + wave;
    if (FORWARD == static_cast<bool>(flags & WDG_NEIGHBOR_SAMPLE_TRANSPOSED)) return;  // the other phase's job
    if (row >= min(job->n, max_rows)) return;  // (wave-uniform, like everything up to the chunk loops)
    if (ns_malformed(job)) return;             // a job outside the contract is left untouched (the host predicate refuses it)
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;

    const philox_words key = philox4x32_10_words(*step_dev, job->stream, seed, NS_KEY_TAG);  // the step key: uniform
    const unsigned k0 = key.w[0], k1 = key.w[1];
    uint64_t kth = NS_NOTHING;  // the fanout-th smallest key so far, wave-uniform
    if (FORWARD) {
        const int fanout = job->fanout, n_cols = job->n_cols;
        if (end - beg >= fanout) {  // (a shorter row has fewer than fanout eligible entries: tau = 2^64 - 1 without a draw)
            const bool diagonal = flags & WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL;
            const global_ptr<const int32_t> col = to_global(job->col);
            uint64_t held = NS_NOTHING;
            for (int e0 = beg; e0 < end; e0 += 64) {
                const int cnt = min(64, end - e0);
                const int j = lane < cnt ? col[e0 + lane] : -1;
                const bool eligible = static_cast<unsigned>(j) < static_cast<unsigned>(n_cols) && !(diagonal && j == row);
                const uint64_t w = eligible ? ns_key(static_cast<unsigned>(row), static_cast<unsigned>(j), k0, k1) : NS_NOTHING;
                // (a key EQUAL to the fanout-th - a second copy of that column - changes no rank below fanout: it need not enter)
                uint64_t cand = __ballot(w < kth);
                if (cand == 0ull) continue;  // (wave-uniform)
                if (__popcll(cand) <= NS_INSERT_MAX) {
                    do {
                        const int src = __builtin_ctzll(cand);
                        cand &= cand - 1ull;
                        const uint64_t c = ns_readlane(w, src);
                        const int pos = __popcll(__ballot(held < c));  // held is ascending: lanes 0 .. pos - 1 rank before c
                        const uint64_t up = __shfl_up(held, 1);
                        held = lane < pos ? held : (lane == pos ? c : up);
                    } while (cand != 0ull);
                } else {
                    held = ns_merge_asc(held, ns_sort_asc(w, lane), lane);
                }
                kth = ns_readlane(held, fanout - 1);
            }
        }
        if (lane == 0) to_global(job->tau)[row] = kth;
    }
    ns_compact<FORWARD>(job, row, beg, end, lane, k0, k1, kth);
}

}  // namespace

extern "C" int wdg_neighbor_sample_batched(const wdg_neighbor_sample_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t phase, uint32_t seed,
                                           const uint32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(max_rows >= 0, "neighbor_sample_batched: negative count");
    if (const int rc = wdg::check_job_table("neighbor_sample_batched", jobs_dev, n_jobs)) return rc;
    WDG_REQUIRE(phase == 0 || phase == 1, "neighbor_sample_batched: unknown phase %d; 0 (select and thin the forward jobs) and 1 (thin the transposed jobs) are defined", phase);
    WDG_REQUIRE(step_dev != nullptr, "neighbor_sample_batched: null step word");
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    const dim3 grid(static_cast<unsigned>(wdg::ceil_div(max_rows, NS_WAVES)), static_cast<unsigned>(n_jobs)), block(64 * NS_WAVES);
    if (phase == 0) {
        hipLaunchKernelGGL(neighbor_sample_kernel<true>, grid, block, 0, wdg::as_stream(stream), jobs_dev, max_rows, seed, step_dev);
        return wdg::check_launch("neighbor_sample_kernel<forward>");
    }
    hipLaunchKernelGGL(neighbor_sample_kernel<false>, grid, block, 0, wdg::as_stream(stream), jobs_dev, max_rows, seed, step_dev);
    return wdg::check_launch("neighbor_sample_kernel<transposed>");
}

// The per-job part of the contract, for a table the caller still holds on the host (neighbor_sample.NeighborSampleBatch calls this on the
// table it is about to upload).
extern "C" int wdg_neighbor_sample_check_jobs(const wdg_neighbor_sample_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("neighbor_sample_check_jobs", jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_neighbor_sample_job &j = jobs_host[i];
        const bool forward = !(j.flags & WDG_NEIGHBOR_SAMPLE_TRANSPOSED);
        WDG_REQUIRE(j.n >= 0 && j.n_cols >= 0 && j.nnz >= 0, "neighbor_sample_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE((j.flags & 1) == 0, "neighbor_sample_check_jobs: job %d sets the flag bit of value 1: there is no tied form (a fan-out belongs to the receiving row)", i);
        WDG_REQUIRE((j.flags & ~NS_KNOWN_FLAGS) == 0, "neighbor_sample_check_jobs: job %d has unknown flag bits 0x%x", i, j.flags & ~NS_KNOWN_FLAGS);
        WDG_REQUIRE(!forward || (j.fanout >= 1 && j.fanout <= WDG_NEIGHBOR_SAMPLE_MAX_FANOUT), "neighbor_sample_check_jobs: job %d has a fan-out of %d; 1 .. %d are supported", i,
                    j.fanout, WDG_NEIGHBOR_SAMPLE_MAX_FANOUT);
        if (j.n == 0) continue;
        WDG_REQUIRE(j.rowptr && j.kept_len, "neighbor_sample_check_jobs: job %d has a null rowptr or kept_len", i);
        WDG_REQUIRE(j.tau || (!forward && j.nnz == 0), "neighbor_sample_check_jobs: job %d has a null tau", i);
        if (j.nnz == 0) continue;
        WDG_REQUIRE(j.col && j.kept_col, "neighbor_sample_check_jobs: job %d has a null col or kept_col", i);
        const uintptr_t a = reinterpret_cast<uintptr_t>(j.col), b = reinterpret_cast<uintptr_t>(j.kept_col), bytes = static_cast<uintptr_t>(j.nnz) * 4;
        WDG_REQUIRE(a + bytes <= b || b + bytes <= a, "neighbor_sample_check_jobs: job %d's kept_col overlaps its col (the pass does not run in place)", i);
        WDG_REQUIRE(!ns_malformed(&j), "neighbor_sample_check_jobs: job %d is malformed", i);
    }
    return WDG_OK;
}
