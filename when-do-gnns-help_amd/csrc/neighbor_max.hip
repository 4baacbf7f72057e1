// The neighbour MAXIMUM and its backward pass (wdg_neighbor_max_batched_f32, wdg_neighbor_max_backward_batched_f32): the pooling
// aggregator of GraphSAGE (Hamilton, Ying, Leskovec: "Inductive Representation Learning on Large Graphs", NeurIPS 2017) over a plain
// CSR pattern or over a thinned pattern as csrc/drop_edge.hip and csrc/neighbor_sample.hip leave it.
//
// why:      every aggregation of the project is a weighted sum over a row's stored entries; a per-column maximum over the neighbours
//           is not a low-pass average at all.  Composed in torch - x[col] gathered into [nnz, F], scatter_reduce(amax) - it has no
//           thinned-pattern form, cannot follow the per-step samples inside a captured epoch and splits a tie's gradient.
// replaces: nothing of the reference, which ships no model code: it stands where the product with the normalised adjacency - normalize,
//           utils/util_funcs.py:29-36, and normalize_tensor, utils/util_funcs.py:365-380 - stands in the other models, beside the
//           tables of gnns_on_syn.py:9-53.
//
// THE CONTRACT (include/wdg.h states it in full; tests/_neighbor_max_ref.py restates it in numpy): the winner of (row, column) is the
// greatest pair (X[j, f], j) over the SET of the row's eligible entries under a TOTAL order - a NaN above everything, -0 == +0, among
// equals the lower j - and Y gets its bits, arg its j.  The maximum of a total order is associative and commutative, so - unlike every
// sum of this library - the row may be walked in any order and in pieces with the same bits.
//
// Forward: a WAVE owns a row and a PANEL of 256 columns (grid y), four columns per lane.  A panel of w columns needs ceil(w / 4) lanes;
// rounded up to a power of two that is P, and the wave holds S = 64 / P SHARES: lane l works columns 4 (l % P) .. + 3 on the entries
// e with e % S == l / P.  At class width (n_feat <= 16) P = 4 and S = 16: sixteen entries are in flight per step where a chain would
// have one.  Every lane reads its own entry's column index (the lanes of a share read one address) and its row piece of X - a 16-byte
// load where the job's pointer, leading dimension and width allow, the wave's decision -, up to 8 steps ahead of the first compare.
// A lane keeps per column the best 64-bit word (key << 32 | ~j: greater = wins) and the winner's bits; at the end the shares are merged
// with log2(S) xor-shuffles under the same order.  There is NO multi-wave path for a hub row (DESIGN 4.34 has the timing that decided).
// Backward: a WAVE owns a row of the TRANSPOSED pattern and a panel; the chain acc += G[i, f] where arg[i, f] == j runs in stored order,
// ONE add per entry - a sum depends on its order, so the CHAIN is not shared out: the lanes of share 0 add every term in entry order.
// The LOADS are: the entries are read 64 at a time, one per lane, the duplicate rule is settled with a ballot, and share t requests
// the arg and G pieces of every S-th entry, NB_DEPTH x S entries in flight before the first add; a term reaches its chain through a
// cross-lane read, as +0 where nothing is to be added (which changes no bit: the chain starts at +0 and never holds -0).
// No LDS, no atomics, no scratch.
#include <cstdint>

#include "neighbor_order.h"
#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // the backward chain is restated bit for bit: nothing may be fused

namespace {

using namespace wdg;

constexpr int NM_WAVES = 4;           // rows per workgroup, both kernels
constexpr int NM_PANEL = 256;         // columns per wave: four per lane
constexpr int NM_MAX_PANELS = 65535;  // gridDim.y
constexpr int NB_DEPTH = 8;           // backward: row loads in flight before the first add of a batch
constexpr int NM_KNOWN_FLAGS = WDG_NEIGHBOR_MAX_MIN;

// (the order itself - nm_key, the image of a value, and nm_shfl_xor64, a lane's word across lanes - is csrc/neighbor_order.h's)

// one step of the lane's share: the U entries e0 + u S + s (those below len), all requested before the first compare
template <bool VEC, int U>
__device__ __forceinline__ void nm_step(const global_ptr<const uint32_t> x_lane, const int64_t ld, const int live, const global_ptr<const int32_t> col,
                                        const int e0, const int len, const int n_cols, const int s, const int S, const bool minimum, uint64_t (&best)[4],
                                        uint32_t (&bits)[4]) {
    int j[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int e = e0 + u * S + s;
        j[u] = e < len ? col[e] : -1;
        if (static_cast<unsigned>(j[u]) >= static_cast<unsigned>(n_cols)) j[u] = -1;  // skipped, never read through
    }
    if (live > 0) {
        uint32_t x[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) load4<VEC>(x_lane + static_cast<int64_t>(max(j[u], 0)) * ld, live, x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t tie = ~static_cast<uint32_t>(j[u]);  // the lower j is the greater word
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t w = static_cast<uint64_t>(nm_key(x[u][k], minimum)) << 32 | tie;
                const bool wins = j[u] >= 0 && w > best[k];
                best[k] = wins ? w : best[k];
                bits[k] = wins ? x[u][k] : bits[k];
            }
        }
    }
}
// the lane's share of the row: entries s, s + S, .. below len, in steps of 8, 4, 2 and 1 entries per share (drop_edge.hip's schedule: a
// long row keeps 8 S loads in flight, a short one requests little it does not need).  Wave-uniform trip counts: every lane is active at
// the merge behind it.
template <bool VEC>
__device__ __forceinline__ void nm_share(const global_ptr<const uint32_t> x_lane, const int64_t ld, const int live, const global_ptr<const int32_t> col,
                                         const int len, const int n_cols, const int s, const int S, const bool minimum, uint64_t (&best)[4],
                                         uint32_t (&bits)[4]) {
    int e0 = 0;
    for (; e0 + 8 * S <= len; e0 += 8 * S) nm_step<VEC, 8>(x_lane, ld, live, col, e0, len, n_cols, s, S, minimum, best, bits);
    if (e0 + 4 * S <= len) nm_step<VEC, 4>(x_lane, ld, live, col, e0, len, n_cols, s, S, minimum, best, bits), e0 += 4 * S;
    if (e0 + 2 * S <= len) nm_step<VEC, 2>(x_lane, ld, live, col, e0, len, n_cols, s, S, minimum, best, bits), e0 += 2 * S;
    for (; e0 < len; e0 += S) nm_step<VEC, 1>(x_lane, ld, live, col, e0, len, n_cols, s, S, minimum, best, bits);  // (at most twice)
}

__global__ __launch_bounds__(64 * NM_WAVES) void neighbor_max_kernel(const wdg_neighbor_max_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_neighbor_max_job> job = (desc_ptr<wdg_neighbor_max_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_cols = job->n_cols, n_feat = job->n_feat, nnz = job->nnz, flags = job->flags;
    const int row = blockIdx.x * NM_WAVES + wave, panel0 = blockIdx.y * NM_PANEL;
    if (row >= min(job->n_rows, max_rows) || panel0 >= n_feat) return;  // (wave-uniform, like everything up to the lane's columns)
    // a job outside the contract is left untouched (wdg_neighbor_max_check_jobs refuses it on the host)
    if (n_cols < 0 || nnz < 0 || (flags & ~NM_KNOWN_FLAGS) || job->reserved != 0 || job->ldx < n_feat || job->ldy < n_feat ||
        (job->arg && job->lda < n_feat) || !job->rowptr || !job->Y)
        return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    int len = thinned_row_len(job->kept_len, row, beg, end);
    if (n_cols == 0 || !job->col || !job->X) len = 0;  // (nothing to look at: every entry is skipped)

    // the lanes the panel's columns need, rounded up to a power of two: P; the S = 64 / P shares of the row's entries
    const int used = (min(NM_PANEL, n_feat - panel0) + 3) >> 2;  // 1 .. 64
#ifdef NM_NO_SPLIT
    const int lg = 6;  // (the timing variant of scripts/time_neighbor_max.py: one share, the idle lanes stay idle)
#else
    const int lg = used <= 1 ? 0 : 32 - __builtin_clz(static_cast<unsigned>(used - 1));
#endif
    const int P = 1 << lg, S = 64 >> lg;
    const int c = lane & (P - 1), s = lane >> lg;
    const int c0 = panel0 + 4 * c, live = max(0, min(4, n_feat - c0));
    const bool minimum = flags & WDG_NEIGHBOR_MAX_MIN;

    uint64_t best[4] = {0, 0, 0, 0};  // 0: no eligible entry yet
    uint32_t bits[4] = {0, 0, 0, 0};
    const global_ptr<const uint32_t> x_lane = (global_ptr<const uint32_t>)to_global(job->X) + c0;
    const global_ptr<const int32_t> col = to_global(job->col) + beg;
    const bool vec = (n_feat & 3) == 0 && aligned16(job->X, job->ldx);
    if (vec) nm_share<true>(x_lane, job->ldx, live, col, len, n_cols, s, S, minimum, best, bits);
    else nm_share<false>(x_lane, job->ldx, live, col, len, n_cols, s, S, minimum, best, bits);
    // the shares of one column group sit P lanes apart: merged under the same order (EVERY lane is active here)
    for (int off = P; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t w = nm_shfl_xor64(best[k], off);
            const uint32_t b = static_cast<uint32_t>(__shfl_xor(static_cast<int>(bits[k]), off));
            const bool wins = w > best[k];
            best[k] = wins ? w : best[k];
            bits[k] = wins ? b : bits[k];
        }
    }
    if (s != 0 || live == 0) return;
    uint32_t who[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        who[k] = best[k] ? ~static_cast<uint32_t>(best[k]) : 0xffffffffu;  // the winner's j, or -1
        bits[k] = best[k] ? bits[k] : 0u;                                  // ... its bits, or +0
    }
    const global_ptr<uint32_t> y = (global_ptr<uint32_t>)to_global(job->Y) + static_cast<int64_t>(row) * job->ldy + c0;
    if ((n_feat & 3) == 0 && aligned16(job->Y, job->ldy)) store4<true>(y, live, bits);
    else store4<false>(y, live, bits);
    if (job->arg) {
        const global_ptr<uint32_t> a = (global_ptr<uint32_t>)to_global(job->arg) + static_cast<int64_t>(row) * job->lda + c0;
        if ((n_feat & 3) == 0 && aligned16(job->arg, job->lda)) store4<true>(a, live, who);
        else store4<false>(a, live, who);
    }
}

// D x S consecutive entries of the chunk the wave holds, from d0: the LOADS are shared out as in the forward pass - share t requests
// the arg and G pieces of the entries d0 + u S + t -, the CHAIN is not: the lanes of share 0 take every term in entry order through
// D x S cross-lane reads and add it.  A term is G[i, f] where arg[i, f] == row, +0 elsewhere (an entry that is skipped, or past the
// chunk's end, included): adding +0 changes no bit, because the chain starts at +0 and a sum of two floats is -0 only when both are -
// acc is never -0.  src: lane d holds the source row of entry d, or -1.  EVERY lane is active at the cross-lane reads.
template <int D, bool VEC_G, bool VEC_A>
__device__ __forceinline__ void nb_batch(const global_ptr<const uint32_t> g_lane, const int64_t ldg, const global_ptr<const uint32_t> a_lane, const int64_t lda,
                                         const int live, const int src, const int d0, const int cnt, const uint32_t me, const int c, const int s,
                                         const int P, const int S, float (&acc)[4]) {
    int r[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
        const int d = d0 + u * S + s;
        const int got = __shfl(src, d & 63);
        r[u] = d < cnt ? got : -1;
    }
    float term[D][4];
    if (live > 0) {
        uint32_t a[D][4], g[D][4];
#pragma unroll
        for (int u = 0; u < D; ++u) {
            load4<VEC_A>(a_lane + static_cast<int64_t>(max(r[u], 0)) * lda, live, a[u]);
            load4<VEC_G>(g_lane + static_cast<int64_t>(max(r[u], 0)) * ldg, live, g[u]);
        }
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) term[u][k] = (r[u] >= 0 && a[u][k] == me) ? __uint_as_float(g[u][k]) : 0.f;
    } else {
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) term[u][k] = 0.f;
    }
    if (S == 1) {  // (every lane holds its own terms)
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] + term[u][k];
    } else {
#pragma unroll
        for (int u = 0; u < D; ++u)
            for (int t = 0; t < S; ++t)  // entry d0 + u S + t sits with share t, P lanes apart
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = acc[k] + __shfl(term[u][k], c + t * P);
    }
}

template <bool VEC_G, bool VEC_A>
__device__ __forceinline__ void nb_row(const global_ptr<const uint32_t> g_lane, const int64_t ldg, const global_ptr<const uint32_t> a_lane, const int64_t lda,
                                       const int live, const global_ptr<const int32_t> col, const int len, const int n_src, const int lane,
                                       const uint32_t me, const int c, const int s, const int P, const int S, float (&acc)[4]) {
    int last = -1;  // (wave-uniform) the i of the latest entry that was not out of range
    for (int e0 = 0; e0 < len; e0 += 64) {
        const int cnt = min(64, len - e0);  // (wave-uniform)
        int src = lane < cnt ? col[e0 + lane] : -1;
        if (static_cast<unsigned>(src) >= static_cast<unsigned>(n_src)) src = -1;
        // the duplicate rule: the entry before this one that was in range - in this chunk, or `last`
        const unsigned long long votes = __ballot(src >= 0);
        const unsigned long long below = votes & ((1ull << lane) - 1ull);
        const int from = below ? 63 - __builtin_clzll(below) : lane;
        const int before = __shfl(src, from);
        const int prev = below ? before : last;
        if (votes) last = __builtin_amdgcn_readlane(src, 63 - __builtin_clzll(votes));
        if (src == prev) src = -1;  // (prev == -1 only where src == -1 already, or where nothing came before)
        int d0 = 0;
        for (; d0 + NB_DEPTH * S <= cnt; d0 += NB_DEPTH * S) nb_batch<NB_DEPTH, VEC_G, VEC_A>(g_lane, ldg, a_lane, lda, live, src, d0, cnt, me, c, s, P, S, acc);
        if (d0 + 4 * S <= cnt) nb_batch<4, VEC_G, VEC_A>(g_lane, ldg, a_lane, lda, live, src, d0, cnt, me, c, s, P, S, acc), d0 += 4 * S;
        if (d0 + 2 * S <= cnt) nb_batch<2, VEC_G, VEC_A>(g_lane, ldg, a_lane, lda, live, src, d0, cnt, me, c, s, P, S, acc), d0 += 2 * S;
        for (; d0 < cnt; d0 += S) nb_batch<1, VEC_G, VEC_A>(g_lane, ldg, a_lane, lda, live, src, d0, cnt, me, c, s, P, S, acc);  // (at most twice)
    }
}

__global__ __launch_bounds__(64 * NM_WAVES) void neighbor_max_backward_kernel(const wdg_neighbor_max_backward_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_neighbor_max_backward_job> job = (desc_ptr<wdg_neighbor_max_backward_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_src = job->n_src, n_feat = job->n_feat, nnz = job->nnz;
    const int row = blockIdx.x * NM_WAVES + wave, panel0 = blockIdx.y * NM_PANEL;
    if (row >= min(job->n_rows, max_rows) || panel0 >= n_feat) return;  // (wave-uniform, like everything up to the lane's columns)
    // a job outside the contract is left untouched (wdg_neighbor_max_backward_check_jobs refuses it on the host)
    if (n_src < 0 || nnz < 0 || job->reserved != 0 || job->reserved2 != 0 || job->ldg < n_feat || job->lda < n_feat || job->ldd < n_feat ||
        !job->rowptr || !job->D)
        return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    int len = thinned_row_len(job->kept_len, row, beg, end);
    if (n_src == 0 || !job->col || !job->G || !job->arg) len = 0;  // (nothing to gather from: every entry is skipped)

    // the forward pass's lane groups: P lanes hold the panel's columns, share t of the S = 64 / P requests every S-th entry's pieces
    const int used = (min(NM_PANEL, n_feat - panel0) + 3) >> 2;  // 1 .. 64
    const int lg = used <= 1 ? 0 : 32 - __builtin_clz(static_cast<unsigned>(used - 1));
    const int P = 1 << lg, S = 64 >> lg;
    const int c = lane & (P - 1), s = lane >> lg;
    const int c0 = panel0 + 4 * c, live = max(0, min(4, n_feat - c0));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const global_ptr<const uint32_t> g_lane = (global_ptr<const uint32_t>)to_global(job->G) + c0, a_lane = (global_ptr<const uint32_t>)to_global(job->arg) + c0;
    const global_ptr<const int32_t> col = to_global(job->col) + beg;
    const bool vg = (n_feat & 3) == 0 && aligned16(job->G, job->ldg), va = (n_feat & 3) == 0 && aligned16(job->arg, job->lda);
    const uint32_t me = static_cast<uint32_t>(row);
    if (vg && va) nb_row<true, true>(g_lane, job->ldg, a_lane, job->lda, live, col, len, n_src, lane, me, c, s, P, S, acc);
    else if (vg) nb_row<true, false>(g_lane, job->ldg, a_lane, job->lda, live, col, len, n_src, lane, me, c, s, P, S, acc);
    else if (va) nb_row<false, true>(g_lane, job->ldg, a_lane, job->lda, live, col, len, n_src, lane, me, c, s, P, S, acc);
    else nb_row<false, false>(g_lane, job->ldg, a_lane, job->lda, live, col, len, n_src, lane, me, c, s, P, S, acc);
    if (s != 0 || live == 0) return;
    const uint32_t out[4] = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])};
    const global_ptr<uint32_t> d = (global_ptr<uint32_t>)to_global(job->D) + static_cast<int64_t>(row) * job->ldd + c0;
    if ((n_feat & 3) == 0 && aligned16(job->D, job->ldd)) store4<true>(d, live, out);
    else store4<false>(d, live, out);
}

// the refusals of the counts both launch entries take -> the grid, or nothing to launch
int nm_check_counts(const char *what, const void *jobs, int32_t n_jobs, int32_t max_rows, int32_t max_feat) {
    WDG_REQUIRE(max_rows >= 0 && max_feat >= 0, "%s: negative count", what);
    if (const int rc = wdg::check_job_table(what, jobs, n_jobs)) return rc;
    WDG_REQUIRE(wdg::ceil_div(max_feat, NM_PANEL) <= NM_MAX_PANELS, "%s: %d columns; one launch takes %d", what, max_feat, NM_PANEL * NM_MAX_PANELS);
    return WDG_OK;
}
dim3 nm_grid(int32_t n_jobs, int32_t max_rows, int32_t max_feat) {
    return dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, NM_WAVES)), static_cast<unsigned>(wdg::ceil_div(max_feat, NM_PANEL)), static_cast<unsigned>(n_jobs));
}

}  // namespace

extern "C" int wdg_neighbor_max_batched_f32(const wdg_neighbor_max_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                            wdg_stream_t stream) {
    if (const int rc = nm_check_counts("neighbor_max_batched", jobs_dev, n_jobs, max_rows, max_feat)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_feat == 0) return WDG_OK;
    hipLaunchKernelGGL(neighbor_max_kernel, nm_grid(n_jobs, max_rows, max_feat), dim3(64 * NM_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("neighbor_max_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host (neighbor_max.NeighborMaxBatch calls this on the
// table it is about to upload).
extern "C" int wdg_neighbor_max_check_jobs(const wdg_neighbor_max_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("neighbor_max_check_jobs", jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_neighbor_max_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_cols >= 0 && j.n_feat >= 0 && j.nnz >= 0, "neighbor_max_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE((j.flags & ~NM_KNOWN_FLAGS) == 0, "neighbor_max_check_jobs: job %d has unknown flag bits 0x%x", i, j.flags & ~NM_KNOWN_FLAGS);
        WDG_REQUIRE(j.reserved == 0, "neighbor_max_check_jobs: job %d has a reserved word of %d", i, j.reserved);
        if (j.n_rows == 0 || j.n_feat == 0) continue;
        WDG_REQUIRE(j.ldx >= j.n_feat && j.ldy >= j.n_feat && (!j.arg || j.lda >= j.n_feat),
                    "neighbor_max_check_jobs: job %d has a leading dimension below its %d columns", i, j.n_feat);
        WDG_REQUIRE(j.rowptr && j.Y, "neighbor_max_check_jobs: job %d has a null rowptr or Y", i);
        WDG_REQUIRE(j.nnz == 0 || j.n_cols == 0 || (j.col && j.X), "neighbor_max_check_jobs: job %d has a null col or X", i);
        WDG_REQUIRE(static_cast<const void *>(j.X) != static_cast<const void *>(j.Y), "neighbor_max_check_jobs: job %d reads and writes one matrix", i);
    }
    return WDG_OK;
}

extern "C" int wdg_neighbor_max_backward_batched_f32(const wdg_neighbor_max_backward_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                                     wdg_stream_t stream) {
    if (const int rc = nm_check_counts("neighbor_max_backward_batched", jobs_dev, n_jobs, max_rows, max_feat)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_feat == 0) return WDG_OK;
    hipLaunchKernelGGL(neighbor_max_backward_kernel, nm_grid(n_jobs, max_rows, max_feat), dim3(64 * NM_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("neighbor_max_backward_kernel");
}

extern "C" int wdg_neighbor_max_backward_check_jobs(const wdg_neighbor_max_backward_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("neighbor_max_backward_check_jobs", jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_neighbor_max_backward_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_src >= 0 && j.n_feat >= 0 && j.nnz >= 0, "neighbor_max_backward_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.reserved == 0 && j.reserved2 == 0, "neighbor_max_backward_check_jobs: job %d has a reserved word that is not 0", i);
        if (j.n_rows == 0 || j.n_feat == 0) continue;
        WDG_REQUIRE(j.ldg >= j.n_feat && j.lda >= j.n_feat && j.ldd >= j.n_feat,
                    "neighbor_max_backward_check_jobs: job %d has a leading dimension below its %d columns", i, j.n_feat);
        WDG_REQUIRE(j.rowptr && j.D, "neighbor_max_backward_check_jobs: job %d has a null rowptr or D", i);
        WDG_REQUIRE(j.nnz == 0 || j.n_src == 0 || (j.col && j.G && j.arg), "neighbor_max_backward_check_jobs: job %d has a null col, G or arg", i);
        WDG_REQUIRE(static_cast<const void *>(j.G) != static_cast<const void *>(j.D), "neighbor_max_backward_check_jobs: job %d reads and writes one matrix", i);
    }
    return WDG_OK;
}
