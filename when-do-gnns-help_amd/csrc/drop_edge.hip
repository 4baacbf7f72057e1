// DropEdge (Rong, Huang, Xu, Huang: "DropEdge: Towards Deep Graph Convolutional Networks on Node Classification", ICLR 2020) on the
// device: the thinning pass that draws a fresh subset of a pattern's stored entries per training step and writes it AS A PATTERN
// (wdg_drop_edge_thin_batched), and the aggregation over such a thinned pattern (wdg_spmm_thinned_batched_f32), whose backward pass is
// the same kernel on the transposed job's thinned pattern with the two scales swapped.
//
// why:      every aggregation of the project reads the same stored entries on every epoch; the one regulariser was dropout on hidden
//           units (csrc/dropout.hip).  Composed by hand - torch.rand over the entries, with_values(mask), degree_norm(use_values), spmm
//           with explicit values, and the mask gathered through transpose_positions for the backward pass - DropEdge stores a mask,
//           gives up the value-free plans and cannot redraw inside a captured epoch.
// replaces: nothing of the reference, which ships no model code: the thinning restates the degree part of its normalisation on the
//           KEPT entries - normalize, utils/util_funcs.py:29-36, and normalize_tensor, utils/util_funcs.py:365-380 - for the models
//           that stand beside the tables of gnns_on_syn.py:9-53.
//
// THE CONTRACT (include/wdg.h states it in full; tests/_drop_edge_ref.py restates it in numpy): whether an entry is kept is a function
// of its FORWARD coordinates and of (seed, stream, step) through Philox4x32-10 (csrc/philox.h), not of where it is stored: the
// transposed job keeps the transposed set without any position map, a column stored twice shares one fate, and with TIED both
// directions of an undirected edge do.  The aggregation is ONE fmaf chain per output element over the kept entries in stored order:
// no row is split, nothing is added across lanes or waves.  The unit is compiled with contraction off and writes the fmaf out.
//
// Thinning: a WAVE owns a row, four rows per workgroup, a job per grid y.  The row goes in chunks of 64 entries, one per lane: the
// lane draws its entry's word, a ballot and the lane's prefix count (mbcnt) give the compacted position, the kept columns are
// stored in stored order, then the wave fills the rest of the row's extent with -1 and lane 0 writes the length and the scale.
// Integer arithmetic plus one division (and a square root) per row.  No LDS, no atomics, no scratch.  There is NO multi-wave path
// for a hub row: squirrel's longest row (1904 entries) is 30 chunks on one wave.  The row's extent, the chunk's compaction and the
// row's tail are csrc/wave_rows.h's, which csrc/neighbor_sample.hip writes the same layout with; the aggregation reads it through
// thinned_row_len there, as csrc/neighbor_max.hip does.
// Aggregation: a WAVE owns a row and a PANEL of 256 columns (grid y); lane l holds the four columns 256 panel + 4 l .. + 3, so an
// entry costs the wave one row piece of X (a 16-byte load per lane where the job's pointer, leading dimension and width allow -
// the wave's decision, csrc/wave_rows.h - element-wise loads elsewhere: same values, same fmaf).  The kept columns and their
// column scales are read 64 at a time, one per lane, and handed out with v_readlane; TS_DEPTH row loads are in flight before the
// first fmaf of a batch, a shorter tail goes in batches of 4, 2, 1 (gt_chains' schedule, restated here: those chains read an
// entry's weight per head from an LDS stage, these carry ONE scale per entry in a register, and gat_lanes.h is left as it is).
#include <cmath>
#include <cstdint>

#include "philox.h"
#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // the chain's fmaf is written out; nothing else may be fused

namespace {

using namespace wdg;

constexpr int DE_WAVES = 4;          // rows per workgroup, both kernels
constexpr int TS_PANEL = 256;        // columns of Y per wave: four per lane
constexpr int TS_MAX_PANELS = 65535; // gridDim.y
constexpr int TS_DEPTH = 8;          // row loads in flight before the first fmaf of a batch
constexpr unsigned DE_KEY_TAG = 0x45444745u;  // "EDGE": the second key word of the step key
constexpr int DE_KNOWN_FLAGS = WDG_DROP_EDGE_TIED | WDG_DROP_EDGE_TRANSPOSED | WDG_DROP_EDGE_KEEP_DIAGONAL | WDG_DROP_EDGE_NORM_SYM;

__global__ __launch_bounds__(64 * DE_WAVES) void drop_edge_thin_kernel(const wdg_drop_edge_job *__restrict__ jobs, const int max_rows,
                                                                       const unsigned drop_threshold, const unsigned seed,
                                                                       const unsigned *__restrict__ step_dev) {
    const desc_ptr<wdg_drop_edge_job> job = (desc_ptr<wdg_drop_edge_job>)(jobs + blockIdx.y);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n = job->n, n_cols = job->n_cols, nnz = job->nnz, flags = job->flags;
    const int row = blockIdx.x * DE_WAVES + wave;
    if (row >= min(n, max_rows)) return;  // (wave-uniform, like everything up to the chunk loop)
    // a job outside the contract is left untouched (wdg_drop_edge_check_jobs refuses it on the host)
    if (n_cols < 0 || nnz < 0 || (flags & ~DE_KNOWN_FLAGS) || job->reserved != 0 || !job->rowptr || !job->kept_len ||
        (nnz > 0 && (!job->col || !job->kept_col || job->kept_col == job->col)))
        return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    const global_ptr<const int32_t> col = to_global(job->col);
    const global_ptr<int32_t> kept_col = to_global(job->kept_col);

    const philox_words key = philox4x32_10_words(*step_dev, job->stream, seed, DE_KEY_TAG);  // the step key: uniform
    const unsigned k0 = key.w[0], k1 = key.w[1];
    const bool tied = flags & WDG_DROP_EDGE_TIED, transposed = flags & WDG_DROP_EDGE_TRANSPOSED, diagonal = flags & WDG_DROP_EDGE_KEEP_DIAGONAL;

    int kept = 0;  // (wave-uniform) kept entries of the chunks so far
    for (int e0 = beg; e0 < end; e0 += 64) {
        const int cnt = min(64, end - e0);
        const int j = lane < cnt ? col[e0 + lane] : -1;
        const bool valid = static_cast<unsigned>(j) < static_cast<unsigned>(n_cols);
        const unsigned fi = transposed ? static_cast<unsigned>(j) : static_cast<unsigned>(row);  // the FORWARD coordinates
        const unsigned fj = transposed ? static_cast<unsigned>(row) : static_cast<unsigned>(j);
        const unsigned a = tied ? min(fi, fj) : fi, b = tied ? max(fi, fj) : fj;
        const unsigned word = philox4x32_10(a, b, k0, k1);
        const bool keep = valid && ((diagonal && j == row) || word >= drop_threshold);
        thinned_row_keep(kept_col, beg, kept, keep, j);
    }
    thinned_row_finish(job, kept_col, row, beg, end, kept, lane, flags & WDG_DROP_EDGE_NORM_SYM);
}

// D consecutive entries d0 .. d0 + D - 1 of the chunk the wave holds: all D row loads, then the D x 4 fmafs in entry order.  src: lane
// d holds the source row of entry d, or -1 for an entry that is skipped (its load goes to row 0 and its fmaf is not applied); cs: its
// column scale.  EVERY lane is active at the readlanes; a lane without columns only skips the loads and the fmafs.
template <int D, bool VEC>
__device__ __forceinline__ void ts_batch(const global_ptr<const float> x_lane, const int64_t ld, const int live, const int src, const float cs,
                                         const int d0, float (&acc)[4]) {
    int r[D];
    float s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        r[d] = __builtin_amdgcn_readlane(src, d0 + d);
        s[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cs), d0 + d));
    }
    if (live > 0) {
        float x[D][4];
#pragma unroll
        for (int d = 0; d < D; ++d) load4<VEC>(x_lane + static_cast<int64_t>(max(r[d], 0)) * ld, live, x[d]);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool ok = r[d] >= 0;  // (uniform)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = ok ? fmaf(s[d], x[d][k], acc[k]) : acc[k];
        }
    }
}

// the chains of the lane's four columns over the row's first `len` kept entries, in stored order
template <bool VEC>
__device__ __forceinline__ void ts_row(const global_ptr<const float> x_lane, const int64_t ld, const int live, const global_ptr<const int32_t> kept_col,
                                       const global_ptr<const float> col_scale, const int beg, const int len, const int n_cols, const int lane,
                                       float (&acc)[4]) {
    for (int e0 = 0; e0 < len; e0 += 64) {
        const int cnt = min(64, len - e0);  // (wave-uniform)
        int src = lane < cnt ? kept_col[beg + e0 + lane] : -1;
        if (static_cast<unsigned>(src) >= static_cast<unsigned>(n_cols)) src = -1;
        const float cs = (col_scale && src >= 0) ? col_scale[src] : 1.0f;
        int d0 = 0;
        for (; d0 + TS_DEPTH <= cnt; d0 += TS_DEPTH) ts_batch<TS_DEPTH, VEC>(x_lane, ld, live, src, cs, d0, acc);
        if (d0 + 4 <= cnt) ts_batch<4, VEC>(x_lane, ld, live, src, cs, d0, acc), d0 += 4;
        if (d0 + 2 <= cnt) ts_batch<2, VEC>(x_lane, ld, live, src, cs, d0, acc), d0 += 2;
        if (d0 + 1 <= cnt) ts_batch<1, VEC>(x_lane, ld, live, src, cs, d0, acc);
    }
}

__global__ __launch_bounds__(64 * DE_WAVES) void spmm_thinned_kernel(const wdg_thinned_spmm_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_thinned_spmm_job> job = (desc_ptr<wdg_thinned_spmm_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_cols = job->n_cols, n_feat = job->n_feat, nnz = job->nnz;
    const int row = blockIdx.x * DE_WAVES + wave, panel0 = blockIdx.y * TS_PANEL;
    if (row >= min(job->n_rows, max_rows) || panel0 >= n_feat) return;  // (wave-uniform, like everything up to the lane's columns)
    // a job outside the contract is left untouched (wdg_spmm_thinned_check_jobs refuses it on the host)
    if (n_cols < 0 || nnz < 0 || job->reserved != 0 || job->ldx < n_feat || job->ldy < n_feat || !job->rowptr || !job->kept_len || !job->Y) return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    int len = thinned_row_len(job->kept_len, row, beg, end);
    if (n_cols == 0 || !job->kept_col || !job->X) len = 0;  // (nothing to gather from: every entry is skipped)

    const int c0 = panel0 + 4 * lane, live = max(0, min(4, n_feat - c0));
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const global_ptr<const float> x_lane = to_global(job->X) + c0;
    if ((n_feat & 3) == 0 && aligned16(job->X, job->ldx))
        ts_row<true>(x_lane, job->ldx, live, to_global(job->kept_col), to_global(job->col_scale), beg, len, n_cols, lane, acc);
    else
        ts_row<false>(x_lane, job->ldx, live, to_global(job->kept_col), to_global(job->col_scale), beg, len, n_cols, lane, acc);
    if (live == 0) return;
    if (job->row_scale) {
        const float rs = to_global(job->row_scale)[row];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = rs * acc[k];  // ONE multiply
    }
    const global_ptr<float> y = to_global(job->Y) + static_cast<int64_t>(row) * job->ldy + c0;
    if ((n_feat & 3) == 0 && aligned16(job->Y, job->ldy)) {
        store_f32x4(y, make_float4(acc[0], acc[1], acc[2], acc[3]));
    } else {  // (store4 of wave_rows.h, written out: through the call the compiler lays this kernel's blocks out differently)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < live) y[k] = acc[k];
    }
}

}  // namespace

extern "C" int wdg_drop_edge_thin_batched(const wdg_drop_edge_job *jobs_dev, int32_t n_jobs, int32_t max_rows, uint32_t drop_threshold,
                                          uint32_t seed, const uint32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(max_rows >= 0, "drop_edge_thin_batched: negative count");
    if (const int rc = wdg::check_job_table("drop_edge_thin_batched", jobs_dev, n_jobs)) return rc;
    WDG_REQUIRE(step_dev != nullptr, "drop_edge_thin_batched: null step word");
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    hipLaunchKernelGGL(drop_edge_thin_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, DE_WAVES)), static_cast<unsigned>(n_jobs)),
                       dim3(64 * DE_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows, drop_threshold, seed, step_dev);
    return wdg::check_launch("drop_edge_thin_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host (drop_edge.DropEdgeBatch calls this on the table it
// is about to upload).
extern "C" int wdg_drop_edge_check_jobs(const wdg_drop_edge_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("drop_edge_check_jobs", jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_drop_edge_job &j = jobs_host[i];
        WDG_REQUIRE(j.n >= 0 && j.n_cols >= 0 && j.nnz >= 0, "drop_edge_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE((j.flags & ~DE_KNOWN_FLAGS) == 0, "drop_edge_check_jobs: job %d has unknown flag bits 0x%x", i, j.flags & ~DE_KNOWN_FLAGS);
        WDG_REQUIRE(j.reserved == 0, "drop_edge_check_jobs: job %d has a reserved word of %d", i, j.reserved);
        if (j.n == 0) continue;
        WDG_REQUIRE(j.rowptr && j.kept_len, "drop_edge_check_jobs: job %d has a null rowptr or kept_len", i);
        if (j.nnz == 0) continue;
        WDG_REQUIRE(j.col && j.kept_col, "drop_edge_check_jobs: job %d has a null col or kept_col", i);
        const uintptr_t a = reinterpret_cast<uintptr_t>(j.col), b = reinterpret_cast<uintptr_t>(j.kept_col), bytes = static_cast<uintptr_t>(j.nnz) * 4;
        WDG_REQUIRE(a + bytes <= b || b + bytes <= a, "drop_edge_check_jobs: job %d's kept_col overlaps its col (the pass does not run in place)", i);
    }
    return WDG_OK;
}

extern "C" int wdg_spmm_thinned_batched_f32(const wdg_thinned_spmm_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                            wdg_stream_t stream) {
    WDG_REQUIRE(max_rows >= 0 && max_feat >= 0, "spmm_thinned_batched: negative count");
    if (const int rc = wdg::check_job_table("spmm_thinned_batched", jobs_dev, n_jobs)) return rc;
    WDG_REQUIRE(wdg::ceil_div(max_feat, TS_PANEL) <= TS_MAX_PANELS, "spmm_thinned_batched: %d columns; one launch takes %d", max_feat,
                TS_PANEL * TS_MAX_PANELS);
    if (n_jobs == 0 || max_rows == 0 || max_feat == 0) return WDG_OK;
    hipLaunchKernelGGL(spmm_thinned_kernel,
                       dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, DE_WAVES)), static_cast<unsigned>(wdg::ceil_div(max_feat, TS_PANEL)),
                            static_cast<unsigned>(n_jobs)),
                       dim3(64 * DE_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("spmm_thinned_kernel");
}

extern "C" int wdg_spmm_thinned_check_jobs(const wdg_thinned_spmm_job *jobs_host, int32_t n_jobs) {
    if (const int rc = wdg::check_job_table("spmm_thinned_check_jobs", jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_thinned_spmm_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_cols >= 0 && j.n_feat >= 0 && j.nnz >= 0, "spmm_thinned_check_jobs: job %d has a negative shape", i);
        WDG_REQUIRE(j.reserved == 0, "spmm_thinned_check_jobs: job %d has a reserved word of %d", i, j.reserved);
        if (j.n_rows == 0 || j.n_feat == 0) continue;
        WDG_REQUIRE(j.ldx >= j.n_feat && j.ldy >= j.n_feat, "spmm_thinned_check_jobs: job %d has a leading dimension below its %d columns", i, j.n_feat);
        WDG_REQUIRE(j.rowptr && j.kept_len && j.Y, "spmm_thinned_check_jobs: job %d has a null rowptr, kept_len or Y", i);
        WDG_REQUIRE(j.nnz == 0 || j.n_cols == 0 || (j.kept_col && j.X), "spmm_thinned_check_jobs: job %d has a null kept_col or X", i);
        WDG_REQUIRE(static_cast<const void *>(j.X) != static_cast<const void *>(j.Y), "spmm_thinned_check_jobs: job %d reads and writes one matrix", i);
    }
    return WDG_OK;
}
