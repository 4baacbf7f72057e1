// ReLU + inverted dropout of many hidden-layer matrices in one launch, IN PLACE, with the transposed copy the backward GEMM reads:
// the mask comes from Philox4x32-10 (csrc/philox.h) at a position that names the element - (job stream, step, row, column group) -
// so nothing is stored, two runs draw the same bits, and a per-graph run of the same (seed, stream, step) draws the batched run's.
//
// replaces: the hidden layer's ReLU + dropout in the training loops behind the GCN and MLP-2 accuracy tables (gnns_on_syn.py:213-249,
//           beside the one-layer tables gnns_on_syn.py:109-154; the loop itself lives upstream of the reference, which has no model
//           code).  In sweep.TrainBatch it stands in for the `hid.clamp_(min=0)` + `hid_t.copy_(hid^T)` pair of an epoch.
//
// One pass over H.  A workgroup owns a 64 x 64 tile: thread (row slot t >> 4, column group t & 15) reads four adjacent columns of
// four rows (16 lanes = one 256-byte piece of a row; one 16-byte access per lane where the job's pointer and leading dimension allow),
// draws ONE Philox block per four columns, writes the result back where it read it and, when the job has a transposed output, into
// a [64][65] LDS tile; after one barrier a wave reads a COLUMN of the tile (lane = row: 65 is odd, the 32 lanes of a half hit 32
// banks) and stores 64 consecutive floats of a row of H^T.  No atomics, no sum: an element depends on its own input and position.
#include "philox.h"
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int DR_TILE = 64, DR_THREADS = 256;
constexpr int DR_MAX_JOBS = 65535;  // gridDim.z: a job per z
constexpr int DR_MAX_COL_TILES = 65535;  // gridDim.y

// the contract of include/wdg.h for one element: kept and positive -> h * scale (one multiply); a NaN stays that NaN; else +0
__device__ __forceinline__ float dr_value(const float h, const unsigned word, const unsigned drop_threshold, const float scale) {
    if (h != h) return h;
    return (word >= drop_threshold && h > 0.f) ? h * scale : 0.f;
}

__global__ __launch_bounds__(DR_THREADS) void relu_dropout_kernel(const wdg_dropout_job *__restrict__ jobs, const unsigned drop_threshold,
                                                                  const float scale, const unsigned seed, const unsigned *__restrict__ step_dev) {
    __shared__ float tile[DR_TILE][DR_TILE + 1];
    const desc_ptr<wdg_dropout_job> job = (desc_ptr<wdg_dropout_job>)(jobs + blockIdx.z);
    const int rows = job->rows, cols = job->cols;
    const int r0 = blockIdx.x * DR_TILE, c0 = blockIdx.y * DR_TILE;
    if (r0 >= rows || c0 >= cols) return;  // (uniform: before the barrier)
    const global_ptr<float> h = to_global(job->h), ht = to_global(job->ht);
    const int64_t ld = job->ld, ld_t = job->ld_t;
    const unsigned stream = job->stream, step = *step_dev;
    const unsigned groups_per_row = (static_cast<unsigned>(cols) + 3u) >> 2;
    const bool vec = ((reinterpret_cast<uintptr_t>(job->h) | static_cast<uintptr_t>(ld * 4)) & 15) == 0;  // (uniform) 16-byte rows
    const bool transposed = job->ht != nullptr;
    const int t = threadIdx.x, gq = t & 15, rr = t >> 4;
    const int c = c0 + 4 * gq;
#pragma unroll
    for (int m = 0; m < DR_TILE / 16; ++m) {
        const int rl = rr + 16 * m, r = r0 + rl;
        if (r >= rows || c >= cols) continue;
        const philox_words w = philox4x32_10_words(static_cast<unsigned>(r) * groups_per_row + (static_cast<unsigned>(c) >> 2), step, seed, stream);
        const global_ptr<float> p = h + static_cast<int64_t>(r) * ld + c;
        float v[4];
        if (vec && c + 3 < cols) {
            const float4 in = load_f32x4(p);
            v[0] = dr_value(in.x, w.w[0], drop_threshold, scale);
            v[1] = dr_value(in.y, w.w[1], drop_threshold, scale);
            v[2] = dr_value(in.z, w.w[2], drop_threshold, scale);
            v[3] = dr_value(in.w, w.w[3], drop_threshold, scale);
            store_f32x4(p, make_float4(v[0], v[1], v[2], v[3]));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = 0.f;
                if (c + k < cols) {
                    v[k] = dr_value(p[k], w.w[k], drop_threshold, scale);
                    p[k] = v[k];
                }
            }
        }
        if (transposed) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[rl][4 * gq + k] = v[k];
        }
    }
    if (!transposed) return;  // (uniform)
    __syncthreads();
    const int rl = t & 63, r = r0 + rl;
    if (r >= rows) return;
#pragma unroll
    for (int m = 0; m < DR_TILE / 4; ++m) {
        const int cl = (t >> 6) + 4 * m;
        if (c0 + cl < cols) ht[static_cast<int64_t>(c0 + cl) * ld_t + r] = tile[rl][cl];
    }
}

}  // namespace

extern "C" int wdg_relu_dropout_batched_f32(const wdg_dropout_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                            uint32_t drop_threshold, float scale, uint32_t seed, const uint32_t *step_dev, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "relu_dropout_batched: negative count");
    WDG_REQUIRE(step_dev != nullptr, "relu_dropout_batched: null step word");
    WDG_REQUIRE(scale == scale, "relu_dropout_batched: the scale is not a number");
    WDG_REQUIRE(n_jobs <= DR_MAX_JOBS, "relu_dropout_batched: %d jobs; one launch takes %d", n_jobs, DR_MAX_JOBS);
    WDG_REQUIRE(static_cast<int64_t>(max_rows) * wdg::ceil_div(max_cols, 4) < (int64_t{1} << 32),
                "relu_dropout_batched: %d rows of %d columns hold 2^32 or more groups of four columns", max_rows, max_cols);
    WDG_REQUIRE(wdg::ceil_div(max_cols, DR_TILE) <= DR_MAX_COL_TILES, "relu_dropout_batched: %d columns; one launch takes %d", max_cols,
                DR_TILE * DR_MAX_COL_TILES);
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "relu_dropout_batched: null job table");
    if (max_rows == 0 || max_cols == 0) return WDG_OK;
    hipLaunchKernelGGL(relu_dropout_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, DR_TILE)), static_cast<unsigned>(wdg::ceil_div(max_cols, DR_TILE)),
                                                 static_cast<unsigned>(n_jobs)),
                       dim3(DR_THREADS), 0, wdg::as_stream(stream), jobs_dev, drop_threshold, scale, seed, step_dev);
    return wdg::check_launch("relu_dropout_kernel");
}
