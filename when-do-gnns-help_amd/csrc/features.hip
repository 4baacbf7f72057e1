// Compact feature matrices -> dense fp32 rows, a whole list of matrices per launch (wdg_features_expand_batched_f32).
//
// why:      the feature matrices of the reference's datasets are 90 - 99 % zeros (cora 1.3 % dense, citeseer 0.9 %, both 0/1), and the
//           sweep uploads each of them as a dense fp32 array.  A matrix travels as CSR (int32 rowptr / col, fp32 val or none) or as
//           the graph container's bit-packed words and is expanded here, optionally with the row-L1 scaling fused.
// replaces: th.FloatTensor(features) / .todense() utils/util_funcs.py:339, preprocess_features utils/util_funcs.py:39-46,
//           f.normalize homophily_tests.py:94.
//
// The work is the STORES (2000 x 3703 x 4 B = 30 MB per citeseer-width matrix; a row's few dozen entries are noise), so a row
// is written exactly once, zeros and values in the same 16-byte stores:
//   - one WAVE per row, four rows per workgroup (a narrow matrix - F = 40 - keeps its 64 lanes busy on a row of its own instead
//     of a 256-thread group on 40 floats);
//   - CSR: the wave zeroes a row IMAGE in LDS, scatters the row's scaled entries into it, and streams the image out.  The image
//     is kept in POSITIONS p = column + a, a = (element address of the row's first output) mod 4: position p is 16-byte aligned
//     in LDS exactly when column p - a is 16-byte aligned in memory, so whole dwordx4 stores need no shifting between lanes;
//     what lies before the first / after the last aligned chunk (ldo and F need not be multiples of 4) goes out as scalars;
//   - a row wider than the image (kFeatImage floats) is written in windows of positions; the columns of a row are sorted, so a
//     window's entries are a contiguous run and a cursor walks the row once;
//   - bits: every lane forms four consecutive columns from the row's words in registers (no image), same positions, same stores.
// No atomics; the image is private to its wave (LDS of one wave is in order: a wavefront fence + barrier orders it for the compiler).
//
// EVERY scatter is guarded: an entry is stored only when `(unsigned)col < (unsigned)n_feat` and its position lies inside the
// window; an entry that fails is skipped (and left out of the row sum), never stored through.  The host wrapper
// (sparse_features.py) hands over sorted, unique, in-range columns; unsorted input may lose entries, it cannot write out of bounds.
//
// Row scaling: the sum is accumulated in fp64 over the row's ENTRIES, a lane at a time and then across the wave - another order
// than row_l1_kernel's (graph_build.hip) walk over the dense row.  The result is bit-identical to wdg_row_l1_normalise_f32 on the
// expanded matrix whenever the fp64 sum is exact in any order (0/1 features, fixed-point values: what the tests use) and to fp64
// rounding of the sum otherwise.  Zeros come out +0: the dense kernel gives r * 0 = -0 in a row whose sum is negative (the two
// compare equal), and NaN where the sum is not finite.
#include <climits>

#include "feat_scale.h"
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int kFeatImage = 2048;     // floats of one row image (8 KB; a multiple of 4): wider rows take several windows
constexpr int kFeatRows = 4;         // rows (= waves) per workgroup: 32 KB of LDS, five workgroups per CU
constexpr int kFeatMaxWidth = 1 << 30;

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// four consecutive positions q .. q + 3 of a row -> memory: one 16-byte store where all four are columns, scalars at the row's ends
__device__ __forceinline__ void store_positions(global_ptr<float> dst, int q, int a, int P, const float4 &v) {
    if (q >= a && q + 4 <= P) {
        store_f32x4(dst + (q - a), v);
    } else {
        if (q + 0 >= a && q + 0 < P) dst[q + 0 - a] = v.x;
        if (q + 1 >= a && q + 1 < P) dst[q + 1 - a] = v.y;
        if (q + 2 >= a && q + 2 < P) dst[q + 2 - a] = v.z;
        if (q + 3 >= a && q + 3 < P) dst[q + 3 - a] = v.w;
    }
}

// (RowScale and the row sum's order: csrc/feat_scale.h, shared with sparse_dense.hip)

__global__ __launch_bounds__(64 * kFeatRows) void features_expand_kernel(const wdg_feat_job *__restrict__ jobs) {
    __shared__ __attribute__((aligned(16))) float images[kFeatRows][kFeatImage];
    const desc_ptr<wdg_feat_job> job = (desc_ptr<wdg_feat_job>)(jobs + blockIdx.y);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * kFeatRows + wave;
    const int F = job->n_feat;
    if (row >= job->n_rows || F <= 0 || F > kFeatMaxWidth) return;  // (wave-uniform; no workgroup barrier below)
    const int mode = job->normalise;
    const int64_t first = static_cast<int64_t>(row) * job->ldo;
    const global_ptr<float> dst = to_global(job->out) + first;
    const int a = static_cast<int>(((reinterpret_cast<uintptr_t>(job->out) >> 2) + static_cast<uint64_t>(first)) & 3);
    const int P = F + a;  // positions a .. P - 1 are the columns 0 .. F - 1

    if (job->kind == WDG_FEAT_BITS) {
        const global_ptr<const uint32_t> words = to_global(job->words) + static_cast<int64_t>(row) * job->ldw;
        const int n_words = (F + 31) >> 5;
        int cnt = 0;
        if (mode != WDG_FEAT_NORM_NONE) {
            for (int w = lane; w < n_words; w += 64) {
                uint32_t v = words[w];
                if (w == n_words - 1 && (F & 31)) v &= (1u << (F & 31)) - 1u;  // bits past F are padding
                cnt += __popc(v);
            }
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        }
        const RowScale scale(mode, static_cast<double>(cnt));
        const float one = scale(1.f);
        auto bit = [&](int c) { return c >= 0 && c < F && ((words[c >> 5] >> (c & 31)) & 1u) ? one : 0.f; };
        for (int q = 4 * lane; q < P; q += 256) {
            const int c = q - a;
            float4 v;
            if (c >= 0 && c + 4 <= F) {  // four columns from at most two words
                const int w0 = c >> 5, w1 = (c + 3) >> 5;
                uint64_t two = words[w0];
                if (w1 != w0) two |= static_cast<uint64_t>(words[w1]) << 32;
                const unsigned b = static_cast<unsigned>(two >> (c & 31));
                v = make_float4(b & 1u ? one : 0.f, b & 2u ? one : 0.f, b & 4u ? one : 0.f, b & 8u ? one : 0.f);
            } else {
                v = make_float4(bit(c), bit(c + 1), bit(c + 2), bit(c + 3));
            }
            store_positions(dst, q, a, P, v);
        }
        return;
    }

    // CSR
    const global_ptr<const int32_t> rowptr = to_global(job->rowptr), col = to_global(job->col);
    const global_ptr<const float> val = to_global(job->val);
    const int beg = rowptr[row], end = rowptr[row + 1];
    const double sum = feat_csr_row_sum(col, val, beg, end, F, mode, lane);
    const RowScale scale(mode, sum);
    float *img = images[wave];
    int cursor = beg;  // the first entry no window has taken yet (wave-uniform)
    for (int p0 = 0; p0 < P; p0 += kFeatImage) {
        const int p1 = min(P, p0 + kFeatImage), span4 = (p1 - p0 + 3) & ~3;  // (<= kFeatImage: a multiple of 4)
        const int c_lo = max(0, p0 - a), c_hi = p1 - a;                       // the window's columns
        for (int i = 4 * lane; i < span4; i += 256) *reinterpret_cast<float4 *>(img + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        wave_lds_sync();
        while (true) {
            const int e = cursor + lane;
            const bool live = e < end;
            const int c = live ? col[e] : INT_MAX;
            if (live && static_cast<unsigned>(c) < static_cast<unsigned>(F)
                && static_cast<unsigned>(c) - static_cast<unsigned>(c_lo) < static_cast<unsigned>(c_hi - c_lo))
                img[c + a - p0] = scale(val ? val[e] : 1.f);  // (index in [0, p1 - p0): inside the image)
            const int taken = __popcll(__ballot(live && c < c_hi));  // sorted columns: a prefix of the 64
            cursor += taken;
            if (taken < 64) break;
        }
        wave_lds_sync();
        for (int i = 4 * lane; i < span4; i += 256) store_positions(dst, p0 + i, a, P, *reinterpret_cast<const float4 *>(img + i));
        // (the next window's zeroes go to the addresses this lane has just read: no hazard between lanes before its scatter's sync)
    }
}

}  // namespace

extern "C" int32_t wdg_features_image_floats(void) { return kFeatImage; }

extern "C" int wdg_features_expand_batched_f32(const wdg_feat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                               wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_feat >= 0, "features_expand_batched: negative size");
    if (n_jobs == 0 || max_rows == 0 || max_feat == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "features_expand_batched: null job table");
    WDG_REQUIRE(max_feat <= kFeatMaxWidth, "features_expand_batched: more than 2^30 features");
    hipStream_t st = wdg::as_stream(stream);
    const unsigned blocks = static_cast<unsigned>(wdg::ceil_div(max_rows, kFeatRows));
    for (int32_t first = 0; first < n_jobs; first += 65535) {  // (the job index rides on grid.y: 65535 at most per launch)
        const unsigned n = static_cast<unsigned>(n_jobs - first < 65535 ? n_jobs - first : 65535);
        hipLaunchKernelGGL(features_expand_kernel, dim3(blocks, n), dim3(64 * kFeatRows), 0, st, jobs_dev + first);
    }
    return wdg::check_launch("features_expand_kernel");
}
