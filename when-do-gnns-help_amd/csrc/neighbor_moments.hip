// The neighbour MOMENTS and their backward pass (wdg_neighbor_moments_batched_f32, wdg_neighbor_moments_backward_batched_f32): the four
// aggregators of PNA (Corso, Cavalleri, Beaini, Lio, Velickovic: "Principal Neighbourhood Aggregation for Graph Nets", NeurIPS 2020) -
// per column the mean, the standard deviation, the maximum and the minimum over a row's stored neighbours - in ONE walk over a plain CSR
// pattern or over a thinned pattern as csrc/drop_edge.hip and csrc/neighbor_sample.hip leave it, with the count of the neighbours.
//
// why:      composed from the library's own kernels the four statistics are four walks over the same row, and the standard deviation
//           comes out as E[x^2] - E[x]^2, which in fp32 loses everything once a column's mean is large against its spread.  Here a
//           row's entries and source rows are read once for all four, and the deviation is the CENTRED one: a second pass over the same
//           values with the mean taken off.
// replaces: nothing of the reference, which ships no model code: it stands where the product with the normalised adjacency - normalize,
//           utils/util_funcs.py:29-36, and normalize_tensor, utils/util_funcs.py:365-380 - stands in the other models, beside the
//           tables of gnns_on_syn.py:9-53.
//
// THE CONTRACT (include/wdg.h states it in full; tests/_neighbor_moments_ref.py restates it in numpy): a sum of a row is FOUR CHAINS BY
// POSITION - chain k takes the entries at positions e with e % 4 == k, in stored order - merged as (c0 + c1) + (c2 + c3); the extremes are
// neighbor_max.hip's, under the order of csrc/neighbor_order.h.
//
// Forward: a WAVE owns a row and a PANEL of 256 columns (grid y), four columns per lane.  A panel of w columns needs ceil(w / 4) lanes;
// rounded up to a power of two that is P.  Of the 64 / P lane groups the first S4 = min(64 / P, 4) work: share t takes the positions e
// with (e % 4) % S4 == t and so owns 4 / S4 whole chains - no chain is split, a column's bits do not depend on S4.  (At class width P = 4
// and four shares walk the row; the other twelve lane groups idle: the position chains allow four shares, not sixteen.)  A lane requests
// up to MO_LOADS rows of X before the first add.  A row of at most MO_LOADS S4 entries - one step - stays in registers for the
// second pass; a longer row is read again (from the cache, mostly).  The shares are merged with xor-shuffles: the chain sums by the
// definition's tree, the count as an integer, the extremes under the order.
// Backward: launch 1 writes A and B per forward (row, column); launch 2 is a wave per row of the TRANSPOSED pattern and per panel with the
// same lane groups: the entries are read 64 at a time, one per lane, the duplicate rule of the routed terms is settled with a ballot
// (neighbor_max.hip's), and a share requests the six row pieces - A, B, g_max, arg_max, g_min, arg_min - of its positions.
// No LDS, no atomics, no scratch.
#include <cmath>
#include <cstdint>

#include "neighbor_order.h"
#include "wave_rows.h"
#include "wdg_common.h"

#pragma clang fp contract(off)  // every sum is restated bit for bit: the fmaf is written out, nothing else may be fused

namespace {

using namespace wdg;

constexpr int MO_WAVES = 4;           // rows per workgroup, all kernels
constexpr int MO_PANEL = 256;         // columns per wave: four per lane
constexpr int MO_MAX_PANELS = 65535;  // gridDim.y
constexpr int MO_LOADS = 8;           // forward: rows of X a lane requests before the first add
constexpr int MB_LOADS = 4;           // backward: entries (six row pieces each) a lane requests before the first add

// what a lane knows of its share of the row (len: 0 in a lane group that does not work)
struct mo_lane {
    global_ptr<const int32_t> col;
    int len, n_cols, s, live;
};

// NG groups of four positions from e0 (a multiple of 4): the lane's G = 4 / S4 entries of every group - their column indices, -1 where
// the entry is skipped or past the row's end (never read through) - and their pieces of X, all requested before anything is used
template <bool VEC, int G, int NG>
__device__ __forceinline__ void mo_load(const mo_lane &L, const global_ptr<const uint32_t> x_lane, const int64_t ld, const int e0, int (&j)[NG * G],
                                        uint32_t (&x)[NG * G][4]) {
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int e = e0 + 4 * u + L.s + (4 / G) * g;
            int jj = e < L.len ? L.col[e] : -1;
            if (static_cast<unsigned>(jj) >= static_cast<unsigned>(L.n_cols)) jj = -1;
            j[u * G + g] = jj;
        }
    if (L.live > 0) {
#pragma unroll
        for (int n = 0; n < NG * G; ++n) load4<VEC>(x_lane + static_cast<int64_t>(max(j[n], 0)) * ld, L.live, x[n]);
    } else {
#pragma unroll
        for (int n = 0; n < NG * G; ++n)
#pragma unroll
            for (int k = 0; k < 4; ++k) x[n][k] = 0u;
    }
}

// the first pass over loaded entries: the count, chain g of s1 (entry u G + g sits at a position of the lane's g-th chain), the extremes
template <int G, int NG>
__device__ __forceinline__ void mo_first(const int (&j)[NG * G], const uint32_t (&x)[NG * G][4], const bool ext, float (&s1)[G][4], int &cnt,
                                         uint64_t (&hi)[4], uint32_t (&hib)[4], uint64_t (&lo)[4], uint32_t (&lob)[4]) {
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int n = u * G + g;
            const bool ok = j[n] >= 0;
            cnt += ok ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s1[g][k] = ok ? s1[g][k] + __uint_as_float(x[n][k]) : s1[g][k];
        }
    if (ext) {
#pragma unroll
        for (int n = 0; n < NG * G; ++n) {
            const uint32_t tie = ~static_cast<uint32_t>(j[n]);  // the lower j is the greater word
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t wh = static_cast<uint64_t>(nm_key(x[n][k], false)) << 32 | tie, wl = static_cast<uint64_t>(nm_key(x[n][k], true)) << 32 | tie;
                const bool up = j[n] >= 0 && wh > hi[k], down = j[n] >= 0 && wl > lo[k];
                hi[k] = up ? wh : hi[k];
                hib[k] = up ? x[n][k] : hib[k];
                lo[k] = down ? wl : lo[k];
                lob[k] = down ? x[n][k] : lob[k];
            }
        }
    }
}

// the second pass: chain g of s2 over the same entries, centred
template <int G, int NG>
__device__ __forceinline__ void mo_second(const int (&j)[NG * G], const uint32_t (&x)[NG * G][4], const float (&mean)[4], float (&s2)[G][4]) {
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int n = u * G + g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = __uint_as_float(x[n][k]) - mean[k];
                s2[g][k] = j[n] >= 0 ? fmaf(d, d, s2[g][k]) : s2[g][k];
            }
        }
}

// the chains of the S4 = 4 / G working shares -> the definition's (c0 + c1) + (c2 + c3) in every working lane.  Share t holds the
// chains t, t + S4, ..: one xor step adds chain pairs (0, 1) and (2, 3), the next the two pair sums; what a lane holds more than one of
// is added inside it, in the same tree.  EVERY lane is active here.
template <int G>
__device__ __forceinline__ void mo_merge(float (&s)[G][4], const int P, float (&out)[4]) {
    for (int off = P; off < P * (4 / G); off <<= 1)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k) s[g][k] = s[g][k] + __shfl_xor(s[g][k], off);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (G == 1) out[k] = s[0][k];
        else if constexpr (G == 2) out[k] = s[0][k] + s[1][k];
        else out[k] = (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]);
    }
}

// the end of the first pass: the merged sums and count -> c (wave-uniform) and the mean, +0 for a row without eligible entries
template <int G>
__device__ __forceinline__ void mo_means(float (&s1)[G][4], int cnt, const int P, float (&mean)[4], int &c) {
    float sum[4];
    mo_merge<G>(s1, P, sum);
    for (int off = P; off < P * (4 / G); off <<= 1) cnt += __shfl_xor(cnt, off);
    c = __builtin_amdgcn_readfirstlane(cnt);  // (lane 0 is a working lane)
#pragma unroll
    for (int k = 0; k < 4; ++k) mean[k] = c > 0 ? sum[k] / static_cast<float>(c) : 0.f;
}
template <int G>
__device__ __forceinline__ void mo_deviation(float (&s2)[G][4], const int P, const int c, const float eps, float (&sd)[4]) {
    float sum[4];
    mo_merge<G>(s2, P, sum);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float var = sum[k] / static_cast<float>(c);
        sd[k] = sqrtf(var + eps);
    }
}

// a row of at most NG groups: ONE step, whose values stay in registers for the second pass
template <bool VEC, int G, int NG>
__device__ __forceinline__ void mo_short(const mo_lane &L, const global_ptr<const uint32_t> x_lane, const int64_t ld, const int P, const bool ext,
                                         const bool want_std, const float eps, float (&mean)[4], float (&sd)[4], int &c, uint64_t (&hi)[4],
                                         uint32_t (&hib)[4], uint64_t (&lo)[4], uint32_t (&lob)[4]) {
    int j[NG * G];
    uint32_t x[NG * G][4];
    float s1[G][4] = {};
    int cnt = 0;
    mo_load<VEC, G, NG>(L, x_lane, ld, 0, j, x);
    mo_first<G, NG>(j, x, ext, s1, cnt, hi, hib, lo, lob);
    mo_means<G>(s1, cnt, P, mean, c);
    if (want_std && c > 0) {
        float s2[G][4] = {};
        mo_second<G, NG>(j, x, mean, s2);
        mo_deviation<G>(s2, P, c, eps, sd);
    }
}

template <bool VEC, int G, int NG>
__device__ __forceinline__ void mo_step_first(const mo_lane &L, const global_ptr<const uint32_t> x_lane, const int64_t ld, const int e0, const bool ext,
                                              float (&s1)[G][4], int &cnt, uint64_t (&hi)[4], uint32_t (&hib)[4], uint64_t (&lo)[4], uint32_t (&lob)[4]) {
    int j[NG * G];
    uint32_t x[NG * G][4];
    mo_load<VEC, G, NG>(L, x_lane, ld, e0, j, x);
    mo_first<G, NG>(j, x, ext, s1, cnt, hi, hib, lo, lob);
}
template <bool VEC, int G, int NG>
__device__ __forceinline__ void mo_step_second(const mo_lane &L, const global_ptr<const uint32_t> x_lane, const int64_t ld, const int e0,
                                               const float (&mean)[4], float (&s2)[G][4]) {
    int j[NG * G];
    uint32_t x[NG * G][4];
    mo_load<VEC, G, NG>(L, x_lane, ld, e0, j, x);
    mo_second<G, NG>(j, x, mean, s2);
}

// The row (len > 0, wave-uniform): its groups of four positions in steps of MO_LOADS, MO_LOADS / 2, .. rows of X per lane - a long row
// keeps MO_LOADS loads per lane in flight, a short one requests little it does not need.  Wave-uniform trip counts: every lane is active
// at the merges.
template <bool VEC, int G>
__device__ __forceinline__ void mo_row(const mo_lane &L, const global_ptr<const uint32_t> x_lane, const int64_t ld, const int len, const int P,
                                       const bool ext, const bool want_std, const float eps, float (&mean)[4], float (&sd)[4], int &c,
                                       uint64_t (&hi)[4], uint32_t (&hib)[4], uint64_t (&lo)[4], uint32_t (&lob)[4]) {
    constexpr int NGMAX = MO_LOADS / G;  // 8, 4, 2
    const int groups = (len + 3) >> 2;
    if (groups <= NGMAX) {
        if (groups <= 1) return mo_short<VEC, G, 1>(L, x_lane, ld, P, ext, want_std, eps, mean, sd, c, hi, hib, lo, lob);
        if (groups <= 2) return mo_short<VEC, G, 2>(L, x_lane, ld, P, ext, want_std, eps, mean, sd, c, hi, hib, lo, lob);
        if constexpr (NGMAX >= 4)
            if (groups <= 4) return mo_short<VEC, G, 4>(L, x_lane, ld, P, ext, want_std, eps, mean, sd, c, hi, hib, lo, lob);
        return mo_short<VEC, G, NGMAX>(L, x_lane, ld, P, ext, want_std, eps, mean, sd, c, hi, hib, lo, lob);
    }
    float s1[G][4] = {};
    int cnt = 0, q = 0;
    for (; q + NGMAX <= groups; q += NGMAX) mo_step_first<VEC, G, NGMAX>(L, x_lane, ld, 4 * q, ext, s1, cnt, hi, hib, lo, lob);
    if constexpr (NGMAX >= 8)
        if (q + 4 <= groups) mo_step_first<VEC, G, 4>(L, x_lane, ld, 4 * q, ext, s1, cnt, hi, hib, lo, lob), q += 4;
    if constexpr (NGMAX >= 4)
        if (q + 2 <= groups) mo_step_first<VEC, G, 2>(L, x_lane, ld, 4 * q, ext, s1, cnt, hi, hib, lo, lob), q += 2;
    if (q + 1 <= groups) mo_step_first<VEC, G, 1>(L, x_lane, ld, 4 * q, ext, s1, cnt, hi, hib, lo, lob);
    mo_means<G>(s1, cnt, P, mean, c);
    if (!want_std || c == 0) return;
    float s2[G][4] = {};
    for (q = 0; q + NGMAX <= groups; q += NGMAX) mo_step_second<VEC, G, NGMAX>(L, x_lane, ld, 4 * q, mean, s2);
    if constexpr (NGMAX >= 8)
        if (q + 4 <= groups) mo_step_second<VEC, G, 4>(L, x_lane, ld, 4 * q, mean, s2), q += 4;
    if constexpr (NGMAX >= 4)
        if (q + 2 <= groups) mo_step_second<VEC, G, 2>(L, x_lane, ld, 4 * q, mean, s2), q += 2;
    if (q + 1 <= groups) mo_step_second<VEC, G, 1>(L, x_lane, ld, 4 * q, mean, s2);
    mo_deviation<G>(s2, P, c, eps, sd);
}

// the wave's lane groups: P lanes hold the panel's columns; of the 64 / P groups the first S4 = min(64 / P, 4) = 4 / G work
__device__ __forceinline__ void mo_groups(const int n_feat, const int panel0, const int lane, int &lg, int &G, int &c, int &s) {
    const int used = (min(MO_PANEL, n_feat - panel0) + 3) >> 2;  // 1 .. 64
    lg = used <= 1 ? 0 : 32 - __builtin_clz(static_cast<unsigned>(used - 1));
    G = 4 >> min(6 - lg, 2);
    c = lane & ((1 << lg) - 1), s = lane >> lg;
}

template <typename T>
__device__ __forceinline__ void mo_store(T *out, const int64_t ld, const int row, const int c0, const int n_feat, const int live, const uint32_t (&v)[4]) {
    if (!out) return;
    const global_ptr<uint32_t> p = (global_ptr<uint32_t>)to_global(out) + static_cast<int64_t>(row) * ld + c0;
    if ((n_feat & 3) == 0 && aligned16(out, ld)) store4<true>(p, live, v);
    else store4<false>(p, live, v);
}

__device__ __forceinline__ bool mo_bad_ld(const void *p, const int64_t ld, const int n_feat) { return p && ld < n_feat; }

__global__ __launch_bounds__(64 * MO_WAVES) void neighbor_moments_kernel(const wdg_neighbor_moments_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_neighbor_moments_job> job = (desc_ptr<wdg_neighbor_moments_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_cols = job->n_cols, n_feat = job->n_feat, nnz = job->nnz;
    const int row = blockIdx.x * MO_WAVES + wave, panel0 = blockIdx.y * MO_PANEL;
    if (row >= min(job->n_rows, max_rows) || panel0 >= n_feat) return;  // (wave-uniform, like everything up to the lane's columns)
    const float eps = job->eps;
    // a job outside the contract is left untouched (wdg_neighbor_moments_check_jobs refuses it on the host)
    if (n_cols < 0 || nnz < 0 || job->flags != 0 || job->reserved != 0 || job->reserved2 != 0 || job->ldx < n_feat || !job->rowptr || !job->cnt ||
        !(eps >= 0.f) || isinf(eps) || mo_bad_ld(job->mean, job->ld_mean, n_feat) || mo_bad_ld(job->std, job->ld_std, n_feat) ||
        mo_bad_ld(job->mx, job->ld_mx, n_feat) || mo_bad_ld(job->mn, job->ld_mn, n_feat) || mo_bad_ld(job->arg_max, job->ld_amax, n_feat) ||
        mo_bad_ld(job->arg_min, job->ld_amin, n_feat))
        return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    int len = thinned_row_len(job->kept_len, row, beg, end);
    if (n_cols == 0 || !job->col || !job->X) len = 0;  // (nothing to look at: every entry is skipped)
    len = max(len, 0);

    int lg, G, c, s;
    mo_groups(n_feat, panel0, lane, lg, G, c, s);
    const int P = 1 << lg, S4 = 4 / G;
    const int c0 = panel0 + 4 * c;
    const bool works = s < S4;
    const int live = works ? max(0, min(4, n_feat - c0)) : 0;
    const bool ext = job->mx || job->mn || job->arg_max || job->arg_min, want_std = job->std != nullptr;

    float mean[4] = {0.f, 0.f, 0.f, 0.f}, sd[4] = {0.f, 0.f, 0.f, 0.f};
    uint64_t hi[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};  // 0: no eligible entry yet
    uint32_t hib[4] = {0, 0, 0, 0}, lob[4] = {0, 0, 0, 0};
    int count = 0;
    if (len > 0) {
        const mo_lane L = {to_global(job->col) + beg, works ? len : 0, n_cols, s, live};
        const global_ptr<const uint32_t> x_lane = (global_ptr<const uint32_t>)to_global(job->X) + c0;
        const int64_t ld = job->ldx;
        const bool vec = (n_feat & 3) == 0 && aligned16(job->X, job->ldx);
        if (vec) {
            if (G == 1) mo_row<true, 1>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
            else if (G == 2) mo_row<true, 2>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
            else mo_row<true, 4>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
        } else {
            if (G == 1) mo_row<false, 1>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
            else if (G == 2) mo_row<false, 2>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
            else mo_row<false, 4>(L, x_lane, ld, len, P, ext, want_std, eps, mean, sd, count, hi, hib, lo, lob);
        }
        if (ext) {  // the working shares of one column group sit P lanes apart: merged under the order (EVERY lane is active here)
            for (int off = P; off < P * S4; off <<= 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t wh = nm_shfl_xor64(hi[k], off), wl = nm_shfl_xor64(lo[k], off);
                    const uint32_t bh = static_cast<uint32_t>(__shfl_xor(static_cast<int>(hib[k]), off));
                    const uint32_t bl = static_cast<uint32_t>(__shfl_xor(static_cast<int>(lob[k]), off));
                    const bool up = wh > hi[k], down = wl > lo[k];
                    hi[k] = up ? wh : hi[k];
                    hib[k] = up ? bh : hib[k];
                    lo[k] = down ? wl : lo[k];
                    lob[k] = down ? bl : lob[k];
                }
            }
        }
    }
    if (lane == 0 && panel0 == 0) to_global(job->cnt)[row] = count;
    if (s != 0 || live == 0) return;
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = __float_as_uint(mean[k]);
    mo_store(job->mean, job->ld_mean, row, c0, n_feat, live, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = __float_as_uint(sd[k]);
    mo_store(job->std, job->ld_std, row, c0, n_feat, live, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = hi[k] ? hib[k] : 0u;  // the winner's bits, or +0
    mo_store(job->mx, job->ld_mx, row, c0, n_feat, live, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = hi[k] ? ~static_cast<uint32_t>(hi[k]) : 0xffffffffu;  // the winner's j, or -1
    mo_store(job->arg_max, job->ld_amax, row, c0, n_feat, live, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = lo[k] ? lob[k] : 0u;
    mo_store(job->mn, job->ld_mn, row, c0, n_feat, live, out);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = lo[k] ? ~static_cast<uint32_t>(lo[k]) : 0xffffffffu;
    mo_store(job->arg_min, job->ld_amin, row, c0, n_feat, live, out);
}

// ---- backward, launch 1: A and B of every forward (row, column).  A wave per forward row and per panel; lane l takes the columns
// panel0 + l, + 64, + 128, + 192.
__global__ __launch_bounds__(64 * MO_WAVES) void neighbor_moments_prepare_kernel(const wdg_neighbor_moments_backward_job *__restrict__ jobs, const int max_src) {
    const desc_ptr<wdg_neighbor_moments_backward_job> job = (desc_ptr<wdg_neighbor_moments_backward_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_feat = job->n_feat;
    const int i = blockIdx.x * MO_WAVES + wave, panel0 = blockIdx.y * MO_PANEL;
    if (i >= min(job->n_src, max_src) || panel0 >= n_feat) return;
    if (job->flags != 0 || job->reserved != 0 || job->ldw < n_feat || !job->A || !job->B || !job->cnt || mo_bad_ld(job->g_mean, job->ld_gmean, n_feat) ||
        mo_bad_ld(job->g_std, job->ld_gstd, n_feat) || mo_bad_ld(job->mean, job->ld_mean, n_feat) || mo_bad_ld(job->std, job->ld_std, n_feat))
        return;
    const int c = __builtin_amdgcn_readfirstlane(to_global(job->cnt)[i]);
    const float fc = static_cast<float>(c);
    const global_ptr<const float> gm = to_global(job->g_mean), gs = to_global(job->g_std), mean = to_global(job->mean), sd = to_global(job->std);
    const bool spread = job->g_std && job->std;  // (a NULL g_std reads as +0: B = +0)
    for (int f = panel0 + lane; f < min(n_feat, panel0 + MO_PANEL); f += 64) {
        float a = 0.f, b = 0.f;
        if (c > 0) {
            if (spread) b = gs[static_cast<int64_t>(i) * job->ld_gstd + f] / (fc * sd[static_cast<int64_t>(i) * job->ld_std + f]);
            const float q = (job->g_mean ? gm[static_cast<int64_t>(i) * job->ld_gmean + f] : 0.f) / fc;
            a = fmaf(-b, job->mean ? mean[static_cast<int64_t>(i) * job->ld_mean + f] : 0.f, q);
        }
        to_global(job->A)[static_cast<int64_t>(i) * job->ldw + f] = a;
        to_global(job->B)[static_cast<int64_t>(i) * job->ldw + f] = b;
    }
}

// ---- backward, launch 2.  NG groups of four positions of the chunk the wave holds, from position d0 (a multiple of 4): the lane's
// entries of them - src: lane d holds the forward row of entry d, or -1; route: the same with the duplicate rule applied - and their six
// row pieces, all requested before the first add.  EVERY lane is active at the cross-lane reads.
template <int G, int NG, bool VEC>
__device__ __forceinline__ void mb_step(const desc_ptr<wdg_neighbor_moments_backward_job> job, const int c0, const int live, const bool works, const int s,
                                        const int src, const int route, const int d0, const int cnt, const uint32_t me, const bool has_max,
                                        const bool has_min, float (&sa)[G][4], float (&sb)[G][4], float (&rm)[G][4], float (&rn)[G][4]) {
    int r[NG * G], t[NG * G];
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int d = d0 + 4 * u + s + (4 / G) * g;
            const int got = __shfl(src, d & 63), via = __shfl(route, d & 63);
            r[u * G + g] = works && d < cnt ? got : -1;
            t[u * G + g] = works && d < cnt ? via : -1;
        }
    if (live <= 0) return;
    float a[NG * G][4], b[NG * G][4];
    uint32_t gx[NG * G][4], ax[NG * G][4], gn[NG * G][4], an[NG * G][4];
    const global_ptr<const float> pa = to_global(job->A) + c0, pb = to_global(job->B) + c0;
    const global_ptr<const uint32_t> pgx = (global_ptr<const uint32_t>)to_global(job->g_max) + c0, pax = (global_ptr<const uint32_t>)to_global(job->arg_max) + c0;
    const global_ptr<const uint32_t> pgn = (global_ptr<const uint32_t>)to_global(job->g_min) + c0, pan = (global_ptr<const uint32_t>)to_global(job->arg_min) + c0;
#pragma unroll
    for (int n = 0; n < NG * G; ++n) {
        const int64_t i = max(r[n], 0);
        load4<VEC>(pa + i * job->ldw, live, a[n]);
        load4<VEC>(pb + i * job->ldw, live, b[n]);
        if (has_max) load4<VEC>(pgx + i * job->ld_gmax, live, gx[n]), load4<VEC>(pax + i * job->ld_amax, live, ax[n]);
        if (has_min) load4<VEC>(pgn + i * job->ld_gmin, live, gn[n]), load4<VEC>(pan + i * job->ld_amin, live, an[n]);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int n = u * G + g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sa[g][k] = r[n] >= 0 ? sa[g][k] + a[n][k] : sa[g][k];
                sb[g][k] = r[n] >= 0 ? sb[g][k] + b[n][k] : sb[g][k];
                if (has_max) rm[g][k] = (t[n] >= 0 && ax[n][k] == me) ? rm[g][k] + __uint_as_float(gx[n][k]) : rm[g][k];
                if (has_min) rn[g][k] = (t[n] >= 0 && an[n][k] == me) ? rn[g][k] + __uint_as_float(gn[n][k]) : rn[g][k];
            }
        }
}

template <int G, bool VEC>
__device__ __forceinline__ void mb_row(const desc_ptr<wdg_neighbor_moments_backward_job> job, const int c0, const int live, const bool works, const int s,
                                       const int P, const int lane, const global_ptr<const int32_t> col, const int len, const int n_src, const uint32_t me,
                                       const bool has_max, const bool has_min, float (&rest)[4], float (&SB)[4]) {
    constexpr int NGMAX = MB_LOADS / G > 0 ? MB_LOADS / G : 1;  // 4, 2, 1
    float sa[G][4] = {}, sb[G][4] = {}, rm[G][4] = {}, rn[G][4] = {};
    int last = -1;  // (wave-uniform) the i of the latest entry that was not out of range
    for (int e0 = 0; e0 < len; e0 += 64) {
        const int cnt = min(64, len - e0);  // (wave-uniform)
        int src = lane < cnt ? col[e0 + lane] : -1;
        if (static_cast<unsigned>(src) >= static_cast<unsigned>(n_src)) src = -1;
        // the duplicate rule (neighbor_max.hip's): the entry before this one that was in range - in this chunk, or `last`
        const unsigned long long votes = __ballot(src >= 0);
        const unsigned long long below = votes & ((1ull << lane) - 1ull);
        const int from = below ? 63 - __builtin_clzll(below) : lane;
        const int before = __shfl(src, from);
        const int prev = below ? before : last;
        if (votes) last = __builtin_amdgcn_readlane(src, 63 - __builtin_clzll(votes));
        const int route = src == prev ? -1 : src;
        const int groups = (cnt + 3) >> 2;
        int q = 0;
        for (; q + NGMAX <= groups; q += NGMAX) mb_step<G, NGMAX, VEC>(job, c0, live, works, s, src, route, 4 * q, cnt, me, has_max, has_min, sa, sb, rm, rn);
        if constexpr (NGMAX >= 4)
            if (q + 2 <= groups) mb_step<G, 2, VEC>(job, c0, live, works, s, src, route, 4 * q, cnt, me, has_max, has_min, sa, sb, rm, rn), q += 2;
        if constexpr (NGMAX >= 2)
            if (q + 1 <= groups) mb_step<G, 1, VEC>(job, c0, live, works, s, src, route, 4 * q, cnt, me, has_max, has_min, sa, sb, rm, rn);
    }
    float SA[4], RM[4], RN[4];
    mo_merge<G>(sa, P, SA);
    mo_merge<G>(sb, P, SB);
    mo_merge<G>(rm, P, RM);
    mo_merge<G>(rn, P, RN);
#pragma unroll
    for (int k = 0; k < 4; ++k) rest[k] = (SA[k] + RM[k]) + RN[k];
}

__device__ __forceinline__ bool mb_vec(const void *p, const int64_t ld) { return !p || aligned16(p, ld); }

__global__ __launch_bounds__(64 * MO_WAVES) void neighbor_moments_backward_kernel(const wdg_neighbor_moments_backward_job *__restrict__ jobs, const int max_rows) {
    const desc_ptr<wdg_neighbor_moments_backward_job> job = (desc_ptr<wdg_neighbor_moments_backward_job>)(jobs + blockIdx.z);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int n_src = job->n_src, n_feat = job->n_feat, nnz = job->nnz;
    const int row = blockIdx.x * MO_WAVES + wave, panel0 = blockIdx.y * MO_PANEL;
    if (row >= min(job->n_rows, max_rows) || panel0 >= n_feat) return;  // (wave-uniform, like everything up to the lane's columns)
    // a job outside the contract is left untouched (wdg_neighbor_moments_backward_check_jobs refuses it on the host)
    if (n_src < 0 || nnz < 0 || job->flags != 0 || job->reserved != 0 || job->ldx < n_feat || job->ldw < n_feat || job->ldd < n_feat || !job->rowptr ||
        !job->X || !job->D || !job->A || !job->B || mo_bad_ld(job->g_max, job->ld_gmax, n_feat) || mo_bad_ld(job->g_min, job->ld_gmin, n_feat) ||
        mo_bad_ld(job->arg_max, job->ld_amax, n_feat) || mo_bad_ld(job->arg_min, job->ld_amin, n_feat))
        return;
    int beg, end;
    if (!row_extent(to_global(job->rowptr), row, nnz, beg, end)) return;
    int len = thinned_row_len(job->kept_len, row, beg, end);
    if (n_src == 0 || !job->col) len = 0;  // (nothing to gather from: every entry is skipped)

    int lg, G, c, s;
    mo_groups(n_feat, panel0, lane, lg, G, c, s);
    const int P = 1 << lg;
    const int c0 = panel0 + 4 * c;
    const bool works = s < 4 / G;
    const int live = works ? max(0, min(4, n_feat - c0)) : 0;
    const bool has_max = job->g_max && job->arg_max, has_min = job->g_min && job->arg_min;  // (a NULL g reads as +0: nothing is routed)
    const bool vec = (n_feat & 3) == 0 && aligned16(job->A, job->ldw) && aligned16(job->B, job->ldw) && mb_vec(job->g_max, job->ld_gmax) &&
                     mb_vec(job->arg_max, job->ld_amax) && mb_vec(job->g_min, job->ld_gmin) && mb_vec(job->arg_min, job->ld_amin);
    const global_ptr<const int32_t> col = to_global(job->col) + beg;
    const uint32_t me = static_cast<uint32_t>(row);
    float rest[4] = {0.f, 0.f, 0.f, 0.f}, SB[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (G == 1) mb_row<1, true>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
        else if (G == 2) mb_row<2, true>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
        else mb_row<4, true>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
    } else {
        if (G == 1) mb_row<1, false>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
        else if (G == 2) mb_row<2, false>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
        else mb_row<4, false>(job, c0, live, works, s, P, lane, col, len, n_src, me, has_max, has_min, rest, SB);
    }
    if (s != 0 || live == 0) return;
    float x[4];
    const global_ptr<const float> xp = to_global(job->X) + static_cast<int64_t>(row) * job->ldx + c0;
    if ((n_feat & 3) == 0 && aligned16(job->X, job->ldx)) load4<true>(xp, live, x);
    else load4<false>(xp, live, x);
    uint32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = __float_as_uint(fmaf(x[k], SB[k], rest[k]));
    mo_store(job->D, job->ldd, row, c0, n_feat, live, out);
}

// the refusals of the counts the launch entries take
int mo_check_counts(const char *what, const void *jobs, int32_t n_jobs, int32_t max_rows, int32_t max_feat) {
    WDG_REQUIRE(max_rows >= 0 && max_feat >= 0, "%s: negative count", what);
    if (const int rc = wdg::check_job_table(what, jobs, n_jobs)) return rc;
    WDG_REQUIRE(wdg::ceil_div(max_feat, MO_PANEL) <= MO_MAX_PANELS, "%s: %d columns; one launch takes %d", what, max_feat, MO_PANEL * MO_MAX_PANELS);
    return WDG_OK;
}
dim3 mo_grid(int32_t n_jobs, int32_t max_rows, int32_t max_feat) {
    return dim3(static_cast<unsigned>(wdg::ceil_div(max_rows, MO_WAVES)), static_cast<unsigned>(wdg::ceil_div(max_feat, MO_PANEL)), static_cast<unsigned>(n_jobs));
}
bool mo_ld_ok(const void *p, int64_t ld, int32_t n_feat) { return !p || ld >= n_feat; }

}  // namespace

extern "C" int wdg_neighbor_moments_batched_f32(const wdg_neighbor_moments_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                                wdg_stream_t stream) {
    if (const int rc = mo_check_counts("neighbor_moments_batched", jobs_dev, n_jobs, max_rows, max_feat)) return rc;
    if (n_jobs == 0 || max_rows == 0 || max_feat == 0) return WDG_OK;
    hipLaunchKernelGGL(neighbor_moments_kernel, mo_grid(n_jobs, max_rows, max_feat), dim3(64 * MO_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("neighbor_moments_kernel");
}

// The per-job part of the contract, for a table the caller still holds on the host (neighbor_moments.NeighborMomentsBatch calls this on
// the table it is about to upload).
extern "C" int wdg_neighbor_moments_check_jobs(const wdg_neighbor_moments_job *jobs_host, int32_t n_jobs) {
    const char *what = "neighbor_moments_check_jobs";
    if (const int rc = wdg::check_job_table(what, jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_neighbor_moments_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_cols >= 0 && j.n_feat >= 0 && j.nnz >= 0, "%s: job %d has a negative shape", what, i);
        WDG_REQUIRE(j.flags == 0, "%s: job %d has unknown flag bits 0x%x", what, i, j.flags);
        WDG_REQUIRE(j.reserved == 0 && j.reserved2 == 0, "%s: job %d has a reserved word that is not 0", what, i);
        WDG_REQUIRE(j.eps >= 0.f && !std::isinf(j.eps), "%s: job %d has an eps that is negative or not finite", what, i);  // (a NaN fails)
        if (j.n_rows == 0 || j.n_feat == 0) continue;
        WDG_REQUIRE(j.ldx >= j.n_feat && mo_ld_ok(j.mean, j.ld_mean, j.n_feat) && mo_ld_ok(j.std, j.ld_std, j.n_feat) && mo_ld_ok(j.mx, j.ld_mx, j.n_feat) &&
                        mo_ld_ok(j.mn, j.ld_mn, j.n_feat) && mo_ld_ok(j.arg_max, j.ld_amax, j.n_feat) && mo_ld_ok(j.arg_min, j.ld_amin, j.n_feat),
                    "%s: job %d has a leading dimension below its %d columns", what, i, j.n_feat);
        WDG_REQUIRE(j.rowptr && j.cnt, "%s: job %d has a null rowptr or cnt", what, i);
        WDG_REQUIRE(j.nnz == 0 || j.n_cols == 0 || (j.col && j.X), "%s: job %d has a null col or X", what, i);
        const void *outs[7] = {j.mean, j.std, j.mx, j.mn, j.arg_max, j.arg_min, j.cnt};
        for (int a = 0; a < 7; ++a) {
            WDG_REQUIRE(!outs[a] || outs[a] != static_cast<const void *>(j.X), "%s: job %d reads and writes one matrix", what, i);
            for (int b = a + 1; b < 7; ++b) WDG_REQUIRE(!outs[a] || outs[a] != outs[b], "%s: job %d writes two results to one address", what, i);
        }
    }
    return WDG_OK;
}

extern "C" int wdg_neighbor_moments_backward_batched_f32(const wdg_neighbor_moments_backward_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_src,
                                                         int32_t max_feat, wdg_stream_t stream) {
    WDG_REQUIRE(max_src >= 0, "%s: negative count", "neighbor_moments_backward_batched");
    if (const int rc = mo_check_counts("neighbor_moments_backward_batched", jobs_dev, n_jobs, max_rows, max_feat)) return rc;
    if (n_jobs == 0 || max_feat == 0) return WDG_OK;
    if (max_src > 0) {
        hipLaunchKernelGGL(neighbor_moments_prepare_kernel, mo_grid(n_jobs, max_src, max_feat), dim3(64 * MO_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_src);
        if (const int rc = wdg::check_launch("neighbor_moments_prepare_kernel")) return rc;
    }
    if (max_rows == 0) return WDG_OK;
    hipLaunchKernelGGL(neighbor_moments_backward_kernel, mo_grid(n_jobs, max_rows, max_feat), dim3(64 * MO_WAVES), 0, wdg::as_stream(stream), jobs_dev, max_rows);
    return wdg::check_launch("neighbor_moments_backward_kernel");
}

extern "C" int wdg_neighbor_moments_backward_check_jobs(const wdg_neighbor_moments_backward_job *jobs_host, int32_t n_jobs) {
    const char *what = "neighbor_moments_backward_check_jobs";
    if (const int rc = wdg::check_job_table(what, jobs_host, n_jobs)) return rc;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const wdg_neighbor_moments_backward_job &j = jobs_host[i];
        WDG_REQUIRE(j.n_rows >= 0 && j.n_src >= 0 && j.n_feat >= 0 && j.nnz >= 0, "%s: job %d has a negative shape", what, i);
        WDG_REQUIRE(j.flags == 0, "%s: job %d has unknown flag bits 0x%x", what, i, j.flags);
        WDG_REQUIRE(j.reserved == 0, "%s: job %d has a reserved word that is not 0", what, i);
        if (j.n_feat == 0 || (j.n_rows == 0 && j.n_src == 0)) continue;
        WDG_REQUIRE(j.ldx >= j.n_feat && j.ldw >= j.n_feat && j.ldd >= j.n_feat && mo_ld_ok(j.g_mean, j.ld_gmean, j.n_feat) &&
                        mo_ld_ok(j.g_std, j.ld_gstd, j.n_feat) && mo_ld_ok(j.g_max, j.ld_gmax, j.n_feat) && mo_ld_ok(j.g_min, j.ld_gmin, j.n_feat) &&
                        mo_ld_ok(j.mean, j.ld_mean, j.n_feat) && mo_ld_ok(j.std, j.ld_std, j.n_feat) && mo_ld_ok(j.arg_max, j.ld_amax, j.n_feat) &&
                        mo_ld_ok(j.arg_min, j.ld_amin, j.n_feat),
                    "%s: job %d has a leading dimension below its %d columns", what, i, j.n_feat);
        WDG_REQUIRE(j.rowptr && j.X && j.D && j.A && j.B && j.cnt, "%s: job %d has a null rowptr, X, D, A, B or cnt", what, i);
        WDG_REQUIRE(j.nnz == 0 || j.n_src == 0 || j.col, "%s: job %d has a null col", what, i);
        WDG_REQUIRE(!j.g_mean || j.mean, "%s: job %d has a g_mean without the forward pass's mean", what, i);
        WDG_REQUIRE(!j.g_std || (j.mean && j.std), "%s: job %d has a g_std without the forward pass's mean and std", what, i);
        WDG_REQUIRE((!j.g_max || j.arg_max) && (!j.g_min || j.arg_min), "%s: job %d has a g_max or g_min without the forward pass's arg", what, i);
        const void *outs[3] = {j.D, j.A, j.B};
        const void *ins[9] = {j.X, j.g_mean, j.g_std, j.g_max, j.g_min, j.mean, j.std, j.arg_max, j.arg_min};
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 9; ++b) WDG_REQUIRE(outs[a] != ins[b], "%s: job %d reads and writes one matrix", what, i);
            for (int b = a + 1; b < 3; ++b) WDG_REQUIRE(outs[a] != outs[b], "%s: job %d writes two results to one address", what, i);
        }
    }
    return WDG_OK;
}
