// The deflation pre-pass that the two kernel-regression solvers share (csrc/kernel_reg.hip: kr_deflate_kernel, 320 threads, one
// workgroup per problem; csrc/kernel_reg_large.hip: kr_large_deflate_kernel, 1024 threads, persistent over the table) and the
// layout of the workspace it leaves for them - both stated here once.
#pragma once
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int KR_MAX_C = 8;  // the right-hand sides a solver's workgroup carries: a problem's classes, or one class window of them
typedef int i32x2_t __attribute__((ext_vector_type(2)));  // a wdg_kr_row_best as one 8-byte store: (value bits, class)
static_assert(sizeof(wdg_kr_row_best) == 8, "a row's (value, class) pair is stored as one 8-byte vector");
constexpr int KR_ALL_C = 16;  // classes of a problem solved in class windows (wdg_kr_job.class_base): what the pre-pass judges labels over

// The deflation workspace of a problem (wdg_kr_job.ws: filled by the pre-pass, read by the solver), as int32 words.  Four header
// words, then four per-row arrays of P words each, then the validation rows (krw_bytes in all).  P is the register solver's 320
// or, for the large solver, the problem's OWN train rows rounded up to 32 (krw_pad); W = krw_offsets(P):
//   [KRW_NT]         rows to solve;
//   [KRW_DEFLATED]   != 0 when fewer than n_train;
//   [KRW_MIXED]      entries of the mixed list;
//   [KRW_DROPPED]    != 0 when rows were dropped below the block's resolution (flags bit 2);
//   [KRW_TRAIN ..]   the solved rows' representatives, padded with -1 up to P;
//   [W.lab ..]       a solved row's label when all members of its duplicate class carry the same one (right-hand side: sqrt(size) in
//                    that column), -1 when none carries a label in range (0 .. KR_ALL_C - 1: ALL classes, whatever the window of
//                    the job - a problem's workspace is the same for each of its window jobs; a zero row), -2 for a class with MIXED labels, whose
//                    non-zero right-hand-side entries are listed in [W.mix ..];
//   [W.scale ..]     sqrt(members) of a solved row's duplicate class (fp32 bits): the solver factors M = S K S, S = diag of these;
//   [W.mix ..]       the mixed list: row << 16 | label << 12 | members with that label (a pair per train row at most: <= P words);
//   [W.val ..]       n_val validation representatives, then n_val labels.
constexpr int KRW_NT = 0, KRW_DEFLATED = 1, KRW_MIXED = 2, KRW_DROPPED = 3, KRW_TRAIN = 4;
__host__ __device__ constexpr int krw_pad(int n_train) { return (n_train + 31) & ~31; }
struct krw_offsets {  // where the arrays after [KRW_TRAIN ..] begin (sums in this order: the solvers' generated code depends on it)
    int lab, scale, mix, val;
    __host__ __device__ constexpr explicit krw_offsets(int P) : lab(KRW_TRAIN + P), scale(lab + P), mix(scale + P), val(mix + P) {}
};
// what a problem's workspace takes, rounded up to 256 bytes (the *_workspace_bytes entry points)
constexpr size_t krw_bytes(int P, int n_val) {
    return (static_cast<size_t>(krw_offsets(P).val + 2 * (n_val > 0 ? n_val : 0)) * 4 + 255) & ~static_cast<size_t>(255);
}

// Deflation pre-pass of ONE problem by a workgroup of THREADS threads, one thread per train row (n_train <= THREADS; P: the stride
// of the problem's workspace arrays, above).  With the row representatives of the matrix K was computed from (wdg_kr_job.rep,
// csrc/row_rep.hip) every id is taken at its representative - duplicate rows of K are then identical by construction -, the train
// rows are DEFLATED to one row per duplicate class with the class's mean one-hot label as right-hand side, and rows whose K_ii is
// exactly 0 (all-zero feature rows under the linear kernel) are dropped.  That is the answer of the reference's
// `np.linalg.pinv(K_train_train) @ label_onehot[idx_train]` (utils/homophily_metrics.py:291-297) on an exactly singular block: the
// minimum-norm solution shares a class's weight among its members, K[v, members] sums it up again.  With B the members-to-class
// incidence matrix and D = B^T B (the class sizes), K_tt = B K_u B^T = Q (D^1/2 K_u D^1/2) Q^T with Q = B D^-1/2 orthonormal, so
// pinv(K_tt) = Q pinv(M) Q^T, M = S K_u S, S = D^1/2: the solver factors the SCALED block M with right-hand sides S^-1 B^T Y (a
// class's label counts over sqrt(size)) and multiplies the solution by S - for a regular K_u the same as K_u^-1 (mean label), and
// for a K_u that is rank deficient beyond its duplicates (texas: aggregated rows that are sums of others) the regularised answer
// keeps the full system's metric (the unscaled form was up to 26 validation rows from the reference there).  The solver reads the
// result from the problem's workspace and factors a positive definite block where round 5 added a rounding-level ridge.
// A job without a workspace is left alone (solved as it is); a job whose n_train the workgroup does not hold is refused by the
// solver's own test, and its workspace says so (rows to solve = -1).  The shared arrays are the routine's own: a caller that
// runs it on problem after problem puts a barrier between them.
template <int THREADS>
__device__ __forceinline__ void kr_deflate_one(const wdg_kr_job *__restrict__ job_ptr, int P) {
    static_assert(THREADS % 64 == 0, "whole waves");
    __shared__ int d_raw[THREADS], d_first[THREADS], d_slot[THREADS], d_mult[THREADS];
    // a slot's label counts over all KR_ALL_C classes, two 16-bit counts per word (a count is at most THREADS <= 4095, the mixed
    // list's own cap: no carry into the neighbour) - fp32 counts of 16 classes would be 64 KB at 1024 threads
    __shared__ unsigned cnt2[THREADS * (KR_ALL_C / 2)];
    __shared__ float wmax[THREADS / 64];
    __shared__ int n_keep, any_mixed, any_drop;
    const desc_ptr<wdg_kr_job> job = (desc_ptr<wdg_kr_job>)job_ptr;
    if (job->ws == nullptr) return;  // (uniform)
    const krw_offsets W(P);
    const int tid = threadIdx.x, nt_in = job->n_train, nv = job->n_val;
    const global_ptr<int32_t> ws = to_global(static_cast<int32_t *>(job->ws));
    if (nt_in <= 0 || nt_in > THREADS) {  // (the solver refuses the problem by its own test; the workspace must still be sane)
        if (tid == 0) ws[KRW_NT] = -1, ws[KRW_DEFLATED] = 0, ws[KRW_MIXED] = 0, ws[KRW_DROPPED] = 0;
        return;
    }
    const global_ptr<const float> K = to_global(job->K);
    const global_ptr<const int32_t> train = to_global(job->train), val = to_global(job->val), labels = to_global(job->labels),
                                    rep = to_global(job->rep);
    const bool has_rep = job->rep != nullptr;  // (without the maps every node is its own representative: zero rows are still dropped)
    const int64_t ldk = job->ldk;
    if (tid == 0) n_keep = 0, any_mixed = 0, any_drop = 0;
    int r = -1, lb = -1;
    float diag = 0.f;
    if (tid < nt_in) {
        const int g = train[tid];
        r = has_rep ? rep[g] : g, lb = labels[g];
        diag = K[static_cast<int64_t>(r) * ldk + r];
    }
    // rows BELOW THE BLOCK'S fp32 RESOLUTION are dropped (weight 0): K_ii <= n eps max K_ii / 64 - the level of the solver's pivot
    // test, so that a row the solver would factor as it is is never dropped (a hub-heavy kernel's diagonal spans 1e-5 of its maximum
    // and more).  The two agree exactly when nothing is merged; after merges the solver tests the merged count against the diagonal
    // of S K S (class sizes >= 1: its maximum is no smaller), so a row kept here may still meet the solver's ridge.  What the rule
    // drops: an all-zero row of K (an isolated node's aggregated features, an all-zero feature row under the linear kernel: an exact
    // zero singular value, which the pseudo-inverse cuts), and the arc-cosine kernel's row of such a node (every entry 1.6e-9: a
    // singular value 1e-12 of the largest, which an fp32 SVD cannot resolve - the reference's pinv leaves it no weight either:
    // measured on texas, where factoring that row exactly, as an fp64 pseudo-inverse would, moved an epoch 24 validation rows away
    // from the reference's)
    float dmax = diag == diag ? diag : 0.f;
    for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = dmax;
    __syncthreads();
    dmax = 0.f;
    for (int w = 0; w < THREADS / 64; ++w) dmax = fmaxf(dmax, wmax[w]);
    if (tid < nt_in && !(diag > static_cast<float>(nt_in) * 1.1920929e-7f * dmax * (1.f / 64.f))) r = -2, any_drop = 1;
    __syncthreads();
    d_raw[tid] = r, d_mult[tid] = 0;
    for (int i = tid; i < THREADS * (KR_ALL_C / 2); i += THREADS) cnt2[i] = 0u;
    __syncthreads();
    int first = r < 0 ? -1 : tid;  // the first train row with this representative
    if (r >= 0)  // (eight ids per step, tested together: a one-at-a-time loop with an early exit waits for every LDS read)
        for (int j0 = 0; j0 < tid && first == tid; j0 += 8) {
            int v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = d_raw[min(j0 + e, THREADS - 1)];
#pragma unroll
            for (int e = 7; e >= 0; --e)
                if (v[e] == r && j0 + e < tid) first = j0 + e;  // (descending: the smallest match stays)
        }
    // a kept row's slot = the kept rows before it (train ids ascend: so do the slots' rows): ballot prefix inside a wave + the
    // earlier waves' counts
    const bool keep = first == tid;
    const unsigned long long kmask = __ballot(keep);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) d_mult[wv] = __popcll(kmask);  // (d_mult doubles as the per-wave counts until the barrier; zeroed again below)
    __syncthreads();
    int slot = -1;
    if (keep) {
        slot = __popcll(kmask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) slot += d_mult[w];
        d_slot[tid] = slot;
    }
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < THREADS / 64; ++w) total += d_mult[w];
        n_keep = total;
    }
    __syncthreads();
    if (tid < THREADS / 64) d_mult[tid] = 0;
    __syncthreads();
    // (no barrier between the two lines below: the first reads d_slot, which only kept rows wrote, two barriers ago; the second
    // writes d_first, which nobody has touched yet - `first` lives in a register - and which is read after the next barrier)
    if (first >= 0 && first != tid) slot = d_slot[first];
    if (first == tid) d_first[slot] = r;  // the kept representatives, compact
    if (slot >= 0) {                      // (counts of small integers: exact in any order)
        atomicAdd(&d_mult[slot], 1);
        if (lb >= 0 && lb < KR_ALL_C) atomicAdd(&cnt2[slot * (KR_ALL_C / 2) + (lb >> 1)], 1u << (16 * (lb & 1)));
    }
    __syncthreads();
    const int kept = n_keep;
    if (tid < P) ws[KRW_TRAIN + tid] = tid < kept ? d_first[tid] : -1;
    // slot `tid`: pure (every member one label -> that label; members without a label in range -> -1: a zero row) or mixed
    int pure = -1;
    bool mixed = false;
    if (tid < kept) {
        const int m = d_mult[tid];
        int nz = 0;
        for (int c = 0; c < KR_ALL_C; ++c) {
            const int cnt = static_cast<int>((cnt2[tid * (KR_ALL_C / 2) + (c >> 1)] >> (16 * (c & 1))) & 0xffffu);
            if (cnt != 0) ++nz, pure = c;
            if (cnt != 0 && cnt != m) mixed = true;
        }
        mixed |= nz > 1;
        if (mixed) {  // (a (row, label) pair per train row at most: the list never outgrows its P words)
            pure = -2;
            for (int c = 0; c < KR_ALL_C; ++c) {
                const int cnt = static_cast<int>((cnt2[tid * (KR_ALL_C / 2) + (c >> 1)] >> (16 * (c & 1))) & 0xffffu);
                if (cnt > 0) ws[W.mix + atomicAdd(&any_mixed, 1)] = (tid << 16) | (c << 12) | cnt;
            }
        }
    }
    if (tid < P) {
        ws[W.lab + tid] = pure;
        ws[W.scale + tid] = __builtin_bit_cast(int, tid < kept ? sqrtf(static_cast<float>(d_mult[tid])) : 1.f);
    }
    for (int v = tid; v < nv; v += THREADS) {
        const int g = val[v];
        ws[W.val + v] = has_rep ? rep[g] : g;
        ws[W.val + nv + v] = labels[g];
    }
    __syncthreads();
    if (tid == 0) ws[KRW_NT] = kept, ws[KRW_DEFLATED] = kept != nt_in, ws[KRW_MIXED] = any_mixed, ws[KRW_DROPPED] = any_drop;
}

}  // namespace
