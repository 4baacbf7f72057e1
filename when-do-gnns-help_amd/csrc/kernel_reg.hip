// Kernel-regression metric on the device: a batched symmetric solver for the per-epoch regressions over the
// kernels that csrc/gram.hip computes once per graph (the kernel of an epoch's sample is a sub-block of the kernel of all nodes),
// on the node sets that csrc/kr_sets.hip draws.
//
// replaces: the kernel-regression branch of classifier_based_performance_metric (utils/homophily_metrics.py:283-297,
//           utils/homophily_plot.py:296-310: `K_val_train @ (np.linalg.pinv(K_train_train) @ onehot[idx_train])`, argmax, accuracy).
//
//   * kr_deflate_kernel the deflation pre-pass: one row per duplicate class of the train rows (csrc/kr_deflate.h: the routine
//                       and the layout of the workspace it fills, shared with csrc/kernel_reg_large.hip);
//   * kr_solve_blocked_kernel
//                       one workgroup per (graph, classifier, epoch, kernel) problem: gathers the train block K[tr, tr] from
//                       the graph's kernel into REGISTERS (up to 320 x 320), factors it (right-looking blocked Cholesky, the
//                       trailing update on the matrix pipe), solves for the one-hot labels, multiplies the validation rows
//                       through and counts correct arg-max predictions.  For a symmetric positive definite block the Cholesky
//                       solution IS pinv(K) Y; when a pivot falls to rounding level (<= n eps max K_ii / 64: a rank-deficient
//                       block, e.g. duplicate nodes) the block is refactored once with the ridge n eps max K_ii / 8: the
//                       least-squares answer of the pseudo-inverse to within one or two validation rows per epoch (measured
//                       against the reference's per-epoch accuracies) - a documented deviation in the coefficients.
#include <cstdlib>

#include "wdg_common.h"
#include "kr_blocks.h"
#include "kr_deflate.h"

namespace {

using namespace wdg;

// ------------------------------------------------------------------------------------------------ batched kernel regression
// One workgroup of 16 waves per (kernel, train rows, validation rows) regression, a right-looking BLOCKED Cholesky with 32 x 32
// blocks: the trailing update, > 90 % of the flops, runs on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: an exact fp32 fma chain,
// fixed order -> bitwise reproducible), every solve against a diagonal block is a product with that block's inverse, and a
// regression takes ~60 workgroup barriers instead of the ~330 of an unblocked factorisation (one per eliminated column).
//
//   layout   block (a, b), b <= a, of the train block lives in ONE wave's registers, TRANSPOSED in the MFMA accumulator layout:
//            lane (i, h) = (lane & 31, lane >> 5) holds A[32 a + i][32 b + j] for the 16 columns j = jmap(h, r) = (r & 3) +
//            8 (r >> 2) + 4 h, r = 0 .. 15 - row i of the block on the lane, the columns in the registers.  With the k index of an
//            MFMA step dealt the same way (half h supplies k = jmap(h, s)), the update T(a, b) -= L_b L_a^T reads both panel
//            blocks from LDS (row-major, stride 36 floats: conflict-free) with four ds_read_b128 per lane and needs no transpose.
//   blocks   enumerated by column (last first), dealt round-robin to the 16 waves: at every step the still-active blocks are a
//            prefix of that order, so the update is balanced to one block; a column's blocks sit on distinct waves.
//   gather   K is symmetric: lane (i, h) reads K[tr[32 b + j]][tr[32 a + i]] - per register a wave-uniform ROW (one per lane
//            half) and 32 ascending columns inside a ~200-column window - instead of 32 different rows per instruction.  Only
//            block columns 0, 1 and diagonal block 0 are fetched up front; the others are ADDED to the collected updates while
//            the diagonal block two steps before them is being factored (the Gram is 16 MB: these reads come from beyond the L2).
//   step kb  the column's blocks go to LDS (row-major); (1) ONE wave factors the diagonal block and inverts it in the same pass
//            (k2_factor_invert: the lower lane half holds the block's rows, the upper half the identity's) - while the other
//            waves run the deferred gathers; (2) the column's blocks: X = A M^T on the matrix pipe, and z_kb = M y_kb; (3) every
//            wave updates its active blocks with 16 MFMAs each, the panel's waves subtract L_a z_kb from the right-hand sides.
//            (History: the first version unrolled the in-wave routines per register slot, 200 KB of straight-line code that ran at
//            the speed of instruction-cache misses; the second solved the panel and the right-hand sides by 32-step recurrences
//            against L_kk - a dependent chain on one wave per block, ~14 000 cycles each)
//   then     back substitution block column by block column (the column's blocks go through LDS once more: the product with
//            L^T sums over the lane index; alpha_kb = M^T v is a 32-term dot product per lane), predictions one wave per four
//            validation rows.
// Rank-deficient blocks: a pivot at rounding level means the block is not positive definite in fp32 (the row is a combination
// of earlier ones: duplicate nodes, a rank-deficient kernel).  The reference's pinv (numpy default rcond 1e-15: every singular
// value of an fp32 block is kept) answers such a system with the least-squares solution plus whatever its rounding-level singular
// values contribute; the ridge system (K + lambda I) alpha = Y approaches the least-squares part as lambda -> 0 (for a PSD kernel
// the validation rows annihilate the null space of the train block).  Measured against the reference's per-epoch accuracies
// (tests/golden/kr_epochs.npz, an fp32 emulation of the factorisation): lambda = n eps max K_ii / 8 with pivots tested against
// n eps max K_ii / 64 is within one validation row on the synthetic sweep graphs and within two (one epoch: four) on texas / cora;
// round 2's 8 n eps max K_ii was 3 - 22 rows off on the rank-deficient real kernels.  The factorisation is redone ONCE on
// K + lambda I, pivots clamped to the test level.
constexpr int K2_THREADS = 1024, K2_WAVES = 16, K2_NB = 10, K2_SLOTS = 3;  // (K2_PS, the image stride: kr_blocks.h)
constexpr int KR_MAX_N = K2_NB * 32;  // train rows of a problem (320; its classes, KR_MAX_C: kr_deflate.h)
// the deflation workspace of a problem (wdg_kr_job.ws; kr_deflate.h holds the layout) at this solver's fixed stride of KR_MAX_N words
constexpr krw_offsets KRW(KR_MAX_N);
constexpr int KRW_LAB = KRW.lab, KRW_SCALE = KRW.scale, KRW_MIX = KRW.mix, KRW_VAL = KRW.val;
static_assert(K2_NB * (K2_NB - 1) / 2 <= K2_WAVES * K2_SLOTS, "every block below the diagonal needs a register slot");

// Deflation pre-pass (kr_deflate.h), one workgroup per problem, one thread per train row
constexpr int KD_THREADS = KR_MAX_N;
__global__ __launch_bounds__(KD_THREADS) void kr_deflate_kernel(const wdg_kr_job *__restrict__ jobs) {
    kr_deflate_one<KD_THREADS>(jobs + blockIdx.x, KR_MAX_N);
}

#ifdef K2_PROFILE  // diagnostic build (make EXTRA=-DK2_PROFILE): thread 0 of workgroup 0 sums the shader clocks spent per phase
#define K2_T(k)                                                                   \
    do {                                                                          \
        if (blockIdx.x == 0 && threadIdx.x == 0) {                                \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();         \
            k2_prof[k] += now_ - k2_last;                                         \
            k2_last = now_;                                                       \
        }                                                                         \
    } while (0)
#else
#define K2_T(k) do { } while (0)
#endif

// PERSISTENT form (round 5): a workgroup takes the problems blockIdx.x, blockIdx.x + gridDim.x, ... one after the other, and the
// PREDICTIONS of a problem (its validation rows' gathers from K: a sixth of a regression's cycles when they ran after the back
// substitution, all sixteen waves waiting on memory) are DEFERRED into the next problem's factorisation: while one wave factors
// and inverts a diagonal block, each of the other fifteen takes one unit of four validation rows of the PREVIOUS problem
// (alpha stays in `al` until the next back substitution; the train rows' ids are double-buffered).  What is left when the
// factorisation ends - and the last problem of a workgroup - is flushed by all waves.  Launched with one workgroup per problem
// (WDG_KR_PERSIST=0) every problem is a last problem: round 3's schedule.  Hit counts do not depend on the schedule.
// WS: every job of the table carries a deflation workspace (kr_deflate_kernel has run): the train rows to solve, their labels /
// right-hand sides and the validation rows' representatives and labels are read from it, and the pivot test is per row.
// WIN: the table holds CLASS-WINDOW jobs (include/wdg.h): a job carries the right-hand sides of classes class_base .. class_base + 7 of
// a problem of up to KR_ALL_C classes and leaves every validation row's best (value, class) of its window in rows_out - an
// instantiation of its own, launched only by the window entry: the plain entries' code reads neither field.
template <bool WS, bool WIN>
__global__ __launch_bounds__(K2_THREADS) void kr_solve_blocked_kernel(const wdg_kr_job *__restrict__ jobs, int n_jobs) {
    __shared__ float P[(K2_NB - 1) * 32 * K2_PS];      // the step's panel L[a, kb], a > kb: [a - kb - 1][row][k], stride 36
    __shared__ float LD[K2_NB * 32 * K2_PS];           // the diagonal blocks L_kk, row-major (kept: the back substitution reads them)
    __shared__ float stash[K2_SLOTS * 32 * K2_PS];     // the factoring wave's own register blocks, while it factors
    __shared__ float LT[32 * K2_PS];                   // the diagonal block being factored, by columns: LT[j][i] = l[i][j] (k2_factor_invert)
    __shared__ float zs[K2_NB * 32 * KR_MAX_C];        // right-hand sides: one-hot labels -> z = L^-1 Y (block by block)
    __shared__ float al[K2_NB * 32 * KR_MAX_C];        // alpha
    __shared__ float part[K2_WAVES][32][KR_MAX_C];     // per-wave partial sums (back substitution)
    __shared__ int tr_idx2[2][K2_NB * 32];             // the train rows' ids: this problem's and the previous one's (its predictions)
    __shared__ signed char blk_a[K2_WAVES * K2_SLOTS], blk_b[K2_WAVES * K2_SLOTS];
    __shared__ float sc[WS ? K2_NB * 32 : 1];            // (WS) sqrt(size) of a solved row's duplicate class: the block factored is S K S
    __shared__ int deficient, pend_hits, pend_next;    // pend_*: the deferred predictions' hit count and next unit of four rows
    __shared__ float red[K2_WAVES];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li_ = lane & 31, h_ = lane >> 5;
#ifdef K2_PROFILE
    unsigned long long k2_prof[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, k2_last = __builtin_amdgcn_s_memtime();
#endif
    // ---- the predictions of a finished problem `pj` (its alpha in `al`, its train ids in `tidx`): units of four validation rows,
    //      sixteen lanes per row, the lanes of a row split the train rows (ascending columns of one row of K); a row's sum: its
    //      lanes' partial sums added by a four-step butterfly - fixed order.  Units are dealt from an LDS counter: at most
    //      `max_units` to the calling wave (wave-uniform call sites).
    int pend_nt = 0;  // (uniform) the pending problem's train rows as solved (fewer than n_train after deflation)
    auto predict_units = [&](const desc_ptr<wdg_kr_job> pj, const int *tidx, int max_units) {
        const global_ptr<const float> pK = to_global(pj->K);
        const int pnv = pj->n_val;
        const int pcb = WIN ? pj->class_base : 0;                         // (uniform) the window's first class
        const int pC = WIN ? min(KR_MAX_C, pj->n_classes - pcb) : pj->n_classes;  // the columns that hold classes
        // with a deflation workspace (wdg_kr_deflate_batched) a validation row's kernel row (its representative) and its label come
        // from two arrays indexed by v - no id -> label chain; without: val[v] and labels[val[v]]
        constexpr bool pws = WS;
        const global_ptr<const int32_t> pval = pws ? to_global(static_cast<const int32_t *>(pj->ws)) + KRW_VAL : to_global(pj->val);
        const global_ptr<const int32_t> plabels = pws ? pval + pnv : to_global(pj->labels);
        const int64_t pldk = pj->ldk;
        const int pnt = pend_nt;
        const int g = lane >> 4, gl = lane & 15;
        for (int u = 0; u < max_units; ++u) {
            int unit = 0;
            if (lane == 0) unit = atomicAdd(&pend_next, 1);
            unit = __builtin_amdgcn_readfirstlane(unit);
            if (4 * unit >= pnv) break;
            const int v = 4 * unit + g, gv = pval[min(v, pnv - 1)];
            // (one uniform base + a 32-bit element offset per gather: a register per address - these loads are issued ten at a time
            // beside the factorisation's 48 accumulator registers; rows and columns are < ldk < 65 536, so row x ldk + column < 2^32:
            // unsigned offsets past 2^31 are exact - tests/test_gpu_kr_solver.py reads rows above 32 768 at ldk = 65 535)
            const unsigned row_off = static_cast<unsigned>(gv) * static_cast<unsigned>(pldk);
            float p[KR_MAX_C];
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c) p[c] = 0.f;
            // (a fixed trip count, predicated: two batches of ten gathers per lane - the K rows come from beyond the L2, and a
            // remainder loop would pay that latency once per leftover step.  The order is pinned - ten gathers, then their ten
            // products, alpha read from LDS as each is used: left alone the scheduler reads all of alpha first, 160 registers
            // beside the factorisation's accumulators)
#pragma unroll 1
            for (int b = 0; b < 2; ++b) {
                float kv[K2_NB];
#pragma unroll
                for (int k = 0; k < K2_NB; ++k) {
                    const int t = gl + 16 * (K2_NB * b + k);
                    const bool ok = t < pnt;
                    kv[k] = ok ? pK[row_off + static_cast<unsigned>(tidx[ok ? t : 0])] : 0.f;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < K2_NB; ++k) {
                    const int t = gl + 16 * (K2_NB * b + k);
                    const int ta = t < pnt ? t : 0;  // (kv is 0 there)
                    const float4 a0 = *reinterpret_cast<const float4 *>(&al[ta * KR_MAX_C]), a1 = *reinterpret_cast<const float4 *>(&al[ta * KR_MAX_C + 4]);
                    p[0] = fmaf(kv[k], a0.x, p[0]), p[1] = fmaf(kv[k], a0.y, p[1]), p[2] = fmaf(kv[k], a0.z, p[2]), p[3] = fmaf(kv[k], a0.w, p[3]);
                    p[4] = fmaf(kv[k], a1.x, p[4]), p[5] = fmaf(kv[k], a1.y, p[5]), p[6] = fmaf(kv[k], a1.z, p[6]), p[7] = fmaf(kv[k], a1.w, p[7]);
                    if (k & 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c)
                for (int o = 8; o > 0; o >>= 1) p[c] += __shfl_xor(p[c], o);  // (inside the row's 16 lanes: every lane ends with the sum)
            int best = 0;
            float bv = -3.4e38f;
            for (int c = 0; c < pC; ++c)
                if (p[c] > bv) {  // first maximum, like torch.argmax
                    bv = p[c];
                    best = c;
                }
            if constexpr (WIN) {  // the row's best of this window, for the combine pass (the pointer is read here: no register held for it)
                const global_ptr<i32x2_t> prow = to_global(reinterpret_cast<i32x2_t *>(pj->rows_out));  // (value, class): one 8-byte store
                best += pcb;
                if (pj->rows_out != nullptr && gl == 0 && v < pnv) prow[v] = i32x2_t{__builtin_bit_cast(int, bv), best};
            }
            const unsigned long long hit = __ballot(gl == 0 && v < pnv && best == plabels[pws ? min(v, pnv - 1) : gv]);
            if (lane == 0 && hit) atomicAdd(&pend_hits, __popcll(hit));
        }
    };
    // the pending problem's remaining units by every wave, then its hit count goes out (all threads call this)
    auto finish_pending = [&](const desc_ptr<wdg_kr_job> pj, const int *tidx) {
        predict_units(pj, tidx, 1 << 30);
        __syncthreads();
        if (tid == 0 && pj->correct_out) *to_global(pj->correct_out) = pend_hits;
        __syncthreads();
    };

    int pending = -1;  // (uniform) the problem whose predictions are still to be made: its alpha sits in `al`, its ids in tr_idx2[pend_buf]
    int pend_buf = 0;
    // Which problems a workgroup takes.  Consecutive problems of a sweep's table read the SAME kernel matrix (the epochs of one
    // (graph, classifier): 100 in a row), workgroup b runs on XCD b mod 8, and a 16-MB matrix is four L2s' worth: with the plain
    // deal (problems b, b + G, ..) the 32 CUs of an XCD work on every matrix in flight at once - 2.5 of them; dealt by XCD (an XCD's
    // workgroups take 32 consecutive problems per round) they share ONE matrix' lines in their L2.
    // (measured, 20 000 regressions: 11.97 -> 11.32 ms; an XCD owning one contiguous eighth of the table instead: 11.6.
    // WDG_KR_PERSIST=0 - one workgroup per problem - keeps the plain order.)
    const int G_ = gridDim.x, per_xcd = G_ >> 3;
    const bool by_xcd = (G_ & 7) == 0 && per_xcd > 0 && G_ < n_jobs;
    const int p_first = by_xcd ? (static_cast<int>(blockIdx.x) & 7) * per_xcd + (static_cast<int>(blockIdx.x) >> 3) : static_cast<int>(blockIdx.x);
  for (int prob = p_first; prob < n_jobs; prob += G_) {
    const desc_ptr<wdg_kr_job> job = (desc_ptr<wdg_kr_job>)(jobs + prob);
    const global_ptr<const float> K = to_global(job->K);
    const global_ptr<const int32_t> train = to_global(job->train), labels = to_global(job->labels);
    const int64_t ldk = job->ldk;
    const int nt_in = job->n_train, C = job->n_classes;
    // a deflation workspace (wdg_kr_deflate_batched has run on this table): the train rows to solve - one representative per class of
    // duplicate nodes, rows with K_ii == 0 dropped -, their right-hand sides (a class's mean one-hot label) and the validation rows'
    // representatives / labels are read from it; the reference's pseudo-inverse answers exactly singular blocks that way
    const global_ptr<const int32_t> ws = to_global(static_cast<const int32_t *>(job->ws));
    constexpr bool has_ws = WS;
    const bool ws_ok = !has_ws || job->ws != nullptr;  // (a table handed to the deflating entry with a job that has no workspace: refused below)
    const int nt = !has_ws ? nt_in : (ws_ok ? ws[KRW_NT] : -1);
    const bool deflated = has_ws && ws_ok && ws[KRW_DEFLATED] != 0;
    const int n_mixed = (has_ws && ws_ok) ? ws[KRW_MIXED] : 0;  // (uniform) listed right-hand-side entries (duplicates with different labels)
    // (ldk: the deferred predictions address K by 32-bit element offsets row x ldk + column, rows and columns < ldk - a wider kernel
    // matrix is refused HERE as well as by the Python launcher, so that a C-ABI caller gets correct_out = -1, not wrong hit counts)
    const int cb = WIN ? job->class_base : 0;  // (uniform) the window's first class
    bool bad_window = false;
    if constexpr (WIN) bad_window = cb < 0 || (cb & (KR_MAX_C - 1)) != 0 || cb >= C || (C > KR_MAX_C && job->rows_out == nullptr);
    if (nt_in <= 0 || nt_in > K2_NB * 32 || nt < 0 || nt > nt_in || C <= 0 || C > (WIN ? KR_ALL_C : KR_MAX_C) || bad_window || ldk <= 0 ||
        ldk >= 65536) {  // (uniform)
        if (tid == 0 && job->correct_out) *to_global(job->correct_out) = -1;
        if (tid == 0 && job->flags_out) *to_global(job->flags_out) = 0;
        continue;
    }
    int *const tr_idx = tr_idx2[pend_buf ^ 1];
    const int *const tr_prev = tr_idx2[pend_buf];
    const desc_ptr<wdg_kr_job> pjob = (desc_ptr<wdg_kr_job>)(jobs + (pending >= 0 ? pending : prob));
    const int nb = (nt + 31) >> 5;
    const int n_blocks = nb * (nb - 1) / 2;  // the blocks BELOW the diagonal live in registers; the diagonal blocks in LDS (LD)
    for (int i = tid; i < K2_NB * 32; i += K2_THREADS) {
        tr_idx[i] = i < nt ? (has_ws ? ws[KRW_TRAIN + i] : train[i]) : -1;
        if (has_ws) sc[i] = i < nt ? __builtin_bit_cast(float, ws[KRW_SCALE + i]) : 1.f;
    }
    if (tid < K2_WAVES * K2_SLOTS) {  // block `tid` of the enumeration: columns nb-2 .. 0, rows b+1 .. nb-1 inside a column
        int idx = tid, b = nb - 2;
        while (b >= 0 && idx >= nb - 1 - b) {
            idx -= nb - 1 - b;
            --b;
        }
        blk_a[tid] = static_cast<signed char>(b >= 0 ? b + 1 + idx : -1);
        blk_b[tid] = static_cast<signed char>(b);
    }
    __syncthreads();
    // max K_ii of the train rows (the scale of the pivot test)
    float dmax = 0.f;
    for (int t = tid; t < nt; t += K2_THREADS) {
        float d = K[static_cast<int64_t>(tr_idx[t]) * ldk + tr_idx[t]];
        if (has_ws) d *= sc[t] * sc[t];
        dmax = fmaxf(dmax, d);
    }
    for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o));
    if (lane == 0) red[wave] = dmax;
    __syncthreads();
    dmax = 0.f;
#pragma unroll
    for (int w = 0; w < K2_WAVES; ++w) dmax = fmaxf(dmax, red[w]);
    const float drop_below = static_cast<float>(nt) * 1.1920929e-7f * dmax * (1.f / 64.f);
    int sa[K2_SLOTS], sb[K2_SLOTS];  // this wave's blocks (wave-uniform)
#pragma unroll
    for (int s = 0; s < K2_SLOTS; ++s) {
        const int idx = wave + K2_WAVES * s;
        sa[s] = __builtin_amdgcn_readfirstlane(idx < n_blocks ? blk_a[idx] : -1);
        sb[s] = __builtin_amdgcn_readfirstlane(idx < n_blocks ? blk_b[idx] : -1);
    }

    f32x16 acc[K2_SLOTS];
    float ridge = 0.f;
    K2_T(0);  // setup
    for (int attempt = 0; attempt < 2; ++attempt) {
        // ---- right-hand sides and the gather
        for (int i = tid; i < K2_NB * 32 * KR_MAX_C; i += K2_THREADS) {
            const int row = i / KR_MAX_C, c = i % KR_MAX_C;
            float v = 0.f;
            if (row < nt) {
                const int lb = has_ws ? ws[KRW_LAB + row] : labels[tr_idx[row]];
                v = lb - cb == c ? (has_ws ? sc[row] : 1.f) : 0.f;  // (lb -1 / -2: never a column of any window)
                if (has_ws && lb == -2)  // (rare) a class of duplicates with different labels: its label counts over sqrt(size)
                    for (int e = 0; e < n_mixed; ++e) {
                        const int w = ws[KRW_MIX + e];
                        if ((w >> 12) == ((row << 4) | (c + cb))) v = static_cast<float>(w & 0xfff) / sc[row];
                    }
            }
            zs[i] = v;
        }  // (`al` is not touched: the back substitution writes every row it or the predictions read, and until then it holds the
        //    PREVIOUS problem's alpha, which the deferred predictions below are reading)
        if (tid == 0) deficient = 0;
        auto gather_block = [&](int a, int b, f32x16 &t) {  // lane (i, h): A[32 a + i][32 b + jmap(h, r)] = K[tr[32 b + j]][tr[32 a + i]]
            int li = li_, h = h_;
            asm volatile("" : "+v"(li), "+v"(h));
            const int gi = tr_idx[32 * a + li];  // the lane's row of the block = the COLUMN it reads (K is symmetric)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = k2_jmap(h, r), gj = tr_idx[32 * b + j];
                const bool diag = a == b && li == j;
                float v = (gi >= 0 && gj >= 0) ? K[static_cast<int64_t>(gj) * ldk + gi] : (diag ? 1.f : 0.f);
                if (has_ws) v *= sc[32 * a + li] * sc[32 * b + j];  // (1 for rows without duplicates: exact)
                if (diag && gi >= 0) v += ridge;
                t[r] = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // Only what the first step needs is gathered up front: block columns 0 and 1 and diagonal block 0.  Every other block starts
        // at zero, collects its updates, and has its K entries ADDED while the factoring wave works on the diagonal block
        // two steps (the diagonal blocks: one step) before it turns into a panel block - the gather of 55 blocks per regression
        // comes from beyond the L2 (a 16-MB Gram per graph and kernel) and was a sixth of the kernel's time in front of step 0.
#pragma unroll
        for (int s = 0; s < K2_SLOTS; ++s) {
            if (sa[s] >= 0 && sb[s] <= 1) gather_block(sa[s], sb[s], acc[s]);
            else
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
        }
        if (wave < nb) {  // the diagonal blocks: straight into their LDS images
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            if (wave == 0) gather_block(0, 0, t);
            k2_store_block(t, &LD[wave * 32 * K2_PS], li_, h_);
        }
        __syncthreads();
        K2_T(1);  // right-hand sides + gather

        // ---- the factorisation
        for (int kb = 0; kb < nb; ++kb) {
            // (lane coordinates made opaque per iteration: otherwise the compiler hoists every LDS address of the loop body -
            // dozens of loop-invariant lane-dependent offsets - out of the loop, spills them next to the 64 accumulator registers
            // and reloads each one from scratch memory, a global-memory round trip, in front of the LDS access that needs it)
            int li = li_, h = h_;
            asm volatile("" : "+v"(li), "+v"(h));
            // the column's blocks below the diagonal -> LDS, row-major: block (a, kb) into P[a - kb - 1]; the diagonal block is in
            // LD already.  role: 0 = this wave factors and inverts the diagonal block (the wave BEFORE the column's first block in
            // the deal: it holds none of the column's blocks and none of the blocks fetched in this step),
            // a - kb = it holds block (a, kb), -1 = neither
            int role = -1;
#pragma unroll
            for (int s = 0; s < K2_SLOTS; ++s) {
                if (sb[s] != kb) continue;  // (wave-uniform; a column's blocks sit on distinct waves)
                role = sa[s] - kb;
                k2_store_block(acc[s], &P[(role - 1) * 32 * K2_PS], li, h);
            }
            {
                // first block of column kb in the enumeration: sum over the columns after it
                const int first = (nb - 1 - kb) * (nb - 2 - kb) / 2;
                if (wave == ((first + K2_WAVES - 1) & (K2_WAVES - 1))) role = 0;
            }
            // (1) one wave factors the diagonal block and inverts it in the same pass: LD[kb] holds M = L_kk^-1 afterwards
            if (role == 0) {  // (wave-uniform)
                // (its own register blocks wait in LDS meanwhile: the routine wants 32 + 32 registers beside its chain)
#pragma unroll
                for (int s = 0; s < K2_SLOTS; ++s) k2_store_block(acc[s], &stash[s * 32 * K2_PS], li, h);
                if (k2_factor_invert(&LD[kb * 32 * K2_PS], LT, li, h, nt - 32 * kb, drop_below, ridge) && lane == 0) deficient = 1;
#pragma unroll
                for (int s = 0; s < K2_SLOTS; ++s) k2_load_block(acc[s], &stash[s * 32 * K2_PS], li, h);
            } else {  // (the other 15 waves would wait at the barrier: the deferred gathers run here, hidden behind the recurrence)
                const int first = (nb - 1 - kb) * (nb - 2 - kb) / 2;
#pragma unroll
                for (int s = 0; s < K2_SLOTS; ++s) {
                    if (sa[s] < 0 || sb[s] != kb + 2) continue;  // (wave-uniform; never the wave that factors at this step)
                    f32x16 t;
                    gather_block(sa[s], sb[s], t);
                    acc[s] += t;
                }
                if (kb + 1 < nb && wave == ((first + K2_WAVES - 2) & (K2_WAVES - 1))) {  // diagonal block kb + 1 (nobody else touches it now)
                    f32x16 t, d;
                    gather_block(kb + 1, kb + 1, t);
                    k2_load_block(d, &LD[(kb + 1) * 32 * K2_PS], li, h);
                    d += t;
                    k2_store_block(d, &LD[(kb + 1) * 32 * K2_PS], li, h);
                }
                // one unit of the previous problem's predictions per step, by the waves that have no block to fetch in this step (a
                // wave's unit takes about as long as the factoring wave's chain: two batches of gathers from beyond the L2; a wave
                // that fetches a block AND predicts holds the step's barrier back - measured: every wave one unit 12.08 ms, every
                // third wave 11.80, the idle waves 11.73 against 12.25 ms without deferral, 20 000 regressions)
                bool busy = kb + 1 < nb && wave == ((first + K2_WAVES - 2) & (K2_WAVES - 1));
#pragma unroll
                for (int s = 0; s < K2_SLOTS; ++s) busy |= sa[s] >= 0 && sb[s] == kb + 2;
                if (pending >= 0 && !busy)
                    predict_units(pjob, tr_prev, 1);  // one unit of the previous problem's predictions per wave and step
            }
            K2_T(2);
            __syncthreads();
            K2_T(3);
            if (deficient && attempt == 0) break;  // (uniform) restart on K + ridge I
            // (2) the column's other blocks: X L_kk^T = A  <=>  X = A M^T, 16 MFMAs per block (lane (i, h): row i of A from P, row i
            //     of M from LD, the k index dealt like the accumulator's columns - the layout of the trailing update); the factoring
            //     wave meanwhile: z_kb = M y_kb
            if (role > 0) {
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.f;
                const float *pa = &P[((role - 1) * 32 + li) * K2_PS + 4 * h];
                const float *pm = &LD[(kb * 32 + li) * K2_PS + 4 * h];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 va = *reinterpret_cast<const float4 *>(pa + 8 * q), vm = *reinterpret_cast<const float4 *>(pm + 8 * q);
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.x, va.x, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.y, va.y, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.z, va.z, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.w, va.w, t, 0, 0, 0);
                }
                k2_store_block(t, &P[(role - 1) * 32 * K2_PS], li, h);  // L[a, kb], final (only this wave touches the image)
            } else if (role == 0) {  // z_kb[i] = sum_k M[i][k] y[k]: the lane halves split k, one cross-half add
                float sum[KR_MAX_C];
#pragma unroll
                for (int c = 0; c < KR_MAX_C; ++c) sum[c] = 0.f;
                const float *mrow = &LD[(kb * 32 + li) * K2_PS + 4 * h];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 m = *reinterpret_cast<const float4 *>(mrow + 8 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float *y = &zs[(32 * kb + 8 * q + 4 * h + e) * KR_MAX_C];
                        const float4 y0 = *reinterpret_cast<const float4 *>(y), y1 = *reinterpret_cast<const float4 *>(y + 4);
                        const float l = e == 0 ? m.x : e == 1 ? m.y : e == 2 ? m.z : m.w;
                        sum[0] = fmaf(l, y0.x, sum[0]), sum[1] = fmaf(l, y0.y, sum[1]), sum[2] = fmaf(l, y0.z, sum[2]), sum[3] = fmaf(l, y0.w, sum[3]);
                        sum[4] = fmaf(l, y1.x, sum[4]), sum[5] = fmaf(l, y1.y, sum[5]), sum[6] = fmaf(l, y1.z, sum[6]), sum[7] = fmaf(l, y1.w, sum[7]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int c = 0; c < KR_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                if (h == 0) {  // (every read of y above precedes these writes: they depend on all of them)
                    *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KR_MAX_C]) = make_float4(sum[0], sum[1], sum[2], sum[3]);
                    *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KR_MAX_C + 4]) = make_float4(sum[4], sum[5], sum[6], sum[7]);
                }
            }
            K2_T(4);
            __syncthreads();
            K2_T(5);
            // (3) the panel's blocks come back into their registers; the trailing update T(a, b) -= L_b L_a^T on the matrix pipe;
            //     the panel's waves subtract L_a z_kb from the right-hand sides
#pragma unroll
            for (int s = 0; s < K2_SLOTS; ++s) {
                if (sb[s] > kb) {
                    const float *pa = &P[((sa[s] - kb - 1) * 32 + li) * K2_PS + 4 * h];
                    const float *pb = &P[((sb[s] - kb - 1) * 32 + li) * K2_PS + 4 * h];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 va = *reinterpret_cast<const float4 *>(pa + 8 * q), vb = *reinterpret_cast<const float4 *>(pb + 8 * q);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.x, va.x, acc[s], 0, 0, 0);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.y, va.y, acc[s], 0, 0, 0);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.z, va.z, acc[s], 0, 0, 0);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.w, va.w, acc[s], 0, 0, 0);
                    }
                } else if (sb[s] == kb && sa[s] > kb) {
                    k2_load_block(acc[s], &P[(sa[s] - kb - 1) * 32 * K2_PS], li, h);  // L[a, kb], final
                    float sum[KR_MAX_C];
#pragma unroll
                    for (int c = 0; c < KR_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float *z = &zs[(32 * kb + k2_jmap(h, r)) * KR_MAX_C];
                        const float4 z0 = *reinterpret_cast<const float4 *>(z), z1 = *reinterpret_cast<const float4 *>(z + 4);
                        const float l = acc[s][r];
                        sum[0] = fmaf(l, z0.x, sum[0]), sum[1] = fmaf(l, z0.y, sum[1]), sum[2] = fmaf(l, z0.z, sum[2]), sum[3] = fmaf(l, z0.w, sum[3]);
                        sum[4] = fmaf(l, z1.x, sum[4]), sum[5] = fmaf(l, z1.y, sum[5]), sum[6] = fmaf(l, z1.z, sum[6]), sum[7] = fmaf(l, z1.w, sum[7]);
                        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int c = 0; c < KR_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                    if (h == 0) {
                        float *y = &zs[(32 * sa[s] + li) * KR_MAX_C];
#pragma unroll
                        for (int c = 0; c < KR_MAX_C; ++c) y[c] -= sum[c];
                    }
                }
            }
            {  // the diagonal blocks (a, a), a > kb, live in LDS: LD[a] -= L[a, kb] L[a, kb]^T, dealt to the waves from the top (the
               // deal of the register blocks fills the waves from the bottom)
                const int da = kb + 1 + (K2_WAVES - 1 - wave);
                if (da < nb) {  // (wave-uniform)
                    f32x16 t;
                    k2_load_block(t, &LD[da * 32 * K2_PS], li, h);
                    const float *pa = &P[((da - kb - 1) * 32 + li) * K2_PS + 4 * h];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 va = *reinterpret_cast<const float4 *>(pa + 8 * q);
                        t = __builtin_amdgcn_mfma_f32_32x32x2f32(-va.x, va.x, t, 0, 0, 0);
                        t = __builtin_amdgcn_mfma_f32_32x32x2f32(-va.y, va.y, t, 0, 0, 0);
                        t = __builtin_amdgcn_mfma_f32_32x32x2f32(-va.z, va.z, t, 0, 0, 0);
                        t = __builtin_amdgcn_mfma_f32_32x32x2f32(-va.w, va.w, t, 0, 0, 0);
                    }
                    k2_store_block(t, &LD[da * 32 * K2_PS], li, h);
                }
            }
            K2_T(6);
            __syncthreads();
            K2_T(7);
        }
        __syncthreads();
        if (!deficient || attempt == 1) break;  // (uniform)
        ridge = 8.f * drop_below;                // = n eps max K_ii / 8
        __syncthreads();
    }

    // ---- what is left of the previous problem's predictions (the back substitution below overwrites its alpha)
    if (pending >= 0) {
        finish_pending(pjob, tr_prev);
        pending = -1;
    }
    if (nt == 0 && tid < KR_MAX_C) al[tid] = 0.f;  // (every train row dropped: no back substitution writes alpha; the predictions' masked reads hit row 0)
    K2_T(14);
    // ---- back substitution L^T alpha = z, block column by block column from the last (L_kk: still in LD)
    for (int kb = nb - 1; kb >= 0; --kb) {
        int li = li_, h = h_;  // (opaque per iteration: see the factorisation loop)
        asm volatile("" : "+v"(li), "+v"(h));
#pragma unroll
        for (int s = 0; s < K2_SLOTS; ++s)  // the column's blocks below the diagonal -> LDS, row-major
            if (sb[s] == kb && sa[s] > kb) k2_store_block(acc[s], &P[(sa[s] - kb - 1) * 32 * K2_PS], li, h);
        __syncthreads();
        K2_T(10);
        // wave w takes block a = kb + 1 + w: lane (j, h) sums L[i][j] alpha_a[i][.] over the 16 rows i of its half
        if (wave < nb - kb - 1) {
            const int a = kb + 1 + wave;
            float sum[KR_MAX_C];
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll 4
            for (int ii = 0; ii < 16; ++ii) {
                const int i = 16 * h + ii;
                const float l = P[(wave * 32 + i) * K2_PS + li];
                const float *av = &al[(32 * a + i) * KR_MAX_C];
                const float4 a0 = *reinterpret_cast<const float4 *>(av), a1 = *reinterpret_cast<const float4 *>(av + 4);
                sum[0] = fmaf(l, a0.x, sum[0]), sum[1] = fmaf(l, a0.y, sum[1]), sum[2] = fmaf(l, a0.z, sum[2]), sum[3] = fmaf(l, a0.w, sum[3]);
                sum[4] = fmaf(l, a1.x, sum[4]), sum[5] = fmaf(l, a1.y, sum[5]), sum[6] = fmaf(l, a1.z, sum[6]), sum[7] = fmaf(l, a1.w, sum[7]);
            }
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < KR_MAX_C; ++c) part[wave][li][c] = sum[c];
            }
        }
        K2_T(11);
        __syncthreads();
        K2_T(12);
        if (wave == 0) {  // alpha_kb = L_kk^-T (z_kb - the blocks' sums): lane = column j, rows k from the last
            float v[KR_MAX_C];
            {
                const float4 r0 = *reinterpret_cast<const float4 *>(&zs[(32 * kb + li) * KR_MAX_C]), r1 = *reinterpret_cast<const float4 *>(&zs[(32 * kb + li) * KR_MAX_C + 4]);
                v[0] = r0.x, v[1] = r0.y, v[2] = r0.z, v[3] = r0.w, v[4] = r1.x, v[5] = r1.y, v[6] = r1.z, v[7] = r1.w;
            }
#pragma unroll 3
            for (int w = 0; w < nb - kb - 1; ++w) {  // (fixed order)
                const float4 p0 = *reinterpret_cast<const float4 *>(&part[w][li][0]), p1 = *reinterpret_cast<const float4 *>(&part[w][li][4]);
                v[0] -= p0.x, v[1] -= p0.y, v[2] -= p0.z, v[3] -= p0.w, v[4] -= p1.x, v[5] -= p1.y, v[6] -= p1.z, v[7] -= p1.w;
            }
            K2_T(13);
            // alpha_kb[i] = sum_j M[j][i] v[j] (M = L_kk^-1 sits in LD[kb]): v goes through the block's z slot so that every lane can
            // read every row of it (one wave: its LDS operations are carried out in issue order); the lane halves split j
            if (h == 0) {
                *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KR_MAX_C]) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KR_MAX_C + 4]) = make_float4(v[4], v[5], v[6], v[7]);
            }
            float sum[KR_MAX_C];
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll 4
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * h + jj;
                const float m = LD[(kb * 32 + j) * K2_PS + li];
                const float *vj = &zs[(32 * kb + j) * KR_MAX_C];
                const float4 v0 = *reinterpret_cast<const float4 *>(vj), v1 = *reinterpret_cast<const float4 *>(vj + 4);
                sum[0] = fmaf(m, v0.x, sum[0]), sum[1] = fmaf(m, v0.y, sum[1]), sum[2] = fmaf(m, v0.z, sum[2]), sum[3] = fmaf(m, v0.w, sum[3]);
                sum[4] = fmaf(m, v1.x, sum[4]), sum[5] = fmaf(m, v1.y, sum[5]), sum[6] = fmaf(m, v1.z, sum[6]), sum[7] = fmaf(m, v1.w, sum[7]);
            }
#pragma unroll
            for (int c = 0; c < KR_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
            if (h == 0) {
                const bool real = 32 * kb + li < nt;
                *reinterpret_cast<float4 *>(&al[(32 * kb + li) * KR_MAX_C]) = real ? make_float4(sum[0], sum[1], sum[2], sum[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(&al[(32 * kb + li) * KR_MAX_C + 4]) = real ? make_float4(sum[4], sum[5], sum[6], sum[7]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __syncthreads();
        K2_T(8);
    }

    // (WS) a class's weight as the predictions apply it: sqrt(size) x the scaled system's solution - once the back substitution, which
    // reads alpha's later blocks, is through (the loop's last barrier has passed)
    if (has_ws && deflated) {
        for (int i = tid; i < nt * KR_MAX_C; i += K2_THREADS) al[i] *= sc[i / KR_MAX_C];
    }
    // ---- this problem's predictions wait for the next problem's factorisation (or for the flush below)
    if (tid == 0) {
        // (bit 2 read here, not held through the factorisation: one live register more there spills)
        const bool dropped = has_ws && ws_ok && ws[KRW_DROPPED] != 0;
        if (job->flags_out) *to_global(job->flags_out) = (ridge > 0.f ? 1 : 0) | (deflated ? 2 : 0) | (dropped ? 4 : 0);
        pend_hits = 0;
        pend_next = 0;
    }
    pending = prob;
    pend_nt = nt;
    pend_buf ^= 1;  // (tr_idx2[pend_buf] = the ids just used)
    __syncthreads();
  }
    if (pending >= 0) finish_pending((desc_ptr<wdg_kr_job>)(jobs + pending), tr_idx2[pend_buf]);
#ifdef K2_PROFILE
    K2_T(9);
    if (blockIdx.x == 0 && tid == 0)
        printf("k2 cycles: setup %llu gather %llu diag %llu b1 %llu panel %llu b2 %llu update %llu b3 %llu bwd-solve %llu pred %llu | bwd: store+bar %llu "
               "contrib %llu bar %llu sums %llu\n", k2_prof[0], k2_prof[1], k2_prof[2], k2_prof[3], k2_prof[4], k2_prof[5], k2_prof[6], k2_prof[7],
               k2_prof[8], k2_prof[9], k2_prof[10], k2_prof[11], k2_prof[12], k2_prof[13]);
#endif
}

template <bool WIN>
int kernel_regress_launch(const wdg_kr_job *jobs_dev, int32_t n_jobs, bool deflated, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "kernel_regress_batched: negative size");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "kernel_regress_batched: null job table");
    // the blocked solver is persistent: one workgroup per CU (its 144 KB of LDS allow no second one) walks the problems and makes a
    // problem's predictions inside the next one's factorisation; WDG_KR_PERSIST=0: one workgroup per problem (round 3's schedule)
    static const bool persist = [] {
        const char *e = getenv("WDG_KR_PERSIST");
        return !(e && atoi(e) == 0 && e[0] != '\0');
    }();
    const int cus = wdg::device_cus();
    if (deflated) {
        hipLaunchKernelGGL(kr_deflate_kernel, dim3(static_cast<unsigned>(n_jobs)), dim3(KD_THREADS), 0, wdg::as_stream(stream), jobs_dev);
        if (const int rc = wdg::check_launch("kr_deflate_kernel")) return rc;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kr_solve_blocked_kernel<true, WIN>), dim3(persist ? (n_jobs < cus ? n_jobs : cus) : n_jobs), dim3(K2_THREADS), 0,
                           wdg::as_stream(stream), jobs_dev, n_jobs);
    } else hipLaunchKernelGGL(HIP_KERNEL_NAME(kr_solve_blocked_kernel<false, WIN>), dim3(persist ? (n_jobs < cus ? n_jobs : cus) : n_jobs), dim3(K2_THREADS), 0,
                              wdg::as_stream(stream), jobs_dev, n_jobs);
    return wdg::check_launch("kr_solve_blocked_kernel");
}

}  // namespace

extern "C" {

int wdg_kernel_regress_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    return kernel_regress_launch<false>(jobs_dev, n_jobs, false, stream);
}

int wdg_kernel_regress_deflated_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream) {
    return kernel_regress_launch<false>(jobs_dev, n_jobs, true, stream);
}

int wdg_kernel_regress_windows_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, int32_t deflate, wdg_stream_t stream) {
    return kernel_regress_launch<true>(jobs_dev, n_jobs, deflate != 0, stream);
}

int32_t wdg_kernel_regress_max_train(void) { return KR_MAX_N; }

size_t wdg_kr_deflate_workspace_bytes(int32_t n_val) { return krw_bytes(KR_MAX_N, n_val); }

}  // extern "C"
