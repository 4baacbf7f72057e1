// Batched C-SVC over a precomputed Gram: the svm_rbf / svm_poly / svm_linear branches of the classifier-based performance metric, every
// (epoch, feature matrix) problem of a call in two launches.
//
// replaces: `G_svm = svm.SVC(kernel='rbf', gamma=0.5, C=0.1).fit(X_agg[idx_train], labels_sample[idx_train])`, its poly / linear
//           variants, the X twins, `G_svm.predict(X_agg[idx_val])` / `X_svm.predict(X[idx_val])` and the two accuracies that follow
//           (utils/homophily_metrics.py:313-333, utils/homophily_plot.py:334-354), called once per epoch of
//           classifier_based_performance_metric (:260-349).
//
// The arithmetic is libsvm's C-SVC as scikit-learn calls it (tol 1e-3, one-vs-one, no shrinking: shrinking changes the path, not the
// eps-optimum), restated line by line in tests/_svm_ref.py, which the tests pin against scikit-learn:
//   launch 1  svm_solve_kernel, grid (pair of classes, problem), ONE wave64 per binary problem.  Row t of the pair (the train rows of
//             class p, then those of class q, ascending) lives in lane t % 64, slot t / 64: alpha and the gradient in fp64 registers,
//             at most 16 slots (1024 rows).  An iteration is two arg-reductions over the wave (butterflies of lane exchanges, the row
//             index breaks ties: libsvm keeps the LAST maximiser / minimiser), two gathered rows of the Gram (row i before the second
//             selection, row j after it; L2 hits, hidden by the other resident waves) and the two-variable update, computed by every
//             lane alike.  No barrier, no atomic, no LDS in the loop; the loop ends at the stopping rule or at max_iter.
//             A kernel entry is formed in fp64 from the fp32 Gram entry and rounded to fp32 (libsvm's kernel cache holds floats).
//   launch 2  svm_predict_kernel, grid (16 validation rows, problem): a wave per validation row, the train rows grouped by class; per
//             class the lanes stride over its rows and sum coefficient x kernel entry (fp64, unrounded) for every opponent class, a
//             butterfly per sum; then a lane per pair forms the decision value and the votes are counted with ballots.
// The solver leaves in ws: per pair its rho, iteration count and cap flag, gamma, and the coefficient table coef[k][t] (libsvm's
// sv_coef: alpha_t y_t of train row t against its k-th opponent class, k skipping the row's own class).
#include "wdg_common.h"

#pragma clang fp contract(off)  // the restatement's bits: a product and the sum it goes into round separately

namespace {

using namespace wdg;

constexpr int SVM_MAX_C = 16;
constexpr int SVM_MAX_TRAIN = 1024;
constexpr int SVM_MAX_SLOTS = SVM_MAX_TRAIN / 64;
constexpr int SVM_PAIR_WORDS = 128;                      // >= 16 * 15 / 2
constexpr int SVM_HEAD_BYTES = 2 * SVM_PAIR_WORDS * 4 + SVM_PAIR_WORDS * 8 + 256;  // iterations, cap flags (int32), rho (fp64), gamma
constexpr int SVM_VAL_PER_BLOCK = 16;
constexpr double SVM_TAU = 1e-12, SVM_EPS = 1e-3;

__device__ __forceinline__ global_ptr<int> svm_iters(const desc_ptr<wdg_svm_job> job) { return to_global(static_cast<int *>(job->ws)); }
__device__ __forceinline__ global_ptr<int> svm_capped(const desc_ptr<wdg_svm_job> job) { return svm_iters(job) + SVM_PAIR_WORDS; }
__device__ __forceinline__ global_ptr<double> svm_rho(const desc_ptr<wdg_svm_job> job) {
    return to_global(reinterpret_cast<double *>(static_cast<char *>(job->ws) + 2 * SVM_PAIR_WORDS * 4));
}
__device__ __forceinline__ global_ptr<double> svm_gamma(const desc_ptr<wdg_svm_job> job) { return svm_rho(job) + SVM_PAIR_WORDS; }
__device__ __forceinline__ global_ptr<double> svm_coef(const desc_ptr<wdg_svm_job> job) {
    return to_global(reinterpret_cast<double *>(static_cast<char *>(job->ws) + SVM_HEAD_BYTES));
}

__device__ __forceinline__ int pair_index(int p, int q, int C) { return p * C - p * (p + 1) / 2 + (q - p - 1); }  // (p, q), p < q

__device__ __forceinline__ bool job_ok(const desc_ptr<wdg_svm_job> job) {
    return job->n_train >= 1 && job->n_train <= SVM_MAX_TRAIN && job->n_classes >= 1 && job->n_classes <= SVM_MAX_C;
}

struct KernelFn {
    int kind, degree;
    double gamma;
    __device__ __forceinline__ double powi(double base) const {  // libsvm's repeated squaring
        double tmp = base, ret = 1.0;
        for (int t = degree; t > 0; t /= 2) {
            if (t % 2 == 1) ret *= tmp;
            tmp = tmp * tmp;
        }
        return ret;
    }
    // fp64 kernel entry from the fp32 half Gram entry and the two rows' squared norms
    __device__ __forceinline__ double entry(float g_half, float n2a, float n2b) const {
        const double g = 2.0 * static_cast<double>(g_half);
        if (kind == WDG_SVM_LINEAR) return g;
        if (kind == WDG_SVM_POLY) return powi(gamma * g);
        return exp(-gamma * ((static_cast<double>(n2a) + static_cast<double>(n2b)) - 2.0 * g));
    }
    __device__ __forceinline__ double diag(float n2) const {
        if (kind == WDG_SVM_LINEAR) return static_cast<double>(n2);
        if (kind == WDG_SVM_POLY) return powi(gamma * static_cast<double>(n2));
        return 1.0;
    }
};

__device__ __forceinline__ double wave_sum(double v) {  // fixed order: every lane ends with the same bits
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave: the train rows' positions grouped by class (ascending within a class) -> rows[], cnt[c] per class (uniform registers).
__device__ __forceinline__ void group_rows(const desc_ptr<wdg_svm_job> job, int lane, int *rows, int (&cnt)[SVM_MAX_C]) {
    const int nt = job->n_train, C = job->n_classes;
    const global_ptr<const int32_t> train = to_global(job->train), labels = to_global(job->labels);
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int c = 0; c < SVM_MAX_C; ++c) cnt[c] = 0;
    for (int base = 0; base < nt; base += 64) {
        const int t = base + lane;
        const int l = t < nt ? labels[train[t]] : -1;
#pragma unroll
        for (int c = 0; c < SVM_MAX_C; ++c)
            if (c < C) cnt[c] += __popcll(__ballot(l == c));
    }
    int fill[SVM_MAX_C];
    int run = 0;
#pragma unroll
    for (int c = 0; c < SVM_MAX_C; ++c) fill[c] = run, run += c < C ? cnt[c] : 0;
    for (int base = 0; base < nt; base += 64) {
        const int t = base + lane;
        const int l = t < nt ? labels[train[t]] : -1;
#pragma unroll
        for (int c = 0; c < SVM_MAX_C; ++c)
            if (c < C) {
                const unsigned long long m = __ballot(l == c);
                if (l == c) rows[fill[c] + __popcll(m & below)] = t;
                fill[c] += __popcll(m);
            }
    }
}

// gamma: the job's, or scikit-learn's 'scale' = 1 / (F var) over all elements of the train rows (one wave; fixed summation order)
__device__ __forceinline__ double resolve_gamma(const desc_ptr<wdg_svm_job> job, int lane) {
    if (job->gamma > 0.0 || job->kernel == WDG_SVM_LINEAR) return job->gamma > 0.0 ? job->gamma : 1.0;
    if (job->row_sum == nullptr || job->F < 1) return 1.0;
    const global_ptr<const int32_t> train = to_global(job->train);
    const global_ptr<const float> norm2 = to_global(job->norm2);
    const global_ptr<const double> row_sum = to_global(job->row_sum);
    double s1 = 0.0, s2 = 0.0;
    for (int t = lane; t < job->n_train; t += 64) {
        const int id = train[t];
        s1 += row_sum[id];
        s2 += static_cast<double>(norm2[id]);
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    const double m = static_cast<double>(job->n_train) * static_cast<double>(job->F);
    const double mean = s1 / m;
    const double var = s2 / m - mean * mean;
    return var > 0.0 ? 1.0 / (static_cast<double>(job->F) * var) : 1.0;
}

// A lane's per-slot state: vectors, not arrays - elements only ever move by constant index, so they stay in registers (the compiler
// turns a chain of selects over ARRAY elements into one load at a selected address, which pins the array to scratch memory)
template <typename T, int R>
struct slots {
    typedef T type __attribute__((ext_vector_type(R)));
};

// the value row t's owner (lane t % 64) holds for it; the other lanes return something of their own that nobody reads
template <int R, typename T, typename V>
__device__ __forceinline__ T owned(const V a, int lane, int t) {
    T v = a[0];
#pragma unroll
    for (int k = 1; k < R; ++k)
        if (k * 64 + lane == t) v = a[k];
    return v;
}

// One binary problem on one wave: rows [0, n_p) are +1, [n_p, n) are -1; row t in lane t % 64, slot t / 64.
template <int R>
__device__ __forceinline__ void svm_solve_pair(const desc_ptr<wdg_svm_job> job, const KernelFn kf, const int *rows_p, const int *rows_q, int n_p, int n,
                               int lane, int col_p, int col_q, int pair) {
    const global_ptr<const float> G = to_global(job->G_half), norm2 = to_global(job->norm2);
    const global_ptr<const int32_t> train = to_global(job->train);
    const int64_t ldk = job->ldk;
    const double Cbox = job->C;
    const int max_iter = job->max_iter;
    typename slots<double, R>::type alpha, grad;
    typename slots<float, R>::type n2, ki, kj;
    typename slots<int, R>::type id;
#pragma unroll
    for (int s = 0; s < R; ++s) {
        const int t = min(s * 64 + lane, n - 1);  // (slots past the end mirror the last row: their loads stay inside the tables)
        id[s] = train[t < n_p ? rows_p[t] : rows_q[t - n_p]];
        n2[s] = norm2[id[s]];
        alpha[s] = 0.0, grad[s] = -1.0, ki[s] = 0.f, kj[s] = 0.f;
    }
    const double inf = __builtin_huge_val();
    int iter = 0, capped = 0;
    for (;;) {
        if (iter >= max_iter) {
            capped = 1;
            break;
        }
        // i: the last maximiser of -y G over the up set; Gmax2: the largest y G over the low set
        double gmax = -inf, gmax2 = -inf;
        int i = -1;
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const int t = s * 64 + lane;
            if (t < n) {
                const bool pos = t < n_p;
                const bool up = pos ? alpha[s] < Cbox : alpha[s] > 0.0, low = pos ? alpha[s] > 0.0 : alpha[s] < Cbox;
                const double m = pos ? -grad[s] : grad[s];
                if (up && m >= gmax) gmax = m, i = t;
                if (low && -m > gmax2) gmax2 = -m;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(gmax, o), o2 = __shfl_xor(gmax2, o);
            const int oi = __shfl_xor(i, o);
            if (ov > gmax || (ov == gmax && oi > i)) gmax = ov, i = oi;
            gmax2 = o2 > gmax2 ? o2 : gmax2;
        }
        if (i < 0 || gmax + gmax2 < SVM_EPS) break;
        const int li = i & 63, si = i >> 6;
        const double y_i = i < n_p ? 1.0 : -1.0;
        const int id_i = __builtin_amdgcn_readfirstlane(__shfl(owned<R, int>(id, lane, i), li));
        const float n2_i = __shfl(owned<R, float>(n2, lane, i), li);
        const double alpha_i = __shfl(owned<R, double>(alpha, lane, i), li);
        const double qd_i = kf.diag(n2_i);
        const global_ptr<const float> g_i = G + static_cast<int64_t>(id_i) * ldk;
#pragma unroll
        for (int s = 0; s < R; ++s)
            if (s * 64 < n) ki[s] = static_cast<float>(kf.entry(g_i[id[s]], n2_i, n2[s]));  // (a wave-uniform skip of the unused slots)
        // j: the last minimiser of -b^2 / a over the low set with b > 0
        double best = inf;
        int j = -1;
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const int t = s * 64 + lane;
            if (t < n) {
                const bool pos = t < n_p;
                const bool low = pos ? alpha[s] > 0.0 : alpha[s] < Cbox;
                const double b = gmax + (pos ? grad[s] : -grad[s]);
                if (low && b > 0.0) {
                    double a = (qd_i + kf.diag(n2[s])) - 2.0 * static_cast<double>(ki[s]);
                    a = a > 0.0 ? a : SVM_TAU;
                    const double obj = -(b * b) / a;
                    if (obj <= best) best = obj, j = t;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o);
            const int oj = __shfl_xor(j, o);
            if (oj >= 0 && (j < 0 || ov < best || (ov == best && oj > j))) best = ov, j = oj;
        }
        if (j < 0) break;
        ++iter;
        const int lj = j & 63, sj = j >> 6;
        const double y_j = j < n_p ? 1.0 : -1.0;
        const int id_j = __builtin_amdgcn_readfirstlane(__shfl(owned<R, int>(id, lane, j), lj));
        const float n2_j = __shfl(owned<R, float>(n2, lane, j), lj);
        const double alpha_j = __shfl(owned<R, double>(alpha, lane, j), lj), grad_j = __shfl(owned<R, double>(grad, lane, j), lj);
        const double q_ij = y_i * y_j * static_cast<double>(__shfl(owned<R, float>(ki, lane, j), lj));
        const global_ptr<const float> g_j = G + static_cast<int64_t>(id_j) * ldk;
#pragma unroll
        for (int s = 0; s < R; ++s)
            if (s * 64 < n) kj[s] = static_cast<float>(kf.entry(g_j[id[s]], n2_j, n2[s]));
        // the two-variable step with libsvm's box clipping (every lane computes it)
        const double grad_i = -y_i * gmax, qd_j = kf.diag(n2_j);
        double ai = alpha_i, aj = alpha_j;
        if (y_i != y_j) {
            double quad = (qd_i + qd_j) + 2.0 * q_ij;
            quad = quad > 0.0 ? quad : SVM_TAU;
            const double delta = (-grad_i - grad_j) / quad, diff = ai - aj;
            ai += delta, aj += delta;
            if (diff > 0.0) {
                if (aj < 0.0) aj = 0.0, ai = diff;
            } else if (ai < 0.0) {
                ai = 0.0, aj = -diff;
            }
            if (diff > 0.0) {
                if (ai > Cbox) ai = Cbox, aj = Cbox - diff;
            } else if (aj > Cbox) {
                aj = Cbox, ai = Cbox + diff;
            }
        } else {
            double quad = (qd_i + qd_j) - 2.0 * q_ij;
            quad = quad > 0.0 ? quad : SVM_TAU;
            const double delta = (grad_i - grad_j) / quad, sum = ai + aj;
            ai -= delta, aj += delta;
            if (sum > Cbox) {
                if (ai > Cbox) ai = Cbox, aj = sum - Cbox;
            } else if (aj < 0.0) {
                aj = 0.0, ai = sum;
            }
            if (sum > Cbox) {
                if (aj > Cbox) aj = Cbox, ai = sum - Cbox;
            } else if (ai < 0.0) {
                ai = 0.0, aj = sum;
            }
        }
        const double d_i = ai - alpha_i, d_j = aj - alpha_j;
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const double y_s = s * 64 + lane < n_p ? 1.0 : -1.0;
            const double q_is = y_i * y_s * static_cast<double>(ki[s]), q_js = y_j * y_s * static_cast<double>(kj[s]);
            grad[s] += q_is * d_i + q_js * d_j;
            if (s == si && lane == li) alpha[s] = ai;
            if (s == sj && lane == lj) alpha[s] = aj;
        }
    }
    // rho: the mean of y G over the free alphas, or the midpoint of the bounds
    double ub = inf, lb = -inf, sum_free = 0.0;
    int n_free = 0;
#pragma unroll
    for (int s = 0; s < R; ++s) {
        const int t = s * 64 + lane;
        if (t < n) {
            const bool pos = t < n_p;
            const double yg = pos ? grad[s] : -grad[s];
            if (alpha[s] >= Cbox) {
                if (pos) lb = yg > lb ? yg : lb; else ub = yg < ub ? yg : ub;
            } else if (alpha[s] <= 0.0) {
                if (pos) ub = yg < ub ? yg : ub; else lb = yg > lb ? yg : lb;
            } else {
                ++n_free, sum_free += yg;
            }
        }
    }
    sum_free = wave_sum(sum_free);
    for (int o = 32; o > 0; o >>= 1) {
        const double ou = __shfl_xor(ub, o), ol = __shfl_xor(lb, o);
        n_free += __shfl_xor(n_free, o);
        ub = ou < ub ? ou : ub, lb = ol > lb ? ol : lb;
    }
    const double rho = n_free > 0 ? sum_free / static_cast<double>(n_free) : (ub + lb) / 2.0;
    const global_ptr<double> coef = svm_coef(job);
    const int nt = job->n_train;
#pragma unroll
    for (int s = 0; s < R; ++s) {
        const int t = s * 64 + lane;
        if (t < n) {
            const bool pos = t < n_p;
            coef[static_cast<int64_t>(pos ? col_p : col_q) * nt + (pos ? rows_p[t] : rows_q[t - n_p])] = pos ? alpha[s] : -alpha[s];
        }
    }
    if (lane == 0) {
        svm_rho(job)[pair] = rho;
        svm_iters(job)[pair] = iter;
        svm_capped(job)[pair] = capped;
    }
}

// grid (pairs of classes, problems), one wave per workgroup; R: the slots per lane the launch provides (64 R >= the largest train block)
template <int R>
__global__ __launch_bounds__(64) void svm_solve_kernel(const wdg_svm_job *__restrict__ jobs) {
    __shared__ int rows[SVM_MAX_TRAIN];
    const desc_ptr<wdg_svm_job> job = (desc_ptr<wdg_svm_job>)(jobs + blockIdx.y);
    const int lane = threadIdx.x, C = job->n_classes, pair = blockIdx.x;
    if (!job_ok(job)) return;
    if (pair == 0 && lane == 0 && job->correct) *to_global(job->correct) = 0;
    if (pair > 0 && pair >= C * (C - 1) / 2) return;
    int p = 0, first = 0;  // pair -> (p, q)
    while (p < C - 2 && pair >= first + (C - 1 - p)) first += C - 1 - p, ++p;
    const int q = p + 1 + (pair - first);
    int cnt[SVM_MAX_C];
    group_rows(job, lane, rows, cnt);
    __syncthreads();  // (one wave: orders the LDS writes before the reads below)
    int start_p = 0, start_q = 0, n_p = 0, n_q = 0;
#pragma unroll
    for (int c = 0; c < SVM_MAX_C; ++c) {
        if (c < p) start_p += cnt[c];
        if (c < q) start_q += cnt[c];
        if (c == p) n_p = cnt[c];
        if (c == q) n_q = cnt[c];
    }
    KernelFn kf;
    kf.kind = job->kernel, kf.degree = job->degree, kf.gamma = resolve_gamma(job, lane);
    if (pair == 0 && lane == 0) *svm_gamma(job) = kf.gamma;
    if (q >= C || n_p == 0 || n_q == 0) return;  // a class of this pair is absent
    const int n = n_p + n_q;
    if (n > 64 * R) return;  // (the launcher sized R by the largest train block it was told of)
    svm_solve_pair<R>(job, kf, rows + start_p, rows + start_q, n_p, n, lane, q - 1, p, pair);
}

// grid (chunks of 16 validation rows, problems): a wave per validation row; workgroup 0 of a problem also writes its info
__global__ __launch_bounds__(256) void svm_predict_kernel(const wdg_svm_job *__restrict__ jobs) {
    __shared__ int rows[SVM_MAX_TRAIN];      // train positions grouped by class
    __shared__ int tid[SVM_MAX_TRAIN];       // ... their row ids
    __shared__ float tn2[SVM_MAX_TRAIN];     // ... and squared norms
    __shared__ int s_cnt[SVM_MAX_C], s_start[SVM_MAX_C], s_rank[SVM_MAX_C];
    __shared__ int s_present, s_stat[3], s_sv[4];
    __shared__ double S[4][SVM_MAX_C][SVM_MAX_C];
    const desc_ptr<wdg_svm_job> job = (desc_ptr<wdg_svm_job>)(jobs + blockIdx.y);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int C = job->n_classes, nt = job->n_train, nv = job->n_val;
    const bool lead = blockIdx.x == 0;
    const global_ptr<int> info = to_global(job->info);
    if (!job_ok(job)) {
        if (lead && t == 0) {
            if (job->correct) *to_global(job->correct) = -1;  // refused
            if (job->info) info[0] = 0, info[1] = 0, info[2] = 0, info[3] = 0;
        }
        return;
    }
    if (!lead && blockIdx.x * SVM_VAL_PER_BLOCK >= nv) return;
    if (w == 0) {
        int cnt[SVM_MAX_C];
        group_rows(job, lane, rows, cnt);
        if (lane == 0) {
            int run = 0, present = 0;
#pragma unroll
            for (int c = 0; c < SVM_MAX_C; ++c) {
                s_cnt[c] = c < C ? cnt[c] : 0, s_start[c] = run, s_rank[c] = present;
                run += c < C ? cnt[c] : 0, present += c < C && cnt[c] > 0;
            }
            s_present = present, s_stat[0] = 0, s_stat[1] = 0, s_stat[2] = 0;
        }
    }
    __syncthreads();
    const global_ptr<const int32_t> train = to_global(job->train);
    const global_ptr<const float> G = to_global(job->G_half), norm2 = to_global(job->norm2);
    for (int u = t; u < nt; u += 256) {
        const int id = train[rows[u]];
        tid[u] = id, tn2[u] = norm2[id];
    }
    const int P = s_present;
    const global_ptr<const double> coef = svm_coef(job);
    unsigned present = 0;  // bit c: class c has train rows
#pragma unroll
    for (int c = 0; c < SVM_MAX_C; ++c) present |= s_cnt[c] > 0 ? 1u << c : 0u;
    if (lead) {  // info: iterations, the largest count, support vectors, flags
        for (int pr = t; pr < C * (C - 1) / 2; pr += 256) {
            int p = 0, first = 0;
            while (p < C - 2 && pr >= first + (C - 1 - p)) first += C - 1 - p, ++p;
            const int q = p + 1 + (pr - first);
            if ((present >> p & 1u) && (present >> q & 1u)) {
                const int it = svm_iters(job)[pr];
                atomicAdd(&s_stat[0], it);
                atomicMax(&s_stat[1], it);
                if (svm_capped(job)[pr]) atomicOr(&s_stat[2], WDG_SVM_FLAG_MAX_ITER);
            }
        }
        int sv = 0;
        if (P >= 2)
            for (int a = 0; a < C; ++a)
                for (int u = t; u < s_cnt[a]; u += 256) {
                    const int pos = rows[s_start[a] + u];
                    bool any = false;
                    for (int b = 0; b < C; ++b)
                        if (b != a && (present >> b & 1u)) any = any || coef[static_cast<int64_t>(b < a ? b : b - 1) * nt + pos] != 0.0;
                    sv += any;
                }
        sv = static_cast<int>(wave_sum(static_cast<double>(sv)));
        if (lane == 0) s_sv[w] = sv;
    }
    __syncthreads();
    if (lead && t == 0 && job->info) {
        info[0] = P >= 2 ? s_stat[0] : 0, info[1] = P >= 2 ? s_stat[1] : 0;
        info[2] = P >= 2 ? s_sv[0] + s_sv[1] + s_sv[2] + s_sv[3] : 0;
        info[3] = P >= 2 ? s_stat[2] : WDG_SVM_FLAG_ONE_CLASS;
    }
    if (P < 2) return;
    KernelFn kf;
    kf.kind = job->kernel, kf.degree = job->degree, kf.gamma = *svm_gamma(job);
    const global_ptr<const int32_t> val = to_global(job->val), labels = to_global(job->labels);
    const int n_pairs = C * (C - 1) / 2;
    int hits = 0;
    for (int k = 0; k < SVM_VAL_PER_BLOCK / 4; ++k) {
        const int r = blockIdx.x * SVM_VAL_PER_BLOCK + k * 4 + w;
        const bool active = r < nv;  // (wave-uniform)
        const int id_v = active ? val[r] : train[0];
        const float n2_v = norm2[id_v];
        const global_ptr<const float> g_v = G + static_cast<int64_t>(id_v) * job->ldk;
        for (int a = 0; a < C; ++a) {
            const int n_a = active ? s_cnt[a] : 0, start = s_start[a];
            if (n_a == 0) continue;
            double acc[SVM_MAX_C - 1];
#pragma unroll
            for (int c = 0; c < SVM_MAX_C - 1; ++c) acc[c] = 0.0;
            for (int u = lane; u < n_a; u += 64) {
                const int pos = rows[start + u];
                const double kv = kf.entry(g_v[tid[start + u]], n2_v, tn2[start + u]);
#pragma unroll
                for (int c = 0; c < SVM_MAX_C - 1; ++c)
                    if (c < C - 1 && (present >> (c < a ? c : c + 1) & 1u)) acc[c] += coef[static_cast<int64_t>(c) * nt + pos] * kv;
            }
#pragma unroll
            for (int c = 0; c < SVM_MAX_C - 1; ++c)
                if (c < C - 1 && (present >> (c < a ? c : c + 1) & 1u)) {
                    const double v = wave_sum(acc[c]);
                    if (lane == c) S[w][a][c] = v;
                }
        }
        __syncthreads();
        // a lane per pair: decision value and vote
        int votes[SVM_MAX_C];
#pragma unroll
        for (int c = 0; c < SVM_MAX_C; ++c) votes[c] = 0;
        for (int pr0 = 0; pr0 < n_pairs; pr0 += 64) {
            const int pr = pr0 + lane;
            int winner = -1;
            if (active && pr < n_pairs) {
                int p = 0, first = 0;
                while (p < C - 2 && pr >= first + (C - 1 - p)) first += C - 1 - p, ++p;
                const int q = p + 1 + (pr - first);
                if (s_cnt[p] > 0 && s_cnt[q] > 0) {
                    double d = S[w][p][q - 1] + S[w][q][p];
                    d -= svm_rho(job)[pr];
                    winner = d > 0.0 ? p : q;
                    if (job->dec) to_global(job->dec)[static_cast<int64_t>(r) * n_pairs + pair_index(s_rank[p], s_rank[q], P)] = d;
                }
            }
#pragma unroll
            for (int c = 0; c < SVM_MAX_C; ++c)
                if (c < C) votes[c] += __popcll(__ballot(winner == c));
        }
        int best = -1, best_v = -1;
#pragma unroll
        for (int c = 0; c < SVM_MAX_C; ++c)
            if (c < C && s_cnt[c] > 0 && votes[c] > best_v) best = c, best_v = votes[c];
        if (active && lane == 0) {
            if (job->pred) to_global(job->pred)[r] = best;
            hits += labels[id_v] == best;
        }
        __syncthreads();
    }
    if (lane == 0 && hits && job->correct) atomicAdd(job->correct, hits);
}

}  // namespace

extern "C" size_t wdg_svm_workspace_bytes(int32_t n_train, int32_t n_classes) {
    if (n_train < 0 || n_classes < 0) return 0;
    const size_t cols = n_classes > 1 ? static_cast<size_t>(n_classes - 1) : 1;
    const size_t b = static_cast<size_t>(SVM_HEAD_BYTES) + cols * static_cast<size_t>(n_train) * sizeof(double);
    return (b + 255) / 256 * 256;
}

extern "C" int wdg_svm_batched_f32(const wdg_svm_job *jobs_dev, int32_t n_jobs, int32_t max_train, int32_t max_val, int32_t max_classes,
                                   wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_train >= 0 && max_val >= 0, "svm_batched: negative size");
    WDG_REQUIRE(max_classes >= 0 && max_classes <= SVM_MAX_C, "svm_batched: at most 16 classes");
    WDG_REQUIRE(max_train <= SVM_MAX_TRAIN, "svm_batched: at most 1024 train rows");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "svm_batched: null job table");
    WDG_REQUIRE(n_jobs <= 65535, "svm_batched: at most 65 535 problems per launch");
    hipStream_t st = wdg::as_stream(stream);
    const unsigned pairs = static_cast<unsigned>(max_classes * (max_classes - 1) / 2);
    const dim3 grid(pairs > 0 ? pairs : 1, n_jobs);
    if (max_train <= 128) hipLaunchKernelGGL(svm_solve_kernel<2>, grid, dim3(64), 0, st, jobs_dev);
    else if (max_train <= 256) hipLaunchKernelGGL(svm_solve_kernel<4>, grid, dim3(64), 0, st, jobs_dev);
    else if (max_train <= 512) hipLaunchKernelGGL(svm_solve_kernel<8>, grid, dim3(64), 0, st, jobs_dev);
    else hipLaunchKernelGGL(svm_solve_kernel<SVM_MAX_SLOTS>, grid, dim3(64), 0, st, jobs_dev);
    hipLaunchKernelGGL(svm_predict_kernel, dim3(static_cast<unsigned>(wdg::ceil_div(max_val > 0 ? max_val : 1, SVM_VAL_PER_BLOCK)), n_jobs),
                       dim3(256), 0, st, jobs_dev);
    return wdg::check_launch("svm_predict_kernel");
}
