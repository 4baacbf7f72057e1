// Every epoch of many multinomial logistic heads in one launch: logits = M W, cross-entropy over the train rows, torch's Adam,
// model selection on the validation hits - one workgroup per model, no host, no hipGraph, nothing between workgroups.
//
// replaces: the training loops behind the SGC-1 and MLP-1 accuracy tables (gnns_on_syn.py:109-154, gnns_on_syn.py:213-249; the loop
//           itself lives upstream of the reference) - for SGC-1 M is the cached A_hat X, for MLP-1 M is X.  The arithmetic restates
//           sweep.TrainBatch.epoch() for kind "sgc" / "mlp1": two batched GEMM launches and ~15 small PyTorch launches per epoch there.
//
// Ownership: thread i of a workgroup holds W[f, :] and dW[f, :] of the features f = i + k * THREADS, k < FPT, in registers; a row of M is
// read as one contiguous (coalesced) row, R rows per step.  The Adam update is thread-local (m, v stay in device memory: one read and one
// write per epoch).  Only the R x C partial logits of a step cross lanes: a reduce-scatter butterfly inside the wave (a value's 64
// partials are added in the order of lane distances 32, 16, .. 1 whatever its slot: P - 1 + log2(64 / P) exchanges for P values), the
// waves' sums through LDS in wave order.  The first P threads finish the rows - softmax with the maximum subtracted, the first maximum
// as the prediction - and hand (softmax - onehot) / n_train back through LDS for dW += x^T G, rows in order.  Every sum has one
// order that depends on the job alone (its F picks THREADS / FPT / R, its C the padded class count): a job's result does not depend on the
// table it is in, two runs are bit-identical, no floating-point atomic is used.
// One pass over M per epoch: pass p walks train | val | test once with W_p - the gradient of epoch p over the train rows, the hits of
// epoch p - 1 over the others - pass 0 stops after the train rows and pass `epochs` starts at the first step that holds another row.
// Steps are aligned to the start of the row list in every pass, so a call of a + b epochs and calls of a, then b epochs do the same sums.
#include "ipow.h"  // b^t in fp64 by squaring: a function of t alone (a call that starts at step0 gets the bits of one that ran through it)
#include "wdg_common.h"

namespace {

using namespace wdg;

constexpr int HT_MAX_F = 4096, HT_MAX_C = 8;
// five shapes of workgroup by F: <= 256, <= 512, <= 1024, <= 2048, <= 4096

__host__ __device__ constexpr int ht_cfg(int F) { return F <= 256 ? 0 : F <= 512 ? 1 : F <= 1024 ? 2 : F <= 2048 ? 3 : 4; }
__host__ __device__ constexpr int ht_cfg_max_f(int cfg) { return 256 << cfg; }
__host__ __device__ constexpr int ht_cp(int C) { return C <= 2 ? 2 : C <= 4 ? 4 : 8; }

// v[0 .. P) of every lane -> the sum over the 64 lanes of value (lane >> (6 - log2 P)), in every lane of that group
template <int K, int P>
__device__ __forceinline__ void ht_scatter_stage(float (&v)[P], const int lane) {  // K values stay, K go to the lane at distance 64 K / P
    if constexpr (K >= 1) {
        constexpr int D = 64 * K / P;
        const bool up = (lane & D) != 0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const float send = up ? v[i] : v[i + K], keep = up ? v[i + K] : v[i];
            v[i] = keep + __shfl_xor(send, D);
        }
        ht_scatter_stage<K / 2, P>(v, lane);
    }
}
template <int P>
__device__ __forceinline__ float ht_wave_reduce_scatter(float (&v)[P], const int lane) {
    ht_scatter_stage<P / 2, P>(v, lane);
    float s = v[0];
#pragma unroll
    for (int d = 32 / P; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

template <int CP, int FPT, int T, int R, int CFG>
__global__ __launch_bounds__(T) void head_train_kernel(const wdg_head_train_job *__restrict__ jobs, const int epochs, const int step0, const float lr,
                                                        const float weight_decay, const float beta1, const float beta2, const float eps) {
    constexpr int P = R * CP, NW = T / kWave;
    constexpr int LOG_P = P == 64 ? 6 : P == 32 ? 5 : P == 16 ? 4 : P == 8 ? 3 : P == 4 ? 2 : 1;
    static_assert(P <= 64 && (P & (P - 1)) == 0 && FPT * T >= ht_cfg_max_f(CFG), "a step's values fit one wave; the threads cover the features");
    __shared__ float red[2][NW][P];  // the waves' sums of a step's P logits, two steps deep
    __shared__ float gsh[P];         // (softmax - onehot) / n_train of the step's rows
    __shared__ int hits[2];
    const desc_ptr<wdg_head_train_job> job = (desc_ptr<wdg_head_train_job>)(jobs + blockIdx.x);
    const int F = job->F, C = job->C, ntr = job->n_train, nva = job->n_val, nte = job->n_test;
    // (uniform) the instantiation that owns this job's shape runs it; a job outside the limits is left untouched
    if (F < 1 || F > HT_MAX_F || C < 1 || C > HT_MAX_C || ht_cfg(F) != CFG || ht_cp(C) != CP) return;
    if (ntr < 1 || nva < 1 || nte < 0 || job->ldm < F) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const global_ptr<const float> M = to_global(job->M);
    const global_ptr<const int32_t> labels = to_global(job->labels), train = to_global(job->train), val = to_global(job->val),
                                    test = to_global(job->test);
    const global_ptr<float> Wg = to_global(job->W), mg = to_global(job->m), vg = to_global(job->v);
    const int64_t ldm = job->ldm;
    const int n_rows = ntr + nva + nte, n_steps = (n_rows + R - 1) / R;
    const int my_r = (t / CP) % R, my_c = t % CP;  // the (row slot, class) a thread of the first P finishes

    float W[FPT][CP], dW[FPT][CP];
#pragma unroll
    for (int k = 0; k < FPT; ++k)
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const int f = t + k * T;
            W[k][c] = (f < F && c < C) ? Wg[static_cast<int64_t>(f) * C + c] : 0.f;
            dW[k][c] = 0.f;
        }
    int best_val = 0, best_test = 0, best_epoch = 0;
    if (t == 0) {
        const global_ptr<const int32_t> b = to_global(static_cast<const int32_t *>(job->best));
        best_val = b[0], best_test = b[1], best_epoch = b[2];
        hits[0] = hits[1] = 0;
    }

    const auto row_id = [&](const int pos) -> int {
        if (pos >= n_rows) return -1;
        return pos < ntr ? train[pos] : pos < ntr + nva ? val[pos - ntr] : test[pos - ntr - nva];
    };
    // the rows of step s (R whole rows, the thread's FPT elements of each) and, for the first P threads, their row's class
    const auto load_step = [&](const int s, float (&x)[R][FPT], int &lab) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int id = row_id(s * R + r);
#pragma unroll
            for (int k = 0; k < FPT; ++k) {
                const int f = t + k * T;
                x[r][k] = (id >= 0 && f < F) ? M[static_cast<int64_t>(id) * ldm + f] : 0.f;
            }
        }
        lab = -1;
        if (t < P) {
            const int id = row_id(s * R + my_r);
            if (id >= 0) lab = labels[id];
        }
    };

    for (int p = 0; p <= epochs; ++p) {
        const bool do_train = p < epochs, do_eval = p > 0;
        const int s_begin = do_train ? 0 : ntr / R, s_end = do_eval ? n_steps : (ntr + R - 1) / R;
        int val_hits = 0, test_hits = 0;
        float xn[R][FPT];
        int labn;
        load_step(s_begin, xn, labn);
        for (int s = s_begin; s < s_end; ++s) {
            float x[R][FPT];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < FPT; ++k) x[r][k] = xn[r][k];
            const int lab = labn;
            if (s + 1 < s_end) load_step(s + 1, xn, labn);  // (in flight through this step's sums)

            float part[P];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < CP; ++c) {
                    float a = 0.f;
#pragma unroll
                    for (int k = 0; k < FPT; ++k) a = fmaf(x[r][k], W[k][c], a);
                    part[r * CP + c] = a;
                }
            const float wsum = ht_wave_reduce_scatter<P>(part, lane);
            if ((lane & ((64 >> LOG_P) - 1)) == 0) red[s & 1][wave][lane >> (6 - LOG_P)] = wsum;
            __syncthreads();
            const bool grad_step = do_train && s * R < ntr;  // (uniform) the step holds a train row
            if (t < P) {
                float z = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) z += red[s & 1][w][t];
                const int pos = s * R + my_r;
                const float zc = my_c < C ? z : -INFINITY;
                float bv = zc;
                int bi = my_c;
#pragma unroll
                for (int o = CP / 2; o >= 1; o >>= 1) {  // the first maximum of the row's classes (torch.argmax), in every lane of the row
                    const float ov = __shfl_xor(bv, o);
                    const int oi = __shfl_xor(bi, o);
                    const bool take = ov > bv || (ov == bv && oi < bi);
                    bv = take ? ov : bv;
                    bi = take ? oi : bi;
                }
                const float e = my_c < C ? expf(z - bv) : 0.f;
                float sum = e;
#pragma unroll
                for (int o = CP / 2; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
                float g = 0.f;
                if (do_train && pos < ntr) g = (e / sum - (my_c == lab ? 1.f : 0.f)) / static_cast<float>(ntr);
                gsh[t] = g;
                if (do_eval && my_c == 0 && pos >= ntr && pos < n_rows && bi == lab) {
                    if (pos < ntr + nva)
                        ++val_hits;
                    else
                        ++test_hits;
                }
            }
            if (grad_step) {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < CP; ++c) {
                        const float g = gsh[r * CP + c];
#pragma unroll
                        for (int k = 0; k < FPT; ++k) dW[k][c] = fmaf(x[r][k], g, dW[k][c]);
                    }
            }
        }
        if (do_eval) {  // the hits of W_p: the evaluation of epoch step0 + p - 1
            if (t < P && my_c == 0) {
                atomicAdd(&hits[0], val_hits);  // (integers: any order gives the same sum)
                atomicAdd(&hits[1], test_hits);
            }
            __syncthreads();
            if (t == 0) {
                if (hits[0] > best_val) best_val = hits[0], best_test = hits[1], best_epoch = step0 + p - 1;
                hits[0] = hits[1] = 0;
            }
        }
        if (do_train) {  // torch.optim.Adam, step step0 + p + 1: the L2 term goes into the gradient
            const int step = step0 + p + 1;
            const float step_size = static_cast<float>(static_cast<double>(lr) / (1.0 - ipow_f64(static_cast<double>(beta1), step)));
            const float bc2_sqrt = static_cast<float>(sqrt(1.0 - ipow_f64(static_cast<double>(beta2), step)));
#pragma unroll
            for (int k = 0; k < FPT; ++k) {
                const int f = t + k * T;
#pragma unroll
                for (int c = 0; c < CP; ++c) {
                    if (f < F && c < C) {
                        const int64_t i = static_cast<int64_t>(f) * C + c;
                        const float g = fmaf(weight_decay, W[k][c], dW[k][c]);
                        const float m1 = beta1 * mg[i] + (1.f - beta1) * g;
                        const float v1 = beta2 * vg[i] + (1.f - beta2) * g * g;
                        mg[i] = m1, vg[i] = v1;
                        W[k][c] -= step_size * (m1 / (sqrtf(v1) / bc2_sqrt + eps));
                    }
                    dW[k][c] = 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FPT; ++k)
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const int f = t + k * T;
            if (f < F && c < C) Wg[static_cast<int64_t>(f) * C + c] = W[k][c];
        }
    if (t == 0) {
        const global_ptr<int32_t> b = to_global(job->best);
        b[0] = best_val, b[1] = best_test, b[2] = best_epoch;
    }
}

template <int CP, int FPT, int T, int R, int CFG>
void ht_launch(const wdg_head_train_job *jobs, int n_jobs, int epochs, int step0, float lr, float wd, float b1, float b2, float eps, hipStream_t st) {
    hipLaunchKernelGGL((head_train_kernel<CP, FPT, T, R, CFG>), dim3(static_cast<unsigned>(n_jobs)), dim3(T), 0, st, jobs, epochs, step0, lr, wd, b1,
                       b2, eps);
}

// rows per step: as many as the wave's 64 reduction slots and the registers of the row elements (two steps deep) allow
template <int CP>
void ht_launch_cfg(int cfg, const wdg_head_train_job *jobs, int n_jobs, int epochs, int step0, float lr, float wd, float b1, float b2, float eps,
                   hipStream_t st) {
    switch (cfg) {
        case 0: return ht_launch<CP, 1, 256, 64 / CP < 8 ? 64 / CP : 8, 0>(jobs, n_jobs, epochs, step0, lr, wd, b1, b2, eps, st);
        case 1: return ht_launch<CP, 2, 256, 64 / CP < 8 ? 64 / CP : 8, 1>(jobs, n_jobs, epochs, step0, lr, wd, b1, b2, eps, st);
        case 2: return ht_launch<CP, 4, 256, 64 / CP < 8 ? 64 / CP : 8, 2>(jobs, n_jobs, epochs, step0, lr, wd, b1, b2, eps, st);
        case 3: return ht_launch<CP, 8, 256, 4, 3>(jobs, n_jobs, epochs, step0, lr, wd, b1, b2, eps, st);
        default: return ht_launch<CP, 8, 512, 1, 4>(jobs, n_jobs, epochs, step0, lr, wd, b1, b2, eps, st);
    }
}

}  // namespace

extern "C" int wdg_head_train_batched_f32(const wdg_head_train_job *jobs_dev, int32_t n_jobs, int32_t max_F, int32_t max_C, int32_t epochs,
                                          int32_t step0, float lr, float weight_decay, float beta1, float beta2, float eps, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "head_train_batched: negative job count");
    WDG_REQUIRE(epochs >= 0 && step0 >= 0 && step0 <= INT32_MAX - 1 - epochs, "head_train_batched: negative epoch count or first step");
    WDG_REQUIRE(lr == lr && weight_decay == weight_decay && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f,
                "head_train_batched: Adam needs 0 <= beta < 1 and eps >= 0");
    if (max_F < 1 || max_F > HT_MAX_F || max_C < 1 || max_C > HT_MAX_C)
        return wdg::fail(WDG_ERR_UNSUPPORTED, "head_train_batched: a head of 1..%d features and 1..%d classes (got %d, %d)", HT_MAX_F, HT_MAX_C, max_F, max_C);
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "head_train_batched: null job table");
    if (epochs == 0) return WDG_OK;
    hipStream_t st = wdg::as_stream(stream);
    // one launch per (padded class count, feature range) that the table can hold: a job runs in the one its own shape names
    for (int cfg = 0; cfg <= ht_cfg(max_F); ++cfg) {
        ht_launch_cfg<2>(cfg, jobs_dev, n_jobs, epochs, step0, lr, weight_decay, beta1, beta2, eps, st);
        if (max_C > 2) ht_launch_cfg<4>(cfg, jobs_dev, n_jobs, epochs, step0, lr, weight_decay, beta1, beta2, eps, st);
        if (max_C > 4) ht_launch_cfg<8>(cfg, jobs_dev, n_jobs, epochs, step0, lr, weight_decay, beta1, beta2, eps, st);
    }
    return wdg::check_launch("head_train_kernel");
}
