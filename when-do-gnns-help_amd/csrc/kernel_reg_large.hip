// Kernel-regression metric on the device, train blocks of up to 1024 rows: a second batched Cholesky solver beside
// csrc/kernel_reg.hip, whose register-resident factor ends at 320 rows.  Here the factor lives in DEVICE MEMORY: a 1024-row lower
// triangle is 2 MiB of fp32, more than a CU's register file.
//
// replaces: the kernel-regression branch of classifier_based_performance_metric (utils/homophily_metrics.py:283-297,
//           utils/homophily_plot.py:296-310: `K_val_train @ (np.linalg.pinv(K_train_train) @ onehot[idx_train])`, argmax, accuracy)
//           for `--sample_max` above 533 (homophily_tests.py:54), where an epoch's train block outgrows the register solver.
//
//   * kr_large_deflate_kernel  the deflation pre-pass (csrc/kr_deflate.h) for up to 1024 train rows, persistent over the table;
//   * kr_large_solve_kernel    one workgroup of 8 waves per problem, persistent over the job table.
//
//   storage  the factor as packed 32 x 32 blocks of the lower triangle (block (a, b), b <= a, at (a (a + 1) / 2 + b) x 4 KiB, row-major,
//            stride 32) in a launch-level scratch buffer: slice blockIdx.x belongs to the RESIDENT WORKGROUP, not to the job - 528 blocks
//            = 2.1 MiB per workgroup, one workgroup per CU, however long the table is.  A workgroup only reads what it wrote itself
//            while it worked on the same problem (its waves share the CU's vector L1; a barrier orders the accesses).  The diagonal
//            block's place holds M = L_kk^-1 (all that the substitutions need of it).
//   column   LEFT-LOOKING by block column kb.  The wave that owns block (a, kb) gathers K[tr, tr] for it straight from the Gram (the
//            symmetric read of kernel_reg.hip: K_tt is never materialised), subtracts sum_j L(a, j) L(kb, j)^T, j ascending, on
//            v_mfma_f32_32x32x2_f32 - the accumulator stays in registers, the block is written once.  The row panel L(kb, .), which all
//            of the column's waves read, is staged in LDS in parts of 8 blocks (stride 36: conflict-free; a whole 31-block panel
//            would be 143 KiB); L(a, .), private to the wave, streams from the L2.  Wave 0 owns the diagonal block alone and
//            factors + inverts it with the register solver's one-wave routine (k2_factor_invert, kr_blocks.h) as soon as its own
//            sum is through; waves 1 .. 7 are dealt the blocks below it round-robin (up to 5 each: 80 accumulator registers).
//            Then the panel: X = A M^T on the matrix pipe (A back from the wave's own scratch block as an MFMA operand), and the
//            right-hand sides inside the same step: z_kb = M y_kb (wave 0), y_a -= L(a, kb) z_kb (the block's wave).
//   then     back substitution block column by block column (each wave sums its blocks a = kb + 1 + wave, + 8, .. ascending, wave
//            0 subtracts the eight partial sums in wave order: alpha_kb = M^T v), predictions K[val, train] alpha four validation
//            rows per wave at a time, arg-max by first maximum, one hit count per problem.
// Every sum has a fixed order that depends on the problem alone - not on the workgroup that took it, not on the table: a relaunch
// is bit-identical.  The numerical contract is the register solver's: pivots tested against n eps max K_ii / 64, ONE refactorisation
// on K + (n eps max K_ii / 8) I (flags bit 0), the deflated block scaled by the square roots of the class sizes (bits 1 and 2),
// ldk < 65 536, the sentinel -1 for shapes out of range.
#include "wdg_common.h"
#include "kr_blocks.h"
#include "kr_deflate.h"

namespace {

using namespace wdg;

constexpr int KL_THREADS = 512, KL_WAVES = 8, KL_NB = 32, KL_MAX_N = KL_NB * 32, KL_MAX_C = KR_MAX_C;
constexpr int KL_SLOTS = 5;                         // blocks of one column a wave holds: ceil((KL_NB - 1) / (KL_WAVES - 1))
constexpr int KL_CH = 8;                            // blocks of the row panel staged in LDS at a time
constexpr int KL_BLOCKS = KL_NB * (KL_NB + 1) / 2;  // 528 blocks of the lower triangle
constexpr size_t KL_WG_BYTES = static_cast<size_t>(KL_BLOCKS) * 4096;
static_assert((KL_NB - 1 + KL_WAVES - 2) / (KL_WAVES - 1) <= KL_SLOTS, "every block of a column needs a register slot");

// Deflation pre-pass (kr_deflate.h: the routine and the layout of the workspace, whose four per-row arrays take P = the problem's OWN
// train rows rounded up to 32 words each here), one thread per train row.  Persistent over the job table like the solver: a table
// without workspaces costs two workgroups per CU that read its ws pointers, not a workgroup per problem
constexpr int KLD_THREADS = KL_MAX_N;
__global__ __launch_bounds__(KLD_THREADS) void kr_large_deflate_kernel(const wdg_kr_job *__restrict__ jobs, int n_jobs) {
    for (int prob = blockIdx.x; prob < n_jobs; prob += gridDim.x) {
        kr_deflate_one<KLD_THREADS>(jobs + prob, krw_pad(((desc_ptr<wdg_kr_job>)(jobs + prob))->n_train));
        __syncthreads();  // (the next problem's pass overwrites the shared arrays)
    }
}

__device__ __forceinline__ int kl_blk(int a, int b) { return a * (a + 1) / 2 + b; }  // b <= a

// WIN: the table holds CLASS-WINDOW jobs (include/wdg.h; the register solver's form of the same name): an instantiation of its own,
// launched only by the window entry - and compiled in a unit of its own (csrc/kernel_reg_large_windows.hip includes this file with
// KL_WINDOWS_UNIT defined): a second instantiation in THIS unit changes the code generated for the first (its register allocation:
// 6 780 -> 6 871 instructions, measured with a copy of the kernel that differed in nothing but the template argument)
#ifdef KL_WINDOWS_UNIT
constexpr bool KL_WIN = true;
#else
constexpr bool KL_WIN = false;
#endif
template <bool WIN>
__global__ __launch_bounds__(KL_THREADS) void kr_large_solve_kernel(const wdg_kr_job *__restrict__ jobs, int n_jobs, float *scratch_all) {
    __shared__ float RP[KL_CH * 32 * K2_PS];           // a part of the row panel L(kb, j0 .. j0 + 7), row-major, stride 36
    __shared__ float LD[32 * K2_PS];                   // the diagonal block: A_kk -> M = L_kk^-1 (k2_factor_invert)
    __shared__ float LT[32 * K2_PS];                   // k2_factor_invert's column buffer
    __shared__ float zs[KL_MAX_N * KL_MAX_C];          // right-hand sides -> z = L^-1 Y (block by block) -> v of the back substitution
    __shared__ float al[KL_MAX_N * KL_MAX_C];          // alpha
    __shared__ float part[KL_WAVES][32][KL_MAX_C];     // per-wave partial sums (back substitution)
    __shared__ int tr_idx[KL_MAX_N];                   // the train rows' ids as solved
    __shared__ float sc[KL_MAX_N];                     // sqrt(size) of a solved row's duplicate class (1 without a workspace)
    __shared__ float red[KL_WAVES];
    __shared__ int deficient, hits;

    // (the wave index as a SCALAR: the branches on it are then scalar branches, and what one side holds in registers - the column's
    // accumulators - is not live through the other - the diagonal block's factorisation)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li_ = lane & 31, h_ = lane >> 5;
    const global_ptr<float> S = to_global(scratch_all) + static_cast<size_t>(blockIdx.x) * (KL_BLOCKS * 1024);  // this workgroup's factor
    for (int prob = blockIdx.x; prob < n_jobs; prob += gridDim.x) {
        const desc_ptr<wdg_kr_job> job = (desc_ptr<wdg_kr_job>)(jobs + prob);
        const global_ptr<const float> K = to_global(job->K);
        const global_ptr<const int32_t> train = to_global(job->train), val = to_global(job->val), labels = to_global(job->labels);
        const global_ptr<const int32_t> ws = to_global(static_cast<const int32_t *>(job->ws));
        const int64_t ldk = job->ldk;
        const int nt_in = job->n_train, nv = job->n_val, C = job->n_classes;
        const bool has_ws = job->ws != nullptr;  // (uniform) the pre-pass has run on this job
        const int cb = WIN ? job->class_base : 0;  // (uniform) the window's first class
        bool refuse = nt_in <= 0 || nt_in > KL_MAX_N || C <= 0 || C > (WIN ? KR_ALL_C : KL_MAX_C) || ldk <= 0 || ldk >= 65536 ||
                      (WIN && (cb < 0 || (cb & (KL_MAX_C - 1)) != 0 || cb >= C || (C > KL_MAX_C && job->rows_out == nullptr))) ||
                      (!has_ws && job->rep != nullptr);  // (representatives without a workspace: not solved as if there were none)
        int nt = nt_in;
        if (!refuse && has_ws) {
            nt = ws[KRW_NT];
            refuse = nt < 0 || nt > nt_in;
        }
        if (refuse) {  // (uniform)
            if (tid == 0 && job->correct_out) *to_global(job->correct_out) = -1;
            if (tid == 0 && job->flags_out) *to_global(job->flags_out) = 0;
            continue;
        }
        const krw_offsets W(krw_pad(nt_in));
        const bool deflated = has_ws && ws[KRW_DEFLATED] != 0;
        const bool dropped = has_ws && ws[KRW_DROPPED] != 0;
        const int n_mixed = has_ws ? ws[KRW_MIXED] : 0;
        const int nb = (nt + 31) >> 5;
        for (int i = tid; i < nb * 32; i += KL_THREADS) {
            tr_idx[i] = i < nt ? (has_ws ? ws[KRW_TRAIN + i] : train[i]) : -1;
            sc[i] = (has_ws && i < nt) ? __builtin_bit_cast(float, ws[W.scale + i]) : 1.f;
        }
        if (tid == 0) hits = 0;
        __syncthreads();
        // max K_ii of the solved rows (the scale of the pivot test)
        float dmax = 0.f;
        for (int t = tid; t < nt; t += KL_THREADS) dmax = fmaxf(dmax, K[static_cast<int64_t>(tr_idx[t]) * ldk + tr_idx[t]] * (sc[t] * sc[t]));
        for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o));
        if (lane == 0) red[wave] = dmax;
        __syncthreads();
        dmax = 0.f;
#pragma unroll
        for (int w = 0; w < KL_WAVES; ++w) dmax = fmaxf(dmax, red[w]);
        const float drop_below = static_cast<float>(nt) * 1.1920929e-7f * dmax * (1.f / 64.f);
        float ridge = 0.f;

        for (int attempt = 0; attempt < 2; ++attempt) {
            // ---- right-hand sides
            for (int i = tid; i < nb * 32 * KL_MAX_C; i += KL_THREADS) {
                const int row = i / KL_MAX_C, c = i % KL_MAX_C;
                float v = 0.f;
                if (row < nt) {
                    const int lb = has_ws ? ws[W.lab + row] : labels[tr_idx[row]];
                    v = lb - cb == c ? sc[row] : 0.f;  // (lb -1 / -2: never a column of any window)
                    if (lb == -2 && has_ws)  // (rare) a class of duplicates with different labels: its label counts over sqrt(size)
                        for (int e = 0; e < n_mixed; ++e) {
                            const int w = ws[W.mix + e];
                            if ((w >> 12) == ((row << 4) | (c + cb))) v = static_cast<float>(w & 0xfff) / sc[row];
                        }
                }
                zs[i] = v;
            }
            if (tid == 0) deficient = 0;
            __syncthreads();
            // lane (i, h): A[32 a + i][32 b + jmap(h, r)] = K[tr[32 b + j]][tr[32 a + i]] (K is symmetric: per register a wave-uniform
            // row per lane half, 32 columns)
            auto gather_block = [&](int a, int b, f32x16 &t) {
                int li = li_, h = h_;
                asm volatile("" : "+v"(li), "+v"(h));
                const int gi = tr_idx[32 * a + li];
                const float si = sc[32 * a + li];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = k2_jmap(h, r), gj = tr_idx[32 * b + j];
                    const bool diag = a == b && li == j;
                    float v = (gi >= 0 && gj >= 0) ? K[static_cast<int64_t>(gj) * ldk + gi] : (diag ? 1.f : 0.f);
                    v *= si * sc[32 * b + j];  // (1 for rows without duplicates: exact)
                    if (diag && gi >= 0) v += ridge;
                    t[r] = v;
                }
            };

            // ---- the factorisation, left-looking by block column
            for (int kb = 0; kb < nb; ++kb) {
                int li = li_, h = h_;  // (opaque per iteration: the loop's lane-dependent addresses are not hoisted out of it)
                asm volatile("" : "+v"(li), "+v"(h));
                // this wave's blocks of the column: wave 0 the diagonal block, waves 1 .. 7 the blocks below it round-robin
                int sa[KL_SLOTS];
                f32x16 acc[KL_SLOTS];
#pragma unroll
                for (int s = 0; s < KL_SLOTS; ++s) {
                    const int i = wave == 0 ? (s == 0 ? 0 : nb) : wave + (KL_WAVES - 1) * s;
                    sa[s] = __builtin_amdgcn_readfirstlane(kb + i < nb ? kb + i : -1);
                    if (sa[s] >= 0) gather_block(sa[s], kb, acc[s]);
                    else
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
                }
                for (int j0 = 0; j0 < kb; j0 += KL_CH) {
                    const int cnt = min(KL_CH, kb - j0);
                    for (int e = tid; e < cnt * 256; e += KL_THREADS) {  // L(kb, j0 + c) -> RP[c]
                        const int c = e >> 8, row = (e >> 3) & 31, q = e & 7;
                        const f32x4_t v = *(global_ptr<const f32x4_t>)(S + kl_blk(kb, j0 + c) * 1024 + row * 32 + 4 * q);
                        *reinterpret_cast<float4 *>(&RP[(c * 32 + row) * K2_PS + 4 * q]) = make_float4(v.x, v.y, v.z, v.w);
                    }
                    __syncthreads();
#pragma unroll
                    for (int s = 0; s < KL_SLOTS; ++s) {
                        if (sa[s] < 0) continue;  // (wave-uniform)
                        for (int c = 0; c < cnt; ++c) {
                            const global_ptr<const float> pa = S + kl_blk(sa[s], j0 + c) * 1024 + li * 32 + 4 * h;
                            const float *pb = &RP[(c * 32 + li) * K2_PS + 4 * h];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const f32x4_t va = *(global_ptr<const f32x4_t>)(pa + 8 * q);
                                const float4 vb = *reinterpret_cast<const float4 *>(pb + 8 * q);
                                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.x, va.x, acc[s], 0, 0, 0);
                                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.y, va.y, acc[s], 0, 0, 0);
                                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.z, va.z, acc[s], 0, 0, 0);
                                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(-vb.w, va.w, acc[s], 0, 0, 0);
                            }
                        }
                    }
                    __syncthreads();
                }
                if (wave == 0) {
                    // the diagonal block: factored and inverted in one pass (LD holds M = L_kk^-1 afterwards), M -> its scratch block,
                    // z_kb = M y_kb (the lane halves split k, one cross-half add)
                    k2_store_block(acc[0], LD, li, h);
                    if (k2_factor_invert(LD, LT, li, h, nt - 32 * kb, drop_below, ridge) && lane == 0) deficient = 1;
                    const float *mrow = &LD[li * K2_PS + 4 * h];
                    const global_ptr<float> md = S + kl_blk(kb, kb) * 1024 + li * 32 + 4 * h;
                    float sum[KL_MAX_C];
#pragma unroll
                    for (int c = 0; c < KL_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 m = *reinterpret_cast<const float4 *>(mrow + 8 * q);
                        *(global_ptr<f32x4_t>)(md + 8 * q) = f32x4_t{m.x, m.y, m.z, m.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float *y = &zs[(32 * kb + 8 * q + 4 * h + e) * KL_MAX_C];
                            const float4 y0 = *reinterpret_cast<const float4 *>(y), y1 = *reinterpret_cast<const float4 *>(y + 4);
                            const float l = e == 0 ? m.x : e == 1 ? m.y : e == 2 ? m.z : m.w;
                            sum[0] = fmaf(l, y0.x, sum[0]), sum[1] = fmaf(l, y0.y, sum[1]), sum[2] = fmaf(l, y0.z, sum[2]), sum[3] = fmaf(l, y0.w, sum[3]);
                            sum[4] = fmaf(l, y1.x, sum[4]), sum[5] = fmaf(l, y1.y, sum[5]), sum[6] = fmaf(l, y1.z, sum[6]), sum[7] = fmaf(l, y1.w, sum[7]);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < KL_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                    if (h == 0) {  // (every read of y above precedes these writes: they depend on all of them)
                        *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KL_MAX_C]) = make_float4(sum[0], sum[1], sum[2], sum[3]);
                        *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KL_MAX_C + 4]) = make_float4(sum[4], sum[5], sum[6], sum[7]);
                    }
                } else {
                    // A(a, kb), updated, -> its scratch block: it comes back below as an MFMA operand (row li, the k index in the registers)
#pragma unroll
                    for (int s = 0; s < KL_SLOTS; ++s) {
                        if (sa[s] < 0) continue;
                        const global_ptr<float> pd = S + kl_blk(sa[s], kb) * 1024 + li * 32 + 4 * h;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            *(global_ptr<f32x4_t>)(pd + 8 * q) = f32x4_t{acc[s][4 * q], acc[s][4 * q + 1], acc[s][4 * q + 2], acc[s][4 * q + 3]};
                    }
                }
                __syncthreads();
                if (deficient && attempt == 0) break;  // (uniform) restart on K + ridge I
                // the panel: X L_kk^T = A  <=>  X = A M^T, 16 MFMAs per block; y_a -= X z_kb
                if (wave != 0) {
#pragma unroll 1
                    for (int s = 0; s < KL_SLOTS; ++s) {
                        const int a = sa[s];
                        if (a < 0) continue;
                        f32x16 t;
#pragma unroll
                        for (int r = 0; r < 16; ++r) t[r] = 0.f;
                        const global_ptr<float> pa = S + kl_blk(a, kb) * 1024 + li * 32 + 4 * h;
                        const float *pm = &LD[li * K2_PS + 4 * h];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x4_t va = *(global_ptr<const f32x4_t>)(pa + 8 * q);
                            const float4 vm = *reinterpret_cast<const float4 *>(pm + 8 * q);
                            t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.x, va.x, t, 0, 0, 0);
                            t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.y, va.y, t, 0, 0, 0);
                            t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.z, va.z, t, 0, 0, 0);
                            t = __builtin_amdgcn_mfma_f32_32x32x2f32(vm.w, va.w, t, 0, 0, 0);
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q)  // L(a, kb), final (the stores depend on every load above through the products)
                            *(global_ptr<f32x4_t>)(pa + 8 * q) = f32x4_t{t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]};
                        float sum[KL_MAX_C];
#pragma unroll
                        for (int c = 0; c < KL_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float *z = &zs[(32 * kb + k2_jmap(h, r)) * KL_MAX_C];
                            const float4 z0 = *reinterpret_cast<const float4 *>(z), z1 = *reinterpret_cast<const float4 *>(z + 4);
                            const float l = t[r];
                            sum[0] = fmaf(l, z0.x, sum[0]), sum[1] = fmaf(l, z0.y, sum[1]), sum[2] = fmaf(l, z0.z, sum[2]), sum[3] = fmaf(l, z0.w, sum[3]);
                            sum[4] = fmaf(l, z1.x, sum[4]), sum[5] = fmaf(l, z1.y, sum[5]), sum[6] = fmaf(l, z1.z, sum[6]), sum[7] = fmaf(l, z1.w, sum[7]);
                        }
#pragma unroll
                        for (int c = 0; c < KL_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                        if (h == 0) {
                            float *y = &zs[(32 * a + li) * KL_MAX_C];
#pragma unroll
                            for (int c = 0; c < KL_MAX_C; ++c) y[c] -= sum[c];
                        }
                    }
                }
                __syncthreads();
            }
            __syncthreads();
            if (!deficient || attempt == 1) break;  // (uniform)
            ridge = 8.f * drop_below;                // = n eps max K_ii / 8
            __syncthreads();
        }

        if (nt == 0 && tid < KL_MAX_C) al[tid] = 0.f;  // (every train row dropped: the predictions' masked reads hit row 0)
        // ---- back substitution L^T alpha = z, block column by block column from the last
        for (int kb = nb - 1; kb >= 0; --kb) {
            int li = li_, h = h_;
            asm volatile("" : "+v"(li), "+v"(h));
            {  // lane (j, h) sums L(a, kb)[i][j] alpha_a[i][.] over the 16 rows i of its half, this wave's blocks a ascending
                float sum[KL_MAX_C];
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c) sum[c] = 0.f;
                for (int a = kb + 1 + wave; a < nb; a += KL_WAVES) {
                    const global_ptr<const float> pl = S + kl_blk(a, kb) * 1024 + (16 * h) * 32 + li;
#pragma unroll 4
                    for (int ii = 0; ii < 16; ++ii) {
                        const float l = pl[ii * 32];
                        const float *av = &al[(32 * a + 16 * h + ii) * KL_MAX_C];
                        const float4 a0 = *reinterpret_cast<const float4 *>(av), a1 = *reinterpret_cast<const float4 *>(av + 4);
                        sum[0] = fmaf(l, a0.x, sum[0]), sum[1] = fmaf(l, a0.y, sum[1]), sum[2] = fmaf(l, a0.z, sum[2]), sum[3] = fmaf(l, a0.w, sum[3]);
                        sum[4] = fmaf(l, a1.x, sum[4]), sum[5] = fmaf(l, a1.y, sum[5]), sum[6] = fmaf(l, a1.z, sum[6]), sum[7] = fmaf(l, a1.w, sum[7]);
                    }
                }
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                if (h == 0) {
#pragma unroll
                    for (int c = 0; c < KL_MAX_C; ++c) part[wave][li][c] = sum[c];
                }
            }
            __syncthreads();
            if (wave == 0) {  // alpha_kb = M^T (z_kb - the waves' sums, in wave order)
                float v[KL_MAX_C];
                {
                    const float4 r0 = *reinterpret_cast<const float4 *>(&zs[(32 * kb + li) * KL_MAX_C]), r1 = *reinterpret_cast<const float4 *>(&zs[(32 * kb + li) * KL_MAX_C + 4]);
                    v[0] = r0.x, v[1] = r0.y, v[2] = r0.z, v[3] = r0.w, v[4] = r1.x, v[5] = r1.y, v[6] = r1.z, v[7] = r1.w;
                }
#pragma unroll
                for (int w = 0; w < KL_WAVES; ++w) {
                    const float4 p0 = *reinterpret_cast<const float4 *>(&part[w][li][0]), p1 = *reinterpret_cast<const float4 *>(&part[w][li][4]);
                    v[0] -= p0.x, v[1] -= p0.y, v[2] -= p0.z, v[3] -= p0.w, v[4] -= p1.x, v[5] -= p1.y, v[6] -= p1.z, v[7] -= p1.w;
                }
                // v goes through the block's z slot so that every lane can read every row of it (one wave: its LDS operations are
                // carried out in issue order); alpha_kb[i] = sum_j M[j][i] v[j], the lane halves split j
                if (h == 0) {
                    *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KL_MAX_C]) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4 *>(&zs[(32 * kb + li) * KL_MAX_C + 4]) = make_float4(v[4], v[5], v[6], v[7]);
                }
                const global_ptr<const float> pm = S + kl_blk(kb, kb) * 1024 + (16 * h) * 32 + li;
                float sum[KL_MAX_C];
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c) sum[c] = 0.f;
#pragma unroll 4
                for (int jj = 0; jj < 16; ++jj) {
                    const float m = pm[jj * 32];
                    const float *vj = &zs[(32 * kb + 16 * h + jj) * KL_MAX_C];
                    const float4 v0 = *reinterpret_cast<const float4 *>(vj), v1 = *reinterpret_cast<const float4 *>(vj + 4);
                    sum[0] = fmaf(m, v0.x, sum[0]), sum[1] = fmaf(m, v0.y, sum[1]), sum[2] = fmaf(m, v0.z, sum[2]), sum[3] = fmaf(m, v0.w, sum[3]);
                    sum[4] = fmaf(m, v1.x, sum[4]), sum[5] = fmaf(m, v1.y, sum[5]), sum[6] = fmaf(m, v1.z, sum[6]), sum[7] = fmaf(m, v1.w, sum[7]);
                }
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c) sum[c] += __shfl_xor(sum[c], 32);
                if (h == 0) {
                    const bool real = 32 * kb + li < nt;
                    *reinterpret_cast<float4 *>(&al[(32 * kb + li) * KL_MAX_C]) = real ? make_float4(sum[0], sum[1], sum[2], sum[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4 *>(&al[(32 * kb + li) * KL_MAX_C + 4]) = real ? make_float4(sum[4], sum[5], sum[6], sum[7]) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            __syncthreads();
        }
        // a class's weight as the predictions apply it: sqrt(size) x the scaled system's solution
        if (deflated) {
            for (int i = tid; i < nt * KL_MAX_C; i += KL_THREADS) al[i] *= sc[i / KL_MAX_C];
        }
        __syncthreads();

        // ---- predictions: units of four validation rows dealt to the waves in turn, sixteen lanes per row; the lanes of a row split
        //      the train rows (t = lane + 16 k, k ascending), a row's sum: its lanes' partial sums added by a four-step butterfly
        {
            const global_ptr<const int32_t> pval = has_ws ? ws + W.val : val;
            const int g = lane >> 4, gl = lane & 15;
            for (int unit = wave; 4 * unit < nv; unit += KL_WAVES) {
                const int v = 4 * unit + g, vv = min(v, nv - 1), gv = pval[vv];
                const global_ptr<const float> krow = K + static_cast<int64_t>(gv) * ldk;
                float p[KL_MAX_C];
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c) p[c] = 0.f;
                for (int t0 = 0; t0 < nt; t0 += 16 * 8) {
                    float kv[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int t = t0 + gl + 16 * k;
                        const bool ok = t < nt;
                        kv[k] = ok ? krow[tr_idx[ok ? t : 0]] : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int t = t0 + gl + 16 * k;
                        const int ta = t < nt ? t : 0;  // (kv is 0 there)
                        const float4 a0 = *reinterpret_cast<const float4 *>(&al[ta * KL_MAX_C]), a1 = *reinterpret_cast<const float4 *>(&al[ta * KL_MAX_C + 4]);
                        p[0] = fmaf(kv[k], a0.x, p[0]), p[1] = fmaf(kv[k], a0.y, p[1]), p[2] = fmaf(kv[k], a0.z, p[2]), p[3] = fmaf(kv[k], a0.w, p[3]);
                        p[4] = fmaf(kv[k], a1.x, p[4]), p[5] = fmaf(kv[k], a1.y, p[5]), p[6] = fmaf(kv[k], a1.z, p[6]), p[7] = fmaf(kv[k], a1.w, p[7]);
                    }
                }
#pragma unroll
                for (int c = 0; c < KL_MAX_C; ++c)
                    for (int o = 8; o > 0; o >>= 1) p[c] += __shfl_xor(p[c], o);  // (inside the row's 16 lanes: every lane ends with the sum)
                int best = 0;
                float bv = -3.4e38f;
                const int Cw = WIN ? min(KL_MAX_C, C - cb) : C;  // the columns that hold classes
                for (int c = 0; c < Cw; ++c)
                    if (p[c] > bv) {  // first maximum, like torch.argmax
                        bv = p[c];
                        best = c;
                    }
                if constexpr (WIN) {  // the row's best of this window, for the combine pass
                    const global_ptr<i32x2_t> prow = to_global(reinterpret_cast<i32x2_t *>(job->rows_out));  // (value, class): one 8-byte store
                    best += cb;
                    if (job->rows_out != nullptr && gl == 0 && v < nv) prow[v] = i32x2_t{__builtin_bit_cast(int, bv), best};
                }
                const int want = has_ws ? ws[W.val + nv + vv] : labels[gv];
                const unsigned long long hit = __ballot(gl == 0 && v < nv && best == want);
                if (lane == 0 && hit) atomicAdd(&hits, __popcll(hit));
            }
        }
        __syncthreads();
        if (tid == 0) {
            if (job->correct_out) *to_global(job->correct_out) = hits;
            if (job->flags_out) *to_global(job->flags_out) = (ridge > 0.f ? 1 : 0) | (deflated ? 2 : 0) | (dropped ? 4 : 0);
        }
        __syncthreads();  // (the next problem's setup overwrites tr_idx, sc and hits)
    }
}

}  // namespace

#ifndef KL_WINDOWS_UNIT
extern "C" {

int32_t wdg_kernel_regress_large_max_train(void) { return KL_MAX_N; }

size_t wdg_kr_large_scratch_bytes(void) { return static_cast<size_t>(wdg::device_cus()) * KL_WG_BYTES; }

size_t wdg_kr_large_workspace_bytes(int32_t n_train, int32_t n_val) {
    return krw_bytes(krw_pad(n_train < 0 ? 0 : (n_train > KL_MAX_N ? KL_MAX_N : n_train)), n_val);
}

}  // extern "C"
#endif

namespace {

template <bool WIN>
int kernel_regress_large_launch(const wdg_kr_job *jobs_dev, int32_t n_jobs, void *scratch, size_t scratch_bytes, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0, "kernel_regress_large_batched: negative size");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "kernel_regress_large_batched: null job table");
    WDG_REQUIRE(scratch != nullptr && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "kernel_regress_large_batched: the scratch buffer must be 16-byte aligned");
    // one resident workgroup per CU (its 125 KB of LDS allow no second one) and per 2.1-MiB slice of the scratch buffer
    const size_t slices = scratch_bytes / KL_WG_BYTES;
    WDG_REQUIRE(slices >= 1, "kernel_regress_large_batched: %zu bytes of scratch, one workgroup needs %zu (wdg_kr_large_scratch_bytes)",
                scratch_bytes, KL_WG_BYTES);
    int wgs = wdg::device_cus();
    if (n_jobs < wgs) wgs = n_jobs;
    if (slices < static_cast<size_t>(wgs)) wgs = static_cast<int>(slices);
    const int dwgs = n_jobs < 2 * wdg::device_cus() ? n_jobs : 2 * wdg::device_cus();
    hipLaunchKernelGGL(kr_large_deflate_kernel, dim3(static_cast<unsigned>(dwgs)), dim3(KLD_THREADS), 0, wdg::as_stream(stream), jobs_dev, n_jobs);
    if (const int rc = wdg::check_launch("kr_large_deflate_kernel")) return rc;
    hipLaunchKernelGGL(kr_large_solve_kernel<WIN>, dim3(static_cast<unsigned>(wgs)), dim3(KL_THREADS), 0, wdg::as_stream(stream), jobs_dev, n_jobs,
                       static_cast<float *>(scratch));
    return wdg::check_launch("kr_large_solve_kernel");
}

}  // namespace

extern "C" {

#ifndef KL_WINDOWS_UNIT
int wdg_kernel_regress_large_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, void *scratch, size_t scratch_bytes, wdg_stream_t stream) {
    return kernel_regress_large_launch<KL_WIN>(jobs_dev, n_jobs, scratch, scratch_bytes, stream);
}
#else
int wdg_kernel_regress_large_windows_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, void *scratch, size_t scratch_bytes, wdg_stream_t stream) {
    return kernel_regress_large_launch<KL_WIN>(jobs_dev, n_jobs, scratch, scratch_bytes, stream);
}
#endif

}  // extern "C"
