// Gram / arc-cosine kernels of the kernel-regression metric: the kernels of a whole graph in one MFMA launch
// with the map fused as its epilogue.  The batched solver that reads them is csrc/kernel_reg.hip, the sampler of the epochs'
// node sets csrc/kr_sets.hip.
//
// replaces: gntk_homophily_ (utils/homophily_metrics.py:232-257, utils/homophily_plot.py:238-268).
//
// The reference recomputes, in each of its 100 epochs, the aggregation, the Gram of the sampled rows and its arc-cosine map,
// moves the kernels to the host and pseudo-inverts the train block with LAPACK (>95 % of the sweep's wall time, SURVEY.md
// 3.3).  None of that depends on the epoch except WHICH rows are sampled: the map is elementwise in (G_ij, |h_i| |h_j|), so
// the kernel of a sample is a sub-block of the kernel of all nodes.  Here:
//   * gram_map_kernel   K = map(A A^T) for ALL nodes of a graph, once: the tile loop of gemm_f32_kernel (v_mfma_f32_32x32x2_f32,
//                       the k-ordered fp32 fma chain) with the map as epilogue - linear (G / 2) and / or arc-cosine (arccos_map);
//   * row_norm2_kernel  |h_i|^2 as the same fma chain (= the Gram's diagonal, bit for bit);
//   * gram_split_kernel the default since round 3 (WDG_GRAM_SPLIT=0: the two above): the same Gram with every fp32 product formed
//                       from bf16 pieces of both operands on v_mfma_f32_32x32x16_bf16 (split_bf16.h: no input bit dropped, fp32
//                       accumulation), gram_diag_split_kernel its diagonal by the same instruction sequence;
//   * the propagated route's transpose / half-diagonal / finish passes and the mean edge cosine that reads a Gram (below).
#include <cstdlib>

#include "wdg_common.h"
#include "split_bf16.h"

namespace {

using namespace wdg;

// The arc-cosine map of utils/homophily_metrics.py:236-242, (g (pi - acos(g / nu)) + sqrt(nu^2 - g^2)) / (2 pi) with nu =
// max(|h_i| |h_j|, 1e-8) and NaN -> 0 in both terms: the one epilogue of the direct kernels and of the propagated route's finish pass.
__device__ __forceinline__ float arccos_map(float g, float nu) {
    const float pi = 3.14159265358979323846f;
    nu = nu > 1e-8f ? nu : 1e-8f;
    float ac = acosf(g / nu);
    float sq = sqrtf(nu * nu - g * g);
    ac = ac != ac ? 0.f : ac;
    sq = sq != sq ? 0.f : sq;
    return (1.f / pi) * (g * (pi - ac) + sq) * 0.5f;
}

// ------------------------------------------------------------------------------------------------ row norms
__global__ __launch_bounds__(256) void row_norm2_kernel(const wdg_gram_job *__restrict__ jobs, int max_n) {
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.y);
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= job->n) return;
    const global_ptr<const float> a = to_global(job->A) + static_cast<int64_t>(row) * job->lda;
    float acc = 0.f;
    for (int k = 0; k < job->F; ++k) acc = fmaf(a[k], a[k], acc);  // the k-ordered chain of the MFMA: = G_ii
    to_global(job->norm2)[row] = acc;
}

// ------------------------------------------------------------------------------------------------ Gram + map
#ifndef WDG_GBK
#define WDG_GBK 16
#define WDG_GPAD 1
#endif
constexpr int GBM = 128, GBN = 64, GBK = WDG_GBK, GTHREADS = 256;
constexpr int GLD = GBK + WDG_GPAD, GQ = GBK / 4;  // (GQ: quadruples of k per tile row)

__global__ __launch_bounds__(GTHREADS) void gram_map_kernel(const wdg_gram_job *__restrict__ jobs) {
    __shared__ float As[GBM * GLD];
    __shared__ float Bs[GBN * GLD];
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.z);
    const global_ptr<const float> A = to_global(job->A), norm2 = to_global(job->norm2);
    const global_ptr<float> Klin = to_global(job->K_linear), Karc = to_global(job->K_arccos);
    const int64_t lda = job->lda, ldk = job->ldk;
    const int n = job->n, K = job->F;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * GBM, n0 = blockIdx.y * GBN;
    if (m0 >= n || n0 >= n) return;
    // The Gram and both maps are symmetric, bit for bit (the products of a k-ordered chain commute, and so do the two norms under
    // the map): tiles that lie entirely above the diagonal are not computed - the tile below writes their entries mirrored.
    if (n0 >= m0 + GBM) return;

    // A thread fetches quadruples of consecutive k: one 16-byte load each when the rows allow it (16-byte aligned base, lda a
    // multiple of 4 - every contiguous fp32 matrix with F % 4 == 0), else four scalar loads (the first version loaded scalars
    // only: 12 load instructions per thread and K step with their address arithmetic - ten VALU instructions per MFMA)
    constexpr int A_PER = GBM * GBK / GTHREADS / 4, B_PER = GBN * GBK / GTHREADS / 4;  // quadruples per thread: 2, 1
    const bool vec = (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(job->A) & 15) == 0;
    float4 ra[A_PER], rb[B_PER];
    auto load_quad = [&](int row, int gk) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) {
            const global_ptr<const float> p = A + static_cast<int64_t>(row) * lda + gk;
            if (vec && gk + 3 < K) {
                const f32x4_t q = *(global_ptr<const f32x4_t>)p;
                v = make_float4(q[0], q[1], q[2], q[3]);
            } else {
                if (gk < K) v.x = p[0];
                if (gk + 1 < K) v.y = p[1];
                if (gk + 2 < K) v.z = p[2];
                if (gk + 3 < K) v.w = p[3];
            }
        }
        return v;
    };
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * GTHREADS;  // quadruple e: row e / GQ of the tile, k = 4 (e % GQ)
            ra[i] = load_quad(m0 + e / GQ, k0 + 4 * (e % GQ));
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int e = tid + i * GTHREADS;
            rb[i] = load_quad(n0 + e / GQ, k0 + 4 * (e % GQ));
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * GTHREADS;
            float *d = &As[(e / GQ) * GLD + 4 * (e % GQ)];
            d[0] = ra[i].x, d[1] = ra[i].y, d[2] = ra[i].z, d[3] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int e = tid + i * GTHREADS;
            float *d = &Bs[(e / GQ) * GLD + 4 * (e % GQ)];
            d[0] = rb[i].x, d[1] = rb[i].y, d[2] = rb[i].z, d[3] = rb[i].w;
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int li = lane & 31, lk = lane >> 5;
    load_tiles(0);
    for (int k0 = 0; k0 < K; k0 += GBK) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (k0 + GBK < K) load_tiles(k0 + GBK);
#pragma unroll
        for (int kk = 0; kk < GBK; kk += 2) {
            const float a = As[(wave * 32 + li) * GLD + kk + lk];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float b = Bs[(t * 32 + li) * GLD + kk + lk];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: C/D map of a 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int row0 = m0 + wave * 32;

#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int gn = n0 + t * 32 + li;
        if (gn >= n) continue;
        const float dn = Karc ? sqrtf(norm2[gn]) : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gm = row0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (gm >= n) continue;
            const float g = acc[t][r];
            // (gn, gm) lies in a tile that was skipped: rows 128 floor(gn / 128) .., columns 64 floor(gm / 64) ..
            const bool mirror = (gm / GBN) * GBN >= (gn / GBM) * GBM + GBM;
            if (Klin) {
                Klin[static_cast<int64_t>(gm) * ldk + gn] = g * 0.5f;
                if (mirror) Klin[static_cast<int64_t>(gn) * ldk + gm] = g * 0.5f;
            }
            if (Karc) {
                const float kv = arccos_map(g, sqrtf(norm2[gm]) * dn);
                Karc[static_cast<int64_t>(gm) * ldk + gn] = kv;
                if (mirror) Karc[static_cast<int64_t>(gn) * ldk + gm] = kv;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ Gram + map, split operands
// The same Gram with every fp32 product formed from bf16 pieces on v_mfma_f32_32x32x16_bf16 (split_bf16.h: three pieces per operand,
// six piece products per 16 k, fp32 accumulation - no input bit dropped, closer to fp64 than the k-ordered chain).  The pieces are
// made ONCE per tile element on the way into LDS and read back as whole MFMA fragments (one ds_read_b128 = 8 k of a row): against
// the fp32 tile loop above that is a sixteenth of the operand reads and of the matrix instructions per k, which is what that loop
// spends its time issuing (ten vector instructions per MFMA).  Same 128 x 64 tiles, same C/D map, same epilogue.
//   * LDS: [piece][row][32 k as bf16 + 8 pad] - rows 80 bytes apart, so the 16 lanes a ds_read_b128 serves together start in 16
//     different bank quadruples (5 i mod 16 is a bijection).
//   * Symmetry: the order of the six piece products is not symmetric in the two operands, so (i, j) and (j, i) computed apart could
//     differ in the last bit: only entries on or below the diagonal are kept, every entry above it is written as the mirror of one
//     below (the fp32 kernel mirrors whole skipped tiles only).  Every (i >= j) lies in a computed tile.
//   * The arc-cosine map wants |h_i|^2 = G_ii with the bits of the Gram's own diagonal: gram_diag_split_kernel runs the SAME
//     instruction sequence on each 32-row block against itself and stores the diagonal (an output element of an MFMA depends on
//     its row of A, its column of B and its accumulator only).
#ifndef WDG_SGBK
#define WDG_SGBK 16  // (16-k steps: 28 KB of LDS per workgroup, four workgroups per CU - 2.13 ms for a shard's 55 Grams; 32-k steps, three per CU: 2.20)
#endif
constexpr int SGBK = WDG_SGBK, SG_QPR = SGBK / 4, SG_HALVES = SGBK / 16;  // k per step; quadruples per tile row; MFMAs (16 k) per step
constexpr int SG_ROW_WORDS = SGBK / 2 + 4;  // 32-bit words per LDS row: the data + 16 bytes of padding (20 / 12 words: rows 5 / 3
                                            // sixteen-byte units apart, odd - the 16 lanes of a ds_read_b128 start in 16 bank quadruples)
#ifndef WDG_SGBN
#define WDG_SGBN 64
#endif
constexpr int SGBM = 128, SGBN = WDG_SGBN, SG_NT = SGBN / 32;  // workgroup tile (a wave: 32 rows x SGBN columns).  128 x 128 tiles
                                                                // (a third fewer row re-reads, two workgroups per CU instead of
                                                                // three) measured 2.29 ms against 2.15 for a shard's 55 Grams
constexpr int SG_A_WORDS = SGBM * SG_ROW_WORDS, SG_B_WORDS = SGBN * SG_ROW_WORDS;

// four consecutive k of one row -> three pieces, 8 bytes each at [piece][row][k]
__device__ __forceinline__ void sg_store_quad(unsigned *base, int piece_words, int row, int kq, const float4 &v) {
    unsigned h[2], m[2], l[2];
    split_pair(v.x, v.y, h[0], m[0], l[0]);
    split_pair(v.z, v.w, h[1], m[1], l[1]);
    u32x2_t *d = reinterpret_cast<u32x2_t *>(base + row * SG_ROW_WORDS + 2 * kq);
    d[0] = u32x2_t{h[0], h[1]};
    d[piece_words / 2] = u32x2_t{m[0], m[1]};
    d[piece_words] = u32x2_t{l[0], l[1]};
}

// the six piece products of one 16-k half step, in the order split_bf16.h names (A piece, B piece)
__device__ __forceinline__ f32x16 sg_products(const u32x4_t &ah, const u32x4_t &am, const u32x4_t &al, const u32x4_t &bh,
                                              const u32x4_t &bm, const u32x4_t &bl, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(al), as_frag(bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(am), as_frag(bm), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(am), as_frag(bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ah), as_frag(bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ah), as_frag(bm), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ah), as_frag(bh), acc, 0, 0, 0);
    return acc;
}

// a tile row's quadruple of k (zero past the matrix); vec: 16-byte aligned rows
// (ags: floats between consecutive 16-column groups of a row - 16 for a row-major A, wdg_gram_job.a_group_stride for a tiled one;
// gk is a multiple of 4: the quadruple lies inside one group)
__device__ __forceinline__ float4 sg_load_quad(global_ptr<const float> A, int64_t lda, int64_t ags, int n, int K, bool vec, int row, int gk) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n) {
        const global_ptr<const float> p = A + static_cast<int64_t>(row) * lda + static_cast<int64_t>(gk >> 4) * ags + (gk & 15);
        if (vec && gk + 3 < K) {
            const f32x4_t q = *(global_ptr<const f32x4_t>)p;
            v = make_float4(q[0], q[1], q[2], q[3]);
        } else {
            if (gk < K) v.x = p[0];
            if (gk + 1 < K) v.y = p[1];
            if (gk + 2 < K) v.z = p[2];
            if (gk + 3 < K) v.w = p[3];
        }
    }
    return v;
}

__global__ __launch_bounds__(GTHREADS) void gram_diag_split_kernel(const wdg_gram_job *__restrict__ jobs) {
    __shared__ unsigned As[3 * SG_A_WORDS];
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.y);
    const global_ptr<const float> A = to_global(job->A);
    const int64_t lda = job->lda;
    const int n = job->n, K = job->F;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lk = lane >> 5;
    const int m0 = blockIdx.x * SGBM;
    if (m0 >= n) return;
    const int64_t ags = job->a_group_stride > 0 ? job->a_group_stride : 16;
    const bool vec = (lda & 3) == 0 && (ags & 3) == 0 && (reinterpret_cast<uintptr_t>(job->A) & 15) == 0;
    constexpr int A_PER = SGBM * SGBK / GTHREADS / 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += SGBK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * GTHREADS;
            sg_store_quad(As, SG_A_WORDS, e / SG_QPR, e % SG_QPR, sg_load_quad(A, lda, ags, n, K, vec, m0 + e / SG_QPR, k0 + 4 * (e % SG_QPR)));
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < SG_HALVES; ++m) {
            const u32x4_t *ap = reinterpret_cast<const u32x4_t *>(As) + (wave * 32 + li) * (SG_ROW_WORDS / 4) + 2 * m + lk;
            const u32x4_t ah = ap[0], am = ap[SG_A_WORDS / 4], al = ap[2 * (SG_A_WORDS / 4)];
            acc = sg_products(ah, am, al, ah, am, al, acc);
        }
    }
    // element (li, li) of the block: register (li >> 3) * 4 + (li & 3) of the lane whose half lk = (li >> 2) & 1
    float d = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) d = (r == (li >> 3) * 4 + (li & 3)) ? acc[r] : d;
    const int row = m0 + wave * 32 + li;
    if (lk == ((li >> 2) & 1) && row < n) to_global(job->norm2)[row] = d;
}

__global__ __launch_bounds__(GTHREADS) void gram_split_kernel(const wdg_gram_job *__restrict__ jobs) {
    __shared__ unsigned As[3 * SG_A_WORDS];
    __shared__ unsigned Bs[3 * SG_B_WORDS];
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.z);
    const global_ptr<const float> A = to_global(job->A), norm2 = to_global(job->norm2);
    const global_ptr<float> Klin = to_global(job->K_linear), Karc = to_global(job->K_arccos);
    const int64_t lda = job->lda, ldk = job->ldk;
    const int n = job->n, K = job->F;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * SGBM, n0 = blockIdx.y * SGBN;
    if (m0 >= n || n0 >= n) return;
    if (n0 >= m0 + SGBM) return;  // entirely above the diagonal: written mirrored by the tile below
    constexpr int A_PER = SGBM * SGBK / GTHREADS / 4, B_PER = SGBN * SGBK / GTHREADS / 4;  // quadruples per thread: 4, 2 (SGBN = 64)
    const int64_t ags = job->a_group_stride > 0 ? job->a_group_stride : 16;
    const bool vec = (lda & 3) == 0 && (ags & 3) == 0 && (reinterpret_cast<uintptr_t>(job->A) & 15) == 0;
    float4 ra[A_PER], rb[B_PER];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int e = tid + i * GTHREADS;  // quadruple e: row e / SG_QPR of the tile, k = 4 (e % SG_QPR)
            ra[i] = sg_load_quad(A, lda, ags, n, K, vec, m0 + e / SG_QPR, k0 + 4 * (e % SG_QPR));
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int e = tid + i * GTHREADS;
            rb[i] = sg_load_quad(A, lda, ags, n, K, vec, n0 + e / SG_QPR, k0 + 4 * (e % SG_QPR));
        }
    };
    f32x16 acc[SG_NT];
#pragma unroll
    for (int t = 0; t < SG_NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int li = lane & 31, lk = lane >> 5;
    load_tiles(0);
    for (int k0 = 0; k0 < K; k0 += SGBK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < A_PER; ++i) sg_store_quad(As, SG_A_WORDS, (tid + i * GTHREADS) / SG_QPR, (tid + i * GTHREADS) % SG_QPR, ra[i]);
#pragma unroll
        for (int i = 0; i < B_PER; ++i) sg_store_quad(Bs, SG_B_WORDS, (tid + i * GTHREADS) / SG_QPR, (tid + i * GTHREADS) % SG_QPR, rb[i]);
        __syncthreads();
        if (k0 + SGBK < K) load_tiles(k0 + SGBK);
#pragma unroll
        for (int m = 0; m < SG_HALVES; ++m) {
            const u32x4_t *ap = reinterpret_cast<const u32x4_t *>(As) + (wave * 32 + li) * (SG_ROW_WORDS / 4) + 2 * m + lk;
            const u32x4_t ah = ap[0], am = ap[SG_A_WORDS / 4], al = ap[2 * (SG_A_WORDS / 4)];
#pragma unroll
            for (int t = 0; t < SG_NT; ++t) {
                const u32x4_t *bp = reinterpret_cast<const u32x4_t *>(Bs) + (t * 32 + li) * (SG_ROW_WORDS / 4) + 2 * m + lk;
                const u32x4_t bh = bp[0], bm = bp[SG_B_WORDS / 4], bl = bp[2 * (SG_B_WORDS / 4)];
                acc[t] = sg_products(ah, am, al, bh, bm, bl, acc[t]);
            }
        }
    }
    // ---- epilogue: C/D map of a 32x32 tile: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Entries on or below the
    // diagonal are stored from the accumulators' layout (a register's 32 lanes = 128 contiguous bytes of a row); their mirrors go
    // through a wave-private 32 x 33 LDS tile so that they, too, leave as 128-byte row segments (stored straight from the registers
    // a mirror instruction writes 4 bytes into each of 64 different lines: 0.5 ms of the 2.2 for the two outputs of a sweep shard)
    const int row0 = m0 + wave * 32;
    __syncthreads();  // every wave is done with the operand tiles: their LDS is the transpose buffers now
    float *const T = reinterpret_cast<float *>(As) + wave * (32 * 33);
    static_assert(4 * 32 * 33 <= 3 * SG_A_WORDS, "transpose buffers fit the A tiles");
#pragma unroll
    for (int t = 0; t < SG_NT; ++t) {
        const int gn = n0 + t * 32 + li;
        const float dn = (Karc && gn < n) ? sqrtf(norm2[gn]) : 0.f;
        if (n0 + t * 32 >= n || n0 + t * 32 > row0 + 31) continue;  // (uniform: no column of the block exists / all of it above the diagonal)
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const global_ptr<float> Kout = which ? Karc : Klin;
            if (!Kout) continue;
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = row0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                const float g = acc[t][r];
                float kv = g * 0.5f;
                if (which) kv = arccos_map(g, sqrtf(norm2[gm < n ? gm : n - 1]) * dn);
                v[r] = kv;
                if (gm < n && gn < n && gm >= gn) Kout[static_cast<int64_t>(gm) * ldk + gn] = kv;
                T[((r & 3) + 8 * (r >> 2) + 4 * lk) * 33 + li] = kv;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = 2 * j + lk;  // column c of the block = row n0 + 32 t + c of the mirror, this lane its column row0 + li
                const float kv = T[li * 33 + c];
                const int mn = n0 + t * 32 + c, mm = row0 + li;
                if (mm < n && mn < n && mm > mn) Kout[static_cast<int64_t>(mn) * ldk + mm] = kv;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (the next output overwrites the tile)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

// ------------------------------------------------------------------------------------------------ the Gram of aggregated features, propagated
// Round 5.  The kernels of the AGGREGATED features are those of Y = A_hat X, and Y Y^T = A_hat (X X^T) A_hat^T: two aggregations
// with n "features" over the Gram of the raw features - which the metric computes anyway, once per feature matrix - instead of a
// dense n x n x F product per graph: 2 nnz n flops each against n^2 F.  For the reference's feature bases (F = 932 .. 3 703, n =
// 2 000, 12 .. 67 entries per row) that is 4 .. 18 x less work, none of it on the matrix pipe's critical path, and the wide
// aggregation Y itself is no longer needed by the metric.  The propagation runs on the quad-row aggregation kernel
// (T = A_hat K_X, U = A_hat T^T, csrc/spmm_quad.hip); this file supplies the two small passes around it: the transpose between the two products and
// the FINISH pass - the lower triangle of U is the half Gram K_linear = G / 2 of the aggregated features; it is mirrored (a
// floating-point A_hat T^T is symmetric only to rounding) and mapped exactly as the direct kernels' epilogue maps their G.
// gram_half_diag_kernel: norm2[i] = 2 U[i][i] = G_ii, so that the arc-cosine of a row with itself is exactly 1 here too.
__global__ __launch_bounds__(256) void transpose_batched_kernel(const wdg_transpose_job *__restrict__ jobs) {
    __shared__ float tile[32][33];
    const desc_ptr<wdg_transpose_job> job = (desc_ptr<wdg_transpose_job>)(jobs + blockIdx.z);
    const int rows = job->rows, cols = job->cols;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    if (r0 >= rows || c0 >= cols) return;
    const global_ptr<const float> src = to_global(job->src);
    const global_ptr<float> dst = to_global(job->dst);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int r = r0 + ty + 8 * m, c = c0 + tx;
        tile[ty + 8 * m][tx] = (r < rows && c < cols) ? src[static_cast<int64_t>(r) * job->ld_src + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = c0 + ty + 8 * m, r = r0 + tx;  // dst[c][r] = src[r][c]
        if (c < cols && r < rows) dst[static_cast<int64_t>(c) * job->ld_dst + r] = tile[tx][ty + 8 * m];
    }
}

__global__ __launch_bounds__(256) void gram_half_diag_kernel(const wdg_gram_job *__restrict__ jobs) {
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.y);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= job->n) return;
    to_global(job->norm2)[i] = 2.f * to_global(job->A)[static_cast<int64_t>(i) * job->lda + i];
}

__global__ __launch_bounds__(256) void gram_finish_kernel(const wdg_gram_job *__restrict__ jobs) {
    __shared__ float t_lin[32][33], t_arc[32][33];
    const desc_ptr<wdg_gram_job> job = (desc_ptr<wdg_gram_job>)(jobs + blockIdx.z);
    const int n = job->n;
    const int ti = blockIdx.y, tj = blockIdx.x;  // tile (ti, tj) of the lower triangle: rows 32 ti .., columns 32 tj ..
    if (tj > ti || 32 * ti >= n) return;
    const global_ptr<const float> H = to_global(job->A), norm2 = to_global(job->norm2);
    const global_ptr<float> Klin = to_global(job->K_linear), Karc = to_global(job->K_arccos);
    const int64_t lda = job->lda, ldk = job->ldk;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j = 32 * tj + tx;
    const float dn = (Karc && j < n) ? sqrtf(norm2[j]) : 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int i = 32 * ti + ty + 8 * m;
        float k = 0.f, kv = 0.f;
        if (i < n && j < n) {
            k = H[static_cast<int64_t>(max(i, j)) * lda + min(i, j)];  // (the lower triangle is the authority; only a diagonal tile has i < j)
            const float g = k + k;
            if (Klin) Klin[static_cast<int64_t>(i) * ldk + j] = k;
            if (Karc) {  // (the same function as the direct kernels' epilogue)
                kv = arccos_map(g, sqrtf(norm2[i]) * dn);
                Karc[static_cast<int64_t>(i) * ldk + j] = kv;
            }
        }
        t_lin[ty + 8 * m][tx] = k;
        t_arc[ty + 8 * m][tx] = kv;
    }
    if (ti == tj) return;  // (workgroup-uniform) a diagonal tile wrote both of its halves itself
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {  // the mirror image: entry (32 tj + ty + 8 m, 32 ti + tx) = entry (32 ti + tx, 32 tj + ty + 8 m)
        const int r = 32 * tj + ty + 8 * m, c = 32 * ti + tx;
        if (r < n && c < n) {
            if (Klin) Klin[static_cast<int64_t>(r) * ldk + c] = t_lin[tx][ty + 8 * m];
            if (Karc) Karc[static_cast<int64_t>(r) * ldk + c] = t_arc[tx][ty + 8 * m];
        }
    }
}

// ------------------------------------------------------------------------------------------------ mean edge cosine from a Gram
// generalized edge homophily (utils/homophily_plot.py:56-66, utils/homophily_metrics.py:164-187) when the features' Gram is at
// hand anyway (the kernel-regression metric computes K_linear = X X^T / 2 per feature matrix): cos(x_u, x_v) =
// G_uv / (|x_u| |x_v|) gathered per stored non-loop entry - no N x N cosine matrix, no per-edge dot products.
// Fixed summation order: a wave's shuffle tree per row, then rows in index order per thread and an LDS tree per graph.
__global__ __launch_bounds__(256) void edge_gram_rows_kernel(const wdg_edge_gram_job *__restrict__ jobs, int max_rows,
                                                             float *__restrict__ row_sum, int32_t *__restrict__ row_cnt) {
    const desc_ptr<wdg_edge_gram_job> job = (desc_ptr<wdg_edge_gram_job>)(jobs + blockIdx.y);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= job->n_rows) return;  // (whole waves)
    const global_ptr<const int32_t> rowptr = to_global(job->rowptr), col = to_global(job->col);
    const global_ptr<const float> K = to_global(job->K_linear), n2 = to_global(job->norm2);
    const int s = rowptr[row], e = rowptr[row + 1];
    const float nu = sqrtf(n2[row]);
    float acc = 0.f;
    int cnt = 0;
    for (int p = s + lane; p < e; p += 64) {
        const int c = col[p];
        if (c == row) continue;
        const float den = nu * sqrtf(n2[c]);
        float v = 2.f * K[static_cast<int64_t>(row) * job->ldk + c] / den;
        v = (v != v || den == 0.f) ? 0.f : v;  // NaN -> 0 (a zero feature row)
        acc += v;
        ++cnt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o);
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) {
        row_sum[static_cast<int64_t>(blockIdx.y) * max_rows + row] = acc;
        row_cnt[static_cast<int64_t>(blockIdx.y) * max_rows + row] = cnt;
    }
}
__global__ __launch_bounds__(256) void edge_gram_reduce_kernel(const wdg_edge_gram_job *__restrict__ jobs, int max_rows,
                                                               const float *__restrict__ row_sum,
                                                               const int32_t *__restrict__ row_cnt) {
    __shared__ double ssum[256];
    __shared__ long long scnt[256];
    const desc_ptr<wdg_edge_gram_job> job = (desc_ptr<wdg_edge_gram_job>)(jobs + blockIdx.x);
    double a = 0.0;
    long long c = 0;
    for (int r = threadIdx.x; r < job->n_rows; r += 256) {
        a += static_cast<double>(row_sum[static_cast<int64_t>(blockIdx.x) * max_rows + r]);
        c += row_cnt[static_cast<int64_t>(blockIdx.x) * max_rows + r];
    }
    ssum[threadIdx.x] = a;
    scnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            ssum[threadIdx.x] += ssum[threadIdx.x + o];
            scnt[threadIdx.x] += scnt[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *to_global(job->mean_out) = scnt[0] > 0 ? ssum[0] / static_cast<double>(scnt[0]) : 0.0;
}

}  // namespace

extern "C" {

int wdg_gram_map_batched_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, wdg_stream_t stream) {
    return wdg_gram_map_batched_flags_f32(jobs_dev, n_jobs, max_n, 0u, stream);
}

int wdg_gram_map_batched_flags_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, uint32_t flags, wdg_stream_t stream) {
    WDG_REQUIRE((flags & ~(WDG_KERNEL_SPLIT | WDG_KERNEL_CHAIN | WDG_OPERAND_TILED)) == 0 &&
                    (flags & (WDG_KERNEL_SPLIT | WDG_KERNEL_CHAIN)) != (WDG_KERNEL_SPLIT | WDG_KERNEL_CHAIN), "gram_map_batched: bad flags");
    WDG_REQUIRE(n_jobs >= 0 && max_n >= 0, "gram_map_batched: negative size");
    if (n_jobs == 0 || max_n == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "gram_map_batched: null job table");
    hipStream_t st = wdg::as_stream(stream);
    // split bf16 operands (gram_split_kernel) unless the caller names the kernel or, with neither flag, WDG_GRAM_SPLIT=0 asks for
    // the k-ordered fp32 chain (gram_map_kernel, row_norm2_kernel: row-major A only)
    bool split = (flags & WDG_KERNEL_CHAIN) == 0;
    if (!(flags & (WDG_KERNEL_SPLIT | WDG_KERNEL_CHAIN)))
        if (const char *e = getenv("WDG_GRAM_SPLIT")) split = atoi(e) != 0;
    if (!split && (flags & WDG_OPERAND_TILED))
        return wdg::fail(WDG_ERR_UNSUPPORTED, "gram_map_batched: the fp32-chain kernels read row-major A only (the table holds a tiled A)");
    if (split) {
        hipLaunchKernelGGL(gram_diag_split_kernel, dim3(wdg::ceil_div(max_n, SGBM), n_jobs), dim3(GTHREADS), 0, st, jobs_dev);
        hipLaunchKernelGGL(gram_split_kernel, dim3(wdg::ceil_div(max_n, SGBM), wdg::ceil_div(max_n, SGBN), n_jobs), dim3(GTHREADS), 0, st,
                           jobs_dev);
        return wdg::check_launch("gram_split_kernel");
    }
    hipLaunchKernelGGL(row_norm2_kernel, dim3(wdg::ceil_div(max_n, 256), n_jobs), dim3(256), 0, st, jobs_dev, max_n);
    hipLaunchKernelGGL(gram_map_kernel, dim3(wdg::ceil_div(max_n, GBM), wdg::ceil_div(max_n, GBN), n_jobs), dim3(GTHREADS), 0, st,
                       jobs_dev);
    return wdg::check_launch("gram_map_kernel");
}

int wdg_transpose_batched_f32(const wdg_transpose_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "transpose_batched: negative size");
    if (n_jobs == 0 || max_rows == 0 || max_cols == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "transpose_batched: null job table");
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(wdg::ceil_div(max_cols, 32), wdg::ceil_div(max_rows, 32), n_jobs), dim3(256), 0,
                       wdg::as_stream(stream), jobs_dev);
    return wdg::check_launch("transpose_batched_kernel");
}

int wdg_gram_finish_batched_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_n >= 0, "gram_finish_batched: negative size");
    if (n_jobs == 0 || max_n == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "gram_finish_batched: null job table");
    hipStream_t st = wdg::as_stream(stream);
    hipLaunchKernelGGL(gram_half_diag_kernel, dim3(wdg::ceil_div(max_n, 256), n_jobs), dim3(256), 0, st, jobs_dev);
    const unsigned tiles = static_cast<unsigned>(wdg::ceil_div(max_n, 32));
    hipLaunchKernelGGL(gram_finish_kernel, dim3(tiles, tiles, n_jobs), dim3(256), 0, st, jobs_dev);
    return wdg::check_launch("gram_finish_kernel");
}

size_t wdg_edge_gram_workspace_bytes(int32_t n_jobs, int32_t max_rows) {
    return static_cast<size_t>(n_jobs > 0 ? n_jobs : 0) * static_cast<size_t>(max_rows > 0 ? max_rows : 0) * 8 + 512;
}

int wdg_edge_gram_mean_batched_f32(const wdg_edge_gram_job *jobs_dev, int32_t n_jobs, int32_t max_rows, void *workspace,
                                   size_t workspace_bytes, wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0, "edge_gram_mean_batched: negative size");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev != nullptr, "edge_gram_mean_batched: null job table");
    if (!workspace || workspace_bytes < wdg_edge_gram_workspace_bytes(n_jobs, max_rows))
        return wdg::fail(WDG_ERR_WORKSPACE, "edge_gram_mean_batched: workspace too small");
    hipStream_t st = wdg::as_stream(stream);
    char *ws = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
    float *row_sum = reinterpret_cast<float *>(ws);
    int32_t *row_cnt = reinterpret_cast<int32_t *>(ws + static_cast<size_t>(n_jobs) * max_rows * 4);
    if (max_rows > 0)
        hipLaunchKernelGGL(edge_gram_rows_kernel, dim3(wdg::ceil_div(max_rows, 4), n_jobs), dim3(256), 0, st, jobs_dev, max_rows,
                           row_sum, row_cnt);
    hipLaunchKernelGGL(edge_gram_reduce_kernel, dim3(n_jobs), dim3(256), 0, st, jobs_dev, max_rows, row_sum, row_cnt);
    return wdg::check_launch("edge_gram_mean");
}

}  // extern "C"
