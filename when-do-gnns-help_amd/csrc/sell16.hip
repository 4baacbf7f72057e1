// CSR -> SELL-16: the build of the index layout that the quad-row aggregation kernel reads (csrc/spmm_quad.hip; the layout's
// contract is csrc/sell16.h; DESIGN.md 4.9 "graph build").  Rows sorted by length into slices of 16, per (column block, slice) the
// width and its index chunks, the entries the kernel's waves work through (split / ghost entries), and the fill of the pre-scaled
// column offsets in one of three orders (WDG_SELL_ORDER: column order, the greedy bank-aware order, the conflict-free orders) -
// for one graph (wdg_csr_to_sell16_count / _fill) or a table of graphs (the _batched twins: the same bodies, blockIdx.y = graph).
#include <algorithm>
#include <cstdlib>

#include "sell16.h"

namespace {

using namespace wdg;

// ------------------------------------------------------------------------------------------------ CSR -> SELL-16
__device__ __forceinline__ int q_lower_bound(const int32_t *col, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the row sort (Q_SORT_MAX_ROWS, sell16.h): one workgroup, keys in LDS
__device__ __forceinline__ void sell16_sort_rows_body(const int32_t *__restrict__ rowptr, int32_t N, int32_t *__restrict__ perm,
                                                      unsigned long long *q_keys) {
    const int padded = (N + Q_ROWS - 1) / Q_ROWS * Q_ROWS;
    if (N > Q_SORT_MAX_ROWS) {
        for (int i = threadIdx.x; i < padded; i += 1024) perm[i] = min(i, N - 1);
        return;
    }
    for (int i = threadIdx.x; i < N; i += 1024)
        q_keys[i] = (static_cast<unsigned long long>(0x7fffffffu - static_cast<unsigned>(rowptr[i + 1] - rowptr[i])) << 32) |
                    static_cast<unsigned>(i);
    __syncthreads();
    int P = 1;
    while (P < N) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {  // comparator network, all ascending, virtual +inf padding (any N)
        for (int i = threadIdx.x; i < N; i += 1024) {
            const int l = i ^ (k - 1);
            if (l > i && l < N && q_keys[i] > q_keys[l]) {
                const unsigned long long t = q_keys[i];
                q_keys[i] = q_keys[l];
                q_keys[l] = t;
            }
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += 1024) {
                const int l = i ^ j;
                if (l > i && l < N && q_keys[i] > q_keys[l]) {
                    const unsigned long long t = q_keys[i];
                    q_keys[i] = q_keys[l];
                    q_keys[l] = t;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < N; i += 1024) perm[i] = static_cast<int32_t>(q_keys[i] & 0xffffffffull);
    __syncthreads();
    // the slots that pad the last slice repeat the last (shortest) row: they compute and store that row's sums again (same
    // bits to the same address), so the kernel's stores need no "is this slot a row" predicate
    if (N > 0)
        for (int i = N + threadIdx.x; i < padded; i += 1024) perm[i] = static_cast<int32_t>(q_keys[N - 1] & 0xffffffffull);
}
__global__ __launch_bounds__(1024) void sell16_sort_rows(const int32_t *__restrict__ rowptr, int32_t N,
                                                         int32_t *__restrict__ perm) {
    extern __shared__ unsigned long long q_keys[];
    sell16_sort_rows_body(rowptr, N, perm, q_keys);
}

// one thread per (column block, REAL slice): width = longest in-block row segment, chunks = ceil(width / 16)
__device__ __forceinline__ void sell16_widths_body(int task, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const int32_t *__restrict__ perm, int32_t N, int32_t n_slices,
                                                   int32_t n_blocks, int32_t block_cols, int32_t *__restrict__ chunks,
                                                   int32_t *__restrict__ widths) {
    if (task >= n_slices * n_blocks) return;
    const int blk = task / n_slices, slice = task % n_slices;
    int width = 0;
    for (int r = 0; r < Q_ROWS; ++r) {
        const int slot = slice * Q_ROWS + r;
        if (slot >= N) break;  // (padding slots repeat row perm[N - 1], which is in this slice)
        const int row = perm[slot];
        const int s = rowptr[row], e = rowptr[row + 1];
        const int a = n_blocks == 1 ? s : q_lower_bound(col, s, e, blk * block_cols);
        const int b = (blk + 1 == n_blocks) ? e : q_lower_bound(col, a, e, (blk + 1) * block_cols);
        width = max(width, b - a);
    }
    chunks[task] = (width + Q_CHUNK - 1) / Q_CHUNK;
    widths[task] = width;
}
__global__ __launch_bounds__(256) void sell16_widths(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const int32_t *__restrict__ perm, int32_t N, int32_t n_slices,
                                                     int32_t n_blocks, int32_t block_cols, int32_t *__restrict__ chunks,
                                                     int32_t *__restrict__ widths) {
    sell16_widths_body(blockIdx.x * 256 + threadIdx.x, rowptr, col, perm, N, n_slices, n_blocks, block_cols, chunks, widths);
}

// the entries (sell16.h) of a graph; one thread: the walk is sequential and a graph has a few hundred slices
__device__ __forceinline__ void sell16_pack_body(const int32_t *__restrict__ widths, int32_t n_slices, int32_t n_blocks,
                                                 int32_t *__restrict__ entry_slice, int32_t *__restrict__ entry_k,
                                                 int32_t *__restrict__ info) {
    int wmax = 0;
    for (int i = 0; i < n_slices * n_blocks; ++i) wmax = max(wmax, widths[i]);
    const bool split = n_blocks == 1 && wmax <= Q_SU * Q_SPLIT_WIDTH;
    int cur = 0;
    for (int s = 0; s < n_slices; ++s) {
        const int n = split ? max(1, (widths[s] + Q_SPLIT_WIDTH - 1) / Q_SPLIT_WIDTH) : 1;
        if ((cur & (Q_SU - 1)) + n > Q_SU)
            while (cur & (Q_SU - 1)) {
                entry_slice[cur] = s - 1;
                entry_k[cur++] = -1;
            }
        for (int k = 0; k < n; ++k) {
            entry_slice[cur] = s;
            entry_k[cur++] = k;
        }
    }
    while (cur & (Q_SU - 1)) {
        entry_slice[cur] = n_slices - 1;
        entry_k[cur++] = -1;
    }
    info[0] = cur;            // entries per column block (a multiple of 4)
    info[1] = split ? 1 : 0;  // every entry <= 32 wide: the kernel's pipelined loop applies
}
__global__ void sell16_pack(const int32_t *__restrict__ widths, int32_t n_slices, int32_t n_blocks,
                            int32_t *__restrict__ entry_slice, int32_t *__restrict__ entry_k, int32_t *__restrict__ info) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sell16_pack_body(widths, n_slices, n_blocks, entry_slice, entry_k, info);
}

// q_ext / q_rows from the packed entries; the trailing pair of q_ext = {total chunks, entries per block | split << 30}
__device__ __forceinline__ void sell16_entries_body(int t, const int32_t *__restrict__ widths, const int32_t *__restrict__ chunk_begin,
                                                    const int32_t *__restrict__ entry_slice, const int32_t *__restrict__ entry_k,
                                                    const int32_t *__restrict__ info, const int32_t *__restrict__ perm,
                                                    int32_t n_slices, int32_t n_blocks, int32_t max_entries,
                                                    int32_t *__restrict__ ext, int32_t *__restrict__ rows) {
    const int n_entries = info[0], split = info[1];
    if (t == 0) {  // {chunk count, entries per block | split}: behind the entries, and at the end of the caller's buffer
        ext[2 * n_blocks * n_entries] = ext[2 * n_blocks * max_entries] = chunk_begin[n_slices * n_blocks];
        ext[2 * n_blocks * n_entries + 1] = ext[2 * n_blocks * max_entries + 1] = n_entries | (split ? Q_CONT : 0);
    }
    if (t < n_blocks * n_entries) {
        const int blk = t / n_entries, e = t % n_entries;
        const int s = entry_slice[e], k = entry_k[e];
        const int w = widths[blk * n_slices + s], c0 = chunk_begin[blk * n_slices + s];
        int chunk, width;
        if (k < 0) {  // ghost
            chunk = c0;
            width = Q_CONT;
        } else if (split) {
            chunk = c0 + 2 * k;
            width = min(Q_SPLIT_WIDTH, w - Q_SPLIT_WIDTH * k) | (k > 0 ? Q_CONT : 0);
            if (w == 0) width = 0;
        } else {
            chunk = c0;
            width = w;
        }
        ext[2 * t] = chunk;
        ext[2 * t + 1] = width;
    }
    if (t < n_entries * Q_ROWS) rows[t] = perm[entry_slice[t / Q_ROWS] * Q_ROWS + t % Q_ROWS];
}
__global__ __launch_bounds__(256) void sell16_entries(const int32_t *__restrict__ widths, const int32_t *__restrict__ chunk_begin,
                                                      const int32_t *__restrict__ entry_slice, const int32_t *__restrict__ entry_k,
                                                      const int32_t *__restrict__ info, const int32_t *__restrict__ perm,
                                                      int32_t n_slices, int32_t n_blocks, int32_t max_entries,
                                                      int32_t *__restrict__ ext, int32_t *__restrict__ rows) {
    sell16_entries_body(blockIdx.x * 256 + threadIdx.x, widths, chunk_begin, entry_slice, entry_k, info, perm, n_slices, n_blocks,
                        max_entries, ext, rows);
}

// ---- the CONFLICT-FREE order of a slice (round 4; graphs in split form: one column block, rows of <= 128 entries).
// The sweep reads, per step, one 64-byte slab row per row of the slice, four rows per LDS cycle ({0,3,5,6}, {1,2,4,7}, + 8): a
// cycle is conflict-free when its four source rows lie in four different bank windows (column mod 4).  Round 2's greedy order
// left 1.13 - 1.30 LDS cycles per group and step on the sweep's graphs (measured: SQ_LDS_BANK_CONFLICT = 25 % of the
// conflict-free cycles, on the pipe that bounds the kernel).  Three freedoms remove most of it:
//   * WHICH four rows share a cycle: the 16 rows of a slice are equally long, any of them may sit in any slot.  The rows are
//     dealt to the four groups so that no group holds more than T entries of one window class (T = the steps the slice is swept
//     for): 64 candidate deals (one per lane: a greedy pass over a pseudo-random row order), the best kept.  q_rows is rewritten;
//   * WHEN a row's padding is read: a row shorter than T reads the zero row T - len times - at any step, and from any window:
//     the slab ends in FOUR zero rows, one per class (block_cols is a multiple of 4);
//   * the order inside a group: with every class total <= T a schedule without conflicts exists (the 4 x 4 count matrix plus the
//     free padding decomposes into T permutations); per step the 24 permutations of (row -> class) are scored - feasible, keeps
//     every class total within the steps left, prefers the fullest classes - by 16 lanes per group, the best applied.
// Simulated on the sweep's graphs: 1.04 - 1.06 cycles per group and step.  A row's sum order changes with it (fixed per graph,
// as before); WDG_SELL_ORDER=0 keeps column order.  Slices that hold padding slots (a graph's last, N % 16 != 0) keep the greedy
// order (their duplicate rows must agree entry by entry).
constexpr int QB_MAXW = 128;  // entries per row in split form
struct QbShared {
    int col[Q_ROWS][QB_MAXW];             // the slice's rows, local columns, column order
    unsigned char order[Q_ROWS][QB_MAXW];  // per row: entry ids sorted by class (stable)
    unsigned char pick[Q_ROWS][QB_MAXW];   // per NEW slot and step: class | real << 2
};
__device__ __forceinline__ int qb_field8(unsigned v, int c) { return (v >> (8 * c)) & 0xff; }
__device__ __forceinline__ int qb_group_slot(int g, int i) {  // slot of member i of LDS service group g
    constexpr unsigned long long tbl = 0x6530ull | (0x7421ull << 16) | (0xedb8ull << 32) | (0xfca9ull << 48);
    return static_cast<int>((tbl >> (16 * g + 4 * i)) & 0xf);
}
__device__ __forceinline__ unsigned qb_perm(int id) {  // the id-th permutation of (0,1,2,3), 2 bits per position
    // lexicographic order; position i (bits 2i, 2i+1) = the class member i takes
    constexpr unsigned char tbl[24] = {0xe4, 0xb4, 0xd8, 0x78, 0x9c, 0x6c, 0xe1, 0xb1, 0xc9, 0x39, 0x8d, 0x2d,
                                       0xd2, 0x72, 0xc6, 0x36, 0x4e, 0x1e, 0x93, 0x63, 0x87, 0x27, 0x4b, 0x1b};
    unsigned long long lo = 0, mid = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        lo |= static_cast<unsigned long long>(tbl[i]) << (8 * i);
        mid |= static_cast<unsigned long long>(tbl[8 + i]) << (8 * i);
        hi |= static_cast<unsigned long long>(tbl[16 + i]) << (8 * i);
    }
    const unsigned long long w = id < 8 ? lo : (id < 16 ? mid : hi);
    return static_cast<unsigned>((w >> (8 * (id & 7))) & 0xff);
}
// -> true when the slice was laid out here (else the caller's greedy order runs)
__device__ __forceinline__ bool sell16_fill_balanced(QbShared &sh, int entry, const int32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ col, const float *__restrict__ val, int32_t *rows,
                                                     int32_t n_entries, int32_t block_cols, const int32_t *__restrict__ ext,
                                                     int32_t *__restrict__ q_col, float *__restrict__ q_val) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q4 = lane >> 4;
    const int chunk0 = ext[2 * entry];
    // ---- the slice's rows (every lane learns row r's extent; lanes r < 16 of quarter 0 speak for it)
    const int row = rows[entry * Q_ROWS + r];
    const int row_next = __shfl(row, (lane & 48) + min(r + 1, 15));
    if (__any(r < 15 && row == row_next)) return false;  // padding slots (duplicate rows): the greedy order keeps them equal
    const int a = rowptr[row], len = rowptr[row + 1] - a;
    int width = len;
    for (int o = 8; o > 0; o >>= 1) width = max(width, __shfl_xor(width, o));
    if (width > QB_MAXW || width == 0) return false;
    const int pieces = (width + Q_SPLIT_WIDTH - 1) / Q_SPLIT_WIDTH;
    const int T = Q_SPLIT_WIDTH * (pieces - 1) + ((width - Q_SPLIT_WIDTH * (pieces - 1) + 3) & ~3);  // steps the kernel sweeps
    // the entries of the slice's run: this one + the CONT entries behind it (pieces and ghosts: they share q_rows)
    int run = 1;
    while (entry + run < n_entries && (ext[2 * (entry + run) + 1] & Q_CONT)) ++run;
    // ---- columns into LDS, class counts (quarter q4 of the wave counts entries q4, q4 + 4, ..)
    unsigned cnt = 0;  // 4 x 8 bits
    for (int j = q4; j < len; j += 4) {
        const int c = col[a + j];
        sh.col[r][j] = c;
        cnt += 1u << (8 * (c & 3));
    }
    cnt += __shfl_xor(cnt, 16);
    cnt += __shfl_xor(cnt, 32);
    __builtin_amdgcn_wave_barrier();
    // per row: entry ids sorted by class (lanes < 16; counting sort, stable)
    if (lane < Q_ROWS) {
        int at[4] = {0, qb_field8(cnt, 0), qb_field8(cnt, 0) + qb_field8(cnt, 1), qb_field8(cnt, 0) + qb_field8(cnt, 1) + qb_field8(cnt, 2)};
        for (int j = 0; j < len; ++j) {
            const int c = sh.col[r][j] & 3;
            const int p = c == 0 ? at[0]++ : (c == 1 ? at[1]++ : (c == 2 ? at[2]++ : at[3]++));
            sh.order[r][p] = static_cast<unsigned char>(j);
        }
    }
    // ---- 64 candidate deals of the rows to the four groups; lane 0 takes them in slot order
    unsigned long long gsum[4] = {0, 0, 0, 0};  // per group: 4 x 16 bits, entries per class
    int gsize[4] = {0, 0, 0, 0};
    unsigned assign = 0;  // 2 bits per row
    {
        unsigned long long perm = 0xfedcba9876543210ull;  // nibble i = the i-th row dealt
        unsigned seed = 0x9e3779b9u * (lane + 1) + 0x85ebca6bu * static_cast<unsigned>(entry);
        if (lane > 0)
            for (int i = 15; i > 0; --i) {  // Fisher-Yates on nibbles
                seed = seed * 1664525u + 1013904223u;
                const int k = static_cast<int>((seed >> 8) % static_cast<unsigned>(i + 1));
                const unsigned long long ni = (perm >> (4 * i)) & 0xf, nk = (perm >> (4 * k)) & 0xf;
                perm = (perm & ~((0xfull << (4 * i)) | (0xfull << (4 * k)))) | (nk << (4 * i)) | (ni << (4 * k));
            }
        for (int i = 0; i < Q_ROWS; ++i) {
            const int rr = static_cast<int>((perm >> (4 * i)) & 0xf);
            const unsigned c8 = __shfl(cnt, rr);
            const unsigned long long c16 = (c8 & 0xffull) | ((c8 & 0xff00ull) << 8) | ((c8 & 0xff0000ull) << 16) | ((c8 & 0xff000000ull) << 24);
            int best = -1, best_key = 0x7fffffff;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned long long t = gsum[g] + c16;
                int over = 0, mx = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int v = static_cast<int>((t >> (16 * c)) & 0xffff);
                    over += max(v - T, 0);
                    mx = max(mx, v);
                }
                const int key = gsize[g] >= 4 ? 0x7fffffff : ((over << 16) | (mx << 2) | g);
                if (key < best_key) {
                    best_key = key;
                    best = g;
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g == best) {
                    gsum[g] += c16;
                    ++gsize[g];
                }
            assign |= static_cast<unsigned>(best) << (2 * rr);
        }
    }
    int total_over = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) total_over += max(static_cast<int>((gsum[g] >> (16 * c)) & 0xffff) - T, 0);
    int key = (total_over << 6) | lane;
    for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o));
    assign = __shfl(assign, key & 63);
    // ---- slots: member `rank` of group g sits in slot qb_group_slot(g, rank); src_of = the old slot whose row moves to slot r
    const int my_g = (assign >> (2 * r)) & 3;
    int rank = 0;
    for (int o = 0; o < Q_ROWS; ++o) rank += (o < r && static_cast<int>((assign >> (2 * o)) & 3) == my_g) ? 1 : 0;
    const int new_slot = qb_group_slot(my_g, rank);
    int src_of = 0;
    for (int o = 0; o < Q_ROWS; ++o) src_of = (__shfl(new_slot, o) == r) ? o : src_of;
    const int n_row = __shfl(row, src_of), n_a = __shfl(a, src_of), n_len = __shfl(len, src_of);
    const unsigned n_cnt = __shfl(cnt, src_of);
    // ---- the schedule of group q4 (16 lanes: two permutations each for the first eight)
    {
        unsigned m[4];
        int pad[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int slot = qb_group_slot(q4, i);
            m[i] = __shfl(n_cnt, slot);
            pad[i] = T - __shfl(n_len, slot);
        }
        for (int step = 0; step < T; ++step) {
            const int left = T - step;
            int colsum[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) colsum[c] = qb_field8(m[0], c) + qb_field8(m[1], c) + qb_field8(m[2], c) + qb_field8(m[3], c);
            int best_key = 0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int id = r + 16 * half;
                if (id < 24) {
                    const unsigned p = qb_perm(id);
                    bool ok = true;
                    int after[4] = {colsum[0], colsum[1], colsum[2], colsum[3]};
                    int score = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = (p >> (2 * i)) & 3;
                        const bool real = qb_field8(m[i], c) > 0;
                        ok = ok && (real || pad[i] > 0);
                        if (real) {
                            score += colsum[c];
#pragma unroll
                            for (int cc = 0; cc < 4; ++cc) after[cc] -= (cc == c) ? 1 : 0;
                        }
                    }
                    int over = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) over += max(after[c] - (left - 1), 0);
                    const int k = ok ? (((1023 - min(over, 1023)) << 18) | (min(score, 2047) << 5) | (31 - id)) : 0;
                    best_key = max(best_key, k);
                }
            }
            for (int o = 8; o > 0; o >>= 1) best_key = max(best_key, __shfl_xor(best_key, o));
            unsigned p;
            if (best_key > 0) {
                p = qb_perm(31 - (best_key & 31));
            } else {  // no conflict-free step is left: every row takes the class it holds most of (a padding row: class 0)
                p = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int bc = 0;
#pragma unroll
                    for (int c = 1; c < 4; ++c) bc = qb_field8(m[i], c) > qb_field8(m[i], bc) ? c : bc;
                    p |= static_cast<unsigned>(bc) << (2 * i);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = (p >> (2 * i)) & 3;
                const bool real = qb_field8(m[i], c) > 0;
                if (real) m[i] -= 1u << (8 * c);
                else --pad[i];
                if (r == i) sh.pick[qb_group_slot(q4, i)][step] = static_cast<unsigned char>(c | (real ? 4 : 0));
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- emit: lane s < 16 writes the row now in slot s; padding reads the zero row of the scheduled class
    if (lane < Q_ROWS) {
        const int n_chunks = (width + Q_CHUNK - 1) / Q_CHUNK;
        int32_t *dst = q_col + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK;
        float *dstv = q_val ? q_val + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK : nullptr;
        int used[4] = {0, 0, 0, 0};
        const int base1 = qb_field8(n_cnt, 0), base2 = base1 + qb_field8(n_cnt, 1), base3 = base2 + qb_field8(n_cnt, 2);
        for (int e = 0; e < n_chunks * Q_CHUNK; ++e) {
            const int at = (e / Q_CHUNK) * Q_CHUNK_INTS + (e % Q_CHUNK);
            int off = block_cols * 64;
            float v = 0.f;
            if (e < T) {
                const int b = sh.pick[r][e], c = b & 3;
                if (b & 4) {
                    const int k = c == 0 ? used[0]++ : (c == 1 ? used[1]++ : (c == 2 ? used[2]++ : used[3]++));
                    const int j = sh.order[src_of][(c == 0 ? 0 : (c == 1 ? base1 : (c == 2 ? base2 : base3))) + k];
                    off = sh.col[src_of][j] * 64;
                    v = val ? val[n_a + j] : 1.f;
                } else {
                    off = (block_cols + c) * 64;
                }
            }
            dst[at] = off;
            if (dstv) dstv[at] = v;
        }
        for (int t = 0; t < run; ++t) rows[(entry + t) * Q_ROWS + r] = n_row;
    }
    return true;
}

// ---- HALF slabs (32-byte slab rows, ds_read_b64): an LDS service group is 32 lanes = EIGHT rows (slots 0 - 7 / 8 - 15 of the
// slice), a row's bank window is 8 (column mod 8) .. + 7: a step is conflict-free when the eight columns read differ mod 8.  Round 4's
// greedy order (below: every row in turn takes a class nobody took yet in this step) left 31 % of the sweep's LDS cycles to conflicts
// on the N = 4000 shard (profiles/r05_c3lit_pmc_summary.txt).  The schedule is an EDGE COLOURING of the bipartite multigraph
// rows x classes (an edge per stored entry, a colour = a step): by Koenig's theorem max(longest row, fullest class) colours
// suffice, i.e. every step is conflict-free whenever no class holds more entries (over the group's eight rows) than the slice has
// steps - and the few entries beyond that (a class total above the step count: ~1 - 3 % on the sweep's graphs) double up.  One
// lane per group colours its edges one by one: a step free at the row and at the class if there is one, else the a / b Kempe
// chain from the class is flipped (a free at the row, b free at the class).  Padding (a row shorter than the schedule) reads one
// of the four zero rows - the one whose window no row of the group reads in that step, when there is one.
struct QhShared {
    unsigned char cls[Q_ROWS][QB_MAXW];       // class (local column mod 8) of entry j of slot r, column order
    unsigned char at_row[Q_ROWS][QB_MAXW];    // per slot and step: the class read (0xff: padding)
    unsigned char at_cls[2][8][QB_MAXW];      // per group, class and step: the slot (0 .. 7) that reads the class's window (0xff: none)
    unsigned long long free_row[Q_ROWS][2], free_cls[2][8][2];  // steps still free (bit s of word s / 64)
    unsigned char need[Q_ROWS][8];            // entries per slot and class
};
union QfShared {
    QbShared b;
    QhShared h;
};
__device__ __forceinline__ int qh_first(unsigned long long lo, unsigned long long hi) {
    return lo ? __ffsll(static_cast<long long>(lo)) - 1 : 64 + __ffsll(static_cast<long long>(hi)) - 1;
}
// -> true when the slice was laid out here (else the caller's greedy order runs)
__device__ __forceinline__ bool sell16_fill_half_coloured(QhShared &sh, int entry, const int32_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ col, const float *__restrict__ val,
                                                          const int32_t *rows, int32_t block_cols, const int32_t *__restrict__ ext,
                                                          int32_t *__restrict__ q_col, float *__restrict__ q_val) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q4 = lane >> 4;
    const int chunk0 = ext[2 * entry];
    const int row = rows[entry * Q_ROWS + r];
    const int row_next = __shfl(row, (lane & 48) + min(r + 1, 15));
    if (__any(r < 15 && row == row_next)) return false;  // padding slots (duplicate rows): the greedy order keeps them equal
    const int a = rowptr[row], len = rowptr[row + 1] - a;
    int width = len;
    for (int o = 8; o > 0; o >>= 1) width = max(width, __shfl_xor(width, o));
    const int n_chunks = (width + Q_CHUNK - 1) / Q_CHUNK, S = n_chunks * Q_CHUNK;
    if (S > QB_MAXW || width == 0) return false;
    // the steps the kernel SWEEPS (split form: 32 per full piece + the last piece rounded up to whole quads): no entry may lie beyond
    const int pieces = (width + Q_SPLIT_WIDTH - 1) / Q_SPLIT_WIDTH;
    const int T = Q_SPLIT_WIDTH * (pieces - 1) + ((width - Q_SPLIT_WIDTH * (pieces - 1) + 3) & ~3);
    // ---- classes into LDS (quarter q4 of the wave takes entries q4, q4 + 4, ..), per-slot class counts
    if (q4 == 0)
        for (int c = 0; c < 8; ++c) sh.need[r][c] = 0;
    for (int j = q4; j < len; j += 4) sh.cls[r][j] = static_cast<unsigned char>(col[a + j] & 7);
    for (int s_ = q4; s_ < S; s_ += 4) sh.at_row[r][s_] = 0xff;
    for (int i = lane; i < 2 * 8 * QB_MAXW; i += 64) (&sh.at_cls[0][0][0])[i] = 0xff;
    __builtin_amdgcn_wave_barrier();
    if (lane < Q_ROWS)
        for (int j = 0; j < len; ++j) ++sh.need[r][sh.cls[r][j]];
    __builtin_amdgcn_wave_barrier();
    // ---- one lane per group of eight slots colours the group's edges
    if (lane == 0 || lane == 8) {
        const int g = lane >> 3, r0 = 8 * g;
        int tot[8], lmax = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) tot[c] = 0;
        for (int i = 0; i < 8; ++i) {
            int l = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) tot[c] += sh.need[r0 + i][c], l += sh.need[r0 + i][c];
            lmax = max(lmax, l);
        }
        int tmax = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) tmax = max(tmax, tot[c]);
        const int steps = min(T, max(lmax, tmax));  // colours in use: padding only where a slot is shorter than the schedule
        const unsigned long long lo = steps >= 64 ? ~0ull : ((1ull << steps) - 1ull), hi = steps <= 64 ? 0ull : (steps >= 128 ? ~0ull : ((1ull << (steps - 64)) - 1ull));
        for (int i = 0; i < 8; ++i) {
            sh.free_row[r0 + i][0] = lo, sh.free_row[r0 + i][1] = hi;
            sh.free_cls[g][i][0] = lo, sh.free_cls[g][i][1] = hi;
        }
        auto take = [&](unsigned long long *m, int s_) { m[s_ >> 6] &= ~(1ull << (s_ & 63)); };
        auto give = [&](unsigned long long *m, int s_) { m[s_ >> 6] |= 1ull << (s_ & 63); };
        int reg[8];  // entries of a class coloured so far: at most `steps` of them can have a step of their own
#pragma unroll
        for (int c = 0; c < 8; ++c) reg[c] = 0;
        for (int i = 0; i < 8; ++i) {
            const int rr = r0 + i;
            for (int c = 0; c < 8; ++c) {
                int n_reg = min(static_cast<int>(sh.need[rr][c]), steps - reg[c]);
                reg[c] += n_reg;
                sh.need[rr][c] -= static_cast<unsigned char>(n_reg);  // (what is left: the entries that double up, placed below)
                for (; n_reg > 0; --n_reg) {
                    unsigned long long *fr = sh.free_row[rr], *fc = sh.free_cls[g][c];
                    const unsigned long long c0 = fr[0] & fc[0], c1 = fr[1] & fc[1];
                    int s_;
                    if (c0 | c1) {
                        s_ = qh_first(c0, c1);
                    } else {  // a: free at the slot (taken at the class), b: free at the class (taken at the slot)
                        const int ca = qh_first(fr[0], fr[1]), cb = qh_first(fc[0], fc[1]);
                        int x = c, r1 = sh.at_cls[g][c][ca];  // the edge (r1, x) leaves colour a ..
                        sh.at_cls[g][c][ca] = 0xff;
                        sh.at_row[r0 + r1][ca] = 0xff;
                        take(fc, cb);  // (c: b taken from now on; a goes to the new edge)
                        for (;;) {     // .. and takes b; what it displaces takes a; and so on along the chain
                            const int c1_ = sh.at_row[r0 + r1][cb];
                            sh.at_cls[g][x][cb] = static_cast<unsigned char>(r1);
                            sh.at_row[r0 + r1][cb] = static_cast<unsigned char>(x);
                            if (c1_ == 0xff) {
                                give(sh.free_row[r0 + r1], ca), take(sh.free_row[r0 + r1], cb);
                                break;
                            }
                            sh.at_cls[g][c1_][cb] = 0xff;
                            const int r2 = sh.at_cls[g][c1_][ca];
                            sh.at_row[r0 + r1][ca] = static_cast<unsigned char>(c1_);
                            sh.at_cls[g][c1_][ca] = static_cast<unsigned char>(r1);
                            if (r2 == 0xff) {
                                give(sh.free_cls[g][c1_], cb), take(sh.free_cls[g][c1_], ca);
                                break;
                            }
                            sh.at_row[r0 + r2][ca] = 0xff;
                            x = c1_, r1 = r2;
                        }
                        s_ = ca;
                    }
                    sh.at_row[rr][s_] = static_cast<unsigned char>(c);
                    sh.at_cls[g][c][s_] = static_cast<unsigned char>(i);
                    take(fr, s_), take(fc, s_);
                }
            }
        }
        // the entries beyond a class's steps: any step the slot still has (they share the class's window with another slot)
        for (int i = 0; i < 8; ++i)
            for (int c = 0; c < 8; ++c)
                for (int k = sh.need[r0 + i][c]; k > 0; --k) {
                    unsigned long long *fr = sh.free_row[r0 + i];
                    const int s_ = qh_first(fr[0], fr[1]);
                    sh.at_row[r0 + i][s_] = static_cast<unsigned char>(c);
                    take(fr, s_);
                }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- emit: lane s < 16 writes the row in slot s: per step the next entry (column order) of the scheduled class
    if (lane < Q_ROWS) {
        int32_t *dst = q_col + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK;
        float *dstv = q_val ? q_val + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK : nullptr;
        int cur[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int g = r >> 3;
        for (int e = 0; e < S; ++e) {
            const int at = (e / Q_CHUNK) * Q_CHUNK_INTS + (e % Q_CHUNK);
            const int c = sh.at_row[r][e];
            int off;
            float v = 0.f;
            if (c != 0xff) {
                int j = 0;
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) j = cc == c ? cur[cc] : j;
                while (sh.cls[r][j] != c) ++j;
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) cur[cc] = cc == c ? j + 1 : cur[cc];
                off = col[a + j] * 32;
                v = val ? val[a + j] : 1.f;
            } else {  // padding: the zero row (four of them behind the block: windows block_cols mod 8 .. + 3) nobody's window collides with
                int k = 0;
                for (int t = 3; t >= 0; --t) k = sh.at_cls[g][(block_cols + t) & 7][e] == 0xff ? t : k;
                off = (block_cols + k) * 32;
            }
            dst[at] = off;
            if (dstv) dstv[at] = v;
        }
    }
    return true;
}

// One wave per (column block, entry that starts a slice); lane r < 16 orders row r's segment.  Bank-aware order (reorder != 0):
// the sweep reads, for entry e of all 16 rows, the 64-byte LDS row of each row's column; the four rows of a service group
// collide when their columns agree mod 4 (64-byte rows: a row's bank window is 16 (column mod 4) .. + 15).  The order of a
// row's entries inside a block is free, so the rows of a group choose step by step, in rank order, a remaining entry whose
// class is not taken yet in this step (the class they hold most of first; the first remaining entry of that class).
__device__ __forceinline__ void sell16_fill_body(int task, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 const float *__restrict__ val, int32_t *rows,
                                                 int32_t n_entries, int32_t n_blocks, int32_t block_cols,
                                                 const int32_t *__restrict__ ext, int32_t *__restrict__ q_col,
                                                 float *__restrict__ q_val, int reorder, QfShared *qb) {
    const int lane = threadIdx.x & 63;
    if (task >= n_entries * n_blocks) return;  // (whole waves: a task is a wave)
    const int blk = task / n_entries, entry = task % n_entries;
    if (ext[2 * task + 1] & Q_CONT) return;  // a continuation / ghost entry: its slice's first entry fills the chunks
    // split form (one column block, <= 128 entries per row): the conflict-free order (reorder 2: WDG_SELL_ORDER=1 keeps round 2's greedy one)
    const int rb = (n_blocks == 1 && block_cols > Q_MAX_BLOCK_COLS) ? 32 : 64;  // bytes of a slab row (HALF slabs: 8 features)
    if (reorder == 2 && rb == 64 && n_blocks == 1 && (ext[2 * n_entries + 1] & Q_CONT) &&
        sell16_fill_balanced(qb->b, entry, rowptr, col, val, rows, n_entries, block_cols, ext, q_col, q_val))
        return;
    // HALF slabs: the edge-coloured order (reorder 2; WDG_SELL_ORDER=1 keeps round 4's greedy one)
    if (reorder == 2 && rb == 32 && n_blocks == 1 && (ext[2 * n_entries + 1] & Q_CONT) && sell16_fill_half_coloured(qb->h, entry, rowptr, col, val, rows, block_cols, ext, q_col, q_val))
        return;
    const int chunk0 = ext[2 * task];
    const int r = lane & 15;
    const bool worker = lane < 16;
    const int row = rows[entry * Q_ROWS + r];
    // the slots that pad a graph's last slice repeat its last row: they must hold that row's entries in the SAME order
    const int row_prev = __shfl(row, (lane & 48) + max(r - 1, 0));
    const bool ghost = r > 0 && row == row_prev;
    const unsigned long long first_mask = __ballot(worker && row == __shfl(row, 15) && !ghost);
    const int last_lane = first_mask ? __ffsll(static_cast<long long>(first_mask)) - 1 : 15;
    int a = 0, len = 0;
    {
        const int s = rowptr[row], e = rowptr[row + 1];
        a = n_blocks == 1 ? s : q_lower_bound(col, s, e, blk * block_cols);
        const int b = (blk + 1 == n_blocks) ? e : q_lower_bound(col, a, e, (blk + 1) * block_cols);
        len = b - a;
    }
    int width = worker ? len : 0;
    for (int o = 8; o > 0; o >>= 1) width = max(width, __shfl_xor(width, o));
    width = __shfl(width, 0);
    const int n_chunks = (width + Q_CHUNK - 1) / Q_CHUNK;
    const int col0 = blk * block_cols;
    const int zero_off = block_cols * rb;  // the (first) all-zero row behind the block's rows
    // service groups of ds_read_b128 in quads (= rows): {0,3,5,6}, {1,2,4,7}, {8,11,13,14}, {9,10,12,15}
    const int x = r & 7;
    const bool g0 = (x == 0 || x == 3 || x == 5 || x == 6);
    const int m0 = g0 ? 0 : 1, m1 = g0 ? 3 : 2, m2 = g0 ? 5 : 4, m3 = g0 ? 6 : 7;
    const int rank = (x == m0) ? 0 : (x == m1) ? 1 : (x == m2) ? 2 : 3;
    const int hi = r & 8;
    // HALF slabs (32-byte rows, ds_read_b64: service groups of 32 lanes = rows 0-7 / 8-15, a row's bank window is
    // 8 (column mod 8) .. + 7): eight classes, the eight rows of a group choose in row order
    const int n_cls = rb == 32 ? 8 : 4, cmask = n_cls - 1;
    const int my_rank = rb == 32 ? x : rank;
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cur[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (reorder)
        for (int j = 0; j < len; ++j) ++cnt[(col[a + j] - col0) & cmask];
    int32_t *dst = q_col + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK;
    float *dstv = q_val ? q_val + static_cast<int64_t>(chunk0) * Q_CHUNK_INTS + r * Q_CHUNK : nullptr;
    for (int e = 0; e < n_chunks * Q_CHUNK; ++e) {
        int pick = -1;
        if (reorder) {
            unsigned used = 0;
            for (int rk = 0; rk < n_cls; ++rk) {
                int cls = -1;
                if (worker && !ghost && my_rank == rk && e < len) {
                    int best = -1, best_any = -1;
#pragma unroll
                    for (int c4 = 0; c4 < 8; ++c4) {
                        if (c4 >= n_cls || cnt[c4] == 0) continue;
                        if (best_any < 0 || cnt[c4] > cnt[best_any]) best_any = c4;
                        if (!((used >> c4) & 1u) && (best < 0 || cnt[c4] > cnt[best])) best = c4;
                    }
                    cls = best >= 0 ? best : best_any;
                    int j = cur[cls];
                    while (((col[a + j] - col0) & cmask) != cls) ++j;
                    pick = j;
                    cur[cls] = j + 1;
                    --cnt[cls];
                }
                const int src_lane = hi + (rb == 32 ? rk : (rk == 0 ? m0 : rk == 1 ? m1 : rk == 2 ? m2 : m3));
                const int got = __shfl(cls, src_lane);
                if (got >= 0) used |= 1u << got;
            }
        } else if (e < len) {
            pick = e;
        }
        const int pick_last = __shfl(pick, last_lane);
        if (ghost) pick = pick_last;
        if (worker) {
            const int at = (e / Q_CHUNK) * Q_CHUNK_INTS + (e % Q_CHUNK);
            dst[at] = pick >= 0 ? (col[a + pick] - col0) * rb : zero_off;
            if (dstv) dstv[at] = pick >= 0 ? (val ? val[a + pick] : 1.f) : 0.f;
        }
    }
}
__global__ __launch_bounds__(256) void sell16_fill(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const float *__restrict__ val, int32_t *rows,
                                                   int32_t n_entries, int32_t n_blocks, int32_t block_cols,
                                                   const int32_t *__restrict__ ext, int32_t *__restrict__ q_col,
                                                   float *__restrict__ q_val, int reorder) {
    __shared__ QfShared qb[4];  // one per wave
    sell16_fill_body((blockIdx.x * 256 + threadIdx.x) >> 6, rowptr, col, val, rows, n_entries, n_blocks, block_cols, ext, q_col, q_val,
                     reorder, &qb[threadIdx.x >> 6]);
}

// ---- the same build for a TABLE of graphs (wdg_sell16_job; blockIdx.y = graph): a sweep shard's SELL-16 copies in six launches
// and one host read-back instead of ten launches and a host sync per graph (the cold, one-pass sweep: synthetic_plot.py:78-109
// visits every graph once).  Per-graph scratch lives in the job's workspace (sell16_ws).
__global__ __launch_bounds__(1024) void sell16_sort_rows_batched(const wdg_sell16_job *__restrict__ jobs) {
    extern __shared__ unsigned long long q_keys[];
    const wdg_sell16_job j = jobs[blockIdx.y];
    if (j.n_rows <= 0) return;
    sell16_sort_rows_body(j.rowptr, j.n_rows, j.q_perm, q_keys);
}
__global__ __launch_bounds__(256) void sell16_widths_batched(const wdg_sell16_job *__restrict__ jobs) {
    const wdg_sell16_job j = jobs[blockIdx.y];
    if (j.n_rows <= 0) return;
    const Sell16Shape sh = sell16_shape(j.n_rows, j.n_cols);
    const Sell16Ws w = sell16_ws(j.workspace, sh.tasks, sh.max_entries);
    sell16_widths_body(blockIdx.x * 256 + threadIdx.x, j.rowptr, j.col, j.q_perm, j.n_rows, sh.n_slices, sh.n_blocks, sh.block_cols,
                       w.chunks, w.widths);
}
// one workgroup per graph: exclusive scan of the (block, slice) chunk counts in place (total behind them), then the packer
__global__ __launch_bounds__(1024) void sell16_scan_pack_batched(const wdg_sell16_job *__restrict__ jobs) {
    __shared__ int buf[1024];
    __shared__ int carry;
    const wdg_sell16_job j = jobs[blockIdx.y];
    if (j.n_rows <= 0) {
        if (threadIdx.x == 0 && j.q_ext) j.q_ext[0] = j.q_ext[1] = 0;  // an empty graph: {0 chunks, 0 entries}
        return;
    }
    const Sell16Shape sh = sell16_shape(j.n_rows, j.n_cols);
    const Sell16Ws w = sell16_ws(j.workspace, sh.tasks, sh.max_entries);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < sh.tasks; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int v = i < sh.tasks ? w.chunks[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
            const int t = threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < sh.tasks) w.chunks[i] = carry + buf[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += buf[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        w.chunks[sh.tasks] = carry;
        sell16_pack_body(w.widths, sh.n_slices, sh.n_blocks, w.entry_slice, w.entry_k, w.info);
    }
}
__global__ __launch_bounds__(256) void sell16_entries_batched(const wdg_sell16_job *__restrict__ jobs) {
    const wdg_sell16_job j = jobs[blockIdx.y];
    if (j.n_rows <= 0) return;
    const Sell16Shape sh = sell16_shape(j.n_rows, j.n_cols);
    const Sell16Ws w = sell16_ws(j.workspace, sh.tasks, sh.max_entries);
    sell16_entries_body(blockIdx.x * 256 + threadIdx.x, w.widths, w.chunks, w.entry_slice, w.entry_k, w.info, j.q_perm, sh.n_slices,
                        sh.n_blocks, static_cast<int32_t>(sh.max_entries), j.q_ext, j.q_rows);
}
__global__ __launch_bounds__(256) void sell16_fill_batched(const wdg_sell16_job *__restrict__ jobs, int reorder) {
    const wdg_sell16_job j = jobs[blockIdx.y];
    if (j.n_rows <= 0 || !j.q_col) return;  // (no SELL-16 copy wanted for this graph: decided by the caller after the count)
    const Sell16Shape sh = sell16_shape(j.n_rows, j.n_cols);
    const int32_t n_entries = j.q_ext[2 * sh.n_blocks * sh.max_entries + 1] & 0x3fffffff;
    __shared__ QfShared qb[4];  // one per wave
    sell16_fill_body((blockIdx.x * 256 + threadIdx.x) >> 6, j.rowptr, j.col, j.val, j.q_rows, n_entries, sh.n_blocks, sh.block_cols,
                     j.q_ext, j.q_col, j.q_val, reorder, &qb[threadIdx.x >> 6]);
}

int q_reorder_mode() {  // entry order inside (row, block) segments; WDG_SELL_ORDER: 0 column order, 1 round 2's greedy bank-aware
    const char *e = getenv("WDG_SELL_ORDER");  // order, 2 (default) the conflict-free order for graphs in split form, greedy for the rest
    if (!e) return 2;
    const int v = atoi(e);
    return v < 0 ? 0 : (v > 2 ? 2 : v);
}

}  // namespace

namespace wdg {

// rows by length, longest first, ties by row index (one workgroup, keys in LDS); more than sort_rows_small_limit() rows: identity.
// perm has 16 ceil(N / 16) slots, the padding repeats the last row.  Shared with the band plan (spmm_band.hip).
int sort_rows_small_limit() { return Q_SORT_MAX_ROWS; }
int sort_rows_by_length_small(const int32_t *rowptr, int32_t N, int32_t *perm, hipStream_t st) {
    static thread_local int configured_dev = -1;
    const int dev = current_device();
    if (configured_dev != dev) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(sell16_sort_rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                                Q_SORT_MAX_ROWS * 8) != hipSuccess)
            return fail(WDG_ERR_LAUNCH, "row sort: cannot raise the dynamic LDS limit");
        configured_dev = dev;
    }
    const size_t sort_lds = N <= Q_SORT_MAX_ROWS ? static_cast<size_t>(N) * 8 : 0;
    hipLaunchKernelGGL(sell16_sort_rows, dim3(1), dim3(1024), sort_lds, st, rowptr, N, perm);
    return check_launch("sell16_sort_rows");
}

}  // namespace wdg

extern "C" {

int32_t wdg_sell16_block_cols(int32_t n_cols) { return q_block_cols_hd(n_cols); }
int32_t wdg_sell16_row_bytes(int32_t n_cols) { return q_row_bytes_hd(n_cols); }

int64_t wdg_sell16_max_entries(int32_t N) { return sell16_shape(N, 1).max_entries; }

size_t wdg_sell16_workspace_bytes(int32_t N, int32_t n_cols) {
    const Sell16Shape sh = sell16_shape(N, n_cols);
    // the size authority: the scan's workspace + the arrays sell16_ws hands out (each 256-byte aligned: the slack covers its six roundings)
    return wdg::exclusive_scan_ws_bytes(sh.tasks + 1) + static_cast<size_t>(2 * sh.tasks + 2 * sh.max_entries + 16) * sizeof(int32_t) + 2048;
}

int wdg_csr_to_sell16_count(const int32_t *rowptr, const int32_t *col, int32_t N, int32_t n_cols, int32_t *q_perm,
                            int32_t *q_ext, int32_t *q_rows, void *workspace, size_t workspace_bytes, wdg_stream_t stream) {
    WDG_REQUIRE(N >= 0 && n_cols >= 0 && q_ext && (N == 0 || (rowptr && q_perm && q_rows)), "csr_to_sell16_count: bad arguments");
    if (!workspace || workspace_bytes < wdg_sell16_workspace_bytes(N, n_cols))
        return wdg::fail(WDG_ERR_WORKSPACE, "csr_to_sell16: workspace too small");
    hipStream_t st = wdg::as_stream(stream);
    const Sell16Shape sh = sell16_shape(N, n_cols);
    const Sell16Ws w = sell16_ws(workspace, sh.tasks, sh.max_entries);
    if (sh.tasks == 0) {  // an empty graph: {0 chunks, 0 entries}
        hipMemsetAsync(q_ext, 0, 2 * sizeof(int32_t), st);
        return WDG_OK;
    }
    if (int e = wdg::sort_rows_by_length_small(rowptr, N, q_perm, st)) return e;
    hipLaunchKernelGGL(sell16_widths, dim3(wdg::ceil_div(sh.tasks, 256)), dim3(256), 0, st, rowptr, col, q_perm, N, sh.n_slices,
                       sh.n_blocks, sh.block_cols, w.chunks, w.widths);
    if (int e = wdg::exclusive_scan_i32(w.chunks, sh.tasks, w.chunks, nullptr, w.scan_ws, st)) return e;
    hipLaunchKernelGGL(sell16_pack, dim3(1), dim3(64), 0, st, w.widths, sh.n_slices, sh.n_blocks, w.entry_slice, w.entry_k, w.info);
    const int64_t threads = std::max<int64_t>(sh.max_entries * sh.n_blocks, sh.max_entries * Q_ROWS);
    hipLaunchKernelGGL(sell16_entries, dim3(wdg::ceil_div(threads, 256)), dim3(256), 0, st, w.widths, w.chunks, w.entry_slice, w.entry_k,
                       w.info, q_perm, sh.n_slices, sh.n_blocks, static_cast<int32_t>(sh.max_entries), q_ext, q_rows);
    return wdg::check_launch("csr_to_sell16_count");
}

int wdg_csr_to_sell16_fill(const int32_t *rowptr, const int32_t *col, const float *val, int32_t N, int32_t n_cols,
                           int32_t *q_rows, const int32_t *q_ext, int32_t n_entries, int32_t *q_col, float *q_val,
                           wdg_stream_t stream) {
    WDG_REQUIRE(N >= 0 && n_cols >= 0 && n_entries >= 0 && q_ext && (N == 0 || q_rows), "csr_to_sell16_fill: bad arguments");
    const Sell16Shape sh = sell16_shape(N, n_cols);
    const int64_t tasks = static_cast<int64_t>(n_entries) * sh.n_blocks;
    if (tasks == 0) return WDG_OK;
    WDG_REQUIRE(rowptr && q_col, "csr_to_sell16_fill: null rowptr / q_col");
    hipLaunchKernelGGL(sell16_fill, dim3(wdg::ceil_div(tasks * 64, 256)), dim3(256), 0, wdg::as_stream(stream), rowptr, col, val,
                       q_rows, n_entries, sh.n_blocks, sh.block_cols, q_ext, q_col, q_val, q_reorder_mode());
    return wdg::check_launch("csr_to_sell16_fill");
}

int wdg_csr_to_sell16_count_batched(const wdg_sell16_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                    wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "csr_to_sell16_count_batched: negative size");
    if (n_jobs == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev, "csr_to_sell16_count_batched: null job table");
    WDG_REQUIRE(max_rows <= Q_SORT_MAX_ROWS, "csr_to_sell16_count_batched: graphs of more than 16 384 rows take the single-graph build");
    hipStream_t st = wdg::as_stream(stream);
    static thread_local int configured_dev = -1;
    const int dev = wdg::current_device();
    if (configured_dev != dev) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(sell16_sort_rows_batched), hipFuncAttributeMaxDynamicSharedMemorySize,
                                Q_SORT_MAX_ROWS * 8) != hipSuccess)
            return wdg::fail(WDG_ERR_LAUNCH, "row sort: cannot raise the dynamic LDS limit");
        configured_dev = dev;
    }
    const Sell16Shape sh = sell16_shape(max_rows, max_cols);  // the bound over the table: sizes the grids
    const unsigned g = static_cast<unsigned>(n_jobs);
    hipLaunchKernelGGL(sell16_sort_rows_batched, dim3(1, g), dim3(1024), static_cast<size_t>(max_rows) * 8, st, jobs_dev);
    if (sh.tasks > 0) hipLaunchKernelGGL(sell16_widths_batched, dim3(wdg::ceil_div(sh.tasks, 256), g), dim3(256), 0, st, jobs_dev);
    hipLaunchKernelGGL(sell16_scan_pack_batched, dim3(1, g), dim3(1024), 0, st, jobs_dev);
    const int64_t threads = std::max<int64_t>(sh.max_entries * sh.n_blocks, sh.max_entries * Q_ROWS);
    hipLaunchKernelGGL(sell16_entries_batched, dim3(wdg::ceil_div(threads, 256), g), dim3(256), 0, st, jobs_dev);
    return wdg::check_launch("csr_to_sell16_count_batched");
}

int wdg_csr_to_sell16_fill_batched(const wdg_sell16_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                   wdg_stream_t stream) {
    WDG_REQUIRE(n_jobs >= 0 && max_rows >= 0 && max_cols >= 0, "csr_to_sell16_fill_batched: negative size");
    if (n_jobs == 0 || max_rows == 0) return WDG_OK;
    WDG_REQUIRE(jobs_dev, "csr_to_sell16_fill_batched: null job table");
    const Sell16Shape sh = sell16_shape(max_rows, max_cols);
    const int64_t tasks = sh.max_entries * sh.n_blocks;
    hipLaunchKernelGGL(sell16_fill_batched, dim3(wdg::ceil_div(tasks * 64, 256), static_cast<unsigned>(n_jobs)), dim3(256), 0,
                       wdg::as_stream(stream), jobs_dev, q_reorder_mode());
    return wdg::check_launch("csr_to_sell16_fill_batched");
}

}  // extern "C"
