// The SELL-16 layout contract: what the build (csrc/sell16.hip: CSR -> SELL-16) writes and the quad-row aggregation kernel
// (csrc/spmm_quad.hip) reads - the slice / chunk / super-unit granules, the column-block rule, the flag bits of q_ext, and the
// shape and scratch layout of one graph's build, shared by its single-graph (host) and batched (device) forms.
#pragma once
#include "wdg_common.h"

namespace wdg {

constexpr int Q_ROWS = 16;             // rows per unit (SELL-16 slice)
constexpr int Q_CHUNK = 16;            // entries per row and index chunk (one 16-byte load per lane)
constexpr int Q_CHUNK_INTS = Q_ROWS * Q_CHUNK;
constexpr int Q_SU = 4;                // slices per super-unit (64 rows): the granule the kernel's waves are dealt
constexpr int Q_MAX_BLOCK_COLS = 2528; // rows of a slab block: (2528 + 4 zero rows) x 64 B = 158.3 KiB of the 160 KiB (+ 256 B of q_ctl)
constexpr int Q_MAX_BLOCKS = 4;        // column blocks (graphs of up to 10 112 columns); more: the CSR kernels

// Graphs of 2 529 .. 5 056 columns keep ONE column block by staging 8 features per source row instead of 16 (HALF slabs, round
// 4: 32-byte slab rows, index offsets pre-scaled by 32, a quad of lanes reads a row with ds_read_b64): the literal N = 4000
// reading of BASELINE configs[2] ran the several-block path at 0.20 of the roofline, staging every block of X per graph.
constexpr int Q_HALF_MAX_BLOCK_COLS = 2 * Q_MAX_BLOCK_COLS;
__host__ __device__ inline bool q_half_hd(int n_cols) { return n_cols > Q_MAX_BLOCK_COLS && n_cols <= Q_HALF_MAX_BLOCK_COLS; }
__host__ __device__ inline int q_row_bytes_hd(int n_cols) { return q_half_hd(n_cols) ? 32 : 64; }

// columns per slab block: the columns cut into the fewest blocks of <= 2528, evenly, a multiple of 4 (column class mod 4 =
// local class mod 4: what the bank-aware order of sell16_fill keys on); HALF slabs: one block of all columns
__host__ __device__ inline int q_block_cols_hd(int n_cols) {
    const int c = n_cols > 0 ? n_cols : 1;
    if (q_half_hd(c)) return (c + 3) & ~3;
    const int blocks = (c + Q_MAX_BLOCK_COLS - 1) / Q_MAX_BLOCK_COLS;
    const int even = (c + blocks - 1) / blocks;
    const int rounded = (even + 3) & ~3;
    return rounded < Q_MAX_BLOCK_COLS ? rounded : Q_MAX_BLOCK_COLS;
}

// perm[slot] = row, rows by total length (longest first, ties by row id): a slice of 16 slots holds rows of similar
// length.  One workgroup, keys in LDS; graphs of more rows keep the identity (they pad by their skew).
constexpr int Q_SORT_MAX_ROWS = 16384;

// The ENTRIES the kernel's waves work through, four per super-unit.  A graph with one column block whose slices hold at most
// 128 entries per row is laid out in SPLIT form: a slice of more than 32 entries per row becomes 2 .. 4 consecutive entries
// of <= 32 (two index chunks: what the kernel's pipeline requests ahead), the later ones flagged CONT - the wave keeps the
// slice's accumulators and stores the running sums after each entry, the last store carrying the final ones.  A slice's
// entries never straddle a super-unit: the super-unit is filled up with GHOST entries (CONT, width 0, the rows of the slice
// before: they store its sums once more).  Other graphs: one entry per slice, ghosts pad the last super-unit.
constexpr int Q_CONT = 1 << 30;
constexpr int Q_SPLIT_WIDTH = 2 * Q_CHUNK;  // entries per row of a split entry

// The shape of a graph's SELL-16 copy: real slices, column blocks, (block, slice) tasks and the bound on its entries per block.
struct Sell16Shape {
    int32_t n_slices, n_blocks, block_cols;
    int64_t tasks, max_entries;
};
__host__ __device__ inline Sell16Shape sell16_shape(int32_t N, int32_t n_cols) {
    Sell16Shape sh;
    sh.n_slices = (N + Q_ROWS - 1) / Q_ROWS;  // (int32 like the kernels' slot indices: 16 n_slices must fit one)
    sh.block_cols = q_block_cols_hd(n_cols);
    sh.n_blocks = ((n_cols > 1 ? n_cols : 1) + sh.block_cols - 1) / sh.block_cols;
    sh.tasks = static_cast<int64_t>(sh.n_slices) * sh.n_blocks;
    sh.max_entries = static_cast<int64_t>(Q_SU) * sh.n_slices + Q_SU;
    return sh;
}
// The per-graph scratch of the build inside the caller's workspace: chunks / chunk_begin [tasks + 2], widths [tasks + 1],
// entry_slice and entry_k [max_entries each], info [4], every array 256-byte aligned; scan_ws = the first byte behind them (the
// single-graph build runs its exclusive scan there).  wdg_sell16_workspace_bytes bounds what this function hands out.
struct Sell16Ws {
    int32_t *chunks, *widths, *entry_slice, *entry_k, *info;
    void *scan_ws;
};
__host__ __device__ inline Sell16Ws sell16_ws(void *workspace, int64_t tasks, int64_t max_entries) {
    char *ws = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~static_cast<uintptr_t>(255));
    auto take = [&](int64_t ints) {
        int32_t *ptr = reinterpret_cast<int32_t *>(ws);
        ws += (static_cast<size_t>(ints) * sizeof(int32_t) + 255) & ~static_cast<size_t>(255);
        return ptr;
    };
    Sell16Ws w;
    w.chunks = take(tasks + 2);
    w.widths = take(tasks + 1);
    w.entry_slice = take(max_entries);
    w.entry_k = take(max_entries);
    w.info = take(4);
    w.scan_ws = ws;
    return w;
}

}  // namespace wdg
