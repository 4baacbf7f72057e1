/*
 * wdg.h - C ABI of libwdg_hip.so: MI355X (gfx950) kernels for the aggregation /
 * homophily-metric hot path of SitaoLuan/When-Do-GNNs-Help.
 *
 * The reference is pure Python and has no FFI layer; the narrowest seam it offers is
 * the set of torch/scipy calls its metric code makes.  Each entry
 * point below replaces one of those calls; the `replaces:` line cites it
 * (paths are into the reference checkout).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - the caller owns all memory (outputs and workspaces are caller-allocated);
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work:
 *     no allocation, no synchronisation, no host copies -> graph-capturable;
 *   - return value: WDG_OK or a negative WDG_ERR_*; wdg_last_error() gives text;
 *   - indices are int32 on the device (int64 only at the COO boundary, matching
 *     torch's `indices()` dtype); sizes that can exceed 2^31 are int64.
 */
#ifndef WDG_H
#define WDG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *wdg_stream_t; /* hipStream_t */

#define WDG_OK 0
#define WDG_ERR_INVALID (-1)     /* bad argument (null pointer, negative size, ...)   */
#define WDG_ERR_LAUNCH (-2)      /* the HIP runtime rejected a launch                  */
#define WDG_ERR_WORKSPACE (-3)   /* workspace too small                                */
#define WDG_ERR_UNSUPPORTED (-4) /* shape outside what the kernels were built for      */

int wdg_version(void);
const char *wdg_last_error(void);
/* number of CUs of the current device (host query, cached). */
int wdg_device_cus(void);

/* ------------------------------------------------------------------ graph construction */
#define WDG_COO_SYMMETRISE 1      /* insert (dst,src) too           : to_undirected            */
#define WDG_COO_BINARISE 2        /* merged value := 1              : to_undirected / (adj>0)  */
#define WDG_COO_ADD_SELF_LOOPS 4  /* + I after merging (loop -> v+1): adj + eye                */
#define WDG_COO_DROP_SELF_LOOPS 8 /* remove (i,i) of the input      : remove_self_loops        */
#define WDG_COO_KEEP_DUPLICATES 16 /* sort only, no merging (edge-index inputs counted with multiplicity) */

/*
 * COO (int64 src/dst, optional fp32 val) -> CSR (int32 rowptr[N+1], col, fp32 val), rows sorted
 * by column, duplicates summed in input order.
 * replaces: torch `.coalesce()` utils/homophily_metrics.py:50,63,127;
 *           `to_undirected` utils/util_funcs.py:225-283;
 *           `adj + sp.eye` / `torch.eye + adj.to_dense()` utils/util_funcs.py:385,420, homophily_tests.py:83;
 *           `sparse_mx_to_torch_sparse_tensor` utils/util_funcs.py:400-407 (index part).
 * col/outval capacity: wdg_coo_to_csr_capacity(E, N, flags) entries.  *nnz_out (device int64) receives nnz.
 * out-of-range indices set *nnz_out = -1 (checked by the host wrapper after the stream syncs).
 */
int64_t wdg_coo_to_csr_capacity(int64_t E, int32_t N, int flags);
size_t wdg_coo_to_csr_workspace_bytes(int64_t E, int32_t N, int flags);
int wdg_coo_to_csr_i32(const int64_t *src, const int64_t *dst, const float *val, int64_t E, int32_t N, int flags,
                       int32_t *rowptr, int32_t *col, float *outval, int64_t *nnz_out, void *workspace,
                       size_t workspace_bytes, wdg_stream_t stream);
/* the same build from 4-byte indices (what wdg_host_pack_coo_i32 produces: half the bytes across PCIe) */
int wdg_coo32_to_csr_i32(const int32_t *src, const int32_t *dst, const float *val, int64_t E, int32_t N, int flags,
                         int32_t *rowptr, int32_t *col, float *outval, int64_t *nnz_out, void *workspace,
                         size_t workspace_bytes, wdg_stream_t stream);

/*
 * A whole sweep shard through ONE COO -> CSR build (the reference's loop builds a graph per iteration, synthetic_plot.py:84-92;
 * here the shard's graphs are laid out as one block-diagonal graph of sum(n_g) nodes, built by a single wdg_coo_to_csr_i32 call,
 * and cut apart again - one launch sequence and one host read-back per shard instead of ~10 launches and a sync per graph).
 *   wdg_coo_blockdiag_offset: the concatenated edge lists of the graphs (graph g holds entries edge_ptr[g] .. edge_ptr[g+1] - 1,
 *     node ids local to the graph) -> ids of the block-diagonal graph, in place: id + node_ptr[g].  An id outside [0, n_g) sets
 *     *bad_out (device int32, zeroed by the call first) to 1 and is left out of range of the whole graph.
 *   wdg_csr_split_blockdiag: the block-diagonal CSR -> per-graph CSRs: rowptr_out (pooled: graph g's n_g + 1 offsets start at
 *     node_ptr[g] + g, rebased to 0), col rebased IN PLACE (col -= node_ptr[g]; graph g's entries stay where they are: at
 *     rowptr[node_ptr[g]]), nnz_out[g] = entries of graph g.  With sell_jobs_dev != NULL the rowptr / col / val fields of
 *     job g of that wdg_sell16_job table are set to graph g's arrays (val only when val != NULL), so that
 *     wdg_csr_to_sell16_count_batched can follow on the same stream without the host knowing where a graph's entries start.
 * replaces: the per-iteration `adj + eye` / `.to_sparse()` / `.coalesce()` of synthetic_plot.py:85-92, homophily_tests.py:83-85.
 */
/*
 * HOST helper of the same shard build (no device call, no stream): the per-graph COO arrays (host pointers, node ids local to each
 * graph, elem_bytes 8 = int64 as the reference's loaders leave them, or 4) -> one pair of int32 arrays of lens[0] + .. entries
 * holding the ids of the block-diagonal union (id + node_ptr[g]) - what wdg_coo_blockdiag_offset does on the device, done while
 * the data is copied into the (ideally page-locked) upload buffer by `threads` threads.  An id outside [0, n_g) becomes -1 and
 * sets *bad_out (host int32) to 1.  replaces: the host side of synthetic_plot.py:85-92's per-iteration torch.load -> dense.
 */
/* HOST helper: a plain copy by `threads` threads (pageable source -> the page-locked upload buffer).  A sweep shard's feature
 * matrices are 4 - 30 MB each: one thread's memcpy (~10 GB/s) was a third of the shard's host time, and torch's own host copy
 * wakes every hardware thread of the host.  replaces: the `.to(device)` of synthetic_plot.py:81-83's feature tensors (host half). */
int wdg_host_memcpy_mt(void *dst_host, const void *src_host, size_t bytes, int threads);
int wdg_host_pack_coo_i32(const void *const *src_ptrs, const void *const *dst_ptrs, const int64_t *lens, const int32_t *node_ptr,
                          int32_t n_graphs, int elem_bytes, int32_t *out_src, int32_t *out_dst, int32_t *bad_out, int threads);
int wdg_coo_blockdiag_offset(int64_t *src, int64_t *dst, const int64_t *edge_ptr_dev, const int32_t *node_ptr_dev, int32_t n_graphs,
                             int64_t n_edges, int32_t *bad_out, wdg_stream_t stream);
struct wdg_sell16_job;
int wdg_csr_split_blockdiag(const int32_t *rowptr, int32_t *col, const float *val, const int32_t *node_ptr_dev, int32_t n_graphs,
                            int32_t n_nodes_total, int32_t *rowptr_out, int64_t *nnz_out, struct wdg_sell16_job *sell_jobs_dev,
                            wdg_stream_t stream);

/*
 * Dense [N,M] fp32 -> CSR of its non-zeros (the "plot" flavour hands dense adjacencies around).
 * replaces: `A.nonzero()`, `A.to_sparse().coalesce()`, `(adj > 0)` utils/homophily_plot.py:48,85,133,151.
 * Two calls: count (fills rowptr), then fill (needs col/val of rowptr[N] entries).
 * An entry is stored when it compares != 0: -0.0 is dropped; NaN, inf and subnormals are kept, bit for bit.  Columns M .. lda - 1 are
 * never read.  A matrix without rows or without columns has no storage: A may be NULL when N == 0 or M == 0, and the count call
 * itself then returns the empty pattern (rowptr = N + 1 zeros) - the wrappers need no case of their own.
 */
int wdg_dense_to_csr_count(const float *A, int64_t lda, int32_t N, int32_t M, int32_t *rowptr, void *workspace,
                           size_t workspace_bytes, wdg_stream_t stream);
int wdg_dense_to_csr_fill(const float *A, int64_t lda, int32_t N, int32_t M, const int32_t *rowptr, int32_t *col,
                          float *val, wdg_stream_t stream);
size_t wdg_scan_workspace_bytes(int64_t n);

/* ------------------------------------------------------------------ normalisation */
#define WDG_NORM_RW 0  /* D^-1 A                                                              */
#define WDG_NORM_SYM 1 /* D^-1/2 A D^-1/2 (row-sum degree on both sides)                       */
#define WDG_PREC_F32 0 /* coefficient arithmetic in fp32: utils/util_funcs.py:29-36,365-380   */
#define WDG_PREC_F64 1 /* in fp64, cast at the end: utils/util_funcs.py:383-390,418-426,:402  */

/*
 * Row sums / counts and the normalisation coefficient d_i (1/rowsum or rowsum^-1/2; inf -> 0; in the
 * F64 path rowsum==0 -> 1).  Any of rowsum / cnt / dinv_f32 / dinv_f64 may be NULL.
 * The row sum is an fp64 sum; rowsum is its fp32 rounding.  F32: 1.0f / s or 1.0f / sqrtf(s) on s = (float)sum, dinv_f64 the same
 * number; F64: 1.0 / sum or 1.0 / sqrt(sum) (two correctly rounded operations: within a last bit of pow(sum, -0.5)), dinv_f32 its
 * fp32 rounding.  A NaN entry or, for SYM, a negative sum makes that row's coefficient NaN and no other's.
 * replaces: the degree part of normalize, normalize_tensor, row_normalized_adjacency,
 *           sys_normalized_adjacency (utils/util_funcs.py:31-33,367-370,376-377,386,421-424).
 */
int wdg_degree_norm(const int32_t *rowptr, const float *val, int32_t N, int mode, int prec, float *rowsum,
                    int32_t *cnt, float *dinv_f32, double *dinv_f64, wdg_stream_t stream);
/* Materialise A_hat's values exactly as the reference would: out[p] = d_i * val[p] (* d_col[p] for SYM).
 * SYM reads dinv[col[p]] from the N row coefficients: every column must be < N, i.e. the pattern square.  The call does not know the
 * column count and cannot check it: graphs.normalise_values refuses a pattern of another shape before it launches. */
int wdg_normalise_values(const int32_t *rowptr, const int32_t *col, const float *val, int32_t N, int mode, int prec,
                         const float *dinv_f32, const double *dinv_f64, float *out, wdg_stream_t stream);
/*
 * Dense row scaling Y = X / rowsum(X) (inf -> 0), or with use_abs the torch F.normalize(p=1) form.
 * replaces: preprocess_features utils/util_funcs.py:39-46; normalize_tensor(features) :365-373
 *           (which the reference does as an O(N^2 F) diag matmul); f.normalize homophily_tests.py:94.
 */
int wdg_row_l1_normalise_f32(const float *X, int64_t ldx, float *Y, int64_t ldy, int32_t N, int32_t F, int use_abs,
                             wdg_stream_t stream);
/*
 * Bit-packed 0/1 feature rows (the graph container of graph_io.py: bit j of word w = feature 32 w + j) -> dense fp32
 * [N, F]; normalise != 0 fuses the row-L1 scaling above (each set bit becomes 1 / #set bits of its row, empty rows stay 0).
 * replaces: th.FloatTensor(features) of the bag-of-words datasets utils/util_funcs.py:339 (+ preprocess_features :39-46).
 */
int wdg_unpack_bits_f32(const uint32_t *words, int64_t ldw, int32_t N, int32_t F, int normalise, float *out, int64_t ldo,
                        wdg_stream_t stream);

/*
 * A LIST of compact feature matrices -> dense fp32 rows in one launch: sparse rows (CSR) or the container's bit-packed words,
 * optionally with the row-L1 scaling of wdg_row_l1_normalise_f32 fused (csrc/features.hip).
 * replaces: th.FloatTensor(features) / .todense() utils/util_funcs.py:339; preprocess_features utils/util_funcs.py:39-46;
 *           f.normalize homophily_tests.py:94 - for feature matrices that are mostly zeros, without a dense host copy.
 * For every job, every element of out[0:n_rows, 0:n_feat] is written (zeros included: no memset first) and nothing outside it:
 * columns n_feat .. ldo - 1 keep what they held, so a job may expand straight into a wider operand.  ldo and n_feat need not be
 * multiples of 4.
 *   kind WDG_FEAT_CSR:  rowptr int32 [n_rows + 1], col int32 [nnz], val fp32 [nnz] or NULL (= 1.0).  Columns sorted and unique
 *        within a row.  An entry whose column is not in [0, n_feat) is skipped - never stored through, left out of the row sum.
 *   kind WDG_FEAT_BITS: words uint32 [n_rows, ldw], bit j of word w = feature 32 w + j (graph_io.py); bits past n_feat are padding.
 *   normalise WDG_FEAT_NORM_SUM: wdg_row_l1_normalise_f32(use_abs = 0) of the expanded matrix - the row sum in fp64, s = (float)sum,
 *        r = 1.0f / s, inf -> 0, y = r * x;  WDG_FEAT_NORM_ABS: use_abs = 1 - s over |x|, y = x / fmaxf(s, 1e-12f).
 *        Bit-identical to that call where the fp64 row sum is exact in any order (0/1 features, fixed-point values), to fp64
 *        rounding of the sum otherwise (the entries are summed in another order).  Zeros are +0 also in a row of negative sum,
 *        where the dense call gives -0 (they compare equal).  WDG_FEAT_BITS equals wdg_unpack_bits_f32 bit for bit, either way.
 * max_rows / max_feat: the largest n_rows / n_feat of the table (0: nothing to do).  Any number of jobs (launched 65535 at a time).
 * wdg_features_image_floats: the floats of one row image of the CSR path - a wider row is written in several windows.
 */
#define WDG_FEAT_CSR 0
#define WDG_FEAT_BITS 1
#define WDG_FEAT_NORM_NONE 0
#define WDG_FEAT_NORM_SUM 1
#define WDG_FEAT_NORM_ABS 2
typedef struct wdg_feat_job {
    const int32_t *rowptr;  /* WDG_FEAT_CSR: [n_rows + 1] */
    const int32_t *col;     /* WDG_FEAT_CSR: [nnz] */
    const float *val;       /* WDG_FEAT_CSR: [nnz] or NULL = 1.0 */
    const uint32_t *words;  /* WDG_FEAT_BITS: [n_rows, ldw] */
    float *out;             /* [n_rows, ldo] */
    int64_t ldw;            /* words between consecutive rows, >= ceil(n_feat / 32) */
    int64_t ldo;            /* elements between consecutive output rows, >= n_feat */
    int32_t n_rows, n_feat;
    int32_t kind;           /* WDG_FEAT_CSR | WDG_FEAT_BITS */
    int32_t normalise;      /* WDG_FEAT_NORM_* */
} wdg_feat_job;
int32_t wdg_features_image_floats(void);
int wdg_features_expand_batched_f32(const wdg_feat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                    wdg_stream_t stream);

/* ------------------------------------------------------------------ aggregation (SpMM) */
/*
 * One aggregation problem:  Y[i,:] = row_scale[i] * sum_p val[p] * col_scale[col[p]] * X[col[p],:]
 * (val / row_scale / col_scale may each be NULL = 1).  rw: row_scale = d;  sym: row_scale = col_scale = d;
 * explicit A_hat: val only.  X is [n_cols, F] row-major with leading dimension ldx (elements), Y [n_rows, F].
 * The sum runs over the STORED entries p of row i: every entry point takes a row's entries in any order and adds a column that is
 * stored several times once per copy (the order only decides the rounding; tests/test_gpu_spmm_edges.py holds every kernel to it) -
 * with ONE condition, on an optional plan: a SELL-16 copy of more than one column block is built from rows in ascending column order.
 * replaces: torch.spmm / torch.mm(adj, X) - utils/homophily_metrics.py:192,199,200,234,235,299,315;
 *           utils/homophily_plot.py:196,246,320,336.
 */
#define WDG_SELL16_CONT (1 << 30) /* flag in the width word of a q_ext pair */
#define WDG_SELL16_SPLIT 1        /* wdg_spmm_job.q_flags */
#define WDG_BAND_HUB_ON_DEVICE (-1) /* wdg_spmm_job.band_n_hub: the kernel takes the count from band_cuts[8] */
#define WDG_SELL16_HALF 2         /* wdg_spmm_job.q_flags: offsets over 32-byte slab rows (wdg_sell16_row_bytes(n_cols) == 32) */
#define WDG_SELL16_X_TRANSPOSED 4 /* wdg_spmm_job.q_flags (the quad-row kernel only: jobs with a SELL-16 copy): X is given TRANSPOSED,
                                     [n_feat, n_cols] with leading dimension ldx - element (column j, feature f) at X[f ldx + j].  The
                                     second product of a propagated kernel, U = A_hat T^T (utils/homophily_metrics.py:234-235 by
                                     K(A_hat X) = A_hat K(X) A_hat^T), reads T where the first product wrote it */
typedef struct wdg_spmm_job {
    const int32_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *row_scale;
    const float *col_scale;
    const void *X; /* fp32, or bf16 for the *_bf16 entry points */
    float *Y;
    int64_t ldx, ldy;
    int32_t n_rows, n_cols, n_feat;
    int32_t reserved; /* must be 0 (bits 0 .. 3 are timing-only ablation switches of the diagnostics scripts: results are wrong when set) */
    /* (rounds 1-3 carried an optional SELL-64 copy here for the row-lane kernels; round 4 retired that family: sweep batches and
       small graphs run the quad-row kernel, single wide-feature graphs the band kernel, <= 8 features the narrow kernel, anything
       else the CSR slab / gather kernels) */
    /* optional SELL-16 copy of the same pattern (wdg_csr_to_sell16_*): enables the quad-row kernel (a quad of lanes per
       row, 16-row slices; graphs of up to 4 column blocks of 2528 columns); NULL = none */
    const int32_t *q_ext;  /* [q_n_blocks * q_n_entries + 1] pairs {first chunk, width | flags} per (block, entry), block-major;
                              an ENTRY is what a wave sweeps and stores in one go: a slice, or - split form - one of the
                              <= 32-entries-per-row pieces of a slice (WDG_SELL16_CONT: the piece continues the slice of
                              the entry before it; CONT with width 0: a ghost that pads a super-unit of four entries);
                              the trailing pair = {chunk count, q_n_entries | WDG_SELL16_CONT if split}                  */
    const int32_t *q_col;  /* chunk c = 256 ints: entry e (0..15) of slice row r at q_col[256 c + 16 r + e], value = 64 x
                              (column - block * q_block_cols) = byte offset of the source row in the staged slab block;
                              padding = 64 x q_block_cols (an all-zero row the kernel appends); a slice's chunks are
                              consecutive (a split entry covers two of them)                                             */
    const float *q_val;    /* same layout, needed when `val` is given (padding 0)                                        */
    const int32_t *q_perm; /* [16 ceil(n_rows/16)] slot -> row (rows by length, longest first; the slots that pad the last
                              slice repeat the last row: they store that row's sums a second time)                       */
    const int32_t *q_rows; /* [16 q_n_entries] the destination rows of every entry (q_perm expanded per entry)            */
    int32_t q_block_cols;  /* columns per block = wdg_sell16_block_cols(n_cols)                                          */
    int32_t q_n_blocks;    /* ceil(n_cols / q_block_cols), 1 .. 4                                                        */
    int32_t q_n_entries;   /* entries per column block, a multiple of 4 (four entries = a super-unit = what a wave is dealt) */
    int32_t q_flags;       /* WDG_SELL16_SPLIT: split form (one column block, every entry <= 32 entries per row)           */
    /* optional band plan of the same pattern (wdg_csr_band_plan): enables the band kernel of the single-graph entry points
       (a wave per row and band of 64..256 features gathered from L2; wide features, any skew, any column count); NULL = none */
    const int32_t *band_perm; /* [wdg_csr_band_perm_len(n_rows)] rows by length, longest first; the first band_n_hub are the hub rows */
    const int32_t *band_cuts; /* [24] cost cuts of the hub rows [0..8] and of the other rows [9..17]; [18], [19] = rows of more than
                                 2048 / 128 entries (the narrow kernel's row classes); the rest 0                                  */
    int32_t band_n_hub;       /* hub rows = rows of more than the plan's hub_len entries (256 unless wdg_csr_band_plan_hub named another;
                                 each is swept by a team of waves), a prefix of band_perm:
                                 the count, or WDG_BAND_HUB_ON_DEVICE = "read band_cuts[8]" for callers that never fetched it      */
    int32_t band_reserved;    /* 0 */
    int64_t y_group_stride;   /* 0: Y is row-major, element (row, f) at Y[row ldy + f].  > 0 (the quad-row kernel only: jobs with a
                                 SELL-16 copy through wdg_spmm_csr_* / wdg_spmm_quad_batched_f32): Y is TILED by 16-feature groups,
                                 element (row, f) at Y[(f / 16) y_group_stride + row ldy + f % 16] with ldy >= 16 - a workgroup (one
                                 feature group) then stores inside one contiguous region instead of 64-byte pieces ldy floats
                                 apart (round 4: the store-heavy k = 2 sweep launch 160 -> 133 us).  wdg_mlp2_job.a_group_stride
                                 reads such a matrix back; every other entry point wants row-major operands */
} wdg_spmm_job;

int wdg_spmm_csr_f32(const wdg_spmm_job *job_host, wdg_stream_t stream);
int wdg_spmm_csr_bf16(const wdg_spmm_job *job_host, wdg_stream_t stream);
/*
 * Many independent graphs in ONE launch (the homophily sweep, synthetic_plot.py:64-109).
 * `jobs_dev` is a device array of n_jobs descriptors; max_rows/max_cols/max_feat bound the job shapes
 * (needed on the host to size the grid and LDS without reading the table back).
 * Jobs are started in table order by persistent workgroups: put the jobs with the most stored entries first
 * so that no long job starts last (results do not depend on the order).
 * This entry runs the CSR families (LDS column slab, row gather); sweep batches take wdg_spmm_quad_batched_f32 /
 * wdg_spmm_narrow_batched_f32 below.
 */
#define WDG_SPMM_ANY_VAL 2  /* some job has explicit values (a SELL-16 copy then carries q_val) */
#define WDG_SPMM_DMA_OK 4   /* every job: X and Y 16-byte aligned, ldx, ldy and n_feat multiples of 4, col_scale NULL (16-byte
                               loads and stores throughout: what the quad-row kernel's pipelined loop needs) */
#define WDG_SPMM_SMALL_OFFSETS 8 /* every job: n_rows x ldy < 2^30 elements, fewer than 2^22 index chunks (byte offsets into Y and
                                   into q_col / q_val fit 32 bits) and a SELL-16 copy in split form (WDG_SELL16_SPLIT): with
                                   WDG_SPMM_DMA_OK the quad-row kernel's pipelined loop */
#define WDG_SPMM_ANY_COL_SCALE 16 /* some job has a column scale (wdg_spmm_narrow_batched_f32 gathers it per entry) */
#define WDG_SPMM_HALF_SLAB 32 /* wdg_spmm_quad_batched_f32: EVERY job has 2529 .. 5056 columns, i.e. a SELL-16 copy over 32-byte
                                 slab rows (WDG_SELL16_HALF); a table must not mix such jobs with others */
int wdg_spmm_batched_f32(const wdg_spmm_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                         int32_t max_feat, int flags, wdg_stream_t stream);
/* Which kernel family a batch of n_jobs such shapes dispatches to behind wdg_spmm_batched_f32 / wdg_spmm_csr_* without SELL-16 copy
 * or band plan (0 = LDS column-slab, 1 = row gather); *slab_out / *threads_out = its template parameters; for tests/bench. */
int wdg_spmm_plan(int32_t n_jobs, int32_t max_rows, int32_t max_cols, int32_t n_feat, int flags, int *slab_out,
                  int *threads_out);

/*
 * CSR -> SELL-16 (the index layout of the quad-row kernel, csrc/sell16.h; built by csrc/sell16.hip): rows sorted by length (q_perm[slot] = row),
 * slices of 16 slots, columns cut into ceil(n_cols / B) blocks of B = wdg_sell16_block_cols(n_cols) <= 2528 (what one
 * 16-feature slab of X occupies in LDS), entries in chunks of 16 per row.  Inside a (row, block) segment the entries are
 * stored in a bank-aware order (the four rows an LDS service group reads together get columns of different classes mod 4),
 * which fixes the order of the row's sum.  Graphs in split form get the CONFLICT-FREE order (round 4): the fill also decides
 * which rows of a slice share a service group - it PERMUTES q_rows inside the slice's entries - and reads a shorter row's
 * padding from one of four zero rows (offsets 64 (B + c), c = 0..3: the kernel appends four zero rows to the slab) at
 * whichever step keeps the group conflict-free; other graphs keep round 2's greedy order (padding = offset 64 B, at the end) -
 * among them the graphs of 2529 .. 5056 columns (32-byte slab rows, wdg_sell16_row_bytes: the greedy order over their EIGHT
 * bank windows, rows 0-7 / 8-15 of a slice read together; padding = offset 32 B).
 * WDG_SELL_ORDER in the environment of the fill call: 0 = column order (the sequential CSR order), 1 = greedy everywhere.
 * The slices are then laid out as ENTRIES, four per super-unit (see
 * wdg_spmm_job.q_ext): graphs with one column block and at most 128 entries per row and block in split form.
 * Two calls: count fills q_perm (16 ceil(N/16) entries), q_ext and q_rows - sized for M = wdg_sell16_max_entries(N) entries per
 * block: q_ext 2 (n_blocks M + 1) ints, q_rows 16 M ints; the pair {chunk count, entries per block | WDG_SELL16_CONT if
 * split} is stored behind the entries AND at pair index n_blocks M, where the caller reads it back to size q_col / q_val:
 * 256 entries per chunk PLUS two chunks of slack that the kernel may read but never uses; then fill.  One-time per graph.
 * Graphs of SEVERAL column blocks (more than 5056 columns): both calls cut a row at the block boundaries by binary search, so every
 * row's columns must ascend (equal neighbours allowed); rows of one-block graphs may be stored in any order.  CsrGraph.ensure_quad
 * checks it and leaves other graphs to the CSR and band kernels.
 */
int32_t wdg_sell16_block_cols(int32_t n_cols);
/* Bytes of a slab row the copy's offsets are scaled by: 64 (16 features of X per workgroup), or 32 for graphs of 2529 .. 5056
 * columns (HALF slabs, round 4: ONE column block of 8-feature rows - the whole graph's X[:, f0 : f0 + 8] in the 160 KiB of LDS, a
 * quad of lanes reads a row with ds_read_b64 - instead of two blocks of 16-feature rows staged one after the other; such graphs
 * are in split form like the smaller ones and run the same pipelined loop). */
int32_t wdg_sell16_row_bytes(int32_t n_cols);
int64_t wdg_sell16_max_entries(int32_t N);
size_t wdg_sell16_workspace_bytes(int32_t N, int32_t n_cols);
int wdg_csr_to_sell16_count(const int32_t *rowptr, const int32_t *col, int32_t N, int32_t n_cols, int32_t *q_perm,
                            int32_t *q_ext, int32_t *q_rows, void *workspace, size_t workspace_bytes, wdg_stream_t stream);
int wdg_csr_to_sell16_fill(const int32_t *rowptr, const int32_t *col, const float *val, int32_t N, int32_t n_cols,
                           int32_t *q_rows /* in / out: see above */, const int32_t *q_ext, int32_t n_entries, int32_t *q_col,
                           float *q_val, wdg_stream_t stream);

/*
 * The same build for a table of graphs (a sweep shard): count = sort + widths + scan / pack + entries of every graph in four
 * launches, fill in one; between the two the caller reads back every graph's {chunk count, entries | split} pair (ONE copy
 * of the q_ext tails for the whole shard), sizes a pooled q_col / q_val and stores the pointers into the table (q_col == NULL:
 * no copy wanted for that graph).  Buffers per job are sized as for the single-graph calls with the job's own n_rows / n_cols;
 * workspace: wdg_sell16_workspace_bytes(n_rows, n_cols) bytes per job.  Graphs of more than 16 384 rows (unsorted layout)
 * take the single-graph calls.  max_rows / max_cols: the largest n_rows / n_cols of the table (they size the grids).
 */
typedef struct wdg_sell16_job {
    const int32_t *rowptr;
    const int32_t *col;
    const float *val;      /* NULL: pattern only */
    int32_t *q_perm, *q_ext, *q_rows;
    int32_t *q_col;        /* fill: NULL = skip this graph */
    float *q_val;          /* fill: NULL = no values */
    void *workspace;
    int32_t n_rows, n_cols;
} wdg_sell16_job;
int wdg_csr_to_sell16_count_batched(const wdg_sell16_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                    wdg_stream_t stream);
int wdg_csr_to_sell16_fill_batched(const wdg_sell16_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                   wdg_stream_t stream);

/*
 * Band plan of a CSR pattern (the row schedule of the band kernel, csrc/spmm_band.hip; the single-graph entry points
 * wdg_spmm_csr_f32 run that kernel for fp32 X of >= 16 features when the job carries the plan and no SELL-16 copy in split
 * form): band_perm = the rows by length, longest first (<= 16 384 rows: ties by row index; more: rows of equal length in no
 * particular order - the order only schedules, every row's sum has a fixed order), wdg_csr_band_perm_len(N) ints;
 * band_cuts = 24 ints (layout: wdg_spmm_job.band_cuts); the number of hub rows - rows with more than 256 entries (wdg_csr_band_plan_hub: hub_len entries), a prefix of
 * band_perm - is band_cuts[8] and STAYS ON THE DEVICE (round 5: the call used to read it back and synchronise the stream; now it
 * only enqueues, like every other entry point): a job passes band_n_hub = WDG_BAND_HUB_ON_DEVICE and the kernel reads the word,
 * or the caller copies band_cuts[8] back whenever it wants the number.  One-time per graph; nothing depends on the feature width.
 * Replaces, with wdg_spmm_csr_f32, `torch.spmm(adj, features)` of utils/homophily_metrics.py:199-200,234-235 for single
 * wide-feature graphs (the full feature matrix of Cora / squirrel / chameleon as classifier_based_performance_metric passes it).
 */
size_t wdg_csr_band_plan_workspace_bytes(int32_t N);
int32_t wdg_csr_band_perm_len(int32_t N);
int wdg_csr_band_plan(const int32_t *rowptr, int32_t N, int32_t *band_perm, int32_t *band_cuts, void *workspace,
                      size_t workspace_bytes, wdg_stream_t stream);
/* The same plan with the HUB THRESHOLD named by the caller (0: the default, 256): rows longer than hub_len are swept by the four waves of
 * a workgroup, the others by one wave each.  A launch ends with its longest single-wave row, so a graph of short rows with a few
 * long ones is better off with a lower threshold (Cora, mean 4.9 entries per row, longest 169: 22 -> 17.5 us at 32); the Python side
 * passes 6 x the mean row length clamped to 32 .. 192 (squirrel: 186 -> 176 us at 192).  Any threshold computes every row's sum in a fixed order (a hub row: its four
 * pieces in piece order).
 * replaces: the same `torch.spmm(adj, features)` call sites as wdg_csr_band_plan (utils/homophily_metrics.py:199-200,234-235). */
int wdg_csr_band_plan_hub(const int32_t *rowptr, int32_t N, int32_t hub_len, int32_t *band_perm, int32_t *band_cuts, void *workspace,
                          size_t workspace_bytes, wdg_stream_t stream);

/*
 * The aggregation for ONE graph with at most 8 features (csrc/spmm_narrow.hip; config C5: twitch-gamers scale with 7 bf16
 * features): the job carries a band plan; `workspace` (wdg_spmm_narrow_workspace_bytes(n_rows, n_cols) bytes) receives the
 * packed sources - column scale, conversion and padding once per column - and every stored entry then costs one gather of
 * wdg_spmm_narrow_col_bytes(n_feat, x_is_bf16, has_col_scale) bytes: 16 when the job has at most four features (four fp32,
 * cs[c] X[c, 0..3]) or bf16 sources and no column scale (the row's eight bf16 as they are: exact), else 32 (eight fp32,
 * cs[c] X[c, 0..7]).  When the packed table exceeds what an XCD's L2 holds (wdg_spmm_narrow_parts(n_cols, col_bytes) = 2, 4
 * or 8 > 1) the columns are cut into that many ranges, each swept by its own XCDs, and the partial rows are summed in range
 * order: the call then needs `part_ptr` = the split positions of every row ([n_rows x (parts - 1)] ints, filled once per
 * graph and `parts` by wdg_spmm_narrow_plan; NULL when parts is 1).  Sums in a fixed order (lanes split a row's entries,
 * fixed butterfly, parts ascending).
 * Replaces `torch.spmm(adj, label_onehot)` utils/homophily_metrics.py:199 and the SGC-1 aggregation on large graphs.
 */
int32_t wdg_spmm_narrow_col_bytes(int32_t n_feat, int32_t x_is_bf16, int32_t has_col_scale);
int32_t wdg_spmm_narrow_parts(int32_t n_cols, int32_t col_bytes);
size_t wdg_spmm_narrow_workspace_bytes(int32_t n_rows, int32_t n_cols);
int wdg_spmm_narrow_plan(const int32_t *rowptr, const int32_t *col, int32_t N, int32_t n_cols, int32_t parts, int32_t *part_ptr,
                         wdg_stream_t stream);
int wdg_spmm_narrow_f32(const wdg_spmm_job *job_host, const int32_t *part_ptr, void *workspace, size_t workspace_bytes,
                        wdg_stream_t stream);
int wdg_spmm_narrow_bf16(const wdg_spmm_job *job_host, const int32_t *part_ptr, void *workspace, size_t workspace_bytes,
                         wdg_stream_t stream);

/*
 * Many graphs with at most 8 features each in one launch (the sweep's logits aggregation A_hat Z with C classes): plain CSR,
 * 16 lanes per row, sources read IN PLACE - every job's X must be 16-byte aligned with ldx a multiple of 4 and >= 4 (>= 8
 * for EVERY job of a table with max_feat > 4, a job of fewer features included: the launch picks its width from max_feat and
 * then reads two float4 of every source row of every job, else one).  flags: WDG_SPMM_ANY_VAL,
 * WDG_SPMM_ANY_COL_SCALE, WDG_NARROW_SLAB_OK.  Sums in a fixed order (lane layout + fixed butterfly).
 * WDG_NARROW_SLAB_OK (the entry cannot see n_cols: it is in the device table) promises that EVERY job is pattern-only (no values, no
 * column scale) and that its sources fit one LDS slab: n_cols x (max_feat > 4 ? 32 : 16) bytes <= WDG_NARROW_SLAB_BYTES.  Such a
 * table runs on a kernel whose workgroups copy their job's source rows into LDS and gather from there - the same sums in the same
 * order, bit for bit (WDG_NARROW_SLAB=0 in the environment: the in-place kernel; a table flagged by mistake gets wrong numbers).
 * wdg_spmm_narrow_slab_launches: how many launches of this process took the slab kernel (tests ask which kernel ran).
 */
#define WDG_NARROW_SLAB_OK 64
#define WDG_NARROW_SLAB_BYTES (72 * 1024) /* two slabs fit the 160 KB of a CU's LDS */
int wdg_spmm_narrow_batched_f32(const wdg_spmm_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat, int flags,
                                wdg_stream_t stream);
int64_t wdg_spmm_narrow_slab_launches(void);

/*
 * The batched aggregation on the quad-row kernel (every job carries its SELL-16 copy).  The caller lays the jobs'
 * super-units (four entries of the SELL-16 copy: what a wave is dealt) out as one tape (jobs in table order, job j
 * contributes q_n_entries_j / 4 of them) and cuts it into n_segments
 * (a multiple of 8) segments of about equal cost; segment s consists of the phases items[seg_ptr[s] .. seg_ptr[s + 1]):
 * a phase is a run of consecutive jobs that aggregate the SAME X (same X, ldx, n_cols, n_feat, col_scale) and the unit
 * range [unit_begin, unit_end) of their concatenated units it covers.  XCD x of the chip processes segments
 * x S .. x S + S - 1 (S = n_segments / 8), one workgroup per (segment, 16-feature group); a workgroup stages X[:, group]
 * once per phase.  Graphs of more than 2528 columns (several column blocks): at most 32 super-units per item.
 * replaces: the same torch.spmm / torch.mm(adj, X) call sites as wdg_spmm_batched_f32, for the loop of
 * synthetic_plot.py:64-109 (every graph of a sweep shard in one launch).
 */
typedef struct wdg_spmm_item {
    int32_t first_job, n_jobs;    /* jobs [first_job, first_job + n_jobs) of the table: they aggregate the same X */
    int32_t unit_begin, unit_end; /* super-units (64 rows) of the jobs' concatenated super-units covered by this item */
    int32_t flags, reserved;      /* 0 */
} wdg_spmm_item;
int wdg_spmm_quad_batched_f32(const wdg_spmm_job *jobs_dev, int32_t n_jobs, const wdg_spmm_item *items_dev,
                              const int32_t *seg_ptr_dev, int32_t n_segments, int32_t max_cols, int32_t max_feat, int flags,
                              wdg_stream_t stream);
/* The same launch; wg_clock_dev (may be NULL): [2 x wdg_spmm_quad_workgroups(n_segments, max_feat, flags)] 64-bit words that receive
 * every workgroup's start and end on the device's 100 MHz clock (workgroup b belongs to XCD b % 8 and serves the segments
 * of that XCD): the caller can balance the segments by what they really cost (ops.SpmmBatch.balance). */
int wdg_spmm_quad_batched_clocked_f32(const wdg_spmm_job *jobs_dev, int32_t n_jobs, const wdg_spmm_item *items_dev,
                                      const int32_t *seg_ptr_dev, int32_t n_segments, int32_t max_cols, int32_t max_feat,
                                      int flags, uint64_t *wg_clock_dev, wdg_stream_t stream);
int32_t wdg_spmm_quad_workgroups(int32_t n_segments, int32_t max_feat, int flags);
/* diagnostics: one thread stores the device's 100 MHz clock to out_dev, in stream order */
int wdg_debug_clock(uint64_t *out_dev, wdg_stream_t stream);

/* ------------------------------------------------------------------ edge / label statistics */
/*
 * One pass over the stored pattern P of a CSR adjacency:
 *   totals[0]=|P|  [1]=#{y_u==y_v}  [2]=#{y_u>=0,y_v>=0}  [3]=matches among [2]
 *   totals[4]=|P'| (non-loop)  [5]=matches among P'
 *   row_nnz[u]=|P_u|  row_nnz_noself[u]=|P'_u|  row_match_noself[u]=#{v in P'_u : y_v==y_u}
 *   compat[i*C+j]=#{(u,v) in P' : y_u=i, y_v=j, both>=0}   classdeg[c]=sum_{y_u=c}(|P_u|-1)
 * Labels outside [0, C): "y_u == y_v" compares the stored int32 values whatever they are (two labels of -1 match, two of C match),
 * and totals[2] / totals[3] ask only for the sign - a label >= C counts there like any other non-negative one.  compat and classdeg
 * hold the classes [0, C) alone: an entry with either label outside [0, C) is in no cell of compat, a row whose label is outside
 * [0, C) is in no element of classdeg (a negative label and one >= C are the same to them).  A row without entries adds -1 to
 * classdeg of its class.  C = 0: compat and classdeg are not touched and may be NULL.
 * All outputs are exact integers (bit-exact parity).  Any per-row output may be NULL.
 * replaces: utils/homophily_metrics.py:50-56 (edge), :73-78 (node), :89-101 (compat), :127-145
 *           (class_distribution); dense twins utils/homophily_plot.py:48-51,85-99,111-122,151-170.
 */
int wdg_edge_label_stats(const int32_t *rowptr, const int32_t *col, const int32_t *labels, int32_t N, int32_t C,
                         int64_t *totals, int32_t *row_nnz, int32_t *row_nnz_noself, int32_t *row_match_noself,
                         int64_t *compat, int64_t *classdeg, wdg_stream_t stream);

typedef struct wdg_stats_job {
    const int32_t *rowptr;
    const int32_t *col;
    const int32_t *labels;
    int64_t *totals;   /* [6]   */
    int64_t *compat;   /* [C*C] */
    int64_t *classdeg; /* [C]   */
    int32_t *row_nnz, *row_nnz_noself, *row_match_noself; /* [N] each, may be NULL */
    int32_t n_rows, n_classes;
} wdg_stats_job;
/* Batched form: outputs must be zeroed by the caller (one memset over a pooled buffer) - totals, compat and classdeg are ADDED to
 * (a second launch without the memset doubles them), the per-row arrays are written.  Jobs may differ in n_rows (0 included) and in
 * n_classes; max_rows / max_classes are the largest of the table.  n_jobs == 0 or max_rows == 0: nothing is launched or written. */
int wdg_edge_label_stats_batched(const wdg_stats_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_classes,
                                 wdg_stream_t stream);

/*
 * The six scalars of a sweep step for every job of a shard, from the pooled counters of wdg_edge_label_stats_batched (totals
 * [n_jobs, 6], rows [n_jobs, 3, max_rows] = row_nnz / row_nnz_noself / row_match_noself padded with zeros, compat [n_jobs, C, C],
 * classdeg [n_jobs, C]), the LAS counts ([n_jobs, 2]) and node counts ([n_jobs] fp32) and the class proportions ([n_jobs, C]):
 * out[j] = {edge homophily, node homophily, class homophily, adjusted homophily, label informativeness, soft LAS} in fp32.
 * replaces: the tails of edge_homophily / node_homophily / our_measure / adjusted_homo / label_informativeness / similarity as
 *           synthetic_plot.py:94-106 calls them (utils/homophily_plot.py:43-160): fp32 arithmetic on integer counters, NaN class
 *           terms skipped, zeros -> 1e-8.  Deterministic (fixed summation order).  1 <= C <= 32.
 * Degenerate jobs get what IEEE arithmetic gives these formulas, and leave the other jobs of the table alone:
 *   totals[4] == 0 (no non-loop entry; totals[5] is 0 then): edge = 0 / 0 = NaN, and with it adjusted homophily;
 *   no non-empty row: node = 0 / 0 = NaN;
 *   classdeg all zero: p = 0 / 0 = NaN (a NaN is not the zero that 1e-8 stands in for): adjusted homophily and label informativeness NaN;
 *   C == 1: class homophily divides by C - 1 = 0 (NaN for a zero sum, +inf for a positive one); p = 1, so adjusted homophily is
 *           (edge - 1) / 0 = -inf (NaN when edge == 1) and label informativeness 2 - 0 / 0 = NaN.
 */
int wdg_sweep_scalars_f32(const int64_t *totals, const int32_t *rows, const int64_t *compat, const int64_t *classdeg,
                          const int64_t *las_counts, const float *las_n, const float *class_prop, int32_t n_jobs, int32_t max_rows,
                          int32_t n_classes, float *out, wdg_stream_t stream);

/*
 * A nine-scalar shard's device results gathered into ONE fp64 vector (one launch, then one copy to the host):
 *   out = [scalars (n_scalars fp32, widened) | ge_mean (n_ge fp64) | kr_correct[i] / kr_n_val[i] (the fp32 quotient, widened; n_kr) |
 *          #problems with flags bit 1 (deflated), #with bit 0 (ridged), #with correct < 0 (refused)]      (n_scalars + n_ge + n_kr + 3)
 * replaces: the result bookkeeping of the sweep loop - `X_results[j] = accuracy(...)`, `G_results[j] = ...` utils/homophily_metrics.py:
 *           293-297 and the scalar appends of synthetic_plot.py:94-109 - as one device pass instead of a dozen library launches.
 */
int wdg_sweep_pack_f64(const float *scalars, int32_t n_scalars, const double *ge_mean, int32_t n_ge, const int32_t *kr_correct,
                       const int32_t *kr_flags, const float *kr_n_val, int32_t n_kr, double *out, wdg_stream_t stream);

/*
 * Batched Gaussian naive Bayes: per problem, fit on the train rows of a feature matrix and predict its validation rows - the GNB branch
 * of the classifier-based performance metric, every (epoch, feature matrix) problem of a call in one call here (three launches).
 * The statistics are scikit-learn's on a float32 matrix, bit for bit: per class present among the train rows the fp32 mean and
 * population variance of every feature by SEQUENTIAL fp32 sums over the train rows IN THE ORDER OF `train` (the reference indexes with
 * boolean masks: ascending node ids), epsilon = float32(1e-9) x the largest fp32 variance of all train rows; the joint log likelihood
 * in fp64, first maximum over the present classes (csrc/gnb.hip: what can differ from numpy is the rounding of two fp64 sums over the
 * features).  correct_out = validation rows whose predicted class is their label; pred (optional) = the predicted class per validation
 * row.  Classes 0 .. n_classes - 1, n_classes <= 16; labels outside are the caller's error.  A problem with n_train < 1 predicts nothing
 * (correct 0, pred untouched).  ws: wdg_gnb_workspace_bytes(F, n_classes) bytes per problem, 256-byte aligned.
 * replaces: `GaussianNB().fit(X[idx_train], labels_sample[idx_train])` / `.predict(X[idx_val])` for X and X_agg and the two accuracies
 *           (utils/homophily_metrics.py:296-312, utils/homophily_plot.py:317-333) inside the epoch loop of
 *           classifier_based_performance_metric (utils/homophily_metrics.py:260-349).
 */
typedef struct {
    const float *X;          /* [n, F] fp32 row-major, leading dimension ldx */
    const int32_t *train;    /* [n_train] row ids, in the order the statistics are summed in */
    const int32_t *val;      /* [n_val] row ids */
    const int32_t *labels;   /* [n] class of every row */
    void *ws;                /* wdg_gnb_workspace_bytes(F, n_classes) bytes */
    int32_t *correct;        /* out: hits among the validation rows (NULL: not wanted) */
    int32_t *pred;           /* out [n_val]: predicted class (NULL: not wanted) */
    int64_t ldx;
    int32_t n_train, n_val, F, n_classes;
} wdg_gnb_job;
size_t wdg_gnb_workspace_bytes(int32_t n_feat, int32_t n_classes);
int wdg_gnb_batched_f32(const wdg_gnb_job *jobs_dev, int32_t n_jobs, int32_t max_feat, int32_t max_val, int32_t max_classes,
                        wdg_stream_t stream);

/* ------------------------------------------------------------------ support vector classifiers (the svm_* base classifiers) */
/*
 * Batched C-SVC over a precomputed Gram: per problem, fit a one-vs-one support vector classifier on the train rows and predict the
 * validation rows - the svm_rbf / svm_poly / svm_linear branches of the classifier-based performance metric, every (epoch, feature
 * matrix) problem of a call in one call here (two launches: the solver, a wave per pair of classes; the predictor).
 * The arithmetic is libsvm's C-SVC as scikit-learn calls it (tol 1e-3, no class weights), restated in tests/_svm_ref.py:
 *   kernel entry  from G = 2 G_half: linear G_ij; poly (gamma G_ij)^degree (coef0 = 0); rbf exp(-gamma (G_ii + G_jj - 2 G_ij)) with
 *                 G_ii = norm2[i]; evaluated in fp64 and rounded to fp32 for the solver (libsvm's kernel cache), fp64 diagonal,
 *                 gradient and alphas; gamma <= 0: scikit-learn's 'scale', 1 / (F var) over all elements of the train rows, formed in
 *                 fp64 from row_sum and norm2;
 *   pair (p, q)   p < q among the classes present in the train rows: the train rows of p as +1, then those of q as -1, in the order
 *                 of `train` (ascending ids, as boolean masks give them);
 *   solver        SMO with second-order working-set selection (the LAST maximiser / minimiser wins a tie), libsvm's box clipping,
 *                 stop at Gmax + Gmax2 < 1e-3 or after max_iter iterations of a pair (flag bit 0); no shrinking;
 *   rho           mean of y G over the free alphas, without any the midpoint of the two bounds;
 *   prediction    dec = sum_t alpha_t y_t K(v, t) - rho per pair in fp64 (unrounded kernel entries); > 0 votes p, otherwise q; the
 *                 first class with the most votes.
 * dec: [n_val, n_classes (n_classes - 1) / 2] fp64; a row's first P (P - 1) / 2 entries are the pairs of the P PRESENT classes in
 * libsvm's order (0,1), (0,2) .. (P-2,P-1) over the present classes in ascending order, the rest is not written.
 * info: {iterations of all pairs, the largest count of a pair, support vectors, flags}; flags bit 0: a pair stopped at max_iter
 * before it converged; bit 1: fewer than two classes among the train rows - nothing is predicted, correct = 0.
 * Limits: n_train <= 1024, n_classes <= 16, n_jobs <= 65535; labels in [0, n_classes).  ws: wdg_svm_workspace_bytes(n_train,
 * n_classes) bytes per problem, 256-byte aligned (the solver leaves the coefficient table there: (n_classes - 1) n_train fp64
 * coefficients, a rho and an iteration count per pair).
 * replaces: `svm.SVC(kernel=.., ..).fit(X[idx_train], labels_sample[idx_train])` / `.predict(X[idx_val])` for X and X_agg and the two
 *           accuracies (utils/homophily_metrics.py:313-333, utils/homophily_plot.py:334-354) inside the epoch loop of
 *           classifier_based_performance_metric (utils/homophily_metrics.py:260-349).
 */
#define WDG_SVM_LINEAR 0
#define WDG_SVM_POLY 1
#define WDG_SVM_RBF 2
#define WDG_SVM_FLAG_MAX_ITER 1
#define WDG_SVM_FLAG_ONE_CLASS 2
typedef struct {
    const float *G_half;     /* [n, n] fp32, leading dimension ldk: K_linear of wdg_gram_map_batched_f32 = G / 2 exactly */
    const float *norm2;      /* [n] the Gram's diagonal G_ii */
    const double *row_sum;   /* [n] sum of every feature row in fp64 (NULL: allowed unless gamma <= 0 with a poly / rbf kernel) */
    const int32_t *train;    /* [n_train] row ids, ascending */
    const int32_t *val;      /* [n_val] row ids */
    const int32_t *labels;   /* [n] class of every row */
    void *ws;                /* wdg_svm_workspace_bytes(n_train, n_classes) bytes */
    int32_t *correct;        /* out: hits among the validation rows */
    int32_t *pred;           /* out [n_val]: predicted class (NULL: not wanted) */
    double *dec;             /* out [n_val, n_classes (n_classes - 1) / 2]: pairwise decision values (NULL: not wanted) */
    int32_t *info;           /* out [4]: total iterations, largest iteration count of a pair, support vectors, flags */
    int64_t ldk;
    double C;                /* box constraint */
    double gamma;            /* <= 0: 'scale' */
    int32_t kernel, degree;  /* WDG_SVM_LINEAR / _POLY / _RBF; degree of the polynomial */
    int32_t max_iter;        /* iteration cap per pair */
    int32_t n_train, n_val, n_classes;
    int32_t F;               /* features per row (for gamma = 'scale') */
    int32_t reserved;
} wdg_svm_job;
size_t wdg_svm_workspace_bytes(int32_t n_train, int32_t n_classes);
int wdg_svm_batched_f32(const wdg_svm_job *jobs_dev, int32_t n_jobs, int32_t max_train, int32_t max_val, int32_t max_classes,
                        wdg_stream_t stream);

/* ------------------------------------------------------------------ per-edge cosine (SDDMM) */
/*
 * out[i] = cos(x_u, x_v) for stored entry e_i = (u, v) (e_i = entries[i], or i when entries == NULL); NaN -> 0;
 * self loops give 0 when skip_self.  Replaces the dense N x N sklearn cosine matrix masked by the adjacency in
 * generalized_edge_homophily (utils/homophily_metrics.py:164-187, utils/homophily_plot.py:56-78): only the pairs
 * that are edges get computed.
 */
int wdg_edge_cosine_f32(const int32_t *rowptr, const int32_t *col, const int32_t *entries, int64_t n_entries,
                        const float *X, int64_t ldx, int32_t N, int32_t F, int skip_self, float *out,
                        wdg_stream_t stream);

/* ------------------------------------------------------------------ label-aggregation similarity */
/*
 * W[i,c] = sum_{j: y_j=c} <H_i, H_j>  computed as H (H^T Y) with fp64 accumulation (never forms n x n),
 * optionally restricted to the rows listed in `rows` (idx_train).  W_out is [n, C] fp64.
 * Then counts: count_out[0] = #{i : soft LAS ratio >= 1}, count_out[1] = #{i : argmax_c W[i,c] == y_i}.
 * replaces: utils/homophily_metrics.py:192-206,216-220,226; utils/homophily_plot.py:196-226,232.
 * `labels` is indexed by node id (full length); `rows` (int32[n], may be NULL = identity) selects the sample.
 * A selected row whose label lies outside [0, C) belongs to no class: it adds to no column of W, still counts in n, and is
 * never a hit of either count.
 * workspace: wdg_las_workspace_bytes(n, F, C).
 */
size_t wdg_las_workspace_bytes(int32_t n, int32_t F, int32_t C);
int wdg_las_f32(const float *H, int64_t ldh, const int32_t *labels, const int32_t *rows, int32_t n, int32_t F,
                int32_t C, double *W_out, int64_t *count_out, void *workspace, size_t workspace_bytes,
                wdg_stream_t stream);

/* Many problems in one launch (every graph of a sweep batch); count_out is reset by the call itself - a job with n == 0
 * inside a non-empty table gets {0, 0} as well (its H, labels, W_out and workspace are not touched). */
typedef struct wdg_las_job {
    const float *H;
    const int32_t *labels;
    const int32_t *rows;  /* NULL = identity */
    double *W_out;        /* [n, C] or NULL */
    int64_t *count_out;   /* [2] */
    void *workspace;      /* wdg_las_workspace_bytes(n, F, C) bytes, private to this job */
    int64_t ldh;
    int32_t n, F, C, reserved;
    /* Optional: the integer counters of wdg_edge_label_stats for the SAME graph, derived from H instead of a second pass over
     * the edges.  Valid when H = diag(row_scale) P onehot(labels) (F == C, rows == NULL) for the 0/1 pattern P the counters
     * describe, P holds exactly one diagonal entry per row (A + I), every label lies in [0, C) and the launch takes the fused
     * one-workgroup path (wdg_las_fused_eligible): then P onehot = H / row_scale holds every node's neighbour-class counts -
     * exact integers after rounding (< 2^22 per entry) - and totals / compat / classdeg / the row arrays follow from an
     * O(n C) pass over them.  counts->rowptr supplies |P_u|; counts->col is not read; the outputs are
     * written, not accumulated (no zeroing needed).  NULL: nothing extra. */
    const struct wdg_stats_job *counts;
    const float *row_scale;
} wdg_las_job;
/* 1 when wdg_las_batched_f32 / wdg_las_f32 take the fused one-workgroup-per-problem kernel for these sizes (needed by `counts`) */
int wdg_las_fused_eligible(int32_t max_n, int32_t max_F, int32_t max_C);
int wdg_las_batched_f32(const wdg_las_job *jobs_dev, int32_t n_jobs, int32_t max_n, int32_t max_F, int32_t max_C,
                        wdg_stream_t stream);

/* ------------------------------------------------------------------ dense feature transform */
#define WDG_ACT_NONE 0
#define WDG_ACT_RELU 1
/*
 * C[M,N] = act(A[M,K] B[K,N] + bias[N]) in exact fp32 on the MFMA pipe (v_mfma_f32_32x32x2_f32).
 * The reference has no X.W (its models live upstream, gnns_on_syn.py:1-249 holds only results);
 * this is the build-defined SGC-1 / GCN-2 transform of SURVEY.md 7.3 (K10), and the Gram products of
 * utils/homophily_metrics.py:234-235,246 (B = A^T via transb).
 * K = 0 is the empty sum: act(bias), or act(0) without a bias, is stored into all of C; A and B may be NULL then and are never
 * dereferenced.  WDG_ACT_RELU in this and the following GEMM entry points turns negative values into 0 and keeps a NaN a NaN
 * (torch.relu's rule, not fmaxf's); the hidden activation of the fused two-layer transform below is fmaxf(v, 0).
 */
int wdg_gemm_f32(const float *A, int64_t lda, const float *B, int64_t ldb, int transb, const float *bias, int act,
                 float *C, int64_t ldc, int32_t M, int32_t N, int32_t K, wdg_stream_t stream);
/*
 * The same product for a classifier-sized N <= 8 and any K (the SGC-1 head X W: Cora 2708 x 1433 x 7): bound by the read of A,
 * so the rows are spread over the whole chip (a wave per row for K > 512, B read through the caches; 16 / 4 / 1 lanes per row and
 * B in LDS for shorter rows) instead of 128-row MFMA tiles.  Summation order: per lane k = l, l + L, ... ascending (L lanes per
 * row), then a fixed butterfly over the row's lanes - bitwise
 * reproducible, within fp32 rounding of wdg_gemm_f32's k-ordered chain (not bit-identical to it).  B is [K, N] (no transb).
 * K = 0 is the empty sum: act(bias), or act(0) without a bias, is stored into all of C; A and B may be NULL then and are never
 * dereferenced.
 */
int wdg_gemm_skinny_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, int act, float *C,
                        int64_t ldc, int32_t M, int32_t N, int32_t K, wdg_stream_t stream);
/* L of the above, the lanes that share a row of K entries: 1 (K <= 16), 4 (K <= 128), 16 (K <= 512) or 64 (a wave per row).  The
 * launcher asks this very function (a host entry point: no device needed). */
int32_t wdg_gemm_skinny_lanes(int32_t K);

/* Many independent products in one launch (every graph of a sweep batch with its own weights); B is [K,N]. */
typedef struct wdg_gemm_job {
    const float *A;
    const float *B;
    const float *bias; /* [N] or NULL */
    float *C;
    int64_t lda, ldb, ldc;
    int32_t M, N, K, act; /* act: WDG_ACT_* */
} wdg_gemm_job;
int wdg_gemm_batched_f32(const wdg_gemm_job *jobs_dev, int32_t n_jobs, int32_t max_M, int32_t max_N,
                         wdg_stream_t stream);
/*
 * Split-K for one product with few output tiles and a long K (the first layer of a GCN on a single wide-feature graph:
 * squirrel's X W0 is 5201 x 2089 x 64, 41 tiles on 256 CUs): K is cut into `splits` ranges (wdg_gemm_splitk_plan: 1 = the shape
 * does not need it), every range a workgroup of its own per tile writing a partial product into `workspace`
 * (wdg_gemm_splitk_workspace_bytes), and a second launch adds the partials in split order, then bias and activation.  Each
 * partial is the k-ordered fma chain of its range and the ranges are added in order: bitwise reproducible, but NOT the single
 * chain of wdg_gemm_f32 - the two agree to fp32 rounding.  Replaces the same `x @ W` as wdg_gemm_f32.
 * K < 16 splits (K = 0 among them) is wdg_gemm_f32's single chain, workspace unused; with K = 0 act(bias), or act(0) without a
 * bias, is stored into all of C, A and B may be NULL and are never dereferenced.
 */
int32_t wdg_gemm_splitk_plan(int32_t M, int32_t N, int32_t K);
size_t wdg_gemm_splitk_workspace_bytes(int32_t M, int32_t N, int32_t splits);
int wdg_gemm_splitk_f32(const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, int act, float *C, int64_t ldc,
                        int32_t M, int32_t N, int32_t K, int32_t splits, void *workspace, size_t workspace_bytes, wdg_stream_t stream);
/* Same, with what the host knows about the table: max_K = the largest K, flags = WDG_GEMM_*.  With WDG_GEMM_A_VEC4 the
 * caller promises that in EVERY job A is 16-byte aligned, lda % 4 == 0 and K % 4 == 0 (any contiguous fp32 row-major
 * activation matrix with K % 4 == 0); tall-skinny tables (max_N <= 64, max_K <= 512, max_M >= 256) then run on the
 * B-resident kernel (B of a job copied to LDS once, A streamed straight into the MFMA operand layout, no K-step
 * barriers).  Results are bit-identical either way (same fp32 fma chain in k order). */
#define WDG_GEMM_A_VEC4 1u
int wdg_gemm_batched_flags_f32(const wdg_gemm_job *jobs_dev, int32_t n_jobs, int32_t max_M, int32_t max_N,
                               int32_t max_K, uint32_t flags, wdg_stream_t stream);
/* 1 when a launch of these sizes whose operands keep the WDG_GEMM_A_VEC4 promise takes the B-resident kernel (wdg_gemm_f32 with
 * n_jobs = 1, or a table with the flag), 0 when it takes the tile kernel; reads WDG_GEMM_TILE / WDG_GEMM_RESIDENT as the launch does */
int wdg_gemm_resident_eligible(int32_t n_jobs, int32_t max_M, int32_t max_N, int32_t K);

/* Fused two-layer feature transform Z = act(A W0 + b0) W1 + b1 for every graph of a batch in one launch and one pass
 * over A (hidden width H <= 64, C <= 8 outputs, K <= 512): the build-defined GCN-2 feature path relu(Y W0) W1 (SURVEY
 * 7.3 / K10; the reference has no model code - gnns_on_syn.py:9-154 is a results table - so the operator is ours).  The
 * hidden activations stay in registers (B-resident kernel with swapped MFMA operands, second product as per-lane fma)
 * and are not stored (a caller that needs them calls wdg_gemm_batched_f32 twice).  Contract as WDG_GEMM_A_VEC4: every A 16-byte aligned, lda % 4 == 0, K % 4 == 0.
 * First product: fp32 products formed from three bf16 pieces of each operand (the pieces sum to the fp32 value; the six
 * piece products of weight >= 2^-16 are issued on the bf16 matrix pipe and accumulated in fp32) - within fp32 rounding of
 * wdg_gemm_f32's k-ordered chain and closer to an fp64 evaluation than it (csrc/gemm.hip, mlp2_split_kernel);
 * WDG_MLP2_SPLIT=0 in the environment selects the chain itself (bit-identical to wdg_gemm_f32).  The second product sums a
 * row's hidden columns per lane in fp32, not in the k order of a separate wdg_gemm_f32 call.  Parity with two calls: 1e-5.
 * Deterministic.  Returns WDG_ERR_UNSUPPORTED for larger shapes: call wdg_gemm_batched_f32 twice. */
typedef struct wdg_mlp2_job {
    const float *A;    /* [M,K] */
    const float *W0;   /* [K,H] */
    const float *b0;   /* [H] or NULL */
    const float *W1;   /* [H,C] */
    const float *b1;   /* [C] or NULL */
    float *Z;          /* [M,C] */
    int64_t lda, ldw0, ldw1, ldz;
    int32_t M, K, H, C, act, reserved; /* act on the hidden layer: WDG_ACT_* */
    int64_t a_group_stride; /* 0: A row-major.  > 0: A tiled by 16-column groups as wdg_spmm_job.y_group_stride writes it, element
                               (m, k) at A[(k / 16) a_group_stride + m lda + k % 16] (the split-operand kernel, the default; with
                               WDG_MLP2_SPLIT=0 in the environment A must be row-major) */
} wdg_mlp2_job;
int wdg_mlp2_batched_f32(const wdg_mlp2_job *jobs_dev, int32_t n_jobs, int32_t max_M, int32_t max_K, int32_t max_H,
                         int32_t max_C, wdg_stream_t stream);
/* The same launch with the kernel NAMED by the caller instead of read from the environment at launch time (a table built for the
 * split-operand kernel - a tiled A - must never be read by the chain kernel, whatever the environment says by then):
 *   WDG_KERNEL_SPLIT / WDG_KERNEL_CHAIN  which kernel (neither: as wdg_mlp2_batched_f32 - the environment decides);
 *   WDG_OPERAND_TILED                    some job of the table has a_group_stride > 0: the chain refuses it (WDG_ERR_UNSUPPORTED). */
#define WDG_KERNEL_SPLIT 1u
#define WDG_KERNEL_CHAIN 2u
#define WDG_OPERAND_TILED 4u
int wdg_mlp2_batched_flags_f32(const wdg_mlp2_job *jobs_dev, int32_t n_jobs, int32_t max_M, int32_t max_K, int32_t max_H,
                               int32_t max_C, uint32_t flags, wdg_stream_t stream);

/* ------------------------------------------------------------------ kernel-regression metric (Gram kernels + solver) */
/*
 * K = map(A A^T) for ALL n rows of A [n, F] (the aggregated features A_hat X of a graph, or X itself), the map fused into
 * the MFMA launch as its epilogue; either output may be NULL:
 *   K_linear = G / 2                                                           (n_layers = 0)
 *   K_arccos = (G (pi - acos(G / nu)) + sqrt(nu^2 - G^2)) / (2 pi),  nu = max(|a_i| |a_j|, 1e-8), NaN -> 0   (n_layers = 1)
 * with |a_i|^2 = G_ii, the Gram's own diagonal bit for bit (norm2 [n] is scratch the call fills).  G is symmetric bit for bit.
 * Symmetric does not mean that bit-identical ROWS of A give bit-identical rows of K: the split-operand kernels compute the entries
 * on or below the diagonal and mirror them, and their piece products are not symmetric in the two operands, so for duplicates
 * d1 < j < d2 the entries K[d1][j] (a mirror) and K[d2][j] may differ in the last bit (equal where both lie on the same side of the
 * diagonal; the chain's products commute: equal everywhere).  The solver reads every id at its representative and does not care.
 * The map inherits the reference's jump at cos = -1: acos of a quotient that rounding pushed below -1 is NaN, NaN -> 0, and the entry
 * of two exactly antiparallel rows is either about 0 or about G / 2, decided by the last bit of G / nu (at cos = +1 both branches
 * agree).  The features of this domain are non-negative, where no cosine is negative.
 * Its fp32 products are formed from three bf16 pieces per operand on the bf16 matrix pipe, fp32 accumulation (no input bit
 * dropped; against fp64 within a small factor of the k-ordered fp32 chain's error, usually below it); WDG_GRAM_SPLIT=0 in the
 * environment selects that chain (then G is bit-identical to wdg_gemm_f32 with transb).
 * replaces: gntk_homophily_ utils/homophily_metrics.py:232-257 (utils/homophily_plot.py:238-268).  The reference maps the
 *           Gram of the rows SAMPLED in an epoch; the map is elementwise in (G_ij, |a_i| |a_j|), so that kernel is the
 *           sub-block [sample, sample] of this one - computed once per graph instead of once per epoch.
 */
typedef struct wdg_gram_job {
    const float *A;   /* [n, F] */
    float *norm2;     /* [n] scratch: |a_i|^2 */
    float *K_linear;  /* [n, n] or NULL */
    float *K_arccos;  /* [n, n] or NULL */
    int64_t lda, ldk;
    int32_t n, F;
    int64_t a_group_stride; /* 0: A row-major.  > 0: A tiled by 16-column groups (wdg_spmm_job.y_group_stride), element (i, k) at
                               A[(k / 16) a_group_stride + i lda + k % 16] - the split-operand kernels (the default; with
                               WDG_GRAM_SPLIT=0 in the environment A must be row-major) */
} wdg_gram_job;
int wdg_gram_map_batched_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, wdg_stream_t stream);
/* the kernel named by the caller (WDG_KERNEL_SPLIT / WDG_KERNEL_CHAIN / WDG_OPERAND_TILED as for wdg_mlp2_batched_flags_f32) */
int wdg_gram_map_batched_flags_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, uint32_t flags, wdg_stream_t stream);

/*
 * The kernels of the AGGREGATED features without a dense product per graph (round 5): with Y = A_hat X, Y Y^T = A_hat (X X^T) A_hat^T, so
 * K_linear(Y) = A_hat K_linear(X) A_hat^T - two aggregations with n "features" over the kernel of the raw features (which the metric
 * computes anyway, once per feature matrix): 2 nnz n flops each instead of n^2 F.  The caller runs
 *     T = A_hat K_linear(X)   (any aggregation entry point, n features),   wdg_transpose_batched_f32: T -> T^T,
 *     U = A_hat T^T,          wdg_gram_finish_batched_f32
 * wdg_gram_finish_batched_f32: job->A = U ([n, n], leading dimension lda; its LOWER triangle is taken as the half Gram G / 2, F is
 * ignored) -> norm2 = 2 diag(U) = G_ii, K_linear = the lower triangle mirrored, K_arccos = the arc-cosine map of G = 2 U exactly
 * as wdg_gram_map_batched_f32 maps its Gram.  K_linear may be U itself (in place).  Deterministic.
 * replaces: the same lines as wdg_gram_map_batched_f32 (utils/homophily_metrics.py:232-243) for the aggregated features - the same
 *           quantity by another association; entries agree with the direct product to fp32 rounding (tests: rtol 2e-5).
 */
typedef struct wdg_transpose_job {
    const float *src; /* [rows, cols], leading dimension ld_src */
    float *dst;       /* [cols, rows], leading dimension ld_dst: dst[c][r] = src[r][c] */
    int64_t ld_src, ld_dst;
    int32_t rows, cols;
} wdg_transpose_job;
int wdg_transpose_batched_f32(const wdg_transpose_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream);
int wdg_gram_finish_batched_f32(const wdg_gram_job *jobs_dev, int32_t n_jobs, int32_t max_n, wdg_stream_t stream);

/*
 * Generalized edge homophily from a Gram: mean over the stored non-loop entries (u, v) of cos(x_u, x_v) = 2 K_linear[u, v] /
 * sqrt(norm2[u] norm2[v]) (NaN -> 0), K_linear / norm2 = a wdg_gram_map_batched_f32 output of the feature matrix.
 * replaces: generalized_edge_homophily utils/homophily_plot.py:56-66 (utils/homophily_metrics.py:164-187, below sample_max):
 *           the dense N x N sklearn cosine matrix masked by the adjacency.  Deterministic (fixed summation order).
 * workspace: wdg_edge_gram_workspace_bytes(n_jobs, max_rows).
 */
typedef struct wdg_edge_gram_job {
    const int32_t *rowptr;
    const int32_t *col;
    const float *K_linear; /* [n, n] = X X^T / 2 */
    const float *norm2;    /* [n] |x_i|^2 */
    double *mean_out;      /* [1] */
    int64_t ldk;
    int32_t n_rows, reserved;
} wdg_edge_gram_job;
size_t wdg_edge_gram_workspace_bytes(int32_t n_jobs, int32_t max_rows);
int wdg_edge_gram_mean_batched_f32(const wdg_edge_gram_job *jobs_dev, int32_t n_jobs, int32_t max_rows, void *workspace,
                                   size_t workspace_bytes, wdg_stream_t stream);

/*
 * Row representatives: rep_out[i] = the smallest row index j <= i whose row is BIT-IDENTICAL to row i (+0 == -0; a NaN equals nothing),
 * of a dense fp32 matrix (WDG_ROW_REP_DENSE: A [n, F], row-major or tiled like wdg_gram_job.A) or of a scaled CSR pattern
 * (WDG_ROW_REP_CSR: rows equal in length, columns, stored order, values - NULL: unit - and row_scale; identical rows of A_hat give
 * identical rows of A_hat X whatever X holds).  A 64-bit row hash, then every candidate verified element by element.  Deterministic.
 * replaces: the part of `np.linalg.pinv(K_train_train)` (utils/homophily_metrics.py:283-297, utils/homophily_plot.py:296-310) that
 *           answers EXACTLY singular train blocks: duplicate nodes give bit-identical rows of the reference's Gram (utils/
 *           homophily_metrics.py:232-247), the pseudo-inverse's minimum-norm answer is the solution of the system deflated to one
 *           representative per duplicate class with the class's mean one-hot label - which wdg_kernel_regress_batched_f32 solves
 *           when a job carries these maps (wdg_kr_job.rep).
 */
#define WDG_ROW_REP_DENSE 0
#define WDG_ROW_REP_CSR 1
typedef struct wdg_row_rep_job {
    const float *A;           /* DENSE: [n, F] */
    const int32_t *rowptr;    /* CSR: [n + 1] */
    const int32_t *col;       /* CSR: [nnz] */
    const float *val;         /* CSR: [nnz] or NULL (unit values) */
    const float *row_scale;   /* CSR: [n] or NULL */
    int32_t *rep_out;         /* [n] */
    void *hash_ws;            /* [n] 8-byte scratch */
    int64_t lda, a_group_stride; /* DENSE: as wdg_gram_job */
    int32_t n, F;
} wdg_row_rep_job;
int wdg_row_rep_batched(const wdg_row_rep_job *jobs_dev, int32_t n_jobs, int32_t max_n, int32_t source, wdg_stream_t stream);

/*
 * Batched kernel regression: for every job, alpha = K[train, train]^-1 onehot(labels[train]) by a register-resident Cholesky
 * factorisation (n_train <= wdg_kernel_regress_max_train() = 320; a job carries the right-hand sides of at most 8 classes - n_classes <= 8,
 * or one CLASS WINDOW of a problem of up to 16 classes, below), predictions K[val, train] alpha, and
 * *correct_out = #{v in val : argmax_c prediction == labels[v]} (first maximum, like torch.argmax); -1 for shapes out of range.
 * replaces: `K_val_train @ (np.linalg.pinv(K_train_train) @ label_onehot[idx_train])`, `.argmax(1).eq(labels[idx_val])`
 *           utils/homophily_metrics.py:283-297 (utils/homophily_plot.py:296-310), once per (graph, classifier, epoch,
 *           kernel) - all of a sweep shard's problems in one launch.  For a positive definite train block the result IS the
 *           pseudo-inverse's; when a pivot falls to rounding level (<= n eps max K_ii: rank-deficient block, duplicate nodes)
 *           the block is refactored once as K + 8 n eps max K_ii I - the pseudo-inverse's least-squares predictions to within
 *           rounding (documented deviation in the coefficients).
 *           wdg_kernel_regress_deflated_batched_f32 - `rep` (wdg_row_rep_batched of the matrix the kernel was computed from) and a
 *           workspace `ws` per job - does not leave EXACT duplicates to the ridge: every train / validation id is read at its representative
 *           (duplicate rows of K are then identical by construction), the train rows are deflated to one row per duplicate class with
 *           the class's mean one-hot label - the pseudo-inverse's minimum-norm answer, by a positive definite factorisation; flags bit 1 reports it.  Rows
 *           below the block's fp32 resolution (K_ii <= n eps max K_ii / 64, the solver's own pivot test: all-zero rows, the
 *           arc-cosine kernel of an all-zero feature row) are dropped like exact zeros - an fp32 SVD cannot resolve their singular
 *           value either; flags bit 2 reports a drop (bit 1 is set with it).  A row above that level is solved, not dropped: a
 *           hub-heavy kernel whose K_ii span 1e-5 of the block's maximum gets the pseudo-inverse's answer.  The deflated block is
 *           scaled by the square roots of the class sizes (pinv(P K_u P^T) = Q pinv(S K_u S) Q^T, Q = P S^-1), so that a block that is
 *           rank deficient beyond its duplicates is regularised in the full system's metric.  wdg_kernel_regress_batched_f32 itself ignores both fields.
 * `train` / `val` index rows of K; `labels` is indexed like K's rows.  Limits: ldk < 65 536 (a kernel matrix is addressed by
 * unsigned 32-bit element offsets: row x ldk + column < 2^32; a problem with a wider ldk answers -1 with flags 0).  The launch is persistent - one workgroup per CU walks the problems, and a problem's predictions are
 * made inside the next problem's factorisation (WDG_KR_PERSIST=0: one workgroup per problem) - which changes no result.
 */
typedef struct wdg_kr_row_best {
    float value;            /* the first maximum over the window's classes; -3.4e38 when no prediction exceeds that (NaN never wins) */
    int32_t cls;            /* its class, as an ABSOLUTE class id (class_base + column); class_base when nothing won */
} wdg_kr_row_best;
typedef struct wdg_kr_job {
    const float *K;         /* [n, n] kernel of all nodes (a wdg_gram_map_batched_f32 output), leading dimension ldk */
    const int32_t *train;   /* [n_train] */
    const int32_t *val;     /* [n_val] */
    const int32_t *labels;  /* [n] */
    int32_t *correct_out;   /* [1]: validation rows predicted right; -1 = problem refused (shape outside the limits) */
    int32_t *flags_out;     /* [1] or NULL: bit 0 = a pivot fell to rounding level and the block was refactored with the ridge;
                               bit 1 = the train rows were deflated (duplicates merged / zero rows dropped);
                               bit 2 = (deflating entry) rows below the block's resolution were dropped */
    int64_t ldk;
    int32_t n_train, n_val, n_classes; /* n_classes: the PROBLEM's classes (also of a window job) */
    int32_t class_base;     /* the first class of the job's window: 0 for the entries without class windows (they do not read it) */
    const int32_t *rep;     /* [n] or NULL: row representatives of the matrix K was computed from (wdg_row_rep_batched) */
    void *ws;               /* NULL, or wdg_kr_deflate_workspace_bytes(n_val) bytes (16-byte aligned) of the problem's own
                               (wdg_kernel_regress_deflated_batched_f32) */
    wdg_kr_row_best *rows_out; /* [n_val] or NULL (not wanted): per validation row, in `val` order, the largest prediction among the
                               window's classes and its class (the window entries; the entries without class windows do not read it) */
} wdg_kr_job;
/* The same regression for a table whose EVERY job carries a workspace `ws` (and, where the matrix has them, the row representatives
 * `rep`; NULL = every node its own): a pre-pass writes per problem the train rows to solve (one representative per class of duplicate
 * nodes, rows with K_ii == 0 dropped), their labels / right-hand sides and the validation rows' representatives and labels into ws,
 * the solver reads them and tests its pivots per row.  Two launches, one call.
 * replaces: the same lines as wdg_kernel_regress_batched_f32 - np.linalg.pinv's answer on exactly singular blocks included
 *           (utils/homophily_metrics.py:291-297). */
size_t wdg_kr_deflate_workspace_bytes(int32_t n_val);
int wdg_kernel_regress_deflated_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);
int32_t wdg_kernel_regress_max_train(void);

/*
 * CLASS WINDOWS: problems of 9 .. 16 classes.  A regression's class columns are independent - the factorisation, the pivot test,
 * the ridge and the deflation do not see the right-hand sides -, and a solver workgroup has room for 8 of them.  A problem of C
 * classes, C <= 16, is therefore solved as ceil(C / 8) WINDOW JOBS over the same kernel, node sets and labels: window job w has
 * class_base = 8 w, n_classes = C (the problem's total) and carries the right-hand sides of classes class_base ..
 * min(class_base + 8, C) - 1; its rows_out receives, per validation row, the first maximum over those classes (value, absolute class id) -
 * the arg-max rule of the plain entries: the value starts at -3.4e38, a strictly greater prediction replaces it, NaN never wins -,
 * its correct_out the hits of the window alone and its flags_out the flags word.  The deflation pre-pass judges a duplicate class's
 * labels (pure / mixed / none in range) over all 16 classes, so a problem's workspace does not depend on the window; every window
 * job carries a workspace of its own all the same.  wdg_kr_combine_windows_batched then takes, per problem and validation row,
 * the first maximum over the problem's windows in window order and counts the hits.
 * A window job is refused (correct_out -1, flags_out 0, rows_out untouched, the table's other jobs unaffected) when n_classes > 16,
 * class_base is not a multiple of 8 or >= n_classes, or n_classes > 8 without rows_out; the limits of the plain entries hold as well.
 * A job with class_base 0, n_classes <= 8 and no rows_out is answered exactly as the plain entry answers it.
 * deflate != 0: wdg_kernel_regress_deflated_batched_f32's pre-pass and solver (every job carries `ws`), else wdg_kernel_regress_batched_f32's.
 * The plain entries above run their own, unchanged kernels: tables with window jobs go through the entries below.
 * replaces: `K_val_train @ (np.linalg.pinv(K_train_train) @ label_onehot[idx_train])` utils/homophily_metrics.py:283-297
 *           (utils/homophily_plot.py:296-310) for the datasets of more than 8 classes that the reference's loaders name
 *           (utils/util_funcs.py:134,138), a window of 8 class columns per job.
 */
int wdg_kernel_regress_windows_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, int32_t deflate, wdg_stream_t stream);
/* The combine pass of a table of window jobs: per problem, for every validation row v the first maximum over rows[w * row_stride + v],
 * w = 0 .. n_windows - 1 in window order (a strictly greater value replaces; start -3.4e38, class 0; NaN never wins), compared with
 * labels[val[v]]; *correct_out = the hits, or -1 when a window job refused (win_correct[w] < 0) or n_windows is outside 1 .. 2;
 * *flags_out = the OR of win_flags[w].  One launch for the whole table; it only enqueues.
 * replaces: `.argmax(1)` / accuracy of utils/homophily_metrics.py:283-297 over the class columns that the window jobs hold apart. */
typedef struct wdg_kr_combine_job {
    const wdg_kr_row_best *rows; /* [n_windows, row_stride]: the window jobs' rows_out */
    const int32_t *win_correct;  /* [n_windows]: the window jobs' correct_out */
    const int32_t *win_flags;    /* [n_windows] or NULL: the window jobs' flags_out */
    const int32_t *val;          /* [n_val] */
    const int32_t *labels;       /* [n] */
    int32_t *correct_out;        /* [1] */
    int32_t *flags_out;          /* [1] or NULL */
    int64_t row_stride;
    int32_t n_val, n_windows;
} wdg_kr_combine_job;
int wdg_kr_combine_windows_batched(const wdg_kr_combine_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);

/*
 * The same regression for train blocks of 1 .. wdg_kernel_regress_large_max_train() = 1024 rows (8 class columns per job as above, ldk < 65 536): the
 * Cholesky factor lives in device memory instead of registers - packed 32 x 32 blocks of the lower triangle in a LAUNCH-LEVEL
 * scratch buffer that the caller allocates, one 2.1-MiB slice (528 blocks x 4 KiB) per resident workgroup:
 * wdg_kr_large_scratch_bytes() = CUs x 2.1 MiB, whatever the length of the table (a shorter buffer runs fewer workgroups; less
 * than one slice is an error).  One workgroup per problem, persistent over the table; left-looking by block column on the fp32
 * matrix pipe; every sum in a fixed order that depends on the problem alone (a relaunch is bit-identical, and no result depends
 * on the workgroup that took the problem).  The numerical contract is wdg_kernel_regress_batched_f32's: pivots tested against
 * n eps max K_ii / 64, one refactorisation with the ridge n eps max K_ii / 8 (flags bit 0), -1 for shapes out of range.
 * Per job: ws != NULL - the deflating pre-pass runs first (row representatives `rep`, NULL = every node its own; scaled block
 * S K S, mean one-hot right-hand sides, the drop rule, flags bits 1 and 2: exactly wdg_kernel_regress_deflated_batched_f32's
 * semantics, above), ws = wdg_kr_large_workspace_bytes(n_train, n_val) bytes (16-byte aligned) of the job's own;
 * ws == NULL and rep == NULL - the block is solved as it is; ws == NULL with rep != NULL answers -1.
 * The caller allocates everything; no hidden synchronisation, no allocation.  Two launches, one call.
 * replaces: `K_val_train @ (np.linalg.pinv(K_train_train) @ label_onehot[idx_train])`, `.argmax(1).eq(labels[idx_val])`
 *           utils/homophily_metrics.py:283-297 (utils/homophily_plot.py:296-310) for `--sample_max` (homophily_tests.py:54)
 *           above 533, where an epoch's train block has more than 320 rows.
 */
/* replaces: the limit on utils/homophily_metrics.py:283-297 that this entry holds (train rows of one regression) */
int32_t wdg_kernel_regress_large_max_train(void);
/* replaces: nothing of its own - the factor storage of utils/homophily_metrics.py:291-297's pinv, owned by the launch */
size_t wdg_kr_large_scratch_bytes(void);
/* replaces: nothing of its own - the per-job workspace of the deflating pre-pass (utils/homophily_metrics.py:291-297 on singular blocks) */
size_t wdg_kr_large_workspace_bytes(int32_t n_train, int32_t n_val);
/* replaces: utils/homophily_metrics.py:283-297, utils/homophily_plot.py:296-310 (see above) */
int wdg_kernel_regress_large_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, void *scratch, size_t scratch_bytes, wdg_stream_t stream);
/* The large solver for a table of window jobs (class windows, above: class_base, rows_out, the same refusals); otherwise
 * wdg_kernel_regress_large_batched_f32's contract, scratch included.
 * replaces: utils/homophily_metrics.py:283-297, utils/homophily_plot.py:296-310 for more than 8 classes (utils/util_funcs.py:134,138)
 *           and train blocks of more than 320 rows */
int wdg_kernel_regress_large_windows_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, void *scratch, size_t scratch_bytes, wdg_stream_t stream);

/*
 * The node sets of the epochs, drawn on the device: per (graph, classifier, epoch) set a class-balanced sample of the nodes
 * and, inside it, the class-balanced train rows; the rest of the sample validates.
 * replaces: the two random_disassortative_splits calls per epoch of classifier_based_performance_metric
 *           (utils/homophily_metrics.py:267-281, utils/homophily_plot.py:286-297; the routine: utils/util_funcs.py:454-475).
 * Same DISTRIBUTION as the reference (per class: the first train_per_class[c] members of a uniform random permutation train,
 * the next sample_per_class[c] - train_per_class[c] validate), a documented generator instead of torch's CPU stream:
 * key(node) = Philox4x32-10(counter {node, set index, 0, 0}, key = seed), first output word; nodes ordered by (class, key,
 * node).  Ids come out ascending (the reference's boolean masks).  A job = n_sets sets of one label vector; set s of the job
 * is written to train_out + s train_stride / val_out + s val_stride (sum of train_per_class / of sample - train entries each).
 * Grid block b serves set b - first_set of the job with first_set <= b < first_set + n_sets (jobs ascending in first_set).
 * Limits: n <= 16 000 nodes, n_classes <= 64.  Labels outside [0, n_classes) are never drawn.
 * A class with fewer members than train_per_class[c] / sample_per_class[c] gives what it has.  A set that comes out shorter than
 * its stride for either reason leaves the remaining entries of its row UNTOUCHED (neither zeroed nor marked): the sums above are
 * then upper bounds of the set's length, and a caller who needs the length fills the outputs with a marker before the launch.
 * Nothing is ever written past a row's stride.
 */
typedef struct wdg_kr_sample_job {
    const int32_t *labels;            /* [n] */
    const int32_t *sample_per_class;  /* [n_classes] s_c: members of class c in an epoch's sample */
    const int32_t *train_per_class;   /* [n_classes] t_c <= s_c */
    int32_t *train_out;               /* [n_sets, train_stride] */
    int32_t *val_out;                 /* [n_sets, val_stride] */
    uint64_t seed;
    int32_t n, n_classes, n_sets, first_set, train_stride, val_stride;
} wdg_kr_sample_job;
int wdg_kr_sample_sets(const wdg_kr_sample_job *jobs_dev, int32_t n_jobs, int32_t n_sets_total, int32_t max_n, wdg_stream_t stream);
int wdg_kernel_regress_batched_f32(const wdg_kr_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);

/*
 * Every epoch of many multinomial logistic heads, logits = M W, in one call: one workgroup trains one model for all `epochs` epochs
 * (cross-entropy over the train rows, torch's Adam with the L2 term in the gradient, model selection on the validation hits), no
 * host in the loop and nothing between workgroups.
 * replaces: the training loops behind the SGC-1 and MLP-1 accuracy tables, gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the
 *           loop itself lives upstream of the reference): M = A_hat X for SGC-1, M = X for MLP-1.  The arithmetic restates the
 *           epoch of sweep.TrainBatch (kind "sgc" / "mlp1": two batched GEMM launches + ~15 PyTorch launches per epoch).
 * For epoch e = 0 .. epochs - 1, Adam step t = step0 + e + 1:
 *   Z = M[train] W;  G = (softmax(Z) - onehot(labels[train])) / n_train (fp32, maximum subtracted);  g = M[train]^T G + weight_decay W;
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  W -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);
 *   with the new W: pred = argmax(M W) (first maximum), the hits on `val` and on `test`;
 *   if val hits > best[0] (strict): best = (val hits, test hits, step0 + e).
 * W, m, v and best are read and written, so a call of a + b epochs and two calls of a, then b epochs (step0 = a) are the same
 * computation, bit for bit; every sum has a fixed order that depends on the job's own shape alone (no floating-point atomics: two
 * runs are bit-identical, and a job's result does not depend on the table it is in).
 * Limits: 1 <= C <= 8, 1 <= F <= 4096 (max_F / max_C: the table's largest; outside: WDG_ERR_UNSUPPORTED), n_train >= 1, n_val >= 1,
 * n_test >= 0, ldm >= F (a job outside them is left untouched); labels outside 0 .. C-1 match no class.  n_jobs == 0 or
 * epochs == 0: nothing is launched.  Jobs run in the kernel instantiation their own (F, C) names: the call enqueues one launch per
 * instantiation that max_F / max_C admit, a workgroup per job in each, and only the owning one works.
 */
typedef struct wdg_head_train_job {
    const float *M;          /* [n, F] fp32 row-major, leading dimension ldm */
    const int32_t *labels;   /* [n] class of every row, 0 .. C-1 */
    const int32_t *train, *val, *test;   /* row ids */
    float *W, *m, *v;        /* [F, C] in/out: weights, Adam first / second moment */
    int32_t *best;           /* in/out [3]: validation hits of the best epoch (-1: none yet), test hits at it, its epoch index */
    int64_t ldm;
    int32_t n_train, n_val, n_test, F, C, reserved;
} wdg_head_train_job;
int wdg_head_train_batched_f32(const wdg_head_train_job *jobs_dev, int32_t n_jobs, int32_t max_F, int32_t max_C,
                               int32_t epochs, int32_t step0, float lr, float weight_decay,
                               float beta1, float beta2, float eps, wdg_stream_t stream);

/*
 * ReLU + inverted dropout of the hidden layer of many two-layer models in one launch, IN PLACE, with the transposed copy the
 * backward GEMM reads (dW1 = H^T dZ) written in the same pass.  The mask is not stored: it is a function of the element's
 * position and of (seed, stream, step) through Philox4x32-10 (counter {c0, c1, 0, 0}, key {k0, k1}: the generator of
 * wdg_kr_sample_sets and wdg_synth_regular_batched), so two runs, an eager and a captured run, and a batched and a per-graph run of
 * the same model draw the same bits.
 * replaces: the hidden layer's ReLU + dropout of the training loops behind the GCN and MLP-2 accuracy tables, gnns_on_syn.py:213-249
 *           (beside the one-layer tables gnns_on_syn.py:109-154; the loop itself lives upstream of the reference, which has no
 *           model code).  In sweep.TrainBatch it stands in for the epoch's `hid.clamp_(min=0)` and `hid_t.copy_(hid^T)`.
 * The definition, for element (r, c) of job j (rows x cols, groups_per_row = ceil(cols / 4)):
 *   g = r * groups_per_row + (c >> 2)                                   (one Philox block serves four adjacent columns)
 *   w = the four output words of Philox4x32-10 with counter {g, *step_dev, 0, 0} and key {seed, jobs[j].stream}
 *   kept = w[c & 3] >= drop_threshold
 *   out = h * scale (ONE fp32 multiply) if kept and h > 0;  h itself if h is a NaN (a diverged run is not hidden);  +0.0f otherwise
 *   h[r][c] = out, and ht[c][r] = out when ht != NULL.
 * The host passes drop_threshold = (uint32_t) floor(p * 2^32), computed in fp64, and scale = (float) (1 / (1 - p)) for a drop
 * probability 0 <= p < 1; p = 0 is (0, 1.0f): every element is kept and the call is a plain ReLU.
 * *step_dev is read from DEVICE memory by the kernel: a captured hipGraph that holds this launch and an increment of the word
 * draws a fresh mask on every replay.
 * The backward pass needs no generator and no stored mask: a result is positive exactly where the unit was positive AND kept, so
 *   dH = (H_out > 0) ? dH * scale : 0.
 * Deterministic, no atomics; an element depends on its own input and position only: a job's result does not depend on the table
 * it is in.  h and ht of a job must not overlap.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, a NULL step_dev, a scale that is
 * not a number, max_rows * ceil(max_cols / 4) >= 2^32 (g is a 32-bit counter word), more than 65535 jobs (a job per grid z),
 * more than 64 * 65535 columns (a 64-column tile per grid y).  n_jobs == 0: WDG_OK, nothing is launched.  A job of 0 rows or 0
 * columns is skipped; rows and columns beyond max_rows / max_cols (the table's largest) are left untouched.
 */
typedef struct wdg_dropout_job {
    float *h;          /* [rows, cols], leading dimension ld; pre-activation in, relu + dropout out, IN PLACE */
    float *ht;         /* NULL, or [cols, rows], leading dimension ld_t: receives the transposed result */
    int64_t ld, ld_t;
    int32_t rows, cols;
    uint32_t stream;   /* generator stream of this job (TrainBatch: the job's index in the batch) */
} wdg_dropout_job;

int wdg_relu_dropout_batched_f32(const wdg_dropout_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                 uint32_t drop_threshold, float scale, uint32_t seed, const uint32_t *step_dev,
                                 wdg_stream_t stream);

/*
 * The sweep's synthetic graphs, generated on the device: every graph of a shard in ONE launch, written as sorted CSR - nothing is
 * uploaded and nothing is sorted.  The family is the one of the reference's pre-generated files (verified on them: N nodes in C
 * equal contiguous classes, every row exactly d = int(k / h) out-neighbours of which exactly k lie in the row's own class, no
 * self loops, no duplicates, the draws uniform without replacement inside the class and outside it).  Same DISTRIBUTION as the
 * reference's files, a documented stream of its own (the position wdg_kr_sample_sets takes for the node sets).
 * replaces: the loads of the adjacency, label and degree files, synthetic_plot.py:84-90 (the generator that wrote them is not in
 *           the reference).
 *
 * The definition, for a graph (n, C = n_classes, k, d, seed) with m = n / C:
 *   key(i, j) = word j & 3 of the four output words of Philox4x32-10 with counter {i, j >> 2, 0, 0} and key {seed low, seed high}
 *               (one Philox block serves four candidate columns);
 *   row i, of class c = i / m, holds
 *     - the k columns j of [c m, (c + 1) m), j != i, with the smallest (key(i, j), j), and
 *     - the d - k columns j outside [c m, (c + 1) m) with the smallest (key(i, j), j),
 *     - with WDG_SYNTH_SELF_LOOPS also column i (the A + I the sweep aggregates over),
 *   written ascending; every stored value is 1; labels[i] = i / m.
 * Outputs of job g: rowptr [n + 1] (local: rowptr[i] = i D, D = d or d + 1 with loops), col / val [n D], labels [n]; and, when
 * rowptr_union != NULL, rowptr_union[i] = nnz_base + i D for i = 0 .. n (the graph's rows inside the row pointer of a shard's
 * block-diagonal union; neighbouring graphs write the shared entry with the same value).
 * The table is given twice: jobs_host, which the entry validates BEFORE anything is launched, and the same bytes on the device.
 * Refused (WDG_ERR_INVALID): a null table with n_jobs > 0, more than 65535 jobs, n outside 1 .. 16384 (the cap of a batched
 * SELL-16 copy), C not dividing n, k outside 1 .. m - 1, d < k, d - k > n - m, unknown flags, a null output.  n_jobs == 0: nothing.
 */
#define WDG_SYNTH_SELF_LOOPS 1
typedef struct wdg_synth_job {
    int32_t *rowptr;        /* out [n + 1] */
    int32_t *col;           /* out [n D] */
    float *val;             /* out [n D]: ones */
    int32_t *labels;        /* out [n] */
    int32_t *rowptr_union;  /* out [n + 1] or NULL: nnz_base + rowptr */
    uint64_t seed;
    int32_t n, n_classes, k, d, flags, nnz_base;
} wdg_synth_job;
int wdg_synth_regular_batched(const wdg_synth_job *jobs_host, const wdg_synth_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);

/*
 * The rows of a base dataset behind a synthetic graph's features: node i of class c = i / (n / n_classes) takes member number
 * (u |class c|) >> 32 of the ASCENDING list of the base rows labelled c, u = the first output word of Philox4x32-10 with counter
 * {i, 0, 0, 0} and key {seed low, seed high} - per class a draw WITH replacement, as in the reference's feature files (which is
 * why they hold duplicate rows).  The multiply-shift favours some members by at most |class c| / 2^32 in relative terms (the
 * 2^32 values of u do not divide evenly among |class c| members): 1e-6 for a class of 4 000 rows.
 * replaces: the loads of the pre-sampled feature files, synthetic_plot.py:81-82 (the sampler that wrote them is not in the reference).
 * rows_out [n] int32; workspace: wdg_synth_feature_rows_workspace_bytes(n_base, n_classes) bytes, whose LAST n_classes int32 words
 * hold |class c| afterwards - a class without base rows leaves its nodes' entries unwritten: the caller checks the counts.
 */
/* replaces: nothing of its own - the member lists of the draw above (synthetic_plot.py:81-82) */
size_t wdg_synth_feature_rows_workspace_bytes(int32_t n_base, int32_t n_classes);
/* replaces: synthetic_plot.py:81-82 (see above) */
int wdg_synth_feature_rows(const int32_t *base_labels, int32_t n_base, int32_t n, int32_t n_classes, uint64_t seed, int32_t *rows_out,
                           void *workspace, size_t workspace_bytes, wdg_stream_t stream);

/*
 * Graphs of the CSBM-H model, generated on the device: classes of ANY sizes, each with an out-degree d[c] and a number k[c] of
 * same-class neighbours of its own (the model's h d_c with h d_c an integer) - the two ablation axes of the reference's command
 * line, csbm-h.py:428-442 (n0 : n1 and d0, d1), which wdg_synth_regular_batched (equal classes, one k, one d) cannot draw.
 * replaces: nothing the reference computes on a graph - csbm-h.py:174-175,187-191 draws the aggregated features from their closed-form
 *           law (csbm-h.py:46-56); this generator makes the graphs on which that law can be measured.
 *
 * The definition, for a graph of C = n_classes contiguous classes in order (class c = rows [s_c, s_c + class_size[c]), n = the sum):
 *   key(i, j) is EXACTLY wdg_synth_regular_batched's: word j & 3 of Philox4x32-10 with counter {i, j >> 2, 0, 0}, key {seed low, high};
 *   row i of class c holds
 *     - the k[c] columns j of its class block, j != i, with the smallest (key(i, j), j), and
 *     - the d[c] - k[c] columns j outside the block with the smallest (key(i, j), j),
 *     - with WDG_SYNTH_SELF_LOOPS also column i,
 *   written ascending; every stored value is 1; labels[i] = c; rowptr = the prefix sum of the rows' lengths D_c = d[c] (+ 1 with loops).
 * With equal class sizes and equal k, d the output is wdg_synth_regular_batched's bit for bit (one row routine: csrc/synth_row.h).
 * k[c] = 0 and d[c] = k[c] are allowed.  All jobs go in one launch; the table is given twice, as to the regular generator.
 * Refused on the HOST copy of the table, before any launch (WDG_ERR_INVALID): a null table with n_jobs > 0, more than 65535 jobs,
 * n_classes outside 1 .. 16, a class of no nodes, n outside 1 .. 16384, k[c] outside 0 .. class_size[c] - 1, d[c] < k[c],
 * d[c] - k[c] > n - class_size[c], unknown flags, a null output.  n_jobs == 0: nothing.
 */
#define WDG_SYNTH_MAX_CLASSES 16
typedef struct wdg_synth_classes_job {
    int32_t *rowptr;        /* out [n + 1] */
    int32_t *col;           /* out [sum_c class_size[c] D_c] */
    float *val;             /* out, as col: ones */
    int32_t *labels;        /* out [n] */
    uint64_t seed;
    int32_t n_classes, flags;
    int32_t class_size[WDG_SYNTH_MAX_CLASSES], k[WDG_SYNTH_MAX_CLASSES], d[WDG_SYNTH_MAX_CLASSES];
} wdg_synth_classes_job;
int wdg_synth_classes_batched(const wdg_synth_classes_job *jobs_host, const wdg_synth_classes_job *jobs_dev, int32_t n_jobs,
                              wdg_stream_t stream);

/*
 * Gaussian class features, drawn on the device: x[i][f] = mean[labels[i]][f] + sd[labels[i]] z(i, f) with z standard normal -
 * the node features of the CSBM-H model, N(mu_c, sigma_c I) with sd = sqrt(sigma_c) (the reference's sigma is a VARIANCE).
 * replaces: np.random.multivariate_normal(mu, sigma * np.eye(2), n), csbm-h.py:174-175 (same distribution, a documented stream).
 *
 * The definition: the Philox4x32-10 block with counter {i, q, 0, 0} and key {seed low, seed high} serves features 4q .. 4q + 3 of
 * row i; its words (w0, w1) and (w2, w3) are two Box-Muller pairs:
 *   u1 = ((w >> 8) + 1) 2^-24 in (0, 1],  u2 = (w' >> 8) 2^-24 in [0, 1)   (both exact in fp32),
 *   r = sqrtf(-2 logf(u1)),  z_a = r cospif(2 u2),  z_b = r sinpif(2 u2)   (features 4q, 4q + 1 from (w0, w1); 4q + 2, 4q + 3 from (w2, w3)),
 *   x = fmaf(sd[c], z, mean[c][f])
 * with the accurate library functions (the unit is compiled without fast-math).  |z| <= sqrt(48 ln 2) = 5.77.  sd = 0 gives the mean
 * exactly.  A label outside [0, n_classes) writes NaN.  Callers give the stream a seed of its own (not the graph's).
 * Refused on the HOST copy of the table, before any launch (WDG_ERR_INVALID): a null table with n_jobs > 0, more than 65535 jobs,
 * n < 0, F outside 1 .. 16, n_classes outside 1 .. 16, ldx < F, a null pointer in a job with n > 0.  n_jobs == 0: nothing.
 */
#define WDG_GAUSS_MAX_F 16
typedef struct wdg_gauss_job {
    float *x;               /* out [n, F], row i at x + i ldx */
    const int32_t *labels;  /* [n] */
    const float *mean;      /* [n_classes, F] */
    const float *sd;        /* [n_classes] */
    int64_t ldx;
    uint64_t seed;
    int32_t n, F, n_classes, reserved;
} wdg_gauss_job;
int wdg_gauss_features_batched_f32(const wdg_gauss_job *jobs_host, const wdg_gauss_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);

/*
 * The errors the Bayes rule of two isotropic Gaussian classes makes on three feature sets of a graph: t = 0 the features x, t = 1
 * the aggregated features h (the caller's A_rw x), t = 2 the high-pass features x - h.  Per job, counts[t][true][predicted] (int32
 * [3, 2, 2]) over the rows whose label is 0 or 1 (other rows are not counted).
 * replaces: the evaluation the reference only has in closed form - chi2comb_error, csbm-h.py:9-37, and PBE, csbm-h.py:40-60.
 *
 * Arithmetic: the high-pass row is ONE fp32 subtraction x[i][f] - h[i][f]; everything after it is fp64, every multiply and add its
 * own rounded operation (the unit is compiled with contraction off):
 *   s_c = sum over f ascending of (z_f - mean[t][c][f])^2   (from +0),   g_c = bias[t][c] - inv2v[t][c] * s_c,
 * class 0 is predicted iff g_0 > g_1 - so a NaN predicts 1.  The HOST forms bias = ln n_c - (F / 2) ln v_c and inv2v = 1 / (2 v_c).
 * A workgroup per job; counts are integer adds in registers and LDS and one plain store per entry: no atomic, nothing to clear
 * beforehand, bit-identical from run to run.
 * Refused on the HOST copy of the table, before any launch (WDG_ERR_INVALID): a null table with n_jobs > 0, more than 65535 jobs,
 * n < 0, F outside 1 .. 16, ldx or ldh < F, a null counts, a null x, h or labels in a job with n > 0.  n_jobs == 0: nothing.
 */
#define WDG_QDA_MAX_F 16
typedef struct wdg_qda_job {
    const float *x;         /* [n, F] */
    const float *h;         /* [n, F] */
    const int32_t *labels;  /* [n] */
    int32_t *counts;        /* out [3, 2, 2]: [set][true][predicted] */
    int64_t ldx, ldh;
    int32_t n, F;
    double mean[3][2][WDG_QDA_MAX_F];
    double inv2v[3][2];
    double bias[3][2];
} wdg_qda_job;
int wdg_qda_errors_batched_i32(const wdg_qda_job *jobs_host, const wdg_qda_job *jobs_dev, int32_t n_jobs, wdg_stream_t stream);

/*
 * The channel mix of an ACM layer (adaptive channel mixing: a low-pass, a high-pass and an identity channel weighted per node)
 * for many models in one launch, and its backward pass.  The reference's loader returns the high-pass operator g_high = I - A_hat
 * beside the low-pass one and its accuracy tables name "mf-" models, but it ships no model code: the layer is DEFINED here
 *  and is not claimed to reproduce those tables.
 * replaces: the use of g_high = I - A_hat, utils/util_funcs.py:198-204, in the model family behind the "mf-GCN" / "mf-SGC" tables,
 *           gnns_on_syn.py:58-104 and gnns_on_syn.py:159-206 (models that live upstream of the reference).
 * The definition, for row r of a job (rows x cols, 1 <= cols <= 256), T = 3, relu = flags & WDG_ACM_RELU:
 *   P_L = low[r,:]    P_H = high[r,:] - high_agg[r,:]  (high_agg == NULL: P_H = high[r,:])    P_I = ident[r,:]
 *   H_c = relu ? (P_c <= 0 ? 0 : P_c) : P_c                                    (a NaN stays a NaN)
 *   s_c = 1 / (1 + exp(-sum_k H_c[k] att[c][k]))                                 c in {L, H, I} = {0, 1, 2}
 *   z_c = sum_j (s_j / T) wmix[j][c]     alpha = softmax(z) with the maximum subtracted
 *   out[r][k] = 3 (alpha_L H_L[k] + alpha_H H_H[k] + alpha_I H_I[k]),  out_t[k][r] = out[r][k] when out_t != NULL
 *   aux[r][0..7] = alpha_L alpha_H alpha_I s_L s_H s_I 0 0
 * One pass: the subtraction, the row sums, the sigmoids, the 3 x 3 product, the softmax and the combination stay in registers.
 * The backward pass reads the same inputs, aux and d_out (g = d_out[r,:]) and writes
 *   dalpha_c = 3 sum_k g[k] H_c[k]      dz_c = alpha_c (dalpha_c - sum_j alpha_j dalpha_j)
 *   ds_j = (1 / T) sum_c wmix[j][c] dz_c      du_c = ds_c s_c (1 - s_c)
 *   dP_c[k] = (3 alpha_c g[k] + du_c att[c][k]) * (relu ? H_c[k] > 0 : 1)  ->  d_low = dP_L, d_high = dP_H, d_ident = dP_I
 *   d_att[c][k] = sum_r du_c H_c[k]      d_wmix[j][c] = sum_r (s_j / T) dz_c
 * (the caller forms d(high_agg) = -d_high).  The sums over rows are bitwise reproducible - no float atomics: the workgroup of
 * rows [64 b, 64 b + 64) adds its rows in a fixed order and stores one vector of 3 cols + 9 floats at partials + b (3 cols + 9);
 * a second launch inside the entry adds the blocks in block order.  partials holds ceil(rows / 64) (3 cols + 9) floats.
 * Every matrix has its own leading dimension (column slices of a wider GEMM or aggregation output are passed in place); att is
 * [3, cols] and wmix [3, 3], contiguous; aux is [rows, 8], contiguous.  Outputs must not overlap inputs or each other.
 * An element of out depends on its own row alone and a job's sums on the job alone: a job answers in a table what it answers alone.
 * Refused before any launch (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per
 * grid z), max_cols > 256.  n_jobs == 0: WDG_OK, nothing is launched.  A job of 0 rows writes nothing forward and zero sums
 * backward; rows beyond max_rows (the table's largest) are left untouched, and a job of more than max_cols columns is skipped.
 */
#define WDG_ACM_RELU 1
#define WDG_ACM_MAX_COLS 256
typedef struct wdg_acm_mix_job {
    const float *low;       /* [rows, cols]: A_hat (M W_L) */
    const float *high;      /* [rows, cols]: M W_H */
    const float *high_agg;  /* [rows, cols]: A_hat (M W_H), or NULL */
    const float *ident;     /* [rows, cols]: M W_I */
    const float *att;       /* [3, cols] */
    const float *wmix;      /* [3, 3] */
    float *out;             /* forward out [rows, cols] */
    float *out_t;           /* forward out [cols, rows], or NULL */
    float *aux;             /* [rows, 8]: forward out, backward in */
    const float *d_out;     /* backward in [rows, cols] */
    float *d_low, *d_high, *d_ident; /* backward out [rows, cols] */
    float *d_att;           /* backward out [3, cols] */
    float *d_wmix;          /* backward out [3, 3] */
    float *partials;        /* backward workspace: ceil(rows / 64) * (3 cols + 9) floats */
    int64_t ld_low, ld_high, ld_high_agg, ld_ident, ld_out, ld_out_t, ld_d_out, ld_d_low, ld_d_high, ld_d_ident;
    int32_t rows, cols, flags, reserved;
} wdg_acm_mix_job;
int wdg_acm_mix_batched_f32(const wdg_acm_mix_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream);
int wdg_acm_mix_backward_batched_f32(const wdg_acm_mix_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                                     wdg_stream_t stream);

/*
 * The same channel mix for STACKED narrow layers (csrc/acm_mix_packed.hip): a job is one layer of `reps` replicas - the splits of
 * one graph trained as one run - of `cols` real columns each, `stride` in {4, 8, 16} floats between replicas, 1 <= cols <= stride,
 * rows >= 0.  Replica p occupies columns p stride .. p stride + cols - 1 of every operand; 1, 2 or 4 adjacent lanes are one replica,
 * so one pass over the rows serves all replicas (wdg_acm_mix_batched_f32 gives the 16 lanes of a row to ONE job).
 * replaces: the use of g_high = I - A_hat, utils/util_funcs.py:198-204, in the model family behind the "mf-GCN" / "mf-SGC" tables,
 *           gnns_on_syn.py:58-104 and gnns_on_syn.py:159-206 (models that live upstream of the reference).
 * The arithmetic of replica p is the definition above, forward and backward, on its column slices, with att [reps, 3, stride] and
 * wmix [reps, 9] - and its BITS are those of a one-job wdg_acm_mix_batched_f32 / wdg_acm_mix_backward_batched_f32 launch on those
 * slices (the same ownership, the same orders of addition; tests/test_gpu_acm_packed.py compares with ==).
 *   low, high, high_agg (NULL: P_H = high), ident, out, d_out, d_low, d_high, d_ident: [rows, reps stride], each with its own
 *   leading dimension;  aux [rows, reps, 8];  d_att [reps, 3, stride];  d_wmix [reps, 9];
 *   partials: ceil(rows / 64) * reps * (3 stride + 12) floats (one vector per 64-row block and replica; no float atomics - a second
 *   launch inside the entry adds the blocks in block order).  There is no transposed output.  flags bit 0 (WDG_ACM_RELU): the whole job.
 * Padding columns (cols .. stride - 1 of a replica) count as +0 on input whatever memory holds, and are WRITTEN +0.0f in out, d_low,
 * d_high, d_ident and d_att (aggregations and the loss kernel downstream read whole rows).
 * Preconditions: 16-byte aligned low, high, high_agg, ident, out, att, aux, d_out, d_low, d_high, d_ident, d_att, partials; leading
 * dimensions that are multiples of 4 and at least reps stride.  The gradient arrays (d_out .. d_wmix, partials) come together or
 * not at all.  Outputs must not overlap inputs or each other.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per
 * grid z), max_width (the table's largest reps stride) above 64 * 65535.  n_jobs == 0: WDG_OK, nothing is launched.  The table lives
 * in device memory, so what is wrong inside a job - a stride outside {4, 8, 16}, cols outside 1 .. stride, reps < 1, rows < 0, a
 * misaligned pointer or leading dimension, a leading dimension below reps stride, a NULL required pointer - is refused by
 * wdg_acm_mix_packed_check_jobs on the HOST copy of the table (no HIP call either); a launch leaves such a job untouched.  A job of
 * 0 rows writes nothing forward and zero sums backward, and its [rows, .] arrays and partials may be NULL (att, wmix and, backward,
 * d_att and d_wmix may not); rows beyond max_rows and columns beyond max_width are left untouched.
 */
typedef struct wdg_acm_packed_job {
    const float *low, *high, *high_agg, *ident; /* [rows, reps stride] */
    const float *att;       /* [reps, 3, stride] */
    const float *wmix;      /* [reps, 9] */
    float *out;             /* forward out [rows, reps stride] */
    float *aux;             /* [rows, reps, 8]: forward out, backward in */
    const float *d_out;     /* backward in [rows, reps stride] */
    float *d_low, *d_high, *d_ident; /* backward out [rows, reps stride] */
    float *d_att;           /* backward out [reps, 3, stride] */
    float *d_wmix;          /* backward out [reps, 9] */
    float *partials;        /* backward workspace: ceil(rows / 64) * reps * (3 stride + 12) floats */
    int64_t ld_low, ld_high, ld_high_agg, ld_ident, ld_out, ld_d_out, ld_d_low, ld_d_high, ld_d_ident;
    int32_t rows, reps, cols, stride, flags, reserved;
} wdg_acm_packed_job;
int wdg_acm_mix_packed_f32(const wdg_acm_packed_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int64_t max_width, wdg_stream_t stream);
int wdg_acm_mix_packed_backward_f32(const wdg_acm_packed_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int64_t max_width,
                                    wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the packed channel mix above (utils/util_funcs.py:198-204), on the host's table */
int wdg_acm_mix_packed_check_jobs(const wdg_acm_packed_job *jobs_host, int32_t n_jobs);

/*
 * The tail of a training epoch for many models whose logits are STACKED along the feature axis - all splits ("replicas") of one
 * graph share A_hat, X and the labels, so their logits are column blocks of one [n, R cs] matrix: the cross-entropy gradient of
 * every replica's train rows, its validation and test hits and its model selection, in one pass.  A job is one graph's stacked
 * logits; n, R, C and cs are the job's own (a ragged table).
 * replaces: the accuracy of utils/util_funcs.py:393 and the loss / accuracy bookkeeping of the training loops behind the accuracy
 *           tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the loop itself lives upstream of the reference).  It stands
 *           in for the softmax / scatter / argmax / gather / where launches of sweep.TrainBatch.train_step and eval_step.
 * The definition, for row i and replica r of a job, with z_k = logits[i][r cs + k], k = 0 .. C - 1; all arithmetic in fp32, in this
 * order (tests/_xent_ref.py restates it in numpy):
 *   WDG_XENT_GRAD:
 *     split[i][r] == 1:  m = max_k z_k;  e_k = exp(z_k - m);  s = e_0 + e_1 + ... + e_{C-1} (in that order);
 *                        dlogits[i][r cs + k] = (e_k / s - [k == labels[i]]) * inv_n_train[r]
 *     otherwise:         dlogits[i][r cs + k] = +0.0f
 *     the padding columns C .. cs - 1 of every replica are written +0.0f (the backward aggregation reads whole rows); the padding
 *     columns of logits are never read; nothing beyond column R cs of a row is read or written.  A label outside 0 .. C - 1 matches no
 *     class (the rule of wdg_head_train_batched_f32).  A NaN among the z's makes all C gradients NaN: a diverged run is not hidden.
 *   WDG_XENT_EVAL:
 *     pred = the first k with z_k == m; a row with a NaN among its z's has no prediction.  A row with split code 2 (validation) or 3
 *     (test) is a hit when pred == labels[i].  After ALL rows are counted, for every r:
 *       if hits[r][0] > best[r][0] (strict):  best[r] = (hits[r][0], hits[r][1], *step_dev);      then hits[r] = (0, 0).
 *     *step_dev is read from DEVICE memory when the kernel runs: a captured epoch that also increments the word records the right
 *     step on every replay.  The selection is a second small launch inside the same call.
 * Deterministic: the hits are integer sums (per workgroup in LDS, then one integer add per workgroup and counter), there is no
 * floating-point atomic, two runs are bit-identical, and a replica's outputs do not depend on which other replicas or jobs are in
 * the table.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, flags outside 1 .. 3, a NULL step_dev
 * with WDG_XENT_EVAL, more than 65535 jobs (a job per grid z).  max_cols names the table's largest C: more than 16 classes (the class
 * limit of wdg_gnb_batched_f32) is WDG_ERR_UNSUPPORTED.  n_jobs == 0: WDG_OK, nothing is launched.  A job with n == 0 or R == 0 is
 * skipped, and so is one whose own C lies outside 1 .. 16 or whose cs < C; rows beyond max_rows (the table's largest n) are left untouched.
 */
#define WDG_XENT_GRAD 1
#define WDG_XENT_EVAL 2
typedef struct wdg_xent_job {
    const float *logits;      /* [n, R*cs] fp32, leading dimension ld_logits; replica r's classes are columns r*cs .. r*cs + C-1 */
    float *dlogits;           /* [n, R*cs], leading dimension ld_dlogits (flag GRAD) */
    const int32_t *labels;    /* [n], shared by the replicas */
    const uint8_t *split;     /* [n, R] row-major: 0 unused, 1 train, 2 validation, 3 test */
    const float *inv_n_train; /* [R]: (float)(1 / n_train_r), computed by the host */
    int32_t *hits;            /* [R, 2] work space, zero before the first call; left zero by every EVAL call */
    int32_t *best;            /* [R, 3] in/out: validation hits of the best epoch (-1: none yet), test hits at it, its step */
    int64_t ld_logits, ld_dlogits;
    int32_t n, R, C, cs;
} wdg_xent_job;
int wdg_xent_eval_batched_f32(const wdg_xent_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                              int32_t flags /* WDG_XENT_GRAD = 1, WDG_XENT_EVAL = 2, or both */,
                              const int32_t *step_dev, wdg_stream_t stream);

/*
 * The Adam step of every parameter tensor of a stacked run (split_train.SplitTrainBatch: the replicas of one model are column blocks
 * of w0 [F, R hidden] and w [F, R cs] and row blocks of w1 [R hidden, cs]) in ONE launch, with the learning rate and the weight decay
 * of every replica read from device memory - a torch parameter group has one of each per tensor - and the step count read from the
 * run's step word.  A job is one parameter TENSOR, not one replica: a run is one, two or three jobs however many replicas it holds,
 * and every access is as wide as the tensor.
 * replaces: the optimiser step (torch.optim.Adam, the L2 term in the gradient) of the training loops behind the accuracy tables
 *           gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the loop itself lives upstream of the reference, which has no model
 *           code).  In SplitTrainBatch(optimizer="device") it stands in for torch's fused Adam over the stacked parameters.
 * Segments: element (r, c) of a job belongs to segment s = (r / seg_rows) * ceil(cols / seg_cols) + c / seg_cols (integer divisions;
 * the last segment of a row or of the tensor may be ragged), and hyper[2 s], hyper[2 s + 1] are its lr and weight_decay.
 *   w0 / w: seg_rows = rows, seg_cols = hidden or cs (a replica = a column block);  w1: seg_rows = hidden, seg_cols = cols (a row block).
 * The definition, for t = *step_dev + 1 (the word wdg_xent_eval_batched_f32 records and wdg_relu_dropout_batched_f32 draws its masks
 * from: read from DEVICE memory when the kernel runs, so a captured epoch that increments the word steps correctly on every replay);
 * every operation below is ONE correctly rounded fp32 operation unless it says double, in this order, nothing fused
 * (csrc/adam.hip is compiled with contraction off; tests/_adam_ref.py restates the bits in numpy):
 *   ipow(b, t) = b^t by square and multiply in double (csrc/ipow.h: r = 1; while t: if t & 1: r *= b; b *= b; t >>= 1)
 *   step_size = (float) ((double) lr / (1.0 - ipow((double) beta1, t)))        bc2_sqrt = (float) sqrt(1.0 - ipow((double) beta2, t))
 *   g1 = g + weight_decay * p
 *   m  = beta1 * m + (1 - beta1) * g1                    (1 - beta1, 1 - beta2: fp32 subtractions)
 *   v  = beta2 * v + ((1 - beta2) * g1) * g1
 *   p  = p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps))
 * - wdg_head_train_batched_f32's step with the multiply-adds written out.  An element depends on its own four inputs, its segment's
 * two numbers and t: a job's result does not depend on the table it is in, there are no atomics, and two launches from the same
 * inputs give the same bits.  A NaN gradient makes that element's p, m and v NaN and no other element's.  g = 0 with p = 0 leaves
 * p, m and v at +0.0f for eps > 0 (the padding columns of a stacked run stay zero).  lr = 0 leaves p unchanged (while the quotient is
 * finite) and still advances m and v.
 * p, m and v of a job must not overlap each other or g, and no two jobs may share an element (the front end checks the first).
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, a NULL step_dev, a beta outside
 * [0, 1), an eps that is not a number, more than 65535 jobs (a job per grid z), more than 64 * 65535 columns (a tile per grid y).
 * The table lives in device memory, so what is wrong inside a job - seg_rows < 1 or seg_cols < 1 on a non-empty job, ld or ld_s
 * below cols, a NULL pointer - is refused by wdg_adam_check_jobs on the HOST copy of the table (ops.AdamBatch calls it before it
 * uploads; no HIP call either); a launch leaves such a job untouched.  n_jobs == 0: WDG_OK, nothing is launched.  A job of 0 rows or
 * 0 columns is skipped; rows beyond max_rows (the table's largest) are left untouched, and so is a job of more than max_cols columns.
 */
typedef struct wdg_adam_job {
    float *p;            /* [rows, cols], leading dimension ld: a parameter, updated IN PLACE */
    const float *g;      /* [rows, cols], leading dimension ld: its gradient */
    float *m, *v;        /* [rows, cols], leading dimension ld_s: first / second moment, in/out */
    const float *hyper;  /* device, [segments, 2]: lr, weight_decay of a segment */
    int64_t ld, ld_s;
    int32_t rows, cols, seg_rows, seg_cols;
} wdg_adam_job;
int wdg_adam_batched_f32(const wdg_adam_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                         float beta1, float beta2, float eps, const int32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the optimiser step above (gnns_on_syn.py:109-154), on the host's table */
int wdg_adam_check_jobs(const wdg_adam_job *jobs_host, int32_t n_jobs);

/*
 * Keep the selected model of a stacked run: copy, of every tensor of a table, exactly the segments of the replicas whose best epoch
 * is the CURRENT step, in one launch - the parameters and the logits of a replica at its best validation epoch stay behind in `dst`
 * while the run goes on, with no host in the epoch.  A job is one TENSOR (wdg_adam_batched_f32's convention), not one replica.
 * replaces: the bookkeeping of the training loops behind the accuracy tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the
 *           loop itself lives upstream of the reference, where it keeps the selected model) - what wdg_xent_eval_batched_f32 cites.
 * The definition, for element (i, j) of a job:
 *   s = (i / seg_rows) * ceil(cols / seg_cols) + j / seg_cols     (integer divisions: wdg_adam_batched_f32's rule; the last segment of
 *                                                                  a row or of the tensor may be ragged)
 *   r = s % reps                                                  (the channel-major ACM weights [F, 3 R w] are one job: 3 R segments)
 *   t = *step_dev, read from DEVICE memory when the kernel runs
 *   dst[i][j] = src[i][j]   iff   best[3 r] >= 0 && best[3 r + 2] == t
 * The copy is of the 32-bit word: NaN payloads and the sign of zero survive.  Every other element of dst is neither read nor
 * written, and the src elements of unselected segments are not loaded; nothing outside columns 0 .. cols - 1 of a row is touched.
 * PRECONDITION: the launch comes after the WDG_XENT_EVAL call of the same step and before the step word advances.  That call writes
 * best[r][2] = *step_dev exactly for the replicas whose validation hits improved; every step recorded earlier is smaller, and the
 * first selection always improves on -1 - so "best[r][2] == t" means "replica r was selected in this step".
 * Access width, per job: 16-byte accesses when src and dst are 16-byte aligned and seg_cols, ld_src and ld_dst are multiples of 4
 * (four adjacent columns then share a segment); word by word otherwise and at a ragged right edge.  Both paths move the same bits.
 * No LDS, no atomics: an element depends on its own source word, its replica's two numbers and t; a job's result does not depend on
 * the table it is in, and two launches from the same inputs give the same bits.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, a NULL step_dev, negative counts, more than 65535
 * jobs (a job per grid z), more than 64 * 65535 columns (a tile per grid y).  These come FIRST, in this order of precedence: a NULL
 * step_dev is refused even when n_jobs == 0 (wdg_adam_batched_f32's order); only then n_jobs == 0: WDG_OK, nothing is launched; a NULL
 * table is looked at after that (n_jobs > 0 only).  The table
 * lives in device memory, so what is wrong inside a job - seg_rows, seg_cols or reps below 1, ld_src or ld_dst below cols, a NULL
 * pointer, src and dst that overlap (their byte ranges intersect, unless both have one leading dimension and their column ranges
 * are disjoint inside it: column ranges of one wider matrix) - makes the kernel SKIP the job, and wdg_keep_best_check_jobs applies
 * the same predicate to the HOST copy of the table (ops.KeepBestBatch calls it before it uploads; no HIP call either).  A job of 0
 * rows or 0 columns is skipped; rows beyond max_rows (the table's largest) are left untouched, and so is a job of more than max_cols
 * columns.  No two jobs may share an element of a dst.
 */
typedef struct wdg_keep_job {
    const float *src; float *dst; /* [rows, cols], leading dimensions ld_src / ld_dst */
    const int32_t *best;      /* [reps, 3], wdg_xent_job.best */
    int64_t ld_src, ld_dst;
    int32_t rows, cols, seg_rows, seg_cols, reps, reserved;
} wdg_keep_job;
int wdg_keep_best_batched_f32(const wdg_keep_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                              const int32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the conditional copy above (gnns_on_syn.py:109-154), on the host's table */
int wdg_keep_best_check_jobs(const wdg_keep_job *jobs_host, int32_t n_jobs);

/*
 * Predictions and confusion counts of many models whose logits are STACKED along the feature axis (wdg_xent_eval_batched_f32's
 * layout: replica r's classes are columns r cs .. r cs + C - 1 of one [n, R cs] matrix), per replica and per part of its split.
 * replaces: the accuracy of utils/util_funcs.py:393 taken apart by class - the per-class view of the models the accuracy tables
 *           gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 train (the loop itself lives upstream of the reference).
 * The definition, for row i and replica r of a job, with z_k = logits[i][r cs + k], k = 0 .. C - 1 (tests/_confusion_ref.py restates it):
 *   pred = the first k with z_k == max_k z_k - exactly WDG_XENT_EVAL's prediction; a NaN among the z's gives no prediction.
 *   pred[i][r] = pred, or 255 for none (where the job has a pred matrix) - for EVERY row, whatever its split code and label.
 *   if s = split[i][r] is in 1 .. 3 and y = labels[i] is in 0 .. C - 1:   counts[r][s - 1][y][pred, or C for none] += 1
 *   a row with split code 0 (or above 3) or a label out of range is not counted.
 * The counts are ADDED to what `counts` holds (the front end zeroes its pool before the launch).  They are integers: counted per
 * workgroup in LDS, then one integer add per workgroup and non-zero counter.  No floating-point atomics: two runs are bit-identical,
 * and a replica's counts do not depend on which other replicas or jobs are in the table.  The padding columns C .. cs - 1 of the
 * logits are never read; nothing beyond column R cs of a row is read.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per
 * grid z).  max_cols names the table's largest C: more than 16 classes is WDG_ERR_UNSUPPORTED.  n_jobs == 0: WDG_OK, nothing is
 * launched.  A job with n == 0 or R == 0 is skipped, and so is one whose own C lies outside 1 .. 16, whose cs < C, whose ld_logits
 * is below R cs or whose logits, labels, split or counts pointer is NULL; wdg_confusion_check_jobs refuses such a job (other than
 * an empty one) on the HOST copy of the table.  Rows beyond max_rows (the table's largest n) are left untouched.
 */
typedef struct wdg_confusion_job {
    const float *logits;      /* [n, R*cs] fp32, leading dimension ld_logits */
    const int32_t *labels;    /* [n], shared by the replicas */
    const uint8_t *split;     /* [n, R] row-major: 0 unused, 1 train, 2 validation, 3 test */
    int32_t *counts;          /* [R, 3, C, C+1] in/out: part (train, validation, test), true class, predicted class (C: none) */
    uint8_t *pred;            /* [n, R] or NULL: the prediction, 255 for none */
    int64_t ld_logits;
    int32_t n, R, C, cs;
} wdg_confusion_job;
int wdg_confusion_batched_i32(const wdg_confusion_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the confusion counts above (utils/util_funcs.py:393), on the host's table */
int wdg_confusion_check_jobs(const wdg_confusion_job *jobs_host, int32_t n_jobs);

/*
 * The evaluation of a training epoch for many models whose logits are STACKED along the feature axis (wdg_xent_eval_batched_f32's
 * layout: replica r owns columns r cs .. r cs + C - 1 of one [n, R cs] matrix), WITH the losses: per replica the mean cross-entropy
 * and the hits of its train, validation and test rows, a row of its learning curve, its model selection by one of three rules and its
 * patience counter - all on the device, inside a captured epoch.  A job is one graph's stacked logits (a ragged table).
 * replaces: the accuracy of utils/util_funcs.py:393 and the loss / accuracy / early-stopping bookkeeping of the training loops behind
 *           the accuracy tables gnns_on_syn.py:109-154 and gnns_on_syn.py:213-249 (the loop itself lives upstream of the reference;
 *           the selection rules are DEFINED here and are not claimed to reproduce its tables).  It stands in for the WDG_XENT_EVAL
 *           call of wdg_xent_eval_batched_f32 where a run asks for losses, another selection rule, a patience or a learning curve.
 * The definition of one call with the step word at s = *step_dev (read from DEVICE memory when the kernel runs), for row i and replica
 * r of a job, z_k = logits[i][r cs + k], k = 0 .. C - 1, part p = split[i][r] - 1 in {0 train, 1 validation, 2 test} (other codes: the
 * row is not looked at); tests/_curve_ref.py restates it in numpy.  All per-row arithmetic in fp32, in this order:
 *     m = max_k z_k;  e_k = exp(z_k - m);  sum = e_0 + e_1 + ... + e_{C-1} (in that order);  term = log(sum) - (z_label - m)
 *   H[r][p] = the rows whose prediction equals labels[i]; the prediction is the first k with z_k == m, and a row with a NaN among its
 *             z's has none (WDG_XENT_EVAL's rule).
 *   S[r][p] = the fp64 sum of the terms, each widened to fp64, IN THIS ORDER: the rows are cut into blocks of 32 (rows 32 b .. 32 b + 31);
 *             a block's partial starts at +0.0 and takes the terms of its rows of part p in ascending row order; S starts at +0.0 and
 *             takes the partials of the blocks 0 .. ceil(n / 32) - 1 in ascending order (blocks without a row of the part add their +0.0).
 *             The order depends on the job's own n alone: not on R, the other jobs of the table, max_rows or which run it is.
 *   L[r][p] = (float) (S[r][p] / n_part[r][p]), or NaN when n_part[r][p] <= 0.
 *   A row whose label lies outside 0 .. C - 1 adds nothing to S and is no hit.  A NaN among the z's of a counted row makes its term,
 *   and with it L[r][p], NaN.  The padding columns C .. cs - 1 are never read; nothing beyond column R cs of a row is read.
 * Curve:      if 0 <= s < curve_rows:  curve_loss[s][r][:] = L[r][:], curve_hits[s][r][:] = H[r][:]; no other row is written.
 * Selection:  only while state[r][1] (stopped_at) < 0; Hv = H[r][1], Lv = L[r][1]:
 *     rule 0 (val_hits):            improved = Hv > best[r][0]
 *     rule 1 (val_loss):            improved = Lv < best_loss[r][1]
 *     rule 2 (val_hits_then_loss):  improved = Hv > best[r][0] || (Hv == best[r][0] && Lv < best_loss[r][1])
 *     (a NaN makes every comparison false)
 *     improved:   best[r] = (Hv, H[r][2], s), best_loss[r][:] = L[r][:], bad = 0;        otherwise: bad += 1
 *     then, if patience > 0 && bad >= patience:  stopped_at = s.
 *   A stopped replica's best, best_loss and state never change again; its curve rows are still written.  With rule 0 and patience 0,
 *   best is what WDG_XENT_EVAL leaves.
 * Two launches: one over the rows (the terms of a row block in LDS, then one thread per replica adds them in row order and STORES the
 * block's partials; the hits are integer adds to `hits`), one that finishes (sums, means, curve, selection; `hits` back to zero).
 * No floating-point atomic: two calls from the same inputs give the same bits, inside any table.
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per grid
 * z), a NULL step_dev.  max_cols names the table's largest C: more than 16 classes is WDG_ERR_UNSUPPORTED.  n_jobs == 0: WDG_OK, nothing
 * is launched.  The table lives in device memory, so what is wrong inside a job - a rule outside 0 .. 2, a negative patience, negative
 * curve_rows or curve_rows > 0 without both curve buffers, C outside 1 .. 16, cs < C, ld_logits below R cs, a NULL pointer - is refused
 * by wdg_xent_curve_check_jobs on the HOST copy of the table (ops.XentCurveBatch calls it before it uploads; no HIP call either), and
 * both launches SKIP such a job without touching its memory.  A job with n == 0 or R == 0 is skipped; rows beyond max_rows (the
 * table's largest n) are not looked at.
 */
typedef struct wdg_xent_curve_job {
    const float *logits;      /* [n, R*cs] fp32, leading dimension ld_logits */
    const int32_t *labels;    /* [n], shared by the replicas */
    const uint8_t *split;     /* [n, R] row-major: 0 unused, 1 train, 2 validation, 3 test */
    const int32_t *n_part;    /* [R, 3]: the train, validation and test rows of a replica, counted by the host */
    int32_t *best;            /* [R, 3] in/out: wdg_xent_job.best - validation hits of the best step (-1: none yet), test hits at it, the step */
    float *best_loss;         /* [R, 3] in/out: L[r][:] of the best step; +inf before the first */
    int32_t *state;           /* [R, 2] in/out: bad (steps since the last improvement), stopped_at (-1: running) */
    float *curve_loss;        /* [curve_rows, R, 3], or NULL with curve_rows == 0 */
    int32_t *curve_hits;      /* [curve_rows, R, 3], or NULL with curve_rows == 0 */
    int32_t *hits;            /* [R, 3] work space: zero before the first call, left zero by every call */
    double *partials;         /* work space of wdg_xent_curve_partials_len(n, R) doubles: written before it is read, any contents */
    int64_t ld_logits;
    int32_t n, R, C, cs;
    int32_t rule, patience, curve_rows, reserved;
} wdg_xent_curve_job;
int wdg_xent_curve_batched_f32(const wdg_xent_curve_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols,
                               const int32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the evaluation above (gnns_on_syn.py:109-154), on the host's table */
int wdg_xent_curve_check_jobs(const wdg_xent_curve_job *jobs_host, int32_t n_jobs);
/* replaces: nothing of its own - the doubles of a job's `partials`: ceil(n / 32) * R * 3 (0 for an empty job) (gnns_on_syn.py:109-154) */
int64_t wdg_xent_curve_partials_len(int32_t n, int32_t R);

/*
 * The exact ROC-AUC of many BINARY models whose logits are STACKED along the feature axis (wdg_xent_job's layout: replica r owns
 * columns r cs and r cs + 1 of one [n, R cs] matrix; the job carries no C, it is 2), per replica and per part of its split, as two
 * integers - with a model selection on the validation AUC, a patience counter and a curve row, all on the device, inside a captured
 * epoch.  A job is one graph's stacked logits (a ragged table).
 * replaces: nothing the reference computes - its only score is the accuracy of utils/util_funcs.py:393, while five of the seven large
 *           data sets its command line accepts (homophily_tests.py:30) are binary and two of the loaders beside them, load_yelpchi_dataset
 *           (utils/datasets.py:82) and load_genius (utils/datasets.py:197), give labels of roughly 85/15 and 80/20, which upstream scores
 *           by ROC-AUC.  It stands in for a copy of the logits to the host and sklearn.metrics.roc_auc_score per replica and epoch.
 * The definition of one call with the step word at s = *step_dev (read from DEVICE memory when the kernel runs); tests/_auc_ref.py
 * restates it in numpy.  For row i and replica r:
 *   score  d = z_1 - z_0 = logits[i][r cs + 1] - logits[i][r cs]: ONE fp32 subtraction, no exponential.
 *   part   p = split[i][r] - 1 in {0 train, 1 validation, 2 test}; a row with another code is not looked at.
 *   pos(r, p) = the rows of the part with labels[i] == 1, neg(r, p) = those with labels[i] == 0; rows with any other label are not looked at.
 *   pairs[r][p] = |pos| |neg|
 *   u2[r][p]    = sum over i in pos, j in neg of (2 [d_j < d_i] + [d_j == d_i])          both int64; AUC = u2 / (2 pairs), the caller's
 *                 division (NaN when pairs == 0).
 *   The comparisons are IEEE's: -0.0 == +0.0, -inf < every finite number < +inf, inf == inf.  A NaN d (inf - inf included) among the
 *   rows of pos or neg makes u2[r][p] = -1; pairs still counts the row.
 * Curve:      if 0 <= s < curve_rows:  curve_u2[s][r][:] = u2[r][:]; no other row is written.
 * Selection:  only when select == 1 and while state[r][1] (stopped_at) < 0:
 *     improved = u2[r][1] >= 0 && u2[r][1] > best_u2[r][1]        (strict: the earliest of equal steps wins; best_u2 starts at -1)
 *     improved:   best_u2[r][:] = u2[r][:], best[r] = (0, 0, s), bad = 0;        otherwise: bad += 1
 *     then, if patience > 0 && bad >= patience:  stopped_at = s.
 *   `best` [R, 3] int32 starts at (-1, 0, 0) and keeps the meaning wdg_keep_best_batched_f32 reads: best[3 r] >= 0 && best[3 r + 2] == t.
 * The route (csrc/auc.hip) sorts nothing: a key = the monotone uint32 image of d (-0 mapped to +0 first); an integer histogram of
 * bin = key >> (32 - bins_log2) per (r, p, class); a scan per replica that adds the pairs ACROSS bins, 2 pos[b] (negatives in lower
 * bins), and turns the counts into offsets; a scatter of the keys into bin-contiguous arrays through an integer cursor per bin (the
 * order inside a bin is arbitrary and no count depends on it); the pairs INSIDE a bin counted against tiles of its negatives in LDS
 * (a bin larger than the tile loops over tiles); a finishing launch.  Every sum is a sum of integers (integer atomics); there is no
 * floating-point atomic: two calls from the same inputs give the same bits, and a replica's numbers do not depend on the table it is
 * in, on max_rows or on bins_log2.  bins_log2 only moves work between the scan (bins) and the in-bin count (rows of a bin, squared):
 * all scores equal puts a part into ONE bin, and the call then costs |pos| |neg| comparisons - quadratic in the part's rows.
 * Five launches on `stream`; the last one leaves the work space as it found it (zero where zero is asked for), so a captured call
 * replays without a memset of its own.
 * Refused before any HIP call (WDG_ERR_INVALID), in this order: negative counts, a NULL step_dev, more than 65535 jobs (a job per grid
 * z), a NULL table with n_jobs > 0.  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  The table lives in device memory, so
 * what is wrong inside a job - cs < 2, ld_logits below R cs (with n > 1), bins_log2 outside 1 .. 16, select outside 0 .. 1, a negative
 * patience or curve_rows, curve_rows > 0 without curve_u2, a negative n or R, a NULL pointer or a work space that is not 8-byte
 * aligned - is refused by wdg_auc_check_jobs on the HOST copy of the table (ops.AucBatch calls it before it uploads; no HIP call
 * either), and every launch SKIPS such a job without touching its memory.  A job with n == 0 or R == 0 is skipped; rows beyond
 * max_rows (the table's largest n) are not looked at.
 */
typedef struct wdg_auc_job {
    const float *logits;      /* [n, R*cs] fp32, leading dimension ld_logits; columns r cs and r cs + 1 are read */
    const int32_t *labels;    /* [n], shared by the replicas */
    const uint8_t *split;     /* [n, R] row-major: 0 unused, 1 train, 2 validation, 3 test */
    int64_t *u2;              /* [R, 3] out */
    int64_t *pairs;           /* [R, 3] out */
    int64_t *best_u2;         /* [R, 3] in/out: u2[r][:] of the best step; -1 before the first */
    int32_t *best;            /* [R, 3] in/out: (0, 0, the best step); (-1, 0, 0) before the first */
    int32_t *state;           /* [R, 2] in/out: bad (steps since the last improvement), stopped_at (-1: running) */
    int64_t *curve_u2;        /* [curve_rows, R, 3], or NULL with curve_rows == 0 */
    void *work;               /* wdg_auc_workspace_bytes(n, R, bins_log2) bytes, 8-byte aligned: ZERO before the first call, left zero by every call */
    int64_t ld_logits;
    int32_t n, R, cs, bins_log2;
    int32_t select, patience, curve_rows, reserved;
} wdg_auc_job;
int wdg_auc_batched_i64(const wdg_auc_job *jobs_dev, int32_t n_jobs, int32_t max_rows, const int32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the AUC above (utils/util_funcs.py:393), on the host's table */
int wdg_auc_check_jobs(const wdg_auc_job *jobs_host, int32_t n_jobs);
/* replaces: nothing of its own - the bytes of a job's `work` (utils/util_funcs.py:393): with B = 2^bins_log2, 72 R of sums and counts,
 *           36 R B of bin counters and bin starts, 4 n R of keys; 0 for an empty job, -1 for bins_log2 outside 1 .. 16 */
int64_t wdg_auc_workspace_bytes(int32_t n, int32_t R, int32_t bins_log2);

/*
 * Y = S W for a SPARSE S and a dense W, a table of products per launch: the first layer of a stacked run on a bag-of-words feature
 * matrix, X [W0_1 | ... | W0_R], and its weight gradient X^T dP, without the dense X (sparse_features.DeviceFeatures).
 * replaces: th.FloatTensor(features) / .todense() utils/util_funcs.py:339 - the densification in front of the first torch call - for
 *           the two products that read X: the job keeps S as the CSR it is on disk.
 * A job: S is CSR - rowptr int32 [n_rows + 1], col int32 sorted ascending and unique inside a row, val fp32 or NULL (= every stored
 * value is 1.0) - with n_cols columns; W [n_cols, m] fp32 with leading dimension ldw, Y [n_rows, m] fp32 with leading dimension ldy.
 * The definition (tests/_sparse_dense_ref.py restates it in numpy, bit for bit):
 *   Y[i][j] = the chain   acc = +0;  for e = rowptr[i] .. rowptr[i + 1] - 1 ascending:  acc = fmaf(val[e], W[col[e]][j], acc)
 *   - one correctly rounded fma per stored entry, the SAME chain for a row of any length: no row is split over lanes or waves, no
 *   partial sums are added, there is no atomic (csrc/sparse_dense.hip is compiled with contraction off and writes the fma out).
 *   wdg_gemm_f32 is this chain over every k in ascending order, and fmaf(0, w, acc) = acc for a finite w: on a W without inf / NaN
 *   the result has the bits of wdg_gemm_f32 on the expanded S wherever that takes its single chain (wdg_gemm_splitk_plan == 1).
 *   Every element of Y[0 : n_rows][0 : m] is written; an empty row gives +0.  Nothing outside that block is written - not the columns
 *   m .. ldy - 1 of a wider Y.  Two launches from the same inputs give the same bits, and a job's bits do not depend on the table it
 *   is in, on max_rows, max_m or on where its workgroups run.
 *   m >= 1 and leading dimensions >= m of any value: 16-byte loads / stores where the pointer, the leading dimension and the four
 *   columns of a lane allow, scalar ones elsewhere (same values, same fma).
 *   An entry whose column lies outside [0, n_cols) is SKIPPED (no fma), never read through: the guard of wdg_features_expand_batched_f32.
 *   order: int32 [n_rows] or NULL - the sequence in which the rows are dealt to the waves (position p works on row order[p]; NULL: p),
 *   nothing else: a permutation with the longest rows first lets the longest chain, which bounds the launch, start first.  A position
 *   whose entry lies outside [0, n_rows) is skipped (its row is then written by nobody).
 * max_rows, max_m: the largest n_rows and m of the table (rows / columns beyond them are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID), in this order: negative counts, more than 65535 jobs (a job per grid y); then
 * n_jobs == 0, max_rows == 0 or max_m == 0 is WDG_OK with nothing launched; then a NULL table.  The table lives in device memory: what
 * is wrong inside a job - a negative n_rows, n_cols or m, a leading dimension below m, a NULL rowptr or Y, a NULL col or W with
 * n_cols > 0, a reserved word that is not 0 - is refused by wdg_sparse_dense_check_jobs on the HOST copy of the table
 * (sparse_features.SparseDenseBatch calls it before it uploads), and the launch leaves such a job untouched.  A job with n_rows == 0
 * or m == 0 is skipped.
 */
typedef struct wdg_sparse_dense_job {
    const int32_t *rowptr;  /* [n_rows + 1] */
    const int32_t *col;     /* [nnz], sorted and unique inside a row */
    const float *val;       /* [nnz] or NULL = 1.0 */
    const int32_t *order;   /* [n_rows] or NULL: the sequence in which rows are dealt */
    const float *W;         /* [n_cols, m], leading dimension ldw */
    float *Y;               /* [n_rows, m], leading dimension ldy */
    int64_t ldw, ldy;
    int32_t n_rows, n_cols, m, reserved;
} wdg_sparse_dense_job;
int wdg_sparse_dense_batched_f32(const wdg_sparse_dense_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_m, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the sparse product above (utils/util_funcs.py:339), on the host's table */
int wdg_sparse_dense_check_jobs(const wdg_sparse_dense_job *jobs_host, int32_t n_jobs);
/*
 * The stored values of a CSR feature matrix under preprocess_features' row scaling, once, in CSR order and in the order of its
 * transposed layout - what the two sparse products above read as `val`.
 * replaces: preprocess_features utils/util_funcs.py:39-46 (normalise WDG_FEAT_NORM_SUM) and f.normalize homophily_tests.py:94
 *           (WDG_FEAT_NORM_ABS) on the stored entries instead of on the dense matrix of utils/util_funcs.py:339.
 * val_scaled[e] = what wdg_features_expand_batched_f32 writes at entry e's position under the same `normalise`, bit for bit: the two
 * kernels share the row sum's order and the scale (csrc/feat_scale.h) - the fp64 sum over the row's entries (an entry whose column is
 * outside [0, n_feat) left out), s = (float)sum, WDG_FEAT_NORM_SUM: r = 1.0f / s, inf -> 0, y = r * x; WDG_FEAT_NORM_ABS: the sum over
 * |x|, y = x / fmaxf(s, 1e-12f); WDG_FEAT_NORM_NONE: y = x.  val NULL = every stored value is 1.0.
 * t_src int32 [nnz] or NULL: entry e of the transposed layout is CSR entry t_src[e]; t_val_scaled[e] = val_scaled[t_src[e]] (+0 for
 * a t_src[e] outside [0, nnz)).  t_src and t_val_scaled are both given or both NULL.  Two launches on `stream`.
 * Refused before any HIP call: negative counts, a normalise that is none of WDG_FEAT_NORM_*; then n_rows == 0 or nnz == 0 is WDG_OK
 * with nothing launched; then a NULL rowptr, col or val_scaled, and t_src without t_val_scaled or the reverse.
 */
int wdg_feat_scaled_values_f32(const int32_t *rowptr, const int32_t *col, const float *val, int32_t n_rows, int32_t n_feat, int normalise,
                               const int32_t *t_src, int32_t nnz, float *val_scaled, float *t_val_scaled, wdg_stream_t stream);

/*
 * Graph attention for many graphs in one launch, and its backward pass: a weight per stored entry, learnt, where every other
 * aggregation of this library takes weights fixed before the launch.  The reference ships no model code: the layer is DEFINED here
 *  and is not claimed to reproduce an upstream table.
 * replaces: the fixed weights of normalize_tensor, utils/util_funcs.py:365-381, in the aggregation, for the attention baseline that
 *           stands beside the GCN / SGC tables of gnns_on_syn.py:1-154 (models that live upstream of the reference).
 * A job: a square CSR PATTERN of n rows - rowptr int32 [n + 1], col int32 [nnz], columns strictly ascending inside a row; stored
 * values and scales are ignored -, heads in 1..8 of width w >= 1 with heads w <= 256, H [n, heads w], S [n, 2 heads] (S[:, h] the
 * row's own score, S[:, heads + h] its score as a neighbour: the caller's product S = H blockdiag(a_dst, a_src)), slope >= 0.
 * The definition, for row i, head h and the row's stored entries p in ascending order, j = col[p]:
 *   pre_p = S[i, h] + S[j, heads + h]          e_p = pre_p > 0 ? pre_p : slope * pre_p
 *   m = max_p e_p          q_p = expf(e_p - m)          Z = sum_p q_p          alpha_p = q_p / Z   (a correctly rounded division)
 *   out[i, h w + k] = sum_p alpha_p H[j, h w + k]     ONE fmaf chain from +0 over ascending p: acc = fmaf(alpha_p, H[j, .], acc)
 *   alpha[p, h] = alpha_p                              [nnz, heads] contiguous: kept for the backward pass and for the caller
 * The backward pass, g = d_out[i, :]:
 *   dalpha_p = sum_k g[h w + k] H[j, h w + k]          ONE fmaf chain from +0 over ascending k
 *   c = sum_p alpha_p dalpha_p                         t_p = dalpha_p - c     u_p = alpha_p * t_p
 *   dpre_p = u_p * (pre_p > 0 ? 1 : slope)  -> d_pre[p, h] (workspace [nnz, heads])          d_S[i, h] = sum_p dpre_p
 * and, over the TRANSPOSED pattern (t_rowptr, t_col; entry q of row j has source row i = t_col[q] and is forward entry p = t_pos[q]):
 *   d_H[j, h w + k] = sum_q alpha[p, h] d_out[i, h w + k]     ONE fmaf chain from +0 over ascending q
 *   d_S[j, heads + h] = sum_q d_pre[p, h]
 * The order of the other sums is fixed too.  A sum over a row's entries - Z, c, d_S[i, h], d_S[j, heads + h] - numbers the entries
 * 0, 1, ... from the row's first: lane l of 64 adds the entries l, l + 64, l + 128, ... in ascending order from +0 (c: acc =
 * fmaf(alpha_p, dalpha_p, acc); the others: acc = acc + term), and the 64 lane sums are then added by a butterfly over lane distances
 * 32, 16, 8, 4, 2, 1, each step v = v + v[lane ^ distance].  The maximum is taken with fmaxf - it skips a NaN - and its value does not
 * depend on an order.  There are no floating-point atomics.  csrc/gat.hip is compiled with contraction off and writes every fmaf out.
 * An empty row writes out = +0 (and +0 gradients) and no alpha.  A NaN stays a NaN: one in row j of H reaches out[i, :] of exactly
 * the rows i that store j, one in d_out[i, :] reaches d_H[j, :] of exactly the columns j that row i stores.  An element depends on
 * its row, or its transposed row, alone, and a job on the job alone: a job answers in a table what it answers alone, and head h of
 * a job has the bits of a one-head job on that head's column slices (every matrix has its own leading dimension: slices are passed
 * in place).  Outputs must not overlap inputs or each other.  16-byte accesses where a matrix's pointer and leading dimension allow,
 * scalar ones elsewhere: the same values.
 * Guards: an entry whose column lies outside [0, n) - or whose t_pos lies outside [0, nnz) - is skipped, never read through; a row
 * whose extent lies outside [0, nnz] is left untouched, and so is a job outside the limits.
 * max_rows: the table's largest n (rows beyond it are not worked on).  wdg_gat_backward_batched_f32 is two launches: the row pass,
 * then the pass over the transposed pattern; it reads the alpha of the last forward launch.
 * Refused before any launch (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per grid
 * z).  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  The table lives in device memory: what is wrong inside a job - heads
 * outside 1..8, w < 1, heads w > 256, a slope that is negative or a NaN, flags other than 0, a negative n or nnz, a NULL rowptr, H, S or
 * out, a NULL col or alpha with nnz > 0, a leading dimension below the row, the backward pointers (d_out, d_H, d_S, t_rowptr; d_pre,
 * t_col, t_pos with nnz > 0) given in part - is refused by wdg_gat_check_jobs on the HOST copy of the table (train.GatBatch calls it
 * before it uploads).  A job with n == 0 is skipped.
 */
#define WDG_GAT_MAX_HEADS 8
#define WDG_GAT_MAX_COLS 256
typedef struct wdg_gat_job {
    const int32_t *rowptr;    /* [n + 1] */
    const int32_t *col;       /* [nnz], strictly ascending inside a row */
    const int32_t *t_rowptr;  /* [n + 1]: the transposed pattern (backward), or NULL */
    const int32_t *t_col;     /* [nnz] */
    const int32_t *t_pos;     /* [nnz]: the forward entry of every transposed entry (wdg_csr_transpose_positions) */
    const float *H;           /* [n, heads w] */
    const float *S;           /* [n, 2 heads] */
    float *out;               /* forward out [n, heads w] */
    float *alpha;             /* [nnz, heads]: forward out, backward in */
    const float *d_out;       /* backward in [n, heads w] */
    float *d_H;               /* backward out [n, heads w] */
    float *d_S;               /* backward out [n, 2 heads] */
    float *d_pre;             /* backward workspace [nnz, heads] */
    int64_t ld_h, ld_s, ld_out, ld_d_out, ld_d_h, ld_d_s;
    int32_t n, heads, w, flags; /* flags: 0 (none is defined) */
    float slope;
    int32_t nnz;              /* rowptr[n]: the extent of col, alpha and d_pre */
} wdg_gat_job;
int wdg_gat_forward_batched_f32(const wdg_gat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
/* replaces: nothing of its own - the backward pass of the layer above (utils/util_funcs.py:365-381) */
int wdg_gat_backward_batched_f32(const wdg_gat_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the layer above (utils/util_funcs.py:365-381), on the host's table */
int wdg_gat_check_jobs(const wdg_gat_job *jobs_host, int32_t n_jobs);
/*
 * t_pos of wdg_gat_job: for every entry q of the transposed CSR (row j, t_col[q] = i) the position p of the forward entry (i, j),
 * found by binary search in forward row i; -1 where there is none.
 * replaces: nothing of the reference - torch autograd transposes the dense A_hat of utils/util_funcs.py:365-381 by itself.
 * bad_dev: one int32 word in device memory, cleared and then COUNTED into: the transposed entries without a match, and the rows
 * of either pattern whose columns are not strictly ascending inside [0, n) or whose extent is not inside the pattern.  A non-zero
 * count marks a pattern with duplicates or unsorted rows, or two patterns that are not each other's transpose (together with equal
 * entry counts, zero proves the bijection).  Refused before any HIP call: a negative n, a NULL count word, NULL row pointers.
 */
int wdg_csr_transpose_positions(const int32_t *rowptr, const int32_t *col, const int32_t *t_rowptr, const int32_t *t_col, int32_t n,
                                int32_t *t_pos, int32_t *bad_dev, wdg_stream_t stream);

/*
 * The attention SCORES of many stacked layers in one launch, and their backward pass: S = H blockdiag(a_dst, a_src) without the
 * operand - of a stacked run's [R heads w, 2 R heads] one part in R is not zero - and without a transposed copy of H for its gradient.
 * replaces: the product that forms wdg_gat_job's S for the layer above (utils/util_funcs.py:365-381), for all replicas of a stacked run.
 * A job: n rows, G groups of w columns each, a block size `heads` in 1..8; H [n, G w], S [n, 2 G], att [2, G w] (plane 0 = a_dst,
 * plane 1 = a_src, [G, w] each; ld_att floats lie between the planes), and for the backward pass d_S [n, 2 G], d_H [n, G w],
 * d_att [2, G w] (ld_d_att between its planes) and a workspace `partial` of wdg_gat_scores_partial_len(n, G, w) floats at a 16-byte
 * boundary.  Every matrix has its own leading dimension and unit inner stride: column slices are passed in place.
 * Score columns: the groups are cut into consecutive blocks of `heads`; the last block may be shorter.  Block b = g / heads holds
 * hb = min(heads, G - heads b) groups, and its group g has   dst(g) = 2 heads b + (g - heads b)   and   src(g) = dst(g) + hb:  a block's
 * dst scores, then its src scores - the S a wdg_gat_job of hb heads reads as the column slice 2 heads b .. 2 heads b + 2 hb.
 * The arithmetic (csrc/gat_scores.hip is compiled with contraction off and writes every fmaf out; tests/_gat_scores_ref.py restates it):
 *   forward    S[i, dst(g)] = ONE fmaf chain from +0 over ascending k:  acc = fmaf(H[i, g w + k], a_dst[g, k], acc);  S[i, src(g)]: a_src
 *   backward   d_H[i, g w + k] = fmaf(d_S[i, src(g)], a_src[g, k], fmaf(d_S[i, dst(g)], a_dst[g, k], d_H[i, g w + k]))
 *              - d_H is ADDED to: the attention kernel's d_H is there already -;
 *              the rows are cut into blocks of WDG_GAT_SCORES_ROW_BLOCK from row 0; per block b and element (p, g, k),
 *              partial[b, p, g w + k] = ONE chain from +0 over the block's rows ascending: acc = fmaf(d_S[i, p ? src(g) : dst(g)], H[i, g w + k], acc),
 *              and d_att[p, g w + k] = the blocks' sums added in ascending b from +0: acc = acc + partial[b, p, g w + k].
 * No floating-point atomics; an element depends on its row (forward, d_H) or its column (d_att) of its job alone: a job has the same bits
 * alone and in any table, and a second launch repeats the first (given d_H as it was).  A NaN in H[i, g w + k] reaches S[i, dst(g)],
 * S[i, src(g)] and d_att[:, g w + k], nothing else.  16-byte accesses where every pointer and leading dimension of a pass and w allow - one
 * decision per job -, scalar ones elsewhere: the same values.  Outputs must not overlap inputs or each other.
 * Limits: heads in 1..WDG_GAT_SCORES_MAX_HEADS, w in 1..WDG_GAT_SCORES_MAX_W, G w < 2^31, at most 65535 jobs (a job per grid z).
 * max_rows / max_groups / max_cols: the table's largest n, G and G w (what lies beyond them is not worked on).  The backward entry is two
 * launches: d_H and the partial sums, then the sums of the blocks.
 * Refused before any launch (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs.  n_jobs == 0 or a
 * zero maximum: WDG_OK, nothing is launched.  The table lives in device memory: what is wrong inside a job - heads outside 1..8, w outside
 * 1..256, a negative n or G, G w >= 2^31, NULL H, S or att with n > 0 and G > 0, a leading dimension below its row (ld_h, ld_d_h < G w;
 * ld_s, ld_d_s < 2 G; ld_att, ld_d_att < G w), the backward pointers (d_S, d_H, d_att, partial) given in part, a workspace that is not
 * 16-byte aligned - is refused by wdg_gat_scores_check_jobs on the HOST copy of the table (train.GatScoresBatch calls it before it
 * uploads).  A job with n == 0 or G == 0 is skipped: it touches nothing, d_att included; the kernels leave a job outside the limits untouched.
 */
#define WDG_GAT_SCORES_MAX_HEADS 8
#define WDG_GAT_SCORES_MAX_W 256
#define WDG_GAT_SCORES_ROW_BLOCK 32
typedef struct wdg_gat_scores_job {
    const float *H;      /* [n, G w] */
    float *S;            /* forward out [n, 2 G] */
    const float *att;    /* [2, G w]: a_dst, a_src */
    const float *d_S;    /* backward in [n, 2 G], or NULL (then d_H, d_att and partial are NULL too) */
    float *d_H;          /* backward in / out [n, G w]: added to */
    float *d_att;        /* backward out [2, G w] */
    float *partial;      /* backward workspace [ceil(n / WDG_GAT_SCORES_ROW_BLOCK), 2, G w] */
    int64_t ld_h, ld_s, ld_att, ld_d_s, ld_d_h, ld_d_att;
    int32_t n, G, w, heads;
} wdg_gat_scores_job;
int wdg_gat_scores_forward_batched_f32(const wdg_gat_scores_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_groups, wdg_stream_t stream);
/* replaces: nothing of its own - the backward pass of the scores above (utils/util_funcs.py:365-381) */
int wdg_gat_scores_backward_batched_f32(const wdg_gat_scores_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_cols, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the scores above (utils/util_funcs.py:365-381), on the host's table */
int wdg_gat_scores_check_jobs(const wdg_gat_scores_job *jobs_host, int32_t n_jobs);
/* the floats of a job's workspace: ceil(n / WDG_GAT_SCORES_ROW_BLOCK) * 2 * G * w; 0 for a negative argument */
int64_t wdg_gat_scores_partial_len(int32_t n, int32_t G, int32_t w);

/*
 * Signed attention for many graphs in one launch, and its backward pass (the layer of FAGCN: Bo et al., "Beyond Low-frequency
 * Information in Graph Convolutional Networks"): a weight per stored entry that is learnt and may be NEGATIVE - tanh where
 * wdg_gat_job has the softmax, so an edge can subtract a neighbour -, times the fixed factored scales of the normalised adjacency.
 * The reference ships no model code: the layer is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: the fixed weights of normalize_tensor, utils/util_funcs.py:365-381, in the aggregation, by signed learnt ones, for the
 *           high-pass baseline that stands beside the GCN / SGC tables of gnns_on_syn.py:1-154 (models that live upstream of the reference).
 * A job: the square CSR PATTERN of wdg_gat_job - rowptr int32 [n + 1], col int32 [nnz], columns strictly ascending inside a row; stored
 * values are ignored -, heads in 1..8 of width w >= 1 with heads w <= 256, H [n, heads w], S [n, 2 heads] (S[:, h] the row's own
 * score, S[:, heads + h] its score as a neighbour), row_scale [n] or NULL and col_scale [n] or NULL (NULL = 1: the two vectors of a
 * factored A_hat = diag(r) A diag(c)), an optional residual res [n, heads w] with the scalar eps (NULL = none; eps is then not read).
 * The definition, for row i, head h and the row's stored entries p in ascending order, j = col[p]:
 *   pre_p  = S[i, h] + S[j, heads + h]          t_p = tanhf(pre_p)
 *   coef_p = row_scale[i] * col_scale[j]        ONE fp32 product; a NULL factor is left out, both NULL: 1
 *   a_p    = t_p * coef_p  -> alpha[p, h]       [nnz, heads] contiguous: the SIGNED weight that is applied, kept for the backward pass
 *   chain  = sum_p a_p H[j, h w + k]            ONE fmaf chain from +0 over ascending p: acc = fmaf(a_p, H[j, .], acc)
 *   out[i, h w + k] = fmaf(eps, res[i, h w + k], chain)          (no residual: out = chain)
 * The backward pass, g = d_out[i, :]:
 *   dalpha_p = sum_k g[h w + k] H[j, h w + k]   ONE fmaf chain from +0 over ascending k
 *   u_p      = fmaf(-t_p, t_p, 1.0f)            t_p recomputed from S by the forward's expression: the same bits
 *   dpre_p   = (dalpha_p * coef_p) * u_p  -> d_pre[p, h] (workspace [nnz, heads])          d_S[i, h] = sum_p dpre_p
 * and, over the TRANSPOSED pattern (t_rowptr, t_col; entry q of row j has source row i = t_col[q] and is forward entry p = t_pos[q]):
 *   d_H[j, h w + k] = sum_q alpha[p, h] d_out[i, h w + k]     ONE fmaf chain from +0 over ascending q
 *   d_S[j, heads + h] = sum_q d_pre[p, h]
 * The residual's gradient, eps * d_out, is the caller's: the kernels do not write it.  d_S[i, h] and d_S[j, heads + h] are summed in
 * the order wdg_gat_job states for its sums over a row's entries: lane l of 64 adds the entries l, l + 64, ... in ascending order from
 * +0 (acc = acc + term), then the butterfly over lane distances 32, 16, 8, 4, 2, 1.  There are no floating-point atomics;
 * csrc/signed_att.hip is compiled with contraction off and writes every fmaf out.  tanhf is the device library's: its error in ulps is
 * measured, not assumed (tests/test_gpu_signed_att.py); where it returns +-1 exactly - large |pre| - u_p is exactly 0.
 * An empty row writes out = fmaf(eps, res, +0) - +0 without a residual - and +0 gradients, and no alpha.  A NaN stays a NaN: one in
 * row j of H reaches out[i, :] of exactly the rows i that store j, one in d_out[i, :] reaches d_H[j, :] of exactly the columns j that
 * row i stores.  An element depends on its row, or its transposed row, alone, and a job on the job alone: a job answers in a table
 * what it answers alone, and head h of a job has the bits of a one-head job on that head's column slices (every matrix has its own
 * leading dimension: slices are passed in place).  Outputs must not overlap inputs or each other.  16-byte accesses where a
 * matrix's pointer and leading dimension allow, scalar ones elsewhere: the same values.
 * Guards: an entry whose column lies outside [0, n) - or whose t_pos lies outside [0, nnz) - is skipped, never read through (its
 * alpha and d_pre are written +0); a row whose extent lies outside [0, nnz] is left untouched, and so is a job outside the limits.
 * max_rows: the table's largest n (rows beyond it are not worked on).  wdg_signed_att_backward_batched_f32 is two launches: the row
 * pass, then the pass over the transposed pattern; it reads the alpha of the last forward launch.
 * Refused before any launch (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs (a job per grid
 * z).  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  The table lives in device memory: what is wrong inside a job - heads
 * outside 1..8, w < 1, heads w > 256, an eps that is infinite or a NaN, flags other than 0, a negative n or nnz, a NULL rowptr, H, S or
 * out, a NULL col or alpha with nnz > 0, a leading dimension below the row (ld_res with res given), the backward pointers (d_out, d_H,
 * d_S, t_rowptr; d_pre, t_col, t_pos with nnz > 0) given in part - is refused by wdg_signed_att_check_jobs on the HOST copy of the
 * table (train.SignedAttBatch calls it before it uploads).  A job with n == 0 is skipped.
 */
#define WDG_SIGNED_ATT_MAX_HEADS 8
#define WDG_SIGNED_ATT_MAX_COLS 256
typedef struct wdg_signed_att_job {
    const int32_t *rowptr;    /* [n + 1] */
    const int32_t *col;       /* [nnz], strictly ascending inside a row */
    const int32_t *t_rowptr;  /* [n + 1]: the transposed pattern (backward), or NULL */
    const int32_t *t_col;     /* [nnz] */
    const int32_t *t_pos;     /* [nnz]: the forward entry of every transposed entry (wdg_csr_transpose_positions) */
    const float *H;           /* [n, heads w] */
    const float *S;           /* [n, 2 heads] */
    float *out;               /* forward out [n, heads w] */
    float *alpha;             /* [nnz, heads]: forward out, backward in */
    const float *d_out;       /* backward in [n, heads w] */
    float *d_H;               /* backward out [n, heads w] */
    float *d_S;               /* backward out [n, 2 heads] */
    float *d_pre;             /* backward workspace [nnz, heads] */
    const float *row_scale;   /* [n], or NULL = 1 */
    const float *col_scale;   /* [n], or NULL = 1 */
    const float *res;         /* [n, heads w]: the residual, or NULL = none */
    int64_t ld_h, ld_s, ld_out, ld_d_out, ld_d_h, ld_d_s, ld_res;
    int32_t n, heads, w, flags; /* flags: 0 (none is defined) */
    float eps;                /* the residual's factor */
    int32_t nnz;              /* rowptr[n]: the extent of col, alpha and d_pre */
} wdg_signed_att_job;
int wdg_signed_att_forward_batched_f32(const wdg_signed_att_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
/* replaces: nothing of its own - the backward pass of the layer above (utils/util_funcs.py:365-381) */
int wdg_signed_att_backward_batched_f32(const wdg_signed_att_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the layer above (utils/util_funcs.py:365-381), on the host's table */
int wdg_signed_att_check_jobs(const wdg_signed_att_job *jobs_host, int32_t n_jobs);

/*
 * A polynomial graph filter of many graphs in one launch (the propagation of GPR-GNN: Chien et al., "Adaptive Universal Generalized
 * PageRank Graph Neural Network"; with frozen coefficients, APPNP): out = sum_{k = 0..K} gamma_k A_hat^k v at class width, all K hops
 * of a few columns inside ONE workgroup, T_k and T_{k+1} of those columns in LDS.  The reference ships no model code: the filter is
 * DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: the ONE fixed aggregation of normalize_tensor / the SGC and GCN tables (utils/util_funcs.py:365-381, gnns_on_syn.py:1-154)
 *           by K of them with a learnt weight per hop, for the baseline that stands beside those tables.
 * A job: the square CSR pattern rowptr int32 [n + 1], col int32 [nnz], its values val [nnz] or NULL (NULL = 1: a binary adjacency),
 * row_scale [n] or NULL and col_scale [n] or NULL (NULL = 1: the two vectors of a factored A_hat = diag(r) A diag(c)), v and out
 * [n, cols] with unit inner stride and leading dimensions ld_v, ld_out (column slices of wider matrices are passed in place), order K in 0..64, gamma [K + 1, n_seg] in
 * DEVICE memory with leading dimension ld_gamma, seg_cols >= 1 with cols = n_seg * seg_cols: segment s is the columns
 * s seg_cols .. (s + 1) seg_cols - 1 and has the coefficients gamma[:, s].  Optionally - both or neither - u [n, cols] (ld_u) and
 * dots [K + 1, n_seg] (ld_dots), with the workspace partials (wdg_poly_filter_partials_len doubles).  group_cols in {1, 2, 4}.
 * The definition, for column c of segment s, row i with the stored entries p = beg .. end - 1, j = col[p]:
 *   T_0 = v
 *   a row of at most WDG_POLY_FILTER_LONG_ROW entries has L = WDG_POLY_FILTER_TEAM = 4 lanes, a longer one L = 64.  Lane l of the L
 *   adds the entries beg + l, beg + l + L, ... in ascending order in ONE fmaf chain from +0: acc = fmaf(coef_p, T_k[j, c], acc), coef_p = val[p] * col_scale[j] -
 *   ONE fp32 product; a NULL factor is 1.0f and the product then exact -;
 *   then the butterfly acc = acc + (the acc of lane l ^ d) over the lane distances d = L/2, L/4, ..., 1; then
 *   T_{k+1}[i, c] = row_scale[i] * sum (a NULL row_scale: 1.0f - the product is exact).  An empty row gives row_scale[i] * +0.
 *   out[i, c] = gamma[0, s] * v[i, c], then for k = 1..K in ascending order out[i, c] = fmaf(gamma[k, s], T_k[i, c], out[i, c]).
 *   dots[k, s] = sum over the rows and the segment's columns of T_k[i, c] * u[i, c]: every product formed in fp64 (exact); per column
 *   and per block of WDG_POLY_FILTER_DOT_ROWS consecutive rows one fp64 sum from +0 over ascending rows; a column's blocks added in
 *   ascending order from +0; the segment's columns added in ascending order from +0; rounded to fp32 ONCE.
 * So the order of every chain and sum is a function of the row's length and of compile-time constants alone - never of the table, of
 * group_cols or of the columns that share a workgroup.  What follows, and what tests/test_gpu_poly_filter.py checks: a job has the same
 * bits alone and inside any table; a column has the same bits for group_cols 1, 2 and 4 and the bits of a one-segment job on its column
 * slice (dots: a segment's); order 0 gives exactly gamma[0, s] * v; columns outside a view are never written; all-zero input gives a
 * zero - +0 in every bit unless EVERY coefficient of the segment is negative: gamma[0, s] * +0 is then -0 and stays -0.
 * T_k is not exposed; a job whose gamma[:, s] is the unit vector e_k returns exactly T_k in segment s (fmaf(1, T_k, +-0)), which is how
 * the tests compare dots for EQUAL BITS with the numpy restatement (tests/_poly_filter_ref.py).
 * No floating-point atomic anywhere; csrc/poly_filter.hip is compiled with contraction off and writes every fmaf out.
 * Shape: grid (column groups, jobs), 1024 threads.  A group is up to group_cols consecutive columns of ONE segment (seg_cols 5 with
 * group_cols 4: groups of 4 and 1); its workgroup holds T_k and T_{k+1} in 2 * n * group_cols * 4 bytes of LDS for all K hops -
 * gathers come from LDS, indices and scales from global memory on every hop, workgroup barriers between hops, no grid-wide
 * synchronisation.  Every team of 4 lanes (wave, for the long rows) owns the same rows on every hop and accumulates out where it lives.
 * Limit: 2 * n * group_cols * 4 <= WDG_POLY_FILTER_LDS_BYTES (160 KiB less 256 bytes kept free, as csrc/spmm.hip keeps them; the
 * kernel has no other scratch): n <= wdg_poly_filter_max_rows(group_cols) = 20448, 10224, 5112.
 * max_groups: the table's largest count of column groups (n_seg * ceil(seg_cols / group_cols)); max_floats: its largest
 * n * group_cols, which sizes the launch's LDS - the launch geometry cannot be read out of a table in device memory.  A job beyond
 * either is left untouched, and so is one that is malformed.  An entry whose column lies outside [0, n) is skipped, never read
 * through; a row whose extent lies outside [0, nnz] counts as empty.
 * wdg_poly_filter_batched_f32 is one launch, and a second small one (a workgroup per job and k adds the partials) when
 * max_dot_rows != 0: the largest order + 1 of the jobs that have dots (0: none has).  Refused before any launch (WDG_ERR_INVALID): a
 * NULL table with n_jobs > 0, negative counts, more than 65535 jobs, max_floats beyond the limit, max_dot_rows beyond 65.  n_jobs == 0:
 * WDG_OK, nothing is launched; max_groups == 0 or max_floats == 0: the filter's launch is left out (the dots of empty jobs are still written).  What
 * is wrong inside a job - order outside 0..64, seg_cols < 1 or cols no multiple of it, u without dots or dots without u or either
 * without partials, group_cols not in {1, 2, 4}, a negative n, nnz or cols, a NULL rowptr, v, out or gamma, a NULL col with nnz > 0,
 * a leading dimension below its row - is refused by wdg_poly_filter_check_jobs on the HOST copy of the table (train.PolyFilterBatch
 * calls it before it uploads), and so is n over the limit of its group_cols, as WDG_ERR_UNSUPPORTED with the limit in the message.  A job with
 * n == 0 or cols == 0 is skipped (its dots are written +0).
 */
#define WDG_POLY_FILTER_MAX_ORDER 64
#define WDG_POLY_FILTER_TEAM 4
#define WDG_POLY_FILTER_LONG_ROW 128
#define WDG_POLY_FILTER_DOT_ROWS 32
#define WDG_POLY_FILTER_LDS_BYTES (160 * 1024 - 256)
typedef struct wdg_poly_filter_job {
    const int32_t *rowptr;    /* [n + 1] */
    const int32_t *col;       /* [nnz] */
    const float *val;         /* [nnz], or NULL = 1 */
    const float *row_scale;   /* [n], or NULL = 1 */
    const float *col_scale;   /* [n], or NULL = 1 */
    const float *v;           /* [n, cols] */
    float *out;               /* [n, cols] */
    const float *gamma;       /* [order + 1, n_seg], device memory */
    const float *u;           /* [n, cols], or NULL: no dots */
    float *dots;              /* [order + 1, n_seg], or NULL */
    double *partials;         /* workspace of wdg_poly_filter_partials_len doubles, with dots */
    int64_t ld_v, ld_out, ld_gamma, ld_u, ld_dots;
    int32_t n, nnz, cols, seg_cols, order, group_cols;
} wdg_poly_filter_job;
int wdg_poly_filter_batched_f32(const wdg_poly_filter_job *jobs_dev, int32_t n_jobs, int32_t max_groups, int32_t max_floats, int32_t max_dot_rows,
                                wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the filter above (utils/util_funcs.py:365-381), on the host's table */
int wdg_poly_filter_check_jobs(const wdg_poly_filter_job *jobs_host, int32_t n_jobs);
/* the largest n of a job with this group_cols (host only); 0 for a group_cols outside {1, 2, 4} */
int32_t wdg_poly_filter_max_rows(int32_t group_cols);
/* the doubles of a job's workspace: (order + 1) * cols * (ceil(n / WDG_POLY_FILTER_DOT_ROWS) + 1); 0 for a negative argument */
int64_t wdg_poly_filter_partials_len(int32_t n, int32_t cols, int32_t order);

/*
 * A graph filter in a basis of ORTHOGONAL polynomials, of many graphs in one launch (the propagation of ChebNet / ChebNetII: He, Wei,
 * Wen, "Convolutional Neural Networks on Graphs with Chebyshev Approximation, Revisited"; of JacobiConv: Wang, Zhang, "How Powerful
 * are Spectral Graph Neural Networks"): out = sum_{k = 0..K} gamma_k T_k with the three-term recurrence every such basis obeys,
 *   T_{k+1} = a_k A_hat T_k + b_k T_k + c_k T_{k-1},
 * all K hops of a few columns inside ONE workgroup.  The reference ships no model code: the filter is DEFINED here and
 * is not claimed to reproduce an upstream table.
 * replaces: the ONE fixed aggregation of normalize_tensor / the SGC and GCN tables (utils/util_funcs.py:365-381, gnns_on_syn.py:1-154)
 *           by K of them combined through a three-term recurrence, for the spectral baselines that stand beside those tables.
 * A job: every member of wdg_poly_filter_job with the same meaning, and recur fp32 [order, 3] in DEVICE memory with leading dimension
 * ld_recur >= 3: row k is (a_k, b_k, c_k), shared by all segments of the job.  recur may be NULL only when order == 0.
 * The definition, for column c of segment s and row i: let P[i, c] be EXACTLY the polynomial filter's hop of T_k stated above - the
 * lane chains (fmaf chains from +0 over the entries beg + l, beg + l + L, ...; coef_p = val[p] * col_scale[j] ONE rounded product),
 * the butterfly over the distances L/2 .. 1, then ONE product with row_scale[i].  Then
 *   T_0 = v
 *   T_1[i, c] = fmaf(a_0, P, b_0 * T_0[i, c])                                      c_0 is not read
 *   T_{k+1}[i, c] = fmaf(a_k, P, fmaf(b_k, T_k[i, c], c_k * T_{k-1}[i, c]))        for k >= 1
 *   out[i, c] = gamma[0, s] * v[i, c], then for k = 1..K in ascending order out[i, c] = fmaf(gamma[k, s], T_k[i, c], out[i, c])
 *   dots[k, s]: the polynomial filter's fp64 order, unchanged, applied to this kernel's T_k.
 * With the table (1, 0, 0) in every row the result compares == with the polynomial filter's on finite inputs (fmaf(1, P, 0 * T) = P up
 * to the sign of a zero).  Everything the polynomial filter's comment says about orders, tables, group_cols, segments and views holds
 * here: a job has the same bits alone and inside any table, a column the same bits for group_cols 1, 2 and 4 and the bits of a
 * one-segment job on its slice, order 0 gives exactly gamma[0, s] * v, columns outside a view are never written; a job whose
 * gamma[:, s] is the unit vector e_k returns exactly T_k.  Because T_k = p_k(A_hat) v, the backward pass is one more job: on the
 * transposed pattern with the two scales swapped and the SAME table, v = d_out and u = H0 give out = d_H0 and dots = d_gamma.
 * No floating-point atomic anywhere; csrc/recur_filter.hip is compiled with contraction off and writes every fmaf out.
 * Shape and limits: the polynomial filter's launch - grid (column groups, jobs), 1024 threads, teams of WDG_POLY_FILTER_TEAM lanes, a
 * wave for rows of more than WDG_POLY_FILTER_LONG_ROW entries, the two images of 2 * n * group_cols * 4 bytes of LDS.  During hop k
 * the image that takes T_{k+1} still holds T_{k-1}; row i of it is read and written by row i's owner alone, which reads T_k[i, :] and
 * T_{k-1}[i, :] with the row's other loads, before its first store: NO LDS beyond the polynomial filter's, so the row limits are
 * wdg_poly_filter_max_rows(group_cols) = 20448, 10224, 5112 and the workspace is wdg_poly_filter_partials_len doubles.
 * max_groups, max_floats, max_dot_rows and the refusals before any launch: as for wdg_poly_filter_batched_f32.  What is wrong inside
 * a job - everything wdg_poly_filter_check_jobs refuses, and a NULL recur or ld_recur < 3 with order > 0 - is refused by
 * wdg_recur_filter_check_jobs on the HOST copy of the table (train.RecurFilterBatch calls it before it uploads); both launches skip
 * such a job.
 */
typedef struct wdg_recur_filter_job {
    const int32_t *rowptr;    /* [n + 1] */
    const int32_t *col;       /* [nnz] */
    const float *val;         /* [nnz], or NULL = 1 */
    const float *row_scale;   /* [n], or NULL = 1 */
    const float *col_scale;   /* [n], or NULL = 1 */
    const float *v;           /* [n, cols] */
    float *out;               /* [n, cols] */
    const float *gamma;       /* [order + 1, n_seg], device memory */
    const float *u;           /* [n, cols], or NULL: no dots */
    float *dots;              /* [order + 1, n_seg], or NULL */
    double *partials;         /* workspace of wdg_poly_filter_partials_len doubles, with dots */
    const float *recur;       /* [order, 3]: row k = (a_k, b_k, c_k), device memory; NULL only with order == 0 */
    int64_t ld_v, ld_out, ld_gamma, ld_u, ld_dots, ld_recur;
    int32_t n, nnz, cols, seg_cols, order, group_cols;
} wdg_recur_filter_job;
int wdg_recur_filter_batched_f32(const wdg_recur_filter_job *jobs_dev, int32_t n_jobs, int32_t max_groups, int32_t max_floats, int32_t max_dot_rows,
                                 wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the filter above (utils/util_funcs.py:365-381), on the host's table */
int wdg_recur_filter_check_jobs(const wdg_recur_filter_job *jobs_host, int32_t n_jobs);

/*
 * The strict two-hop neighbourhood of many graphs (the second aggregation pattern of H2GCN: Zhu et al., "Beyond Homophily in Graph
 * Neural Networks"), built on the device for a table of jobs in two launches.  The reference computes no pattern product: the
 * result is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of its own - the aggregations of normalize_tensor (utils/util_funcs.py:365-381) run on the pattern they are handed;
 *           this builds a second pattern for them.
 * A job: a square CSR pattern A, rowptr int32 [n + 1] and col int32 [rowptr[n]] - inside a row in ANY order, duplicates allowed, no
 * values read.  With B[i, j] = (A stores (i, j) and i != j) - the diagonal of A is ignored as if it were not stored - the result is
 * the CSR pattern T of
 *   R[i, j] = exists k with B[i, k] and B[k, j]                           (so k != i and k != j: reached in exactly two steps)
 *   flags == 0:                            T[i, j] = R[i, j] and not B[i, j] and j != i        (the strict two-hop neighbourhood)
 *   flags & WDG_TWO_HOP_KEEP_ONE_HOP (1):  A's off-diagonal entries are not removed: T[i, j] = (R[i, j] or B[i, j]) ... - every j within
 *                                          two hops of i
 *   flags & WDG_TWO_HOP_KEEP_SELF (2):     ... the diagonal is not removed: T[i, i] = R[i, i] (i has an out-neighbour that points back)
 * Row i is built from OUT-neighbours of OUT-neighbours: on a directed graph T is in general not symmetric.  out_rowptr [n + 1] starts
 * at 0 for every job; the columns of a row of out_col come out strictly ascending and without duplicates whatever the input's order;
 * no values are written (a CsrGraph with val = NULL: every stored value is 1).  The results are the same bits on every run and do not
 * depend on the other jobs of the table or on max_rows.
 * wdg_csr_two_hop_count_batched: every row's count, out_rowptr (an exclusive scan per job) and *total = out_rowptr[n] as int64 - or
 *   -1 when any stored index of the job lies outside [0, n): such an index is skipped, it never addresses the bitmap (the front end
 *   raises IndexError, as for wdg_coo_to_csr_i32's negative count).  A total above 2^31 - 1 is written as it is; out_rowptr has then wrapped
 *   and the caller must not go on to the fill pass.  Two kernels on the stream.  out_col is not read.
 * wdg_csr_two_hop_fill_batched: out_col[out_rowptr[i] .. out_rowptr[i + 1]) = the set bits of row i in ascending order, nothing past a
 *   row's end; a job whose out_col is NULL is skipped.  The bitmap of a row is REBUILT here: no workspace is kept between the passes.
 * Shape: WDG_TWO_HOP_WAVES waves per workgroup, a wave per row at a time with a bitmap of n bits in its slice of LDS, bits set with LDS
 * atomics; no floating point, no global atomic.  max_rows: the table's largest n - it sizes the launch's LDS
 * (WDG_TWO_HOP_WAVES * 4 * ceil(max_rows / 32) bytes) and grid; a job with n > max_rows is left untouched, and so is a malformed one.
 * Limit: WDG_TWO_HOP_WAVES bitmaps in WDG_TWO_HOP_LDS_BYTES (160 KiB less 256 bytes kept free): n <= wdg_csr_two_hop_max_rows() =
 * WDG_TWO_HOP_MAX_ROWS = 163 584.
 * Refused before any launch, by both launches (WDG_ERR_INVALID): a NULL table with n_jobs > 0, a negative n_jobs or max_rows, more than
 * 65535 jobs; max_rows over the limit: WDG_ERR_UNSUPPORTED with the limit in the message.  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is
 * launched (so a table of nothing but n == 0 jobs has nothing written: the caller zeroes out_rowptr[0] and total; in a table that
 * launches, an n == 0 job gets out_rowptr[0] = 0 and total = 0).  What is wrong inside a job - a negative n, a flag bit other than 1 and
 * 2, a NULL out_rowptr or total, a NULL rowptr with n > 0 - is refused by wdg_csr_two_hop_check_jobs on the HOST copy of the table
 * (graphs.TwoHopBatch calls it before it uploads), and so is n over the limit, as WDG_ERR_UNSUPPORTED with the limit in the message.  A NULL
 * col is a pattern without entries.  rowptr is trusted: the job carries no entry count to hold it against.
 */
#define WDG_TWO_HOP_KEEP_ONE_HOP 1
#define WDG_TWO_HOP_KEEP_SELF 2
#define WDG_TWO_HOP_WAVES 8
#define WDG_TWO_HOP_LDS_BYTES (160 * 1024 - 256)
#define WDG_TWO_HOP_MAX_ROWS (WDG_TWO_HOP_LDS_BYTES / (4 * WDG_TWO_HOP_WAVES) * 32)
typedef struct wdg_two_hop_job {
    const int32_t *rowptr;    /* A: n x n, [n + 1] */
    const int32_t *col;       /* [rowptr[n]]: any order inside a row, duplicates allowed; NULL: no entries */
    int32_t n, flags;
    int32_t *out_rowptr;      /* [n + 1], written by the count pass */
    int32_t *out_col;         /* [out_rowptr[n]], written by the fill pass; may be NULL for the count pass */
    int64_t *total;           /* entries of T, or -1 for an index out of range */
} wdg_two_hop_job;
int32_t wdg_csr_two_hop_max_rows(void);
int wdg_csr_two_hop_check_jobs(const wdg_two_hop_job *jobs_host, int32_t n_jobs);
int wdg_csr_two_hop_count_batched(const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
int wdg_csr_two_hop_fill_batched(const wdg_two_hop_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);

/*
 * The k best columns of every row of many dense fp32 matrices in ONE launch: the selection a k-nearest-neighbour FEATURE graph needs
 * (AM-GCN, SimP-GCN, the "kNN-GCN" rows of comparison tables) once the similarity matrix X X^T exists.  The reference builds no such
 * graph: the result is DEFINED here and is not claimed to reproduce an upstream table.
 * stands next to: the dense cosine matrix of generalized_edge_homophily, utils/homophily_metrics.py:167 - its rows are what this ranks
 *                 (and utils/homophily_metrics.py:168, sim[isnan] = 0, is what a column scale of 0 for an all-zero row restates).
 * A job: scores fp32 [rows, cols] with leading dimension ld >= cols, col_scale fp32 [cols] or NULL, row0, k in 1 .. WDG_TOPK_MAX_K, flags.
 *   key(r, j) = scores[r, j] * col_scale[j]          ONE fp32 product, rounded once; col_scale NULL: the score itself
 *   eligible(r, j): key is not a NaN, and - with WDG_TOPK_EXCLUDE_SELF (1) - j != row0 + r   (row r's own node is column row0 + r,
 *                   compared in 64 bits; where it lies outside 0 .. cols - 1 nothing is excluded)
 *   j ranks before j'  iff  key_j > key_j'  or  (key_j == key_j' and j < j')         -0 == +0; +-inf are ordinary values
 *   out_len[r] = min(k, number of eligible j)
 *   out_col[r, 0 .. len - 1]: the first len columns of the ranking in rank order - with WDG_TOPK_SORT_COLUMNS (2) the same set in
 *                   ascending column order
 *   out_key[r, s] (where out_key is not NULL): the key of out_col[r, s] as computed above (a -0 product stays -0)
 *   slots len .. k - 1: out_col = -1, out_key = +0.  Nothing beyond slot k - 1 of a row is written (ld_out may exceed k).
 * The ranking is a total order: the output is a pure function of the job's input - the same bits on every launch, alone or in any
 * table, and a panel of rows of a matrix (row0 = the panel's first row) gives the rows the whole matrix gives.  No atomic of any kind.
 * Shape: a wave owns a row at a time; lane l holds the rank-l candidate as a 64-bit word (the monotone uint32 image of the key above
 * the complemented column); the row is streamed in chunks of 64 columns, a chunk is merged (bitonic sort + bitonic merge over
 * cross-lane moves) only when one of its words beats the current k-th.  No LDS, no scratch.  Grid: (blocks of rows, jobs); max_rows -
 * the table's largest `rows` - sizes the grid only: rows are strided over, so a job with more rows than max_rows is still completed.
 * Refused before any launch (WDG_ERR_INVALID, with a message): a NULL table with n_jobs > 0, a negative n_jobs or max_rows, more than
 * 65535 jobs.  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  What is wrong inside a job is refused by
 * wdg_topk_rows_check_jobs on the HOST copy of the table (graphs.TopkRowsBatch calls it before it uploads): k outside
 * 1 .. WDG_TOPK_MAX_K, negative rows or cols, ld < cols, ld_out < k, NULL scores with rows * cols > 0, NULL out_col or out_len, a flag
 * bit other than 1 and 2; the kernel skips such a job.  rows == 0: nothing to write; cols == 0: every row has length 0.
 *
 * wdg_row_rnorm_f32: out[i] = 1 / ||x_i|| for x fp32 [n, F] with leading dimension ld >= F, and 0 where the row is all zero (a row
 * whose squares overflow gives 1 / inf = 0 as well).  Its arithmetic, a wave per row: lane l's partial s_l = fmaf(v, v, s_l) over
 * v = x[i, f], f = l, l + 64, ... ascending, from s_l = +0; the 64 partials are added by the butterfly s = s + shuffle_xor(s, o),
 * o = 32, 16, 8, 4, 2, 1 (every lane ends with the same sum); out[i] = s == 0 ? 0 : 1.0f / sqrtf(s), the square root and the
 * division each correctly rounded.  Every term is >= 0, so s carries at most ceil(F / 64) + 6 roundings: the relative error of out[i]
 * is at most ((ceil(F / 64) + 6) / 2 + 2) 2^-24 to first order.  Refused: a negative n or F, ld < F, NULL x with n F > 0, NULL out
 * with n > 0.  n == 0: nothing is launched.  F == 0: zeros.
 */
#define WDG_TOPK_EXCLUDE_SELF 1
#define WDG_TOPK_SORT_COLUMNS 2
#define WDG_TOPK_MAX_K 64
typedef struct wdg_topk_job {
    const float *scores;      /* [rows, cols], leading dimension ld */
    const float *col_scale;   /* [cols] or NULL */
    int32_t *out_col;         /* [rows, k], leading dimension ld_out */
    float *out_key;           /* as out_col, or NULL */
    int32_t *out_len;         /* [rows] */
    int64_t ld, ld_out;
    int32_t rows, cols;
    int32_t row0, k;
    int32_t flags, reserved;  /* reserved: not read */
} wdg_topk_job;
int wdg_topk_rows_check_jobs(const wdg_topk_job *jobs_host, int32_t n_jobs);
int wdg_topk_rows_batched_f32(const wdg_topk_job *jobs_dev, int32_t n_jobs, int32_t max_rows, wdg_stream_t stream);
int wdg_row_rnorm_f32(const float *x, int64_t ld, int32_t n, int32_t F, float *out, wdg_stream_t stream);

/*
 * One GCNII layer behind its aggregation, for many layers / graphs in ONE launch, and its backward pass (Chen, Wei, Huang, Ding, Li:
 * "Simple and Deep Graph Convolutional Networks", ICML 2020): the initial residual, the identity mapping, the ReLU and the dropout of
 *   H_l = relu_dropout((1 - beta) S + beta S W),   S = (1 - alpha) P + alpha H0,   P = A_hat H_{l-1} (the caller's aggregation)
 * as one pass over the rows instead of a combine, a product, a combine and an activation.  The reference ships no model code: the layer is
 * DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of the reference - it stands behind the aggregation with the fixed weights of normalize_tensor,
 *           utils/util_funcs.py:365-381, whose result is this layer's P.
 * A job: n rows, w columns (1 <= w <= WDG_GCNII_MAX_W); P [n, w], H0 [n, w], W [w, w] (row k, column c), alpha, beta, a generator
 * stream; outputs out [n, w] and S [n, w] - S may be NULL (inference: nothing reads it again).  For the backward pass d_out [n, w],
 * d_P [n, w], d_H0 [n, w], d_W [w, w] and a workspace `partial` of wdg_gcnii_partial_len(n, w) floats at a 16-byte boundary; the
 * backward pass reads S, W and - with act == 1 - out.  Every matrix has its own leading dimension and unit inner stride.
 * The arithmetic (csrc/gcnii.hip is compiled with contraction off and writes every fmaf out; tests/_gcnii_ref.py restates it), with
 * a1 = 1.0f - alpha and b1 = 1.0f - beta:
 *   forward    S[i, k] = fmaf(alpha, H0[i, k], a1 * P[i, k])
 *              T[i, c] = ONE fmaf chain from +0 over ascending k:  acc = fmaf(S[i, k], W[k, c], acc)
 *              Z[i, c] = fmaf(beta, T[i, c], b1 * S[i, c])
 *              out[i, c] = Z[i, c] when the launch's act is 0; when act is 1, what wdg_relu_dropout_batched_f32 makes of Z[i, c]:
 *                g = i * ceil(w / 4) + (c >> 2), the four words of Philox4x32-10 with counter {g, *step_dev, 0, 0} and key
 *                {seed, jobs[j].stream}, kept = word[c & 3] >= drop_threshold, out = Z * scale (ONE multiply) if kept and Z > 0; Z itself
 *                if Z is a NaN; +0.0f otherwise.  drop_threshold, scale, seed and step_dev are launch arguments as there; (0, 1.0f) is a
 *                plain ReLU (no word is drawn: every word is >= 0).
 *   backward   dZ[i, c] = act ? (out[i, c] > 0 ? d_out[i, c] * scale : +0.0f) : d_out[i, c]
 *              U[i, k] = ONE fmaf chain from +0 over ascending c:  acc = fmaf(dZ[i, c], W[k, c], acc)
 *              dS[i, k] = fmaf(beta, U[i, k], b1 * dZ[i, k])
 *              d_P[i, k] = a1 * dS[i, k]
 *              d_H0[i, k] = fmaf(alpha, dS[i, k], d_H0[i, k])   - d_H0 is ADDED to: the layers of a model accumulate into one tensor,
 *                in the order they are launched -
 *              the rows are cut into blocks of WDG_GCNII_ROW_BLOCK from row 0; per block b and element (k, c),
 *              partial[b, k, c] = ONE chain from +0 over the block's rows ascending:  acc = fmaf(S[i, k], dZ[i, c], acc)
 *   weight     d_W[k, c] = beta * (the blocks' sums added in ascending b from +0: acc = acc + partial[b, k, c])   (ONE multiply)
 *              - an entry of its own, so that a model calls it ONCE after the backward launches of all its layers, with L jobs.
 * No floating-point atomics; an element depends on its own row of its own job (S, out, d_P, d_H0) or its own (k, c) of its own job (d_W):
 * a job has the same bits alone and in any table, and a second launch repeats the first (given d_H0 as it was).  A NaN in P[i, k]
 * reaches row i of S and out, and row k of d_W, nothing else.  16-byte accesses where every pointer, leading dimension and w of a job
 * allow - one decision per job and pass -, scalar ones elsewhere: the same values.  Outputs must not overlap inputs or each other.
 * Limits: w in 1..WDG_GCNII_MAX_W, at most 65535 jobs (a job per grid z).  max_rows / max_w: the table's largest n and w (what lies
 * beyond them is not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): a NULL table with n_jobs > 0, negative counts, more than 65535 jobs, max_w above
 * WDG_GCNII_MAX_W, an act other than 0 and 1, a NULL step_dev with act == 1, a scale that is not a number, max_rows * ceil(max_w / 4)
 * >= 2^32 (g is a 32-bit counter word).  n_jobs == 0 or a zero maximum: WDG_OK, nothing is launched.  The table lives in device memory:
 * what is wrong inside a job - w outside 1..128, a negative n, NULL P, H0, W or out with n > 0, a leading dimension below its row, the
 * backward pointers (d_out, d_P, d_H0, d_W, partial) given in part or without S, a workspace that is not 16-byte aligned - is refused by
 * wdg_gcnii_check_jobs on the HOST copy of the table (train.GcniiBatch calls it before it uploads).  A job with n == 0 is skipped: it
 * touches nothing, d_W included; the kernels leave a job outside the limits untouched.
 */
#define WDG_GCNII_MAX_W 128
#define WDG_GCNII_ROW_BLOCK 32
typedef struct wdg_gcnii_job {
    const float *P;      /* [n, w]: A_hat H_{l-1} */
    const float *H0;     /* [n, w] */
    const float *W;      /* [w, w]: row k, column c */
    float *out;          /* forward out [n, w]; read by the backward pass when act == 1 */
    float *S;            /* forward out [n, w], or NULL (inference); read by the backward pass */
    const float *d_out;  /* backward in [n, w], or NULL (then d_P, d_H0, d_W and partial are NULL too) */
    float *d_P;          /* backward out [n, w] */
    float *d_H0;         /* backward in / out [n, w]: added to */
    float *d_W;          /* weight-gradient out [w, w] */
    float *partial;      /* backward workspace [ceil(n / WDG_GCNII_ROW_BLOCK), w, w] */
    int64_t ld_p, ld_h0, ld_w, ld_out, ld_s, ld_d_out, ld_d_p, ld_d_h0, ld_d_w;
    int32_t n, w;
    float alpha, beta;
    uint32_t stream;     /* generator stream of this job */
    uint32_t reserved;   /* not read */
} wdg_gcnii_job;
int wdg_gcnii_forward_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, int32_t act,
                                  uint32_t drop_threshold, float scale, uint32_t seed, const uint32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the backward pass of the layer above (behind the aggregation of utils/util_funcs.py:365-381):
 *           dZ, d_P, d_H0 += and the blocks' partial sums, one launch */
int wdg_gcnii_backward_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, int32_t act, float scale,
                                   wdg_stream_t stream);
/* replaces: nothing of its own - d_W of the layer above (behind the aggregation of utils/util_funcs.py:365-381) from the partial sums
 *           the backward launches left, one launch for all the layers of a model */
int wdg_gcnii_weight_grad_batched_f32(const wdg_gcnii_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_w, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the layer above (utils/util_funcs.py:365-381), on the host's table */
int wdg_gcnii_check_jobs(const wdg_gcnii_job *jobs_host, int32_t n_jobs);
/* the floats of a job's workspace: ceil(n / WDG_GCNII_ROW_BLOCK) * w * w; 0 for a negative argument */
int64_t wdg_gcnii_partial_len(int32_t n, int32_t w);

/*
 * DropEdge (Rong, Huang, Xu, Huang: "DropEdge: Towards Deep Graph Convolutional Networks on Node Classification", ICLR 2020): a fresh
 * random subset of a pattern's stored entries per training step, renormalised, for a table of patterns in ONE launch.  The pass writes
 * the thinned PATTERN, not a mask: the aggregations behind it (wdg_spmm_thinned_batched_f32) do not depend on the step and draw nothing.
 * A graph appears in the table twice - its forward pattern and its transposed pattern (WDG_DROP_EDGE_TRANSPOSED) - and both keep the same
 * edges, because an entry's fate is a function of its FORWARD coordinates, not of its position in an array: no position map is read.
 * The reference ships no model code: the pass is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of the reference - it restates the degree part of its normalisation on the KEPT entries: normalize,
 *           utils/util_funcs.py:29-36 (WDG_NORM_RW), and normalize_tensor, utils/util_funcs.py:365-380 (the symmetric form) - for the
 *           models that stand beside the tables of gnns_on_syn.py:9-53.
 * A job: a CSR pattern of n rows and n_cols columns - rowptr int32 [n + 1], col int32 [nnz], rows in any order, duplicates allowed -
 * and the outputs kept_col int32 [nnz], kept_len int32 [n], scale fp32 [n] or NULL.  The definition (tests/_drop_edge_ref.py restates it
 * in numpy), Philox4x32-10 being the generator of wdg_relu_dropout_batched_f32 with counter {c0, c1, 0, 0} and key {k0, k1}:
 *   step key     (k0, k1) = output words 0 and 1 of Philox4x32-10 with counter {*step_dev, jobs[j].stream, 0, 0} and key
 *                {seed, 0x45444745} - once per launch and job
 *   coordinates  of the stored column j of row i: the FORWARD coordinates are (i, j), or (j, i) with WDG_DROP_EDGE_TRANSPOSED; the pair
 *                (a, b) is the forward coordinates, or (min, max) of them with WDG_DROP_EDGE_TIED: both directions of an undirected
 *                edge then share one fate (DropEdge as the paper draws it for symmetric graphs; untied is for directed graphs)
 *   kept         when 0 <= j < n_cols and either WDG_DROP_EDGE_KEEP_DIAGONAL is set and i == j (the self loop of A + I is never
 *                dropped) or word 0 of Philox4x32-10 with counter {a, b, 0, 0} and key {k0, k1} is >= drop_threshold.
 *                A column stored twice is kept or dropped together; a column outside [0, n_cols) is never kept.
 *   per row i    the kept columns, in stored order, go to kept_col[rowptr[i] .. rowptr[i] + kept_len[i] - 1]; the rest of the row's extent
 *                is filled with -1; kept_len[i] = their count c; where scale != NULL, scale[i] = the F32 path of wdg_degree_norm on c:
 *                1.0f / (float)c (WDG_NORM_RW) or, with WDG_DROP_EDGE_NORM_SYM, 1.0f / sqrtf((float)c) (WDG_NORM_SYM); inf -> 0.
 *                At drop_threshold 0 on a unit-valued pattern this is wdg_degree_norm's dinv_f32, bit for bit.
 *                A row whose extent lies outside [0, nnz] is left untouched (kept_col, kept_len and scale).
 * The host passes drop_threshold = (uint32_t) floor(p * 2^32), computed in fp64, for a drop probability 0 <= p < 1, as for
 * wdg_relu_dropout_batched_f32; p = 0 keeps every entry with a column inside the pattern.  *step_dev is read from DEVICE memory by the
 * kernel: a captured hipGraph that holds this launch and an increment of the word draws a fresh subset on every replay.
 * Integer arithmetic plus one scale per row; no LDS, no atomics; a job has the same bytes alone and in any table.  A wave per row, 64
 * entries per step: there is NO multi-wave path for a hub row (squirrel's longest row is 30 steps of one wave).
 * max_rows: the table's largest n (rows beyond it are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): negative counts, more than 65535 jobs (a job per grid y), a NULL table with
 * n_jobs > 0, a NULL step_dev.  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  The table lives in device memory: what is
 * wrong inside a job - a negative n, n_cols or nnz, unknown flag bits, a reserved word that is not 0, a NULL rowptr or kept_len with
 * n > 0, a NULL col or kept_col with nnz > 0, a kept_col that overlaps col (the pass does not run in place) - is refused by
 * wdg_drop_edge_check_jobs on the HOST copy of the table (drop_edge.DropEdgeBatch calls it before it uploads), and the launch leaves such
 * a job untouched.  A job with n == 0 is skipped.
 */
#define WDG_DROP_EDGE_TIED 1          /* (a, b) = (min, max) of the forward coordinates */
#define WDG_DROP_EDGE_TRANSPOSED 2    /* the job's pattern is the transposed one: the forward coordinates of (i, j) are (j, i) */
#define WDG_DROP_EDGE_KEEP_DIAGONAL 4 /* an entry with i == j is never dropped */
#define WDG_DROP_EDGE_NORM_SYM 8      /* the norm mode: scale = c^-1/2 (WDG_NORM_SYM); not set: 1 / c (WDG_NORM_RW) */
typedef struct wdg_drop_edge_job {
    const int32_t *rowptr;  /* [n + 1] */
    const int32_t *col;     /* [nnz] */
    int32_t *kept_col;      /* out [nnz]: per row the kept columns in stored order, then -1 */
    int32_t *kept_len;      /* out [n] */
    float *scale;           /* out [n], or NULL */
    int32_t n, n_cols, nnz;
    uint32_t stream;        /* generator stream of this job: the forward and the transposed job of a graph carry the same */
    int32_t flags;          /* WDG_DROP_EDGE_* */
    int32_t reserved;       /* must be 0 */
} wdg_drop_edge_job;
int wdg_drop_edge_thin_batched(const wdg_drop_edge_job *jobs_dev, int32_t n_jobs, int32_t max_rows, uint32_t drop_threshold, uint32_t seed,
                               const uint32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the thinning pass above (utils/util_funcs.py:29-36, 365-380), on the host's table */
int wdg_drop_edge_check_jobs(const wdg_drop_edge_job *jobs_host, int32_t n_jobs);

/*
 * Y = diag(row_scale) A_k diag(col_scale) X over a THINNED pattern A_k as wdg_drop_edge_thin_batched leaves it, a table of products per
 * launch.  The backward pass is the same entry on the transposed job's thinned pattern with the two scales swapped:
 * (R A_k C)^T = C A_k^T R.
 * replaces: nothing of the reference - the product with the normalised adjacency of normalize, utils/util_funcs.py:29-36, and
 *           normalize_tensor, utils/util_funcs.py:365-380, kept factored and restricted to the entries a step keeps, under the models
 *           that stand beside the tables of gnns_on_syn.py:9-53.
 * A job: rowptr int32 [n_rows + 1] - the FULL pattern's, whose extents hold the thinned rows -, kept_col int32 [nnz], kept_len int32
 * [n_rows], row_scale fp32 [n_rows] or NULL, col_scale fp32 [n_cols] or NULL, X [n_cols, n_feat] fp32 with leading dimension ldx,
 * Y [n_rows, n_feat] fp32 with leading dimension ldy.  The definition (tests/_drop_edge_ref.py restates it in numpy, bit for bit):
 *   Y[i, f] = row_scale[i] * acc (ONE multiply; a NULL row_scale: no multiply), with acc = +0 and then, for
 *   q = rowptr[i] .. rowptr[i] + min(kept_len[i], rowptr[i + 1] - rowptr[i]) - 1 in that order:
 *     j = kept_col[q]; an entry with j outside [0, n_cols) - which includes -1 - is SKIPPED (no fmaf), never read through;
 *     acc = fmaf(col_scale ? col_scale[j] : 1.0f, X[j, f], acc)
 *   - one correctly rounded fmaf per kept entry, ONE chain per output element in the stated order whatever the row's length: no row is
 *   split over lanes or waves, no partial sums are added, there is no atomic (csrc/drop_edge.hip is compiled with contraction off and
 *   writes the fmaf out).  A row with no kept entry stores row_scale[i] * +0.  A row whose extent lies outside [0, nnz] is left
 *   untouched.  Every other element of Y[0 : n_rows][0 : n_feat] is written and nothing outside that block.  A job has the same bits
 *   alone and in any table, and a column has the same bits whatever the width of the job it is in.
 *   Leading dimensions >= n_feat of any value: 16-byte loads / stores where the pointer, the leading dimension and n_feat (a multiple of
 *   4) allow - the wave's decision, one for X and one for Y -, element-wise ones elsewhere (same values, same fmaf).  X and Y must not
 *   overlap.
 * A wave per row and per panel of 256 columns (a panel per grid y): n_feat up to 256 * 65535.  max_rows, max_feat: the table's largest
 * n_rows and n_feat (rows / columns beyond them are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): negative counts, more than 65535 jobs (a job per grid z), a NULL table with
 * n_jobs > 0, max_feat above 256 * 65535.  n_jobs == 0, max_rows == 0 or max_feat == 0: WDG_OK, nothing is launched.  What is wrong inside
 * a job - a negative n_rows, n_cols, n_feat or nnz, a reserved word that is not 0, a leading dimension below n_feat, a NULL rowptr,
 * kept_len or Y, a NULL kept_col or X with nnz > 0 and n_cols > 0, X == Y - is refused by wdg_spmm_thinned_check_jobs on the HOST copy of
 * the table (drop_edge.ThinnedSpmmBatch calls it before it uploads), and the launch leaves such a job untouched.  A job with
 * n_rows == 0 or n_feat == 0 is skipped.
 */
typedef struct wdg_thinned_spmm_job {
    const int32_t *rowptr;    /* [n_rows + 1]: the full pattern's */
    const int32_t *kept_col;  /* [nnz]: wdg_drop_edge_job.kept_col */
    const int32_t *kept_len;  /* [n_rows] */
    const float *row_scale;   /* [n_rows] or NULL */
    const float *col_scale;   /* [n_cols] or NULL */
    const float *X;           /* [n_cols, n_feat], leading dimension ldx */
    float *Y;                 /* [n_rows, n_feat], leading dimension ldy */
    int64_t ldx, ldy;
    int32_t n_rows, n_cols, n_feat, nnz;
    int32_t reserved;         /* must be 0 */
} wdg_thinned_spmm_job;
int wdg_spmm_thinned_batched_f32(const wdg_thinned_spmm_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the thinned aggregation above (utils/util_funcs.py:29-36, 365-380), on the
 *           host's table */
int wdg_spmm_thinned_check_jobs(const wdg_thinned_spmm_job *jobs_host, int32_t n_jobs);

/*
 * GraphSAGE's neighbour sampling (Hamilton, Ying, Leskovec: "Inductive Representation Learning on Large Graphs", NeurIPS 2017): per
 * training step EXACTLY `fanout` of every row's eligible entries, uniformly and without replacement, for a table of patterns.  Like
 * wdg_drop_edge_thin_batched the pass writes a thinned PATTERN (kept_col, kept_len, scale) that wdg_spmm_thinned_batched_f32 aggregates
 * over, and a graph appears in the table twice - its forward pattern and its transposed pattern (WDG_NEIGHBOR_SAMPLE_TRANSPOSED) -, both
 * keeping the same edges.  "s of this row's entries" is an order statistic of the row, not a function of the entry: what makes it
 * recomputable from the transposed side without a position map is ONE 64-bit word per forward row, the threshold tau.
 * The reference ships no model code: the pass is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of the reference - its loaders only carry the switch (sage_data, utils/util_funcs.py:207, 342); the pass restates the
 *           degree part of its normalisation on the KEPT entries: normalize, utils/util_funcs.py:29-36 (WDG_NORM_RW), and
 *           normalize_tensor, utils/util_funcs.py:365-380 (the symmetric form) - for the models that stand beside the tables of
 *           gnns_on_syn.py:9-53.
 * A job: a CSR pattern of n rows and n_cols columns - rowptr int32 [n + 1], col int32 [nnz], rows in any order, duplicates allowed -, the
 * outputs kept_col int32 [nnz], kept_len int32 [n], scale fp32 [n] or NULL, and tau uint64: on a forward job an OUTPUT [n], on a
 * transposed job the forward job's tau, an INPUT [n_cols].  The definition (tests/_neighbor_sample_ref.py restates it in numpy),
 * Philox4x32-10 being the generator of wdg_drop_edge_thin_batched with counter {c0, c1, 0, 0} and key {k0, k1}:
 *   step key     (k0, k1) = output words 0 and 1 of Philox4x32-10 with counter {*step_dev, jobs[j].stream, 0, 0} and key
 *                {seed, 0x53414745} ("SAGE": equal seeds give draws unrelated to DropEdge's) - once per launch and job
 *   key          of the stored column j of row i, with FORWARD coordinates (fi, fj) = (i, j), or (j, i) with
 *                WDG_NEIGHBOR_SAMPLE_TRANSPOSED: key = ((uint64_t) word 0 of Philox4x32-10 with counter {fi, fj, 0, 0} and key
 *                {k0, k1}) << 32 | (uint32_t) fj.  A total order within a forward row; a column stored twice shares one key.
 *   eligible     (forward job) the stored entries of row i with 0 <= j < n_cols, minus the protected diagonal: an entry with i == j
 *                under WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL
 *   tau[i]       (forward job) the fanout-th smallest key over the eligible entries of row i, counted with multiplicity;
 *                2^64 - 1 when there are fewer than fanout
 *   kept         when 0 <= j < n_cols and either the entry is a protected diagonal entry or key <= tau[fi] - tau[i] on a forward
 *                job, tau[j] on a transposed one (read only for a valid j).  A duplicate-free row with e eligible entries keeps
 *                exactly min(fanout, e) of them, a uniformly random subset; copies of the threshold column are kept with it; a tie
 *                between different columns (probability 2^-32 per pair) goes to the lower column.  A protected diagonal entry is kept
 *                and is not counted against the fan-out.
 *   per row i    as wdg_drop_edge_thin_batched: the kept columns, in stored order, go to kept_col[rowptr[i] .. rowptr[i] + kept_len[i] - 1];
 *                the rest of the row's extent is filled with -1; kept_len[i] = their count c; where scale != NULL, scale[i] =
 *                1.0f / (float)c or, with WDG_NEIGHBOR_SAMPLE_NORM_SYM, 1.0f / sqrtf((float)c); inf -> 0.
 *                A row whose extent lies outside [0, nnz] is left untouched (kept_col, kept_len, scale and tau).
 * There is no tied form - a fan-out is a property of the receiving row -: the flag bit of value 1 (WDG_DROP_EDGE_TIED's) is refused.
 * phase 0 works the jobs WITHOUT WDG_NEIGHBOR_SAMPLE_TRANSPOSED: it selects, writes tau and thins in the same pass over the row.
 * phase 1 works the jobs WITH it: it thins by tau alone, and must follow phase 0 of the same step in stream order; a forward-only user
 * skips it.  Each phase leaves the other's jobs untouched.  *step_dev is read from DEVICE memory by the kernel: a captured hipGraph that
 * holds both launches and an increment of the word draws a fresh sample on every replay.
 * The result is a pure function of (pattern, fanout, flags, seed, stream, step): a job has the same bytes alone and in any table,
 * whatever algorithm computes it.  Integer arithmetic plus one scale per row; no LDS, no atomics.  A wave per row, 64 entries per step:
 * there is NO multi-wave path for a hub row.  Phase 0 bounds every forward row at fanout kept entries (plus a protected diagonal and
 * copies of the threshold column); the rows of the transposed pattern are NOT bounded.
 * max_rows: the table's largest n (rows beyond it are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): negative counts, more than 65535 jobs (a job per grid y), a NULL table with
 * n_jobs > 0, a phase other than 0 and 1, a NULL step_dev.  n_jobs == 0 or max_rows == 0: WDG_OK, nothing is launched.  The table lives
 * in device memory: what is wrong inside a job - a negative n, n_cols or nnz, the flag bit of value 1, unknown flag bits, a fanout
 * outside 1 .. 64 on a forward job (a transposed job's is not read), a NULL rowptr or kept_len with n > 0, a NULL tau (a transposed job
 * without entries needs none), a NULL col or kept_col with nnz > 0, a kept_col that overlaps col (the pass does not run in place) - is
 * refused by wdg_neighbor_sample_check_jobs on the HOST copy of the table (neighbor_sample.NeighborSampleBatch calls it before it
 * uploads), and the launch leaves such a job untouched.  A job with n == 0 is skipped.
 */
#define WDG_NEIGHBOR_SAMPLE_TRANSPOSED 2    /* the job's pattern is the transposed one: the forward coordinates of (i, j) are (j, i) */
#define WDG_NEIGHBOR_SAMPLE_KEEP_DIAGONAL 4 /* an entry with i == j is always kept and does not count against the fan-out */
#define WDG_NEIGHBOR_SAMPLE_NORM_SYM 8      /* the norm mode: scale = c^-1/2 (WDG_NORM_SYM); not set: 1 / c (WDG_NORM_RW) */
#define WDG_NEIGHBOR_SAMPLE_MAX_FANOUT 64
typedef struct wdg_neighbor_sample_job {
    const int32_t *rowptr;  /* [n + 1] */
    const int32_t *col;     /* [nnz] */
    int32_t *kept_col;      /* out [nnz]: per row the kept columns in stored order, then -1 */
    int32_t *kept_len;      /* out [n] */
    float *scale;           /* out [n], or NULL */
    uint64_t *tau;          /* forward job: out [n]; transposed job: in [n_cols], the forward job's */
    int32_t n, n_cols, nnz;
    uint32_t stream;        /* generator stream of this job: the forward and the transposed job of a graph carry the same */
    int32_t flags;          /* WDG_NEIGHBOR_SAMPLE_* */
    int32_t fanout;         /* 1 .. 64 on a forward job; not read on a transposed one */
} wdg_neighbor_sample_job;
int wdg_neighbor_sample_batched(const wdg_neighbor_sample_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t phase, uint32_t seed,
                                const uint32_t *step_dev, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the sampling pass above (utils/util_funcs.py:29-36, 365-380), on the host's table */
int wdg_neighbor_sample_check_jobs(const wdg_neighbor_sample_job *jobs_host, int32_t n_jobs);

/*
 * The neighbour MAXIMUM: Y[i, f] = the greatest X[j, f] over the stored neighbours j of row i, and which j it was - the pooling aggregator
 * of GraphSAGE (Hamilton, Ying, Leskovec, NeurIPS 2017) and the building block of PNA-style multi-aggregators -, for a table of patterns
 * in ONE launch.  Every other aggregation of this library is a weighted sum; this one is not a low-pass average at all.
 * The reference ships no model code: the operator is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of the reference - it stands where the product with the normalised adjacency of normalize, utils/util_funcs.py:29-36,
 *           and normalize_tensor, utils/util_funcs.py:365-380, stands in the other models, beside the tables of gnns_on_syn.py:9-53.
 * A job: rowptr int32 [n_rows + 1], col int32 [nnz], kept_len int32 [n_rows] or NULL, X [n_cols, n_feat] fp32 with leading dimension
 * ldx, Y [n_rows, n_feat] fp32 with leading dimension ldy, arg int32 [n_rows, n_feat] with leading dimension lda, or NULL (evaluation:
 * not written).  kept_len == NULL: every row's whole extent (a plain CSR pattern); otherwise col is a thinned pattern's kept_col and
 * the row's length is min(kept_len[i], rowptr[i + 1] - rowptr[i]), as in wdg_spmm_thinned_batched_f32.  The definition
 * (tests/_neighbor_max_ref.py restates it in numpy), for row i and column f:
 *   eligible     the row's first `len` stored entries q whose j = col[q] lies in [0, n_cols); the others - -1 included - are SKIPPED,
 *                never read through
 *   the order    a NaN above everything; otherwise the larger X[j, f], with -0 == +0; among equals (two NaNs are equals) the LOWER j -
 *                the tie convention of wdg_topk_rows_batched_f32.  With WDG_NEIGHBOR_MAX_MIN "larger" reads "smaller"; a NaN still
 *                wins and a tie still goes to the lower j.  A TOTAL order on the pairs (X[j, f], j): copies of one j are one pair.
 *   Y[i, f]      the winner's X[j, f] - its BITS, copied: no arithmetic touches a value (a NaN keeps its payload, a zero its sign)
 *   arg[i, f]    the winner's j
 *   A row with no eligible entry stores +0 and -1.  A row whose extent lies outside [0, nnz] is left untouched (Y and arg).  Every
 *   other element of Y / arg [0 : n_rows][0 : n_feat] is written and nothing outside that block.
 * The winner is a function of the SET of eligible entries, so the result has the same bits for any stored order of a row, with
 * duplicates, alone or in any table, and for a column at any job width - whatever walks the row: a wave per row and per panel of 256
 * columns (four per lane), and the lanes that hold no columns take SHARES of the row's entries - at n_feat <= 16 four lanes cover the
 * columns and sixteen entries are in flight per step -; the shares are merged across lanes at the end under the same order, carrying
 * (value, j).  That is bit-safe because the maximum of a total order is associative and commutative; no sum of this library is.
 * There is no multi-wave path for a hub row.  No LDS, no atomics.  16-byte loads / stores where the pointer, the leading dimension and
 * n_feat (a multiple of 4) allow - the wave's decision, one each for X, Y and arg.  X must not overlap Y or arg.
 * max_rows, max_feat: the table's largest n_rows and n_feat (rows / columns beyond them are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): negative counts, more than 65535 jobs (a job per grid z), a NULL table with
 * n_jobs > 0, max_feat above 256 * 65535.  n_jobs == 0, max_rows == 0 or max_feat == 0: WDG_OK, nothing is launched.  What is wrong inside
 * a job - a negative n_rows, n_cols, n_feat or nnz, unknown flag bits, a reserved word that is not 0, a leading dimension below n_feat (lda:
 * where arg is given), a NULL
 * rowptr or Y, a NULL col or X with nnz > 0 and n_cols > 0, X == Y - is refused by wdg_neighbor_max_check_jobs on the HOST copy of the
 * table (neighbor_max.NeighborMaxBatch calls it before it uploads), and the launch leaves such a job untouched.  A job with
 * n_rows == 0 or n_feat == 0 is skipped.
 */
#define WDG_NEIGHBOR_MAX_MIN 1 /* the neighbour MINIMUM: "larger" reads "smaller"; NaN and ties as before */
typedef struct wdg_neighbor_max_job {
    const int32_t *rowptr;    /* [n_rows + 1] */
    const int32_t *col;       /* [nnz]: a CSR pattern's col, or a thinned pattern's kept_col */
    const int32_t *kept_len;  /* [n_rows], or NULL: every row's whole extent */
    const float *X;           /* [n_cols, n_feat], leading dimension ldx */
    float *Y;                 /* out [n_rows, n_feat], leading dimension ldy */
    int32_t *arg;             /* out [n_rows, n_feat], leading dimension lda, or NULL */
    int64_t ldx, ldy, lda;
    int32_t n_rows, n_cols, n_feat, nnz;
    int32_t flags;            /* WDG_NEIGHBOR_MAX_* */
    int32_t reserved;         /* must be 0 */
} wdg_neighbor_max_job;
int wdg_neighbor_max_batched_f32(const wdg_neighbor_max_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the neighbour maximum above (utils/util_funcs.py:29-36, 365-380), on the
 *           host's table */
int wdg_neighbor_max_check_jobs(const wdg_neighbor_max_job *jobs_host, int32_t n_jobs);

/*
 * The backward pass of the neighbour maximum: d_X[j, f] = the sum of d_Y[i, f] over the rows i whose winner in column f was j.  A job on
 * the TRANSPOSED pattern, plain or thinned, which holds the same edges: a gather with one add chain per element, not a scatter.
 * replaces: nothing of the reference - the transposed product that stands behind normalize, utils/util_funcs.py:29-36, and
 *           normalize_tensor, utils/util_funcs.py:365-380, in the other models' backward passes (gnns_on_syn.py:9-53 holds their tables).
 * A job: rowptr int32 [n_rows + 1], col int32 [nnz], kept_len int32 [n_rows] or NULL - of the transposed pattern, as above -,
 * G [n_src, n_feat] fp32 with leading dimension ldg (the forward pass's d_Y), arg int32 [n_src, n_feat] with leading dimension lda (the
 * forward pass's), D [n_rows, n_feat] fp32 with leading dimension ldd (d_X).  The definition (tests/_neighbor_max_ref.py restates it in
 * numpy, bit for bit), for transposed row j and column f:
 *   acc = +0; last = none; then for q = rowptr[j] .. rowptr[j] + len - 1 in that order, len as above:
 *     i = col[q]; an entry with i outside [0, n_src) - which includes -1 - is SKIPPED, never read through;
 *     an entry whose i equals `last`, the i of the previous entry that was not out of range, is SKIPPED too (the duplicate rule);
 *     otherwise last = i and, if arg[i, f] == j: acc = acc + G[i, f]   (one rounded fp32 add; no add where arg differs)
 *   D[j, f] = acc
 *   - ONE add chain per output element in stored order whatever the row's length: no chain is split over lanes or waves, no partial
 *   sums are added, there is no atomic (csrc/neighbor_max.hip is compiled with contraction off).  A sum depends on its order: unlike the
 *   forward pass, this chain cannot be shared out - only the LOADS of a row's entries are, over the lanes that hold no columns; every
 *   term then goes to the one lane that adds it, in entry order - and there is NO multi-wave path for a hub row of the transposed
 *   pattern.
 *   The duplicate rule: an edge stored twice is ONE pair of the forward pass's set and routes its gradient once.  CsrGraph.transpose()
 *   MERGES duplicates (it builds through wdg_coo_to_csr_i32 without WDG_COO_KEEP_DUPLICATES: rows sorted by column, copies summed into
 *   one entry), a transpose built with WDG_COO_KEEP_DUPLICATES sorts every row and so leaves copies adjacent, and the thinning passes
 *   (wdg_drop_edge_thin_batched, wdg_neighbor_sample_batched) keep or drop all copies of a column together and compact in stored
 *   order: adjacent copies stay adjacent.  A pattern whose duplicates are NOT adjacent counts them per occurrence.
 *   A row whose extent lies outside [0, nnz] is left untouched.  A job has the same bits alone and in any table, and a column has the
 *   same bits whatever the width of the job it is in.  D must not overlap G or arg.
 * A wave per row and per panel of 256 columns, 16-byte accesses as above (one decision each for G, arg and D).
 * Refused before any HIP call (WDG_ERR_INVALID): as above.  What is wrong inside a job - a negative n_rows, n_src, n_feat or nnz, a
 * reserved word that is not 0, a leading dimension below n_feat, a NULL rowptr or D, a NULL col, G or arg with nnz > 0 and n_src > 0,
 * G == D - is refused by wdg_neighbor_max_backward_check_jobs on the HOST copy of the table (neighbor_max.NeighborMaxBackwardBatch calls
 * it before it uploads), and the launch leaves such a job untouched.  A job with n_rows == 0 or n_feat == 0 is skipped.
 */
typedef struct wdg_neighbor_max_backward_job {
    const int32_t *rowptr;    /* [n_rows + 1]: the TRANSPOSED pattern's */
    const int32_t *col;       /* [nnz] */
    const int32_t *kept_len;  /* [n_rows], or NULL */
    const float *G;           /* [n_src, n_feat], leading dimension ldg: d_Y */
    const int32_t *arg;       /* [n_src, n_feat], leading dimension lda: the forward pass's */
    float *D;                 /* out [n_rows, n_feat], leading dimension ldd: d_X */
    int64_t ldg, lda, ldd;
    int32_t n_rows, n_src, n_feat, nnz;
    int32_t reserved;         /* must be 0 */
    int32_t reserved2;        /* must be 0 */
} wdg_neighbor_max_backward_job;
int wdg_neighbor_max_backward_batched_f32(const wdg_neighbor_max_backward_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                          wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the backward pass above (utils/util_funcs.py:29-36, 365-380), on the host's
 *           table */
int wdg_neighbor_max_backward_check_jobs(const wdg_neighbor_max_backward_job *jobs_host, int32_t n_jobs);

/*
 * The neighbour MOMENTS: per row and column the mean, the standard deviation, the maximum and the minimum of X over the row's stored
 * neighbours, which neighbours the extremes were, and the neighbour count - the four aggregators of PNA (Corso, Cavalleri, Beaini, Lio,
 * Velickovic, NeurIPS 2020) in ONE walk over the row, for a table of patterns in ONE launch.  The standard deviation is the CENTRED
 * one - a second pass over the same values with the mean taken off -, not E[x^2] - E[x]^2, which in fp32 loses everything once a
 * column's mean is large against its spread.
 * The reference ships no model code: the operator is DEFINED here and is not claimed to reproduce an upstream table.
 * replaces: nothing of the reference - it stands where the product with the normalised adjacency of normalize, utils/util_funcs.py:29-36,
 *           and normalize_tensor, utils/util_funcs.py:365-380, stands in the other models, beside the tables of gnns_on_syn.py:9-53.
 * A job: the pattern as in wdg_neighbor_max_job - rowptr int32 [n_rows + 1], col int32 [nnz], kept_len int32 [n_rows] or NULL (a plain
 * CSR pattern; otherwise col is a thinned pattern's kept_col and a row's length is min(kept_len[i], rowptr[i + 1] - rowptr[i])) -,
 * X [n_cols, n_feat] fp32 with leading dimension ldx, the results mean, std, mx, mn, each [n_rows, n_feat] fp32 with a leading dimension
 * of its own (the four may be column slices of one [n_rows, 4 n_feat] matrix), arg_max and arg_min, int32 [n_rows, n_feat] with leading
 * dimensions of their own, cnt int32 [n_rows], and eps.  A NULL mean, std, mx, mn, arg_max or arg_min is not wanted and not written
 * (std needs the mean internally either way); cnt is always written.  The definition (tests/_neighbor_moments_ref.py restates it in
 * numpy), for row i and column f:
 *   positions    the row's first `len` stored entries sit at positions e = 0 .. len - 1; j = col[rowptr[i] + e].  An entry whose j lies
 *                outside [0, n_cols) - which includes -1 - is SKIPPED, never read through.  c = the number of entries NOT skipped:
 *                copies of a column count per occurrence, in c and in the sums, as in every sum of this library.  cnt[i] = c.
 *   s1           FOUR CHAINS BY POSITION: chain k is acc = acc + X[j, f] from +0 over the entries not skipped with e % 4 == k, in stored
 *                order; s1 = (c0 + c1) + (c2 + c3)
 *   mean[i, f]   s1 / (float)c
 *   s2           the same four chains with d = X[j, f] - mean[i, f]; acc = fmaf(d, d, acc)
 *   std[i, f]    var = s2 / (float)c; sqrtf(var + eps)
 *                - one rounded fp32 operation each, the fmaf written out, nothing else fused (csrc/neighbor_moments.hip is compiled with
 *                contraction off); the division and sqrtf are the correctly rounded ones.  Where a result is a NaN its payload is not
 *                part of the contract.
 *   mx, arg_max  EXACTLY the Y and arg of wdg_neighbor_max_batched_f32 on the same pattern and X: the total order - a NaN above
 *                everything, -0 == +0, a tie to the lower j -, the winner's BITS copied, the SET of the entries not skipped (copies of
 *                one j are one pair)
 *   mn, arg_min  the same with WDG_NEIGHBOR_MAX_MIN
 *   c == 0       mean = std = mx = mn = +0, arg_max = arg_min = -1.  A row whose extent lies outside [0, nnz] is left untouched (cnt
 *                too).  Every other element of the wanted blocks [0 : n_rows][0 : n_feat] is written and nothing outside them.
 * The chains BY POSITION are the point: a column's bits depend neither on the job's width nor on how many lanes share the row - a job
 * has the same bits alone and in any table, a column the same bits at any job width -, a wide job has four independent adds per column,
 * and a narrow one work for four lane groups: a wave per row and per panel of 256 columns (four per lane); of the lane groups that hold
 * no columns up to three more take whole chains (at n_feat <= 16 four lanes cover the columns and four shares walk the row).  The
 * extremes are merged across the shares under the order, the chain sums by the tree above.  A row of one step stays in registers for the
 * second pass, a longer one is read twice.  There is NO multi-wave path for a hub row.  No LDS, no atomics.  16-byte loads / stores where
 * the pointer, the leading dimension and n_feat (a multiple of 4) allow - the wave's decision, one for X and one per result.
 * No two of X and the results may overlap.
 * max_rows, max_feat: the table's largest n_rows and n_feat (rows / columns beyond them are not worked on).
 * Refused before any HIP call (WDG_ERR_INVALID): negative counts, more than 65535 jobs (a job per grid z), a NULL table with
 * n_jobs > 0, max_feat above 256 * 65535.  n_jobs == 0, max_rows == 0 or max_feat == 0: WDG_OK, nothing is launched.  What is wrong inside
 * a job - a negative n_rows, n_cols, n_feat or nnz, flag bits (none is defined), a reserved word that is not 0, an eps that is negative or
 * not finite, a leading dimension below n_feat (of a result: where it is given), a NULL rowptr or cnt, a NULL col or X with nnz > 0 and
 * n_cols > 0, two of X and the results at one address - is refused by wdg_neighbor_moments_check_jobs on the HOST copy of the table
 * (neighbor_moments.NeighborMomentsBatch calls it before it uploads), and the launch leaves such a job untouched.  A job with
 * n_rows == 0 or n_feat == 0 is skipped.
 */
typedef struct wdg_neighbor_moments_job {
    const int32_t *rowptr;    /* [n_rows + 1] */
    const int32_t *col;       /* [nnz]: a CSR pattern's col, or a thinned pattern's kept_col */
    const int32_t *kept_len;  /* [n_rows], or NULL: every row's whole extent */
    const float *X;           /* [n_cols, n_feat], leading dimension ldx */
    float *mean;              /* out [n_rows, n_feat], leading dimension ld_mean, or NULL */
    float *std;               /* out, ld_std, or NULL */
    float *mx;                /* out, ld_mx, or NULL */
    float *mn;                /* out, ld_mn, or NULL */
    int32_t *arg_max;         /* out [n_rows, n_feat], ld_amax, or NULL */
    int32_t *arg_min;         /* out, ld_amin, or NULL */
    int32_t *cnt;             /* out [n_rows] */
    int64_t ldx, ld_mean, ld_std, ld_mx, ld_mn, ld_amax, ld_amin;
    int32_t n_rows, n_cols, n_feat, nnz;
    float eps;                /* >= 0, finite */
    int32_t flags;            /* must be 0 */
    int32_t reserved;         /* must be 0 */
    int32_t reserved2;        /* must be 0 */
} wdg_neighbor_moments_job;
int wdg_neighbor_moments_batched_f32(const wdg_neighbor_moments_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_feat,
                                     wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the neighbour moments above (utils/util_funcs.py:29-36, 365-380), on the
 *           host's table */
int wdg_neighbor_moments_check_jobs(const wdg_neighbor_moments_job *jobs_host, int32_t n_jobs);

/*
 * The backward pass of the neighbour moments: d_X from the gradients of the four statistics, TWO launches inside one entry, no atomics.
 * replaces: nothing of the reference - the transposed product that stands behind normalize, utils/util_funcs.py:29-36, and
 *           normalize_tensor, utils/util_funcs.py:365-380, in the other models' backward passes (gnns_on_syn.py:9-53 holds their tables).
 * A job: rowptr, col, kept_len of the TRANSPOSED pattern, plain or thinned (n_rows rows - the forward pass's columns - over n_src
 * sources - the forward pass's rows); X [n_rows, n_feat] (the forward pass's X); g_mean, g_std, g_max, g_min [n_src, n_feat] fp32 (the
 * gradients of the four statistics: a NULL one reads as +0); mean, std, arg_max, arg_min [n_src, n_feat] and cnt [n_src] (the forward
 * pass's); A and B [n_src, n_feat] fp32 with leading dimension ldw, a WORKSPACE the table owns; D [n_rows, n_feat] fp32 with leading
 * dimension ldd (d_X).  Every matrix has a leading dimension of its own.
 * Launch 1, per forward row i and column f (c = cnt[i]):
 *   c == 0: A[i, f] = B[i, f] = +0.  Otherwise B = g_std[i, f] / ((float)c * std[i, f]) (+0 where g_std is NULL) and
 *   A = fmaf(-B, mean[i, f], g_mean[i, f] / (float)c).
 * Launch 2, per transposed row j and column f, over the row's first `len` entries at positions e, i = col[q]; an entry with i outside
 * [0, n_src) is SKIPPED:
 *   SA, SB       four chains by position each, as in the forward pass, over A[i, f] and B[i, f] of the entries not skipped (copies count
 *                per occurrence, as they did in the forward sums)
 *   RM, Rm       four chains by position each over g_max[i, f] where arg_max[i, f] == j, and over g_min[i, f] where arg_min[i, f] == j,
 *                under the duplicate rule of wdg_neighbor_max_backward_batched_f32: an entry whose i equals the i of the previous
 *                entry that was not skipped routes nothing (one add per routed term, none elsewhere)
 *   every group of four chains is merged (c0 + c1) + (c2 + c3);  D[j, f] = fmaf(X[j, f], SB, (SA + RM) + Rm)
 * - the gradient of mean / sqrt(mean((x - m)^2) + eps) / amax / amin; one rounded operation each, the fmaf written out.  A row of the
 * transposed pattern whose extent lies outside [0, nnz] is left untouched.  A job has the same bits alone and in any table, a column the
 * same bits at any job width.  NO multi-wave path for a hub row.  No LDS, no atomics.  May any two operands alias?  None: D, A and B must
 * not overlap each other or anything the job reads.
 * max_rows, max_src, max_feat: the table's largest n_rows, n_src and n_feat.
 * Refused before any HIP call (WDG_ERR_INVALID): as above (max_src counts as a count).  What is wrong inside a job - a negative shape,
 * flag bits, a reserved word that is not 0, a leading dimension below n_feat, a NULL rowptr, X, D, A, B or cnt, a NULL col with nnz > 0 and
 * n_src > 0, a g_mean without mean, a g_std without mean and std, a g_max or g_min without its arg, D, A or B at the address of another
 * operand - is refused by wdg_neighbor_moments_backward_check_jobs on the HOST copy of the table
 * (neighbor_moments.NeighborMomentsBackwardBatch calls it before it uploads), and the launches leave such a job untouched.
 */
typedef struct wdg_neighbor_moments_backward_job {
    const int32_t *rowptr;    /* [n_rows + 1]: the TRANSPOSED pattern's */
    const int32_t *col;       /* [nnz] */
    const int32_t *kept_len;  /* [n_rows], or NULL */
    const float *X;           /* [n_rows, n_feat], ldx: the forward pass's X */
    const float *g_mean;      /* [n_src, n_feat], ld_gmean, or NULL: +0 */
    const float *g_std;       /* ld_gstd, or NULL */
    const float *g_max;       /* ld_gmax, or NULL */
    const float *g_min;       /* ld_gmin, or NULL */
    const float *mean;        /* [n_src, n_feat], ld_mean: the forward pass's */
    const float *std;         /* ld_std */
    const int32_t *arg_max;   /* ld_amax */
    const int32_t *arg_min;   /* ld_amin */
    const int32_t *cnt;       /* [n_src] */
    float *A;                 /* workspace [n_src, n_feat], ldw */
    float *B;                 /* workspace [n_src, n_feat], ldw */
    float *D;                 /* out [n_rows, n_feat], ldd: d_X */
    int64_t ldx, ld_gmean, ld_gstd, ld_gmax, ld_gmin, ld_mean, ld_std, ld_amax, ld_amin, ldw, ldd;
    int32_t n_rows, n_src, n_feat, nnz;
    int32_t flags;            /* must be 0 */
    int32_t reserved;         /* must be 0 */
} wdg_neighbor_moments_backward_job;
int wdg_neighbor_moments_backward_batched_f32(const wdg_neighbor_moments_backward_job *jobs_dev, int32_t n_jobs, int32_t max_rows, int32_t max_src,
                                              int32_t max_feat, wdg_stream_t stream);
/* replaces: nothing of its own - the per-job refusals of the backward pass above (utils/util_funcs.py:29-36, 365-380), on the host's
 *           table */
int wdg_neighbor_moments_backward_check_jobs(const wdg_neighbor_moments_backward_job *jobs_host, int32_t n_jobs);

#ifdef __cplusplus
}
#endif
#endif /* WDG_H */
