/*
 * stin_hip.h - C ABI of libstin_hip.so: the MI355X (gfx950) kernels behind the
 * STINet graph-convolution hot path.
 *
 * The reference (johnpeterflynn/surface-texture-inpainting-net) is 100 % Python and
 * owns no native ABI: every entry point below replaces a call the reference makes
 * into the third-party torch_geometric / torch_scatter / ATen kernels.  The cited
 * file:line is the reference call site whose arithmetic the entry point takes over
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless noted.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Every call
 *     only ENQUEUES work on that stream: no allocation, no synchronisation, no
 *     ownership transfer; all buffers (incl. workspaces) are caller-owned and must
 *     outlive the enqueued work.  Re-entrant per stream, no global mutable state.
 *   - return value: 0 = ok, < 0 = argument error (STIN_E_*), > 0 = a hipError_t.
 *   - feature matrices are row-major fp32 with an explicit leading dimension `ld*`
 *     (in elements) so that column slices of a wider matrix can be passed.
 *   - graph structure is CSR with int32 `rowptr[N+1]` / `col[E]` (built once per
 *     sample by stin_csr_from_coo_i64 from the int64 index tensors at the Python
 *     boundary).  Within a row, entries keep the ORIGINAL edge order (stable),
 *     so every segmented reduction has a fixed, reproducible summation order -
 *     no float atomics anywhere.
 */
#ifndef STIN_HIP_H
#define STIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STIN_VERSION 102           /* major*10000 + minor*100 + patch */

#define STIN_OK 0
#define STIN_E_NULL (-1)           /* required pointer is NULL */
#define STIN_E_SIZE (-2)           /* negative / inconsistent size or leading dimension */
#define STIN_E_ALIGN (-3)          /* pointer / ld not aligned as the kernel requires */
#define STIN_E_WORKSPACE (-4)      /* workspace too small */
#define STIN_E_UNSUPPORTED (-5)    /* shape outside what this build supports */

typedef void* stin_stream_t;
typedef void* stin_event_t;  /* a hipEvent_t owned by the caller (only stin_net_bwd's optional side stream and timing brackets use events) */
/* bf16 STORAGE variants (*_bf16): the same operation on row-major bfloat16 matrices (raw 16-bit patterns, the
 * upper half of an fp32).  Every kernel widens to fp32 on load, computes and accumulates in fp32 and rounds to
 * nearest-even on store; statistics, weights, biases, index plans and weight gradients stay fp32.  Halves the HBM
 * bytes of the streaming/gather kernels and puts the GEMMs on one bf16 MFMA per k-step.  The reference is
 * fp32-only: this is the build's mixed-precision extension for BASELINE configs 3 and 5 (stated tolerance, not
 * the 1e-4 fp32 bar).  bf16 rows must be 4-channel vectorisable: C % 4 == 0, ld % 4 == 0, 8-byte aligned. */
typedef uint16_t stin_bf16_t;

int stin_version(void);
/* Static, NUL-terminated description of a return code (host pointer). */
const char* stin_error_string(int code);

/* ------------------------------------------------------------------ graph plan --
 * COO -> CSR, grouping `E` (key, val) pairs by key in [0, N).
 *   rowptr[n] .. rowptr[n+1] delimit the entries of key n, in ORIGINAL pair order;
 *   col[e]  = val[perm[e]]  (or perm[e] when val == NULL);
 *   perm[e] = index of the pair now at CSR slot e (may be NULL);
 *   inv_deg[n] = 1 / max(1, rowptr[n+1]-rowptr[n])       (may be NULL);
 *   *bad (device int32, may be NULL) is set non-zero when a key is outside [0, N)
 *   or a val outside [0, val_limit) - the analogue of the IndexError the reference's
 *   index_select / scatter raise on CPU; such pairs are left out of the CSR.
 * Implementation: counting sort (integer-atomic histogram, one scan, atomic fill, rank within
 * row) - the result is the stable order above regardless of atomic arrival order.
 * Replaces the implicit indexing of PyG MessagePassing.propagate
 * (models/modules/edge_conv_filter.py:57 via torch_geometric) and of
 * torch_scatter (models/surfacetextureinpaintingnet.py:384-386,:422):
 *   destination CSR: key = edge_index[1], val = edge_index[0]
 *   source CSR     : key = edge_index[0], val = edge_index[1]
 *   children CSR   : key = hierarchy_trace_index_l, val = NULL
 */
size_t stin_csr_workspace_bytes(int64_t E, int64_t N);
int stin_csr_from_coo_i64(const int64_t* key, const int64_t* val, int64_t E, int64_t N,
                          int64_t val_limit, int32_t* rowptr, int32_t* col, int32_t* perm,
                          float* inv_deg, int32_t* bad, void* workspace, size_t workspace_bytes,
                          stin_stream_t stream);
/* Both CSRs of one directed edge set in the same launches: by destination (col = sources, inv_deg =
 * 1/max(1, in-degree)) for the forward gather and dA, by source (col = targets) for dB.
 * xslot[s] (may be NULL) = destination-CSR slot of the edge at source-CSR slot s: lets the backward
 * find an edge's saved ReLU mask (stored per destination-CSR slot) from the source side;
 * w_src[s] (may be NULL; needs xslot and inv_deg_dst) = inv_deg_dst[col_src[s]], the mean weight of
 * that edge's target, laid out sequentially for the dB pass. */
int stin_csr_pair_from_edges_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N,
                                 int32_t* rowptr_dst, int32_t* col_dst, float* inv_deg_dst,
                                 int32_t* rowptr_src, int32_t* col_src, int32_t* xslot, float* w_src,
                                 int32_t* bad, void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* Every CSR structure of a sample in ONE batch of four kernel launches behind one memset of the counters (round 3; the two entry points above are batches of one job).
 * A job = one CSR grouped by a[] with the value b[] (b == NULL: the pair id itself, e.g. the children of every coarse vertex
 * of hierarchy_trace_index_l) or, with pair != 0, both CSRs of one directed edge set (a = edge_index[1] = targets,
 * b = edge_index[0] = sources; outputs as stin_csr_pair_from_edges_i64).  narrow_out (may be NULL): the int32 copy of a[]
 * (0 where the PAIR is left out: a[] out of range, or - with a value array - b[] out of range) - the `trace` the pool / unpool
 * kernels gather with, written by the first pass over the pairs.
 * jobs: HOST array (copied into the kernel arguments); out-of-range pairs set *bad and are left out, as above.
 * workspace >= stin_plan_build_workspace_bytes(sum of E, sum over jobs of (pair ? 2 : 1) * N + 1). */
#define STIN_PLAN_MAX_JOBS 16
typedef struct stin_plan_job {
    const int64_t *a, *b;
    int64_t E, N, b_limit;
    int32_t *rowptr0, *col0, *perm0;
    float* inv_deg0;
    int32_t *rowptr1, *col1, *xslot;
    float* w_src;
    int32_t* narrow_out;
    int32_t pair, reserved;
} stin_plan_job_t;                                    /* 11 pointers + 3 int64 + 2 int32 = 120 bytes */
size_t stin_plan_build_workspace_bytes(int64_t total_E, int64_t total_counters);
int stin_plan_build_many(const stin_plan_job_t* jobs, int n_jobs, int32_t* bad, void* workspace, size_t workspace_bytes,
                         stin_stream_t stream);
/* Vertex renumbering by locality (round 3; optional - SURVEY 7.3 "optional vertex reordering, inverted at the boundary").  The
 * reference has no counterpart: its kernels (torch_scatter / PyG gathers, models/surfacetextureinpaintingnet.py:384-391 and the
 * EdgeConv message passing) index rows in dataset order; on the GPU the gathered neighbour rows then all cross the fabric.
 *   stin_vertex_order_f32: pos [n0, >= 3] (ld_pos floats per row: x, y, z at columns 0..2 of the pointer passed) -> per level
 *     rank int32 [n + 1] (old id -> new id, rank[n] = n) and order int32 [n] (new -> old; may be NULL).  Level 0: stable sort
 *     by the 30-bit Morton code on the bounding box; level l >= 1: stable sort by the smallest new id among the children under
 *     levels[l].trace (the level l - 1 -> l map, int64 [n_{l-1}]).  Deterministic.
 *   stin_relabel_many_i64: out[i] = rank[ids[i]] (limit where ids[i] is outside [0, limit): the CSR build then flags and drops
 *     it exactly like an out-of-range original id) for up to 16 index arrays in one launch.  A job with rank_fine != NULL is a
 *     TRACE (ids = trace [n_fine], rank = the coarse level's): it also writes fine_out[i] = rank_fine[i] (the pair's second
 *     member, int64 for stin_plan_build_many) and trace_out[rank_fine[i]] = out[i] (int32: new fine id -> new coarse id, 0
 *     where out of range).  Index arrays keep their ORDER: CSR rows and children lists built from them keep the reference's. */
typedef struct stin_order_level {
    int64_t n;
    const int64_t* trace;
    int32_t* rank;
    int32_t* order;
} stin_order_level_t;
size_t stin_vertex_order_workspace_bytes(int64_t n_max);
int stin_vertex_order_f32(const float* pos, int64_t ld_pos, const stin_order_level_t* levels, int n_levels, void* workspace,
                          size_t workspace_bytes, stin_stream_t stream);
#define STIN_RELABEL_MAX_JOBS 16
typedef struct stin_relabel_job {
    const int64_t* ids;
    int64_t n;
    const int32_t* rank;
    int64_t limit;
    int64_t* out;
    const int32_t* rank_fine;
    int64_t* fine_out;
    int32_t* trace_out;
} stin_relabel_job_t;                                  /* 64 bytes */
int stin_relabel_many_i64(const stin_relabel_job_t* jobs, int n_jobs, stin_stream_t stream);
/* dst[i] = (int32) src[i]; *bad set when a value is outside [0, limit). */
int stin_narrow_i64_to_i32(const int64_t* src, int64_t n, int64_t limit, int32_t* dst, int32_t* bad,
                           stin_stream_t stream);

/* -------------------------------------------------------- segmented reductions --
 * out[n, :] = sum_{e in row n} src[col ? col[e] : e, :]        (mean: / max(1, deg))
 * The standalone scatter-add / scatter-mean (torch_scatter.scatter_{sum,mean},
 * models/surfacetextureinpaintingnet.py:384; SAGEConv mean aggregation,
 * models/modules/sage_conv_filter.py:122; backward of `x[traces]`, :391; PyG
 * aggr='add' in utils/metrics/graph_metrics.py:6-16).
 */
#define STIN_SEG_NONTEMPORAL 2   /* OR-ed into `mean`: the gathered source is read once and is larger than the 256 MB Infinity Cache
                                   (the standalone scatter-add of BASELINE: 307 MB) -> non-temporal loads, +5 %; on a
                                   cache-resident source they cost 25-40 %, so the caller decides by the source's size */
int stin_segment_sum_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* col,
                         int64_t N, int C, int mean, float* out, int64_t ld_out, stin_stream_t stream);

/* ------------------------------------------------------------ fused edge stage --
 * EdgeConv(aggr='mean') after the exact algebraic restructure:
 *   h[i, :] = (1/max(1,deg i)) * sum_{j in N(i)} ReLU(A[i, :] + B[j, :])
 * with A = x (Wa-Wb)^T + b1, B = x Wb^T per-VERTEX GEMM outputs.  Takes over the
 * per-edge gather/cat/Linear/ReLU/scatter chain of PyG EdgeConv
 * (models/modules/edge_conv_filter.py:46-57,
 *  models/modules/edge_conv_translation_invariance.py:19-21).
 *   fwd     : destination CSR.  With indicator != 0 the kernel also writes columns
 *             H..H+3 of `out` = ([deg i > 0], 0, 0, 0) (needs ldo >= H+4): the following
 *             per-vertex GEMM against [W2 | b2 | 0 0 0] then yields W2 h + b2 [deg > 0],
 *             i.e. PyG's "vertices without in-edges aggregate to exactly 0".
 *             With mask != NULL (needs H % 128 == 0) it also stores, per destination-CSR edge slot e,
 *             the H ReLU decisions [A[i,c] + B[j,c] > 0] as H bits at mask[e * H/32 ...] (E*H/8 bytes,
 *             32x smaller than an fp32 [E,H] tensor) for the masked backward below.  Bit order inside
 *             a slot is the wave-ballot order of the kernel ([chunk][x,y,z,w][lane]); the three
 *             kernels agree on it, it is not meant to be read elsewhere.
 *   bwd_dst : dA[i,:] = inv_deg[i] * G[i,:] * #{j in N(i) : A[i,:]+B[j,:] > 0}
 *   bwd_src : dB[j,:] = sum_{i : j in N(i)} inv_deg[i] * G[i,:] * [A[i,:]+B[j,:] > 0]
 *             (source CSR; the backward scatter-add becomes a gather, no atomics)
 */
int stin_edge_relu_mean_fwd_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                                const int32_t* rowptr, const int32_t* col, int64_t N, int H,
                                float* out, int64_t ldo, int indicator, uint32_t* mask, stin_stream_t stream);
/* The same stage through a row map: A, B hold M distinct rows and row i of the N stands for row row_map[i] of them (a decoder
 * block behind an unpool step: row_map = the unpool trace, A | B = the first product over the COARSE rows):
 *   out[i,:] = mean_{j in N(i)} ReLU( A[row_map[i],:] + B[row_map[j],:] )
 * Same arithmetic, indicator column and mask words as stin_edge_relu_mean_fwd_f32 on the gathered rows, bit for bit.  fp32 rows,
 * H a saved-mask width (128, 256, 512, 1024, 2048), 16-byte rows; every row_map value must lie in [0, M). */
int stin_edge_relu_mean_fwd_map_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rowptr,
                                    const int32_t* col, const int32_t* row_map, int64_t N, int H, float* out, int64_t ldo,
                                    int indicator, uint32_t* mask, stin_stream_t stream);
/* Backward from the saved mask instead of recomputing it (H % 128 == 0):
 *   bwd_dst_mask: dA[i,:] = inv_deg[i] * G[i,:] * popcount over the in-edge slots of i   (streams H/8 bytes
 *                 per edge instead of gathering a B row)
 *   bwd_src_mask: dB[j,:] = sum_{out-edge slots s: j->i} w_src[s] * G[i,:] * mask[xslot[s]] (gathers G rows and
 *                 mask words: half the bytes of the recompute form) */
int stin_edge_relu_mean_bwd_dst_mask_f32(const float* G, int64_t ldg, const uint32_t* mask, const int32_t* rowptr,
                                         int64_t N, int H, float* dA, int64_t ldda, stin_stream_t stream);
int stin_edge_relu_mean_bwd_src_mask_f32(const float* G, int64_t ldg, const float* w_src, const uint32_t* mask,
                                         const int32_t* rowptr_src, const int32_t* col_src, const int32_t* xslot,
                                         int64_t N, int H, float* dB, int64_t lddb, stin_stream_t stream);
/* bwd_dst_mask and bwd_src_mask in ONE launch (the dB blocks first, then the dA blocks); results bit-identical to the two
 * calls above.  Optional rider (copy_src != NULL): copy_dst[i, :C_copy] = copy_src[i, :C_copy] for all N rows in the same
 * launch (C_copy <= H, multiple of 4 (bf16: 8), 16-byte aligned rows) - the block backward's dY[:, 2H:] = g. */
int stin_edge_relu_mean_bwd_mask_f32(const float* G, int64_t ldg, const uint32_t* mask, const int32_t* rowptr_dst,
                                     const float* w_src, const int32_t* rowptr_src, const int32_t* col_src,
                                     const int32_t* xslot, int64_t N, int H, float* dA, int64_t ldda, float* dB,
                                     int64_t lddb, const float* copy_src, int64_t ld_copy_src, float* copy_dst,
                                     int64_t ld_copy_dst, int C_copy, stin_stream_t stream);
/* Translation-invariant blocks in the COMPACT layout (round 6; STIN_TI_COMPACT below).  The reference's message is
 * nn(x_j - x_i) (models/modules/edge_conv_translation_invariance.py:20-22): W1 (x_j - x_i) + b1 = A_i + B_j with B = x W1^T and
 * A_i = b1 - B_i.  A is therefore not a GEMM output at all:
 *   fwd_ti:      out / mask exactly as stin_edge_relu_mean_fwd_f32 given A_i = fl(b1 - B_i), formed per row (b1 [H] or NULL = zeros);
 *                a GEMM output A = x (-W1)^T + b1 differs from that by <= 1 ulp of the matrix-core accumulator (the MFMA adder is not
 *                symmetric under negation) - both are fp32 evaluations of the same expression;
 *   bwd_mask_ti: D [N, H] = dB - dA (both halves of stin_edge_relu_mean_bwd_mask_f32 for the same row, one rounding for the
 *                difference) - the gradient w.r.t. B in the compact layout - plus colsum [colsum_rows][H]: per-workgroup column sums
 *                of dA in a fixed order (db1 = their sum; sum_i D_i itself is ~ 0).  colsum_rows >= stin_edge_bwd_ti_colsum_rows(N, H).
 *                Same optional row-copy rider as the pair launch.  fp32 rows, H in {128, 256, 512, 1024, 2048}. */
int stin_edge_relu_mean_fwd_ti_f32(const float* b1, const float* B, int64_t ldb, const int32_t* rowptr, const int32_t* col,
                                   int64_t N, int H, float* out, int64_t ldo, int indicator, uint32_t* mask, stin_stream_t stream);
int64_t stin_edge_bwd_ti_colsum_rows(int64_t N, int H);
/* db1 [H] = the sum of the `rows` rows of colsum, in the order stin_edgeconv_wgrad_ti's finalize launch folds them (same bits) */
int stin_edge_bwd_ti_colsum_fold_f32(const float* colsum, int64_t rows, int H, float* db1, stin_stream_t stream);
int stin_edge_relu_mean_bwd_mask_ti_f32(const float* G, int64_t ldg, const uint32_t* mask, const int32_t* rowptr_dst,
                                        const float* w_src, const int32_t* rowptr_src, const int32_t* col_src,
                                        const int32_t* xslot, int64_t N, int H, float* D, int64_t ldd, const float* copy_src,
                                        int64_t ld_copy_src, float* copy_dst, int64_t ld_copy_dst, int C_copy, float* colsum,
                                        int64_t colsum_rows, stin_stream_t stream);
int stin_edge_relu_mean_bwd_dst_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                                    const float* G, int64_t ldg, const int32_t* rowptr,
                                    const int32_t* col, int64_t N, int H, float* dA, int64_t ldda,
                                    stin_stream_t stream);
int stin_edge_relu_mean_bwd_src_f32(const float* A, int64_t lda, const float* B, int64_t ldb,
                                    const float* G, int64_t ldg, const float* inv_deg,
                                    const int32_t* rowptr_src, const int32_t* col_src, int64_t N, int H,
                                    float* dB, int64_t lddb, stin_stream_t stream);

/* --------------------------------------------------------------- pool / unpool --
 * Max pool over the children CSR of each coarse vertex with torch_scatter's CPU
 * rule: strict '>' walking children in ascending fine-vertex order => the FIRST
 * maximum wins ties; empty clusters give value 0 and arg = -1
 * (models/surfacetextureinpaintingnet.py:386).  Backward routes g to arg only.
 */
int stin_pool_max_fwd_f32(const float* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                          int64_t n_coarse, int C, float* out, int64_t ldo, int32_t* arg,
                          stin_stream_t stream);
int stin_pool_max_bwd_f32(const float* g, int64_t ldg, const int32_t* arg, const int32_t* trace,
                          int64_t n_fine, int C, float* gx, int64_t ldgx, stin_stream_t stream);
/* out[v, :] = src[idx[v], :] * (row_scale ? row_scale[idx[v]] : 1): the unpool gather
 * `x[traces]` (models/surfacetextureinpaintingnet.py:390-391) and the mean-pool backward. */
int stin_gather_rows_f32(const float* src, int64_t ld_src, const int32_t* idx, const float* row_scale,
                         int64_t n_out, int C, float* out, int64_t ldo, stin_stream_t stream);
/* out[e, :] = a[idx_a[e], :] + b[idx_b[e], :]: the per-edge pre-activation Lin1([x_i ; x_j - x_i]) = A[dst] + B[src]
 * of the BatchNorm edge MLP (models/modules/edge_conv_filter.py:34-44), one pass instead of two gathers and an add. */
int stin_gather_add_rows_f32(const float* a, int64_t lda, const int32_t* idx_a, const float* b, int64_t ldb,
                             const int32_t* idx_b, int64_t n_out, int C, float* out, int64_t ldo, stin_stream_t stream);
/* (round 5) the same pass WITH the first stage of the column moments of its output - the BatchNorm1d over the E edge rows that
 * follows it (edge_conv_filter.py:36-38): partial [groups][2][C] doubles (per block: sum, sum of squares), groups =
 * stin_gather_add_rows_stats_groups(N, C) (0: not supported for this shape); second stage stin_moments_final_f32.  Saves the
 * separate moments pass over the [E, C] matrix just written. */
int64_t stin_segment_mean_stats_groups(int64_t N, int C);
/* segment MEAN of the rows src[col[e]] over the CSR slots of every output row (stin_segment_sum_f32(mean)'s result, bit for bit)
 * AND partial [groups][2][C] = per-block column sums of the visited source rows and of their squares: the batch statistics of all
 * E edge rows for scatter_mean(BatchNorm1d(m)) (edge_conv_filter.py:40-44 + aggr='mean') from the pass that aggregates them. */
int stin_segment_mean_stats_f32(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* col, int64_t N, int C,
                                float* out, int64_t ldo, double* partial, size_t partial_bytes, stin_stream_t stream);
int64_t stin_gather_add_rows_stats_groups(int64_t N, int C);
int stin_gather_add_rows_stats_f32(const float* a, int64_t lda, const int32_t* idx_a, const float* b, int64_t ldb,
                                   const int32_t* idx_b, int64_t N, int C, float* out, int64_t ldo, double* partial,
                                   size_t partial_bytes, stin_stream_t stream);
/* Per-level graph-id vector (int64, bit-exact): scatter_max(batch, trace) and
 * batch.index_select(0, trace) (models/surfacetextureinpaintingnet.py:421-422,:446-447). */
int stin_batch_pool_i64(const int64_t* batch, const int32_t* rowptr, const int32_t* col, int64_t n_coarse,
                        int64_t* out, stin_stream_t stream);
int stin_gather_i64(const int64_t* src, const int32_t* idx, int64_t n_out, int64_t* out,
                    stin_stream_t stream);
/* Row ids of a batched FastInstanceNorm level in one pass (round 4; was five framework launches per level and step): gid[r] =
 * (int32) batch[r], and - sid != NULL - sid[r] = the reference's linspace slice of row r = the number of boundaries
 * ptr_sum[1 .. B] that are <= r (models/modules/fastinstancenorm.py:53-82 sums over torch.linspace(0, N, B + 1) slices;
 * ptr_sum: device int32 [B + 1]).  B <= 8192. */
int stin_norm_group_ids_i64(const int64_t* batch, const int32_t* ptr_sum, int B, int64_t n_rows, int32_t* gid, int32_t* sid,
                            stin_stream_t stream);

/* ----------------------------------------------- norm statistics and epilogues --
 * Column reductions over contiguous row ranges ptr[b]..ptr[b+1] (ptr == NULL: one
 * range [0, N)), fp64 accumulation in a fixed order, float results out[b, c]:
 *   STIN_RED_SUM     : sum x
 *   STIN_RED_CSQ     : sum (x - mean[gid])^2
 *   STIN_RED_DOT_ELU : out0 = sum dY * xc, out1 = sum dY  with xc = x - mean[gid],
 *                      dY = gout * ELU'(xc * rstd[gid])
 *   STIN_RED_COEF_XC : sum coef[sid] * (x - mean[gid])
 *   STIN_RED_MOMENTS : mean and rstd of each range in ONE pass over x (needs inv_cnt; ignores post)
 * `gid`/`sid` are per-row int32 group ids (NULL = 0).  They implement
 * FastInstanceNorm (models/modules/fastinstancenorm.py:42-107) including its
 * linspace-slice quirk (sums over `ptr` slices, centring through `gid`).
 * `post` finalises out0 (and out1) from the fp64 sums with the per-range factor
 * inv_cnt[b] (device float[B]; required unless post == STIN_POST_NONE).
 * workspace: stin_colreduce_workspace_bytes(C, B) bytes.
 */
#define STIN_RED_SUM 0
#define STIN_RED_CSQ 1
#define STIN_RED_DOT_ELU 2
#define STIN_RED_COEF_XC 3
#define STIN_RED_MOMENTS 4          /* one pass: out0 = mean, out1 = 1/sqrt(biased var + eps) from fp64 sum x, sum x^2 */
#define STIN_RED_DOT_BN 5           /* BatchNorm-with-affine backward sums (one range): d = gout (* [gamma n + beta > 0] with
                                       STIN_RED_DOT_BN_RELU), n = (x - mean) rstd; out0 = sum d n (= dgamma), out1 = sum d
                                       (= dbeta); coef = [gamma ; beta] as 2 x C floats                          */
#define STIN_RED_DOT_BN_RELU 6
#define STIN_POST_NONE 0            /* out = s                                  */
#define STIN_POST_SCALE 1           /* out = s * inv_cnt[b]            (mean)    */
#define STIN_POST_RSTD 2            /* out = 1/sqrt(s * inv_cnt[b] + eps)        */
#define STIN_POST_NORM_COEF 3       /* DOT_ELU only, ranges == graphs: out0 = -rstd^3 s0 inv_cnt, out1 = -rstd s1 inv_cnt:
                                       the k / m coefficients of stin_norm_act_bwd_* in the same launch (stin_norm_bwd_coef_f32) */
size_t stin_colreduce_workspace_bytes(int C, int B);
int stin_colreduce_f32(int mode, const float* x, int64_t ldx, const float* gout, int64_t ldg, int64_t N,
                       int C, const int32_t* ptr, int B, const int32_t* gid, const int32_t* sid,
                       const float* mean, const float* rstd, const float* coef, int post,
                       const float* inv_cnt, float eps, float* out0, float* out1,
                       void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* The arithmetic of the reductions, operation by operation (every line one IEEE operation, fp32 unless it says fp64; no fused
 * multiply-add; bf16 rows are widened to fp32 first, which is exact).  Per element, then added in fp64:
 *   SUM      t = double(x)
 *   CSQ      d = x - mean[gid];  t = double(d * d)
 *   DOT_ELU  xc = x - mean[gid];  n = xc * rstd[gid];  e = n > 0 ? 1 : exp(n);  dy = gout * e;  t0 = double(dy * xc), t1 = double(dy)
 *   COEF_XC  t = double(coef[sid] * (x - mean[gid]))
 *   MOMENTS  d = double(x);  t0 = d, t1 = d * d (fp64)
 *   DOT_BN   n = (x - mean) * rstd;  d = gout, or 0 where DOT_BN_RELU and not (gamma * n + beta > 0);  t0 = double(d * n), t1 = double(d)
 * (exp is the device's fast exponential, not correctly rounded: exact only where its argument is 0 or its result rounds to 0).
 * The fp64 sums are formed in a fixed order that depends on the route, so they are reproducible but defined to the bit only where
 * every partial sum is exact.  A range without rows gives the sum 0.  From the fp64 sum s of range b:
 *   POST_NONE       float(s)
 *   POST_SCALE      float(s) * inv_cnt[b]
 *   POST_RSTD       1 / sqrt(float(s) * inv_cnt[b] + eps)
 *   POST_NORM_COEF  r = rstd[b, c]:  out0 = ((-((r * r) * r)) * float(s0)) * inv_cnt[b],  out1 = (-(r * float(s1))) * inv_cnt[b]
 *   MOMENTS         all fp64: ic = double(inv_cnt[b]);  mu = s0 * ic;  var = s1 * ic - mu * mu, raised to 0 where negative;
 *                   mean = float(mu);  rstd = float(1 / sqrt(var + double(eps)))
 *
 * stin_colreduce_route: the route a reduction takes, host only - nothing is launched, no device is touched; stin_colreduce_*
 * launch from the same function.  nout = 1 or 2 outputs (2: DOT_ELU, MOMENTS, DOT_BN*); vec4 = the operands allow four channels
 * per lane (C % 4 == 0, rows of x / gout start on four elements at pitches that are multiples of four, mean / rstd / coef on 16
 * bytes); f32_rows = fp32 storage; cu > 0 = the compute units of the device the rules are asked for.  out8 (eight int64) =
 * { family (STIN_COLREDUCE_*), GC - the columns of a column group (one launch) - or the channels per lane 4 / 1 (two stages), row
 * chunks R (one launch) or nch (two stages), grid x, y, z of the first launch, fp64 partials the route writes into the workspace,
 * column groups ncg (one launch; else 0) }.  partials * 8 + 256 <= stin_colreduce_workspace_bytes(C, B) on every route.  Returns
 * STIN_E_UNSUPPORTED for bf16 rows without vec4, as the reduction itself does, or an argument error, and then writes nothing. */
#define STIN_COLREDUCE_ONE_LAUNCH 1     /* k_colreduce_t: partial [B][ncg][R][nout][GC], folded by the last block of a column group */
#define STIN_COLREDUCE_TWO_STAGE 2      /* k_colreduce: partial [B][nch][nout][C], then k_colreduce_final / k_moments_final */
int stin_colreduce_route(int64_t N, int C, int B, int nout, int vec4, int f32_rows, int cu, int64_t* out8);
/* Channels per lane of the elementwise passes stin_norm_act_res_fwd_* / stin_norm_act_bwd_*: 8 (bf16 rows, C % 8 == 0, data
 * pointers on 16 bytes, pitches multiples of 8), 4 (C % 4 == 0, data pointers on four elements, pitches multiples of 4), 1 (fp32
 * rows otherwise) or STIN_E_UNSUPPORTED (bf16 rows otherwise); 8 and 4 also need the per-group vectors on 16 bytes.  Host only.
 * elem_bytes 4 / 2; data_align: bytes that divide every data pointer; ld_align: elements that divide every row pitch. */
int stin_norm_lane_class(int C, int elem_bytes, int data_align, int stats_aligned16, int ld_align);
/* y = res + ELU((x - mean[gid]) * rstd[gid])    (res may be NULL; act: 1 = ELU, 0 = none)
 * In operations: n = (x - mean[gid]) * rstd[gid];  act: n = n > 0 ? n : expm1(n) (the device's expm1f);  y = n + res.  bf16 rows:
 * fp32 arithmetic on the widened values, y rounded to nearest-even once.
 * GraphResnetBlock epilogue (models/surfacetextureinpaintingnet.py:510-521) and the
 * tail norm+ELU (:465-466). */
int stin_norm_act_res_fwd_f32(const float* x, int64_t ldx, const float* mean, const float* rstd,
                              const int32_t* gid, const float* res, int64_t ldres, int64_t N, int C, int act,
                              float* y, int64_t ldy, stin_stream_t stream);
/* ... with the residual read through a row map: y[r] = res[row_map[r]] + ELU(...) (res, row_map not NULL) */
int stin_norm_act_res_fwd_map_f32(const float* x, int64_t ldx, const float* mean, const float* rstd, const int32_t* gid,
                                  const float* res, int64_t ldres, const int32_t* row_map, int64_t N, int C, int act, float* y,
                                  int64_t ldy, stin_stream_t stream);
/* dx = a[gid] * dY + k[sid] * (x - mean[gid]) + m[sid],  dY = gout * act'((x-mean[gid])*rstd[gid])
 * In operations: xc = x - mean[gid];  dY = gout (act 0), or gout * e with e of DOT_ELU above;  dx = (a[gid] * dY + k[sid] * xc) + m[sid]. */
int stin_norm_act_bwd_f32(const float* x, int64_t ldx, const float* gout, int64_t ldg, const float* mean,
                          const float* rstd, const float* a, const float* k, const float* m,
                          const int32_t* gid, const int32_t* sid, int64_t N, int C, int act, float* dx,
                          int64_t lddx, stin_stream_t stream);

/* ------------------------------------------------------------ per-vertex GEMMs --
 * Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMMs for the tall-skinny per-VERTEX products the
 * restructure leaves (reference: the per-EDGE aten::addmm of Lin1/Lin2 in
 * models/modules/edge_conv_filter.py:47-52, the shortcut Linear at
 * models/surfacetextureinpaintingnet.py:515-516 and the tail Linears :464,:467).
 *   nt: C[M, Nc] = A[M, K] . W[Nc, K]^T + bias[Nc] * (row_mask ? row_mask[m * ld_mask] : 1) (+ residual[M, Nc])
 *       forward, and dgrad with W := W^T.  row_mask = the [deg > 0] indicator gives PyG's
 *       "no in-edges -> exactly 0" (bias only where a vertex aggregated something).
 *       `precision` picks the matrix-core path: exact fp32 MFMA, or the bf16 cores (16x the fp32
 *       MFMA rate) on operands split on the fly into 2 or 3 bf16 pieces with fp32 accumulation.
 *   tn: dW[Nc, K (+1)] = G[M, Nc]^T . [X[M, K] | w]       weight gradient; with ones_column the
 *       extra last column is the bias gradient sum_m w[m] G[m, :] (w = row_weight or 1).
 *       Split over M into slabs that are summed in a fixed order (deterministic, no atomics).
 */
#define STIN_GEMM_F32 0      /* v_mfma_f32_32x32x2_f32: exact fp32 fmaf chain                          */
#define STIN_GEMM_BF16X3 2   /* fp32 operands split into 2 bf16 pieces, 3 bf16 MFMAs, ~2^-17 / product */
#define STIN_GEMM_BF16X6 3   /* 3 pieces (exact split), 6 bf16 MFMAs, ~2^-22 / product                 */
#define STIN_GEMM_F16X3 4    /* nt only: 2 fp16 pieces (11 bits each), 3 fp16 MFMAs, ~2^-22 / product for
                                |a| >= 2^-6, |w| >= 2^-9 (absolute 2^-28 / 2^-31 below: made for normalised
                                activations); A, W pre-scaled by 2^3, 2^6 internally (exact); needs
                                |A| < 8188, |W| < 1023 (outside: inf/NaN, never a silently wrong value)   */
#define STIN_GEMM_W_BF16 0x200     /* stin_gemm_nt_bf16 flag / stin_edgeconv_pack_f32 mode: the weight operand holds bf16 [Nc][K]
                                       (ldw in bf16 elements, K % 8 == 0, 16-byte aligned rows) instead of fp32 */
#define STIN_GEMM_W_PRESPLIT 0x100 /* nt, OR-ed into BF16X3 / F16X3: W already holds its two 16-bit pieces, per 4-wide
                                      k-group [hi x 4 | lo x 4] in the 16 bytes of the fp32 values it replaces (same
                                      shape / ld / footprint; made by stin_gemm_split_weights_f32 or the pack kernel) -
                                      the weight split is then done once per step instead of once per block    */
#define STIN_GEMM_W_FRAG 0x400     /* nt, OR-ed into PRESPLIT: the pre-split W is stored in MFMA FRAGMENT order where the shape
                                      takes it (stin_gemm_w_is_frag(Nc, K): the shapes of the resident-strip kernel - K % 64 == 0,
                                      Nc % 32 == 0, 128 <= K <= 256, Nc >= 320 - and of the all-columns kernel - Nc = 256 with
                                      K >= 512 or Nc = 128 with K >= 256, K % 64 == 0; other shapes keep the k-group form above,
                                      so the flag may be set unconditionally): for the 32-column tile t
                                      and the 16-wide k-step s, 2 KB at byte ((t * K/16 + s) * 64 + lane) * 32 hold lane
                                      (k-half h, column r) = h * 32 + r's [hi x 8 | lo x 8] of k = 16 s + 8 h .. + 7 - what the
                                      resident-strip kernel loads straight into its B fragments (same footprint as fp32; ldw
                                      is ignored).  Producer and consumer must agree: pass the same flag to
                                      stin_gemm_split_weights_f32 / stin_edgeconv_pack_f32 and to stin_gemm_nt_f32             */
int stin_gemm_w_is_frag(int Nc, int K);
int stin_gemm_split_weights_f32(const float* W, int64_t ldw, int Nc, int K, int precision, float* out, int64_t ldo,
                                stin_stream_t stream);
int stin_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                     const float* row_mask, int64_t ld_mask, const float* residual, int64_t ld_res, int64_t M,
                     int Nc, int K, float* C, int64_t ldc, int precision, stin_stream_t stream);
size_t stin_gemm_tn_workspace_bytes(int64_t M, int Nc, int K, int ones_column);
int stin_gemm_tn_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int Nc, int K,
                     int ones_column, const float* row_weight, int64_t ld_weight, float* dW, int64_t lddw,
                     int precision, void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* The geometry a TN product of this shape runs on - host only: nothing is launched, no device is touched; the TN entry points ask the
 * same function (tn_route, csrc/gemm_tn_route.inc).  storage 0 = fp32 rows, 1 = bf16 rows; ldg / ldx in elements; aligned16 != 0: both
 * operand bases are 16-byte aligned; precision as stin_gemm_tn_f32 (bf16 rows: STIN_GEMM_BF16X3).  out8 = { TI, TJ, tiles_i, tiles_j,
 * rows_per_chunk, chunks, vec, ws_eligible }: the output tile (TI == 0: the skinny-K kernel, whose block owns all columns), the tile
 * counts along Nc and K, the rows of one chunk and the number of chunks = partial slabs, vec = 16-byte operand loads, ws_eligible =
 * the producer / consumer kernel takes it.  The A/B switches STIN_TN_WS, STIN_TN_BIG and STIN_TN_TR are honoured as by the products
 * themselves; returns their argument errors and then writes nothing. */
int stin_gemm_tn_geometry(int storage, int64_t M, int Nc, int K, int64_t ldg, int64_t ldx, int aligned16, int ones_column,
                          int precision, int32_t* out8);
/* The same query with the kernel named: out10 (ten int32) = the eight values of stin_gemm_tn_geometry, then the kernel family
 * (STIN_TN_FAMILY_*) and the blocks of its grid.  A query of its own because stin_gemm_tn_geometry's callers hold eight values. */
#define STIN_TN_FAMILY_NONE 0      /* no rows: only the fold is launched */
#define STIN_TN_FAMILY_SKINNY 1    /* k_gemm_tn_skinny (fp32 rows, K <= 16: exact fp32 whatever the precision) */
#define STIN_TN_FAMILY_F32 2       /* k_gemm_tn, exact fp32 tiles */
#define STIN_TN_FAMILY_BF16S 3     /* k_gemm_tn_bf16s, the four-wave split-bf16 kernel (bf16x3 / bf16x6) */
#define STIN_TN_FAMILY_PC 4        /* k_gemm_tn_ws, the producer / consumer kernel (bf16x3, 128 x 128) */
#define STIN_TN_FAMILY_B16_REG 5   /* k_gemm_tn_b16, bf16 rows transposed in registers */
#define STIN_TN_FAMILY_B16_TR 6    /* k_gemm_tn_b16_tr, bf16 rows through transposed LDS reads (128 x 128, 256 x 256) */
int stin_gemm_tn_route(int storage, int64_t M, int Nc, int K, int64_t ldg, int64_t ldx, int aligned16, int ones_column,
                       int precision, int32_t* out10);

/* The route an NT product takes - which kernel family, on what tile, grid and LDS - host only: nothing is launched, no device is
 * touched.  The counterpart of stin_gemm_tn_geometry; the NT entry points ask the same function (csrc/gemm_nt_route.inc).
 *   storage 0 = fp32 rows (stin_gemm_nt_f32 and its variants), 1 = bf16 rows (stin_gemm_nt_bf16);
 *   precision: fp32 rows - STIN_GEMM_* with its W_PRESPLIT / W_FRAG flags; bf16 rows - 0 or STIN_GEMM_W_BF16;
 *   parts: STIN_NT_PART_* OR-ed - what the call carries besides the product; align: STIN_NT_ALIGN_* OR-ed - the 16-byte facts;
 *   cu > 0: the compute units of the device the rules are asked for.
 * out10 (ten int32) = { family (STIN_NT_*), BM, BN (the block's output tile), the family's parameter (panel: 32-row tiles per block;
 * strip: 21 / 22 / 41; all-columns: waves along M; stream: column tiles per block), vec (16-byte operand loads), vec_out (16-byte
 * stores; strip: the restaged epilogue), dynamic LDS bytes, grid x, grid y, statistics groups of the fused epilogue (0: none) }.
 * The STIN_NT_* / STIN_STRIP_CFG / STIN_DOTELU_FUSED switches are honoured as by the products themselves.  Returns the refusal the
 * product itself would answer (STIN_E_UNSUPPORTED, STIN_E_ALIGN) or an argument error, and then writes nothing. */
#define STIN_NT_NONE 0        /* no rows: nothing is launched */
#define STIN_NT_TILED 1       /* k_gemm_nt / k_gemm_nt_bf16s */
#define STIN_NT_STREAM 2      /* k_gemm_nt_stream */
#define STIN_NT_STRIP 3       /* k_gemm_nt_strip (fragment-order weights) */
#define STIN_NT_WIDE 4        /* k_gemm_nt_wide, the all-columns kernel (fragment-order weights, Nc = 128 / 256) */
#define STIN_NT_PANEL 5       /* k_gemm_nt_panel (fragment-order weights, Nc % 128 == 0) */
#define STIN_NT_B16_TILED 6   /* k_gemm_nt_b16 */
#define STIN_NT_B16_GLDS 7    /* k_gemm_nt_b16_glds */
#define STIN_NT_PART_BIAS 0x1
#define STIN_NT_PART_ROW_MASK 0x2
#define STIN_NT_PART_RESIDUAL 0x4
#define STIN_NT_PART_COLSTATS 0x8         /* stin_gemm_nt_colstats_f32; with DOTELU: stin_gemm_nt_dotelu_f32 */
#define STIN_NT_PART_DOTELU 0x10
#define STIN_NT_PART_BN_TF 0x20           /* the BatchNorm + ReLU operand transform (stin_gemm_nt_bn_f32) */
#define STIN_NT_PART_BN_BWD_STATS 0x40    /* stin_gemm_nt_bn_bwd_stats_f32 */
#define STIN_NT_PART_BN_BWD_APPLY 0x80    /* stin_gemm_nt_bn_bwd_apply_f32 */
#define STIN_NT_PART_OUT_F32 0x100        /* bf16 rows: fp32 output */
#define STIN_NT_PART_STREAM_ONLY 0x200    /* the streaming kernel asked for by name (stin_gemm_nt_stream_f32): no row threshold */
#define STIN_NT_ALIGN_IN 0x1              /* rows of A and W (BatchNorm backward: and of X) are 16-byte vectors: ld and base */
#define STIN_NT_ALIGN_OUT 0x2             /* rows of C and of the residual are */
#define STIN_NT_ALIGN_TF 0x4              /* the four vectors of the operand transform are */
#define STIN_NT_ALIGN_BIAS 0x8            /* the bias vector is (the streaming kernel's epilogue reads it 16 bytes at a time) */
int stin_gemm_nt_geometry(int storage, int64_t M, int Nc, int K, int precision, int parts, int align, int cu, int32_t* out10);

/* The same product with the weight gradient dW [Nc, K] (row pitch lddw >= K) and the bias gradient db [Nc] as SEPARATE
 * destinations (ones column implied): what torch.nn.Linear's backward hands to weight.grad / bias.grad
 * (models/surfacetextureinpaintingnet.py:461-466 `final_linear1`, and every generic nn.Linear of the build) without an
 * [Nc, K + 1] intermediate and the two slicing copies behind it. */
int stin_gemm_tn_wb_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, int64_t M, int Nc, int K,
                        const float* row_weight, int64_t ld_weight, float* dW, int64_t lddw, float* db, int precision,
                        void* workspace, size_t workspace_bytes, stin_stream_t stream);

/* The network's last layer in one launch per direction: y = tanh(x W^T + b), W [Nc, K], Nc <= 4 output (colour) channels,
 * K % 4 == 0, K <= 256 (STIN_E_UNSUPPORTED otherwise: callers fall back to stin_gemm_nt_* + a tanh) - replaces
 * `torch.tanh(self.final_linear2(vertex_features))` of models/surfacetextureinpaintingnet.py:470-471 and its autograd backward.
 *   fwd: x [N, K] rows (ldx), y [N, Nc] fp32 contiguous.  Exact fp32 products, per-row sums in a fixed order.
 *   bwd: g = dL/dy [N, Nc] and y [N, Nc] fp32 contiguous; dz = g (1 - y^2); dx [N, K] = dz W (NULL: not wanted),
 *        dW [Nc, K] = dz^T x, db [Nc] = column sums of dz (NULL: no bias) - block partials folded in a fixed order by the last
 *        block to arrive (deterministic, one launch); workspace >= stin_linear_tanh_bwd_workspace_bytes.
 * The bf16 variants read / write bf16 activation rows (x, dx); W, b, g, y and the gradients stay fp32. */
size_t stin_linear_tanh_bwd_workspace_bytes(int64_t N, int K, int Nc);
int stin_linear_tanh_fwd_f32(const float* x, int64_t ldx, const float* W, const float* b, int64_t N, int K, int Nc, float* y,
                             stin_stream_t stream);
int stin_linear_tanh_bwd_f32(const float* g, const float* y, const float* x, int64_t ldx, const float* W, int64_t N, int K, int Nc,
                             float* dx, int64_t lddx, float* dW, float* db, void* workspace, size_t workspace_bytes,
                             stin_stream_t stream);

/* dst[n, c] += alpha * src[n, c] * [rowptr[n + 1] > rowptr[n]] for c in [c0, c1), in place (fl(dst + fl(alpha src)); bf16 rows: the
 * same in fp32, rounded once to bf16; rows without an in-edge and the other columns are not written): the translation-invariant SAGE
 * message of models/modules/sage_conv_filter.py:87-90 (x_j[:, 3:9] -= x_i[:, 3:9]) under the mean aggregation, applied to the
 * aggregated rows (alpha = -1, rowptr = destination CSR) and, in the backward pass, to the input gradient. */
int stin_cols_axpy_rowmask_f32(float* dst, int64_t ldd, const float* src, int64_t lds, const int32_t* rowptr, int64_t N, int c0,
                               int c1, float alpha, stin_stream_t stream);
int stin_cols_axpy_rowmask_bf16(stin_bf16_t* dst, int64_t ldd, const stin_bf16_t* src, int64_t lds, const int32_t* rowptr,
                                int64_t N, int c0, int c1, float alpha, stin_stream_t stream);

/* out [N, Cp] (contiguous) = [x [N, Cin] (row pitch ldx) | zeros]: the network input - 10 channels per vertex,
 * datasets/scannetcolorgraph_dataloader.py:83-156 - padded to the 16-byte rows the first block's GEMM reads. */
int stin_pad_rows_f32(const float* x, int64_t ldx, int64_t N, int Cin, int Cp, float* out, stin_stream_t stream);
int stin_pad_rows_bf16(const stin_bf16_t* x, int64_t ldx, int64_t N, int Cin, int Cp, stin_bf16_t* out, stin_stream_t stream);

/* stin_gemm_nt_f32 (pre-split fragment-order weights) plus the FIRST stage of the instance-norm + ELU backward statistics of the
 * layer whose output gradient this product IS - inside the block backward the input gradient of block k (dY Wcat, + g for an
 * identity shortcut; models/surfacetextureinpaintingnet.py:507-521) is the output gradient of block k - 1, whose
 * FastInstanceNorm backward (models/modules/fastinstancenorm.py:42-107 through autograd) starts with two column sums over
 * (nx = that block's pre-norm rows, g).  partial [groups][2][Nc] doubles: per row group sum of dy (nx - nmean) and of dy with
 * dy = C ELU'((nx - nmean) nrstd); groups = stin_gemm_nt_dotelu_groups (0: shape / precision not served - keep
 * stin_colreduce_f32(STIN_RED_DOT_ELU)).  stin_norm_coef_from_partials_f32 folds them in a fixed order into the coefficients
 * k, m [C] of stin_norm_act_bwd_f32 for ONE graph (inv_cnt[0] = 1 / rows): the tail of stin_colreduce_f32(.., STIN_POST_NORM_COEF). */
int64_t stin_gemm_nt_dotelu_groups(int64_t M, int Nc, int K, int precision);
int stin_gemm_nt_dotelu_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* residual,
                            int64_t ld_res, int64_t M, int Nc, int K, float* C, int64_t ldc, int precision, const float* nx,
                            int64_t ld_nx, const float* nmean, const float* nrstd, double* partial, size_t partial_bytes,
                            stin_stream_t stream);
int stin_norm_coef_from_partials_f32(const double* partial, int64_t groups, int C, const float* rstd, const float* inv_cnt,
                                     float* k, float* m, stin_stream_t stream);

/* BatchNorm1d-with-affine over ALL rows, optionally followed by ReLU, for the per-edge MLP of SingleConvMeshNet
 * (models/modules/edge_conv_filter.py:34-44: Lin - BatchNorm1d - ReLU - Lin - BatchNorm1d over the E edge rows):
 *   fwd: y = act(gamma * (x - mean) * rstd + beta)            mean / rstd [C] from stin_colreduce_f32(STIN_RED_MOMENTS)
 *   bwd: dx = rstd * gamma * (d - Q * inv_n - n * P * inv_n)   d = gout * act'(.), n = (x - mean) * rstd,
 *        P = sum d n (= dgamma), Q = sum d (= dbeta) from stin_colreduce_f32(STIN_RED_DOT_BN[_RELU]).
 * act: 0 = none, 1 = ReLU.
 * In operations (fp32, no fused multiply-add): n = (x - mean) * rstd;  z = gamma * n + beta;  y = z, or 0 where act and not (z > 0);
 *   bwd: d = gout, or 0 where act and not (z > 0);  dx = (rstd * gamma) * ((d - Q * inv_n) - n * (P * inv_n)).
 */
int stin_bn_act_fwd_f32(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int64_t N, int C, int act, float* y, int64_t ldy, stin_stream_t stream);
int stin_bn_act_bwd_f32(const float* x, int64_t ldx, const float* gout, int64_t ldg, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, const float* P, const float* Q, float inv_n, int64_t N,
                        int C, int act, float* dx, int64_t lddx, stin_stream_t stream);

/* BatchNorm1d over the E edge rows followed by aggr='mean' (the second norm of that edge MLP): the affine map commutes with
 * the mean, so the forward normalises the N aggregated rows (stin_segment_sum_f32(mean) then stin_bn_act_fwd_f32, rows
 * without in-edges zeroed); this is the joint backward - the gradient of the raw edge rows m [E, C] from the VERTEX
 * gradient g [N, C] (zero on rows without in-edges):
 *   dm[e] = gamma rstd (g[dst e] * inv_deg[dst e] - Q inv_e - nhat_e P inv_e),  nhat_e = (m[e] - mean) rstd,
 * with P = sum_i g_i nhat(agg_i), Q = sum_i g_i from stin_colreduce_f32(STIN_RED_DOT_BN) over the N aggregated rows. */
int stin_bn_mean_bwd_f32(const float* m, int64_t ldm, const float* g, int64_t ldg, const int32_t* dst, const float* inv_deg,
                         const float* mean, const float* rstd, const float* gamma, const float* P, const float* Q,
                         float inv_e, int64_t E, int C, float* dm, int64_t lddm, stin_stream_t stream);

/* nn.BatchNorm1d's running-statistics update from the batch statistics (mean, rstd = 1/sqrt(biased var + eps)) in one
 * launch: running_mean <- (1 - m) running_mean + m mean; running_var <- (1 - m) running_var + m * unbias * max(1/rstd^2 -
 * eps, 0), unbias = n / (n - 1).  In operations: var = max(1 / (rstd * rstd) - eps, 0);  running_mean = (1 - m) * running_mean
 * + m * mean;  running_var = (1 - m) * running_var + m * (var * unbias). */
int stin_bn_running_stats_f32(const float* mean, const float* rstd, int C, float eps, float unbias, float momentum,
                              float* running_mean, float* running_var, stin_stream_t stream);

/* Round 5: the small passes of one fused EdgeConv(BN) layer of SingleConvMeshNet (singleconvmeshnet.EdgeConvBNLayerFn; reference
 * models/modules/edge_conv_filter.py:34-44 inside models/singleconvmeshnet.py:37-66 `ResBlock`), which were framework kernels:
 * stin_scmn_pack_f32: W1 [h2, 2 cin] (trans_inv: [h2, cin]), W2 [cout, h2], the two BatchNorm1d affine pairs ->
 *   wcat [2 h2, cin] = [Wa - Wb ; Wb] (trans_inv: [-W1 ; W1]), wcatT [cin, 2 h2], w2T [h2, cout],
 *   gb1 [2, h2] = [gamma1 ; beta1], gb2 [2, cout] (the `coef` operand of stin_colreduce_f32(STIN_RED_DOT_BN*)).
 * stin_scmn_unpack_f32: dwcat [2 h2, cin] -> dW1 in the reference layout (d/dWa = top, d/dWb = bottom - top; trans_inv: bottom - top).
 * stin_bn_affine_res_fwd_f32: y = [relu](res + [rowptr[r + 1] > rowptr[r]] (gamma ((x - mean) rstd) + beta)) over N rows - the
 *   BatchNorm affine of the aggregated rows, the "vertex has an in-edge" mask, the ResBlock's `x + f(x)` and its ReLU
 *   (singleconvmeshnet.py:60-66) in one pass; rowptr / res may be NULL.  Every operation is rounded on its own, in this order:
 *   gamma * ((x - mean) * rstd) + beta, times 1.0 or 0.0 (the mask IS a multiplication: 0 * inf = NaN), res + ., relu = (z > 0 ? z : +0).
 * stin_relu_mask_bwd_f32: g_eff = g [y > 0] (relu != 0; else g), g_in = g_eff [row has an in-edge]; g_eff may be NULL; both
 *   outputs are [N, C] with pitch C.  A y of +0, -0 or NaN fails y > 0 and gives +0; y is not read when relu == 0. */
/* The per-EDGE Linear of that layer with the BatchNorm1d + ReLU of its input applied while the operand rows are staged
 * (edge_conv_filter.py:36-40: Lin -> BN -> ReLU -> Lin): the normalised [E, 2 cout] matrix is never written.
 *   stin_gemm_nt_bn_f32: C [M, Nc] = relu(gamma ((A - mean) rstd) + beta) W^T, W plain fp32 [Nc, K] (no pre-split flags);
 *   stin_gemm_tn_bn_f32: dW [Nc, K] = G^T relu(gamma ((X - mean) rstd) + beta)  (the weight gradient from the pre-norm rows).
 * mean / rstd / gamma / beta: [K] fp32.  The transform is evaluated as relu(v s + t) with s = gamma rstd, t = beta - mean s
 * (3 operations per element on the vector-ALU-bound staging threads; equals stin_bn_act_fwd_f32(act = 1) to fp32 rounding,
 * ~1e-7 relative; both entry points use the same form).  precision as stin_gemm_nt_f32 / stin_gemm_tn_f32; workspace = stin_gemm_tn_workspace_bytes(M, Nc, K, 0). */
int stin_gemm_nt_bn_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int64_t M, int Nc, int K, float* C, int64_t ldc, int precision,
                        stin_stream_t stream);
int stin_gemm_tn_bn_f32(const float* G, int64_t ldg, const float* X, int64_t ldx, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int64_t M, int Nc, int K, float* dW, int64_t lddw, int precision,
                        void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* (round 5) The per-EDGE input-gradient product of that layer, dh = A W^T with A = dm [E, cout], W = W2^T [2 cout, cout], is only
 * ever the output gradient of BatchNorm1d + ReLU over the pre-norm rows X [E, 2 cout] (edge_conv_filter.py:36-38).  Instead of
 * storing it, reducing it (stin_colreduce_f32 DOT_BN_RELU) and rewriting it (stin_bn_act_bwd_f32) the product runs twice:
 *   stin_gemm_nt_bn_bwd_stats_f32: nothing stored; sums [2][Nc] floats = P | Q (P = sum d nhat, Q = sum d, d = dh [gamma nhat + beta > 0],
 *     nhat = (X - mean) rstd: the gradients of gamma | beta) through partial [groups][2][Nc] doubles (fixed-order fp64 fold);
 *   stin_gemm_nt_bn_bwd_apply_f32: dx [M, Nc] = rstd gamma (d - Q inv_n - nhat P inv_n) - stin_bn_act_bwd_f32's expression.
 * groups = stin_gemm_nt_bn_bwd_groups(M, Nc, K, precision); 0: not served (K not 64 or 128: the pair is kept to K <= 128, the plain product below takes every multiple of 64 up to 512; a pre-split precision flag,
 * STIN_NT_BNBWD=0) - keep the three-launch route.  Rows of A / W 16-byte aligned.  The accumulators equal stin_gemm_nt_f32's
 * bit for bit (same tiles, k order, MFMA order); the sums differ from the reduction kernel's only by fp64 summation order. */
/* The streaming-rows kernel behind them, as the plain product (mean == NULL) or with stin_gemm_nt_bn_f32's operand transform:
 * persistent blocks whose waves own 32-row tiles staged through wave-private LDS, the weight slice split once per block - for
 * M >> 1e5 rows with K = 64 .. 512 (a multiple of 64) and plain fp32 weights; STIN_E_UNSUPPORTED otherwise.  Bit-identical to the tiled
 * kernels (same k and MFMA order).  stin_gemm_nt_f32 (no bias / mask / residual) and stin_gemm_nt_bn_f32 route M >= 65 536 rows
 * here (STIN_NT_STREAM=0: never). */
int stin_gemm_nt_stream_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, int64_t M, int Nc, int K, float* C, int64_t ldc, int precision,
                            stin_stream_t stream);
int64_t stin_gemm_nt_bn_bwd_groups(int64_t M, int Nc, int K, int precision);
int stin_gemm_nt_bn_bwd_stats_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* X, int64_t ldx,
                                  const float* mean, const float* rstd, const float* gamma, const float* beta, int64_t M, int Nc,
                                  int K, int precision, double* partial, size_t partial_bytes, float* sums, stin_stream_t stream);
int stin_gemm_nt_bn_bwd_apply_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* X, int64_t ldx,
                                  const float* mean, const float* rstd, const float* gamma, const float* beta, const float* sums,
                                  float inv_n, int64_t M, int Nc, int K, float* dx, int64_t lddx, int precision,
                                  stin_stream_t stream);
int stin_scmn_pack_f32(const float* W1, const float* W2, const float* gamma1, const float* beta1, const float* gamma2,
                       const float* beta2, int cin, int h2, int cout, int trans_inv, float* wcat, float* wcatT, float* w2T,
                       float* gb1, float* gb2, stin_stream_t stream);
int stin_scmn_unpack_f32(const float* dwcat, int cin, int h2, int trans_inv, float* dW1, stin_stream_t stream);
int stin_bn_affine_res_fwd_f32(const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, const int32_t* rowptr, const float* res, int64_t ldres, int64_t N, int C,
                               int relu, float* y, int64_t ldy, stin_stream_t stream);
int stin_relu_mask_bwd_f32(const float* g, int64_t ldg, const float* y, int64_t ldy, const int32_t* rowptr, int64_t N, int C,
                           int relu, float* g_eff, float* g_in, stin_stream_t stream);
/* out[r] = [ skip[r, :cs] | coarse[trace[r], :cu] ], r < N: the decoder's torch.cat((skip, x[trace]), -1) with the unpool gather writing
 * straight into its half (models/singleconvmeshnet.py:146-150); trace values must lie in [0, rows of coarse) (validated when the
 * pooling map is built).  Backward needs no kernel of its own: the skip gradient is the left column block of the incoming gradient,
 * the coarse gradient stin_segment_sum_f32 over the right one. */
int stin_concat_unpool_f32(const float* skip, int64_t ld_skip, const float* coarse, int64_t ld_coarse, const int32_t* trace, int64_t N,
                           int cs, int cu, float* out, int64_t ldo, stin_stream_t stream);

/* ------------------------------------------------------- parameter-side helpers --
 * pack: the reference-layout EdgeConv parameters (first_filter.nn.0.{weight,bias} = W1 [H, 2Cin]
 * (or [H, Cin] for EdgeConvTransInv), first_filter.nn.2.weight = W2 [Cout, H], shortcut.{weight,bias})
 * -> the per-vertex GEMM operands  wcat [Yw, Cin] = [Wa-Wb ; Wb ; Ws] (trans_inv: [-W1 ; W1 ; Ws]),
 * bcat [Yw] = [b1 ; 0 ; bs], wcatT = wcat^T, w2T = W2^T; Yw = 2H (+ Cout).  The inner dimension may be zero-padded
 * from Cin to Cp (a multiple of 4) so that a 10-channel network input still takes the 16-byte GEMM paths.
 * trans_inv = STIN_TI_COMPACT (2, round 6; every entry point that takes trans_inv): the translation-invariant filter with ONLY
 * B = x W1^T materialised - wcat = [W1 ; Ws], bcat = [0 ; bs], Yw = H (+ Cout); A_i = b1 - B_i is formed by the edge stage
 * (stin_edge_relu_mean_fwd_ti_f32: mode 1's values up to one ulp of A) and the backward pass carries D = dB - dA in H columns
 * (stin_edge_relu_mean_bwd_mask_ti_f32) - half the first Linear's GEMM work in every direction.  fp32 rows with a saved-mask
 * width H; unpack then takes dW1 = rows [0, H) as they are and leaves db1 to the caller (the column sums of dA).
 * unpack: dwb [Yw, Cp + 1] (gemm_tn output over the padded rows: Cp weight-gradient columns, of which the first Cin are used, and
 *   the bias gradient in column Cp) -> dW1, db1, dWs, dbs; and dw2b [Cout, H+1] (optional) -> contiguous dW2 [Cout, H], db2 [Cout].
 *   dWa = the top H rows, dWb = bottom - top (one fp32 subtraction; trans_inv 1: dW1 = bottom - top); db1 / dbs / db2 may be NULL;
 *   outputs the mode does not have (db1 in COMPACT mode, dWs / dbs without a shortcut, dW2 / db2 without dw2b) are left alone.
 * pack, to the bit: Wa - Wb is one fp32 subtraction, -W1 a sign flip, the padding columns Cin .. Cp - 1 are +0, a NULL b1 / bs counts
 *   as zeros; w2s is written when it is passed (required with a fwd_split).  Storage STIN_GEMM_W_BF16 rounds each value to bf16
 *   (nearest even) into [rows][cols] bf16 at the START of the operand's buffer; the second half of the buffer is not written.
 *   The two pieces of a split precision are hi = rn16(s v), lo = rn16(s v - hi) with s = 64 for fp16 pieces and 1 for bf16 pieces
 *   (rn16: round to nearest even into the 16-bit format; the subtraction in fp32), in the k-group or fragment layout above.
 * (models/modules/edge_conv_filter.py:46-52, models/surfacetextureinpaintingnet.py:505-506)
 * norm_bwd_coef: k = -rstd^3 T1 inv_cnt, m = -rstd S0 inv_cnt for stin_norm_act_bwd_f32; evaluated in fp32 as
 *   k = ((-((rstd rstd) rstd)) T1) inv_cnt[b] and m = (-(rstd S0)) inv_cnt[b], operands [B, C], inv_cnt [B].
 * fwd_split / bwd_split (0, STIN_GEMM_F16X3 or STIN_GEMM_BF16X3, optionally | STIN_GEMM_W_FRAG): write the forward
 * operands (wcat, and a copy w2s [Cout, H] of W2) / the backward operands (wcatT, w2T) directly in the
 * STIN_GEMM_W_PRESPLIT form of that precision (each operand in fragment order where its shape allows, see W_FRAG).
 */
/* pack_many: the pack of EVERY block of a network in one launch.  `jobs_device` = n_jobs records in DEVICE memory (the
 * arguments of stin_edgeconv_pack_f32 as a struct; written once per model - the pointers do not change from step to step),
 * max_elems = max over the jobs of Yw * Cp + H * Cout.  The same argument rules as stin_edgeconv_pack_f32 apply per job
 * (not re-checked on the device).  A block op of stin_net_fwd then takes STIN_BLOCK_PACKED in fwd_split. */
typedef struct stin_pack_job {
    const float *W1, *b1, *Ws, *bs, *W2;
    float *wcat, *bcat, *wcatT, *w2T, *w2s;
    int Cin, Cp, H, Cout, has_shortcut, trans_inv, fwd_split, bwd_split;
} stin_pack_job_t;                                   /* 10 pointers + 8 ints = 112 bytes */
int stin_edgeconv_pack_many_f32(const stin_pack_job_t* jobs_device, int n_jobs, int64_t max_elems, stin_stream_t stream);
int stin_edgeconv_pack_f32(const float* W1, const float* b1, const float* Ws, const float* bs, const float* W2,
                           int Cin, int Cp, int H, int Cout, int has_shortcut, int trans_inv, float* wcat,
                           float* bcat, float* wcatT, float* w2T, float* w2s, int fwd_split, int bwd_split,
                           stin_stream_t stream);
int stin_edgeconv_unpack_grads_f32(const float* dwb, const float* dw2b, int Cin, int Cp, int H, int Cout,
                                   int has_shortcut, int trans_inv, float* dW1, float* db1, float* dWs, float* dbs,
                                   float* dW2, float* db2, stin_stream_t stream);
int stin_norm_bwd_coef_f32(const float* T1, const float* S0, const float* rstd, const float* inv_cnt, int B, int C,
                           float* k, float* m, stin_stream_t stream);
/* linspace-slice quirk of FastInstanceNorm (fastinstancenorm.py:53-82): m = -(rstd S0 + U) inv_cnt, where
 * U = stin_colreduce(STIN_RED_COEF_XC, coef = k) - the second coefficient of stin_norm_act_bwd_* when slices != graphs; evaluated
 * as (-((rstd S0) + U)) inv_cnt[b], every operation rounded on its own. */
int stin_norm_bwd_coef_m_quirk_f32(const float* S0, const float* U, const float* rstd, const float* inv_cnt, int B, int C,
                                   float* m, stin_stream_t stream);

/* ----------------------------------------------------------- train-step epilogues --
 * masked_l1_loss: the trainer's loss and its gradient in one pass
 * (trainers/inpainting3d_trainer.py:127-137): pred = mask > 0 ? out : color,
 * loss = mean |pred - color| * 0.99^mask (use_weight = trainer.use_mask_weighted_loss),
 * grad = dloss/dout.  fp64 block partials summed in a fixed order.  mask: int64 [N].
 *   To the bit: inv = fl(1 / (float)(N C)); on a row with mask > 0, d = out - color, grad = (sign(d) w) inv with w = powf(0.99f,
 *   (float)mask) or 1, and the element's term is (double)(|d| w); other rows give grad = +0 and term 0.  Element t belongs to block
 *   t / 256; a block adds its 256 terms in a pairwise tree (for s = 128, 64 .. 1: term[i] += term[i + s], i < s); the finaliser's
 *   thread i adds the block sums i, i + 256, i + 512 .. in that order, the 256 results go through the same tree, and
 *   loss = (float)(sum * (double)inv).  stin_total_variation_f32 folds its per-row sums the same way (row r in block r / 256).
 * adam: torch.optim.Adam(amsgrad) on ONE flat parameter/gradient/state buffer (the reference's
 * optimizer, experiments/3d_inpainting/config/...json:95-102), step = 1-based update count; the hyper-parameters are
 * doubles (python floats in torch) and the bias corrections 1 - beta^step are formed in double on the host, as torch does.
 *   To the bit: the scalars -(lr / (1 - beta1^step)), 1 - beta1, beta2, 1 - beta2, eps, weight_decay and sqrt(1 - beta2^step) are
 *   formed in double and cast once to fp32; per element, every operation rounded on its own: g' = g + wd p (only when wd != 0),
 *   m' = m + (1 - beta1) (g' - m), v' = beta2 v + ((1 - beta2) g') g', vh = amsgrad ? max(vmax, v') : v' (vmax' = vh),
 *   p' = p + (nss m') / (sqrt(vh) / bc2s + eps).  amsgrad = 0: vmax may be NULL and is not touched.  Bases that are all 16-byte
 *   aligned take a four-wide kernel, others a scalar one: same bits.
 */
size_t stin_masked_l1_workspace_bytes(int64_t N, int C);
int stin_masked_l1_loss_f32(const float* out, const float* color, const int64_t* mask, int64_t N, int C,
                            int use_weight, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                            stin_stream_t stream);
/* segmentation: the criterion of the segmentation trainer (trainers/segmentation_trainer.py:54, torch.nn.CrossEntropyLoss with
 * weight and ignore_index, reduction 'mean') and its confusion matrix (ConfusionMatrixDCM.add, :125-166 / :206-235) in ONE pass
 * over fp32 logits [., C] of row stride ld (STIN_SEG_MIN_CLASSES <= C <= STIN_SEG_MAX_CLASSES), int64 targets [N], optional fp32
 * class weights [C].  rows (optional, int64 [N]): target i reads logits row rows[i] of the M rows (the evaluation's
 * output[original_index_traces] without materialising it); without rows, M >= N and target i reads row i.
 *   loss (optional): loss[0] = sum w_y nll_i / sum w_y over the targets != ignore_index (fp32; fp64 block partials summed in a
 *     fixed order, the grid depends on N only: same bits on every run and device); den[0] = sum w_y (fp64, for the backward).
 *     Needs den and a workspace of stin_seg_ce_workspace_bytes(N).
 *   confusion (optional): int64 [C][C] += counts of (target, first arg-max of the row; NaN maximal), rows = target; a target
 *     equal to ignore_index that is a valid class IS counted (as the reference's matrix does).  Integer atomics: exact.
 * At least one of loss / confusion.  A target outside [0, C) other than ignore_index (any target outside [0, C) when loss is
 * NULL), or a rows[i] outside [0, M), adds to neither and sets *bad = 1 (bad may be NULL).
 * bwd: dlogits[i, :] = g w_y (softmax(z_i) - onehot(y_i)) / den with g = grad_loss[0] and den from the forward, both read on
 * the device; rows whose target is ignored or invalid get zeros.  No row gather. */
#define STIN_SEG_MIN_CLASSES 2
#define STIN_SEG_MAX_CLASSES 128
size_t stin_seg_ce_workspace_bytes(int64_t N);
int stin_seg_ce_fwd_f32(const float* logits, int64_t ld, int64_t M, const int64_t* rows, const int64_t* target, int64_t N, int C,
                        const float* weight, int64_t ignore_index, float* loss, double* den, int64_t* confusion, int32_t* bad,
                        void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_seg_ce_bwd_f32(const float* logits, int64_t ld, const int64_t* target, int64_t N, int C, const float* weight,
                        int64_t ignore_index, const float* grad_loss, const double* den, float* dlogits, int64_t ldd,
                        stin_stream_t stream);
/* graph total variation, the per-step smoothness metric of the trainer (utils/metrics/graph_metrics.py:34-38,
 * trainers/inpainting3d_trainer.py:254-263): out[0] = sum_e sum_c |x[src_e, c] - x[dst_e, c]| / (N * C) over the
 * destination CSR the forward pass has built (rowptr_dst / col_dst), fp64 partial sums in a fixed order: per destination row an
 * fp64 sum over its CSR entries, in order, of the fp32 channel sum (c = 0 .. C - 1, from 0) of |x[col[e], c] - x[row, c]|; the rows
 * are folded as the loss folds its elements, with inv = fl(1 / fl((float)N (float)C)). */
size_t stin_total_variation_workspace_bytes(int64_t N);
int stin_total_variation_f32(const float* x, int64_t ldx, const int32_t* rowptr_dst, const int32_t* col_dst, int64_t N, int C,
                             float* out, void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* graph Laplace of the same metrics module (utils/metrics/graph_metrics.py:6-16, GraphLaplaceOperator: propagate [1 | x] with
 * aggr = 'add', then prop[:, 1:] - prop[:, 0:1] * x): out[i, c] = sum_{j in N(i)} x[j, c] - deg_i x[i, c] over the destination CSR,
 * fp32 adds in edge order - the numbers of the reference's composition, bit for bit: s - fl((float)deg_i x[i, c]), s summed from 0. */
int stin_graph_laplace_f32(const float* x, int64_t ldx, const int32_t* rowptr_dst, const int32_t* col_dst, int64_t N, int C,
                           float* out, int64_t ldo, stin_stream_t stream);
/* the trainer's seven per-step metrics in one call (trainers/inpainting3d_trainer.py:254-271: loss, l1, mse, graph_tv, graph_lap_var,
 * psnr, psnr_mask_only), written as ONE row of 8 floats into a caller-owned device table - nothing is read back, so a training
 * loop pays no queue drain per metric.  P = composite ? where(mask > 0, out, color) : out, G = color, n = N * C:
 *   row_out[0] loss            sum |P - G| (use_weight ? 0.99^mask : 1) / n; with loss != NULL: loss[0] (computed elsewhere) copied
 *   row_out[1] l1              sum |P - G| / n
 *   row_out[2] mse             sum (P - G)^2 / n
 *   row_out[3] graph_tv        sum_e sum_c |P[src_e, c] - P[dst_e, c]| / n
 *   row_out[4] graph_lap_var   population variance over the vertices of L_i = sum_{j -> i} g_j - deg_i g_i, g = 0.299 R + 0.587 G +
 *                              0.114 B of P; L_i as stin_graph_laplace_f32 forms it (fp32 adds in CSR = edge order).  C == 1: NaN
 *   row_out[5] psnr            -10 log10(mse / data_range^2 + 1e-8)
 *   row_out[6] psnr_mask_only  the same over the rows with mask > 0; NaN when there are none (as the reference)
 *   row_out[7] number of rows with mask > 0 (exact: N <= 2^24 is required)
 * out [N, C] fp32 with leading dimension ldo, color [N, C] contiguous, mask int64 [N], C = 1 or 3 (STIN_E_SIZE otherwise);
 * rowptr_dst / col_dst = the destination CSR of level 0.  perm (optional, int32 [N]): CSR row r is the caller's row perm[r] (a plan
 * whose vertices were renumbered by locality: GraphPlan.order0); NULL = identity.  fp32 terms, fp64 block partials folded in a
 * fixed order by the finaliser (divisions, log10 and variance in double): same bits on every run; no float atomics.
 * layout: STIN_METRICS_ONE_PASS (2 launches, every neighbour's P row rebuilt from out / color / mask: 32 bytes per edge) or
 * STIN_METRICS_STAGED (3 launches, P rows + gray staged as float4 in the workspace in CSR row order: 16 bytes per edge); the
 * two give identical bits.  Workspace: stin_inpaint_metrics_workspace_bytes(N) for either layout. */
#define STIN_METRICS_ONE_PASS 0
#define STIN_METRICS_STAGED 1
size_t stin_inpaint_metrics_workspace_bytes(int64_t N);
int stin_inpaint_metrics_f32(const float* out, int64_t ldo, const float* color, const int64_t* mask, const int32_t* rowptr_dst,
                             const int32_t* col_dst, const int32_t* perm, int64_t N, int C, int composite, int use_weight,
                             float data_range, const float* loss, int layout, float* row_out, void* workspace,
                             size_t workspace_bytes, stin_stream_t stream);
int stin_adam_f32(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, int amsgrad, stin_stream_t stream);

/* GEMM + first stage of the instance-norm statistics of its output (the all-columns NT kernel's blocks own whole rows):
 * colstats [groups][2][Nc] doubles = per 64-row group the column sums of the stored values and of their squares;
 * groups = stin_gemm_nt_colstats_groups(M, Nc, K, precision) (0: shape / precision not supported - Nc = 128 / 256 in
 * fragment order only).  stin_moments_final_f32 turns them into mean / rstd of ONE instance (inv_cnt[0] = 1 / M).
 * Replaces GEMM2 + stin_colreduce_f32(MOMENTS) of a single-graph block (fastinstancenorm.py:44-98 on the conv output). */
int64_t stin_gemm_nt_colstats_groups(int64_t M, int Nc, int K, int precision);
int stin_gemm_nt_colstats_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                              const float* row_mask, int64_t ld_mask, const float* residual, int64_t ld_res, int64_t M,
                              int Nc, int K, float* C, int64_t ldc, int precision, double* colstats, size_t colstats_bytes,
                              stin_stream_t stream);
int stin_moments_final_f32(const double* partial, int64_t groups, int C, const float* inv_cnt, float eps, float* mean,
                           float* rstd, stin_stream_t stream);
/* Round 5: the fold of per-row-group statistics partials INSIDE the elementwise launch (single graph, fp32 rows, C % 32 == 0,
 * 16-byte rows): every workgroup folds the partials of its own 32 columns with the arithmetic of stin_moments_final_f32 /
 * stin_norm_coef_from_partials_f32 and then runs stin_norm_act_res_fwd_f32 / stin_norm_act_bwd_f32's expression on its rows:
 * bit-identical to the two-launch route, one launch less on the critical path of a block.  Replaces the same reference lines as
 * those entry points (models/modules/fastinstancenorm.py:44-49 + the ELU / residual of surfacetextureinpaintingnet.py:507-521).
 * stin_norm_fold_rows: rows per workgroup the form would use for (N, C, groups), or 0 when it does not apply / does not pay (the
 * grid would read more fold bytes than half its elementwise traffic; STIN_NORM_FOLD=0).  The two launches return
 * STIN_E_UNSUPPORTED - before anything is enqueued - when the form does not apply: the caller then takes the two-launch route.
 * fwd: partial [groups][2][C] (sum, sum of squares) -> mean, rstd [C] written; y = ELU((x - mean) rstd) (+ res).
 * bwd: partial [groups][2][C] (sum of dy xc, sum of dy) with mean, rstd [C] given -> dx = rstd dy + k xc + m. */
int stin_norm_fold_rows(int64_t N, int C, int64_t groups);
int stin_norm_act_res_fwd_fold_f32(const double* partial, int64_t groups, const float* x, int64_t ldx, const float* res,
                                   int64_t ldres, const float* inv_cnt, float eps, int64_t N, int C, float* mean, float* rstd,
                                   float* y, int64_t ldy, stin_stream_t stream);
/* the forward form with the residual read through a row map (y[r] += res[row_map[r]]; res, row_map not NULL) */
int stin_norm_act_res_fwd_fold_map_f32(const double* partial, int64_t groups, const float* x, int64_t ldx, const float* res,
                                       int64_t ldres, const int32_t* row_map, const float* inv_cnt, float eps, int64_t N, int C,
                                       float* mean, float* rstd, float* y, int64_t ldy, stin_stream_t stream);
int stin_norm_act_bwd_fold_f32(const double* partial, int64_t groups, const float* x, int64_t ldx, const float* gout, int64_t ldg,
                               const float* mean, const float* rstd, const float* inv_cnt, int64_t N, int C, float* dx,
                               int64_t lddx, stin_stream_t stream);

/* --------------------------------------------------- bf16-storage variants of the path --
 * Same semantics, argument order and reference call sites as the *_f32 entry points above, on bf16 rows
 * (stin_bf16_t, see the typedef).  What stays fp32: instance-norm statistics (fp64 accumulation), inv_deg / w_src /
 * row_scale, the weight operand W and bias of the GEMMs, the weight gradients dW and every index plan.
 * Vector kernels only: C % 4 == 0, ld % 4 == 0, 8-byte aligned rows, else STIN_E_UNSUPPORTED; the edge stage
 * needs the saved ReLU mask (H in {128, 256, 512, 1024, 2048}) in backward.  With 16-byte aligned rows (ld % 8 == 0)
 * the edge stage gives every lane 8 channels (the same 16 bytes per lane and request as the fp32 kernels); the mask
 * kernels REQUIRE that alignment (STIN_E_ALIGN otherwise) because the lane geometry fixes the bit order inside a mask
 * slot: a bf16 mask is only meaningful to the bf16 backward kernels, an fp32 mask to the fp32 ones.
 * gemm_nt_bf16: A, row_mask, residual bf16; W, bias fp32 (W is rounded to bf16 while staged); one
 *   v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulate, bias/mask/residual added in fp32, one rounding;
 *   C is bf16 (c_is_f32 = 0) or fp32 (c_is_f32 = 1: the network's final [N, 3] output); OR-ing STIN_GEMM_W_BF16 into
 *   c_is_f32 declares W as a bf16 [Nc][K] operand (written by stin_edgeconv_pack_f32 in that mode).
 * gemm_tn_bf16: G, X, row_weight bf16 -> fp32 dW; workspace = stin_gemm_tn_workspace_bytes.
 */
int stin_segment_sum_bf16(const stin_bf16_t* src, int64_t ld_src, const int32_t* rowptr, const int32_t* col,
                          int64_t n_rows, int C, int mean, stin_bf16_t* out, int64_t ld_out, stin_stream_t stream);
int stin_edge_relu_mean_fwd_bf16(const stin_bf16_t* A, int64_t lda, const stin_bf16_t* B, int64_t ldb,
                                 const int32_t* rowptr, const int32_t* col, int64_t N, int H, stin_bf16_t* out,
                                 int64_t ldo, int indicator, uint32_t* mask, stin_stream_t stream);
int stin_edge_relu_mean_bwd_dst_mask_bf16(const stin_bf16_t* G, int64_t ldg, const uint32_t* mask,
                                          const int32_t* rowptr, int64_t N, int H, stin_bf16_t* dA, int64_t ldda,
                                          stin_stream_t stream);
int stin_edge_relu_mean_bwd_src_mask_bf16(const stin_bf16_t* G, int64_t ldg, const float* w_src, const uint32_t* mask,
                                          const int32_t* rowptr_src, const int32_t* col_src, const int32_t* xslot,
                                          int64_t N, int H, stin_bf16_t* dB, int64_t lddb, stin_stream_t stream);
int stin_edge_relu_mean_bwd_mask_bf16(const stin_bf16_t* G, int64_t ldg, const uint32_t* mask, const int32_t* rowptr_dst,
                                      const float* w_src, const int32_t* rowptr_src, const int32_t* col_src,
                                      const int32_t* xslot, int64_t N, int H, stin_bf16_t* dA, int64_t ldda,
                                      stin_bf16_t* dB, int64_t lddb, const stin_bf16_t* copy_src, int64_t ld_copy_src,
                                      stin_bf16_t* copy_dst, int64_t ld_copy_dst, int C_copy, stin_stream_t stream);
int stin_pool_max_fwd_bf16(const stin_bf16_t* x, int64_t ldx, const int32_t* rowptr, const int32_t* col,
                           int64_t n_coarse, int C, stin_bf16_t* out, int64_t ldo, int32_t* arg, stin_stream_t stream);
int stin_pool_max_bwd_bf16(const stin_bf16_t* g, int64_t ldg, const int32_t* arg, const int32_t* trace,
                           int64_t n_fine, int C, stin_bf16_t* gx, int64_t ldgx, stin_stream_t stream);
int stin_gather_rows_bf16(const stin_bf16_t* src, int64_t ld_src, const int32_t* idx, const float* row_scale,
                          int64_t n_out, int C, stin_bf16_t* out, int64_t ldo, stin_stream_t stream);
int stin_colreduce_bf16(int mode, const stin_bf16_t* x, int64_t ldx, const stin_bf16_t* gout, int64_t ldg, int64_t N,
                        int C, const int32_t* ptr, int B, const int32_t* gid, const int32_t* sid, const float* mean,
                        const float* rstd, const float* coef, int post, const float* inv_cnt, float eps, float* out0,
                        float* out1, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_norm_act_res_fwd_bf16(const stin_bf16_t* x, int64_t ldx, const float* mean, const float* rstd,
                               const int32_t* gid, const stin_bf16_t* res, int64_t ldres, int64_t N, int C, int act,
                               stin_bf16_t* y, int64_t ldy, stin_stream_t stream);
int stin_norm_act_bwd_bf16(const stin_bf16_t* x, int64_t ldx, const stin_bf16_t* gout, int64_t ldg, const float* mean,
                           const float* rstd, const float* a, const float* k, const float* m, const int32_t* gid,
                           const int32_t* sid, int64_t N, int C, int act, stin_bf16_t* dx, int64_t lddx,
                           stin_stream_t stream);
int stin_gemm_nt_bf16(const stin_bf16_t* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                      const stin_bf16_t* row_mask, int64_t ld_mask, const stin_bf16_t* residual, int64_t ld_res,
                      int64_t M, int Nc, int K, void* C, int64_t ldc, int c_is_f32, stin_stream_t stream);
int stin_gemm_tn_bf16(const stin_bf16_t* G, int64_t ldg, const stin_bf16_t* X, int64_t ldx, int64_t M, int Nc, int K,
                      int ones_column, const stin_bf16_t* row_weight, int64_t ld_weight, float* dW, int64_t lddw,
                      void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* (bf16 activation rows: stin_gemm_tn_wb_f32 and the stin_linear_tanh_* pair above) */
int stin_gemm_tn_wb_bf16(const stin_bf16_t* G, int64_t ldg, const stin_bf16_t* X, int64_t ldx, int64_t M, int Nc, int K,
                         const stin_bf16_t* row_weight, int64_t ld_weight, float* dW, int64_t lddw, float* db,
                         void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_linear_tanh_fwd_bf16(const stin_bf16_t* x, int64_t ldx, const float* W, const float* b, int64_t N, int K, int Nc,
                              float* y, stin_stream_t stream);
int stin_linear_tanh_bwd_bf16(const float* g, const float* y, const stin_bf16_t* x, int64_t ldx, const float* W, int64_t N, int K,
                              int Nc, stin_bf16_t* dx, int64_t lddx, float* dW, float* db, void* workspace,
                              size_t workspace_bytes, stin_stream_t stream);

/* ------------------------------------------------------ whole-block launch sequences --
 * The graph part of the network - or any part of it, down to ONE block - in one call per direction: every fused
 * EdgeConv + instance-norm block and the pool / unpool steps between them, in network order
 * (models/surfacetextureinpaintingnet.py:404-455: input blocks, `for` over the encoder levels - `_pooling` :384-386 then a
 * block -, the bottleneck blocks, `for` over the decoder levels - `_unpooling` :390-391 then a block -, the output blocks).
 * stin_net_fwd / stin_net_bwd only ENQUEUE the entry points above with the per-op pointers of a HOST op array, so the
 * arithmetic is identical to calling them one by one (bit-identical to the per-kernel calls) - what they remove is host
 * time: ~9 / ~16 foreign calls per block and direction and one autograd node per op (the launch-bound sizes: 20 k-vertex
 * crops, the 8-crop batches).  storage: 0 = fp32 rows, 1 = bf16 rows (x, Y, hE, agg, out, g, dx).
 *   op i reads `x` (ops[0]: the input padded to Cp channels; else ops[i - 1].out) and writes `out`;
 *   bwd walks the ops in reverse: the gradient of op i's output is ops[i + 1].dx (the call's `g` for the last op), op i writes
 *   its input gradient to `dx` (NULL for ops[0] when the input needs none).
 *   STIN_OP_BLOCK: one GraphResnetBlock (EdgeConv(mean) -> instance norm -> ELU -> + residual,
 *     models/surfacetextureinpaintingnet.py:507-521) over n_out = n_in = N rows, in the order of the fused block:
 *     pack -> Y GEMM -> edge stage -> agg GEMM -> moments -> norm / ELU / residual; and its backward.
 *     Precondition (callers use the individual entry points otherwise): H supports the saved ReLU mask.
 *     fwd: x [N, Cp] (input zero-padded to Cp columns), reference-layout parameters W1 .. bs, destination CSR, norm groups
 *        (ptr_sum / gid may be NULL for one graph; inv_cnt [B]); writes what backward needs - wcatT [Cp, Yw], w2T [H, Cout]
 *        (fp32 or pre-split per bwd_split), Y [N, Yw], hE [N, H + pad] (column H = [deg > 0]), mask [E * H / 32],
 *        agg [N, Cout], mean / rstd [B, Cout] - and out [N, Cout].  Yw = 2 H (+ Cout with a shortcut); H (+ Cout) when
 *        trans_inv == STIN_TI_COMPACT.  fwd_ws: stin_edgeconv_block_fwd_workspace_bytes.
 *        mask may be NULL for a forward nobody differentiates (the reference's validation loop,
 *        trainers/inpainting3d_trainer.py:204-263: model(data) under torch.no_grad()): same kernels, same rows bit for
 *        bit, the E * H / 8 mask bytes per block are not written.
 *     slice_quirk != 0 (fwd) / sid != NULL (bwd): the reference's linspace-slice statistics for batches of unequal graphs
 *        (fastinstancenorm.py:53-82) - sums over the `ptr_sum` slices, centring through gid: two-pass statistics forward,
 *        the extra COEF_XC reduction backward; ptr_true are the true per-graph row ranges.
 *     bwd: dx [N, Cp]; parameter gradients dW1 .. dbs in the reference layout (NULL where the parameter does not exist).
 *        All temporaries live in bwd_ws (stin_edgeconv_block_bwd_workspace_bytes).
 *        Side stream: the weight-gradient products and their finalize launch are off the dx <- g critical path.  With
 *        use_side != 0 and a `wgrad_stream` other than `stream` they are enqueued there behind ev_dy (recorded on `stream`
 *        when dY is complete) and followed by ev_done (recorded on wgrad_stream).  Nothing joins the two streams: the
 *        CALLER must order any reader of dW1 .. dbs after ev_done and keep bwd_ws, x, hE and g alive until then.  Without
 *        use_side a non-NULL ev_done is recorded on `stream` behind the block's last gradient write.  The events are
 *        caller-owned hipEvent_t.
 *     y_from_src != 0 (forward, fp32 rows, a shortcut block in the wide layout right behind the STIN_OP_UNPOOL op whose output
 *        it reads): x_up[v] = x_c[trace[v]] makes every row of Y = x_up Wcat^T + bcat a copy of a row of Yc = x_c Wcat^T + bcat
 *        (a row of an NT product depends on no other row), so the product runs over the unpool op's n_in COARSE rows - Y is
 *        [n_in, Yw] - and the edge stage and the residual read Y through the trace (stin_edge_relu_mean_fwd_map_f32,
 *        stin_norm_act_res_fwd*_map_f32).  hE, mask, agg, mean / rstd and out have the same bits as with 0 (the behaviour of every
 *        earlier caller); backward reads x and never Y.  The unpool op's gather still runs when it has an `out`
 *        (x is kept for backward); with out == NULL - a forward nobody differentiates, or x_from_src - it is skipped and the
 *        block's x is unused.
 *        A flag on a block where these conditions do not hold is STIN_E_UNSUPPORTED (its Y is sized for the coarse rows).
 *     x_from_src != 0 (both directions, only together with y_from_src and where stin_edgeconv_wgrad_map_supported says 1): the
 *        block's x is never materialised.  The one backward reader of x, the packed weight-gradient product dY^T [x | 1], reads
 *        row v at x_c[trace[v]] through the unpool op in front (stin_edgeconv_wgrad_map: the same slabs bit for bit), so that op
 *        takes out == NULL in a training forward as well, the block's x is NULL in both calls and the unpooled rows are neither
 *        written nor kept.  0 = the behaviour of every earlier caller.
 *     g_in_dy != 0 (backward, fp32 rows, a shortcut block with its own bwd_ws): a PERMISSION for stin_net_bwd to let the op
 *        behind this block write its input gradient - this block's g - straight into the shortcut columns of this block's
 *        dY = [dA | dB | g] inside bwd_ws (leading dimension Yw) instead of into its `dx`, which is then not written; the block
 *        reads g there and the copy of g into dY goes away.  Taken where stin_net_bwd_g_in_dy says 1 (same rows and width, no
 *        channel padding in between, 16-byte aligned columns), ignored elsewhere; never for ops[0].dx.  Same values, same
 *        order of every sum: bit-identical gradients.  0 = the behaviour of every earlier caller.
 *   STIN_OP_POOL_MAX: x [n_in, Cout] -> out [n_out, Cout], arg [n_out, Cout]; rowptr_dst / col_dst = the children CSR, trace = the
 *     fine -> coarse map (backward).  STIN_OP_UNPOOL: out[v] = x[trace[v]] (n_out fine rows); backward = the segment sum
 *     over the children CSR. */
#define STIN_TI_COMPACT 2         /* value of `trans_inv`: translation-invariant, compact layout (see the pack documentation above) */
#define STIN_BLOCK_PACKED 0x800   /* OR-ed into a block op's fwd_split: the caller has already run the pack (e.g.
                                     stin_edgeconv_pack_many_f32) with the same modes into wcatT / w2T and into THIS fwd_ws
                                     at the offsets stin_edgeconv_block_fwd_pack_offsets reports - the call then skips it    */
size_t stin_edgeconv_block_fwd_workspace_bytes(int Cin, int Cp, int H, int Cout, int has_shortcut, int B);
/* byte offsets of wcat [Yw, Cp], w2s [Cout, H] and bcat [Yw] from the workspace pointer rounded UP to 256 bytes */
int stin_edgeconv_block_fwd_pack_offsets(int Cp, int H, int Cout, int has_shortcut, size_t* off_wcat, size_t* off_w2s,
                                         size_t* off_bcat);
size_t stin_edgeconv_block_bwd_workspace_bytes(int64_t N, int Cp, int H, int Cout, int has_shortcut, int B, int storage);
#define STIN_OP_BLOCK 0
#define STIN_OP_POOL_MAX 1
#define STIN_OP_UNPOOL 2
typedef struct stin_net_op {
    int32_t kind, Cin, Cp, H, Cout, has_shortcut, trans_inv, prec_fwd, fwd_split, bwd_split, B, slice_quirk, use_side, y_from_src,
        x_from_src, g_in_dy;
    float eps;
    int32_t reserved3;
    int64_t n_out, n_in, ldx, ldo, lddx, ldy, ldh;
    uint64_t fwd_ws_bytes, bwd_ws_bytes;
    const void* x;
    void* out;
    void* dx;
    const float *W1, *b1, *W2, *b2, *Ws, *bs;
    float *wcatT, *w2T;
    void* fwd_ws;
    const int32_t *rowptr_dst, *col_dst, *rowptr_src, *col_src, *xslot;
    const float* w_src;
    const int32_t *ptr_sum, *ptr_true, *gid, *sid;
    const float* inv_cnt;
    void *Y, *hE;
    uint32_t* mask;
    void* agg;
    float *mean, *rstd;
    int32_t* arg;
    const int32_t* trace;
    float *dW1, *db1, *dW2, *db2, *dWs, *dbs;
    void* bwd_ws;
    stin_event_t ev_dy, ev_done;
    stin_event_t ev_edge0, ev_edge1;  /* optional (block ops): recorded on `stream` right before / after the block's edge-stage launch
                                         (forward: stin_edge_relu_mean_fwd_*, backward: stin_edge_relu_mean_bwd_mask_*) - a timing
                                         bracket inside the call (bench.py's live roofline figure); NULL = none */
} stin_net_op_t;                      /* 16 int32 + float + int32 + 7 int64 + 2 uint64 + 42 pointers = 480 bytes */
int stin_net_fwd(int storage, const stin_net_op_t* ops, int n_ops, stin_stream_t stream);
int stin_net_bwd(int storage, const stin_net_op_t* ops, int n_ops, const void* g, int64_t ldg, int prec_bwd, stin_stream_t stream,
                 stin_stream_t wgrad_stream);
/* 1 when stin_net_bwd writes ops[i].dx into the dY of ops[i - 1] (g_in_dy above), else 0.  Host only: reads the records, no pointer. */
int stin_net_bwd_g_in_dy(int storage, const stin_net_op_t* ops, int n_ops, int i);

/* All weight gradients of one fused block in two launches (round 3): BOTH transposed products
 *   dW2 | db2 = dagg^T [hE[:, :H] | hE[:, H]]        (second Linear; db2 weighted by the [deg > 0] column of hE)
 *   [dW1 ; dWs | db1 ; dbs] = dY^T [x | 1]           (first Linear + shortcut in the packed operand layout)
 * as ONE grid of the producer / consumer TN kernel (csrc/stin_wgrad.hip) where both have 128 x 128 tiles and 16-byte rows
 * (otherwise one TN launch each), then ONE kernel that sums the partial slabs in the fixed order of the stand-alone
 * stin_gemm_tn_* reduction and writes the reference-layout gradients directly - bit-identical to
 * stin_gemm_tn_f32 x 2 + stin_edgeconv_unpack_grads_f32, which it replaces inside a block op's backward.
 * Replaces the autograd backward of the two nn.Linear modules of edge_conv_filter.py:46-57 and of the shortcut Linear
 * (models/surfacetextureinpaintingnet.py:489-492) for the gradients w.r.t. their parameters.
 * storage: 0 = fp32 rows, 1 = bf16 rows (dagg, hE, dY, x); hE has at least H + 1 columns; precision as stin_gemm_tn_f32. */
size_t stin_edgeconv_wgrad_workspace_bytes(int64_t N, int Cp, int H, int Cout, int has_shortcut);
int stin_edgeconv_wgrad(int storage, const void* dagg, int64_t ld_dagg, const void* hE, int64_t ldh, const void* dY,
                        int64_t ldy, const void* x, int64_t ldx, int64_t N, int Cin, int Cp, int H, int Cout,
                        int has_shortcut, int trans_inv, int precision, float* dW1, float* db1, float* dW2, float* db2,
                        float* dWs, float* dbs, void* workspace, size_t workspace_bytes, stin_stream_t stream);
/* ... for every trans_inv mode.  trans_inv == STIN_TI_COMPACT: dY = [D | g] is [N, H (+ Cout)], dW1 = the first H rows of the packed
 * product as they are, and db1 = the sum of the ti_rows rows of ti_colsum [ti_rows][H] (stin_edge_relu_mean_bwd_mask_ti_f32's column
 * partials of dA), folded by the same finalize launch; other modes ignore the two arguments. */
int stin_edgeconv_wgrad_ti(int storage, const void* dagg, int64_t ld_dagg, const void* hE, int64_t ldh, const void* dY,
                           int64_t ldy, const void* x, int64_t ldx, int64_t N, int Cin, int Cp, int H, int Cout,
                           int has_shortcut, int trans_inv, int precision, float* dW1, float* db1, float* dW2, float* db2,
                           float* dWs, float* dbs, const float* ti_colsum, int64_t ti_rows, void* workspace,
                           size_t workspace_bytes, stin_stream_t stream);
/* stin_edgeconv_wgrad with the rows of x read through a map: x is [x_rows, ldx] and row m of the packed product's operand is
 * x[x_row_map[m]] (x_row_map [N], 16-byte aligned, values in [0, x_rows)) - the unpooled rows x_up = x_c[trace] of a decoder block
 * without the gather that writes them.  Only the row addresses of the producer / consumer kernel's X loads change: the same slabs,
 * the same gradients bit for bit as stin_edgeconv_wgrad on x[x_row_map].  fp32 rows, not the compact layout, and only where
 * stin_edgeconv_wgrad_map_supported (host only; STIN_TN_WS honoured) says 1 - the shapes whose packed product runs on that kernel;
 * STIN_E_UNSUPPORTED elsewhere (those shapes keep the gather).  x_row_map == NULL: stin_edgeconv_wgrad. */
int stin_edgeconv_wgrad_map_supported(int64_t N, int Cp, int H, int Cout, int has_shortcut, int precision);
int stin_edgeconv_wgrad_map(int storage, const void* dagg, int64_t ld_dagg, const void* hE, int64_t ldh, const void* dY,
                            int64_t ldy, const void* x, int64_t ldx, int64_t N, int Cin, int Cp, int H, int Cout,
                            int has_shortcut, int trans_inv, int precision, float* dW1, float* db1, float* dW2, float* db2,
                            float* dWs, float* dbs, const int32_t* x_row_map, int64_t x_rows, void* workspace,
                            size_t workspace_bytes, stin_stream_t stream);

/* ------------------------------------------------- offline preprocessing on the GPU --
 * The dilated-edge walk of preprocessing/graph_dilation.py:85-137 (`compute_dilated_edges`), one thread per
 * directed adjacency entry (centre c = row_of[e], one-hop h = col[e]) of the COALESCED adjacency CSR
 * (`rowptr`/`col`: neighbours of every vertex sorted by id, duplicates removed - pyg.utils.coalesce, :53-56):
 * from h the walker repeatedly moves to the neighbour whose direction, pushed through the reference's
 * plane_projection (:27-28) with the current vertex normal, has the largest cosine with the running direction
 * (candidates adjacent to c or equal to the previous vertex excluded, similarity must be >= 0, the last maximum in
 * adjacency order wins, :104-118) and records the vertex reached after d hops for every requested d.
 *   dilations: HOST array of n_dil ascending ints in [2, 63];
 *   out[i * E + e] = vertex reached for dilations[i] (the edge is [out, c]), -1 where the walk ended earlier.
 * pos / nrm: [N, 3] row-major in the arithmetic type of the call (the pipeline passes float64,
 * preprocessing/graph_level_generation.py:463-465; the reference's dil_test float32).  Bit-identical to
 * oracle/dilation_oracle.py (fixed operation order, IEEE divide / sqrt, no FMA).
 */
int stin_dilated_walk_f32(const int32_t* rowptr, const int32_t* col, const int32_t* row_of, const float* pos,
                          const float* nrm, int64_t N, int64_t E, const int32_t* dilations, int n_dil, int32_t* out,
                          stin_stream_t stream);
int stin_dilated_walk_f64(const int32_t* rowptr, const int32_t* col, const int32_t* row_of, const double* pos,
                          const double* nrm, int64_t N, int64_t E, const int32_t* dilations, int n_dil, int32_t* out,
                          stin_stream_t stream);

/* Voxel (Rossignac) vertex clustering, preprocessing/graph_level_generation.py:193-244 (`vertex_clustering`):
 *   bins = coords // voxel (numpy's floor division, fp64), coarse ids = np.unique(bins, axis=0)'s lexicographic bin order,
 *   trace[v] = coarse id of vertex v, new_coords[c] = fp64 mean of the members' coordinates (in vertex order) as fp32.
 * coords [N, 3] fp64 row-major; trace [N] int64; new_coords [N, 3] fp32 (the first Nc rows are written);
 * state: 5 x int64 DEVICE words written by the call - state[3] != 0: unsupported input (a non-finite coordinate or more
 * than 2^21 bins along an axis), state[4] = Nc.  Stable radix sort of one 63-bit key per vertex + scan: deterministic.
 * stin_coalesce_pairs_i64 = pyg.utils.coalesce on (a[e], b[e]) pairs (graph_level_generation.py:236-241 on the coarse edges,
 * graph_dilation.py:53-56): optionally mapped through map[map_n] first (the trace), self loops dropped when drop_loops, sorted by
 * (a, b), duplicates removed; values in [0, n); out_a / out_b [E] int64 (the first state[4] entries are written);
 * state[3] != 0: an index was outside [0, n), or - with a map - a raw endpoint outside [0, map_n) (checked BEFORE map[] is read:
 * the torch formulation trace[edge_index[0]] this replaces raises there). */
size_t stin_voxel_cluster_workspace_bytes(int64_t N);
int stin_voxel_cluster_f64(const double* coords, int64_t N, double voxel, int64_t* trace, float* new_coords, int64_t* state,
                           void* workspace, size_t workspace_bytes, stin_stream_t stream);
size_t stin_coalesce_workspace_bytes(int64_t E);
int stin_coalesce_pairs_i64(const int64_t* a, const int64_t* b, const int64_t* map, int64_t map_n, int64_t E, int64_t n, int drop_loops,
                            int64_t* out_a, int64_t* out_b, int64_t* state, void* workspace, size_t workspace_bytes,
                            stin_stream_t stream);

/* Mesh clustering: voxel clustering that keeps the result a TRIANGLE MESH, so that QEM levels can follow it - the step the
 * reference shells out to vcglib's trimesh_clustering for (graph_level_generation.py, a --qem level that is no digit string).
 * preprocessing.cluster_mesh drives the two entry points below.  A contract of this project's own, restated in numpy by
 * tests/_meshcluster_oracle.py (bit-exact parity); it is NOT pinned against vcglib, and differs from it on purpose: the grid origin
 * is 0 (as in the reference's own python vertex_clustering; vcglib anchors the grid on an inflated bounding box) and a cell's
 * position is the unweighted mean of its members (vcglib weights by face corners).  Everything is fp64.
 *   faces in    range-checked; faces that repeat a vertex are dropped at once (stin_qem_remap_faces_i64 with parent == NULL).
 *   cells       bin = coords // cell_size per axis (numpy's floor division: the floor_div of stin_voxel_cluster_f64); cluster ids =
 *               the ranks of the bin triples in lexicographic order (np.unique(bins, axis=0)); ALL N vertices are clustered,
 *               referenced by a face or not: trace and Nc are those of stin_voxel_cluster_f64 bit for bit.
 *   positions   per cluster the members' coordinates summed in ascending vertex id from 0.0, divided by the count (as a double)
 *               with one IEEE division: stin_voxel_cluster_f64's value before its cast to fp32.
 *   faces out   image = trace[face], corner order kept; images with two equal corners are dropped; among images with the same
 *               vertex SET only the one of the lowest input face id survives, with that face's orientation (a fold makes most such
 *               duplicates opposite in orientation); survivors keep their relative input order.
 * Clusters that no surviving face references stay (they count in Nc and have no edges).  The result may be non-manifold (an edge
 * with more than two faces).
 * stin_voxel_cluster_mean_f64: stin_voxel_cluster_f64 with new_coords [N, 3] fp64 (the first Nc rows are written) - same state
 *     words, same workspace (stin_voxel_cluster_workspace_bytes).
 * stin_face_cluster_i64: faces [F, 3] int64, trace [N] int64 with values in [0, Nc) -> out_faces [F, 3] int64 (the first state[4]
 *     rows are written).  One kernel forms image, degenerate flag and the key of the sorted triple (three 21-bit ids), a stable
 *     radix sort of (key, face id), head flags by face id, a scan and a compaction follow - all inside the workspace
 *     (>= stin_face_cluster_workspace_bytes(F)); nothing allocates or synchronises, no float atomics, identical from run to run.
 *     state: 5 x int64 DEVICE words written by the call - state[3] bit 0: a face index outside [0, N) or a trace entry outside
 *     [0, Nc) (checked before anything is read through it; that face is left out), bit 1: Nc > 2^21, three ids do not fit the key
 *     and nothing else was done (the caller takes another route); state[4] = number of surviving faces. */
int stin_voxel_cluster_mean_f64(const double* coords, int64_t N, double voxel, int64_t* trace, double* new_coords, int64_t* state,
                                void* workspace, size_t workspace_bytes, stin_stream_t stream);
size_t stin_face_cluster_workspace_bytes(int64_t F);
int stin_face_cluster_i64(const int64_t* faces, int64_t F, const int64_t* trace, int64_t N, int64_t Nc, int64_t* out_faces,
                          int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream);

/* circle masks: the reference's circle inpainting masks (preprocessing/observed_texture_map_generation.py:530-603,
 * process_frame_circles) and the training transforms of the 3-D inpainting recipe, on the device.
 * stin_mask_adjacency_i64: both directions of every (src[e], dst[e]) pair -> int32 CSR rowptr [N + 1], col [2E] (order within a
 *     row unspecified; duplicates and self loops are kept - harmless to a hop distance).  Pairs with an endpoint outside [0, N)
 *     are left out and set *bad.  Workspace >= stin_mask_adjacency_workspace_bytes(N).
 * stin_circle_mask_run: dist[m][v] = min(R, hop distance from v to the nearest centre of mask m), mask[m][v] = R - dist (mask may
 *     be NULL).  Graph g owns vertices [ptr[g], ptr[g + 1]) (edges never cross graphs).  Each (mask, graph) instance j = m * B + g
 *     runs the reference's batch loop: k = min(10, n); after each batch total += k, cur = masked / n (fp64), stop when
 *     cur >= frac, else k = min(n, int(total * (frac / cur - 1))) and stop when k <= 0; centres of batch b are drawn with
 *     replacement from the graph's range by a counter-based hash of (seed, m, b, i); graph_seeds (HOST array of B <= 64 values, or
 *     NULL) gives graph g the seed graph_seeds[g] instead (a graph's masks then do not depend on the batch it is collated in).  Exactly max_iters batch launches (no host
 *     synchronisation); an instance still running after max_iters batches is flagged as capped.  centres != NULL (one mask, one
 *     graph): a single batch over the given global vertex ids instead.
 *     info: [M * B][5 + 2 * max_iters] int64 = batches run, done, capped, masked vertices, total centres, the batch sizes, the
 *     masked count after each batch; then one status word: bit 0 = the overflow drain did not finish, bit 1 = centre_log too short.
 *     centre_log (may be NULL): [M * B][log_cap] int64, the centres drawn by each instance in order.
 *     Needs M * N < 2^31 and a workspace of stin_circle_mask_workspace_bytes(N, M, B).  The distances are independent of the
 *     schedule (integer atomicMin, a vertex expanded only by the workgroup that lowered it).
 * stin_augment_rewrite_f32: one pass over x [N, ldx >= 10] of the sample: dist != NULL: x[:, 0:3] = color * known, x[:, 9] = known,
 *     mask[v] = R - dist[v] (known = dist >= R); rot != NULL: x[:, 3:6] = x[:, 3:6] @ rot; lin / rot: x[:, 6:9] = (x[:, 6:9] @ lin)
 *     @ rot with the product rounded to fp32 in between.  lin, rot: HOST pointers to 9 floats (row-major 3 x 3) or NULL. */
size_t stin_mask_adjacency_workspace_bytes(int64_t N);
int stin_mask_adjacency_i64(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int32_t* rowptr, int32_t* col,
                            int32_t* bad, void* workspace, size_t workspace_bytes, stin_stream_t stream);
size_t stin_circle_mask_workspace_bytes(int64_t N, int num_masks, int num_graphs);
int stin_circle_mask_run(const int32_t* rowptr, const int32_t* col, int64_t N, const int64_t* ptr, int num_graphs, int num_masks,
                         int radius, double frac, uint64_t seed, const int64_t* graph_seeds, int max_iters, const int64_t* centres,
                         int64_t num_centres,
                         int32_t* dist, int64_t* mask, int64_t* info, int64_t* centre_log, int64_t log_cap, void* workspace,
                         size_t workspace_bytes, stin_stream_t stream);
int stin_augment_rewrite_f32(float* x, int64_t ldx, const float* color, int64_t ldc, const int32_t* dist, int radius, int64_t* mask,
                             int64_t N, const float* lin, const float* rot, stin_stream_t stream);

/* training crops: the reference's preprocessing/crop_training_samples.py (`process_frame` :51-237) for ALL crops of a scene in one
 * batched pass.  The scene is a DEVICE table of segments (built by the caller); `n` = elements per crop, `base` = first index of
 * the segment's [n_crops][n] block in the flat flag / position arrays (blocks do not overlap; `total` = their summed size):
 *   STIN_CROP_VERTICES  src = float rows [n, width >= 3] (x, y, z first), ibase = first index of its [n_crops][n] block in `inbox`,
 *                       out = kept rows (float, same width), ids_out (may be NULL) = the kept rows' original indices (int64);
 *   STIN_CROP_EDGES     src = int64 [n, 2], vseg = index of the level's VERTICES segment, out = int64 [., 2] relabelled rows;
 *   STIN_CROP_DILATED   as EDGES; a row is kept when both endpoints are KEPT vertices; aux = -1: relabelled by the level's new ids,
 *                       aux = index of an OCCURS segment: by the rank among the vertices that occur in this filtered set (what the
 *                       reference's np.unique(..., return_inverse=True) yields);
 *   STIN_CROP_OCCURS    n = the level's vertex count; flags only;
 *   STIN_CROP_TRACE     (no flags: base unused) n = fine vertex count, vseg / aux = the fine / coarse VERTICES segments, src = the
 *                       scene's fine -> coarse map (int64 [n]), out = int64 trace per kept fine vertex, p0 = int32 query list (same
 *                       length), p1 = uint8 "has a predecessor" per kept coarse vertex (zeroed by the caller), ibase = row of the
 *                       segment in `info`.
 * The output of a segment is the concatenation of its crops in crop order; bounds[seg][c] (int64 [n_segs][n_crops + 1]) are the
 * crop boundaries in it, bounds[seg][n_crops] - bounds[seg][0] rows in all: the caller reads the table once to size the outputs.
 *   stin_crop_mark:   boxes = double [n_crops][4] (lo_x, hi_x, lo_y, hi_y; closed; z unbounded), inbox uint8 [inbox_total], flags
 *                     uint8 [total + 1], pos int32 [total + 1] (exclusive scan of flags), status int32 [2]: status[0] != 0 = an edge
 *                     endpoint outside its level.  Needs total + 1 < 2^31 and stin_crop_workspace_bytes(total).
 *   stin_crop_gather: writes every `out` / `ids_out` of the table (segments with out == NULL are skipped).
 *   stin_crop_traces: after the gather (it reads the kept positions from the VERTICES outputs).  info int32 [n_trace][n_crops][4],
 *                     zeroed by the caller: [0] redirected vertices (target not kept: nearest kept coarse vertex to the vertex's
 *                     own position, fp64 ((dx dx + dy dy) + dz dz), lowest index on a tie), [1] != 0: some vertex kept its
 *                     target, [2] kept coarse vertices without a predecessor (the caller repairs these).  status[1] != 0 = a
 *                     trace value outside the coarse level.
 *   stin_label_pool_i64: out[v] = most frequent labels[i] over trace0[i] == v (lowest label on a tie, 0 without any), v < n0;
 *                     integer histogram in the workspace; *status != 0: a trace or label value out of range.
 * max_n = the largest n of the table (sizes the grid).  Nothing allocates or synchronises. */
#define STIN_CROP_VERTICES 0
#define STIN_CROP_EDGES 1
#define STIN_CROP_DILATED 2
#define STIN_CROP_OCCURS 3
#define STIN_CROP_TRACE 4
#define STIN_CROP_MAX_SEGS 1024
#define STIN_CROP_MAX_CROPS 65535
typedef struct stin_crop_seg {
    int64_t kind, level, vseg, aux, n, base, width, ibase;
    const void* src;
    void* out;
    int64_t* ids_out;
    void *p0, *p1;
    int64_t reserved[3];
} stin_crop_seg_t;                                     /* 16 x 8 = 128 bytes */
size_t stin_crop_workspace_bytes(int64_t total);
int stin_crop_mark(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, const double* boxes, int n_crops, int64_t total,
                   int64_t inbox_total, uint8_t* inbox, uint8_t* flags, int32_t* pos, int64_t* bounds, int32_t* status,
                   void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_crop_gather(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, int n_crops, const uint8_t* flags, const int32_t* pos,
                     stin_stream_t stream);
int stin_crop_traces(const stin_crop_seg_t* segs, int n_segs, int64_t max_n, int n_crops, const uint8_t* flags, const int32_t* pos,
                     int32_t* info, int32_t* status, stin_stream_t stream);
size_t stin_label_pool_workspace_bytes(int64_t n0, int n_labels);
int stin_label_pool_i64(const int64_t* trace0, const int64_t* labels, int64_t n_orig, int64_t n0, int n_labels, int64_t* out,
                        int32_t* status, void* workspace, size_t workspace_bytes, stin_stream_t stream);

/* graph levels: the python around the decimator of the reference's preprocessing/graph_level_generation.py (csv2npy :135-191,
 * get_color_and_labels :98-116, nearest_neighbor_interpolation_for_unassigned_traces :284-295) reduced to one primitive and a
 * few integer kernels (stin_levels.hip).
 *   stin_nearest_f64: for query i < Q the index of the nearest of points [P, 3] (fp64, row-major), with
 *                     d = (dx dx + dy dy) + dz dz in fp64 without contraction and strict < in ascending index order (the lowest
 *                     index wins a tie) - numpy's argmin of the same expression.  queries: fp64 [n_query_rows, 3].
 *                     q_index == NULL: query i is row i and out_index[i] / out_d2[i] (may be NULL: squared distance) its answer
 *                     (Q <= n_query_rows).  q_index != NULL (int64 [Q]): query i is row q_index[i] and the answer goes to
 *                     out_index[q_index[i]] (out arrays of n_query_rows entries; rows not listed are left alone).
 *                     q_count (may be NULL): DEVICE word, only the first min(Q, *q_count) queries are run.
 *                     chunks: the points are cut into this many parts (1 .. 64; stin_nearest_chunks(Q, P) picks it from the
 *                     device's CU count), each writing partial (d, index) pairs [chunks][Q] into the workspace
 *                     (stin_nearest_workspace_bytes(Q, chunks); 0 for chunks <= 1) that a second launch folds by the same rule.
 *                     flags: one DEVICE int64 word, OR-ed (never cleared here): 1 = non-finite query, 2 = non-finite point,
 *                     4 = q_index entry outside [0, n_query_rows).  Q == 0: nothing is done; P == 0 (with Q > 0): STIN_E_SIZE;
 *                     P >= 2^31 - 1: STIN_E_UNSUPPORTED.
 *   traces (csv2npy): R rows of a decimator's CSV, row r = new vertex new_id[r] and the old vertices old_id[row_ptr[r] ..
 *                     row_ptr[r + 1]) (row_of[t] = the row of entry t).  state: int64 [5] on the device -
 *                     [0] old vertices named by more than one entry, [1] new vertices for which a row came after an earlier row
 *                     WITH old vertices (an earlier row without any is tolerated, as in the reference), [2] new vertices that no
 *                     row and no old vertex points to, [3] flag word (the bits of stin_nearest_f64; 8 = an id out of range,
 *                     16 = a trace entry still unassigned or out of range at the check), [4] number of unassigned old vertices.
 *     stin_trace_scatter_i64    clears state and workspace; trace[:] = -1; trace[old_id[t]] = new_id[row_of[t]]; counts hits per
 *                               old vertex and rows / rows with entries / the last row per new vertex.
 *     stin_trace_unassigned_i64 list[0 .. state[4]) = the old vertices with trace == -1 (order unspecified; state[4] is reset first).
 *                               Meant as q_index / q_count of stin_nearest_f64 with out_index = trace.
 *     stin_trace_check_i64      after the fill: state[0], state[1], state[2] from the counts in the SAME workspace.
 *   Workspace of the three: stin_trace_workspace_bytes(n_old, n_new).  Nothing allocates or synchronises.
 *   stin_cluster_mean_f32: out[c] = float32 mean of coords[order[seg_ptr[c] .. seg_ptr[c + 1])] (float32 [n, 3]) accumulated one
 *                     row after the other in float32 - what numpy's mean(axis=0) gives the reference's vertex clustering when a
 *                     level is clustered from float32 positions (every level after the first). */
int stin_nearest_chunks(int64_t Q, int64_t P);
size_t stin_nearest_workspace_bytes(int64_t Q, int chunks);
int stin_nearest_f64(const double* queries, int64_t n_query_rows, const double* points, int64_t P, const int64_t* q_index,
                     const int64_t* q_count, int64_t Q, int chunks, int64_t* out_index, double* out_d2, int64_t* flags,
                     void* workspace, size_t workspace_bytes, stin_stream_t stream);
size_t stin_trace_workspace_bytes(int64_t n_old, int64_t n_new);
int stin_trace_scatter_i64(const int64_t* new_id, const int64_t* row_ptr, int64_t R, const int64_t* old_id, const int64_t* row_of,
                           int64_t n_entries, int64_t n_old, int64_t n_new, int64_t* trace, int64_t* state, void* workspace,
                           size_t workspace_bytes, stin_stream_t stream);
int stin_trace_unassigned_i64(const int64_t* trace, int64_t n_old, int64_t* list, int64_t* state, stin_stream_t stream);
int stin_trace_check_i64(const int64_t* trace, int64_t n_old, const int64_t* row_ptr, int64_t R, int64_t n_new, int64_t* state,
                         void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_cluster_mean_f32(const float* coords, int64_t n, const int64_t* order, const int64_t* seg_ptr, int64_t n_seg, float* out,
                          stin_stream_t stream);

/* k nearest neighbours: stin_nearest_f64 with k answers per query and a point set that can be restricted in place
 * (stin_knn.hip) - the primitive under the fill of unseen vertices that Open3D's colour-map pipeline ends with (the reference's
 * preprocessing/texture_map_optimization.py; see "Frame colours") and under a nearest-known-vertex inpainting baseline.  A
 * contract of the project's own, NOT pinned against Open3D; tests/_knn_oracle.py restates it in numpy and agrees bit for bit.
 * Everything is fp64 and IEEE, the operations in the order written, nothing contracted.
 *   distance    d(q, p) = (dx dx + dy dy) + dz dz: the expression of stin_nearest_f64.
 *   candidates  the points p with p_valid == NULL || p_valid[p] != 0 (p_valid: uint8 [P]).  An invalid point is skipped IN PLACE:
 *               its index is never reported, its coordinates are never looked at (they may be non-finite), and every index is an
 *               index into the full points array - nothing is compacted, so "the lowest index wins a tie" keeps its meaning
 *               for a subset such as "seen vertices only".
 *   answer      for query i the k smallest candidates under the total order (d, index), ascending: out_index[row][0 .. k) int64 and,
 *               out_d2 != NULL, out_d2[row][0 .. k) fp64 (both [n_query_rows][k], dense).  Fewer than k candidates: the remaining
 *               slots hold index -1 and d2 = +inf.  numpy: np.argsort(d[valid], kind='stable')[:k] mapped back through
 *               np.flatnonzero(valid).  A candidate whose d is not < +inf (squares that overflow) is never reported, as in
 *               stin_nearest_f64.  1 <= k <= STIN_KNN_MAX_K.
 *   queries     q_index / q_count exactly as in stin_nearest_f64: query i is row q_index[i] (NULL: row i, Q <= n_query_rows) and its
 *               answers go to output row q_index[i]; q_count (may be NULL) is a DEVICE word, only the first min(Q, *q_count) queries
 *               are run; rows not listed are not written.
 *   flags       the int64 DEVICE word and bits of stin_nearest_f64, OR-ed: 1 = non-finite query, 2 = non-finite VALID point,
 *               4 = q_index entry outside [0, n_query_rows) (that query is skipped).
 *   chunks      1 .. 64, stin_knn_chunks(Q, P, k) picks it; each chunk writes its k-list per query into the workspace
 *               (stin_knn_workspace_bytes(Q, chunks, k); 0 for chunks <= 1), a second launch merges the lists in ascending chunk
 *               order under (d, index).  The result does not depend on chunks.
 *   sizes       Q == 0: nothing is done.  P == 0 is allowed (every listed row becomes -1 / +inf).  Negative sizes, k or chunks out
 *               of range, Q > n_query_rows without q_index: STIN_E_SIZE; P >= 2^31 - 1: STIN_E_UNSUPPORTED; all before any launch.
 * stin_knn_mean_f32: the mean of the neighbours' rows.  values float32 [P][C] (row pitch ld_values), idx int64 [n_rows][k] (what
 *     stin_knn_f64 wrote), out float32 [n_rows][C] (row pitch ld_out), filled uint8 [n_rows] (may be NULL), q_index / q_count / Q as
 *     above.  For a listed row with m >= 1 neighbours - the leading entries of its idx row that lie in [0, P) -
 *       out[row][c] = (float)((((double)v1 + (double)v2) + ...) / (double)m),   the sum left to right in neighbour order,
 *     and filled[row] = 1; a row with m == 0 is left untouched and gets filled[row] = 0; a row id outside [0, n_rows) is skipped.
 *     1 <= C <= STIN_KNN_MAX_C.  values and out MAY BE THE SAME ARRAY provided no listed row is a neighbour of any listed row
 *     (in the fill the listed rows are the unseen vertices and the candidates the seen ones: disjoint); otherwise they must not
 *     overlap.
 * Caller-owned buffers and workspace, the caller's stream; nothing allocates or synchronises. */
#define STIN_KNN_MAX_K 16
#define STIN_KNN_MAX_C 16
int stin_knn_chunks(int64_t Q, int64_t P, int k);
size_t stin_knn_workspace_bytes(int64_t Q, int chunks, int k);
int stin_knn_f64(const double* queries, int64_t n_query_rows, const double* points, const uint8_t* p_valid, int64_t P,
                 const int64_t* q_index, const int64_t* q_count, int64_t Q, int k, int chunks, int64_t* out_index, double* out_d2,
                 int64_t* flags, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_knn_mean_f32(const float* values, int64_t ld_values, int64_t P, int C, const int64_t* idx, int k, const int64_t* q_index,
                      const int64_t* q_count, int64_t Q, int64_t n_rows, float* out, int64_t ld_out, uint8_t* filled,
                      stin_stream_t stream);

/* QEM: a deterministic, parallel quadric-error-metric edge-collapse decimator and vertex normals (stin_qem.hip) - the step the
 * reference shells out to vcglib's tridecimator for (graph_level_generation.py, --qem), with the fine -> coarse trace as a result
 * instead of a CSV.  preprocessing.decimate_qem drives it: a loop of rounds, per round the sorts on the host side (torch) and the
 * entry points below, one host read (the number of selected edges).  All arithmetic is fp64 with the association written out in the
 * kernels and no contraction; tests/_qem_oracle.py restates it in numpy and agrees bit for bit.  Every index array is int64; every
 * index read from memory is compared with its array's size before it is used (an entry that fails is skipped / makes its edge
 * invalid); nothing allocates or synchronises.
 * A quadric is the row q[10] = a00 a01 a02 a03 a11 a12 a13 a22 a23 a33 of a symmetric 4 x 4 matrix; the cost of a point h = (p, 1)
 * is r_k = ((q_k0 x + q_k1 y) + q_k2 z) + q_k3, cost = ((x r_0 + y r_1) + z r_2) + r_3.
 *   stin_qem_face_quadrics_f64      per face (a, b, c): n = (v_b - v_a) x (v_c - v_a), len = sqrt(n . n), u = n / len, d = -(u . v_a),
 *                                   face_quadrics[f] = (len / 2) p p^T with p = (u, d), face_normals[f] = u; both zero when
 *                                   len is not > 0 or an index is out of range.  Either output may be NULL.
 *   stin_qem_boundary_quadrics_f64  per boundary edge b (bi[b] < bj[b], the one face bface[b]): e = v_j - v_i, m = e x
 *                                   face_normals[bface], u = m / |m|, d = -(u . v_i): |e|^2 p p^T, zero when |m| is not > 0.
 *   stin_qem_vertex_sum_f64         out[v] (+)= sum of table[col[s]] (rows of `width` <= 10 doubles) for s = rowptr[v] ..
 *                                   rowptr[v + 1) IN THAT ORDER - the fixed-order segmented sum of the vertex quadrics (faces in
 *                                   ascending face id, then, accumulate = 1, boundary edges in ascending (min, max) order); no float
 *                                   atomics.  normalize = 1 (width 3): out[v] = sum / |sum|, (0, 0, 1) for a zero sum - vertex
 *                                   normals from the unit face normals.
 *   stin_qem_edges_f64              one round's candidate edges (ei[e] < ej[e], unique, sorted by (ei, ej); faces_on_edge[e] faces)
 *                                   on the round's unmodified mesh: Q = Q_i + Q_j; A x = b (A = Q[:3,:3], b = -Q[:3,3]) by explicit
 *                                   cofactors, taken when |det A| > 1e-10 (max|A|)^3 and |x - mid| <= |v_i - v_j|, else the cheapest
 *                                   of v_i, v_j, mid (ties in that order); cost[e] = max(h^T Q h, 0), x[e] = h.
 *                                   valid[e] = cost finite, 1 <= faces_on_edge <= 2, link condition (|N(i) & N(j)| == faces_on_edge,
 *                                   two sorted lists of the neighbour CSR) and flip condition (every face of i or j without both,
 *                                   through the vertex -> face CSR: n_old . n_new > 0.2 |n_old| |n_new|, so a zero-area face blocks).
 *   stin_qem_select_i64             order of the valid edges: (cost, e).  vertex_min[v] = the first valid edge of v (nbr_edge[s] =
 *                                   the edge of neighbour slot s; -1: none), ring_min[v] = the first of vertex_min over the closed
 *                                   one-ring, selected[e] = valid and ring_min[ei] == ring_min[ej] == e: the minimum among all
 *                                   valid edges with an endpoint in N[i] | N[j].  No two selected edges share or neighbour an
 *                                   endpoint.  Segmented minima: no atomics, identical from run to run.
 *   stin_qem_collapse_f64           per listed edge e (edge_ids[S]): vertices[i] = x[e], quadrics[i] += quadrics[j], parent[j] = i.
 *   stin_qem_remap_faces_i64        faces [F, 3] in place through parent (NULL: unchanged); keep[f] = every index in [0, N) and no
 *                                   repeated vertex (the caller compacts, keeping the order); *status (device int32, OR-ed) |= 1
 *                                   for an index outside [0, N).  With parent == NULL this is the range check of the input.
 *   stin_qem_trace_i64              trace[v] = rank[r], r the end of v's parent chain (parent[r] == r); *status |= 2 and -1 for a
 *                                   chain that leaves [0, N) or does not end within N steps. */
int stin_qem_face_quadrics_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, double* face_quadrics,
                               double* face_normals, stin_stream_t stream);
int stin_qem_boundary_quadrics_f64(const double* vertices, int64_t N, const int64_t* bi, const int64_t* bj, const int64_t* bface,
                                   int64_t B, const double* face_normals, int64_t F, double* boundary_quadrics, stin_stream_t stream);
int stin_qem_vertex_sum_f64(const int64_t* rowptr, const int64_t* col, int64_t nnz, const double* table, int64_t n_items, int width,
                            int64_t N, double* out, int accumulate, int normalize, stin_stream_t stream);
int stin_qem_edges_f64(const double* vertices, const double* quadrics, int64_t N, const int64_t* ei, const int64_t* ej,
                       const int64_t* faces_on_edge, int64_t E, const int64_t* nbr_rowptr, const int64_t* nbr_col, int64_t nbr_nnz,
                       const int64_t* vf_rowptr, const int64_t* vf_face, int64_t vf_nnz, const int64_t* faces, int64_t F, double* x,
                       double* cost, uint8_t* valid, stin_stream_t stream);
int stin_qem_select_i64(const int64_t* ei, const int64_t* ej, int64_t E, const int64_t* nbr_rowptr, const int64_t* nbr_col,
                        const int64_t* nbr_edge, int64_t nbr_nnz, const double* cost, const uint8_t* valid, int64_t N,
                        int64_t* vertex_min, int64_t* ring_min, uint8_t* selected, stin_stream_t stream);
int stin_qem_collapse_f64(const int64_t* edge_ids, int64_t S, const int64_t* ei, const int64_t* ej, int64_t E, const double* x,
                          double* vertices, double* quadrics, int64_t* parent, int64_t N, stin_stream_t stream);
int stin_qem_remap_faces_i64(int64_t* faces, int64_t F, const int64_t* parent, int64_t N, uint8_t* keep, int32_t* status,
                             stin_stream_t stream);
int stin_qem_trace_i64(const int64_t* parent, const int64_t* rank, int64_t N, int64_t* trace, int32_t* status, stin_stream_t stream);

/* Observer masks: which vertices of a mesh does each camera pose of a scan see (stin_observe.hip; the rasteriser under it and
 * under "Render" is stin_raster.hip: cull, coverage and depth below are its contract for both) - the `observers` mode of the
 * reference's preprocessing/observed_texture_map_generation.py (compute_observed_vertex_map :159-251, which renders the mesh with
 * PyTorch3D's MeshRasterizer at 256 x 256 and keeps pix_to_face; generate_mask_from_vertex_observing_poses :259-267), as a
 * depth-tested triangle rasteriser.  The projection below is what compute_projection_matrix (:117-133) composed with PyTorch3D's
 * documented NDC convention amounts to (z_sign = -1 and the left / up NDC axes cancel into a plain pinhole with the principal point
 * at the image centre and the full field of view stretched onto the square image); it is derived from reading that code and is NOT
 * pinned against a PyTorch3D run.  Everything is fp64 and IEEE, the operations in the order written, nothing contracted;
 * tests/_observers_oracle.py restates it in numpy (per pixel over all faces) and agrees bit for bit.
 *
 *   poses     RT [P][12] = the rows of E[:3, :4], E = inverse of the camera-to-world pose (ScanNet's *.pose.txt), formed on the host
 *             (preprocessing.pose_extrinsics); valid [P] bytes: 0 for a pose with a non-finite entry (ScanNet writes -inf for lost
 *             tracking) - it observes nothing.
 *   view      xv = ((R00 x + R01 y) + R02 z) + t0, likewise yv, zv.
 *   screen    X = (sx xv / zv + 1.0) (0.5 S) - 0.5, Y likewise with sy, yv; sx = 2 fx / width, sy = 2 fy / height; pixel (row i,
 *             column j) has its centre at (X, Y) = (j, i).
 *   cull      a face is skipped for a pose when a corner has zv < z_near (faces that cross the near plane are DROPPED, not clipped:
 *             ScanNet faces are centimetres across), an index is outside [0, N), a screen coordinate is not finite, or
 *             area2 = edge(a, b, c) is 0;  edge(p, q, r) = (q.x - p.x) (r.y - p.y) - (q.y - p.y) (r.x - p.x).
 *   coverage  wa = edge(b, c, pix), wb = edge(c, a, pix), wc = edge(a, b, pix): covered when all three are >= 0 (area2 > 0) or all
 *             <= 0 (area2 < 0): inclusive edges, no fill rule, both orientations.
 *   depth     la = wa / area2, lb, lc likewise; zp = 1.0 / ((la / za + lb / zb) + lc / zc); key = bits(float32(zp)) << 32 | face id;
 *             the pixel keeps the MINIMUM key (64-bit integer atomicMin): the nearest face after rounding to fp32, the lowest id on a tie.
 *   observers vertex v is observed by pose p when it is a corner of the winning face of at least one pixel of p:
 *             bits [N][words] uint32, bit (p & 31) of word (p >> 5); words >= ceil(P / 32).  Integer atomicOr.
 * stin_observe_poses_f64: poses in batches of `batch` (1 .. STIN_OBSERVE_MAX_BATCH) whose z-buffers (batch S S 8 bytes) and screen
 *     coordinates (batch N 24 bytes) live in the workspace; the result does not depend on batch.  Per batch: clear, transform every
 *     vertex once, rasterise with one thread per (face, pose), resolve with one thread per (pixel, pose).  A face whose clamped box
 *     holds more than large_box centres (<= 0: STIN_OBSERVE_LARGE_BOX) goes through a queue to a second rasteriser that spreads it
 *     over a wavefront (64: a wavefront's worth of centres, measured in profiles/r20_observers.md); the result does not depend on
 *     large_box either.  faces are narrowed to int32 once.  S <= STIN_OBSERVE_MAX_SIZE,
 *     N, F < 2^31 - 1, z_near > 0 (STIN_E_SIZE otherwise).  *status (device int32, written): STIN_OBSERVE_BAD_INDEX - a face had an
 *     index outside [0, N) (it is skipped, the others are unaffected); STIN_OBSERVE_LARGE_FACE - informational: a face went
 *     through the large-face rasteriser.  bits is written in full.  Nothing allocates or synchronises.
 * stin_observe_mask_u32: count[m][v] = popcount(bits[v] & visible_words[m]) over the words, mask[m][v] = (count >= min_num_poses) ^
 *     invert as int64 - the reference's values with invert = 0 (1 = seen by enough poses of the subset).  mask or count may be NULL. */
#define STIN_OBSERVE_BAD_INDEX 1
#define STIN_OBSERVE_LARGE_FACE 2
#define STIN_OBSERVE_LARGE_BOX 64
#define STIN_OBSERVE_MAX_SIZE 4096
#define STIN_OBSERVE_MAX_BATCH 1024
size_t stin_observe_workspace_bytes(int64_t N, int64_t F, int S, int batch);
int stin_observe_poses_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const double* RT, const uint8_t* valid,
                           int64_t P, double sx, double sy, int S, double z_near, int batch, int64_t large_box, uint32_t* bits,
                           int64_t words, int32_t* status, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_observe_mask_u32(const uint32_t* bits, int64_t N, int64_t words, const uint32_t* visible_words, int M, int min_num_poses,
                          int invert, int64_t* mask, int32_t* count, stin_stream_t stream);

/* Frame colours: per-vertex colours of a mesh from a scan's RGB-D frames and camera trajectory (stin_frames.hip) - what the
 * reference's preprocessing/texture_map_optimization.py asks of Open3D's colour-map pipeline with maximum_iteration = 0: nothing is
 * optimised, every vertex is projected into every frame that sees it, the colour image is sampled bilinearly and the samples are
 * averaged.  Neither Open3D nor cv2 can run beside this project, so this is a contract of the project's own, NOT a port and NOT
 * pinned against an Open3D run; tests/_frames_oracle.py restates it in numpy (per pose over all vertices) and agrees bit for bit.
 * Everything is fp64 and IEEE, the operations in the order written, nothing contracted; integers where stated.
 *
 *   poses     RT [B][12], valid [B]: the rows of preprocessing.pose_extrinsics' output for one batch of poses (see "Observer
 *             masks"); first_pose = the scan-wide id of the batch's first pose, p = first_pose + b.  An invalid pose contributes nothing.
 *   view      xv = ((R00 x + R01 y) + R02 z) + t0, likewise yv, zv (the observers' expression).
 *   cameras   one for the colour frames (Hc x Wc) and one for the depth frames (Hd x Wd), each (fx, fy, cx, cy) in pixels of its own
 *             frame size; the sizes may differ.  u = fx xv / zv + cx, v = fy yv / zv + cy; pixel (row i, column j) is centred at
 *             (u, v) = (j, i).  A pair (vertex, pose) is skipped when zv < z_near (z_near > 0; no clipping at the near plane) or when
 *             any of u, v of a camera in use is not finite.
 *   depth     uint16 [B][Hd][Wd] raw sensor units; r = raw, r = 0 where raw / depth_scale > depth_trunc; 0 = no measurement.
 *   edges     the depth-discontinuity mask, exact integer arithmetic on r with row and column indices clamped to the image:
 *               gx = (r[i-1,j+1] + 2 r[i,j+1] + r[i+1,j+1]) - (r[i-1,j-1] + 2 r[i,j-1] + r[i+1,j-1])
 *               gy = (r[i+1,j-1] + 2 r[i+1,j] + r[i+1,j+1]) - (r[i-1,j-1] + 2 r[i-1,j] + r[i-1,j+1])
 *             edge0 = (double)(gx gx + gy gy) > T T (the sum in int64), T = discontinuity_threshold depth_scale;
 *             edge[i,j] = any edge0 in the (2 k + 1)^2 window around it that lies inside the image, k = half_kernel >= 0.
 *             UNIT of discontinuity_threshold: metres of SOBEL response, not metres of depth - a depth step of s metres between two
 *             columns gives |gx| = 4 s (8 s across a two-pixel ramp).  Open3D's option value 0.1 is in the same unit.
 *   visible   from depth: ui = rint(u_d), vi = rint(v_d) (ties to even), 0 <= ui < Wd, 0 <= vi < Hd, rr = r[b, vi, ui] != 0,
 *             d = rr / depth_scale, !(d > max_depth), !edge[b, vi, ui], |zv - d| < depth_threshold;
 *             or, depth == NULL, from observer bits: bit (p & 31) of word (p >> 5) of bits[v] (stin_observe_poses_f64's layout).
 *   sample    colour frames uint8 [B][Hc][Wc][3], RGB, channel last (3-byte pixels: read as bytes, no alignment assumed).  Required:
 *             margin <= u <= Wc - 1 - margin and margin <= v <= Hc - 1 - margin (integer margin >= 0).  x0 = floor(u), y0 = floor(v),
 *             a = u - x0, b = v - y0, x1 = min(x0 + 1, Wc - 1), y1 likewise; per channel
 *               val = (((1-a)(1-b)) I[y0,x0] + (a(1-b)) I[y0,x1]) + (((1-a) b) I[y1,x0] + (a b) I[y1,x1]),  q = (int64) rint(val 65536.0).
 *   sums      sum[v][c] += q (int64), count[v] += 1 (int32), bit p of seen[v] set (optional; uint32 [N][seen_words]).  Integers: the
 *             result depends neither on the order of the poses, nor on the batching, nor on how the work is split over threads.
 *             q < 2^24: int64 cannot overflow below 2^31 poses.  Integer atomics only; no float atomics.
 *   finish    colour[v][c] = float32(sum[v][c] / (count[v] 16711680.0)) in [0, 1] (16711680 = 65536 * 255); observed[v] = count[v] > 0;
 *             a vertex with count 0 gets (fill_r, fill_g, fill_b).  The k-nearest-neighbour fill of unseen vertices that Open3D's
 *             pipeline ends with is a separate step on top of this one (preprocessing.fill_unseen_colors: stin_knn_f64 with
 *             p_valid = count > 0, then stin_knn_mean_f32; see "k nearest neighbours") - the mean colour of the k nearest
 *             coloured vertices, k = 3 being Open3D's default (invisible_vertex_color_knn) as far as we know; neither the default
 *             nor Open3D's tie handling could be checked against a run of it.
 * stin_frames_depth_edges_u16: depth [B][Hd][Wd] -> edge bytes [B][Hd][Wd] (0 / 1), two passes: the gradient test into the
 *     workspace (stin_frames_edges_workspace_bytes), then the dilation (separable, through LDS).  half_kernel <=
 *     STIN_FRAMES_MAX_HALF_KERNEL, depth_scale > 0, sizes in [1, STIN_FRAMES_MAX_SIZE], B <= STIN_FRAMES_MAX_BATCH (STIN_E_SIZE).
 * stin_frames_accumulate_f64: one batch of poses into sum / count / seen, which are ACCUMULATED INTO, not cleared: the caller zeroes
 *     them once per scene; batches of one scene arrive in any order and any size (on one stream, or otherwise ordered).
 *     cameras: HOST array of STIN_FRAMES_CAMERA_DOUBLES doubles = colour (fx, fy, cx, cy), depth (fx, fy, cx, cy); params: HOST array
 *     of STIN_FRAMES_PARAM_DOUBLES doubles = depth_scale, depth_trunc, max_depth, depth_threshold, z_near (read during the call).  Depth mode:
 *     depth, edge and the depth camera and parameters; bits mode (depth == NULL): bits with words >= ceil((first_pose + B) / 32).
 *     seen may be NULL; else seen_words >= ceil((first_pose + B) / 32).  Lanes run along the vertices and a thread keeps its vertex's
 *     sums in registers over a chunk of poses.  route: STIN_FRAMES_ROUTE_AUTO - a host decision from N and B alone: with enough
 *     vertices to fill the chip (or few poses) one thread owns a vertex for the whole batch and stores without atomics
 *     (STIN_FRAMES_ROUTE_OWNER), else the poses are split over a second grid dimension and every chunk adds its four values with one
 *     integer atomicAdd each (STIN_FRAMES_ROUTE_SPLIT); both give identical bits.  N < 2^31 - 1, first_pose + B < 2^31.
 * stin_frames_finish_f32: sum, count -> colours float32 [N][3], observed bytes [N] (either may be NULL).
 * Null pointers are allowed where a count is 0.  Nothing allocates or synchronises. */
#define STIN_FRAMES_MAX_SIZE 16384
#define STIN_FRAMES_MAX_BATCH 4096
#define STIN_FRAMES_MAX_HALF_KERNEL 15
#define STIN_FRAMES_CAMERA_DOUBLES 8
#define STIN_FRAMES_PARAM_DOUBLES 5
#define STIN_FRAMES_ROUTE_AUTO 0
#define STIN_FRAMES_ROUTE_OWNER 1
#define STIN_FRAMES_ROUTE_SPLIT 2
size_t stin_frames_edges_workspace_bytes(int B, int Hd, int Wd);
int stin_frames_depth_edges_u16(const uint16_t* depth, int B, int Hd, int Wd, double depth_scale, double depth_trunc,
                                double discontinuity_threshold, int half_kernel, uint8_t* edge, void* workspace,
                                size_t workspace_bytes, stin_stream_t stream);
int stin_frames_accumulate_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                               const uint8_t* color, int Hc, int Wc, const uint16_t* depth, const uint8_t* edge, int Hd, int Wd,
                               const double* cameras, const double* params, const uint32_t* bits, int64_t words, int margin,
                               int route, int64_t* sum, int32_t* count, uint32_t* seen, int64_t seen_words, stin_stream_t stream);
int stin_frames_finish_f32(const int64_t* sum, const int32_t* count, int64_t N, float fill_r, float fill_g, float fill_b,
                           float* colors, uint8_t* observed, stin_stream_t stream);

/* Colour-map optimisation: the photometric normal equations of every camera pose (stin_colormap.hip) - the hot part of the rigid
 * optimiser that Open3D's colour-map pipeline runs with maximum_iteration > 0 (Zhou & Koltun 2014), on top of "Frame colours":
 * preprocessing.optimize_poses_rigid refines the poses from the frames before the colours are averaged.  A contract of the
 * project's own, NOT a port of Open3D and NOT pinned against a run of it; tests/_colormap_oracle.py restates it in numpy (per pose
 * over all vertices) and agrees byte for byte.  Everything is fp64 and IEEE, the operations in the order written, nothing
 * contracted; integers where stated.  The non-rigid optimiser (per-camera warp grids) builds on this one: see "Non-rigid
 * colour-map optimisation" below.
 *
 *   inputs    vertices fp64 [N][3]; poses RT [B][12], valid [B], first_pose and the view (xv, yv, zv) as in "Frame colours"; colour
 *             frames uint8 [B][H][W][3]; ONE camera (fx, fy, cx, cy), the colour camera; bits uint32 [N][words], the FIXED
 *             visibility in stin_observe_poses_f64's / seen's layout; z_near > 0; integer margin >= 1.
 *   images    per pixel, int32: G = 299 R + 587 G + 114 B (<= 255000), and gx, gy = the two Sobel expressions that "Frame colours"
 *             writes for r under `edges`, on G, with row and column indices clamped to the image (|value| <= 1 020 000).  Stored as
 *             one 16-byte pixel (G, gx, gy, 0): int32 [B][H][W][4].  Intensity in [0, 1] is G / 255000.0; the derivative per pixel
 *             is gx / 2040000.0 (the Sobel response / 8: Gauss-Newton needs the true derivative), likewise gy.
 *   pairs     (v, p) contributes when pose p is valid, bit p of bits[v] is set, !(zv < z_near), u = fx xv / zv + cx and v = fy yv /
 *             zv + cy are finite, margin <= u <= W - 1 - margin and margin <= v <= H - 1 - margin: the test of
 *             stin_frames_accumulate_f64's bits mode, word for word.  The bits stay fixed over an optimisation; the projection moves.
 *   proxy     from the sums of stin_frames_accumulate_f64 in bits mode AT THE SAME POSES (sum, count zeroed first):
 *             num = 299 sum[v][0] + 587 sum[v][1] + 114 sum[v][2] (int64); proxy[v] = (double) num / ((double) count[v]
 *             16711680000.0) (= 65536 * 255 * 1000), 0 where count[v] is 0.  The pair set is the same: a contributing pair has count >= 1.
 *   per pair  sI, sX, sY = the `sample` expression of "Frame colours" (x0, y0, a, b, x1, y1, val) on G, gx, gy promoted to fp64;
 *             I = sI / 255000.0, dIdx = sX / 2040000.0, dIdy = sY / 2040000.0; r = I - proxy[v]; iz = 1.0 / zv;
 *             v0 = (dIdx fx) iz, v1 = (dIdy fy) iz, v2 = -((v0 xv + v1 yv) iz);
 *             J = ((-zv v1) + yv v2, zv v0 - xv v2, (-yv v0) + xv v1, v0, v1, v2): rotation x, y, z and translation x, y, z of an
 *             increment multiplied from the LEFT onto the extrinsic.
 *   per pose  one row of STIN_COLORMAP_ROW_DOUBLES = 28 doubles: A[i][j] += J_i J_j for i <= j in row-major order of the upper
 *             triangle (21), b[i] += J_i r (6), e += r r (1); and an int32 count n += 1.
 *   order     vertices are cut into consecutive tiles of 256 STIN_COLORMAP_U ids.  Lane l (0 .. 255) of a tile starts at +0.0 and
 *             adds its terms for the vertices base + l + 256 i, i = 0 .. STIN_COLORMAP_U - 1 ascending (a pair that does not
 *             contribute adds +0.0, i.e. nothing); the 256 lane sums x[] are folded by the halving tree, for s = 128, 64, .. 1:
 *             x[i] += x[i + s] for i < s; the tile sums x[0] are added in ascending tile order, starting at +0.0.  A function of N
 *             alone: the result depends neither on B, nor on first_pose, nor on how poses are split over launches or grid
 *             dimensions, nor on the run.  No float atomics.  A tile without a contributing pair for a pose may skip the tree: its
 *             sum is +0.0 either way (no lane sum can be -0.0).  Visible pairs are NOT compacted: that would move terms in the tree.
 *   update    on the host (preprocessing.optimize_poses_rigid): x = solve(A, -b) per pose on the symmetrised 6 x 6;
 *             D(x) = [[Rz(x2) Ry(x1) Rx(x0), x[3:6]], [0 0 0 1]]; E' = D(x) E.
 * stin_colormap_gradients_u8: colour [B][H][W][3] -> images int32 [B][H][W][4] (16-byte aligned), one workgroup per 64 x 16 tile
 *     through LDS.  16 bytes per pixel: 4.9 MB per 480 x 640 frame.  Sizes and B as for the frame kernels (STIN_E_SIZE).
 * stin_colormap_proxy_f64: sum int64 [N][3], count int32 [N] -> proxy fp64 [N].
 * stin_colormap_normal_f64: one batch of poses -> rows fp64 [B][28], counts int32 [B] (written, not accumulated), in two kernels:
 *     per (tile, chunk of poses) the tile sums into the workspace (stin_colormap_workspace_bytes: tiles x B x 116 bytes, rounded),
 *     then one thread per (pose, value) over the tiles.  images: those of the batch's B frames.  camera: HOST array of
 *     STIN_COLORMAP_CAMERA_DOUBLES doubles (read during the call).  words >= ceil((first_pose + B) / 32), margin >= 1, z_near > 0,
 *     N < 2^31 - 1, B <= STIN_FRAMES_MAX_BATCH, sizes in [1, STIN_FRAMES_MAX_SIZE] (STIN_E_SIZE otherwise).  N = 0: rows of +0.0.
 * Null pointers are allowed where a count is 0.  Nothing allocates or synchronises. */
#define STIN_COLORMAP_ROW_DOUBLES 28
#define STIN_COLORMAP_U 4
#define STIN_COLORMAP_CAMERA_DOUBLES 4
int stin_colormap_gradients_u8(const uint8_t* color, int B, int H, int W, int32_t* images, stin_stream_t stream);
int stin_colormap_proxy_f64(const int64_t* sum, const int32_t* count, int64_t N, double* proxy, stin_stream_t stream);
size_t stin_colormap_workspace_bytes(int64_t N, int B);
int stin_colormap_normal_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                             const int32_t* images, int H, int W, const double* camera, double z_near, const uint32_t* bits,
                             int64_t words, int margin, const double* proxy, double* rows, int32_t* counts, void* workspace,
                             size_t workspace_bytes, stin_stream_t stream);

/* Non-rigid colour-map optimisation: a low-resolution warp lattice per frame on top of the rigid optimiser (stin_nonrigid.hip) -
 * Zhou & Koltun 2014, section 5, the step the reference's preprocessing/texture_map_optimization.py actually asks of Open3D
 * (run_non_rigid_optimizer); preprocessing.optimize_poses_nonrigid.  It removes what a rigid pose cannot: rolling shutter, lens
 * distortion, a depth/colour misregistration that differs across the frame.  A contract of the project's own, NOT a port of Open3D
 * and NOT pinned against a run of it; tests/_nonrigid_oracle.py restates it in numpy (per pose over all vertices, every cell summed
 * by a plain loop) and agrees byte for byte.  Everything is fp64 and IEEE, the operations in the order written, nothing contracted;
 * integers where stated.  Inputs, images, the view and the projection (u, v) are those of "Colour-map optimisation".
 *
 *   lattice   step S, a positive integer in pixels of the colour frame (H, W >= 2).  Aw = ceil((W - 1) / S) + 1 and Ah = ceil((H -
 *             1) / S) + 1 anchors at the pixel coordinates (j S, i S); cells = (Ah - 1)(Aw - 1), cell (ci, cj) numbered ci (Aw - 1) +
 *             cj.  flow fp64 [P][Ah][Aw][2]: the x, then the y offset of every anchor in pixels; zero at the start.
 *   cell      gu = u / (double) S, cj = min((int) floor(gu), Aw - 2), a = gu - (double) cj; likewise gv, ci, b from v.
 *             w00 = (1 - a)(1 - b), w01 = a (1 - b), w10 = (1 - a) b, w11 = a b: the weights of the anchors (ci, cj), (ci, cj + 1),
 *             (ci + 1, cj), (ci + 1, cj + 1) with the flows f00 .. f11.  A point on a lattice line belongs to the cell it opens
 *             (a = 0), on the last line to the last cell (a = 1).
 *   warp      u' = u + ((w00 f00x + w01 f01x) + (w10 f10x + w11 f11x)); v' likewise with the y offsets.
 *   pairs     (v, p) contributes under the test of "Colour-map optimisation", word for word, on (u, v), and when in addition u', v'
 *             are finite, margin <= u' <= W - 1 - margin and margin <= v' <= H - 1 - margin.  The visibility bits stay fixed.
 *   sums      stin_nonrigid_accumulate_f64 = stin_frames_accumulate_f64 in bits mode with the colour frame sampled at (u', v'): the
 *             same q, int64 sum, int32 count, optional seen; both routes, identical bits, independent of batching and order.  With a
 *             zero flow it equals stin_frames_accumulate_f64 byte for byte (margin >= 0 here too).  The proxy is
 *             stin_colormap_proxy_f64 on these sums, unchanged.
 *   per pair  sI, sX, sY sampled from the (G, gx, gy, 0) images at (u', v'); I, dIdx, dIdy, r, iz, v0, v1, v2 and J[0 .. 5] exactly
 *             as in "Colour-map optimisation", with xv, yv, zv UNWARPED; J[6 + 2 k] = dIdx w_k, J[7 + 2 k] = dIdy w_k for k = 00, 01,
 *             10, 11: STIN_NONRIGID_LOCAL = 14 local unknowns, the pose's six and the x, y offsets of the cell's four anchors.
 *   per (pose, cell)  one block of STIN_NONRIGID_BLOCK_DOUBLES = 120 doubles: J_i J_j for i <= j in row-major order of the upper
 *             triangle (105), J_i r (14), r r (1); and an int32 pair count.
 *   order     the terms of a (pose, cell) are added one after another in ASCENDING VERTEX ID, starting at +0.0: a function of the
 *             inputs alone, not of B, first_pose, the split of the poses over launches, or the run.  A cell without pairs is 120 x
 *             +0.0.  No float atomics.
 *   update    on the host (preprocessing.nonrigid_update; its linear solve alone on the device: "Non-rigid solve" below, a second
 *             solver with its own bytes), per free, valid pose whose pair count n_p (the sum of its cells' counts)
 *             is >= min_pairs: unknown k < 6 is the pose's, unknown 6 + 2 (i Aw + j) + c the offset c (0: x, 1: y) of anchor (i, j).
 *             The (6 + 2 Ah Aw)^2 system A, b is assembled from the blocks, cells ascending, every entry starting at +0.0; every
 *             anchor unknown k is regularised with wgt = (anchor_weight (double) n_p) / (double) N: A[k][k] += wgt wgt, b[k] += (wgt
 *             wgt) f_k.  That is the shape of Open3D's non_rigid_anchor_point_weight term (default 0.316) as far as we know; it
 *             could NOT be checked against Open3D here.  x = solve(A, -b) on the symmetrised A; E' = D(x[0:6]) E with the D of
 *             "Colour-map optimisation"; f += x[6:].  An anchor that no pair touches keeps f = 0 through the regulariser alone; with
 *             wgt = 0 the system is then singular and the pose does not move (COLORMAP_SINGULAR, as in the rigid update).
 * stin_nonrigid_accumulate_f64: one batch of poses into sum / count / seen (ACCUMULATED INTO); flow: the batch's [B][Ah][Aw][2];
 *     camera: HOST array of STIN_COLORMAP_CAMERA_DOUBLES doubles; route as for stin_frames_accumulate_f64.
 * stin_nonrigid_keys_f64 + a sort + stin_nonrigid_normal_f64: one batch of poses -> blocks fp64 [B][cells][120], counts int32
 *     [B][cells] (written, not accumulated).  The key kernel writes one int64 per (pose, vertex) into `keys` (at least
 *     stin_nonrigid_workspace_bytes = 8 N B bytes, exactly): (b cells + cell) << 31 | vertex for a contributing pair, INT64_MAX
 *     otherwise.  The CALLER sorts the B N keys ascending (any sort: the keys are distinct) and hands them to
 *     stin_nonrigid_normal_f64 with the same poses, flow and sizes: one workgroup of 128 threads per (pose, cell) finds its run of
 *     keys by binary search, stages up to 128 pairs' (J, r) in LDS at a time, one pair per thread, and 120 threads add one product
 *     each over the staged pairs in order.  B cells < 2^31 - 1, H, W in [2, STIN_FRAMES_MAX_SIZE], lattice_step >= 1, margin >= 1
 *     (>= 0 for the accumulate), z_near > 0, N < 2^31 - 1, B <= STIN_FRAMES_MAX_BATCH (STIN_E_SIZE otherwise; the workspace size is
 *     0 then).  N = 0: blocks of +0.0.  Keys that were not made from the same inputs give unspecified sums, never a wild access.
 * Null pointers are allowed where a count is 0.  Nothing allocates or synchronises. */
#define STIN_NONRIGID_BLOCK_DOUBLES 120
#define STIN_NONRIGID_LOCAL 14
int stin_nonrigid_accumulate_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                                 const uint8_t* color, int H, int W, const double* flow, int lattice_step, const double* camera,
                                 double z_near, const uint32_t* bits, int64_t words, int margin, int route, int64_t* sum,
                                 int32_t* count, uint32_t* seen, int64_t seen_words, stin_stream_t stream);
size_t stin_nonrigid_workspace_bytes(int64_t N, int B, int H, int W, int lattice_step);
int stin_nonrigid_keys_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                           int H, int W, const double* flow, int lattice_step, const double* camera, double z_near,
                           const uint32_t* bits, int64_t words, int margin, void* keys, size_t keys_bytes, stin_stream_t stream);
int stin_nonrigid_normal_f64(const double* vertices, int64_t N, const double* RT, const uint8_t* valid, int B, int64_t first_pose,
                             const int32_t* images, int H, int W, const double* flow, int lattice_step, const double* camera,
                             double z_near, int margin, const double* proxy, const void* sorted_keys, size_t keys_bytes,
                             double* blocks, int32_t* counts, stin_stream_t stream);

/* Non-rigid solve: the update's linear solve on the device (stin_nonrigid_solve.hip) - one banded-arrow Cholesky per pose on the
 * blocks that stin_nonrigid_normal_f64 wrote, so that an iteration reads back x instead of the blocks; preprocessing.nonrigid_solve,
 * optimize_poses_nonrigid(solver='banded').  A SECOND solver beside the host's np.linalg.solve ('dense', the default, unchanged):
 * the two agree to rounding, not in bytes, hence a contract of its own.  tests/_nonrigid_solve_oracle.py restates it in numpy
 * (dense storage, left-looking, plain loops) and agrees byte for byte.  Everything is fp64 and IEEE, every operation in the order
 * and association written, nothing contracted and no fma; `/` and sqrt are the correctly rounded operations, never a multiplication
 * by a reciprocal; integers where stated.
 *
 *   inputs    per pose p: blocks[p] fp64 [cells][120] and counts[p] int32 [cells] as stin_nonrigid_normal_f64 writes them; flow[p]
 *             fp64 [Ah][Aw][2]; valid[p], free[p] bytes; the scalars n_vertices (int64), anchor_weight (fp64), min_pairs (int64).
 *   poses     pairs[p] = the integer sum of counts[p] (int64).  residual[p] = ((+0.0 + blocks[p][0][119]) + blocks[p][1][119]) + ..,
 *             cells ascending - written for EVERY pose.  A pose is SOLVED iff free && valid && pairs >= min_pairs; free && valid but
 *             pairs < min_pairs: status STIN_NONRIGID_FEW_PAIRS.  A pose that is not solved gets an x row of +0.0.
 *   assembly  that of "Non-rigid colour-map optimisation", update: unknown k < 6 the pose's, 6 + 2 (i Aw + j) + c the offset c of
 *             anchor (i, j); a cell's 14 local unknowns are the pose's six and the offsets of its anchors (ci, cj), (ci, cj + 1),
 *             (ci + 1, cj), (ci + 1, cj + 1); entry t of a block, t < 105, is the t-th pair (a, b), a <= b, of the row-major upper
 *             triangle of the 14 x 14 and is added to A[g(a)][g(b)] (g ascending in a cell: the upper triangle), entry 105 + a to
 *             b[g(a)]; every target starts at +0.0 and takes its cells in ASCENDING cell number: acc = acc + entry.  Then
 *             wgt = (anchor_weight (double) pairs) / (double) n_vertices, w2 = wgt wgt, and for every anchor unknown k (f_k its
 *             offset in flow[p], flattened): A[k][k] = A[k][k] + w2, b[k] = b[k] + w2 f_k.  A is symmetric: A[j][i] = A[i][j].
 *             These are the numbers the host update builds, bit for bit.  On the device a GATHER: one thread per stored entry
 *             adds the at most four cells that hold both its anchors, the 21 + 6 pose entries add all cells; no atomics.
 *   ordering  the pose LAST: q = [6 .. n - 1, 0 .. 5], M[i][j] = A[q_i][q_j], r_i = -b[q_i] (a negation: -(+0.0) is -0.0).
 *             m = 2 Ah Aw, n = m + 6, w = 2 Aw + 3.  Envelope: lo(i) = max(0, i - w) for i < m, lo(i) = 0 for the six border rows:
 *             anchors that share a cell differ by at most Aw + 1, their unknowns by at most w, so M is zero outside it.
 *   factor    M = L L^T over the envelope.  For i ascending, j = lo(i) .. i ascending:
 *                 t = M[i][j];  for k = max(lo(i), lo(j)) .. j - 1 ascending: t = t - L[i][k] L[j][k];
 *                 j < i: L[i][j] = t / L[j][j];   j = i: !(t > 0) -> the pose is STIN_NONRIGID_SINGULAR, else L[i][i] = sqrt(t).
 *             Structural zeros inside the envelope take part like every other entry (that fixes the signs of zeros).  A
 *             right-looking factorisation gives every entry the same subtractions in the same ascending pivot order: the kernel is
 *             right-looking, the restatement left-looking, the bytes are the same.
 *   forward   y: t = r_i; for k = lo(i) .. i - 1 ascending: t = t - L[i][k] y_k; y_i = t / L[i][i] - the arithmetic of one more
 *             border row, and implemented as one.
 *   backward  for i descending: t = y_i; for k = n - 1 down to i + 1, those with lo(k) <= i: t = t - L[k][i] x_k;
 *             x_i = t / L[i][i] - what a column-oriented sweep produces.
 *   finish    x is un-permuted (x[q_i] = x_i).  Any component not finite: STIN_NONRIGID_SINGULAR.  A SINGULAR pose's x row is +0.0.
 *             No loop bound and no barrier depends on a data value: on the device a failed pivot sets a flag and the arithmetic
 *             runs on; a NaN or infinite block ends as SINGULAR like any other input and leaves the other poses alone.
 *   versus 'dense'   LAPACK's LU moves a pose whose matrix is indefinite but non-singular, Cholesky reports it SINGULAR; J^T J plus
 *             a non-negative diagonal is never indefinite in exact arithmetic.  An anchor that no pair touches under anchor_weight = 0
 *             is SINGULAR under both (the pivot is exactly 0).
 * stin_nonrigid_solve_f64: B poses in three launches - per pose the pair count, residual and status; the gather into band storage
 *     [B][m][w + 1] (row i, column c: M[i][i - w + c]) and border storage [B][7][n] (the pose's six rows of M, then r); one
 *     workgroup of 256 threads per pose that factors and solves in place through a window of w + 1 band rows and the border's 7 rows
 *     over the same columns in LDS: ((w + 1)(w + 8) + 42 + w + 7) doubles, 19.8 KB at Aw = 21 and 63.5 KB at Aw = 41, within the
 *     64 KB a workgroup gets without raising a limit - hence Aw <= STIN_NONRIGID_SOLVE_MAX_AW = 41 (step 16 at 640 pixels); Ah is
 *     free (the window does not grow with it).  Outputs: x fp64 [B][n] in the ORIGINAL order of the unknowns, residual fp64 [B],
 *     pairs int64 [B], status int32 [B] (WRITTEN: FEW_PAIRS / SINGULAR of this call only).  The workspace
 *     (stin_nonrigid_solve_workspace_bytes; 8-byte aligned) holds the factor afterwards.  Ah >= 2, 2 <= Aw <= 41, Ah Aw < 2^22,
 *     0 <= B <= STIN_NONRIGID_SOLVE_MAX_BATCH: otherwise the workspace size is 0 and the call returns STIN_E_SIZE.  B = 0: nothing
 *     is launched.  Nothing allocates or synchronises.
 * stin_nonrigid_solve_stages_f64: the same with `stages`, 0 = all, else a mask of STIN_NONRIGID_SOLVE_STAGE_*: only those kernels
 *     are launched, on what earlier calls left in the workspace (for per-stage timing, profiles/nonrigid_solve.py; the outputs are
 *     defined for 0 only.  No kernel's loop bounds depend on the values, so a stage's time is its time in a whole call). */
#define STIN_NONRIGID_FEW_PAIRS 4
#define STIN_NONRIGID_SINGULAR 8
#define STIN_NONRIGID_SOLVE_MAX_AW 41
#define STIN_NONRIGID_SOLVE_MAX_BATCH 65535
#define STIN_NONRIGID_SOLVE_STAGE_STATS 1
#define STIN_NONRIGID_SOLVE_STAGE_ASSEMBLE 2
#define STIN_NONRIGID_SOLVE_STAGE_FACTOR 4
size_t stin_nonrigid_solve_workspace_bytes(int B, int Ah, int Aw);
int stin_nonrigid_solve_f64(const double* blocks, const int32_t* counts, const double* flow, const uint8_t* valid,
                            const uint8_t* free_, int B, int Ah, int Aw, int64_t n_vertices, double anchor_weight, int64_t min_pairs,
                            double* x, double* residual, int64_t* pairs, int32_t* status, void* workspace, size_t workspace_bytes,
                            stin_stream_t stream);
int stin_nonrigid_solve_stages_f64(const double* blocks, const int32_t* counts, const double* flow, const uint8_t* valid,
                                   const uint8_t* free_, int B, int Ah, int Aw, int64_t n_vertices, double anchor_weight,
                                   int64_t min_pairs, double* x, double* residual, int64_t* pairs, int32_t* status, void* workspace,
                                   size_t workspace_bytes, int stages, stin_stream_t stream);

/* Render: colour, depth and face-id images of a vertex-coloured mesh from the camera poses of a scan (stin_render.hip on stin_raster.hip) - the
 * direction the two sections above lack, mesh -> images.  It stands in for what the reference shows in an Open3D window
 * (utils/ColorCompletionVisualizer.py: unlit vertex colours, a screenshot key) on machines without a display; it is a contract of the
 * project's own, NOT pinned against Open3D's renderer.  tests/_render_oracle.py restates it in numpy (per pose and per pixel over all
 * faces) and agrees bit for bit.  Everything is fp64 and IEEE, the operations in the order written, nothing contracted; integers where
 * stated.
 *
 *   poses     RT [P][12], valid [P]: preprocessing.pose_extrinsics' output (see "Observer masks").  An invalid pose renders the
 *             background only.
 *   view      xv = ((R00 x + R01 y) + R02 z) + t0, likewise yv, zv (the observers' expression).
 *   screen    X = fx xv / zv + cx, Y = fy yv / zv + cy: the projection and the camera (fx, fy, cx, cy) of "Frame colours", a real
 *             pinhole; pixel (row i, column j) is centred at (X, Y) = (j, i); the image is H x W, H != W allowed.
 *   cull, coverage, depth key   those of "Observer masks", word for word, with (W - 1, H - 1) where it has S - 1: a face is skipped
 *             for a pose when a corner has zv < z_near (DROPPED, not clipped), an index is outside [0, N), a screen coordinate is not
 *             finite, or area2 = edge(a, b, c) is 0; wa = edge(b, c, pix), wb = edge(c, a, pix), wc = edge(a, b, pix), covered when all
 *             three are >= 0 (area2 > 0) or all <= 0 (area2 < 0); la = wa / area2, lb, lc likewise;
 *             zp = 1.0 / ((la / za + lb / zb) + lc / zc); key = bits(float32(zp)) << 32 | face id; the pixel keeps the MINIMUM key
 *             (64-bit integer atomicMin).
 *   resolve   per (pixel, pose), with the winning face: la, lb, lc, zp recomputed from the stored screen coordinates;
 *     colour  qa = (la / za) zp, qb = (lb / zb) zp, qc = (lc / zc) zp (perspective-correct weights);
 *             val_k = (qa Ca_k + qb Cb_k) + qc Cc_k, C = vertex colours float32 [N][K], 1 <= K <= 4, promoted to fp64;
 *             color_f32 = float32(val_k); color_u8 = (uint8) rint(t 255.0), t = (double) color_f32, t = 0 when !(t > 0) (so NaN
 *             gives 0), t = 1 when t > 1.
 *     depth   uint16: mm = rint(zp depth_scale), stored when it is finite and 0 < mm < 65535, else 0 - the raw format "Frame
 *             colours" reads.
 *     face    int32: the winning face id, or -1.
 *             A pixel nobody covers gets background[K] (floats, quantised by the same rule for color_u8), depth 0 and face -1.
 * stin_render_poses_f64: poses in batches of `batch` (1 .. STIN_RENDER_MAX_BATCH) whose keys (batch H W 8 bytes, plus one resolve
 *     tile) and screen coordinates (batch N 24 bytes) live in the workspace.  Per batch: clear, transform every vertex once, rasterise
 *     with one thread per (face, pose) - the clamped box is formed first, a face outside the frustum costs six loads - and resolve.  A
 *     face whose clamped box holds more than large_box centres (<= 0: STIN_RENDER_LARGE_BOX, measured in profiles/r26_render.md)
 *     goes through a queue to a second rasteriser that spreads it over a wavefront; at a scan's frame sizes that is the main route.
 *     The images depend neither on batch, nor on large_box, nor on how the work is split.  camera: HOST array of
 *     STIN_RENDER_CAMERA_DOUBLES doubles (fx, fy, cx, cy); background: HOST array of K floats (both read during the call).
 *     Outputs color_f32 [P][H][W][K], color_u8 [P][H][W][K], depth [P][H][W], face_ids [P][H][W]; every one may be NULL.  The
 *     resolve pass stages 512 consecutive pixels of the flattened arrays per workgroup in LDS and streams them out 16 bytes per
 *     lane where the array's base is 16-byte aligned (by element otherwise): 3- and 12-byte pixels need no alignment of their own.
 *     stages: 0 = all; else a mask of STIN_RENDER_STAGE_* - only those kernels are launched, on what earlier calls left in the
 *     workspace (for per-stage timing, profiles/render.py; the images are defined for 0 only).
 *     H, W <= STIN_RENDER_MAX_SIZE, N, F, P < 2^31 - 1, z_near > 0, depth_scale > 0 (STIN_E_SIZE otherwise).  *status (device
 *     int32, written): STIN_RENDER_BAD_INDEX - a face had an index outside [0, N) (it is skipped, the others are unaffected);
 *     STIN_RENDER_LARGE_FACE - informational: a face went through the large-face rasteriser.  Null pointers are allowed where a
 *     count is 0.  Nothing allocates or synchronises. */
#define STIN_RENDER_BAD_INDEX 1
#define STIN_RENDER_LARGE_FACE 2
#define STIN_RENDER_LARGE_BOX 32
#define STIN_RENDER_MAX_SIZE 4096
#define STIN_RENDER_MAX_BATCH 1024
#define STIN_RENDER_CAMERA_DOUBLES 4
#define STIN_RENDER_STAGE_CLEAR 1
#define STIN_RENDER_STAGE_TRANSFORM 2
#define STIN_RENDER_STAGE_RASTER 4
#define STIN_RENDER_STAGE_LARGE 8
#define STIN_RENDER_STAGE_RESOLVE 16
size_t stin_render_workspace_bytes(int64_t N, int64_t F, int H, int W, int batch);
int stin_render_poses_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const float* colors, int K,
                          const double* RT, const uint8_t* valid, int64_t P, const double* camera, int H, int W, double z_near,
                          double depth_scale, const float* background, int batch, int64_t large_box, int stages, float* color_f32,
                          uint8_t* color_u8, uint16_t* depth, int32_t* face_ids, int32_t* status, void* workspace,
                          size_t workspace_bytes, stin_stream_t stream);

/* View metrics: PSNR and SSIM (Wang et al. 2004) of two sets of rendered views, prediction against ground truth, per pose
 * (stin_view_metrics.hip) - what an evaluation run asks of the images "Render" makes, without reading them back.  A contract of the
 * project's own: it is NOT pinned against skimage or piq.  The window has INTEGER taps; there is no padding, no luma conversion and
 * no multi-scale SSIM.  Every quantity that is summed is an integer, so the table is the same bytes for every tiling, batch size and
 * launch order; no float atomics.  tests/_viewmetrics_oracle.py restates it in numpy (one 121-tap sum per window) and agrees
 * byte for byte.
 *
 *   inputs    a, b uint8 [P][H][W][K], 1 <= K <= 4; covered, region uint8 [P][H][W], each optional: NULL = every pixel is covered /
 *             in the region.  A pixel is covered when covered != 0 and in the region when region != 0.
 *   pixels    per pose, over the pixels that are covered and in the region: n_pix their number, sum_abs = sum_k |a - b|,
 *             sum_sq = sum_k (a - b)^2.
 *   window    11 x 11, separable, taps w = {67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67}: the Gaussian of
 *             sigma 1.5 scaled to 2^16 and rounded, the centre tap raised by 1 so that they sum to 65536; the 2-D weight
 *             w[i] w[j] sums to 2^32.  A window counts for its pose when all 121 pixels lie inside the image ('valid' mode), all 121
 *             are covered, and its CENTRE pixel is in the region.
 *   moments   per counted window and channel, exact integers: Sa = sum w a, Sb = sum w b, Saa = sum w a^2, Sbb = sum w b^2,
 *             Sab = sum w a b (a 1-D row sum is below 2^32, a 2-D sum below 2^48).
 *   value     fp64, IEEE, in the order written, nothing contracted: s = 2^-32; ma = Sa s; mb = Sb s; va = Saa s - ma ma;
 *             vb = Sbb s - mb mb; c = Sab s - ma mb;
 *             v = ((2.0 ma mb + C1) (2.0 c + C2)) / ((ma ma + mb mb + C1) (va + vb + C2)), C1 = 6.5025 = (0.01 255)^2,
 *             C2 = 58.5225 = (0.03 255)^2;  q = (int64) rint(v 2^32), ties to even.
 *             n_win = the pose's counted windows, ssim_q = sum of q over them and the channels.
 *   table     int64 [P][STIN_VIEW_METRICS_COLS] = n_pix, sum_abs, sum_sq, n_win, ssim_q.  Written by the call: the caller need not
 *             clear it.  (In [0, 1] colour units: l1 = sum_abs / (255 K n_pix), mse = sum_sq / (255^2 K n_pix),
 *             ssim = ssim_q / (2^32 K n_win): views.view_metrics.)
 * stin_view_metrics_u8: one kernel.  A workgroup owns 16 x 32 window corners of one pose; it stages their 26 x 42 pixels of a, b and
 *     the masks in LDS with 16-byte loads of the 16-byte lines the rows lie in (a line that is not wholly inside its array goes by
 *     element, so no byte outside an array is read and no base or row needs an alignment), makes the horizontal pass of one channel
 *     at a time into five uint32 planes, the vertical pass in 64-bit registers, evaluates v and q, counts a window's covered pixels
 *     as an integer box sum that must be 121, sums the tile's own 16 x 32 pixels, reduces in integers and adds the five figures to
 *     the pose's row with one 64-bit integer atomic each.
 *     H, W in [1, STIN_RENDER_MAX_SIZE] (below 11: n_win = 0), 0 <= P < 2^31 - 1, 1 <= K <= 4 (STIN_E_SIZE otherwise); a, b, table
 *     missing with P > 0: STIN_E_NULL.  stin_view_metrics_workspace_bytes is 0 today (and for sizes out of range): workspace may be
 *     NULL.  Nothing allocates or synchronises. */
#define STIN_VIEW_METRICS_COLS 5
#define STIN_VIEW_METRICS_WINDOW 11
size_t stin_view_metrics_workspace_bytes(int64_t P, int H, int W, int K);
int stin_view_metrics_u8(const uint8_t* a, const uint8_t* b, const uint8_t* covered, const uint8_t* region, int64_t P, int H, int W,
                         int K, int64_t* table, void* workspace, size_t workspace_bytes, stin_stream_t stream);

/* ------------------------------------------------- 2-D image-graph inpainting experiment --
 * What the reference's ImageGraphTextureDataSet builds per item on CPU workers (datasets/imagegraph_dataloader.py:46-160) and what
 * the graph branch of its 2-D trainer reads back per step (trainers/inpainting2d_trainer.py:382-398, without lpips), stin_image.hip.
 *
 * stin_grid_levels_i64: the grid graph and the "fake traces" of B images of side S over L levels (side of level l: S >> l; S must be
 *     divisible by 2^(L-1), L <= STIN_GRID_MAX_LEVELS, B S S < 2^31), one launch.  `out` (int64, out_elems >=
 *     stin_grid_levels_elems(B, S, L); that query returns 0 for an unsupported shape) holds, in this order:
 *       for l = 0 .. L-1:  edges of level l [2][B E_l], E_l = 4 s (s - 1), row 0 = source; then, for l >= 1, the trace of level l
 *                          [B sf sf], sf = side of level l - 1: trace[b sf sf + r sf + c] = b sc sc + (r / 2) sc + (c / 2);
 *       batch [B S S] (image of every level-0 vertex).
 *     Edge order (the reference iterates a Python set: its order means nothing): image-major, then the source vertex in row-major
 *     order, then its neighbours up, left, right, down (those that exist); image b's ids are offset by b s s (the increments of
 *     HierarchicalData.__inc__).  num_vertices: int32 [B][L] = s_l^2.
 * stin_image_samples_u8: one launch builds B samples from resident raw H x W x 3 uint8 images (pool: device bytes, any alignment).
 *     records: int64 [B][STIN_IMAGE_RECORD_HEAD + 2 num_circles] on the device = pool byte offset, h, w, k (rotation, 0..3), flip
 *     (0 / 1), then (row_start, col_start) of every circle window.  Pixel pipeline of the training recipe: v = fl32(u8) fl32(1 / 255),
 *     v 2 - 1 in fp32 (Normalize); centre crop at h0 = (h - S) / 2, w0 = (w - S) / 2 (CenterCrop); np.rot90(img, k) (RandomRotation:
 *     ndimage.rotate by 90 k degrees is that, bit for bit, on a square image); flip along axis 1 (RandomFlip).  mask = OR over the
 *     windows of the template (r - R)^2 + (c - R)^2 <= R^2 on [0, 2R)^2.  Outputs: color [B S S][3] f32, mask [B S S] bytes (0 / 1),
 *     x [B S S][4] f32 = (color * !mask, mask), 16-byte aligned.  Rescale (cv2.INTER_AREA) is NOT part of this call: the caller
 *     guarantees min(h, w) == S, every window inside the image and every image inside the pool (the host wrapper raises
 *     otherwise); a pixel whose source bytes fall outside [0, pool_bytes) is written as 0, never read.
 * stin_image_metrics_f32: the 2-D trainer's step metrics as ONE row of 8 floats of a caller-owned device table.  N = num_images
 *     n rows, image b = rows [b n, (b + 1) n).  P = composite ? where(mask, out, color) : out, d = P - color in fp32:
 *       row_out[0] loss  loss[0] when loss != NULL, else row_out[1]
 *       row_out[1] l1    sum |d| / (N C)
 *       row_out[2] mse   sum d^2 / (N C)
 *       row_out[3] psnr  piq's: the MEAN over the images of -10 log10(mse_b / data_range^2 + 1e-8) (not the whole-batch value of
 *                        stin_inpaint_metrics_f32)
 *       row_out[4] number of rows with mask != 0 (exact: N <= 2^24);  row_out[5..7] = 0
 *     out [N, C] fp32 with leading dimension ldo, color [N, C] contiguous, mask bytes [N] (a bool tensor's storage), C = 1 .. 4.
 *     fp64 block partials per image, folded in a fixed order by the finaliser: same bits on every run, no float atomics.
 *     Workspace: stin_image_metrics_workspace_bytes(N, num_images).  Nothing allocates or synchronises. */
#define STIN_GRID_MAX_LEVELS 8
#define STIN_IMAGE_RECORD_HEAD 5
int64_t stin_grid_levels_elems(int B, int S, int L);
int stin_grid_levels_i64(int B, int S, int L, int64_t* out, int64_t out_elems, int32_t* num_vertices, stin_stream_t stream);
int stin_image_samples_u8(const uint8_t* pool, int64_t pool_bytes, const int64_t* records, int B, int S, int R, int num_circles,
                          float* x, float* color, uint8_t* mask, stin_stream_t stream);
size_t stin_image_metrics_workspace_bytes(int64_t N, int num_images);
int stin_image_metrics_f32(const float* out, int64_t ldo, const float* color, const uint8_t* mask, int64_t N, int num_images, int C,
                           int composite, float data_range, const float* loss, float* row_out, void* workspace,
                           size_t workspace_bytes, stin_stream_t stream);

/* ------------------------------------------------------------------------------- Image resize --
 * What the reference asks cv2.resize for: colour frames to the depth size (preprocessing/texture_map_optimization.py:93, the
 * default = bilinear) and Rescale of the 2-D experiment (datasets/imagegraph_dataloader.py:215, INTER_AREA), stin_resize.hip.
 *
 * Images are uint8, row-major [H, W, C], C = 1, 3 or 4.  A source H x W becomes h x w; every side lies in
 * [1, STIN_RESIZE_MAX_SIDE].  Integer arithmetic only: the result does not depend on batching, tiling or route.
 *
 * STIN_RESIZE_LINEAR: bilinear with half-pixel centres and 11-bit coefficients, for enlarging and for reducing (no
 *     antialiasing).  Per axis, for output index d of n_out from n_in:
 *         num = (2 d + 1) n_in - n_out,  den = 2 n_out,  s = floor(num / den) (floor also for num < 0),  r = num - s den,
 *         b = (4096 r + den) / (2 den) (integer division: round(2048 frac), halves up),  a = 2048 - b;
 *         s < 0: s = 0, b = 0;   s >= n_in - 1: s = n_in - 1, b = 0;   second tap = min(s + 1, n_in - 1).
 *     With (sy, ay, by) of the row, (sx, ax, bx) of the column and v00 .. v11 the four taps (first index: row tap):
 *         out = (ay (ax v00 + bx v01) + by (ax v10 + bx v11) + 2^21) >> 22
 *     - one rounding; every term fits in int32.  Equal sizes give the input back byte for byte.
 *     |out - exact bilinear| <= 0.5 + 255 (2^-12 + 2^-12 + 2^-24) < 0.625: within one grey level of any correctly rounded
 *     bilinear resize with half-pixel centres.  That is what cv2.resize does on 8-bit images to our knowledge; it is NOT pinned
 *     against a run of cv2.
 * STIN_RESIZE_AREA: the exact area average; h <= H and w <= W (cv2 switches to a bilinear variant when enlarging, which is not
 *     restated: such a job is unsupported - see below for what the library, which sees the table on the device only, does).  With ox(j, x) = max(0, min((x + 1) w, (j + 1) W) - max(x w, j W)) the overlap of
 *     source column x with output column j in units of 1 / w of a source pixel, oy(i, y) the same with h, H:
 *         S = sum_y sum_x oy(i, y) ox(j, x) v[y, x],   out = (2 S + W H) / (2 W H)   (integer division: halves up)
 *     S reaches 255 * 2^28: the sums are 64-bit.  Not pinned against cv2.INTER_AREA either.
 * The reference applies Rescale after Normalize, on float32; here it runs on the bytes, which differs by at most half a grey level.
 *
 * stin_resize_u8: J jobs in one launch.  jobs: int64 [J][STIN_RESIZE_JOB_WORDS] on the device = src_off, H, W, dst_off, h, w:
 *     the source image starts at byte src_off of `src` (src_bytes long), the result at byte dst_off of `dst` (dst_bytes long); any
 *     alignment, the jobs may be of different sizes (a pool of images) or equal (a [B, H, W, C] batch).  The table is read on the
 *     device only: a job with a side outside [1, STIN_RESIZE_MAX_SIDE], an image that does not lie inside its buffer, or AREA with
 *     h > H or w > W writes NOTHING (the host wrappers raise before the launch); no byte outside [dst_off, dst_off + h w C) of a job
 *     is written and no byte outside `src` is read.  Results of jobs must not overlap each other or `src`.
 *     Source rows are staged through LDS with 16-byte loads, results leave as 16-byte stores where the address allows; the
 *     per-column coefficients / overlaps are formed once per block and column, the per-row ones once per block and row.  A
 *     footprint of any size (2000 rows to 3) is a loop over source rows and column chunks.  No workspace, no allocation, no
 *     synchronisation, no float, no atomics.  J <= 0, channels not in {1, 3, 4}, an unknown mode: STIN_E_SIZE. */
#define STIN_RESIZE_MAX_SIDE 16384
#define STIN_RESIZE_JOB_WORDS 6
#define STIN_RESIZE_LINEAR 0
#define STIN_RESIZE_AREA 1
int stin_resize_u8(const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* jobs, int J, int channels,
                   int mode, stin_stream_t stream);

/* ------------------------------------------------------------------------------- Surface samples --
 * Area-uniform points on a triangle mesh, thinned to a minimum spacing, as centres of the circle masks (stin_surface.hip): the
 * sampler the reference's process_frame_circles planned (preprocessing/observed_texture_map_generation.py:545-562, "TODO: Sample
 * using poisson disk") and replaced by a uniform draw over vertex ids.  A contract of the project's own: NOT pinned against Open3D's
 * sample_points_poisson_disk (weighted sample elimination); spacing is Euclidean, not geodesic.  tests/_surface_oracle.py restates
 * it in numpy and agrees bit for bit.  All arithmetic is fp64, every product and sum rounded once (no contraction).
 *
 * Face weights (stin_surface_weights_f64).  vertices [N, 3] fp64, faces [F, 3] int64, F <= STIN_SURFACE_MAX_FACES.  e1 = b - a, e2 = c - a;
 *     nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz = e1x e2y - e1y e2x;  A2 = sqrt((nx nx + ny ny) + nz nz) (IEEE sqrt).
 *     A face with an index outside [0, N) (flag bit 0; nothing is read through it) or a non-finite A2 (flag bit 1: a non-finite
 *     vertex, or an overflow) has A2 = 0.  Amax = max A2 (an integer maximum of bit patterns: order-free), (_, e) = frexp(Amax),
 *     W_f = (int64) floor(ldexp(A2_f, 40 - e)) < 2^40; all W = 0 when Amax = 0.  cum [F] int64 = the inclusive scan of W (integers:
 *     the same bytes on any schedule), T = cum[F - 1] < 2^62.  A face that repeats a vertex has e1, e2 or e1 - e2 = 0,
 *     hence A2 = 0 exactly: it is never drawn, which is the rule of stin_qem_remap_faces_i64 (such faces are dropped).
 *     state: 4 x int64 DEVICE words written by the call: [0] bits of Amax, [1] flags, [2] T, [3] 0.
 *     Workspace >= stin_surface_weights_workspace_bytes(F).
 * Samples (stin_surface_sample_f64).  With mix64 the finaliser of the circle masks' hash (splitmix64), G = 0x9E3779B97F4A7C15 and
 *     uint64 wrap arithmetic:  base = mix64(seed + G),  r_k = mix64(base + (3 (first + i) + k) G), k = 0, 1, 2.
 *         face   u = (r_0 T) >> 64 (the high word of the 128-bit product), f = the first face with cum[f] > u
 *         point  x1 = (r_1 >> 11) 2^-53, x2 = (r_2 >> 11) 2^-53, s = sqrt(x1);  b0 = 1 - s, b1 = s (1 - x2), b2 = s x2;
 *                p = (b0 a + b1 b) + b2 c per component
 *     Sample i depends on (seed, first + i) only: a stream can be extended or split over launches with the same bytes.  Outputs:
 *     points [n, 3] fp64, face [n] int64, bary [n, 3] fp64.  T = 0 (no positive weight): flag bit 2 is OR-ed into state[1] and
 *     nothing is written.  state is the array stin_surface_weights_f64 wrote.
 *
 * Poisson-disk subset in index order.  Candidate i of points [C, 3] fp64 is accepted iff no accepted j < i has
 *     d2(i, j) = (dx dx + dy dy) + dz dz < r2 = r r (strict).  The accepted set is the unique sequential-greedy one, and every
 *     prefix of it is the result for the same prefix of candidates.
 *     Grid (stin_poisson_grid_f64): origin o = the component-wise minimum, cell edge h = r (1 + 2^-20), cell = floor((p - o) / h)
 *     per axis, three 21-bit cells in one key (x highest), a stable radix sort of (key, index): order [C] int32 = the indices in
 *     key order, ascending inside a cell.  runs [C][18] int32: for candidate i the nine ranges [beg, end) of `order` that hold the
 *     cells (cx + dx, cy + dy, cz - 1 .. cz + 1), dx, dy in {-1, 0, 1} (three consecutive keys each).  decided [C] bytes = 0.
 *     state: 8 x int64 DEVICE words: [0..2] / [3..5] the minimum / maximum per axis as order-preserving integer keys (sign bit
 *     flipped for v >= 0, all bits for v < 0), [6] flags: bit 0 a non-finite candidate, bit 1 more than 2^21 cells along an axis;
 *     with a flag set the runs are empty and the caller must not go on.  Workspace >= stin_poisson_grid_workspace_bytes(C).
 *     Why the 27 cells suffice, i.e. why the grid cannot change the result: a pair with computed d2 < r2 has dx dx < r2 (1 + 2 eps),
 *     so the exact |p_i - p_j| < r (1 + 4 eps) on each axis, eps = 2^-53, allowing for the rounding of dx itself.  The exact
 *     quotients (p - o) / h of the two therefore differ by less than (1 + 4 eps) / (1 + 2^-20) < 1 - 2^-21.  A computed quotient
 *     (one rounded subtraction, one rounded division) is off by at most 2 eps q <= 2^21 2^-52 = 2^-31 for q < 2^21.  The computed
 *     quotients hence differ by less than 1 - 2^-21 + 2^-30 < 1, and their floors by at most 1.
 *     Rounds (stin_poisson_rounds_f64): `rounds` (1 .. 64) launches of one decision round.  decided[i]: 0 undecided, 1 accepted,
 *     2 rejected.  An undecided i scans its conflicting j < i: one accepted -> rejected; else one undecided -> i waits; else
 *     accepted.  States only move from undecided to the value they have in the greedy set, so a thread may read states written in the
 *     same round (relaxed agent-scope byte loads and stores): that changes how many rounds are needed, never the result.
 *     remaining [rounds] int64 DEVICE words: the candidates still undecided after each round.  The lowest undecided index always
 *     decides, so C rounds are enough for any input; the host loops until a remaining count is 0.  No kernel waits for another
 *     workgroup.
 *
 * stin_first_occurrence_i64: keep[i] = 1 iff i is the lowest position with the value ids[i] (ids [n] int64 in [0, N); an integer
 *     atomicMin per value into first_pos [N] int64, then one compare): a stream of vertex ids without its repeats, in stream order.
 *     *bad (device int32) = 1 when an id lies outside [0, N) (keep = 0 there).
 *
 * Circle masks on surface samples (preprocessing.circle_masks_on_surface; host loop over the calls above, stin_nearest_f64 and
 *     stin_circle_mask_run with given centres): mask m draws its centre stream with the seed
 *         seed_m = mix64(mix64(seed + G) + (m + 1) G)
 *     and runs the batch rule of stin_circle_mask_run (10 centres, then k = int(total (frac / cur - 1)) until cur >= frac or
 *     k <= 0), each batch taking the next k entries of the stream; a stream with fewer than k entries left gives what it has
 *     and the mask ends `exhausted`.  Radii are hop counts, as before. */
#define STIN_SURFACE_MAX_FACES 4194304
size_t stin_surface_weights_workspace_bytes(int64_t F);
int stin_surface_weights_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, int64_t* cum, int64_t* state,
                             void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_surface_sample_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const int64_t* cum, int64_t n,
                            uint64_t seed, uint64_t first, double* points, int64_t* face, double* bary, int64_t* state,
                            stin_stream_t stream);
size_t stin_poisson_grid_workspace_bytes(int64_t C);
int stin_poisson_grid_f64(const double* points, int64_t C, double radius, int32_t* order, int32_t* runs, uint8_t* decided,
                          int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_poisson_rounds_f64(const double* points, int64_t C, double radius, const int32_t* order, const int32_t* runs,
                            uint8_t* decided, int rounds, int64_t* remaining, stin_stream_t stream);
int stin_first_occurrence_i64(const int64_t* ids, int64_t n, int64_t N, int64_t* first_pos, uint8_t* keep, int32_t* bad,
                              stin_stream_t stream);

/* --------------------------------------------------------------------------- Geodesic distances --
 * Circle masks whose radius is a length along the surface in the units of the vertices, not a hop count (stin_geodesic.hip):
 * shortest paths over the mesh EDGES weighted by their Euclidean length, from many centres at once, cut off at the radius.  This is
 * the Dijkstra metric of the edge graph, NOT the exact polyhedral geodesic (which crosses faces); it is never shorter than that.
 * A contract of the project's own; tests/_geodesic_oracle.py restates it (heap Dijkstra, and Bellman-Ford sweeps) and the device
 * agrees bit for bit.  All arithmetic is fp64, every product and sum rounded once (no contraction), division and sqrt are IEEE.
 *
 * Edge length (stin_geodesic_lengths_f64).  vertices [N, 3] fp64 (float32 input is promoted first); rowptr [N + 1], col [E2] the
 *     int32 CSR of stin_mask_adjacency_i64 (E2 = 2E slots, reused as it is; its row order is unspecified and nothing depends on
 *     it).  length [E2] fp64, slot e of row u with v = col[e]:  d = pos[u] - pos[v],  len = sqrt((dx dx + dy dy) + dz dz).
 *     Symmetric bit for bit (d only changes sign).  flags: one int64 DEVICE word written by the call - bit 0: a length is not
 *     finite (a non-finite vertex, or an overflow), bit 1: col[e] outside [0, N) (nothing is read through it, the slot gets +inf).
 *     A slot whose length is not finite is never relaxed.  One pass, no workspace.
 * Distance.  Instance m with the source set S_m and a cut-off cap > 0 (+inf allowed): D[m][v] = the minimum, over all edge paths
 *     from any source of S_m to v, of the path's length folded from the source outward, ((0 + l1) + l2) + ...  This is the unique
 *     fixed point of D[s] = 0, D[v] = min_u fl(D[u] + len(u, v)) (fp64 addition of non-negative numbers is monotone), so heap
 *     Dijkstra and ANY order of relaxations reach the same bits.  Result: dist[m][v] = D[m][v] where D < cap (strict), +inf
 *     elsewhere - a vertex at exactly cap, an unreachable and an isolated vertex all give +inf.  (Prefix sums are monotone, so not
 *     expanding a vertex with D >= cap changes nothing below cap.)  Duplicate edges, self loops, zero-length edges (coincident
 *     vertices) and repeated sources are legal.
 *     stin_geodesic_begin_f64: dist [M][N] = +inf, then 0 at sources[i] of instance source_instance[i] (int32 [S], or NULL: all
 *         instance 0), which are listed for round 0.  Writes state and prepares the workspace
 *         (>= stin_geodesic_workspace_bytes(N, M); needs M * max(N, 1) < 2^31).
 *     stin_geodesic_rounds_f64: `rounds` (1 .. 4096) launches, rounds first_round, first_round + 1, ... of the call sequence that
 *         stin_geodesic_begin_f64 started (same dist, state, workspace, cap; first_round = rounds launched so far).  A round takes
 *         the vertices listed for it, relaxes their edges (64-bit integer atomicMin on the bit patterns; no float atomics) and
 *         lists every vertex it lowered for the next round (once: a stamp word per (m, v)); a workgroup follows the vertices it
 *         lowered itself for up to `levels` (1 .. 64) levels in LDS before it lists them.  `levels` changes the number of rounds
 *         and the work, never the result.  A round whose list is empty returns at once.  No host synchronisation, no kernel waits
 *         for another workgroup (one last-arrival ticket per round), every in-kernel loop is bounded by its arguments.  N rounds are
 *         enough for any input (a shortest path has fewer than N edges).
 *     state: 4 x int64 DEVICE words - [0] flags: bit 1 a source or instance index out of range (left out), bit 2 the worklist is
 *         not empty after the last round run (= not converged yet); [1] vertices waiting for the next round; [2] rounds that found
 *         work; [3] directed edges relaxed so far (fl(D[u] + len) formed), the schedule's work.
 * Mask value (stin_geodesic_mask_f64).  rings >= 1, 0 < radius < inf, ring = radius / rings:  mask[i] = 0 if dist[i] >= radius,
 *     else min(rings, (int64) ceil((radius - dist[i]) / ring)): a centre gets `rings`, the rim 1, everything outside 0.
 * Circle masks (preprocessing.circle_masks_geodesic; a host loop): circle_masks_on_surface's centre streams, batch rule and info,
 *     with batch b of ALL masks still running in one distance call (one instance per mask) and cap = radius. */
int stin_geodesic_lengths_f64(const double* vertices, int64_t N, const int32_t* rowptr, const int32_t* col, int64_t E2, double* length,
                              int64_t* flags, stin_stream_t stream);
size_t stin_geodesic_workspace_bytes(int64_t N, int num_instances);
int stin_geodesic_begin_f64(const int64_t* sources, const int32_t* source_instance, int64_t S, int64_t N, int num_instances,
                            double* dist, int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_geodesic_rounds_f64(const int32_t* rowptr, const int32_t* col, const double* length, int64_t N, int64_t E2,
                             int num_instances, double cap, double* dist, int first_round, int rounds, int levels, int64_t* state,
                             void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_geodesic_mask_f64(const double* dist, int64_t count, double radius, int rings, int64_t* mask, stin_stream_t stream);

/* --------------------------------------------------------------------------------- Harmonic fill --
 * Harmonic (diffusion, Laplace) inpainting on a graph (stin_harmonic.hip): every masked vertex becomes the weighted mean of its
 * neighbours with the known vertices as boundary values - the zero of the graph Laplacian on the hole, the minimiser of
 * sum_edges w (x_i - x_j)^2 - by Jacobi-preconditioned conjugate gradients in a FIXED order of operations.  A contract of the
 * project's own; tests/_harmonic_oracle.py restates it in numpy and the device agrees bit for bit.  A graph Laplacian with uniform
 * or given (e.g. inverse-length) weights, NOT cotangent weights; one global solve for all holes, zero start.
 * All arithmetic is fp64 and IEEE: every product and every sum is rounded once (no contraction), `/` is the correctly rounded
 * division.  "fold" = a plain left-to-right sum that starts from +0.0.
 *
 * Inputs.  rowptr [N + 1], col [E2] int32: stin_mask_adjacency_i64's CSR as it is (slot order is part of the input: the folds
 *     below follow it).  weight [E2] fp64 aligned with col, or NULL = every weight is exactly 1.0.  values [N, C] float32
 *     (contiguous), 1 <= C <= STIN_HARMONIC_MAX_C, promoted to fp64.  masked [N] uint8, non-zero = to be filled.
 *     A slot with col == row is skipped everywhere; a duplicate slot counts as often as it occurs.  A slot whose col lies outside
 *     [0, N), or a row whose rowptr range is not inside [0, E2], is skipped and sets status bit 2 (nothing is read through it).
 * Reached.  A masked vertex is reached if it has a slot to a known (unmasked) vertex or to a reached masked vertex: the least fixed
 *     point.  stin_harmonic_reach_u8 computes it in rounds over one byte per vertex (0 known, 1 masked, 2 reached; a byte only ever
 *     goes 1 -> 2, so a round may see flags set in the same launch: the fixed point is the same).  first_round == 0 initialises
 *     the bytes and the state table; every round is one ordinary launch, `rounds` (1 .. 64) of them per call; the caller reads
 *     state[3] (vertices reached by the LAST round of the call) and stops when it is 0.  Masked vertices that are never reached
 *     (an isolated vertex, a masked component with no known vertex on its rim) take no part in the solve and receive `fill`.
 * System.  The unknowns are the reached vertices in ascending vertex id, u = 0 .. n_U - 1.  Over the slots of row i in ascending
 *     slot order (self slots skipped):  d_i = fold of w;  b_i = fold of w * v_j over the slots whose j is known;
 *     (A p)_i = d_i * p_i - acc,  acc = fold of w * p_j over the slots whose j is an unknown.  Status bit 0: a weight of a slot of an
 *     unknown's row is not finite or not > 0; bit 1: a known value next to an unknown is not finite (any channel).
 * Inner products.  <a, b>: tile t holds the products a_u * b_u of the unknowns [256 t, 256 t + 256), missing entries +0.0; inside
 *     a tile s[j] += s[j + h] for h = 128, 64, ..., 1 (j < h); the tile sums s[0] are folded in ascending t.  Independent of the
 *     launch geometry.
 * Iteration.  Every channel runs on its own scalars, x = 0 at the start:
 *         r = b,  z = r / d,  p = z,  rz = <r, z>,  bb = <b, b>,  rr = bb;      bb == 0: the channel is DONE with 0 iterations
 *     iteration k:  q = A p,  pq = <p, q>;  if not (pq > 0): the channel STOPS (flag bit 1, breakdown), nothing else changes;
 *         alpha = rz / pq,  x = x + alpha * p,  r = r - alpha * q,  rr = <r, r>,  iterations += 1;
 *         if rr <= (tol * tol) * bb: DONE (flag bit 0);
 *         else  z = r / d,  rzn = <r, z>,  beta = rzn / rz,  p = z + beta * p,  rz = rzn.
 *     A channel that is done or stopped is frozen on the device: later iterations change none of its bytes, so the result does not
 *     depend on how many iterations are launched after it, nor on how they are grouped into calls.
 *     Kernels: two ordinary launches per iteration over one workgroup per tile - the product (forms the new p of a row and of its
 *     neighbours on the fly from z and the old p, ping-pong p buffers, writes the <p, q> tile sums) and the update (x, r, z and the
 *     <r, r>, <r, z> tile sums); every workgroup folds the tile sums itself in the fixed order, so there are no atomics, no
 *     cooperative launch and no grid-wide wait.  stin_harmonic_iterate_f64 launches iterations first_iteration ..
 *     first_iteration + count - 1 (count 1 .. 4096) of the sequence stin_harmonic_setup_f64 started and then refreshes the state
 *     table; no host synchronisation.
 * Output (stin_harmonic_finish_f32).  out [N, C] float32: known rows = the input bit for bit, reached rows = (float) x, unreached
 *     masked rows = fill.  Channels that are neither done nor stopped get flag bit 2 (not converged); their current x is the result.
 * state: STIN_HARMONIC_STATE int64 DEVICE words.  [0] status bits (above); [1] n_U; [2] masked vertices never reached (written
 *     by finish); [3] vertices reached by the last reach round run; [4] masked vertices; [5 .. 7] 0; then 4 words per channel c at
 *     8 + 4 c: iterations, the bits of rr, the bits of bb, flags (bit 0 done, bit 1 breakdown, bit 2 not converged). Words of
 *     channels >= C are 0.
 * Call sequence: reach (until state[3] == 0; the host then knows n_U = state[1]), setup, iterate (any grouping), finish - all with
 *     the same flag, state and workspace (>= stin_harmonic_workspace_bytes(N, E2, n_U, C), 0 = unsupported sizes). */
#define STIN_HARMONIC_MAX_C 16
#define STIN_HARMONIC_STATE 72
size_t stin_harmonic_workspace_bytes(int64_t N, int64_t E2, int64_t n_unknown, int C);
int stin_harmonic_reach_u8(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t E2, const uint8_t* masked, int first_round,
                           int rounds, uint8_t* flag, int64_t* state, stin_stream_t stream);
int stin_harmonic_setup_f64(const int32_t* rowptr, const int32_t* col, const double* weight, int64_t N, int64_t E2,
                            const float* values, int C, const uint8_t* flag, int64_t n_unknown, int64_t* state, void* workspace,
                            size_t workspace_bytes, stin_stream_t stream);
int stin_harmonic_iterate_f64(const double* weight, int64_t N, int64_t E2, int C, int64_t n_unknown, double tol, int first_iteration,
                              int count, int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream);
int stin_harmonic_finish_f32(const float* values, const uint8_t* flag, int64_t N, int64_t E2, int C, int64_t n_unknown, double tol,
                             float fill, float* out, int64_t* state, void* workspace, size_t workspace_bytes, stin_stream_t stream);

/* ------------------------------------------------------------------------------------ Mesh files --
 * The body of a binary PLY file decoded on the device, and the per-face label vote of the Matterport scans (stin_ply.hip).  The
 * header of the file is text and is parsed on the host (scene_io.read_ply_header); what it yields - where an element's records
 * start, how long a record is, where each property sits in it - is the input here.  The file's bytes are uploaded once as they
 * are: `body` [body_bytes] is a DEVICE buffer whose base is 16-byte aligned; `first`, `stride` and every offset may have any
 * alignment.  A contract of the project's own; tests/_ply_oracle.py restates it with numpy structured dtypes and the device
 * agrees byte for byte.  Not pinned against open3d or plyfile themselves (neither is installed here).
 *
 * Both decoders check on the HOST, before any launch, that 0 <= first, 1 <= stride <= STIN_PLY_MAX_STRIDE, 0 <= count <=
 * STIN_PLY_MAX_RECORDS and first + count * stride <= body_bytes (without overflow), and that every field lies inside its record;
 * they return STIN_E_SIZE / _NULL / _ALIGN / _UNSUPPORTED otherwise.  A workgroup owns 256 consecutive records: it copies the
 * 16-byte chunks that cover them into LDS with aligned loads (a chunk that would cross the end of the buffer byte by byte) and
 * takes the fields from there, so no byte outside [0, body_bytes) is read for any input.
 *
 * stin_ply_decode.  `count` records of `stride` bytes from byte `first`, unpacked into typed columns in one launch.  `fields`
 *     is a HOST table of n_fields <= STIN_PLY_MAX_FIELDS rows of STIN_PLY_FIELD_WORDS int64 words:
 *         [0] byte offset of the scalar in the record   [1] its type, STIN_PLY_INT8 .. STIN_PLY_FLOAT64 (the eight PLY scalars)
 *         [2] destination DEVICE pointer (aligned to its element)   [3] destination type, STIN_PLY_TO_*
 *         [4] destination row stride in elements, 1 .. STIN_PLY_MAX_FIELDS   [5] destination column, 0 <= column < row stride
 *     Record r goes to destination[r * row_stride + column].  Multi-byte scalars are little endian, or big endian with
 *     big_endian = 1.  The conversions are value preserving and nothing else is accepted (STIN_E_UNSUPPORTED):
 *         _TO_F64  any scalar (integers are below 2^32 in magnitude: exact; float32 widens exactly)
 *         _TO_F32  float32 only, bit for bit            _TO_I64  any integer scalar
 *         _TO_I32  any integer scalar but uint32         _TO_U8   uint8 only
 *         _TO_UNORM_F64  uint8 only: (double) v / 255.0 with one IEEE division - numpy's u8.astype(float64) / 255.0
 *     row_stride consecutive rows of the table that fill the columns 0, 1, ... of one destination in order (an [N, 3] position,
 *     colour or normal matrix; any single column) leave as one dense matrix with consecutive lanes on consecutive elements; any
 *     other row is written with its stride.  Destinations must not overlap.
 *
 * stin_ply_faces.  The face element when every list has K entries, K = 3 or 4: each record is scalar properties and ONE list
 *     property, stride = the scalars + the count field + K indices.  list_offset = byte offset of the count field in the record;
 *     count_type and index_type are integer scalar types.  Signed fields are sign extended, uint32 is not.  A record whose count
 *     field is not K sets STIN_PLY_COUNT_DIFFERS and writes -1 into its rows (the stride assumption is void: the caller parses the
 *     file another way); a record with an index outside [0, n_vertices) sets STIN_PLY_BAD_INDEX and is written as decoded.
 *     faces: int64 [count * (K - 2), 3] in record order, a quad (a, b, c, d) as (a, b, c), (a, c, d).
 *     status: 4 x int64 DEVICE words written by the call: [0] the flags (an integer atomic or), [1] the lowest record whose count
 *     differs, [2] the lowest record with a bad index (integer atomic minima; 2^63 - 1 = none), [3] 0.  No float atomics.
 *
 * stin_face_label_vote.  Per-face labels to per-vertex labels, the Matterport step of the reference (preprocessing/
 *     graph_level_generation.py:328-336): hist[v][l] = the number of corners (f, i) with faces[f][i] = v and face_labels[f] = l;
 *     vertex_labels[v] = the lowest l that attains max_l hist[v][l] - np.argmax over the rows, 0 for a vertex without faces.
 *     faces [F, 3] int64, face_labels [F] int64 in [0, C), 1 <= C <= STIN_VOTE_MAX_CLASSES, vertex_labels [N] int64.  Integer
 *     counts (int32 atomic adds) only: the same bytes for every launch order.  A corner whose label lies outside [0, C) sets
 *     STIN_VOTE_BAD_LABEL and is not counted; a corner whose vertex lies outside [0, N) sets STIN_VOTE_BAD_INDEX and is not
 *     counted.  status: 4 x int64 DEVICE words: [0] flags, [1] / [2] the lowest face with a bad label / a bad index (2^63 - 1 =
 *     none), [3] 0.  Workspace >= stin_face_label_vote_workspace_bytes(N, C) (the histogram; 0 = unsupported sizes). */
#define STIN_PLY_INT8 0
#define STIN_PLY_UINT8 1
#define STIN_PLY_INT16 2
#define STIN_PLY_UINT16 3
#define STIN_PLY_INT32 4
#define STIN_PLY_UINT32 5
#define STIN_PLY_FLOAT32 6
#define STIN_PLY_FLOAT64 7
#define STIN_PLY_TO_F64 0
#define STIN_PLY_TO_F32 1
#define STIN_PLY_TO_I64 2
#define STIN_PLY_TO_I32 3
#define STIN_PLY_TO_U8 4
#define STIN_PLY_TO_UNORM_F64 5
#define STIN_PLY_FIELD_WORDS 6
#define STIN_PLY_MAX_FIELDS 32
#define STIN_PLY_MAX_STRIDE 240
#define STIN_PLY_MAX_RECORDS 2147483647
#define STIN_PLY_COUNT_DIFFERS 1
#define STIN_PLY_BAD_INDEX 2
#define STIN_VOTE_BAD_LABEL 1
#define STIN_VOTE_BAD_INDEX 2
#define STIN_VOTE_MAX_CLASSES 64
#define STIN_VOTE_MAX_FACES 536870912
#define STIN_VOTE_MAX_VERTICES 1073741824
int stin_ply_decode(const uint8_t* body, int64_t body_bytes, int64_t first, int64_t stride, int64_t count, int big_endian,
                    const int64_t* fields, int n_fields, stin_stream_t stream);
int stin_ply_faces(const uint8_t* body, int64_t body_bytes, int64_t first, int64_t stride, int64_t count, int big_endian,
                   int list_offset, int count_type, int index_type, int K, int64_t n_vertices, int64_t* faces, int64_t* status,
                   stin_stream_t stream);
size_t stin_face_label_vote_workspace_bytes(int64_t N, int C);
int stin_face_label_vote(const int64_t* faces, const int64_t* face_labels, int64_t F, int64_t N, int C, int64_t* vertex_labels,
                         int64_t* status, void* workspace, size_t workspace_bytes, stin_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* STIN_HIP_H */
