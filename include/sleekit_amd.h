/*
 * sleekit_amd.h -- C ABI of the MI355X (gfx950) GPTQ/OBQ layer-quantization engine.
 *
 * Drop-in boundary for the hot path of Coloquinte/sleekit.  The reference is pure
 * Python/NumPy and has no FFI of its own; each entry point below replaces one
 * NumPy function (cited as file:line relative to the reference tree) and is what
 * a ctypes binding in the reference would bind.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (hipMalloc / torch);
 *     matrices are dense row-major; `R` = output rows of W, `n` = input columns;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work and never
 *     synchronise, allocate or copy from host memory, so they can be captured
 *     into a hipGraph (zero-fills and copies inside the library are kernels, not
 *     hipMemsetAsync / hipMemcpyAsync, whose graph nodes did not replay faithfully on ROCm 7.2);
 *   - scratch comes from a caller-provided workspace of at least
 *     slk_workspace_bytes(R, n) bytes, 256-byte aligned; one workspace may be
 *     shared by consecutive calls on the same stream;
 *   - return value: SLK_OK or a negative SLK_E_* code; slk_last_error() gives the
 *     message of the last failure on the calling thread;
 *   - a uniform codebook is (levels, lo, hi): `levels` evenly spaced values on
 *     [lo, hi]; step and zero are formed in float32 exactly as the reference does.
 */
#ifndef SLEEKIT_AMD_H
#define SLEEKIT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLK_OK 0
#define SLK_E_ARG (-1)    /* invalid argument (shape, mode, null pointer)            */
#define SLK_E_NOT_PD (-2) /* reported through `info`, see slk_chol_inverse_upper     */
#define SLK_E_HIP (-3)    /* a HIP runtime call or kernel launch failed              */
#define SLK_E_WS (-4)     /* workspace too small                                     */
/* value of a factorisation's status word (`info`) when its chain of workgroups lost one another: a hand-off between two
 * workgroups of one launch was not seen within 2 s (never observed; the wait is bounded so that nothing can hang the GPU) */
#define SLK_INFO_HANDOFF_TIMEOUT 0x7fffffff

/* Codebooks.  Every entry point that quantizes takes (levels, lo, hi, table):
 *   table == NULL  UniformCodebook(levels, lo, hi)            (sleekit/codebook.py:4-95)
 *   table != NULL  general Codebook of `levels` <= 256 entries (sleekit/codebook.py:98-190): a DEVICE array of
 *                  `levels` increasing float32 values followed by the `levels - 1` bin limits; the index of x
 *                  is np.digitize(x, limits); lo / hi are ignored.
 * codebook maps, slk_codebook_apply `what` */
#define SLK_CB_VALUE 0 /* float32 out */
#define SLK_CB_INDEX 1 /* uint8 out (levels <= 256) */
#define SLK_CB_UP 2    /* float32 out */
#define SLK_CB_DOWN 3  /* float32 out */
#define SLK_CB_INDEX16 4 /* uint16 out (levels <= 65536): UniformCodebook above 256 entries, codebook.py:50-54 */
#define SLK_CB_INDEX32 5 /* uint32 out */

/* column orders, slk_hessian_prepare `order_mode` (obq.py:58-86) */
#define SLK_ORDER_NONE 0
#define SLK_ORDER_DIAG 1
#define SLK_ORDER_ERR 2   /* needs `miss` = column sums of |q(W) - W|   */
#define SLK_ORDER_SQERR 3 /* needs `miss` = column sums of (q(W) - W)^2 */
#define SLK_ORDER_KEYS 4  /* `miss` is reinterpreted as n float64 sort keys (ascending), e.g. from
                             slk_inverse_diag_keys for the inv_diag / combined_diag orders       */

typedef void *slk_stream_t;

/* Library / device ---------------------------------------------------------
 * slk_abi_version: 8.  History: 2 = every quantizing entry takes (levels, lo, hi, table); 3 adds the batch forms
 * (slk_gptq_quantize_batch, slk_row_errors_batch, slk_workspace_bytes_batch) and slk_symmetry_flag; 4 adds the
 * `trace` and `gains` arguments of slk_local_search, slk_set_option / slk_get_option and the batched factorisation
 * (slk_hessian_prepare_batch, slk_chol_inverse_upper_batch, slk_factor_workspace_bytes_batch); 5 adds codebook training
 * (slk_codebook_stats, slk_sort_f32, slk_unique_f32), slk_local_search_batch and slk_factor_unpack_upper_batch; 6 adds
 * slk_chol_inverse_upper_lookahead and slk_release_helpers (the look-ahead is an argument of the call, not a process-wide switch)
 * and turns the loop's `unscale` argument into `flags` (SLK_LOOP_UNSCALE = 1 as before, SLK_LOOP_LATENCY = 2); slk_local_search(_batch)
 * gain `row_err` (the rows' errors after the moves), slk_probe_panel_cycles is new; 7 adds slk_stack_rows and the option "panel_split";
 * 8: no new entry point -- the factorisation's default form is the CHAIN (an outer block's panels in one launch of workgroups that
 * hand the panels on through flags in memory: option "panel_split" 0 / 3; 1 / 2 = round 3's panel kernels; past 4 GiB of one
 * float64 factor, ld * ld * 8 > 2^32, always the panel kernels, whose pointers are 64-bit), whose status word can
 * read SLK_INFO_HANDOFF_TIMEOUT; the factorisation's workspace holds its flags (slk_factor_workspace_bytes_batch grew by
 * 8 * (ld / 64) bytes per matrix); new option "rows_below_wide" ("tall_error" was one of ABI 8 too and is gone).  Still 8, with entries added alongside: the
 * group-scale forms slk_gptq_quantize_grouped, slk_column_miss_grouped, slk_scale_search_grouped and slk_dequantize_grouped
 * (one scale per row and per group of columns; nothing existing changed), then slk_gptq_quantize_grouped_batch (the grouped
 * loop over a batch of layers stacked by rows; slk_gptq_quantize_grouped is its batch of one), then slk_local_search_grouped (the
 * best-first search with the group quantizer's candidates), then the asymmetric group quantizer (an offset per row and group
 * beside the scale): slk_gptq_quantize_grouped_asym, slk_gptq_quantize_grouped_asym_batch, slk_column_miss_grouped_asym,
 * slk_dequantize_grouped_asym, slk_group_midpoints and slk_group_center, then bit-packed indices: slk_pack_indices,
 * slk_unpack_indices and slk_dequantize_packed, then slk_gptq_quantize_batch_error (the loop that carries the layer error)
 * and the option "no_loop_error", then slk_gptq_quantize_layers (the same loop over layers that are not one stack: per-layer
 * pointers), then slk_packed_gemm (a linear layer computed from the packed indices; an addition within 8, nothing existing
 * changed), then slk_hadamard_rows (the block Hadamard rotation of sleekit_amd/rotation.py; likewise), then MXFP4
 * activations: slk_mx_quantize_act4, slk_mx_gemm_a4 and slk_mx_rotate_quantize_act (likewise), then MXFP6 (E2M3)
 * activations: slk_mx_quantize_act6, slk_mx_dequantize_act6, slk_mx_gemm_a6 and slk_mx_rotate_quantize_act6 (likewise), then MXFP6
 * (E2M3) layers: slk_mx_scale_search6, slk_mx_pack6, slk_mx_unpack6 and slk_mx_gemm_w6 (likewise), then the expert-grouped
 * product: slk_mx_experts_workspace_bytes and slk_mx_gemm_experts (likewise), then the gated MLP: slk_mx_glu, slk_mx_gemm_glu
 * and slk_mx_gemm_glu_experts (likewise), then the weight-only products of an MX layer against 16-bit activations:
 * slk_mx_gemm_a16 and slk_mx_gemm_experts_a16 (likewise), then the gated MLP's product in front of a rotated down layer:
 * slk_mx_gemm_glu_rot and slk_mx_gemm_glu_experts_rot (likewise), then MoE routing: slk_moe_topk, slk_moe_sort_workspace_bytes,
 * slk_moe_sort, slk_mx_quantize_act_rows and slk_moe_combine (likewise). */
int slk_abi_version(void);
const char *slk_last_error(void);
/* Run-time switches between code paths that give the same results (the tests hold them to that) or that shape a
 * measurement: "no_window2", "no_fast_leaf", "no_defer", "win_dbg", "no_regular_search", "no_fast_search_div",
 * "no_error_splitk", "error_cb", "no_sym_error", "no_bf16_error", "no_bf16_dma", "no_bf16_hessian", "no_bf16_asym", "no_sym_average",
 * "error_f32_below", "no_wave_search", "no_loop_error" (see slk_gptq_quantize_batch_error), "lookahead" (EVERY factorisation forks the bulk of its outer updates onto a helper stream: a measurement
 * switch; one call at a time asks for it through slk_chol_inverse_upper_lookahead instead), "window_rows" (16 or 32 rows per
 * window workgroup, forced; 0 = 32, or 16 under SLK_LOOP_LATENCY), "panel_split" (the factorisation's panel step: 1 = two launches, diagonal tile then
 * the rest, 2 = one launch in which every workgroup below the diagonal tile repeats its pivot chain; 0 = two for batches and from 8192
 * columns up, one otherwise and always in the look-ahead form), "chain_carries_below" (the chain's launch also makes the rows below the diagonal block,
 * wherever the cap on waiting workgroups allows and the call does not look ahead: 1 = yes, 2 = never, 0 = the rule; "rows_below_wide" 1 | 2 and
 * "panel_split" 1 | 2 force the launches they name) (case-insensitive,
 * an "SLK_" prefix is accepted).  Initial values are read ONCE from the environment (SLK_NO_WINDOW2=1 ...);
 * afterwards only these calls change them.  Process-wide, thread-safe; no reference counterpart.              */
int slk_set_option(const char *name, int value);
int slk_get_option(const char *name);
/* Scratch bytes that any call below may use for an (R, n) layer. */
size_t slk_workspace_bytes(int R, int n);

/* a7  UniformCodebook / Codebook .quantize_value/index/up/down  (sleekit/codebook.py:43-95, 150-190)
 *     out[i] = map(x[i]); float32 arithmetic, IEEE divide, round-half-even.    */
int slk_codebook_apply(const float *x, size_t count, int levels, double lo, double hi, const float *table,
                       int what, void *out, slk_stream_t stream);

/* Codebook TRAINING (Lloyd-Max).  OUTSIDE the hot path of SURVEY.md section 8 (section 2 row 3 marks it out of scope): the
 * rest of the `sleekit.codebook` surface, built after the path's own work.  What one round of Codebook.improve / centroids /
 * probabilities / mse reads off the data  (sleekit/codebook.py:190-267), in one pass:
 *     counts[k] = #{i : index(x[i]) == k}                      (np.bincount of quantize_index)
 *     sums[k]   = sum of those x[i], float64                   (-> centroid = sums / counts)
 *     *sqerr    = sum_i (x[i] - value(x[i]))^2, the difference in float32 and the sum in float64  (-> mse = sqerr / count)
 * for a codebook of 1..256 entries (a general one may hold a single value: every x falls in bin 0).
 * by_position != 0: the "bin" of x[i] is the part of np.array_split(x, levels) that POSITION i falls in, the codebook
 * is ignored and *sqerr = 0: the part means of Codebook.equiprobable (codebook.py:327-331) on sorted data.
 * Results do not depend on scheduling: integer counts, sums in 64-bit fixed point scaled by max|x| (exact to
 * max|x| * 2^-(62 - ceil(log2 count))), sqerr over a fixed tree.  count < 2^31.  Device outputs; workspace of
 * slk_codebook_stats_workspace_bytes().                                                                          */
size_t slk_codebook_stats_workspace_bytes(void);
int slk_codebook_stats(const float *x, size_t count, int levels, double lo, double hi, const float *table, int by_position,
                       long long *counts, double *sums, double *sqerr, void *workspace, size_t ws_bytes, slk_stream_t stream);
/* np.sort / np.unique of float32 data on the device, the first step of lloyd_max and of its two initialisations
 * (codebook.py:283, 327, 356).  `out` must not alias the input; *n_out (device) receives the number of distinct
 * values.  Workspace of slk_sort_workspace_bytes(count) serves either call.                                       */
size_t slk_sort_workspace_bytes(size_t count);
int slk_sort_f32(const float *x, size_t count, float *out, void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_unique_f32(const float *sorted, size_t count, float *out, int *n_out, void *workspace, size_t ws_bytes,
                   slk_stream_t stream);

/* a14 apply_scaling on axis 0  (sleekit/scaling.py:21-25, 73, 80)
 *     invert == 0: out[r][j] = x[r][j] / scale[r]
 *     invert == 1: out[r][j] = x[r][j] / (1.0f / scale[r])   (two IEEE divides)  */
int slk_rows_divide(const float *x, const float *scale, int R, int n, int invert, float *out,
                    slk_stream_t stream);

/* The row shards of `batch` layers (host array of device pointers, each to rows x cols contiguous float32) stacked into
 * dst[batch][rows_padded][cols], the padding rows set to `fill`: what a rank of several does with its rows of a round's
 * layers before the batch entry points (whole 128-row tiles per layer).  No reference counterpart (the reference has
 * one layer, all rows: sleekit/obq.py:310-336); one launch per 64 layers instead of a copy per layer.               */
int slk_stack_rows(const float *const *src, int batch, int rows, int rows_padded, int cols, float fill, float *dst,
                   slk_stream_t stream);

/* a2  remove_input_bias  (sleekit/obq.py:14-25): out = H - mean mean^T (float32). */
int slk_hessian_strip_mean(const float *H, const float *mean, int n, float *out,
                           slk_stream_t stream);

/* a2  remove_dead_values  (sleekit/obq.py:28-35), in place:
 *     H[d][d] = mean(diag H) and W[:, d] = 0 for every d with H[d][d] == 0.
 *     The mean follows NumPy's float32 pairwise order. `W` may be NULL (R = 0). */
int slk_hessian_patch_dead(float *H, float *W, int R, int n, void *workspace, size_t ws_bytes,
                           slk_stream_t stream);

/* a1  Sleekit.add_batch, Linear branch  (sleekit/statistics.py:41-43, 76-87)
 *     X: T tokens x n features, row-major.  With c = count_before, c' = c + T:
 *     mean = mean * (c/c') + colsum(X) / c';   H = H * (c/c') + X^T X / c'.
 *     In float32, one rounding per operation: f = (float)((double)c / c'), cnt = (float)c' (c' past 2^24
 *     rounds), mean = fl(fl(mean f) + fl(s / cnt)), H = fl(fl(H f) + fl(V / cnt)); H comes out bit-wise
 *     symmetric (the lower triangle is computed and mirrored).  V = X^T X matches the reference to float32
 *     GEMM tolerance: a float32 MFMA chain over the tokens, or -- n a multiple of 128 and a workspace of at
 *     least 4096 + 6 n 32 bytes -- six of the nine products of three bfloat16 pieces per operand (mfma_bf16x3.h)
 *     on the bfloat16 MFMA.  That path takes the tokens in chunks of (ws_bytes - 4096) / (6 n) rounded down to
 *     a multiple of 32; the first chunk applies f, each later one adds fl(V_chunk / cnt) to what is there, so
 *     a chunked call rounds once more per chunk than a whole one.  X needs no alignment.  workspace may be
 *     NULL (float32 MFMA at every width).                                                                   */
int slk_hessian_accumulate(float *H, float *mean, const float *X, int n, int T,
                           long long count_before, void *workspace, size_t ws_bytes, slk_stream_t stream);

/* a1, for a mixture of experts: E running statistics in one call, the host reading nothing.
 *   - X: M x n float32, rows sorted by expert; offsets: E + 1 int32 in DEVICE memory under the rule of slk_mx_gemm_experts
 *     (offsets[0] == 0, non-decreasing, offsets[E] == M); H: E x n x n; mean: E x n; counts: E int64 in DEVICE memory,
 *     read and written, >= 0; flag: one int in device memory.
 *   - An expert e with T_e = offsets[e + 1] - offsets[e] > 0 rows: H[e] and mean[e] become what slk_hessian_accumulate(H[e],
 *     mean[e], X + offsets[e] n, n, T_e, counts[e], ...) makes them, bit for bit on any data -- the same kernel bodies run
 *     the same steps, with f = (float)((double)c / c') and cnt = (float)c' formed on the device -- and counts[e] becomes
 *     counts[e] + T_e.  An expert without rows: no byte of H[e], mean[e] or counts[e] is read or written.
 *   - A one-workgroup prologue checks the offsets rule before any address is made from an offset: broken, flag[0] = 1 and H,
 *     mean and counts stay unwritten; kept, flag[0] = 0.  Everything runs in order on the caller's stream.
 *   - Two paths, as in the single call: the float32 MFMA chain at every n; the bfloat16 x 3 path when n % 128 == 0 and the
 *     workspace has slk_hessian_experts_workspace_bytes(E, n, M) bytes.  The grouped entry never chunks: its bfloat16 path
 *     equals the single call whose workspace holds all T_e tokens; with less room, a NULL workspace or M / 32 + E above
 *     65535 it takes the float32 path.
 *   - slk_hessian_experts_workspace_bytes(E, n, M) = align_up(32 (1 + E), 256) + (n % 128 == 0 ? 6 n 32 (M / 32 + min(E, M))
 *     : 0): the table of the prologue (8 ints of head, 8 ints an expert: first row, rows, first 32-token slab, f, cnt), then
 *     the planes of every expert's tokens padded to 32.  0 for E, n or M < 1.
 * SLK_E_ARG, before any launch, slk_last_error() naming the offender: E < 1 or E > SLK_MX_MAX_EXPERTS, n or M < 1, a NULL
 *   pointer other than the workspace, a workspace off 16-byte alignment, a non-NULL workspace below the table's 32 (1 + E)
 *   bytes.
 *
 * slk_hessian_accumulate_experts_mx: the same statistics of MX-coded rows -- a_codes / a_scales, M rows as the activation
 *   quantizers and slk_mx_gemm_glu* write them, a_fmt SLK_MX_ACT_FP8, _FP4 or _FP6, n % 32 == 0, a_codes aligned to 16 bytes
 *   -- that is of x = value(code) 2^(b - 127), with the same per-expert running-mean arithmetic, prologue, table and
 *   empty-expert rule.  Every such x is a bfloat16 exactly, so X^T X is one bfloat16 MFMA pass with exact products and
 *   float32 sums, at every n.  Exactness is promised for scale bytes 10 .. 245 (every E4M3 value 2^-9 2^(b - 127) .. 448
 *   2^(b - 127) is then a normal bfloat16; the 4- and 6-bit formats lie inside that) and no further.  flag is TWO ints:
 *   flag[0] the offsets rule's, flag[1] = 1 when a scale byte of a row is 255 (E8M0's NaN, as slk_mx_dequantize_act
 *   raises it).  The workspace holds the table only: slk_hessian_experts_workspace_bytes(E, 32, M) bytes suffice.        */
size_t slk_hessian_experts_workspace_bytes(int E, int n, int M);
int slk_hessian_accumulate_experts(float *H, float *mean, const float *X, const int *offsets, int E, int n, int M,
                                   long long *counts, int *flag, void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_hessian_accumulate_experts_mx(float *H, float *mean, const uint8_t *a_codes, const uint8_t *a_scales, int a_fmt,
                                      const int *offsets, int E, int n, int M, long long *counts, int *flag, void *workspace,
                                      size_t ws_bytes, slk_stream_t stream);

/* a4  column statistics for the err / sqerr orders  (sleekit/obq.py:60-69)
 *     miss[j] = sum over rows, in row order, of |q(W) - W| (squared == 0) or its square; for n == 1 in NumPy's pairwise
 *     order over the R rows, which is how NumPy reduces an (R, 1) array along axis 0 (the grouped forms likewise). */
int slk_column_miss(const float *W, int R, int n, int levels, double lo, double hi, const float *table,
                    int squared, float *miss, slk_stream_t stream);

/* a3+a4+a5  damping, ordering, permutation  (sleekit/obq.py:198-204)
 *     Hd = float64(H) + float32(damp * mean(diag H)) * I
 *     order = argsort(-diag(Hd) [* miss])            (stable on ties)
 *     order_out[n] (int64) and the permuted, index-reversed damped Hessian that
 *     slk_chol_inverse_upper consumes are written to the workspace-independent
 *     outputs `order_out` and `A` (float64, ld = slk_factor_ld(n)).            */
int slk_hessian_prepare(const float *H, int n, float damp, int order_mode, const float *miss,
                        long long *order_out, double *A, void *workspace, size_t ws_bytes,
                        slk_stream_t stream);
/* Sort keys of the orders that need diag(Hd^-1) (sleekit/obq.py:70-75): given the factor U of the
 * damped Hessian in its ORIGINAL order (order_mode NONE), keys[j] = diag(Hd^-1)[j] = sum_i U[i][j]^2
 * (combined == 0, "inv_diag") or -diag(Hd)[j] / diag(Hd^-1)[j] (combined != 0, "combined_diag").  */
int slk_inverse_diag_keys(const double *U, const float *H, int n, float damp, int combined, double *keys,
                          void *workspace, size_t ws_bytes, slk_stream_t stream);
/* Sort keys of the "pivot" order (greedy pivoted Cholesky, sleekit/obq.py:78, 140-166): keys[j] = the
 * step at which column j of Hd = float64(H) + float32(damp * mean(diag H)) * I is picked.  A cold path:
 * 2 n small launches, n^3 / 6 divide-subtract terms; needs 8 n^2 + O(n) bytes of workspace.          */
int slk_pivot_keys(const float *H, int n, float damp, double *keys, void *workspace, size_t ws_bytes,
                   slk_stream_t stream);
/* Leading dimension (and row count) of the padded float64 matrices A / scratch. */
int slk_factor_ld(int n);
/* Same layout from a float64 matrix as is (no damping, no order): A = reversed lower
 * triangle of M, padded.  Entry for compute_hessian_chol on a caller's own matrix.  */
int slk_factor_load(const double *M, int n, double *A, slk_stream_t stream);

/* a6  compute_hessian_chol  (sleekit/obq.py:38-55)
 *     A: output of slk_hessian_prepare (destroyed).  U: n x n float64 row-major,
 *     upper triangular with U^T U = Hd[order][:, order]^-1, zeros below the diagonal.
 *     info[0] = 0 on success, else 1 + k, k the first index IN THE ORDER OF THE FACTORISATION whose pivot is not > 0
 *     (negative, zero or NaN): row k of the index-reversed matrix A, that is column n - 1 - k of Hd[order][:, order],
 *     column order[n - 1 - k] of H -- the reference raises numpy.linalg.LinAlgError there.  With several such pivots
 *     the smallest k; the padding rows of A never count; in a batch every matrix has its own word.  (Or
 *     SLK_INFO_HANDOFF_TIMEOUT, see above.)  U is void when info[0] != 0.                                        */
int slk_chol_inverse_upper(double *A, int n, double *U, int *info, void *workspace,
                           size_t ws_bytes, slk_stream_t stream);
/*     The same with LOOK-AHEAD: after a block's panels only the next block's tile columns are updated on `stream`, the
 *     rest of the trailing triangle runs on a helper stream beside the next block's panels (forked and joined by events
 *     inside the call: the caller still sees one stream).  Same updates per tile in the same order: U bit for bit.  For
 *     ONE layer at a time (latency); with several factorisations in flight on streams of their own the plain form is
 *     faster.  The helper stream and its events are made at first use per (device, stream) and live until
 *     slk_release_helpers(), which drains BOTH the helper streams and the caller streams they belong to, then destroys
 *     the helpers (call it before destroying such a stream).  The one call of this library that is not safe beside others:
 *     no look-ahead factorisation may be enqueued from another thread while it runs.                                        */
int slk_chol_inverse_upper_lookahead(double *A, int n, double *U, int *info, void *workspace,
                                     size_t ws_bytes, slk_stream_t stream);
int slk_release_helpers(void);

/* (a3-a6 for `batch` layers of ONE width n at once: every launch covers all the layers -- blockIdx.z is the layer --
 * so a round of small layers costs the launches of one.  Small layers are bound by the host's launch rate, not by the
 * GPU (a 768-column layer is ~50 launches of a few microseconds each): OPT-125M's 72 layers go from 48 ms to the time
 * of ~10 rounds.  H: HOST array of `batch` device pointers; order_out batch x n; A batch x ld x ld (ld = slk_factor_ld(n));
 * U batch x n x n; info `batch` ints.  Orders: SLK_ORDER_NONE / SLK_ORDER_DIAG.  Same results as the single-layer calls.
 * Workspace: slk_factor_workspace_bytes_batch(batch, n).                                                          */
int slk_hessian_prepare_batch(const float *const *H, int batch, int n, float damp, int order_mode,
                              long long *order_out, double *A, void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_chol_inverse_upper_batch(double *A, int batch, int n, double *U, int *info, void *workspace,
                                 size_t ws_bytes, slk_stream_t stream);
size_t slk_factor_workspace_bytes_batch(int batch, int n);

/* Multi-GPU payload of one layer's factor: one buffer of 8-byte words,
 *   [0] status word, [1..n] order, then the upper triangle of U row by row,
 * slk_factor_payload_words(n) = n (n + 1) / 2 + n + 1 words -- what the single RCCL broadcast per
 * layer carries.  Unpack restores the square U (zeros below the diagonal).   */
size_t slk_factor_payload_words(int n);
int slk_factor_pack(const double *U, const long long *order, const int *info, int n, void *payload,
                    slk_stream_t stream);
int slk_factor_unpack(const void *payload, int n, double *U, long long *order, int *info,
                      slk_stream_t stream);
/*     ... writing the diagonal and above only: for a U buffer whose lower triangle is zero already (zeroed once,
 *     reused round after round: a third less traffic than rewriting the zeros).                          */
int slk_factor_unpack_upper(const void *payload, int n, double *U, long long *order, int *info,
                            slk_stream_t stream);
/*     ... and a round's payloads (a HOST array of `batch` device pointers) into stacked factors U (batch, n, n),
 *     order (batch, n), info (batch) in one launch; verdict (may be NULL): (batch) int32, the word that FOLLOWS each
 *     payload's slk_factor_payload_words(n) (sleekit_amd.dist appends the root's symmetry verdict of the layer's
 *     Hessian there: the buffers must then be one word longer).                                            */
int slk_factor_unpack_upper_batch(const void *const *payloads, int batch, int n, double *U, long long *order, int *info,
                                  int *verdict, slk_stream_t stream);

/* a5+a8+a9+a10  quantize_opt without local search  (sleekit/obq.py:106-137, 202-213)
 *     W: R x n float32.  scale: per-row divisor applied on load (NULL: W is used as is).
 *     Runs the blocked column-sequential loop in the order `order` with factor U and
 *     the reference's recursion (min_block, num_blocks), float64 updates rounded to
 *     float32 at the reference's rounding points.
 *     order (may be NULL): identity, i.e. _quantize_opt_block on Q as given (obq.py:121-137).
 *     Q (R x n float32, original column order): codebook VALUES in the scaled domain, or -- flags & SLK_LOOP_UNSCALE,
 *       scale given -- de-scaled like quantize_with_scaling's result (scaling.py:80: q / (1 / scale[r])).
 *     flags: SLK_LOOP_UNSCALE | SLK_LOOP_LATENCY.  SLK_LOOP_LATENCY: this layer is alone on the GPU -- the window kernel
 *       takes 16 rows per workgroup (shortest launch) instead of 32 (least chip time, for streams of layers whose kernels
 *       overlap); the results are the same bit for bit.
 *     idx (may be NULL): codebook indices, uint8, original column order.
 *     E_out (may be NULL): the scaled errors E of obq.py:115, R x n, in PROCESSING order. */
#define SLK_LOOP_UNSCALE 1
#define SLK_LOOP_LATENCY 2
int slk_gptq_quantize(const float *W, const float *scale, const long long *order, const double *U,
                      int R, int n, int levels, double lo, double hi, const float *table, int min_block,
                      int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out, void *workspace,
                      size_t ws_bytes, slk_stream_t stream);

/* (e) The same loop over `batch` layers of one shape at once, stacked by rows: W, Q, idx, E_out are
 *     (batch * rows_per_layer) x n, scale has batch * rows_per_layer entries, order is batch x n and U is
 *     batch x n x n (layer b's rows use order[b], U[b]).  Results are those of `batch` separate calls, bit for
 *     bit -- rows never interact (obq.py:106-137) -- but every launch covers all the layers: the row shards of
 *     a multi-GPU run (R / G rows each) fill the chip together where each alone leaves most of it
 *     idle.  batch in 1..64; batch > 1 needs rows_per_layer % 64 == 0 and the orders.
 *     Workspace: slk_workspace_bytes_batch(batch, rows_per_layer, n).                                       */
int slk_gptq_quantize_batch(const float *W, const float *scale, const long long *order, const double *U,
                            int batch, int rows_per_layer, int n, int levels, double lo, double hi,
                            const float *table, int min_block, int num_blocks, int flags, float *Q,
                            uint8_t *idx, float *E_out, void *workspace, size_t ws_bytes, slk_stream_t stream);
size_t slk_workspace_bytes_batch(int batch, int rows_per_layer, int n);

/* (e') slk_gptq_quantize_batch that also returns the layer error, carried by the loop instead of a product of its own:
 *     row_err ((batch * rows_per_layer) float32) = (W - Q) H_b (W - Q)^T per row (obq.py:89-95 before the mean), Q being
 *     the values this call stores, from the scaled errors E the loop keeps for its trailing updates (obq.py:115).  With
 *     Hd = H + lambda I the damped Hessian the factor was made from, U^T U = Hd[order][:, order]^-1, error propagation gives
 *         row_err[r] = float32(scale_r^2 * sum_j E[r][j]^2 - lambda_b * sum_j (W[r][j] - Q[r][j])^2),
 *     lambda_b = float32(damp) * mean(diag H_b) formed as slk_hessian_prepare forms it, the differences in float32, squares
 *     and sums in float64, scale_r = 1 without scales: one pass over E and W in the loop's last kernel (16 R n bytes
 *     where the plain loop's moves 8 R n), no atomics -- the same inputs give the same bits on every run and stream.
 *     H: HOST array of `batch` device pointers (as slk_row_errors_batch takes them), b = r / rows_per_layer; damp: the
 *     damping the factor was made with.
 *     WHEN it is the reference's error: H bit-wise symmetric (the factor reads one triangle of H, the product all of it)
 *     and U the factor of THIS H with THIS damp in this order; nothing here checks either -- a caller that cannot vouch
 *     for them calls slk_row_errors_batch.  HOW CLOSE: the identity is exact up to the loop's own roundings (float64
 *     updates, float32 stores); against the float64 product the worst row is below 1e-6 relative on well-conditioned
 *     Hessians (the reference's own float32 product: 2e-7 ... 1e-6), a few 1e-5 on a steeply decaying spectrum where the
 *     reference's float32 product is 1e-3 off: at least as close to float64 as the reference's float32 result, and not
 *     bit-equal to slk_row_errors_batch.
 *     scale given: flags must hold SLK_LOOP_UNSCALE (the error is that of the de-scaled Q); SLK_E_ARG otherwise.
 *     Everything else as slk_gptq_quantize_batch; batch = 1 serves a single layer.  Workspace:
 *     slk_workspace_bytes_batch(batch, rows_per_layer, n) (slk_workspace_bytes(R, n) for batch = 1).
 *     Option "no_loop_error": sleekit_amd's callers (engine.loop_error_route) then never take this entry and compute the
 *     product as before -- an A/B switch inside one build, and a way out.                                      */
int slk_gptq_quantize_batch_error(const float *W, const float *scale, const long long *order, const double *U,
                                  const float *const *H, float damp, int batch, int rows_per_layer, int n, int levels,
                                  double lo, double hi, const float *table, int min_block, int num_blocks, int flags,
                                  float *Q, uint8_t *idx, float *E_out, float *row_err, void *workspace, size_t ws_bytes,
                                  slk_stream_t stream);

/* (e'') The loop of (e) and (e') over `batch` layers that are NOT one stack: W, scale, order, U (and H) are HOST arrays of
 *     `batch` device pointers, one per layer -- W[b] rows_per_layer x n, scale[b] rows_per_layer entries, order[b] n, U[b]
 *     n x n -- each contiguous, anywhere in memory and in any order: no copy into a stack before the loop (two 4096-column
 *     factors are 268 MB read and written).  The kernels read every layer through a table of these pointers (one scalar
 *     load per workgroup); the stacked entries fill the same table from their base pointers.  What the call WRITES stays one
 *     stack: Q, idx, E_out (batch * rows_per_layer) x n and row_err (batch * rows_per_layer), layer b at rows
 *     [b * rows_per_layer, (b + 1) * rows_per_layer).  Results: those of `batch` separate calls, bit for bit.
 *     scale may be NULL (no scales; otherwise every entry is given).  H and row_err both given: the error-carrying loop of
 *     (e') with `damp`; both NULL: the plain one (damp ignored).  batch in 1..16 (the table's size); batch > 1 needs
 *     rows_per_layer % 64 == 0.  A U that is not 16-byte aligned sends every layer of the call to the general window kernel.
 *     gscale / group_size: must be NULL / 0 -- group scales are taken stacked only (slk_gptq_quantize_grouped_batch); SLK_E_ARG
 *     otherwise.  Everything else, and the workspace, as slk_gptq_quantize_batch.                                 */
int slk_gptq_quantize_layers(const float *const *W, const float *const *scale, const long long *const *order,
                             const double *const *U, const float *const *H, float damp, const float *const *gscale,
                             int group_size, int batch, int rows_per_layer, int n, int levels, double lo, double hi,
                             const float *table, int min_block, int num_blocks, int flags, float *Q, uint8_t *idx,
                             float *E_out, float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream);

/* Group scales.  gscale: R x G float32, positive, G = n / group_size (group_size >= 1 must divide n); element (r, c)
 * belongs to group c / group_size.  The group quantizer maps x in column c of row r to
 *     codebook(x / s) / (1 / s),   s = gscale[r][c / group_size]   (float32 IEEE divides, as scaling.py:73, 80).
 * slk_gptq_quantize_grouped: quantize_opt(W, H, group quantizer, ...) (sleekit/obq.py:169-217) without local search: the
 *     loop of slk_gptq_quantize on the UNSCALED W, only its leaves scale.  Q: de-scaled values, original column order;
 *     idx (may be NULL, levels <= 256): the codebook indices of Q / s; E_out (may be NULL): errors in processing order.
 *     flags: SLK_LOOP_LATENCY only (accepted; the grouped loop runs 16 rows per window workgroup either way).
 *     Workspace: slk_workspace_bytes(R, n).
 * slk_gptq_quantize_grouped_batch: the same loop over `batch` layers of one shape stacked by rows, as slk_gptq_quantize_batch:
 *     W, Q, idx, E_out are (batch * rows_per_layer) x n, gscale (batch * rows_per_layer) x G, order batch x n, U
 *     batch x n x n.  Results are those of `batch` separate slk_gptq_quantize_grouped calls, bit for bit.  batch in 1..64;
 *     batch > 1 needs rows_per_layer % 64 == 0 and the orders.  Workspace: slk_workspace_bytes_batch(batch, rows_per_layer, n)
 *     (it covers the loop's 2 R n floats and 2 batch n ints with room to spare, R = batch * rows_per_layer).
 * slk_column_miss_grouped: slk_column_miss with the group quantizer (the err / sqerr keys of the grouped loop).
 * slk_scale_search_grouped: slk_scale_search on every group at once: row r G + k of the (R G, group_size) view of W is
 *     group k of row r, with base[r G + k] and, hdiag given (length n), the slice hdiag[k group_size : (k + 1) group_size];
 *     out: R x G.
 * slk_dequantize_grouped: Q[r][c] = value(idx[r][c]) / (1 / s), bit for bit the Q that slk_gptq_quantize_grouped returned. */
int slk_gptq_quantize_grouped(const float *W, const float *gscale, int group_size, const long long *order, const double *U,
                              int R, int n, int levels, double lo, double hi, const float *table, int min_block,
                              int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out, void *workspace,
                              size_t ws_bytes, slk_stream_t stream);
int slk_gptq_quantize_grouped_batch(const float *W, const float *gscale, int group_size, const long long *order, const double *U,
                                    int batch, int rows_per_layer, int n, int levels, double lo, double hi, const float *table,
                                    int min_block, int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out,
                                    void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_column_miss_grouped(const float *W, const float *gscale, int group_size, int R, int n, int levels, double lo,
                            double hi, const float *table, int squared, float *miss, slk_stream_t stream);
int slk_scale_search_grouped(const float *W, const float *base, const float *factors, int n_factors, const float *hdiag,
                             int group_size, int R, int n, int levels, double lo, double hi, const float *table, float *out,
                             slk_stream_t stream);
int slk_dequantize_grouped(const uint8_t *idx, const float *gscale, int group_size, int R, int n, int levels, double lo,
                           double hi, const float *table, float *Q, slk_stream_t stream);

/* Group scales with offsets (asymmetric).  goffset: R x G float32 beside gscale, element (r, c) has s = gscale[r][k] and
 * o = goffset[r][k], k = c / group_size.  The ASYMMETRIC group quantizer maps x to
 *     codebook((x - o) / s) / (1 / s) + o     (float32 IEEE, in this order: subtract, divide, codebook, divide, add);
 * with goffset all zero it is the group quantizer above.
 * slk_gptq_quantize_grouped_asym(_batch): slk_gptq_quantize_grouped(_batch) with that quantizer in the leaves; the loop runs
 *     on the unscaled, uncentred W.  idx (may be NULL): codebook indices from which slk_dequantize_grouped_asym rebuilds Q
 *     bit for bit.  Same flags, shapes and workspace as the symmetric forms; the batch gives the results of separate calls.
 * slk_column_miss_grouped_asym: slk_column_miss with the asymmetric group quantizer.
 * slk_dequantize_grouped_asym: Q[r][c] = value(idx[r][c]) / (1 / s) + o.
 * slk_group_midpoints: goffset[r][k] = 0.5f * (min + max) of group k of row r; Wc (may be NULL): the centred weights
 *     W - goffset by element (R x n).
 * slk_group_center: Wc = W - goffset by element, goffset given. */
int slk_gptq_quantize_grouped_asym(const float *W, const float *gscale, const float *goffset, int group_size, const long long *order,
                                   const double *U, int R, int n, int levels, double lo, double hi, const float *table,
                                   int min_block, int num_blocks, int flags, float *Q, uint8_t *idx, float *E_out,
                                   void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_gptq_quantize_grouped_asym_batch(const float *W, const float *gscale, const float *goffset, int group_size,
                                         const long long *order, const double *U, int batch, int rows_per_layer, int n,
                                         int levels, double lo, double hi, const float *table, int min_block, int num_blocks,
                                         int flags, float *Q, uint8_t *idx, float *E_out, void *workspace, size_t ws_bytes,
                                         slk_stream_t stream);
int slk_column_miss_grouped_asym(const float *W, const float *gscale, const float *goffset, int group_size, int R, int n,
                                 int levels, double lo, double hi, const float *table, int squared, float *miss,
                                 slk_stream_t stream);
int slk_dequantize_grouped_asym(const uint8_t *idx, const float *gscale, const float *goffset, int group_size, int R, int n,
                                int levels, double lo, double hi, const float *table, float *Q, slk_stream_t stream);
int slk_group_midpoints(const float *W, int group_size, int R, int n, float *goffset, float *Wc, slk_stream_t stream);
int slk_group_center(const float *W, const float *goffset, int group_size, int R, int n, float *Wc, slk_stream_t stream);

/* Packed indices: uint8 codebook indices at `bits` = b bits each (1 <= b <= 8), the compact form of (idx, S[, O]).
 *   - each row is cut into chunks of 32 consecutive indices; the last one is padded with zero indices.  A row takes
 *     b * ceil(n / 32) 32-bit words and starts on a word boundary: `words` is R x (b * ceil(n / 32)).
 *   - chunk k of row r is words [b k, b k + b) of that row, read as ONE little-endian integer of 32 b bits (word j holds
 *     bits [32 j, 32 j + 32)); index 32 k + i sits in its bits [i b, i b + b).
 *   - only the low b bits of an index are stored: an index >= 2^b is a caller error and comes back masked.
 *   - b = 8 is the idx bytes read as little-endian words, each row padded to a multiple of 32 bytes.
 *   A stack of B layers of one width, (B, R, n), is B R rows: no batch form is needed.
 * slk_pack_indices: idx (R x n uint8) -> words.
 * slk_unpack_indices: words -> idx (R x n uint8).
 * slk_dequantize_packed: out[r][c] = value(k), k = min(index, levels - 1), de-scaled by at most one of
 *     scale (R float32):               value(k) / (1 / scale[r])            (the loop's per-row de-scale)
 *     gscale (R x n / group_size):     value(k) / (1 / gscale[r][c / group_size])   (slk_dequantize_grouped)
 *     gscale and goffset:              value(k) / (1 / s) + goffset[r][c / group_size]  (slk_dequantize_grouped_asym)
 *   in float32 (bit for bit the paths named), or that float32 value rounded to nearest even as bfloat16 / float16
 *   (`out_dtype`).  scale and gscale are exclusive; goffset needs gscale; group_size is read only with gscale. */
#define SLK_DTYPE_F32 0
#define SLK_DTYPE_BF16 1
#define SLK_DTYPE_F16 2
int slk_pack_indices(const uint8_t *idx, int R, int n, int bits, uint32_t *words, slk_stream_t stream);
int slk_unpack_indices(const uint32_t *words, int R, int n, int bits, uint8_t *idx, slk_stream_t stream);
int slk_dequantize_packed(const uint32_t *words, int R, int n, int bits, int levels, double lo, double hi, const float *table,
                          const float *scale, const float *gscale, const float *goffset, int group_size, int out_dtype, void *out,
                          slk_stream_t stream);

/* MXFP4: the OCP MX block format the MI355X computes in.  A BLOCK is 32 consecutive original columns of one row
 * (n % 32 == 0, else SLK_E_ARG); it shares one power-of-two scale, and its elements are FP4 E2M1 codes.
 *   - element: code = sign << 3 | m, 4 bits; magnitudes m = 0 .. 7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.  The codebook is the
 *     15-entry table -6, -4, -3, -2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2, 3, 4, 6 with the midpoints as limits (a tie goes
 *     upward); table index i < 7 is code 8 | (7 - i), otherwise code i - 7.  Code 0x8 (-0) is never written and reads back
 *     as index 7, value +0.  An index above 14 is a caller error and is stored as code 7.
 *   - codes: uint8 R x n / 2; byte j of a row holds column 2 j in its low nibble and column 2 j + 1 in its high nibble
 *     (the bytes of slk_pack_indices at 4 bits applied to the codes).
 *   - scales: uint8 R x n / 32, E8M0: byte b means 2^(b - 127).  Scales chosen here have b in [71, 253] (2^-56 .. 2^126:
 *     s and 1 / s are normal float32); byte 255 (NaN) is never written and raises `flag` on input.
 *   Known answers: indices 0 .. 14 in order are codes f e d c b a 9 0 1 2 3 4 5 6 7; columns with codes 1, 2, 0xf, 0 pack
 *   to bytes 0x21 0x0f; the scale 0.0078125 is byte 120.
 *   With such a scale s the group quantizer of slk_gptq_quantize_grouped (group_size 32, that table) is exact in every step:
 *   Q = value(idx) / (1 / s) = +-magnitude * 2^(b - 127) bit for bit, which is what slk_mx_dequantize rebuilds.
 * slk_mx_scale_search: per block, b0 = max(max / 6, min / -6, 1e-16) in float32 (sleekit/scaling.py:44-55), base the smallest
 *   power of two >= b0; SLK_MX_MAX gives base; SLK_MX_MSE and SLK_MX_DIAG run the loop body of compute_min_mse_scaling
 *   (sleekit/scaling.py:127-134) over the factors 0.125, 0.25, 0.5, 1 in this order: the error sum_j [hdiag_j] E_j^2 of the
 *   round-to-nearest quantization with scale f * base in NumPy's summation order, the FIRST minimum kept; the result is
 *   base * best factor (base itself where no error is below +inf).  hdiag: diag(H), n float32, with SLK_MX_DIAG only.
 *   scales (uint8) and S (the same scales as float32), R x n / 32 each; either may be NULL.  Weights must be finite.
 * slk_mx_pack: idx (R x n uint8 table indices) -> codes, and S (R x n / 32 float32) -> scales; either pair may be NULL.
 *   A scale that is not a positive normal power of two sets flag[0] = 1 (DEVICE int, zeroed by the call; may be NULL).
 * slk_mx_unpack: codes -> idx and scales -> S; either pair may be NULL.  flag[0] = 1 if a scale byte is 255.
 * slk_mx_dequantize: out[r][c] = value(code) * 2^(b - 127), R x n float32, or that value rounded to nearest even as
 *   bfloat16 / float16 (`out_dtype`, SLK_DTYPE_*).  flag as in slk_mx_unpack.
 *   idx, codes and out must be aligned to 16 bytes (SLK_E_ARG otherwise). */
#define SLK_MX_MAX 0
#define SLK_MX_MSE 1
#define SLK_MX_DIAG 2
int slk_mx_scale_search(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S,
                        slk_stream_t stream);
int slk_mx_pack(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag,
                slk_stream_t stream);
int slk_mx_unpack(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag,
                  slk_stream_t stream);
int slk_mx_dequantize(const uint8_t *codes, const uint8_t *scales, int R, int n, int out_dtype, void *out, int *flag,
                      slk_stream_t stream);

/* A linear layer from the packed form, on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4).  The weights are
 * `codes` / `scales` above (rows are output features, blocks run along K); the activations are quantized to MXFP8:
 *   - a_scales: uint8 M x K / 32, E8M0.  Per block, b0 = max(amax / 448, 1e-16) in float32 (amax the block's largest |x|
 *     as float32), the scale the smallest power of two >= b0, the byte its exponent + 127: slk_mx_scale_search's
 *     SLK_MX_MAX with 448 in place of 6.  A block of zeros gives byte 74.  The scale does not saturate.
 *   - a_codes: uint8 M x K, OCP E4M3 (e4m3fn: bias 7, subnormals k 2^-9, largest 448 = 0x7e), code = sign << 7 | exp << 3
 *     | man: x / s (exact) rounded to nearest, ties to even, clamped at +-448.  A zero magnitude is written as 0x00
 *     (never -0); 0x7f / 0xff (NaN) are never written.
 *   Known answers: a block whose amax is 1.0 has byte 119 and its elements 1.0, -0.3, 0.001, 0 the codes 78 ea 28 00;
 *   amax 1.75 gives byte 119 and 1.75, -1.75, 0.01, 1e-5 the codes 7e fe 42 01; after scaling 17 -> 58 (the tie goes to
 *   16), 19 -> 5a, 2^-10 -> 00, 1.5 * 2^-9 -> 02.
 * slk_mx_quantize_act: X (M x K row-major, `x_dtype` SLK_DTYPE_*) -> a_codes, a_scales.  flag[0] = 1 (DEVICE int, zeroed
 *   by the call, required) if X holds a NaN or an infinity; the outputs are then not meaningful.
 * slk_mx_dequantize_act: out[m][k] = value(code) * 2^(b - 127), float32 or that value rounded to nearest even as
 *   bfloat16 / float16.  flag (may be NULL): 1 if a scale byte is 255.
 * slk_mx_gemm: out[m][n] = sum_k A[m][k] W[n][k] (+ bias[n]), A and W the de-quantized operands, the products exact and
 *   the sum in float32 inside the MFMA, over K in a fixed order (no atomics: a repeated call gives the same bits); out is
 *   M x N float32, or that value rounded to nearest even as bfloat16 / float16.  bias: N float32, may be NULL.  Any
 *   M, N >= 1.  Scale byte 255 is not looked for: the hardware reads it as NaN and so does the result.
 *   K % 32 != 0 or K < 32, M or N < 1, a NULL required pointer, an unknown dtype, or X, a_codes, w_codes or out off
 *   16-byte alignment: SLK_E_ARG, before any launch. */
int slk_mx_quantize_act(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag,
                        slk_stream_t stream);
int slk_mx_dequantize_act(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                          slk_stream_t stream);
int slk_mx_gemm(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                const float *bias, int M, int N, int K, int out_dtype, void *out, slk_stream_t stream);

/* A linear layer from packed indices (the format of slk_pack_indices above), de-quantized inside a bfloat16 / float16 MFMA
 * GEMM (v_mfma_f32_16x16x32_bf16 / _f16): no de-quantized weight is written to memory and there is no workspace.
 * slk_packed_gemm: out[m][n] = sum_k Xc[m][k] Wc[n][k] (+ bias[n]) for a layer of N rows (output features) and K columns:
 *   - Wc is bit for bit slk_dequantize_packed(words, N, K, ..., out_dtype = compute_dtype): value(min(index, levels - 1))
 *     / (1 / s) [+ o] in float32, true divides in this order, rounded once to nearest even to the compute type;
 *     (scale | gscale [, goffset], group_size) as there;
 *   - Xc is X (M x K row-major, `x_dtype`) rounded to nearest even to the compute type (the identity when it has it);
 *   - compute_dtype is SLK_DTYPE_BF16 or SLK_DTYPE_F16; the products are exact in float32, the sums float32 over K in a
 *     fixed order (no atomics: a repeated call gives the same bits); the float32 bias (N, may be NULL) is added in float32
 *     and the result rounded once to `out_dtype` (M x N row-major).
 *   X is not looked at for NaN or infinity (they propagate); 16-bit subnormals behave as the hardware defines them.
 *   Any M, N >= 1; K >= 8 and K % 8 == 0; with gscale, group_size % 8 == 0 and group_size divides K (so that the 8 consecutive
 *   k a lane feeds the MFMA lie inside one row under one scale; K % 32 != 0 is fine).  Up to M = 16 a workgroup is one
 *   16-column tile of out whose 8 waves share K; above, a workgroup is a 64 x 64 tile that de-quantizes its weights into LDS.
 *   SLK_E_ARG, before any launch, with slk_last_error() naming the offender: K % 8 != 0 or K < 8, M or N < 1, bits outside
 *   1..8, levels < 2 or > 2^bits, scale together with gscale, goffset without gscale, group_size % 8 != 0 or not dividing K,
 *   a NULL X, words or out, an unknown x_dtype or out_dtype, compute_dtype not BF16 or F16, X or out off 16-byte alignment,
 *   words off 4, and, for M > 16, ceil(M / 64) * ceil(N / 64) above 2^31 - 1 (the 64 x 64 tiles of one launch).  Layers outside these shapes: slk_dequantize_packed and any GEMM. */
int slk_packed_gemm(const void *X, int x_dtype, const uint32_t *words, int bits, int levels, double lo, double hi, const float *table,
                    const float *scale, const float *gscale, const float *goffset, int group_size, const float *bias, int M, int N,
                    int K, int compute_dtype, int out_dtype, void *out, slk_stream_t stream);

/* The randomized block Hadamard rotation of the input features (sleekit_amd/rotation.py): no reference counterpart.
 * slk_hadamard_rows: Y = X R (transposed == 0) or Y = X R^T (transposed != 0), R = diag(s) blockdiag(H_block) / sqrt(block),
 *   H_block the Sylvester-Hadamard matrix.  X and Y are rows x n, contiguous; s = `signs`, n float32 of +-1, or NULL for all +1.
 *   Per row and per block of `block` consecutive columns, with v in the compute type -- float64 when X is float64 (Y then
 *   must be too), float32 otherwise (Y float32, bfloat16 or float16) -- one rounding per operation, no fused multiply-add:
 *     1. v_i = x_i, converted (exact); transposed == 0: v_i = s_i v_i (a sign flip, exact).
 *     2. for h = 1, 2, 4, ..., block / 2 in this order, every pair (i, i + h) with (i & h) == 0:
 *            (v_i, v_{i+h}) <- (v_i + v_{i+h}, v_i - v_{i+h})        (the upper element takes lower - upper).
 *     3. y_i = v_i c, c the compute-type rounding of 1.0 / sqrt((double)block); transposed != 0: y_i = s_i y_i.
 *     4. y_i converted to y_dtype, round to nearest even (a NaN becomes the quiet NaN 0x7fc0 in bfloat16).
 *   The network fixes the two operands of every addition, so the bits do not depend on how a kernel spreads the stages
 *   over registers, lanes and waves, and a repeated call gives the same bits.  A non-finite element reaches its own block
 *   of its own row and nothing else.  For block a power of 4, c is a power of two and X R R^T == X wherever nothing
 *   overflows or goes subnormal on the way.
 *   In place (Y == X, same dtype) is allowed; any other overlap is not.  No alignment beyond the element's own is asked
 *   for; where X, Y and signs start on 16 bytes and n % 16 == 0 the kernel moves 16 bytes at a time.  No workspace.
 *   SLK_E_ARG, before any launch: block not a power of two in 2 .. 4096, n % block != 0, rows or n < 1, a NULL X or Y, an
 *   unknown dtype, float64 on one side only, rows * ceil(n / 16) above (2^31 - 1) * 256 (one grid covers the matrix: about
 *   8.8e12 elements).  rows may pass 65535 (and 2^31).                                                                  */
#define SLK_DTYPE_F64 3 /* slk_hadamard_rows only */
int slk_hadamard_rows(const void *X, int x_dtype, void *Y, int y_dtype, long long rows, int n, int block,
                      const float *signs, int transposed, slk_stream_t stream);

/* MXFP4 activations: W4A4 on the block-scaled MFMA (both operands E2M1: twice the E4M3 rate, half the activation bytes).
 * X is M x K row-major, K % 32 == 0, float32, bfloat16 or float16.
 *   - a_scales: uint8 M x K / 32, E8M0: the MXFP8 rule above with 6 in place of 448.  Per block, b0 = max(amax / 6, 1e-16)
 *     in float32, the scale s the smallest power of two >= b0, the byte its exponent + 127.  A block of zeros gives byte 74.
 *     The scale does not saturate.
 *   - elements: x / s (exact) rounded to nearest on the E2M1 grid 0, .5, 1, 1.5, 2, 3, 4, 6, ties to the even code
 *     (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), magnitudes clamped at 6; code = sign << 3 |
 *     magnitude index.  A zero magnitude is written as 0x0, never 0x8.
 *   - a_codes: uint8 M x K / 2, the even k in the low nibble: the weights' own layout, so slk_mx_dequantize reads it.
 *   Known answers: a block whose amax is 6.0 has byte 127 and its elements 6, -0.3, 0.75, 2.5 the codes 7 9 2 4; amax 1.0
 *   gives byte 125 (s = 0.25) and 1.0, -1.0, 0.3, 0.0625 the codes 6 e 2 0.
 * slk_mx_quantize_act4: X -> a_codes, a_scales.  flag[0] = 1 (DEVICE int, zeroed by the call, required) if X holds a NaN or
 *   an infinity; the outputs are then not meaningful.  Arguments and refusals as slk_mx_quantize_act.
 * slk_mx_gemm_a4: slk_mx_gemm with such activations (a_codes M x K / 2): the same contract -- exact products, float32 sums
 *   inside the MFMA over K in a fixed order, no atomics, a repeated call gives the same bits, any M, N >= 1 -- and the
 *   same refusals.
 * slk_mx_rotate_quantize_act: the rotation of slk_hadamard_rows fused into the quantizer.  a_codes, a_scales and flag are,
 *   bit for bit, those of slk_hadamard_rows(X -> float32 Y, transposed = 0) followed by slk_mx_quantize_act (fmt
 *   SLK_MX_ACT_FP8; a_codes rows x n) or slk_mx_quantize_act4 (SLK_MX_ACT_FP4; rows x n / 2) on Y: steps 1 to 3 of the
 *   transform's contract unchanged, no step-4 rounding, then the quantizer on the float32 value.  Y is never written: the
 *   call reads X and writes the codes.  block: a power of two in 2 .. 4096 dividing n; n % 32 == 0; signs n float32 or NULL.
 *   SLK_E_ARG, before any launch, slk_last_error() naming the offender: such a block or n, rows < 1, a NULL X, a_codes,
 *   a_scales or flag, an unknown x_dtype (float64 included) or fmt, X, signs or a_codes off 16-byte alignment, the grid
 *   limit of slk_hadamard_rows. */
#define SLK_MX_ACT_FP8 0
#define SLK_MX_ACT_FP4 1
int slk_mx_quantize_act4(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag,
                         slk_stream_t stream);
int slk_mx_gemm_a4(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                   const float *bias, int M, int N, int K, int out_dtype, void *out, slk_stream_t stream);
int slk_mx_rotate_quantize_act(const void *X, int x_dtype, long long rows, int n, int block, const float *signs, int fmt,
                               uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream);

/* MXFP6 activations: W4A6 on the block-scaled MFMA (A in E2M3, cbsz = 2: the E2M1 rate -- FP6 runs at the FP4 rate on this
 * chip -- on three quarters of MXFP8's activation bytes, with E4M3's three mantissa bits inside a block).
 * X is M x K row-major, K % 32 == 0, float32, bfloat16 or float16.  Blocks of 32 along K, one E8M0 byte per (row, block).
 *   - a_scales: uint8 M x K / 32, E8M0: the MXFP8 rule above with 7.5 in place of 448.  Per block, b0 = max(amax /
 *     float32(7.5), float32(1e-16)) in float32 (amax the block's largest |x| as float32), the scale s the smallest power of
 *     two >= b0, the byte its exponent + 127.  A block of zeros gives byte 74.  The scale does not saturate.
 *   - elements: x / s (exact) rounded to nearest onto OCP E2M3: bias 1, no infinities or NaNs, subnormals m / 8 (m = 0 ..
 *     7), normals 2^(e - 1) (1 + m / 8) for e = 1 .. 3 -- the 32 magnitudes 0, 0.125 .. 1.875 in steps of 0.125, 2 .. 3.75
 *     in steps of 0.25, 4 .. 7.5 in steps of 0.5.  Ties go to the even code (every midpoint, those at 1 / 2 / 4 where the
 *     spacing changes included, lies between an odd and an even code), magnitudes are clamped at 7.5.
 *     code = sign << 5 | e << 3 | m.  A zero magnitude is written as 0x00, never 0x20.
 *   - a_codes: uint8 M x 3 K / 4.  A row is a little-endian bit stream, element k at bits 6 k .. 6 k + 5: a block is 24
 *     bytes, and four elements c0 .. c3 make the three bytes of c0 | c1 << 6 | c2 << 12 | c3 << 18.  a_codes must start on
 *     16 bytes; rows then start on 8.
 *   Known answers: amax 7.5 gives byte 127, and 7.5, -0.3, 0.0625, 0.1875 the codes 1f 22 00 02 (0.0625 ties to 0, 0.1875
 *   to 0.25), bytes 9f 08 08; amax 1.0 gives byte 125, and 1.0, -1.0, 0.3, 0.0625 the codes 18 38 0a 02, bytes 18 ae 08;
 *   under amax 7.5, 1.0625, 3.9, -3.875, 5.25 give 08 18 38 1a, bytes 08 86 6b; amax 1.75 gives byte 125 and +-1.75 the
 *   codes 1e / 3e; amax 1e-20 gives byte 74 and all codes 0.
 * slk_mx_quantize_act6: X -> a_codes, a_scales.  flag[0] = 1 (DEVICE int, zeroed by the call, required) if X holds a NaN or
 *   an infinity; the outputs are then not meaningful.
 * slk_mx_dequantize_act6: out[m][k] = value(code) * 2^(b - 127), M x K: exact in float32, or that value rounded once to
 *   nearest even as bfloat16 / float16.  flag (may be NULL): 1 if a scale byte is 255.
 * slk_mx_gemm_a6: slk_mx_gemm with such activations (a_codes M x 3 K / 4): the same contract -- exact products (4 + 2
 *   significant bits), float32 sums inside the MFMA over K in a fixed order, no atomics, a repeated call gives the same
 *   bits, any M, N >= 1.  Nothing past the 3 M K / 4 bytes of a_codes is read.
 * slk_mx_rotate_quantize_act6: slk_mx_rotate_quantize_act for this format: a_codes (rows x 3 n / 4), a_scales and flag are,
 *   bit for bit, those of slk_hadamard_rows(X -> float32 Y, transposed = 0) followed by slk_mx_quantize_act6 on Y.
 * SLK_E_ARG, before any launch, slk_last_error() naming the offender: K (n) % 32 != 0 or < 32, M, N or rows < 1, a NULL
 *   required pointer (bias and the de-quantizer's flag may be NULL), an unknown dtype, X, a_codes, w_codes, signs or out off
 *   16-byte alignment; for the rotation also what slk_mx_rotate_quantize_act refuses of block and grid.                  */
int slk_mx_quantize_act6(const void *X, int x_dtype, int M, int K, uint8_t *a_codes, uint8_t *a_scales, int *flag,
                         slk_stream_t stream);
int slk_mx_dequantize_act6(const uint8_t *a_codes, const uint8_t *a_scales, int M, int K, int out_dtype, void *out, int *flag,
                           slk_stream_t stream);
int slk_mx_gemm_a6(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                   const float *bias, int M, int N, int K, int out_dtype, void *out, slk_stream_t stream);
int slk_mx_rotate_quantize_act6(const void *X, int x_dtype, long long rows, int n, int block, const float *signs,
                                uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream);

/* MXFP6 layers: E2M3 weights, 6.25 bits a weight, W6A8 / W6A6 on the block-scaled MFMA (B in E2M3, blgp = 2: FP6 operands
 * run at the FP4 rate on this chip).  Blocks and `scales` are MXFP4's (above), byte 255 included; only the elements differ.
 *   - elements: OCP E2M3, code = sign << 5 | e << 3 | m, exactly the MXFP6 activations' values (above).
 *   - the codebook is the 63-entry table -7.5 .. 7.5 (the 31 non-zero magnitudes on both sides of 0) whose limits are the
 *     midpoints, a tie going upward.  Table index i < 31 is code 0x20 | (31 - i), otherwise i - 31.  Code 0x20 (-0) is
 *     never written and reads back as index 31, value +0; an index above 62 is a caller error and is stored as code 0x1f.
 *   - codes: uint8 R x 3 n / 4.  A row is a little-endian bit stream, element k at bits 6 k .. 6 k + 5: a block is 24 bytes
 *     and four elements c0 .. c3 make the three bytes of c0 | c1 << 6 | c2 << 12 | c3 << 18 -- the MXFP6 activations' form,
 *     so slk_mx_dequantize_act6(codes, scales) rebuilds Q = value(idx) / (1 / s) bit for bit.  codes must start on 16
 *     bytes; rows then start on 8.
 *   Known answers: indices 0, 1, 30, 31, 32, 61, 62 are codes 3f 3e 21 00 01 1e 1f; columns with codes [01, 02, 3f, 00] pack
 *   to bytes [81, f0, 03]; indices [0, 62, 31, 32] pack to bytes [ff, 07, 04]; the scale 0.0078125 is byte 120.
 * slk_mx_scale_search6: slk_mx_scale_search with E2M3 and 7.5 in place of E2M1 and 6: b0 = max(max / 7.5, min / -7.5, 1e-16),
 *   base the smallest power of two >= b0, the same modes, factors, float32 row sums and first minimum.
 * slk_mx_pack6 / slk_mx_unpack6: slk_mx_pack's / slk_mx_unpack's contracts (either pair may be NULL, the same scale checks
 *   and flag) with the index <-> code map and the stream above.
 * slk_mx_gemm_w6: slk_mx_gemm against such a layer (w_codes N x 3 K / 4): a_fmt SLK_MX_ACT_FP8 (a_codes M x K, W6A8) or
 *   SLK_MX_ACT_FP6 (a_codes M x 3 K / 4, W6A6); SLK_MX_ACT_FP4 is refused.  The same contract -- exact products, float32
 *   sums inside the MFMA over K in a fixed order, no atomics, a repeated call gives the same bits, any M, N >= 1.  Nothing
 *   past the 3 N K / 4 bytes of w_codes is read.
 * SLK_E_ARG as for their MXFP4 twins, and an a_fmt other than the two above.                                          */
#define SLK_MX_ACT_FP6 2
int slk_mx_scale_search6(const float *W, const float *hdiag, int mode, int R, int n, uint8_t *scales, float *S,
                         slk_stream_t stream);
int slk_mx_pack6(const uint8_t *idx, const float *S, int R, int n, uint8_t *codes, uint8_t *scales, int *flag,
                 slk_stream_t stream);
int slk_mx_unpack6(const uint8_t *codes, const uint8_t *scales, int R, int n, uint8_t *idx, float *S, int *flag,
                   slk_stream_t stream);
int slk_mx_gemm_w6(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                   const float *bias, int M, int N, int K, int a_fmt, int out_dtype, void *out, slk_stream_t stream);

/* A mixture-of-experts layer in one call: E packed layers of one shape N x K, every row of A multiplied with the layer of
 * its expert.  The rows are sorted by expert, and `offsets` -- E + 1 ints in DEVICE memory, never read by the host -- says
 * where each expert's rows are: rows offsets[e] .. offsets[e + 1] - 1 of A and of out (M x N) belong to expert e.
 *   - w_codes: the E layers one after the other, E x N x (K bits / 8) bytes, expert e's at byte e * N * (K / 32) * 16
 *     (SLK_MX_W_FP4, E2M1) or * 24 (SLK_MX_W_FP6, E2M3); w_scales E x N x K / 32; bias E x N float32, may be NULL.
 *   - a_codes / a_scales: M rows as the activation quantizers write them; a_fmt SLK_MX_ACT_FP8, _FP4 or _FP6.  The pairs
 *     are the dense entries': the three activation formats against SLK_MX_W_FP4, and SLK_MX_ACT_FP8 or SLK_MX_ACT_FP6
 *     against SLK_MX_W_FP6; SLK_MX_ACT_FP4 against SLK_MX_W_FP6 is refused.
 *   - for the rows of expert e, out[m][n] = sum_k A[m][k] W_e[n][k] (+ bias[e][n]) under slk_mx_gemm's contract -- exact
 *     products, float32 sums inside the MFMA over K in a fixed order, no atomics, a repeated call gives the same bits --
 *     and BIT FOR BIT what slk_mx_gemm / _a4 / _a6 / _w6 gives for that slice of A alone against that expert's layer: an
 *     expert with up to 64 rows takes the dense entries' few-rows form, one with more their many-rows form.
 *   - offsets rule: offsets[0] == 0, offsets[e] <= offsets[e + 1], offsets[E] == M (an expert may have no rows).  It is
 *     checked on the device before any address is made from an offset: if it does not hold, flag[0] = 1 and out is not
 *     written.  flag: DEVICE int, required, written by the call (0 where the rule holds).
 *   - workspace: slk_mx_experts_workspace_bytes(E, M) bytes, aligned to 4; it holds the row tiles of the call (as ints:
 *     the number of 16-row and of 64-row tiles at [0] and [1], from [4] the M / 16 + E entries (expert, first row, row
 *     bound) of the 16-row tiles, after them the M / 64 + E entries of the 64-row tiles).
 *   Everything runs in order on `stream`: nothing waits on another workgroup, and the host reads nothing.  Nothing is read
 *   past a_codes, w_codes, w_scales or bias of exactly the sizes above.
 * SLK_E_ARG, before any launch, slk_last_error() naming the offender: E < 1 or E > SLK_MX_MAX_EXPERTS, M or N < 1, K % 32
 *   != 0 or K < 32, a NULL pointer other than bias, an unknown dtype, a_fmt or w_fmt, the refused pair, a_codes, w_codes or
 *   out off 16-byte alignment, a workspace off 4 bytes or below slk_mx_experts_workspace_bytes(E, M), M / 64 + E above the
 *   65535 row tiles of one launch.  slk_mx_experts_workspace_bytes is 0 for E or M < 1.                                */
#define SLK_MX_W_FP4 0
#define SLK_MX_W_FP6 1
#define SLK_MX_MAX_EXPERTS 1024
size_t slk_mx_experts_workspace_bytes(int E, int M);
int slk_mx_gemm_experts(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                        const float *bias, const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, int out_dtype,
                        void *out, int *flag, void *workspace, size_t ws_bytes, slk_stream_t stream);

/* A gated MLP, down(act(gate(x)) * up(x)), between its two products.  The gate, all float32, every operation rounded once
 * (no multiply contracted with an add), the same exp at every site:
 *     g' = g > limit ? limit : g                          (a NaN passes through; limit = +inf: no clamp)
 *     u' = u > limit ? limit : (u < -limit ? -limit : u)
 *     s  = 1 / (1 + exp(-(alpha g')))
 *     h  = (u' + shift) (g' s)
 *   alpha = 1, limit = +inf, shift = 0: SwiGLU (Llama, Mixtral, Qwen); alpha = 1.702, limit = 7, shift = 1: gpt-oss.
 *   `interleaved` says where gate and up of hidden column j are among 2 N columns (of Y) or rows (of the layer, of its bias):
 *   0: gate j, up N + j;  1: gate 2 j, up 2 j + 1 (gpt-oss).
 *
 * slk_mx_glu: H (M x N, out_dtype) = h of Y (M x 2 N; float32, bfloat16 or float16 by x_dtype), the float32 h rounded once.
 *
 * slk_mx_gemm_glu: the product of a_codes / a_scales (M x K, format a_fmt, as slk_mx_quantize_act* writes them) with a layer of
 *   2 N rows (w_codes, w_scales; w_fmt; the pairs of slk_mx_gemm_experts), + bias (2 N float32, may be NULL) in float32, the
 *   gate, and the quantizer of a_fmt on h, in one launch: h_codes (M x N bits / 8) and h_scales (M x N / 32) are bit for bit
 *   what slk_mx_gemm* to float32, slk_mx_glu to float32 and slk_mx_quantize_act* of that format write.  The gate and up sums
 *   are slk_mx_gemm's to float32 bit for bit (M <= 64: its few-rows form, above: its many-rows form).  N % 32 == 0.
 *   flag: DEVICE int that the CALLER zeroes; the call sets it to 1, and never clears it, when a block of h holds a NaN or an
 *   infinity (the quantizers' rule).  Rows >= M and everything outside h_codes / h_scales of exactly these sizes are neither
 *   read nor written.
 *
 * slk_mx_gemm_glu_experts: the same over rows sorted by expert (slk_mx_gemm_experts: offsets, workspace of
 *   slk_mx_experts_workspace_bytes(E, M), the same prologue); w_codes E x 2 N x (K bits / 8), w_scales E x 2 N x K / 32, bias
 *   E x 2 N.  flag: TWO device ints: flag[0] the offsets rule, written by the call; flag[1] the non-finite rule, zeroed by the
 *   caller.  Offsets that break the rule leave h_codes and h_scales untouched.  Each expert's rows are bit for bit
 *   slk_mx_gemm_glu of that slice.
 *
 * slk_mx_gemm_glu_rot, slk_mx_gemm_glu_experts_rot: slk_mx_gemm_glu / _experts for a down layer that sits behind a block
 *   Hadamard rotation of the N hidden columns, R = diag(s) blockdiag(H_block) / sqrt(block) of slk_hadamard_rows, with a block
 *   of 2, 4, 8, 16 or 32: a block of R then lies inside one MX block of h, and the product's epilogue rotates each row's block
 *   before it quantizes it, still in one launch.  signs: N float32 of +-1, DEVICE, aligned to 16 bytes, or NULL for all +1; the
 *   expert form shares the one rotation among all experts.  h_codes, h_scales and the flag(s) are bit for bit those of
 *   slk_mx_gemm* to float32, slk_mx_glu to float32 and slk_mx_rotate_quantize_act / _act6 with that block and those signs:
 *   steps 1 to 3 of slk_hadamard_rows (transposed == 0) on the float32 h -- v = s h; the butterflies for h = 1, 2, ...,
 *   block / 2 in that order, lower + upper and lower - upper; y = v c, c the float32 rounding of 1 / sqrt((double)block) -- with
 *   no rounding in between, then the quantizer of a_fmt.  The flags are those of the plain entries: a NaN or an infinity
 *   anywhere in a block of h reaches its whole Hadamard block and raises the non-finite flag (the outputs are then not
 *   meaningful, as for the quantizers).  Blocks above 32 are not taken here: a caller runs the three entries named above.
 *
 * SLK_E_ARG, before any launch: M < 1, N no positive multiple of 32 (slk_mx_glu: N < 1), K as in slk_mx_gemm, a NULL pointer
 *   other than bias, an unknown dtype, a_fmt or w_fmt, the refused pair, Y, H, a_codes, w_codes or h_codes off 16-byte
 *   alignment, limit not above 0 (a NaN included), alpha or shift not finite, interleaved not 0 or 1, and for the experts
 *   what slk_mx_gemm_experts refuses; for the _rot entries also a block that is no power of two in 2 .. 32 and signs off
 *   16-byte alignment.                                                                                                 */
int slk_mx_glu(const void *Y, int x_dtype, int M, int N, float alpha, float limit, float shift, int interleaved, int out_dtype,
               void *H, slk_stream_t stream);
int slk_mx_gemm_glu(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                    const float *bias, int M, int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift,
                    int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag, slk_stream_t stream);
int slk_mx_gemm_glu_experts(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                            const float *bias, const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, float alpha,
                            float limit, float shift, int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag,
                            void *workspace, size_t ws_bytes, slk_stream_t stream);
int slk_mx_gemm_glu_rot(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                        const float *bias, int M, int N, int K, int a_fmt, int w_fmt, float alpha, float limit, float shift,
                        int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag, int block, const float *signs,
                        slk_stream_t stream);
int slk_mx_gemm_glu_experts_rot(const uint8_t *a_codes, const uint8_t *a_scales, const uint8_t *w_codes, const uint8_t *w_scales,
                                const float *bias, const int *offsets, int E, int M, int N, int K, int a_fmt, int w_fmt, float alpha,
                                float limit, float shift, int interleaved, uint8_t *h_codes, uint8_t *h_scales, int *flag,
                                void *workspace, size_t ws_bytes, int block, const float *signs, slk_stream_t stream);

/* A stored MX layer against 16-bit activations, weight-only (W4A16, W6A16): the layer as slk_mx_pack / slk_mx_pack6 left it,
 * de-quantized inside a bfloat16 / float16 MFMA GEMM (v_mfma_f32_16x16x32_bf16 / _f16).  No de-quantized weight is written
 * to memory, nothing quantizes the activations, and the dense call is one launch without a workspace.
 * slk_mx_gemm_a16: out[m][n] = sum_k Xc[m][k] Wc[n][k] (+ bias[n]) for a layer of N rows (output features) and K columns:
 *   - Wc is what the layer's de-quantizer writes in the compute type, slk_mx_dequantize (w_fmt SLK_MX_W_FP4, E2M1; w_codes
 *     N x K / 2) or slk_mx_dequantize_act6 (SLK_MX_W_FP6, E2M3; w_codes N x 3 K / 4) with out_dtype = compute_dtype:
 *     value(code) 2^(b - 127) in float32, b the block's byte of w_scales (N x K / 32), rounded once to nearest even;
 *   - Xc is X (M x K row-major, `x_dtype`: float32, bfloat16 or float16) rounded to nearest even to the compute type through
 *     float32 (the identity when it has it);
 *   - compute_dtype is SLK_DTYPE_BF16 or SLK_DTYPE_F16; the products are exact in float32, the sums float32 inside the MFMA
 *     over K in a fixed order (no atomics: a repeated call gives the same bits); the float32 bias (N, may be NULL) is added
 *     in float32 and the result rounded once to `out_dtype` (M x N row-major).
 *   Exactness.  The operand contract is promised where every non-zero Wc is a NORMAL number of the compute type: scale bytes
 *   10 .. 245 for bfloat16 (as slk_hessian_accumulate_experts_mx words it), 116 .. 140 for float16.  Outside these ranges Wc
 *   is still the de-quantizer's value for every scale byte -- the float32 product rounded to nearest even: a subnormal, a
 *   zero or an infinity of the compute type -- and what a subnormal operand then contributes is the MFMA's own treatment of
 *   subnormals, which this library does not examine.  (One bit of Wc differs from the de-quantizer's and no sum can show it:
 *   the E2M1 code 0x8 is -0 where the de-quantizer writes +0.)  Scale byte 255 is not looked for: its block's products are
 *   NaN, as in slk_mx_gemm.  X is not looked at for NaN or infinity either: they propagate as in any GEMM.
 *   Up to M = 64 a workgroup is one 16 x 16 tile of out whose 8 waves share K (the layer is read once per 16 rows); above, a
 *   workgroup is a 64 x 64 tile that de-quantizes its weights into LDS -- the switch of slk_mx_gemm.
 * slk_mx_gemm_experts_a16: the same over the E layers of a mixture-of-experts layer, rows sorted by expert, under
 *   slk_mx_gemm_experts' rules word for word: w_codes / w_scales / bias E layers one after the other, offsets (DEVICE, E + 1
 *   ints) and their rule, flag (DEVICE int, written by the call; 1 and out untouched where the rule breaks), an expert
 *   without rows, the workspace of slk_mx_experts_workspace_bytes(E, M) and its layout, three launches in order on `stream`.
 *   Each expert's rows are BIT FOR BIT slk_mx_gemm_a16 on that slice of X with that expert's layer and bias.
 * SLK_E_ARG, before any launch, slk_last_error() naming the offender: M or N < 1, K % 32 != 0 or K < 32, a NULL X, w_codes,
 *   w_scales or out, an unknown x_dtype, out_dtype or w_fmt, compute_dtype not BF16 or F16, X, w_codes or out off 16-byte
 *   alignment, ceil(M / 64) above the 65535 row tiles of one launch; for the experts what slk_mx_gemm_experts refuses. */
int slk_mx_gemm_a16(const void *X, int x_dtype, const uint8_t *w_codes, const uint8_t *w_scales, int w_fmt, const float *bias,
                    int M, int N, int K, int compute_dtype, int out_dtype, void *out, slk_stream_t stream);
int slk_mx_gemm_experts_a16(const void *X, int x_dtype, const uint8_t *w_codes, const uint8_t *w_scales, int w_fmt,
                            const float *bias, const int *offsets, int E, int M, int N, int K, int compute_dtype, int out_dtype,
                            void *out, int *flag, void *workspace, size_t ws_bytes, slk_stream_t stream);

/* MoE routing: from router logits to the combined output around the grouped products above, every step a launch on `stream`
 * -- top-k gates, the stable sort by expert, the activation quantizer behind a row map, the gate-weighted sum.  T tokens take
 * k experts of E each: n = T k routed rows, entry t k + j the j-th choice of token t.  All pointers are DEVICE pointers; the
 * host reads nothing.  Two rules hold for every kernel: no workgroup waits for another (order comes from the launches alone),
 * and no address is made from an index read from device memory before it has been checked against its range -- a bad index
 * raises the call's flag, and neither reads nor writes anything.  Every flag is zeroed by its call, as slk_mx_quantize_act's.
 *
 * slk_moe_topk: logits (T x E; float32, bfloat16 or float16 by `dtype`, converted to float32, which is exact) -> expert_ids
 *   (int32 T x k) and gates (float32 T x k).
 *   - selection: column j is the j-th largest logit of the token; expert a ranks before expert b when v[a] > v[b], or when
 *     v[a] == v[b] and a < b: +0 and -0 tie, and of equal values the lower index wins.
 *   - gates, all float32, every operation rounded once, nothing contracted: m = the token's largest logit, e = expf(v - m),
 *     g = e / s (the IEEE quotient).  SLK_MOE_GATE_SELECTED: s is the sum of the k selected e's -- a softmax over the selected
 *     logits (gpt-oss; also Mixtral's and Qwen3's softmax, top-k, renormalise, the same function) -- as the tree
 *     ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)) + the same of e8 .. e15, an absent e being +0.  SLK_MOE_GATE_ALL: s is
 *     the sum over all E experts, the selected probabilities left as they are: with a[l] = e[l] + e[l + 64] + e[l + 128] + ...
 *     from left to right for l = 0 .. 63, r[i] that tree over a[16 i] .. a[16 i + 15], s = (r[0] + r[1]) + (r[2] + r[3]).
 *   - flag[0] = 1 when a token's row holds a NaN or +inf, or fewer than k of its logits are above -inf (-inf is otherwise
 *     legal: it masks an expert).  Whatever the logits, the ids written lie in 0 .. E - 1 and are distinct within a token; a
 *     flagged token's gates are 0.
 *   One wave a token, the token's logits in registers, no LDS, no barrier.
 * slk_moe_sort: the stable counting sort of n int32 expert ids.  order[p] (int32 n) is the entry t k + j that is p-th in
 *   sorted order -- ids ascending, equal ids in their original order --, pos (int32 n) its inverse, pos[order[p]] == p, and
 *   offsets (int32 E + 1) where each expert's rows begin: the rule of slk_mx_gemm_experts, offsets[0] == 0, offsets[e] <=
 *   offsets[e + 1], offsets[E] == n.  An id outside 0 .. E - 1 raises flag[0] and is clamped into the range for the sort, so
 *   the outputs obey the rule whatever the ids.  The result does not depend on timing (counts are integer atomics in LDS,
 *   whose sums commute; no place comes from an atomic's return value): a repeated call gives the same bits.  n <= 1024 is one
 *   launch of one workgroup and needs no workspace (NULL, 0 are taken); above, three launches -- counts per chunk of 2048
 *   entries (from 2^21 entries up: of ceil(n / 1024) rounded up to 64), their scan in expert-major order, the placement -- and
 *   slk_moe_sort_workspace_bytes(n, E) = 4 E chunks bytes, aligned to 4.  slk_moe_sort_workspace_bytes is 0 for n <= 1024 and
 *   for sizes the sort refuses.
 * slk_mx_quantize_act_rows: slk_mx_quantize_act (a_fmt SLK_MX_ACT_FP8), _act4 (_FP4) or _act6 (_FP6) behind a row map: row i
 *   of a_codes / a_scales, i < M, is the quantization of row rows[i] / div of X (T x K): BIT FOR BIT what that entry writes
 *   for the gathered matrix, which is never in memory.  The route calls it with rows = order, div = k, M = n.  flag is TWO
 *   ints: flag[0] = 1 for a NaN or an infinity in a row that is mapped (rows that are not are not read); flag[1] = 1 for a
 *   source row outside 0 .. T - 1, whose blocks are encoded from zeros and load nothing.
 * slk_moe_combine: out[t][c] = sum_j gates[t][j] * Y[pos[t k + j]][c] for Y (n x N, y_dtype) and out (T x N, out_dtype): Y
 *   converted to float32, each product rounded, then each add rounded, in the order j = 0, 1, ..., k - 1 starting from the
 *   first term itself, the sum rounded once to out_dtype (to nearest even).  gates == NULL means ones, and no multiply.  A
 *   pos outside 0 .. n - 1 raises flag[0] and its term is left out.  No atomics: a repeated call gives the same bits.  Where
 *   N is a multiple of a 16-byte piece of Y (4 float32, 8 of a 16-bit type) a thread moves such a piece; otherwise rows do
 *   not start on 16-byte boundaries and every column goes alone.
 * SLK_E_ARG, before any launch, slk_last_error() naming the offender: a NULL pointer other than combine's gates and a sort's
 *   unneeded workspace; logits off its element's alignment, X, a_codes, Y or out off 16 bytes, any other pointer off 4; E < 1
 *   or E > SLK_MX_MAX_EXPERTS; k < 1, k > E or k > SLK_MOE_MAX_K (slk_moe_topk; slk_moe_combine takes any k >= 1); an unknown
 *   dtype, gating or a_fmt; T, N, M or n < 1; K % 32 != 0 or K < 32; div < 1; a workspace below
 *   slk_moe_sort_workspace_bytes(n, E); n = T k (M for the quantizer) above 2^24.                                       */
#define SLK_MOE_GATE_SELECTED 0
#define SLK_MOE_GATE_ALL 1
#define SLK_MOE_MAX_K 16
int slk_moe_topk(const void *logits, int dtype, int T, int E, int k, int gating, int *expert_ids, float *gates, int *flag,
                 slk_stream_t stream);
size_t slk_moe_sort_workspace_bytes(int n, int E);
int slk_moe_sort(const int *expert_ids, int n, int E, int *order, int *pos, int *offsets, int *flag, void *workspace,
                 size_t ws_bytes, slk_stream_t stream);
int slk_mx_quantize_act_rows(const void *X, int x_dtype, int T, int K, const int *rows, int div, int M, int a_fmt,
                             uint8_t *a_codes, uint8_t *a_scales, int *flag, slk_stream_t stream);
int slk_moe_combine(const void *Y, int y_dtype, const int *pos, const float *gates, int T, int k, int N, void *out,
                    int out_dtype, int *flag, slk_stream_t stream);

/* a11 channelwise_error  (sleekit/obq.py:89-95): row_err[r] = (W-Q)[r] H (W-Q)[r]^T.
 *     G (may be NULL): the R x n product (W - Q) @ H, reused by the local search. */
int slk_row_errors(const float *W, const float *Q, const float *H, int R, int n, float *row_err,
                   float *G, void *workspace, size_t ws_bytes, slk_stream_t stream);
/*     ... of `batch` layers stacked by rows (see slk_gptq_quantize_batch): H is a HOST array of `batch` device
 *     pointers, one n x n Hessian each; batch > 1 needs rows_per_layer % 128 == 0.                          */
int slk_row_errors_batch(const float *W, const float *Q, const float *const *H, int batch, int rows_per_layer,
                         int n, const int *symmetric, float *row_err, void *workspace, size_t ws_bytes,
                         slk_stream_t stream);
/*     The error of a bit-wise symmetric H takes half the products; the verdict is reached on the device.
 *     `symmetric` (device, `batch` ints, may be NULL = checked inside): verdicts from slk_symmetry_flag, so that
 *     ranks sharing a Hessian check it once (the factor's root) instead of once each.  flag[0] = 1 iff
 *     H[i][j] == H[j][i] bit for bit.                                                                   */
int slk_symmetry_flag(const float *H, int n, int *flag, slk_stream_t stream);

/* a12+a13 quantize_local_search  (sleekit/obq.py:220-358)
 *     W, Q: R x n float32 in the scaled domain; Q is updated in place, idx
 *     (may be NULL) receives the indices of the result.  `moves` best-first
 *     single-weight moves per row.  The interaction sum of every move (obq.py:328) is taken in NumPy's
 *     pairwise order, so that from equal initial gains the moves are the reference's bit for bit.
 *     trace (may be NULL): R x moves int32, the moves taken -- 2 * column + (1: up, 0: down), or -1 from
 *     the first move on at which the row had nothing left to gain (parity tests compare it with the
 *     reference's sequence of moves to find where, if anywhere, a near-tie fell the other way).  A "move" onto the
 *     value a weight already holds changes nothing and the reference repeats it until its moves run out: the search
 *     of that row ends there and the trace says -1 ("stay") from that move on, where a record of the reference's own
 *     do_move() calls would show the repeated non-move.  (The carried gains of gains_mode 1 / 2 then lack the reference's
 *     additions of +0.0: at most the sign of a zero differs.)
 *     gains / gains_mode: the state of the reference's stateful LocalSearchQuantizer (obq.py:234-346) between calls --
 *     R x 2 x n float32, per row the n up-gains then the n down-gains.  gains_mode 0: none (gains may be NULL);
 *     1: the initial gains are built from (W - Q) H as usual, and the gains after the moves are stored (moves == 0
 *     gives the constructor's state, obq.py:259-262); 2: the gains are LOADED, the moves made, the gains stored --
 *     k calls with moves = 1 are then one call with moves = k, bit for bit, like k calls of do_move().
 *     row_err (may be NULL; gains_mode 0 or 1): R float32, the rows' errors (W - Q) H (W - Q)^T AFTER the moves, in the domain of
 *     W and Q: the error before them comes out of the product that makes the initial gains, and every move takes its gain off
 *     it -- how the reference's LocalSearchQuantizer carries `err` (obq.py:254, 290) -- so the layer error of a searched layer
 *     needs no product of its own (a row shard of BLOOM-560M spent as long on that product as on the search).                */
int slk_local_search(const float *W, float *Q, const float *H, int R, int n, int levels, double lo,
                     double hi, const float *table, int moves, uint8_t *idx, int *trace, float *gains,
                     int gains_mode, float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream);
/* The same search over `batch` layers of one shape stacked by rows (rows [b R, (b + 1) R) of W, Q, idx against H[b], a
 * HOST array of `batch` device pointers; R = rows_per_layer, a multiple of 128 when batch > 1): the results of `batch`
 * separate calls bit for bit, in ONE product and ONE launch of moves -- the row shards of a round on several ranks (a few
 * hundred rows per layer) are bound by the host's launch rate otherwise.  symmetric: as in slk_row_errors_batch (may be NULL).
 * row_err (may be NULL): batch * rows_per_layer float32, the rows' errors after the moves (see slk_local_search).
 * Workspace: slk_workspace_bytes_batch(batch, rows_per_layer, n).                                                     */
int slk_local_search_batch(const float *W, float *Q, const float *const *H, int batch, int rows_per_layer, int n,
                           int levels, double lo, double hi, const float *table, int moves, uint8_t *idx,
                           const int *symmetric, float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream);
/* slk_local_search with the GROUP QUANTIZER of gscale (R x n / group_size float32, positive; group_size >= 1 divides n): the
 * candidates of element (r, c) are codebook.quantize_up / quantize_down(x / s) / (1 / s) with s = gscale[r][c / group_size],
 * float32 IEEE divides (sleekit/obq.py:234-346 with that quantizer, on W unscaled, Q de-scaled and H undamped in original column
 * order).  Gains, moves, `trace`, `row_err`, the refusals and the workspace are slk_local_search's; there are no carried gains.
 * idx (may be NULL; levels <= 256): the codebook indices of Q / s, from which slk_dequantize_grouped rebuilds Q bit for bit.  */
int slk_local_search_grouped(const float *W, float *Q, const float *H, const float *gscale, int group_size, int R, int n,
                             int levels, double lo, double hi, const float *table, int moves, uint8_t *idx, int *trace,
                             float *row_err, void *workspace, size_t ws_bytes, slk_stream_t stream);

/* Scale selection: the callers' pre-step -------------------------- */
/* compute_non_saturating_scaling (sleekit/scaling.py:44-55): scale[r] = max(max_r / hi_code,
 * min_r / lo_code, 1e-16) with the codebook's extreme values lo_code < 0 < hi_code; NaN for a
 * row that holds a NaN, like NumPy's min / max / maximum (slk_scale_norm likewise).          */
int slk_scale_minmax(const float *W, int R, int n, double lo_code, double hi_code, float *scale,
                     slk_stream_t stream);
/* compute_norm_scaling (sleekit/scaling.py:35-41): sqrt(max(mean(row^2), 1e-16)), float32,
 * row sums in NumPy's pairwise order.                                                        */
int slk_scale_norm(const float *W, int R, int n, float *scale, slk_stream_t stream);
/* compute_min_mse_scaling with H = None (hdiag NULL) or a diagonal Hessian (sleekit/scaling.py:
 * 84-134): for each factor f (float32, in order) quantize the row round-to-nearest with scale
 * f * base[r], take the error sum_j [hdiag_j] E_j^2 in NumPy's summation order, keep the first
 * minimum; out[r] = base[r] * best factor.                                                   */
int slk_scale_search(const float *W, const float *base, const float *factors, int n_factors,
                     const float *hdiag, int R, int n, int levels, double lo, double hi, const float *table,
                     float *out, slk_stream_t stream);
/* Book-keeping of the searches whose row errors come from slk_row_errors (full Hessian, OBQ-aware;
 * sleekit/scaling.py:131-133, 187-189): init != 0 resets best_err / best_f to +inf; err != NULL
 * applies `better = err < best_err`.                                                          */
int slk_search_step(const float *err, float factor, int R, float *best_err, float *best_f, int init,
                    slk_stream_t stream);
/* out[r] = a[r] * b[r]  (b != NULL)  or  a[r] * c. */
int slk_scale_times(const float *a, const float *b, float c, int R, float *out, slk_stream_t stream);

/* Diagnostics used by tests ------------------------------------------------ */
/* NumPy-ordered float32 mean of diag(H) -> out[0]. */
int slk_diag_mean(const float *H, int n, float *out, void *workspace, size_t ws_bytes,
                  slk_stream_t stream);
/* Peak probes: every wave of `blocks` 256-thread workgroups issues `iters` x 4 independent
 * v_mfma_f64_16x16x4_f64 (2048 flop each) / v_mfma_f32_32x32x2_f32 (4096 flop each).      */
int slk_probe_mfma_f64(double *sink, int blocks, int iters, slk_stream_t stream);
int slk_probe_mfma_f32(float *sink, int blocks, int iters, slk_stream_t stream);
/* float64 probe with `nacc` (8 or 16) independent accumulators per wave: iters x nacc MFMAs per wave. */
int slk_probe_mfma_f64_acc(double *sink, int blocks, int iters, int nacc, slk_stream_t stream);
/* One wave runs `iters` steps of a dependent chain (mode 0: fma f64, 1: 8 independent fma f64,
 * 2: fma f32, 3: rsq f64, 4: divide f64, 5: divide f32, 6: f64->f32->f64 + mul);
 * out[0] = shader cycles, out[1] = 100 MHz ticks, out[2] = checksum.                      */
int slk_probe_chain(double *out, int iters, int mode, slk_stream_t stream);
/* Debug: cycle counters of workgroup 0 of the window kernel, filled when SLK_WIN_DBG has bit 3 set.
 * host_out: 80 int64 on the HOST (16 counters + 64 per-period entries of the standard-schedule kernel).  Synchronises the device.  No reference counterpart. */
int slk_probe_window_cycles(long long *host_out, int reset);
/* Debug: cycle counters of workgroup 1 (wave 0) of the panel kernel, filled when SLK_WIN_DBG has bit 3 set: 16 int64 on the
 * HOST -- [0] staging, [1] diagonal-tile update, [2] pivot chains, [3] barriers and next-strip blocks, [4] tail up to the last
 * barrier, [5] last column of L21 + stores, [15] launches counted.  Synchronises the device.  No reference counterpart. */
int slk_probe_panel_cycles(long long *host_out, int reset);
/* Debug: the leaf chain alone (32-column leaves, 8-level grid) on one workgroup with one or two waves per
 * SIMD.  out (DEVICE, 2 doubles): cycles wave 0 spent on `iters` leaves, checksum. */
int slk_probe_leaf_chain(double *out, int iters, int waves_per_simd, slk_stream_t stream);

/* Per-launch timing (off by default).  While enabled, every kernel launch is bracketed by
 * HIP events on its own stream.  slk_profile_report synchronises on them and writes a JSON
 * array with, per kernel name, the launch count, total milliseconds and the ALGORITHMIC
 * flops / bytes of those launches (the roofline numerators of DESIGN.md); it returns the
 * length needed, like snprintf.  Do not enable while capturing a hipGraph.          */
int slk_profile_enable(int on);
int slk_profile_reset(void);
int slk_profile_report(char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SLEEKIT_AMD_H */
