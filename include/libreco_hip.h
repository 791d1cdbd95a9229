/*
 * libreco_hip.h — C ABI of the MI355X (gfx950) hot path for LibRecommender.
 *
 * The reference (massquantity/LibRecommender v1.5.2) has no FFI for this path: its
 * "kernels" are TensorFlow / PyTorch / numpy calls made from Python.  Each entry point
 * below therefore cites the reference *call site* it replaces (path:line relative to the
 * reference checkout) instead of an existing binding.  INTEGRATION.md shows the ctypes
 * stub a LibRecommender maintainer would add to call them.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - tensors are dense row-major, fp32 unless stated, indices int32 (the reference feeds
 *     tf.int32 placeholders, e.g. algorithms/deepfm.py:176-177), 64-bit counts/sizes;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); kernels are
 *     enqueued asynchronously, nothing synchronises, nothing allocates;
 *   - scratch memory is provided by the caller (`ws`, `ws_bytes`); the matching
 *     `*_ws_bytes` query is a pure host function;
 *   - return value: LR_OK (0) on success, a negative LR_E* code for argument errors,
 *     or a positive hipError_t from the launch.  `lr_strerror` renders either.
 *   - no global state; safe to call from several host threads on distinct streams.
 */
#ifndef LIBRECO_HIP_H_
#define LIBRECO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LR_OK 0
#define LR_EINVAL (-1)    /* bad argument (null pointer, negative size, ...)            */
#define LR_ESHAPE (-2)    /* shape not supported by the compiled kernels (see function) */
#define LR_EWORKSPACE (-3) /* workspace too small                                        */

typedef void* lr_stream_t;

const char* lr_strerror(int code);
/* ABI version of this header: bumped on any signature change. */
int lr_abi_version(void);
/* Nodes of a captured hipGraph (a hipGraph_t) that are neither kernel nor empty nodes — a captured training step must hold
 * kernel nodes only (memset / memcpy nodes replayed beside eager work faulted on this stack).  *n_nodes_out (nullable):
 * all nodes.  < 0: the negated error.  Host-only call.                                                             */
int lr_graph_foreign_nodes(void* graph, int* n_nodes_out);

/* ------------------------------------------------------------------------------------
 * (a1) Row gather — replaces tf.nn.embedding_lookup at layers/embedding.py:23,
 * tfops/features.py:40,69,102, algorithms/two_tower.py:307,325,370-374 and the batch-row
 * gathers of training/torch_trainer.py:154-156.
 *   out[i, :] = table[idx[i], :]   for i in [0, n);  idx outside [0, V) yields a zero row
 *   (TF-on-GPU semantics; TF-on-CPU raises).  Any K >= 1; K % 4 == 0 takes the 16-byte path.
 * ---------------------------------------------------------------------------------- */
int lr_embed_gather_f32(const float* table, int64_t V, int K, const int32_t* idx,
                        int64_t n, float* out, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a2) Fixed-length bag pooling with OOV -> 0 — replaces multi_sparse_alone
 * (tfops/features.py:90-118) and seq_embeds_pooling (layers/embedding.py:54-85).
 *   idx is [nbags, bag_len]; entries equal to `oov` (or outside [0,V)) contribute a zero
 *   vector; out[b,:] = sum / d, d = 1 (sum), count (mean) or sqrt(count) (sqrtn) of the
 *   non-OOV entries, with x/0 = 0 (tf.div_no_nan).  The reference zeroes the OOV row *in the
 *   variable* on every forward (quirk 8); here the row is simply never read.
 * ---------------------------------------------------------------------------------- */
#define LR_COMBINER_SUM 0
#define LR_COMBINER_MEAN 1
#define LR_COMBINER_SQRTN 2
int lr_embed_bag_pool_f32(const float* table, int64_t V, int K, const int32_t* idx,
                          int64_t nbags, int bag_len, int combiner, int32_t oov,
                          float* out, lr_stream_t stream);
/* backward of the pooling: expands d(out)[nbags,K] to per-entry gradients
 * gentry[nbags*bag_len, K] (zero for OOV entries), ready for lr_embed_scatter_*.      */
int lr_embed_bag_pool_bwd_f32(const float* gout, int K, const int32_t* idx, int64_t V,
                              int64_t nbags, int bag_len, int combiner, int32_t oov,
                              float* gentry, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Segment construction ("CSR by touched row") — the index half of the gradient path that
 * TF performs inside the IndexedSlices gradient of embedding_lookup + AdamOptimizer
 * (training/tf_trainer.py:120-121: duplicates are summed before the update).
 *   Sorts (idx[i], i) by idx (stable), then emits
 *     seg_pos   [n]      : original positions i, grouped by row, ascending i inside a row
 *     seg_rows  [n]      : the distinct rows, ascending          (first *n_seg valid)
 *     seg_start [n + 1]  : start of each row's run in seg_pos    (first *n_seg + 1 valid)
 *     n_seg     [1]      : number of distinct rows (device int32; never read by the host)
 *     pos_to_seg[n]      : (nullable) run number of every position, -1 for dropped entries —
 *                          the inverse map that turns a de-duplicated row cache back into
 *                          per-position slots (multi-GPU row exchange)
 *   Entries with idx outside [0,V) are dropped (their run is not emitted).
 *   Bit-exact integer work: the oracle is np.unique/argsort(kind="stable").
 * ---------------------------------------------------------------------------------- */
size_t lr_segments_ws_bytes(int64_t n, int64_t V);
int lr_segments_build(const int32_t* idx, int64_t n, int64_t V, int32_t* seg_pos,
                      int32_t* seg_rows, int32_t* seg_start, int32_t* n_seg,
                      int32_t* pos_to_seg, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a1 bwd / a11) Gradient scatter — replaces the IndexedSlices gradient of
 * tf.nn.embedding_lookup and nn.Embedding's dense gradient
 * (training/torch_trainer.py:116-121).
 *   lr_embed_segment_sum_f32 : grows[s,:] = sum_{p in run s} grad[seg_pos[p], :]
 *                              (deterministic: ascending position order per row)
 *   lr_embed_scatter_add_f32 : table[seg_rows[s],:] += alpha * (that sum)   (SGD-style / dense-grad build)
 * ---------------------------------------------------------------------------------- */
/* Long runs (a Zipf head row collecting thousands of positions) are cut into 512-position chunks summed by whole
 * workgroups when a workspace of lr_embed_scatter_ws_bytes(n_max, K) bytes is passed (`ws`; NULL: every run is walked by
 * one row group).  Chunk partials are added in chunk order: results stay run-to-run identical.  Vector path only
 * (K in {16, 32, 64, 128}, 16-byte aligned operands). */
size_t lr_embed_scatter_ws_bytes(int64_t n_max, int K);
int lr_embed_segment_sum_f32(const float* grad, int K, const int32_t* seg_pos,
                             const int32_t* seg_start, const int32_t* n_seg,
                             int64_t n_max, float* grows, void* ws, size_t ws_bytes,
                             lr_stream_t stream);
int lr_embed_scatter_add_f32(float* table, int64_t V, int K, const float* grad,
                             const int32_t* seg_pos, const int32_t* seg_rows,
                             const int32_t* seg_start, const int32_t* n_seg,
                             int64_t n_max, float alpha, void* ws, size_t ws_bytes,
                             lr_stream_t stream);

/* Adam hyper-parameters.  TF1 form (tf.train.AdamOptimizer, training/tf_trainer.py:120):
 *   lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t);  w -= lr_t * m / (sqrt(v) + eps)
 * torch form (torch.optim.Adam, training/torch_trainer.py:63-69; `tf_style` = 0):
 *   w -= lr / (1 - beta1^t) * m / (sqrt(v / (1 - beta2^t)) + eps), g += weight_decay * w */
typedef struct lr_adam_hp {
  double lr;           /* doubles: the reference passes Python floats; (1 - beta) is formed  */
  double beta1;        /* in fp32 by TF (1.f - 0.999f) but in double by torch (1 - 0.999),   */
  double beta2;        /* a 1.3e-5 relative difference that both styles reproduce exactly    */
  double eps;
  double weight_decay; /* torch-style L2 added to the gradient of touched rows (0 = off)     */
  int32_t step;        /* t >= 1, the step being applied                                     */
  int32_t tf_style;    /* 1 = TF1 (sparse-apply form), 0 = torch.optim.Adam                  */
} lr_adam_hp;

/* Fused segment-sum + row-wise Adam on touched rows only ("lazy" Adam): one pass that
 * reads each gradient row once and read-modify-writes w, m, v of each distinct row once. */
int lr_embed_scatter_adam_f32(float* table, float* m, float* v, int64_t V, int K,
                              const float* grad, const int32_t* seg_pos,
                              const int32_t* seg_rows, const int32_t* seg_start,
                              const int32_t* n_seg, int64_t n_max, lr_adam_hp hp,
                              void* ws, size_t ws_bytes, lr_stream_t stream);
/* The same update on a table AND its per-row linear weight ([V,1] arrays, scalar gradients glin [n_max])
 * from one pass over the segments — the owner-side update of the row-sharded tables. */
int lr_embed_scatter_adam_lin_f32(float* table, float* m, float* v, int64_t V, int K, const float* grad,
                                  float* lin, float* lin_m, float* lin_v, const float* glin,
                                  const int32_t* seg_pos, const int32_t* seg_rows,
                                  const int32_t* seg_start, const int32_t* n_seg, int64_t n_max,
                                  lr_adam_hp hp, lr_stream_t stream);
/* (e) The owner-side update of the row-sharded tables straight from the peers' lists: after the gradient all-to-all
 * the owner holds W lists back to back (peer_counts[p] entries each, a HOST array), ids[i] = local row, grad [n, K] /
 * glin [n] its gradients; a row appears at most once per list.  Rows are grouped through peer_tab (int32 [V * W], all
 * zero on entry and on return; unused and may be NULL for W == 1) instead of a sort; gradients of a row are added in
 * ascending peer order — the order (and the bits) of lr_segments_build + lr_embed_scatter_adam_lin_f32 on the same
 * lists.  lin / lin_m / lin_v / glin may all be NULL (no per-row linear weight).  K in {16, 32, 64, 128}, W <= 64,
 * 16-byte aligned arrays; otherwise LR_ESHAPE (use the segment path).                                              */
int lr_embed_peer_adam_f32(float* table, float* m, float* v, int64_t V, int K, const float* grad, float* lin,
                           float* lin_m, float* lin_v, const float* glin, const int32_t* ids,
                           const int64_t* peer_counts, int W, int32_t* peer_tab, lr_adam_hp hp, lr_stream_t stream);
/* Dense Adam over the whole table with TF1 semantics (every row decays m, v and moves every
 * step, training/tf_trainer.py:120; SURVEY §7 "TF1 Adam is dense").  `grows`/`seg_rows`
 * are the segment sums of the touched rows (may be empty); `l2` adds 2*l2*w to every row's
 * gradient (tf.keras.regularizers.l2, tfops/configs.py:20-26).  `row_slot` is an int32[V]
 * scratch array owned by the caller; it must be all -1 on entry and is all -1 on return.
 * With `seg_rows == NULL` and `grows != NULL`, `grows` is a full dense gradient [V,K] (the
 * dense-layer parameters: MLP kernels/biases, BatchNorm gamma/beta) and no scratch is used.
 * `vmax` (nullable, [V,K]) switches on AMSGrad (torch.optim.Adam(amsgrad=True),
 * training/torch_trainer.py:63-69): running element-wise maximum of v used in the denominator. */
int lr_adam_dense_f32(float* table, float* m, float* v, float* vmax, int64_t V, int K,
                      const float* grows, const int32_t* seg_rows, const int32_t* n_seg,
                      int64_t n_max, int32_t* row_slot, float l2, lr_adam_hp hp,
                      lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a4) FM pairwise interaction — replaces algorithms/fm.py:158-161, deepfm.py:160-163:
 *   pair[b,k] = 0.5 * ((sum_f e[b,f,k])^2 - sum_f e[b,f,k]^2)
 * Stand-alone forward/backward on a materialised e[B,F,K] ...
 * ---------------------------------------------------------------------------------- */
int lr_fm_pairwise_fwd_f32(const float* e, int64_t B, int F, int K, float* pair,
                           float* fsum /* [B,K] or NULL */, lr_stream_t stream);
/* ge[b,f,k] (+)= gpair[b,k] * (fsum[b,k] - e[b,f,k]);  accumulate != 0 adds to ge. */
int lr_fm_pairwise_bwd_f32(const float* e, const float* fsum, const float* gpair,
                           int64_t B, int F, int K, float* ge, int accumulate,
                           lr_stream_t stream);
/* ... and the fused form the models use: gather F rows per sample from one table addressed
 * by global row ids (user / item / sparse fields concatenated with offsets, the layout of
 * tfops/features.py:6-44), write them once as the MLP input e[B,F,K] and reduce the
 * pairwise term in the same pass (one wavefront per sample, no second read of e).
 * `e` may be NULL (plain FM has no deep part).  `lin` / `lin_out[B,F]` (both or neither)
 * additionally gather the linear weights (the `*_linear_var` tables, deepfm.py:181-192) in
 * the same pass.                                                                        */
int lr_fm_embed_fwd_f32(const float* table, const float* lin, int64_t V, int K,
                        const int32_t* idx, int64_t B, int F, float* e, float* pair,
                        float* fsum, float* lin_out, lr_stream_t stream);
/* Fused backward + optimiser for the same layout: for every distinct row r touched by the
 * batch, with P(r) its (b,f) positions (segments built over idx[B*F]),
 *   g_r = sum_{(b,f) in P(r)} ( gdeep[b,f,:] - bn_a[f,:]
 *                               + gpair[b,:] * (fsum[b,:] - table[r,:]) - bn_c[f,:] * table[r,:] )
 * then one row-wise Adam update of (table, m, v)[r]; with `lin` != NULL also
 *   glin_r = sum glin[f,b] and one Adam update of (lin, lin_m, lin_v)[r].  `glin` is
 *   FIELD-MAJOR [F,B] (a row's positions share f: its reads stay in one L2-resident strip).
 * `gdeep` may be NULL (plain FM).  bn_a / bn_c [F,K] (both or neither) carry the per-feature
 * affine terms of a batch-statistics BatchNorm folded into the first dense layer
 * (layers/dense.py:30-31: d x = G - a - c*x), so the normalised copy of e is never formed.
 * Valid because every position of row r holds the same value table[r] (no bag pooling).
 * Runs longer than 32 positions (Zipf head) are summed by a whole workgroup; `ws` holds that
 * work list.  Deterministic: no floating-point atomics.                                  */
size_t lr_fm_embed_bwd_ws_bytes(int64_t B, int F);
int lr_fm_embed_bwd_adam_f32(float* table, float* m, float* v, float* lin, float* lin_m,
                             float* lin_v, int64_t V, int K, const float* gdeep,
                             const float* gpair, const float* fsum, const float* glin,
                             const float* bn_a, const float* bn_c, int64_t B, int F,
                             const int32_t* seg_pos, const int32_t* seg_rows,
                             const int32_t* seg_start, const int32_t* n_seg, lr_adam_hp hp,
                             void* ws, size_t ws_bytes, lr_stream_t stream);

/* "Rows" form for row-sharded tables: `row_cache[U,K]` holds the batch's distinct
 * rows in run order (fetched from their owners); the summed per-row gradients are written to
 * grows_out[U,K] / glin_out[U] instead of being applied, to be sent back to the owning ranks. */
int lr_fm_embed_bwd_rows_f32(const float* row_cache, int K, const float* gdeep,
                             const float* gpair, const float* fsum, const float* glin,
                             const float* bn_a, const float* bn_c, int64_t B, int F,
                             const int32_t* seg_pos, const int32_t* seg_start,
                             const int32_t* n_seg, float* grows_out, float* glin_out, void* ws,
                             size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a1 + a4 + a5, fused) DeepFM: embedding lookup fused with the FIRST Dense layer of dense_nn on
 * the f32 MFMA pipe — replaces the concatenation deep_embed [B, F*K] (algorithms/deepfm.py:236-247),
 * its batch_normalization + first tf_dense (layers/dense.py:30-41 via deepfm.py:163-169), the FM
 * terms (deepfm.py:158-162) and, in the backward, the IndexedSlices gradient + AdamOptimizer
 * (training/tf_trainer.py:120-121).  deep_embed and its gradient never exist in memory.
 *
 * Wp [F*K, H1] is the BatchNorm-FOLDED first kernel, Wp = diag(gamma * rsqrt(var + eps)) @ W1, and
 * `bias` = b1 + (beta - mean * gamma * rsqrt(var + eps)) @ W1, both formed by the caller from the
 * batch statistics (lr_fm_field_stats_f32 reads them off the batch's runs); the remaining BatchNorm
 * backward terms enter lr_fm_rows_adam_f32 as bn_a / bn_c (dx = G - a - c * x).
 * Shapes compiled: (K, H1) with lr_deepfm_l1_supported(K, H1) != 0; others return LR_ESHAPE.
 *
 *   lr_deepfm_l1_pack_f32   Wp -> WpA / WpB (F*K*H1 floats each): MFMA fragment order for the
 *                           forward / the row-gradient kernel (one coalesced 16-byte load per lane
 *                           and four MFMAs).
 *   lr_deepfm_l1_fwd_f32    z1[b,:]   = sum_f table[idx[b,f],:] @ Wp[f*K:(f+1)*K,:] + bias
 *                           fsum[b,:] = sum_f table[idx[b,f],:];  pair = 0.5*(fsum^2 - sum_f row^2)
 *                           lin_out[b,f] = lin[idx[b,f]]          (lin / lin_out both NULL or both set)
 *                           ids outside [0,V) contribute a zero row.
 *   lr_deepfm_l1_wgrad_f32  partial[c, f*K+i, n] = sum over the samples of batch chunk c of
 *                           table[idxT[f,b], i] * gz[b, n];  dWp = sum_c partial[c] (caller, fixed
 *                           order).  idxT is idx transposed to [F, B] (lr_idx_transpose_i32);
 *                           n_chunks from lr_deepfm_l1_wgrad_chunks (any value >= 1 is valid).
 *   lr_deepfm_l1_dgrad_f32  ge[slotT[f,b], :] = gz[b,:] @ Wp[f*K:(f+1)*K,:]^T + gl[b]*wp[:]*fsum[b,:]
 *                           i.e. the per-position row gradient WITHOUT the terms that only depend on
 *                           the row itself, written in RUN ORDER (slotT from lr_segments_build_fields;
 *                           positions with slot -1 are written to the spare row B*F: ge holds B*F + 1 rows).  gl = d loss / d logit, wp = the
 *                           output layer's weights of the pairwise term (deepfm.py:171-172: the FM
 *                           term feeds one Dense(1), so d loss / d pair[b,:] = gl[b] * wp[:]).
 *   lr_fm_rows_adam_f32     per distinct row r (run s of n positions, field f):
 *                             g = sum_p ge[p] - n*bn_a[f] - w_r * (n*bn_c[f] + wp * sum_p gl[b(p)])
 *                             Adam(w_r, m_r, v_r, g);  lin rows: g_lin = lin_scale[f] * sum_p gl[b(p)]
 *                           (lin_scale[f] = d logit / d lin_out[b,f] = out_kernel[0] * linear_kernel[f]).
 *                           Same bucketing / determinism as lr_fm_embed_bwd_adam_f32; `ws` sized by
 *                           lr_fm_embed_bwd_ws_bytes.
 * ---------------------------------------------------------------------------------- */
int lr_deepfm_l1_supported(int K, int H1);
/* Round 4: the forward and the row-gradient kernel exist in two tilings — 32 samples per workgroup (two workgroups per CU)
 * and 64 samples per workgroup with one wave per SIMD and two accumulators per wave (half the L2 -> CU weight traffic;
 * chosen when the batch fills the chip with one workgroup per CU: B >= 12,288).  Both run the same k-ordered f32 fma
 * chain per output element: bit-identical results.  `tile` = 32 or 64 pins the family (tests, profiling), 0 restores the
 * automatic choice.  (The weight-gradient kernel has the 32-sample form only: its wide form measured slower.) */
void lr_deepfm_l1_tile_override(int tile);
int lr_deepfm_l1_pack_f32(const float* Wp, int F, int K, int H1, float* WpA, float* WpB,
                          lr_stream_t stream);
int lr_idx_transpose_i32(const int32_t* idx, int64_t B, int F, int32_t* idxT, lr_stream_t stream);
int lr_deepfm_l1_fwd_f32(const float* table, const float* lin, int64_t V, int K,
                         const int32_t* idx, int64_t B, int F, const float* WpA, const float* bias,
                         int H1, float* z1, float* pair, float* fsum, float* lin_out,
                         lr_stream_t stream);
/* Round 5: the three contractions of the layer as SPLIT-bf16 MFMA products with f32 accumulation (csrc/deepfm_l1_sb.hip) — every
 * f32 operand split exactly into three bf16 values, a product taken as the six largest cross terms (v_mfma_f32_32x32x16_bf16).
 * As close to f64 as the f32 fma chain above on this layer's reductions (relative rms error 1.88e-6 vs 2.08e-6 at K = 12,928,
 * profiles/r04_bf16_split_probe.txt), NOT bit-identical to it; the host mirror selects it by default where the shape is
 * compiled (K = 64, H1 = 128: lr_deepfm_l1_sb_supported; LR_ESHAPE otherwise) and keeps the f32 chain selectable.
 * Same contracts as lr_deepfm_l1_fwd / wgrad / dgrad_f32 except the packed operands:
 *   lr_deepfm_l1_sb_pack     W [F*K, H1] row-major (optional row scale = the BatchNorm fold) -> WsbA (forward) and / or WsbB
 *                            (row gradient): three bf16 planes in fragment order, lr_deepfm_l1_sb_pack_bytes bytes each
 *   lr_deepfm_l1_sb_gz_pack  gz [B, H1] -> planes for the weight gradient (lr_deepfm_l1_sb_gz_pack_bytes bytes; samples
 *                            padded with zeros to a multiple of 16)
 *   lr_deepfm_l1_fwd_sb_f32  `ws` (lr_deepfm_l1_fwd_sb_ws_bytes): partial sums when the fields are split across workgroups
 *                            (batches that do not fill the chip with 128-sample tiles); z1 / pair / fsum are then summed in
 *                            field-group order by a second launch
 *   lr_deepfm_l1_wgrad_sb_f32  n_chunks: any value >= 1 (lr_deepfm_l1_wgrad_sb_chunks: the grid that fills the chip)
 * All pointers 16-byte aligned.                                                                                              */
int lr_deepfm_l1_sb_supported(int K, int H1);
int lr_deepfm_l1_fwd_sb_supported(int K, int H1);   /* = lr_deepfm_l1_sb_supported (round-4 name) */
size_t lr_deepfm_l1_sb_pack_bytes(int F, int K, int H1);
/* `red_partial` / `red_nblk` / `red_out` (NULL / 0 / NULL: none): the launch also sums the `red_nblk` slab partials [red_nblk][H1]
 * of the folded bias into red_out [H1] (the arithmetic of lr_reduce_partials_f32, ceil(H1 / 16) extra workgroups). */
int lr_deepfm_l1_sb_pack(const float* W, const float* scale, int F, int K, int H1, void* WsbA, void* WsbB,
                         const float* red_partial, int red_nblk, float* red_out, lr_stream_t stream);
size_t lr_deepfm_l1_sb_gz_pack_bytes(int64_t B, int H1);
int lr_deepfm_l1_sb_gz_pack(const float* gz, int64_t B, int H1, void* gzp, lr_stream_t stream);
/* profiling / tests (same results in every mode up to the order of the field-group sums): samples per workgroup of the forward
 * (64 / 128; 0 = automatic), field groups of the forward / row-gradient grids (0 = automatic), multiplying waves (4 / 8) and
 * fields (2 / 4) per workgroup of the weight gradient (0 = automatic) */
void lr_deepfm_l1_sb_override(int fwd_tile, int ksplit, int wgrad_cw, int wgrad_fg);
size_t lr_deepfm_l1_fwd_sb_ws_bytes(int64_t B, int F);
int lr_deepfm_l1_fwd_sb_f32(const float* table, const float* lin, int64_t V, int K, const int32_t* idx, int64_t B,
                            int F, const void* WsbA, const float* bias, int H1, float* z1, float* pair, float* fsum,
                            float* lin_out, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_deepfm_l1_wgrad_sb_chunks(int64_t B, int F);
int lr_deepfm_l1_wgrad_sb_f32(const float* table, int64_t V, int K, const int32_t* idxT, int64_t B, int F,
                              const void* gzp, int H1, int n_chunks, float* partial, lr_stream_t stream);
int lr_deepfm_l1_dgrad_sb_f32(const float* gz, int H1, const void* WsbB, int K, int F, int64_t B, const float* gl,
                              const float* wp, const float* fsum, const int32_t* slotT, float* ge, lr_stream_t stream);
int lr_deepfm_l1_wgrad_chunks(int64_t B, int F);
int lr_deepfm_l1_wgrad_f32(const float* table, int64_t V, int K, const int32_t* idxT, int64_t B,
                           int F, const float* gz, int H1, int n_chunks, float* partial,
                           lr_stream_t stream);
int lr_deepfm_l1_dgrad_f32(const float* gz, int H1, const float* WpB, int K, int F, int64_t B,
                           const float* gl, const float* wp, const float* fsum,
                           const int32_t* slotT, float* ge, lr_stream_t stream);
/* Row-sharded tables: the batch's rows live in a per-step row cache [n_cache, K] addressed through the
 * position -> cache-slot map `slots` [B*F]; the segments are the per-field runs of the GLOBAL row ids.
 *   lr_fm_field_stats_slots_f32  lr_fm_field_stats_f32 with the run's row read from cache[slots[first position]]
 *   lr_fm_rows_grad_f32          lr_fm_rows_adam_f32's per-row gradient WITHOUT the update: grows[slot] = g,
 *                                glin_rows[slot] = g_lin (handed to the owners by the gradient all-to-all) */
int lr_fm_field_stats_slots_f32(const float* cache, int K, const int32_t* seg_rows, const int32_t* seg_start,
                                const int32_t* n_seg, const int32_t* field_row_start, int F, int C,
                                float* partial, const int32_t* seg_pos, const int32_t* slots,
                                lr_stream_t stream);
int lr_fm_rows_grad_f32(const float* cache, const float* lin_cache, int64_t n_cache, int K, const float* ge,
                        const float* gl, const float* wp, const float* bn_a, const float* bn_c,
                        const float* lin_scale, int64_t B, int F, const int32_t* seg_pos,
                        const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg,
                        const int32_t* slots, float* grows, float* glin_rows, void* ws, size_t ws_bytes,
                        lr_stream_t stream);
/* The reference's own optimiser semantics on the fused step (training/tf_trainer.py:120 — tf.train.AdamOptimizer moves EVERY row
 * of a table every step, touched or not):
 *   lr_fm_rows_grad_compact_f32  lr_fm_rows_adam_f32's per-row gradient WITHOUT the update, rows read from the tables
 *                                themselves, run s writing grows[s] / glin_rows[s] (compact: n_seg rows)
 *   lr_adam_dense_rows_f32       ONE streaming pass over (table, m, v) [V,K] and (lin, lin_m, lin_v) [V] (nullable, all or
 *                                none): every row decays its moments and moves; the rows listed in seg_rows[0 .. *n_seg) take
 *                                grows[s] / glin_rows[s].  `row_slot`: int32[V] scratch, all -1 on entry and on return.
 *                                K in {16, 32, 64, 128}.  `_dc_`: coefficients from device memory (hipGraph-captured steps). */
int lr_fm_rows_grad_compact_f32(const float* table, const float* lin, int64_t V, int K, const float* ge,
                                const float* gl, const float* wp, const float* bn_a, const float* bn_c,
                                const float* lin_scale, int64_t B, int F, const int32_t* seg_pos,
                                const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg,
                                float* grows, float* glin_rows, void* ws, size_t ws_bytes, lr_stream_t stream);
/* row_slot[seg_rows[s]] = s for s < *n_seg (set != 0), or = -1 (set == 0): the row -> segment map the dense passes read */
int lr_row_slots_i32(const int32_t* seg_rows, const int32_t* n_seg, int64_t n_max, int32_t* row_slot, int set,
                     lr_stream_t stream);
int lr_adam_dense_rows_f32(float* table, float* m, float* v, float* lin, float* lin_m, float* lin_v, int64_t V, int K,
                           const float* grows, const float* glin_rows, const int32_t* seg_rows, const int32_t* n_seg,
                           int64_t n_max, int32_t* row_slot, lr_adam_hp hp, lr_stream_t stream);
int lr_adam_dense_rows_dc_f32(float* table, float* m, float* v, float* lin, float* lin_m, float* lin_v, int64_t V, int K,
                              const float* grows, const float* glin_rows, const int32_t* seg_rows, const int32_t* n_seg,
                              int64_t n_max, int32_t* row_slot, const void* coef_dev, lr_stream_t stream);
int lr_fm_rows_adam_f32(float* table, float* m, float* v, float* lin, float* lin_m, float* lin_v,
                        int64_t V, int K, const float* ge, const float* gl, const float* wp,
                        const float* bn_a, const float* bn_c, const float* lin_scale, int64_t B,
                        int F, const int32_t* seg_pos, const int32_t* seg_rows,
                        const int32_t* seg_start, const int32_t* n_seg, lr_adam_hp hp, void* ws,
                        size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a5 + a10) DeepFM "tail": the layers of dense_nn after the first Dense (layers/dense.py:33-49:
 * relu -> batch-statistics BatchNorm -> Dense, last layer linear), the output layer over
 * [linear term | pairwise term | deep term] (algorithms/deepfm.py:158, 171-172), the sigmoid
 * cross-entropy loss (tfops/loss.py:14-16) and their backward — as a few small launches cut only
 * where BatchNorm needs a batch-wide reduction.  Widths: multiples of 16, <= 256
 * (lr_mlp_tail_supported).  Every batch reduction is a per-workgroup partial (64 samples) + a
 * fixed-order second pass: no atomics, run-to-run bit identical.
 *   lr_mlp_colstats_f32     partial[blk][{sum, sumsq}][d] of relu(z)
 *   lr_mlp_bn_finalize_f32  mean, rsqrt(var + eps) (biased var) + moving averages (momentum)
 *   lr_mlp_layer_fwd_f32    z_out = BN(relu(z_in)) @ W + b  (+ colstats of relu(z_out)); BN pointers NULL = none
 *   lr_mlp_head_f32         logits, gl = d loss / d logit, per-workgroup partials
 *                           [d wo (1+K+dn) | d bo | d wl (F) | d bl | loss sum]  (dn+K+F+4 floats each).
 *                           Plain form (the output layer of DIN / YouTubeRanking, algorithms/din.py:190-192):
 *                           F == 0 (lin_out, wl, bl NULL) drops the linear term and wo[0]; K == 0 (pair NULL) the
 *                           pairwise term: logit = zn @ wo + bo, partials [d wo (K+dn) | d bo | loss sum].
 *   lr_mlp_layer_bwd_f32    through z_out = h_in @ W + b: upstream gz_out = gl*wd (mode 0: z_out is the
 *                           last layer) or the activation/BatchNorm backward of gh_out (mode 1);
 *                           gh_in = gz_out @ W^T, partials of dW, db and of the input BatchNorm's
 *                           (sum gh_in, sum gh_in * x_hat_in) = (d beta, d gamma)
 *   lr_mlp_first_bwd_f32    gz_1 from gh_1 (+ partial column sums)
 *   lr_reduce_partials_f32  out[c] = sum_k partial[k*stride + c], fixed order
 * ---------------------------------------------------------------------------------- */
/* Round 5: the whole tail of a THREE-layer dense_nn (128 -> 64 -> 32 after the first Dense: the reference's default
 * hidden_units) as ONE persistent launch — the same per-tile arithmetic as the chain of lr_mlp_* launches below (bit-identical
 * results), min(tiles, CUs) resident workgroups meeting at four grid barriers where a batch-statistics BatchNorm needs the whole
 * batch.  Inputs z0 = first Dense output [B, 128], pair [B, K] / lin_out [B, F] / labels as lr_mlp_head_f32; buffers as the
 * chain's (tiles = ceil(B / 64)): z1 [B, 64], z2 [B, 32], gh0 [B, 128], gh1 [B, 64], stat* / bnp* [tiles, 2, d], dW*p
 * [tiles, d_in * d_out], db*p [tiles, d_out], headp [tiles, G + 1], gl [B], gz0 [B, 128], sgzp [tiles, 128]; mean* / inv* [d]:
 * the batch statistics; d gamma / d beta of both BatchNorms are written in full, the weight / bias / head partials are left
 * for lr_reduce_partials_multi_f32.  A BatchNorm's pointers (gamma, beta, dgamma, dbeta, stat, bnp, mean, inv; mm / mv
 * optional) are NULL together.
 * `sync`: 24 device words the caller allocates ZEROED once and then only reads: [0] arrival counter (left at 0 by every launch
 * that completes: the last workgroup to finish clears it, so no zeroing launch precedes the kernel), [1] "a launch gave up",
 * [2..17] phase time stamps of workgroup 0 (a profiling aid), [18] the STICKY error word, never cleared by the library,
 * [19] the poll bound in polls (0: the default, ~2 s), [20] finished-workgroup counter, [21..23] reserved.  The launch is a plain
 * one whose grid barrier needs every workgroup resident at once, so the grid is min(tiles, CUs of the current device x the
 * kernel's own occupancy) — lr_mlp_tail3_resident_blocks() — and the poll is bounded: when a barrier does not complete (other
 * work holds the CUs), the workgroups stop BEFORE the next phase, write NaN into their loss partials (headp) and set sync[1] and
 * sync[18]; every later launch on the same `sync` returns at once with a NaN loss.  The caller reads sync[18] where it reads
 * the loss back and raises (librecommender_amd/layers/tail.py:DeepFMTail.check). */
typedef struct lr_mlp_tail3_args {
  int64_t B;
  int K, F;
  const float* z0; const float* pair; const float* lin_out; const float* labels;
  float eps0, mom0; float* mm0; float* mv0; const float* gamma0; const float* beta0; float* dgamma0; float* dbeta0;
  float eps1, mom1; float* mm1; float* mv1; const float* gamma1; const float* beta1; float* dgamma1; float* dbeta1;
  const float* W1; const float* b1; const float* W2; const float* b2;
  const float* wl; const float* bl; const float* wo; const float* bo;
  float* z1; float* z2; float* gh0; float* gh1;
  float* stat0; float* stat1; float* bnp0; float* bnp1;
  float* mean0; float* inv0; float* mean1; float* inv1;
  float* dW1p; float* db1p; float* dW2p; float* db2p; float* headp;
  float* gl; float* gz0; float* sgzp;
  uint32_t drop_seed; float keep;
  unsigned* sync;
} lr_mlp_tail3_args;
int lr_mlp_tail3_supported(int d0, int d1, int d2, int K, int F);
int lr_mlp_tail3_f32(const lr_mlp_tail3_args* args, lr_stream_t stream);
int lr_mlp_tail3_resident_blocks(void);
int lr_mlp_tail_supported(int d_in, int d_out);
int lr_mlp_colstats_f32(const float* z, int64_t B, int d, float* partial, lr_stream_t stream);
int lr_mlp_bn_finalize_f32(const float* partial, int nblk, int d, int64_t B, float eps, float momentum,
                           float* moving_mean, float* moving_var, float* mean_out, float* inv_out,
                           lr_stream_t stream);
int lr_mlp_layer_fwd_f32(const float* z_in, int64_t B, int d_in, const float* mean, const float* inv,
                         const float* gamma, const float* beta, const float* W, const float* bias,
                         int d_out, float* z_out, float* partial_out, uint32_t drop_seed, float drop_keep,
                         int drop_layer, lr_stream_t stream);
int lr_mlp_head_f32(const float* zn, int dn, const float* pair, int K, const float* lin_out, int F,
                    const float* labels, const float* wl, const float* bl, const float* wo,
                    const float* bo, int64_t B, float* logits, float* gl, float* partial,
                    lr_stream_t stream);
int lr_mlp_layer_bwd_f32(int mode, const float* gl, const float* wd, const float* gh_out,
                         const float* z_out, const float* up_mean, const float* up_inv,
                         const float* up_gamma, const float* up_dgamma, const float* up_dbeta,
                         const float* z_in, const float* in_mean, const float* in_inv,
                         const float* in_gamma, const float* in_beta, const float* W, int d_in,
                         int d_out, int64_t B, float* gh_in, float* dW_partial, float* db_partial,
                         float* bn_partial, uint32_t drop_seed, float drop_keep, int drop_layer, lr_stream_t stream);
/* Dropout (layers/dense.py:44-47: after a hidden layer's BatchNorm; kept entries scaled by 1 / keep): `drop_keep` < 1 applies
 * the mask keep(seed, layer, sample, column) = [u < drop_keep], u = the low 24 bits of splitmix64's finaliser over
 * (sample * 4096 + column) ^ (seed * 0x9E3779B97F4A7C15 + layer * 0xD1B54A32D192ED03), to h_in = BN(relu(z_in)) in the
 * forward kernel and regenerates it in the backward kernel (the Dense's input for dW, the gradient through the dropout);
 * `drop_keep` >= 1: no dropout.  The caller passes the same (seed, layer) to both kernels of a layer and a new seed per step. */
int lr_mlp_first_bwd_f32(const float* gh, const float* z, const float* mean, const float* inv,
                         const float* gamma, const float* dgamma, const float* dbeta, int64_t B, int d,
                         float* gz, float* partial, lr_stream_t stream);
int lr_reduce_partials_f32(const float* partial, int nblk, int64_t n, int64_t stride, float* out,
                           lr_stream_t stream);
/* n_jobs independent lr_reduce_partials_f32 in one launch; `jobs_dev`: DEVICE array of
 * { const float* partial; float* out; int64_t n; int64_t stride; int32_t nblk; float div; }
 * (lr_reduce_job_bytes() = 40), max_n = the largest n among them.  div != 0: out = (float)sum / div (the loss's 1 / B). */
size_t lr_reduce_job_bytes(void);
int lr_reduce_partials_multi_f32(const void* jobs_dev, int n_jobs, int64_t max_n, lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * Streaming in-batch softmax cross-entropy (csrc/softmax_ce.hip) — replaces, for the two-tower
 * retrieval loss, `softmax_cross_entropy` (libreco/tfops/loss.py:71-75) over `adjust_logits`
 * (libreco/algorithms/two_tower.py:458-479): logits = X Y^T (+ col_bias[j] = -log Q(j)), entries
 * with row_ids[i] == col_ids[j] and j != pos0 + i masked to float32.min (accidental hits), labels
 * = the diagonal (column pos0 + i for row i; pos0 > 0 when the columns are the all-gathered
 * item-tower outputs of every rank).  The B x N logits are never written.
 *   lr_softmax_ce_fwd_f32       lse[i] = logsumexp_j logits[i][:], pos_logit[i] = logits[i][pos0+i]
 *                               (loss_i = lse - pos_logit) and, if W != NULL,
 *                               W[i] = sum_j softmax(logits[i])[j] Y[j]   so that
 *                               d loss_i / d X[i] = W[i] - Y[pos0+i]
 *   lr_softmax_ce_bwd_cols_f32  V[j] = sum_i g[i] softmax(logits[i])[j] X[i]   so that
 *                               d (sum_i g_i loss_i) / d Y[j] = V[j] - [j = pos0+i] g[i] X[i]
 * When the rows are a small share of the columns (a rank's users against the all-gathered items) the forward
 * sweep is cut into column ranges and merged (workspace from lr_softmax_ce_fwd_ws_bytes).
 * Fixed summation order (run-to-run identical).  D <= 128, D % 4 == 0
 * (lr_softmax_ce_supported); col_bias and the id pair are nullable; pointers 16-byte aligned.
 * `arith`: the arithmetic of the two contractions — an explicit argument of the workspace query and of both launches (it
 * decides the launch shape and the workspace size; the library keeps no setting of its own):
 *   1  every f32 product as six bf16 MFMA products (each operand split exactly into three bf16
 *      values), f32 accumulation — error against f64 = that of the f32 fma chain;
 *   0  the f32 MFMA fma chain.
 * ---------------------------------------------------------------------------------- */
int lr_softmax_ce_supported(int64_t B, int64_t N, int D);
size_t lr_softmax_ce_fwd_ws_bytes(int64_t B, int64_t N, int D, int arith);   /* 0 unless B is a small share of N */
int lr_softmax_ce_fwd_f32(const float* X, int64_t B, const float* Y, int64_t N, int D,
                          const float* col_bias, const int32_t* row_ids, const int32_t* col_ids,
                          int64_t pos0, float* lse, float* pos_logit, float* W, void* ws, size_t ws_bytes,
                          int arith, lr_stream_t stream);
int lr_softmax_ce_bwd_cols_f32(const float* X, int64_t B, const float* Y, int64_t N, int D,
                               const float* col_bias, const int32_t* row_ids, const int32_t* col_ids,
                               int64_t pos0, const float* lse, const float* g, float* V,
                               int arith, lr_stream_t stream);

/* BatchNorm-fold algebra of the fused first layer (csrc/deepfm_fold.hip) — `tf.layers.batch_normalization`
 * on the concatenated embeddings (libreco/layers/dense.py:30-31) folded into the first Dense of `dense_nn`:
 *   lr_deepfm_l1_fold_stats_f32  per-field partial sums (lr_fm_field_stats_f32, [F][C][2][K]) -> mean,
 *                                inv = rsqrt(var + eps), s = gamma * inv, t = beta - mean * s; moving
 *                                averages updated in place (momentum)
 *   lr_deepfm_l1_pack_scaled_f32 lr_deepfm_l1_pack_f32 of diag(scale) W without materialising it
 *   lr_deepfm_l1_fold_bias_f32   partial[slab][h] = sum_{r in slab} t[r] W[r][h], last slab = b:
 *                                lr_reduce_partials_f32 over lr_deepfm_l1_fold_bias_slabs(n_rows) slabs
 *                                gives the folded bias b + t^T W
 *   lr_deepfm_l1_fold_bwd_f32    weight-gradient slabs of lr_deepfm_l1_wgrad_f32 (summed in slab order)
 *                                + sgz -> dW, dgamma, dbeta, db, bn_a, bn_c (gamma == NULL: dW, db only)
 * Round 6 — the same algebra in two launches instead of four (bit-identical results):
 *   lr_deepfm_l1_fold_stats_bias_f32  = fold_stats + fold_bias: the workgroup of a 64-row slab finalises the statistics of
 *                                its own rows, then forms the slab's bias partial
 *   the pack launches' `red_*` arguments = the reduction of those partials as extra workgroups of the weight pack
 * ---------------------------------------------------------------------------------- */
int lr_deepfm_l1_fold_stats_f32(const float* partial, int F, int C, int K, int64_t B, float eps,
                                float momentum, const float* gamma, const float* beta,
                                float* moving_mean, float* moving_var, float* mean, float* inv, float* s,
                                float* t, lr_stream_t stream);
int lr_deepfm_l1_fold_stats_bias_f32(const float* partial, int F, int C, int K, int64_t B, float eps,
                                     float momentum, const float* gamma, const float* beta,
                                     float* moving_mean, float* moving_var, float* mean, float* inv, float* s,
                                     float* t, const float* W, const float* b, int H1, float* bias_partial,
                                     lr_stream_t stream);
int lr_deepfm_l1_pack_scaled_f32(const float* W, const float* scale, int F, int K, int H1, float* WpA,
                                 float* WpB, const float* red_partial, int red_nblk, float* red_out,
                                 lr_stream_t stream);
int lr_deepfm_l1_fold_bias_slabs(int n_rows);
int lr_deepfm_l1_fold_bias_f32(const float* t, const float* W, const float* b, int n_rows, int H1,
                               float* partial, lr_stream_t stream);
int lr_deepfm_l1_fold_bwd_f32(const float* part, int n_slabs, int n_rows, int H1, int64_t B,
                              const float* sgz, const float* W, const float* gamma, const float* beta,
                              const float* mean, const float* inv, float* dW, float* dgamma,
                              float* dbeta, float* db, float* bn_a, float* bn_c, lr_stream_t stream);

/* Step-dependent Adam coefficients in DEVICE memory — for training steps captured in a hipGraph
 * (one `sess.run` per step in the reference, training/tf_trainer.py:76-101): kernel arguments are
 * frozen at capture, so the bias corrections / decayed learning rate of step t are written into a
 * small device buffer (lr_adam_coef_store: a one-thread kernel enqueued ahead of the replay, stream
 * ordered) that the `_dc` forms read.  Same arithmetic as the by-value forms.                     */
size_t lr_adam_coef_bytes(void);
int lr_adam_coef_store(lr_adam_hp hp, void* coef_dev, lr_stream_t stream);
int lr_adam_dense_dc_f32(float* table, float* m, float* v, int64_t n, const float* grad,
                         const void* coef_dev, lr_stream_t stream);
int lr_fm_rows_adam_dc_f32(float* table, float* m, float* v, float* lin, float* lin_m, float* lin_v,
                           int64_t V, int K, const float* ge, const float* gl, const float* wp,
                           const float* bn_a, const float* bn_c, const float* lin_scale, int64_t B,
                           int F, const int32_t* seg_pos, const int32_t* seg_rows,
                           const int32_t* seg_start, const int32_t* n_seg, const void* coef_dev,
                           void* ws, size_t ws_bytes, lr_stream_t stream);
/* lr_embed_scatter_adam_f32 / lr_embed_scatter_adam_lin_f32 with device-resident coefficients: the table update of
 * the general feature nets' captured step (DIN / YouTube* / Transformer / SIM: algorithms/din.py:241-250 runs as one
 * sess.run, training/tf_trainer.py:76-101). */
int lr_embed_scatter_adam_dc_f32(float* table, float* m, float* v, int64_t V, int K, const float* grad,
                                 const int32_t* seg_pos, const int32_t* seg_rows, const int32_t* seg_start,
                                 const int32_t* n_seg, int64_t n_max, const void* coef_dev,
                                 void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_embed_scatter_adam_lin_dc_f32(float* table, float* m, float* v, int64_t V, int K, const float* grad,
                                     float* lin, float* lin_m, float* lin_v, const float* glin,
                                     const int32_t* seg_pos, const int32_t* seg_rows,
                                     const int32_t* seg_start, const int32_t* n_seg, int64_t n_max,
                                     const void* coef_dev, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a5) First Dense layer of dense_nn over a MATERIALISED block of rows (the general feature nets, e.g. DIN's
 * concat([user, item, sparse..., attention output]), algorithms/din.py:186-192, layers/dense.py:12-49): the block is
 * a [rows, K] array addressed through an id map idx [B, F], so lr_deepfm_l1_fwd/wgrad/dgrad_f32 and the fold kernels
 * run on it as on an embedding table.  The two HBM-bound pieces that are specific to it:
 *   lr_table_colstats_f32  partial[f][c][{sum, sumsq}][K] over the samples of chunk c (contiguous ranges of
 *                          ceil(B / C) samples) of table[idx[b, f], :]  — input of lr_deepfm_l1_fold_stats_f32
 *                          (batch statistics of tf.layers.batch_normalization(training=True), layers/dense.py:30-31);
 *                          ids outside [0, V) contribute zeros.  K in {16, 32, 64, 128}.
 *   lr_bn_remainder_f32    G[r, :] -= a[p(r), :] + c[p(r), :] * x[r, :]: the part of the BatchNorm backward that does not
 *                          pass through the GEMM (dx = G - a - c * x).  period == 0: block stored plane by plane
 *                          ([P][B][Kp], p(r) = r / rows_per_plane); period == P > 0: row-major [B, P * Kp] block viewed
 *                          as B * P rows (p(r) = r % P — a materialised deep_embed [B, F * K], deepfm.py:236-247).
 *                          a, c are [P * Kp].
 * ---------------------------------------------------------------------------------- */
int lr_table_colstats_f32(const float* table, int64_t V, int K, const int32_t* idx, int64_t B, int F, int C,
                          float* partial, lr_stream_t stream);
int lr_bn_remainder_f32(float* G, const float* x, const float* a, const float* c, int64_t rows,
                        int64_t rows_per_plane, int64_t period, int Kp, lr_stream_t stream);

/* Field-partitioned segment build: same outputs as lr_segments_build for idx [B, F] whose column
 * f only holds rows of [field_row_start[f], field_row_start[f+1]) (the feature models' global row
 * layout, algorithms/deepfm.py:181-234 as one table); entries outside their field's range are
 * dropped.  Takes the TRANSPOSED ids idxT [F, B]; every column is sorted on its own in LDS (stable
 * 8-bit LSD passes over the local id), so no device-wide sort runs.  slotT [F, B] (nullable):
 * index of position (b, f) in seg_pos, -1 if dropped.  B <= 16384, otherwise LR_ESHAPE (use
 * lr_segments_build).  Bit-exact integer work.                                               */
size_t lr_segments_fields_ws_bytes(int64_t B, int F);
int lr_segments_build_fields(const int32_t* idxT, int64_t B, int F, const int32_t* field_row_start,
                             int32_t* seg_pos, int32_t* seg_rows, int32_t* seg_start,
                             int32_t* n_seg, int32_t* slotT, void* ws, size_t ws_bytes,
                             lr_stream_t stream);
/* The same build, also writing runT [F, B]: the RUN NUMBER (index into seg_rows / seg_start) of position (b, f), -1 if
 * dropped — what maps a position to its row in a per-step row cache laid out in run order.                          */
int lr_segments_build_fields_runs(const int32_t* idxT, int64_t B, int F, const int32_t* field_row_start,
                                  int32_t* seg_pos, int32_t* seg_rows, int32_t* seg_start,
                                  int32_t* n_seg, int32_t* slotT, int32_t* runT, void* ws, size_t ws_bytes,
                                  lr_stream_t stream);

/* (e) Owner partition of a batch's distinct rows for the row-sharded tables (round-robin rows: owner = row % W, the
 * owner's local row = row / W) — the device half of the id exchange the reference does not have (it trains on one
 * device).  rows[0 .. *n_seg) are distinct (any order; ascending from the builds above).  Writes the
 * STABLE owner-major order: perm[r] = place of rows[r], send_ids[perm[r]] = its local row at the owner,
 * counts[o] (int64) = rows asked from owner o, counts[W] = their total.  No sort.  W <= 64 (LR_ESHAPE).  n_max =
 * capacity of rows / perm / send_ids.  Bit-exact integer work.                                                       */
size_t lr_owner_partition_ws_bytes(int64_t n_max, int W);
int lr_owner_partition_i32(const int32_t* rows, const int32_t* n_seg, int64_t n_max, int W, int32_t* perm,
                           int32_t* send_ids, int64_t* counts, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a7) DIN attention pooling — replaces DIN._build_seq_attention (algorithms/din.py:241-250)
 * + din_attention (layers/attention.py:28-64) + the [N+1,K'] materialisation of
 * combine_seq_features (tfops/features.py:151-202, quirk: rebuilt every step) by gathering
 * only the rows a batch touches.
 *   q[b,:]   = item_table[item[b], :]
 *   key[b,l] = item_table[seq[b,l], :]           l < L (pad id allowed, masked by len)
 *   h  = sigmoid( [q, key, q-key, q*key] @ W1[4K,H] + b1[H] )          H = 16 in the reference
 *   s  = (h @ W2[H] + b2) * rsqrt(K);  s[l >= len[b]] = -(2^32) + 1
 *   a  = softmax_l(s);   out[b,:] = sum_l a[l] * key[b,l,:]
 * fwd saves a[B,L] for the backward.  bwd returns per-position gradients w.r.t. the gathered
 * rows (gq[B,K], gkey[B,L,K]; masked positions are written as zeros) and the MLP parameter
 * gradients gW1[4K,H], gb1[H], gW2[H], gb2[1] (overwritten; reduced block-wise in a fixed
 * order through `ws`, no atomics).  K in {16,32,64,128}, H == 16 (the reference's value),
 * otherwise LR_ESHAPE.
 * The `_dense_` forms take already materialised q[B,K'] / keys[B,L,K'] (items with side
 * features: K' = K*(1+n_item_feats), tfops/features.py:204-218) instead of table + ids.
 * ---------------------------------------------------------------------------------- */
size_t lr_din_attn_ws_bytes(int64_t B, int L, int K, int H);   /* 0 where the backward has no kernel (lr_din_attn_path) */
/* The supported (K, L) region, the one the dispatchers themselves use: 0 = no kernel (the entry points return LR_ESHAPE),
 * 1 = the shuffle kernels, 2 = the MFMA kernels (the only ones that take `hid` / `order`).  K in {16, 32, 64, 128}; L <= 2048
 * runs on the MFMA kernels; longer sequences run on the shuffle kernels while their LDS fits a workgroup's 160 KB:
 *   forward   (64 K + 4 L) * 4 bytes:        L <= 9,984 / 9,728 / 9,216 / 8,192   at K = 16 / 32 / 64 / 128
 *   backward  (256 K + 144 + 4 L) * 4 bytes: L <= 9,180 / 8,156 / 6,108 / none    at K = 16 / 32 / 64 / 128
 * `backward` != 0 asks for the backward's region, which is the smaller one: a shape may have a forward and no backward. */
int lr_din_attn_path(int K, int L, int backward);
/* The id stream of the fused DIN step (nets/din_fused.py) in one launch: ids[(2 + n_plain + 2 + L) * B], plane-major
 * [users + user_off | items + item_off | sparse[b][cols[p]] + sparse_off (cols NULL: column p) | -1 (the attention-output plane) |
 *  items + item_off (the query rows) | seqs[b][l] + item_off for l < lens[b], else -1] — the global row ids of
 * libreco/tfops/features.py:6-44 and the pad rule of libreco/batch/sequence.py:56-58. */
int lr_din_build_ids_i32(const int32_t* users, const int32_t* items, const int32_t* sparse, int sparse_ld,
                         const int32_t* cols, int n_plain, const int32_t* seqs, const int32_t* lens, int64_t B, int L,
                         int32_t user_off, int32_t item_off, int32_t sparse_off, int32_t* ids, lr_stream_t stream);
int lr_din_attn_pool_fwd_f32(const float* item_table, int64_t V, int K,
                             const int32_t* item, const int32_t* seq, const int32_t* len,
                             int64_t B, int L, const float* W1, const float* b1,
                             const float* W2, const float* b2, int H, float* out,
                             float* attn, float* hid /* [B*L, 16] or NULL */, int32_t* order_out /* [B] or NULL */,
                             lr_stream_t stream);
int lr_din_attn_pool_bwd_f32(const float* item_table, int64_t V, int K,
                             const int32_t* item, const int32_t* seq, const int32_t* len,
                             int64_t B, int L, const float* W1, const float* b1,
                             const float* W2, const float* b2, int H, const float* attn,
                             const float* gout, float* gq, float* gkey, float* gW1,
                             float* gb1, float* gW2, float* gb2, void* ws, size_t ws_bytes,
                             lr_stream_t stream);
/* The same backward cut in two for callers that run the halves on different streams (nets/din_fused.py: the
 * parameter half beside the table update): parts = 1: data half (gq, gkey and the dz spill in `ws`), 2: parameter
 * half (gW1, gb1, gW2, gb2 from the spill: must follow the data half of the same ws in stream / event order, and —
 * it re-reads the key rows — must not run beside an update of item_table), 3: both.  keep_pad_rows != 0: rows gkey[b, l >= len[b]] are left untouched instead of zeroed (for callers that
 * drop those positions from the table update: 103 MB of zeros per launch at BASELINE cfg 3).                      */
int lr_din_attn_pool_bwd_parts_f32(const float* item_table, int64_t V, int K,
                                   const int32_t* item, const int32_t* seq, const int32_t* len,
                                   int64_t B, int L, const float* W1, const float* b1,
                                   const float* W2, const float* b2, int H, const float* attn,
                                   const float* gout, float* gq, float* gkey, float* gW1,
                                   float* gb1, float* gW2, float* gb2, void* ws, size_t ws_bytes,
                                   int parts, int keep_pad_rows, const float* hid /* or NULL */,
                                   const int32_t* order /* [B] or NULL */, lr_stream_t stream);
/* When BOTH `hid` and the order buffer are given, `hid` must hold B * L * 16 + 3 * (K / 16) * 256 floats: the forward's extra
 * workgroup also leaves the data kernel's transposed weight images behind the hidden activations, and a backward given `hid` and
 * `order` reads them from there (the pair belongs to ONE forward / backward of the same W1). */
/* `order` (round 6, MFMA widths only): a permutation of the samples — slot s of the backward kernels' wave-strided walk takes
 * sample order[s].  The forward writes it on request (`order_out`, one extra workgroup of its launch): the stable partition by
 * descending key-tile count (class = min(ceil(len / 16), min(ceil(L / 16), 16))), which hands every wave one sample of each
 * length class (fixed strides left a third of the kernels' run time to a fraction of the waves).  Results per sample do not
 * depend on it; the parameter gradients are summed per wave, so a DIFFERENT order changes their last bits (a fixed order keeps
 * them run-to-run identical). */
/* `hid` (round 6; K in 16 / 32 / 64 / 128, otherwise LR_ESHAPE): the forward keeps the attention MLP's hidden activations
 * h = sigmoid(z) of every live (sample, key) pair ([B*L, 16] floats, rows past a sample's length untouched); the data half of
 * the backward given the same buffer reads them instead of recomputing the first layer (half of its MFMAs, no forward weight
 * images) — the gradients are those of the forward's own h.  NULL on both sides: the recomputing form. */
int lr_din_attn_dense_fwd_f32(const float* q, const float* keys, int K, const int32_t* len,
                              int64_t B, int L, const float* W1, const float* b1,
                              const float* W2, const float* b2, int H, float* out,
                              float* attn, lr_stream_t stream);
int lr_din_attn_dense_bwd_f32(const float* q, const float* keys, int K, const int32_t* len,
                              int64_t B, int L, const float* W1, const float* b1,
                              const float* W2, const float* b2, int H, const float* attn,
                              const float* gout, float* gq, float* gkey, float* gW1,
                              float* gb1, float* gW2, float* gb2, void* ws, size_t ws_bytes,
                              lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a16 + a17) Full-catalog scoring with fused top-k — replaces
 * `preds = user_embed @ item_embeds.T` (recommendation/recommend.py:66-68,
 * bases/dyn_embed_base.py:146) + rank_recommendations (recommendation/ranking.py:10-56,
 * filter_items :59-61, partition_select :76-78) + tf.math.top_k (bases/dyn_embed_base.py:303).
 *   scores[u,i] = <users[u,:], items[i,:]>   (exact f32 fma chain on the f32 MFMA pipe)
 *   per user: drop consumed items (CSR consumed_ptr/consumed_idx: ascending GLOBAL item ids,
 *   only for users with filter_flag[u] != 0 — the host sets it per ranking.py:38), keep the
 *   k largest, return them sorted by (score desc, id asc).
 *   out_ids are GLOBAL ids (= local row + item_base) so item-sharded callers can merge.
 *   Rows past the number of valid candidates are filled with id -1 / score -inf.
 * The B x N score matrix is never materialised.
 * ---------------------------------------------------------------------------------- */
/* Test hook of the loose lockstep between the workgroups of an item range (csrc/score_topk.hip): user-tile workgroup `ut` never
 * publishes its progress word, as if it were not resident — its partners run into the bound of the window-edge wait and drop the
 * lockstep; results must not change.  -1 (the default) mutes nobody. */
void lr_score_topk_test_mute(int ut);
size_t lr_score_topk_ws_bytes(int64_t B, int64_t N, int D, int k);
int lr_score_topk_f32(const float* users, int64_t B, const float* items, int64_t N, int D,
                      const int64_t* consumed_ptr /* [B+1] or NULL */,
                      const int32_t* consumed_idx, const uint8_t* filter_flag /* [B] or NULL */,
                      int k, int64_t item_base, float* out_scores /* [B,k] */,
                      int64_t* out_ids /* [B,k] */, void* ws, size_t ws_bytes,
                      lr_stream_t stream);
/* The same contract (same arguments, same workspace) with the scores taken as SPLIT-bf16 products: users and items are each
 * split exactly into three bf16 planes (the items on the fly, when a stage is written to LDS — no second copy of the catalogue),
 * the six largest cross products go through v_mfma_f32_32x32x16_bf16 with f32 accumulation.  Scores equal the f32 chain's to
 * f32 rounding (both within 1e-6 relative of fp64 at D = 128), NOT bit for bit, so the order of items whose fp64 scores differ by
 * less than that can differ.  Reduction widths above 128 run the f32 chain. */
int lr_score_topk_sb_f32(const float* users, int64_t B, const float* items, int64_t N, int D,
                         const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag,
                         int k, int64_t item_base, float* out_scores, int64_t* out_ids, void* ws, size_t ws_bytes,
                         lr_stream_t stream);
/* Filtered form (csrc/score_topk.hip, "Filtered scoring"): a one-product bf16 MFMA pass keeps, per user, the
 * k' = lr_score_topk_filter_kp(k) items of largest UPPER BOUND approx + 0.004 |u| |i| >= exact (the term rides in the MFMA chain);
 * their scores are recomputed in f32 and the k best kept; the result of a user is accepted only when its k-th exact score exceeds
 * the k'-th bound, which PROVES that no item outside the k' can belong to the top k — every other user is re-run by the exact
 * kernel (`exact_arith`: 0 the f32 chain, 1 split-bf16; the users concerned are gathered to the front on the device, few of them run
 * under a plan for 128 users) and its rows replaced.  Output contract = lr_score_topk_f32's, for any data (scores are f32 dot products; ids those of the exact ranking
 * up to the order of scores closer than f32 rounding).  Taken at N >= 2^20 items (flags bit 0: at any N), reduction widths 33..128,
 * k <= 100 (kp == 0 above) and k' < N; every other shape runs the exact kernel directly.  `failed_out` (nullable, [B] bytes):
 * 1 where a user went to the exact pass.  Workspace: lr_score_topk_filter_ws_bytes, 256-byte aligned. */
int lr_score_topk_filter_kp(int k);
size_t lr_score_topk_filter_ws_bytes(int64_t B, int64_t N, int D, int k);
int lr_score_topk_filter_f32(const float* users, int64_t B, const float* items, int64_t N, int D,
                             const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag,
                             int k, int64_t item_base, float* out_scores, int64_t* out_ids, void* ws, size_t ws_bytes,
                             int exact_arith, int flags, uint8_t* failed_out /* [B] or NULL */, lr_stream_t stream);
/* k-way merge of per-shard results (multi-GPU: after all-gather of [S,B,k] candidates). */
int lr_topk_merge_f32(const float* scores /* [S,B,k] */, const int64_t* ids /* [S,B,k] */,
                      int S, int64_t B, int k, float* out_scores, int64_t* out_ids,
                      lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a12) CSR SpMM — replaces torch.sparse.mm(laplacian_norm, all_embeddings[-1])
 * (algorithms/torch_modules/lightgcn_module.py:80).  Y[r,:] = sum_j val[j] * X[col[j],:].
 * `beta_acc` != NULL fuses the layer mean of lightgcn_module.py:83-84:
 *   acc[r,:] += Y[r,:] (the running sum of E^0..E^L, divided by L+1 by the caller).
 * Y == NULL with acc != NULL: accumulate only (acc += A X, the product's rows are not stored) — the
 * row-sharded net multiplies by one column block of its slice per arrived chunk of X and adds
 * block after block into one table.  Holds for the bucketed / masked forms below as well.
 * Â is symmetric, so the backward is the same operator.
 * ---------------------------------------------------------------------------------- */
int lr_spmm_csr_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                    int64_t rows, const float* X, int K, float* Y, float* acc,
                    lr_stream_t stream);
/* Degree-bucketed form of the same product (Zipf-degree graphs): rows of more than 128 nonzeros are cut
 * into 2,048-nonzero chunks listed by a device pre-pass and summed by whole workgroups (every workgroup takes
 * its share of the chunks, then of the short rows); multi-chunk rows are finished in chunk order (fixed summation order per row, no atomics
 * on the data).  `nnz` = rowptr[rows]; workspace from lr_spmm_csr_ws_bytes(rows, nnz, K), 16-byte
 * aligned.  Shapes the vector kernels do not take (K not in {16,32,64,128} or unaligned) run
 * lr_spmm_csr_f32. */
size_t lr_spmm_csr_ws_bytes(int64_t rows, int64_t nnz, int K);
int lr_spmm_csr_bucketed_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t rows,
                             int64_t nnz, const float* X, int K, float* Y, float* acc, void* ws,
                             size_t ws_bytes, int lists_ready, lr_stream_t stream);
/* `lists_ready` != 0: `ws` still holds the chunk lists of an earlier call with the SAME rowptr (they depend on the
 * graph's row lengths alone) — the classification pre-pass is skipped (LightGCN multiplies by one static graph six times
 * per step).  The chunk-sum scratch inside `ws` is rewritten by every call. */
/* The same product restricted by row bitmaps (uint32 words, bit r of word r / 32; each nullable):
 *   xmask  rows of X whose bit is clear are known to be zero and are not read — the first backward product of a LightGCN
 *          training step multiplies by d loss / d (layer sum), nonzero on the batch's rows only (lightgcn_module.py:66-88
 *          under autograd; torchops/loss.py:bpr_loss reads the batch's rows).  Same bits as the plain product (y + a * 0 == y).
 *   ymask  only the rows of Y whose bit is set are computed and written (the others keep their contents) — the last forward
 *          product of a training step is read at the batch's rows only.
 * K in {16, 32, 64, 128} and 16-byte aligned operands (LR_ESHAPE otherwise).  lr_bitmap_ids_i32 sets (set != 0) the bits of the
 * listed ids or clears their words (set == 0: use it with the list that set them). */
int lr_spmm_csr_masked_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t rows, int64_t nnz,
                           const float* X, int K, float* Y, float* acc, const uint32_t* xmask, const uint32_t* ymask,
                           void* ws, size_t ws_bytes, int lists_ready, lr_stream_t stream);
int lr_bitmap_ids_i32(const int32_t* ids, int64_t n, int64_t n_bits, uint32_t* bitmap, int set, lr_stream_t stream);
/* The product whose rows ARE the gradient of a parameter table, with the optimiser step as its epilogue (the last backward
 * product of a LightGCN step: libreco/algorithms/torch_modules/lightgcn_module.py:66-88 under autograd, then
 * libreco/training/torch_trainer.py:63-69): for every row r, g = sum_j val[j] X[col[j]] (+ alpha * gsum[row_slot[r]] where
 * row_slot[r] >= 0: the loss's own gradient rows of the batch, summed per distinct row) and one Adam step of (w, m, v[, vmax])
 * row r with g — the arithmetic of lr_embed_scatter_add_f32 + lr_adam_dense_f32 without the gradient table in between.
 * `row_slot` int32[rows] / `gsum` [n, K]: both or neither.  K in {16, 32, 64, 128}, 16-byte aligned (LR_ESHAPE otherwise). */
int lr_spmm_csr_adam_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t rows, int64_t nnz,
                         const float* X, int K, float* w, float* m, float* v, float* vmax, const int32_t* row_slot,
                         const float* gsum, float alpha, lr_adam_hp hp, void* ws, size_t ws_bytes, int lists_ready,
                         lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a19) Pointwise scoring — replaces predict_from_embedding (prediction/predict.py:36-40):
 *   out[i] = <U[user[i],:], I[item[i],:]>
 * ---------------------------------------------------------------------------------- */
int lr_pair_dot_f32(const float* U, int64_t nU, const float* I, int64_t nI, int D,
                    const int32_t* user, const int32_t* item, int64_t n, float* out,
                    lr_stream_t stream);

/* Batch statistics of the gathered block e[B,F,K] (the input of the first BatchNorm,
 * layers/dense.py:30-31) computed from the batch's segments instead of from e:
 *   sum_b e[b,f,k] = sum over field f's runs of len(run) * table[row,k]   (same for squares).
 * `field_row_start[F+1]` (device) gives each field's global row range; the runs must come from
 * lr_segments_build over the same idx.  Writes C partial sums per field:
 * partial[F][C][2][K] = {sum, sum of squares}; the caller adds the C chunks (fixed order).     */
int lr_fm_field_stats_f32(const float* table, int K, const int32_t* seg_rows,
                          const int32_t* seg_start, const int32_t* n_seg,
                          const int32_t* field_row_start, int F, int C, float* partial,
                          lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a12) Normalised bipartite Laplacian on the device — replaces LightGCNModel._build_laplacian_matrix
 * (algorithms/torch_modules/lightgcn_module.py:36-61).  Input: the interaction list (users[e], items[e]), any
 * order, repeats allowed (they collapse, like the reference's dok assignment); pairs outside the id ranges are
 * dropped.  Output: CSR over nodes [users | items] of  A^ = D^-1/2 [[0,R],[R^T,0]] D^-1/2  with ascending columns
 * per row: rowptr [n_users + n_items + 1], col / val [2 * n_pairs] (caller sizes them for 2 * E), the number of
 * distinct pairs in n_pairs[0] (device), and — if tperm != NULL — the transpose map  A^T.val = A.val[tperm]
 * (needed by edge dropout, lightgcn_module.py:90-96).  Integer work bit-exact; val = fp32 product of
 * deg^-1/2 factors rounded from double.  2 * E < 2^31.  Workspace from lr_csr_laplacian_ws_bytes(E).
 * ---------------------------------------------------------------------------------- */
size_t lr_csr_laplacian_ws_bytes(int64_t E);
int lr_csr_laplacian_build(const int32_t* users, const int32_t* items, int64_t E, int64_t n_users,
                           int64_t n_items, int64_t* rowptr, int32_t* col, float* val, int32_t* tperm,
                           int64_t* n_pairs, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (a15, device form — SURVEY row f1) Negative sampling on the device with the acceptance rules of
 * sampling/negatives.py:17-31 (random: != positive) and :55-82 (unconsumed: additionally not among
 * the negatives already drawn for that positive and, for the first 10 of 20 tries, not in the
 * user's consumed list), driven by a counter-based generator: out[p*num_neg + j] is a pure
 * function of (seed, p, j).  consumed_ptr/consumed_idx (both or neither): CSR of ascending item
 * ids per user.  The host samplers of the reference use numpy / Python RNG streams; this sampler
 * is opt-in and has its own bit-exact oracle.
 * ---------------------------------------------------------------------------------- */
int lr_sample_negatives_i32(const int32_t* users, const int32_t* items_pos, int64_t n,
                            int num_neg, int32_t n_items, const int64_t* consumed_ptr,
                            const int32_t* consumed_idx, uint64_t seed, int32_t* out,
                            lr_stream_t stream);

/* (f2) MLP tail of a DeepFM (user, item) pair for full-catalog ranking without the feature cross product
 * (libreco/recommendation/recommend.py:81-105, preprocess.py:110-172 materialise one feature row per pair):
 *   out[u][i] (+)= sum_c relu( sum_k relu(P[u][k] + Q[i][k]) * W2[k][c] + b2[c] ) * v3[c] + c3
 * P [B,H1] / Q [N,H1]: user / item part of the first Dense layer; W2 [H1,H2], b2, v3 [H2], c3: the rest of a
 * three-layer `dense_nn` + output weights with the inference BatchNorms folded (recommendation/catalog.py).
 * (H1, H2) in {64,128} x {32,64} (lr_pair_mlp_supported); out row stride ld_out >= N. */
int lr_pair_mlp_supported(int H1, int H2);
int lr_pair_mlp_f32(const float* P, int64_t B, const float* Q, int64_t N, int H1, const float* W2,
                    const float* b2, int H2, const float* v3, float c3, float* out, int64_t ld_out,
                    int accumulate, lr_stream_t stream);
/* The same contract with the H1 x H2 product as six-term split-bf16 products (relu(p + q) split exactly into three bf16 planes
 * per pair on the fly, W2's planes in LDS, f32 accumulation): equal to lr_pair_mlp_f32 to f32 rounding, not bit for bit. */
int lr_pair_mlp_sb_f32(const float* P, int64_t B, const float* Q, int64_t N, int H1, const float* W2,
                       const float* b2, int H2, const float* v3, float c3, float* out, int64_t ld_out,
                       int accumulate, lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * Alternating least squares (csrc/als.hip) — replaces the CPU solver of ALS, `als_update` with `_least_squares`
 * (libreco/algorithms/_als.pyx:99-167, per-row `sposv`) and `_least_squares_cg` (_als.pyx:170-268, cg_steps CG iterations
 * from the current row), and the `initialA` Gram of both (_als.pyx:116-120, 189-193).  K in 1..128 (lr_als_supported).
 *   lr_als_gram_f32        G0 [K, K] = Y^T Y + reg I over the N rows of Y (implicit != 0) or reg I (explicit); the Gram is
 *                          split over workgroups into K x K partials (ws: lr_als_gram_ws_bytes(N, K)) summed in a fixed order.
 *   lr_als_plan_params     out3 = {light cap, heavy degree, chunk}: rows of degree <= light cap are solved one per wave from
 *                          LDS (CG only), rows of degree > heavy degree are formed in `chunk`-interaction slabs over many
 *                          workgroups, the rest one per workgroup.  Host-only.
 *   lr_als_ws_bytes        slab workspace of a half-sweep whose heavy rows hold n_chunks chunks (host-only).
 *   lr_als_half_sweep_f32  every row m of X [rows, K] (in place) against Y: A_m = G0 + sum_i w_i y_i y_i^T, b_m = sum_i
 *                          beta_i y_i over the CSR row (int64 rowptr, int32 col, f32 val); implicit: w = val - 1, beta = val
 *                          (val = the confidence alpha r + 1); explicit: w = 1, beta = val.  use_cg: cg_steps CG iterations
 *                          from x (continue when r.r < 1e-10, break when the new r.r < 1e-10), else the Cholesky solve; a
 *                          non-positive pivot k sets fail[m] = k + 1 and leaves row m unchanged (fail: int32 [rows], the
 *                          caller zeroes it; may be NULL with use_cg).  `plan` (int32): light rows [n_light], medium rows
 *                          [n_medium], heavy rows [n_heavy], chunk_begin [n_heavy + 1] (prefix sums of ceil(deg / chunk)),
 *                          chunk_row [n_chunks] (the heavy slot of each chunk); every row listed exactly once.
 *                          stage_mask: 1 light, 2 medium, 4 heavy slabs, 8 heavy solves (15 = the whole sweep; the parts
 *                          exist for per-kernel timing, 8 needs 4 first).  No atomics: identical bits run to run. */
int lr_als_supported(int K);
int lr_als_plan_params(int K, int32_t* out3);
size_t lr_als_ws_bytes(int64_t n_chunks, int K);
size_t lr_als_gram_ws_bytes(int64_t N, int K);
int lr_als_gram_f32(const float* Y, int64_t N, int K, float reg, int implicit, float* G0, void* ws, size_t ws_bytes,
                    lr_stream_t stream);
int lr_als_half_sweep_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t rows, float* X,
                          const float* Y, int K, const float* G0, int implicit, int use_cg, int cg_steps,
                          const int32_t* plan, int64_t n_light, int64_t n_medium, int64_t n_heavy, int64_t n_chunks,
                          int32_t* fail, void* ws, size_t ws_bytes, int stage_mask, lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * UserCF / ItemCF (csrc/cf_sim.hip, csrc/cf_rank.hip) — replace the similarity engine of the CF models,
 * `invert_*` / `forward_*` of libreco/utils/_similarities.pyx:17-533 (called by utils/similarities.py:32-203), and the
 * pure-Python ranking of libreco/bases/cf_base.py:212-250 (compute_pred), :310-355 (rank_recommendations,
 * get_top_k_sims), algorithms/item_cf.py:70-149 and algorithms/user_cf.py:70-147 (predict, recommend_one).
 *   lr_cf_sim_tile_cols   columns per LDS tile of the similarity kernel (host-only).
 *   lr_cf_sim_ws_bytes    workspace of lr_cf_sim_f32 (one work counter; host-only).
 *   lr_cf_sim_f32         the similarity of X (forward CSR, n_x rows, int64 rowptr, int32 ascending col, f32 val) with Y
 *                         (its transpose): for every pair the products of the shared y are summed in ascending y with an
 *                         unfused multiply and add, the count of shared y is kept; sim_type 0 cosine (norm = row norms),
 *                         1 pearson (val of X and Y already mean-centred per x row, norm = the centred norms), 2 jaccard
 *                         (cnt = row degrees, val / norm unused).  A pair is kept when count >= min_common (values below
 *                         1 act as 1) and its value is not 0.  Work items (item_row, item_tile) are (row, column tile)
 *                         pairs in row order then tile order, run in the order `order` (any permutation of the items);
 *                         pass 0 writes item_nnz (int64 [n_items]), pass 1 writes the kept columns ascending with their
 *                         values at item_off (int64 [n_items], the exclusive scan of item_nnz).  No atomics on values:
 *                         identical bits run to run.
 *   lr_cf_select_max      keys sorted per round by the selection of the top-k and recommend kernels (host-only).
 *   lr_cf_topk_f32        for every CSR row the first min(k, len) entries by (value descending, column ascending):
 *                         out_ids / out_sims [n_rows, k], out_len [n_rows].
 *   lr_cf_recommend_ws_bytes / lr_cf_recommend_f32   for every user u = users[b]: ItemCF (user_cf 0) adds sim * label over
 *                         u's items (ui: user x item CSR) in ascending id and each item's top-k list (tk_*, [.., tk_k]) in
 *                         order; UserCF (user_cf 1) over u's top-k users in order and each one's items in ascending id;
 *                         f32 products and sequential f32 sums.  The touched items are the candidates; with
 *                         filter_consumed the items of row b of the consumed CSR (cons_ptr int64 [B + 1]) are removed.
 *                         out_ids / out_scores [B, n_rec] by (score descending, id ascending), out_len = min(n_rec,
 *                         out_ncand), out_fallback: 0 ranked, 1 nothing touched, 2 every candidate consumed.  ws:
 *                         B x n_items f32 scores and flags.
 *   lr_cf_predict_f32     for every pair q the first k entries of similarity row srow[q] (column order) that appear in
 *                         the sorted interaction row irow[q] with a positive value: rating (rating != 0) sum(l * s / S) /
 *                         sum(s / S) clipped to [lower, upper], ranking the mean of s; none[q] = 1 and pred[q] =
 *                         default_pred when there is none. */
int lr_cf_sim_tile_cols(void);
size_t lr_cf_sim_ws_bytes(void);
int lr_cf_sim_f32(const int64_t* x_ptr, const int32_t* x_col, const float* x_val, const int64_t* y_ptr,
                  const int32_t* y_col, const float* y_val, int64_t n_x, const float* norm, const int32_t* cnt,
                  int sim_type, int min_common, const int32_t* item_row, const int32_t* item_tile,
                  const int32_t* order, int64_t n_items, int pass, int64_t* item_nnz, const int64_t* item_off,
                  int32_t* out_col, float* out_val, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_cf_select_max(void);
int lr_cf_topk_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, int64_t k,
                   int32_t* out_ids, float* out_sims, int32_t* out_len, lr_stream_t stream);
size_t lr_cf_recommend_ws_bytes(int64_t B, int64_t n_items);
int lr_cf_recommend_f32(const int32_t* users, int64_t B, int user_cf, const int64_t* ui_ptr, const int32_t* ui_col,
                        const float* ui_val, const int32_t* tk_ids, const float* tk_sims, const int32_t* tk_len,
                        int64_t tk_k, int64_t n_items, const int64_t* cons_ptr, const int32_t* cons_idx,
                        int filter_consumed, int64_t n_rec, int32_t* out_ids, float* out_scores, int32_t* out_len,
                        int64_t* out_ncand, int32_t* out_fallback, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_cf_predict_f32(const int32_t* srow, const int32_t* irow, int64_t n, const int64_t* s_ptr, const int32_t* s_col,
                      const float* s_val, const int64_t* i_ptr, const int32_t* i_col, const float* i_val, int64_t k,
                      int rating, float lower, float upper, float default_pred, float* pred, int32_t* none,
                      lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * RsUserCF / RsItemCF (csrc/cf_sim.hip, csrc/cf_state.hip) — replace the engine of the reference's incremental
 * neighbourhood models: rust/src/similarities.rs:13-180 (compute_sum_squares, invert_cosine), incremental.rs:9-115
 * (update_sum_squares, update_cosine, accumulate_cosine) and the predict of item_cf.rs:118-153 / user_cf.rs:113-148 with
 * inference.rs:11-71.  The state of n_x rows is a symmetric CSR without diagonal (int64 rowptr, int32 ascending col) of
 * every pair with a count above 0, carrying prod f32, cnt int32 and sim f32, and sumsq f32 [n_x].  No floating-point
 * atomics anywhere: identical bits run to run.
 *   lr_cf_pair_state_f32   the accumulation of lr_cf_sim_f32 (same X / Y, work items, passes and workspace,
 *                         lr_cf_sim_ws_bytes) with another epilogue: every column whose count of shared y is above 0 is
 *                         written with its product sum (out_prod, ascending y, unfused multiply and add) and its count
 *                         (out_cnt), a sum of exactly 0 included; nothing is normalised.
 *   lr_cf_sumsq_f32       out[r] = s (accumulate 0) or out[r] + s (accumulate != 0, one f32 add), s the sequential f32 fold
 *                         from 0 of val * val over CSR row r in stored (ascending column) order; out f32 [n_rows].
 *   lr_cf_state_merge_f32 the row-wise union of the old state (o_*, o_nnz entries) and a delta (d_*, d_nnz entries, from
 *                         lr_cf_pair_state_f32), both over n_x rows (the caller pads the old rowptr for new rows).  Pass 0
 *                         writes is_new (uint8 [d_nnz]): 1 where the old row lacks the delta entry's column.  Pass 1 takes
 *                         rank (int64 [d_nnz + 1], the exclusive scan of is_new with the total last) and writes the
 *                         o_nnz + rank[d_nnz] entries of the union in row order with ascending columns: a pair of the
 *                         delta gets prod = old + delta (the delta alone if new), cnt = old + delta and
 *                         sim = prod / (sqrt(sumsq[x1]) * sqrt(sumsq[x2])), correctly rounded, 0 if prod or either sum
 *                         is 0; every other pair keeps its three values bit for bit.  The new rowptr is
 *                         o_ptr + rank[d_ptr] (the caller's).  Entries, not rows, are spread over the workgroups, so
 *                         rows of any length are handled alike.  Columns must be below n_x.
 *   lr_cf_predict_topk_f32   for every pair q the first min(k, tk_len) entries of the top-k list of row srow[q] (tk_*, as
 *                         written by lr_cf_topk_f32) that the sorted interaction row irow[q] holds, whatever their
 *                         label: ranking (rating 0) S / n with S the sequential f32 sum of the hit sims in list order,
 *                         rating the sequential sum of (label * sim) / S; unclipped.  none[q] = 1 and pred[q] =
 *                         default_pred where there is no hit. */
int lr_cf_pair_state_f32(const int64_t* x_ptr, const int32_t* x_col, const float* x_val, const int64_t* y_ptr,
                         const int32_t* y_col, const float* y_val, int64_t n_x, const int32_t* item_row,
                         const int32_t* item_tile, const int32_t* order, int64_t n_items, int pass, int64_t* item_nnz,
                         const int64_t* item_off, int32_t* out_col, float* out_prod, int32_t* out_cnt, void* ws,
                         size_t ws_bytes, lr_stream_t stream);
int lr_cf_sumsq_f32(const int64_t* ptr, const float* val, int64_t n_rows, int accumulate, float* out,
                    lr_stream_t stream);
int lr_cf_state_merge_f32(const int64_t* o_ptr, const int32_t* o_col, const float* o_prod, const int32_t* o_cnt,
                          const float* o_sim, int64_t o_nnz, const int64_t* d_ptr, const int32_t* d_col,
                          const float* d_prod, const int32_t* d_cnt, int64_t d_nnz, int64_t n_x, const float* sumsq,
                          int pass, uint8_t* is_new, const int64_t* rank, int32_t* out_col, float* out_prod,
                          int32_t* out_cnt, float* out_sim, lr_stream_t stream);
int lr_cf_predict_topk_f32(const int32_t* srow, const int32_t* irow, int64_t n, const int32_t* tk_ids,
                           const float* tk_sims, const int32_t* tk_len, int64_t tk_k, int64_t k, const int64_t* i_ptr,
                           const int32_t* i_col, const float* i_val, int rating, float default_pred, float* pred,
                           int32_t* none, lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * Swing (csrc/swing.hip) — replaces the score engine of the reference's Swing model, rust/src/graph.rs:143-233
 * (compute_single_swing: every user pair of every item, the pair's term scattered over the pair's common items, with a
 * 100 M-entry cache of intersections and a thread pool; compute_swing_scores: the weights 1 / sqrt(|I_u|), :210-213).
 * The score CSR has the layout of the CF similarity, so lr_cf_topk_f32 / lr_cf_recommend_f32 / lr_cf_predict_f32 rank it.
 *   lr_swing_tile_cols    columns per LDS tile of the pair-table kernel (host-only).
 *   lr_swing_lds_users    the longest intersection a wave of the score kernel keeps in LDS (host-only).
 *   lr_swing_pairs_ws_bytes   workspace of lr_swing_pairs_f32 (one work counter; host-only).
 *   lr_swing_pairs_f32    the user-pair table: for every u and every v > u that shares an item with u,
 *                         f_uv = (w_u * w_v) * (1 / (alpha + (c_uv - 1))) with c_uv the number of shared items and
 *                         w_u = 1 / sqrt(|I_u|), correctly rounded f32 operations, no fused multiply-add
 *                         (graph.rs:185-186).  u_ptr / u_col: user x item CSR, i_ptr / i_col: its transpose (int64 rowptr,
 *                         int32 ascending col).  Work items (item_row, item_tile) are (user, column tile) pairs in row then
 *                         tile order, run in the order `order`; pass 0 writes item_nnz (int64 [n_items]), pass 1 writes
 *                         the columns ascending and the values at item_off (the exclusive scan of item_nnz).  The counts
 *                         are accumulated with integer LDS atomics; no floating-point atomics.
 *   lr_swing_scores_ws_bytes / lr_swing_scores_f32   the scores on a given pattern: s_ptr / s_col is a symmetric item x
 *                         item CSR pattern (columns ascending, no diagonal) whose entries (i, j) all have at least two
 *                         common users, s_row the row of every entry, i_ptr / i_col the item x user CSR, max_item_users
 *                         its longest row, p_* the pair table over n_users users.  One wave per entry with j > i intersects U_i and U_j and
 *                         sums f_uv over the pairs u < v of the intersection (found in row u by binary search, or by offset when the row holds
 *                         every v > u; each lane a fixed stride of the pairs, then
 *                         a fixed butterfly); the sum is written to (i, j) and (j, i): identical bits run to run and
 *                         s == s^T bit for bit.  ws: a work counter and, when max_item_users exceeds
 *                         lr_swing_lds_users, one slot of max_item_users int32 per resident wave. */
int lr_swing_tile_cols(void);
int lr_swing_lds_users(void);
size_t lr_swing_pairs_ws_bytes(void);
int lr_swing_pairs_f32(const int64_t* u_ptr, const int32_t* u_col, const int64_t* i_ptr, const int32_t* i_col,
                       int64_t n_users, float alpha, const int32_t* item_row, const int32_t* item_tile,
                       const int32_t* order, int64_t n_items, int pass, int64_t* item_nnz, const int64_t* item_off,
                       int32_t* out_col, float* out_val, void* ws, size_t ws_bytes, lr_stream_t stream);
size_t lr_swing_scores_ws_bytes(int64_t max_item_users);
int lr_swing_scores_f32(const int64_t* i_ptr, const int32_t* i_col, int64_t max_item_users, int64_t n_users,
                        const int64_t* p_ptr, const int32_t* p_col, const float* p_val, const int64_t* s_ptr,
                        const int32_t* s_col, const int32_t* s_row, int64_t nnz, float* s_val, void* ws, size_t ws_bytes,
                        lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * BPR — replaces the loop of libreco/algorithms/_bpr.pyx:116-399 (SGD / momentum / Adam over (user, positive, negative)
 * triples) and the forward / backward of the TF graph of libreco/algorithms/bpr.py:161-204.
 *   lr_bpr_triple_score_f32  per sample s < W:  d = sum_{j < D} U[users[s], j] (I[pos[s], j] - I[neg[s], j])
 *       (+ ibias[pos[s]] - ibias[neg[s]] if ibias != NULL),  c[s] = 1 / (1 + exp(d)) in [0, 1],  loss[s] (nullable)
 *       = -log sigmoid(d), finite for every d.  A sample with an id outside its table gets c = -1, loss = 0 and takes no part
 *       in what follows.  U is [nU, ldu], I is [nI, ldi] (ldu, ldi >= D).  mode:
 *         LR_BPR_SCORE  nothing else is written;
 *         LR_BPR_STASH  gu [W, D] = I[pos] - I[neg], the window-start difference the user pass of the engine reads;
 *         LR_BPR_GRAD   the per-position gradient rows of gscale * sum_s loss[s] (gscale = 1 / B for the mean):
 *                       gu [W, D] = -a (p - q), gi [2 W, D] = -a u (row 2 s, the positive) and +a u (row 2 s + 1, the
 *                       negative), gb [2 W] (nullable) = -a, +a, with a = gscale * c[s] — ready for lr_embed_scatter_*.
 *   lr_bpr_row_update_f32    the ordered row update of one window.  (seg_*, n_seg) is lr_segments_build over the window's
 *       ids: the W user ids (other_ids == NULL, n == W; `other` is the stash gu [W, D], other_rows = W), or the 2 W item ids
 *       interleaved positive, negative per sample (other_ids = users [W], n == 2 W; `other` is the user table
 *       [other_rows, D], not yet updated for this window), so ascending position is ascending sample order.  Every touched
 *       row takes, once per occurrence and in that order, the reference's step with the gradient
 *       g = +-c[s] other[.] - reg * row_at_window_start on its columns j < Dw (Dw = D - 1 for users: their bias column is
 *       never written; Dw = D for items): sgd x += lr g; momentum (0.9) v = 0.9 v + lr g, x += v (state1); adam (0.9,
 *       0.999, 1e-8, bias correction by `epoch`) m, h in state1, state2.  table / state* are [V, D].  The row and its state
 *       are read and written once and the chain runs in registers: same bits from run to run, no atomics; the loop is
 *       bounded by the run length, so no id can make it wait.
 * D in [1, 256] (lr_bpr_supported), otherwise LR_ESHAPE.
 * ---------------------------------------------------------------------------------- */
#define LR_BPR_SCORE 0
#define LR_BPR_STASH 1
#define LR_BPR_GRAD 2
#define LR_BPR_SGD 0
#define LR_BPR_MOMENTUM 1
#define LR_BPR_ADAM 2
int lr_bpr_supported(int D);
int lr_bpr_triple_score_f32(const float* U, int64_t nU, int ldu, const float* I, int64_t nI, int ldi,
                            const float* ibias, int D, const int32_t* users, const int32_t* pos,
                            const int32_t* neg, int64_t W, int mode, float gscale, float* c, float* loss,
                            float* gu, float* gi, float* gb, lr_stream_t stream);
int lr_bpr_row_update_f32(int optimizer, float* table, float* state1, float* state2, int64_t V, int D, int Dw,
                          const int32_t* seg_pos, const int32_t* seg_rows, const int32_t* seg_start,
                          const int32_t* n_seg, int64_t n, const float* c, int64_t W, const float* other,
                          int64_t other_rows, const int32_t* other_ids, double lr, double reg, int epoch,
                          lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * SVD / SVD++ — replace the forward / backward of the TF graphs of libreco/algorithms/svd.py:103-144 and
 * libreco/algorithms/svdpp.py:102-135,196-214 (f32, rows of K floats, K in [1, 512]: lr_svd_supported, otherwise LR_ESHAPE).
 * No float atomics anywhere: same bits from run to run.  Ids outside a table are dropped, never dereferenced.
 *   lr_svdpp_pool_f32  out[r, :] = P[row(r), :] + |N|^-1/2 sum_e Y[hist_idx[e], :] over e in hist_ptr[row(r)] ..
 *       hist_ptr[row(r) + 1], in that order (the `sqrtn` combiner of safe_embedding_lookup_sparse: a repeated item counts
 *       twice in the sum and in |N|).  P [n_users, K] may be NULL (only the pooled term is written).  `rows` int32 [n_rows]
 *       lists the users, or is NULL: row(r) = r (n_rows <= n_users).  `n_rows_dev` (nullable, needs `rows`): a device int32
 *       holding how many leading entries of `rows` are valid (the n_seg of lr_segments_build); the rows beyond are not
 *       written.  An empty history returns P's row bit for bit (zeros without P).  hist_ptr int64 [n_users + 1], hist_idx
 *       int32 [nnz]; an entry outside [0, n_items) adds nothing but counts in |N|; a user outside [0, n_users) gives a zero row.
 *       `scale_out` (nullable) [n_rows] receives |N|^-1/2 (0 for an empty history).  A history of any length is one launch.
 *   lr_mf_score_f32    per sample s < B:  score = bu[users[s]] + bi[items[s]] + <X[x(s), :], Q[items[s], :]> with x(s) =
 *       xidx[s] (the sample's slot of a pooled block X [nX, K]) or, xidx == NULL, users[s] (X is the user table);  loss[s]:
 *         LR_MF_MSE            (score - label)^2
 *         LR_MF_CROSS_ENTROPY  max(s, 0) - s label + log1p(exp(-|s|))
 *         LR_MF_FOCAL          w (1 - p_t)^2 bce, w = 0.25 label + 0.75 (1 - label), p_t = label p + (1 - label)(1 - p)
 *       and g[s] = gscale * d loss[s] / d score (gscale = 1 / B for the mean); all three finite for |score| in the
 *       thousands.  bu, bi nullable (0).  A sample with an id (user, item or x) outside its table gets score = loss = g = 0.
 *       mode LR_MF_SCORE writes nothing else; LR_MF_GRAD also gx [B, K] = g Q[item] and gq [B, K] = g X[x].
 *   lr_svdpp_hist_grad_f32  the gradient of Y.  An entry e < n of the concatenated histories of the batch's distinct users
 *       is (its Y row, ent_slot[e] = its user's slot); (seg_*, n_seg) is lr_segments_build over the n Y rows.  Every touched
 *       row takes gsum = sum_e scale[ent_slot[e]] * G[ent_slot[e], :] over its run, in run order (G [n_slots, K]: the
 *       per-user sums of gx; scale [n_slots]: scale_out of the pool); runs of more than 64 entries are summed in chunks of 64
 *       whose partials are added in chunk order (needs ws of lr_svdpp_hist_grad_ws_bytes(n, K) bytes, contents arbitrary;
 *       with ws == NULL such runs are walked by one lane group).  No [n, K] buffer is read or written.  mode:
 *         LR_SVD_HIST_ADAM  Y, m, v [n_items, K]: one Adam step (hp) of every touched row with gsum;
 *         LR_SVD_HIST_ROWS  grows [>= n_seg, K] = gsum per run, for lr_adam_dense_f32.
 * ---------------------------------------------------------------------------------- */
#define LR_MF_MSE 0
#define LR_MF_CROSS_ENTROPY 1
#define LR_MF_FOCAL 2
#define LR_MF_SCORE 0
#define LR_MF_GRAD 1
#define LR_SVD_HIST_ADAM 0
#define LR_SVD_HIST_ROWS 1
int lr_svd_supported(int K);
int lr_svdpp_pool_f32(const float* P, const float* Y, int64_t n_users, int64_t n_items, int K,
                      const int64_t* hist_ptr, const int32_t* hist_idx, int64_t nnz, const int32_t* rows,
                      const int32_t* n_rows_dev, int64_t n_rows, float* out, float* scale_out, lr_stream_t stream);
int lr_mf_score_f32(const float* X, int64_t nX, const int32_t* xidx, const float* Q, int64_t n_items,
                    const float* bu, int64_t n_users, const float* bi, int K, const int32_t* users,
                    const int32_t* items, const float* labels, int64_t B, int loss_kind, int mode, float gscale,
                    float* score, float* loss, float* g, float* gx, float* gq, lr_stream_t stream);
size_t lr_svdpp_hist_grad_ws_bytes(int64_t n_max, int K);
int lr_svdpp_hist_grad_f32(int mode, float* Y, float* m, float* v, int64_t n_items, int K, const float* G,
                           const float* scale, int64_t n_slots, const int32_t* ent_slot, const int32_t* seg_pos,
                           const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg, int64_t n,
                           float* grows, lr_adam_hp hp, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Recurrent layers — one GRU or LSTM layer of libreco/layers/recurrent.py:27-45 (the Keras layers of the TF2 branch with a
 * sequence mask) over a padded, left-aligned batch, f32, D inputs and H units, both in [1, 128] (lr_rnn_supported,
 * otherwise LR_ESHAPE).  No float atomics anywhere: same bits from run to run.
 *   LR_RNN_GRU   Keras v2, reset_after: W [D, 3H], U [H, 3H], b [2, 3H], gate order z, r, h:
 *                  mx = x_t W + b[0], mh = h U + b[1], z = sigmoid(mx_z + mh_z), r = sigmoid(mx_r + mh_r),
 *                  c = act(mx_h + r * mh_h), h' = z * h + (1 - z) * c
 *   LR_RNN_LSTM  W [D, 4H], U [H, 4H], b [4H], gate order i, f, c, o:  c' = f * c + i * act(.), h' = o * act(c')
 *   `act` != 0: tanh; 0: the identity (the reference's activation=None under use_layer_norm).
 * Input: x [B, L, D], or x == NULL and (table [V, D], ids int32 [B, L]) read in place (no [B, L, D] buffer is written).
 * `lens` int32 [B] is clamped to [0, L].  Step t of sample b is MASKED when t >= lens[b], or on the table path when its id is
 * outside [0, V): h (and c) are carried, hs[b, t] = the carried h (hs[:, L-1] is the last valid state; all 0 for lens = 0),
 * the id is never dereferenced and the row it names is never used; gx is exactly 0 there.
 * Dropout (nullable, constant over time, drawn and scaled by 1 / (1 - p) by the caller): x_t * in_mask [B, D] feeds the W
 * product, h * rec_mask [B, H] feeds the U product only; the carry term z * h uses the unmasked state.
 *   forward   writes every element of hs [B, L, H] and of `saved` (lr_rnn_fwd_saved_bytes(cell, B, L, H) bytes: the gates,
 *             and the LSTM's cell state, that the backward reads), masked steps included.
 *   backward  ghs [B, L, H] = the gradient with respect to every output step.  Writes every element of gx [B, L, D], gW, gU and
 *             gb (the shapes of W, U, b).  The weight gradients are summed over B and L as per-chunk partials in `ws`
 *             (lr_rnn_bwd_ws_bytes(cell, B, L, D, H) bytes, contents arbitrary on entry) added in chunk order.
 * ---------------------------------------------------------------------------------- */
#define LR_RNN_GRU 0
#define LR_RNN_LSTM 1
int lr_rnn_supported(int cell, int D, int H);
size_t lr_rnn_fwd_saved_bytes(int cell, int64_t B, int L, int H);
size_t lr_rnn_bwd_ws_bytes(int cell, int64_t B, int L, int D, int H);
int lr_rnn_layer_fwd_f32(int cell, int act, const float* x, const float* table, int64_t V, const int32_t* ids,
                         const int32_t* lens, int64_t B, int L, int D, int H, const float* W, const float* U,
                         const float* b, const float* in_mask, const float* rec_mask, float* hs, void* saved,
                         size_t saved_bytes, lr_stream_t stream);
int lr_rnn_layer_bwd_f32(int cell, int act, const float* x, const float* table, int64_t V, const int32_t* ids,
                         const int32_t* lens, int64_t B, int L, int D, int H, const float* W, const float* U,
                         const float* in_mask, const float* rec_mask, const float* hs, const void* saved,
                         const float* ghs, float* gx, float* gW, float* gU, float* gb, void* ws, size_t ws_bytes,
                         lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * WaveNet — the user side of libreco/algorithms/wave_net.py:181-222 (TF2 branch) in one forward launch: n_blocks *
 * n_per_block dilated causal convolutions of kernel size 2 with ReLU, a 1x1 convolution with ReLU and a max pool over time,
 * f32 on the VALU.  L, D (table width) and F (filters) in [1, 128], at most 16 dilated layers (lr_wavenet_supported, otherwise
 * LR_ESHAPE).  No float atomics anywhere: same bits from run to run.
 *   a_0[b, t] = table[ids[b, t]] (table [V, D], ids int32 [B, L], read in place; an id outside [0, V) is never dereferenced:
 *   a zero input row, gx exactly 0).  There is no sequence mask: pad positions take part like any other.
 *   layer j < n_layers:  a_{j+1}[t] = relu(bias_j + a_j[t - d_j] K_j[0] + a_j[t] K_j[1]), d_j = 2^(j mod n_per_block),
 *                        a_j[t - d_j] = 0 for t < d_j (Keras padding="causal"; tap 0 is the earlier step); K_j [2, C_j, F],
 *                        C_0 = D, C_j = F after that
 *   layer n_layers:      relu(bias + a K), K [1, F, F]
 *   pooled[b, f] = max_t of the last layer, arg[b, f] = the smallest t that attains it.  ReLU's derivative at 0 is 0.
 * Parameter layout (the contract; it is how layers/dense.py `DenseParams` lays out tensors added in this order): one f32
 * buffer holding, for j = 0 .. n_layers, K_j (row-major [taps, C_j, F]) then bias_j [F], every tensor starting on a 16-byte
 * boundary (its length rounded up to 4 floats; the gap is not read).  lr_wavenet_params_bytes is the buffer's length.
 * `gparams` has the same layout; the backward writes every element of it (the gaps as 0).
 *   forward   writes every element of acts (lr_wavenet_fwd_acts_bytes: [n_layers + 1, B, L, F] row-major, slab j = the post-ReLU
 *             output of layer j), pooled [B, F] and arg int32 [B, F].
 *   backward  from gpooled [B, F]: writes every element of gx [B, L, D] and gparams.  The ReLU pattern is acts > 0.  Weight and
 *             bias gradients are summed over B L as per-chunk partials in `ws` (lr_wavenet_bwd_ws_bytes bytes, contents
 *             arbitrary on entry) added in chunk order.
 * ---------------------------------------------------------------------------------- */
int lr_wavenet_supported(int L, int D, int F, int n_blocks, int n_per_block);
size_t lr_wavenet_params_bytes(int D, int F, int n_blocks, int n_per_block);
size_t lr_wavenet_fwd_acts_bytes(int64_t B, int L, int F, int n_blocks, int n_per_block);
size_t lr_wavenet_bwd_ws_bytes(int64_t B, int L, int D, int F, int n_blocks, int n_per_block);
int lr_wavenet_fwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int D, int F, int n_blocks,
                       int n_per_block, const float* params, float* acts, size_t acts_bytes, float* pooled, int32_t* arg,
                       lr_stream_t stream);
int lr_wavenet_bwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int D, int F, int n_blocks,
                       int n_per_block, const float* params, const float* acts, const float* gpooled, const int32_t* arg,
                       float* gx, float* gparams, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Caser — the user side of libreco/algorithms/caser.py:177-221 up to the Dense layer, in one forward launch, f32 on the VALU.
 * L (window) in [1, 64], K (table width) in [1, 128], nh and nv (horizontal and vertical filters) in [1, 64]
 * (lr_caser_supported, otherwise LR_ESHAPE).  No float atomics anywhere: same bits from run to run.
 *   x[b, t] = table[ids[b, t]] (table [V, K], ids int32 [B, L], read in place; an id outside [0, V) is never dereferenced: a
 *   zero input row, gx exactly 0).  There is no sequence mask: pad positions take part like any other.
 *   horizontal, i = 1 .. L:  z_i[b, t, f] = relu(bh_i[f] + sum_{tau < i, c < K} x[b, t + tau, c] Wh_i[tau, c, f]), t = 0 .. L - i
 *                            (one fmaf chain from the bias, tau ascending, c ascending: positions with equal receptive fields
 *                            give equal bits); h_i[b, f] = max_t z_i, arg = the smallest t that attains it
 *   vertical:                v[b, c, g] = relu(bv[g] + sum_t x[b, t, c] Wv[t, g]) (one chain, t ascending)
 *   feat[b] = concat(h_1, .., h_L, v flattened [c][g]), width L nh + K nv; arg int32 [B, L nh] in the order of feat.  A sample's
 *   row has the same bits whatever batch it is part of and whether or not arg is written.  ReLU's derivative at 0 is 0: a
 *   filter whose every position is <= 0 has feat == 0, arg == 0 and passes no gradient.
 * Parameter layout (the contract; it is how layers/dense.py `DenseParams` lays out tensors added in this order): one f32
 * buffer holding, for i = 1 .. L, Wh_i (row-major [i, K, nh]) then bh_i [nh], then Wv (row-major [1, L, nv]) and bv [nv],
 * every tensor starting on a 16-byte boundary (its length rounded up to 4 floats; the gap is not read).
 * lr_caser_params_bytes is the buffer's length.  `gparams` has the same layout; the backward writes every element of it (the
 * gaps as 0).
 *   forward   writes every element of feat [B, L nh + K nv] and, unless `arg` is NULL (inference), of arg.
 *   backward  from gfeat [B, L nh + K nv], with feat and arg as the forward left them: writes every element of gx [B, L, K]
 *             (gather form per (b, t, c), a fixed order) and gparams.  The horizontal gradient flows only through position arg
 *             of a unit with feat > 0, the vertical one through units with feat > 0.  Parameter gradients are summed over
 *             slabs of the batch as partials in `ws` (lr_caser_bwd_ws_bytes bytes, contents arbitrary on entry; the number of
 *             slabs is capped, so the workspace does not grow with B beyond that) added in slab order.
 * ---------------------------------------------------------------------------------- */
int lr_caser_supported(int L, int K, int nh, int nv);
size_t lr_caser_params_bytes(int L, int K, int nh, int nv);
size_t lr_caser_bwd_ws_bytes(int64_t B, int L, int K, int nh, int nv);
int lr_caser_fwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int K, int nh, int nv,
                     const float* params, float* feat, int32_t* arg, lr_stream_t stream);
int lr_caser_bwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int K, int nh, int nv,
                     const float* params, const float* feat, const int32_t* arg, const float* gfeat, float* gx,
                     float* gparams, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * AutoInt — the interaction stack of libreco/algorithms/autoint.py:146-168 (layers/attention.py:67-101, the Keras
 * MultiHeadAttention(use_bias=False) branch) and its Dense(1) read-out in one forward launch, f32 on the VALU.  T (fields), D
 * (embedding width) and H * head_dims[l] in [1, 64], H in [1, 8], 1 to 8 layers (lr_autoint_supported, otherwise LR_ESHAPE).
 * `head_dims` is a HOST array of n_layers ints, read during the call.  No float atomics anywhere: same bits from run to run.
 *   A_0 = x [B, T, D] (read in place).  Layer l = 1 .. n_layers, hd = head_dims[l - 1], M = H * hd:
 *     Q = A Wq, Kx = A Wk, V = A Wv (kernels [D, M], head h = columns [h hd, (h + 1) hd)); per head S = (Q_h / sqrt(hd)) Kx_h^T,
 *     P = softmax(S) over the last axis with the row maximum subtracted, O_h = P V_h; Y = concat_h(O_h) Wo (Wo [M, D]);
 *     A_l = A_{l-1} + Y if `residual`, else Y.  No mask, bias, activation or normalisation.
 *   logits[b] = flatten(A_n[b]) . w + c (w [T * D], c [1]).
 * Parameter layout (the contract; it is how layers/dense.py `DenseParams` lays out tensors added in this order): one f32
 * buffer holding, per layer, the query, key, value and attention_output kernels (row-major [D, M], [D, M], [D, M], [M, D]),
 * then dense/kernel [T * D] and dense/bias [1], every tensor starting on a 16-byte boundary (its length rounded up to 4
 * floats; the gap is not read).  lr_autoint_params_bytes is the buffer's length.  `gparams` has the same layout; the backward
 * writes every element of it (the gaps as 0).
 *   forward   writes every element of logits [B] and, unless `acts` is NULL, of acts (lr_autoint_fwd_acts_bytes: [n_layers, B,
 *             T, D] row-major, slab l - 1 = A_l).  acts == NULL is inference: nothing but the logits is written.  A sample's
 *             logit has the same bits whatever batch it is part of and whether or not acts is written.  `saved`
 *             (lr_autoint_fwd_saved_bytes, contents arbitrary on entry) is whatever else the backward wants: currently 0 bytes,
 *             the backward recomputes Q, Kx, V, P and O from acts, and `saved` may be NULL.
 *   backward  from glogits [B], with x, params and acts as the forward saw and left them: writes every element of gx [B, T, D]
 *             and gparams.  Parameter gradients are summed over the batch as per-workgroup partials in `ws`
 *             (lr_autoint_bwd_ws_bytes bytes, contents arbitrary on entry) added in workgroup order.
 * ---------------------------------------------------------------------------------- */
int lr_autoint_supported(int T, int D, int H, int n_layers, const int* head_dims);
size_t lr_autoint_params_bytes(int T, int D, int H, int n_layers, const int* head_dims);
size_t lr_autoint_fwd_acts_bytes(int64_t B, int T, int D, int n_layers);
size_t lr_autoint_fwd_saved_bytes(int64_t B, int T, int D, int H, int n_layers, const int* head_dims);
size_t lr_autoint_bwd_ws_bytes(int64_t B, int T, int D, int H, int n_layers, const int* head_dims);
int lr_autoint_fwd_f32(const float* x, int64_t B, int T, int D, int H, int n_layers, const int* head_dims, int residual,
                       const float* params, float* acts, size_t acts_bytes, void* saved, size_t saved_bytes, float* logits,
                       lr_stream_t stream);
int lr_autoint_bwd_f32(const float* x, int64_t B, int T, int D, int H, int n_layers, const int* head_dims, int residual,
                       const float* params, const float* acts, const void* saved, const float* glogits, float* gx,
                       float* gparams, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Sequence attention — the scaled-dot-product core of libreco/layers/attention.py:5-25 (`tf_attention`, the keras Attention
 * pooling) and :67-126 (the Keras MultiHeadAttention branch) with the mask of libreco/algorithms/transformer.py:281-328, on
 * already projected rows: one launch forward, one backward, f32 on the VALU.  Tq, Tk in [1, 64], hd in [1, 128], H in [1, 8],
 * H * hd <= 256 (lr_seq_attn_supported, otherwise LR_ESHAPE).  No float atomics: same bits from run to run, and a sample's
 * output and gradients have the same bits at B = 1 and inside any batch.
 *   q [B, Tq, M], k [B, Tk, M], v [B, Tk, M] contiguous, M = H * hd, head h = columns [h hd, (h + 1) hd).  Per head
 *     S = (q_h * scale) k_h^T (`scale` as given: 1 / sqrt(hd) for multi-head attention, 1 for tf_attention);
 *     allowed(b, i, j) = key_ok(b, j) || (causal_or && j <= i); S[i, j] += -1e9f where not allowed — an f32 addition, as keras
 *     `_masked_softmax` / `_apply_scores` do it, not -inf: a row with nothing allowed is the softmax of the rounded values
 *     (uniform for |S| < 32) and its gradient still reaches q and k;
 *     P = softmax(S) over j with the row maximum subtracted; out [B, Tq, M]: O_h = P v_h.
 *   key_ok(b, j): `key_ok` uint8 [B, Tk] (any pattern, non-zero = valid), or `lens` int32 [B] (j < lens[b]), or both NULL (every
 *     key valid); both given is LR_EINVAL.  causal_or needs Tq == Tk, otherwise LR_EINVAL (transformer.py:323-328 ORs the
 *     sequence mask with the causal one).
 *   `v` may be the pointer `k` (the keys are the values: the pooling form); the forward then reads the rows once where a
 *     head's columns fit one pass.  gk and gv are always distinct buffers (LR_EINVAL otherwise): the caller adds them.
 *   forward   writes every element of out.  `saved` (lr_seq_attn_saved_bytes, contents arbitrary on entry) takes every row's
 *             maximum and sum of exponentials [B, H, Tq, 2]; NULL is inference: nothing but out is written.
 *   backward  from gout [B, Tq, M], with q, k, v and the masks as the forward saw them and `saved` as it left it: recomputes S
 *             and P, writes every element of gq [B, Tq, M], gk and gv [B, Tk, M].  No workspace.
 *   B = 0 writes nothing and returns LR_OK.
 *   lr_seq_attn_plan_params   the launch plan of a forward (bwd = 0) or backward (bwd != 0) call of this shape, as the launch
 *             itself derives it; `aligned`: whether every pointer of the call is on a 16-byte boundary.  Host only, launches
 *             nothing; for tests that assert the branch they run.  LR_ESHAPE for an unsupported shape, LR_EINVAL for B < 1 or
 *             a null out8.  out8 = {
 *               TB         units (sample, head) per workgroup, 1 .. 64; the grid is ceil(B H / TB) workgroups,
 *               nch        column chunks per head (hd <= nch CW),
 *               CW         columns per chunk (a multiple of 4 where nch > 1; the last chunk holds hd - (nch - 1) CW),
 *               CS         LDS stride of a chunk row in floats, 4 (ceil(CW / 4) | 1),
 *               ST         LDS stride of a score row in floats, Tk | 1,
 *               G          lanes per softmax row, 1, 2, 4 or 8 (from Tk alone),
 *               vec        1: rows move 16 bytes at a time (hd % 4 == 0 and aligned), 0: float by float,
 *               lds_bytes  dynamic LDS of a workgroup, at most 65536 }
 * ---------------------------------------------------------------------------------- */
int lr_seq_attn_supported(int Tq, int Tk, int H, int hd);
size_t lr_seq_attn_saved_bytes(int64_t B, int Tq, int Tk, int H, int hd);
int lr_seq_attn_plan_params(int64_t B, int Tq, int Tk, int H, int hd, int bwd, int aligned, int32_t* out8);
int lr_seq_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t B, int Tq, int Tk, int H, int hd, float scale,
                        const uint8_t* key_ok, const int32_t* lens, int causal_or, float* out, void* saved,
                        size_t saved_bytes, lr_stream_t stream);
int lr_seq_attn_bwd_f32(const float* q, const float* k, const float* v, int64_t B, int Tq, int Tk, int H, int hd, float scale,
                        const uint8_t* key_ok, const int32_t* lens, int causal_or, const void* saved, const float* gout,
                        float* gq, float* gk, float* gv, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Skip-gram word2vec in windows: the training of Item2Vec and DeepWalk, which the reference leaves to
 * gensim.Word2Vec on CPU threads (libreco/bases/gensim_base.py, algorithms/item2vec.py, algorithms/deepwalk.py).  The word
 * index is the item's inner id.  Every random choice is H(seed, stream, a, b) = mix64(mix64(mix64(seed + G stream) + G (a + 1))
 * + G (b + 1)), G = 0x9e3779b97f4a7c15, mix64 the splitmix64 finaliser: integers are bit-exact against tests/w2v_oracle.py.
 * Rows are D = 1 .. 256 floats (lr_w2v_supported, otherwise LR_ESHAPE).  An id outside its table takes no part.  No float
 * atomics: same bits from run to run.
 *   walks        walk w starts at starts[w] and takes up to walk_length - 1 steps over the successor CSR (succ_ptr [n_items + 1],
 *                succ_idx [n_edges], duplicates kept): successor number (hi32(H(seed, 1, pass, w walk_length + step)) * degree)
 *                >> 32.  A node without successors ends the walk.  Writes walks [n_walks, walk_length] (-1 padded) and lens.
 *   keep         keep[i] = hi32(H(seed, 2, epoch, i)) < keep_thr[tokens[i]] (keep_thr [n_items]: the host's
 *                floor(2^32 * keep probability), 0 for a word that never occurs).
 *   pairs        over the compacted corpus (ctok the kept tokens, craw their raw positions, csent their sentence, cptr
 *                [n_sent + 1] the compacted sentence starts): position i has reach r = window - H(seed, 3, epoch, craw[i]) % window
 *                and emits (input ctok[j], predicted ctok[i], centre craw[i]) for every j != i in [i - r, i + r] inside
 *                the sentence, in ascending (i, j).  `count` writes the number per position; `emit` takes their exclusive
 *                scan `offs` and writes at most n_pairs pairs.
 *   targets      per pair p, LR_W2V_NEGATIVES + 1 slots and then the Huffman path of the predicted word (hs_ptr [n_items + 1],
 *                hs_nodes / hs_codes [hs_len]; hs_ptr NULL: none).  offs == NULL counts (lens[p]); otherwise offs [W + 1] is
 *                the exclusive scan of lens and rows / labels / slot_in [n_slots] are filled: the predicted word (label 1),
 *                the draws k = 0 .. 4: the first word whose cum[] exceeds hi32(H(seed, 4, epoch, (pair_base + p) * 5 + k))
 *                (cum [n_items]: the host's cumulative count^0.75 table scaled to 2^32; label 0; row -1 when the draw is the
 *                predicted word), then (node row, 1 - code) along the path.  slot_in repeats the pair's input id per slot.
 *   score        one row group per pair of a window: f = syn0[in] . syn1[row] per target, g = (label - 1 / (1 + expf(-f))) *
 *                alpha, 0 when |f| >= 6, the row is outside [0, V1) or the input id is outside [0, n_items); alpha =
 *                max(1e-4, 0.025 - (0.025 - 1e-4) * (pos0 + centre[p]) * inv_total).  Writes g at every slot of the window's
 *                pairs, stash [W, D] (row p = sum of g * syn1[row]) and, unless NULL, loss [W] (the sum of -log sigmoid(+-f)
 *                over the pair's live targets).  offs holds W + 1 entries that index rows / labels / g (n_slots long).
 *   out_update   the ordered update of the touched rows of `table` (runs of lr_segments_build over n positions).  With
 *                slot_in: position q adds g[q] * other[slot_in[q]] (the output table; other = syn0, other_rows = n_items; g
 *                and slot_in point at the window's first slot).  With g and slot_in NULL: position q adds other[q] (the
 *                input table; other = the stash, other_rows >= n).  Ascending position within a row.
 * ---------------------------------------------------------------------------------- */
#define LR_W2V_NEGATIVES 5
int lr_w2v_supported(int D);
int lr_w2v_walks_i32(const int32_t* starts, int64_t n_walks, int walk_length, const int64_t* succ_ptr,
                     const int32_t* succ_idx, int64_t n_items, int64_t n_edges, uint64_t seed, int64_t pass,
                     int32_t* walks, int32_t* lens, lr_stream_t stream);
int lr_w2v_keep_u8(const int32_t* tokens, int64_t n, const int64_t* keep_thr, int64_t n_items, uint64_t seed,
                   int64_t epoch, uint8_t* keep, lr_stream_t stream);
int lr_w2v_pairs_count_i32(const int32_t* craw, const int32_t* csent, const int64_t* cptr, int64_t nc, int64_t n_sent,
                           int window, uint64_t seed, int64_t epoch, int32_t* counts, lr_stream_t stream);
int lr_w2v_pairs_emit_i32(const int32_t* ctok, const int32_t* craw, const int32_t* csent, const int64_t* cptr, int64_t nc,
                          int64_t n_sent, int window, uint64_t seed, int64_t epoch, const int64_t* offs, int64_t n_pairs,
                          int32_t* in_ids, int32_t* pred, int32_t* centre, lr_stream_t stream);
int lr_w2v_targets_i32(const int32_t* in_ids, const int32_t* pred, int64_t W, int64_t pair_base, int64_t n_items,
                       const int64_t* cum, const int32_t* hs_ptr, const int32_t* hs_nodes, const int32_t* hs_codes,
                       int64_t hs_len, uint64_t seed, int64_t epoch, const int64_t* offs, int32_t* lens, int64_t n_slots,
                       int32_t* rows, int32_t* labels, int32_t* slot_in, lr_stream_t stream);
int lr_w2v_score_f32(const float* syn0, int64_t n_items, const float* syn1, int64_t V1, int D, const int32_t* in_ids,
                     const int32_t* centre, int64_t W, const int64_t* offs, const int32_t* rows, const int32_t* labels,
                     int64_t n_slots, double pos0, double inv_total, float* g, float* stash, float* loss,
                     lr_stream_t stream);
int lr_w2v_out_update_f32(float* table, int64_t V, int D, const int32_t* seg_pos, const int32_t* seg_rows,
                          const int32_t* seg_start, const int32_t* n_seg, int64_t n, const float* g, const int32_t* slot_in,
                          const float* other, int64_t other_rows, lr_stream_t stream);

/* ------------------------------------------------------------------------------------
 * GraphSage: the neighbour sampling and the tower of libreco/algorithms/graphsage.py (sampling/random_walks.py,
 * sampling/negatives.py, torch_modules/graphsage_module.py).  Every random choice is H(seed, stream, a, b) of the word2vec block
 * above; an index below len is (hi32(H) * len) >> 32; integers are bit-exact against tests/sage_oracle.py.  The graph is two CSRs
 * with int64 pointers and int32 indices, duplicates kept: item_ptr / item_idx the consumers of an item, user_ptr / user_idx the
 * items of a user.  One walk from an item is a uniform consumer (half 0) and then a uniform item of that consumer (half 1); an
 * item nobody consumed, or an id outside the graph, walks to itself.  No float atomics: same bits from run to run.
 *   neighbors    out [n_nodes, num_neighbors] (1 .. 10).  Slot j of node i draws H(seed, 16, step * 8 + level, ((i * 16 + j) * 16 +
 *                attempt) * 2 + half): attempt 0; if that is the node itself or one of its slots < j, attempts 1 .. 5 until neither
 *                holds; then attempts 6 .. 10 until it is not the node itself; then attempt 11 stands.
 *   pairs        walk w of start i (num_walks each, walk_len steps) draws H(seed, 17, step, (((i * num_walks + w) * walk_len) + s)
 *                * 2 + half) and emits (cur, next) where next != cur, or with focus_start (start, next) where next != start; walk 0
 *                of a start all of whose consumers hold one item emits (start, start) first.  offs == NULL counts per (start,
 *                walk) into counts; otherwise offs is their exclusive scan and at most n_pairs pairs are written, in ascending
 *                (start, walk, step).
 *   starts       out[i] = (hi32(H(seed, 18, step, i)) * n_items) >> 32, or with cum [n_items] (a cumulative table scaled to 2^32)
 *                the first item whose cum[] exceeds hi32(H).
 *   negatives    out [n, num_neg]: slot q = i * num_neg + k draws H(seed, 19, step, q * 16 + attempt).  mode 0 (random): uniform,
 *                redrawn up to 10 times while it equals items_pos[i] or items[i] (items may be NULL); mode 1 (popular): from cum,
 *                redrawn once on that condition; mode 2 (out-batch): uniform, redrawn up to 10 times while in_batch[draw] != 0
 *                (in_batch [n_items]).  The last draw stands.
 *   dropout      keep [n_nodes, K]: hi32(H(seed, 20, step, (((node * 128 + column) * 2 + role) * 4 + level) * 4 + layer)) >=
 *                floor(p * 2^32); role 0 the node itself, 1 the node as a neighbour; node counts inside its level of the batch.
 *   fwd / bwd    B trees of levels 0 .. num_layers with num_neighbors^k nodes; rows / scale [B N, T] hold every node's T slots
 *                (row of table [V, K], scale; scale NULL: all 1) level-major: level k starts at node B (1 + n + .. + n^(k-1)) and
 *                tree b's nodes i n^k-wise at b n^k + i; node i of level k has the children i n .. i n + n - 1 of level k + 1.
 *                params (lr_sage_params_bytes): proj W^T [T K, K], proj b [K], then per layer W^T [2 K, K], b [K].  h_0 =
 *                proj(concat(scale * row)); layer l: h[v] = act(W [drop(h[v]); mean_children drop(h[child])] + b) over levels 0 ..
 *                L - l - 1, ReLU on all but the last layer; repr [B, K] = level 0 after the last layer.  Every element is one fmaf
 *                chain (bias, inputs ascending).  train == 0 or dropout == 0 draws nothing.  bwd recomputes the activations from
 *                the same arguments and writes grow [B N, T, K] (the slot-row gradients times the slot's scale, exactly 0 for a row
 *                outside [0, V)), gparams (the layout of params) and, unless NULL, relu_out: per ReLU layer l a block
 *                [B, nodes with an output in layer l, K] of 0 / 1.  ws holds lr_sage_bwd_ws_bytes: lr_sage_bwd_slabs slabs of
 *                partials, added in slab order.  Shapes: lr_sage_supported (K 1 .. 64, T 1 .. 16, num_layers 0 .. 3,
 *                num_neighbors 1 .. 10 with num_neighbors^num_layers <= 100), otherwise LR_ESHAPE.
 * ---------------------------------------------------------------------------------- */
int lr_sage_supported(int K, int T, int num_layers, int num_neighbors);
size_t lr_sage_params_bytes(int K, int T, int num_layers);
int lr_sage_bwd_slabs(int64_t B, int K, int T, int num_layers, int num_neighbors);
size_t lr_sage_bwd_ws_bytes(int64_t B, int K, int T, int num_layers, int num_neighbors);
int lr_sage_neighbors_i32(const int32_t* nodes, int64_t n_nodes, int num_neighbors, const int64_t* item_ptr,
                          const int32_t* item_idx, int64_t n_items, int64_t n_item_idx, const int64_t* user_ptr,
                          const int32_t* user_idx, int64_t n_users, int64_t n_user_idx, uint64_t seed, int64_t step, int level,
                          int32_t* out, lr_stream_t stream);
int lr_sage_pairs_i32(const int32_t* starts, int64_t n_starts, int num_walks, int walk_len, int focus_start,
                      const int64_t* item_ptr, const int32_t* item_idx, int64_t n_items, int64_t n_item_idx,
                      const int64_t* user_ptr, const int32_t* user_idx, int64_t n_users, int64_t n_user_idx, uint64_t seed,
                      int64_t step, int32_t* counts, const int64_t* offs, int64_t n_pairs, int32_t* items, int32_t* items_pos,
                      lr_stream_t stream);
int lr_sage_starts_i32(int64_t n, int64_t n_items, const int64_t* cum, uint64_t seed, int64_t step, int32_t* out,
                       lr_stream_t stream);
int lr_sage_negatives_i32(const int32_t* items, const int32_t* items_pos, int64_t n, int num_neg, int64_t n_items, int mode,
                          const int64_t* cum, const uint8_t* in_batch, uint64_t seed, int64_t step, int32_t* out,
                          lr_stream_t stream);
int lr_sage_dropout_u8(int64_t n_nodes, int K, double p, uint64_t seed, int64_t step, int layer, int level, int role,
                       uint8_t* keep, lr_stream_t stream);
int lr_sage_fwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, int64_t B, int K, int T,
                    int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed, int64_t step,
                    int train, float* repr, lr_stream_t stream);
int lr_sage_bwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, int64_t B, int K, int T,
                    int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed, int64_t step,
                    const float* grepr, float* grow, float* gparams, uint8_t* relu_out, void* ws, size_t ws_bytes,
                    lr_stream_t stream);

/* ----------------------------------------------------------------------------------
 * PinSage: the importance-walk neighbour sampling and the tower of libreco/algorithms/pinsage.py
 * (sampling/random_walks.py, graph/neighbor_walk.py, torch_modules/pinsage_module.py).  The graph, H, the one-walk rule, the
 * trees, the slots and the level-major layout are those of the GraphSage block above; integers are bit-exact against
 * tests/pinsage_oracle.py.  No float atomics: same bits from run to run.
 *   neighbors    ids / counts [n_nodes, num_neighbors] (1 .. 10; num_walks * walk_len <= 64, otherwise LR_ESHAPE).  Node i of
 *                the level runs num_walks walks of at most walk_len steps; step s of walk w draws H(seed, 21, step * 8 + level,
 *                (i * 64 + w * walk_len + s) * 4 + kind), kind 0 the consumer, 1 the item, 2 the continue draw.  Step 0 is always
 *                taken; before a later step the walk continues iff hi32(H) >= floor(termination_prob * 2^32), compared in 64
 *                bits (>= 1: never, 0: always).  The visited items in ascending (walk, step) lose every occurrence of the node
 *                itself, unless nothing else was visited, in which case one stays; then, where tree_exclude != NULL,
 *                tree_exclude[b] >= 0 and the node equals tree_target[b] for its tree b = i / num_neighbors^level, every
 *                occurrence of tree_exclude[b] by the same rule (tree_target / tree_exclude [n_trees], n_nodes == n_trees *
 *                num_neighbors^level).  The num_neighbors most visited items follow in descending count, ties by first visit,
 *                with their counts; unused slots hold id -1 and count 0.  A node all of whose consumers hold one item, an item
 *                nobody consumed and an id outside the graph give themselves with count 1.
 *   fwd / bwd    the arguments of lr_sage_fwd_f32 / lr_sage_bwd_f32 and weights [B (N - 1)]: the importance weight of every
 *                node of the levels 1 .. num_layers, at the node's position in the level-major arrays minus B (may be NULL
 *                when num_layers == 0).  params (lr_pinsage_params_bytes): proj W^T [T K, K], proj b [K]; per layer Q^T [K, K],
 *                bq [K], W^T [2 K, K], bw [K]; the head G1^T [K, K], b1 [K], G2^T [K, K].  Layer l over the levels k < L - l:
 *                nb = drop(relu(Q h[child] + bq)) (the flags of lr_sage_dropout_u8 with role 1, layer l, level k + 1), agg =
 *                sum_j w_j nb_j in child order with a child of weight 0 skipped, z = relu(W [h[v]; agg] + bw), h'[v] = z / |z|
 *                with a norm of exactly 0 replaced by 1; repr [B, K] = G2 relu(G1 h[0] + b1).  Every element is one fma chain
 *                (bias, inputs ascending) accumulated in f64 and rounded to f32 once, |z|^2 likewise over the columns: a target
 *                has the same bits alone and in any batch.  bwd recomputes the activations and writes grow [B N, T, K] (times the slot's scale, exactly 0
 *                for a row outside [0, V)), gparams (the layout of params) and, unless NULL, relu_out: per layer l a block
 *                [B, n_l - 1, K] of the q flags (the nodes 1 .. n_l - 1 of a tree, n_l the nodes of the levels 0 .. L - l) and a
 *                block [B, m_l, K] of the w flags (m_l the nodes of the levels 0 .. L - l - 1), then the head's flags [B, K].
 *                ws holds lr_pinsage_bwd_ws_bytes: lr_pinsage_bwd_slabs slabs of partials, added in slab order in f64.  Shapes:
 *                lr_pinsage_supported (K 1 .. 64, T 1 .. 16, num_layers 0 .. 3, num_neighbors 1 .. 10 with
 *                num_neighbors^num_layers <= 100: one tree's backward image then fits in 96 KB of LDS), otherwise LR_ESHAPE.
 * ---------------------------------------------------------------------------------- */
int lr_pinsage_supported(int K, int T, int num_layers, int num_neighbors);
size_t lr_pinsage_params_bytes(int K, int T, int num_layers);
int lr_pinsage_bwd_slabs(int64_t B, int K, int T, int num_layers, int num_neighbors);
size_t lr_pinsage_bwd_ws_bytes(int64_t B, int K, int T, int num_layers, int num_neighbors);
int lr_pinsage_neighbors_i32(const int32_t* nodes, int64_t n_nodes, int num_neighbors, int num_walks, int walk_len,
                             double termination_prob, const int32_t* tree_target, const int32_t* tree_exclude, int64_t n_trees,
                             const int64_t* item_ptr, const int32_t* item_idx, int64_t n_items, int64_t n_item_idx,
                             const int64_t* user_ptr, const int32_t* user_idx, int64_t n_users, int64_t n_user_idx, uint64_t seed,
                             int64_t step, int level, int32_t* ids, int32_t* counts, lr_stream_t stream);
int lr_pinsage_fwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, const float* weights, int64_t B,
                       int K, int T, int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed,
                       int64_t step, int train, float* repr, lr_stream_t stream);
int lr_pinsage_bwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, const float* weights, int64_t B,
                       int K, int T, int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed,
                       int64_t step, const float* grepr, float* grow, float* gparams, uint8_t* relu_out, void* ws,
                       size_t ws_bytes, lr_stream_t stream);

/* ---- FTRL-proximal (the wide side of Wide & Deep; csrc/ftrl.hip) -------------------------------------------------------
 * TF1's ApplyFtrl / SparseApplyFtrl with lr_power = -0.5 and no l2 shrinkage, per element with gradient g:
 *   new_accum = accum + g*g;  linear += g - (sqrt(new_accum) - sqrt(accum)) / lr * var;
 *   var = |linear| > l1 ? (sign(linear)*l1 - linear) / (sqrt(new_accum)/lr + 2*l2) : 0;  accum = new_accum.
 * lr > 0, l1 >= 0, l2 >= 0.  TF's slots start at accum = 0.1, linear = 0.
 *
 * lr_ftrl_rows_f32: `var`, `accum`, `linear` are scalar-row tables of V floats; `grad` holds one float per position of the
 *   segments (lr_segments_build; n positions, n_seg read on the device).  The gradient of a distinct row is the sum over its
 *   run, added in a fixed order that does not depend on the grid (no float atomics: two calls give the same bits); the row's
 *   three values are read and written once, rows outside the stream are not written.  Runs of more than 32 positions are cut
 *   into 256-position chunks summed by one wave each when a workspace of lr_ftrl_rows_ws_bytes(n) bytes is passed (`ws`;
 *   NULL: every run is walked by one lane; contents arbitrary on entry).  A non-NULL `ws` with ws_bytes below that size:
 *   LR_EWORKSPACE.  n == 0: nothing is launched.
 * lr_ftrl_dense_f32: the same update on every element of a flat range of n floats with g = grad[i] + l2_grad_coef * var[i]. */
size_t lr_ftrl_rows_ws_bytes(int64_t n_max);
int lr_ftrl_rows_f32(float* var, float* accum, float* linear, int64_t V, const float* grad, const int32_t* seg_pos,
                     const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg, int64_t n, double lr, double l1,
                     double l2, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_ftrl_dense_f32(float* var, float* accum, float* linear, int64_t n, const float* grad, double l2_grad_coef, double lr,
                      double l1, double l2, lr_stream_t stream);

/* ---- NCF (csrc/ncf.hip): the two-field front and back of a step, and the inference tower in one launch -------------------
 * u = table[user row], i = table[item row] (global rows of ONE [V, K] table; an id outside [0, V) reads as a zero row, as in
 * lr_embed_gather_f32).  K % 4 == 0, 4 <= K <= 128; table, x, gmf, G, wg and every W[l] 16-byte aligned (LR_EINVAL otherwise).
 *
 * lr_ncf_pair_fwd_f32: idx [B, 2] = (user row, item row) per sample -> x [B, 2K] = [u | i] and gmf [B, K] = u * i, one f32
 *   multiply per element (bit-exact against numpy f32).
 * lr_ncf_pair_bwd_f32: adds the GMF path to the MLP's row gradient in place:
 *   G[b, k] = fmaf(gl[b] * wg[k], x[b, K + k], G[b, k]),  G[b, K + k] = fmaf(gl[b] * wg[k], x[b, k], G[b, K + k]);
 *   afterwards G viewed [2B, K] is the per-position gradient in the order of idx viewed [2B].
 * lr_ncf_score_f32: out[p] = sum_k u_k i_k wg[k] + h_L . wd + c for the n pairs (users[p], items[p]), where x = [u | i],
 *   h_l = relu(h_{l-1} W[l] + b[l]) * s[l] + t[l] for l < L and h_L = h_{L-1} W[L] + b[L] (W[l] row-major [d_in, widths[l]];
 *   `W`, `b`, `s`, `t`: host arrays of n_layers device pointers; `s` / `t` or single entries of both may be NULL: identity;
 *   the entries of the last layer are ignored).  The caller folds an input BatchNorm into (W[0], b[0]) and passes each hidden
 *   BatchNorm's inference affine as (s, t).  One launch: workgroups of 256 threads take 64 pairs per pass and stay resident
 *   over the tiles, the weights are staged into LDS once per workgroup, products run on v_mfma_f32_32x32x2_f32.  Every
 *   output is one k-ordered f32 fma chain per product; no atomics: two calls give the same bits.
 *   Envelope (lr_ncf_score_supported, the single source of truth): K as above, 1 <= n_layers <= 4, widths multiples of 16 in
 *   [16, 256], and weights ([d_in][widths[l] rounded up to 32]) + two [width][68] activation tiles within 160 KB of LDS.
 *   Outside it: LR_ESHAPE, nothing is written. */
int lr_ncf_pair_fwd_f32(const float* table, int64_t V, int K, const int32_t* idx, int64_t B, float* x, float* gmf,
                        lr_stream_t stream);
int lr_ncf_pair_bwd_f32(const float* x, const float* gl, const float* wg, float* G, int64_t B, int K, lr_stream_t stream);
int lr_ncf_score_supported(int K, int n_layers, const int* widths);
int lr_ncf_score_f32(const float* table, int64_t V, int K, const int32_t* users, const int32_t* items, int64_t n, int n_layers,
                     const int* widths, const float* const* W, const float* const* b, const float* const* s,
                     const float* const* t, const float* wg, const float* wd, float c, float* out, lr_stream_t stream);

/* ---- IVF-Flat index (csrc/ivf.hip): inner-product inverted file over f32 rows ---------------------------------------------
 * Rows, centroids and queries are [*, D] f32, D % 4 == 0, 4 <= D <= 256, 16-byte aligned; nlist <= 65536; fewer than 2^31 rows
 * (LR_ESHAPE otherwise, nothing written).  No floating-point atomics anywhere: two calls give the same bits.
 *
 * lr_ivf_assign_f32: list_of[r] = the centroid of largest inner product with row r, ties to the lowest list id (a row whose
 *   scores are all NaN goes to list 0); best_score (nullable) [n] = that inner product.
 * lr_ivf_build_lists: stable counting sort of list_of (values in [0, nlist)) -> list_ptr int64 [nlist + 1] (CSR of the lists)
 *   and list_ids int32 [n] (row ids, ascending within a list).  Integer work only.  The rows in list order are
 *   lr_embed_gather_f32(rows, list_ids).  Workspace: lr_ivf_build_ws_bytes, 256-byte aligned.
 * lr_ivf_centroids_f32: centroids[l] = (sum of rows[list_ids[p]] over list l, p ascending, in a fixed order) / f32(count), one
 *   division per element; an empty list keeps its row of `centroids`.  `n` = list_ptr[nlist] entries, ids below n_rows.
 *   Workspace: lr_ivf_centroids_ws_bytes, contents arbitrary.
 * lr_ivf_search_f32: per query the `nprobe` lists of largest (inner product with the centroid desc, list id asc), found by
 *   lr_score_topk_f32; among the rows of those lists (list_rows [N, D] = the catalogue in list order, list_ids their global ids)
 *   the k largest by (score desc, global id asc), consumed ids of flagged queries dropped.  consumed_ptr / consumed_idx /
 *   filter_flag and out_scores / out_ids [B, k] exactly as in lr_score_topk_f32 (id -1 / score -inf beyond the surviving
 *   candidates).  Scores are f32 fma chains; no B x N block exists.  Envelope (lr_ivf_supported, the single source of truth):
 *   D as above, 1 <= k <= 1024, 1 <= nprobe <= nlist <= min(N, 65536), nprobe within lr_score_topk_f32's k (4096), N < 2^31 and
 *   at most 4 GiB of partial keys.  Workspace: lr_ivf_search_ws_bytes (0 outside the envelope), 256-byte aligned. */
int lr_ivf_supported(int64_t B, int64_t N, int D, int k, int nprobe, int nlist);
size_t lr_ivf_search_ws_bytes(int64_t B, int64_t N, int D, int k, int nprobe, int nlist);
size_t lr_ivf_build_ws_bytes(int64_t n, int nlist);
size_t lr_ivf_centroids_ws_bytes(int64_t n, int D);
int lr_ivf_assign_f32(const float* rows, int64_t n, const float* centroids, int nlist, int D, int32_t* list_of,
                      float* best_score /* [n] or NULL */, lr_stream_t stream);
int lr_ivf_build_lists(const int32_t* list_of, int64_t n, int nlist, int64_t* list_ptr, int32_t* list_ids, void* ws,
                       size_t ws_bytes, lr_stream_t stream);
int lr_ivf_centroids_f32(const float* rows, int64_t n_rows, int D, const int64_t* list_ptr, const int32_t* list_ids, int64_t n,
                         int nlist, float* centroids /* [nlist, D], in place */, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_ivf_search_f32(const float* queries, int64_t B, const float* centroids, int nlist, const int64_t* list_ptr,
                      const int32_t* list_ids, const float* list_rows, int64_t N, int D, const int64_t* consumed_ptr,
                      const int32_t* consumed_idx, const uint8_t* filter_flag, int k, int nprobe, float* out_scores,
                      int64_t* out_ids, void* ws, size_t ws_bytes, lr_stream_t stream);

/* ---- IVF-SQ8 index (csrc/ivf_sq8.hip): the lists of an IVF index as int8 codes + one f32 scale per row, exact re-rank -------
 * Training and lists are the IVF-Flat entry points above.  Code rows are `code_stride` bytes, D <= code_stride <= 256,
 * code_stride % 16 == 0, 16-byte aligned; D as above (LR_ESHAPE otherwise, nothing written).  No floating-point atomics.
 *
 * lr_ivf_sq8_encode_f32: for j < n, x = rows[list_ids[j]] (rows[j] when list_ids is NULL; an id outside [0, n_rows) reads as a
 *   zero row): a = max |x_d|, scales[j] = a / 127 (one correctly rounded f32 division), codes[j, d] = clamp(rint(x_d /
 *   scales[j]), -127, 127) (correctly rounded division, half to even); a == 0 gives scale 0 and codes 0; codes[j, D ..
 *   code_stride) = 0.  Finite input only.
 * lr_ivf_sq8_search_f32: lr_ivf_search_f32 with score_j = scales[j] * (sum_d q_d * float(codes[j, d])), the sum in f32 (fma
 *   chain per lane, then pair sums), the product one rounded f32 multiply; the kk largest by (score desc, global id asc) with the
 *   same consumed / flag / fill contract.  Envelope: that of lr_ivf_search_f32 with k = kk.  Workspace:
 *   lr_ivf_sq8_search_ws_bytes (0 outside the envelope), 256-byte aligned.
 * lr_ivf_sq8_supported: the envelope of search + re-rank for a caller's k and refine: 0 <= refine <= 64, 1 <= k <= 1024 and
 *   lr_ivf_sq8_search_f32's at kk = refine == 0 ? k : min(k * refine, 1024).
 * lr_ivf_rerank_f32: per query the candidates cand_ids[b, 0..kk) (global ids; entries outside [0, N), -1 among them, are
 *   skipped; ids distinct) are scored as f32 inner products with rows[id] and the k largest by (score desc, id asc) written,
 *   id -1 / score -inf beyond them.  1 <= k, kk <= 1024. */
int lr_ivf_sq8_supported(int64_t B, int64_t N, int D, int k, int nprobe, int nlist, int refine);
size_t lr_ivf_sq8_search_ws_bytes(int64_t B, int64_t N, int D, int kk, int nprobe, int nlist);
int lr_ivf_sq8_encode_f32(const float* rows, int64_t n_rows, int D, const int32_t* list_ids /* [n] or NULL: identity */, int64_t n,
                          int8_t* codes /* [n, code_stride] */, int code_stride, float* scales /* [n] */, lr_stream_t stream);
int lr_ivf_sq8_search_f32(const float* queries, int64_t B, const float* centroids, int nlist, const int64_t* list_ptr,
                          const int32_t* list_ids, const int8_t* codes, int code_stride, const float* scales, int64_t N, int D,
                          const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag, int kk, int nprobe,
                          float* out_scores /* [B, kk] */, int64_t* out_ids /* [B, kk] */, void* ws, size_t ws_bytes,
                          lr_stream_t stream);
int lr_ivf_rerank_f32(const float* queries, int64_t B, const float* rows, int64_t N, int D, const int64_t* cand_ids /* [B, kk] */,
                      int kk, int k, float* out_scores /* [B, k] */, int64_t* out_ids /* [B, k] */, lr_stream_t stream);

/* ---- Evaluation metrics (csrc/eval_metrics.hip) — replaces the sklearn / numpy / Python-set work of
 * libreco/evaluation/metrics.py (roc_gauc, precision_at_k, recall_at_k, average_precision_at_k, ndcg_at_k, coverage) and
 * libreco/evaluation/evaluate.py:62-193 (roc_auc_score, precision_recall_curve + auc, log_loss, balanced_accuracy_score,
 * r2_score, rmse, mae).  Fewer than 2^31 rows (LR_ESHAPE otherwise, nothing written).  No floating-point atomics: two calls give
 * the same bits.  Every output element is written by every call; workspaces may hold anything.
 *
 * lr_eval_keys_f32: key[i] = (group[i] << 32) | image(score[i]), group 0 when `group` is NULL (groups are >= 0).  image is the
 *   order-preserving unsigned 32-bit image of the float: -0.0 is +0.0 first, subnormals are not flushed.  bad[0] = the number of
 *   NaN scores.  Sorting the keys ascending (the caller's job, carrying the labels) orders rows by (group, score).
 * lr_eval_rank_stats: one segmented scan over tie runs (equal key) and groups (equal high word) of the SORTED keys; label != 0
 *   is a positive.  out_i64 = {num2, P, Nneg}: num2 = sum over runs of pos_run * (2 * neg_below + neg_run), neg_below counted
 *   within the run's group (with one group: ROC AUC = num2 / (2 P Nneg), exactly the tie-corrected rank statistic);
 *   out_f64 = {gauc, pr_auc}: gauc = (sum over groups with both classes of n_g * num2_g / (2 P_g N_g)) / n (metrics.py roc_gauc;
 *   a single-class group adds 0); pr_auc = the trapezoid area under sklearn's precision_recall_curve (thresholds = the distinct
 *   keys, the last point recall 0 / precision 1), which reads the rows as one sequence and means something for one group only.
 *   fp64 throughout, fixed summation order.  Workspace: lr_eval_rank_ws_bytes (0 outside the envelope), 256-byte aligned.
 * lr_eval_point_sums_f32: out_f64 = {sum (y - p)^2, sum |y - p|, sum y, sum (y - mean)^2, log-loss sum}, differences and sums in
 *   fp64; the log-loss term of a row is -log(clip(p)) for y != 0 and -log(clip(float32(1 - p))) otherwise, clip to
 *   [2^-23, 1 - 2^-23] (sklearn's log_loss on float32 input).  out_i64 = {TP, TN, P, N} for labels in {0, 1} and the class
 *   rint(p) (half to even: 0.5 is class 0).  Workspace: lr_eval_point_ws_bytes.
 * lr_eval_listwise: reco int32 [U, k] (-1 padded, distinct ids), truth_items ascending and distinct within a user's
 *   truth_ptr range, truth_len[u] >= 1 the divisor of recall, disc f64 [k] = 1 / log2(j + 2).  out f64 [4, U] = precision
 *   (hits / k), recall (hits / truth_len), AP (mean of cumhits_j / (j + 1) over hit positions, 0 without hits) and NDCG
 *   (sum hit_j disc_j / sum_{j < hits} disc_j, 0 without hits).  1 <= k <= 1024 (LR_ESHAPE otherwise).
 * lr_eval_coverage_i32: flags int32 [n_items] = 1 where an id of reco[0 .. n) in [0, n_items) occurs, else 0; count[0] = the
 *   number of set flags. */
size_t lr_eval_rank_ws_bytes(int64_t n);
size_t lr_eval_point_ws_bytes(int64_t n);
int lr_eval_keys_f32(const float* score, const int32_t* group /* [n] or NULL */, int64_t n, int64_t* key, int32_t* bad /* [1] */,
                     lr_stream_t stream);
int lr_eval_rank_stats(const int64_t* key_sorted, const uint8_t* label_sorted, int64_t n, int64_t* out_i64 /* [3] */,
                       double* out_f64 /* [2] */, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_eval_point_sums_f32(const float* pred, const float* label, int64_t n, double mean, double* out_f64 /* [5] */,
                           int64_t* out_i64 /* [4] */, void* ws, size_t ws_bytes, lr_stream_t stream);
int lr_eval_listwise(const int32_t* reco, const int64_t* truth_ptr, const int32_t* truth_items, const int32_t* truth_len,
                     const double* disc, int64_t U, int k, double* out /* [4, U] */, lr_stream_t stream);
int lr_eval_coverage_i32(const int32_t* reco, int64_t n, int64_t n_items, int32_t* flags /* [n_items] */,
                         int64_t* count /* [1] */, lr_stream_t stream);

/* Measurement probe (scripts/mfma_peak.py): iters x 8 back-to-back v_mfma_f32_32x32x2_f32 per wave on
 * 256 x waves_per_simd workgroups — the f32 MFMA rate the chip sustains at the clock it holds under that load. */
int lr_mfma_f32_probe(int iters, int waves_per_simd, float* out, lr_stream_t stream);
/* Test aid (tests/test_tail_fused_gpu.py): `grid` workgroups that each claim `lds_bytes` of LDS (160 KB: one per CU) and
 * idle for `usec` microseconds — takes residency away from whatever runs beside it on another stream. */
int lr_probe_occupy(int grid, size_t lds_bytes, int64_t usec, lr_stream_t stream);
/* Measurement aid (bench.py): out[2 s] = s_memtime (shader-clock ticks), out[2 s + 1] = s_memrealtime (constant rate) read by one
 * lane on the compute unit of slot s = (XCC id, shader engine, shader array, CU); `out` holds 2 * lr_clock_probe_slots() words
 * the caller zeroes once.  Only differences of the SAME slot between two calls mean anything (the counters of different CUs carry
 * different offsets): two calls around a timed region give the mean shader clock the part sustained over it. */
int lr_clock_probe_slots(void);
int lr_clock_probe(uint64_t* out, lr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LIBRECO_HIP_H_ */
