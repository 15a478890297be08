/*
 * include/emdr2_ops.h -- C ABI of the transformer-block kernels (libemdr2_hip.so): what the encoder / reader
 * forward + backward of the EMDR2 hot path are made of.
 *
 * The reference runs these through torch / cuBLAS / apex from Python; the entry points below are what a binding
 * next to megatron/model/transformer.py would call.  Each comment names the reference code it replaces.
 * Conventions as in emdr2_mips.h: device pointers, element strides, int status (0 ok), enqueue on `stream`.
 * Activations and weights are bf16 (round-to-nearest-even), accumulation and statistics fp32.
 */
#ifndef EMDR2_OPS_H
#define EMDR2_OPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/*
 * C[b1,b2][m,n] = epi( alpha * sum_k A[b1,b2][m,k] * B[b1,b2][n,k] ),  epi = (+bias[n]) -> (GELU) -> (dropout) -> (+residual[m,n])
 * Replaces F.linear (mpu/layers.py:255,353), baddbmm/bmm (transformer.py:309-312,371), bias+GELU
 * (transformer.py:103-104; exact erf), bias-dropout-add (transformer.py:397-413).
 * drop_p > 0 (unbatched, no split-K): element (m, n) is kept iff keep(seed, row m, column n) of csrc/rng.h (drop_p quantised to 2^-16);
 * survivors are scaled by 1/(1-p); emdr2_dropout() applies the same mask to the incoming gradient in the backward.
 * K % 32 == 0; lda, ldb and the A/B batch strides multiples of 8 elements; A, B 16-byte aligned.
 * pre_act (optional, bf16, indexed like C): value before GELU, kept for the backward.  gelu == 2 (needs pre_act): GELU as with 1, but
 * pre_act receives gelu'(value before GELU) instead -- the only thing the backward ever does with the pre-activation, computed here
 * from the fp32 value and next to the activation's own exponential (residual_mode 2 consumes it).
 * residual_mode 0: + residual (`residual` may be C itself: every element is read before it is written, by the same lane -- a data gradient
 * added onto a running sum in place).  1: the `residual` buffer holds a saved GELU pre-activation u and the result is MULTIPLIED by gelu'(u) --
 * the backward of bias-GELU fused into the GEMM that produces d(activation) (saves one 3 x [tokens, ffn] elementwise pass).
 * 2: the result is MULTIPLIED by residual[m, n] (a gelu' saved by gelu == 2: the same backward without the erf arithmetic).
 * split_k > 1: the reduction is cut into split_k slices accumulated with fp32 atomics into a PRE-ZEROED fp32 C (weight
 * gradients: few output tiles, very long K); no epilogue options in that mode.
 */
int emdr2_gemm_nt_bf16(const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, int M, int N, int K,
                       int batch1, int64_t sA1, int64_t sB1, int64_t sC1, int batch2, int64_t sA2, int64_t sB2, int64_t sC2,
                       float alpha, const float *bias, int gelu, void *pre_act, const void *residual, int residual_mode, int out_f32,
                       int split_k, float drop_p, uint32_t seed, void *stream);

/* Weight-gradient GEMM, "TN" form: C[i, j] (fp32) = sum_r A[r, i] * B[r, j], A [R, I] and B [R, J] row-major bf16 (dW = dy^T x without
 * transposing either operand through HBM: LDS transpose reads, see csrc/gemm_tn.hip).  Replaces the autograd weight gradient of F.linear
 * (mpu/layers.py:255,353).  R % 32 == 0, I, J, lda, ldb multiples of 8.  colsum_a (optional, fp32 [I]) accumulates the column sums
 * of A (the bias gradient).  split_k > 1 accumulates reduction slices with atomics into a PRE-ZEROED C. */
int emdr2_gemm_tn_bf16(const void *A, int64_t lda, const void *B, int64_t ldb, float *C, int64_t ldc, int I, int J, int R, int split_k,
                       float *colsum_a, void *stream);

/* ---- Ordered sums ("deterministic gradients"): the gradient entries that add across workgroups, with no float atomics -----------------------
 * Contract of every *_ordered entry: the total of a destination element is computed in an order that is a function of the entry's arguments
 * and compile-time constants only (never of the CU count, of which workgroup finished first, or of what else runs), and is then added to
 * the destination with ONE fp32 add per element per call: dst = dst + total.  The destination therefore holds zeros or earlier contributions
 * (no pre-zeroing contract), and two calls with the same arguments on the same data give the same bits.  Partial sums go through `ws`
 * (device memory, 16-byte aligned, at least *_ws_bytes; contents irrelevant before and after) and are finished by a second launch on the
 * same stream.  The order of each sum is written at its kernel (csrc/gemm_tn.hip, csrc/layernorm.hip, csrc/embedding.hip, csrc/ordered_sum.h).  Not promised:
 * equality with the atomic entries, across different split_k, or across different row counts.  -2: ws_bytes too small.
 *
 * emdr2_gemm_tn_bf16_ordered mirrors emdr2_gemm_tn_bf16 (same operands, same dispatch between the two kernels, same slices): C += A^T B and
 * colsum_a += column sums of A.  ws_bytes covers either kernel; ldc >= J. */
int emdr2_gemm_tn_ordered_ws_bytes(int I, int J, int R, int split_k, size_t *bytes);
int emdr2_gemm_tn_bf16_ordered(const void *A, int64_t lda, const void *B, int64_t ldb, float *C, int64_t ldc, int I, int J, int R, int split_k,
                               float *colsum_a, void *ws, size_t ws_bytes, void *stream);
/* mirrors emdr2_layernorm_bwd (dmask == NULL) and emdr2_layernorm_bwd_mask (dmask != NULL: H == 768 and aligned only, -4 otherwise); dx and dmask
 * have the bits of those entries, dgamma / dbeta += the ordered column sums. */
int emdr2_layernorm_bwd_ordered_ws_bytes(int64_t rows, int H, size_t *bytes);
int emdr2_layernorm_bwd_ordered(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres, void *dx,
                                float *dgamma, float *dbeta, int64_t rows, int H, void *dmask, float drop_p, uint32_t seed, void *ws, size_t ws_bytes,
                                void *stream);
/* mirrors emdr2_embedding_bwd (cu == NULL: tokens % S == 0) and emdr2_embedding_packed_bwd (cu != NULL, nseq sequences, tokens = packed rows).
 * order (int64 [tokens]): the STABLE ascending sort of the token indices by ids -- ids[order[q]] ascending, equal ids in ascending token index.
 * Vocabulary rows without tokens and positions no sequence reaches are not written.  nseq of the ws_bytes call: the number of sequences
 * (tokens / S when dense). */
int emdr2_embedding_bwd_ordered_ws_bytes(int64_t tokens, int nseq, int S, int H, int n_types, size_t *bytes);
int emdr2_embedding_bwd_ordered(const int64_t *ids, const int64_t *types, const int32_t *cu, int nseq, const int64_t *order, const void *dout, float *dW,
                                float *dP, float *dT, int64_t tokens, int S, int H, int n_types, float drop_p, uint32_t seed, void *ws, size_t ws_bytes,
                                void *stream);

/* out[r, c] = keep(seed, r, c) ? x[r, c] / (1 - p) : 0 over a contiguous bf16 [n / cols, cols] tensor (the mask of a dropout site,
 * regenerated; cols % 8 == 0). */
int emdr2_dropout(const void *x, void *out, int64_t n, int cols, float drop_p, uint32_t seed, void *stream);

/* out[b1,b2][c, r] = in[b1,b2][r, c] (bf16), optional fp32 column sums colsum[c] += sum_r in[r, c] over all batches
 * (bias gradients: the reduce of the reference's autograd over [s, b]). */
int emdr2_transpose_bf16(const void *in, int64_t ld_in, void *out, int64_t ld_out, int rows, int cols,
                         int batch1, int64_t sI1, int64_t sO1, int batch2, int64_t sI2, int64_t sO2, float *colsum,
                         void *stream);

/* LayerNorm over the last dim (torch.nn.LayerNorm / apex FusedLayerNorm, mpu/layers.py:28-36; eps 1e-5, arguments.py:199).
 * x, y bf16 [rows, H]; gamma, beta, mean, rstd fp32.  bwd: dx (+ dres, the residual-branch gradient, optional), dgamma / dbeta
 * ACCUMULATED into fp32 buffers. */
int emdr2_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd, int64_t rows, int H,
                        float eps, void *stream);
int emdr2_layernorm_bwd(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres, void *dx,
                        float *dgamma, float *dbeta, int64_t rows, int H, void *stream);
/* The same, ALSO writing dmask = dx * keep(seed, row, col) / (1 - drop_p) (bf16 [rows, H], the bits of emdr2_dropout(dx, ...)): the operand of the
 * backward GEMMs of the bias-dropout-add (transformer.py:397-413) that produced x.  H == 768 only; -4 otherwise. */
int emdr2_layernorm_bwd_mask(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres, void *dx,
                             float *dgamma, float *dbeta, int64_t rows, int H, void *dmask, float drop_p, uint32_t seed, void *stream);

/* Scale-mask-softmax, the path the shipped scripts run (fused_softmax.py:113-125): masked scores are REPLACED by -10000
 * (bert/t5_attention_mask_func), masks derived on the fly from token ids (pad id 0; mask_creation_utils.py:17-42),
 * `causal` adds the history mask.  scores bf16 [batch, heads, sq, sk] in place; m, l: row max / sum-exp (fp32 [batch, heads, sq]).
 * drop_p > 0: attention dropout (transformer.py:262,366) applied to the stored probabilities AFTER normalisation (m, l are those of the
 * un-dropped softmax); keep bit = keep(seed, row, k) of csrc/rng.h, row = (b * heads + n) * sq + q.
 * _bwd: dprobs -> dscores in place, d = rowsum(P*dP_eff).  With m, l given, `probs` holds the raw scaled scores and P is rebuilt from
 * the statistics (the forward need not keep the [sq, sk] probabilities); dropout requires that form.
 * _t: transposed twin for the attention backward: S^T -> dropped P^T, dP^T -> dS^T (see softmax.hip). */
int emdr2_softmax_mask_fwd(void *scores, const int64_t *ids_q, const int64_t *ids_k, int batch, int heads, int sq, int sk, int causal,
                           float *m, float *l, float drop_p, uint32_t seed, void *stream);
int emdr2_softmax_mask_bwd(const void *probs, void *dprobs, const int64_t *ids_q, const int64_t *ids_k, const float *m, const float *l,
                           int batch, int heads, int sq, int sk, int causal, float drop_p, uint32_t seed, float *d, void *stream);
int emdr2_softmax_mask_t(void *scores_t, void *dprobs_t, const int64_t *ids_q, const int64_t *ids_k, const float *m, const float *l,
                         const float *d, int batch, int heads, int sq, int sk, int causal, float drop_p, uint32_t seed, void *stream);

/* Fused attention forward for head_dim 64, sk % 32 == 0 (transformer.py:283-381 without the [sq, sk] score matrix): o = dropout(softmax(mask(q k^T
 * scale))) v.  q [b, sq, heads, 64] / k [b, sk, heads, 64] strided views (element strides: batch, sequence, head; last dim contiguous),
 * v likewise, o [b, sq, heads, 64] contiguous, masks from token ids (pad id 0) + causal, masked scores REPLACED by -10000.
 * m / l (row max and row sum of exp, fp32 [b, heads, sq]) feed the backward.  Dropout keep-bit = keep(seed, row (b*heads+n)*sq+q,
 * column key) of csrc/rng.h (same generator as emdr2_dropout / emdr2_softmax_mask_*).  Returns -4 for shapes it does not cover. */
int emdr2_attention_fwd(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                        const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, void *o, const int64_t *ids_q, const int64_t *ids_k, int batch, int heads, int sq, int sk, int head_dim,
                        int causal, float scale, float drop_p, uint32_t seed, float *m, float *l, void *stream);

/* Fused attention backward for the same shapes (csrc/attention_bwd.hip): dq, dk, dv [b, s, heads, 64] with caller-given batch / sequence element
 * strides (heads 64 apart: they may be slices of one packed QKV gradient) from q, k, v (strided views),
 * the forward output o and its gradient dout (contiguous), and the forward's m, l.  dstat (fp32 [4, b, heads, sq], caller-owned scratch;
 * ABI 2: four times the ABI-1 size) receives what the dq kernel leaves for the dk / dv kernel per query: the exp2 offset
 * m log2(e) + log2(l), D = rowsum(dout * o), the dropout row hash and the real-token flag (the last two as bit patterns).
 * Same masks, scale and dropout stream as the forward. */
int emdr2_attention_bwd(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                        const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, const void *o, const void *dout, void *dq, int64_t dq_sb, int64_t dq_ss,
                        void *dk, void *dv, int64_t dkv_sb, int64_t dkv_ss,
                        const int64_t *ids_q, const int64_t *ids_k, const float *m, const float *l, float *dstat, int batch, int heads, int sq,
                        int sk, int head_dim, int causal, float scale, float drop_p, uint32_t seed, void *stream);

/* ---- packed ("varlen") sequences: the encoder stacks without their [PAD] rows (csrc/seqpack.hip) -------------------------------------
 * The reference runs [batch, S] token grids through every layer (transformer.py:283-381, emdr2_model.py:148-210); a padded key adds
 * exp(-10000 - max) == 0 to every real query and a padded query's row is never consumed, so dropping those rows changes no consumed value.
 * Layout: sequence i keeps its first len[i] tokens, len[i] = 1 + index of its last non-pad (id != 0) token (S for an all-pad row), and
 * owns rows [cu[i], cu[i+1]) of a [rows, ...] tensor; cu = exclusive prefix sum of len (int32 [n+1]).
 *
 * emdr2_seq_lengths: cu from ids [n, S]; totals[0] = cu[n], totals[1] = sum len^2, totals[2] = max len (int64 [3], device).  n <= 38000 (the lengths are scanned in LDS).
 * emdr2_seq_pack_ids: rowmap[t] (int32 [rows_padded]) = dense row i*S+pos of packed row t (-1 for t >= total: tail rows up to a GEMM-friendly
 *   multiple), inverse[i*S+pos] (int32 [n*S]) = packed row or -1, ids_packed / types_packed (int64 [rows_padded], 0 in the tail).
 * emdr2_gather_rows: out[r, :] = map[r] >= 0 ? in[map[r], :] : 0 (bf16 rows of H, H % 8 == 0) -- dense -> packed with rowmap, packed -> dense
 *   (zeros at pad rows) with inverse, token-0 rows of a packed tensor with cu.  emdr2_scatter_rows: out[map[r], :] = in[r, :] (map[r] >= 0). */
int emdr2_seq_lengths(const int64_t *ids, int n, int S, int32_t *cu, int64_t *totals, void *stream);
int emdr2_seq_pack_ids(const int64_t *ids, const int64_t *types, const int32_t *cu, int n, int S, int64_t total, int64_t rows_padded,
                       int32_t *rowmap, int32_t *inverse, int64_t *ids_packed, int64_t *types_packed, void *stream);
int emdr2_gather_rows(const void *in, const int32_t *map, void *out, int64_t rows_out, int H, void *stream);
int emdr2_scatter_rows(const void *in, const int32_t *map, void *out, int64_t rows_in, int H, void *stream);

/* Embedding.forward / backward over packed rows (language_model.py:169-181): position = rowmap[t] % S; tail rows (rowmap < 0) are zeros.
 * bwd: the position sums walk the sequences through cu (position p exists in sequence i iff p < len[i]). */
int emdr2_embedding_packed_fwd(const int64_t *ids_packed, const int64_t *types_packed, const int32_t *rowmap, const void *W, const void *P, const void *T,
                               void *out, int64_t rows, int S, int H, float drop_p, uint32_t seed, void *stream);
int emdr2_embedding_packed_bwd(const int64_t *ids_packed, const int64_t *types_packed, const int32_t *cu, int nseq, const void *dout, float *dW, float *dP,
                               float *dT, int64_t rows, int S, int H, int n_types, float drop_p, uint32_t seed, void *stream);

/* The fused attention kernels over packed operands (same kernels as emdr2_attention_fwd / _bwd): cu_q and / or cu_k (int32 [batch+1], either
 * may be NULL = that side is dense [batch, s] with its batch stride) give sequence b's rows [cu[b], cu[b+1]) of q / o / dq (k, v / dk, dv);
 * ids_q / ids_k are indexed the same way (packed ids for a packed side).  max_sq / max_sk: the longest sequence (grid size; dense side: s);
 * a packed key side takes ANY lengths >= 1 (keys past the end are masked).  With cu_q the row statistics m, l are [heads, total_q] and dstat is [4, heads, total_q].
 * pairs = sum_b sq_b * sk_b (flop accounting of the timing hooks only).  Replaces transformer.py:283-381 for the packed stacks and the
 * FiD cross-attention of emdr2_model.py:166-183 over the packed encoder output (cu_k = every K-th entry of the encoder's cu). */
int emdr2_attention_varlen_fwd(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                               const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, void *o, const int64_t *ids_q, const int64_t *ids_k,
                               const int32_t *cu_q, const int32_t *cu_k, int64_t total_q, int64_t pairs, int batch, int heads, int max_sq, int max_sk,
                               int head_dim, int causal, float scale, float drop_p, uint32_t seed, float *m, float *l, void *stream);
int emdr2_attention_varlen_bwd(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                               const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, const void *o, const void *dout, void *dq, int64_t dq_sb,
                               int64_t dq_ss, void *dk, void *dv, int64_t dkv_sb, int64_t dkv_ss, const int64_t *ids_q, const int64_t *ids_k,
                               const int32_t *cu_q, const int32_t *cu_k, int64_t total_q, int64_t pairs, const float *m, const float *l, float *dstat,
                               int batch, int heads, int max_sq, int max_sk, int head_dim, int causal, float scale, float drop_p, uint32_t seed, void *stream);

/* Split-key launches of the same kernels for FEW queries over VERY MANY keys: the FiD decoder's cross-attention (emdr2_model.py:166-183:
 * batch questions x 32 decoder positions over the ~20,000 / 40,000 packed encoder tokens of a question's 50 / 100 passages) and the cached
 * decoding steps of search_strategy.py:185-240.  One workgroup per (batch, head) walking every key block leaves most of the chip idle when
 * batch x heads is a few hundred; here the key blocks of a (batch, head) are dealt, 32 blocks (2,048 keys) each, to `ksplit` workgroups whose
 * fp32 partials (forward: unnormalised O + (m, l); backward: dQ) go through the caller's workspace and are folded by a small second kernel,
 * in split order (deterministic).  Queries are DENSE [batch, sq <= 128] (q_sb / dq_sb strides); cu_k as above or NULL for dense keys.  Same
 * results as the unsplit launch up to the order of fp32 additions (the softmax reference points are whole binades, so the bf16
 * probabilities do not depend on where a walk over the keys starts).
 *   _plan: ksplit for these extents (1 = do not split: more than 128 queries or fewer than 4,096 keys; never a function of the batch, so a
 *   question's result does not depend on what it is batched with) and the workspace bytes of the two launches (16-byte aligned ws). */
int emdr2_attention_splitkv_plan(int batch, int heads, int max_sq, int max_sk, int *ksplit, size_t *fwd_bytes, size_t *bwd_bytes);
int emdr2_attention_fwd_splitkv(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                                const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, void *o, const int64_t *ids_q, const int64_t *ids_k,
                                const int32_t *cu_k, int64_t pairs, int batch, int heads, int sq, int max_sk, int head_dim, int causal, float scale,
                                float drop_p, uint32_t seed, float *m, float *l, int ksplit, void *ws, size_t ws_bytes, void *stream);
int emdr2_attention_bwd_splitkv(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                                const void *v, int64_t v_sb, int64_t v_ss, int64_t v_sn, const void *o, const void *dout, void *dq, int64_t dq_sb,
                                int64_t dq_ss, void *dk, void *dv, int64_t dkv_sb, int64_t dkv_ss, const int64_t *ids_q, const int64_t *ids_k,
                                const int32_t *cu_k, int64_t pairs, const float *m, const float *l, float *dstat, int batch, int heads, int sq,
                                int max_sk, int head_dim, int causal, float scale, float drop_p, uint32_t seed, int ksplit, void *ws, size_t ws_bytes,
                                void *stream);

/* Attention probability mass per key segment (csrc/attention_mass.hip): which keys a forward launch read.  The operands and the masking rule
 * are those of emdr2_attention_fwd_splitkv -- q dense bf16 [batch, sq <= 128, heads, 64] as a strided view, keys dense ([batch, sk],
 * sk % 32 == 0) or packed through cu_k, pad id 0 masked -- plus that forward's row statistics m, l (fp32 [batch, heads, sq], of the
 * un-dropped softmax), a segment table seg (int32 [batch, n_seg + 1]: key offsets relative to the first key of sequence b, non-decreasing,
 * inside the sequence; empty segments give 0, keys outside every segment are not counted) and query weights w (fp32 [batch, sq]; NULL = 1):
 *     mass[b, h, g] (+)= sum_{i : ids_q[b, i] != 0} w[b, i] sum_{j in seg g} exp(s_ij - (m_i + ln l_i))
 *     s_ij = scale q_i . k_j, REPLACED by -10000 where the key is masked
 * mass is fp32 [batch, heads, n_seg].  No history mask, no dropout (the pre-dropout probability); a query whose token id is 0 contributes
 * nothing whatever w says.  accumulate != 0 adds to what mass holds.  Every element is written by one workgroup in a fixed order: results
 * are bit-reproducible and a sequence's do not depend on what it is batched with.
 * -1: null q, k, ids, m, l, seg or mass, batch / heads / sq / n_seg < 1, q or k not 16-byte aligned; -4: head_dim != 64, sq > 128,
 * max_sk > 65,536, dense sk % 32 != 0, strides that are no multiple of 8 elements. */
int emdr2_attention_key_mass(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss, int64_t k_sn,
                             const int64_t *ids_q, const int64_t *ids_k, const int32_t *cu_k, const float *m, const float *l,
                             const int32_t *seg, const float *w, float *mass, int batch, int heads, int sq, int max_sk, int n_seg, int head_dim,
                             float scale, int accumulate, void *stream);

/* The same with a weight per (head, key) -- value-norm weighted attention mass, kw = ||v_j||_2 from emdr2_head_row_norms:
 *     mass[b, h, g] (+)= sum_{i : ids_q[b, i] != 0} w[b, i] sum_{j in seg g} p_ij kw[h * kw_ld + krow0(b) + j]
 * krow0(b) + j is the row the kernel indexes ids_k with: b * sk + j for dense keys, cu_k[b] + j for packed ones; kw is fp32 [heads, kw_ld]
 * (dense keys: kw_ld >= batch * max_sk).  Same grid, same order of additions as the unweighted entry (one more fp32 multiplication per
 * term): kw == 1.0 gives its bits.  Only kw of keys INSIDE a segment is read (the load is clamped to the segment like the key-row load,
 * 4-byte loads, no alignment beyond 4 bytes); kw elsewhere may hold anything, NaN included.
 * Contract: kw is finite for every key inside a segment, pad keys (token id 0) included -- a masked key's p underflows to 0, and
 * 0 * NaN would not be 0.
 * Return codes of the unweighted entry, plus -1: kw null or not 4-byte aligned; -4: kw_ld < 1, or dense keys and kw_ld < batch * max_sk. */
int emdr2_attention_key_mass_weighted(const void *q, int64_t q_sb, int64_t q_ss, int64_t q_sn, const void *k, int64_t k_sb, int64_t k_ss,
                                      int64_t k_sn, const int64_t *ids_q, const int64_t *ids_k, const int32_t *cu_k, const float *m,
                                      const float *l, const int32_t *seg, const float *w, const float *kw, int64_t kw_ld, float *mass, int batch,
                                      int heads, int sq, int max_sk, int n_seg, int head_dim, float scale, int accumulate, void *stream);

/* norm[h * ld + r] = sqrt(sum_{d < 64} x[r, h, d]^2) in fp32 (csrc/attention_mass.hip): x bf16 as a strided view, row r = b * sk + s at
 * element offset b * x_sb + s * x_ss, head stride x_sn -- the (k_sb, k_ss, k_sn) conventions above, so kv[:, :, 1] of the packed KV
 * projection is passed as it is; a packed operand is batch = 1, sk = rows.  norm is fp32 [heads, ld], ld >= batch * sk, head-major (the
 * layout kw above wants).  Order of additions: 8 lanes x 16 bytes per (row, head); a lane adds its 8 exact squares in order (7 additions),
 * a 3-level xor butterfly (3), one square root.  No atomics: a repeated call gives identical bits.
 * Range: the relative accuracy (10 2^-24 on the sum, one ulp on the root) holds while the sum of squares is a normal fp32 number that
 * does not overflow, i.e. for rows with 2^-59 <= max |x| and every |x| <= 2^60; smaller rows are right to an ABSOLUTE 2^-60 (squares
 * below 2^-126 may be flushed), an all-zero row gives exactly 0.
 * -1: null x or norm, batch / sk / heads < 1, x not 16-byte or norm not 4-byte aligned; -4: head_dim != 64, strides that are no multiple
 * of 8 elements, ld < batch * sk. */
int emdr2_head_row_norms(const void *x, int64_t x_sb, int64_t x_ss, int64_t x_sn, float *norm, int64_t ld, int batch, int sk, int heads,
                         int head_dim, void *stream);

/* dpre = dact * gelu'(pre), exact-erf GELU (transformer.py:80,103-104; the tanh fusion of fused_bias_gelu.py is off in all scripts) */
int emdr2_gelu_bwd(const void *pre, const void *dact, void *dpre, int64_t n, void *stream);

/* Embedding.forward (language_model.py:169-181): out[t] = dropout(W[ids[t]] + P[t % S] (+ T[types[t]])); bwd scatter-adds the (masked)
 * gradient into fp32 grads (word rows: atomics; position rows: one owner thread per (position, column), no atomics; the <= 4 type rows:
 * register partials, one atomic per (position, column)).  tokens % S == 0.  Dropout element = (row t, column i). */
int emdr2_embedding_fwd(const int64_t *ids, const int64_t *types, const void *W, const void *P, const void *T, void *out, int64_t tokens, int S,
                        int H, float drop_p, uint32_t seed, void *stream);
int emdr2_embedding_bwd(const int64_t *ids, const int64_t *types, const void *dout, float *dW, float *dP, float *dT, int64_t tokens, int S, int H,
                        int n_types, float drop_p, uint32_t seed, void *stream);

/* log-softmax over the vocabulary + gather of the gold token (train_e2eqa.py:79-96,152-160): gold[row] = logits[row, label] - lse */
int emdr2_lse_gather_fwd(const void *logits, const int64_t *labels, float *gold, float *lse, int64_t rows, int V, void *stream);
int emdr2_lse_gather_bwd(const void *logits, const int64_t *labels, const float *lse, const float *w, void *dlogits, int64_t rows, int V,
                         void *stream);

/* Optimizer step on fp32 masters (FP16_Optimizer + apex FusedAdam, training.py:89-93, fp16/fp16.py:420-474): global-norm clip
 * (mpu/grads.py:74-127) folded in through gnorm_sq; decoupled weight decay; writes the bf16 working copy. */
/* *out += sum g[i]^2, deterministically (block partials summed in index order by the last block): data-parallel replicas derive
 * bit-identical clip factors.  scratch: 1025 floats, zero-initialised once by the caller (1024 partials + a counter the kernel resets). */
int emdr2_sumsq_f32(const float *g, int64_t n, float *out, float *scratch, void *stream);
int emdr2_adam_step(float *master, const float *grad, float *m, float *v, void *param_bf16, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, const float *gnorm_sq, float clip, void *stream);
/* The same update over one FLAT bucket of parameters (masters, gradients, both moments and the bf16 working copies of many tensors stored back
 * to back; apex runs FusedAdam through amp_C.multi_tensor_apply for the same reason, fp16/fp16.py:420-474): elements [0, decay_split) take
 * the weight decay, the rest none.  n, decay_split multiples of 4; fp32 buffers 16-byte aligned. */
int emdr2_adam_step_flat(float *master, const float *grad, float *m, float *v, void *work_bf16, int64_t n, int64_t decay_split, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int step, const float *gnorm_sq, float clip, void *stream);
/* ---- Step guard (--skip-nonfinite-steps): a step whose global gradient norm is not finite stores nothing, decided and applied on the
 * device.  Replaces FP16_Optimizer._check_overflow and the early return of FP16_Optimizer.step (fp16/fp16.py:294-302,420-474) and the
 * skipped-iteration branch of train_step (training.py:223-228) -- without their host read of the overflow flag. */
/* emdr2_sumsq_f32 with a census of the non-finite elements riding in the same pass (fp16/fp16.py:294-302 looks for them in a pass of its
 * own): *out receives exactly the bits emdr2_sumsq_f32 gives for the same g, n and prior *out (same grid rule, same order of partials,
 * same last-block sum).  census: device uint64[4], 8-byte aligned -- [0] += NaN elements, [1] += +-Inf elements, [2] = min([2], (bucket
 * << 40) | index) over the non-finite elements (all ones: none), [3] reserved.  Integer atomics, at most one per census word and wave,
 * none from a wave that saw finite elements only.  n < 2^40, 0 <= bucket < 2^23 (-1 otherwise). */
int emdr2_sumsq_census_f32(const float *g, int64_t n, float *out, float *scratch, uint64_t *census, int bucket, void *stream);
/* The verdict of step `step` (>= 1), one single-workgroup launch after the last bucket's census and before the first Adam launch
 * (fp16/fp16.py:420-474 returns before the update; training.py:223-228 counts the skip): skipped exactly when *gnorm_sq is NaN or +-Inf.
 * state: device uint64[8], zero before the first use -- [0] the verdict (0 applied, 1 skipped), [1] steps skipped in total, [2] current
 * run of consecutive skips, [3] longest run, [4..7] the STICKY record of the first skipped step since the caller last zeroed these four
 * words ([4] == 0: empty): its step, its first-offender key (census[2]; all ones when the sum overflowed over finite elements), its NaN
 * and Inf counts.  Leaves the census ready for the next step: {0, 0, all ones, 0} -- which is also what the caller sets it to once. */
int emdr2_step_verdict(const float *gnorm_sq, uint64_t *census, uint64_t *state, int64_t step, void *stream);
/* emdr2_adam_step_flat under the verdict (fp16/fp16.py:420-474: no update on overflow): state[0] == 1 -- every thread returns before its
 * first load of grad / m / v / master and nothing is stored; state[0] == 0 -- the arithmetic and the bits of emdr2_adam_step_flat (one
 * kernel template).  state non-NULL, 8-byte aligned. */
int emdr2_adam_step_flat_guarded(float *master, const float *grad, float *m, float *v, void *work_bf16, int64_t n, int64_t decay_split,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float *gnorm_sq,
                                 float clip, const uint64_t *state, void *stream);
/* Gradient exchange in 16 bits (the reference all-reduces fp16 gradients pre-divided by the world size, model/distributed.py:53-62):
 * dst = bf16(scale * src) before the all-reduce, dst = float(src) after it.  n % 4 == 0. */
int emdr2_scale_cast_f32_to_bf16(const float *src, void *dst, int64_t n, float scale, void *stream);
int emdr2_widen_bf16_to_f32(const void *src, float *dst, int64_t n, void *stream);
int emdr2_cast_f32_to_bf16(const float *src, void *dst, int64_t n, void *stream);
int emdr2_accum_bf16_to_f32(const void *src, float *dst, int64_t n, float scale, void *stream);

/* ---- State audit (--audit-optimizer-state-interval; not in the reference): ONE streaming pass over one flat optimizer bucket -- fp32
 * masters, both Adam moments and the bf16 working copies, 14 bytes per element, each read exactly once -- that leaves a digest of the
 * three fp32 arrays and five counts with their first offenders (csrc/state_audit.hip).  It writes nothing but block_keys and report.
 * Integer folds only (sums mod 2^64, xor, min; integer atomics): the words do not depend on the grid, the workgroup order or the device.
 * The audit states that bits are equal and that the invariants below hold; it does not state that the values are right.
 *
 * THE DIGEST -- fixed here; change it only for a reason written here.  It is taken over the 32-bit patterns w[i] of an array's n
 * elements: -0.0 and +0.0 differ, and so do two NaNs with different payloads.  mix = splitmix64's finaliser (digest_mix of
 * csrc/mips_digest.h, the function of the index digest of emdr2_mips.h), G = 0x9E3779B97F4A7C15, all sums mod 2^64:
 *   pair p holds elements 2p and 2p + 1:     e(p) = mix((((uint64)w[2p + 1] << 32) | w[2p]) + (p + 1) * G)
 *   block j = elements [8192 j, 8192 (j + 1)), the last one may be short; n_blocks = ceil(n / 8192):
 *                                            key_a(j) = mix((sum of e(p) over the block's pairs) ^ ((j + 1) * G) ^ TAG_a)
 *   TAG_a = 0x4D535452 << 32 for a = 0 master, 0x45585041 << 32 for a = 1 exp_avg (m), 0x45585053 << 32 for a = 2 exp_avg_sq (v)
 *   block_keys[a * n_blocks + j] = key_a(j); the digest of array a = (sum over j of key_a(j), xor over j of key_a(j)).
 * The pair's position is inside e, the block's inside the key and the array's in the tag: exchanging two pairs, two blocks or two arrays
 * changes the digest, and one flipped bit changes exactly one key.
 *
 * THE REPORT: device uint64[18] (held by callers as int64 bit patterns, like the step guard's words), set by the call itself:
 *   [0] n    [1] non-finite elements of master, [2] of m, [3] of v    [4] elements of v below zero (-Inf counts, -0.0 and NaN do not: a
 *   second moment is a sum of squares)    [5] work_mismatch: elements whose working copy differs in bits from f2bf(master), f2bf being the
 *   converter of csrc/prims.h that the Adam kernel and the cast kernel apply (the same function: exact for every input, NaN included)
 *   [6..10] for each of the checks [1..5] the lowest offending index inside the bucket, all ones when there is none
 *   [11] master sum, [12] master xor, [13] m sum, [14] m xor, [15] v sum, [16] v xor    [17] n_blocks
 * Two launches: one wave that sets the report, then the pass -- workgroups of 256 threads, min(n_blocks, 1024) of them, a function of n
 * alone; 16-byte loads of the fp32 arrays, 8-byte loads of the working copies.
 * n >= 8, n % 8 == 0 (bucket slots are 8-element aligned), master / m / v 16-byte, work_bf16 / block_keys / report 8-byte aligned, none
 * NULL: -1 otherwise, before any launch.  block_keys: emdr2_state_audit_ws_bytes(n) = 3 * n_blocks * 8 bytes. */
int emdr2_state_audit_ws_bytes(int64_t n, size_t *bytes);
int emdr2_state_audit(const float *master, const float *m, const float *v, const void *work_bf16, int64_t n, uint64_t *block_keys,
                      uint64_t *report, void *stream);

/* ---- Parameter statistics (--log-param-stats-interval; Megatron-LM: --log-params-norm, --log-num-zeros-in-grad): ONE streaming pass over
 * one flat optimizer bucket -- fp32 gradients, masters and both Adam moments, 16 bytes per element, each read exactly once -- that leaves
 * eight words for EVERY parameter of the bucket (csrc/param_stats.hip).  It writes nothing but workspace and out.  No atomics: every
 * floating-point addition happens in the order stated below, so data-parallel replicas, which hold the same buckets after the gradient
 * exchange, get the same bits with no collective.
 *
 * THE PLAN (emdr2_param_stats_plan: host only, touches no GPU; the one place where the chunk rule lives).  A bucket of n elements is
 * described by its parameters' element offsets and lengths: offsets multiples of 8 (FlatAdam's slot alignment), ascending, not
 * overlapping, length >= 1, offset + length <= n, n >= 8 and n % 8 == 0, n_params >= 1 -- anything else returns -1.  Parameter p is cut into
 * chunks of PARAM_STATS_CHUNK = 8192 elements from ITS OWN start, the last one may be short; a chunk is an ITEM.
 *   items: int64 [n_items, 2] = (first element inside the bucket, length), parameter after parameter, chunks ascending; NULL: only count
 *   first: int64 [n_params + 1], first[p] = index of parameter p's first item, first[n_params] = n_items (never NULL)
 * The padding between two tensors belongs to no item and never reaches a result.
 *
 * THE WORDS: out is uint64 [n_params, 8], every word written by the call; the workspace holds one record of the same eight words per item
 * (emdr2_param_stats_ws_bytes(n_items) = n_items * 64 bytes).
 *   [0] sum g^2 as float64 bits (the gradient as it lies in the bucket: unclipped)    [1] sum w^2 as float64 bits (fp32 masters)
 *   [2] sum d^2 as float64 bits, d = (m / bc1) / (sqrtf(v / bc2) + eps) evaluated in fp32, statement for statement the Adam kernel's
 *       (csrc/optimizer.hip, adam_flat_kernel), bc1 = 1 - powf(beta1, step), bc2 = 1 - powf(beta2, step) from the function the Adam entries
 *       call (csrc/adam_bias.h): the Adam part of the last applied update without the learning rate.  step == 0: 0, m and v are not read
 *   [3] max |g|, [4] max |w|: the fp32 bit pattern of the absolute value in the low 32 bits, compared as integers; NaN elements are left
 *       out, Inf elements counted in (0x7f800000)
 *   [5] gradient elements equal to +-0 (denormals are not zeros)    [6] non-finite gradient elements    [7] the parameter's element count
 *
 * THE ORDER of the additions -- fixed here; change it only for a reason written here.  Squares are formed and added in double (the square
 * of an fp32 value is exact in double, so only the order counts).
 *   1. First launch, 256 threads, min(n_items, 1024) workgroups (a function of the plan alone); workgroup g takes items g, g + grid, ...
 *      Thread t takes the 4-element groups t, t + 256, ... of the item (one 16-byte load per array) and adds into its own sums from 0.0:
 *      groups ascending, elements ascending; elements at or beyond the item's end are masked out one by one
 *   2. the xor butterfly over the 64 lanes of a wave, x += x[lane ^ o] for o = 32, 16, 8, 4, 2, 1
 *   3. the four waves through LDS: (w0 + w1) + (w2 + w3).  That is the item's record
 *   4. Second launch, one wave per parameter: lane group s = 0 .. 7 adds, from 0.0, the records of the parameter's items s, s + 8, ... in
 *      ascending order; then the xor butterfly over the groups, x += x[s ^ o] for o = 4, 2, 1
 * Maxima and counts are integer folds along the same paths.
 * Null pointers, master / grad / m / v not 16-byte or items / first / workspace / out not 8-byte aligned, n < 8, n % 8, n_items < 1,
 * n_params < 1, n_params > n_items, step < 0: -1 before any launch.  items and first are DEVICE copies of the plan. */
int emdr2_param_stats_plan(const int64_t *offsets, const int64_t *lengths, int64_t n_params, int64_t n, int64_t *items, int64_t *first,
                           int64_t *n_items);
int emdr2_param_stats_ws_bytes(int64_t n_items, size_t *bytes);
int emdr2_param_stats(const float *master, const float *grad, const float *m, const float *v, int64_t n, const int64_t *items, int64_t n_items,
                      const int64_t *first, int64_t n_params, float beta1, float beta2, float eps, int step, uint64_t *workspace, uint64_t *out,
                      void *stream);

/* C[m, n-tile partials]: the tied LM head without the logits (language_model.py:28-41 + the log-softmax / gather of
 * train_e2eqa.py:79-96).  For x[m, n] = bf16(alpha * sum_k A[m,k] B[n,k] + bias[n]) -- the value the unfused path would have stored -- writes per
 * row m and per 64-column block j (N / 64 of them): part_max[m, j] = max_n x, part_sum[m, j] = sum_n exp(x - part_max), and gold[m] =
 * x[m, labels[m]].  emdr2_lse_combine turns them into gold - logsumexp.  M % 256 == 0, N % 256 == 0, K % 128 == 0. */
int emdr2_gemm_nt_lse_bf16(const void *A, int64_t lda, const void *B, int64_t ldb, int M, int N, int K, float alpha, const float *bias,
                           const int64_t *labels, float *part_max, float *part_sum, float *gold, void *stream);

/* out[row] = gold[row] - logsumexp(row) from the per-block partials of emdr2_gemm_nt_lse_bf16 (slots = N / 64); lse optional. */
int emdr2_lse_combine(const float *part_max, const float *part_sum, const float *gold, float *out, float *lse, int64_t rows, int slots,
                      void *stream);

/* Retriever prior over the K retrieved passages (emdr2_model.py:134-145): logp[b, k] = log_softmax_k( <q[b], c[b, k]> * scale ), scale =
 * 1/sqrt(H) with --retriever-score-scaling; q bf16 [batch, H], c bf16 [batch, K, H], logp / prob (= exp(logp), kept for the backward) fp32
 * [batch, K]; K <= 1024 (-4 above).  bwd: bf16 gradients dq [batch, H], dc [batch, K, H] (either may be NULL: --no-query/context-embedder-training). */
int emdr2_retriever_prior_fwd(const void *q, const void *c, float *logp, float *prob, int batch, int K, int H, float scale, void *stream);
int emdr2_retriever_prior_bwd(const float *dlogp, const float *prob, const void *q, const void *c, void *dq, void *dc, int batch, int K, int H,
                              float scale, void *stream);
/* The same prior with fp16 contexts: c fp16 [batch, K, H], row-major, 16-byte aligned -- rows gathered from the evidence index
 * (emdr2_mips_gather_rows, --context-embeddings-from-index).  q bf16 and c fp16 are both widened exactly to fp32, fp32 accumulation, * scale,
 * log-softmax over K: the kernels of the entries above instantiated for the other context element, not a cast (fp16 -> bf16 would drop three
 * mantissa bits of every stored value).  Same checks: K > 1024 -> -4; null or misaligned q / c, H < 8 or H & 7 -> -1.  The contexts are
 * constants of the step: the backward writes dq (bf16 [batch, H]) only. */
int emdr2_retriever_prior_h16_fwd(const void *q, const void *c, float *logp, float *prob, int batch, int K, int H, float scale, void *stream);
int emdr2_retriever_prior_h16_bwd(const float *dlogp, const float *prob, const void *q, const void *c, void *dq, int batch, int K, int H,
                                  float scale, void *stream);
/* EMDR2 marginal likelihood (train_e2eqa.py:98-123): marginal[b, l] = logsumexp_k( prior[b, k] + gold[b, k, l] ), gold = per-passage gold
 * log-likelihoods of the no-grad one-context pass (constants).  bwd: dprior[b, k] = sum_l dmarginal[b, l] * posterior[b, k, l].  All fp32. */
int emdr2_marginal_fwd(const float *prior, const float *gold, float *marginal, int batch, int K, int L, void *stream);
int emdr2_marginal_bwd(const float *prior, const float *gold, const float *marginal, const float *dmarginal, float *dprior, int batch, int K, int L,
                       void *stream);

/* Measurement hooks (bench.py): with timing on, every GEMM / attention launch of this library is bracketed by hipEvents recorded on its launch
 * stream.  collect() waits for them and returns, per kind (0 NT GEMM, 1 TN GEMM, 2 attention forward, 3 attention backward), the summed
 * milliseconds, the summed algorithmic flops and the number of launches since the last set_timing / collect.  kinds >= 4. */
int emdr2_ops_set_timing(int enabled);
int emdr2_ops_timing_collect(double *ms, double *flops, int64_t *launches, int kinds);

#ifdef __cplusplus
}
#endif
#endif
