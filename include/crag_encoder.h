/*
 * crag_encoder.h — C ABI of the hand-written HIP operators of the Qwen3-Embedding encoder lane
 * (libcrag_dense.so, gfx950).  They replace the arithmetic the reference delegates to an external
 * Triton/ONNX gateway (/root/reference/app/embeddings.py:53-59 ->
 * P620_TRITON_QWEN3_4B_EMBEDDING_RUNBOOK.md:618-649,683-716): everything of the decoder forward
 * except the plain linear layers (library GEMMs), plus the gateway's pooling / slice / L2-norm
 * post-processing (RUNBOOK:703-715).
 *
 * Conventions as in crag_dense.h: 0 = ok, negative = error (crag_last_error()); all pointers are
 * DEVICE pointers on the current device; `stream` is a hipStream_t as void*.  bf16 tensors are
 * raw uint16 storage, row-major.  Sequences are PACKED (no padding): T tokens total,
 * cu_seqlens[B+1] int32 prefix sums.
 */
#ifndef CRAG_ENCODER_H
#define CRAG_ENCODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRAG_HEAD_DIM 128 /* Qwen3 head_dim; the attention / rope kernels are specialised for it */

/* x[t, :] = table[ids[t], :]            (embed_tokens).  hidden % 8 == 0.  An id outside the table is clamped, not
 * refused: ids[t] < 0 reads row 0, ids[t] >= vocab reads row vocab - 1. */
int crag_enc_embed_gather(const int32_t *ids, const uint16_t *table, uint16_t *out, int64_t n_tokens,
                          int hidden, int64_t vocab, void *stream);

/* RMSNorm with optional fused residual add (the pre-norm residual stream):
 *   s = x (+ residual_in);  residual_out = s (if non-NULL);  out = weight * bf16(s * rsqrt(mean(s^2)+eps))
 * rows x hidden, hidden % 8 == 0, hidden <= 8192. */
int crag_enc_rmsnorm(const uint16_t *x, const uint16_t *residual_in, const uint16_t *weight,
                     uint16_t *out, uint16_t *residual_out, int64_t rows, int hidden, float eps,
                     void *stream);

/* In-place per-head RMSNorm (q_norm / k_norm weights, [128]) + rotary embedding (rotate-half
 * form) on the q and k parts of the fused projection qkv[T, (hq + 2*hkv) * 128];
 * cos_sin[max_pos, 64, 2] fp32 table; positions[T] int32 (position inside its sequence). */
int crag_enc_qk_norm_rope(uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                          const float *cos_sin, const int32_t *positions, int64_t n_tokens, int hq,
                          int hkv, float eps, void *stream);

/* V part of qkv -> Vt[hkv][128][t_pad] (keys on the fast axis, each sequence starting at a
 * 32-aligned padded offset, pads zero).  tok_of_pad[t_pad] int32: packed token of a padded slot
 * or -1.  Inside every 32-slot block the slots are stored in the order the attention kernel's PV
 * fragments consume them: stored index 16*s2 + 8*h + 4*g + r holds slot 16*s2 + 8*g + 4*h + r
 * (s2, h, g in {0,1}, r in 0..3), i.e. one lane's 8 keys of one MFMA are 16 contiguous bytes. */
int crag_enc_v_transpose(const uint16_t *qkv, uint16_t *vt, const int32_t *tok_of_pad, int64_t t_pad,
                         int hq, int hkv, void *stream);

/* Causal grouped-query flash attention over packed sequences, head_dim 128, bf16 in/out,
 * fp32 softmax and accumulation.  One workgroup per (q block of 32 rows, kv head): its 4 waves are
 * the hq/hkv = 4 query heads of the group.  blk_seq / blk_q0 [n_blocks] int32: sequence and first
 * row (inside the sequence) of every q block.  qkv rows must extend 32 rows past T (any finite or
 * non-finite content).  out[T, hq*128]. */
int crag_enc_attention(const uint16_t *qkv, const uint16_t *vt, uint16_t *out, const int32_t *cu_seqlens,
                       const int32_t *cu_pad, const int32_t *blk_seq, const int32_t *blk_q0,
                       int n_blocks, int64_t t_pad, int hq, int hkv, float scale, void *stream);

/* out[t, i] = silu(gu[t, i]) * gu[t, inter + i]   (gate | up fused projection): silu = g / (1 + exp(-g)) in fp32,
 * rounded to bf16, the product rounded to bf16.  Where exp(-g) overflows fp32 (bf16 gates <= -89) silu is taken as g * exp(g), so
 * it stays the small negative number it is (-2e-37 at -89) down to the denormals instead of becoming -0.  The fused
 * epilogues further down keep the quotient alone: they give crag_enc_swiglu's bits for gates above -89. */
int crag_enc_swiglu(const uint16_t *gate_up, uint16_t *out, int64_t rows, int inter, void *stream);

/* Pooling + post-processing of the gateway: per sequence take the last token (mode 0) or the
 * mean over its tokens (mode 1) of the FINAL-NORMED hidden state, keep the first out_dim
 * components, L2-normalise in fp32 with max(norm, 1e-12).  For mode 0 `hidden_states` is the
 * un-normed residual stream and the final RMSNorm (weight, eps) is applied to the pooled rows
 * only; for mode 1 it must already be normed (weight may be NULL).  out[B, out_dim] fp32. */
int crag_enc_pool_normalize(const uint16_t *hidden_states, const uint16_t *final_norm_w,
                            const int32_t *cu_seqlens, float *out, int n_seqs, int hidden, int out_dim,
                            int mode, float eps, void *stream);
/* Same, with the last sub-block's output `delta` (nullable; mode 0 only) added to the residual stream for the
 * pooled rows only: hidden = bf16(hidden_states + delta) -- the model's final `hidden + mlp(...)` without a pass
 * over every token. */
int crag_enc_pool_normalize_add(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                                const int32_t *cu_seqlens, float *out, int n_seqs, int hidden, int out_dim,
                                int mode, float eps, void *stream);
/* Last-token pooling with the pooled rows given as DATA: sequence b pools row rows[b] of hidden_states (+ delta, nullable)
 * -- what a graph replay over padded sequences needs (the real last token of every sequence) without gathering the rows
 * first. */
int crag_enc_pool_normalize_rows(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                                 const int64_t *rows, float *out, int n_seqs, int hidden, int out_dim, float eps,
                                 void *stream);

/* Linear layer for m_rows <= 32 tokens -- ONE query per /retrieve request (retrieve.py:427) -- as a weight stream:
 * out[m_rows, n] = x[m_rows, k] @ W[n, k]^T (bf16 in, fp32 accumulate, bf16 out).
 *   x      [m_pad, k] bf16, m_pad = 16 or 32 rows allocated (rows >= m_rows are padding and never stored)
 *   wsw    the weight in MFMA A-fragment order: [n/16][k/32][lane = 16 (kk/8) + row][8] = W[16 tile + row][32 step +
 *          8 (lane >> 4) + e]  (torch: W.view(n/16, 16, k/32, 4, 8).permute(0, 2, 3, 1, 4).contiguous())
 *   epilogue 0: out [m_rows, n].
 *   epilogue 1 (gate|up projection): the rows of W are interleaved per 8 features -- tile t = gate rows 8t..8t+7,
 *          then up rows 8t..8t+7 -- and out [m_rows, n/2] = silu(gate) * up with the model's bf16 roundings
 *          (crag_enc_swiglu's arithmetic).
 * Built for the Qwen3-Embedding-4B widths: k = 2560, 4096 (epilogue 0) or 9728 (epilogue 0); k = 2560 (epilogue 1). */
int crag_enc_skinny_gemm(const uint16_t *x, const uint16_t *wsw, uint16_t *out, int m_rows, int m_pad, int n, int k,
                         int epilogue, void *stream);

/* crag_enc_qk_norm_rope and crag_enc_v_transpose in ONE launch (disjoint columns of the fused qkv rows). */
int crag_enc_qk_rope_vt(uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w, const float *cos_sin,
                        const int32_t *positions, int64_t n_tokens, int hq, int hkv, float eps, uint16_t *vt,
                        const int32_t *tok_of_pad, int64_t t_pad, void *stream);

/* ---- the decoder layer at 16 / 32 token rows (one short query per /retrieve request, retrieve.py:427) as five
 * launches: csrc/crag_encoder_small.hip ----
 *
 * crag_enc_small_gemm: out[m_rows, n (or n/2)] = X[m_pad, k] @ W[n, k]^T with the weights streamed once from HBM.
 *   wsw: W in tile order [n / rows_per_tile][k / 32][4][rows_per_tile][8] (a tile's k-step is one contiguous block
 *        whose 16-byte pieces are the MFMA A-operand registers of a lane);  rows_per_tile in {10, 12, 16}.
 *   norm_w != NULL (RMSNorm prologue, k = 2560): X = weight * bf16((x + delta) * rsqrt(mean((x + delta)^2) + eps)),
 *        the sum x + delta rounded to bf16 first (the residual stream); delta is required (zeros for none);
 *        res_out (nullable, must not alias x or delta) receives x + delta.
 *   norm_w == NULL: X = x; delta and res_out must be NULL.
 *   epilogue 1 (rows_per_tile 16): a tile is 8 gate rows then the 8 up rows of the same features; out [m_rows, n/2]
 *        = silu(gate) * up with crag_enc_swiglu's roundings.
 * Built for the Qwen3-Embedding-4B widths: (k 2560, prologue, 12-row tiles), (k 2560, prologue, SwiGLU, 16-row
 * tiles), (k 4096, 10-row tiles), (k 9728, 10-row tiles).  m_pad = 16 or 32 rows are read, m_rows written. */
int crag_enc_small_gemm(const uint16_t *x, const uint16_t *delta, const uint16_t *norm_w, uint16_t *res_out,
                        const uint16_t *wsw, uint16_t *out, int m_rows, int m_pad, int n, int k, int rows_per_tile,
                        int epilogue, float eps, void *stream);

/* Per-head q/k RMSNorm + RoPE (crag_enc_qk_norm_rope's arithmetic) + causal attention for n_tokens <= 32 packed
 * token rows in one launch, one workgroup per q head.  qkv[T, (hq + 2 hkv) * 128] holds the raw projections and is
 * not modified; positions[T] (position inside its sequence) also tells the sequences apart: tokens t and u belong
 * to the same sequence iff t - positions[t] == u - positions[u].  cos_sin: the [max_pos, 64, 2] table of
 * crag_enc_qk_norm_rope, or with cos_sin_by_token != 0 its rows gathered per token, [T, 64, 2] (done once per forward
 * it takes a dependent load out of every layer).  out[T, hq * 128]. */
int crag_enc_small_attention(const uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                             const float *cos_sin, int cos_sin_by_token, const int32_t *positions, uint16_t *out,
                             int n_tokens, int hq, int hkv, float eps, float scale, void *stream);
/* The same kernel over a packed batch of n_seqs SHORT sequences (every one <= max_len <= 32 tokens; cu_seqlens[n_seqs + 1]
 * = their first rows, as crag_enc_attention takes it): one workgroup per (q head, sequence), grid (hq, n_seqs) -- q/k-norm
 * + RoPE + attention of a batch of short queries (3 to 8 of them: the gateway's batch sizes) in ONE launch instead of
 * crag_enc_qk_rope_vt + crag_enc_attention.  positions[T], cos_sin as above; qkv is not modified. */
int crag_enc_small_attention_seqs(const uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                                  const float *cos_sin, int cos_sin_by_token, const int32_t *positions,
                                  const int32_t *cu_seqlens, int n_seqs, int max_len, uint16_t *out, int hq, int hkv,
                                  float eps, float scale, void *stream);
/* The same with the qkv projection handed over as the split-K partial tiles of crag_enc_wide_gemm_rows
 * (qkv_partial_rows[splitk][m_pad][(hq + 2 hkv) * 128] fp32): every head vector is bf16(sum over the splits, in split
 * order) -- what crag_enc_wide_reduce would have written -- summed while it is loaded. */
int crag_enc_small_attention_seqs_parts(const float *qkv_partial_rows, int splitk, int m_pad, const uint16_t *q_norm_w,
                                        const uint16_t *k_norm_w, const float *cos_sin, int cos_sin_by_token,
                                        const int32_t *positions, const int32_t *cu_seqlens, int n_seqs, int max_len,
                                        uint16_t *out, int hq, int hkv, float eps, float scale, void *stream);

/* ---- the linear layers at 32 / 64 / 96 / 128 token rows: what the gateway's batcher hands the model (RUNBOOK:304,331-334:
 * max_batch_size 8, preferred_batch_size [1, 2, 4, 8]) -- csrc/crag_encoder_wide.hip ----
 *
 * crag_enc_wide_gemm: partial[s] = X[m_pad, K_s] @ W[n, K_s]^T for the K ranges s = 0 .. splitk-1 (fp32), the weights
 * streamed once from HBM, the activations staged through LDS; 4 waves = 128 rows of W per workgroup, grid
 * (n / 128, splitk).
 *   x   [m_pad, k] bf16, m_pad = 32, 64, 96 or 128 rows allocated and READ (padding rows must hold finite values)
 *   ww  W in MFMA A-fragment order for v_mfma_f32_32x32x16_bf16: [n/32][k/16][lane = 32 (kk/8) + row][8]
 *       (torch: W.view(n/32, 32, k/16, 2, 8).permute(0, 2, 3, 1, 4).contiguous())
 *   partial  crag_enc_wide_partial_bytes(m_pad, n, splitk) bytes of scratch: the accumulators in register order
 *   n % 128 == 0, k % 128 == 0, 1 <= splitk <= k / 128.
 * crag_enc_wide_reduce: out = bf16(sum over the splits, in split order) -- one rounding, as an unsplit GEMM --,
 *   epilogue 0: out [m_rows, n];  epilogue 1 (gate|up: every 32 rows of W are 16 gate rows then the 16 up rows of the
 *   same features): out [m_rows, n/2] = silu(gate) * up with crag_enc_swiglu's roundings. */
int64_t crag_enc_wide_partial_bytes(int m_pad, int n, int splitk);
int crag_enc_wide_gemm(const uint16_t *x, const uint16_t *ww, float *partial, int m_pad, int n, int k, int splitk,
                       void *stream);
/* The unsplit form in ONE launch: out = bf16(X @ W^T) (epilogue 0) or silu(gate) * up (epilogue 1) written by the GEMM
 * kernel itself -- no partial tiles, no reduce launch; n / 128 workgroups (gate|up: 152). */
int crag_enc_wide_gemm_direct(const uint16_t *x, const uint16_t *ww, uint16_t *out, int m_rows, int m_pad, int n, int k,
                              int epilogue, void *stream);
int crag_enc_wide_reduce(const float *partial, uint16_t *out, int m_rows, int m_pad, int n, int splitk, int epilogue,
                         void *stream);
/* A split-K projection whose consumer is the residual add + RMSNorm of the next sub-block (down -> ln1): the partial
 * tiles TOKEN-MAJOR, partial_rows[splitk][m_pad][n] fp32 (crag_enc_wide_partial_bytes bytes as well), and the norm that
 * reads them -- delta = bf16(sum over the splits, in split order), the rounding of crag_enc_wide_reduce, then
 * crag_enc_rmsnorm's arithmetic with residual_in (required) / residual_out (nullable; may alias residual_in): two
 * launches (reduce, norm) become one.  hidden = n <= 4096. */
int crag_enc_wide_gemm_rows(const uint16_t *x, const uint16_t *ww, float *partial_rows, int m_pad, int n, int k, int splitk,
                            void *stream);
int crag_enc_rmsnorm_partials(const float *partial_rows, int splitk, int m_pad, const uint16_t *residual_in,
                              const uint16_t *weight, uint16_t *out, uint16_t *residual_out, int rows, int hidden,
                              float eps, void *stream);

/* ---- the Qwen3-Reranker forward: csrc/crag_attention.hip (attention), csrc/crag_rerank.hip (head) ----
 *
 * crag_enc_attention_prefixed: crag_enc_attention with a per-sequence parent[B] int32 (-1: a root; otherwise the index
 *   of a ROOT sequence of the same batch, the shared prefix segment).  A child's queries attend to every key of its
 *   parent, then causally to their own keys, under one softmax; a root is attended exactly as by crag_enc_attention.
 *   The caller gives a child's tokens the positions plen(parent) + j.  hq / hkv = 2 or 4.  Every other input as
 *   crag_enc_attention (blk_seq / blk_q0: the q blocks of every sequence, parents included).
 * crag_enc_rerank_head: per pair b: x = bf16(hidden_states[rows[b]] + delta[rows[b]]) (delta nullable), the final
 *   RMSNorm with crag_enc_pool_normalize's roundings, then fp32 dot products with lm_rows[0] ("yes") and lm_rows[1]
 *   ("no"), lm_rows [2, hidden] bf16.  out[n_pairs, 3] fp32 = (logit_yes, logit_no, exp(log_softmax([no, yes])[1])).
 *   hidden <= 8192. */
int crag_enc_attention_prefixed(const uint16_t *qkv, const uint16_t *vt, uint16_t *out, const int32_t *cu_seqlens,
                                const int32_t *cu_pad, const int32_t *blk_seq, const int32_t *blk_q0,
                                const int32_t *parent, int n_blocks, int64_t t_pad, int hq, int hkv, float scale,
                                void *stream);
int crag_enc_rerank_head(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                         const int64_t *rows, const uint16_t *lm_rows, float *out, int n_pairs, int hidden, float eps,
                         void *stream);

/* ---- autoregressive decoding: csrc/crag_decode.hip ----
 *
 * The KV cache of ONE layer is two bf16 arrays [n_slots][hkv][max_len][128] (keys: normed and rotated; values: raw).
 * A slot holds one sequence; how many tokens it holds is the caller's knowledge and comes from the HOST.
 *
 * crag_enc_decode_attention: one new token for each of n_seqs (1..CRAG_DECODE_MAX_SEQS) sequences.
 *   qkv_new [n_seqs, (hq + 2 hkv) * 128]: the raw fused projections of the new tokens (not modified);
 *   h_slots / h_cache_len [n_seqs]: HOST arrays -- the slot of every sequence and the number of tokens it holds, which
 *   is also the new token's position.  Per sequence: q/k RMSNorm + RoPE of the new row with the arithmetic and the
 *   roundings of crag_enc_qk_norm_rope (the cached key of a token is the same bits whichever entry wrote it), the key
 *   and the raw value stored at position len of the slot, attention of the hq queries over the len + 1 keys (fp32
 *   softmax and accumulation), out [n_seqs, hq * 128] bf16.  Cache rows at or beyond len + 1 are never read.
 *   The key range is cut into splits of CRAG_DECODE_SPLIT keys, one workgroup per (split, kv head, sequence), combined
 *   in ascending split order by a second kernel: no atomics, and a sequence's output bits depend on nothing but its own
 *   data -- not on n_seqs, the slot or the other sequences.  hq / hkv = 2 or 4.
 *   workspace: crag_enc_decode_workspace_bytes(n_seqs, hq, max_len) bytes of device scratch, 16-byte aligned.
 *   CRAG_EINVAL, nothing enqueued: a NULL pointer, n_seqs outside 1..8, a length < 0 or >= max_len (or >= max_pos, the
 *   rows of cos_sin), a slot outside 0..n_slots - 1 or named twice in the call.  CRAG_E2BIG: the workspace is too small.
 * crag_enc_decode_attention_shared: crag_enc_decode_attention over FORKED sequences, which share leading cache rows
 *   without holding copies of them.  Two more HOST arrays per sequence: sequence b reads its logical row j from slot
 *   h_parent[b] when j < h_shared_len[b] and from its own slot h_slots[b] otherwise; the new token is appended at row
 *   cache_len of its own slot.  h_parent[b] == h_slots[b] or h_shared_len[b] == 0: not forked.  Rows below shared_len of
 *   a forked sequence's own slot are never read, nor any row at or beyond cache_len + 1.
 *   Output bits and appended bits are those crag_enc_decode_attention gives on a slot that holds a private copy of the
 *   same logical rows: the same splits, every row read by the same lanes and dotted in the same order, the same
 *   combine; only the address of a row changes, and how many sequences one load serves.  The sequences of a call that
 *   read one parent (the parent itself included when it is in the call) form a group: a split that lies wholly below
 *   the shared length of every member is computed by one workgroup per (split, kv head, two members of the group -- the
 *   kernel takes up to eight; two is what measures best), which loads each key and value row once for its
 *   members' query heads.  The other splits run per sequence.  Three launches, no atomics; the workspace of
 *   crag_enc_decode_workspace_bytes.
 *   CRAG_EINVAL, nothing enqueued: every refusal of crag_enc_decode_attention; a NULL h_parent / h_shared_len; a parent
 *   outside 0..n_slots - 1; a shared_len outside 0..cache_len; a forked sequence whose parent slot is a sequence of the
 *   call with cache_len < that shared_len (a shared row would be written during the call).  A parent slot that is not
 *   in the call is allowed.
 * crag_enc_decode_attention_rows: crag_enc_decode_attention_shared with h_new_len[b] >= 1 new rows per sequence (HOST
 *   array), appended back to back behind h_cache_len[b]: R = the sum of h_new_len, 1..CRAG_DECODE_MAX_ROWS.  qkv_new
 *   [R, (hq + 2 hkv) * 128] and out [R, hq * 128] hold the sequences' rows in call order.  h_parent / h_shared_len are
 *   nullable TOGETHER: nobody is forked.  Row i of sequence b has position cache_len + i; its key and raw value go to
 *   that row of the sequence's own slot, and it attends the logical rows 0 .. cache_len + i -- the parent's below
 *   shared_len, its own otherwise, the rows appended earlier in this call among them.  The bits of out and of every
 *   appended row are those new_len[b] successive calls of crag_enc_decode_attention (_shared for a forked sequence) give
 *   on a private copy of the logical rows: the same 128-key splits, every row read by the same 16-lane group and dotted
 *   in the same order, the same combine.  A workgroup of the split launch serves a run of consecutive rows of ONE
 *   sequence (DESIGN 6d for how many) and loads each key and value row once for all of them; a key behind a row's own
 *   position scores -inf for that row only.  Nothing at or beyond cache_len + new_len is read, nor a forked sequence's
 *   own rows below shared_len.  Three launches (prepare: one workgroup per row; split; combine), no atomics; the
 *   workspace is crag_enc_decode_workspace_bytes(R, hq, max_len), indexed by row.
 *   CRAG_EINVAL, nothing enqueued: every refusal of crag_enc_decode_attention_shared (a NULL h_parent with a NULL
 *   h_shared_len excepted); a NULL h_new_len; new_len < 1; R > CRAG_DECODE_MAX_ROWS; cache_len + new_len > max_len or
 *   > max_pos.  CRAG_E2BIG: the workspace is too small.
 * crag_enc_lm_head: per row r < n_rows (1..8): x = bf16(hidden_states[r] + delta[r]) (delta nullable), the final RMSNorm
 *   with crag_enc_rerank_head's roundings, logits[r, v] = fp32 dot with lm_head[v] for EVERY v < vocab (lm_head
 *   [vocab, hidden] bf16; a tied model passes embed_tokens), token[r] = the lowest id among the maxima of logits[r]
 *   that is not in banned[n_banned] (device int32, nullable with n_banned 0; at most CRAG_LM_HEAD_MAX_BANNED) -- -1 when
 *   no id is left.  hidden % 64 == 0, n_rows * (hidden + 8) <= CRAG_LM_HEAD_MAX_ELEMS (the rows live in LDS). */
#define CRAG_DECODE_MAX_SEQS 8
#define CRAG_DECODE_MAX_ROWS 8
#define CRAG_DECODE_SPLIT 128
#define CRAG_LM_HEAD_MAX_BANNED 64
#define CRAG_LM_HEAD_MAX_ELEMS 32760
int64_t crag_enc_decode_workspace_bytes(int n_seqs, int hq, int max_len);
int crag_enc_decode_attention(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                              const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                              int max_len, const int32_t *h_slots, const int32_t *h_cache_len, int n_seqs, int hq, int hkv,
                              float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                              void *stream);
int crag_enc_decode_attention_shared(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                                     const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                                     int max_len, const int32_t *h_slots, const int32_t *h_cache_len,
                                     const int32_t *h_parent, const int32_t *h_shared_len, int n_seqs, int hq, int hkv,
                                     float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                                     void *stream);
int crag_enc_decode_attention_rows(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                                   const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                                   int max_len, const int32_t *h_slots, const int32_t *h_cache_len, const int32_t *h_new_len,
                                   const int32_t *h_parent, const int32_t *h_shared_len, int n_seqs, int hq, int hkv,
                                   float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                                   void *stream);
int crag_enc_lm_head(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                     const uint16_t *lm_head, float *logits, int32_t *token, const int32_t *banned, int n_banned,
                     int n_rows, int hidden, int64_t vocab, float eps, void *stream);

/* ---- continuing cached sequences: csrc/crag_extend.hip ----
 *
 * crag_enc_extend_attention: h_new_len[b] >= 1 new tokens for each of n_seqs (1..CRAG_DECODE_MAX_SEQS) sequences, over
 *   the cache of ONE layer (the layout above).  Sequence b sits in slot h_slots[b] and holds h_cache_len[b] >= 0 tokens;
 *   its new rows lie back to back, in the order of the sequences, in qkv_new [T_new, (hq + 2 hkv) * 128] (raw fused
 *   projections, not modified; T_new = the sum of h_new_len) and in out [T_new, hq * 128] bf16.  h_slots / h_cache_len /
 *   h_new_len are HOST arrays.
 *   New row i of sequence b has position cache_len + i.  q/k RMSNorm + RoPE with the arithmetic and the roundings of
 *   crag_enc_qk_norm_rope; the key and the raw value are stored at row cache_len + i of the slot -- the bits prefill
 *   and crag_enc_decode_attention would have appended -- and the rotated query goes to the workspace.  Query row i
 *   then sees the keys 0 .. cache_len + i of its slot: causal GQA flash attention on bf16 MFMA with fp32 online
 *   softmax, one workgroup per (kv head, block of CRAG_EXTEND_BLOCK query rows of one sequence), its waves the hq / hkv
 *   = 2 or 4 query heads, walking tiles of CRAG_EXTEND_TILE keys read in place from the cache.  No cache row at or
 *   beyond cache_len + new_len is read, nothing beyond max_len.  A sequence with at most CRAG_EXTEND_SPLIT_ROWS new
 *   rows cuts the keys of a query block into splits of CRAG_EXTEND_SPLIT keys, one workgroup each, combined in
 *   ascending split order by a third kernel.  No atomics, and a sequence's output bits and appended bits depend on
 *   its own data alone -- not on n_seqs, the slot or the other sequences.
 *   workspace: crag_enc_extend_workspace_bytes(n_seqs, hq, max_new_rows, max_len) bytes of device scratch, 16-byte
 *   aligned, max_new_rows >= T_new.
 *   CRAG_EINVAL, nothing enqueued: a NULL pointer, n_seqs outside 1..8, hq / hkv not 2 or 4, new_len < 1, cache_len < 0,
 *   cache_len + new_len > max_len or > max_pos (the rows of cos_sin), a slot outside 0..n_slots - 1 or named twice in
 *   the call, a misaligned pointer.  CRAG_E2BIG: the workspace is too small. */
#define CRAG_EXTEND_BLOCK 32
#define CRAG_EXTEND_TILE 32
#define CRAG_EXTEND_SPLIT 512
#define CRAG_EXTEND_SPLIT_ROWS 512
int64_t crag_enc_extend_workspace_bytes(int n_seqs, int hq, int max_new_rows, int max_len);
int crag_enc_extend_attention(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                              const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                              int max_len, const int32_t *h_slots, const int32_t *h_cache_len, const int32_t *h_new_len,
                              int n_seqs, int hq, int hkv, float eps, float scale, void *workspace,
                              int64_t workspace_bytes, uint16_t *out, void *stream);

/* ---- greedy selection under a byte automaton: csrc/crag_grammar.hip ----
 *
 * Serves the reference's Phase 5, item 2 (PHASED_PLAN.md: every sentence of an answer cites evidence ids of the pack):
 * the decoder can only produce token sequences whose bytes a deterministic byte automaton accepts.
 *
 * The automaton: class_of [256] (byte -> class < n_classes), trans [n_states, n_classes] uint16 (the next state;
 *   CRAG_GRAMMAR_DEAD = no way on), accept [n_states] (non-zero: a stop token is allowed here).
 * The tokens: tok_offsets [vocab + 1] into tok_bytes (the raw bytes of every id, back to back), tok_kind [vocab]:
 *   0 an ordinary token, walked byte by byte; 1 a stop token; 2 never allowed.
 * crag_enc_grammar_argmax: per row r < n_rows (1..CRAG_DECODE_MAX_SEQS), with s = state[r] (device, in/out): token t
 *   is allowed when kind[t] == 1 and accept[s], or kind[t] == 0, t has at least one byte and the walk of its bytes
 *   from s never meets CRAG_GRAMMAR_DEAD (nor an index outside the tables).  token[r] = the lowest id among the maxima
 *   of logits[r] ([n_rows, vocab] fp32) over the allowed tokens, NaNs left out -- crag_enc_lm_head's tie rule -- and
 *   state[r] becomes the end state of its walk (unchanged for a stop token).  Nothing allowed, or s outside
 *   0..n_states - 1: token[r] = -1, state[r] unchanged.  allowed_bits (nullable) [n_rows, ceil(vocab / 32)]: bit
 *   t % 32 of word t / 32 is the allowed flag of token t, the bits at and beyond vocab zero.
 *   One workgroup per row; no atomics; a row's results depend on its own logits and state alone.
 *   CRAG_EINVAL, nothing enqueued: a NULL pointer (allowed_bits excepted), n_rows outside 1..8, n_states outside
 *   1..CRAG_GRAMMAR_MAX_STATES, n_classes outside 1..CRAG_GRAMMAR_MAX_CLASSES, vocab outside 1..2^31 - 1, a pointer
 *   that is not aligned to its element. */
#define CRAG_GRAMMAR_MAX_STATES 4096
#define CRAG_GRAMMAR_MAX_CLASSES 64
#define CRAG_GRAMMAR_DEAD 0xFFFF
int crag_enc_grammar_argmax(const float *logits, int64_t vocab, const int32_t *tok_offsets, const uint8_t *tok_bytes,
                            const uint8_t *tok_kind, const uint8_t *class_of, const uint16_t *trans, const uint8_t *accept,
                            int n_states, int n_classes, int32_t *state, int32_t *token, uint32_t *allowed_bits, int n_rows,
                            void *stream);

/* ---- seeded sampling: csrc/crag_sample.hip ----
 *
 * crag_enc_sample: per row r < n_rows (1..CRAG_DECODE_MAX_SEQS) of logits [n_rows, vocab] fp32, one token drawn from the
 *   row's softmax at temperature T = h_temperature[r] under the cuts h_top_k[r], h_top_p[r] and h_min_p_cut[r].  The h_*
 *   arrays are HOST arrays of n_rows entries; seed and step hold for the whole call.
 *   Candidates: the ids whose bit is set in allowed_bits[r] ([n_rows, ceil(vocab / 32)], crag_enc_grammar_argmax's layout;
 *   NULL: every id) and whose logit is neither NaN nor -inf.  m = their maximum.
 *     no candidate          token -1, kept 0, cut NaN
 *     m == +inf, or T == 0  token = the lowest id holding m (crag_enc_lm_head's rule), kept = the ids holding m, cut = m
 *   Otherwise every cut is a threshold on the logit, so equal logits stay together (-0 == +0):
 *     t_k   the top_k-th largest candidate logit (top_k == 0, or no more candidates than top_k: none)
 *     t_m   (l - m) >= min_p_cut in fp32; the host passes fp32(T * ln min_p), -inf for min_p == 0
 *     t_p   inside S = {l >= t_k, t_m holds}, with w = exp((l - m) / T): the largest logit value such that the weights of
 *           the logits >= t_p reach top_p of the weights of S (top_p == 1: none).  The weights are summed as 64-bit
 *           fixed-point integers (unit 2^-40), so the sums do not depend on any order.
 *   The kept ids are those of S at or above t_p; kept[r] (nullable) is their number and cut[r] (nullable) the lowest
 *   kept logit.  The draw is the Gumbel maximum: u_i = ((x0 >> 8) + 0.5) * 2^-24 with x0 = word 0 of Philox4x32-10,
 *   key (seed lo, seed hi), counter (i, step, h_stream[r], 0); key_i = (l_i - m) / T - ln(-ln u_i); token[r] = the kept
 *   id with the largest key, the lowest id among equals.
 *   One workgroup per row; integer atomics on LDS only; the same inputs give the same token, kept and cut bits on every
 *   run, and a row's outputs depend on its own logits, bits and parameters alone -- not on n_rows or its position.
 *   CRAG_EINVAL, nothing enqueued: a NULL pointer (allowed_bits, kept and cut excepted), n_rows outside 1..8, vocab
 *   outside 1..2^31 - 1, a temperature that is neither 0 nor in CRAG_SAMPLE_MIN_TEMPERATURE..CRAG_SAMPLE_MAX_TEMPERATURE,
 *   top_k outside 0..vocab, top_p outside (0, 1], min_p_cut > 0 or NaN, a device pointer not aligned to 4 bytes.
 * crag_enc_grammar_advance: per row r < n_rows, one lane each: state[r] (device, in/out) becomes the state behind the
 *   bytes of token[r] walked from it, with crag_enc_grammar_argmax's tables and its checks before every table read.
 *   The state stays for a stop token, for -1, for an id outside 0..vocab - 1, for a state outside the table and for a
 *   token the state does not allow (kind 2, no bytes, a walk that dies).  Under a grammar the decoder samples among
 *   allowed_bits and then calls this: the state crag_enc_grammar_argmax leaves is the one behind ITS token.
 *   CRAG_EINVAL, nothing enqueued: a NULL pointer, n_rows / n_states / n_classes / vocab outside their ranges (as
 *   above), a pointer that is not aligned to its element. */
#define CRAG_SAMPLE_MIN_TEMPERATURE 0.01f
#define CRAG_SAMPLE_MAX_TEMPERATURE 100.0f
int crag_enc_sample(const float *logits, int64_t vocab, const uint32_t *allowed_bits, const float *h_temperature,
                    const int32_t *h_top_k, const float *h_top_p, const float *h_min_p_cut, const uint32_t *h_stream,
                    uint64_t seed, uint32_t step, int32_t *token, int32_t *kept, float *cut, int n_rows, void *stream);
int crag_enc_grammar_advance(const int32_t *tok_offsets, const uint8_t *tok_bytes, const uint8_t *tok_kind, int64_t vocab,
                             const uint8_t *class_of, const uint16_t *trans, int n_states, int n_classes, int32_t *state,
                             const int32_t *token, int n_rows, void *stream);

/* ---- token log-probabilities: csrc/crag_logprobs.hip ----
 *
 * crag_enc_logprobs: per row r < n_rows (1..CRAG_DECODE_MAX_SEQS) of logits [n_rows, vocab] fp32, the model's own
 *   distribution (temperature 1, no cut) at the id token[r] (device int32), whatever picked that id.
 *   A CANDIDATE is an id whose logit is not NaN (-inf is one); an ALLOWED candidate has its bit set in allowed_bits[r]
 *   ([n_rows, ceil(vocab / 32)], crag_enc_grammar_argmax's layout; NULL: every candidate).  m_all / m_alw = the maximum
 *   logit of the two sets.  Every output is a device array; all but logprob are nullable.
 *     lse_all[r]      m_all + ln sum exp(l - m_all) over the candidates
 *     lse_allowed[r]  the same over the allowed candidates, relative to m_alw: finite however far they lie below m_all
 *                     (lse_allowed - lse_all <= 0 is the log of the probability mass a grammar left allowed)
 *                     Either: -inf for an empty set and for a set of -inf alone, +inf for a set whose maximum is +inf.
 *     logprob[r]      l_token - lse_all[r] in fp32, by IEEE rules (finite - +inf = -inf, inf - inf = NaN); NaN when
 *                     token[r] is outside 0..vocab - 1 or its logit is NaN
 *     rank[r]         int32, 1 + the candidates whose logit is strictly greater than l_token (-0 == +0); 0 for a token
 *                     outside 0..vocab - 1 or with a NaN logit
 *     top_id [n_rows, n_top] int32 / top_logprob [n_rows, n_top] fp32: the n_top (0..CRAG_LOGPROBS_MAX_TOP) first
 *                     candidates -- of all ids, not of the allowed ones -- in the order (logit descending, id
 *                     ascending), each with l - lse_all[r]; a row with fewer candidates is padded with id -1 and NaN.
 *   The weights are expf(l - m) summed as 64-bit fixed-point integers (unit 2^-40; crag_enc_sample's coarser unit for a
 *   vocabulary whose sum would not fit), the counts integer sums, the top entries an exact selection on the
 *   order-preserving key of the logit.  One workgroup per row; integer adds on LDS are the only atomics; every store is
 *   a plain vector store.  The same inputs give the same bits on every run, and a row's outputs depend on its own
 *   logits, bits and token alone -- not on n_rows or its position.
 *   CRAG_EINVAL, nothing enqueued: a NULL logits, token or logprob; n_rows outside 1..8; vocab outside 1..2^31 - 1;
 *   n_top outside 0..CRAG_LOGPROBS_MAX_TOP or above vocab; n_top > 0 with top_id or top_logprob NULL; a pointer that is
 *   not aligned to its element. */
#define CRAG_LOGPROBS_MAX_TOP 16
int crag_enc_logprobs(const float *logits, int64_t vocab, const uint32_t *allowed_bits, const int32_t *token,
                      float *logprob, float *lse_all, float *lse_allowed, int32_t *rank, int32_t *top_id,
                      float *top_logprob, int n_top, int n_rows, void *stream);

/* ---- repetition control: csrc/crag_penalty.hip ----
 *
 * crag_enc_adjust_logits: per row r < n_rows (1..CRAG_DECODE_MAX_SEQS) of logits [n_rows, vocab] fp32, the logits a
 *   caller that wants the model to move away from what it has said picks its next token from, and the greedy token on
 *   them.  out [n_rows, vocab] fp32 may be logits itself.  The rule, operation by operation, is
 *   cadence_rag_amd/penalties.py (adjust_host); the kernel gives its bits.
 *   history [n_history_rows, history_stride] int32 (device) is a token log: row r reads the first h_total_len[r] ids of
 *   log row h_history_row[r] -- H, of which the first h_prompt_len[r] are the prompt P and the rest the output O.  Two
 *   rows may name one log row with different lengths (a sequence's rows under speculation).  An id of the log outside
 *   0..vocab - 1 is ignored.  seen(t): t occurs in H; c(t): how often t occurs in O.  The h_* arrays are HOST arrays of
 *   n_rows entries, h_bias_offsets of n_rows + 1.  Per id t, from l = logits[r][t]:
 *     1. unless bit t % 32 of exempt_bits[t / 32] is set (device, [ceil(vocab / 32)], shared by the rows; NULL: no id):
 *        a. seen(t) and h_repetition[r] != 1:  l = l / rp when l > 0, else l * rp -- one correctly rounded operation; a
 *           NaN takes the else arm
 *        b. c(t) > 0:  l = (l - fp32(h_frequency[r] * fp32(c))) - h_presence[r] -- three roundings, never a fused
 *           multiply-add
 *        c. n = h_ngram[r] > 0 and some j with j + n - 1 < |O| has O[j .. j+n-2] equal to the last n - 1 ids of O and
 *           O[j+n-1] == t:  l = -inf
 *     2. t == bias_ids[k] for a k in h_bias_offsets[r] .. h_bias_offsets[r + 1] - 1:  l = l + bias_values[k].  bias_ids /
 *        bias_values are device arrays, the ids of a row's slice strictly ascending inside 0..vocab - 1; the three are
 *        NULL together: no bias.
 *   token[r] (device int32) = the lowest id among the maxima of out[r], NaNs left out, -1 when nothing is left:
 *   crag_enc_lm_head's rule.
 *   One workgroup per row, which zeroes a [vocab] int32 slice of the workspace, scatters the history, the n-gram
 *   continuations and the bias flags into it and walks the vocabulary once; the history has no cap.  Integer atomics on
 *   the row's own slice are the only atomics, every store is a plain vector store.  The same inputs give the same bits
 *   on every run, and a row's out bits and token depend on its own logits, history and parameters alone -- not on
 *   n_rows or its position.
 *   workspace: crag_enc_adjust_workspace_bytes(n_rows, vocab) bytes of device scratch, 16-byte aligned (0: n_rows or
 *   vocab out of range).  A row is read 16 bytes at a time from its first 16-byte aligned id on; out is stored that way
 *   when its rows have the misalignment of the logits rows (out == logits, or two tensors of one shape).
 *   CRAG_EINVAL, nothing launched: a NULL pointer (exempt_bits and the three bias arrays excepted, those three only
 *   together), n_rows outside 1..8, vocab outside 1..2^31 - 1, a repetition penalty outside CRAG_ADJUST_MIN_REPETITION..
 *   CRAG_ADJUST_MAX_REPETITION, a frequency or presence penalty outside -CRAG_ADJUST_MAX_ADDITIVE..
 *   CRAG_ADJUST_MAX_ADDITIVE (a NaN is outside), an n-gram size that is neither 0 nor in 2..CRAG_ADJUST_MAX_NGRAM,
 *   prompt_len > total_len, total_len > history_stride, a negative length, a history row outside the log, a bias slice
 *   longer than CRAG_ADJUST_MAX_BIAS, offsets that do not rise from 0, bias ids not strictly ascending or outside the
 *   vocabulary (a call with bias entries reads the ids back with one small synchronous copy to see them; one without
 *   makes no copy), a device pointer not aligned to 4 bytes, a workspace not aligned to 16.  CRAG_E2BIG: the workspace is too small. */
#define CRAG_ADJUST_MIN_REPETITION 0.1f
#define CRAG_ADJUST_MAX_REPETITION 10.0f
#define CRAG_ADJUST_MAX_ADDITIVE 2.0f
#define CRAG_ADJUST_MAX_NGRAM 8
#define CRAG_ADJUST_MAX_BIAS 256
int64_t crag_enc_adjust_workspace_bytes(int n_rows, int64_t vocab);
int crag_enc_adjust_logits(const float *logits, float *out, int64_t vocab, const int32_t *history, int64_t history_stride,
                           int n_history_rows, const int32_t *h_history_row, const int32_t *h_prompt_len,
                           const int32_t *h_total_len, const float *h_repetition, const float *h_frequency,
                           const float *h_presence, const int32_t *h_ngram, const uint32_t *exempt_bits,
                           const int32_t *bias_ids, const float *bias_values, const int32_t *h_bias_offsets,
                           int32_t *token, void *workspace, int64_t workspace_bytes, int n_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRAG_ENCODER_H */
