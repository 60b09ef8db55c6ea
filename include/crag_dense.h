/*
 * crag_dense.h — C ABI of the MI355X-native dense-retrieval lane (libcrag_dense.so).
 *
 * This is the drop-in boundary for the reference's dense path.  The reference has no FFI
 * today: its "interface" for this path is (a) the pgvector SQL issued by
 *   _fetch_chunks_dense        /root/reference/app/retrieve.py:326-354
 *   _fetch_artifacts_dense     /root/reference/app/retrieve.py:357-389
 *   _estimate_dense_candidates /root/reference/app/retrieve.py:303-323
 * and the per-row `UPDATE … SET embedding = CAST(:lit AS vector(1024))` of
 *   _update_embeddings         /root/reference/app/embedding_pipeline.py:149-168
 * and (b) the HTTP embedding gateway behind embed_texts
 *                              /root/reference/app/embeddings.py:48-82
 * (gateway math: P620_TRITON_QWEN3_4B_EMBEDDING_RUNBOOK.md:683-716).
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success and a negative CRAG_E* code on error
 * (never throws); crag_last_error() returns a thread-local message for the last failure on
 * the calling thread.  Plain pointers and sizes only — no torch / HIP types.  "dev" pointers
 * are device (HBM) addresses on the index's device; `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  The library owns the device corpus.
 */
#ifndef CRAG_DENSE_H
#define CRAG_DENSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRAG_OK 0
#define CRAG_EINVAL (-1)   /* bad argument */
#define CRAG_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define CRAG_ENOMEM (-3)   /* capacity exceeded / allocation failed */
#define CRAG_E2BIG (-5)    /* an input exceeds what one call takes; the caller splits it (crag_tech_lane_host) */
#define CRAG_ENODEV (-4)   /* no usable gfx950 device */

#define CRAG_MAX_K 128     /* reference uses k = 50 / 10 (retrieve.py:18-19); BASELINE asks 10..100 */
#define CRAG_DIM 1024      /* vector(1024): alembic/versions/0001_initial_schema.py:87 */

typedef struct crag_index crag_index;

const char *crag_last_error(void);
const char *crag_version(void);
/* Number of HIP devices visible (0 if none / no driver). */
int crag_device_count(void);

/* ---- corpus: replaces the pgvector `embedding vector(1024)` column + its scan ---------- */

/* Allocate an empty index for up to `capacity` rows of `dim` (<= 1024) floats on `device`.
 * Replaces: the table column + HNSW/seq-scan storage (0001_initial_schema.py:87,98-102).
 * HBM per row: 4 KiB (the fp32 row, source of truth) + 2 KiB (fp16 mirror of the unit row, what the prefilter scan
 * streams) + 12 bytes.  Environment, read once here: CRAG_NO_FP16_MIRROR=1 leaves the mirror out (the prefilter scan
 * then streams the fp32 rows: twice the bytes per search, two thirds of the footprint); CRAG_NO_PREFILTER=1 keeps
 * every search on the exact fp32 MFMA scan.  Results are bit-identical in all three modes.  (Developer switches,
 * same place: CRAG_PF_NT=0/1 and CRAG_PF_NT_ABOVE_MB=<n> override when the mirror scan uses the streaming cache
 * policy -- by default for mirrors above 1.5 GB; CRAG_PF_WAITS=tile|fragment forces the wait schedule of the
 * mirror scan's loads -- by default per-fragment waits for a mirror the Infinity Cache holds, see
 * crag_index_scan_waits.) */
int crag_index_create(int device, int dim, int64_t capacity, crag_index **out);
int crag_index_destroy(crag_index *ix);

/* Append n rows ([n, dim] row-major fp32; host OR device pointer, detected) with their
 * 64-bit ids (NULL => consecutive ids continuing from the current size).  ids must be strictly
 * ascending and above every id already stored (CRAG_EINVAL otherwise, nothing is stored): the
 * backfill feeds rows `ORDER BY id` (embedding_pipeline.py:136), and this is what makes the search
 * order below "descending score, then ascending id".  A row embedded late (its id below the stored
 * maximum) goes in through crag_index_insert.
 * Rows with a zero or non-finite norm are stored but never returned (pgvector gives them a NaN
 * distance).
 * Replaces: _update_embeddings' per-row UPDATE (embedding_pipeline.py:157-168).
 * Appending is safe while searches enqueued earlier with crag_index_search_async are still running (they
 * never read past the size they were launched with); crag_index_update rewrites rows in place and must
 * not overlap in time with searches in flight on other streams -- those of crag_index_search_pipelined run on
 * streams of the index's own: crag_index_join + a synchronisation of the joined stream come first. */
int crag_index_add(crag_index *ix, const float *rows, const int64_t *ids, int64_t n);

/* Overwrite the vectors of rows [pos, pos+n) (positions, not ids; host OR device pointer) — re-embed in place.
 * pos < 0, n < 0, pos + n > size or rows == NULL with n > 0 give CRAG_EINVAL and change nothing; n == 0 is CRAG_OK.
 * Afterwards the index is what a fresh build, with crag_index_add, from the resulting rows would be: the same
 * crag_index_get_rows, every search the same ids / scores / counts bit for bit, the same crag_index_count_eligible and
 * the same scan kernel chosen -- an index whose only row with a norm outside [1e-30, 1e30] is overwritten by an
 * ordinary one returns to the prefilter path, one that receives such a row leaves it. */
int crag_index_update(crag_index *ix, int64_t pos, const float *rows, int64_t n);

/* ---- in-place edits.  After any of the three the index is indistinguishable from one built fresh, with
 * crag_index_add, from the same rows in id order: same size and ids, crag_index_get_rows bit-exact, every search path
 * the same ids / scores / counts bit for bit, the same scan kernel chosen, the same crag_index_count_eligible, the same
 * next crag_index_add accepted.  Rows that stay are copied through the layout (fp32 pieces, fp16 mirror pieces,
 * 1/||row||, id), never recomputed; rows in front of the first changed position are not touched; vacated positions
 * return to the state crag_index_create leaves them in.  The move works in chunks of CRAG_EDIT_CHUNK_ROWS destination
 * rows (environment, a multiple of 32, read once at crag_index_create; default 16384) through a bounce buffer of at
 * most 128 MiB that is held only during the call.
 * All three are synchronous like crag_index_add, take the index's lock and WAIT FOR EVERY SEARCH IN FLIGHT on the index
 * before the first row moves -- the searches of crag_index_search_async on the callers' streams (the workspaces'
 * streams) and those of crag_index_search_pipelined on the index's own pipe streams: the device is synchronised.  A
 * search enqueued after the call returns sees the edited index.  size is right afterwards and the largest stored id is
 * that of the last row, or none when the index is empty (an emptied index accepts ids from any value again).  n == 0
 * is CRAG_OK.  Mixed remove-and-insert in one call does not exist: call one after the other. */

/* Remove the rows whose ids are listed (host OR device pointer, any order, repeats allowed; ids that are not stored are
 * ignored).  out_removed (nullable) receives the number of rows actually removed.
 * Replaces: what `calls(call_id) ON DELETE CASCADE` does to chunks, analysis_artifacts and artifact_chunks
 * (alembic/versions/0001_initial_schema.py:59,79,123, 0006_add_artifact_chunks.py:23-24): a call deleted or re-ingested
 * upstream takes its rows with it. */
int crag_index_remove(crag_index *ix, const int64_t *ids, int64_t n, int64_t *out_removed);

/* The same by position: keep_mask is a HOST pointer in the row_mask encoding over the current size (bit (i & 7) of byte
 * i >> 3 = row at position i; 4-byte aligned, ceil(size/32)*4 bytes, bits beyond size ignored); a cleared bit removes
 * the row.  out_size (nullable) receives the new size.  Same reference lines as crag_index_remove (the caller has
 * resolved the cascade to row positions already, as DenseTable.delete_calls does). */
int crag_index_compact(crag_index *ix, const uint8_t *keep_mask, int64_t *out_size);

/* Insert n rows whose ids may lie anywhere between the stored ones (rows / ids: host OR device pointers; ids strictly
 * ascending, CRAG_EINVAL otherwise).  An id that is stored already gives CRAG_EINVAL, a size above the capacity
 * CRAG_ENOMEM -- both are checked before anything moves, the index is unchanged.  Ids that all lie above the largest
 * stored id take exactly the crag_index_add route.
 * Replaces: _update_embeddings' per-row `UPDATE ... SET embedding` (app/embedding_pipeline.py:149-168) for rows that
 * arrive in arbitrary id order -- the backfill embeds whichever rows are NULL, and a row embedded late has an id below
 * the stored maximum. */
int crag_index_insert(crag_index *ix, const float *rows, const int64_t *ids, int64_t n);

/* Rows currently stored / capacity / dim. */
int64_t crag_index_size(const crag_index *ix);
int64_t crag_index_capacity(const crag_index *ix);
int crag_index_dim(const crag_index *ix);

/* Copy rows [pos, pos+n) back out as [n, dim] row-major fp32 (host or device pointer) and,
 * if ids != NULL, their ids.  Bit-exact with what was added (the corpus is stored raw). */
int crag_index_get_rows(crag_index *ix, int64_t pos, int64_t n, float *rows, int64_t *ids);

/* Number of rows that can be returned for a (shared, nullable) mask: rows with a finite
 * non-zero norm whose mask bit is set.  Replaces: _estimate_dense_candidates' COUNT(*)
 * (retrieve.py:303-323).  mask: host or device pointer. */
int crag_index_count_eligible(crag_index *ix, const uint8_t *row_mask, int64_t *out_count);

/* Exact cosine top-k, synchronous; every pointer may be host or device (detected).
 *   queries     [nq, dim] row-major fp32 (need not be normalised)
 *   row_mask    nullable.  Bit (i & 7) of byte row_mask[q*mask_stride + (i >> 3)] set =>
 *               row at position i is eligible for query q.  mask_stride = 0 => one mask
 *               shared by all queries; otherwise a multiple of 4 bytes >= ceil(size/32)*4.
 *               Base address 4-byte aligned.  (Encodes _build_filter_clause, retrieve.py:93-120.)
 *   out_ids     [nq, k]  best first; -1 padded
 *   out_scores  [nq, k]  cosine similarity = 1 - (embedding <=> q), clamped to [-1, 1]; NaN padded
 *   out_counts  [nq]     valid entries per query (<= k)
 * Order: descending score, equal scores by ascending id (crag_index_add keeps ids
 * ascending with the row position, so the scan breaks ties on the position).  The reference SQL has
 * no tie-break at all.
 * Replaces: _fetch_chunks_dense / _fetch_artifacts_dense `ORDER BY embedding <=> q LIMIT k`
 * (retrieve.py:339-353, 369-388). */
int crag_index_search(crag_index *ix, const float *queries, int nq, int k,
                      const uint8_t *row_mask, int64_t mask_stride, int64_t *out_ids,
                      float *out_scores, int32_t *out_counts);

/* Same, all pointers DEVICE, enqueued on `stream` with no host synchronisation (the form
 * bench.py, the multi-GPU lane and hipGraph capture use). */
int crag_index_search_async(crag_index *ix, const float *d_queries, int nq, int k,
                            const uint8_t *d_row_mask, int64_t mask_stride, int64_t *d_out_ids,
                            float *d_out_scores, int32_t *d_out_counts, void *stream);

/* Throughput form of crag_index_search_async for ONE caller stream that issues a run of INDEPENDENT searches (a
 * batch job: the eval harness, bulk re-ranking, bench.py): consecutive calls take turns on three streams the index
 * owns (CRAG_PIPE_STREAMS=1..4) -- each with its own workspace --, so that the small kernels of one search (query
 * preparation, selection) run beside the scan of another; an in-order stream leaves most of the chip idle during them
 * (12 of 48 us per search at 100 000 rows x 64 queries, k = 10: 40 us per step pipelined).  Searches with k > 24 gain
 * nothing from it (their scans disturb each other's bound exchange) and run in stream order on the caller's stream.  What the caller gives up is the stream order between a search and what follows:
 *   * the OUTPUTS of a call are defined on `stream` only behind crag_index_join(ix, stream) (which makes `stream`
 *     wait for every pipelined search issued so far; it does not block the host);
 *   * flags & CRAG_PIPE_INPUTS_READY: the caller states that queries / row_mask are complete in memory when the call
 *     is made (resident inputs); without it the library orders its internal stream behind everything enqueued on
 *     `stream` so far (one event per call).
 * Results are the same bits as crag_index_search_async's.  Same reference call sites as crag_index_search
 * (retrieve.py:339-353, 369-388); the reference itself runs one query per request and has no counterpart. */
#define CRAG_PIPE_INPUTS_READY 1
int crag_index_search_pipelined(crag_index *ix, const float *d_queries, int nq, int k,
                                const uint8_t *d_row_mask, int64_t mask_stride, int64_t *d_out_ids,
                                float *d_out_scores, int32_t *d_out_counts, void *stream, int flags);
int crag_index_join(crag_index *ix, void *stream);

/* Near-duplicate suppression of ranked lists (hybrid /retrieve: the fused list of a side before it reaches the reranker
 * and the evidence pack).  Stands in for: the redundancy control the reference plans but has NO code for yet --
 * PHASED_PLAN.md:299-303 "enforce per-call diversity caps and dedupe rules" and IMPLEMENTATION_PLAN.md:150-158 "Top
 * evidence is not overly redundant (dedupe + per-call caps)"; the per-call cap exists on both sides, the dedupe rule is
 * defined here.  Per query the list is walked in rank order: item i is DROPPED iff some KEPT item j < i has
 * cos(row_i, row_j) >= threshold, else kept (greedy over the kept set: a ~ b, b ~ c, a !~ c keeps a and c).  An id that
 * is not stored, the -1 pad and a stored row with a zero or non-finite norm are always kept and never suppress; a
 * repeated id is a pair like any other (cosine 1 with itself).
 *   cos(i, j) = clamp(dot(i, j) * (inv_norm[i] * inv_norm[j]), -1, 1), dot a fixed-order fp32 accumulation over the raw
 *   stored rows: cos(i, j) and cos(j, i) are the same bits, which depend on the two rows only (not on the slot, width,
 *   nq or the rows' positions).  They need not equal the bits of a search score.
 *   d_ids [nq, width] best first; d_counts [nq], clamped to [0, width] -- the shape crag_rrf_fuse emits
 *   threshold       finite, in (-1, 1]
 *   d_out_ids [nq, width]     the kept ids in their original order, -1 padded (may be d_ids itself)
 *   d_out_counts [nq]         (may be d_counts itself)
 *   d_out_dup_of [nq, width]  nullable: per INPUT slot -1 if the item is kept (or lies beyond the count), else the input
 *                             slot of the item that suppressed it (the lowest kept one at or above the threshold)
 *   d_out_sim [nq, width]     nullable: that pair's cosine, NaN where the item is kept
 * All pointers DEVICE; one launch on `stream`, no host synchronisation, no workspace of the index.  Ordering against
 * edits as for crag_index_search_async (edits synchronise the device first).
 * CRAG_EINVAL, nothing enqueued: NULL index or required pointer, nq < 0, width < 1, width > CRAG_DEDUPE_MAX_WIDTH, a
 * non-finite or out-of-range threshold.  nq == 0 is CRAG_OK. */
#define CRAG_DEDUPE_MAX_WIDTH 256
int crag_index_dedupe_async(crag_index *ix, const int64_t *d_ids, const int32_t *d_counts, int nq, int width,
                            float threshold, int64_t *d_out_ids, int32_t *d_out_counts,
                            int32_t *d_out_dup_of, float *d_out_sim, void *stream);

/* Exact cosine top-k and scores over LISTED rows: the id_subset half of search(query_vecs, k, row_mask|id_subset).  Only
 * the listed rows are read (4 KiB each), where a masked search streams the whole table.
 * Replaces: the reference's "exact" dense mode -- _choose_dense_mode (retrieve.py:277-287) answers "exact" for a scoped
 * request whose filters pass at most EMBEDDINGS_EXACT_SCAN_THRESHOLD rows, and `ORDER BY embedding <=> q LIMIT k`
 * (retrieve.py:339-353) then reads those rows only -- and serves the exact cosine of a query with rows another lane found
 * (BM25 / exact-token hits for the debug lanes, reranker features).
 *   d_queries [nq, dim] fp32, raw
 *   d_ids     [nq, width] int64 when list_stride == width; ONE [width] list shared by all queries when list_stride == 0
 *             (as mask_stride == 0 means a shared mask)
 *   d_counts  [nq] ([1] for a shared list), clamped to [0, width]
 *   d_out_ids [nq, k] (-1 pad), d_out_scores [nq, k] (NaN pad), d_out_counts [nq]: EXACTLY what crag_index_search_async
 *             returns for the same queries and k under a mask whose set bits are the positions of the listed ids -- ids,
 *             score bits and counts; descending score, then ascending id.
 *   d_out_slot_scores  nullable [nq, width]: per INPUT slot the score of (query, that id), the same bits; NaN where the
 *             slot lies beyond the count or the pair is ignored.  A repeated id receives its score in every slot it holds.
 *   d_scratch crag_index_search_ids_scratch_bytes(nq, width) bytes, 8-byte aligned, owned by the caller, one per stream in
 *             use (as for crag_bm25_lane_host)
 * A list is a set: its order and repeated ids change nothing in the top-k outputs.  An id that is not stored, the -1 pad, a
 * row with a zero or non-finite norm and every row for a zero or non-finite query are ignored (the count falls
 * accordingly).  The score of a (query, row) pair depends on those two alone: not on the slot, width, nq, k, shared or
 * per-query lists, the row's position or the row layout (with or without the fp16 mirror).
 * All pointers DEVICE; two launches on `stream`, no host synchronisation, no allocation, no workspace of the index.
 * Ordering against edits as for crag_index_dedupe_async (edits synchronise the device first).  An empty index is valid:
 * every count is 0.
 * CRAG_EINVAL, checked before any HIP call, nothing enqueued: NULL index or required pointer, nq < 0 (or > 65535),
 * width < 1, k outside [1, CRAG_MAX_K], list_stride neither 0 nor width, scratch too small or not 8-byte aligned.
 * CRAG_E2BIG, nothing enqueued: width > CRAG_SUBSET_MAX_WIDTH -- the caller uses the row_mask route.  nq == 0 is CRAG_OK. */
#define CRAG_SUBSET_MAX_WIDTH 4096
int64_t crag_index_search_ids_scratch_bytes(int nq, int width);
int crag_index_search_ids_async(crag_index *ix, const float *d_queries, int nq, const int64_t *d_ids,
                                const int32_t *d_counts, int width, int64_t list_stride, int k, int64_t *d_out_ids,
                                float *d_out_scores, int32_t *d_out_counts, float *d_out_slot_scores, void *d_scratch,
                                int64_t scratch_bytes, void *stream);

/* Exact cosine top-k under a cap per group ("grouping search" / collapse with inner hits): per query the eligible rows
 * are ranked by (score descending, id ascending) -- scores and eligibility of crag_index_search: mask bit set, finite
 * non-zero row norm, finite non-zero query --, the ranking is walked, a row is kept iff its group holds fewer than
 * per_group kept rows, and the walk stops at k.  Equivalently: the top-k of the union of every group's own top-per_group.
 * The cap holds over the whole table, not over a prefix of the ranking.
 * Stands in for: the per-call quota the reference applies only when it packs evidence -- _pack keeps at most
 * DEFAULT_MAX_QUOTES_PER_CALL = 2 quotes per call (retrieve.py:829) of whatever `ORDER BY embedding <=> q LIMIT 50`
 * (retrieve.py:339-353) returned, so one long call can fill the dense lane -- and for what the reference plans but has
 * no code for: PHASED_PLAN.md:299-303 "enforce per-call diversity caps", IMPLEMENTATION_PLAN.md:150-158, and the
 * hierarchical strategy of APP_SPEC.md 9.2 / 9.5 (shortlist calls by their best chunk: per_group = 1, group = call).
 *   d_queries   [nq, dim] fp32, raw
 *   d_row_group [size] int32 by row POSITION: the row's group number.  A row whose number lies outside [0, n_groups) is
 *               ignored; its number is never used as an index.  The caller keeps the column in step with edits, as it does
 *               for masks (cadence_rag_amd.filters.FilterColumns.d_call_slot / n_calls is such a column).
 *   d_row_mask / mask_stride  exactly as in crag_index_search (nullable; shared or per query)
 *   d_out_ids [nq, k] (-1 pad), d_out_scores [nq, k] (NaN pad), d_out_groups nullable [nq, k] (-1 pad), d_out_counts [nq]
 *   d_scratch   crag_index_search_grouped_scratch_bytes(nq, n_groups, per_group) bytes (8 per (query, group, slot) + 4 per
 *               query), 8-byte aligned, owned by the caller, one per stream in use.  The call clears whatever it reads of
 *               it: a dirty or reused scratch is fine.
 * The score of a (query, row) pair is the same bits crag_index_search_async returns for that pair; it depends on the pair
 * alone: not on k, per_group, nq, the grouping, the mask form, the row's position or the row layout.  The outputs are a
 * function of the inputs alone, bit for bit, from run to run.
 * All pointers DEVICE; three launches on `stream`, no host synchronisation, no allocation, no workspace of the index.
 * Ordering against edits as for crag_index_search_ids_async.  An empty index is valid: every count is 0.
 * CRAG_EINVAL with a message that contains "search_grouped", checked before any HIP call, nothing enqueued: NULL index
 * or required pointer, nq < 0 (or > 65535), k outside [1, CRAG_MAX_K], per_group outside [1, CRAG_GROUP_MAX_PER],
 * n_groups < 1 or >= 2^31, a mask stride crag_index_search refuses, scratch too small or not 8-byte aligned.
 * nq == 0 is CRAG_OK. */
#define CRAG_GROUP_MAX_PER 8
int64_t crag_index_search_grouped_scratch_bytes(int nq, int64_t n_groups, int per_group);
int crag_index_search_grouped_async(crag_index *ix, const float *d_queries, int nq, int k, const int32_t *d_row_group,
                                    int64_t n_groups, int per_group, const uint8_t *d_row_mask, int64_t mask_stride,
                                    int64_t *d_out_ids, float *d_out_scores, int32_t *d_out_groups, int32_t *d_out_counts,
                                    void *d_scratch, int64_t scratch_bytes, void *stream);

/* Maximal marginal relevance (MMR) over ranked lists: the graded redundancy control of the dense lane, next to the two
 * hard gates (the per-call cap of crag_index_search_grouped_async, the cosine threshold of crag_index_dedupe_async).
 * Stands in for: the redundancy control the reference plans but has NO code for -- PHASED_PLAN.md:286-303 "improve
 * top-of-pack precision and reduce redundancy" and IMPLEMENTATION_PLAN.md:150-158.  Meant for lists whose relevance is
 * on the cosine scale (a search's scores, crag_index_search_ids_async's slot scores): relevance and pair similarity
 * are then one scale.
 *   d_ids [nq, width] int64, d_rel [nq, width] fp32 the relevance of each slot (any finite value is legal), d_counts
 *   [nq] clamped to [0, width] -- the shape crag_index_search_async and crag_rrf_fuse emit
 *   lambda  finite, in [0, 1];  mu = 1.0f - lambda, computed once in fp32;  k in [1, CRAG_MMR_MAX_WIDTH]
 * A slot is a CANDIDATE when it lies below the count, its id is not -1, its rel is finite and no earlier slot below the
 * count holds the same id; every other slot is ignored.  A candidate is COMPARABLE when its id is stored with
 * inv_norm > 0 (dedupe's eligibility); one that is not can be picked, is never penalised and never penalises anyone.
 * The walk, t = 0, 1, ... while t < k and candidates remain:
 *   value[i] = lambda * rel[i] - mu * pen[i]      three fp32 operations (mul, mul, sub), each rounded once, no contraction
 *   the candidate with the largest value is picked; equal values go to the lower id
 *   pen[i] = 0 until a picked comparable item p is compared with a comparable i: the first comparison sets
 *   pen[i] = sim(p, i), later ones pen[i] = max(pen[i], sim(p, i))
 * lambda = 1 therefore yields the candidates in (rel descending, id ascending) order: crag_index_search_ids_async's
 * order when rel holds its slot scores.
 *   sim(i, j) = the bits crag_index_dedupe_async reports for the pair: clamp(dot(i, j) * (inv_norm[i] * inv_norm[j]),
 *   -1, 1), the same fixed-order fp32 accumulation.  Symmetric; it depends on the two rows alone (not on the slot, width,
 *   nq, k, lambda or the row layout, with or without the fp16 mirror).
 * Outputs, per query, count = min(k, candidates):
 *   d_out_ids [nq, k]          the picks in pick order, -1 padded
 *   d_out_rel [nq, k]          their rel, NaN padded
 *   d_out_value [nq, k]        nullable: the winning value bits, NaN padded
 *   d_out_slots [nq, k]        nullable: the input slot of each pick, -1 padded
 *   d_out_sim_rows [nq, k, width]  nullable: for pick t, sim(pick, slot) for every slot; NaN where the pair is not
 *                              comparable or the slot is ignored; every cell of the rows t >= count is NaN
 *   d_out_counts [nq]
 *   d_scratch  crag_index_mmr_scratch_bytes(nq, width) bytes (the queries' pair-cosine matrices), 8-byte aligned, owned
 *              by the caller, one per stream in use.  The call overwrites whatever it reads of it.
 * All pointers DEVICE; two launches on `stream`, no host synchronisation, no allocation, no workspace of the index.  The
 * outputs are a function of the inputs alone, bit for bit, from run to run.  Ordering against edits as for
 * crag_index_dedupe_async.  An empty index is valid: nothing is comparable, the picks go by rel alone.
 * CRAG_EINVAL with a message that contains "mmr", checked before any HIP call, nothing enqueued: NULL index or required
 * pointer, nq < 0 (or > 65535), width < 1 or > CRAG_MMR_MAX_WIDTH, k outside [1, CRAG_MMR_MAX_WIDTH], a non-finite
 * lambda or one outside [0, 1], scratch too small or not 8-byte aligned.  nq == 0 is CRAG_OK and excuses nothing else. */
#define CRAG_MMR_MAX_WIDTH 256
int64_t crag_index_mmr_scratch_bytes(int nq, int width);
int crag_index_mmr_async(crag_index *ix, const int64_t *d_ids, const float *d_rel, const int32_t *d_counts,
                         int nq, int width, float lambda, int k,
                         int64_t *d_out_ids, float *d_out_rel, float *d_out_value, int32_t *d_out_slots,
                         float *d_out_sim_rows, int32_t *d_out_counts,
                         void *d_scratch, int64_t scratch_bytes, void *stream);

/* Merge per-shard results (the multi-GPU exchange step: each rank's [nq, k] top-k after an
 * RCCL all-gather) into the global top-k.  All pointers DEVICE.
 *   d_ids/d_scores/d_counts  [n_lists, nq, k] / [n_lists, nq, k] / [n_lists, nq]
 * Same ordering rule as crag_index_search (score desc, id asc). */
int crag_merge_topk(int device, const int64_t *d_ids, const float *d_scores,
                    const int32_t *d_counts, int n_lists, int nq, int k, int64_t *d_out_ids,
                    float *d_out_scores, int32_t *d_out_counts, void *stream);

/* One-collective form of the exchange step.  A "result record" holds one rank's search output as
 * [ids nq*k int64][scores nq*k fp32][counts nq int32], padded to a multiple of 8 bytes
 * (crag_result_record_bytes).  Each rank lets crag_index_search_async write straight into its
 * record, ONE all-gather moves the records, and this merges n_lists consecutive records. */
int64_t crag_result_record_bytes(int nq, int k);
int crag_merge_topk_packed(int device, const void *d_records, int n_lists, int nq, int k,
                           int64_t *d_out_ids, float *d_out_scores, int32_t *d_out_counts, void *stream);

/* Reciprocal-rank fusion of up to 8 retrieval lanes on the GPU (hybrid /retrieve, BASELINE configs[4]).
 * Replaces: _rrf_merge (retrieve.py:245-260) — score += 1/(rrf_k + rank) per lane in lane order (fp64,
 * bit-identical to the Python floats), stable descending order (ties keep first-insertion order).
 *   d_lane_ids[l]    device [nq, lane_width[l]] int64 keys of lane l, best first (may be NULL when lane_width[l] is 0)
 *   d_lane_counts[l] device [nq] valid entries per query (clamped to [0, lane_width[l]])
 *   outputs          [nq, out_k]: fused keys (-1 pad), fp64 scores (NaN pad), lane-hit bit masks; [nq] counts
 * The pointer arrays themselves live on the HOST. */
int crag_rrf_fuse(int n_lanes, const int64_t *const *d_lane_ids, const int32_t *const *d_lane_counts,
                  const int *lane_width, int nq, int rrf_k, int out_k, int64_t *d_out_ids,
                  double *d_out_scores, uint32_t *d_out_lanes, int32_t *d_out_counts, void *stream);

/* Exact-token lane for a batch of up to 64 queries (hybrid /retrieve).  Replaces: _fetch_chunks_tech /
 * _fetch_artifacts_tech (retrieve.py:183-242): rows whose token set overlaps the query's, first k in
 * the order (call_started_at DESC, id ASC).  Tokens are 64-bit hashes of the exact token strings; the value 0 marks
 * an empty table slot inside the kernel, so hashes 0 and 1 are ONE token to the lane (on the row and the query side).
 *   d_order [n] int32   row position at each rank r of that static order
 *   d_row_ptr [n+1] int64, d_tokens [nnz] uint64   CSR of the rows' token hashes, stored BY RANK
 *                       (CSR row r = the row at position d_order[r]) so the scan streams coalesced
 *   d_query_tokens [nq, 32] uint64, d_query_token_counts [nq] int32 (<= 32 tokens per query)
 *   d_row_mask as in crag_index_search (bit per row POSITION; nullable); with a mask, mask_stride is 0 (shared) or a
 *                       multiple of 4 >= ceil(n_rows/32)*4 -- CRAG_EINVAL otherwise, nothing is enqueued
 *   d_bitmap_scratch [max(1, ceil(n/64)) * nq] uint64
 *   d_out_ids [nq, k] (-1 pad), d_out_counts [nq] */
int crag_tech_lane(const int32_t *d_order, const int64_t *d_row_ptr, const uint64_t *d_tokens,
                   const int64_t *d_ids, int64_t n_rows, const uint64_t *d_query_tokens,
                   const int32_t *d_query_token_counts, int nq, int k, const uint8_t *d_row_mask,
                   int64_t mask_stride, uint64_t *d_bitmap_scratch, int64_t *d_out_ids,
                   int32_t *d_out_counts, void *stream);

/* The same lane for a caller that holds the query tokens on the HOST (the gateway does: extract_tech_tokens runs there).
 * An upload slot = a pinned host buffer, its device twin and the event of the last copy that read the host buffer; a
 * caller keeps a small ring of them per stream (the call waits for the slot's previous copy only).  The call packs the
 * hashes (duplicates inside a query dropped, first occurrence kept), enqueues ONE host-to-device copy and the two
 * kernels on `stream` and returns.
 *   h_token_hashes  host: the queries' token hashes back to back;  h_token_counts host [nq]: tokens per query
 *   CRAG_E2BIG: a query holds more than 32 DISTINCT tokens -- nothing was enqueued, the caller runs it in passes. */
typedef struct crag_upload_slot crag_upload_slot;
crag_upload_slot *crag_upload_slot_create(void);
void crag_upload_slot_destroy(crag_upload_slot *slot);
int crag_tech_lane_host(const int32_t *d_order, const int64_t *d_row_ptr, const uint64_t *d_tokens,
                        const int64_t *d_ids, int64_t n_rows, const uint64_t *h_token_hashes,
                        const int32_t *h_token_counts, int nq, int k, const uint8_t *d_row_mask, int64_t mask_stride,
                        crag_upload_slot *slot, uint64_t *d_bitmap_scratch, int64_t *d_out_ids, int32_t *d_out_counts,
                        void *stream);

/* BM25 lexical lane for a batch of up to 64 queries (hybrid /retrieve, and the reference's lexical-only mode).
 * Stands in for: _fetch_chunks_bm25 / _fetch_artifacts_bm25 (retrieve.py:123-180) -- `text @@@ :query` ordered by
 * pdb.score(id) DESC LIMIT k over the pg_search index.  NOT parity with pg_search: Tantivy's arithmetic is not in the
 * reference tree; this is a self-defined restatement of the published form it uses (DESIGN.md 4.7 lists the departures):
 *   score(row) = sum over the query's terms t, ascending term id, of w_t * tf / (tf + k1 * (1 - b + b * dl / avgdl)),
 *   k1 = 1.2, b = 0.75, w_t = qtf * ln(1 + (N - df + 0.5) / (df + 0.5)) * (k1 + 1) computed by the caller in fp64 and
 *   rounded once to fp32; the rest is fp32 on the device, one rounding per operation, in that fixed order.
 * The index is an inverted CSR the caller keeps on the device (cadence_rag_amd.bm25.Bm25Index builds it):
 *   d_post_ptr [n_terms + 1] int64, d_post_pos [nnz] int32 row positions ascending inside a term, d_post_tf [nnz]
 *   uint16 (saturated), d_doc_len [n_rows] int32, d_ids [n_rows] ascending with the position (NULL: ids = positions).
 * The queries come from the HOST in CSR form: h_q_ptr [nq + 1] int32 (h_q_ptr[0] = 0), per query its term ids
 * (strictly ascending, inside [0, n_terms)) and their weights -- any number of terms per query.  A query without terms
 * returns nothing.  Only rows that hold at least one of the query's terms are returned (OR semantics; score > 0).
 *   d_row_mask / mask_stride as in crag_index_search (bit per row POSITION; nullable)
 *   slot       an upload slot as for crag_tech_lane_host (ONE host-to-device copy per call; it grows when a call needs more)
 *   d_scratch  crag_bm25_scratch_bytes(n_rows, nq, k) bytes, 8-byte aligned, owned by the caller, one per stream in use
 *   outputs    as crag_index_search: d_out_ids [nq, k] (-1 pad), d_out_scores [nq, k] fp32 (NaN pad), d_out_counts [nq]
 * Order: descending score, equal scores by ascending id.  Everything is enqueued on `stream`; results do not depend on
 * the launch geometry (same bits for the same (tf..., dl) whatever nq, k or the row's position).
 * CRAG_EINVAL: NULL pointer, nq > 64, k > CRAG_MAX_K, n_rows >= 2^31, bad q_ptr / term ids / weights / mask_stride,
 * scratch too small -- nothing was enqueued. */
int64_t crag_bm25_scratch_bytes(int64_t n_rows, int nq, int k);
int crag_bm25_lane_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const uint16_t *d_post_tf,
                        const int32_t *d_doc_len, const int64_t *d_ids, int64_t n_rows, int64_t n_terms, float avgdl,
                        const int32_t *h_q_ptr, const int32_t *h_term_ids, const float *h_weights, int nq, int k,
                        const uint8_t *d_row_mask, int64_t mask_stride, crag_upload_slot *slot, void *d_scratch,
                        int64_t scratch_bytes, int64_t *d_out_ids, float *d_out_scores, int32_t *d_out_counts,
                        void *stream);

/* Query clauses of the BM25 lane as row masks for up to 64 queries: required (+), excluded (-) and
 * quoted-phrase clauses become one row mask per query, which crag_bm25_lane_host then scores under -- its arithmetic is
 * untouched.  The reference hands the user's string to `text @@@ :query` (retrieve.py:141,173), where pg_search runs
 * Tantivy's query parser.  NOT parity with it: the rule is this tree's own.
 * Parsing (host, cadence_rag_amd.bm25.parse_query):
 *   Items are separated by whitespace outside double quotes.  `"` opens a quoted item (and ends an unquoted one); an
 *   unclosed quote runs to the end of the string.  An item may carry ONE prefix, `+` or `-`, directly in front of it, at the start of the string or
 *   after whitespace (anywhere else, and inside quotes, the character is text).  Every item's text goes through the
 *   lane's tokenizer; an item with no tokens is dropped.
 *   An unquoted item: each of its tokens is a term clause of the item's kind -- `+` required, `-` excluded, no prefix
 *   optional (`+foo-bar` is two required terms).
 *   A quoted item: one token makes a term clause, two or more make a phrase clause; either is required unless the item
 *   is prefixed `-` (then excluded).  An unprefixed quoted phrase is a REQUIREMENT (in Tantivy it is a SHOULD clause with
 *   a phrase score).  Nothing else is syntax: `field:`, `*`, `~` and parentheses separate tokens as before -- `*` and `~`
 *   unless `expand` (parse_query(text, expand=True), crag_bm25_expand_host below).
 * Matching.  A row passes a query iff its input mask bit is set, it holds every required term, no excluded term, every
 *   required phrase and no excluded phrase.  A row holds the phrase t0 .. t(m-1) iff some token position p exists with
 *   token t_i at position p + i for every i.  Positions index the tokens the tokenizer keeps for that row (they count as
 *   doc_len does); a phrase never spans two rows; a term may repeat inside a phrase.  Positions at or above 65 535 are
 *   NOT indexed (16-bit positions; the reference's chunks hold at most 600 tokens).
 * Unknown tokens: in a required term or phrase the query matches nothing (kind 4); in an excluded clause the clause is
 *   dropped; in an optional clause the token is dropped.
 * Scoring.  The scored bag is the tokens of every non-excluded item (optional terms, required terms, members of required
 *   phrases) with the qtf counting of the lane; excluded tokens score nothing.  A row is returned only if it passes AND
 *   scores > 0, so a query of excluded clauses alone returns nothing, and a query without prefix or quote gives the
 *   lane's result bit for bit.
 * Limits (design decisions): at most CRAG_BM25_MAX_CLAUSES constraint clauses per query (required terms, excluded terms
 *   and phrases count one each; optional terms are no clauses), at most CRAG_BM25_MAX_PHRASE terms per phrase.
 *
 *   d_post_ptr [n_terms + 1], d_post_pos [nnz]  the postings of crag_bm25_lane_host
 *   d_post_off [nnz + 1] int64, d_post_where [d_post_off[nnz]] uint16: posting j (the order of d_post_pos) holds its
 *               term at the token positions d_post_where[d_post_off[j] .. d_post_off[j + 1]), ascending.  Both may be
 *               NULL when no clause is a phrase.
 *   Clauses from the HOST in CSR form: h_c_ptr [nq + 1] int32 (h_c_ptr[0] = 0), h_c_kind [n_clauses] -- 0 required
 *               term, 1 excluded term, 2 required phrase, 3 excluded phrase, 4 "matches nothing" (no terms) --,
 *               h_ct_ptr [n_clauses + 1] int32 (h_ct_ptr[0] = 0), h_ct_terms: term ids in phrase order.
 *   d_in_mask / in_stride  as in crag_attr_masks_host (nullable: every row is admitted; in_stride 0: one shared run; bits
 *               at positions >= n_rows are ignored).  The in and out masks must NOT overlap; this is not checked.
 *   d_out_mask  nq runs of mask_stride bytes in the row_mask encoding of crag_index_search (4-byte aligned); mask_stride a
 *               multiple of 4 >= ceil(n_rows/32)*4.  EVERY byte of every run is written -- bits at positions >= n_rows
 *               and the bytes up to mask_stride are 0 --, nothing outside nq * mask_stride bytes is; plain stores, never
 *               OR: the buffer may be uninitialised and reused.  The output depends on the input alone, whatever the
 *               launch geometry.  A query without clauses copies its input mask (all ones below n_rows without one).
 *   slot        an upload slot as for crag_tech_lane_host: ONE host-to-device copy per call (the clause arrays)
 * Everything is enqueued on `stream`, no host synchronisation.
 * CRAG_EINVAL with a message that contains "bm25_clause_masks_host", checked before any HIP call, nothing enqueued: a
 * NULL required pointer, nq outside 1..64, n_rows outside [0, 2^31), n_terms outside [0, 2^31), bad mask_stride or
 * in_stride, a misaligned mask, h_c_ptr / h_ct_ptr not ascending from 0, an unknown kind, a term id outside
 * [0, n_terms), a term clause without exactly one term, a kind-4 clause with terms, a phrase with fewer than 2 or more
 * than 8 terms, more than 16 clauses in a query, a phrase clause with NULL position arrays.
 * n_rows == 0 is CRAG_OK (the runs are zeroed when mask_stride > 0). */
#define CRAG_BM25_MAX_CLAUSES 16
#define CRAG_BM25_MAX_PHRASE  8
int crag_bm25_clause_masks_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const int64_t *d_post_off,
                                const uint16_t *d_post_where, int64_t n_rows, int64_t n_terms,
                                const int32_t *h_c_ptr, const int32_t *h_c_kind, const int32_t *h_ct_ptr,
                                const int32_t *h_ct_terms, int nq, const uint8_t *d_in_mask, int64_t in_stride,
                                crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride, void *stream);

/* Prefix and fuzzy terms of the BM25 lane, expanded over the vocabulary on the device.  `deploy*` stands
 * for the vocabulary terms that begin with "deploy", `kubernets~` for those within edit distance 1 of "kubernets".  The
 * reference's pg_search would read `*` and `~` with Tantivy's parser; the rule here is this tree's own, NOT parity.
 * Parsing (host, cadence_rag_amd.bm25.parse_query(text, expand=True); without `expand` nothing below is syntax):
 *   An UNQUOTED item (behind its optional `+` / `-` prefix) may end in ONE operator: `*` (a prefix item, kind 0), `~` or
 *   `~1` (a fuzzy item of distance 1, kind 1), `~2` (distance 2, kind 2).  The operator counts only if the text in front
 *   of it goes through the tokenizer to EXACTLY ONE token; otherwise the whole item is read by the rule of
 *   crag_bm25_clause_masks_host: `b)*` is the prefix item "b", `~2` alone is the text "2", `foo-bar*` is the two plain
 *   tokens "foo" and "bar", `x~3` and `x~0` are plain text, `x**` is the prefix item "x" (the last `*` is the operator,
 *   the one in front of it separates tokens as ever).  Nothing inside quotes is syntax.  `+` makes the item required, `-`
 *   excluded, none optional.  The item's token is neither in the scored bag nor a clause of the clause entry; the text
 *   handed to a lane without clauses (the trigram field) holds it, operator removed, unless the item is excluded.
 *   Limits: at most CRAG_BM25_MAX_EXPAND_ITEMS expanding items per query; required and excluded expanding items count
 *   towards the CRAG_BM25_MAX_CLAUSES constraint clauses of the query.
 * Matching is over the Unicode code points of the (lower-cased) token and of the vocabulary's terms.
 *   Prefix: the term's code points begin with the pattern's; the term equal to the pattern is included; every match has
 *   distance 0.
 *   Fuzzy: the plain Levenshtein distance (insertions, deletions and substitutions of one code point cost 1 each, so a
 *   transposition of two neighbours costs 2) is at most d; the term equal to the pattern is included, distance 0.
 *   A pattern is 1 to 255 bytes of UTF-8 (the tokenizer's limit); there is no other length limit.
 * Kept expansions.  Per pattern the first CRAG_BM25_MAX_EXPANSIONS matches are kept in this order: distance ascending,
 *   then df descending (df(t) = d_post_ptr[t + 1] - d_post_ptr[t]), then term id ascending.  The number of ALL matches is
 *   reported beside them.  DEPARTURE: matches beyond the 64th take no part in scoring or in the item's clause (Tantivy's
 *   fuzzy and prefix queries expand to 50 terms by default and rank them differently).
 * Clauses (crag_bm25_group_masks_host).  A required expanding item passes the rows that hold AT LEAST ONE of its kept terms;
 *   an excluded item fails the rows that hold ANY of them.  An item without a match behaves as an unknown token does: a
 *   required one makes the query match nothing, an excluded or optional one is dropped.
 * Scoring.  Excluded items score nothing.  For an item j that is not excluded, with kept terms T_j:
 *     df*    = the largest df over T_j
 *     base_j = ln(1 + (N - df* + 0.5) / (df* + 0.5)) * (k1 + 1)                       (fp64)
 *   and a term of T_j at distance d contributes base_j * 2^(-d).  The weight of a term is the lane's qtf * idf * (k1 + 1)
 *   (one product, when the term is in the plain bag) plus the contributions of the items in item order, all in fp64,
 *   rounded ONCE to fp32; terms reach crag_bm25_lane_host in ascending id.  Its kernels are untouched.
 *
 * crag_bm25_expand_host:
 *   d_term_ptr [n_terms + 1] int64, d_term_bytes: the UTF-8 bytes of the terms in term-id order, term t at
 *               d_term_bytes[d_term_ptr[t] .. d_term_ptr[t + 1]); d_post_ptr [n_terms + 1] as for crag_bm25_lane_host
 *   Patterns from the HOST in CSR form: h_pat_ptr [n_patterns + 1] int32 byte offsets (h_pat_ptr[0] = 0), h_pat_bytes,
 *               h_pat_kind [n_patterns] (0 prefix, 1 fuzzy 1, 2 fuzzy 2); 0 <= n_patterns <= CRAG_BM25_MAX_PATTERNS
 *   slot        an upload slot as for crag_tech_lane_host: ONE host-to-device copy per call
 *   d_scratch   crag_bm25_expand_scratch_bytes(n_terms, n_patterns) bytes (-1: arguments out of range), 8-byte aligned
 *   outputs (device): d_out_terms [n_patterns, 64] int32 kept term ids in the order above, -1 padded; d_out_dist
 *               [n_patterns, 64] int32 their distances, -1 padded; d_out_kept [n_patterns] int32; d_out_total [n_patterns]
 *               int64, the number of all matches
 * Everything is enqueued on `stream`, no host synchronisation; the output depends on the input alone, whatever the slice
 * size or the grid.  n_patterns == 0 is CRAG_OK and writes nothing; n_terms == 0 writes the padding and zero counts.
 * CRAG_EINVAL with a message that contains "bm25_expand_host", checked before any HIP call, nothing enqueued: a NULL
 * required pointer, n_patterns outside [0, 512], n_terms outside [0, 2^31), h_pat_ptr not ascending from 0, an empty
 * pattern or one above 255 bytes, an unknown kind, misaligned arrays, a scratch that is too small or misaligned.
 *
 * crag_bm25_group_masks_host: the any-of clauses of up to 64 queries as row masks.
 *   Groups from the HOST in CSR form: h_g_ptr [nq + 1] int32 (h_g_ptr[0] = 0; at most 16 groups per query), h_g_kind
 *               [n_groups] -- 0 required-any, 1 excluded-any --, h_gt_ptr [n_groups + 1] int32 (h_gt_ptr[0] = 0; 0 to 64
 *               terms per group), h_gt_terms: term ids.
 *   out = in_mask AND (for every required group: the OR of its terms' rows) AND NOT (the OR of the excluded groups'
 *   terms' rows).  An empty required group matches nothing; an empty excluded group has no effect.
 *   d_in_mask / in_stride / d_out_mask / mask_stride / slot: the contract of crag_bm25_clause_masks_host, word for word --
 *   every byte of every run is written with plain stores (never OR), bits at positions >= n_rows and the bytes up to
 *   mask_stride are 0, in_stride 0 is one shared input run, a query without groups copies its input, in and out must not
 *   overlap.  Everything is enqueued on `stream`.
 * CRAG_EINVAL with a message that contains "bm25_group_masks_host", checked before any HIP call, nothing enqueued: a NULL
 * required pointer, nq outside 1..64, n_rows or n_terms outside [0, 2^31), bad mask_stride or in_stride, a misaligned
 * mask, h_g_ptr / h_gt_ptr not ascending from 0, an unknown kind, a term id outside [0, n_terms), a group of more than 64
 * terms, more than 16 groups in a query.  n_rows == 0 is CRAG_OK (the runs are zeroed when mask_stride > 0). */
#define CRAG_BM25_MAX_EXPANSIONS   64
#define CRAG_BM25_MAX_EXPAND_ITEMS 8
#define CRAG_BM25_MAX_PATTERNS     512
int64_t crag_bm25_expand_scratch_bytes(int64_t n_terms, int n_patterns);
int crag_bm25_expand_host(const int64_t *d_term_ptr, const uint8_t *d_term_bytes, const int64_t *d_post_ptr,
                          int64_t n_terms, const int32_t *h_pat_ptr, const uint8_t *h_pat_bytes,
                          const int32_t *h_pat_kind, int n_patterns, crag_upload_slot *slot, void *d_scratch,
                          int64_t scratch_bytes, int32_t *d_out_terms, int32_t *d_out_dist, int32_t *d_out_kept,
                          int64_t *d_out_total, void *stream);
int crag_bm25_group_masks_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, int64_t n_rows, int64_t n_terms,
                               const int32_t *h_g_ptr, const int32_t *h_g_kind, const int32_t *h_gt_ptr,
                               const int32_t *h_gt_terms, int nq, const uint8_t *d_in_mask, int64_t in_stride,
                               crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride, void *stream);

/* Query-aware snippet windows of the BM25 word lane: for every (query, row) pair of a batch, where in
 * the row a window of `window` tokens holds the most of the query, read from the token positions the index keeps on the
 * device (d_post_off / d_post_where, the arrays of the phrase clauses).  The reference has no code for this
 * (APP_SPEC.md:269 asks for "snippets [that] are actually relevant (not just 'first N chars of the doc')"): the rule is
 * this tree's own.
 *
 * The rule.  A query is its term slots j = 0 .. m - 1 (m <= CRAG_BM25_SNIPPET_MAX_TERMS), each a term id and an fp32
 * weight, finite and >= 0.  For a pair (query, row r), a window width W and a start s:
 *   covered(s) = the slots whose term has a token position of row r in [s, s + W),
 *   score(s)   = the fp32 sum of the weights of covered(s), added one by one in ascending slot order onto +0.0f (no
 *                FMA, no reassociation).
 *   A start is a position of row r that holds the term of some slot (an occurrence).  Starts in between need no
 *   trying: a window moved right to the first occurrence inside it still holds every occurrence it held, so its covered
 *   set does not shrink, and -- the weights are >= 0 and a rounded addition is monotone -- its score does not fall.
 *   The answer is the start with the largest score; among equal scores the lowest start.
 * Only positions the index holds (< 65 535) exist for this rule.
 *   Queries from the HOST in CSR form (what crag_bm25_lane_host takes): h_q_ptr [nq + 1] int32 (h_q_ptr[0] = 0), h_terms,
 *               h_weights.  The rows of every query likewise: h_r_ptr [nq + 1] int32 (h_r_ptr[0] = 0), h_rows [npairs]
 *               row POSITIONS in [0, n_rows), in any order, repeats allowed.  1 <= window <= 65535.
 *   Outputs [npairs], laid out along h_r_ptr: d_start int32 (-1 when no slot's term occurs in the row; the other three are
 *               then 0), d_last int32 (the largest occurrence inside the chosen window), d_score fp32, d_covered uint64
 *               (bit j for slot j).
 * One upload through `slot` and one launch on `stream`, asynchronous; integer work and the fixed-order sum: the outputs
 * are a function of the inputs alone.
 * CRAG_EINVAL with a message that contains "bm25_snippets_host", checked before any HIP call, nothing enqueued: a NULL
 * required pointer (the position arrays included), nq outside 1..64, n_rows or n_terms outside [0, 2^31), h_q_ptr or
 * h_r_ptr not ascending from 0, a query of more than 64 slots, a term id outside [0, n_terms), a weight that is negative or
 * not finite, a row outside [0, n_rows), window outside 1..65535.  npairs == 0 is CRAG_OK and enqueues nothing. */
#define CRAG_BM25_SNIPPET_MAX_TERMS 64
int crag_bm25_snippets_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const int64_t *d_post_off,
                            const uint16_t *d_post_where, int64_t n_rows, int64_t n_terms, const int32_t *h_q_ptr,
                            const int32_t *h_terms, const float *h_weights, const int32_t *h_r_ptr, const int32_t *h_rows,
                            int nq, int window, crag_upload_slot *slot, int32_t *d_start, int32_t *d_last, float *d_score,
                            uint64_t *d_covered, void *stream);

/* Character-trigram field of the BM25 lane: the inverted CSR crag_bm25_lane_host scores, built on the device from the
 * rows' bytes (cadence_rag_amd.ngram.NgramIndex drives it).  Stands in for the reference's second index over every
 * lexical column, the `pdb.ngram(3,3)` aliases of alembic/versions/0005_add_bm25_ngram.py and 0006_add_artifact_chunks.py
 * ("BM25 ngram robustness (ASR noise)", PHASED_PLAN.md:113,379).  NOT parity with Tantivy's ngram tokenizer: the rule is
 * this tree's own (DESIGN.md 4.7b lists the departures).  It works on the BYTES of one row:
 *   Decode.  A lead byte 0xxxxxxx / 110xxxxx / 1110xxxx / 11110xxx starts a sequence of 1 / 2 / 3 / 4 bytes; the following
 *     bytes must be 10xxxxxx and lie inside the row; the value is what the payload bits give (overlong forms and the
 *     surrogate range are NOT checked); a 4-byte value above 0x10FFFF is malformed.  A malformed or cut-off lead, any
 *     other byte (0xF8-0xFF) and a continuation byte no valid lead consumed are each one separator of one byte, and
 *     decoding resumes at the next byte.
 *   Fold and classify.  'A'-'Z' become 'a'-'z' (no other case mapping).  A code point is a gram character if it is an
 *     ASCII letter or digit or if it is >= 0x80; every other ASCII code point is a separator.
 *   Grams.  Every three consecutive gram characters form one gram, one per start position, overlapping; runs of one or two
 *     characters yield nothing.   key = cp0 << 42 | cp1 << 21 | cp2: exact, below 2^63 - 1, no hashing.
 *   Row statistics.  dl = the row's number of grams; tf = occurrences of a gram in the row, stored saturating at 65 535.
 *   Term ids.  The term id of a key is its rank among the distinct keys of the index, ascending.
 * The build is three calls around a sort and a prefix sum that the CALLER runs with any correct routine (the result is
 * integers, fully determined by the rule):
 *   1. crag_ngram_extract: one slot per byte position p of the text, d_slot_keys[p] = the key of the gram that starts at p
 *      or CRAG_NGRAM_NO_KEY (above every key), d_slot_rows[p] = the row of p; d_doc_len [n_rows] is zeroed and counted.
 *      The number of grams is the sum of d_doc_len.
 *   -- the caller sorts the n_bytes slots by key, STABLE (or by (key, row)): the first n_grams sorted slots are the grams,
 *      rows ascending inside a key --
 *   2. crag_ngram_heads: d_flags[i] = (sorted gram i opens a (key, row) run) + 2^32 * (it opens a key run).
 *   -- the caller takes the inclusive prefix sum d_scan of d_flags; its last element is nnz + 2^32 * n_terms --
 *   3. crag_ngram_emit: d_keys [n_terms] ascending, d_post_ptr [n_terms + 1], d_post_pos [nnz] row positions ascending
 *      inside a term, d_post_tf [nnz] -- with d_doc_len the arrays of crag_bm25_lane_host.  n_grams = 0 writes
 *      d_post_ptr[0] = 0 alone.
 *   d_text      [n_bytes] the rows' bytes concatenated, 16-byte aligned;  d_text_ptr [n_rows + 1] int64, row r is
 *               [d_text_ptr[r], d_text_ptr[r + 1]), rows may be empty
 *   d_scratch   crag_ngram_scratch_bytes(n_bytes, n_rows) bytes, 8-byte aligned, owned by the caller; calls 1 and 3 use it
 * Memory the caller sizes: 12 bytes of slots per byte of text, 8 + 4 per gram sorted, 8 per gram of flags (the scan may
 * overwrite them), 4 per byte of scratch.  The kernels read the text in tiles of CRAG_NGRAM_TILE bytes; the result does
 * not depend on where the tiles' edges fall.  Nothing is allocated by any of the calls.  Everything is enqueued on
 * `stream`; crag_ngram_extract alone waits for the stream once, for the check of d_text_ptr, before it touches the text.
 * CRAG_E2BIG: n_bytes > 2^31 - 1 (checked first, from the argument alone) -- a larger corpus is split by rows into
 * several indexes by the caller.  CRAG_EINVAL: d_text_ptr not ascending from 0 to n_bytes, NULL / misaligned pointer,
 * n_rows >= 2^31, scratch too small, counts that cannot be (n_terms <= nnz <= n_grams).  On an error nothing was written
 * but the scratch.  crag_ngram_scratch_bytes returns the same negative codes for sizes it does not take. */
#define CRAG_NGRAM_TILE 4096
#define CRAG_NGRAM_NO_KEY INT64_MAX
int64_t crag_ngram_scratch_bytes(int64_t n_bytes, int64_t n_rows);
int crag_ngram_extract(const uint8_t *d_text, int64_t n_bytes, const int64_t *d_text_ptr, int64_t n_rows,
                       int64_t *d_slot_keys, int32_t *d_slot_rows, int32_t *d_doc_len, void *d_scratch,
                       int64_t scratch_bytes, void *stream);
int crag_ngram_heads(const int64_t *d_sorted_keys, const int32_t *d_sorted_rows, int64_t n_grams, int64_t *d_flags,
                     void *stream);
int crag_ngram_emit(const int64_t *d_sorted_keys, const int32_t *d_sorted_rows, const int64_t *d_scan, int64_t n_grams,
                    int64_t n_terms, int64_t nnz, int64_t *d_keys, int64_t *d_post_ptr, int32_t *d_post_pos,
                    uint16_t *d_post_tf, void *d_scratch, int64_t scratch_bytes, void *stream);

/* Filter row masks for up to 64 queries, built on the device from device-resident columns: the producer of the
 * `row_mask` every lane above takes (crag_index_search*, crag_index_count_eligible, crag_tech_lane*, crag_bm25_lane_host).
 * Replaces: _build_filter_clause (retrieve.py:93-120) -- call_started_at >= :date_from, <= :date_to, call_id = ANY(:ids),
 * calls.tags && :tags; the last two arrive resolved to the table's call dictionary (cadence_rag_amd.filters).
 *   d_started_us [n_rows] int64  the row's call_started_at in us since the epoch; INT64_MIN = NULL / NaT
 *   d_call_slot [n_rows] int32   the dense number, in [0, n_calls), of the row's call
 *   h_call_qset [n_calls] HOST, nullable: bit q of word c set <=> query q admits call c (a query without call scoping has
 *                                its bit set in every word; NULL: no query is call-scoped)
 *   h_date_from, h_date_to [nq] HOST: inclusive bounds in us; INT64_MIN = no lower bound, INT64_MAX = no upper bound
 * Bit (q, i) is set iff   (h_call_qset == NULL or 0 <= slot[i] < n_calls and bit q of qset[slot[i]] is set)
 *                     and (from[q] == INT64_MIN or started[i] != INT64_MIN and started[i] >= from[q])
 *                     and (to[q]   == INT64_MAX or started[i] != INT64_MIN and started[i] <= to[q]).
 * A NULL timestamp passes a query without a date bound and fails one with any (what SQL and numpy do with NULL / NaT);
 * a slot outside [0, n_calls) is never dereferenced: with h_call_qset given that row passes no query.
 *   d_out_mask  nq runs of mask_stride bytes in the row_mask encoding of crag_index_search (4-byte aligned); mask_stride a
 *               multiple of 4 >= ceil(n_rows/32)*4.  EVERY byte of every run is written -- bits at positions >= n_rows
 *               and the bytes up to mask_stride are 0 --, nothing outside nq * mask_stride bytes is; plain stores, never
 *               OR: the buffer may be uninitialised and reused.  The output depends on the input alone.
 *   slot        an upload slot as for crag_tech_lane_host: ONE host-to-device copy per call (bounds + qset)
 * Everything is enqueued on `stream`, no host synchronisation.  CRAG_EINVAL with a message, checked before any HIP call
 * and nothing enqueued: NULL required pointer, nq < 1, nq > 64, n_rows < 0, n_rows >= 2^31, n_calls < 0, bad mask_stride.
 * n_rows == 0 is CRAG_OK (the runs are zeroed when mask_stride > 0). */
#define CRAG_FILTER_MAX_QUERIES 64
int crag_filter_masks_host(const int64_t *d_started_us, const int32_t *d_call_slot, int64_t n_rows, int64_t n_calls,
                           const uint64_t *h_call_qset, const int64_t *h_date_from, const int64_t *h_date_to, int nq,
                           crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride, void *stream);

/* Attribute row masks for up to 64 queries: row-level filters by entity, speaker and kind, built on the device from a
 * device-resident CSR of per-row attribute ids.  The reference plans these filters and has no code for
 * them: PHASED_PLAN.md:355-380 (RetrieveFilters.entity_filters = [{label, value}], "implemented in SQL using joins to
 * entities/mentions"), APP_SPEC.md:311-341 (entities, chunk_entities, artifact_entities), APP_SPEC.md:616-619 (entity
 * constraints; the who_said intent is a speaker constraint).  The rule is this tree's own.
 *   d_attr_ptr [n_rows+1] int64, d_attr_ids [d_attr_ptr[n_rows]] int32: CSR by row POSITION; the ids are those of the
 *                         table's attribute dictionary (exact strings numbered by first appearance, no hashing).
 *                         Duplicates inside a row are allowed.  An id outside [0, n_attrs) matches nothing and is never
 *                         used as an index.
 *   h_keys [n_keys] HOST  the distinct attribute ids any query lists: strictly ascending, in [0, n_attrs)
 *   h_key_sets [n_keys][8] HOST: bit q of word (j, c) set <=> clause c of query q lists key j
 *   h_clause_sets [8] HOST: bit q of word c set <=> query q has a clause c.  A clause bit with no key anywhere admits
 *                         nothing.
 *   d_in_mask             nullable (NULL: every row is admitted): masks in the row_mask encoding of crag_index_search,
 *                         in_stride == 0: one run shared by all queries, otherwise one run per query (a multiple of 4
 *                         >= ceil(n_rows/32)*4); 4-byte aligned; bits at positions >= n_rows are ignored.
 *                         d_in_mask == d_out_mask with in_stride == mask_stride is allowed (in place); any other
 *                         overlap is undefined.
 * Bit (q, i) is set iff i < n_rows and in(q, i) and, for every c with bit q of clause_sets[c], some attribute a of row i
 * equals keys[j] with bit q of key_sets[j][c]: AND across a query's clauses, OR inside a clause.
 * NULL rule: a namespace a table lacks (no speaker column, entities never tracked) has no attribute in any row and no key
 * in the dictionary, so every clause over it admits nothing -- what SQL does with NULL = ANY(...), and the NaT rule of
 * crag_filter_masks_host.
 *   d_out_mask  nq runs of mask_stride bytes in the row_mask encoding of crag_index_search (4-byte aligned); mask_stride a
 *               multiple of 4 >= ceil(n_rows/32)*4.  EVERY byte of every run is written -- bits at positions >= n_rows
 *               and the bytes up to mask_stride are 0 --, nothing outside nq * mask_stride bytes is; plain stores, never
 *               OR: the buffer may be uninitialised and reused.  The output depends on the input alone, whatever the
 *               launch geometry.
 *   slot        an upload slot as for crag_tech_lane_host: ONE host-to-device copy per call (keys + their sets)
 * Everything is enqueued on `stream`, no host synchronisation.
 * CRAG_EINVAL with a message that contains "attr_masks_host", checked before any HIP call, nothing enqueued: NULL
 * required pointer, nq outside 1..64, n_rows outside [0, 2^31), n_attrs < 0, n_keys < 0, keys not strictly ascending or
 * out of range, a set bit at or above nq, key_sets[j][c] not a subset of clause_sets[c], bad mask_stride or in_stride, a
 * misaligned output or input mask.
 * CRAG_E2BIG, nothing enqueued: n_keys > CRAG_ATTR_MAX_KEYS -- the caller splits the batch by queries.
 * n_rows == 0 is CRAG_OK (the runs are zeroed when mask_stride > 0). */
#define CRAG_ATTR_MAX_QUERIES 64
#define CRAG_ATTR_MAX_CLAUSES 8
#define CRAG_ATTR_MAX_KEYS    512   /* distinct keys per call */
int crag_attr_masks_host(const int64_t *d_attr_ptr, const int32_t *d_attr_ids, int64_t n_rows, int64_t n_attrs,
                         const int32_t *h_keys, const uint64_t *h_key_sets, int n_keys,
                         const uint64_t *h_clause_sets, int nq,
                         const uint8_t *d_in_mask, int64_t in_stride,
                         crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride, void *stream);

/* Facet counts for up to 64 queries: per query and requested namespace, which attributes the rows that pass the query's
 * mask carry and how many rows hold each -- the "facets can be computed" line of the reference's
 * "Entities + faceting" phase (PHASED_PLAN.md:355-380), which has no code there.  The rule is this tree's own.
 *   FACET IDS number the table's attributes by (namespace, value) ascending (cadence_rag_amd.filters.FacetColumns): a
 *   namespace is one contiguous range [lo, hi) of ids, and ascending id is ascending value inside it.
 *   d_post_ptr [n_attrs+1] int64, d_post_rows [n_postings] int32, d_post_fid [n_postings] int32: the postings, i.e. the
 *                         transpose of the CSR of crag_attr_masks_host -- attribute a is held by the row positions
 *                         d_post_rows[d_post_ptr[a] .. d_post_ptr[a+1]), ascending, each (attribute, row) pair ONCE;
 *                         d_post_fid[j] is the attribute posting j belongs to.  A posting whose attribute lies outside
 *                         the range being walked, or whose row lies outside [0, n_rows), counts nothing and is never used
 *                         as an index; a d_post_ptr value outside [0, n_postings] is clamped.
 *   d_masks               nullable (NULL: every row passes every query): nq runs of mask_stride bytes in the row_mask
 *                         encoding of crag_index_search, what crag_filter_masks_host / crag_attr_masks_host write; 4-byte
 *                         aligned, mask_stride a multiple of 4 >= ceil(n_rows/32)*4.  Bits at positions >= n_rows are
 *                         ignored.
 *   h_range_lo, h_range_hi [n_ranges] HOST: the requested namespaces as ranges of facet ids, 0 <= lo <= hi <= n_attrs,
 *                         pairwise disjoint; lo == hi is a namespace the table lacks.  Attributes outside every range are
 *                         never read.
 *   d_workspace           caller-owned, 8-byte aligned, workspace_bytes large: the query sets (8 bytes per row when
 *                         d_masks is given) followed by the count table nq x W x 4 bytes, W = the sum of hi - lo;
 *                         crag_facet_workspace_bytes gives the sum.  Its contents before and after are meaningless.
 * With count(q, a) = the number of i < n_rows with bit (q, i) set (or d_masks NULL) for which row i holds a:
 *   d_out_ids [nq][n_ranges][top] int32     the facet ids of the range with count > 0, by count descending, then id
 *                                           ascending; -1 beyond the list
 *   d_out_counts [nq][n_ranges][top] uint32 their counts; 0 beyond the list
 *   d_out_distinct [nq][n_ranges] int32     how many attributes of the range have count > 0
 *   d_out_rows [nq] int64                   the number of set bits below n_rows (n_rows without masks)
 * Every output byte is written; the outputs are a function of the inputs alone, whatever the launch geometry (integer
 * adds only).  Everything is enqueued on `stream`, no host synchronisation, no host-to-device copy (the ranges travel as
 * kernel arguments, which is why this entry takes no upload slot).
 * CRAG_EINVAL with a message that contains "facet_counts_host", checked before any HIP call, nothing enqueued: nq outside
 * 1..64, top outside 1..CRAG_FACET_MAX_TOP, n_ranges outside 0..CRAG_FACET_MAX_NAMESPACES, n_rows outside [0, 2^31),
 * n_attrs or n_postings negative, a range outside [0, n_attrs] or with lo > hi, overlapping ranges, a misaligned mask or
 * workspace, a bad mask_stride, a NULL required pointer (outputs; ranges when n_ranges > 0; postings when n_postings > 0;
 * the workspace when it has to hold anything).
 * CRAG_E2BIG, nothing enqueued: the workspace is smaller than crag_facet_workspace_bytes -- the caller splits the batch
 * by queries. */
#define CRAG_FACET_MAX_QUERIES    64
#define CRAG_FACET_MAX_NAMESPACES 16
#define CRAG_FACET_MAX_TOP        64
int64_t crag_facet_workspace_bytes(int64_t n_rows, int nq, int64_t width, int has_masks);
int crag_facet_counts_host(const int64_t *d_post_ptr, const int32_t *d_post_rows, const int32_t *d_post_fid,
                           int64_t n_postings, int64_t n_rows, int64_t n_attrs,
                           const uint8_t *d_masks, int64_t mask_stride,
                           const int32_t *h_range_lo, const int32_t *h_range_hi, int n_ranges, int nq, int top,
                           void *d_workspace, int64_t workspace_bytes,
                           int32_t *d_out_ids, uint32_t *d_out_counts, int32_t *d_out_distinct, int64_t *d_out_rows,
                           void *stream);

/* Live kernel timing for bench.py's roofline: enabled = N > 0 records HIP events around the scan
 * (and merge) kernel of every N-th search, on the stream it is launched on (N = 1: every search;
 * larger N perturbs the timed region less); 0 disables.  crag_index_profile_read sums and clears
 * the recorded samples (synchronises the events); n_launches = number of samples; scan_ms_total = the scan
 * kernel alone, merge_ms_total = everything else of a search (query preparation, rescoring / merge). */
int crag_index_profile_enable(crag_index *ix, int enabled);
int crag_index_profile_read(crag_index *ix, int64_t *n_launches, double *scan_ms_total,
                            double *merge_ms_total);
/* The same + event_pair_ms_total: every sample also records two events back to back in front of the scan launch;
 * their elapsed time is what an event pair measures with NOTHING between (the part of scan_ms_total that is event
 * processing, not kernel: rocprofv3's begin/end timestamps of the kernel do not contain it). */
int crag_index_profile_read_ex(crag_index *ix, int64_t *n_launches, double *scan_ms_total,
                               double *merge_ms_total, double *event_pair_ms_total);

/* Byte accounting of the prefilter path (fp16 MFMA scan + exact fp32 rescoring of the candidates, the path
 * searches over corpora of >= 128 rows per workgroup take): sums since the last call, then cleared.
 * candidates = rows that passed the proven-bound filter, rescored_rows = rows re-read (4 KiB each) for the
 * exact fp32 score.  The records are kept per workspace (= per stream in use, up to eight) and per query, written with
 * plain stores by the one selection block that owns them: searches overlapping on different streams do not lose counts;
 * a search of more than 256 queries folds its queries onto 256 records and may (results never depend on it).  A search
 * answered by the overflow fallback is not counted.  Synchronises the device. */
int crag_index_prefilter_stats(crag_index *ix, int64_t *searches, int64_t *candidates, int64_t *rescored_rows);

/* Developer probe (index created with CRAG_PHASE_TRACE=1 in the environment, else CRAG_EINVAL): 128 words written by
 * the selection blocks of query 0 of the most recent prefilter search -- [block r of the query][16]: 100 MHz
 * timestamps at the phase boundaries (0 start, 1 candidates loaded, 2 k-th approximate score, 3 survivors rescored,
 * 4 own list written + ticket, 5 lists gathered, 6 end), [8] candidates, [9] rows this block rescored.
 * Synchronises the device.  No reference counterpart (measurement only). */
int crag_index_phase_trace(crag_index *ix, uint64_t *out128);

/* Name of the scan kernel the most recent search on this index launched ("crag::scan_pipe_kernel", ...),
 * as rocprofv3 prints it; "" before the first search.  For bench.py's roofline object. */
const char *crag_index_last_scan_kernel(const crag_index *ix);

/* Wait schedule of the corpus loads of that scan: "fragment" (the fp16-mirror prefilter scan of a cache-sized
 * mirror: every k-step waits for its own fragment) or "tile"; "" before the first search.  The kernel name above
 * is the same for both.  Measurement and tests only. */
const char *crag_index_scan_waits(const crag_index *ix);

/* Bytes of one corpus row the prefilter scan streams: dim*2 when the index keeps the fp16 mirror of the unit rows
 * (default; + dim*2 bytes of HBM per row beside the dim*4 fp32 row, which stays the source of truth: candidates
 * are rescored from it), dim*4 when it was created with CRAG_NO_FP16_MIRROR=1, 0 with CRAG_NO_PREFILTER=1.
 * the bytes of a prefilter are declared separately -- bench.py's roofline uses this figure. */
int64_t crag_index_prefilter_row_bytes(const crag_index *ix);

/* Launch geometry of the scan kernel for the current size (for DESIGN/bench reporting). */
int crag_index_scan_geometry(const crag_index *ix, int nq, int *workgroups, int *threads,
                             int *query_blocks, int64_t *algorithmic_bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* CRAG_DENSE_H */
