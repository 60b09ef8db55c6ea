// crag_kernels.h — parameter blocks and launchers shared by the kernel units (crag_search.hip, crag_edit.hip, ...) and
// the host units of the C ABI (crag_api.hip, crag_api_search.hip, crag_api_store.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_arch.h"
#include "crag_rows.h"

namespace crag {

constexpr int TILE_ROWS = 32;                 // corpus rows per tile (= MFMA N)
constexpr int DIM = 1024;                     // padded vector width
constexpr int TILE_FLOATS = TILE_ROWS * DIM;  // 128 KiB per tile
constexpr int SCAN_WAVES = 8;                 // split-K ways per workgroup
constexpr int SCAN_THREADS = SCAN_WAVES * 64;
constexpr int KSLICE = DIM / SCAN_WAVES;      // 128 dims per wave
constexpr int GB_CELLS = 32;                  // global-bound buckets per query (>= k of the pipelined kernel)

struct ScanParams {
    const float *corpus;      // tile32 layout
    const float *inv_norm;    // [cap_rows] 1/||row||, 0 = never eligible
    const float *queries;     // [nq, dim] row-major fp32, raw (only scan_kernel, the A/B baseline, reads them)
    const float *a32;         // the same queries in A-fragment order, zero padded (prep_queries_kernel)
    const float *qinv;        // [nq_pad] 1/||q|| (0: zero / non-finite query)
    const uint32_t *gate;     // nullable; when set and *gate == 0 the scan exits at once (fallback launch)
    int wide;                 // 1: the 64-queries-per-pass kernel (two query blocks per pass)
    const uint32_t *mask;     // nullable; 32 rows per word
    int64_t mask_stride_w;    // words between consecutive queries' masks (0 = shared)
    uint2 *partial;           // [q_blocks][G][32][k] keys
    uint32_t *gbound;         // [q_blocks*32][GB_CELLS] score buckets, zero between searches
    int64_t n_rows;
    int64_t cap_rows;
    int nq;
    int dim;
    int k;
    int G;
    int nb;                   // global-bound buckets in use: min(k, GB_CELLS)
    int pub_rank;             // rank (0-based) of the key a workgroup publishes: nb * (pub_rank + 1) >= k
    int reverse;              // walk each workgroup's range back to front (alternates per search)
    int unpipelined;          // 1: use the unpipelined kernel also for k <= 32 (A/B testing, CRAG_UNPIPELINED=1)
    int piece_shift;          // layout of the fp32 rows: crag_piece_shift(index has the fp16 mirror)
};

struct MergeParams {
    const uint2 *partial;
    const int64_t *ids;       // [cap_rows] row position -> external id (nullable)
    uint32_t *gbound;         // zeroed per query after use (nullable)
    int64_t id_base;          // used when ids == nullptr
    int64_t *out_ids;
    float *out_scores;
    int32_t *out_counts;
    int k;
    int G;
};

// ---- prefilter path (fp16 MFMA scan + exact rescoring), see crag_search.hip --------------------------------
// per-query bound record: 128 class maxima (4 sets x 32 row classes), padded to five 128-byte lines so that the
// records of two queries never share a line
constexpr int PF_BOUND_CELLS = 160;
constexpr int PF_STAT_WS = 8;                 // search workspaces per index (crag_index.h MAX_WS): a block of records each
constexpr int PF_STAT_SLOTS = 2048;           // per-query statistics records (summed on the host when read)
constexpr int PF_MIN_ROWS_PER_GROUP = 128;    // below this many rows per workgroup the plain fp32 scan is used
// Wait schedule of the mirror scan (prefilter_kernel's FRAG).  A mirror up to the size of the 256 MiB Infinity Cache
// takes the per-fragment waits, a larger one whole-tile bursts.  From the sweep in DESIGN.md 4.1: the per-fragment
// schedule wins 0.3-1.2 us per search up to 125 000 rows (244 MiB), ties at 150 000 (293 MiB) and loses at 250 000.
enum PfWaits { PF_WAITS_TILE = 0, PF_WAITS_FRAGMENT = 1 };
constexpr int64_t PF_FRAG_WAITS_MAX_BYTES = 256ll << 20;

struct PrepParams {
    const float *queries;     // [nq, dim] row-major fp32
    int nq, dim;
    float *qinv;              // [nq_pad]
    float *a32;               // nullable (a prefilter search: nothing reads them); [nq_pad/32][8 waves][16][64] float4:
                              // raw queries in fp32 A-fragment order, the fp32 scan kernels' A operand
    _Float16 *a16;            // nullable; [nq_pad/32][8 waves][8][64][8]: unit queries in fp16 A-fragment order
};

struct PfParams {
    const float *corpus;
    const _Float16 *corpus16; // fp16 mirror of the unit rows in B-operand order (nullable: scan the fp32 rows)
    const float *inv_norm;
    const _Float16 *a16;
    const float *qinv;
    const uint32_t *mask;
    int64_t mask_stride_w;
    uint32_t *gbound;         // [nq_pad][PF_BOUND_CELLS] class maxima (orderable scores, atomic max)
    const uint32_t *gbound_idle;  // [>= G][PF_BOUND_CELLS] zeros that nothing writes: where the loads of dead queries go
    uint2 *cand;              // [nq_pad][cap]: x = orderable approximate score, y = row position
    uint32_t *count;          // [nq_pad]
    uint32_t *flags;          // [0] = sequence number of the search whose candidate list overflowed, [1] = fallback tickets
    uint32_t seq;             // this search's sequence number on its workspace (never 0)
    int64_t n_rows;
    int nq, k, G, reverse;
    int sets;                 // 1, 2 or 4 class sets (32 * sets >= k)
    int pub0;                 // rows of a workgroup's FIRST tile that publish their score per query (sets > 1): sets, or 8
    int nt;                   // corpus loads with the streaming cache policy (corpus larger than the Infinity Cache)
    int derive_lag, read_lag; // tiles between a publish of class maxima and the delegates' derivation / every wave's read
    int cap;
};

struct FinParams {
    const float *corpus;
    const float *inv_norm;
    const float *qinv;          // (the raw queries themselves: scan.queries / scan.dim)
    const uint2 *cand;
    uint32_t *count;            // [nq_pad]; zeroed per query after use
    uint32_t *gbound;           // [nq_pad][PF_BOUND_CELLS]; zeroed per query after use
    const uint32_t *flags;
    uint32_t seq;
    const int64_t *ids;
    int64_t *out_ids;
    float *out_scores;
    int32_t *out_counts;
    unsigned long long *stats;  // nullable; the workspace's PF_STAT_SLOTS / PF_STAT_WS records {candidates, rescored rows, searches}
    int k, cap;
    int nq;                     // selection blocks of the launch: [0, nq * rsplit)
    int rsplit;                 // selection blocks per query (R)
    uint64_t *xkeys;            // R > 1: [nq][R][k] exact keys of each block's own top-k
    int64_t *xids;              //        [nq][R][k] their external ids
    uint2 *xcount;              //        [nq][R] {keys written, rows rescored}
    uint32_t *xticket;          //        [nq] arrival tickets, zero between searches
    // fallback role (flags[0] != 0: a candidate list overflowed): fb_blocks = scan.G * ceil(nq / 32) workgroups behind
    // the selection blocks run the exact fp32 scan, the one that finishes last merges
    int fb_blocks;
    uint32_t *fb_done;          // ticket counter, zero between searches
    unsigned long long *trace;  // nullable (developer probe, CRAG_PHASE_TRACE=1): 100 MHz timestamps of the phases of the
                                // selection blocks of query 0: [rpart * 16 + phase]

    ScanParams scan;
    MergeParams merge;
};

struct XMergeParams {
    const int64_t *ids;
    const float *scores;
    const int32_t *counts;
    int64_t *out_ids;
    float *out_scores;
    int32_t *out_counts;
    int64_t stride_ids, stride_scores, stride_counts;  // elements between consecutive lists
    int n_lists;
    int nq;
    int k;
};

// kernel_name (nullable) receives the name of the kernel that was launched (a string literal)
hipError_t launch_scan(const ScanParams &p, int q_blocks, hipStream_t st, const char **kernel_name);
hipError_t launch_prep_queries(const PrepParams &p, int nq_pad, hipStream_t st);
// passes = number of 32*nqb-query passes (grid.y); nqb = 1 or 2; frag_waits: the per-fragment wait schedule (mirror
// with plain loads only, see pf_waits_for)
hipError_t launch_prefilter(const PfParams &p, int nqb, int passes, int frag_waits, hipStream_t st,
                            const char **kernel_name);
hipError_t launch_finalize(const FinParams &p, hipStream_t st);
hipError_t launch_merge_partials(const MergeParams &p, int nq, hipStream_t st);
hipError_t launch_merge_results(const XMergeParams &p, hipStream_t st);
hipError_t launch_store_rows(const float *rows, int dim, int64_t pos, int64_t n, float *corpus,
                             float *inv_norm, uint32_t *irregular, _Float16 *mirror, hipStream_t st);
hipError_t launch_load_rows(const float *corpus, int dim, int64_t pos, int64_t n, float *rows, int piece_shift,
                            hipStream_t st);
// fp32 row layout (pieces of 2^shift float4 per row and tile): 5 for an index with the fp16 mirror, 2 without
inline int crag_piece_shift(bool has_mirror) { return has_mirror ? 5 : 2; }
hipError_t launch_count_eligible(const float *inv_norm, int64_t n, const uint32_t *mask,
                                 unsigned long long *out, hipStream_t st);
hipError_t launch_check_ids(const int64_t *ids, int64_t n, int64_t prev, unsigned long long *out_bad,
                            hipStream_t st);
hipError_t launch_fill_ids(int64_t *ids, int64_t pos, int64_t n, int64_t first, hipStream_t st);

// ---- in-place edits (crag_edit.hip) ----
// the four arrays a row lives in: the index's own, or a bounce buffer laid out like so many rows of the index
struct RowStore {
    float *corpus;        // tile32 layout
    _Float16 *mirror;     // nullable; with it the fp32 rows are PS_BIG, without PS_SMALL
    float *inv_norm;
    int64_t *ids;
};
// binary search of ids[0, n) in the ascending stored[0, size): pos (nullable) = stored ids below each (+ j with
// add_index), drop (nullable) = bit mask of the positions found, found (nullable) += their number
hipError_t launch_lookup_ids(const int64_t *stored, int64_t size, const int64_t *ids, int64_t n, int64_t *pos,
                             int add_index, uint32_t *drop, unsigned long long *found, hipStream_t st);
// source position of destinations [d0, d0 + m): of a removal (keep mask + its per-word popcount prefix, n_words + 1
// entries) / of an insertion (newpos ascending; -1 marks the slot of a new row)
hipError_t launch_remove_srcpos(const uint32_t *keep, const uint32_t *prefix, int64_t n_words, int64_t d0, int64_t m,
                                int64_t *srcpos, hipStream_t st);
hipError_t launch_insert_srcpos(const int64_t *newpos, int64_t n_new, int64_t d0, int64_t m, int64_t *srcpos,
                                hipStream_t st);
// one chunk: index rows srcpos[0, m) -> bounce rows [0, m) -> index rows [d0, d0 + m) (two launches in stream order)
hipError_t launch_move_rows(const RowStore &index, const RowStore &bounce, const int64_t *srcpos, int64_t d0, int64_t m,
                            hipStream_t st);
// launch_store_rows' bits at listed positions, + the ids
hipError_t launch_store_rows_at(const float *rows, int dim, const int64_t *dstpos, const int64_t *new_ids, int64_t n,
                                const RowStore &index, uint32_t *irregular, hipStream_t st);
hipError_t launch_clear_rows(const RowStore &index, int64_t pos, int64_t n, hipStream_t st);
// *flag = 1 when a row of [0, n) has a norm outside [1e-30, 1e30] (the caller zeroes it first)
hipError_t launch_irregular_flag(const float *inv_norm, int64_t n, uint32_t *flag, hipStream_t st);

// ---- BM25 lexical lane (crag_bm25.hip) ----
constexpr int BM25_RANGE = 16384;             // row positions per workgroup: their fp32 accumulators fill 64 KiB of LDS
constexpr int BM25_MAX_Q = 64;

struct Bm25Params {
    const int64_t *post_ptr;    // [V + 1] postings of term t: [post_ptr[t], post_ptr[t + 1])
    const int32_t *post_pos;    // [nnz] row positions, ascending inside a term
    const uint16_t *post_tf;    // [nnz]
    const int32_t *doc_len;     // [n]
    const int64_t *ids;         // [n], nullable (ids = positions)
    const int32_t *q_ptr;       // [nq + 1] terms of query q: [q_ptr[q], q_ptr[q + 1])
    const int32_t *q_term;      // term ids, strictly ascending inside a query
    const float *q_w;           // qtf * idf * (k1 + 1)
    const uint32_t *mask;       // nullable
    int64_t mask_stride_w;      // words between the masks of consecutive queries (0: shared)
    uint64_t *part_keys;        // [nq][n_ranges][k] (score bits << 32) | ~position, best first
    int32_t *part_cnt;          // [nq][n_ranges]
    int64_t n;
    int n_ranges, nq, k;
    float avgdl;
    int64_t *out_ids;
    float *out_scores;
    int32_t *out_counts;
};
int64_t bm25_scratch_bytes(int64_t n_rows, int nq, int k);
hipError_t launch_bm25(const Bm25Params &p, hipStream_t st);

// ---- BM25 query clauses and any-of groups as row masks (crag_bm25_clause.hip) ----
constexpr int BM25_RANGE_WORDS = BM25_RANGE / 32;   // mask words one workgroup owns
constexpr int BM25_CLAUSE_MAX = 16;                 // constraint clauses per query
constexpr int BM25_PHRASE_MAX = 8;                  // terms per phrase
constexpr int BM25_KIND_REQ_TERM = 0, BM25_KIND_EXC_TERM = 1, BM25_KIND_REQ_PHRASE = 2, BM25_KIND_EXC_PHRASE = 3,
              BM25_KIND_NOTHING = 4;
constexpr int BM25_GROUP_MAX = 16;                  // any-of groups per query
constexpr int BM25_GROUP_REQ = 0, BM25_GROUP_EXC = 1;

// one block for both mask kernels: "clause" below is a clause of bm25_clause_mask_kernel or a group of
// bm25_group_mask_kernel (whose launch leaves post_off, post_where and has_phrase unset)
struct Bm25MaskParams {
    const int64_t *post_ptr;     // [V + 1]
    const int32_t *post_pos;     // [nnz] row positions, ascending inside a term
    const int64_t *post_off;     // [nnz + 1] token positions of posting j: post_where[post_off[j] .. post_off[j + 1])
    const uint16_t *post_where;  // token positions, ascending inside a posting (NULL with post_off: no phrase clause)
    const int32_t *c_ptr;        // [nq + 1] clauses of query q: [c_ptr[q], c_ptr[q + 1]), at most BM25_CLAUSE_MAX / _GROUP_MAX
    const int32_t *c_kind;       // [n_clauses] BM25_KIND_* / BM25_GROUP_*
    const int32_t *ct_ptr;       // [n_clauses + 1] terms of clause c: ct_terms[ct_ptr[c] .. ct_ptr[c + 1]); a group: at most 64
    const int32_t *ct_terms;     // term ids, in phrase order
    const uint32_t *in;          // nullable: every row below n is admitted
    int64_t in_stride_w;         // mask words per input run, 0: one run shared by all queries
    uint32_t *out;               // [nq][stride_w]
    int64_t stride_w;            // mask words per output run
    int64_t n, n_words;          // rows; ceil(n / 32): the words an input run is sure to hold
    int nq;
    int has_phrase;              // some clause is a phrase: the kernel variant with the phrase's LDS
};
hipError_t launch_bm25_clause(const Bm25MaskParams &p, hipStream_t st);
hipError_t launch_bm25_groups(const Bm25MaskParams &p, hipStream_t st);

// ---- BM25 prefix and fuzzy terms expanded over the vocabulary (crag_bm25_expand.hip) ----
constexpr int BM25_EXPAND_SLICE = 4096;             // vocabulary terms per workgroup of the match kernel
constexpr int BM25_EXPAND_KEEP = 64;                // kept expansions per pattern (CRAG_BM25_MAX_EXPANSIONS)
constexpr int BM25_EXPAND_MAX_PATTERNS = 512;       // patterns per call
constexpr int BM25_EXPAND_MAX_BYTES = 255;          // bytes per pattern (the tokenizer's limit)
constexpr int BM25_EXPAND_PREFIX = 0, BM25_EXPAND_FUZZY1 = 1, BM25_EXPAND_FUZZY2 = 2;

struct Bm25ExpandParams {
    const int64_t *term_ptr;     // [V + 1] byte offsets of the terms in term_bytes
    const uint8_t *term_bytes;   // UTF-8, term-id order
    const int64_t *post_ptr;     // [V + 1]: df(t) = post_ptr[t + 1] - post_ptr[t]
    const int32_t *pat_ptr;      // [np + 1] byte offsets of the patterns in pat_bytes
    const int32_t *pat_kind;     // [np] BM25_EXPAND_*
    const uint8_t *pat_bytes;
    uint64_t *slice_keys;        // [np][n_slices][BM25_EXPAND_KEEP] sorted descending, 0 padded
    int32_t *slice_count;        // [np][n_slices] matches of the slice
    int32_t *out_terms;          // [np][BM25_EXPAND_KEEP] -1 padded
    int32_t *out_dist;           // [np][BM25_EXPAND_KEEP] -1 padded
    int32_t *out_kept;           // [np]
    int64_t *out_total;          // [np]
    int64_t n_terms;
    int n_slices;
    int np;
    int pat_chunk;               // patterns per workgroup of the match kernel (blockIdx.y picks the chunk)
};
int64_t bm25_expand_scratch_bytes(int64_t n_terms, int np);
hipError_t launch_bm25_expand(const Bm25ExpandParams &p, hipStream_t st);

// ---- BM25 query-aware snippet windows (crag_bm25_snippet.hip) ----
constexpr int BM25_SNIPPET_TERMS = 64;              // term slots per query: one per lane (CRAG_BM25_SNIPPET_MAX_TERMS)
constexpr int BM25_SNIPPET_STAGE = 1024;            // positions of one pair the kernel keeps in LDS (bm25.SNIPPET_STAGE)

struct Bm25SnippetParams {
    const int64_t *post_ptr;     // [V + 1]
    const int32_t *post_pos;     // [nnz] row positions, ascending inside a term
    const int64_t *post_off;     // [nnz + 1] token positions of posting j: post_where[post_off[j] .. post_off[j + 1])
    const uint16_t *post_where;  // token positions, ascending inside a posting
    const int32_t *q_ptr;        // [nq + 1] slots of query q: [q_ptr[q], q_ptr[q + 1]), at most BM25_SNIPPET_TERMS
    const int32_t *terms;        // term ids
    const float *weights;
    const int32_t *r_ptr;        // [nq + 1] pairs of query q: [r_ptr[q], r_ptr[q + 1])
    const int32_t *rows;         // [npairs] row positions
    int32_t *out_start;          // [npairs]
    int32_t *out_last;
    float *out_score;
    uint64_t *out_covered;
    int nq, npairs, window;
};
hipError_t launch_bm25_snippets(const Bm25SnippetParams &p, hipStream_t st);


// ---- near-duplicate suppression of ranked lists (crag_dedupe.hip) ----
struct DedupeParams {
    RowView rows;               // the stored rows (crag_rows.h)
    const int64_t *ids;         // [nq, width] ranked lists, best first
    const int32_t *counts;      // [nq], clamped to [0, width]
    int width;                  // <= CRAG_DEDUPE_MAX_WIDTH
    float threshold;
    int64_t *out_ids;           // [nq, width] kept ids in their order, -1 padded
    int32_t *out_counts;        // [nq]
    int32_t *out_dup_of;        // nullable [nq, width]: -1 kept, else the slot of the suppressor
    float *out_sim;             // nullable [nq, width]: that pair's cosine, NaN where kept
};
hipError_t launch_dedupe(const DedupeParams &p, int nq, hipStream_t st);

// ---- exact top-k and scores over listed rows (crag_subset.hip) ----
struct SubsetParams {
    RowView rows;               // the stored rows (crag_rows.h)
    const float *queries;       // [nq, dim] row-major fp32, raw
    int nq, dim, k;
    const int64_t *ids;         // [nq, width] lists (list_stride == width) or one shared [width] list (list_stride == 0)
    const int32_t *counts;      // [nq] / [1], clamped to [0, width]
    int width;                  // <= CRAG_SUBSET_MAX_WIDTH
    int64_t list_stride;
    uint64_t *keys;             // scratch [nq, width]: (orderable score << 32) | ~position per slot, 0 = ignored
    int64_t *out_ids;           // [nq, k], -1 padded
    float *out_scores;          // [nq, k], NaN padded
    int32_t *out_counts;        // [nq]
    float *out_slot_scores;     // nullable [nq, width]: the score of each input slot, NaN where ignored
};
int64_t subset_scratch_bytes(int nq, int width);
hipError_t launch_subset(const SubsetParams &p, hipStream_t st);

// ---- exact top-k under "at most per_group rows per group" (crag_group.hip) ----
struct GroupParams {
    RowView rows;               // the stored rows (crag_rows.h)
    const float *queries;       // [nq, dim] row-major fp32, raw
    int nq, dim, k;
    const int32_t *row_group;   // [size] group number by row position; outside [0, n_groups): the row is ignored
    int64_t n_groups;
    int per_group;              // <= CRAG_GROUP_MAX_PER
    const uint32_t *mask;       // nullable; 32 rows per word
    int64_t mask_stride_w;      // words between consecutive queries' masks (0 = shared)
    uint64_t *table;            // scratch [nq][n_groups][per_group] keys, best first, 0 = empty
    float *qinv;                // scratch [nq] the canonical 1/||q|| (0: zero / non-finite query)
    int64_t *out_ids;           // [nq, k], -1 padded
    float *out_scores;          // [nq, k], NaN padded
    int32_t *out_groups;        // nullable [nq, k], -1 padded
    int32_t *out_counts;        // [nq]
};
// the table, then the 1/||q|| (padded to 8 bytes)
int64_t group_scratch_bytes(int nq, int64_t n_groups, int per_group);
hipError_t launch_grouped(const GroupParams &p, hipStream_t st);

// ---- MMR diversification of ranked lists (crag_mmr.hip) ----
struct MmrParams {
    RowView rows;               // the stored rows (crag_rows.h)
    const int64_t *ids;         // [nq, width]
    const float *rel;           // [nq, width] relevance of each slot
    const int32_t *counts;      // [nq], clamped to [0, width]
    int nq, width, k;           // width, k <= CRAG_MMR_MAX_WIDTH
    float lambda, mu;           // mu = 1.0f - lambda, rounded once on the host
    float *gram;                // scratch [nq][width_pad][width_pad] pair cosines, NaN: not comparable
    int64_t *out_ids;           // [nq, k] picks in pick order, -1 padded
    float *out_rel;             // [nq, k], NaN padded
    float *out_value;           // nullable [nq, k] the winning value, NaN padded
    int32_t *out_slots;         // nullable [nq, k] the input slot of each pick, -1 padded
    float *out_sim_rows;        // nullable [nq, k, width] cos(pick, slot), NaN: not comparable / ignored / no pick
    int32_t *out_counts;        // [nq]
};
// the queries' Gram matrices: width rounded up to whole blocks of 32, squared, fp32
int64_t mmr_scratch_bytes(int nq, int width);
hipError_t launch_mmr(const MmrParams &p, hipStream_t st);

}  // namespace crag
