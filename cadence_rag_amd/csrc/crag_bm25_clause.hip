// crag_bm25_clause.hip -- query clauses and any-of groups of the BM25 lane as row masks on the GPU (gfx950), DESIGN.md
// 4.7c and 4.7d.
// The reference hands the user's string to `text @@@ :query` (app/retrieve.py:141,173), where pg_search runs Tantivy's
// query parser: `+timeout -staging "connection reset"` means something there.  The rule here is this tree's own
// (include/crag_dense.h states it): the host parses the string into clauses -- required term, excluded term, required
// phrase, excluded phrase -- and, for prefix and fuzzy items, into any-of groups of the terms they expand to
// (crag_bm25_expand.hip); this unit turns a batch's clauses or groups into one row mask per query, and the two kernels of
// crag_bm25.hip score under that mask with the bits they always had.
//
// Both kernels are one frame (crag_postings.h), grid (ranges of BM25_RANGE row positions, queries): a workgroup owns the
// 512 mask words of its range and query, one word per thread.  `keep` starts as the input mask (all ones below n without
// one) and every clause ANDs into it:
//   - all clause terms' range bounds come from binary searches on post_pos, one term per lane;
//   - a clause's rows are gathered in the LDS bitmap `tmp` (its terms' postings of the range are streamed, coalesced, and
//     their bits set with LDS atomicOr), and then keep &= tmp (required) or keep &= ~tmp (excluded);
//   - a range whose keep is all zero skips the clauses left (also the searches: a range beyond n reads no posting).
// Every word of the run is then written with a plain store -- the words beyond ceil(n / 32) and the bits beyond n are 0
// because keep never held them.  Integer work only, no global atomics, LDS atomics are ORs: the output is a function of
// the input alone.  A required or excluded term clause is an any-of group of one term, "matches nothing" an empty
// required group: the two kernels give the same words for them.
//
// bm25_clause_mask_kernel (at most 128 clause terms, one search round) adds to the frame:
//   - a term clause is streamed by the whole workgroup;
//   - a phrase clause streams every member term into a bitmap of its own, keeps the number of set bits in front of every
//     word beside it, ANDs the bitmaps with `keep` into a candidate set and compacts the candidates' local positions into
//     an LDS list (block prefix sums over the words' popcounts: the list is ascending, whatever the scheduling).  One
//     candidate row per lane: the row's posting in a member's range slice is the slice's start plus the row's rank in the
//     member's bitmap (postings ascend), the member with the fewest positions anchors the walk, and every anchor position
//     is checked against the other members' post_where slices by binary search.  Matches are set in `tmp`.  A launch
//     without a phrase clause runs the variant without the phrase's 56 KiB of LDS.
// bm25_group_mask_kernel (at most 1024 group terms, two search rounds) adds: a group's terms are streamed into the one
// bitmap one term per wave at a time (integer LDS atomicOr: it commutes); an empty excluded group is skipped.
// Known weakness: the lanes of one wave that stream a dense term OR into the same LDS word one after another (up to 32
// postings per word); a term that fills its range pays 32 serialised ORs per wave instruction.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_postings.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int CL_THREADS = BM25_RANGE_WORDS;                     // one thread per mask word of the range
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_TERMS = BM25_CLAUSE_MAX * BM25_PHRASE_MAX;      // clause terms of one query, at most
constexpr int GR_TERMS = BM25_GROUP_MAX * BM25_EXPAND_KEEP;      // group terms of one query, at most

static_assert(CL_THREADS == 512 && CL_TERMS <= CL_THREADS, "one lane per clause term in the search round");
static_assert(BM25_RANGE <= 65536, "the candidate list holds local positions in 16 bits");
static_assert(BM25_CLAUSE_MAX == CRAG_BM25_MAX_CLAUSES && BM25_PHRASE_MAX == CRAG_BM25_MAX_PHRASE, "one set of limits");
static_assert(BM25_GROUP_MAX == CRAG_BM25_MAX_CLAUSES, "groups count as constraint clauses");

// is token position x in where[a .. a + len) (ascending)?
__device__ __forceinline__ bool cl_has_where(const uint16_t *where, int64_t a, int len, int x) {
    const int lo = lower_bound_u16(where + a, len, x);
    return lo < len && (int)where[a + lo] == x;
}

// exclusive prefix sum of v over the workgroup's threads, and the total; s_wtot: CL_WAVES ints.  Ends with a barrier, so
// that the next call may write s_wtot at once
__device__ __forceinline__ int cl_block_scan(int v, int *s_wtot, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    int off = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) {
        const int t = s_wtot[w];
        if (w < wave) off += t;
        total += t;
    }
    __syncthreads();
    return off;
}

// PHRASES = false: a launch without a phrase clause, which leaves the phrase's 56 KiB of LDS out
template <bool PHRASES>
__global__ __launch_bounds__(CL_THREADS) void bm25_clause_mask_kernel(Bm25MaskParams p) {
    __shared__ uint32_t keep[CL_THREADS];
    __shared__ uint32_t tmp[CL_THREADS];
    __shared__ int64_t s_lo[CL_TERMS];
    __shared__ int s_len[CL_TERMS];
    __shared__ int s_wtot[CL_WAVES];
    const int rg = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t gw = (int64_t)rg * BM25_RANGE_WORDS + tid;
    int64_t base, end;
    range_span(rg, p.n, base, end);

    const uint32_t word = load_mask_word(p.in, p.in_stride_w, q, gw, p.n, p.n_words);
    keep[tid] = word;
    const int c0 = p.c_ptr[q], c1 = p.c_ptr[q + 1];
    bool alive = c1 > c0 && __syncthreads_or(word != 0u);   // (c1 > c0 is uniform)
    if (alive) {
        const int tt0 = p.ct_ptr[c0], ntm = p.ct_ptr[c1] - tt0;   // <= CL_TERMS (the host checked the limits)
        if (tid < ntm) {   // lanes search different terms: the workgroup pays one latency chain
            int64_t lo, hi;
            posting_slice(p.post_ptr, p.post_pos, p.ct_terms[tt0 + tid], base, end, lo, hi);
            s_lo[tid] = lo;
            s_len[tid] = (int)(hi - lo);
        }
        __syncthreads();
        for (int c = c0; c < c1 && alive; ++c) {
            const int kind = p.c_kind[c];
            const int a = p.ct_ptr[c] - tt0, m = p.ct_ptr[c + 1] - p.ct_ptr[c];
            if (kind == BM25_KIND_REQ_TERM || kind == BM25_KIND_EXC_TERM) {
                tmp[tid] = 0u;
                __syncthreads();
                stream_bitmap(p.post_pos, s_lo[a], s_len[a], base, end, tmp, tid, CL_THREADS);
                __syncthreads();
                alive = mask_apply(keep, tmp, tid, kind == BM25_KIND_REQ_TERM);
            } else if constexpr (PHRASES) {
                if (kind == BM25_KIND_NOTHING) {
                    keep[tid] = 0u;
                    break;
                }
                __shared__ uint32_t mbits[BM25_PHRASE_MAX][CL_THREADS];   // the members' bitmaps of the range ...
                __shared__ uint16_t mpre[BM25_PHRASE_MAX][CL_THREADS];    // ... and the set bits in front of every word
                __shared__ uint16_t s_list[BM25_RANGE];                   // local positions of the candidate rows, ascending
                // ---- candidates: rows still kept that hold every member term ----
                uint32_t cw = keep[tid];
                int total = 0;
                for (int j = 0; j < m; ++j) {
                    mbits[j][tid] = 0u;
                    __syncthreads();
                    stream_bitmap(p.post_pos, s_lo[a + j], s_len[a + j], base, end, mbits[j], tid, CL_THREADS);
                    __syncthreads();
                    const uint32_t w = mbits[j][tid];
                    cw &= w;
                    mpre[j][tid] = (uint16_t)cl_block_scan(__popc(w), s_wtot, total);
                }
                // ---- compaction: the candidates' offsets are a prefix sum of the words' popcounts ----
                tmp[tid] = 0u;   // the matches go here
                int off = cl_block_scan(__popc(cw), s_wtot, total);
                for (uint32_t bits = cw; bits; bits &= bits - 1u)
                    s_list[off++] = (uint16_t)(tid * 32 + (__ffs(bits) - 1));
                __syncthreads();
                // ---- verification: one candidate row per lane ----
                for (int ci = tid; ci < total; ci += CL_THREADS) {
                    const int li = s_list[ci], wi = li >> 5, bi = li & 31;
                    int64_t wa[BM25_PHRASE_MAX];
                    int wl[BM25_PHRASE_MAX];
                    bool ok = true;
                    int64_t anc_a = 0;
                    int anc_len = 0x7fffffff, anc_i = 0;
#pragma unroll
                    for (int i = 0; i < BM25_PHRASE_MAX; ++i) {
                        wa[i] = 0;
                        wl[i] = 0;
                        if (i < m) {
                            // the row's posting in the member's slice: postings ascend, so its rank is the number of the
                            // member's rows in front of it -- two LDS reads instead of a binary search in memory
                            const int rank = (int)mpre[i][wi] + __popc(mbits[i][wi] & ((1u << bi) - 1u));
                            if (rank < s_len[a + i]) {
                                const int64_t pi = s_lo[a + i] + rank;
                                if ((int64_t)p.post_pos[pi] == base + li)   // (fails only for a list that does not ascend)
                                    wl[i] = where_slice(p.post_off, pi, wa[i]);
                            }
                            if (wl[i] == 0) ok = false;   // (only positions at or above 65 535, or malformed arrays)
                            if (wl[i] < anc_len) {        // the first member with the fewest positions anchors the walk
                                anc_len = wl[i];
                                anc_a = wa[i];
                                anc_i = i;
                            }
                        }
                    }
                    bool hit = false;
                    if (ok) {
                        for (int x = 0; x < anc_len && !hit; ++x) {
                            const int p0 = (int)p.post_where[anc_a + x] - anc_i;   // where the phrase would start
                            if (p0 < 0) continue;
                            bool all = true;
#pragma unroll
                            for (int i = 0; i < BM25_PHRASE_MAX; ++i)
                                if (all && i < m && i != anc_i) all = cl_has_where(p.post_where, wa[i], wl[i], p0 + i);
                            hit = all;
                        }
                    }
                    if (hit) atomicOr(&tmp[wi], 1u << bi);
                }
                __syncthreads();
                alive = mask_apply(keep, tmp, tid, kind == BM25_KIND_REQ_PHRASE);
            } else {   // "matches nothing" (a phrase cannot be here: the host launches PHRASES for one)
                keep[tid] = 0u;
                break;
            }
        }
    }
    // keep[tid] is this thread's own word from the first line to the last: no barrier is needed for it
    store_mask_word(p.out, p.stride_w, q, gw, keep[tid]);
}

__global__ __launch_bounds__(CL_THREADS) void bm25_group_mask_kernel(Bm25MaskParams p) {
    __shared__ uint32_t keep[CL_THREADS];
    __shared__ uint32_t tmp[CL_THREADS];
    __shared__ int64_t s_lo[GR_TERMS];
    __shared__ int s_len[GR_TERMS];
    const int rg = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t gw = (int64_t)rg * BM25_RANGE_WORDS + tid;
    int64_t base, end;
    range_span(rg, p.n, base, end);

    const uint32_t word = load_mask_word(p.in, p.in_stride_w, q, gw, p.n, p.n_words);
    keep[tid] = word;
    const int g0 = p.c_ptr[q], g1 = p.c_ptr[q + 1];
    bool alive = g1 > g0 && __syncthreads_or(word != 0u);   // (g1 > g0 is uniform)
    if (alive) {
        const int tt0 = p.ct_ptr[g0], ntm = p.ct_ptr[g1] - tt0;   // <= GR_TERMS (the host checked the limits)
        for (int i = tid; i < ntm; i += CL_THREADS) {
            int64_t lo, hi;
            posting_slice(p.post_ptr, p.post_pos, p.ct_terms[tt0 + i], base, end, lo, hi);
            s_lo[i] = lo;
            s_len[i] = (int)(hi - lo);
        }
        __syncthreads();
        for (int g = g0; g < g1 && alive; ++g) {
            const int kind = p.c_kind[g];
            const int a = p.ct_ptr[g] - tt0, m = p.ct_ptr[g + 1] - p.ct_ptr[g];
            if (kind == BM25_GROUP_EXC && m == 0) continue;   // (uniform) an empty excluded group has no effect
            tmp[tid] = 0u;
            __syncthreads();
            for (int j = tid >> 6; j < m; j += CL_WAVES)   // one wave per term
                stream_bitmap(p.post_pos, s_lo[a + j], s_len[a + j], base, end, tmp, tid & 63, 64);
            __syncthreads();
            alive = mask_apply(keep, tmp, tid, kind == BM25_GROUP_REQ);
        }
    }
    // keep[tid] is this thread's own word from the first line to the last: no barrier is needed for it
    store_mask_word(p.out, p.stride_w, q, gw, keep[tid]);
}

}  // namespace

hipError_t launch_bm25_clause(const Bm25MaskParams &p, hipStream_t st) {
    const int64_t n_ranges = (p.stride_w + BM25_RANGE_WORDS - 1) / BM25_RANGE_WORDS;
    if (n_ranges > 0) {
        const dim3 grid((unsigned)n_ranges, (unsigned)p.nq), block(CL_THREADS);
        if (p.has_phrase) hipLaunchKernelGGL(bm25_clause_mask_kernel<true>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(bm25_clause_mask_kernel<false>, grid, block, 0, st, p);
    }
    return hipGetLastError();
}

hipError_t launch_bm25_groups(const Bm25MaskParams &p, hipStream_t st) {
    const int64_t n_ranges = (p.stride_w + BM25_RANGE_WORDS - 1) / BM25_RANGE_WORDS;
    if (n_ranges > 0)
        hipLaunchKernelGGL(bm25_group_mask_kernel, dim3((unsigned)n_ranges, (unsigned)p.nq), dim3(CL_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag

namespace {

// what a clause or group of one kind may hold: min..max terms (min < 0: no such kind), and whether it reads positions
struct MaskKindRule {
    int min_terms, max_terms;
    bool positions;
};

MaskKindRule clause_kind_rule(int kind) {
    switch (kind) {
    case crag::BM25_KIND_REQ_TERM:
    case crag::BM25_KIND_EXC_TERM: return {1, 1, false};
    case crag::BM25_KIND_REQ_PHRASE:
    case crag::BM25_KIND_EXC_PHRASE: return {2, CRAG_BM25_MAX_PHRASE, true};
    case crag::BM25_KIND_NOTHING: return {0, 0, false};
    default: return {-1, -1, false};
    }
}

MaskKindRule group_kind_rule(int kind) {
    if (kind == crag::BM25_GROUP_REQ || kind == crag::BM25_GROUP_EXC) return {0, crag::BM25_EXPAND_KEEP, false};
    return {-1, -1, false};
}

// The two mask entries: `noun` is "clause" or "group" (its first letter heads the names of the entry's CSR arrays:
// c_ptr / ct_ptr, g_ptr / gt_ptr), per_query the number of them one query may hold.
int bm25_masks_host(const char *op, const char *noun, int per_query, MaskKindRule (*rule)(int),
                    hipError_t (*launch)(const crag::Bm25MaskParams &, hipStream_t), const int64_t *d_post_ptr,
                    const int32_t *d_post_pos, const int64_t *d_post_off, const uint16_t *d_post_where, int64_t n_rows,
                    int64_t n_terms, const int32_t *h_ptr, const int32_t *h_kind, const int32_t *h_t_ptr,
                    const int32_t *h_terms, int nq, const uint8_t *d_in_mask, int64_t in_stride, crag_upload_slot *slot,
                    uint8_t *d_out_mask, int64_t mask_stride, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    const char outer[] = {noun[0], '_', 'p', 't', 'r', 0}, inner[] = {noun[0], 't', '_', 'p', 't', 'r', 0};
    int rc = check_bm25_counts(op, nq, 1, n_rows, n_terms);
    if (rc == CRAG_OK) rc = check_mask_strides(op, n_rows, d_in_mask, in_stride, d_out_mask, mask_stride);
    if (rc != CRAG_OK) return rc;
    if (!h_ptr || !slot) return fail(CRAG_EINVAL, "%s: NULL pointer argument", op);
    if (n_rows > 0 && (!d_post_ptr || !d_post_pos)) return fail(CRAG_EINVAL, "%s: NULL postings pointer", op);
    rc = check_csr(op, outer, "query", h_ptr, nq, per_query);
    if (rc != CRAG_OK) return rc;
    const int nc = h_ptr[nq];
    if (nc > 0 && (!h_kind || !h_t_ptr)) return fail(CRAG_EINVAL, "%s: NULL %s arrays", op, noun);
    if (nc > 0 && (rc = check_csr(op, inner, noun, h_t_ptr, nc, -1)) != CRAG_OK) return rc;
    bool has_phrase = false;
    for (int c = 0; c < nc; ++c) {
        const MaskKindRule k = rule(h_kind[c]);
        const int m = h_t_ptr[c + 1] - h_t_ptr[c];
        if (k.min_terms < 0) return fail(CRAG_EINVAL, "%s: %s %d has the unknown kind %d", op, noun, c, h_kind[c]);
        if (m < k.min_terms || m > k.max_terms)
            return fail(CRAG_EINVAL, "%s: %s %d of kind %d holds %d terms, it must hold %d..%d", op, noun, c, h_kind[c], m,
                        k.min_terms, k.max_terms);
        if (k.positions && (!d_post_off || !d_post_where))
            return fail(CRAG_EINVAL, "%s: %s %d needs the position arrays", op, noun, c);
        has_phrase |= k.positions;
    }
    const int ntm = nc > 0 ? h_t_ptr[nc] : 0;
    if (ntm > 0 && !h_terms) return fail(CRAG_EINVAL, "%s: NULL term array", op);
    if ((rc = check_terms(op, h_terms, 0, ntm, n_terms)) != CRAG_OK) return rc;
    if (mask_stride == 0) return CRAG_OK;   // (n_rows is 0: the runs are empty)

    // slot layout: ptr [BM25_MAX_Q + 4] int32 | kind [nc] | t_ptr [nc + 1] | terms [ntm]
    UploadPack up;
    const int i_ptr = up.add(h_ptr, (size_t)nq + 1, (size_t)(crag::BM25_MAX_Q + 4) * 4);
    const int i_kind = up.add(h_kind, (size_t)nc);
    const int i_t_ptr = up.add(h_t_ptr, nc > 0 ? (size_t)nc + 1 : 0, ((size_t)nc + 1) * 4);
    const int i_terms = up.add(h_terms, (size_t)ntm);
    if ((rc = up.begin(slot)) != CRAG_OK) return rc;
    if (nc == 0) *up.host<int32_t>(i_t_ptr) = 0;   // (the caller's t_ptr may be NULL then)
    if ((rc = up.commit(slot, stream)) != CRAG_OK) return rc;

    crag::Bm25MaskParams p = {};
    p.post_ptr = d_post_ptr;
    p.post_pos = d_post_pos;
    p.post_off = d_post_off;
    p.post_where = d_post_where;
    p.c_ptr = up.dev<int32_t>(i_ptr);
    p.c_kind = up.dev<int32_t>(i_kind);
    p.ct_ptr = up.dev<int32_t>(i_t_ptr);
    p.ct_terms = up.dev<int32_t>(i_terms);
    p.in = (const uint32_t *)d_in_mask;
    p.in_stride_w = d_in_mask ? in_stride / 4 : 0;
    p.out = (uint32_t *)d_out_mask;
    p.stride_w = mask_stride / 4;
    p.n = n_rows;
    p.n_words = (n_rows + 31) / 32;
    p.nq = nq;
    p.has_phrase = has_phrase ? 1 : 0;
    HIP_TRY(launch(p, (hipStream_t)stream));
    return CRAG_OK;
}

}  // namespace

extern "C" int crag_bm25_clause_masks_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const int64_t *d_post_off,
                                           const uint16_t *d_post_where, int64_t n_rows, int64_t n_terms,
                                           const int32_t *h_c_ptr, const int32_t *h_c_kind, const int32_t *h_ct_ptr,
                                           const int32_t *h_ct_terms, int nq, const uint8_t *d_in_mask, int64_t in_stride,
                                           crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride,
                                           void *stream) {
    return bm25_masks_host("bm25_clause_masks_host", "clause", CRAG_BM25_MAX_CLAUSES, clause_kind_rule,
                           crag::launch_bm25_clause, d_post_ptr, d_post_pos, d_post_off, d_post_where, n_rows, n_terms,
                           h_c_ptr, h_c_kind, h_ct_ptr, h_ct_terms, nq, d_in_mask, in_stride, slot, d_out_mask, mask_stride,
                           stream);
}

extern "C" int crag_bm25_group_masks_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, int64_t n_rows,
                                          int64_t n_terms, const int32_t *h_g_ptr, const int32_t *h_g_kind,
                                          const int32_t *h_gt_ptr, const int32_t *h_gt_terms, int nq,
                                          const uint8_t *d_in_mask, int64_t in_stride, crag_upload_slot *slot,
                                          uint8_t *d_out_mask, int64_t mask_stride, void *stream) {
    return bm25_masks_host("bm25_group_masks_host", "group", crag::BM25_GROUP_MAX, group_kind_rule,
                           crag::launch_bm25_groups, d_post_ptr, d_post_pos, nullptr, nullptr, n_rows, n_terms, h_g_ptr,
                           h_g_kind, h_gt_ptr, h_gt_terms, nq, d_in_mask, in_stride, slot, d_out_mask, mask_stride, stream);
}
