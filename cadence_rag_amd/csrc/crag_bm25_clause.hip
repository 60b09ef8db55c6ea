// crag_bm25_clause.hip -- query clauses of the BM25 lane as row masks on the GPU (gfx950), DESIGN.md 4.7c.
// The reference hands the user's string to `text @@@ :query` (app/retrieve.py:141,173), where pg_search runs Tantivy's
// query parser: `+timeout -staging "connection reset"` means something there.  The rule here is this tree's own
// (include/crag_dense.h states it): the host parses the string into clauses -- required term, excluded term, required
// phrase, excluded phrase --, this unit turns a batch's clauses into one row mask per query, and the two kernels of
// crag_bm25.hip score under that mask with the bits they always had.
//
// bm25_clause_mask_kernel, grid (ranges of BM25_RANGE row positions, queries): a workgroup owns the 512 mask words of its
// range and query, one word per thread.  `keep` starts as the input mask (all ones below n without one) and every clause
// ANDs into it:
//   - all clause terms' range bounds come from binary searches on post_pos, one term per lane, in one round;
//   - a term clause streams the term's postings of the range (coalesced), sets their bits in `tmp` with LDS atomicOr,
//     and then keep &= tmp (required) or keep &= ~tmp (excluded);
//   - a phrase clause streams every member term into a bitmap of its own, keeps the number of set bits in front of every
//     word beside it, ANDs the bitmaps with `keep` into a candidate set and compacts the candidates' local positions into
//     an LDS list (block prefix sums over the words' popcounts: the list is ascending, whatever the scheduling).  One
//     candidate row per lane: the row's posting in a member's range slice is the slice's start plus the row's rank in the
//     member's bitmap (postings ascend), the member with the fewest positions anchors the walk, and every anchor position
//     is checked against the other members' post_where slices by binary search.  Matches are set in `tmp`; keep &= tmp or
//     &= ~tmp.  A launch without a phrase clause runs the variant without the phrase's 56 KiB of LDS;
//   - a range whose keep is all zero skips the clauses left (also the searches: a range beyond n reads no posting).
// Every word of the run is then written with a plain store -- the words beyond ceil(n / 32) and the bits beyond n are 0
// because keep never held them.  Integer work only, no global atomics, LDS atomics are ORs: the output is a function of
// the input alone.
// Known weakness: the lanes of one wave that stream a dense term OR into the same LDS word one after another (up to 32
// postings per word); a term that fills its range pays 32 serialised ORs per wave instruction.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int CL_THREADS = BM25_RANGE_WORDS;                     // one thread per mask word of the range
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_TERMS = BM25_CLAUSE_MAX * BM25_PHRASE_MAX;      // clause terms of one query, at most

static_assert(CL_THREADS == 512 && CL_TERMS <= CL_THREADS, "one lane per clause term in the search round");
static_assert(BM25_RANGE <= 65536, "the candidate list holds local positions in 16 bits");
static_assert(BM25_CLAUSE_MAX == CRAG_BM25_MAX_CLAUSES && BM25_PHRASE_MAX == CRAG_BM25_MAX_PHRASE, "one set of limits");

// is token position x in where[a .. a + len) (ascending)?
__device__ __forceinline__ bool cl_has_where(const uint16_t *where, int64_t a, int len, int x) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)where[a + mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && (int)where[a + lo] == x;
}

// tmp |= the rows of [base, end) that hold the term whose postings of the range are post_pos[l0 .. l0 + len)
__device__ __forceinline__ void cl_stream_term(const int32_t *post_pos, int64_t l0, int len, int64_t base, int64_t end,
                                               uint32_t *tmp, int tid) {
    for (int i = tid; i < len; i += CL_THREADS) {
        const int64_t li = (int64_t)post_pos[l0 + i] - base;
        if ((uint64_t)li >= (uint64_t)(end - base)) continue;   // (a list that does not ascend)
        atomicOr(&tmp[li >> 5], 1u << (li & 31));
    }
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
__global__ __launch_bounds__(CL_THREADS) void bm25_clause_mask_kernel(Bm25ClauseParams p) {
    __shared__ uint32_t keep[CL_THREADS];
    __shared__ uint32_t tmp[CL_THREADS];
    __shared__ int64_t s_lo[CL_TERMS];
    __shared__ int s_len[CL_TERMS];
    __shared__ int s_wtot[CL_WAVES];
    const int rg = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t gw = (int64_t)rg * BM25_RANGE_WORDS + tid;
    const int64_t base = (int64_t)rg * BM25_RANGE;
    int64_t end = base + BM25_RANGE < p.n ? base + BM25_RANGE : p.n;
    if (end < base) end = base;   // a range of the stride padding: no rows

    uint32_t word = 0;
    if (gw < p.n_words) {
        word = p.in ? p.in[(int64_t)q * p.in_stride_w + gw] : 0xffffffffu;
        if (gw == p.n_words - 1 && (p.n & 31)) word &= (1u << (p.n & 31)) - 1u;
    }
    keep[tid] = word;
    const int c0 = p.c_ptr[q], c1 = p.c_ptr[q + 1];
    bool alive = c1 > c0 && __syncthreads_or(word != 0u);   // (c1 > c0 is uniform)
    if (alive) {
        const int tt0 = p.ct_ptr[c0], ntm = p.ct_ptr[c1] - tt0;   // <= CL_TERMS (the host checked the limits)
        if (tid < ntm) {   // lanes search different terms: the workgroup pays one latency chain
            const int term = p.ct_terms[tt0 + tid];
            const int64_t a = p.post_ptr[term], b = p.post_ptr[term + 1];
            const int64_t lo = lower_bound_asc(p.post_pos, a, b, base);
            const int64_t hi = lower_bound_asc(p.post_pos, lo, b, end);
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
                cl_stream_term(p.post_pos, s_lo[a], s_len[a], base, end, tmp, tid);
                __syncthreads();
                keep[tid] = kind == BM25_KIND_REQ_TERM ? keep[tid] & tmp[tid] : keep[tid] & ~tmp[tid];
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
                    cl_stream_term(p.post_pos, s_lo[a + j], s_len[a + j], base, end, mbits[j], tid);
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
                                if ((int64_t)p.post_pos[pi] == base + li) {   // (fails only for a list that does not ascend)
                                    wa[i] = p.post_off[pi];
                                    const int64_t len = p.post_off[pi + 1] - wa[i];
                                    wl[i] = len > 0 ? (int)(len < 65536 ? len : 65536) : 0;
                                }
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
                keep[tid] = kind == BM25_KIND_REQ_PHRASE ? keep[tid] & tmp[tid] : keep[tid] & ~tmp[tid];
            } else {   // "matches nothing" (a phrase cannot be here: the host launches PHRASES for one)
                keep[tid] = 0u;
                break;
            }
            // (the barrier of this vote also orders this clause's reads of tmp before the next clause zeroes it)
            alive = __syncthreads_or(keep[tid] != 0u);
        }
    }
    // keep[tid] is this thread's own word from the first line to the last: no barrier is needed for it
    if (gw < p.stride_w) p.out[(int64_t)q * p.stride_w + gw] = keep[tid];
}

}  // namespace

hipError_t launch_bm25_clause(const Bm25ClauseParams &p, hipStream_t st) {
    const int64_t n_ranges = (p.stride_w + BM25_RANGE_WORDS - 1) / BM25_RANGE_WORDS;
    if (n_ranges > 0) {
        const dim3 grid((unsigned)n_ranges, (unsigned)p.nq), block(CL_THREADS);
        if (p.has_phrase) hipLaunchKernelGGL(bm25_clause_mask_kernel<true>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(bm25_clause_mask_kernel<false>, grid, block, 0, st, p);
    }
    return hipGetLastError();
}

}  // namespace crag

extern "C" int crag_bm25_clause_masks_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const int64_t *d_post_off,
                                           const uint16_t *d_post_where, int64_t n_rows, int64_t n_terms,
                                           const int32_t *h_c_ptr, const int32_t *h_c_kind, const int32_t *h_ct_ptr,
                                           const int32_t *h_ct_terms, int nq, const uint8_t *d_in_mask, int64_t in_stride,
                                           crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride,
                                           void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (nq < 1 || nq > crag::BM25_MAX_Q) return fail(CRAG_EINVAL, "bm25_clause_masks_host: need 1 <= nq <= 64 (nq=%d)", nq);
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(CRAG_EINVAL, "bm25_clause_masks_host: n_rows must be in [0, 2^31)");
    if (n_terms < 0 || n_terms > INT32_MAX) return fail(CRAG_EINVAL, "bm25_clause_masks_host: n_terms must be in [0, 2^31)");
    const int64_t min_stride = (n_rows + 31) / 32 * 4;
    if (mask_stride < 0 || mask_stride % 4 != 0 || mask_stride < min_stride || mask_stride > ((int64_t)1 << 32))
        return fail(CRAG_EINVAL, "bm25_clause_masks_host: mask_stride must be a multiple of 4 in [ceil(n_rows/32)*4, 2^32]");
    if (d_in_mask && in_stride != 0 && (in_stride % 4 != 0 || in_stride < min_stride || in_stride > ((int64_t)1 << 32)))
        return fail(CRAG_EINVAL, "bm25_clause_masks_host: in_stride must be 0 or a multiple of 4 in [ceil(n_rows/32)*4, 2^32]");
    if (!h_c_ptr || !slot) return fail(CRAG_EINVAL, "bm25_clause_masks_host: NULL pointer argument");
    if (n_rows > 0 && (!d_post_ptr || !d_post_pos)) return fail(CRAG_EINVAL, "bm25_clause_masks_host: NULL postings pointer");
    if (mask_stride > 0 && !d_out_mask) return fail(CRAG_EINVAL, "bm25_clause_masks_host: NULL output pointer");
    if (((uintptr_t)d_out_mask & 3) != 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: the output must be 4-byte aligned");
    if (((uintptr_t)d_in_mask & 3) != 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: the input mask must be 4-byte aligned");
    if (h_c_ptr[0] != 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: c_ptr[0] must be 0");
    for (int q = 0; q < nq; ++q) {
        const int64_t cnt = (int64_t)h_c_ptr[q + 1] - h_c_ptr[q];
        if (cnt < 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: c_ptr must not descend (query %d)", q);
        if (cnt > CRAG_BM25_MAX_CLAUSES)
            return fail(CRAG_EINVAL, "bm25_clause_masks_host: query %d has %lld clauses, at most %d", q, (long long)cnt,
                        CRAG_BM25_MAX_CLAUSES);
    }
    const int nc = h_c_ptr[nq];
    if (nc > 0 && (!h_c_kind || !h_ct_ptr)) return fail(CRAG_EINVAL, "bm25_clause_masks_host: NULL clause arrays");
    if (nc > 0 && h_ct_ptr[0] != 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: ct_ptr[0] must be 0");
    bool has_phrase = false;
    for (int c = 0; c < nc; ++c) {
        const int kind = h_c_kind[c];
        const int64_t m = (int64_t)h_ct_ptr[c + 1] - h_ct_ptr[c];
        if (m < 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: ct_ptr must not descend (clause %d)", c);
        switch (kind) {
        case crag::BM25_KIND_REQ_TERM:
        case crag::BM25_KIND_EXC_TERM:
            if (m != 1) return fail(CRAG_EINVAL, "bm25_clause_masks_host: term clause %d must hold exactly one term", c);
            break;
        case crag::BM25_KIND_REQ_PHRASE:
        case crag::BM25_KIND_EXC_PHRASE:
            if (m < 2 || m > CRAG_BM25_MAX_PHRASE)
                return fail(CRAG_EINVAL, "bm25_clause_masks_host: phrase clause %d must hold 2..%d terms", c, CRAG_BM25_MAX_PHRASE);
            if (!d_post_off || !d_post_where)
                return fail(CRAG_EINVAL, "bm25_clause_masks_host: a phrase clause needs the position arrays");
            has_phrase = true;
            break;
        case crag::BM25_KIND_NOTHING:
            if (m != 0) return fail(CRAG_EINVAL, "bm25_clause_masks_host: clause %d of kind 4 must hold no term", c);
            break;
        default:
            return fail(CRAG_EINVAL, "bm25_clause_masks_host: clause %d has the unknown kind %d", c, kind);
        }
        if (m > 0 && !h_ct_terms) return fail(CRAG_EINVAL, "bm25_clause_masks_host: NULL term array");
        for (int i = h_ct_ptr[c]; i < h_ct_ptr[c + 1]; ++i)
            if (h_ct_terms[i] < 0 || (int64_t)h_ct_terms[i] >= n_terms)
                return fail(CRAG_EINVAL, "bm25_clause_masks_host: term id %d of clause %d is outside [0, n_terms)", h_ct_terms[i], c);
    }
    if (mask_stride == 0) return CRAG_OK;   // (n_rows is 0: the runs are empty)

    const int ntm = nc > 0 ? h_ct_ptr[nc] : 0;
    // slot layout: c_ptr [BM25_MAX_Q + 4] int32 | c_kind [nc] | ct_ptr [nc + 1] | ct_terms [ntm]
    const size_t head = (size_t)(crag::BM25_MAX_Q + 4) * 4;
    const size_t bytes = head + ((size_t)nc + (size_t)nc + 1 + (size_t)ntm) * 4;
    void *h = nullptr, *d = nullptr;
    int rc = crag_upload_slot_begin_(slot, bytes, &h, &d);
    if (rc != CRAG_OK) return rc;
    int32_t *hk = (int32_t *)((char *)h + head), *hp = hk + nc, *ht = hp + nc + 1;
    memcpy(h, h_c_ptr, (size_t)(nq + 1) * 4);
    if (nc > 0) {
        memcpy(hk, h_c_kind, (size_t)nc * 4);
        memcpy(hp, h_ct_ptr, (size_t)(nc + 1) * 4);
        if (ntm > 0) memcpy(ht, h_ct_terms, (size_t)ntm * 4);
    } else {
        hp[0] = 0;
    }
    rc = crag_upload_slot_commit_(slot, bytes, stream);
    if (rc != CRAG_OK) return rc;

    crag::Bm25ClauseParams p;
    p.post_ptr = d_post_ptr;
    p.post_pos = d_post_pos;
    p.post_off = d_post_off;
    p.post_where = d_post_where;
    p.c_ptr = (const int32_t *)d;
    p.c_kind = (const int32_t *)((const char *)d + head);
    p.ct_ptr = p.c_kind + nc;
    p.ct_terms = p.ct_ptr + nc + 1;
    p.in = (const uint32_t *)d_in_mask;
    p.in_stride_w = d_in_mask ? in_stride / 4 : 0;
    p.out = (uint32_t *)d_out_mask;
    p.stride_w = mask_stride / 4;
    p.n = n_rows;
    p.n_words = (n_rows + 31) / 32;
    p.nq = nq;
    p.has_phrase = has_phrase ? 1 : 0;
    HIP_TRY(crag::launch_bm25_clause(p, (hipStream_t)stream));
    return CRAG_OK;
}
