// crag_bm25_snippet.hip -- query-aware snippet windows of the BM25 word lane on the GPU (gfx950), DESIGN.md 4.7e.
// /retrieve ranks a chunk for the words it holds and then showed its first 800 characters, whichever words those were
// (the reference's APP_SPEC.md:269 asks for snippets that "are actually relevant"; it has no code for it).  The token
// positions of every (row, term) pair are on the device already (post_off / post_where), so choosing
// where a snippet should begin is a lookup and a scan over them.  include/crag_dense.h states the rule.
//
// bm25_snippet_kernel, one wave (= one workgroup) per (query, row) pair:
//   - the pair's query is the one whose r_ptr range holds the pair: one compare per lane, one ballot;
//   - round 1: lane j takes slot j, binary-searches its term's postings for the row (lower_bound_asc) and keeps the
//     posting's post_where slice, or length 0 -- the wave pays one latency chain, not one per term.  The slots the row
//     holds are compacted, in slot order, into LDS with the prefix sum of their lengths (shuffles);
//   - staging: when the pair's positions number at most BM25_SNIPPET_STAGE they are copied to LDS, slice behind slice,
//     and round 2 reads them there; otherwise it reads memory.  Same walk, same bits;
//   - round 2: the occurrences are the candidate starts, dealt to the lanes strided.  For a candidate the kept slots are
//     walked in ascending order; a slot is covered when the lower bound of s in its slice is below s + W, and its weight is
//     added with one rounded fp32 addition.  A lane keeps the largest (score, -s) of its candidates;
//   - the wave reduces that key with xor shuffles: it is a total order, so every lane ends with the same winner whatever
//     the schedule;
//   - lane j then finds its slot's largest position inside the winning window (one lower bound of s + W): the ballot of the
//     lanes that have one is `covered`, the largest of them is `last`.  Lane 0 writes the four outputs with plain stores.
// Integer work and a fixed-order fp32 sum, no atomics: the outputs are a function of the inputs alone.
// A workgroup is one wave because nothing asks for more: 22 VGPRs and 3.3 KiB of LDS leave the CU's cap on waves as the
// only limit on residency, and the two barriers below are then barriers of one wave.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_postings.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int SN_LANES = 64;
static_assert(BM25_SNIPPET_TERMS == SN_LANES && BM25_MAX_Q <= SN_LANES, "one lane per slot, one lane per query");
static_assert(BM25_SNIPPET_TERMS == CRAG_BM25_SNIPPET_MAX_TERMS, "one limit");

// the kept slots of the pair, in slot order
struct SnSlots {
    int64_t off[SN_LANES];      // the slot's slice: post_where[off .. off + len)
    int len[SN_LANES];
    int base[SN_LANES + 1];     // occurrences in front of the slice (where it starts in the staged copy); [cnt] = total
    float w[SN_LANES];
};

// the kept slot that holds occurrence i: the last k with base[k] <= i
__device__ __forceinline__ int sn_slot_of(const SnSlots &sl, int cnt, int i) {
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sl.base[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// round 2 and its reduction; STAGED: the slices are read from `stage`, else from post_where
template <bool STAGED>
__device__ __forceinline__ void sn_search(const SnSlots &sl, const uint16_t *stage, const uint16_t *where, int cnt, int total,
                                          int window, int lane, float &best, int &start) {
    best = -INFINITY;
    start = INT32_MAX;
    for (int i = lane; i < total; i += SN_LANES) {
        int s;
        if constexpr (STAGED) {
            s = stage[i];
        } else {
            const int k = sn_slot_of(sl, cnt, i);
            s = where[sl.off[k] + (i - sl.base[k])];
        }
        float sc = 0.f;
        for (int k = 0; k < cnt; ++k) {
            const int n = sl.len[k];
            int at, v = INT32_MAX;
            if constexpr (STAGED) {
                const uint16_t *a = stage + sl.base[k];
                at = lower_bound_u16(a, n, s);
                if (at < n) v = a[at];
            } else {
                const uint16_t *a = where + sl.off[k];
                at = lower_bound_u16(a, n, s);
                if (at < n) v = a[at];
            }
            if (v < s + window) sc = __fadd_rn(sc, sl.w[k]);
        }
        if (sc > best || (sc == best && s < start)) {
            best = sc;
            start = s;
        }
    }
#pragma unroll
    for (int d = 1; d < SN_LANES; d <<= 1) {
        const float ob = __shfl_xor(best, d);
        const int os = __shfl_xor(start, d);
        if (ob > best || (ob == best && os < start)) {
            best = ob;
            start = os;
        }
    }
}

__global__ __launch_bounds__(SN_LANES) void bm25_snippet_kernel(Bm25SnippetParams p) {
    __shared__ SnSlots sl;
    __shared__ uint16_t stage[BM25_SNIPPET_STAGE];
    const int pair = blockIdx.x, lane = threadIdx.x;
    if (pair >= p.npairs) return;
    const bool mine = lane < p.nq && p.r_ptr[lane] <= pair && pair < p.r_ptr[lane + 1];
    const unsigned long long owner = __ballot(mine);
    if (!owner) return;   // (r_ptr does not cover the pair: the host checked that it does)
    const int q = __ffsll(owner) - 1;
    const int64_t r = p.rows[pair];
    const int t0 = p.q_ptr[q], ns = p.q_ptr[q + 1] - t0;   // <= SN_LANES (the host checked)

    // ---- round 1: lane j looks the row up in the postings of slot j ----
    int64_t off = 0;
    int len = 0;
    float w = 0.f;
    if (lane < ns) {
        const int term = p.terms[t0 + lane];
        w = p.weights[t0 + lane];
        const int64_t a = p.post_ptr[term], b = p.post_ptr[term + 1];
        const int64_t pi = lower_bound_asc(p.post_pos, a, b, r);
        if (pi < b && (int64_t)p.post_pos[pi] == r) len = where_slice(p.post_off, pi, off);
    }
    const unsigned long long kept = __ballot(len > 0);
    if (!kept) {
        if (lane == 0) {
            p.out_start[pair] = -1;
            p.out_last[pair] = 0;
            p.out_score[pair] = 0.f;
            p.out_covered[pair] = 0ull;
        }
        return;
    }
    int incl = len;
#pragma unroll
    for (int d = 1; d < SN_LANES; d <<= 1) {
        const int u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
    }
    const int total = __shfl(incl, SN_LANES - 1);   // <= 64 * 65536
    const int cnt = __popcll(kept);
    if (len > 0) {
        const int k = __popcll(kept & ((1ull << lane) - 1ull));
        sl.off[k] = off;
        sl.len[k] = len;
        sl.base[k] = incl - len;
        sl.w[k] = w;
    }
    if (lane == 0) sl.base[cnt] = total;
    __syncthreads();

    // ---- staging and round 2 ----
    const bool staged = total <= BM25_SNIPPET_STAGE;   // (uniform)
    float best;
    int start;
    if (staged) {
        for (int i = lane; i < total; i += SN_LANES) {
            const int k = sn_slot_of(sl, cnt, i);
            stage[i] = p.post_where[sl.off[k] + (i - sl.base[k])];
        }
        __syncthreads();
        sn_search<true>(sl, stage, p.post_where, cnt, total, p.window, lane, best, start);
    } else {
        sn_search<false>(sl, stage, p.post_where, cnt, total, p.window, lane, best, start);
    }

    // ---- the winning window: which slots it covers, and its last occurrence ----
    int last = -1;
    if (len > 0) {
        const int end = start + p.window;
        int at, v = -1;
        if (staged) {
            const uint16_t *a = stage + (incl - len);
            at = lower_bound_u16(a, len, end);
            if (at > 0) v = a[at - 1];
        } else {
            const uint16_t *a = p.post_where + off;
            at = lower_bound_u16(a, len, end);
            if (at > 0) v = a[at - 1];
        }
        if (v >= start) last = v;
    }
    const unsigned long long covered = __ballot(last >= 0);
#pragma unroll
    for (int d = 1; d < SN_LANES; d <<= 1) {
        const int o = __shfl_xor(last, d);
        last = o > last ? o : last;
    }
    if (lane == 0) {
        p.out_start[pair] = start;
        p.out_last[pair] = last;
        p.out_score[pair] = best;
        p.out_covered[pair] = covered;
    }
}

}  // namespace

hipError_t launch_bm25_snippets(const Bm25SnippetParams &p, hipStream_t st) {
    if (p.npairs > 0) hipLaunchKernelGGL(bm25_snippet_kernel, dim3((unsigned)p.npairs), dim3(SN_LANES), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag

extern "C" int crag_bm25_snippets_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const int64_t *d_post_off,
                                       const uint16_t *d_post_where, int64_t n_rows, int64_t n_terms,
                                       const int32_t *h_q_ptr, const int32_t *h_terms, const float *h_weights,
                                       const int32_t *h_r_ptr, const int32_t *h_rows, int nq, int window,
                                       crag_upload_slot *slot, int32_t *d_start, int32_t *d_last, float *d_score,
                                       uint64_t *d_covered, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    int rc = check_bm25_counts("bm25_snippets_host", nq, 1, n_rows, n_terms);
    if (rc != CRAG_OK) return rc;
    if (window < 1 || window > 65535)
        return fail(CRAG_EINVAL, "bm25_snippets_host: window must be in [1, 65535] (got %d)", window);
    if (!h_q_ptr || !h_r_ptr || !slot) return fail(CRAG_EINVAL, "bm25_snippets_host: NULL pointer argument");
    if (!d_post_ptr || !d_post_pos) return fail(CRAG_EINVAL, "bm25_snippets_host: NULL postings pointer");
    if (!d_post_off || !d_post_where)
        return fail(CRAG_EINVAL, "bm25_snippets_host: NULL position arrays (an index built without positions)");
    rc = check_csr("bm25_snippets_host", "q_ptr", "query", h_q_ptr, nq, CRAG_BM25_SNIPPET_MAX_TERMS);
    if (rc == CRAG_OK) rc = check_csr("bm25_snippets_host", "r_ptr", "query", h_r_ptr, nq, -1);
    if (rc != CRAG_OK) return rc;
    const int nt = h_q_ptr[nq], npairs = h_r_ptr[nq];
    if (nt > 0 && (!h_terms || !h_weights)) return fail(CRAG_EINVAL, "bm25_snippets_host: NULL term or weight array");
    if ((rc = check_terms("bm25_snippets_host", h_terms, 0, nt, n_terms)) != CRAG_OK) return rc;
    for (int i = 0; i < nt; ++i)
        if (!(h_weights[i] >= 0.f) || isinf(h_weights[i]))
            return fail(CRAG_EINVAL, "bm25_snippets_host: weight %d must be finite and >= 0", i);
    if (npairs > 0 && !h_rows) return fail(CRAG_EINVAL, "bm25_snippets_host: NULL row array");
    for (int i = 0; i < npairs; ++i)
        if (h_rows[i] < 0 || (int64_t)h_rows[i] >= n_rows)
            return fail(CRAG_EINVAL, "bm25_snippets_host: row %d is outside [0, n_rows)", h_rows[i]);
    if (npairs > 0 && (!d_start || !d_last || !d_score || !d_covered))
        return fail(CRAG_EINVAL, "bm25_snippets_host: NULL output pointer");
    if (((uintptr_t)d_start & 3) || ((uintptr_t)d_last & 3) || ((uintptr_t)d_score & 3) || ((uintptr_t)d_covered & 7))
        return fail(CRAG_EINVAL, "bm25_snippets_host: misaligned output pointer");
    if (npairs == 0) return CRAG_OK;

    // slot layout: q_ptr [BM25_MAX_Q + 4] int32 | r_ptr [BM25_MAX_Q + 4] | terms [nt] | weights [nt] fp32 | rows [npairs]
    const size_t head = (size_t)(crag::BM25_MAX_Q + 4) * 4;
    UploadPack up;
    const int i_q = up.add(h_q_ptr, (size_t)nq + 1, head);
    const int i_r = up.add(h_r_ptr, (size_t)nq + 1, head);
    const int i_terms = up.add(h_terms, (size_t)nt);
    const int i_w = up.add(h_weights, (size_t)nt);
    const int i_rows = up.add(h_rows, (size_t)npairs);
    if ((rc = up.begin(slot)) != CRAG_OK || (rc = up.commit(slot, stream)) != CRAG_OK) return rc;

    crag::Bm25SnippetParams p;
    p.post_ptr = d_post_ptr;
    p.post_pos = d_post_pos;
    p.post_off = d_post_off;
    p.post_where = d_post_where;
    p.q_ptr = up.dev<int32_t>(i_q);
    p.r_ptr = up.dev<int32_t>(i_r);
    p.terms = up.dev<int32_t>(i_terms);
    p.weights = up.dev<float>(i_w);
    p.rows = up.dev<int32_t>(i_rows);
    p.out_start = d_start;
    p.out_last = d_last;
    p.out_score = d_score;
    p.out_covered = d_covered;
    p.nq = nq;
    p.npairs = npairs;
    p.window = window;
    HIP_TRY(crag::launch_bm25_snippets(p, (hipStream_t)stream));
    return CRAG_OK;
}
