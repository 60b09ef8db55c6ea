// crag_postings.h -- what the kernels of the BM25 lane share (crag_bm25.hip, crag_bm25_clause.hip, crag_bm25_expand.hip,
// crag_bm25_snippet.hip): the row span of a range, a term's postings inside it, the frame of a mask kernel -- load a word
// of the input mask, stream postings into an LDS bitmap, AND the bitmap into `keep` and vote, store --, the lower bound in
// ascending 16-bit token positions, a posting's slice of them, and the rank of a key among at most a few dozen.
// Device code without state, in the style of crag_rows.h, whose lower_bound_asc does the searching here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_kernels.h"

namespace crag {

// the rows [base, end) of range rg among n rows
__device__ __forceinline__ void range_span(int rg, int64_t n, int64_t &base, int64_t &end) {
    base = (int64_t)rg * BM25_RANGE;
    end = base + BM25_RANGE < n ? base + BM25_RANGE : n;
    if (end < base) end = base;   // a range of the stride padding: no rows
}

// the postings of `term` whose rows lie in [base, end): post_pos[lo .. hi)
__device__ __forceinline__ void posting_slice(const int64_t *post_ptr, const int32_t *post_pos, int term, int64_t base,
                                              int64_t end, int64_t &lo, int64_t &hi) {
    const int64_t a = post_ptr[term], b = post_ptr[term + 1];
    lo = lower_bound_asc(post_pos, a, b, base);
    hi = lower_bound_asc(post_pos, lo, b, end);
}

// word gw of query q's input mask: all ones without one (in == NULL), one run for all queries with stride 0, nothing
// beyond the n_words = ceil(n / 32) words a run is sure to hold, and no bit at or beyond n
__device__ __forceinline__ uint32_t load_mask_word(const uint32_t *in, int64_t in_stride_w, int q, int64_t gw, int64_t n,
                                                   int64_t n_words) {
    uint32_t word = 0;
    if (gw < n_words) {
        word = in ? in[(int64_t)q * in_stride_w + gw] : 0xffffffffu;
        if (gw == n_words - 1 && (n & 31)) word &= (1u << (n & 31)) - 1u;
    }
    return word;
}

// bits |= the rows of [base, end) among post_pos[l0 .. l0 + len); the callers' threads take first, first + step, ...
__device__ __forceinline__ void stream_bitmap(const int32_t *post_pos, int64_t l0, int len, int64_t base, int64_t end,
                                              uint32_t *bits, int first, int step) {
    for (int i = first; i < len; i += step) {
        const int64_t li = (int64_t)post_pos[l0 + i] - base;
        if ((uint64_t)li >= (uint64_t)(end - base)) continue;   // (a list that does not ascend)
        atomicOr(&bits[li >> 5], 1u << (li & 31));
    }
}

// keep &= tmp (required) or keep &= ~tmp (excluded), one word per thread; is any row of the range still kept?
// (the barrier of the vote also orders this clause's reads of tmp before the next clause zeroes it)
__device__ __forceinline__ bool mask_apply(uint32_t *keep, const uint32_t *tmp, int tid, bool required) {
    keep[tid] = required ? keep[tid] & tmp[tid] : keep[tid] & ~tmp[tid];
    return __syncthreads_or(keep[tid] != 0u);
}

// word gw of query q's output run: a plain store, the stride padding included
__device__ __forceinline__ void store_mask_word(uint32_t *out, int64_t stride_w, int q, int64_t gw, uint32_t word) {
    if (gw < stride_w) out[(int64_t)q * stride_w + gw] = word;
}

// first index of a[0 .. n) (ascending uint16, LDS or memory) whose value is >= x
template <class P> __device__ __forceinline__ int lower_bound_u16(P a, int n, int x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the token positions of posting pi: post_where[off .. off + the returned length), at most 65 536 of them
__device__ __forceinline__ int where_slice(const int64_t *post_off, int64_t pi, int64_t &off) {
    off = post_off[pi];
    const int64_t len = post_off[pi + 1] - off;
    return len > 0 ? (int)(len < 65536 ? len : 65536) : 0;
}

// the number of keys[0 .. n) above `mine`: over distinct keys the ranks are a permutation of 0 .. n - 1, best first
template <class K> __device__ __forceinline__ int rank_desc(const K *keys, int n, K mine) {
    int r = 0;
    for (int i = 0; i < n; ++i) r += keys[i] > mine;
    return r;
}

}  // namespace crag
