// crag_maskspan.h -- what the kernels of the row-mask lane share (crag_filter.hip, crag_attr.hip; the span constants of
// crag_facet.hip): the span frame of a kernel that writes packed row masks for up to 64 queries -- a workgroup of four
// waves owns MASK_SPAN = 1024 consecutive row positions = 32 mask words of every query --, the 64 x 64 bit transpose by
// ballots that turns one 64-bit query set per row into one 64-bit row word per query, the staging of a group's words in
// LDS and the write-out of a span.  Device code without state, in the style of crag_rows.h and crag_postings.h.
//
// A kernel on the frame evaluates, per 64-row group, one query set per lane (`bits`: bit q = the lane's row passes query
// q; 0 for a lane at or beyond n_rows, which loads nothing), and then
//
//   stage_group(s_words, gl, lane, nq, ballot_transpose(bits, nq, lane));     for each of its MASK_GROUPS groups
//   __syncthreads();
//   store_span(s_words, span, ...);
//
// with a second barrier behind store_span where the workgroup goes on to another span.  The grid (or the span loop)
// covers the words [0, stride_w) of a run, so the zeros beyond n_rows and in the stride padding come from the same code
// as the bits.  Stores only, no atomics: the output is a function of the input alone, whatever the launch geometry.
//
// What is deliberately not here: the tail-bit trim of load_mask_word (crag_postings.h) -- an input word is ANDed in as
// it stands, its bits at or beyond n_rows meet zeros --, and anything a kernel does between the frame's steps.
// The two facet kernels keep their own ballot loops (the 64-bit-shift form): facet_transpose_kernel walks its spans with
// MASK_SPAN and MASK_GROUPS and takes nothing else.  It transposes rows, not queries, with n = 64 known at compile time:
// through ballot_transpose the compiler unrolls all 64 ballots, which took it from 79 to 106 SGPRs with 202 spilled and
// from 8 to 7 waves per SIMD; facet_count_kernel stayed at 8 but paid 4 SGPRs more, for four lines saved
// (profiles/row_mask_refactor_check.jsonl).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crag {

constexpr int MASK_THREADS = 256;
constexpr int MASK_WAVES = MASK_THREADS / 64;
constexpr int MASK_SPAN = 1024;                                  // row positions per span
constexpr int MASK_SPAN_WORDS = MASK_SPAN / 32;                  // mask words per query and span
constexpr int MASK_GROUPS = MASK_SPAN / 64 / MASK_WAVES;         // 64-row groups per wave and span
constexpr int MASK_LDS_STRIDE = MASK_SPAN_WORDS + 1;             // odd: the column write and the row read miss each other's banks
constexpr int MASK_MAX_QUERIES = 64;                             // one ballot lane and one set bit per query
constexpr int MASK_LDS_WORDS = MASK_MAX_QUERIES * MASK_LDS_STRIDE;   // s_words of a kernel on the frame

static_assert(MASK_SPAN_WORDS == 32, "the write-out maps 32 consecutive threads to one query's words");
static_assert(MASK_MAX_QUERIES == 64, "one ballot lane per query: a wave has 64");
static_assert(MASK_GROUPS * MASK_WAVES * 2 == MASK_SPAN_WORDS, "a group is two words of every query");

// The 64 x 64 bit matrix of a wave transposed: lane l holds `bits`, the result of lane q < n is the word whose bit l is
// bit q of lane l's `bits`; a lane at or beyond n gets 0.  EVERY lane of the wave takes part in every ballot: the call
// stands in wave-uniform control flow, a lane without a row passes bits = 0.  Two loops over 32-bit halves, so that
// the per-ballot shift is a 32-bit one.
__device__ __forceinline__ uint64_t ballot_transpose(uint64_t bits, int n, int lane) {
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    uint64_t mine = 0;
    for (int q = 0; q < n && q < 32; ++q) {
        const uint64_t b = __ballot((lo >> q) & 1u);
        if (lane == q) mine = b;
    }
    for (int q = 32; q < n; ++q) {
        const uint64_t b = __ballot((hi >> (q - 32)) & 1u);
        if (lane == q) mine = b;
    }
    return mine;
}

// lane q < nq puts its two words of group gl (the group's number inside the span) into s_words[q][2 gl, 2 gl + 1]
__device__ __forceinline__ void stage_group(uint32_t *s_words, int gl, int lane, int nq, uint64_t mine) {
    if (lane < nq) {
        s_words[lane * MASK_LDS_STRIDE + 2 * gl] = (uint32_t)mine;
        s_words[lane * MASK_LDS_STRIDE + 2 * gl + 1] = (uint32_t)(mine >> 32);
    }
}

// The write-out of span `span`, behind a barrier: 32 consecutive threads write one query's 32 words, 128 contiguous
// bytes; a word at or beyond the stride belongs to the next run and is left alone.  `in` (nullable; it may be `out`
// itself when in_stride_w == stride_w, the same thread reads and writes a word) is ANDed in: in_stride_w words per
// query, 0 = one run shared by all; it is read only below n_words = ceil(n_rows / 32), the words an input run is sure to
// hold -- beyond them the staged word is 0 anyway.
__device__ __forceinline__ void store_span(const uint32_t *s_words, int64_t span, int64_t stride_w, int nq, uint32_t *out,
                                           const uint32_t *in, int64_t in_stride_w, int64_t n_words) {
    const int tid = threadIdx.x, w = tid & 31;
    const int64_t gw = span * MASK_SPAN_WORDS + w;
    if (gw < stride_w)
        for (int q = tid >> 5; q < nq; q += MASK_THREADS / 32) {
            uint32_t word = s_words[q * MASK_LDS_STRIDE + w];
            if (in && gw < n_words) word &= in[(int64_t)q * in_stride_w + gw];
            out[(int64_t)q * stride_w + gw] = word;
        }
}

}  // namespace crag
