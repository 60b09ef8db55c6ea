// crag_filter.hip -- filter row masks built on the GPU from device-resident columns (gfx950), DESIGN.md 4.10.
// The device counterpart of _build_filter_clause (the reference's app/retrieve.py:93-120) for up to 64 queries at once:
// per row its call_started_at (us since the epoch, INT64_MIN = NULL) and the dense number of its call; per query an
// inclusive date range and, transposed, per call the 64-bit set of the queries that admit it.
//
//   bit (q, i) = (no call scoping, or 0 <= slot[i] < n_calls and bit q of qset[slot[i]])
//              & (from[q] == INT64_MIN or started[i] != INT64_MIN and started[i] >= from[q])
//              & (to[q]   == INT64_MAX or started[i] != INT64_MIN and started[i] <= to[q])
//
// One launch on the span frame of crag_maskspan.h: a workgroup owns one span of 1024 row positions, the grid covers the
// words [0, mask_stride / 4) of a run (rows at or beyond n_rows contribute 0 and load nothing).  What is this file's own
// is the middle: per 64-row group every lane loads its row's timestamp and slot (coalesced), gathers qset[slot] (8 bytes;
// the table stays in L2) and clears the bits of the queries whose date range the row fails -- a wave-uniform loop over
// only the queries that carry a bound.  The transpose, the LDS staging and the write-out are the header's; a reused
// buffer keeps no stale bit.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_host.h"
#include "crag_maskspan.h"

namespace crag {
namespace {

static_assert(CRAG_FILTER_MAX_QUERIES == MASK_MAX_QUERIES, "one ballot lane and one qset bit per query");

struct FilterParams {
    const int64_t *started;     // [n]
    const int32_t *slot;        // [n]
    const uint64_t *qset;       // [n_calls], nullptr: no query is call-scoped
    const int64_t *from;        // [nq]
    const int64_t *to;          // [nq]
    uint64_t dated;             // bit q: query q carries a date bound
    int64_t n, n_calls;
    int64_t stride_w;           // mask words per run
    int nq;
    uint32_t *out;              // [nq][stride_w]
};

__global__ __launch_bounds__(MASK_THREADS) void filter_masks_kernel(FilterParams p) {
    __shared__ uint32_t s_words[MASK_LDS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * MASK_SPAN;

    for (int g = 0; g < MASK_GROUPS; ++g) {
        const int gl = wave * MASK_GROUPS + g;            // the group's number inside the span
        const int64_t i = row0 + (int64_t)gl * 64 + lane;
        uint64_t bits = 0;
        int64_t ts = INT64_MIN;
        if (i < p.n) {
            ts = p.started[i];
            if (p.qset) {
                const int32_t s = p.slot[i];
                if (s >= 0 && (int64_t)s < p.n_calls) bits = p.qset[s];   // a slot outside the table is never followed
            } else {
                bits = ~0ull;
            }
        }
        // only the queries with a date bound; a NULL timestamp fails every one of them (INT64_MIN as `from` / INT64_MAX as
        // `to` is the open side of a query that bounds the other one: every non-NULL timestamp passes it as an integer)
        for (uint64_t d = p.dated; d; d &= d - 1) {
            const int q = __builtin_ctzll(d);
            const bool pass = ts != INT64_MIN && ts >= p.from[q] && ts <= p.to[q];
            if (!pass) bits &= ~(1ull << q);
        }
        // every lane takes part in every ballot: the lanes beyond n_rows hold 0
        stage_group(s_words, gl, lane, p.nq, ballot_transpose(bits, p.nq, lane));
    }
    __syncthreads();
    store_span(s_words, blockIdx.x, p.stride_w, p.nq, p.out, nullptr, 0, 0);
}

}  // namespace
}  // namespace crag

extern "C" int crag_filter_masks_host(const int64_t *d_started_us, const int32_t *d_call_slot, int64_t n_rows,
                                      int64_t n_calls, const uint64_t *h_call_qset, const int64_t *h_date_from,
                                      const int64_t *h_date_to, int nq, crag_upload_slot *slot, uint8_t *d_out_mask,
                                      int64_t mask_stride, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (nq < 1 || nq > CRAG_FILTER_MAX_QUERIES) return fail(CRAG_EINVAL, "filter_masks_host: need 1 <= nq <= 64");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(CRAG_EINVAL, "filter_masks_host: n_rows must be in [0, 2^31)");
    if (n_calls < 0) return fail(CRAG_EINVAL, "filter_masks_host: n_calls must not be negative");
    int rc = check_mask_strides("filter_masks_host", n_rows, nullptr, 0, d_out_mask, mask_stride);
    if (rc != CRAG_OK) return rc;
    if (!h_date_from || !h_date_to || !slot) return fail(CRAG_EINVAL, "filter_masks_host: NULL pointer argument");
    if (n_rows > 0 && (!d_started_us || !d_call_slot)) return fail(CRAG_EINVAL, "filter_masks_host: NULL column pointer");
    if (mask_stride == 0) return CRAG_OK;   // (n_rows is 0: the runs are empty)

    // slot layout: from [64] int64 | to [64] int64 | qset [n_calls] uint64
    const size_t head = (size_t)CRAG_FILTER_MAX_QUERIES * 8;
    UploadPack up;
    const int i_from = up.add(h_date_from, (size_t)nq, head);
    const int i_to = up.add(h_date_to, (size_t)nq, head);
    const int i_qset = up.add(h_call_qset, h_call_qset ? (size_t)n_calls : 0);
    if ((rc = up.begin(slot)) != CRAG_OK) return rc;
    if ((rc = up.commit(slot, stream)) != CRAG_OK) return rc;

    crag::FilterParams p;
    p.started = d_started_us;
    p.slot = d_call_slot;
    p.qset = h_call_qset ? up.dev<uint64_t>(i_qset) : nullptr;
    p.from = up.dev<int64_t>(i_from);
    p.to = up.dev<int64_t>(i_to);
    p.dated = 0;
    for (int q = 0; q < nq; ++q)
        if (h_date_from[q] != INT64_MIN || h_date_to[q] != INT64_MAX) p.dated |= 1ull << q;
    p.n = n_rows;
    p.n_calls = n_calls;
    p.stride_w = mask_stride / 4;
    p.nq = nq;
    p.out = (uint32_t *)d_out_mask;
    const int64_t blocks = (p.stride_w + crag::MASK_SPAN_WORDS - 1) / crag::MASK_SPAN_WORDS;
    hipLaunchKernelGGL(crag::filter_masks_kernel, dim3((unsigned)blocks), dim3(crag::MASK_THREADS), 0, (hipStream_t)stream, p);
    return launch_ok("filter_masks");
}
