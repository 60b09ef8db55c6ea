// crag_filter.hip -- filter row masks built on the GPU from device-resident columns (gfx950), DESIGN.md 4.10.
// The device counterpart of _build_filter_clause (the reference's app/retrieve.py:93-120) for up to 64 queries at once:
// per row its call_started_at (us since the epoch, INT64_MIN = NULL) and the dense number of its call; per query an
// inclusive date range and, transposed, per call the 64-bit set of the queries that admit it.
//
//   bit (q, i) = (no call scoping, or 0 <= slot[i] < n_calls and bit q of qset[slot[i]])
//              & (from[q] == INT64_MIN or started[i] != INT64_MIN and started[i] >= from[q])
//              & (to[q]   == INT64_MAX or started[i] != INT64_MIN and started[i] <= to[q])
//
// One launch.  A workgroup of four waves owns FILTER_SPAN = 1024 consecutive row positions = 32 mask words of every
// query; the grid covers the words [0, mask_stride / 4) of a run, so the zeros beyond n_rows and in the stride padding
// come from the same code as the bits (rows at or beyond n_rows contribute 0 and load nothing).  A wave takes four
// groups of 64 rows: every lane loads its row's timestamp and slot (coalesced), gathers qset[slot] (8 bytes; the table
// stays in L2), clears the bits of the queries whose date range the row fails -- a wave-uniform loop over only the
// queries that carry a bound -- and nq ballots transpose the 64 x 64 bit matrix: ballot q is the group's two mask words
// of query q, kept by lane q.  The words meet in LDS ([query][33]: the odd stride keeps the column write and the row
// read off each other's banks) and leave as 128 contiguous bytes per query and workgroup.  Stores only, no atomics: the
// output is a function of the input alone, whatever the launch geometry, and a reused buffer keeps no stale bit.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_host.h"


namespace crag {
namespace {

constexpr int FILTER_THREADS = 256;
constexpr int FILTER_WAVES = FILTER_THREADS / 64;
constexpr int FILTER_SPAN = 1024;                       // row positions per workgroup
constexpr int FILTER_SPAN_WORDS = FILTER_SPAN / 32;     // mask words per query and workgroup
constexpr int FILTER_GROUPS = FILTER_SPAN / 64 / FILTER_WAVES;   // 64-row groups per wave
constexpr int FILTER_LDS_STRIDE = FILTER_SPAN_WORDS + 1;

static_assert(FILTER_SPAN_WORDS == 32, "the write-out maps 32 consecutive threads to one query's words");
static_assert(CRAG_FILTER_MAX_QUERIES == 64, "one ballot lane and one qset bit per query");

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

__global__ __launch_bounds__(FILTER_THREADS) void filter_masks_kernel(FilterParams p) {
    __shared__ uint32_t s_words[CRAG_FILTER_MAX_QUERIES * FILTER_LDS_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * FILTER_SPAN;
    const int nq = p.nq;

    for (int g = 0; g < FILTER_GROUPS; ++g) {
        const int gl = wave * FILTER_GROUPS + g;          // the group's number inside the span
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
        const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
        uint64_t mine = 0;
        for (int q = 0; q < nq && q < 32; ++q) {
            const uint64_t b = __ballot((lo >> q) & 1u);
            if (lane == q) mine = b;
        }
        for (int q = 32; q < nq; ++q) {
            const uint64_t b = __ballot((hi >> (q - 32)) & 1u);
            if (lane == q) mine = b;
        }
        if (lane < nq) {
            s_words[lane * FILTER_LDS_STRIDE + 2 * gl] = (uint32_t)mine;
            s_words[lane * FILTER_LDS_STRIDE + 2 * gl + 1] = (uint32_t)(mine >> 32);
        }
    }
    __syncthreads();
    // 32 consecutive threads write one query's 32 words; a word at or beyond the stride belongs to the next run
    const int w = tid & 31;
    const int64_t gw = (int64_t)blockIdx.x * FILTER_SPAN_WORDS + w;
    if (gw < p.stride_w)
        for (int q = tid >> 5; q < nq; q += FILTER_THREADS / 32) p.out[(int64_t)q * p.stride_w + gw] = s_words[q * FILTER_LDS_STRIDE + w];
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
    if (mask_stride < 0 || mask_stride % 4 != 0 || mask_stride < (n_rows + 31) / 32 * 4 || mask_stride > ((int64_t)1 << 32))
        return fail(CRAG_EINVAL, "filter_masks_host: mask_stride must be a multiple of 4 in [ceil(n_rows/32)*4, 2^32]");
    if (!h_date_from || !h_date_to || !slot) return fail(CRAG_EINVAL, "filter_masks_host: NULL pointer argument");
    if (n_rows > 0 && (!d_started_us || !d_call_slot)) return fail(CRAG_EINVAL, "filter_masks_host: NULL column pointer");
    if (mask_stride > 0 && !d_out_mask) return fail(CRAG_EINVAL, "filter_masks_host: NULL output pointer");
    if (((uintptr_t)d_out_mask & 3) != 0) return fail(CRAG_EINVAL, "filter_masks_host: the output must be 4-byte aligned");
    if (mask_stride == 0) return CRAG_OK;   // (n_rows is 0: the runs are empty)

    // slot layout: from [64] int64 | to [64] int64 | qset [n_calls] uint64
    const size_t head = (size_t)CRAG_FILTER_MAX_QUERIES * 8;
    const size_t bytes = 2 * head + (h_call_qset ? (size_t)n_calls * 8 : 0);
    void *h = nullptr, *d = nullptr;
    int rc = crag_upload_slot_begin_(slot, bytes, &h, &d);
    if (rc != CRAG_OK) return rc;
    memcpy(h, h_date_from, (size_t)nq * 8);
    memcpy((char *)h + head, h_date_to, (size_t)nq * 8);
    if (h_call_qset && n_calls > 0) memcpy((char *)h + 2 * head, h_call_qset, (size_t)n_calls * 8);
    rc = crag_upload_slot_commit_(slot, bytes, stream);
    if (rc != CRAG_OK) return rc;

    crag::FilterParams p;
    p.started = d_started_us;
    p.slot = d_call_slot;
    p.qset = h_call_qset ? (const uint64_t *)((const char *)d + 2 * head) : nullptr;
    p.from = (const int64_t *)d;
    p.to = (const int64_t *)((const char *)d + head);
    p.dated = 0;
    for (int q = 0; q < nq; ++q)
        if (h_date_from[q] != INT64_MIN || h_date_to[q] != INT64_MAX) p.dated |= 1ull << q;
    p.n = n_rows;
    p.n_calls = n_calls;
    p.stride_w = mask_stride / 4;
    p.nq = nq;
    p.out = (uint32_t *)d_out_mask;
    const int64_t blocks = (p.stride_w + crag::FILTER_SPAN_WORDS - 1) / crag::FILTER_SPAN_WORDS;
    hipLaunchKernelGGL(crag::filter_masks_kernel, dim3((unsigned)blocks), dim3(crag::FILTER_THREADS), 0, (hipStream_t)stream, p);
    return launch_ok("filter_masks");
}
