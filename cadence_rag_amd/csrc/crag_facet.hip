// crag_facet.hip -- facet counts on the GPU (gfx950), DESIGN.md 4.14: attribute histograms under a filter, the second half
// of the reference's "Entities + faceting" phase (PHASED_PLAN.md:355-380, "facets can be computed"), for up to 64 queries
// and 16 requested namespaces at once.
//
//   count(q, a) = the number of row positions i < n_rows with bit (q, i) of the masks set whose attribute list holds a
//
// The table's attributes arrive as postings (the transpose of the CSR crag_attr_masks_host reads): the facet ids number
// the attributes by (namespace, value) ascending, so a namespace is one contiguous range of ids AND one contiguous run of
// postings, and ascending id is the tie order of the lists.  Each (attribute, row) pair is stored once.  Three kernels on
// one stream, integer arithmetic only:
//
//   1. facet_transpose_kernel turns the masks [nq][stride] into one 64-bit query set per row position (bit q of word i =
//      bit (q, i); rows at or beyond n_rows and queries at or beyond nq give 0), so that a posting reads ONE word for all
//      queries.  A workgroup takes spans of 1024 rows (128 contiguous bytes of every query's run); lane q of a wave reads
//      query q's 64 bits of a 64-row group, 64 ballots transpose the bit matrix.  rows[q] is the popcount of the same
//      words: summed per lane, per workgroup in LDS, one 64-bit atomic per workgroup and query.  Skipped when the call
//      has no masks (every posting then counts for every query, rows[q] = n_rows).
//   2. facet_count_kernel walks the postings of the requested ranges only, in chunks of FACET_CHUNK = 4096 postings
//      taken with a grid stride, one lane per posting.  Postings are sorted by attribute, so the lanes of one attribute
//      are neighbours: a head ballot cuts the wave into segments; nq ballots hand lane q the set of lanes whose row
//      passes query q, and per segment a popcount under the segment's lane mask gives lane q the segment's count of query
//      q -- one atomic instruction per segment for all queries.  A segment of the chunk's FIRST attribute adds into LDS
//      (one global atomic per chunk and query at the end: a hot attribute that fills whole chunks costs nq atomics per
//      4096 postings, not per posting); every other segment adds straight into the table in HBM -- the long tail (one
//      posting per attribute) meets no contention there.  Integer adds commute: the table is exact whatever the geometry.
//   3. facet_select_kernel, one workgroup per (query, range), streams its slice of the table, keeps the `top` largest
//      keys (count << 32) | ~facet_id under a running threshold (a 512-key LDS buffer, bitonic sort when it fills),
//      counts the non-zero entries for `distinct` and writes the padded lists.  Every output byte is written here.
//
// Bounds: a posting whose facet id lies outside its range or whose row lies outside [0, n_rows) counts nothing and is
// never used as an index; a post_ptr value outside [0, n_postings] is clamped.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_host.h"
#include "crag_maskspan.h"

namespace crag {
namespace {

constexpr int FACET_THREADS = MASK_THREADS;                // the transpose walks the spans of crag_maskspan.h
constexpr int FACET_CHUNK = 4096;                          // postings per workgroup chunk
constexpr int FACET_BUF = 512;                             // keys of the selection buffer: top (<= 64) + pending
constexpr int FACET_SELECT_LOADS = 8;                      // table entries a selection thread loads before it looks at any
constexpr int FACET_WGS_PER_CU = 4;                        // persistent grids = this many workgroups per CU, at most

static_assert(CRAG_FACET_MAX_QUERIES == MASK_MAX_QUERIES, "one ballot lane and one set bit per query");
static_assert(CRAG_FACET_MAX_TOP + FACET_THREADS <= FACET_BUF, "a tile of candidates always fits behind the list");
static_assert(CRAG_FACET_MAX_NAMESPACES <= 64, "one lane per range reads its posting bounds");

struct FacetRanges {
    int32_t lo[CRAG_FACET_MAX_NAMESPACES], hi[CRAG_FACET_MAX_NAMESPACES];   // facet ids [lo, hi), lo <= hi
    int64_t col[CRAG_FACET_MAX_NAMESPACES];                                 // first column of the range in a table row
    int n;
};

__global__ __launch_bounds__(FACET_THREADS) void facet_transpose_kernel(const uint32_t *masks, int64_t stride_w, int64_t n_rows,
                                                                        int nq, uint64_t *qsets, unsigned long long *out_rows) {
    __shared__ uint32_t s_rows[CRAG_FACET_MAX_QUERIES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < CRAG_FACET_MAX_QUERIES) s_rows[tid] = 0;
    __syncthreads();
    const int64_t n_groups = (n_rows + 63) / 64;
    const int64_t n_spans = (n_rows + MASK_SPAN - 1) / MASK_SPAN;
    uint32_t my_rows = 0;   // of query `lane`, over this wave's groups (n_rows < 2^31)
    for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x)
        for (int k = 0; k < MASK_GROUPS; ++k) {
            const int64_t g = span * (MASK_SPAN / 64) + wave * MASK_GROUPS + k;
            if (g >= n_groups) break;   // (uniform in the wave)
            const int64_t base = g * 64, w0 = g * 2;
            uint64_t w = 0;
            if (lane < nq) {
                const uint32_t *run = masks + (int64_t)lane * stride_w;
                w = run[w0];                                             // base < n_rows: the stride holds this word
                if (w0 + 1 < stride_w) w |= (uint64_t)run[w0 + 1] << 32;
                const int64_t rem = n_rows - base;
                if (rem < 64) w &= (1ull << rem) - 1;                    // junk at and beyond n_rows does not count
                my_rows += (uint32_t)__popcll(w);
            }
            uint64_t mine = 0;
            for (int r = 0; r < 64; ++r) {
                const uint64_t b = __ballot((w >> r) & 1ull);
                if (lane == r) mine = b;
            }
            if (base + lane < n_rows) qsets[base + lane] = mine;
        }
    if (lane < nq && my_rows) atomicAdd(&s_rows[lane], my_rows);
    __syncthreads();
    if (tid < nq && s_rows[tid]) atomicAdd(&out_rows[tid], (unsigned long long)s_rows[tid]);
}

struct FacetCountParams {
    const int64_t *post_ptr;    // [n_attrs + 1]
    const int32_t *post_rows;   // [n_postings]
    const int32_t *post_fid;    // [n_postings]
    const uint64_t *qsets;      // [n_rows], NULL: every row passes every query
    uint32_t *counts;           // [nq][width]
    int64_t n_postings, n_rows, width;
    int nq;
    FacetRanges rg;
};

__global__ __launch_bounds__(FACET_THREADS) void facet_count_kernel(FacetCountParams p) {
    __shared__ int64_t s_ps[CRAG_FACET_MAX_NAMESPACES], s_pe[CRAG_FACET_MAX_NAMESPACES];
    __shared__ int64_t s_c0[CRAG_FACET_MAX_NAMESPACES + 1];   // the first chunk number of every range
    __shared__ uint32_t s_acc[CRAG_FACET_MAX_QUERIES];        // of the chunk's first attribute
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = p.nq;
    const uint64_t all = nq == 64 ? ~0ull : (1ull << nq) - 1;
    if (tid < p.rg.n) {
        int64_t ps = p.post_ptr[p.rg.lo[tid]], pe = p.post_ptr[p.rg.hi[tid]];
        ps = ps < 0 ? 0 : ps > p.n_postings ? p.n_postings : ps;
        pe = pe < ps ? ps : pe > p.n_postings ? p.n_postings : pe;
        s_ps[tid] = ps;
        s_pe[tid] = pe;
    }
    if (tid < CRAG_FACET_MAX_QUERIES) s_acc[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int64_t c = 0;
        for (int r = 0; r < p.rg.n; ++r) {
            s_c0[r] = c;
            c += (s_pe[r] - s_ps[r] + FACET_CHUNK - 1) / FACET_CHUNK;
        }
        s_c0[p.rg.n] = c;
    }
    __syncthreads();
    const int64_t n_chunks = s_c0[p.rg.n];
    for (int64_t g = blockIdx.x; g < n_chunks; g += gridDim.x) {
        int r = 0;
        while (s_c0[r + 1] <= g) ++r;   // g < n_chunks = s_c0[n]: ends at r < n
        const int64_t c_begin = s_ps[r] + (g - s_c0[r]) * FACET_CHUNK;
        const int64_t c_end = c_begin + FACET_CHUNK < s_pe[r] ? c_begin + FACET_CHUNK : s_pe[r];
        const int32_t lo = p.rg.lo[r], hi = p.rg.hi[r];
        uint32_t *col0 = p.counts + p.rg.col[r];
        const int32_t f0 = p.post_fid[c_begin];   // (c_begin < c_end: the chunk is not empty)
        for (int64_t base = c_begin + wave * 64; base < c_end; base += FACET_THREADS) {
            const int64_t idx = base + lane;
            int32_t fid = -1;
            uint64_t word = 0;
            if (idx < c_end) {
                const int32_t f = p.post_fid[idx], row = p.post_rows[idx];
                if (f >= lo && f < hi) {
                    fid = f;
                    if (row >= 0 && (int64_t)row < p.n_rows) word = p.qsets ? p.qsets[row] & all : all;
                }
            }
            if (__ballot(word != 0) == 0) continue;   // no row of these 64 postings passes any query (uniform)
            const int32_t prev = __shfl_up(fid, 1);
            uint64_t heads = __ballot(fid >= 0 && (lane == 0 || prev != fid));
            // lane q takes the lanes whose row passes query q: the 64 x 64 bit matrix transposed, as in the kernel above
            uint64_t mine = 0;
            for (int q = 0; q < nq; ++q) {
                const uint64_t b = __ballot((word >> q) & 1ull);
                if (lane == q) mine = b;
            }
            // segment by segment (`heads` is uniform): a segment runs from its head up to the lane in front of the next
            // head (lanes without an attribute in between hold word 0); lane q adds the segment's count of query q, so a
            // segment costs ONE atomic instruction for all queries
            while (heads) {
                const int sl = __ffsll((unsigned long long)heads) - 1;
                heads &= heads - 1;
                const uint64_t below_next = heads ? (1ull << (__ffsll((unsigned long long)heads) - 1)) - 1 : ~0ull;
                const int32_t f = __shfl(fid, sl);   // in [lo, hi): lane sl is a head
                const uint32_t c = (uint32_t)__popcll(mine & below_next & (~0ull << sl));
                if (c) {   // (lanes at and beyond nq hold 0)
                    if (f == f0) atomicAdd(&s_acc[lane], c);
                    else atomicAdd(col0 + (f - lo) + (int64_t)lane * p.width, c);
                }
            }
        }
        __syncthreads();
        if (tid < nq) {
            const uint32_t v = s_acc[tid];
            if (v) {   // (then some lane held f0 inside [lo, hi))
                atomicAdd(col0 + (f0 - lo) + (int64_t)tid * p.width, v);
                s_acc[tid] = 0;
            }
        }
        __syncthreads();   // the next chunk adds into s_acc
    }
}

// bitonic sort of FACET_BUF keys in LDS, descending, by the workgroup; in order behind the last barrier
__device__ __forceinline__ void facet_sort_desc(uint64_t *keys) {
    const int tid = threadIdx.x;
    for (int k2 = 2; k2 <= FACET_BUF; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < FACET_BUF / 2; t += FACET_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = keys[i], b = keys[l];
                if ((i & k2) == 0 ? a < b : a > b) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
}

struct FacetSelectParams {
    const uint32_t *counts;   // [nq][width]
    int64_t width, n_rows;
    int top, write_rows;      // write_rows: the call has no masks, rows[q] = n_rows comes from here
    int32_t *out_ids;         // [nq][n][top]
    uint32_t *out_counts;     // [nq][n][top]
    int32_t *out_distinct;    // [nq][n]
    int64_t *out_rows;        // [nq]
    FacetRanges rg;
};

// grid (max(n, 1), nq): workgroup (r, q) answers range r of query q
__global__ __launch_bounds__(FACET_THREADS) void facet_select_kernel(FacetSelectParams p) {
    __shared__ uint64_t s_keys[FACET_BUF];   // [0, 64): the list so far, descending, 0 = none; behind it the pending keys
    __shared__ int s_fill, s_distinct;
    const int tid = threadIdx.x, r = blockIdx.x, q = blockIdx.y;
    if (p.write_rows && r == 0 && tid == 0) p.out_rows[q] = p.n_rows;
    if (r >= p.rg.n) return;   // (a call without ranges: the rows alone)
    const int top = p.top;
    const int32_t lo = p.rg.lo[r];
    const int64_t w = (int64_t)p.rg.hi[r] - lo;
    const uint32_t *slice = p.counts + (int64_t)q * p.width + p.rg.col[r];
    for (int s = tid; s < FACET_BUF; s += FACET_THREADS) s_keys[s] = 0;
    if (tid == 0) {
        s_fill = CRAG_FACET_MAX_TOP;
        s_distinct = 0;
    }
    __syncthreads();
    uint64_t thr = 0;   // a key has to beat it: the top-th key once the list is full, else 0 (a live key is >= 2^32)
    int distinct = 0;
    for (int64_t t0 = 0; t0 < w; t0 += FACET_SELECT_LOADS * FACET_THREADS) {
        // FACET_SELECT_LOADS independent loads per thread in flight at once (one workgroup streams the whole slice: what it
        // waits for is memory latency), then tile by tile through the buffer
        uint32_t c[FACET_SELECT_LOADS];
#pragma unroll
        for (int k = 0; k < FACET_SELECT_LOADS; ++k) {
            const int64_t j = t0 + k * FACET_THREADS + tid;
            c[k] = j < w ? slice[j] : 0u;
        }
#pragma unroll
        for (int k = 0; k < FACET_SELECT_LOADS; ++k) {
            if (t0 + k * FACET_THREADS >= w) break;   // (uniform)
            const int fill = s_fill;
            __syncthreads();   // every thread has read the same s_fill before any thread appends again
            if (fill + FACET_THREADS > FACET_BUF) {
                facet_sort_desc(s_keys);
                thr = s_keys[top - 1];   // (top <= 64: the clearing below leaves it alone)
                for (int s = CRAG_FACET_MAX_TOP + tid; s < FACET_BUF; s += FACET_THREADS) s_keys[s] = 0;
                if (tid == 0) s_fill = CRAG_FACET_MAX_TOP;
                __syncthreads();
            }
            if (c[k]) {
                ++distinct;
                const int64_t j = t0 + k * FACET_THREADS + tid;
                const uint64_t key = ((uint64_t)c[k] << 32) | (uint32_t)~(uint32_t)(lo + (int32_t)j);
                if (key > thr) s_keys[atomicAdd(&s_fill, 1)] = key;
            }
            __syncthreads();
        }
    }
    facet_sort_desc(s_keys);
    if (distinct) atomicAdd(&s_distinct, distinct);
    __syncthreads();
    const int64_t o = ((int64_t)q * p.rg.n + r) * top;
    if (tid < top) {
        const uint64_t key = s_keys[tid];
        p.out_ids[o + tid] = key ? (int32_t)~(uint32_t)key : -1;
        p.out_counts[o + tid] = (uint32_t)(key >> 32);
    }
    if (tid == 0) p.out_distinct[(int64_t)q * p.rg.n + r] = s_distinct;
}

}  // namespace
}  // namespace crag

extern "C" int64_t crag_facet_workspace_bytes(int64_t n_rows, int nq, int64_t width, int has_masks) {
    if (n_rows < 0 || nq < 0 || width < 0) return -1;
    return (has_masks ? n_rows * 8 : 0) + (int64_t)nq * width * 4;
}

extern "C" int crag_facet_counts_host(const int64_t *d_post_ptr, const int32_t *d_post_rows, const int32_t *d_post_fid,
                                      int64_t n_postings, int64_t n_rows, int64_t n_attrs, const uint8_t *d_masks,
                                      int64_t mask_stride, const int32_t *h_range_lo, const int32_t *h_range_hi,
                                      int n_ranges, int nq, int top, void *d_workspace, int64_t workspace_bytes,
                                      int32_t *d_out_ids, uint32_t *d_out_counts, int32_t *d_out_distinct,
                                      int64_t *d_out_rows, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (nq < 1 || nq > CRAG_FACET_MAX_QUERIES) return fail(CRAG_EINVAL, "facet_counts_host: need 1 <= nq <= 64");
    if (top < 1 || top > CRAG_FACET_MAX_TOP) return fail(CRAG_EINVAL, "facet_counts_host: need 1 <= top <= %d", CRAG_FACET_MAX_TOP);
    if (n_ranges < 0 || n_ranges > CRAG_FACET_MAX_NAMESPACES)
        return fail(CRAG_EINVAL, "facet_counts_host: need 0 <= n_ranges <= %d", CRAG_FACET_MAX_NAMESPACES);
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(CRAG_EINVAL, "facet_counts_host: n_rows must be in [0, 2^31)");
    if (n_attrs < 0 || n_attrs >= INT32_MAX) return fail(CRAG_EINVAL, "facet_counts_host: n_attrs must be in [0, 2^31 - 1)");
    if (n_postings < 0) return fail(CRAG_EINVAL, "facet_counts_host: n_postings must not be negative");
    if (n_ranges > 0 && (!h_range_lo || !h_range_hi)) return fail(CRAG_EINVAL, "facet_counts_host: NULL range pointer");
    crag::FacetRanges rg;
    memset(&rg, 0, sizeof(rg));
    rg.n = n_ranges;
    int64_t width = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const int32_t lo = h_range_lo[r], hi = h_range_hi[r];
        if (lo < 0 || hi < lo || (int64_t)hi > n_attrs)
            return fail(CRAG_EINVAL, "facet_counts_host: range %d = [%d, %d) must lie in [0, n_attrs] with lo <= hi", r, lo, hi);
        for (int s = 0; s < r; ++s)
            if (lo < hi && rg.lo[s] < rg.hi[s] && lo < rg.hi[s] && rg.lo[s] < hi)
                return fail(CRAG_EINVAL, "facet_counts_host: ranges %d and %d overlap", s, r);
        rg.lo[r] = lo;
        rg.hi[r] = hi;
        rg.col[r] = width;
        width += hi - lo;
    }
    const int rc = check_mask_input("facet_counts_host", n_rows, d_masks, mask_stride);
    if (rc != CRAG_OK) return rc;
    if (n_postings > 0 && (!d_post_ptr || !d_post_rows || !d_post_fid))
        return fail(CRAG_EINVAL, "facet_counts_host: NULL postings pointer");
    if (!d_out_rows || (n_ranges > 0 && (!d_out_ids || !d_out_counts || !d_out_distinct)))
        return fail(CRAG_EINVAL, "facet_counts_host: NULL output pointer");
    if (workspace_bytes < 0 || ((uintptr_t)d_workspace & 7) != 0)
        return fail(CRAG_EINVAL, "facet_counts_host: the workspace must be 8-byte aligned and its size not negative");
    const bool masked = d_masks != nullptr && n_rows > 0;
    const int64_t need = crag_facet_workspace_bytes(n_rows, nq, width, masked);
    if (need > workspace_bytes)
        return fail(CRAG_E2BIG, "facet_counts_host: %d queries x %lld columns need %lld bytes of workspace, the call has %lld: split the batch",
                    nq, (long long)width, (long long)need, (long long)workspace_bytes);
    if (need > 0 && !d_workspace) return fail(CRAG_EINVAL, "facet_counts_host: NULL workspace");

    hipStream_t st = (hipStream_t)stream;
    uint64_t *qsets = masked ? (uint64_t *)d_workspace : nullptr;
    uint32_t *counts = (uint32_t *)((char *)d_workspace + (masked ? n_rows * 8 : 0));
    const int64_t cap = (int64_t)cu_count() * crag::FACET_WGS_PER_CU;
    const dim3 block(crag::FACET_THREADS);
    if (d_masks) HIP_TRY(hipMemsetAsync(d_out_rows, 0, (size_t)nq * 8, st));   // (no rows: the zeros are the answer)
    if (masked) {
        const int64_t n_spans = (n_rows + crag::MASK_SPAN - 1) / crag::MASK_SPAN;
        hipLaunchKernelGGL(crag::facet_transpose_kernel, dim3((unsigned)(n_spans < cap ? n_spans : cap)), block, 0, st,
                           (const uint32_t *)d_masks, mask_stride / 4, n_rows, nq, qsets, (unsigned long long *)d_out_rows);
    }
    if (width > 0) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)nq * width * 4, st));
    if (width > 0 && n_postings > 0 && n_rows > 0) {
        crag::FacetCountParams c;
        c.post_ptr = d_post_ptr;
        c.post_rows = d_post_rows;
        c.post_fid = d_post_fid;
        c.qsets = qsets;
        c.counts = counts;
        c.n_postings = n_postings;
        c.n_rows = n_rows;
        c.width = width;
        c.nq = nq;
        c.rg = rg;
        // at most this many chunks: the ranges are disjoint runs of the postings, each rounds up once
        const int64_t most = (n_postings + crag::FACET_CHUNK - 1) / crag::FACET_CHUNK + n_ranges;
        hipLaunchKernelGGL(crag::facet_count_kernel, dim3((unsigned)(most < cap ? most : cap)), block, 0, st, c);
    }
    crag::FacetSelectParams s;
    s.counts = counts;
    s.width = width;
    s.n_rows = n_rows;
    s.top = top;
    s.write_rows = d_masks ? 0 : 1;
    s.out_ids = d_out_ids;
    s.out_counts = d_out_counts;
    s.out_distinct = d_out_distinct;
    s.out_rows = d_out_rows;
    s.rg = rg;
    hipLaunchKernelGGL(crag::facet_select_kernel, dim3((unsigned)(n_ranges > 0 ? n_ranges : 1), (unsigned)nq), block, 0, st, s);
    return launch_ok("facet_counts");
}
