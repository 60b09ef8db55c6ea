// crag_attr.hip -- attribute row masks built on the GPU (gfx950), DESIGN.md 4.13: the row-level filters of the reference's
// plan (PHASED_PLAN.md:355-380 entity_filters, APP_SPEC.md:311-341 entities / chunk_entities / artifact_entities,
// APP_SPEC.md:616-619 entity constraints and the who_said intent), for up to 64 queries at once.
//
// A row holds a variable-length list of attribute ids (CSR by row POSITION; ids from the table's dictionary); a query
// holds up to 8 clauses, each a set of keys.  A row passes a query iff every clause of the query is hit by at least one
// of the row's attributes:
//
//   have[c](i)  = OR over the attributes a of row i with a == keys[j] of key_sets[j][c]       (a 64-bit query set)
//   bit (q, i)  = i < n_rows  &  in(q, i)  &  for every c: bit q of (have[c](i) | ~clause_sets[c])
//
// One launch of persistent workgroups (four waves).  A workgroup builds, ONCE, an open-addressing table in LDS from key
// id to entry number (ATTR_SLOTS = 1024 slots for at most 512 distinct keys: load <= 0.5, LDS compare-and-swap on the
// slot, linear probing behind a multiplicative hash) and copies the entries' query sets [n_keys][NU] beside it, NU = the
// number of clauses any query uses, rounded up to 1, 2, 4 or 8 (the kernel is instantiated per NU, so that have[] lives
// in registers).  It then walks the spans of crag_maskspan.h (1024 consecutive row positions = 32 mask words of every
// query) with a grid stride; the spans cover the words [0, mask_stride / 4) of a run.  What is this file's own is the
// middle: one lane per row reads its attr_ptr pair, walks its ids (neighbouring lanes' lists are neighbours in memory),
// probes the table per id and ORs the hit's words into have[].  The transpose, the LDS staging and the write-out are the
// header's; the input mask is applied at the write-out, where a thread holds (query, word): the same thread reads and
// writes a word, which is what makes the in-place form safe.  Plain stores only, no global atomics.
// Known weakness: a row with hundreds of attributes holds its wave for the length of its list.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_host.h"
#include "crag_maskspan.h"

namespace crag {
namespace {

constexpr int ATTR_SLOTS = 1024;                        // of the key table: a power of two >= 2 * CRAG_ATTR_MAX_KEYS
constexpr int ATTR_SLOT_BITS = 10;
constexpr int32_t ATTR_EMPTY = -1;                      // no key is negative
constexpr int ATTR_WGS_PER_CU = 2;                      // persistent grid = this many workgroups per CU, at most

static_assert(CRAG_ATTR_MAX_QUERIES == MASK_MAX_QUERIES, "one ballot lane and one set bit per query");
static_assert(ATTR_SLOTS == 1 << ATTR_SLOT_BITS && ATTR_SLOTS >= 2 * CRAG_ATTR_MAX_KEYS, "load <= 0.5");
static_assert(CRAG_ATTR_MAX_CLAUSES == 8, "NU is one of 1, 2, 4, 8");

struct AttrParams {
    const int64_t *attr_ptr;    // [n + 1]
    const int32_t *attr_ids;    // [attr_ptr[n]]
    const int32_t *keys;        // [n_keys], distinct, in [0, n_attrs)
    const uint64_t *sets;       // [n_keys][NU]
    uint64_t clause[CRAG_ATTR_MAX_CLAUSES];   // [NU] used, the rest 0: bit q <=> query q has this clause
    int64_t n, n_attrs;
    int64_t n_words;            // ceil(n / 32): the words an input run is sure to hold
    int64_t stride_w;           // mask words per output run
    int64_t in_stride_w;        // mask words per input run, 0: one run shared by all queries
    int n_keys, nq;
    const uint32_t *in;         // nullable; may be `out` itself when in_stride_w == stride_w
    uint32_t *out;              // [nq][stride_w]
};

__device__ __forceinline__ uint32_t attr_hash(int32_t id) { return ((uint32_t)id * 0x9E3779B1u) >> (32 - ATTR_SLOT_BITS); }

template <int NU>
__global__ __launch_bounds__(MASK_THREADS) void attr_masks_kernel(AttrParams p) {
    __shared__ int32_t s_key[ATTR_SLOTS];
    __shared__ uint16_t s_ent[ATTR_SLOTS];
    __shared__ uint64_t s_sets[CRAG_ATTR_MAX_KEYS * NU];
    __shared__ uint32_t s_words[MASK_LDS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = p.nq, n_keys = p.n_keys;

    // the key table and the entries' query sets, once per workgroup
    for (int s = tid; s < ATTR_SLOTS; s += MASK_THREADS) s_key[s] = ATTR_EMPTY;
    for (int e = tid; e < n_keys * NU; e += MASK_THREADS) s_sets[e] = p.sets[e];
    __syncthreads();
    for (int j = tid; j < n_keys; j += MASK_THREADS) {
        const int32_t key = p.keys[j];
        uint32_t h = attr_hash(key);
        // keys are distinct and n_keys <= ATTR_SLOTS / 2: a free slot exists, the walk ends
        for (int step = 0; step < ATTR_SLOTS; ++step) {
            if (atomicCAS(&s_key[h], ATTR_EMPTY, key) == ATTR_EMPTY) {
                s_ent[h] = (uint16_t)j;
                break;
            }
            h = (h + 1) & (ATTR_SLOTS - 1);
        }
    }
    __syncthreads();

    const int64_t n_spans = (p.stride_w + MASK_SPAN_WORDS - 1) / MASK_SPAN_WORDS;
    for (int64_t span = blockIdx.x; span < n_spans; span += gridDim.x) {
        const int64_t row0 = span * MASK_SPAN;
        for (int g = 0; g < MASK_GROUPS; ++g) {
            const int gl = wave * MASK_GROUPS + g;            // the group's number inside the span
            const int64_t i = row0 + (int64_t)gl * 64 + lane;
            uint64_t bits = 0;
            if (i < p.n) {
                uint64_t have[NU];
#pragma unroll
                for (int c = 0; c < NU; ++c) have[c] = 0;
                const int64_t lo = p.attr_ptr[i], hi = p.attr_ptr[i + 1];
                for (int64_t a = lo; a < hi; ++a) {
                    const int32_t id = p.attr_ids[a];
                    if (id < 0 || (int64_t)id >= p.n_attrs) continue;   // outside the dictionary: matches nothing
                    uint32_t h = attr_hash(id);
                    for (int step = 0; step < ATTR_SLOTS; ++step) {
                        const int32_t k = s_key[h];
                        if (k == id) {
                            const int e = s_ent[h];
#pragma unroll
                            for (int c = 0; c < NU; ++c) have[c] |= s_sets[e * NU + c];
                            break;
                        }
                        if (k == ATTR_EMPTY) break;
                        h = (h + 1) & (ATTR_SLOTS - 1);
                    }
                }
                bits = ~0ull;
#pragma unroll
                for (int c = 0; c < NU; ++c) bits &= have[c] | ~p.clause[c];
            }
            // every lane takes part in every ballot: the lanes beyond n_rows hold 0
            stage_group(s_words, gl, lane, nq, ballot_transpose(bits, nq, lane));
        }
        __syncthreads();
        store_span(s_words, span, p.stride_w, nq, p.out, p.in, p.in_stride_w, p.n_words);
        __syncthreads();   // the next span overwrites s_words
    }
}

}  // namespace
}  // namespace crag

extern "C" int crag_attr_masks_host(const int64_t *d_attr_ptr, const int32_t *d_attr_ids, int64_t n_rows, int64_t n_attrs,
                                    const int32_t *h_keys, const uint64_t *h_key_sets, int n_keys,
                                    const uint64_t *h_clause_sets, int nq, const uint8_t *d_in_mask, int64_t in_stride,
                                    crag_upload_slot *slot, uint8_t *d_out_mask, int64_t mask_stride, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (nq < 1 || nq > CRAG_ATTR_MAX_QUERIES) return fail(CRAG_EINVAL, "attr_masks_host: need 1 <= nq <= 64");
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(CRAG_EINVAL, "attr_masks_host: n_rows must be in [0, 2^31)");
    if (n_attrs < 0) return fail(CRAG_EINVAL, "attr_masks_host: n_attrs must not be negative");
    if (n_keys < 0) return fail(CRAG_EINVAL, "attr_masks_host: n_keys must not be negative");
    int rc = check_mask_strides("attr_masks_host", n_rows, d_in_mask, in_stride, d_out_mask, mask_stride);
    if (rc != CRAG_OK) return rc;
    if (!h_clause_sets || !slot) return fail(CRAG_EINVAL, "attr_masks_host: NULL pointer argument");
    if (n_keys > 0 && (!h_keys || !h_key_sets)) return fail(CRAG_EINVAL, "attr_masks_host: NULL key pointer");
    if (n_rows > 0 && (!d_attr_ptr || !d_attr_ids)) return fail(CRAG_EINVAL, "attr_masks_host: NULL column pointer");
    if (n_keys > CRAG_ATTR_MAX_KEYS)
        return fail(CRAG_E2BIG, "attr_masks_host: %d distinct keys, one call takes %d: split the batch", n_keys, CRAG_ATTR_MAX_KEYS);
    const uint64_t beyond = nq == 64 ? 0 : ~0ull << nq;   // the bits of queries the call does not have
    int used[CRAG_ATTR_MAX_CLAUSES], n_used = 0;
    for (int c = 0; c < CRAG_ATTR_MAX_CLAUSES; ++c) {
        if (h_clause_sets[c] & beyond) return fail(CRAG_EINVAL, "attr_masks_host: clause_sets[%d] has a bit at or above nq", c);
        if (h_clause_sets[c]) used[n_used++] = c;
    }
    for (int j = 0; j < n_keys; ++j) {
        if (h_keys[j] < 0 || (int64_t)h_keys[j] >= n_attrs || (j > 0 && h_keys[j] <= h_keys[j - 1]))
            return fail(CRAG_EINVAL, "attr_masks_host: keys must be strictly ascending in [0, n_attrs) (key %d)", j);
        for (int c = 0; c < CRAG_ATTR_MAX_CLAUSES; ++c)
            if (h_key_sets[(size_t)j * CRAG_ATTR_MAX_CLAUSES + c] & ~h_clause_sets[c])
                return fail(CRAG_EINVAL, "attr_masks_host: key_sets[%d][%d] is not a subset of clause_sets[%d]", j, c, c);
    }
    if (mask_stride == 0) return CRAG_OK;   // (n_rows is 0: the runs are empty)

    const int nu = n_used <= 1 ? 1 : n_used <= 2 ? 2 : n_used <= 4 ? 4 : 8;
    // slot layout: sets [n_keys][nu] uint64 | keys [n_keys] int32 -- the clauses in use only, in clause order
    UploadPack up;
    const int i_sets = up.add((const uint64_t *)nullptr, 0, (size_t)n_keys * nu * 8);   // repacked from [n_keys][8] below
    const int i_keys = up.add(h_keys, (size_t)n_keys);
    if (up.bytes > 0) {   // (a call without keys uploads nothing)
        if ((rc = up.begin(slot)) != CRAG_OK) return rc;
        uint64_t *hs = up.host<uint64_t>(i_sets);
        for (int j = 0; j < n_keys; ++j)
            for (int u = 0; u < nu; ++u)
                hs[(size_t)j * nu + u] = u < n_used ? h_key_sets[(size_t)j * CRAG_ATTR_MAX_CLAUSES + used[u]] : 0;
        if ((rc = up.commit(slot, stream)) != CRAG_OK) return rc;
    }

    crag::AttrParams p;
    p.attr_ptr = d_attr_ptr;
    p.attr_ids = d_attr_ids;
    p.sets = up.dev<uint64_t>(i_sets);
    p.keys = up.dev<int32_t>(i_keys);
    for (int u = 0; u < CRAG_ATTR_MAX_CLAUSES; ++u) p.clause[u] = u < n_used ? h_clause_sets[used[u]] : 0;
    p.n = n_rows;
    p.n_attrs = n_attrs;
    p.n_words = (n_rows + 31) / 32;
    p.stride_w = mask_stride / 4;
    p.in_stride_w = in_stride / 4;
    p.n_keys = n_keys;
    p.nq = nq;
    p.in = (const uint32_t *)d_in_mask;
    p.out = (uint32_t *)d_out_mask;
    const int64_t n_spans = (p.stride_w + crag::MASK_SPAN_WORDS - 1) / crag::MASK_SPAN_WORDS;
    const int64_t cap = (int64_t)cu_count() * crag::ATTR_WGS_PER_CU;
    const dim3 grid((unsigned)(n_spans < cap ? n_spans : cap)), block(crag::MASK_THREADS);
    switch (nu) {
    case 1: hipLaunchKernelGGL(crag::attr_masks_kernel<1>, grid, block, 0, (hipStream_t)stream, p); break;
    case 2: hipLaunchKernelGGL(crag::attr_masks_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    case 4: hipLaunchKernelGGL(crag::attr_masks_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(crag::attr_masks_kernel<8>, grid, block, 0, (hipStream_t)stream, p); break;
    }
    return launch_ok("attr_masks");
}
