// crag_bm25_expand.hip -- prefix and fuzzy query terms of the BM25 lane expanded over the vocabulary on the GPU (gfx950),
// DESIGN.md 4.7d (the any-of row masks they become are made in crag_bm25_clause.hip).  `deploy*` stands for every vocabulary term that begins with
// "deploy", `kubernets~` for every term within Levenshtein distance 1 of it; the rule (include/crag_dense.h states it) is
// this tree's own.  The vocabulary lives on the device as a CSR of UTF-8 bytes in term-id order, df is a difference of
// post_ptr, and the two kernels of crag_bm25.hip score the kept terms with the bits they always had.
//
// bm25_expand_match_kernel, grid (slices of BM25_EXPAND_SLICE terms, pattern chunks): the workgroup reads its slice's
// offsets and bytes ONCE (byte offsets and code-point counts go to LDS) and then serves every pattern of its chunk against
// it, so the dictionary streams from memory once per chunk, not once per pattern; only the bytes of the terms that pass
// the length test are read again (from cache).  One chunk holds all patterns when the slices alone fill the chip; a small
// vocabulary splits the patterns until about 1024 workgroups exist (DESIGN.md 4.7d has the measurement behind it).
// A prefix pattern compares bytes (a byte prefix that is whole UTF-8 is a code-point prefix); a fuzzy pattern is rejected
// by the difference of the code-point counts and otherwise runs a Levenshtein recurrence over the five diagonals around
// the main one (exact for distances up to 2), the term decoded as it goes.
// A match becomes the 64-bit key (2 - dist) << 62 | df << 31 | (2^31 - 1 - term id) in an LDS list; the slice's largest 64
// are written sorted, with the number of matches.
// bm25_expand_merge_kernel, one workgroup per pattern: the largest 64 keys over the slices' lists (compacted into LDS
// first when at most 4096 are set), unpacked into term ids and distances, and the sum of the counts.
// Both selections are one routine: the keys are distinct (the term id is in them), so the 64th largest is found bit by bit
// from the top with one block-wide count per bit (the idea of crag_bm25.hip), and the at most 64 keys at or above it are
// ranked by counting.  LDS atomics only hand out list slots; what is kept and its order are functions of the key set.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_postings.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_WAVES = EX_THREADS / 64;
constexpr int EX_INF = 1 << 20;
constexpr int EX_MERGE_LDS = 4096;                               // keys the merge kernel holds in LDS
constexpr int EX_TARGET_GROUPS = 1024;                           // workgroups wanted of the match launch (256 CUs x 4)

static_assert(BM25_EXPAND_KEEP == CRAG_BM25_MAX_EXPANSIONS && BM25_EXPAND_KEEP == 64, "one lane per kept key");
static_assert(BM25_EXPAND_MAX_PATTERNS == CRAG_BM25_MAX_PATTERNS &&
              BM25_EXPAND_MAX_PATTERNS == BM25_MAX_Q * CRAG_BM25_MAX_EXPAND_ITEMS, "64 queries of 8 expanding items");

// next code point of b[0 .. len) at pos (pos < len); never reads at or beyond len, whatever the bytes
__device__ __forceinline__ uint32_t ex_decode(const uint8_t *b, int len, int &pos) {
    uint32_t c = b[pos++];
    if (c < 0x80u) return c;
    const int extra = c >= 0xF0u ? 3 : c >= 0xE0u ? 2 : c >= 0xC0u ? 1 : 0;
    c &= 0x3Fu >> extra;
    for (int k = 0; k < extra && pos < len && (b[pos] & 0xC0u) == 0x80u; ++k) c = (c << 6) | (b[pos++] & 0x3Fu);
    return c;
}

__device__ __forceinline__ int ex_count_points(const uint8_t *b, int len) {
    int pos = 0, n = 0;
    while (pos < len) {
        (void)ex_decode(b, len, pos);
        ++n;
    }
    return n;
}

// Levenshtein distance between the term tb[0 .. tlen) (n code points) and pat[0 .. m), |n - m| <= 2, over the diagonals
// j - i in [-2, 2]: exact when it is at most 2, above 2 otherwise.  Cell o of a row is column j = i + o - 2
__device__ __forceinline__ int ex_lev_band(const uint8_t *tb, int tlen, int n, const uint32_t *pat, int m, int d) {
    int prev[5], cur[5];
#pragma unroll
    for (int o = 0; o < 5; ++o) prev[o] = (o >= 2 && o - 2 <= m) ? o - 2 : EX_INF;
    int pos = 0;
    for (int i = 1; i <= n; ++i) {
        const uint32_t c = pos < tlen ? ex_decode(tb, tlen, pos) : 0xffffffffu;
        int best = EX_INF;
#pragma unroll
        for (int o = 0; o < 5; ++o) {
            const int j = i + o - 2;
            int v = EX_INF;
            if (j == 0) {
                v = i;
            } else if (j > 0 && j <= m) {
                v = prev[o] + (pat[j - 1] != c ? 1 : 0);
                if (o < 4) v = min(v, prev[o + 1] + 1);
                if (o > 0) v = min(v, cur[o - 1] + 1);
            }
            cur[o] = v;
            best = min(best, v);
        }
        if (best > d) return EX_INF;
#pragma unroll
        for (int o = 0; o < 5; ++o) prev[o] = cur[o];
    }
    int out = EX_INF;
#pragma unroll
    for (int o = 0; o < 5; ++o)
        if (o == m - n + 2) out = prev[o];
    return out;
}

// sum of v over the workgroup's EX_THREADS threads; s_red: EX_WAVES slots.  Ends with a barrier: s_red is free again
__device__ __forceinline__ long long ex_block_sum(long long v, long long *s_red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long tot = 0;
#pragma unroll
    for (int w = 0; w < EX_WAVES; ++w) tot += s_red[w];
    __syncthreads();
    return tot;
}

// The largest BM25_EXPAND_KEEP of keys[0 .. n) (zero: no key; the others distinct), sorted descending into out[0 .. 64),
// zero padded.  Called by the whole workgroup with the same arguments; keys and out may be LDS or memory; ends with a barrier
__device__ void ex_select_top(const uint64_t *keys, int64_t n, uint64_t *out, uint64_t *s_top, int *s_cnt,
                              long long *s_red) {
    const int tid = threadIdx.x;
    long long c = 0;
    for (int64_t i = tid; i < n; i += EX_THREADS) c += keys[i] != 0ull;
    const long long nz = ex_block_sum(c, s_red);
    uint64_t thr = 1ull;
    if (nz > BM25_EXPAND_KEEP) {   // the 64th largest key, bit by bit: exactly 64 keys are >= it
        thr = 0ull;
        for (int b = 63; b >= 0; --b) {
            const uint64_t cand = thr | (1ull << b);
            c = 0;
            for (int64_t i = tid; i < n; i += EX_THREADS) c += keys[i] >= cand;
            const long long tot = ex_block_sum(c, s_red);
            if (tot >= BM25_EXPAND_KEEP) {
                thr = cand;
                if (tot == BM25_EXPAND_KEEP) break;
            }
        }
    }
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += EX_THREADS) {
        const uint64_t k = keys[i];
        if (k >= thr) {   // (thr >= 1: never a zero)
            const int slot = atomicAdd(s_cnt, 1);
            if (slot < BM25_EXPAND_KEEP) s_top[slot] = k;
        }
    }
    __syncthreads();
    const int kept = min(*s_cnt, BM25_EXPAND_KEEP);
    if (tid < BM25_EXPAND_KEEP) {
        if (tid < kept) {   // the ranks of distinct keys are a permutation of 0 .. kept - 1
            const uint64_t mine = s_top[tid];
            out[rank_desc(s_top, kept, mine)] = mine;
        } else {
            out[tid] = 0ull;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(EX_THREADS) void bm25_expand_match_kernel(Bm25ExpandParams p) {
    __shared__ uint32_t s_off[BM25_EXPAND_SLICE + 1];   // byte offsets of the slice's terms, from the slice's first byte
    __shared__ uint16_t s_cpl[BM25_EXPAND_SLICE];       // their code-point counts (saturating: no pattern is that long)
    __shared__ uint64_t s_keys[BM25_EXPAND_SLICE];      // the matches of one pattern
    __shared__ uint32_t s_pat[BM25_EXPAND_MAX_BYTES];   // the pattern's code points
    __shared__ uint64_t s_top[BM25_EXPAND_KEEP];
    __shared__ long long s_red[EX_WAVES];
    __shared__ int s_n, s_m, s_cnt;
    const int tid = threadIdx.x, slice = blockIdx.x;
    const int64_t t0 = (int64_t)slice * BM25_EXPAND_SLICE;
    const int cnt = (int)(p.n_terms - t0 < BM25_EXPAND_SLICE ? p.n_terms - t0 : BM25_EXPAND_SLICE);
    const int64_t byte0 = p.term_ptr[t0];
    const uint8_t *bytes = p.term_bytes + byte0;
    for (int i = tid; i <= cnt; i += EX_THREADS) {
        const int64_t o = p.term_ptr[t0 + i] - byte0;
        s_off[i] = o > 0 ? (uint32_t)o : 0u;
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += EX_THREADS) {
        const uint32_t a = s_off[i], b = s_off[i + 1];
        const int n = b > a ? ex_count_points(bytes + a, (int)(b - a)) : 0;
        s_cpl[i] = (uint16_t)(n < 65535 ? n : 65535);
    }
    const int pi0 = blockIdx.y * p.pat_chunk, pi1 = pi0 + p.pat_chunk < p.np ? pi0 + p.pat_chunk : p.np;
    for (int pi = pi0; pi < pi1; ++pi) {
        const int pa = p.pat_ptr[pi], plen = p.pat_ptr[pi + 1] - pa, kind = p.pat_kind[pi];
        const uint8_t *pb = p.pat_bytes + pa;
        if (tid == 0) {
            int pos = 0, m = 0;
            while (pos < plen) s_pat[m++] = ex_decode(pb, plen, pos);   // (m <= plen <= 255)
            s_m = m;
            s_n = 0;
        }
        __syncthreads();   // (also: s_cpl is written, the last pattern's selection is over)
        const int m = s_m;
        for (int i = tid; i < cnt; i += EX_THREADS) {
            const uint32_t a = s_off[i], b = s_off[i + 1];
            const int tlen = b > a ? (int)(b - a) : 0;
            int dist = -1;
            if (kind == BM25_EXPAND_PREFIX) {
                if (tlen >= plen) {
                    int x = 0;
                    while (x < plen && bytes[a + x] == pb[x]) ++x;
                    if (x == plen) dist = 0;
                }
            } else {
                const int n = s_cpl[i];
                if (n - m <= kind && m - n <= kind) {
                    const int dd = ex_lev_band(bytes + a, tlen, n, s_pat, m, kind);
                    if (dd <= kind) dist = dd;
                }
            }
            if (dist >= 0) {
                const int64_t t = t0 + i;
                int64_t df = p.post_ptr[t + 1] - p.post_ptr[t];
                df = df < 0 ? 0 : df > 0x7fffffffll ? 0x7fffffffll : df;
                const uint64_t key = ((uint64_t)(2 - dist) << 62) | ((uint64_t)df << 31) | (uint64_t)(0x7fffffffll - t);
                s_keys[atomicAdd(&s_n, 1)] = key;   // (at most one match per term: at most cnt slots)
            }
        }
        __syncthreads();
        const int n_match = s_n;
        const int64_t cell = (int64_t)pi * p.n_slices + slice;
        ex_select_top(s_keys, n_match, p.slice_keys + cell * BM25_EXPAND_KEEP, s_top, &s_cnt, s_red);
        if (tid == 0) p.slice_count[cell] = n_match;
    }
}

__global__ __launch_bounds__(EX_THREADS) void bm25_expand_merge_kernel(Bm25ExpandParams p) {
    __shared__ uint64_t s_top[BM25_EXPAND_KEEP];
    __shared__ uint64_t s_sorted[BM25_EXPAND_KEEP];
    __shared__ long long s_red[EX_WAVES];
    __shared__ int s_cnt;
    __shared__ uint64_t s_list[EX_MERGE_LDS];   // the slices' keys without the padding, when they fit
    __shared__ int s_n;
    const int tid = threadIdx.x, pi = blockIdx.x;
    const int64_t first = (int64_t)pi * p.n_slices;
    const uint64_t *keys = p.slice_keys + first * BM25_EXPAND_KEEP;
    const int64_t n_keys = (int64_t)p.n_slices * BM25_EXPAND_KEEP;
    // most slices hold few matches: the keys are compacted into LDS once, so that the selection's passes (up to 65 over
    // all keys) do not go to memory.  The slots' order does not matter: the selection is a function of the key set
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int64_t i = tid; i < n_keys; i += EX_THREADS) {
        const uint64_t k = keys[i];
        if (k != 0ull) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < EX_MERGE_LDS) s_list[slot] = k;
        }
    }
    __syncthreads();
    if (s_n <= EX_MERGE_LDS) ex_select_top(s_list, s_n, s_sorted, s_top, &s_cnt, s_red);
    else ex_select_top(keys, n_keys, s_sorted, s_top, &s_cnt, s_red);
    long long c = 0;
    for (int s = tid; s < p.n_slices; s += EX_THREADS) c += p.slice_count[first + s];
    const long long total = ex_block_sum(c, s_red);
    c = tid < BM25_EXPAND_KEEP && s_sorted[tid] != 0ull;
    const long long kept = ex_block_sum(c, s_red);
    if (tid < BM25_EXPAND_KEEP) {
        const uint64_t key = s_sorted[tid];
        const int64_t at = (int64_t)pi * BM25_EXPAND_KEEP + tid;
        p.out_terms[at] = key ? (int32_t)(0x7fffffffll - (int64_t)(key & 0x7fffffffull)) : -1;
        p.out_dist[at] = key ? 2 - (int32_t)(key >> 62) : -1;
    }
    if (tid == 0) {
        p.out_kept[pi] = (int32_t)kept;
        p.out_total[pi] = total;
    }
}

// scratch layout: slice_keys [np][n_slices][64] uint64 | slice_count [np][n_slices] int32
inline int64_t ex_slices(int64_t n_terms) { return (n_terms + BM25_EXPAND_SLICE - 1) / BM25_EXPAND_SLICE; }

}  // namespace

int64_t bm25_expand_scratch_bytes(int64_t n_terms, int np) {
    const int64_t cells = ex_slices(n_terms) * (int64_t)np;
    return cells * BM25_EXPAND_KEEP * 8 + (cells * 4 + 7) / 8 * 8;
}

hipError_t launch_bm25_expand(const Bm25ExpandParams &p, hipStream_t st) {
    if (p.n_slices > 0) {
        const int n_chunks = (p.np + p.pat_chunk - 1) / p.pat_chunk;
        hipLaunchKernelGGL(bm25_expand_match_kernel, dim3((unsigned)p.n_slices, (unsigned)n_chunks), dim3(EX_THREADS), 0, st,
                           p);
    }
    hipLaunchKernelGGL(bm25_expand_merge_kernel, dim3((unsigned)p.np), dim3(EX_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag

extern "C" int64_t crag_bm25_expand_scratch_bytes(int64_t n_terms, int n_patterns) {
    if (n_terms < 0 || n_terms > INT32_MAX || n_patterns < 0 || n_patterns > crag::BM25_EXPAND_MAX_PATTERNS) return -1;
    return crag::bm25_expand_scratch_bytes(n_terms, n_patterns);
}

extern "C" int crag_bm25_expand_host(const int64_t *d_term_ptr, const uint8_t *d_term_bytes, const int64_t *d_post_ptr,
                                     int64_t n_terms, const int32_t *h_pat_ptr, const uint8_t *h_pat_bytes,
                                     const int32_t *h_pat_kind, int n_patterns, crag_upload_slot *slot, void *d_scratch,
                                     int64_t scratch_bytes, int32_t *d_out_terms, int32_t *d_out_dist, int32_t *d_out_kept,
                                     int64_t *d_out_total, void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (n_patterns < 0 || n_patterns > crag::BM25_EXPAND_MAX_PATTERNS)
        return fail(CRAG_EINVAL, "bm25_expand_host: need 0 <= n_patterns <= %d (got %d)", crag::BM25_EXPAND_MAX_PATTERNS,
                    n_patterns);
    int rc = check_bm25_counts("bm25_expand_host", 0, 0, 0, n_terms);   // (no queries, no rows: the vocabulary alone)
    if (rc != CRAG_OK) return rc;
    if (n_patterns == 0) return CRAG_OK;   // no pattern: no output
    if (!h_pat_ptr || !h_pat_bytes || !h_pat_kind || !slot)
        return fail(CRAG_EINVAL, "bm25_expand_host: NULL pointer argument");
    if (!d_out_terms || !d_out_dist || !d_out_kept || !d_out_total)
        return fail(CRAG_EINVAL, "bm25_expand_host: NULL output pointer");
    if (((uintptr_t)d_out_terms & 3) || ((uintptr_t)d_out_dist & 3) || ((uintptr_t)d_out_kept & 3) ||
        ((uintptr_t)d_out_total & 7))
        return fail(CRAG_EINVAL, "bm25_expand_host: the outputs must be aligned to their element size");
    if (n_terms > 0 && (!d_term_ptr || !d_term_bytes || !d_post_ptr))
        return fail(CRAG_EINVAL, "bm25_expand_host: NULL dictionary pointer");
    if (((uintptr_t)d_term_ptr & 7) || ((uintptr_t)d_post_ptr & 7))
        return fail(CRAG_EINVAL, "bm25_expand_host: term_ptr and post_ptr must be 8-byte aligned");
    rc = check_csr("bm25_expand_host", "pat_ptr", "pattern", h_pat_ptr, n_patterns, crag::BM25_EXPAND_MAX_BYTES);
    if (rc != CRAG_OK) return rc;
    for (int i = 0; i < n_patterns; ++i) {
        if (h_pat_ptr[i + 1] == h_pat_ptr[i]) return fail(CRAG_EINVAL, "bm25_expand_host: pattern %d is empty", i);
        if (h_pat_kind[i] < crag::BM25_EXPAND_PREFIX || h_pat_kind[i] > crag::BM25_EXPAND_FUZZY2)
            return fail(CRAG_EINVAL, "bm25_expand_host: pattern %d has the unknown kind %d", i, h_pat_kind[i]);
    }
    const int64_t need = crag::bm25_expand_scratch_bytes(n_terms, n_patterns);
    if (need > 0) {
        if (!d_scratch) return fail(CRAG_EINVAL, "bm25_expand_host: NULL scratch");
        rc = check_scratch("bm25_expand_host", d_scratch, scratch_bytes, need, "crag_bm25_expand_scratch_bytes");
        if (rc != CRAG_OK) return rc;
    }

    // slot layout: pat_ptr [np + 1] int32 | pat_kind [np] int32 | the patterns' bytes
    UploadPack up;
    const int i_ptr = up.add(h_pat_ptr, (size_t)n_patterns + 1);
    const int i_kind = up.add(h_pat_kind, (size_t)n_patterns);
    const int i_bytes = up.add(h_pat_bytes, (size_t)h_pat_ptr[n_patterns]);
    if ((rc = up.begin(slot)) != CRAG_OK || (rc = up.commit(slot, stream)) != CRAG_OK) return rc;

    crag::Bm25ExpandParams p;
    p.term_ptr = d_term_ptr;
    p.term_bytes = d_term_bytes;
    p.post_ptr = d_post_ptr;
    p.pat_ptr = up.dev<int32_t>(i_ptr);
    p.pat_kind = up.dev<int32_t>(i_kind);
    p.pat_bytes = up.dev<uint8_t>(i_bytes);
    p.n_terms = n_terms;
    p.n_slices = (int)crag::ex_slices(n_terms);
    p.np = n_patterns;
    // a small vocabulary has few slices: the patterns are then split over blockIdx.y until about EX_TARGET_GROUPS
    // workgroups exist (each re-reads its slice; the cells they fill do not depend on the split)
    const int want = p.n_slices > 0 ? (crag::EX_TARGET_GROUPS + p.n_slices - 1) / p.n_slices : 1;
    const int n_chunks = want < n_patterns ? want : n_patterns;
    p.pat_chunk = (n_patterns + n_chunks - 1) / n_chunks;
    p.slice_keys = (uint64_t *)d_scratch;
    p.slice_count = (int32_t *)((char *)d_scratch + (int64_t)p.n_slices * n_patterns * crag::BM25_EXPAND_KEEP * 8);
    p.out_terms = d_out_terms;
    p.out_dist = d_out_dist;
    p.out_kept = d_out_kept;
    p.out_total = d_out_total;
    HIP_TRY(crag::launch_bm25_expand(p, (hipStream_t)stream));
    return CRAG_OK;
}
