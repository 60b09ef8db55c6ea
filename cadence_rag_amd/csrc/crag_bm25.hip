// crag_bm25.hip -- the BM25 lexical lane of hybrid /retrieve on the GPU (gfx950).
// A self-defined restatement of the published BM25 form Tantivy (pg_search) uses -- NOT parity with pg_search, whose
// arithmetic is not in the reference tree (DESIGN.md 4.7 lists the departures).  It stands in for the SQL of
// _fetch_chunks_bm25 / _fetch_artifacts_bm25 (the reference's app/retrieve.py:123-180).
//
//   score(row) = sum over the query's terms t, ascending term id, of  w_t * tf / (tf + k1 * (1 - b + b * dl / avgdl))
//   w_t = qtf * idf * (k1 + 1), fp64 on the host, rounded once; everything else fp32 here, one rounding per operation.
//
// Launch 1, bm25_score_kernel, grid (row ranges, queries): a range is BM25_RANGE consecutive row positions whose fp32
// accumulators live in LDS.  Term after term the workgroup streams the term's postings that fall into the range and adds
// their contributions with a plain LDS read-add-write (positions inside one term's list are distinct) and a barrier
// between terms: no floating-point atomics, and a fixed order of the sum.  It then selects the range's top k among the
// touched, unmasked accumulators and writes them as a sorted list of 64-bit keys.
// Launch 2, bm25_merge_kernel, one workgroup per query: top k of the ranges' lists, ids and scores written out.
// Both selections are the same routine: the keys of a workgroup are distinct, so the k-th largest is found bit by bit
// from the top (one block-wide count per bit, the keys stay in registers) and exactly k keys are >= it.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_postings.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int BM25_THREADS = 1024;
constexpr int BM25_WAVES = BM25_THREADS / 64;
constexpr int BM25_PER = BM25_RANGE / BM25_THREADS;  // accumulators per thread in the selection (contiguous)
constexpr int BM25_TCHUNK = 256;                     // query terms located per round (any number of rounds)
constexpr int BM25_MERGE_PER = 5;                    // keys per thread and round of the merge
constexpr float BM25_K1 = 1.2f, BM25_B = 0.75f;

static_assert(BM25_RANGE == 1 << 14, "the range-local key packs the position into 14 bits");
static_assert(BM25_PER == 16, "one half mask word per thread");
static_assert(BM25_MERGE_PER * BM25_THREADS >= 2 * CRAG_MAX_K, "a merge round takes the running best plus one list");

// Number of keys >= thr in the workgroup.  s_part: 16 ints; consecutive calls alternate between two such buffers, so one
// barrier per call is enough (a wave can be at most one call ahead of the slowest reader).
template <int NPER>
__device__ __forceinline__ int block_count_ge(const uint64_t (&key)[NPER], uint64_t thr, int *s_part) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < NPER; ++j) c += __popcll(__ballot(key[j] >= thr));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < BM25_WAVES; ++w) tot += s_part[w];
    return tot;
}

// The kk-th largest key (1 <= kk <= number of non-zero keys; non-zero keys are distinct): exactly kk keys are >= it.
template <int NPER>
__device__ __forceinline__ uint64_t select_threshold(const uint64_t (&key)[NPER], int kk, int top_bit, int *s_part2) {
    uint64_t thr = 0;
    int pass = 0;
    for (int b = top_bit; b >= 0; --b, ++pass) {
        const uint64_t cand = thr | (1ull << b);
        const int c = block_count_ge(key, cand, s_part2 + (pass & 1) * BM25_WAVES);
        if (c >= kk) {
            thr = cand;
            if (c == kk) break;
        }
    }
    __syncthreads();
    return thr;
}

__global__ __launch_bounds__(BM25_THREADS) void bm25_score_kernel(Bm25Params p) {
#pragma clang fp contract(off)
    __shared__ alignas(16) float acc[BM25_RANGE];
    __shared__ int64_t s_lo[BM25_TCHUNK];
    __shared__ int s_len[BM25_TCHUNK];
    __shared__ float s_w[BM25_TCHUNK];
    __shared__ int s_part[2 * BM25_WAVES];
    __shared__ uint64_t s_sel[CRAG_MAX_K];
    __shared__ int s_n;
    const int rg = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t base = (int64_t)rg * BM25_RANGE;
    const int64_t end = base + BM25_RANGE < p.n ? base + BM25_RANGE : p.n;   // (n_ranges comes from n: no empty range)
    const int t0 = p.q_ptr[q], t1 = p.q_ptr[q + 1];
    int32_t *cnt_out = p.part_cnt + ((size_t)q * p.n_ranges + rg);
    bool zeroed = false;
    if (tid == 0) s_n = 0;
    for (int c0 = t0; c0 < t1; c0 += BM25_TCHUNK) {
        const int nt = t1 - c0 < BM25_TCHUNK ? t1 - c0 : BM25_TCHUNK;
        int64_t lo = 0, hi = 0;
        if (tid < nt)   // lanes search different terms: the workgroup pays one latency chain per round
            posting_slice(p.post_ptr, p.post_pos, p.q_term[c0 + tid], base, end, lo, hi);
        // (the barrier of this vote also keeps the previous round's readers of s_lo / s_len ahead of the writes below)
        if (!__syncthreads_or(hi > lo)) continue;   // no term of this round has a posting in the range
        if (tid < nt) {
            s_lo[tid] = lo;
            s_len[tid] = (int)(hi - lo);
            s_w[tid] = p.q_w[c0 + tid];
        }
        if (!zeroed) {
            float4 *a4 = (float4 *)acc;
            for (int i = tid; i < BM25_RANGE / 4; i += BM25_THREADS) a4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            zeroed = true;
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {   // ascending term id: the order of every row's sum
            const int len = s_len[t];
            if (len == 0) continue;
            const int64_t l0 = s_lo[t];
            const float w = s_w[t];
            for (int i = tid; i < len; i += BM25_THREADS) {
                const int32_t pos = p.post_pos[l0 + i];
                if ((uint64_t)((int64_t)pos - base) >= (uint64_t)(end - base)) continue;   // (a list that does not ascend)
                const float tf = (float)p.post_tf[l0 + i];
                const float dl = (float)p.doc_len[pos];
                float x = dl / p.avgdl;
                x = x * BM25_B;
                x = x + (1.0f - BM25_B);
                x = x * BM25_K1;
                const float den = tf + x;
                const float frac = tf / den;
                const int li = (int)((int64_t)pos - base);
                acc[li] = acc[li] + w * frac;
            }
            __syncthreads();
        }
    }
    if (!zeroed) {   // (uniform) nothing of the query in this range
        if (tid == 0) *cnt_out = 0;
        return;
    }
    // ---- the range's top k among the touched, unmasked rows ----
    const int l0 = tid * BM25_PER;
    const int64_t g0 = base + l0;
    uint32_t mbits = g0 < p.n ? 0xffffu : 0u;
    if (p.mask && g0 < p.n) mbits = (p.mask[(size_t)q * (size_t)p.mask_stride_w + (size_t)(g0 >> 5)] >> (g0 & 31)) & 0xffffu;
    uint64_t key[BM25_PER];
#pragma unroll
    for (int j4 = 0; j4 < BM25_PER / 4; ++j4) {
        const float4 v = ((const float4 *)(acc + l0))[j4];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j4 * 4 + u;
            const uint32_t bits = __float_as_uint(f[u]);   // > 0 exactly when a term touched the row (idf > 0)
            const bool ok = bits != 0u && ((mbits >> j) & 1u);
            // positive floats order as integers; the lower position wins a tie
            key[j] = ok ? ((uint64_t)bits << 14) | (uint64_t)(BM25_RANGE - 1 - (l0 + j)) : 0ull;
        }
    }
    const int nz = block_count_ge(key, 1ull, s_part);
    __syncthreads();
    const int kk = nz < p.k ? nz : p.k;
    if (kk == 0) {
        if (tid == 0) *cnt_out = 0;
        return;
    }
    const uint64_t thr = nz <= p.k ? 1ull : select_threshold(key, kk, 44, s_part);
#pragma unroll
    for (int j = 0; j < BM25_PER; ++j) {
        if (key[j] >= thr) {
            const int slot = atomicAdd(&s_n, 1);   // (integer LDS counter: the order is fixed by the sort below)
            const uint32_t gpos = (uint32_t)(g0 + j);
            if (slot < CRAG_MAX_K) s_sel[slot] = ((key[j] >> 14) << 32) | (uint64_t)(0xffffffffu - gpos);
        }
    }
    __syncthreads();
    if (tid < kk) {
        const uint64_t mine = s_sel[tid];
        p.part_keys[((size_t)q * p.n_ranges + rg) * p.k + rank_desc(s_sel, kk, mine)] = mine;
    }
    if (tid == 0) *cnt_out = kk;
}

__global__ __launch_bounds__(BM25_THREADS) void bm25_merge_kernel(Bm25Params p) {
    __shared__ uint64_t s_best[CRAG_MAX_K];
    __shared__ uint64_t s_sel[CRAG_MAX_K];
    __shared__ int s_part[2 * BM25_WAVES];
    __shared__ int s_n;
    const int q = blockIdx.x, tid = threadIdx.x, k = p.k;
    const uint64_t *lists = p.part_keys + (size_t)q * p.n_ranges * k;
    const int32_t *cnts = p.part_cnt + (size_t)q * p.n_ranges;
    const int per_round = (BM25_MERGE_PER * BM25_THREADS - CRAG_MAX_K) / k;   // lists per round, >= 1
    int nb = 0;   // entries of s_best (unordered until the end)
    for (int r0 = 0; r0 < p.n_ranges; r0 += per_round) {
        const int nl = p.n_ranges - r0 < per_round ? p.n_ranges - r0 : per_round;
        if (tid == 0) s_n = 0;
        uint64_t key[BM25_MERGE_PER];
#pragma unroll
        for (int j = 0; j < BM25_MERGE_PER; ++j) {
            const int i = tid + j * BM25_THREADS;
            uint64_t v = 0ull;
            if (i < nl * k) {
                const int l = i / k, e = i - l * k;
                if (e < cnts[r0 + l]) v = lists[(size_t)(r0 + l) * k + e];
            } else if (i - nl * k < nb) {
                v = s_best[i - nl * k];
            }
            key[j] = v;
        }
        const int nz = block_count_ge(key, 1ull, s_part);
        __syncthreads();   // (also: s_best has been read, s_n is visible)
        const int kk = nz < k ? nz : k;
        if (kk == 0) continue;
        const uint64_t thr = nz <= k ? 1ull : select_threshold(key, kk, 62, s_part);
#pragma unroll
        for (int j = 0; j < BM25_MERGE_PER; ++j) {
            if (key[j] >= thr) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < CRAG_MAX_K) s_sel[slot] = key[j];
            }
        }
        __syncthreads();
        if (tid < kk) s_best[tid] = s_sel[tid];
        nb = kk;
        __syncthreads();
    }
    if (tid < k) {
        int64_t id = -1;
        float sc = __uint_as_float(0x7fc00000u);
        if (tid < nb) {
            const uint64_t mine = s_best[tid];
            const int r = rank_desc(s_best, nb, mine);
            const int64_t pos = (int64_t)(0xffffffffu - (uint32_t)mine);
            p.out_ids[(size_t)q * k + r] = p.ids ? p.ids[pos] : pos;
            p.out_scores[(size_t)q * k + r] = __uint_as_float((uint32_t)(mine >> 32));
        } else {
            p.out_ids[(size_t)q * k + tid] = id;
            p.out_scores[(size_t)q * k + tid] = sc;
        }
    }
    if (tid == 0) p.out_counts[q] = nb;
}

}  // namespace

int64_t bm25_scratch_bytes(int64_t n_rows, int nq, int k) {
    const int64_t ranges = (n_rows + BM25_RANGE - 1) / BM25_RANGE;
    const int64_t keys = ranges * nq * (int64_t)k * 8, cnt = ranges * nq * 4;
    return ((keys + cnt + 255) & ~(int64_t)255) + 256;
}

hipError_t launch_bm25(const Bm25Params &p, hipStream_t st) {
    if (p.n_ranges > 0)
        hipLaunchKernelGGL(bm25_score_kernel, dim3((unsigned)p.n_ranges, (unsigned)p.nq), dim3(BM25_THREADS), 0, st, p);
    hipLaunchKernelGGL(bm25_merge_kernel, dim3((unsigned)p.nq), dim3(BM25_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag

extern "C" {

// ---- the lane from host query terms (uploaded through the slot of crag_fusion.hip) ----

int64_t crag_bm25_scratch_bytes(int64_t n_rows, int nq, int k) {
    if (n_rows < 0 || n_rows > INT32_MAX || nq < 0 || nq > crag::BM25_MAX_Q || k <= 0 || k > CRAG_MAX_K) return -1;
    return crag::bm25_scratch_bytes(n_rows, nq, k);
}

int crag_bm25_lane_host(const int64_t *d_post_ptr, const int32_t *d_post_pos, const uint16_t *d_post_tf,
                        const int32_t *d_doc_len, const int64_t *d_ids, int64_t n_rows, int64_t n_terms, float avgdl,
                        const int32_t *h_q_ptr, const int32_t *h_term_ids, const float *h_weights, int nq, int k,
                        const uint8_t *d_row_mask, int64_t mask_stride, crag_upload_slot *slot, void *d_scratch,
                        int64_t scratch_bytes, int64_t *d_out_ids, float *d_out_scores, int32_t *d_out_counts,
                        void *stream) {
    // every check comes before the first HIP call: on error nothing is enqueued
    if (!d_post_ptr || !d_post_pos || !d_post_tf || !d_doc_len || !h_q_ptr || !slot || !d_scratch || !d_out_ids ||
        !d_out_scores || !d_out_counts)
        return fail(CRAG_EINVAL, "bm25_lane_host: NULL pointer argument");
    if (((uintptr_t)d_scratch & 7) != 0) return fail(CRAG_EINVAL, "bm25_lane_host: scratch must be 8-byte aligned");
    int rc = check_bm25_counts("bm25_lane_host", nq, 0, n_rows, n_terms);
    if (rc != CRAG_OK) return rc;
    if (k <= 0 || k > CRAG_MAX_K) return fail(CRAG_EINVAL, "bm25_lane_host: need 1 <= k <= %d (k=%d)", CRAG_MAX_K, k);
    if (n_rows > 0 && !(avgdl > 0.0f && avgdl < 3.0e38f)) return fail(CRAG_EINVAL, "bm25_lane_host: avgdl must be positive and finite");
    if (d_row_mask) {
        if (((uintptr_t)d_row_mask & 3) != 0) return fail(CRAG_EINVAL, "bm25_lane_host: row_mask must be 4-byte aligned");
        if (mask_stride != 0 && (mask_stride % 4 != 0 || mask_stride < (n_rows + 31) / 32 * 4))
            return fail(CRAG_EINVAL, "bm25_lane_host: mask_stride must be 0 or a multiple of 4 >= ceil(n_rows/32)*4");
    }
    if (scratch_bytes < crag::bm25_scratch_bytes(n_rows, nq, k))
        return fail(CRAG_EINVAL, "bm25_lane_host: scratch too small (crag_bm25_scratch_bytes)");
    if (nq == 0) return CRAG_OK;
    if ((rc = check_csr("bm25_lane_host", "q_ptr", "query", h_q_ptr, nq, -1)) != CRAG_OK) return rc;
    const int nt = h_q_ptr[nq];
    if (nt > 0 && (!h_term_ids || !h_weights)) return fail(CRAG_EINVAL, "bm25_lane_host: NULL term arrays");
    if ((rc = check_terms("bm25_lane_host", h_term_ids, 0, nt, n_terms)) != CRAG_OK) return rc;
    for (int q = 0; q < nq; ++q)
        for (int i = h_q_ptr[q]; i < h_q_ptr[q + 1]; ++i) {
            if (i > h_q_ptr[q] && h_term_ids[i] <= h_term_ids[i - 1])
                return fail(CRAG_EINVAL, "bm25_lane_host: the term ids of query %d must ascend strictly", q);
            if (!(h_weights[i] > 0.0f && h_weights[i] < 3.0e38f))
                return fail(CRAG_EINVAL, "bm25_lane_host: weights must be positive and finite");
        }
    // slot layout: q_ptr [BM25_MAX_Q + 4] int32 | term ids [nt] int32 | weights [nt] fp32
    UploadPack up;
    const int i_ptr = up.add(h_q_ptr, (size_t)nq + 1, (size_t)(crag::BM25_MAX_Q + 4) * 4);
    const int i_terms = up.add(h_term_ids, (size_t)nt);
    const int i_w = up.add(h_weights, (size_t)nt);
    if ((rc = up.begin(slot)) != CRAG_OK || (rc = up.commit(slot, stream)) != CRAG_OK) return rc;
    crag::Bm25Params p;
    p.post_ptr = d_post_ptr;
    p.post_pos = d_post_pos;
    p.post_tf = d_post_tf;
    p.doc_len = d_doc_len;
    p.ids = d_ids;
    p.q_ptr = up.dev<int32_t>(i_ptr);
    p.q_term = up.dev<int32_t>(i_terms);
    p.q_w = up.dev<float>(i_w);
    p.mask = (const uint32_t *)d_row_mask;
    p.mask_stride_w = mask_stride / 4;
    p.n = n_rows;
    p.n_ranges = (int)((n_rows + crag::BM25_RANGE - 1) / crag::BM25_RANGE);
    p.nq = nq;
    p.k = k;
    p.avgdl = avgdl;
    p.part_keys = (uint64_t *)d_scratch;
    p.part_cnt = (int32_t *)((char *)d_scratch + (size_t)p.n_ranges * nq * k * 8);
    p.out_ids = d_out_ids;
    p.out_scores = d_out_scores;
    p.out_counts = d_out_counts;
    HIP_TRY(crag::launch_bm25(p, (hipStream_t)stream));
    return CRAG_OK;
}

}  // extern "C"
