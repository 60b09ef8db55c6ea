// crag_penalty.hip — repetition control on a row of fp32 logits (gfx950): repetition, presence and frequency penalties,
// the n-gram ban, an exemption mask, a bias list, and the greedy token of the adjusted row.  C ABI: include/crag_encoder.h;
// the rule, operation by operation: cadence_rag_amd/penalties.py (adjust_host), which the kernel is held to bit for bit.
//
//   crag_enc_adjust_logits   per row: out = the adjusted logits, token = the lowest id among their maxima.
//
// One workgroup of 1024 threads per row.  The row owns a [vocab] int32 slice of the workspace, one word per id:
//   (c_out << 3) | biased << 2 | banned << 1 | seen_in_prompt        seen(t) = seen_in_prompt or c_out > 0
//   zero      the slice, with plain stores
//   scatter   a thread per history position: an integer atomic add of 8 for an id of the output, an atomic or of 1 for an
//             id of the prompt; a thread per output position j: when O[j .. j+n-2] equals the last n - 1 ids of O, an
//             atomic or of 2 on O[j+n-1]; a thread per bias entry: an atomic or of 4.  The operations commute: the slice
//             does not depend on their order.  The history has no cap: nothing of it lives in LDS.
//   walk      the vocabulary once: logit, slice word and exempt bit give the adjusted logit (adjust(), no contraction, the
//             correctly rounded division), a biased id finds its value by a binary search of the row's <= 256 entries in
//             LDS, the value is stored, and the thread keeps its best (value, id).  block_best merges them.
// Between the phases the workgroup fences at device scope and meets at a barrier: the atomics act in L2, and the walk's
// plain loads must not be served by lines the zeroing left in the CU's cache.
// Rows are only 4-byte aligned for a general vocabulary (4099, 33).  The slice is laid out with the logits row's own
// misalignment (id i sits at word i + mis of a 16-byte aligned slot, mis = the row's address / 4 mod 4), so from the first
// id at which the row is 16-byte aligned both are read 16 bytes at a time, ADJUST_UNROLL loads of each in flight per thread;
// the up to three ids before it and behind the last whole group are single 4-byte accesses.  out is stored 16 bytes at a
// time when its row has the logits row's misalignment (out == logits; two tensors of one shape), 4 bytes at a time
// otherwise.  Integer atomics on the row's own slice are the only atomics, every store is a plain vector store, and no
// float is summed: a row's bits are the same on every run and depend on its own logits, history and parameters alone.

#include <math.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

constexpr int ADJUST_THREADS = 1024;
constexpr int ADJUST_WAVES = ADJUST_THREADS / 64;
constexpr int ADJUST_UNROLL = 4;   // 16-byte loads of the row, and of the slice, a thread has in flight
constexpr uint32_t SEEN = 1u, BANNED = 2u, BIASED = 4u, COUNT_SHIFT = 3u;

struct AdjustParams {
    const float *logits;
    float *out;
    int64_t vocab;
    const int32_t *history;
    int64_t history_stride;
    const uint32_t *exempt_bits;
    const int32_t *bias_ids;
    const float *bias_values;
    int32_t *token;
    uint32_t *slices;
    int64_t slice_stride;
    int history_row[CRAG_DECODE_MAX_SEQS], prompt_len[CRAG_DECODE_MAX_SEQS], total_len[CRAG_DECODE_MAX_SEQS];
    int ngram[CRAG_DECODE_MAX_SEQS], bias_lo[CRAG_DECODE_MAX_SEQS], bias_n[CRAG_DECODE_MAX_SEQS];
    float repetition[CRAG_DECODE_MAX_SEQS], frequency[CRAG_DECODE_MAX_SEQS], presence[CRAG_DECODE_MAX_SEQS];
};

// steps a, b and c of the rule on one logit; `word` is the id's slice word.  Every operation rounds once, in this order.
__device__ __forceinline__ float adjust(float l, uint32_t word, float rp, float frequency, float presence) {
#pragma clang fp contract(off)
    const uint32_t c = word >> COUNT_SHIFT;
    if (((word & SEEN) || c) && rp != 1.0f) l = l > 0.0f ? __fdiv_rn(l, rp) : l * rp;
    if (c) {
        const float step = frequency * (float)c;
        l = l - step;
        l = l - presence;
    }
    if (word & BANNED) l = -INFINITY;
    return l;
}

__global__ __launch_bounds__(ADJUST_THREADS) void adjust_kernel(const AdjustParams p) {
#pragma clang fp contract(off)
    __shared__ int32_t s_bias_id[CRAG_ADJUST_MAX_BIAS];
    __shared__ float s_bias_value[CRAG_ADJUST_MAX_BIAS];
    __shared__ float s_bv[ADJUST_WAVES];
    __shared__ int s_bi[ADJUST_WAVES];

    const int tid = threadIdx.x, r = blockIdx.x;
    const int64_t vocab = p.vocab;
    const float *row = p.logits + (int64_t)r * vocab;
    float *out = p.out + (int64_t)r * vocab;
    uint32_t *slot = p.slices + (int64_t)r * p.slice_stride;              // 16-byte aligned, vocab + 4 words or more
    const int mis = (int)(((uintptr_t)row >> 2) & 3);                       // id i of the slice sits beside id i of the row
    uint32_t *slice = slot + mis;
    const bool wide_out = (((uintptr_t)out >> 2) & 3) == (uintptr_t)mis;
    const int32_t *hist = p.history + (int64_t)p.history_row[r] * p.history_stride;
    const int prompt_len = p.prompt_len[r], total = p.total_len[r], n_out = total - prompt_len;
    const int32_t *outp = hist + prompt_len;
    const int ngram = p.ngram[r], n_bias = p.bias_n[r];
    const float rp = p.repetition[r], frequency = p.frequency[r], presence = p.presence[r];

    if (tid < n_bias) {
        s_bias_id[tid] = p.bias_ids[p.bias_lo[r] + tid];
        s_bias_value[tid] = p.bias_values[p.bias_lo[r] + tid];
    }
    // ---- zero: the whole slot, 16 bytes at a time ----
    for (int64_t q = tid; q < p.slice_stride / 4; q += ADJUST_THREADS) reinterpret_cast<uint4 *>(slot)[q] = uint4{0u, 0u, 0u, 0u};
    __threadfence();
    __syncthreads();

    // ---- scatter: the history, the continuations of the last n - 1 output ids, the bias flags ----
    for (int i = tid; i < total; i += ADJUST_THREADS) {
        const int32_t t = hist[i];
        if (t >= 0 && (int64_t)t < vocab) {
            if (i < prompt_len)
                atomicOr(&slice[t], SEEN);
            else
                atomicAdd(&slice[t], 1u << COUNT_SHIFT);
        }
    }
    if (ngram > 0 && n_out >= ngram) {   // fewer output ids than n: no n-gram is complete yet, nothing to repeat
        const int m = ngram - 1;
        const int32_t *tail = outp + (n_out - m);
        for (int j = tid; j + m < n_out; j += ADJUST_THREADS) {
            bool same = true;
            for (int k = 0; k < m; ++k) same = same && outp[j + k] == tail[k];
            const int32_t t = outp[j + m];
            if (same && t >= 0 && (int64_t)t < vocab) atomicOr(&slice[t], BANNED);
        }
    }
    if (tid < n_bias) {
        const int32_t t = s_bias_id[tid];
        if (t >= 0 && (int64_t)t < vocab) atomicOr(&slice[t], BIASED);
    }
    __threadfence();
    __syncthreads();

    // ---- walk ----
    float bv = 0.f;
    int bid = -1;
    // the adjusted logit of id i from its logit, slice word and exempt bit; the thread's best so far
    auto finish = [&](int64_t i, float v, uint32_t word, uint32_t exempt_word) -> float {
        if (!((exempt_word >> (i & 31)) & 1u)) v = adjust(v, word, rp, frequency, presence);
        if (word & BIASED) {   // ascending ids: the entry of id i
            int lo = 0, hi = n_bias - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)s_bias_id[mid] < i) lo = mid + 1; else hi = mid;
            }
            v = v + s_bias_value[lo];
        }
        if (v == v && better(v, (int)i, bv, bid)) {
            bv = v;
            bid = (int)i;
        }
        return v;
    };
    const uint32_t *ex = p.exempt_bits;
    const int64_t head = ((4 - mis) & 3) < vocab ? ((4 - mis) & 3) : vocab;   // ids before the first aligned one
    const int64_t groups = (vocab - head) >> 2;                               // whole groups of four ids
    const int64_t tail0 = head + 4 * groups;
    if (tid < 8) {   // the single ids: head 0..2, tail 0..2
        const int64_t i = tid < 4 ? (int64_t)tid : tail0 + (tid - 4);
        if (tid < 4 ? i < head : i < vocab) out[i] = finish(i, row[i], slice[i], ex ? ex[i >> 5] : 0u);
    }
    for (int64_t base = tid; base < groups; base += (int64_t)ADJUST_THREADS * ADJUST_UNROLL) {
        float4 l[ADJUST_UNROLL];
        uint4 w[ADJUST_UNROLL];
        uint32_t e0[ADJUST_UNROLL], e1[ADJUST_UNROLL];
#pragma unroll
        for (int u = 0; u < ADJUST_UNROLL; ++u) {
            const int64_t q = base + (int64_t)u * ADJUST_THREADS;
            const bool in = q < groups;
            const int64_t i = head + 4 * (in ? q : 0);
            l[u] = *reinterpret_cast<const float4 *>(row + i);
            w[u] = *reinterpret_cast<const uint4 *>(slice + i);
            e0[u] = ex ? ex[i >> 5] : 0u;                 // a group may straddle two words of the mask
            e1[u] = ex ? ex[(i + 3) >> 5] : 0u;
        }
#pragma unroll
        for (int u = 0; u < ADJUST_UNROLL; ++u) {
            const int64_t q = base + (int64_t)u * ADJUST_THREADS;
            if (q >= groups) continue;
            const int64_t i = head + 4 * q;
            const bool split = ((i + 3) >> 5) != (i >> 5);
            float4 v;
            v.x = finish(i, l[u].x, w[u].x, e0[u]);
            v.y = finish(i + 1, l[u].y, w[u].y, (split && ((i + 1) & 31) < 3) ? e1[u] : e0[u]);
            v.z = finish(i + 2, l[u].z, w[u].z, (split && ((i + 2) & 31) < 3) ? e1[u] : e0[u]);
            v.w = finish(i + 3, l[u].w, w[u].w, e1[u]);
            if (wide_out) {
                *reinterpret_cast<float4 *>(out + i) = v;
            } else {
                out[i] = v.x;
                out[i + 1] = v.y;
                out[i + 2] = v.z;
                out[i + 3] = v.w;
            }
        }
    }
    const Best best = block_best<ADJUST_WAVES, false>(bv, bid, 0, s_bv, s_bi, nullptr);
    if (tid == 0) p.token[r] = best.id;
}

// words of a row's slot: the ids, up to three words in front of them, rounded up to whole 16-byte groups
int64_t slice_stride_of(int64_t vocab) { return ((vocab + 3) & ~(int64_t)3) + 4; }

}  // namespace

extern "C" {

int64_t crag_enc_adjust_workspace_bytes(int n_rows, int64_t vocab) {
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS || vocab <= 0 || vocab > 0x7fffffff) return 0;
    return (int64_t)n_rows * slice_stride_of(vocab) * (int64_t)sizeof(uint32_t);
}

int crag_enc_adjust_logits(const float *logits, float *out, int64_t vocab, const int32_t *history, int64_t history_stride,
                           int n_history_rows, const int32_t *h_history_row, const int32_t *h_prompt_len,
                           const int32_t *h_total_len, const float *h_repetition, const float *h_frequency,
                           const float *h_presence, const int32_t *h_ngram, const uint32_t *exempt_bits,
                           const int32_t *bias_ids, const float *bias_values, const int32_t *h_bias_offsets,
                           int32_t *token, void *workspace, int64_t workspace_bytes, int n_rows, void *stream) {
    if (!logits || !out || !history || !h_history_row || !h_prompt_len || !h_total_len || !h_repetition || !h_frequency ||
        !h_presence || !h_ngram || !token || !workspace)
        return efail("adjust_logits: NULL pointer (only exempt_bits and the three bias arrays may be NULL)");
    if ((bias_ids != nullptr) != (bias_values != nullptr) || (bias_ids != nullptr) != (h_bias_offsets != nullptr))
        return efail("adjust_logits: NULL pointer: bias_ids, bias_values and h_bias_offsets are given or left out together");
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS)
        return efail("adjust_logits: n_rows must be in 1..%d (got %d)", CRAG_DECODE_MAX_SEQS, n_rows);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("adjust_logits: vocab must be in 1..2^31 - 1");
    if (history_stride < 1 || history_stride > 0x7fffffff || n_history_rows < 1)
        return efail("adjust_logits: the history log needs at least one row of 1..2^31 - 1 ids");
    if ((((uintptr_t)logits | (uintptr_t)out | (uintptr_t)history | (uintptr_t)exempt_bits | (uintptr_t)bias_ids |
          (uintptr_t)bias_values | (uintptr_t)token) & 3) || ((uintptr_t)workspace & 15))
        return efail("adjust_logits: every device pointer must be 4-byte aligned, the workspace 16-byte aligned");
    AdjustParams p;
    int n_bias_all = 0;
    for (int r = 0; r < n_rows; ++r) {
        if (h_history_row[r] < 0 || h_history_row[r] >= n_history_rows)
            return efail("adjust_logits: row %d names history row %d of %d", r, h_history_row[r], n_history_rows);
        if (h_total_len[r] < 0 || (int64_t)h_total_len[r] > history_stride)
            return efail("adjust_logits: row %d: total_len %d outside 0..history_stride = %lld", r, h_total_len[r],
                         (long long)history_stride);
        if (h_prompt_len[r] < 0 || h_prompt_len[r] > h_total_len[r])
            return efail("adjust_logits: row %d: prompt_len %d outside 0..total_len = %d", r, h_prompt_len[r],
                         h_total_len[r]);
        if (!(h_repetition[r] >= CRAG_ADJUST_MIN_REPETITION && h_repetition[r] <= CRAG_ADJUST_MAX_REPETITION))
            return efail("adjust_logits: row %d: repetition penalty %g outside %g..%g", r, (double)h_repetition[r],
                         (double)CRAG_ADJUST_MIN_REPETITION, (double)CRAG_ADJUST_MAX_REPETITION);
        if (!(fabsf(h_frequency[r]) <= CRAG_ADJUST_MAX_ADDITIVE))
            return efail("adjust_logits: row %d: frequency penalty %g outside -%g..%g", r, (double)h_frequency[r],
                         (double)CRAG_ADJUST_MAX_ADDITIVE, (double)CRAG_ADJUST_MAX_ADDITIVE);
        if (!(fabsf(h_presence[r]) <= CRAG_ADJUST_MAX_ADDITIVE))
            return efail("adjust_logits: row %d: presence penalty %g outside -%g..%g", r, (double)h_presence[r],
                         (double)CRAG_ADJUST_MAX_ADDITIVE, (double)CRAG_ADJUST_MAX_ADDITIVE);
        if (h_ngram[r] != 0 && (h_ngram[r] < 2 || h_ngram[r] > CRAG_ADJUST_MAX_NGRAM))
            return efail("adjust_logits: row %d: no_repeat_ngram %d is neither 0 nor in 2..%d", r, h_ngram[r],
                         CRAG_ADJUST_MAX_NGRAM);
        p.history_row[r] = h_history_row[r];
        p.prompt_len[r] = h_prompt_len[r];
        p.total_len[r] = h_total_len[r];
        p.ngram[r] = h_ngram[r];
        p.repetition[r] = h_repetition[r];
        p.frequency[r] = h_frequency[r];
        p.presence[r] = h_presence[r];
        p.bias_lo[r] = p.bias_n[r] = 0;
        if (h_bias_offsets) {
            const int lo = h_bias_offsets[r], hi = h_bias_offsets[r + 1];
            if (lo < 0 || hi < lo || (r == 0 && lo != 0) || hi - lo > CRAG_ADJUST_MAX_BIAS)
                return efail("adjust_logits: row %d: a bias slice of 0..%d entries, offsets rising from 0 (got %d..%d)", r,
                             CRAG_ADJUST_MAX_BIAS, lo, hi);
            p.bias_lo[r] = lo;
            p.bias_n[r] = hi - lo;
            n_bias_all = hi;
        }
    }
    const int64_t need = crag_enc_adjust_workspace_bytes(n_rows, vocab);
    if (workspace_bytes < need)
        return fail(CRAG_E2BIG, "adjust_logits: the workspace holds %lld bytes, %d rows of %lld ids need %lld",
                    (long long)workspace_bytes, n_rows, (long long)vocab, (long long)need);
    if (n_bias_all > 0) {
        // the ids lie in device memory: they are read back, one small synchronous copy, to be checked before anything is
        // launched (a pointer the host can read is read in place)
        static thread_local int32_t ids[CRAG_DECODE_MAX_SEQS * CRAG_ADJUST_MAX_BIAS];
        const int32_t *seen = bias_ids;
        if (is_device_ptr(bias_ids)) {
            HIP_TRY(hipMemcpyAsync(ids, bias_ids, (size_t)n_bias_all * sizeof(int32_t), hipMemcpyDeviceToHost,
                                   (hipStream_t)stream));
            HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            seen = ids;
        }
        for (int r = 0; r < n_rows; ++r)
            for (int k = 0; k < p.bias_n[r]; ++k) {
                const int32_t t = seen[p.bias_lo[r] + k];
                if (t < 0 || (int64_t)t >= vocab || (k > 0 && t <= seen[p.bias_lo[r] + k - 1]))
                    return efail("adjust_logits: row %d: bias ids must be strictly ascending inside 0..vocab - 1 (entry %d "
                                 "is %d)", r, k, t);
            }
    }
    p.logits = logits;
    p.out = out;
    p.vocab = vocab;
    p.history = history;
    p.history_stride = history_stride;
    p.exempt_bits = exempt_bits;
    p.bias_ids = bias_ids;
    p.bias_values = bias_values;
    p.token = token;
    p.slices = (uint32_t *)workspace;
    p.slice_stride = slice_stride_of(vocab);
    hipLaunchKernelGGL(adjust_kernel, dim3((unsigned)n_rows), dim3(ADJUST_THREADS), 0, (hipStream_t)stream, p);
    return hip_ok("adjust_logits");
}

}  // extern "C"
