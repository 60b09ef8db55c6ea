// crag_logprobs.hip — the log-probability of a chosen token, its rank, the mass a grammar left allowed and the top
// candidates of a row of fp32 logits (gfx950).  C ABI: include/crag_encoder.h.
//
//   crag_enc_logprobs   per row: lse_all, lse_allowed, logprob = l_token - lse_all, rank, the n_top best (id, logprob).
//
// One workgroup of 1024 threads per row, two passes over the row (the second comes from L2).  A logit becomes
// crag_sample.hip's order-preserving key (fkey: -0 folded into +0), a candidate the 64-bit word (key << 32) | ~id, whose
// integer order is (logit descending, id ascending) read from the top:
//   pass 1      the largest key over the candidates (not NaN) and over the allowed ones, the number of candidates and the
//               number whose key lies above the token's: integer maxima and integer sums.
//   pass 2      the weights expf(l - m_all) and expf(l - m_alw) as 64-bit fixed-point integers (SampleParams::scale's
//               unit), summed per thread, per wave by shuffles and per workgroup by an integer add on LDS; and the
//               candidates at or above `floor` go into LDS.  floor = the smallest of the 16 waves' own maxima from pass
//               1: sixteen different candidates lie at or above it, so the n_top <= 16 best do, and on a row without
//               long runs of equal logits only a few dozen more.
//   top         every candidate in LDS counts the ones ahead of it; the one with c < n_top ahead is entry c.  When more
//               than LOGPROBS_CAP candidates reach the floor (a row of equal logits, a row that is NaN for whole waves)
//               n_top rounds of a workgroup maximum over the row take its place: the largest word below the last one.
// Every atomic is an integer add on LDS, every store a plain vector store, every sum an integer sum: a row's outputs are
// the same bits on every run and depend on the row's own logits, bits and token alone.

#include <math.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

typedef unsigned long long u64;

constexpr int LOGPROBS_THREADS = 1024;
constexpr int LOGPROBS_WAVES = LOGPROBS_THREADS / 64;
constexpr int LOGPROBS_CAP = 4096;    // candidates in LDS: 32 KiB
constexpr int LOGPROBS_UNROLL = 8;    // loads of a thread in flight

static_assert(CRAG_LOGPROBS_MAX_TOP <= LOGPROBS_WAVES, "the floor of pass 2 stands for at most one candidate per wave");

struct LogprobParams {
    const float *logits;
    int64_t vocab;
    const uint32_t *allowed_bits;
    int64_t n_words;
    const int32_t *token;
    double scale;   // fixed-point unit of a weight: 2^40, less for a vocabulary whose sum would not fit 64 bits
    int n_top;
    float *logprob;
    float *lse_all;
    float *lse_allowed;
    int32_t *rank;
    int32_t *top_id;
    float *top_logprob;
};

__device__ __forceinline__ u64 word_of(uint32_t key, int32_t id) { return ((u64)key << 32) | (u64)(~(uint32_t)id); }
__device__ __forceinline__ int32_t word_id(u64 w) { return (int32_t)(~(uint32_t)w); }

// m + ln(sum / scale) for the weights relative to the maximum key kmax; 0 stands for "no candidate"
__device__ __forceinline__ float lse_of(uint32_t kmax, u64 sum, double scale) {
    if (kmax == 0u) return -INFINITY;
    const float m = kfloat(kmax);
    if (m == INFINITY || m == -INFINITY) return m;
    return m + logf((float)((double)sum / scale));
}

__global__ __launch_bounds__(LOGPROBS_THREADS) void logprobs_kernel(const LogprobParams p) {
    __shared__ u64 s_word[LOGPROBS_CAP];
    __shared__ u64 s_sum[2];               // the fixed-point weights: all, allowed
    __shared__ u64 s_red[LOGPROBS_WAVES];
    __shared__ uint32_t s_kall[LOGPROBS_WAVES];
    __shared__ uint32_t s_kalw[LOGPROBS_WAVES];
    __shared__ uint32_t s_count[2];        // candidates, candidates above the token
    __shared__ uint32_t s_n;               // candidates at or above the floor
    __shared__ u64 s_prev;
    __shared__ float s_lse;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const int64_t vocab = p.vocab;
    const float *row = p.logits + (int64_t)r * vocab;
    const uint32_t *bits = p.allowed_bits ? p.allowed_bits + (int64_t)r * p.n_words : nullptr;
    const int n_top = p.n_top;

    const int32_t t = p.token[r];
    const float lt = (t >= 0 && (int64_t)t < vocab) ? row[t] : __uint_as_float(0x7fc00000u);
    const bool t_ok = lt == lt;
    const uint32_t tkey = t_ok ? fkey(lt) : 0xFFFFFFFFu;

    // the candidates of the row -- not NaN -- with their allowed flag, a thread's ids in ascending order.
    // LOGPROBS_UNROLL loads are in flight before the first is used: a row is one workgroup, bound by load latency.
    auto for_candidates = [&](auto &&f) {
        for (int64_t base = tid; base < vocab; base += (int64_t)LOGPROBS_THREADS * LOGPROBS_UNROLL) {
            float l[LOGPROBS_UNROLL];
            uint32_t w[LOGPROBS_UNROLL];
#pragma unroll
            for (int u = 0; u < LOGPROBS_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * LOGPROBS_THREADS;
                l[u] = i < vocab ? row[i] : __uint_as_float(0x7fc00000u);
                w[u] = (bits && i < vocab) ? bits[i >> 5] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int u = 0; u < LOGPROBS_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * LOGPROBS_THREADS;
                if (l[u] == l[u]) f((int32_t)i, l[u], ((w[u] >> (i & 31)) & 1u) != 0u);
            }
        }
    };

    if (tid == 0) {
        s_sum[0] = s_sum[1] = 0;
        s_count[0] = s_count[1] = 0;
        s_n = 0;
        s_prev = ~0ull;
    }

    // ---- pass 1: the two maxima, the candidates, the candidates above the token ----
    uint32_t kall = 0, kalw = 0, ncand = 0, ngt = 0;   // key 0 belongs to a NaN: no candidate has it
    for_candidates([&](int32_t, float l, bool allowed) {
        const uint32_t key = fkey(l);
        kall = key > kall ? key : kall;
        if (allowed) kalw = key > kalw ? key : kalw;
        ++ncand;
        ngt += key > tkey ? 1u : 0u;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oa = __shfl_xor(kall, o), ow = __shfl_xor(kalw, o);
        kall = oa > kall ? oa : kall;
        kalw = ow > kalw ? ow : kalw;
        ncand += __shfl_xor(ncand, o);
        ngt += __shfl_xor(ngt, o);
    }
    __syncthreads();   // the zeroes above
    if (lane == 0) {
        s_kall[wave] = kall;
        s_kalw[wave] = kalw;
        atomicAdd(&s_count[0], ncand);
        atomicAdd(&s_count[1], ngt);
    }
    __syncthreads();
    uint32_t floor_key = 0xFFFFFFFFu;
    kall = kalw = 0;
    for (int k = 0; k < LOGPROBS_WAVES; ++k) {
        const uint32_t a = s_kall[k], w = s_kalw[k];
        kall = a > kall ? a : kall;
        kalw = w > kalw ? w : kalw;
        floor_key = a < floor_key ? a : floor_key;   // 0 when a wave saw no candidate: everything is at or above it
    }
    ncand = s_count[0];
    const float m_all = kfloat(kall), m_alw = kfloat(kalw);
    const bool sum_all = kall != 0u && m_all != INFINITY && m_all != -INFINITY;
    const bool sum_alw = bits && p.lse_allowed && kalw != 0u && m_alw != INFINITY && m_alw != -INFINITY;

    // ---- pass 2: the weights, and the candidates at or above the floor into LDS ----
    if (sum_all || sum_alw || n_top > 0) {
        u64 wa = 0, ww = 0;
        for_candidates([&](int32_t i, float l, bool allowed) {
            if (sum_all) wa += (u64)((double)expf(l - m_all) * p.scale);
            if (sum_alw && allowed) ww += (u64)((double)expf(l - m_alw) * p.scale);
            if (n_top > 0) {
                const uint32_t key = fkey(l);
                if (key >= floor_key) {
                    const uint32_t slot = atomicAdd(&s_n, 1u);
                    if (slot < (uint32_t)LOGPROBS_CAP) s_word[slot] = word_of(key, i);
                }
            }
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            wa += __shfl_xor(wa, o);
            ww += __shfl_xor(ww, o);
        }
        if (lane == 0) {
            if (sum_all) atomicAdd(&s_sum[0], wa);
            if (sum_alw) atomicAdd(&s_sum[1], ww);
        }
    }
    __syncthreads();

    if (tid == 0) {
        const float lse = lse_of(kall, s_sum[0], p.scale);
        s_lse = lse;
        if (p.lse_all) p.lse_all[r] = lse;
        if (p.lse_allowed) p.lse_allowed[r] = bits ? lse_of(kalw, s_sum[1], p.scale) : lse;
        p.logprob[r] = lt - lse;   // a NaN lt (an id outside the row, a NaN logit) gives NaN
        if (p.rank) p.rank[r] = t_ok ? (int32_t)(1u + s_count[1]) : 0;
    }
    if (n_top == 0) return;
    __syncthreads();
    const float lse = s_lse;
    int32_t *top_id = p.top_id + (int64_t)r * n_top;
    float *top_lp = p.top_logprob + (int64_t)r * n_top;
    // the entries behind the last candidate
    if (tid < n_top && (uint32_t)tid >= ncand) {
        top_id[tid] = -1;
        top_lp[tid] = __uint_as_float(0x7fc00000u);
    }
    const uint32_t n_lds = s_n;
    if (n_lds <= (uint32_t)LOGPROBS_CAP) {
        // all of the n_top best are in LDS; words are distinct, so the counts are a permutation
        for (uint32_t i = tid; i < n_lds; i += LOGPROBS_THREADS) {
            const u64 mine = s_word[i];
            uint32_t ahead = 0;
            for (uint32_t j = 0; j < n_lds; ++j) ahead += s_word[j] > mine ? 1u : 0u;
            if (ahead < (uint32_t)n_top) {
                top_id[ahead] = word_id(mine);
                top_lp[ahead] = kfloat((uint32_t)(mine >> 32)) - lse;
            }
        }
        return;
    }
    // too many candidates share the top: round k takes the largest word below round k - 1's
    const int rounds = ncand < (uint32_t)n_top ? (int)ncand : n_top;
    for (int k = 0; k < rounds; ++k) {
        const u64 prev = s_prev;
        u64 best = 0;
        for_candidates([&](int32_t i, float l, bool) {
            const u64 w = word_of(fkey(l), i);
            if (w < prev && w > best) best = w;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 ob = __shfl_xor(best, o);
            best = ob > best ? ob : best;
        }
        if (lane == 0) s_red[wave] = best;
        __syncthreads();
        if (tid == 0) {
            for (int j = 1; j < LOGPROBS_WAVES; ++j) best = s_red[j] > best ? s_red[j] : best;
            top_id[k] = word_id(best);
            top_lp[k] = kfloat((uint32_t)(best >> 32)) - lse;
            s_prev = best;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int crag_enc_logprobs(const float *logits, int64_t vocab, const uint32_t *allowed_bits, const int32_t *token,
                      float *logprob, float *lse_all, float *lse_allowed, int32_t *rank, int32_t *top_id,
                      float *top_logprob, int n_top, int n_rows, void *stream) {
    if (!logits || !token || !logprob) return efail("logprobs: NULL pointer (logits, token and logprob are required)");
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS)
        return efail("logprobs: n_rows must be in 1..%d (got %d)", CRAG_DECODE_MAX_SEQS, n_rows);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("logprobs: vocab must be in 1..2^31 - 1");
    if (n_top < 0 || n_top > CRAG_LOGPROBS_MAX_TOP || (int64_t)n_top > vocab)
        return efail("logprobs: n_top must be in 0..%d and at most vocab (got %d)", CRAG_LOGPROBS_MAX_TOP, n_top);
    if (n_top > 0 && (!top_id || !top_logprob)) return efail("logprobs: n_top > 0 needs top_id and top_logprob, not NULL");
    if (((uintptr_t)logits | (uintptr_t)allowed_bits | (uintptr_t)token | (uintptr_t)logprob | (uintptr_t)lse_all |
         (uintptr_t)lse_allowed | (uintptr_t)rank | (uintptr_t)top_id | (uintptr_t)top_logprob) & 3)
        return efail("logprobs: every pointer must be 4-byte aligned");
    LogprobParams p;
    p.logits = logits;
    p.vocab = vocab;
    p.allowed_bits = allowed_bits;
    p.n_words = (vocab + 31) / 32;
    p.token = token;
    int width = 0;   // bits of vocab: vocab weights of at most `scale` each sum below 2^62 (crag_enc_sample's unit)
    while (((int64_t)1 << width) <= vocab) ++width;
    p.scale = ldexp(1.0, 62 - width < 40 ? 62 - width : 40);
    p.n_top = n_top;
    p.logprob = logprob;
    p.lse_all = lse_all;
    p.lse_allowed = lse_allowed;
    p.rank = rank;
    p.top_id = top_id;
    p.top_logprob = top_logprob;
    hipLaunchKernelGGL(logprobs_kernel, dim3((unsigned)n_rows), dim3(LOGPROBS_THREADS), 0, (hipStream_t)stream, p);
    return hip_ok("logprobs");
}

}  // extern "C"
