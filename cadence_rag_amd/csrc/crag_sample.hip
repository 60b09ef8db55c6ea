// crag_sample.hip — seeded token sampling over fp32 logits, and the automaton step behind a sampled token (gfx950).
// C ABI: include/crag_encoder.h.
//
//   crag_enc_sample           per row: temperature, top-k, top-p and min-p cuts as thresholds on the logit, then a draw by
//                             the Gumbel maximum with Philox4x32-10 noise keyed on (seed; token id, step, stream).
//   crag_enc_grammar_advance  per row: the automaton state behind the chosen token (grammar.next_state_host's rule).
//
// One workgroup of 1024 threads per row.  A logit becomes an order-preserving 32-bit key (-0 folded into +0), so every
// cut is an exact integer selection and ties stay together:
//   pass 1            the maximum m, the lowest id holding it and the number of ids holding it.  A T == 0 row, a row with
//                     no candidate and a row whose maximum is +inf end here: a greedy row costs what lm_argmax_kernel costs.
//   top-k             radix selection of the k-th largest key, 11 + 11 + 10 bits: a count histogram in LDS per level.
//   top-p             the same selection on weights: w = expf((l - m) / T) as a 64-bit fixed-point integer, so the
//                     histogram sums are integer sums -- exact, and independent of the order the atomics arrive in.
//   compaction        behind the first level of either selection the ids at or above the chosen bin are known to be
//                     n_ge; when n_ge <= SAMPLE_CAP one pass copies their (key, id) pairs into LDS and every later pass
//                     -- the lower levels, the other selection, the draw -- runs over LDS.  Otherwise they stay on the row.
//   draw              over the kept ids: Philox, the Gumbel key (l - m) / T - ln(-ln u), the (key, lowest id) maximum;
//                     the kept count and the lowest kept logit fall out of the same pass.  An id whose key cannot
//                     reach a key another kept id already has is left out of the maximum before its noise is computed.
// The min-p cut is the predicate (l - m) >= min_p_cut, applied wherever the row is read.  Every atomic is an integer
// add on LDS, every store a plain vector store, every sum an integer sum or a fixed tree: a row's outputs are the same
// bits on every run and depend on the row's own logits, bits and parameters alone.

#include <math.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

typedef unsigned long long u64;

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_CAP = 4096;      // (key, id) pairs in LDS: 32 KiB
constexpr int SAMPLE_BINS = 2048;     // the widest level: 11 bits
constexpr int SAMPLE_UNROLL = 8;      // loads of a thread in flight
constexpr float SAMPLE_SKIP = -21.f;  // see draw: below this (l - m) / T no noise can reach the maximum's key

struct SampleParams {
    const float *logits;
    int64_t vocab;
    const uint32_t *allowed_bits;
    int64_t n_words;
    float temperature[CRAG_DECODE_MAX_SEQS];
    int32_t top_k[CRAG_DECODE_MAX_SEQS];
    float top_p[CRAG_DECODE_MAX_SEQS];
    float min_p_cut[CRAG_DECODE_MAX_SEQS];
    uint32_t stream[CRAG_DECODE_MAX_SEQS];
    uint32_t seed_lo, seed_hi, step;
    double scale;   // fixed-point unit of a weight: 2^40, less for a vocabulary whose sum would not fit 64 bits
    int32_t *token;
    int32_t *kept;
    float *cut;
};

struct Pick {
    uint32_t bin, n_ge;
    u64 above, target;
    int nocut;
};

// word 0 of Philox4x32-10
__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// an upper bound of gumbel(x0) from integer work alone.  With v = 1 - u = (k' + 0.5) / 2^24, k' = 2^24 - 1 - (x0 >> 8):
// -ln u >= v, so -ln(-ln u) <= 24 ln 2 - ln(k' + 0.5) <= 16.64 - ln 2 * floor(log2(k' + 0.5)); 16.7 leaves the fp32
// errors of gumbel() far behind.  (Below u = 1/2 the true value is at most 0.37 and the bound at least 0.7.)
__device__ __forceinline__ float gumbel_bound(uint32_t x0) {
    const uint32_t kp = 0xFFFFFFu - (x0 >> 8);
    const int e = kp ? 31 - __clz((int)kp) : -1;
    return 16.7f - 0.6931f * (float)e;
}

// floats as integers of the same order, for an integer maximum
__device__ __forceinline__ int fint(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

// -ln(-ln u), u = ((x0 >> 8) + 0.5) / 2^24.  Both branches start from a number fp32 holds exactly: u itself below one
// half, 1 - u above it (log1pf), so the value keeps its relative precision up to the last u before 1.
__device__ __forceinline__ float gumbel(uint32_t x0) {
    const uint32_t k = x0 >> 8;
    float t;
    if (k < (1u << 23))
        t = -logf(((float)k + 0.5f) * 0x1p-24f);
    else
        t = -log1pf(-((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f);
    return -logf(t);
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(const SampleParams p) {
    __shared__ uint32_t s_cnt[SAMPLE_BINS];
    __shared__ u64 s_wq[SAMPLE_BINS];
    __shared__ uint32_t s_ckey[SAMPLE_CAP];
    __shared__ int32_t s_cid[SAMPLE_CAP];
    __shared__ float s_v[SAMPLE_WAVES];
    __shared__ int s_i[SAMPLE_WAVES];
    __shared__ uint32_t s_c[SAMPLE_WAVES];
    __shared__ uint32_t s_k[SAMPLE_WAVES];
    __shared__ float s_m;
    __shared__ int s_stop;
    __shared__ uint32_t s_n;
    __shared__ Pick s_pick;
    __shared__ int s_best;   // draw: the largest key any thread holds so far, as fint(); it prunes, it decides nothing

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const int64_t vocab = p.vocab;
    const float *row = p.logits + (int64_t)r * vocab;
    const uint32_t *bits = p.allowed_bits ? p.allowed_bits + (int64_t)r * p.n_words : nullptr;
    const float T = p.temperature[r];
    const float mcut = p.min_p_cut[r];

    // the candidates of the row -- allowed, not NaN, not -inf -- a thread's ids in ascending order.  SAMPLE_UNROLL loads
    // are in flight before the first is used: a row is one workgroup, so a pass is bound by load latency, not by bytes.
    auto for_candidates = [&](auto &&f) {
        for (int64_t base = tid; base < vocab; base += (int64_t)SAMPLE_THREADS * SAMPLE_UNROLL) {
            float l[SAMPLE_UNROLL];
            uint32_t w[SAMPLE_UNROLL];
#pragma unroll
            for (int u = 0; u < SAMPLE_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * SAMPLE_THREADS;
                l[u] = i < vocab ? row[i] : -INFINITY;
                w[u] = (bits && i < vocab) ? bits[i >> 5] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int u = 0; u < SAMPLE_UNROLL; ++u) {
                const int64_t i = base + (int64_t)u * SAMPLE_THREADS;
                if (l[u] > -INFINITY && ((w[u] >> (i & 31)) & 1u)) f(i, l[u]);
            }
        }
    };

    // ---- pass 1: the maximum, the lowest id holding it, how many ids hold it ----
    float bv = 0.f;
    int bid = -1;
    uint32_t ties = 0;
    for_candidates([&](int64_t i, float l) {
        if (bid < 0 || l > bv) {   // ascending ids: an equal value keeps the lower id
            bv = l;
            bid = (int)i;
            ties = 1;
        } else if (l == bv) {
            ++ties;
        }
    });
    auto merge = [&](float ov, int oi, uint32_t oc) {
        if (oi < 0) return;
        if (bid >= 0 && ov == bv) {
            ties += oc;
            bid = oi < bid ? oi : bid;
        } else if (bid < 0 || ov > bv) {
            bv = ov;
            bid = oi;
            ties = oc;
        }
    };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bid, o);
        const uint32_t oc = __shfl_xor(ties, o);
        merge(ov, oi, oc);
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bid;
        s_c[wave] = ties;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < SAMPLE_WAVES; ++k) merge(s_v[k], s_i[k], s_c[k]);
        const bool done = bid < 0 || T == 0.f || bv == INFINITY;
        if (done) {
            p.token[r] = bid;
            if (p.kept) p.kept[r] = bid < 0 ? 0 : (int32_t)ties;
            if (p.cut) p.cut[r] = bid < 0 ? __uint_as_float(0x7fc00000u) : bv;
        }
        s_m = bv;
        s_stop = done;
        s_best = fint(-INFINITY);
    }
    __syncthreads();
    if (s_stop) return;
    const float m = s_m;

    // ---- the source of every later pass: the row, or the (key, id) pairs compacted into LDS ----
    bool in_lds = false;
    uint32_t n_lds = 0;
    auto for_each = [&](auto &&f) {
        if (in_lds) {
            for (uint32_t i = tid; i < n_lds; i += SAMPLE_THREADS) f(s_ckey[i], s_cid[i]);
        } else {
            for_candidates([&](int64_t i, float l) {
                if ((l - m) >= mcut) f(fkey(l), (int32_t)i);
            });
        }
    };
    auto weight = [&](uint32_t key) -> u64 {
        const float w = expf((kfloat(key) - m) / T);
        return (u64)((double)w * p.scale);
    };

    // the bin, counted from the top, at which the running measure (counts, or weights) reaches the target.  Wave 0 alone:
    // a lane sums its share of the bins in descending order, the lanes are scanned, the lane that crosses walks its bins.
    auto find_bin = [&](int nbins, bool weighted, bool first, u64 target, float top_p) {
        if (tid < 64) {
            const int per = nbins / 64, hi = nbins - 1 - tid * per;
            u64 ms = 0;
            uint32_t cs = 0;
            for (int j = 0; j < per; ++j) {
                cs += s_cnt[hi - j];
                ms += weighted ? s_wq[hi - j] : (u64)s_cnt[hi - j];
            }
            u64 mi = ms;
            uint32_t ci = cs;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 tm = __shfl_up(mi, o);
                const uint32_t tc = __shfl_up(ci, o);
                if (lane >= o) {
                    mi += tm;
                    ci += tc;
                }
            }
            const u64 total = __shfl(mi, 63);
            bool nocut = false;
            if (first) {
                if (weighted) {
                    const double want = ceil((double)top_p * (double)total);
                    target = want >= (double)total ? total : (u64)want;
                    if (target < 1) target = 1;
                } else {
                    nocut = total <= target;   // fewer candidates than k: top-k cuts nothing
                }
            }
            if (nocut) {
                if (tid == 0) s_pick.nocut = 1;
            } else if (mi - ms < target && target <= mi) {
                u64 acc = mi - ms;
                uint32_t cacc = ci - cs;
                for (int j = 0; j < per; ++j) {
                    const uint32_t cb = s_cnt[hi - j];
                    const u64 mb = weighted ? s_wq[hi - j] : (u64)cb;
                    if (acc + mb >= target) {
                        s_pick.bin = (uint32_t)(hi - j);
                        s_pick.n_ge = cacc + cb;
                        s_pick.above = acc;
                        s_pick.target = target;
                        s_pick.nocut = 0;
                        break;
                    }
                    acc += mb;
                    cacc += cb;
                }
            }
        }
        __syncthreads();
    };

    // copies the pairs of the row at or above low_key into LDS; the caller knows there are at most SAMPLE_CAP
    auto compact = [&](uint32_t low_key) {
        if (tid == 0) s_n = 0;
        __syncthreads();
        for_each([&](uint32_t key, int32_t id) {
            if (key >= low_key) {
                const uint32_t slot = atomicAdd(&s_n, 1u);
                if (slot < (uint32_t)SAMPLE_CAP) {
                    s_ckey[slot] = key;
                    s_cid[slot] = id;
                }
            }
        });
        __syncthreads();
        n_lds = s_n < (uint32_t)SAMPLE_CAP ? s_n : (uint32_t)SAMPLE_CAP;
        in_lds = true;
    };

    // radix selection among the keys >= floor_key: by count (the target-th largest) or by weight (the largest key whose
    // weights from the top reach top_p of all).  Returns false when a count selection has nothing to cut.
    auto select = [&](bool weighted, uint32_t floor_key, u64 target, float top_p, uint32_t &out_key) -> bool {
        uint32_t prefix = 0;
        for (int level = 0; level < 3; ++level) {
            const int shift = level == 0 ? 21 : level == 1 ? 10 : 0;
            const int nbits = level == 2 ? 10 : 11;
            const int nbins = 1 << nbits;
            for (int b = tid; b < nbins; b += SAMPLE_THREADS) {
                s_cnt[b] = 0;
                s_wq[b] = 0;
            }
            if (tid == 0) {
                s_pick.bin = 0;
                s_pick.n_ge = 0;
                s_pick.above = 0;
                s_pick.target = 1;
                s_pick.nocut = 0;
            }
            __syncthreads();
            for_each([&](uint32_t key, int32_t) {
                if (key < floor_key) return;
                if (level > 0 && (key >> (shift + nbits)) != prefix) return;
                const uint32_t digit = (key >> shift) & (uint32_t)(nbins - 1);
                atomicAdd(&s_cnt[digit], 1u);
                if (weighted) atomicAdd(&s_wq[digit], weight(key));
            });
            __syncthreads();
            find_bin(nbins, weighted, level == 0, target, top_p);
            const Pick pick = s_pick;
            __syncthreads();   // s_pick and the histograms are rewritten by the next level
            if (pick.nocut) return false;
            target = pick.target - pick.above;
            prefix = (prefix << nbits) | pick.bin;
            if (level == 0 && !in_lds && pick.n_ge <= (uint32_t)SAMPLE_CAP) {
                const uint32_t low = pick.bin << 21;
                compact(low > floor_key ? low : floor_key);
            }
        }
        out_key = prefix;
        return true;
    };

    // ---- the cuts ----
    uint32_t thr = 0;   // the lowest key kept so far (min-p apart: it is in for_each)
    const int top_k = p.top_k[r];
    if (top_k > 0 && (int64_t)top_k < vocab) {
        uint32_t key_k;
        if (select(false, 0u, (u64)top_k, 1.f, key_k)) thr = key_k;
    }
    const float top_p = p.top_p[r];
    if (top_p < 1.f) {
        uint32_t key_p = thr;
        select(true, thr, 0, top_p, key_p);
        thr = key_p > thr ? key_p : thr;
    }

    // ---- the draw over the kept ids ----
    // Pruning, exact: an id is left out of the maximum only when an upper bound of its key lies below a key some kept id
    // has -- then it can neither win nor tie, so the token does not depend on when a thread saw which bound.  The bounds:
    // the Gumbel term is below 17.4 (u <= 1 - 2^-25) before Philox has run, gumbel_bound() after; the key to beat is the
    // thread's own best or s_best, the workgroup's.  And below SAMPLE_SKIP no id can beat the maximum's own key, which is
    // at least -ln(-ln 2^-25) > -2.9.  A pruned id is still counted as kept.
    float gv = 0.f;
    int gid = -1;
    uint32_t kept = 0, low = 0xFFFFFFFFu;
    for_each([&](uint32_t key, int32_t id) {
        if (key < thr) return;
        ++kept;
        low = key < low ? key : low;
        const float a = (kfloat(key) - m) / T;
        if (a < SAMPLE_SKIP) return;
        const int shared = s_best;
        const int own = gid >= 0 ? fint(gv) : shared;
        const int beat = own > shared ? own : shared;
        if (fint(a + 17.4f) < beat) return;
        const uint32_t x0 = philox_x0((uint32_t)id, p.step, p.stream[r], 0u, p.seed_lo, p.seed_hi);
        if (fint(a + gumbel_bound(x0)) < beat) return;
        const float g = a + gumbel(x0);
        if (better(g, id, gv, gid)) {
            gv = g;
            gid = id;
            if (fint(g) > shared) atomicMax(&s_best, fint(g));
        }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(gv, o);
        const int oi = __shfl_xor(gid, o);
        const uint32_t oc = __shfl_xor(kept, o);
        const uint32_t ok = __shfl_xor(low, o);
        if (oi >= 0 && better(ov, oi, gv, gid)) {
            gv = ov;
            gid = oi;
        }
        kept += oc;
        low = ok < low ? ok : low;
    }
    if (lane == 0) {
        s_v[wave] = gv;
        s_i[wave] = gid;
        s_c[wave] = kept;
        s_k[wave] = low;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < SAMPLE_WAVES; ++k) {
            if (s_i[k] >= 0 && better(s_v[k], s_i[k], gv, gid)) {
                gv = s_v[k];
                gid = s_i[k];
            }
            kept += s_c[k];
            low = s_k[k] < low ? s_k[k] : low;
        }
        p.token[r] = gid;
        if (p.kept) p.kept[r] = (int32_t)kept;
        if (p.cut) p.cut[r] = kfloat(low);
    }
}

struct AdvanceParams {
    const int32_t *tok_offsets;
    const uint8_t *tok_bytes;
    const uint8_t *tok_kind;
    int64_t vocab;
    const uint8_t *class_of;
    const uint16_t *trans;
    int n_states, n_classes;
    int32_t *state;
    const int32_t *token;
    int n_rows;
};

// one lane per row: the walk of grammar_argmax_kernel for the one chosen token
__global__ __launch_bounds__(64) void grammar_advance_kernel(const AdvanceParams p) {
    const int r = threadIdx.x;
    if (r >= p.n_rows) return;
    const int32_t t = p.token[r];
    const int s0 = p.state[r];
    if (t < 0 || (int64_t)t >= p.vocab || s0 < 0 || s0 >= p.n_states) return;
    if (p.tok_kind[t] != 0) return;   // a stop token leaves the state; a token that is never allowed moves nothing
    const int32_t b0 = p.tok_offsets[t], b1 = p.tok_offsets[t + 1];
    int s = b1 > b0 ? s0 : -1;
    for (int32_t b = b0; b < b1 && s >= 0; ++b) {
        const int c = p.class_of[p.tok_bytes[b]];
        const int nxt = c < p.n_classes ? (int)p.trans[s * p.n_classes + c] : p.n_states;
        s = nxt < p.n_states ? nxt : -1;   // 0xFFFF, the dead state, is >= n_states
    }
    if (s >= 0) p.state[r] = s;   // a walk that dies (a token the state does not allow) leaves the state too
}

}  // namespace

extern "C" {

int crag_enc_sample(const float *logits, int64_t vocab, const uint32_t *allowed_bits, const float *h_temperature,
                    const int32_t *h_top_k, const float *h_top_p, const float *h_min_p_cut, const uint32_t *h_stream,
                    uint64_t seed, uint32_t step, int32_t *token, int32_t *kept, float *cut, int n_rows, void *stream) {
    if (!logits || !h_temperature || !h_top_k || !h_top_p || !h_min_p_cut || !h_stream || !token)
        return efail("sample: NULL pointer");
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS)
        return efail("sample: n_rows must be in 1..%d (got %d)", CRAG_DECODE_MAX_SEQS, n_rows);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("sample: vocab must be in 1..2^31 - 1");
    if (((uintptr_t)logits | (uintptr_t)allowed_bits | (uintptr_t)token | (uintptr_t)kept | (uintptr_t)cut) & 3)
        return efail("sample: logits, allowed_bits, token, kept and cut must be 4-byte aligned");
    SampleParams p;
    for (int r = 0; r < CRAG_DECODE_MAX_SEQS; ++r) {
        const int s = r < n_rows ? r : 0;   // the unused entries repeat row 0: no workgroup reads them
        const float T = h_temperature[s], tp = h_top_p[s], mc = h_min_p_cut[s];
        if (r < n_rows) {
            if (!(T == 0.f || (T >= CRAG_SAMPLE_MIN_TEMPERATURE && T <= CRAG_SAMPLE_MAX_TEMPERATURE)))
                return efail("sample: temperature must be 0 or in %g..%g (row %d: %g)", (double)CRAG_SAMPLE_MIN_TEMPERATURE,
                             (double)CRAG_SAMPLE_MAX_TEMPERATURE, r, (double)T);
            if (h_top_k[s] < 0 || (int64_t)h_top_k[s] > vocab)
                return efail("sample: top_k must be in 0..vocab (row %d: %d)", r, h_top_k[s]);
            if (!(tp > 0.f && tp <= 1.f)) return efail("sample: top_p must be in (0, 1] (row %d: %g)", r, (double)tp);
            if (!(mc <= 0.f)) return efail("sample: min_p_cut must be <= 0, -inf for none (row %d: %g)", r, (double)mc);
        }
        p.temperature[r] = T;
        p.top_k[r] = h_top_k[s];
        p.top_p[r] = tp;
        p.min_p_cut[r] = mc;
        p.stream[r] = h_stream[s];
    }
    p.logits = logits;
    p.vocab = vocab;
    p.allowed_bits = allowed_bits;
    p.n_words = (vocab + 31) / 32;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.step = step;
    int width = 0;   // bits of vocab: vocab weights of at most `scale` each sum below 2^62
    while (((int64_t)1 << width) <= vocab) ++width;
    p.scale = ldexp(1.0, 62 - width < 40 ? 62 - width : 40);
    p.token = token;
    p.kept = kept;
    p.cut = cut;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)n_rows), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, p);
    return hip_ok("sample");
}

int crag_enc_grammar_advance(const int32_t *tok_offsets, const uint8_t *tok_bytes, const uint8_t *tok_kind, int64_t vocab,
                             const uint8_t *class_of, const uint16_t *trans, int n_states, int n_classes, int32_t *state,
                             const int32_t *token, int n_rows, void *stream) {
    if (!tok_offsets || !tok_bytes || !tok_kind || !class_of || !trans || !state || !token)
        return efail("grammar_advance: NULL pointer");
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS)
        return efail("grammar_advance: n_rows must be in 1..%d (got %d)", CRAG_DECODE_MAX_SEQS, n_rows);
    if (n_states < 1 || n_states > CRAG_GRAMMAR_MAX_STATES)
        return efail("grammar_advance: n_states must be in 1..%d (got %d)", CRAG_GRAMMAR_MAX_STATES, n_states);
    if (n_classes < 1 || n_classes > CRAG_GRAMMAR_MAX_CLASSES)
        return efail("grammar_advance: n_classes must be in 1..%d (got %d)", CRAG_GRAMMAR_MAX_CLASSES, n_classes);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("grammar_advance: vocab must be in 1..2^31 - 1");
    if ((((uintptr_t)tok_offsets | (uintptr_t)state | (uintptr_t)token) & 3) || ((uintptr_t)trans & 1))
        return efail("grammar_advance: tok_offsets, state and token must be 4-byte aligned, trans 2-byte");
    AdvanceParams p;
    p.tok_offsets = tok_offsets;
    p.tok_bytes = tok_bytes;
    p.tok_kind = tok_kind;
    p.vocab = vocab;
    p.class_of = class_of;
    p.trans = trans;
    p.n_states = n_states;
    p.n_classes = n_classes;
    p.state = state;
    p.token = token;
    p.n_rows = n_rows;
    hipLaunchKernelGGL(grammar_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    return hip_ok("grammar_advance");
}

}  // extern "C"
