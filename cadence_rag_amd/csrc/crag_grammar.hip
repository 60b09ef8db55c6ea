// crag_grammar.hip — greedy selection under a byte automaton (gfx950).  C ABI: include/crag_encoder.h.
//
//   crag_enc_grammar_argmax   per row: the lowest id among the maxima of the logits over the tokens the row's automaton
//                             state allows, and the state behind the chosen token.  A token is allowed when it is a
//                             stop token in an accepting state, or an ordinary token whose bytes, walked from the
//                             row's state, never reach the dead state.
//
// One workgroup per row, as lm_argmax_kernel (crag_decode.hip): a thread walks its ids in ascending order, so the
// (value, id) merge of the threads (block_best, crag_enc_common.h) gives the lowest id among equal maxima.  class_of sits in LDS; the transition table
// too when it fits GRAMMAR_LDS_TRANS entries, otherwise it is read through the cache (two instantiations).  Without
// allowed_bits a thread walks only a token whose logit beats its own best so far; with allowed_bits every token is
// walked and a wave stores its 64 flags as two words (ballot; lanes 0 and 32 store).  Every store is a plain vector
// store; no atomics.  Every table index is checked against n_states / n_classes before it is used, so a malformed
// table refuses tokens, it does not read out of bounds.

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

constexpr int GRAMMAR_THREADS = 1024;
constexpr int GRAMMAR_WAVES = GRAMMAR_THREADS / 64;
constexpr int GRAMMAR_LDS_TRANS = 24576;   // uint16 entries: 48 KiB of the workgroup's LDS
constexpr int GRAMMAR_NONE = -1;           // a walk that died

struct GrammarParams {
    const float *logits;
    int64_t vocab;
    const int32_t *tok_offsets;
    const uint8_t *tok_bytes;
    const uint8_t *tok_kind;
    const uint8_t *class_of;
    const uint16_t *trans;
    const uint8_t *accept;
    int n_states, n_classes;
    int32_t *state;
    int32_t *token;
    uint32_t *allowed_bits;
    int64_t n_words;
};

template <bool BITS, bool TRANS_LDS>
__global__ __launch_bounds__(GRAMMAR_THREADS) void grammar_argmax_kernel(const GrammarParams p) {
    __shared__ uint8_t s_cls[256];
    __shared__ float sv[GRAMMAR_WAVES];
    __shared__ int si[GRAMMAR_WAVES];
    __shared__ int ss[GRAMMAR_WAVES];
    extern __shared__ __align__(16) unsigned char grammar_smem[];
    uint16_t *s_trans = reinterpret_cast<uint16_t *>(grammar_smem);
    const int tid = threadIdx.x, r = blockIdx.x;
    const int n_states = p.n_states, n_classes = p.n_classes;
    if (tid < 256) s_cls[tid] = p.class_of[tid];
    if (TRANS_LDS)
        for (int i = tid; i < n_states * n_classes; i += GRAMMAR_THREADS) s_trans[i] = p.trans[i];
    const int s0 = p.state[r];                       // read by every thread before the barrier, stored after the last one
    const bool live = s0 >= 0 && s0 < n_states;      // a state outside the table allows nothing
    const bool accepting = live && p.accept[s0] != 0;
    __syncthreads();
    const uint16_t *trans = TRANS_LDS ? s_trans : p.trans;
    const float *row = p.logits + (int64_t)r * p.vocab;
    float bv = 0.f;
    int bid = -1, bstate = s0;
    for (int64_t base = 0; base < p.vocab; base += GRAMMAR_THREADS) {   // uniform trip count: the ballot below needs every lane
        const int64_t i = base + tid;
        bool ok = false;
        if (live && i < p.vocab) {
            const float v = row[i];
            const bool cand = v == v && (bid < 0 || v > bv);   // NaN never; ascending ids: an equal value keeps the lower id
            if (BITS || cand) {
                const int kind = p.tok_kind[i];
                int end = s0;
                if (kind == 1) {
                    ok = accepting;
                } else if (kind == 0) {
                    const int32_t b0 = p.tok_offsets[i], b1 = p.tok_offsets[i + 1];
                    int s = b1 > b0 ? s0 : GRAMMAR_NONE;        // no bytes: never allowed
                    for (int32_t b = b0; b < b1 && s != GRAMMAR_NONE; ++b) {
                        const int c = s_cls[p.tok_bytes[b]];
                        const int nxt = c < n_classes ? (int)trans[s * n_classes + c] : n_states;
                        s = nxt < n_states ? nxt : GRAMMAR_NONE;   // 0xFFFF, the dead state, is >= n_states
                    }
                    ok = s != GRAMMAR_NONE;
                    end = s;
                }
                if (ok && cand) {
                    bv = v;
                    bid = (int)i;
                    bstate = end;
                }
            }
        }
        if (BITS) {
            const unsigned long long flags = __ballot(ok);
            const int lane = tid & 63;
            const int64_t word = (base + (tid - lane)) >> 5;   // the wave's 64 ids start at a multiple of 64
            if (lane == 0 && word < p.n_words) p.allowed_bits[(int64_t)r * p.n_words + word] = (uint32_t)flags;
            if (lane == 32 && word + 1 < p.n_words)
                p.allowed_bits[(int64_t)r * p.n_words + word + 1] = (uint32_t)(flags >> 32);
        }
    }
    const Best best = block_best<GRAMMAR_WAVES, true>(bv, bid, bstate, sv, si, ss);   // the end state travels with the winner
    if (tid == 0) {
        p.token[r] = best.id;
        if (best.id >= 0) p.state[r] = best.payload;   // nothing allowed: the state stays
    }
}

}  // namespace

extern "C" {

int crag_enc_grammar_argmax(const float *logits, int64_t vocab, const int32_t *tok_offsets, const uint8_t *tok_bytes,
                            const uint8_t *tok_kind, const uint8_t *class_of, const uint16_t *trans, const uint8_t *accept,
                            int n_states, int n_classes, int32_t *state, int32_t *token, uint32_t *allowed_bits, int n_rows,
                            void *stream) {
    if (!logits || !tok_offsets || !tok_bytes || !tok_kind || !class_of || !trans || !accept || !state || !token)
        return efail("grammar_argmax: NULL pointer");
    if (n_rows < 1 || n_rows > CRAG_DECODE_MAX_SEQS)
        return efail("grammar_argmax: n_rows must be in 1..%d (got %d)", CRAG_DECODE_MAX_SEQS, n_rows);
    if (n_states < 1 || n_states > CRAG_GRAMMAR_MAX_STATES)
        return efail("grammar_argmax: n_states must be in 1..%d (got %d)", CRAG_GRAMMAR_MAX_STATES, n_states);
    if (n_classes < 1 || n_classes > CRAG_GRAMMAR_MAX_CLASSES)
        return efail("grammar_argmax: n_classes must be in 1..%d (got %d)", CRAG_GRAMMAR_MAX_CLASSES, n_classes);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("grammar_argmax: vocab must be in 1..2^31 - 1");
    if ((((uintptr_t)logits | (uintptr_t)tok_offsets | (uintptr_t)state | (uintptr_t)token | (uintptr_t)allowed_bits) & 3) ||
        ((uintptr_t)trans & 1))
        return efail("grammar_argmax: logits, tok_offsets, state, token and allowed_bits must be 4-byte aligned, trans 2-byte");
    GrammarParams p;
    p.logits = logits;
    p.vocab = vocab;
    p.tok_offsets = tok_offsets;
    p.tok_bytes = tok_bytes;
    p.tok_kind = tok_kind;
    p.class_of = class_of;
    p.trans = trans;
    p.accept = accept;
    p.n_states = n_states;
    p.n_classes = n_classes;
    p.state = state;
    p.token = token;
    p.allowed_bits = allowed_bits;
    p.n_words = (vocab + 31) / 32;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_rows), block(GRAMMAR_THREADS);
    const int entries = n_states * n_classes;
    const bool in_lds = entries <= GRAMMAR_LDS_TRANS;
    const size_t smem = in_lds ? (size_t)entries * sizeof(uint16_t) : 0;
    if (allowed_bits) {
        if (in_lds)
            hipLaunchKernelGGL((grammar_argmax_kernel<true, true>), grid, block, smem, st, p);
        else
            hipLaunchKernelGGL((grammar_argmax_kernel<true, false>), grid, block, smem, st, p);
    } else {
        if (in_lds)
            hipLaunchKernelGGL((grammar_argmax_kernel<false, true>), grid, block, smem, st, p);
        else
            hipLaunchKernelGGL((grammar_argmax_kernel<false, false>), grid, block, smem, st, p);
    }
    return hip_ok("grammar_argmax");
}

}  // extern "C"
