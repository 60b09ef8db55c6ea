// crag_rerank.hip — the operator a Qwen3-Reranker forward adds after the decoder layers (gfx950).
// C ABI: include/crag_encoder.h.
//
//   crag_enc_rerank_head         residual add + final RMSNorm of the pooled rows, then the "yes" / "no" rows of lm_head
//                                and the model card's score, exp(log_softmax([no, yes])[1]).
//
// The reranker's other operator, shared-prefix attention (crag_enc_attention_prefixed), is the PREFIXED instantiation
// of the encoder's attention kernel and lives with it in crag_attention.hip.

#include <math.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// rerank head: one workgroup per pair
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_THREADS = 256;

__global__ __launch_bounds__(HEAD_THREADS) void rerank_head_kernel(const u16 *hs, const u16 *delta, const u16 *w,
                                                                   const int64_t *rows, const u16 *lm, float *out,
                                                                   int hidden, float eps) {
    __shared__ float sh[HEAD_THREADS / 64];
    __shared__ float row[8192];
    const int b = blockIdx.x;
    const int64_t r = rows[b];
    const u16 *x = hs + r * hidden;
    const u16 *dl = delta ? delta + r * hidden : nullptr;
    float ss = 0.f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = dl ? bf2f(f2bf(bf2f(x[i]) + bf2f(dl[i]))) : bf2f(x[i]);
        row[i] = v;
        ss += v * v;
    }
    ss = block_sum(ss, sh);
    const float rstd = rsqrtf(ss / (float)hidden + eps);
    // the final norm's output in the model's bf16 (pool_normalize_kernel's roundings), then fp32 dots with the two rows
    float dy = 0.f, dn = 0.f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = bf2f(f2bf(bf2f(w[i]) * bf2f(f2bf(row[i] * rstd))));
        dy += v * bf2f(lm[i]);
        dn += v * bf2f(lm[hidden + i]);
    }
    dy = block_sum(dy, sh);
    dn = block_sum(dn, sh);
    if (threadIdx.x == 0) {
        // exp(log_softmax([no, yes])[1]) = 1 / (1 + exp(no - yes)), in the form that cannot overflow
        const float d = dy - dn;
        const float e = expf(-fabsf(d));
        const float score = d >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        out[3 * (int64_t)b + 0] = dy;
        out[3 * (int64_t)b + 1] = dn;
        out[3 * (int64_t)b + 2] = score;
    }
}

}  // namespace

extern "C" {

int crag_enc_rerank_head(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                         const int64_t *rows, const uint16_t *lm_rows, float *out, int n_pairs, int hidden, float eps,
                         void *stream) {
    if (!hidden_states || !final_norm_w || !rows || !lm_rows || !out) return efail("rerank_head: NULL pointer");
    if (hidden <= 0 || hidden > 8192) return efail("rerank_head: hidden must be in 1..8192 (got %d)", hidden);
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(rerank_head_kernel, dim3((unsigned)n_pairs), dim3(HEAD_THREADS), 0, (hipStream_t)stream,
                       hidden_states, delta, final_norm_w, rows, lm_rows, out, hidden, eps);
    return hip_ok("rerank_head");
}

}  // extern "C"
