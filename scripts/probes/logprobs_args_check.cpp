// logprobs_args_check.cpp -- the argument checks of crag_enc_logprobs under the host sanitizers, on the CPU.  A
// stand-alone program in the style of sample_args_check.cpp and rows_args_check.cpp: it compiles the unit's host code with
// AddressSanitizer and UBSan and walks every refusal of the entry (each returns before the first HIP call, so no GPU is
// needed or touched).
// Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_logprobs.hip ../../scripts/probes/logprobs_args_check.cpp -o /tmp/logprobs_args_check && /tmp/logprobs_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/crag_dense.h"
#include "../../include/crag_encoder.h"

static char g_error[512];
extern "C" void crag_set_error_(const char *msg) {   // crag_api.hip's, which this program does not link
    strncpy(g_error, msg, sizeof(g_error) - 1);
}

alignas(16) static uint64_t some[64];   // stands for device memory: a refusal comes before any use

struct Args {
    const void *logits = some, *bits = some, *token = some;
    void *logprob = some, *lse_all = some, *lse_allowed = some, *rank = some, *top_id = some, *top_logprob = some;
    int64_t vocab = 151936;
    int n_top = 16, n_rows = 8;
};

static int call(const Args &a) {
    g_error[0] = 0;
    return crag_enc_logprobs((const float *)a.logits, a.vocab, (const uint32_t *)a.bits, (const int32_t *)a.token,
                             (float *)a.logprob, (float *)a.lse_all, (float *)a.lse_allowed, (int32_t *)a.rank,
                             (int32_t *)a.top_id, (float *)a.top_logprob, a.n_top, a.n_rows, nullptr);
}

int main() {
    int failures = 0, cases = 0;
    auto expect = [&](const char *what, int rc, const char *tag) {
        ++cases;
        if (rc != CRAG_EINVAL || !strstr(g_error, "logprobs") || !strstr(g_error, tag)) {
            printf("FAIL %s: returned %d (%s), expected %d with \"%s\"\n", what, rc, g_error, CRAG_EINVAL, tag);
            ++failures;
        }
    };
    const Args ok;
    Args a;
    a = ok, a.logits = nullptr, expect("NULL logits", call(a), "NULL");
    a = ok, a.token = nullptr, expect("NULL token", call(a), "NULL");
    a = ok, a.logprob = nullptr, expect("NULL logprob", call(a), "NULL");
    a = ok, a.n_rows = 0, expect("0 rows", call(a), "n_rows");
    a = ok, a.n_rows = -1, expect("-1 rows", call(a), "n_rows");
    a = ok, a.n_rows = CRAG_DECODE_MAX_SEQS + 1, expect("9 rows", call(a), "n_rows");
    a = ok, a.vocab = 0, expect("vocab 0", call(a), "vocab");
    a = ok, a.vocab = -7, expect("a negative vocab", call(a), "vocab");
    a = ok, a.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(a), "vocab");
    a = ok, a.n_top = -1, expect("n_top -1", call(a), "n_top");
    a = ok, a.n_top = CRAG_LOGPROBS_MAX_TOP + 1, expect("n_top 17", call(a), "n_top");
    a = ok, a.vocab = 5, a.n_top = 6, expect("n_top above vocab", call(a), "n_top");
    a = ok, a.top_id = nullptr, expect("n_top > 0 without top_id", call(a), "top_id");
    a = ok, a.top_logprob = nullptr, expect("n_top > 0 without top_logprob", call(a), "top_logprob");
    a = ok, a.logits = (const char *)some + 2, expect("misaligned logits", call(a), "aligned");
    a = ok, a.bits = (const char *)some + 1, expect("misaligned allowed_bits", call(a), "aligned");
    a = ok, a.token = (const char *)some + 2, expect("a misaligned token", call(a), "aligned");
    a = ok, a.logprob = (char *)some + 3, expect("a misaligned logprob", call(a), "aligned");
    a = ok, a.lse_all = (char *)some + 2, expect("a misaligned lse_all", call(a), "aligned");
    a = ok, a.lse_allowed = (char *)some + 1, expect("a misaligned lse_allowed", call(a), "aligned");
    a = ok, a.rank = (char *)some + 2, expect("a misaligned rank", call(a), "aligned");
    a = ok, a.top_id = (char *)some + 2, expect("a misaligned top_id", call(a), "aligned");
    a = ok, a.top_logprob = (char *)some + 3, expect("a misaligned top_logprob", call(a), "aligned");
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
