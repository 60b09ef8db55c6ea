// adjust_args_check.cpp -- the argument checks of crag_enc_adjust_logits under the host sanitizers, on the CPU.  A
// stand-alone program in the style of logprobs_args_check.cpp: it compiles the unit's host code with AddressSanitizer and
// UBSan and walks every refusal of the entry.  Each returns before anything is launched; the bias ids, which the entry
// reads to check their order, are plain host memory here and are read in place, so no GPU is needed or touched.
// Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_penalty.hip ../../scripts/probes/adjust_args_check.cpp -o /tmp/adjust_args_check && /tmp/adjust_args_check
#include <math.h>
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
    const void *logits = some, *history = some, *exempt = some, *bias_ids = nullptr, *bias_values = some;
    void *out = some, *token = some, *workspace = some;
    int64_t vocab = 151936, stride = 8192, workspace_bytes = 8 * (151936 + 4) * 4;
    int n_history_rows = 8, n_rows = 8;
    int32_t row[9] = {0, 1, 2, 3, 4, 5, 6, 7, 0}, prompt[9] = {0, 1, 100, 100, 100, 100, 100, 8192, 0},
            total[9] = {0, 1, 100, 101, 4096, 8192, 8192, 8192, 0}, ngram[9] = {0, 2, 3, 8, 0, 0, 0, 0, 0},
            offsets[9] = {0, 0, 1, 3, 3, 3, 3, 3, 259};
    float repetition[9] = {1.f, 0.1f, 10.f, 1.3f, 1.f, 1.f, 1.f, 1.f, 1.f}, frequency[9] = {0.f, 2.f, -2.f, 0.f},
          presence[9] = {0.f, -2.f, 2.f, 0.f};
    int null_host = -1;   // which of the eight host arrays is passed as NULL (none)
};

static int32_t ids[259];

static int call(const Args &a) {
    g_error[0] = 0;
    auto host = [&](int which, auto *p) { return a.null_host == which ? nullptr : p; };
    return crag_enc_adjust_logits((const float *)a.logits, (float *)a.out, a.vocab, (const int32_t *)a.history, a.stride,
                                  a.n_history_rows, host(0, a.row), host(1, a.prompt), host(2, a.total),
                                  host(3, a.repetition), host(4, a.frequency), host(5, a.presence), host(6, a.ngram),
                                  (const uint32_t *)a.exempt, a.bias_ids ? (const int32_t *)a.bias_ids : ids,
                                  (const float *)a.bias_values, host(7, a.offsets),
                                  (int32_t *)a.token, a.workspace, a.workspace_bytes, a.n_rows, nullptr);
}

int main() {
    int failures = 0, cases = 0;
    auto expect_code = [&](const char *what, int rc, int code, const char *tag) {
        ++cases;
        if (rc != code || !strstr(g_error, "adjust_logits") || !strstr(g_error, tag)) {
            printf("FAIL %s: returned %d (%s), expected %d with \"%s\"\n", what, rc, g_error, code, tag);
            ++failures;
        }
    };
    auto expect = [&](const char *what, int rc, const char *tag) { expect_code(what, rc, CRAG_EINVAL, tag); };
    for (int i = 0; i < 259; ++i) ids[i] = i;
    ids[1] = 7, ids[2] = 7;   // row 2's slice (entries 1, 2) does not ascend: the LAST check, behind every other one
    const Args ok;            // every other argument of `ok` is valid, so each case below is refused for its own reason
    Args a;
    a = ok, expect("bias ids that do not ascend", call(a), "ascending");
    ids[2] = 151936, expect("a bias id outside the vocabulary", call(a), "ascending");
    ids[2] = 8;
    a = ok, a.logits = nullptr, expect("NULL logits", call(a), "NULL");
    a = ok, a.out = nullptr, expect("NULL out", call(a), "NULL");
    a = ok, a.history = nullptr, expect("NULL history", call(a), "NULL");
    a = ok, a.token = nullptr, expect("NULL token", call(a), "NULL");
    a = ok, a.workspace = nullptr, expect("NULL workspace", call(a), "NULL");
    a = ok, a.null_host = 0, expect("NULL h_history_row", call(a), "NULL");
    a = ok, a.null_host = 1, expect("NULL h_prompt_len", call(a), "NULL");
    a = ok, a.null_host = 2, expect("NULL h_total_len", call(a), "NULL");
    a = ok, a.null_host = 3, expect("NULL h_repetition", call(a), "NULL");
    a = ok, a.null_host = 4, expect("NULL h_frequency", call(a), "NULL");
    a = ok, a.null_host = 5, expect("NULL h_presence", call(a), "NULL");
    a = ok, a.null_host = 6, expect("NULL h_ngram", call(a), "NULL");
    a = ok, a.bias_values = nullptr, expect("bias ids without values", call(a), "together");
    a = ok, a.null_host = 7, expect("bias ids without offsets", call(a), "together");
    a = ok, a.n_rows = 0, expect("0 rows", call(a), "n_rows");
    a = ok, a.n_rows = -1, expect("-1 rows", call(a), "n_rows");
    a = ok, a.n_rows = CRAG_DECODE_MAX_SEQS + 1, expect("9 rows", call(a), "n_rows");
    a = ok, a.vocab = 0, expect("vocab 0", call(a), "vocab");
    a = ok, a.vocab = -7, expect("a negative vocab", call(a), "vocab");
    a = ok, a.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(a), "vocab");
    a = ok, a.stride = 0, expect("a log without columns", call(a), "history");
    a = ok, a.n_history_rows = 0, expect("a log without rows", call(a), "history");
    a = ok, a.row[3] = 8, expect("a history row behind the log", call(a), "history row");
    a = ok, a.row[3] = -1, expect("a negative history row", call(a), "history row");
    a = ok, a.total[4] = 8193, expect("total_len above the stride", call(a), "total_len");
    a = ok, a.total[4] = -1, a.prompt[4] = -1, expect("a negative total_len", call(a), "total_len");
    a = ok, a.prompt[3] = 102, expect("prompt_len above total_len", call(a), "prompt_len");
    a = ok, a.prompt[3] = -1, expect("a negative prompt_len", call(a), "prompt_len");
    a = ok, a.repetition[5] = 0.05f, expect("a repetition penalty below 0.1", call(a), "repetition");
    a = ok, a.repetition[5] = 10.5f, expect("a repetition penalty above 10", call(a), "repetition");
    a = ok, a.repetition[5] = NAN, expect("a NaN repetition penalty", call(a), "repetition");
    a = ok, a.frequency[5] = 2.5f, expect("a frequency penalty above 2", call(a), "frequency");
    a = ok, a.frequency[5] = -2.5f, expect("a frequency penalty below -2", call(a), "frequency");
    a = ok, a.frequency[5] = NAN, expect("a NaN frequency penalty", call(a), "frequency");
    a = ok, a.presence[5] = 2.5f, expect("a presence penalty above 2", call(a), "presence");
    a = ok, a.presence[5] = -INFINITY, expect("a presence penalty of -inf", call(a), "presence");
    a = ok, a.ngram[6] = 1, expect("an n-gram size of 1", call(a), "no_repeat_ngram");
    a = ok, a.ngram[6] = 9, expect("an n-gram size of 9", call(a), "no_repeat_ngram");
    a = ok, a.ngram[6] = -2, expect("a negative n-gram size", call(a), "no_repeat_ngram");
    a = ok, a.offsets[0] = 1, expect("offsets that do not start at 0", call(a), "bias slice");
    a = ok, a.offsets[4] = 2, expect("offsets that fall", call(a), "bias slice");
    a = ok, a.offsets[3] = a.offsets[4] = a.offsets[5] = a.offsets[6] = a.offsets[7] = 2;   // row 7: 2..259
    expect("a bias slice of 257 entries", call(a), "bias slice");
    a = ok, a.logits = (const char *)some + 2, expect("misaligned logits", call(a), "aligned");
    a = ok, a.out = (char *)some + 1, expect("a misaligned out", call(a), "aligned");
    a = ok, a.history = (const char *)some + 2, expect("a misaligned history", call(a), "aligned");
    a = ok, a.exempt = (const char *)some + 3, expect("misaligned exempt_bits", call(a), "aligned");
    a = ok, a.bias_ids = (const char *)ids + 2, expect("misaligned bias_ids", call(a), "aligned");
    a = ok, a.bias_values = (const char *)some + 2, expect("misaligned bias_values", call(a), "aligned");
    a = ok, a.token = (char *)some + 2, expect("a misaligned token", call(a), "aligned");
    a = ok, a.workspace = (char *)some + 2, expect("a misaligned workspace", call(a), "aligned");
    a = ok, a.workspace_bytes -= 1, expect_code("a workspace one byte short", call(a), CRAG_E2BIG, "workspace");
    a = ok, a.workspace_bytes = 0, expect_code("no workspace bytes", call(a), CRAG_E2BIG, "workspace");
    ++cases;
    if (crag_enc_adjust_workspace_bytes(8, 151936) != (int64_t)8 * 151940 * 4 ||
        crag_enc_adjust_workspace_bytes(1, 33) != 40 * 4 ||
        crag_enc_adjust_workspace_bytes(0, 33) != 0 || crag_enc_adjust_workspace_bytes(9, 33) != 0 ||
        crag_enc_adjust_workspace_bytes(1, 0) != 0) {
        printf("FAIL crag_enc_adjust_workspace_bytes\n");
        ++failures;
    }
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
