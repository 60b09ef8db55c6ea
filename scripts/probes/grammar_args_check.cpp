// grammar_args_check.cpp -- the argument checks of crag_enc_grammar_argmax under the host sanitizers, on the CPU.  A
// stand-alone program in the style of decode_args_check.cpp: it compiles the unit's host code with AddressSanitizer and
// UBSan and walks every refusal of the entry (each returns before the first HIP call, so no GPU is needed or touched).
// Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_grammar.hip ../../scripts/probes/grammar_args_check.cpp -o /tmp/grammar_args_check && /tmp/grammar_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/crag_dense.h"
#include "../../include/crag_encoder.h"

static char g_error[512];
extern "C" void crag_set_error_(const char *msg) {   // crag_api.hip's, which this program does not link
    strncpy(g_error, msg, sizeof(g_error) - 1);
}

struct Args {
    const void *logits, *offsets, *bytes, *kind, *class_of, *trans, *accept;
    void *state, *token, *bits = nullptr;
    int64_t vocab = 151936;
    int n_states = 280, n_classes = 44, n_rows = 8;
};

static int call(const Args &a) {
    g_error[0] = 0;
    return crag_enc_grammar_argmax((const float *)a.logits, a.vocab, (const int32_t *)a.offsets, (const uint8_t *)a.bytes,
                                   (const uint8_t *)a.kind, (const uint8_t *)a.class_of, (const uint16_t *)a.trans,
                                   (const uint8_t *)a.accept, a.n_states, a.n_classes, (int32_t *)a.state, (int32_t *)a.token,
                                   (uint32_t *)a.bits, a.n_rows, nullptr);
}

int main() {
    alignas(16) static uint64_t some[64];   // stands for device memory: a refusal comes before any use
    int failures = 0, cases = 0;
    auto expect = [&](const char *what, int rc, const char *tag) {
        ++cases;
        if (rc != CRAG_EINVAL || !strstr(g_error, "grammar_argmax") || !strstr(g_error, tag)) {
            printf("FAIL %s: returned %d (%s), expected %d with \"%s\"\n", what, rc, g_error, CRAG_EINVAL, tag);
            ++failures;
        }
    };
    Args ok;
    ok.logits = ok.offsets = ok.bytes = ok.kind = ok.class_of = ok.trans = ok.accept = some;
    ok.state = ok.token = some;
    Args a;
    a = ok, a.logits = nullptr, expect("NULL logits", call(a), "NULL");
    a = ok, a.offsets = nullptr, expect("NULL tok_offsets", call(a), "NULL");
    a = ok, a.bytes = nullptr, expect("NULL tok_bytes", call(a), "NULL");
    a = ok, a.kind = nullptr, expect("NULL tok_kind", call(a), "NULL");
    a = ok, a.class_of = nullptr, expect("NULL class_of", call(a), "NULL");
    a = ok, a.trans = nullptr, expect("NULL trans", call(a), "NULL");
    a = ok, a.accept = nullptr, expect("NULL accept", call(a), "NULL");
    a = ok, a.state = nullptr, expect("NULL state", call(a), "NULL");
    a = ok, a.token = nullptr, expect("NULL token", call(a), "NULL");
    a = ok, a.n_rows = 0, expect("0 rows", call(a), "n_rows");
    a = ok, a.n_rows = CRAG_DECODE_MAX_SEQS + 1, expect("9 rows", call(a), "n_rows");
    a = ok, a.n_rows = -1, expect("-1 rows", call(a), "n_rows");
    a = ok, a.n_states = 0, expect("0 states", call(a), "n_states");
    a = ok, a.n_states = CRAG_GRAMMAR_MAX_STATES + 1, expect("4097 states", call(a), "n_states");
    a = ok, a.n_classes = 0, expect("0 classes", call(a), "n_classes");
    a = ok, a.n_classes = CRAG_GRAMMAR_MAX_CLASSES + 1, expect("65 classes", call(a), "n_classes");
    a = ok, a.vocab = 0, expect("vocab 0", call(a), "vocab");
    a = ok, a.vocab = -7, expect("a negative vocab", call(a), "vocab");
    a = ok, a.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(a), "vocab");
    a = ok, a.trans = (const char *)a.trans + 1, expect("a misaligned trans", call(a), "aligned");
    a = ok, a.logits = (const char *)a.logits + 2, expect("misaligned logits", call(a), "aligned");
    a = ok, a.state = (char *)a.state + 1, expect("a misaligned state", call(a), "aligned");
    a = ok, a.bits = (char *)some + 2, expect("misaligned allowed_bits", call(a), "aligned");
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
