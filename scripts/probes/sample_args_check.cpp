// sample_args_check.cpp -- the argument checks of crag_enc_sample and crag_enc_grammar_advance under the host
// sanitizers, on the CPU.  A stand-alone program in the style of grammar_args_check.cpp: it compiles the unit's host code
// with AddressSanitizer and UBSan and walks every refusal of the two entries (each returns before the first HIP call, so
// no GPU is needed or touched).  The per-row arrays are exactly n_rows long, so a read beyond them is an ASan report.
// Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_sample.hip ../../scripts/probes/sample_args_check.cpp -o /tmp/sample_args_check && /tmp/sample_args_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/crag_dense.h"
#include "../../include/crag_encoder.h"

static char g_error[512];
extern "C" void crag_set_error_(const char *msg) {   // crag_api.hip's, which this program does not link
    strncpy(g_error, msg, sizeof(g_error) - 1);
}

alignas(16) static uint64_t some[64];   // stands for device memory: a refusal comes before any use

struct Sample {
    const void *logits = some, *bits = nullptr;
    void *token = some, *kept = nullptr, *cut = nullptr;
    int64_t vocab = 151936;
    int n_rows = 3;
    std::vector<float> t{1.f, 0.f, 0.7f}, p{1.f, 1.f, 0.9f}, m{-INFINITY, 0.f, -2.1f};
    std::vector<int32_t> k{0, 5, 151936};
    std::vector<uint32_t> s{0, 1, 2};
    bool null_t = false, null_k = false, null_p = false, null_m = false, null_s = false;
};

static int call(const Sample &a) {
    g_error[0] = 0;
    return crag_enc_sample((const float *)a.logits, a.vocab, (const uint32_t *)a.bits, a.null_t ? nullptr : a.t.data(),
                           a.null_k ? nullptr : a.k.data(), a.null_p ? nullptr : a.p.data(), a.null_m ? nullptr : a.m.data(),
                           a.null_s ? nullptr : a.s.data(), 0x123456789abcdef0ull, 7u, (int32_t *)a.token, (int32_t *)a.kept,
                           (float *)a.cut, a.n_rows, nullptr);
}

struct Advance {
    const void *offsets = some, *bytes = some, *kind = some, *class_of = some, *trans = some, *token = some;
    void *state = some;
    int64_t vocab = 151936;
    int n_states = 280, n_classes = 44, n_rows = 8;
};

static int call(const Advance &a) {
    g_error[0] = 0;
    return crag_enc_grammar_advance((const int32_t *)a.offsets, (const uint8_t *)a.bytes, (const uint8_t *)a.kind, a.vocab,
                                    (const uint8_t *)a.class_of, (const uint16_t *)a.trans, a.n_states, a.n_classes,
                                    (int32_t *)a.state, (const int32_t *)a.token, a.n_rows, nullptr);
}

int main() {
    int failures = 0, cases = 0;
    const char *entry = "sample";
    auto expect = [&](const char *what, int rc, const char *tag) {
        ++cases;
        if (rc != CRAG_EINVAL || !strstr(g_error, entry) || !strstr(g_error, tag)) {
            printf("FAIL %s: returned %d (%s), expected %d with \"%s\"\n", what, rc, g_error, CRAG_EINVAL, tag);
            ++failures;
        }
    };
    const Sample ok;
    Sample a;
    a = ok, a.logits = nullptr, expect("NULL logits", call(a), "NULL");
    a = ok, a.token = nullptr, expect("NULL token", call(a), "NULL");
    a = ok, a.null_t = true, expect("NULL temperature", call(a), "NULL");
    a = ok, a.null_k = true, expect("NULL top_k", call(a), "NULL");
    a = ok, a.null_p = true, expect("NULL top_p", call(a), "NULL");
    a = ok, a.null_m = true, expect("NULL min_p_cut", call(a), "NULL");
    a = ok, a.null_s = true, expect("NULL stream", call(a), "NULL");
    a = ok, a.n_rows = 0, expect("0 rows", call(a), "n_rows");
    a = ok, a.n_rows = -1, expect("-1 rows", call(a), "n_rows");
    a = ok, a.n_rows = CRAG_DECODE_MAX_SEQS + 1, expect("9 rows", call(a), "n_rows");
    a = ok, a.vocab = 0, expect("vocab 0", call(a), "vocab");
    a = ok, a.vocab = -7, expect("a negative vocab", call(a), "vocab");
    a = ok, a.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(a), "vocab");
    a = ok, a.t[2] = -0.5f, expect("a negative temperature", call(a), "temperature");
    a = ok, a.t[0] = 0.009f, expect("a temperature below the floor", call(a), "temperature");
    a = ok, a.t[1] = 100.5f, expect("a temperature above the cap", call(a), "temperature");
    a = ok, a.t[2] = NAN, expect("a NaN temperature", call(a), "temperature");
    a = ok, a.t[2] = INFINITY, expect("an infinite temperature", call(a), "temperature");
    a = ok, a.k[1] = -1, expect("a negative top_k", call(a), "top_k");
    a = ok, a.k[2] = 151937, expect("top_k beyond vocab", call(a), "top_k");
    a = ok, a.p[0] = 0.f, expect("top_p 0", call(a), "top_p");
    a = ok, a.p[2] = 1.0001f, expect("top_p above 1", call(a), "top_p");
    a = ok, a.p[1] = NAN, expect("a NaN top_p", call(a), "top_p");
    a = ok, a.m[0] = 0.25f, expect("a positive min_p_cut", call(a), "min_p_cut");
    a = ok, a.m[2] = NAN, expect("a NaN min_p_cut", call(a), "min_p_cut");
    a = ok, a.logits = (const char *)some + 2, expect("misaligned logits", call(a), "aligned");
    a = ok, a.token = (char *)some + 1, expect("a misaligned token", call(a), "aligned");
    a = ok, a.bits = (const char *)some + 2, expect("misaligned allowed_bits", call(a), "aligned");
    a = ok, a.kept = (char *)some + 3, expect("a misaligned kept", call(a), "aligned");
    a = ok, a.cut = (char *)some + 2, expect("a misaligned cut", call(a), "aligned");

    entry = "grammar_advance";
    const Advance fine;
    Advance b;
    b = fine, b.offsets = nullptr, expect("NULL tok_offsets", call(b), "NULL");
    b = fine, b.bytes = nullptr, expect("NULL tok_bytes", call(b), "NULL");
    b = fine, b.kind = nullptr, expect("NULL tok_kind", call(b), "NULL");
    b = fine, b.class_of = nullptr, expect("NULL class_of", call(b), "NULL");
    b = fine, b.trans = nullptr, expect("NULL trans", call(b), "NULL");
    b = fine, b.state = nullptr, expect("NULL state", call(b), "NULL");
    b = fine, b.token = nullptr, expect("NULL token", call(b), "NULL");
    b = fine, b.n_rows = 0, expect("0 rows", call(b), "n_rows");
    b = fine, b.n_rows = CRAG_DECODE_MAX_SEQS + 1, expect("9 rows", call(b), "n_rows");
    b = fine, b.n_states = 0, expect("0 states", call(b), "n_states");
    b = fine, b.n_states = CRAG_GRAMMAR_MAX_STATES + 1, expect("4097 states", call(b), "n_states");
    b = fine, b.n_classes = 0, expect("0 classes", call(b), "n_classes");
    b = fine, b.n_classes = CRAG_GRAMMAR_MAX_CLASSES + 1, expect("65 classes", call(b), "n_classes");
    b = fine, b.vocab = 0, expect("vocab 0", call(b), "vocab");
    b = fine, b.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(b), "vocab");
    b = fine, b.trans = (const char *)some + 1, expect("a misaligned trans", call(b), "aligned");
    b = fine, b.offsets = (const char *)some + 2, expect("misaligned tok_offsets", call(b), "aligned");
    b = fine, b.state = (char *)some + 1, expect("a misaligned state", call(b), "aligned");
    b = fine, b.token = (const char *)some + 2, expect("a misaligned token", call(b), "aligned");
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
