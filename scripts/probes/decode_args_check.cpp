// decode_args_check.cpp -- the argument checks of crag_enc_decode_attention and crag_enc_lm_head under the host
// sanitizers, on the CPU.  A stand-alone program: it compiles the unit's host code with AddressSanitizer and UBSan and
// walks every refusal of the two entries (each returns before the first HIP call, so no GPU is needed or touched).
// Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_decode.hip ../../scripts/probes/decode_args_check.cpp -o /tmp/decode_args_check && /tmp/decode_args_check
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

struct Attn {
    const void *qkv, *qw, *kw, *cs;
    int max_pos = 64;
    void *kc, *vc;
    int n_slots = 4, max_len = 32;
    std::vector<int32_t> slots{2, 0, 3}, lens{0, 31, 7};
    int n_seqs = 3, hq = 8, hkv = 2;
    void *work;
    int64_t work_bytes = 0;
    void *out;
};

static int call(const Attn &a) {
    g_error[0] = 0;
    return crag_enc_decode_attention((const uint16_t *)a.qkv, (const uint16_t *)a.qw, (const uint16_t *)a.kw, (const float *)a.cs,
                                     a.max_pos, (uint16_t *)a.kc, (uint16_t *)a.vc, a.n_slots, a.max_len,
                                     a.slots.empty() ? nullptr : a.slots.data(), a.lens.empty() ? nullptr : a.lens.data(),
                                     a.n_seqs, a.hq, a.hkv, 1e-6f, 0.088f, a.work, a.work_bytes, (uint16_t *)a.out, nullptr);
}

struct Head {
    const void *hs, *delta, *w, *lm;
    void *logits, *token;
    const void *banned = nullptr;
    int n_banned = 0, n_rows = 5, hidden = 2560;
    int64_t vocab = 4099;
};

static int call(const Head &h) {
    g_error[0] = 0;
    return crag_enc_lm_head((const uint16_t *)h.hs, (const uint16_t *)h.delta, (const uint16_t *)h.w, (const uint16_t *)h.lm,
                            (float *)h.logits, (int32_t *)h.token, (const int32_t *)h.banned, h.n_banned, h.n_rows, h.hidden,
                            h.vocab, 1e-6f, nullptr);
}

int main() {
    alignas(16) static uint64_t some[64];   // stands for device memory: a refusal comes before any use
    int failures = 0, cases = 0;
    auto expect = [&](const char *what, int rc, int code, const char *tag) {
        ++cases;
        if (rc != code || !strstr(g_error, tag)) {
            printf("FAIL %s: returned %d (%s), expected %d\n", what, rc, g_error, code);
            ++failures;
        }
    };
    Attn ok;
    ok.qkv = ok.qw = ok.kw = ok.cs = some;
    ok.kc = ok.vc = ok.work = ok.out = some;
    ok.work_bytes = crag_enc_decode_workspace_bytes(ok.n_seqs, ok.hq, ok.max_len);
    ++cases;
    if (ok.work_bytes != 3 * 8 * (128 * 2 + 128 * 4 + 2 * 4)) {   // one split at max_len 32
        printf("FAIL workspace bytes: %lld\n", (long long)ok.work_bytes);
        ++failures;
    }
    ++cases;
    if (crag_enc_decode_workspace_bytes(9, 8, 32) != 0 || crag_enc_decode_workspace_bytes(0, 8, 32) != 0) {
        printf("FAIL workspace bytes of a refused shape\n");
        ++failures;
    }
    const char *T = "decode_attention";
    Attn a;
    a = ok, a.lens[1] = 32, expect("len == max_len", call(a), CRAG_EINVAL, T);
    a = ok, a.lens[2] = 1 << 30, expect("a huge len", call(a), CRAG_EINVAL, T);
    a = ok, a.lens[0] = -1, expect("a negative len", call(a), CRAG_EINVAL, T);
    a = ok, a.max_pos = 31, expect("a position beyond the RoPE table", call(a), CRAG_EINVAL, T);
    a = ok, a.n_seqs = 9, a.slots.resize(9), a.lens.resize(9), expect("n_seqs 9", call(a), CRAG_EINVAL, T);
    a = ok, a.n_seqs = 0, expect("n_seqs 0", call(a), CRAG_EINVAL, T);
    a = ok, a.slots[2] = 2, expect("a repeated slot", call(a), CRAG_EINVAL, T);
    a = ok, a.slots[1] = 4, expect("slot == n_slots", call(a), CRAG_EINVAL, T);
    a = ok, a.slots[1] = -1, expect("a negative slot", call(a), CRAG_EINVAL, T);
    a = ok, a.hq = 6, expect("hq / hkv 3", call(a), CRAG_EINVAL, T);
    a = ok, a.hq = 2, expect("hq / hkv 1", call(a), CRAG_EINVAL, T);
    a = ok, a.hkv = 0, expect("hkv 0", call(a), CRAG_EINVAL, T);
    a = ok, a.max_len = 0, expect("max_len 0", call(a), CRAG_EINVAL, T);
    a = ok, a.n_slots = 0, expect("n_slots 0", call(a), CRAG_EINVAL, T);
    a = ok, a.qkv = nullptr, expect("NULL qkv", call(a), CRAG_EINVAL, T);
    a = ok, a.qw = nullptr, expect("NULL q_norm", call(a), CRAG_EINVAL, T);
    a = ok, a.kw = nullptr, expect("NULL k_norm", call(a), CRAG_EINVAL, T);
    a = ok, a.cs = nullptr, expect("NULL cos_sin", call(a), CRAG_EINVAL, T);
    a = ok, a.kc = nullptr, expect("NULL k cache", call(a), CRAG_EINVAL, T);
    a = ok, a.vc = nullptr, expect("NULL v cache", call(a), CRAG_EINVAL, T);
    a = ok, a.out = nullptr, expect("NULL out", call(a), CRAG_EINVAL, T);
    a = ok, a.work = nullptr, expect("NULL workspace", call(a), CRAG_EINVAL, T);
    a = ok, a.slots.clear(), expect("NULL slots", call(a), CRAG_EINVAL, T);
    a = ok, a.lens.clear(), expect("NULL lengths", call(a), CRAG_EINVAL, T);
    a = ok, a.kc = (char *)a.kc + 8, expect("a misaligned cache", call(a), CRAG_EINVAL, T);
    a = ok, a.work_bytes -= 1, expect("the workspace one byte short", call(a), CRAG_E2BIG, T);

    const char *L = "lm_head";
    Head hk;
    hk.hs = hk.delta = hk.w = hk.lm = some;
    hk.logits = hk.token = some;
    Head h;
    h = hk, h.n_rows = 0, expect("0 rows", call(h), CRAG_EINVAL, L);
    h = hk, h.n_rows = 9, expect("9 rows", call(h), CRAG_EINVAL, L);
    h = hk, h.hidden = 2568, expect("hidden no multiple of 64", call(h), CRAG_EINVAL, L);
    h = hk, h.n_rows = 1, h.hidden = 32768, expect("one row beyond the LDS", call(h), CRAG_EINVAL, L);
    h = hk, h.hidden = 0, expect("hidden 0", call(h), CRAG_EINVAL, L);
    h = hk, h.n_rows = 8, h.hidden = 4096, expect("8 rows of 4096", call(h), CRAG_EINVAL, L);
    h = hk, h.vocab = 0, expect("vocab 0", call(h), CRAG_EINVAL, L);
    h = hk, h.vocab = (int64_t)1 << 31, expect("vocab 2^31", call(h), CRAG_EINVAL, L);
    h = hk, h.n_banned = 3, expect("banned ids without a list", call(h), CRAG_EINVAL, L);
    h = hk, h.banned = some, h.n_banned = 65, expect("65 banned ids", call(h), CRAG_EINVAL, L);
    h = hk, h.n_banned = -1, expect("a negative banned count", call(h), CRAG_EINVAL, L);
    h = hk, h.hs = nullptr, expect("NULL hidden states", call(h), CRAG_EINVAL, L);
    h = hk, h.w = nullptr, expect("NULL norm weight", call(h), CRAG_EINVAL, L);
    h = hk, h.lm = nullptr, expect("NULL lm_head", call(h), CRAG_EINVAL, L);
    h = hk, h.logits = nullptr, expect("NULL logits", call(h), CRAG_EINVAL, L);
    h = hk, h.token = nullptr, expect("NULL token", call(h), CRAG_EINVAL, L);
    h = hk, h.lm = (const char *)h.lm + 2, expect("a misaligned lm_head", call(h), CRAG_EINVAL, L);
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
