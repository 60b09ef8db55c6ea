// rows_args_check.cpp -- the argument checks of crag_enc_decode_attention_rows under the host sanitizers, on the CPU.
// A stand-alone program: it compiles the unit's host code with AddressSanitizer and UBSan and walks every refusal of
// the entry -- those it shares with crag_enc_decode_attention_shared and those of the row counts (the entry returns
// before the first HIP call, so no GPU is needed or touched).  Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_decode.hip ../../scripts/probes/rows_args_check.cpp -o /tmp/rows_args_check && /tmp/rows_args_check
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
    int n_slots = 5, max_len = 32;
    // slot 2 is not forked and brings 2 rows; slot 0 shares 7 rows of slot 2 (in the call, 7 rows) and brings 1 row up
    // to the last row of the cache; slot 3 shares 20 of slot 4 (not in the call) and brings 5: 8 rows in all
    std::vector<int32_t> slots{2, 0, 3}, lens{7, 31, 20}, news{2, 1, 5}, parents{2, 2, 4}, shared{0, 7, 20};
    bool forks = true;
    int n_seqs = 3, hq = 8, hkv = 2;
    void *work;
    int64_t work_bytes = 0;
    void *out;
};

static const int32_t *ptr(const std::vector<int32_t> &v) { return v.empty() ? nullptr : v.data(); }

static int call(const Attn &a) {
    g_error[0] = 0;
    return crag_enc_decode_attention_rows((const uint16_t *)a.qkv, (const uint16_t *)a.qw, (const uint16_t *)a.kw,
                                          (const float *)a.cs, a.max_pos, (uint16_t *)a.kc, (uint16_t *)a.vc, a.n_slots,
                                          a.max_len, ptr(a.slots), ptr(a.lens), ptr(a.news), a.forks ? ptr(a.parents) : nullptr,
                                          a.forks ? ptr(a.shared) : nullptr, a.n_seqs, a.hq, a.hkv, 1e-6f, 0.088f, a.work,
                                          a.work_bytes, (uint16_t *)a.out, nullptr);
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
    ok.work_bytes = crag_enc_decode_workspace_bytes(8, ok.hq, ok.max_len);
    const char *T = "decode_attention_rows";
    Attn a;
    // the checks of decode_attention
    a = ok, a.lens[2] = 1 << 30, expect("a huge len", call(a), CRAG_EINVAL, T);
    a = ok, a.lens[0] = -1, expect("a negative len", call(a), CRAG_EINVAL, "negative");
    a = ok, a.n_seqs = 9, a.slots.resize(9), a.lens.resize(9), a.news.resize(9), a.parents.resize(9), a.shared.resize(9),
        expect("n_seqs 9", call(a), CRAG_EINVAL, T);
    a = ok, a.n_seqs = 0, expect("n_seqs 0", call(a), CRAG_EINVAL, T);
    a = ok, a.slots[2] = 2, expect("a repeated slot", call(a), CRAG_EINVAL, "twice");
    a = ok, a.slots[1] = 5, expect("slot == n_slots", call(a), CRAG_EINVAL, T);
    a = ok, a.slots[1] = -1, expect("a negative slot", call(a), CRAG_EINVAL, T);
    a = ok, a.hq = 6, expect("hq / hkv 3", call(a), CRAG_EINVAL, T);
    a = ok, a.hq = 2, expect("hq / hkv 1", call(a), CRAG_EINVAL, T);
    a = ok, a.hkv = 0, expect("hkv 0", call(a), CRAG_EINVAL, T);
    a = ok, a.max_len = 0, expect("max_len 0", call(a), CRAG_EINVAL, T);
    a = ok, a.n_slots = 0, expect("n_slots 0", call(a), CRAG_EINVAL, T);
    a = ok, a.qkv = nullptr, expect("NULL qkv", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.qw = nullptr, expect("NULL q_norm", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.kw = nullptr, expect("NULL k_norm", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.cs = nullptr, expect("NULL cos_sin", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.kc = nullptr, expect("NULL k cache", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.vc = nullptr, expect("NULL v cache", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.out = nullptr, expect("NULL out", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.work = nullptr, expect("NULL workspace", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.slots.clear(), expect("NULL slots", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.lens.clear(), expect("NULL lengths", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.kc = (char *)a.kc + 8, expect("a misaligned cache", call(a), CRAG_EINVAL, "aligned");
    a = ok, a.work_bytes -= 1, expect("the workspace one byte short", call(a), CRAG_E2BIG, "workspace");
    // the row counts
    a = ok, a.news.clear(), expect("NULL new lengths", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.news[1] = 0, expect("no new row", call(a), CRAG_EINVAL, "at least one");
    a = ok, a.news[2] = -3, expect("a negative row count", call(a), CRAG_EINVAL, "at least one");
    a = ok, a.news[2] = 6, expect("9 rows in all", call(a), CRAG_EINVAL, "at most 8");
    a = ok, a.news[0] = 0x7fffffff, expect("a huge row count", call(a), CRAG_EINVAL, "at most 8");
    a = ok, a.news[1] = 2, a.news[2] = 4, expect("one row beyond max_len", call(a), CRAG_EINVAL, "do not fit");
    a = ok, a.lens[1] = 32, expect("len == max_len", call(a), CRAG_EINVAL, "do not fit");
    a = ok, a.max_pos = 31, expect("a position beyond the RoPE table", call(a), CRAG_EINVAL, "do not fit");
    a = ok, a.lens[1] = 10, a.max_pos = 24, expect("the last of five rows beyond the RoPE table", call(a), CRAG_EINVAL, "do not fit");
    // the fork checks
    a = ok, a.parents.clear(), expect("NULL parents alone", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.shared.clear(), expect("NULL shared lengths alone", call(a), CRAG_EINVAL, "NULL");
    a = ok, a.parents[1] = 5, expect("parent == n_slots", call(a), CRAG_EINVAL, "parent 5");
    a = ok, a.parents[2] = -1, expect("a negative parent", call(a), CRAG_EINVAL, "parent -1");
    a = ok, a.parents[0] = 1 << 30, expect("a huge parent", call(a), CRAG_EINVAL, "parent");
    a = ok, a.shared[1] = -1, expect("a negative shared length", call(a), CRAG_EINVAL, "shared length -1");
    a = ok, a.shared[1] = 32, expect("a shared length beyond the cache length", call(a), CRAG_EINVAL, "shared length 32");
    a = ok, a.shared[2] = 21, expect("a shared length of cache_len + 1", call(a), CRAG_EINVAL, "shared length 21");
    a = ok, a.shared[0] = 1 << 30, expect("a huge shared length", call(a), CRAG_EINVAL, "shared length");
    a = ok, a.shared[1] = 8, expect("a row the parent appends in this call", call(a), CRAG_EINVAL, "which holds 7");
    a = ok, a.lens[0] = 6, expect("the parent in the call one row short", call(a), CRAG_EINVAL, "which holds 6");
    // both fork arrays NULL: nobody is forked, and the same refusals come first
    a = ok, a.forks = false, a.news[2] = 6, expect("9 rows, no forks", call(a), CRAG_EINVAL, "at most 8");
    a = ok, a.forks = false, a.work_bytes = 16, expect("a tiny workspace, no forks", call(a), CRAG_E2BIG, "workspace");
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
