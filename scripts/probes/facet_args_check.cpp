// facet_args_check.cpp -- the argument checks of crag_facet_counts_host under the host sanitizers, on the CPU.
// A stand-alone program: it compiles the unit's host code with AddressSanitizer and UBSan and walks every refusal of the
// entry (each returns before the first HIP call, so no GPU is needed or touched).  Build and run from csrc/:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         crag_facet.hip ../../scripts/probes/facet_args_check.cpp -o /tmp/facet_args_check && /tmp/facet_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/crag_dense.h"

static char g_error[512];
extern "C" void crag_set_error_(const char *msg) {   // crag_api.hip's, which this program does not link
    strncpy(g_error, msg, sizeof(g_error) - 1);
}

struct Args {
    const void *ptr, *rows, *fid;
    int64_t n_postings = 50, n_rows = 100, n_attrs = 10;
    const uint8_t *masks;
    int64_t stride = 16;
    std::vector<int32_t> lo{0, 4}, hi{4, 10};
    int n_ranges = 2, nq = 2, top = 5;
    void *work;
    int64_t work_bytes = 100 * 8 + 2 * 10 * 4;
    void *ids, *counts, *distinct, *out_rows;
};

static int call(const Args &a) {
    g_error[0] = 0;
    return crag_facet_counts_host((const int64_t *)a.ptr, (const int32_t *)a.rows, (const int32_t *)a.fid, a.n_postings, a.n_rows,
                                  a.n_attrs, a.masks, a.stride, a.lo.empty() ? nullptr : a.lo.data(),
                                  a.hi.empty() ? nullptr : a.hi.data(), a.n_ranges, a.nq, a.top, a.work, a.work_bytes,
                                  (int32_t *)a.ids, (uint32_t *)a.counts, (int32_t *)a.distinct, (int64_t *)a.out_rows, nullptr);
}

int main() {
    static uint64_t some[64];   // stands for device memory: a refusal comes before any use
    Args ok;
    ok.ptr = ok.rows = ok.fid = some;
    ok.masks = (const uint8_t *)some;
    ok.work = ok.ids = ok.counts = ok.distinct = ok.out_rows = some;
    int failures = 0, cases = 0;
    auto expect = [&](const char *what, Args a, int code) {
        const int rc = call(a);
        ++cases;
        if (rc != code || !strstr(g_error, "facet_counts_host")) {
            printf("FAIL %s: returned %d (%s), expected %d\n", what, rc, g_error, code);
            ++failures;
        }
    };
    Args a;
    a = ok, a.nq = 0, expect("nq 0", a, CRAG_EINVAL);
    a = ok, a.nq = 65, expect("nq 65", a, CRAG_EINVAL);
    a = ok, a.top = 0, expect("top 0", a, CRAG_EINVAL);
    a = ok, a.top = 65, expect("top 65", a, CRAG_EINVAL);
    a = ok, a.n_attrs = 20, a.n_ranges = 17, a.lo.resize(17), a.hi.resize(17);
    for (int r = 0; r < 17; ++r) a.lo[r] = r, a.hi[r] = r + 1;
    expect("17 ranges", a, CRAG_EINVAL);
    a = ok, a.hi = {4, 11}, expect("a range beyond n_attrs", a, CRAG_EINVAL);
    a = ok, a.lo = {-1, 4}, expect("a negative range", a, CRAG_EINVAL);
    a = ok, a.lo = {5, 6}, expect("lo > hi", a, CRAG_EINVAL);
    a = ok, a.lo = {0, 3}, expect("overlapping ranges", a, CRAG_EINVAL);
    a = ok, a.masks += 2, expect("a misaligned mask", a, CRAG_EINVAL);
    a = ok, a.stride = 12, expect("a short stride", a, CRAG_EINVAL);
    a = ok, a.stride = 18, expect("a stride that is no multiple of 4", a, CRAG_EINVAL);
    a = ok, a.n_rows = -1, expect("negative n_rows", a, CRAG_EINVAL);
    a = ok, a.n_rows = (int64_t)1 << 31, a.stride = (int64_t)1 << 28, expect("n_rows 2^31", a, CRAG_EINVAL);
    a = ok, a.ids = nullptr, expect("NULL ids", a, CRAG_EINVAL);
    a = ok, a.counts = nullptr, expect("NULL counts", a, CRAG_EINVAL);
    a = ok, a.distinct = nullptr, expect("NULL distinct", a, CRAG_EINVAL);
    a = ok, a.out_rows = nullptr, expect("NULL rows", a, CRAG_EINVAL);
    a = ok, a.lo.clear(), expect("NULL ranges", a, CRAG_EINVAL);
    a = ok, a.ptr = nullptr, expect("NULL postings", a, CRAG_EINVAL);
    a = ok, a.work = nullptr, expect("NULL workspace", a, CRAG_EINVAL);
    a = ok, a.work = (char *)a.work + 4, expect("a misaligned workspace", a, CRAG_EINVAL);
    a = ok, a.work_bytes -= 1, expect("the workspace one byte short", a, CRAG_E2BIG);
    a = ok, a.masks = nullptr, a.work_bytes = 2 * 10 * 4 - 1, expect("no masks, one byte short", a, CRAG_E2BIG);
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
