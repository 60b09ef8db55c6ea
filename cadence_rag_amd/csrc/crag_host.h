// crag_host.h — the host helpers shared by the translation units of the C ABI: error reporting, device selection,
// grow-only device buffers, host-or-device inputs, the CU count, the argument checks of the BM25 and row-mask entries and
// their upload packer.  Host code only; hidden visibility: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/crag_dense.h"

// stores the message crag_last_error() returns; the thread-local storage lives in crag_api.hip alone
extern "C" void crag_set_error_(const char *msg);
// the upload slot of the lanes that take host query data (crag_fusion.hip): wait for its last copy and hand out its
// buffers, at least `bytes` large / one asynchronous copy of their first `bytes` on `stream`
extern "C" int crag_upload_slot_begin_(crag_upload_slot *s, size_t bytes, void **host, void **dev);
extern "C" int crag_upload_slot_commit_(crag_upload_slot *s, size_t bytes, void *stream);

#pragma GCC visibility push(hidden)

// records the formatted message and returns `code`: every C entry point reports an error through this
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    crag_set_error_(buf);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(CRAG_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// The two argument checks every entry point that works in a caller's scratch makes; `op` heads its messages, `sizer`
// names the function that tells the size.
inline int check_nq(const char *op, int nq) {   // (a grid dimension)
    if (nq < 0 || nq > 65535) return fail(CRAG_EINVAL, "%s: nq must be in [0, 65535] (got %d)", op, nq);
    return CRAG_OK;
}
inline int check_scratch(const char *op, const void *scratch, int64_t have, int64_t need, const char *sizer) {
    if (have < need || ((uintptr_t)scratch & 7))
        return fail(CRAG_EINVAL, "%s: scratch too small or not 8-byte aligned (%s)", op, sizer);
    return CRAG_OK;
}

// The argument checks the BM25 entries share (crag_bm25*.hip).  All of them are host work: an entry runs them before its
// first HIP call.
// ptr [n + 1] is a CSR pointer: it starts at 0, never descends, and no entry holds more than `limit` (< 0: any number)
inline int check_csr(const char *op, const char *name, const char *noun, const int32_t *ptr, int n, int64_t limit) {
    if (ptr[0] != 0) return fail(CRAG_EINVAL, "%s: %s[0] must be 0", op, name);
    for (int i = 0; i < n; ++i) {
        const int64_t cnt = (int64_t)ptr[i + 1] - ptr[i];
        if (cnt < 0) return fail(CRAG_EINVAL, "%s: %s must not descend (%s %d)", op, name, noun, i);
        if (limit >= 0 && cnt > limit)
            return fail(CRAG_EINVAL, "%s: %s %d holds %lld by %s, at most %lld", op, noun, i, (long long)cnt, name,
                        (long long)limit);
    }
    return CRAG_OK;
}
inline int check_terms(const char *op, const int32_t *terms, int64_t a, int64_t b, int64_t n_terms) {
    for (int64_t i = a; i < b; ++i)
        if (terms[i] < 0 || (int64_t)terms[i] >= n_terms)
            return fail(CRAG_EINVAL, "%s: term id %d (entry %lld) is outside [0, n_terms)", op, terms[i], (long long)i);
    return CRAG_OK;
}
inline int check_bm25_counts(const char *op, int nq, int nq_min, int64_t n_rows, int64_t n_terms) {
    if (nq < nq_min || nq > 64) return fail(CRAG_EINVAL, "%s: need %d <= nq <= 64 (nq=%d)", op, nq_min, nq);
    if (n_rows < 0 || n_rows > INT32_MAX) return fail(CRAG_EINVAL, "%s: n_rows must be in [0, 2^31)", op);
    if (n_terms < 0 || n_terms > INT32_MAX) return fail(CRAG_EINVAL, "%s: n_terms must be in [0, 2^31)", op);
    return CRAG_OK;
}
// The runs of packed row masks an entry writes or reads (crag_filter.hip, crag_attr.hip, crag_facet.hip,
// crag_bm25_clause.hip): a stride in bytes is a multiple of 4 in [ceil(n_rows/32)*4, 2^32]
inline bool mask_stride_ok(int64_t n_rows, int64_t stride) {
    return stride >= (n_rows + 31) / 32 * 4 && stride % 4 == 0 && stride <= ((int64_t)1 << 32);
}
// the input and output runs of an entry that writes row masks (d_in NULL: it reads none)
inline int check_mask_strides(const char *op, int64_t n_rows, const void *d_in, int64_t in_stride, const void *d_out,
                              int64_t out_stride) {
    if (!mask_stride_ok(n_rows, out_stride))
        return fail(CRAG_EINVAL, "%s: mask_stride must be a multiple of 4 in [ceil(n_rows/32)*4, 2^32]", op);
    if (d_in && in_stride != 0 && !mask_stride_ok(n_rows, in_stride))
        return fail(CRAG_EINVAL, "%s: in_stride must be 0 or a multiple of 4 in [ceil(n_rows/32)*4, 2^32]", op);
    if (out_stride > 0 && !d_out) return fail(CRAG_EINVAL, "%s: NULL output pointer", op);
    if (((uintptr_t)d_out & 3) != 0) return fail(CRAG_EINVAL, "%s: the output must be 4-byte aligned", op);
    if (((uintptr_t)d_in & 3) != 0) return fail(CRAG_EINVAL, "%s: the input mask must be 4-byte aligned", op);
    return CRAG_OK;
}
// the runs of an entry that only reads row masks, one run per query (d_masks NULL: every row passes, no stride to check)
inline int check_mask_input(const char *op, int64_t n_rows, const void *d_masks, int64_t stride) {
    if (((uintptr_t)d_masks & 3) != 0) return fail(CRAG_EINVAL, "%s: the masks must be 4-byte aligned", op);
    if (d_masks && !mask_stride_ok(n_rows, stride))
        return fail(CRAG_EINVAL, "%s: mask_stride must be a multiple of 4 in [ceil(n_rows/32)*4, 2^32]", op);
    return CRAG_OK;
}

// One upload through a slot, laid out once: add() declares the arrays in slot order (count elements are copied from p,
// `reserve` bytes are kept for them -- a padded head reserves more than it copies), begin() takes the slot's buffers and
// copies, commit() enqueues the upload, dev<T>(i) is array i on the device.  What begin() does not copy is not written.
struct UploadPack {
    static constexpr int MAX_ARRAYS = 6;
    const void *src[MAX_ARRAYS];
    size_t copy[MAX_ARRAYS], off[MAX_ARRAYS];
    int n = 0;
    size_t bytes = 0;
    char *h = nullptr, *d = nullptr;
    template <class T> int add(const T *p, size_t count, size_t reserve) {
        src[n] = p;
        copy[n] = count * sizeof(T);
        off[n] = bytes;
        bytes += reserve;
        return n++;
    }
    template <class T> int add(const T *p, size_t count) { return add(p, count, count * sizeof(T)); }
    int begin(crag_upload_slot *slot) {
        void *hv = nullptr, *dv = nullptr;
        const int rc = crag_upload_slot_begin_(slot, bytes, &hv, &dv);
        if (rc != CRAG_OK) return rc;
        h = (char *)hv;
        d = (char *)dv;
        for (int i = 0; i < n; ++i)
            if (copy[i] > 0) memcpy(h + off[i], src[i], copy[i]);
        return CRAG_OK;
    }
    int commit(crag_upload_slot *slot, void *stream) { return crag_upload_slot_commit_(slot, bytes, stream); }
    template <class T> T *host(int i) const { return (T *)(h + off[i]); }
    template <class T> const T *dev(int i) const { return (const T *)(d + off[i]); }
};

// behind one or more hipLaunchKernelGGL
inline int launch_ok(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CRAG_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return CRAG_OK;
}

// the compute units of the current device, asked once per process (256 when the runtime does not say): what the
// persistent grids are sized by
inline int cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            n = v;
        else
            n = 256;
    }
    return n;
}

inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // plain host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct DevBuf {  // grow-only device scratch
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return CRAG_OK;
        release();
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(CRAG_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        bytes = want;
        return CRAG_OK;
    }
    // for a buffer whose users leave it zeroed: grown, the whole of it is zeroed on `st` before they see it
    int ensure_zeroed(size_t need, hipStream_t st) {
        if (need <= bytes) return CRAG_OK;
        int rc = ensure(need);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(p, 0, bytes, st));
        return CRAG_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// an input the caller may hold on either side: *dev = p itself, or its copy in `stage` (synchronous upload)
template <class T> int stage_in(DevBuf &stage, const T *p, size_t bytes, const T **dev) {
    *dev = p;
    if (is_device_ptr(p)) return CRAG_OK;
    int rc = stage.ensure(bytes);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(stage.p, p, bytes, hipMemcpyHostToDevice));
    *dev = (const T *)stage.p;
    return CRAG_OK;
}

// the bits of a row mask's last word that stand for stored rows
inline uint32_t tail_mask(int64_t size) { return (size & 31) ? (1u << (size & 31)) - 1u : 0xffffffffu; }

#pragma GCC visibility pop
