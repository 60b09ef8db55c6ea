// crag_host.h — the host helpers shared by the translation units of the C ABI: error reporting, device selection,
// grow-only device buffers, host-or-device inputs.  Host code only; hidden visibility: nothing here is exported.
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

// behind one or more hipLaunchKernelGGL
inline int launch_ok(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CRAG_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return CRAG_OK;
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
