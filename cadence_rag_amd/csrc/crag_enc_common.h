// crag_enc_common.h — the small helpers shared by the encoder-lane translation units (crag_encoder.hip,
// crag_attention.hip, crag_encoder_small.hip, crag_encoder_wide.hip, crag_rerank.hip): vector types, error reporting,
// bf16 conversion, fragment load, block reduction.  Internal linkage: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "crag_arch.h"

extern "C" void crag_set_error_(const char *msg);  // defined in crag_api.hip

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16;

// records the message for crag_last_error(); every C entry point returns through one of these two
int efail(const char *fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    crag_set_error_(buf);
    return -1;
}

int hip_ok(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s launch failed: %s", what, hipGetErrorString(e));
        crag_set_error_(buf);
        return -2;
    }
    return 0;
}

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) {  // round-to-nearest-even, NaN stays NaN (v_cvt_pk_bf16_f32)
    return __builtin_bit_cast(u16, (__bf16)f);
}

__device__ __forceinline__ bf16x8 ld_frag(const u16 *p) { return *reinterpret_cast<const bf16x8 *>(p); }

// sum over the workgroup; `sh` holds one float per wave.  Every thread returns the total.
__device__ __forceinline__ float block_sum(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wv] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    __syncthreads();
    return t;
}

}  // namespace
