// crag_enc_common.h — the small helpers shared by the encoder-lane translation units (crag_encoder.hip,
// crag_attention.hip, crag_encoder_small.hip, crag_encoder_wide.hip, crag_rerank.hip): vector types, error reporting,
// bf16 conversion, fragment load, block reduction.  Internal linkage: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_arch.h"
#include "crag_host.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16;

// records the message for crag_last_error(); every C entry point of the encoder lane returns through one of these
// two: -1 for a bad argument, -2 behind a launch that failed (the values of CRAG_EINVAL / CRAG_EHIP)
#define efail(...) fail(-1, __VA_ARGS__)
int hip_ok(const char *what) { return launch_ok(what); }

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
