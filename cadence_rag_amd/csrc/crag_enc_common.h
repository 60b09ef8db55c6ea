// crag_enc_common.h — the small helpers shared by the encoder-lane translation units (crag_encoder.hip,
// crag_attention.hip, crag_encoder_small.hip, crag_encoder_wide.hip, crag_rerank.hip, crag_decode.hip, crag_extend.hip,
// crag_grammar.hip, crag_sample.hip, crag_logprobs.hip, crag_penalty.hip): vector types, error reporting, bf16 conversion, fragment load,
// block and half-wave reductions, the per-head RMSNorm + RoPE of one head vector, the append of a row to the KV cache, the
// order-preserving key of a float, the (value, id) order of every greedy selection and its workgroup merge.  Internal linkage: nothing here is exported.
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

struct alignas(16) Pack8 {
    u16 v[8];
};

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

// A lane holds keys 4h.. of ITS query row (c = lane & 31, h = lane >> 5): a row's 32 keys of a tile sit in lanes c and
// c + 32 (crag_attention.hip, crag_extend.hip).  The two half-waves are combined with v_permlane32_swap instead of an
// LDS-crossbar shuffle.
__device__ __forceinline__ float halfwave_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float halfwave_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---------------------------------------------------------------------------------------------
// per-head q/k RMSNorm + rotate-half RoPE: 16 lanes per head vector, 8 elements each (chunk `sub` = lane & 15); lane j
// of the group pairs with lane j ^ 8 for rotate_half (element i <-> i + 64)
// ---------------------------------------------------------------------------------------------
// cos / sin of position `pos` for the 8 elements of chunk `sub`
__device__ __forceinline__ void rope_chunk(const float *cos_sin, int pos, int sub, float (&c)[8], float (&sn)[8]) {
    const float *cs = cos_sin + ((int64_t)pos * 64 + (sub & 7) * 8) * 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // the model casts cos/sin to bf16
        c[e] = bf2f(f2bf(cs[2 * e]));
        sn[e] = bf2f(f2bf(cs[2 * e + 1]));
    }
}

// chunk `a` of one head vector under the norm weights `w8`; first_half (sub < 8): elements [0, 64),
// out = x*cos - x[i+64]*sin ; else x*cos + x[i-64]*sin.  All 16 lanes of the group call it together.
__device__ __forceinline__ Pack8 norm_rope_chunk(const Pack8 &a, const Pack8 &w8, const float (&c)[8], const float (&sn)[8],
                                                 bool first_half, float eps) {
    float v[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = bf2f(a.v[e]);
        ss += v[e] * v[e];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o);  // 16-lane group
    const float rstd = rsqrtf(ss / (float)CRAG_HEAD_DIM + eps);
    float n[8], partner[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) n[e] = bf2f(f2bf(bf2f(w8.v[e]) * bf2f(f2bf(v[e] * rstd))));
#pragma unroll
    for (int e = 0; e < 8; ++e) partner[e] = __shfl_xor(n[e], 8);  // rotate_half: element i <-> i + 64
    Pack8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float rot = first_half ? -partner[e] : partner[e];
        o.v[e] = f2bf(n[e] * c[e] + rot * sn[e]);
    }
    return o;
}

// first element of row `pos` of (slot, kv head) in a cache [n_slots][hkv][max_len][128].  hkv and max_len by reference:
// the caller's parameter struct is then read where the value is used, which keeps the attention kernels' code as it was
__device__ __forceinline__ int64_t kv_row(const int &hkv, const int &max_len, int slot, int kvh, int pos) {
    return (((int64_t)slot * hkv + kvh) * max_len + pos) * CRAG_HEAD_DIM;
}

// One workgroup of KV_APPEND_THREADS appends one token: `row` is its raw [hq | hkv | hkv] projection.  The normed and
// rotated q heads go to q_rot_row [hq][128], the normed and rotated k heads and the raw v heads to row `pos` of the slot.
constexpr int KV_APPEND_THREADS = 256;  // 16 groups of 16 lanes: a group norms and rotates one head vector

__device__ __forceinline__ void kv_append_row(const u16 *row, const u16 *qw, const u16 *kw, const float *cos_sin,
                                              u16 *k_cache, u16 *v_cache, u16 *q_rot_row, int hq, int hkv, int max_len,
                                              int slot, int pos, float eps) {
    const int heads = hq + hkv;
    const int g = threadIdx.x >> 4;
    const int sub = threadIdx.x & 15;
    const Pack8 wq8 = *reinterpret_cast<const Pack8 *>(qw + sub * 8);
    const Pack8 wk8 = *reinterpret_cast<const Pack8 *>(kw + sub * 8);
    float c[8], sn[8];
    rope_chunk(cos_sin, pos, sub, c, sn);
    for (int hd = g; hd < heads; hd += KV_APPEND_THREADS / 16) {
        const Pack8 a = *reinterpret_cast<const Pack8 *>(row + (int64_t)hd * CRAG_HEAD_DIM + sub * 8);
        const Pack8 o = norm_rope_chunk(a, hd < hq ? wq8 : wk8, c, sn, sub < 8, eps);
        u16 *dst = hd < hq ? q_rot_row + (int64_t)hd * CRAG_HEAD_DIM : k_cache + kv_row(hkv, max_len, slot, hd - hq, pos);
        *reinterpret_cast<Pack8 *>(dst + sub * 8) = o;
    }
    for (int i = threadIdx.x; i < hkv * 16; i += KV_APPEND_THREADS) {
        const int kvh = i >> 4, ch = i & 15;
        *reinterpret_cast<Pack8 *>(v_cache + kv_row(hkv, max_len, slot, kvh, pos) + ch * 8) =
            *reinterpret_cast<const Pack8 *>(row + (int64_t)(heads + kvh) * CRAG_HEAD_DIM + ch * 8);
    }
}

// float <-> key (crag_sample.hip's cuts, crag_logprobs.hip's rank and top entries): a > b as floats exactly when
// key(a) > key(b); -0 and +0 share a key
__device__ __forceinline__ uint32_t fkey(float f) {
    uint32_t b = __float_as_uint(f);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kfloat(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---------------------------------------------------------------------------------------------
// The order of every greedy selection (lm_head's token, grammar_argmax, sample at T = 0 and its draw): a higher value
// wins, equal values go to the lower id -- the lowest id among the maxima.  bid < 0: nothing held yet.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool better(float v, int id, float bv, int bid) {
    return bid < 0 || v > bv || (v == bv && id < bid);
}

// Merges the (value, id) every thread of a workgroup of WAVES waves holds, and with PAYLOAD an int that travels with the
// winner: the lanes of a wave by shuffles, then thread 0 over the waves' entries in sv / si / sp (WAVES each; sp is not
// touched without PAYLOAD).  Thread 0 returns the winner, id < 0 when no thread held one.
struct Best {
    float v;
    int id, payload;
};

template <int WAVES, bool PAYLOAD>
__device__ __forceinline__ Best block_best(float bv, int bid, int payload, float *sv, int *si, int *sp) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bid, o);
        const int op = PAYLOAD ? __shfl_xor(payload, o) : 0;
        if (oi >= 0 && better(ov, oi, bv, bid)) {
            bv = ov;
            bid = oi;
            if (PAYLOAD) payload = op;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bid;
        if (PAYLOAD) sp[threadIdx.x >> 6] = payload;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < WAVES; ++k)
            if (si[k] >= 0 && better(sv[k], si[k], bv, bid)) {
                bv = sv[k];
                bid = si[k];
                if (PAYLOAD) payload = sp[k];
            }
    }
    return Best{bv, bid, payload};
}

}  // namespace
