// crag_rerank.hip — the two operators a Qwen3-Reranker forward adds to the encoder lane (gfx950).
// C ABI: include/crag_encoder.h.
//
//   crag_enc_attention_prefixed  causal GQA flash attention in which a sequence may name a PARENT segment of the same
//                                packed batch: its queries see every key of the parent, then their own keys causally.
//                                The 40-80 (query, document) pairs of one rerank request share their first 60-100
//                                tokens (system prompt, instruction, query); the shared tokens run once, as a root
//                                segment, and every document segment attends to it.
//   crag_enc_rerank_head         residual add + final RMSNorm of the pooled rows, then the "yes" / "no" rows of lm_head
//                                and the model card's score, exp(log_softmax([no, yes])[1]).
//
// The attention kernel is crag_encoder.hip's attention_kernel (one workgroup per (kv head, 32-row q block), GROUP =
// hq/hkv waves, LDS-staged double-buffered K / V^T tiles, one online softmax) with a longer key walk: the parent's
// tiles first, the sequence's own after them.  attention_kernel itself is not touched.

#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/crag_encoder.h"

extern "C" void crag_set_error_(const char *msg);  // defined in crag_api.hip

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16;

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
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }
__device__ __forceinline__ bf16x8 ld_frag(const u16 *p) { return *reinterpret_cast<const bf16x8 *>(p); }

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

// ---------------------------------------------------------------------------------------------
// shared-prefix causal GQA flash attention (head_dim 128)
// ---------------------------------------------------------------------------------------------
struct PrefixAttnParams {
    const u16 *qkv;
    const u16 *vt;
    u16 *out;
    const int32_t *cu, *cu_pad, *blk_seq, *blk_q0, *parent;
    int64_t t_pad;
    int hq, hkv;
    float scale_log2;
};

constexpr int ATT_KROW = 136;  // u16 per staged K row (128 + 8 pad): conflict-free ds_read_b128
constexpr int ATT_VROW = 40;   // u16 per staged V^T row (32 + 8 pad)

template <int GROUP>
__global__ __launch_bounds__(64 * GROUP) __attribute__((amdgpu_waves_per_eu(2, 8)))
void attention_prefixed_kernel(PrefixAttnParams p) {
    constexpr int K_BUF = 32 * ATT_KROW, V_BUF = CRAG_HEAD_DIM * ATT_VROW;
    static_assert(GROUP * 32 * ATT_KROW <= 2 * (K_BUF + V_BUF), "output tiles must fit the staging pool");
    __shared__ __attribute__((aligned(16))) u16 s_pool[2 * (K_BUF + V_BUF)];
    u16(*s_k)[K_BUF] = reinterpret_cast<u16(*)[K_BUF]>(s_pool);
    u16(*s_v)[V_BUF] = reinterpret_cast<u16(*)[V_BUF]>(s_pool + 2 * K_BUF);
    constexpr int nthr = 64 * GROUP;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int kvh = blockIdx.x;
    const int head = kvh * GROUP + wave;
    const int seq = p.blk_seq[blockIdx.y];
    const int q0 = p.blk_q0[blockIdx.y];
    const int s_begin = p.cu[seq];
    const int len = p.cu[seq + 1] - s_begin;
    const int par = p.parent[seq];
    const int p_begin = par >= 0 ? p.cu[par] : 0;
    const int plen = par >= 0 ? p.cu[par + 1] - p_begin : 0;
    const int n_pt = (plen + 31) / 32;  // parent key tiles, walked first
    const int n_all = n_pt + q0 / 32 + 1;
    const int c = lane & 31, h = lane >> 5;
    const int64_t row_stride = (int64_t)(p.hq + 2 * p.hkv) * CRAG_HEAD_DIM;

    bf16x8 qf[8];
    {
        const u16 *qp = p.qkv + (int64_t)(s_begin + q0 + c) * row_stride + (int64_t)head * CRAG_HEAD_DIM + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = ld_frag(qp + 16 * s);
    }
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 oacc[4] = {zero, zero, zero, zero};
    float m = -INFINITY, l = 0.f;
    const u16 *kown = p.qkv + (int64_t)s_begin * row_stride + (int64_t)(p.hq + kvh) * CRAG_HEAD_DIM;
    const u16 *vown = p.vt + (int64_t)kvh * CRAG_HEAD_DIM * p.t_pad + p.cu_pad[seq];
    const u16 *kpar = p.qkv + (int64_t)p_begin * row_stride + (int64_t)(p.hq + kvh) * CRAG_HEAD_DIM;
    const u16 *vpar = p.vt + (int64_t)kvh * CRAG_HEAD_DIM * p.t_pad + (par >= 0 ? p.cu_pad[par] : 0);

    // tile kt < n_pt: keys 32 kt .. of the parent (its padded tail masked); after them the sequence's own tiles.
    // Key rows past a segment's end are rows of the next segment or of the 32 rows qkv extends past T, and their
    // V^T slots are the zero pads of the segment's 32-aligned range: read, then masked.
    constexpr int per = 512 / nthr;
    struct Stage {
        bf16x8 k[per], v[per];
    };
    auto fetch = [&](int kt, Stage &st) {
        const bool in_par = kt < n_pt;
        const int k0 = (in_par ? kt : kt - n_pt) * 32;
        const u16 *kg = in_par ? kpar : kown;
        const u16 *vg = in_par ? vpar : vown;
#pragma unroll
        for (int i = 0; i < per; ++i) {
            const int ch = tid + i * nthr;
            st.k[i] = ld_frag(kg + (int64_t)(k0 + (ch >> 4)) * row_stride + 8 * (ch & 15));
            st.v[i] = ld_frag(vg + (int64_t)(ch >> 2) * p.t_pad + k0 + 8 * (ch & 3));
        }
    };
    auto stash = [&](int buf, const Stage &st) {
#pragma unroll
        for (int i = 0; i < per; ++i) {
            const int ch = tid + i * nthr;
            *reinterpret_cast<bf16x8 *>(&s_k[buf][(ch >> 4) * ATT_KROW + 8 * (ch & 15)]) = st.k[i];
            *reinterpret_cast<bf16x8 *>(&s_v[buf][(ch >> 2) * ATT_VROW + 8 * (ch & 3)]) = st.v[i];
        }
    };
    Stage st;
    fetch(0, st);
    stash(0, st);
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // clean vmcnt scoreboard at the loop head (see attention_kernel)

    for (int kt = 0; kt < n_all; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < n_all) fetch(kt + 1, st);
        bf16x8 fr[8];
        {
            const u16 *kp = &s_k[buf][c * ATT_KROW + 8 * h];
#pragma unroll
            for (int s = 0; s < 8; ++s) fr[s] = *reinterpret_cast<const bf16x8 *>(kp + 16 * s);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 sacc = zero;
#pragma unroll
        for (int s = 0; s < 8; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[s], qf[s], sacc, 0, 0, 0);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                fr[2 * dt + s2] = *reinterpret_cast<const bf16x8 *>(&s_v[buf][(32 * dt + c) * ATT_VROW + 8 * h + 16 * s2]);
        __builtin_amdgcn_sched_barrier(0);
        // visible keys of this tile for query row q0 + c: tile-relative index < lim
        //   parent tile: all of the parent's keys;  own tile: causal on the diagonal tile, all before it
        int lim;
        if (kt < n_pt) lim = plen - kt * 32;
        else lim = (kt == n_all - 1) ? q0 + c - (kt - n_pt) * 32 + 1 : 32;
        float sv[16];
        float mloc = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
            float v = sacc[i] * p.scale_log2;
            if (r >= lim) v = -INFINITY;
            sv[i] = v;
            mloc = fmaxf(mloc, v);
        }
        {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mloc), __float_as_uint(mloc), false, false);
            mloc = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
        }
        // finite from the first tile on: key 0 of the parent (plen >= 1) or of the sequence (<= q0 + c) is visible
        const float mnew = fmaxf(m, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sv[i] = __builtin_amdgcn_exp2f(sv[i] - mnew);
            lsum += sv[i];
        }
        {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(lsum), __float_as_uint(lsum), false, false);
            lsum = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
        l = l * alpha + lsum;
        if (__any(mnew != m)) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
        }
        m = mnew;
        bf16x8 pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pf[s2][jj] = (short)f2bf(sv[8 * s2 + jj]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2 * dt + s2], pf[s2], oacc[dt], 0, 0, 0);
        if (kt + 1 < n_all) stash(buf ^ 1, st);
        __syncthreads();
    }
    // the 32 x 128 output tile transposed through LDS and written as whole rows (attention_kernel's epilogue)
    {
        u16 *ot = s_pool + wave * (32 * ATT_KROW);
        const float inv = 1.f / l;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint2 w;
                w.x = (uint32_t)f2bf(oacc[dt][4 * g4] * inv) | ((uint32_t)f2bf(oacc[dt][4 * g4 + 1] * inv) << 16);
                w.y = (uint32_t)f2bf(oacc[dt][4 * g4 + 2] * inv) | ((uint32_t)f2bf(oacc[dt][4 * g4 + 3] * inv) << 16);
                *reinterpret_cast<uint2 *>(ot + c * ATT_KROW + 32 * dt + 8 * g4 + 4 * h) = w;
            }
        u16 *obase = p.out + (int64_t)(s_begin + q0) * ((int64_t)p.hq * CRAG_HEAD_DIM) + (int64_t)head * CRAG_HEAD_DIM;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = (lane >> 4) + 4 * it, chunk = lane & 15;
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(ot + row * ATT_KROW + 8 * chunk);
            if (q0 + row < len)
                *reinterpret_cast<bf16x8 *>(obase + (int64_t)row * ((int64_t)p.hq * CRAG_HEAD_DIM) + 8 * chunk) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// rerank head: one workgroup per pair
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_THREADS = 256;

__global__ __launch_bounds__(HEAD_THREADS) void rerank_head_kernel(const u16 *hs, const u16 *delta, const u16 *w,
                                                                   const int64_t *rows, const u16 *lm, float *out,
                                                                   int hidden, float eps) {
    __shared__ float sh[HEAD_THREADS / 64];
    __shared__ float row[8192];
    const int b = blockIdx.x;
    const int64_t r = rows[b];
    const u16 *x = hs + r * hidden;
    const u16 *dl = delta ? delta + r * hidden : nullptr;
    float ss = 0.f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = dl ? bf2f(f2bf(bf2f(x[i]) + bf2f(dl[i]))) : bf2f(x[i]);
        row[i] = v;
        ss += v * v;
    }
    ss = block_sum(ss, sh);
    const float rstd = rsqrtf(ss / (float)hidden + eps);
    // the final norm's output in the model's bf16 (pool_normalize_kernel's roundings), then fp32 dots with the two rows
    float dy = 0.f, dn = 0.f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = bf2f(f2bf(bf2f(w[i]) * bf2f(f2bf(row[i] * rstd))));
        dy += v * bf2f(lm[i]);
        dn += v * bf2f(lm[hidden + i]);
    }
    dy = block_sum(dy, sh);
    dn = block_sum(dn, sh);
    if (threadIdx.x == 0) {
        // exp(log_softmax([no, yes])[1]) = 1 / (1 + exp(no - yes)), in the form that cannot overflow
        const float d = dy - dn;
        const float e = expf(-fabsf(d));
        const float score = d >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        out[3 * (int64_t)b + 0] = dy;
        out[3 * (int64_t)b + 1] = dn;
        out[3 * (int64_t)b + 2] = score;
    }
}

}  // namespace

extern "C" {

int crag_enc_attention_prefixed(const uint16_t *qkv, const uint16_t *vt, uint16_t *out, const int32_t *cu_seqlens,
                                const int32_t *cu_pad, const int32_t *blk_seq, const int32_t *blk_q0,
                                const int32_t *parent, int n_blocks, int64_t t_pad, int hq, int hkv, float scale,
                                void *stream) {
    if (!qkv || !vt || !out || !cu_seqlens || !cu_pad || !blk_seq || !blk_q0 || !parent)
        return efail("attention_prefixed: NULL pointer");
    if (hkv <= 0 || hq % hkv != 0 || (hq / hkv != 2 && hq / hkv != 4))
        return efail("attention_prefixed: hq/hkv must be 2 or 4");
    if (n_blocks <= 0) return 0;
    if (n_blocks > 65535 * 64) return efail("attention_prefixed: too many q blocks (%d)", n_blocks);
    PrefixAttnParams p;
    p.qkv = qkv;
    p.vt = vt;
    p.out = out;
    p.cu = cu_seqlens;
    p.cu_pad = cu_pad;
    p.blk_seq = blk_seq;
    p.blk_q0 = blk_q0;
    p.parent = parent;
    p.t_pad = t_pad;
    p.hq = hq;
    p.hkv = hkv;
    p.scale_log2 = scale * 1.4426950408889634f;
    const dim3 grid((unsigned)hkv, (unsigned)n_blocks);
    if (hq / hkv == 2) hipLaunchKernelGGL(attention_prefixed_kernel<2>, grid, dim3(128), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(attention_prefixed_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return hip_ok("attention_prefixed");
}

int crag_enc_rerank_head(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                         const int64_t *rows, const uint16_t *lm_rows, float *out, int n_pairs, int hidden, float eps,
                         void *stream) {
    if (!hidden_states || !final_norm_w || !rows || !lm_rows || !out) return efail("rerank_head: NULL pointer");
    if (hidden <= 0 || hidden > 8192) return efail("rerank_head: hidden must be in 1..8192 (got %d)", hidden);
    if (n_pairs <= 0) return 0;
    hipLaunchKernelGGL(rerank_head_kernel, dim3((unsigned)n_pairs), dim3(HEAD_THREADS), 0, (hipStream_t)stream,
                       hidden_states, delta, final_norm_w, rows, lm_rows, out, hidden, eps);
    return hip_ok("rerank_head");
}

}  // extern "C"
