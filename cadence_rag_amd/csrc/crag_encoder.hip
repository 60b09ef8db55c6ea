// crag_encoder.hip — hand-written HIP operators of the Qwen3-Embedding encoder lane for gfx950.
// C ABI: include/crag_encoder.h.  Everything of the decoder forward except the plain linear layers
// (library GEMMs issued by the Python host) lives here: embedding gather, RMSNorm (+ residual),
// per-head q/k RMSNorm + RoPE, V transpose, SwiGLU, the gateway's pooling / slice / L2 normalisation and the
// skinny GEMM; causal GQA flash attention (bf16 MFMA) is crag_attention.hip.
//
// Reference math (not code): P620_TRITON_QWEN3_4B_EMBEDDING_RUNBOOK.md:683-716 for the
// post-processing; the model family's public architecture for the layer (checked against
// transformers' Qwen3Model in tests/test_encoder_gpu.py).

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// embedding gather
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_gather_kernel(const int32_t *ids, const u16 *table, u16 *out,
                                                           int64_t n_tokens, int hidden, int64_t vocab) {
    const int chunks = hidden >> 3;
    for (int64_t t = blockIdx.x; t < n_tokens; t += gridDim.x) {
        int64_t id = ids[t];
        if (id < 0) id = 0;
        if (id >= vocab) id = vocab - 1;
        const Pack8 *src = reinterpret_cast<const Pack8 *>(table + id * hidden);
        Pack8 *dst = reinterpret_cast<Pack8 *>(out + t * hidden);
        for (int c = threadIdx.x; c < chunks; c += blockDim.x) dst[c] = src[c];
    }
}

// ---------------------------------------------------------------------------------------------
// RMSNorm (+ residual add)
// ---------------------------------------------------------------------------------------------
constexpr int NORM_THREADS = 256;
constexpr int NORM_MAX_CHUNKS = 4;  // hidden <= 8 * 256 * 4 = 8192

__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_kernel(const u16 *x, const u16 *res_in, const u16 *w,
                                                               u16 *out, u16 *res_out, int64_t rows, int hidden,
                                                               float eps) {
    __shared__ float sh[NORM_THREADS / 64];
    const int chunks = hidden >> 3;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const Pack8 *xr = reinterpret_cast<const Pack8 *>(x + r * hidden);
        const Pack8 *rr = res_in ? reinterpret_cast<const Pack8 *>(res_in + r * hidden) : nullptr;
        float v[NORM_MAX_CHUNKS][8];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NORM_MAX_CHUNKS; ++i) {
            const int c = threadIdx.x + i * NORM_THREADS;
            if (c < chunks) {
                const Pack8 a = xr[c];
                Pack8 s8;
                if (rr) {
                    const Pack8 b = rr[c];
#pragma unroll
                    for (int e = 0; e < 8; ++e) s8.v[e] = f2bf(bf2f(a.v[e]) + bf2f(b.v[e]));  // bf16 add, as the model does
                } else {
                    s8 = a;
                }
                if (res_out) reinterpret_cast<Pack8 *>(res_out + r * hidden)[c] = s8;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[i][e] = bf2f(s8.v[e]);
                    ss += v[i][e] * v[i][e];
                }
            }
        }
        ss = block_sum(ss, sh);
        const float rstd = rsqrtf(ss / (float)hidden + eps);
#pragma unroll
        for (int i = 0; i < NORM_MAX_CHUNKS; ++i) {
            const int c = threadIdx.x + i * NORM_THREADS;
            if (c < chunks) {
                const Pack8 w8 = reinterpret_cast<const Pack8 *>(w)[c];
                Pack8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o.v[e] = f2bf(bf2f(w8.v[e]) * bf2f(f2bf(v[i][e] * rstd)));
                reinterpret_cast<Pack8 *>(out + r * hidden)[c] = o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// per-head q/k RMSNorm + RoPE, in place on the fused qkv rows (norm_rope_chunk, crag_enc_common.h: 16 lanes per head
// vector, 8 elements each)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void qk_norm_rope_body(u16 *qkv, const u16 *qw, const u16 *kw, const float *cos_sin,
                                                  const int32_t *positions, int64_t n_tokens, int hq, int hkv,
                                                  float eps, int64_t first_token, int64_t token_stride) {
    // One block trip = one token: group g (16 lanes) walks the head vectors g, g + 16, g + 32, ... of the token with
    // the token's cos/sin chunk and the norm weights in registers (loaded per head vector they were 64 B of table
    // reads per 16 B of q/k: twice the data traffic, from the caches).
    const int heads = hq + hkv;  // q heads then k heads are contiguous in the row
    const int64_t row_stride = (int64_t)(hq + 2 * hkv) * CRAG_HEAD_DIM;
    const int g = threadIdx.x >> 4;
    const int sub = threadIdx.x & 15;  // 8-element chunk of the head
    const bool first_half = sub < 8;   // elements [0, 64): out = x*cos - x[i+64]*sin ; else x*cos + x[i-64]*sin
    const Pack8 wq8 = *reinterpret_cast<const Pack8 *>(qw + sub * 8);
    const Pack8 wk8 = *reinterpret_cast<const Pack8 *>(kw + sub * 8);
    for (int64_t t = first_token; t < n_tokens; t += token_stride) {
        float c[8], sn[8];
        rope_chunk(cos_sin, positions[t], sub, c, sn);
        for (int hd = g; hd < heads; hd += 16) {
            u16 *p = qkv + t * row_stride + (int64_t)hd * CRAG_HEAD_DIM + sub * 8;
            const Pack8 a = *reinterpret_cast<Pack8 *>(p);
            *reinterpret_cast<Pack8 *>(p) = norm_rope_chunk(a, hd < hq ? wq8 : wk8, c, sn, first_half, eps);
        }
    }
}

__global__ __launch_bounds__(256) void qk_norm_rope_kernel(u16 *qkv, const u16 *qw, const u16 *kw,
                                                           const float *cos_sin, const int32_t *positions,
                                                           int64_t n_tokens, int hq, int hkv, float eps) {
    qk_norm_rope_body(qkv, qw, kw, cos_sin, positions, n_tokens, hq, hkv, eps, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// V transpose: qkv[T, ..] V part -> Vt[hkv][128][t_pad]; one block per (32 padded slots, kv head)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void v_transpose_body(const u16 *qkv, u16 *vt, const int32_t *tok_of_pad, int64_t t_pad,
                                                 int hq, int hkv, int slot_block, int kvh_,
                                                 u16 (*tile)[CRAG_HEAD_DIM + 8]) {
    const int64_t p0 = (int64_t)slot_block * 32;
    const int kvh = kvh_;
    const int64_t row_stride = (int64_t)(hq + 2 * hkv) * CRAG_HEAD_DIM;
    {
        const int slot = threadIdx.x >> 3, c8 = threadIdx.x & 7;  // 32 slots x 8 chunks of 16 elements
        const int32_t tok = (p0 + slot < t_pad) ? tok_of_pad[p0 + slot] : -1;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int d0 = c8 * 16 + half * 8;
            Pack8 a;
#pragma unroll
            for (int e = 0; e < 8; ++e) a.v[e] = 0;
            if (tok >= 0)
                a = *reinterpret_cast<const Pack8 *>(qkv + (int64_t)tok * row_stride +
                                                     (int64_t)(hq + hkv + kvh) * CRAG_HEAD_DIM + d0);
#pragma unroll
            for (int e = 0; e < 8; ++e) tile[slot][d0 + e] = a.v[e];
        }
    }
    __syncthreads();
    {
        // each thread writes 16 slots (32 B) of one d row: 128 d rows x 2 halves = 256 threads.
        // Inside a 32-slot block the slots are stored in PV-fragment order (see attention_kernel, crag_attention.hip): stored
        // index 16 s2 + 8 h + 4 g + r holds slot 16 s2 + 8 g + 4 h + r, so that the 8 keys one lane feeds
        // to one PV MFMA are 16 contiguous bytes.
        const int d = threadIdx.x >> 1, half = threadIdx.x & 1;
        u16 *dst = vt + ((int64_t)kvh * CRAG_HEAD_DIM + d) * t_pad + p0 + half * 16;
        Pack8 o0, o1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o0.v[e] = tile[half * 16 + 8 * (e >> 2) + (e & 3)][d];      // h = 0
            o1.v[e] = tile[half * 16 + 8 * (e >> 2) + 4 + (e & 3)][d];  // h = 1
        }
        reinterpret_cast<Pack8 *>(dst)[0] = o0;
        reinterpret_cast<Pack8 *>(dst)[1] = o1;
    }
}

__global__ __launch_bounds__(256) void v_transpose_kernel(const u16 *qkv, u16 *vt, const int32_t *tok_of_pad,
                                                          int64_t t_pad, int hq, int hkv) {
    __shared__ u16 tile[32][CRAG_HEAD_DIM + 8];
    v_transpose_body(qkv, vt, tok_of_pad, t_pad, hq, hkv, blockIdx.x, blockIdx.y, tile);
}

// Both in ONE launch (they touch disjoint columns of the fused qkv rows: q|k in place, v -> V^T): blocks
// [0, rope_blocks) walk the tokens, the rest are the (slot block, kv head) tiles of the transpose.  At 16 tokens a
// decoder layer is eight launches of a few microseconds each; every boundary removed is ~4 us of 80.
__global__ __launch_bounds__(256) void qk_rope_vt_kernel(u16 *qkv, const u16 *qw, const u16 *kw, const float *cos_sin,
                                                         const int32_t *positions, int64_t n_tokens, int hq, int hkv,
                                                         float eps, u16 *vt, const int32_t *tok_of_pad, int64_t t_pad,
                                                         int rope_blocks) {
    __shared__ u16 tile[32][CRAG_HEAD_DIM + 8];
    if ((int)blockIdx.x < rope_blocks) {
        qk_norm_rope_body(qkv, qw, kw, cos_sin, positions, n_tokens, hq, hkv, eps, blockIdx.x, rope_blocks);
    } else {
        const int b = (int)blockIdx.x - rope_blocks;
        v_transpose_body(qkv, vt, tok_of_pad, t_pad, hq, hkv, b / hkv, b % hkv, tile);
    }
}

// ---------------------------------------------------------------------------------------------
// SwiGLU
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swiglu_kernel(const u16 *gu, u16 *out, int64_t rows, int inter) {
    // one row per block trip, 16-byte chunks across the threads: no index division, all loads of a trip in flight
    const int chunks = inter >> 3;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const Pack8 *gp = reinterpret_cast<const Pack8 *>(gu + r * 2 * inter);
        const Pack8 *up = reinterpret_cast<const Pack8 *>(gu + r * 2 * inter + inter);
        Pack8 *op = reinterpret_cast<Pack8 *>(out + r * inter);
        for (int c0 = threadIdx.x; c0 < chunks; c0 += 4 * 256) {
            Pack8 g[4], u[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q * 256;
                if (c < chunks) {
                    g[q] = gp[c];
                    u[q] = up[c];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q * 256;
                if (c < chunks) {
                    Pack8 o;
                    float lowest = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float x = bf2f(g[q].v[e]);
                        lowest = fminf(lowest, x);
                        const float act = bf2f(f2bf(x / (1.f + __expf(-x))));  // silu in fp32, rounded to bf16 like the model
                        o.v[e] = f2bf(act * bf2f(u[q].v[e]));
                    }
                    // Gates of -89 and below (the bf16 values past -88.5): exp(-x) is +inf in fp32 and the quotient -0,
                    // while silu(x) is still a normal number down to -92 (-2e-37 at -89).  There 1 + e^-x is e^-x, so
                    // silu = x e^x, with e^x taken 2^64 too large so that it is no denormal (-inf: -inf * 0 = NaN, as the
                    // quotient).  One test per chunk, and the chunk read again inside it: nothing of this stays in
                    // registers on the path of the chunks that hold no such gate.
                    if (lowest <= -89.f) {
                        const Pack8 g2 = gp[c], u2 = up[c];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float x = bf2f(g2.v[e]);
                            if (x <= -89.f) {
                                const float act = bf2f(f2bf(x * __expf(x + 44.3614196f) * 0x1p-64f));  // 64 ln 2
                                o.v[e] = f2bf(act * bf2f(u2.v[e]));
                            }
                        }
                    }
                    op[c] = o;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// pooling + final norm + slice + L2 normalise (one block per sequence)
// ---------------------------------------------------------------------------------------------
// `delta` (nullable, mode 0): the last sub-block's output, added to the residual stream for the pooled rows only
// (bf16 add, as the model's `hidden + mlp(...)`), instead of a pass over every token just to pool one per sequence.
// `rows` (nullable, mode 0): the pooled row of sequence b is rows[b] instead of the sequence's last row (a graph replay
// pools at the real last token of every padded sequence: data, not shape).
__global__ __launch_bounds__(256) void pool_normalize_kernel(const u16 *hs, const u16 *delta, const u16 *w, const int32_t *cu,
                                                             const int64_t *rows, float *out, int hidden, int out_dim,
                                                             int mode, float eps) {
    __shared__ float sh[4];
    __shared__ float row[8192];
    const int b = blockIdx.x;
    const int t0 = rows ? (int)rows[b] : cu[b], t1 = rows ? t0 + 1 : cu[b + 1];
    if (t1 <= t0) {
        for (int i = threadIdx.x; i < out_dim; i += blockDim.x) out[(int64_t)b * out_dim + i] = 0.f;
        return;
    }
    if (mode == 0) {  // last token of the residual stream, final RMSNorm applied here
        const u16 *x = hs + (int64_t)(t1 - 1) * hidden;
        const u16 *dl = delta ? delta + (int64_t)(t1 - 1) * hidden : nullptr;
        float ss = 0.f;
        for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
            const float v = dl ? bf2f(f2bf(bf2f(x[i]) + bf2f(dl[i]))) : bf2f(x[i]);
            row[i] = v;
            ss += v * v;
        }
        ss = block_sum(ss, sh);
        const float rstd = rsqrtf(ss / (float)hidden + eps);
        for (int i = threadIdx.x; i < hidden; i += blockDim.x)
            row[i] = bf2f(f2bf(bf2f(w[i]) * bf2f(f2bf(row[i] * rstd))));
    } else {  // mean over the (already normed) tokens
        const float invn = 1.f / (float)(t1 - t0);
        for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
            float acc = 0.f;
            for (int t = t0; t < t1; ++t) acc += bf2f(hs[(int64_t)t * hidden + i]);
            row[i] = acc * invn;
        }
    }
    __syncthreads();
    float ss = 0.f;
    for (int i = threadIdx.x; i < out_dim; i += blockDim.x) ss += row[i] * row[i];
    ss = block_sum(ss, sh);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);  // RUNBOOK:510-513 max(norm, 1e-12)
    for (int i = threadIdx.x; i < out_dim; i += blockDim.x) out[(int64_t)b * out_dim + i] = row[i] * inv;
}


// ---------------------------------------------------------------------------------------------
// Skinny GEMM: out[M, N] = x[M, K] @ W[N, K]^T for M <= 32 tokens -- the encoder at the reference's own operating
// point, ONE query per /retrieve request (retrieve.py:427).  At that size a linear layer is a WEIGHT STREAM (202 MB of
// bf16 weights per decoder layer against 16-32 rows of activations): HBM bound, 25 us per layer at 8 TB/s, where the
// library's GEMM kernels for 16 rows measured ~1 TB/s (profiles/r03_small_encode_kernel_stats.csv).
//   * weights are stored a second time in MFMA A-fragment order (Qwen3Encoder._small_weights):
//     wsw[n_tile of 16 rows][k-step of 32][lane = 16 (k/8) + row][8 bf16], so a wave-instruction reads 1 KiB of
//     contiguous HBM and the loaded registers ARE the A operand of v_mfma_f32_16x16x32_bf16 (rows = output features);
//   * the activations are the B operand (columns = tokens), each wave keeps the fragments of ITS K range in registers
//     for the whole kernel (x is 80-300 KB, L2 resident); the K dimension is split over the WAVES waves of a workgroup,
//     the partial 16x16 tiles are summed through LDS in wave order (deterministic);
//   * a workgroup owns NT n-tiles; its waves keep 12 weight loads (12 KiB per wave) in flight;
//   * EPI = 1: the rows of an n-tile are 8 gate rows followed by the 8 up rows of the same features (weights
//     interleaved that way), and the epilogue writes silu(gate) * up with the model's bf16 roundings (gate and up
//     rounded to bf16 as a linear layer's output would be, silu in fp32 rounded to bf16, product rounded to bf16).
// ---------------------------------------------------------------------------------------------
struct SkinnyParams {
    const u16 *x;    // [16 * MG, K] bf16, rows >= m_rows are padding (never stored)
    const u16 *wsw;  // fragment-ordered weights
    u16 *out;        // [m_rows, ld_out] bf16
    int m_rows, n, k, ld_out;
};

template <int MG, int NT, int KS, int WAVES, int EPI>
__global__ __launch_bounds__(WAVES * 64) void skinny_gemm_kernel(SkinnyParams p) {
    __shared__ f32x4_t red[WAVES][NT][MG][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ksteps = p.k >> 5;
    const int kw0 = w * KS;  // first k-step of this wave
    // activations: B[k = 8 (lane >> 4) + j][col = lane & 15] = x[token 16 mg + (lane & 15)][32 (kw0 + s) + 8 (lane >> 4) + j]
    bf16x8 xb[MG][KS];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
        const u16 *xr = p.x + (size_t)(16 * mg + (lane & 15)) * p.k + (size_t)kw0 * 32 + 8 * (lane >> 4);
#pragma unroll
        for (int s = 0; s < KS; ++s) xb[mg][s] = *reinterpret_cast<const bf16x8 *>(xr + 32 * s);
    }
    constexpr int TOT = NT * KS, D = TOT < 12 ? TOT : 12;
    const u16 *wbase = p.wsw + ((size_t)blockIdx.x * NT * ksteps + (size_t)kw0) * 512 + lane * 8;
    auto wptr = [&](int idx) -> const bf16x8 * {
        const int nt = idx / KS, s = idx % KS;
        return reinterpret_cast<const bf16x8 *>(wbase + ((size_t)nt * ksteps + s) * 512);
    };
    bf16x8 wr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) wr[i] = __builtin_nontemporal_load(wptr(i));
    f32x4_t acc[NT][MG];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) acc[nt][mg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TOT; ++i) {
        const int nt = i / KS, s = i % KS;
        const bf16x8 wv = wr[i % D];
        if (i + D < TOT) wr[i % D] = __builtin_nontemporal_load(wptr(i + D));
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
            acc[nt][mg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv, xb[mg][s], acc[nt][mg], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) red[w][nt][mg][lane] = acc[nt][mg];
    __syncthreads();
    // D[row = 4 (lane >> 4) + reg][col = lane & 15]: a (tile, token group, lane) unit = 4 consecutive features of one token
    constexpr int UNITS = NT * MG * 64;
    for (int u = threadIdx.x; u < UNITS; u += WAVES * 64) {
        const int l = u & 63, mg = (u >> 6) % MG, nt = (u >> 6) / MG;
        const int token = 16 * mg + (l & 15);
        if (EPI == 1 && l >= 32) continue;  // the up half is consumed by the thread of its gate half
        f32x4_t sum = red[0][nt][mg][l];
#pragma unroll
        for (int ww = 1; ww < WAVES; ++ww) sum += red[ww][nt][mg][l];
        if (token >= p.m_rows) continue;
        const int tile = (int)blockIdx.x * NT + nt;
        if (EPI == 0) {
            u16 o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = f2bf(sum[r]);
            *reinterpret_cast<uint2 *>(p.out + (size_t)token * p.ld_out + 16 * tile + 4 * (l >> 4)) =
                make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
        } else {
            f32x4_t up = red[0][nt][mg][l + 32];
#pragma unroll
            for (int ww = 1; ww < WAVES; ++ww) up += red[ww][nt][mg][l + 32];
            u16 o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float g = bf2f(f2bf(sum[r]));
                const float act = bf2f(f2bf(g / (1.f + __expf(-g))));
                o[r] = f2bf(act * bf2f(f2bf(up[r])));
            }
            *reinterpret_cast<uint2 *>(p.out + (size_t)token * p.ld_out + 8 * tile + 4 * (l >> 4)) =
                make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
        }
    }
}

}  // namespace

extern "C" {

int crag_enc_embed_gather(const int32_t *ids, const uint16_t *table, uint16_t *out, int64_t n_tokens, int hidden,
                          int64_t vocab, void *stream) {
    if (!ids || !table || !out) return efail("embed_gather: NULL pointer");
    if (hidden <= 0 || (hidden & 7) || vocab <= 0 || n_tokens < 0) return efail("embed_gather: bad sizes");
    if (n_tokens == 0) return 0;
    const unsigned grid = (unsigned)(n_tokens < 65535 * 16 ? n_tokens : 65535 * 16);
    hipLaunchKernelGGL(embed_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ids, table, out, n_tokens,
                       hidden, vocab);
    return hip_ok("embed_gather");
}

int crag_enc_rmsnorm(const uint16_t *x, const uint16_t *residual_in, const uint16_t *weight, uint16_t *out,
                     uint16_t *residual_out, int64_t rows, int hidden, float eps, void *stream) {
    if (!x || !weight || !out) return efail("rmsnorm: NULL pointer");
    if (hidden <= 0 || (hidden & 7) || hidden > 8 * NORM_THREADS * NORM_MAX_CHUNKS)
        return efail("rmsnorm: hidden must be a multiple of 8 and <= %d (got %d)", 8 * NORM_THREADS * NORM_MAX_CHUNKS, hidden);
    if (rows <= 0) return 0;
    const unsigned grid = (unsigned)(rows < 1048576 ? rows : 1048576);
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(grid), dim3(NORM_THREADS), 0, (hipStream_t)stream, x, residual_in, weight,
                       out, residual_out, rows, hidden, eps);
    return hip_ok("rmsnorm");
}

int crag_enc_qk_norm_rope(uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w, const float *cos_sin,
                          const int32_t *positions, int64_t n_tokens, int hq, int hkv, float eps, void *stream) {
    if (!qkv || !q_norm_w || !k_norm_w || !cos_sin || !positions) return efail("qk_norm_rope: NULL pointer");
    if (hq <= 0 || hkv <= 0) return efail("qk_norm_rope: bad head counts");
    if (n_tokens <= 0) return 0;
    const unsigned grid = (unsigned)(n_tokens < 65536 * 16 ? n_tokens : 65536 * 16);
    hipLaunchKernelGGL(qk_norm_rope_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, qkv,
                       q_norm_w, k_norm_w, cos_sin, positions, n_tokens, hq, hkv, eps);
    return hip_ok("qk_norm_rope");
}

int crag_enc_v_transpose(const uint16_t *qkv, uint16_t *vt, const int32_t *tok_of_pad, int64_t t_pad, int hq, int hkv,
                         void *stream) {
    if (!qkv || !vt || !tok_of_pad) return efail("v_transpose: NULL pointer");
    if (t_pad <= 0 || (t_pad & 31)) return efail("v_transpose: t_pad must be a positive multiple of 32");
    hipLaunchKernelGGL(v_transpose_kernel, dim3((unsigned)(t_pad / 32), (unsigned)hkv), dim3(256), 0,
                       (hipStream_t)stream, qkv, vt, tok_of_pad, t_pad, hq, hkv);
    return hip_ok("v_transpose");
}

int crag_enc_qk_rope_vt(uint16_t *qkv, const uint16_t *q_norm_w, const uint16_t *k_norm_w, const float *cos_sin,
                        const int32_t *positions, int64_t n_tokens, int hq, int hkv, float eps, uint16_t *vt,
                        const int32_t *tok_of_pad, int64_t t_pad, void *stream) {
    if (!qkv || !q_norm_w || !k_norm_w || !cos_sin || !positions || !vt || !tok_of_pad) return efail("qk_rope_vt: NULL pointer");
    if (hq <= 0 || hkv <= 0) return efail("qk_rope_vt: bad head counts");
    if (t_pad <= 0 || (t_pad & 31)) return efail("qk_rope_vt: t_pad must be a positive multiple of 32");
    if (n_tokens <= 0) return 0;
    const int rope_blocks = (int)(n_tokens < 65536 ? n_tokens : 65536);
    const unsigned grid = (unsigned)rope_blocks + (unsigned)(t_pad / 32) * (unsigned)hkv;
    hipLaunchKernelGGL(qk_rope_vt_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, qkv, q_norm_w, k_norm_w,
                       cos_sin, positions, n_tokens, hq, hkv, eps, vt, tok_of_pad, t_pad, rope_blocks);
    return hip_ok("qk_rope_vt");
}

int crag_enc_swiglu(const uint16_t *gate_up, uint16_t *out, int64_t rows, int inter, void *stream) {
    if (!gate_up || !out) return efail("swiglu: NULL pointer");
    if (inter <= 0 || (inter & 7)) return efail("swiglu: inter must be a positive multiple of 8");
    if (rows <= 0) return 0;
    const unsigned grid = (unsigned)(rows < 65536 * 16 ? rows : 65536 * 16);
    hipLaunchKernelGGL(swiglu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, gate_up, out, rows, inter);
    return hip_ok("swiglu");
}

int crag_enc_pool_normalize(const uint16_t *hidden_states, const uint16_t *final_norm_w, const int32_t *cu_seqlens,
                            float *out, int n_seqs, int hidden, int out_dim, int mode, float eps, void *stream) {
    return crag_enc_pool_normalize_add(hidden_states, nullptr, final_norm_w, cu_seqlens, out, n_seqs, hidden, out_dim,
                                       mode, eps, stream);
}

int crag_enc_pool_normalize_add(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                                const int32_t *cu_seqlens, float *out, int n_seqs, int hidden, int out_dim, int mode,
                                float eps, void *stream) {
    if (!hidden_states || !cu_seqlens || !out) return efail("pool_normalize: NULL pointer");
    if (mode == 0 && !final_norm_w) return efail("pool_normalize: last-token mode needs the final norm weight");
    if (delta && mode != 0) return efail("pool_normalize: a delta is only added in last-token mode");
    if (hidden <= 0 || hidden > 8192 || out_dim <= 0 || out_dim > hidden) return efail("pool_normalize: bad sizes");
    if (n_seqs <= 0) return 0;
    hipLaunchKernelGGL(pool_normalize_kernel, dim3((unsigned)n_seqs), dim3(256), 0, (hipStream_t)stream, hidden_states,
                       delta, final_norm_w, cu_seqlens, (const int64_t *)nullptr, out, hidden, out_dim, mode, eps);
    return hip_ok("pool_normalize");
}

int crag_enc_pool_normalize_rows(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                                 const int64_t *rows, float *out, int n_seqs, int hidden, int out_dim, float eps,
                                 void *stream) {
    if (!hidden_states || !final_norm_w || !rows || !out) return efail("pool_normalize_rows: NULL pointer");
    if (hidden <= 0 || hidden > 8192 || out_dim <= 0 || out_dim > hidden) return efail("pool_normalize_rows: bad sizes");
    if (n_seqs <= 0) return 0;
    hipLaunchKernelGGL(pool_normalize_kernel, dim3((unsigned)n_seqs), dim3(256), 0, (hipStream_t)stream, hidden_states,
                       delta, final_norm_w, (const int32_t *)nullptr, rows, out, hidden, out_dim, 0, eps);
    return hip_ok("pool_normalize_rows");
}

int crag_enc_skinny_gemm(const uint16_t *x, const uint16_t *wsw, uint16_t *out, int m_rows, int m_pad, int n, int k,
                         int epilogue, void *stream) {
    if (!x || !wsw || !out) return efail("skinny_gemm: NULL pointer");
    if (m_rows <= 0 || m_rows > m_pad || (m_pad != 16 && m_pad != 32)) return efail("skinny_gemm: m_pad must be 16 or 32 and m_rows <= m_pad");
    if (epilogue != 0 && epilogue != 1) return efail("skinny_gemm: epilogue must be 0 or 1");
    if (n <= 0 || (n & 15)) return efail("skinny_gemm: n must be a positive multiple of 16");
    SkinnyParams p;
    p.x = x;
    p.wsw = wsw;
    p.out = out;
    p.m_rows = m_rows;
    p.n = n;
    p.k = k;
    p.ld_out = epilogue ? n / 2 : n;
    const int tiles = n / 16;
    hipStream_t st = (hipStream_t)stream;
#define CRAG_SKINNY(MG_, NT_, KS_, WAVES_, EPI_)                                                              \
    hipLaunchKernelGGL((skinny_gemm_kernel<MG_, NT_, KS_, WAVES_, EPI_>), dim3((unsigned)(tiles / NT_)),      \
                       dim3(WAVES_ * 64), 0, st, p)
    const int mg = m_pad / 16;
    // n-tiles per workgroup (NT): a workgroup reads the activations of its K range once per NT tiles, but tiles / NT
    // workgroups must still cover the chip -- measured per shape (scripts/probes/skinny_bench.py): two tiles for the
    // wide projections (qkv 10.1 vs 10.7 us, gate|up 22.4 vs 23.1 with four), one for o and down (160 n-tiles: with
    // two tiles per workgroup only 80 CUs work, 12.3 vs 8.4 us and 24.1 vs 16.7)
    if (k == 2560 && epilogue == 0) {
        if (tiles & 1) return efail("skinny_gemm: n / 16 must be even for k = 2560");
        if (mg == 1) CRAG_SKINNY(1, 2, 10, 8, 0); else CRAG_SKINNY(2, 2, 10, 8, 0);
    } else if (k == 2560 && epilogue == 1) {
        if (tiles & 1) return efail("skinny_gemm: the SwiGLU form needs an even number of n-tiles");
        if (mg == 1) CRAG_SKINNY(1, 2, 10, 8, 1); else CRAG_SKINNY(2, 2, 10, 8, 1);
    } else if (k == 4096 && epilogue == 0) {
        if (mg == 1) CRAG_SKINNY(1, 1, 16, 8, 0); else CRAG_SKINNY(2, 1, 16, 8, 0);
    } else if (k == 9728 && epilogue == 0) {
        if (mg == 1) CRAG_SKINNY(1, 1, 38, 8, 0); else CRAG_SKINNY(2, 1, 19, 16, 0);
    } else {
        return efail("skinny_gemm: unsupported shape k=%d epilogue=%d (built for the Qwen3-Embedding-4B widths: k = 2560 / 4096 / 9728)", k, epilogue);
    }
#undef CRAG_SKINNY
    return hip_ok("skinny_gemm");
}

}  // extern "C"
