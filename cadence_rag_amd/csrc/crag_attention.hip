// crag_attention.hip — causal GQA flash attention of the encoder lane for gfx950 (bf16 MFMA, head_dim 128).
// C ABI: include/crag_encoder.h.
//
//   crag_enc_attention           every sequence of the packed batch attends to its own keys, causally.
//   crag_enc_attention_prefixed  a sequence may name a PARENT segment of the same packed batch: its queries see every
//                                key of the parent, then their own keys causally.  The 40-80 (query, document) pairs
//                                of one rerank request share their first 60-100 tokens (system prompt, instruction,
//                                query); the shared tokens run once, as a root segment, and every document segment
//                                attends to it.
//
// One workgroup per (kv head, 32-row q block), one wave = 32 query rows of one query head:
//   S^T = K . Q^T   (A = K tile rows, B = Q^T)   -> lane holds 16 of the 32 keys of ONE query row
//   O^T += V^T . P^T (A = V^T tile from the transposed copy, B = P^T taken straight from the S^T
//                     accumulator registers, bf16-packed; k order as the 32x32 C/D map gives it)
// Two kernels, one parameter struct, one staging layout, one pair of half-wave reductions:
//   attention_kernel<GROUP, PREFIXED>  32 keys per step; PREFIXED walks the parent's tiles first
//   attention_pair_kernel<GROUP>       64 keys per step (GROUP >= 4), plain launch only
// The index prologue and the output epilogue stand in both kernels as the same statements in the same order rather
// than as shared functions: every function form tried (struct by value or reference, scalars by value or reference,
// precomputed pointers) changed the instruction stream of one kernel or another, and the order of the statements is
// part of what keeps the generated code as measured (the compiler keeps the order of the loads).

#include <stdlib.h>
#include <type_traits>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

struct AttnParams {
    const u16 *qkv;
    const u16 *vt;
    u16 *out;
    const int32_t *cu, *cu_pad, *blk_seq, *blk_q0;
    int64_t t_pad;
    int hq, hkv;
    float scale_log2;
    const int32_t *parent;  // per sequence: index of its parent segment or -1; null for (and never read by) the plain launch
};

// The 4 (hq/hkv) waves of a workgroup are the query heads of one GQA group: they need the SAME K and V
// tiles.  Loading fragments straight from global memory uses 32 B of every 128-B line per instruction
// and repeats the traffic per wave, which makes the kernel L1-bound; instead the workgroup stages each
// 32-key tile once, fully coalesced, in LDS (double-buffered, one barrier per tile) and the waves read
// their MFMA fragments from there (rows padded to 272 / 80 bytes: conflict-free ds_read_b128).
// The V^T rows are read in the order v_transpose_body (crag_encoder.hip) writes them: inside a 32-slot block the 8
// keys one lane feeds to one PV MFMA are 16 contiguous bytes.
constexpr int ATT_KROW = 136;   // u16 per staged K row (128 + 8 pad)
constexpr int ATT_VROW = 40;    // u16 per staged V^T row (32 + 8 pad)
constexpr int ATT_VROW2 = 72;   // u16 per staged V^T row of a 64-key pair (64 + 8 pad)

// A lane holds keys 4h.. of ITS query row (c = lane & 31, h = lane >> 5): a row's 32 keys of a tile sit in lanes c and
// c + 32, combined by halfwave_max / halfwave_sum (crag_enc_common.h).

// ---- 32 keys per iteration.  PREFIXED selects where a key tile is fetched from (the parent's tiles first, then the
// sequence's own), how many tiles are walked and the mask; everything else is one text. ----
template <int GROUP, bool PREFIXED>
__global__ __launch_bounds__(64 * GROUP) __attribute__((amdgpu_waves_per_eu(GROUP >= 2 ? 2 : 1, 8)))
void attention_kernel(AttnParams p) {
    // one pool: K buffers, then V^T buffers; the epilogue reuses its start for the per-wave output tiles
    constexpr int K_BUF = 32 * ATT_KROW, V_BUF = CRAG_HEAD_DIM * ATT_VROW;
    static_assert(GROUP * 32 * ATT_KROW <= 2 * (K_BUF + V_BUF), "output tiles must fit the staging pool");
    __shared__ __attribute__((aligned(16))) u16 s_pool[2 * (K_BUF + V_BUF)];
    u16(*s_k)[K_BUF] = reinterpret_cast<u16(*)[K_BUF]>(s_pool);
    u16(*s_v)[V_BUF] = reinterpret_cast<u16(*)[V_BUF]>(s_pool + 2 * K_BUF);
    constexpr int nthr = 64 * GROUP;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // kv head on the fast grid axis: workgroups go to the 8 XCDs round-robin by linear id, so with 8 kv heads
    // every XCD serves ONE kv head and the q blocks that re-read a sequence's K/V tiles share that XCD's L2
    const int kvh = blockIdx.x;
    const int head = kvh * GROUP + wave;  // GROUP = query heads per kv head = waves per workgroup
    const int seq = p.blk_seq[blockIdx.y];
    const int q0 = p.blk_q0[blockIdx.y];
    const int s_begin = p.cu[seq];
    const int len = p.cu[seq + 1] - s_begin;
    // PREFIXED looks its parent up before the Q loads and reads cu_pad[seq] after them; the plain form does the
    // reverse.  Both orders are those of the kernels this template replaced, kept so that each instantiation's code is
    // what it was.  The plain instantiation never reads p.parent.
    int par = -1, p_begin = 0, plen = 0, n_pt = 0, n_kt = 0;  // n_kt: key tiles walked, the diagonal one last
    if constexpr (PREFIXED) {
        par = p.parent[seq];
        p_begin = par >= 0 ? p.cu[par] : 0;
        plen = par >= 0 ? p.cu[par + 1] - p_begin : 0;
        n_pt = (plen + 31) / 32;  // parent key tiles, walked first
        n_kt = n_pt + q0 / 32 + 1;
    }
    int64_t pad_base = 0;
    if constexpr (!PREFIXED) pad_base = p.cu_pad[seq];
    const int c = lane & 31, h = lane >> 5;
    const int64_t row_stride = (int64_t)(p.hq + 2 * p.hkv) * CRAG_HEAD_DIM;
    // Q^T fragments (B operand): B[k = 8h + j][col c] = Q[q0 + c][16 s + 8h + j]
    bf16x8 qf[8];
    {
        const u16 *qp = p.qkv + (int64_t)(s_begin + q0 + c) * row_stride + (int64_t)head * CRAG_HEAD_DIM + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = ld_frag(qp + 16 * s);
    }
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 oacc[4] = {zero, zero, zero, zero};
    float m = -INFINITY, l = 0.f;
    if constexpr (!PREFIXED) n_kt = q0 / 32 + 1;
    const u16 *kglob = p.qkv + (int64_t)s_begin * row_stride + (int64_t)(p.hq + kvh) * CRAG_HEAD_DIM;
    const u16 *vglob = p.vt + (int64_t)kvh * CRAG_HEAD_DIM * p.t_pad + (PREFIXED ? (int64_t)p.cu_pad[seq] : pad_base);
    // PREFIXED, tile kt < n_pt: keys 32 kt .. of the parent (its padded tail masked); after them the sequence's own tiles.
    // Key rows past a segment's end are rows of the next segment or of the 32 rows qkv extends past T, and their
    // V^T slots are the zero pads of the segment's 32-aligned range: read, then masked.
    const u16 *kpar = nullptr, *vpar = nullptr;
    if constexpr (PREFIXED) {
        kpar = p.qkv + (int64_t)p_begin * row_stride + (int64_t)(p.hq + kvh) * CRAG_HEAD_DIM;
        vpar = p.vt + (int64_t)kvh * CRAG_HEAD_DIM * p.t_pad + (par >= 0 ? p.cu_pad[par] : 0);
    }

    // cooperative staging: the K tile is 32 rows x 16 chunks of 16 B, the V^T tile 128 rows x 4 chunks; with
    // `nthr` threads every thread moves 512 / nthr chunks of each (nthr = 64 * group, group in {1, 2, 4})
    constexpr int per = 512 / nthr;
    struct Stage {
        bf16x8 k[per], v[per];
    };
    auto fetch = [&](int kt, Stage &st) {
        auto tile = [&](const u16 *const &kg, const u16 *const &vg, const int k0) {
#pragma unroll
            for (int i = 0; i < per; ++i) {
                const int ch = tid + i * nthr;
                st.k[i] = ld_frag(kg + (int64_t)(k0 + (ch >> 4)) * row_stride + 8 * (ch & 15));
                st.v[i] = ld_frag(vg + (int64_t)(ch >> 2) * p.t_pad + k0 + 8 * (ch & 3));
            }
        };
        if constexpr (PREFIXED) {
            const bool in_par = kt < n_pt;
            const int k0 = (in_par ? kt : kt - n_pt) * 32;
            const u16 *kg = in_par ? kpar : kglob;
            const u16 *vg = in_par ? vpar : vglob;
            tile(kg, vg, k0);
        } else {
            tile(kglob, vglob, kt * 32);
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
    // empty the compiler's vmcnt scoreboard: otherwise the loop keeps conservative waits on the Q fragment
    // loads above in every iteration and drains the prefetch issued at the top of each tile
    __builtin_amdgcn_s_waitcnt(0x0F70);

    for (int kt = 0; kt < n_kt; ++kt) {
        const int k0 = kt * 32, buf = kt & 1;
        if (kt + 1 < n_kt) fetch(kt + 1, st);  // in flight during this tile's MFMAs and softmax
        // all 8 K fragments first, then the MFMA chain: LDS latency is paid once, not per MFMA
        bf16x8 fr[8];
        {
            const u16 *kp = &s_k[buf][c * ATT_KROW + 8 * h];  // A[row = key c][k = 8h + j]
#pragma unroll
            for (int s = 0; s < 8; ++s) fr[s] = *reinterpret_cast<const bf16x8 *>(kp + 16 * s);
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 sacc = zero;
#pragma unroll
        for (int s = 0; s < 8; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[s], qf[s], sacc, 0, 0, 0);
        // V^T fragments into the same registers while the softmax runs:
        // A operand V^T[d = 32 dt + c][8 keys of (s2, h)], contiguous in the staged (PV-fragment) order
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                fr[2 * dt + s2] = *reinterpret_cast<const bf16x8 *>(&s_v[buf][(32 * dt + c) * ATT_VROW + 8 * h + 16 * s2]);
        __builtin_amdgcn_sched_barrier(0);
        // lane: query row q0 + c; register i: key r = (i&3) + 8*(i>>2) + 4h of the tile
        const bool diag = (kt == n_kt - 1);
        [[maybe_unused]] int lim = 32;  // PREFIXED: the visible keys of this tile for query row q0 + c are those with r < lim
        if constexpr (PREFIXED) {
            // parent tile: all of the parent's keys;  own tile: causal on the diagonal tile, all before it
            if (kt < n_pt) lim = plen - kt * 32;
            else lim = diag ? q0 + c - (kt - n_pt) * 32 + 1 : 32;
        }
        float sv[16];
        float mloc = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
            float v = sacc[i] * p.scale_log2;
            // the two mask forms are not bit-identical on a root-only batch: the plain form lets the compiler split the
            // loop on `diag` and contract scale * s - m into one fma in the copy without a mask, this one does not
            if constexpr (PREFIXED) {
                if (r >= lim) v = -INFINITY;
            } else {
                const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (diag && key > q0 + c) v = -INFINITY;
            }
            sv[i] = v;
            mloc = fmaxf(mloc, v);
        }
        mloc = halfwave_max(mloc);
        // finite from the first tile on: key 0 of the sequence (<= q0 + c) is never masked and, PREFIXED, neither is
        // key 0 of the parent (plen >= 1)
        const float mnew = fmaxf(m, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sv[i] = __builtin_amdgcn_exp2f(sv[i] - mnew);
            lsum += sv[i];
        }
        l = l * alpha + halfwave_sum(lsum);
        if (__any(mnew != m)) {  // wave-uniform: once the running maxima have settled no rescale is needed
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
        }
        m = mnew;
        // P^T fragments (B operand of k-step s2): element j = register 8*s2 + j
        bf16x8 pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pf[s2][jj] = (short)f2bf(sv[8 * s2 + jj]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)  // 4 independent accumulator chains
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2 * dt + s2], pf[s2], oacc[dt], 0, 0, 0);
        if (kt + 1 < n_kt) stash(buf ^ 1, st);  // that buffer was last read in tile kt-1, before the previous barrier
        __syncthreads();
    }
    // O[q0 + c][32 dt + (i&3) + 8 (i>>2) + 4h] = oacc[dt][i] / l.  Stored straight from these registers a wave
    // instruction would write 16 bytes into each of 32 rows (partial lines: 40 % of the kernel's time at
    // 256-token chunks); instead the wave transposes its 32 x 128 tile through LDS (the K staging buffer is free
    // after the last barrier) and writes whole 256-byte rows, 16 bytes per lane.
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
        // same wave, LDS operations complete in order: no barrier between these writes and the reads below
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

// ---- 64 keys per iteration (GROUP >= 4): two 32-key tiles share one softmax update, one barrier and one
// staging round, and their QK chains interleave.  A q block with an odd number of key tiles ends with a
// half pair (HALF): only its first tile exists (its second would lie entirely above the diagonal). ----
template <int GROUP>
__global__ __launch_bounds__(64 * GROUP) __attribute__((amdgpu_waves_per_eu(2, 8)))
void attention_pair_kernel(AttnParams p) {
    static_assert(GROUP >= 4, "staging is sized for at least 256 threads");
    // one pool: K buffers, then V^T buffers; the epilogue reuses its start for the per-wave output tiles
    constexpr int K_BUF = 64 * ATT_KROW, V_BUF = CRAG_HEAD_DIM * ATT_VROW2;
    static_assert(GROUP * 32 * ATT_KROW <= 2 * (K_BUF + V_BUF), "output tiles must fit the staging pool");
    __shared__ __attribute__((aligned(16))) u16 s_pool[2 * (K_BUF + V_BUF)];
    u16(*s_k)[K_BUF] = reinterpret_cast<u16(*)[K_BUF]>(s_pool);
    u16(*s_v)[V_BUF] = reinterpret_cast<u16(*)[V_BUF]>(s_pool + 2 * K_BUF);
    constexpr int nthr = 64 * GROUP;
    constexpr int per = 1024 / nthr;  // 16-byte chunks of K and of V^T per thread and pair
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int kvh = blockIdx.x;
    const int head = kvh * GROUP + wave;
    const int seq = p.blk_seq[blockIdx.y];
    const int q0 = p.blk_q0[blockIdx.y];
    const int s_begin = p.cu[seq];
    const int len = p.cu[seq + 1] - s_begin;
    const int64_t pad_base = p.cu_pad[seq];
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
    const int n_kt = q0 / 32 + 1;          // 32-key tiles up to and including the diagonal one
    const int n_pairs = (n_kt + 1) >> 1;
    const bool last_half = (n_kt & 1) != 0;
    const u16 *kglob = p.qkv + (int64_t)s_begin * row_stride + (int64_t)(p.hq + kvh) * CRAG_HEAD_DIM;
    const u16 *vglob = p.vt + (int64_t)kvh * CRAG_HEAD_DIM * p.t_pad + pad_base;

    struct Stage {
        bf16x8 k[per], v[per];
    };
    // K pair: 64 rows x 16 chunks; V^T pair: 128 rows x 8 chunks.  A half pair moves only the first tile.
    // per-thread bases computed once; chunk i and pair pr only add wave-uniform offsets
    const u16 *kthr = kglob + (int64_t)(tid >> 4) * row_stride + 8 * (tid & 15);
    const u16 *vthr = vglob + (int64_t)(tid >> 3) * p.t_pad + 8 * (tid & 7);
    const int64_t kstep = (int64_t)(nthr >> 4) * row_stride, vstep = (int64_t)(nthr >> 3) * p.t_pad;
    auto fetch = [&](int pr, bool half, Stage &st) {
        const u16 *kp = kthr + (int64_t)(pr * 64) * row_stride;
        const u16 *vp = vthr + pr * 64;
#pragma unroll
        for (int i = 0; i < per; ++i) {
            // K rows (tid >> 4) + i * nthr / 16: the second tile's rows are i >= per / 2; V^T columns 8 * (tid & 7)
            if (!(half && i >= per / 2)) st.k[i] = ld_frag(kp + i * kstep);
            if (!(half && (tid & 7) >= 4)) st.v[i] = ld_frag(vp + i * vstep);
        }
    };
    auto stash = [&](int buf, const Stage &st) {
#pragma unroll
        for (int i = 0; i < per; ++i) {
            const int ch = tid + i * nthr;
            *reinterpret_cast<bf16x8 *>(&s_k[buf][(ch >> 4) * ATT_KROW + 8 * (ch & 15)]) = st.k[i];
            *reinterpret_cast<bf16x8 *>(&s_v[buf][(ch >> 3) * ATT_VROW2 + 8 * (ch & 7)]) = st.v[i];
        }
    };
    Stage st;
#pragma unroll
    for (int i = 0; i < per; ++i) st.k[i] = st.v[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    fetch(0, n_pairs == 1 && last_half, st);
    stash(0, st);
    __syncthreads();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // clean vmcnt scoreboard at the loop head (see attention_kernel)

    // one pair of key tiles; HALF: only the first tile; DIAG: the pair's last existing tile is the diagonal one
    auto pair = [&](int pr, auto HALF_, auto DIAG_) {
        constexpr bool HALF = decltype(HALF_)::value, DIAG = decltype(DIAG_)::value;
        const int k0 = pr * 64, buf = pr & 1;
        if (pr + 1 < n_pairs) fetch(pr + 1, (pr + 2 == n_pairs) && last_half, st);
        f32x16 sa = zero, sb = zero;
        {
            const u16 *kp = &s_k[buf][c * ATT_KROW + 8 * h];
#pragma unroll
            for (int half4 = 0; half4 < 2; ++half4) {  // 4 k-steps of both tiles per round: 8 fragments in flight
                bf16x8 fa[4], fb[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    fa[s] = *reinterpret_cast<const bf16x8 *>(kp + 16 * (4 * half4 + s));
                    if constexpr (!HALF) fb[s] = *reinterpret_cast<const bf16x8 *>(kp + 32 * ATT_KROW + 16 * (4 * half4 + s));
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s], qf[4 * half4 + s], sa, 0, 0, 0);
                    if constexpr (!HALF) sb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[s], qf[4 * half4 + s], sb, 0, 0, 0);
                }
            }
        }
        // V^T fragments of the first tile are requested now and arrive during the softmax
        bf16x8 fv[8];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                fv[2 * dt + s2] = *reinterpret_cast<const bf16x8 *>(&s_v[buf][(32 * dt + c) * ATT_VROW2 + 8 * h + 16 * s2]);
        __builtin_amdgcn_sched_barrier(0);
        // lane: query row q0 + c; register i of tile t: key k0 + 32 t + (i&3) + 8*(i>>2) + 4h
        // the softmax scale is positive, so the row maximum is taken on the raw scores and the scale is folded
        // into the exponent's fma: p = exp2(s * scale - m), m = scale * max(s)
        float mloc = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (DIAG && HALF && key > q0 + c) sa[i] = -INFINITY;
            mloc = fmaxf(mloc, sa[i]);
            if constexpr (!HALF) {
                if (DIAG && key + 32 > q0 + c) sb[i] = -INFINITY;
                mloc = fmaxf(mloc, sb[i]);
            }
        }
        mloc = halfwave_max(mloc);
        const float mnew = fmaxf(m, mloc * p.scale_log2);  // finite: key k0 (<= q0 + c) is never masked
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sa[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(sa[i], p.scale_log2, -mnew));
            lsum += sa[i];
            if constexpr (!HALF) {
                sb[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(sb[i], p.scale_log2, -mnew));
                lsum += sb[i];
            }
        }
        l = l * alpha + halfwave_sum(lsum);
        if (__any(mnew != m)) {  // wave-uniform: once the running maxima have settled no rescale is needed
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
        }
        m = mnew;
        bf16x8 pa[2], pb[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                pa[s2][jj] = (short)f2bf(sa[8 * s2 + jj]);
                if constexpr (!HALF) pb[s2][jj] = (short)f2bf(sb[8 * s2 + jj]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)  // 4 independent accumulator chains
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fv[2 * dt + s2], pa[s2], oacc[dt], 0, 0, 0);
        if constexpr (!HALF) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    fv[2 * dt + s2] = *reinterpret_cast<const bf16x8 *>(&s_v[buf][(32 * dt + c) * ATT_VROW2 + 8 * h + 32 + 16 * s2]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fv[2 * dt + s2], pb[s2], oacc[dt], 0, 0, 0);
        }
        if (pr + 1 < n_pairs) stash(buf ^ 1, st);  // that buffer was last read one barrier ago
        __syncthreads();
    };

    for (int pr = 0; pr + 1 < n_pairs; ++pr) pair(pr, std::false_type{}, std::false_type{});
    if (last_half) pair(n_pairs - 1, std::true_type{}, std::true_type{});
    else pair(n_pairs - 1, std::false_type{}, std::true_type{});

    // the 32 x 128 output tile transposed through LDS and written as whole rows (see attention_kernel)
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

AttnParams attn_params(const uint16_t *qkv, const uint16_t *vt, uint16_t *out, const int32_t *cu_seqlens,
                       const int32_t *cu_pad, const int32_t *blk_seq, const int32_t *blk_q0, const int32_t *parent,
                       int64_t t_pad, int hq, int hkv, float scale) {
    AttnParams p;
    p.qkv = qkv;
    p.vt = vt;
    p.out = out;
    p.cu = cu_seqlens;
    p.cu_pad = cu_pad;
    p.blk_seq = blk_seq;
    p.blk_q0 = blk_q0;
    p.t_pad = t_pad;
    p.hq = hq;
    p.hkv = hkv;
    p.scale_log2 = scale * 1.4426950408889634f;  // log2(e): the kernels' exponentials are exp2
    p.parent = parent;
    return p;
}

}  // namespace

extern "C" {

int crag_enc_attention(const uint16_t *qkv, const uint16_t *vt, uint16_t *out, const int32_t *cu_seqlens,
                       const int32_t *cu_pad, const int32_t *blk_seq, const int32_t *blk_q0, int n_blocks,
                       int64_t t_pad, int hq, int hkv, float scale, void *stream) {
    if (!qkv || !vt || !out || !cu_seqlens || !cu_pad || !blk_seq || !blk_q0) return efail("attention: NULL pointer");
    if (hkv <= 0 || hq % hkv != 0 || (hq / hkv != 1 && hq / hkv != 2 && hq / hkv != 4 && hq / hkv != 8))
        return efail("attention: hq/hkv must be 1, 2, 4 or 8");
    if (n_blocks <= 0) return 0;
    if (n_blocks > 65535 * 64) return efail("attention: too many q blocks (%d)", n_blocks);
    const AttnParams p = attn_params(qkv, vt, out, cu_seqlens, cu_pad, blk_seq, blk_q0, nullptr, t_pad, hq, hkv, scale);
    const dim3 grid((unsigned)hkv, (unsigned)n_blocks);
    switch (hq / hkv) {
        case 1: hipLaunchKernelGGL((attention_kernel<1, false>), grid, dim3(64), 0, (hipStream_t)stream, p); break;
        case 2: hipLaunchKernelGGL((attention_kernel<2, false>), grid, dim3(128), 0, (hipStream_t)stream, p); break;
        case 4:
            if (getenv("CRAG_ATTN_SINGLE")) hipLaunchKernelGGL((attention_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, p);
            else hipLaunchKernelGGL(attention_pair_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
            break;
        default: hipLaunchKernelGGL(attention_pair_kernel<8>, grid, dim3(512), 0, (hipStream_t)stream, p); break;
    }
    return hip_ok("attention");
}

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
    const AttnParams p = attn_params(qkv, vt, out, cu_seqlens, cu_pad, blk_seq, blk_q0, parent, t_pad, hq, hkv, scale);
    const dim3 grid((unsigned)hkv, (unsigned)n_blocks);
    if (hq / hkv == 2) hipLaunchKernelGGL((attention_kernel<2, true>), grid, dim3(128), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((attention_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, p);
    return hip_ok("attention_prefixed");
}

}  // extern "C"
