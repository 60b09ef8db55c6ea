// crag_extend.hip — continue cached sequences with many tokens at once (gfx950).  C ABI: include/crag_encoder.h.
//
//   crag_enc_extend_attention   sequence b holds cache_len[b] tokens in its slot and gets new_len[b] new rows.  Two or
//                               three launches: prepare (q/k-norm + RoPE of every new row, the append of its key and
//                               value, the rotated q to scratch), flash attention of the new rows over the slot's
//                               cache rows 0 .. cache_len + i, read in place, and -- where a short suffix stands
//                               behind a long cache -- combine (the key splits of a query block in ascending order).
//
// The attention kernel is attention_kernel's (crag_attention.hip) walk: one workgroup per (kv head, 32-row query block
// of one sequence), one wave per query head of the kv head, 32-key tiles staged once per workgroup in LDS
// (double-buffered, one barrier per tile), S^T = K . Q^T and O^T += V^T . P^T on v_mfma_f32_32x32x16_bf16 with P^T taken
// from the S^T accumulator registers, fp32 online softmax.  What differs is where K and V come from: the cache rows
// [slot][kv head][max_len][128], V row-major.  The V tile is staged as it lies in memory, [32 keys][128 + 32 pad], and
// the V^T operand is read from that one image with ds_read_b64_tr_b16 (row stride 320 bytes: the four rows a 32-lane
// half reads fall 16 banks apart, 4 x 16 banks = all 64, conflict-free).
//
// A key row at or beyond the last key the query block may see is never loaded: its K and V chunks are staged as zeros.
//
// The key split.  A suffix of a few hundred rows is a handful of query blocks, each walking thousands of keys one tile
// behind the other.  A sequence with at most EXTEND_SPLIT_ROWS new rows therefore cuts the keys of a query block into
// splits of EXTEND_SPLIT keys, one workgroup each: a block with one split stores its output itself, a block with more
// leaves (m, l, unnormalised o) in fp32 per split and extend_combine_kernel sums them in ascending split order.  A
// sequence with more new rows has blocks enough and is never split.
//
// Nothing here depends on n_seqs, on the slot or on a launch size chosen at run time: whether a sequence is split and
// where follows from its own two lengths, a workgroup always walks its keys in ascending tiles of EXTEND_TILE with the
// same lanes, and the splits are summed in ascending order, so a sequence's output bits and the bits appended to its
// slot are a function of its own data alone.  No atomics.

#include <math.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

typedef short bf16x4 __attribute__((ext_vector_type(4)));

constexpr int EXTEND_MAX_SEQS = CRAG_DECODE_MAX_SEQS;
constexpr int EXTEND_BLOCK = CRAG_EXTEND_BLOCK;   // query rows per workgroup and wave
constexpr int EXTEND_TILE = CRAG_EXTEND_TILE;     // keys per step
constexpr int EXTEND_SPLIT = CRAG_EXTEND_SPLIT;   // keys per workgroup of a split query block
constexpr int EXTEND_SPLIT_ROWS = CRAG_EXTEND_SPLIT_ROWS;   // a sequence with more new rows than this is never split
constexpr int SPLIT_TILES = EXTEND_SPLIT / EXTEND_TILE;
constexpr int PART_O = EXTEND_BLOCK * CRAG_HEAD_DIM;   // floats of one partial o: (query block, head, split)
constexpr int PART_ML = EXTEND_BLOCK * 2;              // floats of its (m, l) pairs
static_assert(EXTEND_SPLIT % EXTEND_TILE == 0, "a split is whole tiles");
constexpr int PREP_THREADS = 256;
static_assert(PREP_THREADS == KV_APPEND_THREADS, "the prepare kernel is kv_append_row's workgroup");
constexpr int EXT_KROW = 136;                     // u16 per staged K row (128 + 8 pad: conflict-free ds_read_b128)
constexpr int EXT_VROW = 160;                     // u16 per staged V row (128 + 32 pad: conflict-free transposed reads)
static_assert(EXTEND_BLOCK == 32 && EXTEND_TILE == 32, "the MFMA maps below are those of 32 x 32 tiles");

// the host-validated per-sequence data travel as kernel arguments
struct ExtendSeqs {
    int32_t len[EXTEND_MAX_SEQS];     // tokens the slot holds
    int32_t n_new[EXTEND_MAX_SEQS];   // new rows
    int32_t row0[EXTEND_MAX_SEQS];    // first of them in qkv_new / out
    int32_t slot[EXTEND_MAX_SEQS];
    int32_t splits[EXTEND_MAX_SEQS];  // key splits of the sequence's last query block; 1: the sequence is not split
    int32_t part0[EXTEND_MAX_SEQS];   // its first (query block, split) pair in the partial arrays
};

struct ExtendParams {
    const u16 *qkv_new;   // [T_new, (hq + 2 hkv) * 128] raw projections
    const u16 *qw, *kw;   // [128]
    const float *cos_sin; // [max_pos, 64, 2]
    u16 *k_cache;         // [n_slots][hkv][max_len][128]
    u16 *v_cache;
    u16 *q_rot;           // workspace: [T_new][hq][128] bf16
    float *part_o;        // workspace: [(query block, split) pairs][hq][PART_O], in the accumulator's lane order
    float *part_ml;       // workspace: [(query block, split) pairs][hq][32 rows][2]
    u16 *out;             // [T_new, hq * 128]
    int hq, hkv, max_len;
    float eps, scale_log2;
    ExtendSeqs seqs;
};

// prepare: one workgroup per (new row, sequence) appends row i at position len + i (kv_append_row, crag_enc_common.h)
__global__ __launch_bounds__(PREP_THREADS) void extend_prepare_kernel(const ExtendParams p) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (i >= p.seqs.n_new[b]) return;   // (uniform)
    const int pos = p.seqs.len[b] + i, slot = p.seqs.slot[b];
    const int64_t t = (int64_t)p.seqs.row0[b] + i;
    kv_append_row(p.qkv_new + t * (p.hq + 2 * p.hkv) * CRAG_HEAD_DIM, p.qw, p.kw, p.cos_sin, p.k_cache, p.v_cache,
                  p.q_rot + t * p.hq * CRAG_HEAD_DIM, p.hq, p.hkv, p.max_len, slot, pos, p.eps);
}

// ds_read_b64_tr_b16: the 16 lanes of a group name a block of 4 rows x 16 columns (lane 4q + p: row q, columns 4p..) and
// lane i of the group receives column i, row q in element q.  EXEC must be all ones: every call below stands in
// workgroup-uniform control flow.
__device__ __forceinline__ bf16x4 ld_tr(const u16 *lds) {
    typedef __attribute__((address_space(3))) bf16x4 lds_v4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4 *)lds);
}

// ---------------------------------------------------------------------------------------------
// attention: workgroup (kv head, (query block, split), sequence).  Query row i = q0 + c sees the keys 0 .. len + i of
// its slot; the block's keys are 0 .. n_keys - 1, n_keys = len + min(q0 + 32, n_new), and the workgroup walks the tiles
// of its split of them (all of them in a sequence that is not split).
// ---------------------------------------------------------------------------------------------
template <int GROUP>
__global__ __launch_bounds__(64 * GROUP) void extend_attention_kernel(const ExtendParams p) {
    // one pool: K buffers, then V buffers; the epilogue reuses its start for the per-wave output tiles
    constexpr int K_BUF = EXTEND_TILE * EXT_KROW, V_BUF = EXTEND_TILE * EXT_VROW;
    static_assert(GROUP * 32 * EXT_KROW <= 2 * (K_BUF + V_BUF), "output tiles must fit the staging pool");
    __shared__ __attribute__((aligned(16))) u16 s_pool[2 * (K_BUF + V_BUF)];
    u16(*s_k)[K_BUF] = reinterpret_cast<u16(*)[K_BUF]>(s_pool);
    u16(*s_v)[V_BUF] = reinterpret_cast<u16(*)[V_BUF]>(s_pool + 2 * K_BUF);
    constexpr int nthr = 64 * GROUP;
    const int kvh = blockIdx.x, b = blockIdx.z;
    const int seq_splits = p.seqs.splits[b];
    const int blk = blockIdx.y / seq_splits, split = blockIdx.y % seq_splits;
    const int q0 = blk * EXTEND_BLOCK;
    const int n_new = p.seqs.n_new[b];
    if (q0 >= n_new) return;   // (uniform)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int head = kvh * GROUP + wave;
    const int len = p.seqs.len[b];
    const int64_t t0 = (int64_t)p.seqs.row0[b] + q0;
    const int rows = n_new - q0 < EXTEND_BLOCK ? n_new - q0 : EXTEND_BLOCK;   // live query rows of the block
    const int n_keys = len + q0 + rows;
    const int n_tiles = (n_keys + EXTEND_TILE - 1) / EXTEND_TILE;
    // an earlier block of a split sequence may need fewer splits than the last one, down to one
    const int blk_splits = seq_splits == 1 ? 1 : (n_keys + EXTEND_SPLIT - 1) / EXTEND_SPLIT;
    if (split >= blk_splits) return;   // (uniform)
    const int kt_begin = split * SPLIT_TILES;
    const int kt_end = seq_splits == 1 || kt_begin + SPLIT_TILES > n_tiles ? n_tiles : kt_begin + SPLIT_TILES;
    const int c = lane & 31, h = lane >> 5;
    // the last key row c sees; a row past the block's live ones (never stored) sees what the last live row sees
    const int vis = len + q0 + (c < rows ? c : rows - 1);
    // Q^T fragments (B operand): B[k = 8h + j][col c] = Q[q0 + c][16 s + 8h + j]
    bf16x8 qf[8];
    {
        const u16 *qp = p.q_rot + ((t0 + (c < rows ? c : rows - 1)) * p.hq + head) * CRAG_HEAD_DIM + 8 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) qf[s] = ld_frag(qp + 16 * s);
    }
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 oacc[4] = {zero, zero, zero, zero};
    float m = -INFINITY, l = 0.f;
    const u16 *kglob = p.k_cache + kv_row(p.hkv, p.max_len, p.seqs.slot[b], kvh, 0);
    const u16 *vglob = p.v_cache + kv_row(p.hkv, p.max_len, p.seqs.slot[b], kvh, 0);

    // cooperative staging: a K tile and a V tile are 32 rows x 16 chunks of 16 B each; with `nthr` threads every
    // thread moves 512 / nthr chunks of each.  Rows at or beyond n_keys are not read: zeros take their place.
    constexpr int per = 512 / nthr;
    struct Stage {
        bf16x8 k[per], v[per];
    };
    auto fetch = [&](int kt, Stage &st) {
#pragma unroll
        for (int i = 0; i < per; ++i) {
            const int ch = tid + i * nthr;
            const int key = kt * EXTEND_TILE + (ch >> 4);
            st.k[i] = st.v[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (key < n_keys) {
                st.k[i] = ld_frag(kglob + (int64_t)key * CRAG_HEAD_DIM + 8 * (ch & 15));
                st.v[i] = ld_frag(vglob + (int64_t)key * CRAG_HEAD_DIM + 8 * (ch & 15));
            }
        }
    };
    auto stash = [&](int buf, const Stage &st) {
#pragma unroll
        for (int i = 0; i < per; ++i) {
            const int ch = tid + i * nthr;
            *reinterpret_cast<bf16x8 *>(&s_k[buf][(ch >> 4) * EXT_KROW + 8 * (ch & 15)]) = st.k[i];
            *reinterpret_cast<bf16x8 *>(&s_v[buf][(ch >> 4) * EXT_VROW + 8 * (ch & 15)]) = st.v[i];
        }
    };
    Stage st;
    fetch(kt_begin, st);
    stash(kt_begin & 1, st);
    __syncthreads();

    // transposed V read, lane (group g16 = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3): row 4h + q of an 8-row band,
    // columns 16 (g16 & 1) + 4 pp ..; the lane receives column (lane & 31) = c of the band's rows 4h .. 4h + 3
    const int v_lane = (4 * h + ((lane >> 2) & 3)) * EXT_VROW + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int k0 = kt * EXTEND_TILE, buf = kt & 1;
        if (kt + 1 < kt_end) fetch(kt + 1, st);  // in flight during this tile's MFMAs and softmax
        bf16x8 fr[8];
        {
            const u16 *kp = &s_k[buf][c * EXT_KROW + 8 * h];  // A[row = key c][k = 8h + j]
#pragma unroll
            for (int s = 0; s < 8; ++s) fr[s] = *reinterpret_cast<const bf16x8 *>(kp + 16 * s);
        }
        f32x16 sacc = zero;
#pragma unroll
        for (int s = 0; s < 8; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[s], qf[s], sacc, 0, 0, 0);
        // V^T fragments while the softmax runs: A operand V^T[d = 32 dt + c][k], element j of k-step s2 = key
        // 16 s2 + 8 (j >> 2) + 4h + (j & 3) of the tile, the order the S^T accumulator gives P^T in
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u16 *vp = &s_v[buf][v_lane + (16 * s2) * EXT_VROW + 32 * dt];
                const bf16x4 lo = ld_tr(vp), hi = ld_tr(vp + 8 * EXT_VROW);
                fr[2 * dt + s2] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
        // lane: query row q0 + c; register i: key r = (i&3) + 8*(i>>2) + 4h of the tile, visible while k0 + r <= vis.
        // That bound also masks the zero rows staged past n_keys - 1 (vis <= n_keys - 1).
        const int lim = vis - k0 + 1;
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
        mloc = halfwave_max(mloc);
        // finite from the first tile on in split 0: key 0 of the slot (<= vis) is never masked.  A later split may hold
        // no key a row sees: its maximum stays -inf, and the exponents are taken against 0 so that every weight, l and
        // o of that row stay 0 instead of becoming NaN.
        const float mnew = fmaxf(m, mloc);
        const float mref = mnew == -INFINITY ? 0.f : mnew;
        const float alpha = __builtin_amdgcn_exp2f(m - mref);
        float lsum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sv[i] = __builtin_amdgcn_exp2f(sv[i] - mref);
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
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)  // 4 independent accumulator chains
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[2 * dt + s2], pf[s2], oacc[dt], 0, 0, 0);
        if (kt + 1 < kt_end) stash(buf ^ 1, st);  // that buffer was last read in tile kt-1, before the previous barrier
        __syncthreads();
    }
    // O[q0 + c][32 dt + (i&3) + 8 (i>>2) + 4h] = oacc[dt][i] / l.
    if (blk_splits > 1) {
        // one split of several: (m, l) and the unnormalised accumulator as it lies in the registers -- quad (dt, g4) of
        // lane (c, h) at float4 index ((4 dt + g4) * 2 + h) * 32 + c, so that a wave stores 1 KiB at a stretch
        const int64_t part = ((int64_t)p.seqs.part0[b] + blk * seq_splits + split) * p.hq + head;
        float *po = p.part_o + part * PART_O;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<float4 *>(po + ((((4 * dt + g4) * 2 + h) * 32 + c) << 2)) =
                    make_float4(oacc[dt][4 * g4], oacc[dt][4 * g4 + 1], oacc[dt][4 * g4 + 2], oacc[dt][4 * g4 + 3]);
        if (h == 0) *reinterpret_cast<float2 *>(p.part_ml + part * PART_ML + 2 * c) = make_float2(m, l);
    } else {
        // the only split: the wave transposes its 32 x 128 tile through LDS (the staging pool is free after the last
        // barrier) and writes whole 256-byte rows, 16 bytes per lane; rows of a partial block are not stored.
        u16 *ot = s_pool + wave * (32 * EXT_KROW);
        const float inv = 1.f / l;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint2 w;
                w.x = (uint32_t)f2bf(oacc[dt][4 * g4] * inv) | ((uint32_t)f2bf(oacc[dt][4 * g4 + 1] * inv) << 16);
                w.y = (uint32_t)f2bf(oacc[dt][4 * g4 + 2] * inv) | ((uint32_t)f2bf(oacc[dt][4 * g4 + 3] * inv) << 16);
                *reinterpret_cast<uint2 *>(ot + c * EXT_KROW + 32 * dt + 8 * g4 + 4 * h) = w;
            }
        // same wave, LDS operations complete in order: no barrier between these writes and the reads below
        const int64_t out_stride = (int64_t)p.hq * CRAG_HEAD_DIM;
        u16 *obase = p.out + t0 * out_stride + (int64_t)head * CRAG_HEAD_DIM;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = (lane >> 4) + 4 * it, chunk = lane & 15;
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(ot + row * EXT_KROW + 8 * chunk);
            if (row < rows) *reinterpret_cast<bf16x8 *>(obase + (int64_t)row * out_stride + 8 * chunk) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// combine: workgroup (q head, query block, sequence) of a split sequence, 256 threads; a thread owns four quads of the
// block's 32 x 128 outputs in the order the partials lie in.  The splits in ascending order; rows of a partial block are
// not stored.  A block with one split has stored its output itself.
// ---------------------------------------------------------------------------------------------
constexpr int COMBINE_THREADS = 256;

__global__ __launch_bounds__(COMBINE_THREADS) void extend_combine_kernel(const ExtendParams p) {
    const int head = blockIdx.x, blk = blockIdx.y, b = blockIdx.z;
    const int seq_splits = p.seqs.splits[b];
    const int q0 = blk * EXTEND_BLOCK;
    const int n_new = p.seqs.n_new[b];
    if (seq_splits == 1 || q0 >= n_new) return;   // (uniform)
    const int rows = n_new - q0 < EXTEND_BLOCK ? n_new - q0 : EXTEND_BLOCK;
    const int n_keys = p.seqs.len[b] + q0 + rows;
    const int blk_splits = (n_keys + EXTEND_SPLIT - 1) / EXTEND_SPLIT;
    if (blk_splits == 1) return;                  // (uniform)
    const int64_t part0 = ((int64_t)p.seqs.part0[b] + blk * seq_splits) * p.hq + head;   // split s: + s * hq
    const int c = threadIdx.x & 31;
    if (c >= rows) return;
    const float *ml = p.part_ml + part0 * PART_ML + 2 * c;
    float m = -INFINITY;   // finite: row c sees key 0, which lies in split 0
    for (int s = 0; s < blk_splits; ++s) m = fmaxf(m, ml[(int64_t)s * p.hq * PART_ML]);
    float l = 0.f;
    for (int s = 0; s < blk_splits; ++s) {
        const float *e = ml + (int64_t)s * p.hq * PART_ML;
        l += e[1] * exp2f(e[0] - m);
    }
    const float inv = 1.f / l;
    u16 *orow = p.out + ((int64_t)p.seqs.row0[b] + q0 + c) * ((int64_t)p.hq * CRAG_HEAD_DIM) + (int64_t)head * CRAG_HEAD_DIM;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int quad = (threadIdx.x >> 5) + 8 * it;          // (4 dt + g4) * 2 + h
        const int d0 = 32 * (quad >> 3) + 8 * ((quad >> 1) & 3) + 4 * (quad & 1);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int s = 0; s < blk_splits; ++s) {
            const float w = exp2f(ml[(int64_t)s * p.hq * PART_ML] - m);
            const float4 a = *reinterpret_cast<const float4 *>(p.part_o + (part0 + (int64_t)s * p.hq) * PART_O + ((quad * 32 + c) << 2));
            o.x += a.x * w;
            o.y += a.y * w;
            o.z += a.z * w;
            o.w += a.w * w;
        }
        uint2 w2;
        w2.x = (uint32_t)f2bf(o.x * inv) | ((uint32_t)f2bf(o.y * inv) << 16);
        w2.y = (uint32_t)f2bf(o.z * inv) | ((uint32_t)f2bf(o.w * inv) << 16);
        *reinterpret_cast<uint2 *>(orow + d0) = w2;
    }
}

// (query block, split) pairs a sequence of these two lengths leaves partials for, and its splits (1: not split)
int seq_splits(int len, int n_new) {
    if (n_new > EXTEND_SPLIT_ROWS) return 1;
    return (len + n_new + EXTEND_SPLIT - 1) / EXTEND_SPLIT;
}
int64_t seq_parts(int len, int n_new) {
    const int sp = seq_splits(len, n_new);
    return sp == 1 ? 0 : (int64_t)((n_new + EXTEND_BLOCK - 1) / EXTEND_BLOCK) * sp;
}
constexpr int64_t PART_BYTES = (int64_t)(PART_O + PART_ML) * 4;

}  // namespace

extern "C" {

int64_t crag_enc_extend_workspace_bytes(int n_seqs, int hq, int max_new_rows, int max_len) {
    if (n_seqs <= 0 || n_seqs > EXTEND_MAX_SEQS || hq <= 0 || max_new_rows <= 0 || max_len <= 0) return 0;
    // q_rot: the rotated queries of every new row; the partials of the split sequences at their most: every sequence
    // with as many of the rows as are split at all, behind a cache that fills max_len
    int64_t blocks = ((int64_t)max_new_rows + EXTEND_BLOCK - 1) / EXTEND_BLOCK + n_seqs;
    const int64_t most = (int64_t)n_seqs * (EXTEND_SPLIT_ROWS / EXTEND_BLOCK);
    if (blocks > most) blocks = most;
    const int64_t splits = ((int64_t)max_len + EXTEND_SPLIT - 1) / EXTEND_SPLIT;
    return (int64_t)max_new_rows * hq * CRAG_HEAD_DIM * 2 + (splits > 1 ? blocks * splits * hq * PART_BYTES : 0);
}

int crag_enc_extend_attention(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                              const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                              int max_len, const int32_t *h_slots, const int32_t *h_cache_len, const int32_t *h_new_len,
                              int n_seqs, int hq, int hkv, float eps, float scale, void *workspace,
                              int64_t workspace_bytes, uint16_t *out, void *stream) {
    if (!qkv_new || !q_norm_w || !k_norm_w || !cos_sin || !k_cache || !v_cache || !h_slots || !h_cache_len || !h_new_len ||
        !workspace || !out)
        return efail("extend_attention: NULL pointer");
    if (n_seqs < 1 || n_seqs > EXTEND_MAX_SEQS)
        return efail("extend_attention: n_seqs must be in 1..%d (got %d)", EXTEND_MAX_SEQS, n_seqs);
    if (hq <= 0 || hkv <= 0 || hq % hkv || (hq / hkv != 2 && hq / hkv != 4))
        return efail("extend_attention: hq / hkv must be 2 or 4 (got %d / %d)", hq, hkv);
    if (n_slots <= 0 || max_len <= 0 || max_pos <= 0) return efail("extend_attention: n_slots, max_len and max_pos must be positive");
    if (((uintptr_t)qkv_new | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)workspace | (uintptr_t)q_norm_w |
         (uintptr_t)k_norm_w | (uintptr_t)out) & 15)
        return efail("extend_attention: qkv_new, the norm weights, the cache, the workspace and out must be 16-byte aligned");
    ExtendParams p;
    int64_t total = 0, parts = 0;
    int most = 0, most_y = 0, most_split_blocks = 0;
    for (int b = 0; b < n_seqs; ++b) {
        const int len = h_cache_len[b], n_new = h_new_len[b], slot = h_slots[b];
        if (len < 0) return efail("extend_attention: cache length %d of sequence %d is negative", len, b);
        if (n_new < 1) return efail("extend_attention: new_len %d of sequence %d must be at least 1", n_new, b);
        if ((int64_t)len + n_new > max_len)
            return efail("extend_attention: %d cached + %d new rows of sequence %d exceed max_len = %d", len, n_new, b, max_len);
        if ((int64_t)len + n_new > max_pos)
            return efail("extend_attention: the positions of sequence %d (%d + %d) run beyond the RoPE table (%d rows)", b,
                         len, n_new, max_pos);
        if (slot < 0 || slot >= n_slots) return efail("extend_attention: slot %d of sequence %d is outside 0..%d", slot, b, n_slots - 1);
        for (int a = 0; a < b; ++a)
            if (h_slots[a] == slot) return efail("extend_attention: slot %d is named twice in one call", slot);
        p.seqs.len[b] = len;
        p.seqs.n_new[b] = n_new;
        p.seqs.row0[b] = (int32_t)total;
        p.seqs.slot[b] = slot;
        p.seqs.splits[b] = seq_splits(len, n_new);
        p.seqs.part0[b] = (int32_t)parts;
        const int blocks = (n_new + EXTEND_BLOCK - 1) / EXTEND_BLOCK;
        total += n_new;
        parts += seq_parts(len, n_new);
        most = n_new > most ? n_new : most;
        most_y = blocks * p.seqs.splits[b] > most_y ? blocks * p.seqs.splits[b] : most_y;
        if (p.seqs.splits[b] > 1 && blocks > most_split_blocks) most_split_blocks = blocks;
    }
    for (int b = n_seqs; b < EXTEND_MAX_SEQS; ++b) {
        p.seqs.len[b] = p.seqs.n_new[b] = p.seqs.row0[b] = p.seqs.slot[b] = p.seqs.part0[b] = 0;
        p.seqs.splits[b] = 1;
    }
    const int64_t q_bytes = total * hq * CRAG_HEAD_DIM * 2;   // (a multiple of 16)
    const int64_t need = q_bytes + parts * hq * PART_BYTES;
    if (workspace_bytes < need)
        return fail(CRAG_E2BIG, "extend_attention: the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes,
                    (long long)need);
    p.qkv_new = qkv_new;
    p.qw = q_norm_w;
    p.kw = k_norm_w;
    p.cos_sin = cos_sin;
    p.k_cache = k_cache;
    p.v_cache = v_cache;
    p.q_rot = (u16 *)workspace;
    p.part_o = (float *)((char *)workspace + q_bytes);
    p.part_ml = p.part_o + parts * hq * PART_O;
    p.out = out;
    p.hq = hq;
    p.hkv = hkv;
    p.max_len = max_len;
    p.eps = eps;
    p.scale_log2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(extend_prepare_kernel, dim3((unsigned)most, (unsigned)n_seqs), dim3(PREP_THREADS), 0, st, p);
    const dim3 grid((unsigned)hkv, (unsigned)most_y, (unsigned)n_seqs);
    if (hq / hkv == 2)
        hipLaunchKernelGGL(extend_attention_kernel<2>, grid, dim3(128), 0, st, p);
    else
        hipLaunchKernelGGL(extend_attention_kernel<4>, grid, dim3(256), 0, st, p);
    if (most_split_blocks)
        hipLaunchKernelGGL(extend_combine_kernel, dim3((unsigned)hq, (unsigned)most_split_blocks, (unsigned)n_seqs),
                           dim3(COMBINE_THREADS), 0, st, p);
    return hip_ok("extend_attention");
}

}  // extern "C"
