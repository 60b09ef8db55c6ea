// crag_decode.hip — the operators autoregressive decoding adds to the Qwen3 forward (gfx950).  C ABI: include/crag_encoder.h.
//
//   crag_enc_decode_attention   one new token per sequence against a KV cache: q/k-norm + RoPE of the new row, the append
//                               of its key and value, attention over the len + 1 keys.  Three launches: prepare (norm,
//                               rope, append), split (one workgroup per (128-key split, kv head, sequence) -> partial
//                               (m, l, o) in fp32), combine (the splits in ascending order).
//   crag_enc_lm_head            final RMSNorm (+ delta) of up to 8 rows, fp32 logits against every row of lm_head (the
//                               weights streamed once through bf16 MFMA), greedy token = lowest id among the maxima,
//                               banned ids left out.
//
//   crag_enc_decode_attention_shared   the same over FORKED sequences: a sequence reads its first shared_len rows from
//                               a parent slot and the rest from its own.  The split launch runs units: the sequences of
//                               one parent form group units, each of which loads every row of a wholly shared split
//                               once for its members' query heads; every sequence is a unit of its own for its other
//                               splits.
//   crag_enc_decode_attention_rows     the same with SEVERAL new rows per sequence (a pending token and its drafts): row i
//                               sees the keys up to its own position, the rows appended before it in the call among
//                               them.  A unit of the split launch is a run of consecutive rows of one sequence, with
//                               one key more for each member.
//
// Nothing here depends on the number of sequences, on the slot or on a launch size chosen at run time: a split is
// always DECODE_SPLIT keys, its keys are always walked by the same lanes in the same order, and the splits are summed
// in ascending order, so a sequence's output bits are a function of its own data alone.  No atomics.

#include <math.h>
#include <string.h>

#include "../../include/crag_encoder.h"
#include "crag_enc_common.h"

namespace {

constexpr int DECODE_MAX_SEQS = CRAG_DECODE_MAX_SEQS;
constexpr int DECODE_SPLIT = CRAG_DECODE_SPLIT;  // keys per workgroup of the split kernel
constexpr int DECODE_THREADS = 256;              // 16 groups of 16 lanes: a group reads one 256-byte key / value row
constexpr int DECODE_GROUPS = DECODE_THREADS / 16;
constexpr int DECODE_ITERS = DECODE_SPLIT / DECODE_GROUPS;

// the host-validated per-sequence data travel as kernel arguments
struct DecodeSeqs {
    int32_t len[DECODE_MAX_SEQS];
    int32_t slot[DECODE_MAX_SEQS];
};

struct DecodeParams {
    const u16 *qkv_new;   // [n_seqs, (hq + 2 hkv) * 128] raw projections
    const u16 *qw, *kw;   // [128]
    const float *cos_sin; // [max_pos, 64, 2]
    u16 *k_cache;         // [n_slots][hkv][max_len][128]
    u16 *v_cache;
    u16 *q_rot;           // workspace: [n_seqs][hq][128] bf16
    float *part_o;        // workspace: [n_seqs][hq][max_splits][128]
    float *part_ml;       // workspace: [n_seqs][hq][max_splits][2]
    u16 *out;             // [n_seqs, hq * 128]
    int hq, hkv, max_len, max_splits;
    float eps, scale_log2;
    DecodeSeqs seqs;
};

static_assert(DECODE_THREADS == KV_APPEND_THREADS, "the prepare kernel is kv_append_row's workgroup");

// prepare: one workgroup per sequence appends the new token at position len (kv_append_row, crag_enc_common.h)
__global__ __launch_bounds__(DECODE_THREADS) void decode_prepare_kernel(const DecodeParams p) {
    const int b = blockIdx.x;
    const int pos = p.seqs.len[b], slot = p.seqs.slot[b];
    kv_append_row(p.qkv_new + b * (int64_t)(p.hq + 2 * p.hkv) * CRAG_HEAD_DIM, p.qw, p.kw, p.cos_sin, p.k_cache, p.v_cache,
                  p.q_rot + (int64_t)b * p.hq * CRAG_HEAD_DIM, p.hq, p.hkv, p.max_len, slot, pos, p.eps);
}

// ---------------------------------------------------------------------------------------------
// split: workgroup (split s, kv head, sequence) over the keys [128 s, min(128 s + 128, len + 1)).  A 16-lane group
// reads one key row (16 bytes per lane) and every load serves the G query heads of the kv head.  Scores and weights
// pass through LDS in fp32; the 16 groups' partial outputs are summed in group order.
// ---------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(DECODE_THREADS) void decode_split_kernel(const DecodeParams p) {
    __shared__ float sc[G][DECODE_SPLIT];                       // raw dot products, then the weights
    __shared__ float red[DECODE_GROUPS][G][CRAG_HEAD_DIM];      // 32 KiB at G = 4
    __shared__ float ml[G][2];
    const int s = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int n_keys = p.seqs.len[b] + 1;   // the prepare launch appended the new token's own key
    const int k0 = s * DECODE_SPLIT;
    if (k0 >= n_keys) return;               // (uniform)
    const int slot = p.seqs.slot[b];
    const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const u16 *kc = p.k_cache + kv_row(p.hkv, p.max_len, slot, kvh, 0);
    const u16 *vc = p.v_cache + kv_row(p.hkv, p.max_len, slot, kvh, 0);

    float q[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const Pack8 a = *reinterpret_cast<const Pack8 *>(p.q_rot + ((int64_t)b * p.hq + kvh * G + g) * CRAG_HEAD_DIM + sub * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[g][e] = bf2f(a.v[e]);
    }
    // scores
#pragma unroll 4
    for (int it = 0; it < DECODE_ITERS; ++it) {
        const int j = it * DECODE_GROUPS + grp;
        const bool live = k0 + j < n_keys;   // positions at or beyond len + 1 are never read
        Pack8 a;
#pragma unroll
        for (int e = 0; e < 8; ++e) a.v[e] = 0;
        if (live) a = *reinterpret_cast<const Pack8 *>(kc + (int64_t)(k0 + j) * CRAG_HEAD_DIM + sub * 8);
        float d[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            d[g] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d[g] += q[g][e] * bf2f(a.v[e]);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1)
#pragma unroll
            for (int g = 0; g < G; ++g) d[g] += __shfl_xor(d[g], o);
        if (sub == 0) {
#pragma unroll
            for (int g = 0; g < G; ++g) sc[g][j] = live ? d[g] : -INFINITY;
        }
    }
    __syncthreads();
    // softmax of the split: wave w = query head w of the group
    {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (w < G) {
            float x[DECODE_SPLIT / 64];
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < DECODE_SPLIT / 64; ++i) {
                x[i] = sc[w][lane + 64 * i];
                m = fmaxf(m, x[i]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
            float l = 0.f;
#pragma unroll
            for (int i = 0; i < DECODE_SPLIT / 64; ++i) {
                const float pr = exp2f((x[i] - m) * p.scale_log2);   // the split holds at least one key: m is finite
                sc[w][lane + 64 * i] = pr;
                l += pr;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o);
            if (lane == 0) {
                ml[w][0] = m;
                ml[w][1] = l;
            }
        }
    }
    __syncthreads();
    // weighted values
    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
#pragma unroll 4
    for (int it = 0; it < DECODE_ITERS; ++it) {
        const int j = it * DECODE_GROUPS + grp;
        if (k0 + j < n_keys) {
            const Pack8 a = *reinterpret_cast<const Pack8 *>(vc + (int64_t)(k0 + j) * CRAG_HEAD_DIM + sub * 8);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float pr = sc[g][j];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] += pr * bf2f(a.v[e]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[grp][g][sub * 8 + e] = acc[g][e];
    __syncthreads();
    for (int i = threadIdx.x; i < G * CRAG_HEAD_DIM; i += DECODE_THREADS) {
        const int g = i / CRAG_HEAD_DIM, d = i % CRAG_HEAD_DIM;
        float o = 0.f;
#pragma unroll
        for (int r = 0; r < DECODE_GROUPS; ++r) o += red[r][g][d];
        const int64_t part = ((int64_t)b * p.hq + kvh * G + g) * p.max_splits + s;
        p.part_o[part * CRAG_HEAD_DIM + d] = o;
        if (d < 2) p.part_ml[part * 2 + d] = ml[g][d];
    }
}

// ---------------------------------------------------------------------------------------------
// split over forked sequences.  A unit (blockIdx.z) is a list of member sequences that read the SAME rows in the splits
// [s_begin, s_end): logical row j comes from slot `parent` when j < shared and from slot `own` otherwise.  A group unit
// holds 2..FORK_UNIT_MEMBERS sequences of one parent over the splits wholly below the shared_len of every sequence of
// that parent; a sequence's other splits are a unit of one member.  decode_split_kernel's arithmetic per (sequence, head, split): a row is read by
// the same 16-lane group and dotted in the same element and shuffle order, the 16 groups are summed in group order.
// A lane keeps its 8 key rows, then its 8 value rows, in registers (one Pack8 each) while the members pass by: their
// rotated queries wait in LDS, their scores in sc[member]; red is reused member after member.
// ---------------------------------------------------------------------------------------------
constexpr int FORK_MAX_UNITS = DECODE_MAX_SEQS + DECODE_MAX_SEQS / 2;   // every sequence alone + the units of >= 2
// Sequences one group unit serves.  Measured at 32 / 8 heads with 8 children of one parent (profiles/fork_bench.jsonl,
// the lines with "unit_members"): units of 8 take 36 / 51 us at 1024 / 4096 shared keys, units of 4 28 / 41 us, units
// of 2 22 / 43 us, private copies 23 / 50 us -- a unit works its members off one after the other, and with 8 or 32
// splits per kv head the launch has too few workgroups to hide that.  Two is the size that loses nowhere; the kernel
// itself takes any size up to 8.
constexpr int FORK_UNIT_MEMBERS = 2;
static_assert(FORK_UNIT_MEMBERS >= 2 && FORK_UNIT_MEMBERS <= DECODE_MAX_SEQS, "a group unit holds 2..8 sequences");

struct ForkUnits {
    int32_t n_members[FORK_MAX_UNITS];
    int32_t s_begin[FORK_MAX_UNITS], s_end[FORK_MAX_UNITS];
    int32_t parent[FORK_MAX_UNITS], own[FORK_MAX_UNITS];   // slots
    int32_t shared[FORK_MAX_UNITS], n_keys[FORK_MAX_UNITS];
    int8_t member[FORK_MAX_UNITS][DECODE_MAX_SEQS];         // sequence indices
    static constexpr bool ragged = false;                   // every member of a unit sees the same keys
    __device__ int row(int unit, int m) const { return member[unit][m]; }
    __device__ int keys(int unit, int) const { return n_keys[unit]; }
};

// The units of crag_enc_decode_attention_rows: up to M consecutive new rows of ONE sequence.  Member m is row row0 + m
// of the call and sees one key more than member m - 1: n_keys is what the LAST member sees.
constexpr int ROWS_MAX = CRAG_DECODE_MAX_ROWS;
static_assert(ROWS_MAX == DECODE_MAX_SEQS, "the rows of a call travel in DecodeSeqs, one entry per row");
struct RowUnits {
    int32_t n_members[ROWS_MAX];
    int32_t s_begin[ROWS_MAX], s_end[ROWS_MAX];
    int32_t parent[ROWS_MAX], own[ROWS_MAX];   // slots
    int32_t shared[ROWS_MAX], n_keys[ROWS_MAX];
    int32_t row0[ROWS_MAX];
    static constexpr bool ragged = true;
    __device__ int row(int unit, int m) const { return row0[unit] + m; }
    __device__ int keys(int unit, int m) const { return n_keys[unit] - (n_members[unit] - 1 - m); }
};

// Lane i of every 16-lane row <- lane (i + N) % 16 of the row, on the VALU (DPP row_ror).  In a butterfly over the
// strides 8, 4, 2, 1 it stands for __shfl_xor(v, N) bit for bit: behind the stages of the larger strides every lane
// holds what its partners across those strides hold (a + b == b + a), and (i + N) % 16 differs from i ^ N in the bits
// of those strides only.
template <int N>
__device__ __forceinline__ float row_ror(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x120 + N, 0xF, 0xF, true));
}

// The body serves both kinds of unit (Units = ForkUnits or RowUnits) with up to M members.  Under Units::ragged member
// m sees the keys below u.keys(unit, m) only, ascending in m up to the unit's n_keys: a key behind them scores -inf for
// that member and its value is skipped, as decode_split_kernel does past its n_keys; the members that see no key of
// the split -- the first m_first -- are left out of it, as decode_split_kernel leaves a sequence out.
template <int G, int M, class Units>
__device__ __forceinline__ void split_units(const DecodeParams &p, const Units &u) {
    __shared__ float sc[M][G][DECODE_SPLIT];                    // raw dot products, then the weights
    __shared__ float red[DECODE_GROUPS][G][CRAG_HEAD_DIM];      // 32 KiB at G = 4
    __shared__ float ml[M][G][2];
    __shared__ __align__(16) u16 qs[M][G][CRAG_HEAD_DIM];       // the members' rotated queries
    const int s = blockIdx.x, kvh = blockIdx.y, unit = blockIdx.z;
    if (s < u.s_begin[unit] || s >= u.s_end[unit]) return;   // (uniform)
    const int n_mem = u.n_members[unit], n_keys = u.n_keys[unit], shared = u.shared[unit];
    const int k0 = s * DECODE_SPLIT;
    int m_first = 0;
    if constexpr (Units::ragged) m_first = k0 - n_keys + n_mem > 0 ? k0 - n_keys + n_mem : 0;
    const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const u16 *kp = p.k_cache + kv_row(p.hkv, p.max_len, u.parent[unit], kvh, 0);
    const u16 *vp = p.v_cache + kv_row(p.hkv, p.max_len, u.parent[unit], kvh, 0);
    const u16 *ko = p.k_cache + kv_row(p.hkv, p.max_len, u.own[unit], kvh, 0);
    const u16 *vo = p.v_cache + kv_row(p.hkv, p.max_len, u.own[unit], kvh, 0);

    for (int i = threadIdx.x; i < n_mem * G * 16; i += DECODE_THREADS) {
        const int m = i / (G * 16), g = i / 16 % G, ch = i % 16;
        *reinterpret_cast<Pack8 *>(&qs[m][g][ch * 8]) = *reinterpret_cast<const Pack8 *>(
            p.q_rot + ((int64_t)u.row(unit, m) * p.hq + kvh * G + g) * CRAG_HEAD_DIM + ch * 8);
    }
    Pack8 rows[DECODE_ITERS];
#pragma unroll
    for (int it = 0; it < DECODE_ITERS; ++it) {
        const int j = k0 + it * DECODE_GROUPS + grp;
#pragma unroll
        for (int e = 0; e < 8; ++e) rows[it].v[e] = 0;
        if (j < n_keys)   // positions at or beyond len + 1 are never read, nor a child's own rows below shared_len
            rows[it] = *reinterpret_cast<const Pack8 *>((j < shared ? kp : ko) + (int64_t)j * CRAG_HEAD_DIM + sub * 8);
    }
    __syncthreads();
    // scores
    for (int m = m_first; m < n_mem; ++m) {
        const int m_keys = Units::ragged ? u.keys(unit, m) : n_keys;
        float q[G][8];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const Pack8 a = *reinterpret_cast<const Pack8 *>(&qs[m][g][sub * 8]);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[g][e] = bf2f(a.v[e]);
        }
        float d[DECODE_ITERS][G];
#pragma unroll
        for (int it = 0; it < DECODE_ITERS; ++it)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                d[it][g] = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d[it][g] += q[g][e] * bf2f(rows[it].v[e]);
            }
#pragma unroll
        for (int it = 0; it < DECODE_ITERS; ++it)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                d[it][g] += row_ror<8>(d[it][g]);
                d[it][g] += row_ror<4>(d[it][g]);
                d[it][g] += row_ror<2>(d[it][g]);
                d[it][g] += row_ror<1>(d[it][g]);
            }
        if (sub == 0) {
#pragma unroll
            for (int it = 0; it < DECODE_ITERS; ++it) {
                const int j = it * DECODE_GROUPS + grp;
#pragma unroll
                for (int g = 0; g < G; ++g) sc[m][g][j] = k0 + j < m_keys ? d[it][g] : -INFINITY;
            }
        }
    }
    // the value rows travel while the softmax runs
#pragma unroll
    for (int it = 0; it < DECODE_ITERS; ++it) {
        const int j = k0 + it * DECODE_GROUPS + grp;
        if (j < n_keys)
            rows[it] = *reinterpret_cast<const Pack8 *>((j < shared ? vp : vo) + (int64_t)j * CRAG_HEAD_DIM + sub * 8);
    }
    __syncthreads();
    // softmax of the split: a wave takes every fourth (member, query head), SM_HEADS of them side by side so that
    // their reductions overlap (the strides 32 and 16 cross the 16-lane rows: shuffles; below them row_ror)
    {
        constexpr int WAVES = DECODE_THREADS / 64;
        constexpr int SM_HEADS = M * G >= 4 * WAVES ? 4 : M * G > WAVES ? 2 : 1;
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int n_heads = n_mem * G;
        for (int h0 = m_first * G + w; h0 < n_heads; h0 += SM_HEADS * WAVES) {   // (uniform in the wave)
            float x[SM_HEADS][DECODE_SPLIT / 64], mx[SM_HEADS], l[SM_HEADS];
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) {
                const int hd = h0 + t * WAVES < n_heads ? h0 + t * WAVES : h0;   // past the last head: h0 again, not stored
                mx[t] = -INFINITY;
#pragma unroll
                for (int i = 0; i < DECODE_SPLIT / 64; ++i) {
                    x[t][i] = sc[hd / G][hd % G][lane + 64 * i];
                    mx[t] = fmaxf(mx[t], x[t][i]);
                }
            }
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], 32));
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], 16));
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) {
                mx[t] = fmaxf(mx[t], row_ror<8>(mx[t]));
                mx[t] = fmaxf(mx[t], row_ror<4>(mx[t]));
                mx[t] = fmaxf(mx[t], row_ror<2>(mx[t]));
                mx[t] = fmaxf(mx[t], row_ror<1>(mx[t]));
                l[t] = 0.f;
#pragma unroll
                for (int i = 0; i < DECODE_SPLIT / 64; ++i) {
                    x[t][i] = exp2f((x[t][i] - mx[t]) * p.scale_log2);   // the split holds at least one key: mx is finite
                    l[t] += x[t][i];
                }
            }
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) l[t] += __shfl_xor(l[t], 32);
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) l[t] += __shfl_xor(l[t], 16);
#pragma unroll
            for (int t = 0; t < SM_HEADS; ++t) {
                l[t] += row_ror<8>(l[t]);
                l[t] += row_ror<4>(l[t]);
                l[t] += row_ror<2>(l[t]);
                l[t] += row_ror<1>(l[t]);
                const int hd = h0 + t * WAVES;
                if (hd < n_heads) {
#pragma unroll
                    for (int i = 0; i < DECODE_SPLIT / 64; ++i) sc[hd / G][hd % G][lane + 64 * i] = x[t][i];
                    if (lane == 0) {
                        ml[hd / G][hd % G][0] = mx[t];
                        ml[hd / G][hd % G][1] = l[t];
                    }
                }
            }
        }
    }
    __syncthreads();
    // weighted values, member after member
    for (int m = m_first; m < n_mem; ++m) {
        const int m_keys = Units::ragged ? u.keys(unit, m) : n_keys;
        float acc[G][8];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
#pragma unroll
        for (int it = 0; it < DECODE_ITERS; ++it) {
            const int j = it * DECODE_GROUPS + grp;
            if (k0 + j < m_keys) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float pr = sc[m][g][j];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[g][e] += pr * bf2f(rows[it].v[e]);
                }
            }
        }
        if (m > m_first) __syncthreads();   // the sums of the member before have been read
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[grp][g][sub * 8 + e] = acc[g][e];
        __syncthreads();
        const int b = u.row(unit, m);
        for (int i = threadIdx.x; i < G * CRAG_HEAD_DIM; i += DECODE_THREADS) {
            const int g = i / CRAG_HEAD_DIM, d = i % CRAG_HEAD_DIM;
            float o = 0.f;
#pragma unroll
            for (int r = 0; r < DECODE_GROUPS; ++r) o += red[r][g][d];
            const int64_t part = ((int64_t)b * p.hq + kvh * G + g) * p.max_splits + s;
            p.part_o[part * CRAG_HEAD_DIM + d] = o;
            if (d < 2) p.part_ml[part * 2 + d] = ml[m][g][d];
        }
    }
}

template <int G>
__global__ __launch_bounds__(DECODE_THREADS) void decode_split_shared_kernel(const DecodeParams p, const ForkUnits u) {
    split_units<G, FORK_UNIT_MEMBERS>(p, u);
}

// Rows one unit of crag_enc_decode_attention_rows serves.  Measured at 32 / 8 heads with a library built at each value
// (profiles/speculate_bench.jsonl, the lines with "unit_rows"): 8 rows of one sequence take 18 / 21 / 43 us
// at 128 / 1024 / 4096 cached tokens in units of 2, 19 / 23 / 45 in units of 1, 23 / 25 / 47 in units of 4 and 34 / 36 /
// 51 in units of 8 -- as with forks a unit works its members off one after the other, and a launch of at most 33 splits
// x 8 kv heads has too few workgroups to hide that.  Two is the size that loses nowhere; the kernel takes 1..8.
constexpr int ROWS_UNIT_MEMBERS = 2;
static_assert(ROWS_UNIT_MEMBERS >= 1 && ROWS_UNIT_MEMBERS <= ROWS_MAX, "a unit holds 1..8 rows");

template <int G>
__global__ __launch_bounds__(DECODE_THREADS) void decode_split_rows_kernel(const DecodeParams p, const RowUnits u) {
    split_units<G, ROWS_UNIT_MEMBERS>(p, u);
}

// combine: workgroup (q head, sequence), 128 threads = the 128 output elements; the splits in ascending order
__global__ __launch_bounds__(CRAG_HEAD_DIM) void decode_combine_kernel(const DecodeParams p) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const int n_splits = p.seqs.len[b] / DECODE_SPLIT + 1;   // ceil((len + 1) / split)
    const int64_t part0 = ((int64_t)b * p.hq + h) * p.max_splits;
    float m = -INFINITY;
    for (int s = 0; s < n_splits; ++s) m = fmaxf(m, p.part_ml[(part0 + s) * 2]);
    float l = 0.f, o = 0.f;
    for (int s = 0; s < n_splits; ++s) {
        const float w = exp2f((p.part_ml[(part0 + s) * 2] - m) * p.scale_log2);
        l += p.part_ml[(part0 + s) * 2 + 1] * w;
        o += p.part_o[(part0 + s) * CRAG_HEAD_DIM + d] * w;
    }
    p.out[((int64_t)b * p.hq + h) * CRAG_HEAD_DIM + d] = f2bf(o / l);
}

// ---------------------------------------------------------------------------------------------
// lm_head: a workgroup norms the n rows into LDS (rerank_head_kernel's roundings: the normed row in the model's bf16),
// then its four waves stream LM_ROWS_PER_WG rows of lm_head in tiles of 16 rows: D[vocab row][x row] +=
// W[vocab row][k] X[x row][k] with v_mfma_f32_16x16x32_bf16, the x rows n..15 zero.  A lane reads 32 contiguous bytes
// of its weight row per 64-element k block (the 4 lanes of a row: one 128-byte line) and the same elements of its x
// row from LDS; which elements meet in which MFMA does not matter to a dot product as long as both operands agree.
// The rows live in LDS with a 16-byte pad each: n * (hidden + 8) <= CRAG_LM_HEAD_MAX_ELEMS (64 KiB less the sums).
// ---------------------------------------------------------------------------------------------
constexpr int LM_THREADS = 256;
constexpr int LM_ROWS_PER_WG = 256;
constexpr int LM_MAX_ROWS = CRAG_DECODE_MAX_SEQS;
constexpr int LM_PAD = 8;   // elements: consecutive x rows start 4 banks apart

__global__ __launch_bounds__(LM_THREADS) void lm_head_kernel(const u16 *hs, const u16 *delta, const u16 *w, const u16 *lm,
                                                            float *logits, int n, int hidden, int64_t vocab, float eps) {
    extern __shared__ __align__(16) unsigned char lm_smem[];
    const int ld = hidden + LM_PAD;
    u16 *xn = reinterpret_cast<u16 *>(lm_smem);   // [n][hidden + 8] bf16, then block_sum's four floats
    float *sh = reinterpret_cast<float *>(lm_smem + (size_t)n * ld * sizeof(u16));
    for (int r = 0; r < n; ++r) {
        const u16 *x = hs + (int64_t)r * hidden;
        const u16 *dl = delta ? delta + (int64_t)r * hidden : nullptr;
        float ss = 0.f;
        for (int i = threadIdx.x; i < hidden; i += LM_THREADS) {
            const u16 s = dl ? f2bf(bf2f(x[i]) + bf2f(dl[i])) : x[i];
            xn[r * ld + i] = s;   // (this thread's own elements: read back below without a barrier)
            const float v = bf2f(s);
            ss += v * v;
        }
        ss = block_sum(ss, sh);
        const float rstd = rsqrtf(ss / (float)hidden + eps);
        for (int i = threadIdx.x; i < hidden; i += LM_THREADS)
            xn[r * ld + i] = f2bf(bf2f(w[i]) * bf2f(f2bf(bf2f(xn[r * ld + i]) * rstd)));
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t v0 = (int64_t)blockIdx.x * LM_ROWS_PER_WG;
    const int64_t v1 = v0 + LM_ROWS_PER_WG < vocab ? v0 + LM_ROWS_PER_WG : vocab;
    const bool has_x = r16 < n;
    const u16 *xp = xn + (has_x ? r16 : 0) * ld + kq * 16;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t0 = v0 + wave * 16; t0 < v1; t0 += 64) {
        const int64_t vr = t0 + r16 < v1 ? t0 + r16 : v1 - 1;   // a tile's rows past the end re-read the last row; never stored
        const u16 *wp = lm + vr * hidden + kq * 16;
        f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
        int k0 = 0;
        for (; k0 + 256 <= hidden; k0 += 256) {   // four k blocks: 128 bytes of the weight row per lane in flight
            bf16x8 a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = ld_frag(wp + k0 + 64 * (u >> 1) + 8 * (u & 1));
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bf16x8 b = has_x ? ld_frag(xp + k0 + 64 * (u >> 1) + 8 * (u & 1)) : zero;
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b, acc, 0, 0, 0);
            }
        }
        for (; k0 < hidden; k0 += 64) {
            const bf16x8 a0 = ld_frag(wp + k0), a1 = ld_frag(wp + k0 + 8);
            const bf16x8 b0 = has_x ? ld_frag(xp + k0) : zero, b1 = has_x ? ld_frag(xp + k0 + 8) : zero;
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
        }
        // D[row = vocab row 4 kq + r of the tile][col = x row r16]
        if (has_x) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t v = t0 + 4 * kq + r;
                if (v < v1) logits[(int64_t)r16 * vocab + v] = acc[r];
            }
        }
    }
}

// greedy token of one row: the lowest id among the maxima of its logits, banned ids and NaNs left out; -1 when nothing
// is left.  One workgroup per row; a thread walks its ids in ascending order, the threads are merged on (value, id).
constexpr int ARGMAX_THREADS = 1024;

__global__ __launch_bounds__(ARGMAX_THREADS) void lm_argmax_kernel(const float *logits, int64_t vocab, const int32_t *banned,
                                                                   int n_banned, int32_t *token) {
    __shared__ float sv[ARGMAX_THREADS / 64];
    __shared__ int si[ARGMAX_THREADS / 64];
    const float *row = logits + (int64_t)blockIdx.x * vocab;
    float bv = 0.f;
    int bid = -1;
    for (int64_t i = threadIdx.x; i < vocab; i += ARGMAX_THREADS) {
        const float v = row[i];
        if (v != v || !(bid < 0 || v > bv)) continue;
        bool ban = false;
        for (int k = 0; k < n_banned; ++k) ban |= banned[k] == (int32_t)i;
        if (!ban) {
            bv = v;
            bid = (int)i;
        }
    }
    const Best best = block_best<ARGMAX_THREADS / 64, false>(bv, bid, 0, sv, si, nullptr);
    if (threadIdx.x == 0) token[blockIdx.x] = best.id;
}

// The checks the three attention entries share, in the order they are made.  `what` names the entry.
struct DecodeArgs {
    const uint16_t *qkv_new, *q_norm_w, *k_norm_w;
    const float *cos_sin;
    int max_pos;
    uint16_t *k_cache, *v_cache;
    int n_slots, max_len;
    const int32_t *h_slots, *h_cache_len;
    int n_seqs, hq, hkv;
    float eps, scale;
    void *workspace;
    int64_t workspace_bytes;
    uint16_t *out;
};

int decode_check_shape(const char *what, const DecodeArgs &a) {
    if (!a.qkv_new || !a.q_norm_w || !a.k_norm_w || !a.cos_sin || !a.k_cache || !a.v_cache || !a.h_slots || !a.h_cache_len ||
        !a.workspace || !a.out)
        return efail("%s: NULL pointer", what);
    if (a.n_seqs < 1 || a.n_seqs > DECODE_MAX_SEQS)
        return efail("%s: n_seqs must be in 1..%d (got %d)", what, DECODE_MAX_SEQS, a.n_seqs);
    if (a.hq <= 0 || a.hkv <= 0 || a.hq % a.hkv || (a.hq / a.hkv != 2 && a.hq / a.hkv != 4))
        return efail("%s: hq / hkv must be 2 or 4 (got %d / %d)", what, a.hq, a.hkv);
    if (a.n_slots <= 0 || a.max_len <= 0 || a.max_pos <= 0)
        return efail("%s: n_slots, max_len and max_pos must be positive", what);
    if (((uintptr_t)a.qkv_new | (uintptr_t)a.k_cache | (uintptr_t)a.v_cache | (uintptr_t)a.workspace | (uintptr_t)a.q_norm_w |
         (uintptr_t)a.k_norm_w) & 15)
        return efail("%s: qkv_new, the norm weights, the cache and the workspace must be 16-byte aligned", what);
    return CRAG_OK;
}

int decode_check_slot(const char *what, const DecodeArgs &a, int b) {
    const int slot = a.h_slots[b];
    if (slot < 0 || slot >= a.n_slots) return efail("%s: slot %d of sequence %d is outside 0..%d", what, slot, b, a.n_slots - 1);
    for (int c = 0; c < b; ++c)
        if (a.h_slots[c] == slot) return efail("%s: slot %d is named twice in one call", what, slot);
    return CRAG_OK;
}

// the workspace check and the parameter block of a launch over n_rows query rows (p.seqs is the caller's)
int decode_fill(const char *what, const DecodeArgs &a, int n_rows, DecodeParams &p) {
    const int64_t need = crag_enc_decode_workspace_bytes(n_rows, a.hq, a.max_len);
    if (a.workspace_bytes < need)
        return fail(CRAG_E2BIG, "%s: the workspace holds %lld bytes, %lld are needed", what, (long long)a.workspace_bytes,
                    (long long)need);
    const int max_splits = (a.max_len + DECODE_SPLIT - 1) / DECODE_SPLIT;
    const int64_t heads = (int64_t)n_rows * a.hq;
    p.qkv_new = a.qkv_new;
    p.qw = a.q_norm_w;
    p.kw = a.k_norm_w;
    p.cos_sin = a.cos_sin;
    p.k_cache = a.k_cache;
    p.v_cache = a.v_cache;
    p.q_rot = (u16 *)a.workspace;
    p.part_o = (float *)((char *)a.workspace + heads * CRAG_HEAD_DIM * 2);
    p.part_ml = p.part_o + heads * max_splits * CRAG_HEAD_DIM;
    p.out = a.out;
    p.hq = a.hq;
    p.hkv = a.hkv;
    p.max_len = a.max_len;
    p.max_splits = max_splits;
    p.eps = a.eps;
    p.scale_log2 = a.scale * 1.4426950408889634f;
    return CRAG_OK;
}

// one new row per sequence: the checks of decode_attention and decode_attention_shared, p.seqs per sequence
int decode_setup(const char *what, const DecodeArgs &a, DecodeParams &p) {
    const int rc = decode_check_shape(what, a);
    if (rc != CRAG_OK) return rc;
    for (int b = 0; b < a.n_seqs; ++b) {
        const int len = a.h_cache_len[b];
        if (len < 0 || len >= a.max_len)
            return efail("%s: cache length %d of sequence %d is outside 0..max_len - 1 = %d", what, len, b, a.max_len - 1);
        if (len >= a.max_pos)
            return efail("%s: position %d of sequence %d is beyond the RoPE table (%d rows)", what, len, b, a.max_pos);
        const int bad = decode_check_slot(what, a, b);
        if (bad != CRAG_OK) return bad;
        p.seqs.len[b] = len;
        p.seqs.slot[b] = a.h_slots[b];
    }
    for (int b = a.n_seqs; b < DECODE_MAX_SEQS; ++b) p.seqs.len[b] = p.seqs.slot[b] = 0;
    return decode_fill(what, a, a.n_seqs, p);
}

// The fork checks: sequence b (slot slots[b], lens[b] rows) reads its first h_shared_len[b] rows in slot h_parent[b].
// from[b] / below[b]: the slot its leading rows come from, and how many rows do.
int fork_check(const char *what, const int32_t *slots, const int32_t *lens, const int32_t *h_parent,
               const int32_t *h_shared_len, int n_seqs, int n_slots, int *from, int *below) {
    for (int b = 0; b < n_seqs; ++b) {
        const int parent = h_parent[b], shared = h_shared_len[b];
        if (parent < 0 || parent >= n_slots)
            return efail("%s: parent %d of sequence %d is outside 0..%d", what, parent, b, n_slots - 1);
        if (shared < 0 || shared > lens[b])
            return efail("%s: shared length %d of sequence %d is outside 0..its cache length %d", what, shared, b, lens[b]);
        const bool forked = parent != slots[b] && shared > 0;
        from[b] = forked ? parent : slots[b];
        below[b] = forked ? shared : lens[b];
        for (int a = 0; forked && a < n_seqs; ++a)   // a shared row must not be the one a parent appends in this call
            if (slots[a] == parent && lens[a] < shared)
                return efail("%s: sequence %d shares %d rows of slot %d, which holds %d", what, b, shared, parent, lens[a]);
    }
    return CRAG_OK;
}

// fork_check for decode_attention_shared and the units of its split launch (p.seqs is checked and filled).  Unit
// b < n_seqs is sequence b alone over the splits no group unit covers; behind them the group units: the sequences of
// the call that read one parent -- the parent itself counts when it is in the call: all of its rows are its own -- in
// units of FORK_UNIT_MEMBERS, over the splits that lie wholly below the shared length of every one of them.
int fork_plan(const DecodeSeqs &seqs, const int32_t *h_parent, const int32_t *h_shared_len, int n_seqs, int n_slots,
              ForkUnits &u, int &n_units) {
    const char *what = "decode_attention_shared";
    if (!h_parent || !h_shared_len) return efail("%s: NULL pointer", what);
    int from[DECODE_MAX_SEQS], below[DECODE_MAX_SEQS];
    const int rc = fork_check(what, seqs.slot, seqs.len, h_parent, h_shared_len, n_seqs, n_slots, from, below);
    if (rc != CRAG_OK) return rc;
    int covered[DECODE_MAX_SEQS] = {};   // leading splits a group unit computes for the sequence
    memset(&u, 0, sizeof(u));
    n_units = n_seqs;
    for (int b = 0; b < n_seqs; ++b) {
        int members[DECODE_MAX_SEQS], count = 0, lowest = below[b];
        for (int a = 0; a < n_seqs; ++a)
            if (from[a] == from[b]) {
                lowest = below[a] < lowest ? below[a] : lowest;
                members[count++] = a;
            }
        const int splits = lowest / DECODE_SPLIT;
        if (members[0] != b || splits == 0) continue;
        // group units of FORK_UNIT_MEMBERS sequences, the rest one more if it is two or more: every unit holds at least
        // two of the n_seqs sequences, so at most DECODE_MAX_SEQS / 2 units are made in all
        for (int m0 = 0; count - m0 >= 2; m0 += FORK_UNIT_MEMBERS) {
            const int n = count - m0 < FORK_UNIT_MEMBERS ? count - m0 : FORK_UNIT_MEMBERS;
            u.n_members[n_units] = n;
            u.s_end[n_units] = splits;
            u.parent[n_units] = u.own[n_units] = from[b];
            u.shared[n_units] = u.n_keys[n_units] = splits * DECODE_SPLIT;
            for (int m = 0; m < n; ++m) {
                u.member[n_units][m] = (int8_t)members[m0 + m];
                covered[members[m0 + m]] = splits;
            }
            ++n_units;
        }
    }
    for (int b = 0; b < n_seqs; ++b) {
        u.n_members[b] = 1;
        u.member[b][0] = (int8_t)b;
        u.s_begin[b] = covered[b];
        u.s_end[b] = seqs.len[b] / DECODE_SPLIT + 1;
        u.parent[b] = from[b];
        u.own[b] = seqs.slot[b];
        u.shared[b] = from[b] == seqs.slot[b] ? 0 : below[b];
        u.n_keys[b] = seqs.len[b] + 1;
    }
    return CRAG_OK;
}

// crag_enc_decode_attention_rows: every check of the entry, p.seqs per ROW (len = the row's position, slot = its
// sequence's) and the units of the split launch: the rows of a sequence in runs of ROWS_UNIT_MEMBERS.
int rows_setup(const DecodeArgs &a, const int32_t *h_new_len, const int32_t *h_parent, const int32_t *h_shared_len,
               DecodeParams &p, RowUnits &u, int &n_rows, int &n_units, int &splits) {
    const char *what = "decode_attention_rows";
    int rc = decode_check_shape(what, a);
    if (rc != CRAG_OK) return rc;
    if (!h_new_len || !h_parent != !h_shared_len) return efail("%s: NULL pointer", what);
    n_rows = 0;
    for (int b = 0; b < a.n_seqs; ++b) {
        const int len = a.h_cache_len[b], add = h_new_len[b];
        if (len < 0) return efail("%s: cache length %d of sequence %d is negative", what, len, b);
        if (add < 1) return efail("%s: sequence %d brings %d new rows, at least one is needed", what, b, add);
        if (add > ROWS_MAX - n_rows)
            return efail("%s: a call takes at most %d new rows in all (sequence %d brings %d behind %d)", what, ROWS_MAX, b,
                         add, n_rows);
        if (len > a.max_len - add || len > a.max_pos - add)
            return efail("%s: rows %d..%d of sequence %d do not fit max_len %d and the RoPE table (%d rows)", what, len,
                         len + add - 1, b, a.max_len, a.max_pos);
        if ((rc = decode_check_slot(what, a, b)) != CRAG_OK) return rc;
        n_rows += add;
    }
    int from[DECODE_MAX_SEQS], below[DECODE_MAX_SEQS];
    for (int b = 0; b < a.n_seqs; ++b) from[b] = a.h_slots[b], below[b] = 0;
    if (h_parent &&
        (rc = fork_check(what, a.h_slots, a.h_cache_len, h_parent, h_shared_len, a.n_seqs, a.n_slots, from, below)) != CRAG_OK)
        return rc;
    if ((rc = decode_fill(what, a, n_rows, p)) != CRAG_OK) return rc;
    memset(&p.seqs, 0, sizeof(p.seqs));
    memset(&u, 0, sizeof(u));
    n_units = splits = 0;
    for (int b = 0, row = 0; b < a.n_seqs; ++b) {
        const int len = a.h_cache_len[b], add = h_new_len[b], slot = a.h_slots[b];
        for (int i = 0; i < add; ++i) {
            p.seqs.len[row + i] = len + i;
            p.seqs.slot[row + i] = slot;
        }
        for (int i0 = 0; i0 < add; i0 += ROWS_UNIT_MEMBERS, ++n_units) {
            const int n = add - i0 < ROWS_UNIT_MEMBERS ? add - i0 : ROWS_UNIT_MEMBERS;
            u.n_members[n_units] = n;
            u.row0[n_units] = row + i0;
            u.n_keys[n_units] = len + i0 + n;   // the last row of the unit sees itself and everything before it
            u.s_end[n_units] = (u.n_keys[n_units] + DECODE_SPLIT - 1) / DECODE_SPLIT;
            u.parent[n_units] = from[b];
            u.own[n_units] = slot;
            u.shared[n_units] = from[b] == slot ? 0 : below[b];
            splits = u.s_end[n_units] > splits ? u.s_end[n_units] : splits;
        }
        row += add;
    }
    return CRAG_OK;
}

}  // namespace

extern "C" {

int64_t crag_enc_decode_workspace_bytes(int n_seqs, int hq, int max_len) {
    if (n_seqs <= 0 || n_seqs > DECODE_MAX_SEQS || hq <= 0 || max_len <= 0) return 0;
    const int64_t splits = ((int64_t)max_len + DECODE_SPLIT - 1) / DECODE_SPLIT;
    const int64_t heads = (int64_t)n_seqs * hq;
    // q_rot (bf16, rounded up to 16 bytes per head anyway) + partial o + partial (m, l)
    return heads * CRAG_HEAD_DIM * 2 + heads * splits * CRAG_HEAD_DIM * 4 + heads * splits * 2 * 4;
}

int crag_enc_decode_attention(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                              const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                              int max_len, const int32_t *h_slots, const int32_t *h_cache_len, int n_seqs, int hq, int hkv,
                              float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                              void *stream) {
    DecodeParams p;
    const DecodeArgs a{qkv_new, q_norm_w, k_norm_w, cos_sin, max_pos, k_cache, v_cache, n_slots, max_len, h_slots,
                       h_cache_len, n_seqs, hq, hkv, eps, scale, workspace, workspace_bytes, out};
    const int rc = decode_setup("decode_attention", a, p);
    if (rc != CRAG_OK) return rc;
    int longest = 0;
    for (int b = 0; b < n_seqs; ++b) longest = p.seqs.len[b] > longest ? p.seqs.len[b] : longest;
    const int splits = longest / DECODE_SPLIT + 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_prepare_kernel, dim3((unsigned)n_seqs), dim3(DECODE_THREADS), 0, st, p);
    const dim3 grid((unsigned)splits, (unsigned)hkv, (unsigned)n_seqs);
    if (hq / hkv == 2)
        hipLaunchKernelGGL(decode_split_kernel<2>, grid, dim3(DECODE_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL(decode_split_kernel<4>, grid, dim3(DECODE_THREADS), 0, st, p);
    hipLaunchKernelGGL(decode_combine_kernel, dim3((unsigned)hq, (unsigned)n_seqs), dim3(CRAG_HEAD_DIM), 0, st, p);
    return hip_ok("decode_attention");
}

int crag_enc_decode_attention_shared(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                                     const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                                     int max_len, const int32_t *h_slots, const int32_t *h_cache_len,
                                     const int32_t *h_parent, const int32_t *h_shared_len, int n_seqs, int hq, int hkv,
                                     float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                                     void *stream) {
    DecodeParams p;
    ForkUnits u;
    int n_units = 0;
    const DecodeArgs a{qkv_new, q_norm_w, k_norm_w, cos_sin, max_pos, k_cache, v_cache, n_slots, max_len, h_slots,
                       h_cache_len, n_seqs, hq, hkv, eps, scale, workspace, workspace_bytes, out};
    int rc = decode_setup("decode_attention_shared", a, p);
    if (rc == CRAG_OK) rc = fork_plan(p.seqs, h_parent, h_shared_len, n_seqs, n_slots, u, n_units);
    if (rc != CRAG_OK) return rc;
    int longest = 0;
    for (int b = 0; b < n_seqs; ++b) longest = p.seqs.len[b] > longest ? p.seqs.len[b] : longest;
    const int splits = longest / DECODE_SPLIT + 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_prepare_kernel, dim3((unsigned)n_seqs), dim3(DECODE_THREADS), 0, st, p);
    const dim3 grid((unsigned)splits, (unsigned)hkv, (unsigned)n_units);
    if (hq / hkv == 2)
        hipLaunchKernelGGL(decode_split_shared_kernel<2>, grid, dim3(DECODE_THREADS), 0, st, p, u);
    else
        hipLaunchKernelGGL(decode_split_shared_kernel<4>, grid, dim3(DECODE_THREADS), 0, st, p, u);
    hipLaunchKernelGGL(decode_combine_kernel, dim3((unsigned)hq, (unsigned)n_seqs), dim3(CRAG_HEAD_DIM), 0, st, p);
    return hip_ok("decode_attention_shared");
}

int crag_enc_decode_attention_rows(const uint16_t *qkv_new, const uint16_t *q_norm_w, const uint16_t *k_norm_w,
                                   const float *cos_sin, int max_pos, uint16_t *k_cache, uint16_t *v_cache, int n_slots,
                                   int max_len, const int32_t *h_slots, const int32_t *h_cache_len, const int32_t *h_new_len,
                                   const int32_t *h_parent, const int32_t *h_shared_len, int n_seqs, int hq, int hkv,
                                   float eps, float scale, void *workspace, int64_t workspace_bytes, uint16_t *out,
                                   void *stream) {
    DecodeParams p;
    RowUnits u;
    int n_rows = 0, n_units = 0, splits = 0;
    const DecodeArgs a{qkv_new, q_norm_w, k_norm_w, cos_sin, max_pos, k_cache, v_cache, n_slots, max_len, h_slots,
                       h_cache_len, n_seqs, hq, hkv, eps, scale, workspace, workspace_bytes, out};
    const int rc = rows_setup(a, h_new_len, h_parent, h_shared_len, p, u, n_rows, n_units, splits);
    if (rc != CRAG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // prepare and combine see the rows of the call as sequences of their own: row r sits at position p.seqs.len[r]
    hipLaunchKernelGGL(decode_prepare_kernel, dim3((unsigned)n_rows), dim3(DECODE_THREADS), 0, st, p);
    const dim3 grid((unsigned)splits, (unsigned)hkv, (unsigned)n_units);
    if (hq / hkv == 2)
        hipLaunchKernelGGL(decode_split_rows_kernel<2>, grid, dim3(DECODE_THREADS), 0, st, p, u);
    else
        hipLaunchKernelGGL(decode_split_rows_kernel<4>, grid, dim3(DECODE_THREADS), 0, st, p, u);
    hipLaunchKernelGGL(decode_combine_kernel, dim3((unsigned)hq, (unsigned)n_rows), dim3(CRAG_HEAD_DIM), 0, st, p);
    return hip_ok("decode_attention_rows");
}

int crag_enc_lm_head(const uint16_t *hidden_states, const uint16_t *delta, const uint16_t *final_norm_w,
                     const uint16_t *lm_head, float *logits, int32_t *token, const int32_t *banned, int n_banned,
                     int n_rows, int hidden, int64_t vocab, float eps, void *stream) {
    if (!hidden_states || !final_norm_w || !lm_head || !logits || !token) return efail("lm_head: NULL pointer");
    if (n_rows < 1 || n_rows > LM_MAX_ROWS) return efail("lm_head: n_rows must be in 1..%d (got %d)", LM_MAX_ROWS, n_rows);
    if (hidden <= 0 || (hidden & 63)) return efail("lm_head: hidden must be a positive multiple of 64 (got %d)", hidden);
    if ((int64_t)n_rows * (hidden + LM_PAD) > CRAG_LM_HEAD_MAX_ELEMS)
        return efail("lm_head: n_rows * (hidden + 8) must not exceed %d (got %d * %d)", CRAG_LM_HEAD_MAX_ELEMS, n_rows,
                     hidden + LM_PAD);
    if (vocab <= 0 || vocab > 0x7fffffff) return efail("lm_head: vocab must be in 1..2^31 - 1");
    if (n_banned < 0 || n_banned > CRAG_LM_HEAD_MAX_BANNED || (n_banned > 0 && !banned))
        return efail("lm_head: n_banned must be in 0..%d, with a list when it is positive", CRAG_LM_HEAD_MAX_BANNED);
    if (((uintptr_t)lm_head | (uintptr_t)hidden_states) & 15) return efail("lm_head: lm_head and hidden_states must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((vocab + LM_ROWS_PER_WG - 1) / LM_ROWS_PER_WG);
    const size_t smem = (size_t)n_rows * (hidden + LM_PAD) * sizeof(u16) + (LM_THREADS / 64) * sizeof(float);
    hipLaunchKernelGGL(lm_head_kernel, dim3(grid), dim3(LM_THREADS), smem, st, hidden_states, delta, final_norm_w, lm_head,
                       logits, n_rows, hidden, vocab, eps);
    hipLaunchKernelGGL(lm_argmax_kernel, dim3((unsigned)n_rows), dim3(ARGMAX_THREADS), 0, st, logits, vocab, banned, n_banned,
                       token);
    return hip_ok("lm_head");
}

}  // extern "C"
