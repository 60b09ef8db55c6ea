// crag_mmr.hip -- maximal marginal relevance over ranked lists on the GPU (gfx950), DESIGN.md 4.15.
//
// Per query: up to CRAG_MMR_MAX_WIDTH (id, relevance) slots.  A slot is a CANDIDATE when it lies below the count, its id
// is not -1, its relevance is finite and no earlier slot below the count holds the same id; a candidate is COMPARABLE
// when its id is stored with 1/||row|| > 0 (dedupe's eligibility).  k times, while candidates remain, the candidate with
// the largest
//     value[i] = lambda * rel[i] - mu * pen[i]          (fp32 mul, mul, sub: three roundings, never contracted)
// is picked, equal values going to the lower id; pen[i] is 0 until a picked comparable item p meets a comparable i, then
// the largest cos(p, i) so far.  An item that is not comparable is never penalised and never penalises.
//
//   cos(i, j) is crag_gram.h's block of pair cosines, the one crag_dedupe.hip runs: the same code, hence the same bits.
//   cos(i, j) and cos(j, i) are the same bits and depend on the two rows alone.
//
// Two launches:
//  1. mmr_gram_kernel<PS>: grid (block pairs bi <= bj of 32 slots, queries), 512 threads.  A workgroup finds the row
//     positions of its two blocks (comparable_row, crag_rows.h), computes the (bi, bj) block -- gram_block_partial per
//     wave, gram_block_cosines -- and writes the block and its transpose into the query's [width_pad, width_pad]
//     matrix in the scratch, NaN where either item is not comparable.  Only block pairs below ceil(count / 32) are
//     computed; the walk reads nothing else.
//  2. mmr_walk_kernel: one 256-thread workgroup per query, one thread per slot.  Candidates and the rank of each id
//     among the list's ids (the tie-break) from an all-pairs compare in LDS; per pick the values, a workgroup argmax
//     over the 64-bit key (f2ord(value), 255 - id rank, slot), one coalesced read of the pick's Gram row, the penalty
//     update, the row to out_sim_rows when asked.
// Plain vector stores only, no atomics: the outputs are a function of the inputs alone, from run to run.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_exact.h"
#include "crag_gram.h"
#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {
namespace {

constexpr int MM_W = CRAG_MMR_MAX_WIDTH;

static_assert(MM_W == 256, "the walk runs one thread per slot in a 256-thread workgroup; slot and rank share a key word");

struct GramLds {
    GramPartials part;
    float tile[32 * GRAM_STRIDE];       // cos(item 32 bi + i, item 32 bj + j); NaN: no pair.  The transposed write reads a column
    int64_t pos[64];                    // row position of the items of block bi (0..31) and bj (32..63), -1: not comparable
    float inv[64];                      // 1/||row||, 0: not comparable
};

__device__ __forceinline__ int mmr_width_pad(int width) { return (width + 31) & ~31; }

template <int PS>
__global__ __launch_bounds__(SCAN_THREADS) void mmr_gram_kernel(MmrParams p) {
    __shared__ GramLds L;
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = clamp_count(p.counts[q], p.width);
    // block pair blockIdx.x -> (bi <= bj), column blocks ascending
    int bj = 0;
    while ((bj + 1) * (bj + 2) / 2 <= (int)blockIdx.x) ++bj;
    const int bi = (int)blockIdx.x - bj * (bj + 1) / 2;
    if (bj >= ((count + 31) >> 5)) return;   // (uniform: the whole workgroup leaves)
    const int wp = mmr_width_pad(p.width);
    float *gram = p.gram + (size_t)q * wp * wp;

    // ---- ids -> positions of the two blocks ----
    if (tid < 64) {
        const int slot = (tid < 32 ? bi : bj) * 32 + (tid & 31);
        int64_t pos = -1;
        float inv = 0.f;
        if (slot < count) comparable_row(p.rows, p.ids[(size_t)q * p.width + slot], pos, inv);
        L.pos[tid] = pos;
        L.inv[tid] = inv;
    }
    __syncthreads();

    // ---- the block pair's cosines: one K slice per wave, then the eight partials in LDS ----
    const f32x16 acc = gram_block_partial<PS>(p.rows.corpus, L.pos[lane & 31], L.pos[32 + (lane & 31)], bi == bj, w, lane);
    gram_block_cosines(acc, L.part, L.inv, L.inv + 32, L.tile, GRAM_STRIDE);
    // ---- the block and its transpose, rows of 32 consecutive floats each ----
#pragma unroll
    for (int e = tid; e < 1024; e += SCAN_THREADS) {
        const int a = e >> 5, b = e & 31;
        gram[(size_t)(bi * 32 + a) * wp + bj * 32 + b] = L.tile[a * GRAM_STRIDE + b];
        if (bi < bj) gram[(size_t)(bj * 32 + a) * wp + bi * 32 + b] = L.tile[b * GRAM_STRIDE + a];
    }
}

__global__ __launch_bounds__(MM_W) void mmr_walk_kernel(MmrParams p) {
    __shared__ int64_t s_id[MM_W];
    __shared__ unsigned long long s_best[2][MM_W / 64];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = clamp_count(p.counts[q], p.width);
    const int wp = mmr_width_pad(p.width);
    const float *gram = p.gram + (size_t)q * wp * wp;
    const float nan = __builtin_nanf("");

    // ---- candidates, and the rank of each candidate's id among the list's ids ----
    int64_t id = -1;
    float rel = nan;
    if (tid < count) {
        id = p.ids[(size_t)q * p.width + tid];
        rel = p.rel[(size_t)q * p.width + tid];
    }
    s_id[tid] = id;
    __syncthreads();
    bool cand = tid < count && id != -1 && (__float_as_uint(rel) & 0x7f800000u) != 0x7f800000u;
    int rank = 0;
    if (cand) {
        for (int s = 0; s < count; ++s) {
            const int64_t other = s_id[s];
            rank += other < id;
            if (s < tid && other == id) cand = false;
        }
    }

    // ---- the picks ----
    float pen = 0.f;
    bool has_pen = false, picked = false;
    const size_t o = (size_t)q * p.k;
    int t = 0;
    for (; t < p.k; ++t) {
        float v;
        {
#pragma clang fp contract(off)
            const float a = p.lambda * rel;
            const float b = p.mu * pen;
            v = a - b;
        }
        unsigned long long key = 0ull;   // larger = better: value, then the lower id; 0: not in the running
        if (cand && !picked)
            key = mk64(f2ord(v == 0.f ? 0.f : v), ((uint32_t)(MM_W - 1 - rank) << 16) | (uint32_t)tid);   // (-0 ties +0)
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) {
            const unsigned long long other = __shfl_xor(key, x);
            key = other > key ? other : key;
        }
        if (lane == 0) s_best[t & 1][w] = key;
        __syncthreads();   // (one barrier a pick: the next pick writes the other half of s_best)
        unsigned long long best = s_best[t & 1][0];
#pragma unroll
        for (int ww = 1; ww < MM_W / 64; ++ww) best = s_best[t & 1][ww] > best ? s_best[t & 1][ww] : best;
        if (best == 0ull) break;   // (uniform) no candidate is left
        const int pick = (int)(best & 0xffffull);
        const float s = cand ? gram[(size_t)pick * wp + tid] : nan;   // NaN: the pair is not comparable
        if (tid == pick) {
            picked = true;
            p.out_ids[o + t] = id;
            p.out_rel[o + t] = rel;
            if (p.out_value) p.out_value[o + t] = v;
            if (p.out_slots) p.out_slots[o + t] = tid;
        }
        if (s == s) {
            pen = has_pen ? (s > pen ? s : pen) : s;
            has_pen = true;
        }
        if (p.out_sim_rows && tid < p.width) p.out_sim_rows[(o + t) * p.width + tid] = s;
    }

    // ---- padding behind the picks ----
    for (int e = t + tid; e < p.k; e += MM_W) {
        p.out_ids[o + e] = -1;
        p.out_rel[o + e] = nan;
        if (p.out_value) p.out_value[o + e] = nan;
        if (p.out_slots) p.out_slots[o + e] = -1;
    }
    if (p.out_sim_rows)
        for (int e = tid; e < (p.k - t) * p.width; e += MM_W) p.out_sim_rows[(o + t) * p.width + e] = nan;
    if (tid == 0) p.out_counts[q] = t;
}

}  // namespace

int64_t mmr_scratch_bytes(int nq, int width) {
    const int64_t wp = ((int64_t)(width > 1 ? width : 1) + 31) & ~(int64_t)31;
    return (int64_t)(nq > 1 ? nq : 1) * wp * wp * (int64_t)sizeof(float);
}

hipError_t launch_mmr(const MmrParams &p, hipStream_t st) {
    if (p.nq <= 0) return hipSuccess;
    const int nbw = (p.width + 31) >> 5;
    const dim3 grid(nbw * (nbw + 1) / 2, p.nq);
    if (p.rows.piece_shift == PS_BIG) hipLaunchKernelGGL(mmr_gram_kernel<PS_BIG>, grid, dim3(SCAN_THREADS), 0, st, p);
    else hipLaunchKernelGGL(mmr_gram_kernel<PS_SMALL>, grid, dim3(SCAN_THREADS), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mmr_walk_kernel, dim3(p.nq), dim3(MM_W), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag
