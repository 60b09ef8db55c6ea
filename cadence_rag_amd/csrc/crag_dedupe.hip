// crag_dedupe.hip -- near-duplicate suppression of ranked lists on the GPU (gfx950), DESIGN.md 4.9.
//
// Per query: a ranked list of up to CRAG_DEDUPE_MAX_WIDTH row ids, best first.  Walking it in rank order, item i is dropped iff
// some KEPT item j < i has cos(row_i, row_j) >= threshold; the lowest such j is its suppressor.  An id that is not
// stored, the -1 pad and a row with 1/||row|| == 0 are kept and never suppress.
//
// The cosines are crag_gram.h's: cos(i, j) and cos(j, i) are the same bits, and they depend on nothing but the two rows
// (not on the slot, the block, the width, the number of queries or the row positions).
//
// One launch, one 512-thread workgroup per query, three phases:
//  1. ids -> row positions and 1/||row|| of the eligible items (comparable_row, crag_rows.h).
//  2. the list is cut into blocks of 32 items.  For column block bj (ascending) and row block bi <= bj, wave w computes
//     the 32 x 32 partial Gram block over dims [128w, 128w + 128) -- 64 MFMA steps on fragments gathered straight from
//     the tile32 layout (with PS_BIG a row's slice is 512 contiguous bytes) --, and the block's cosines are left in a
//     [items][32] panel of cosines of column block bj.  The column block's fragments are loaded once per bj.
//  3. when a column block's panel is complete every earlier item's fate is known, so one wave walks the block's 32
//     items in order: a ballot over the kept earlier items at or above the threshold, the lowest set bit suppresses.
// The kept ids are then compacted in their order.  Only blocks below ceil(count / 32) are computed.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_gram.h"
#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {
namespace {

constexpr int DD_W = CRAG_DEDUPE_MAX_WIDTH;

static_assert(DD_W == 256, "four 64-bit kept masks, one item per lane and mask");
static_assert(SCAN_THREADS >= 2 * DD_W, "phase 1 and the output use one thread per slot");

struct DedupeLds {
    GramPartials part;
    float panel[DD_W * GRAM_STRIDE];         // cos(item i, item 32 bj + j) of the current column block; NaN: no pair
    int64_t pos[DD_W];                       // row position, -1: not eligible
    float inv[DD_W];                         // 1/||row||, 0: not eligible
    int32_t dup[DD_W];
    float sim[DD_W];
    unsigned long long kept[DD_W / 64];
};

template <int PS>
__global__ __launch_bounds__(SCAN_THREADS) void dedupe_kernel(DedupeParams p) {
    __shared__ DedupeLds L;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = clamp_count(p.counts[q], p.width);
    const int64_t *ids = p.ids + (size_t)q * p.width;

    // ---- 1. ids -> positions ----
    int64_t my_id = -1;   // (read here, written at the end: the list may be deduped in place)
    if (tid < DD_W) {
        int64_t pos = -1;
        float inv = 0.f;
        if (tid < count) comparable_row(p.rows, my_id = ids[tid], pos, inv);
        L.pos[tid] = pos;
        L.inv[tid] = inv;
        L.dup[tid] = -1;
        L.sim[tid] = __builtin_nanf("");
    }
    __syncthreads();

    const int nb = (count + 31) >> 5;
    unsigned long long kept[DD_W / 64] = {0ull, 0ull, 0ull, 0ull};   // wave 0's, uniform
    for (int bj = 0; bj < nb; ++bj) {
        // ---- 2. the column block's panel ----
        f32x4 fb[16];
        load_block<PS>(p.rows.corpus, L.pos[bj * 32 + (lane & 31)], w, lane >> 5, fb);
        for (int bi = 0; bi <= bj; ++bi) {
            const f32x16 acc = gram_block_partial<PS>(p.rows.corpus, L.pos[bi * 32 + (lane & 31)], fb, bi == bj, w, lane);
            gram_block_cosines(acc, L.part, L.inv + bi * 32, L.inv + bj * 32, L.panel + bi * 32 * GRAM_STRIDE, GRAM_STRIDE);
        }
        // ---- 3. the walk over the column block's items ----
        if (w == 0) {
            const int j_end = (count - bj * 32) < 32 ? (count - bj * 32) : 32;
            for (int jj = 0; jj < j_end; ++jj) {
                const int gj = bj * 32 + jj;
                int sup = -1;
#pragma unroll
                for (int c = 0; c < DD_W / 64; ++c) {
                    const int i = c * 64 + lane;
                    bool hit = false;
                    if (c * 64 < gj && i < gj && ((kept[c] >> lane) & 1ull)) hit = L.panel[i * GRAM_STRIDE + jj] >= p.threshold;
                    const unsigned long long m = __ballot(hit);
                    if (sup < 0 && m) sup = c * 64 + __builtin_ctzll(m);
                }
                if (sup < 0) {
#pragma unroll
                    for (int c = 0; c < DD_W / 64; ++c)
                        if ((gj >> 6) == c) kept[c] |= 1ull << (gj & 63);
                } else if (lane == 0) {
                    L.dup[gj] = sup;
                    L.sim[gj] = L.panel[sup * GRAM_STRIDE + jj];
                }
            }
        }
        __syncthreads();
    }
    if (w == 0 && lane < DD_W / 64) {
        unsigned long long k = kept[0];
#pragma unroll
        for (int c = 1; c < DD_W / 64; ++c)
            if (lane == c) k = kept[c];
        L.kept[lane] = k;
    }
    __syncthreads();

    // ---- output: kept ids compacted in their order ----
    if (tid < p.width) {
        const size_t o = (size_t)q * p.width;
        int total = 0, rank = 0;
#pragma unroll
        for (int c = 0; c < DD_W / 64; ++c) {
            const unsigned long long k = L.kept[c];
            total += __popcll(k);
            if (c < (tid >> 6)) rank += __popcll(k);
            else if (c == (tid >> 6)) rank += __popcll(k & ((1ull << (tid & 63)) - 1ull));
        }
        if (tid >= total) p.out_ids[o + tid] = -1;
        if ((L.kept[tid >> 6] >> (tid & 63)) & 1ull) p.out_ids[o + rank] = my_id;
        if (tid == 0) p.out_counts[q] = total;
        if (p.out_dup_of) p.out_dup_of[o + tid] = L.dup[tid];
        if (p.out_sim) p.out_sim[o + tid] = L.sim[tid];
    }
}

}  // namespace

hipError_t launch_dedupe(const DedupeParams &p, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (p.rows.piece_shift == PS_BIG) hipLaunchKernelGGL(dedupe_kernel<PS_BIG>, dim3(nq), dim3(SCAN_THREADS), 0, st, p);
    else hipLaunchKernelGGL(dedupe_kernel<PS_SMALL>, dim3(nq), dim3(SCAN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag
