// crag_dedupe.hip -- near-duplicate suppression of ranked lists on the GPU (gfx950), DESIGN.md 4.9.
//
// Per query: a ranked list of up to CRAG_DEDUPE_MAX_WIDTH row ids, best first.  Walking it in rank order, item i is dropped iff
// some KEPT item j < i has cos(row_i, row_j) >= threshold; the lowest such j is its suppressor.  An id that is not
// stored, the -1 pad and a row with 1/||row|| == 0 are kept and never suppress.
//
//   cos(i, j) = clamp(dot(i, j) * (inv_norm[i] * inv_norm[j]), -1, 1)
//   dot(i, j) = sum over the 8 K slices w, in the order w = 0..7, of the slice's chain of v_mfma_f32_32x32x2_f32 steps
//               (== an fmaf chain, 128 terms) over the raw stored rows.
// A step multiplies A[i][k] * B[k][j]; both operands of a pair are loaded by the same routine, so they pair the same
// dims in the same order whichever of the two rows is the A row: the products commute, the chain and the slice sum have
// one order, the norm product commutes -- cos(i, j) and cos(j, i) are the same bits, and they depend on nothing but the
// two rows (not on the slot, the block, the width, the number of queries or the row positions).
//
// One launch, one 512-thread workgroup per query, three phases:
//  1. ids -> row positions: a binary search per item in the ascending stored ids; 1/||row|| of the rows found.
//  2. the list is cut into blocks of 32 items.  For column block bj (ascending) and row block bi <= bj, wave w computes
//     the 32 x 32 partial Gram block over dims [128w, 128w + 128) -- 64 MFMA steps on fragments gathered straight from
//     the tile32 layout (with PS_BIG a row's slice is 512 contiguous bytes) --, the eight partials meet in LDS and are
//     summed in wave order, scaled, clamped and left in a [items][32] panel of cosines of column block bj.
//  3. when a column block's panel is complete every earlier item's fate is known, so one wave walks the block's 32
//     items in order: a ballot over the kept earlier items at or above the threshold, the lowest set bit suppresses.
// The kept ids are then compacted in their order.  Only blocks below ceil(count / 32) are computed.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {
namespace {

constexpr int DD_W = CRAG_DEDUPE_MAX_WIDTH;
constexpr int DD_PANEL_STRIDE = 33;   // floats per panel row: the walk reads a column, one item per lane

static_assert(DD_W == 256, "four 64-bit kept masks, one item per lane and mask");
static_assert(SCAN_THREADS >= 2 * DD_W, "phase 1 and the output use one thread per slot");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct DedupeLds {
    float part[SCAN_WAVES][16][64];          // 32 KiB: the waves' partial Gram blocks, accumulator order
    float panel[DD_W * DD_PANEL_STRIDE];     // cos(item i, item 32 bj + j) of the current column block; NaN: no pair
    int64_t pos[DD_W];                       // row position, -1: not eligible
    float inv[DD_W];                         // 1/||row||, 0: not eligible
    int32_t dup[DD_W];
    float sim[DD_W];
    unsigned long long kept[DD_W / 64];
};

// The wave's K slice of the 32 items of a block as MFMA operand fragments: lane (j = lane & 31, h = lane >> 5) holds
// float4 2t + h of the slice of its item j (row position pos; -1: not eligible, zeros) in f[t].  Step (t, c) of the
// chain takes f[t][c] from every lane: dim 128 w + 8 t + c on lanes 0..31 and dim 128 w + 8 t + 4 + c on lanes 32..63.
template <int PS>
__device__ __forceinline__ void load_block(const float *corpus, int64_t pos, int w, int h, f32x4 (&f)[16]) {
    if (pos >= 0) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
            f[t] = *reinterpret_cast<const f32x4 *>(corpus + row_f4_offset<PS>(pos, w * 32 + 2 * t + h));
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) f[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int PS>
__global__ __launch_bounds__(SCAN_THREADS) void dedupe_kernel(DedupeParams p) {
    __shared__ DedupeLds L;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int count = p.counts[q];
    count = count < 0 ? 0 : (count > p.width ? p.width : count);
    const int64_t *ids = p.ids + (size_t)q * p.width;

    // ---- 1. ids -> positions ----
    int64_t my_id = -1;   // (read here, written at the end: the list may be deduped in place)
    if (tid < DD_W) {
        int64_t pos = -1;
        float inv = 0.f;
        if (tid < count) {
            const int64_t id = my_id = ids[tid];
            int64_t lo = 0, hi = p.size;   // first position whose id is >= id
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (p.stored[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            if (id != -1 && lo < p.size && p.stored[lo] == id) {
                inv = p.inv_norm[lo];
                if (inv > 0.f) pos = lo;
                else inv = 0.f;
            }
        }
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
        load_block<PS>(p.corpus, L.pos[bj * 32 + (lane & 31)], w, lane >> 5, fb);
        for (int bi = 0; bi <= bj; ++bi) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (bi < bj) {
                f32x4 fa[16];
                load_block<PS>(p.corpus, L.pos[bi * 32 + (lane & 31)], w, lane >> 5, fa);
#pragma unroll
                for (int t = 0; t < 16; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t][c], fb[t][c], acc, 0, 0, 0);
            } else {
#pragma unroll
                for (int t = 0; t < 16; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[t][c], fb[t][c], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) L.part[w][r][lane] = acc[r];
            __syncthreads();
            // accumulator register r of lane (j, h) is row (r & 3) + 8 (r >> 2) + 4 h of the A block, column j of the B block
#pragma unroll
            for (int e = tid; e < 1024; e += SCAN_THREADS) {
                const int r = e >> 6, ln = e & 63;
                float s = L.part[0][r][ln];
#pragma unroll
                for (int ww = 1; ww < SCAN_WAVES; ++ww) s += L.part[ww][r][ln];
                const int i = bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), j = ln & 31;
                const float ii = L.inv[i], ij = L.inv[bj * 32 + j];
                float c = s * (ii * ij);
                c = c > 1.f ? 1.f : (c < -1.f ? -1.f : c);   // (a NaN stays one: it suppresses nothing)
                if (!(ii > 0.f) || !(ij > 0.f)) c = __builtin_nanf("");
                L.panel[i * DD_PANEL_STRIDE + j] = c;
            }
            __syncthreads();
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
                    if (c * 64 < gj && i < gj && ((kept[c] >> lane) & 1ull)) hit = L.panel[i * DD_PANEL_STRIDE + jj] >= p.threshold;
                    const unsigned long long m = __ballot(hit);
                    if (sup < 0 && m) sup = c * 64 + __builtin_ctzll(m);
                }
                if (sup < 0) {
#pragma unroll
                    for (int c = 0; c < DD_W / 64; ++c)
                        if ((gj >> 6) == c) kept[c] |= 1ull << (gj & 63);
                } else if (lane == 0) {
                    L.dup[gj] = sup;
                    L.sim[gj] = L.panel[sup * DD_PANEL_STRIDE + jj];
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
    if (p.piece_shift == PS_BIG) hipLaunchKernelGGL(dedupe_kernel<PS_BIG>, dim3(nq), dim3(SCAN_THREADS), 0, st, p);
    else hipLaunchKernelGGL(dedupe_kernel<PS_SMALL>, dim3(nq), dim3(SCAN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag
