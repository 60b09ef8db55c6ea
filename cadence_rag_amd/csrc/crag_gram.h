// crag_gram.h -- the 32 x 32 block of pair cosines that crag_dedupe.hip and crag_mmr.hip are built on, once: both
// operators return THESE bits (tests/test_list_ops_bits_gpu.py pins them to a recording).
//
//   cos(i, j) = clamp(dot(i, j) * (inv_norm[i] * inv_norm[j]), -1, 1), NaN where either item is not comparable
//   dot(i, j) = sum over the 8 K slices w, in the order w = 0..7, of the slice's chain of v_mfma_f32_32x32x2_f32 steps
//               (== an fmaf chain, 128 terms) over the raw stored rows.
// A step multiplies A[i][k] * B[k][j]; both operands of a pair are loaded by load_block, so they pair the same dims in
// the same order whichever of the two rows is the A row: the products commute, the chain and the slice sum have one
// order, the norm product commutes -- cos(i, j) and cos(j, i) are the same bits, and they depend on nothing but the two
// rows.  A workgroup of SCAN_THREADS computes a block: wave w the partial block over dims [128w, 128w + 128)
// (gram_block_partial), then all of them the sum, the scale and the clamp (gram_block_cosines).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float GramPartials[SCAN_WAVES][16][64];   // 32 KiB of LDS: the waves' partial blocks, accumulator order
constexpr int GRAM_STRIDE = 33;                   // floats per row of a finished block in LDS: a column reads without conflicts

// The wave's K slice of the 32 items of a block as MFMA operand fragments: lane (j = lane & 31, h = lane >> 5) holds
// float4 2t + h of the slice of its item j (row position pos; -1: not comparable, zeros) in f[t].  Step (t, c) of the
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

// Wave w's partial of the block (row items A) x (column items B): the 64-step chain.  pos_a is the position of this
// lane's item (lane & 31) of the A block, fb the lane's fragments of the B block; on the diagonal (A is B: uniform over
// the workgroup) nothing more is loaded.
template <int PS>
__device__ __forceinline__ f32x16 gram_block_partial(const float *corpus, int64_t pos_a, const f32x4 (&fb)[16], bool diagonal,
                                                     int w, int lane) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (!diagonal) {
        f32x4 fa[16];
        load_block<PS>(corpus, pos_a, w, lane >> 5, fa);
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
    return acc;
}

// ... for a caller that holds no fragments of the B block yet: pos_b is the position of the lane's item of the B block
template <int PS>
__device__ __forceinline__ f32x16 gram_block_partial(const float *corpus, int64_t pos_a, int64_t pos_b, bool diagonal, int w,
                                                     int lane) {
    f32x4 fb[16];
    load_block<PS>(corpus, pos_b, w, lane >> 5, fb);
    return gram_block_partial<PS>(corpus, pos_a, fb, diagonal, w, lane);
}

// The eight partials meet in LDS and become the block's cosines: summed in wave order, scaled by the two 1/||row||
// (inv_a[32] of the row items, inv_b[32] of the column items; 0: not comparable), clamped, NaN where either item is not
// comparable; cos(row item i, column item j) goes to dst[i * stride + j].  Called by the whole workgroup; a barrier
// in front of the sum and one behind the block.
__device__ __forceinline__ void gram_block_cosines(const f32x16 &acc, GramPartials &part, const float *inv_a, const float *inv_b,
                                                   float *dst, int stride) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[w][r][lane] = acc[r];
    __syncthreads();
    // accumulator register r of lane (j, h) is row (r & 3) + 8 (r >> 2) + 4 h of the A block, column j of the B block
#pragma unroll
    for (int e = tid; e < 1024; e += SCAN_THREADS) {
        const int r = e >> 6, ln = e & 63;
        float s = part[0][r][ln];
#pragma unroll
        for (int ww = 1; ww < SCAN_WAVES; ++ww) s += part[ww][r][ln];
        const int i = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), j = ln & 31;
        const float ii = inv_a[i], ij = inv_b[j];
        float c = s * (ii * ij);
        c = c > 1.f ? 1.f : (c < -1.f ? -1.f : c);   // (a NaN stays one)
        if (!(ii > 0.f) || !(ij > 0.f)) c = __builtin_nanf("");
        dst[i * stride + j] = c;
    }
    __syncthreads();
}

}  // namespace crag
