// crag_layout.h -- the tile32 row layout and the one routine that writes a row into it, shared by the layout kernels
// of crag_search.hip (store_rows_kernel) and the edit kernels of crag_edit.hip (scattered store, row move, tail clear).
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_kernels.h"

namespace crag {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a row piece = 2^PS float4 (template parameter PS of everything that touches the fp32 rows).  Two layouts:
//  * PS_SMALL = 2 (64-byte pieces) for an index WITHOUT the fp16 mirror, whose every search streams the fp32 rows: a scan
//    instruction reads half of each line it touches and the next one the other half.  [Measured against 3 and 4 on
//    one box: with 128-byte pieces a scan instruction reads a quarter of each line and the scan of the fp32 rows
//    slows from 73 to 83 us at 100 000 rows x 64 queries.]
//  * PS_BIG = 5 (512-byte pieces = a wave's whole K slice of a row) for an index WITH the mirror (the default): there
//    the fp32 rows are read by the exact rescoring of the prefilter path -- a survivor's row is then 8 x 512 contiguous
//    bytes in full 128-byte lines, where 64-byte pieces use half of every line they fetch: the 8 400 rows x 4 KiB of a
//    top-100 search over 64 queries were 10-16 us of a 28 us selection launch, HBM-bound at twice the useful bytes --
//    and by the fp32 scans of small corpora, irregular indices and the overflow fallback, which are latency-bound or
//    rare (and ~13 % slower per byte in this layout).
constexpr int PS_SMALL = 2, PS_BIG = 5;

// float offset of the float4 that holds dims [4kq, 4kq+3] of the row at position `row`
template <int PS>
__device__ __forceinline__ size_t row_f4_offset(int64_t row, int kq) {
    return (size_t)(row >> 5) * TILE_FLOATS + ((size_t)(kq >> PS) * 32 + (row & 31)) * (4 << PS) + (kq & ((1 << PS) - 1)) * 4;
}

// _Float16 offset of mirror piece p (0..127, 16 bytes each: K slice w = p >> 4, k-step t8 = (p >> 1) & 7, half
// h = p & 1) of the row at position `row` -- everything of the fp16 mirror that belongs to that row
__device__ __forceinline__ size_t row_mirror_piece_offset(int64_t row, int p) {
    const int w = p >> 4, t8 = (p >> 1) & 7, h = p & 1;
    return ((((size_t)(row >> 5) * SCAN_WAVES + w) * 8 + t8) * 64 + h * 32 + (size_t)(row & 31)) * 8;
}

__device__ __forceinline__ double block_sum_256(double v, double *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wv] = v;
    __syncthreads();
    const double t = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return t;
}

// a norm far outside fp32's comfortable range: an index that holds such a row is kept off the fp16 prefilter path
__device__ __forceinline__ bool irregular_inv_norm(float inv) { return inv > 0.f && (inv < 1.0e-30f || inv > 1.0e30f); }

// One row ([dim] fp32 at src) -> tile32 layout at row position `row`; also 1/||row||.  Called by all 256 threads of a
// block: thread kq moves dims [4kq, 4kq+3].
// With a mirror (nullable): the unit row rounded to fp16, in the order the prefilter scan's MFMA wants its B
// operand -- [tile][K slice w][k-step t8][lane (h, j)][8 halves], the halves being dims 128w + 16 t8 + 8 (e >> 2) +
// 4h + (e & 3) -- computed exactly as the scan would on the fly (fp32 multiply by 1/||row||, v_cvt_pk_f16_f32), so a
// scan of the mirror sees bit for bit the operand a scan of the fp32 rows builds in registers.
template <int PS>
__device__ __forceinline__ void store_row(const float *src, int dim, int64_t row, float *corpus, float *inv_norm,
                                          uint32_t *irregular, _Float16 *mirror) {
    __shared__ double sh[4];
    __shared__ float sh_inv;
    const int kq = threadIdx.x;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (4 * kq + 3 < dim && (dim & 3) == 0) {
        v = *reinterpret_cast<const f32x4 *>(src + 4 * kq);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * kq + c < dim) v[c] = src[4 * kq + c];
    }
    float *dst = corpus + row_f4_offset<PS>(row, kq);
    *reinterpret_cast<f32x4 *>(dst) = v;
    double ss = (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
    ss = block_sum_256(ss, sh);
    if (kq == 0) {
        // zero or non-finite norm (NaN/Inf anywhere in the row) => never eligible
        const bool ok = (ss > 0.0) && (ss < 1.0e300) && (ss == ss);
        float inv = ok ? (float)(1.0 / sqrt(ss)) : 0.f;
        if (!(inv > 0.f) || !(inv < 3.0e38f)) inv = 0.f;
        inv_norm[row] = inv;
        sh_inv = inv;
        if (irregular_inv_norm(inv)) *irregular = 1u;
    }
    if (mirror) {
        __syncthreads();
        const float inv = sh_inv;
        typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
        typedef float f32x2_t __attribute__((ext_vector_type(2)));
        const f32x4 u = v * inv;
        const f16x2_t lo = __builtin_convertvector((f32x2_t{u[0], u[1]}), f16x2_t);
        const f16x2_t hi = __builtin_convertvector((f32x2_t{u[2], u[3]}), f16x2_t);
        f16x4_t o = f16x4_t{lo[0], lo[1], hi[0], hi[1]};
        if (!(inv > 0.f)) {  // never eligible: NaN scores, whatever the query
            const _Float16 qnan = __builtin_bit_cast(_Float16, (unsigned short)0x7e00);
            o = f16x4_t{qnan, qnan, qnan, qnan};
        }
        const int w = kq >> 5, d = (4 * kq) & 127, t8 = d >> 4, g = (d >> 3) & 1, h = (d >> 2) & 1;
        const size_t idx = ((((size_t)(row >> 5) * SCAN_WAVES + w) * 8 + t8) * 64 + h * 32 + (size_t)(row & 31)) * 8 + 4 * g;
        *reinterpret_cast<f16x4_t *>(mirror + idx) = o;
    }
}

}  // namespace crag
