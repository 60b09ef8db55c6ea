// crag_exact.h -- the exact-score arithmetic of the dense lane, in one place: the 64-bit candidate key, the canonical
// 1/||q||, one 128-dim slice of the exact fp32 dot product and the score -> key expression.  crag_search.hip (the scans
// and the selection kernel), crag_subset.hip (the search over id lists) and crag_group.hip (the search with a cap per
// group) include it, so a (query, row) pair has the same score bits on every path; crag_mmr.hip includes it for the key
// helpers of its walk (its cosines are crag_gram.h's, not these scores).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {

// ------------------------------------------------------------------------------------------
// key helpers: a candidate is the 64-bit key (orderable(score) << 32) | ~row ; larger = better
// (higher score, then lower row position).  Key 0 is the "empty" sentinel.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2ord(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t mk64(uint32_t hi, uint32_t lo) {
    return ((uint64_t)hi << 32) | lo;
}

// Bitonic sort of P keys in LDS (P a power of two), descending, by the SCAN_THREADS threads of a workgroup; the keys are
// in order behind the barrier the last pass ends with.  (subset_select_kernel, group_select_kernel)
__device__ __forceinline__ void sort_keys_desc(uint64_t *keys, int P) {
    const int tid = threadIdx.x;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += SCAN_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = keys[i], b = keys[l];
                const bool desc = (i & k2) == 0;
                if (desc ? a < b : a > b) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
}

// ---- the canonical 1/||q||: ONE piece of arithmetic for every kernel that needs a query's norm -------------------
// Thread t < 256 holds dims 4t .. 4t+3 of the query (zeros beyond dim / for threads >= 256); squares in fp64, a
// butterfly sum inside each of the first four waves, the four wave sums added in wave order.  prep_queries_kernel,
// the selection kernel and the fallback scan all call this, so the exact scores (x 1/||row|| x 1/||q||) are the same
// bits on every path.  All threads of the workgroup must call it (two barriers); sh: 4 doubles of LDS.
__device__ __forceinline__ f32x4 load_query_quad(const float *queries, int dim, int q, int nq, int t) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q < nq && t < 256) {
        const float *src = queries + (size_t)q * dim;
        if ((dim & 3) == 0) {
            if (4 * t < dim) v = *reinterpret_cast<const f32x4 *>(src + 4 * t);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * t + c < dim) v[c] = src[4 * t + c];
        }
    }
    return v;
}

// s + (the s of lane ^ X), the exchange on the VALU: the two halves of the double travel as two 32-bit registers.
// [__shfl_xor of a double is two ds_bpermute, an LDS round trip per stage of a chain in which every stage waits for the
// one before.]  X = 32 / 16: v_permlane32_swap / v_permlane16_swap of a register with itself leave {own, partner} in
// the lanes whose bit X is clear and {partner, own} in the others; the sum of the two is own + partner in either (an fp
// add is commutative bit for bit; only which NaN payload survives depends on the order, and a NaN total is discarded).
// X < 16: DPP inside the 16-lane row -- row_ror:8, row_half_mirror then quad_perm [3,2,1,0] (^7 ^3 = ^4), quad_perm
// [2,3,0,1], quad_perm [1,0,3,2].  All 64 lanes must be active.
template <int X>
__device__ __forceinline__ double lane_xor_add_f64(double s) {
    const uint64_t u = (uint64_t)__double_as_longlong(s);
    const uint32_t lo = (uint32_t)u, hi = (uint32_t)(u >> 32);
    if constexpr (X == 32 || X == 16) {
        uint32_t l0, l1, h0, h1;
        if constexpr (X == 32) {
            const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
            const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
            l0 = l[0], l1 = l[1], h0 = h[0], h1 = h[1];
        } else {
            const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
            const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
            l0 = l[0], l1 = l[1], h0 = h[0], h1 = h[1];
        }
        return __longlong_as_double((long long)(((uint64_t)h0 << 32) | l0)) +
               __longlong_as_double((long long)(((uint64_t)h1 << 32) | l1));
    } else {
        static_assert(X == 8 || X == 4 || X == 2 || X == 1, "lane_xor_add_f64: no pattern");
        uint32_t pl, ph;
        if constexpr (X == 4) {
            pl = (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)lo, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
            ph = (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)hi, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
        } else {
            constexpr int ctrl = X == 8 ? 0x128 : (X == 2 ? 0x4E : 0xB1);
            pl = (uint32_t)__builtin_amdgcn_mov_dpp((int)lo, ctrl, 0xF, 0xF, true);
            ph = (uint32_t)__builtin_amdgcn_mov_dpp((int)hi, ctrl, 0xF, 0xF, true);
        }
        return s + __longlong_as_double((long long)(((uint64_t)ph << 32) | pl));
    }
}

// The sum of 8 consecutive lanes' values in lane order, d = p0; d += p1; ... d += p7 (the scan kernels' split-K
// reduction order), valid in the FIRST lane of each aligned group of 8: DPP row shifts (row_shl:n: lane i reads lane
// i + n of its 16-lane row, which holds two groups) in place of eight ds_bpermute shuffles.  The other lanes of a group
// end with a sum that runs into the next group or into zeros.  All 64 lanes must be active.
__device__ __forceinline__ float group8_sum_in_order(float part) {
    float d = part;
#define CRAG_SHL_(N_) d += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(part), 0x100 + (N_), 0xF, 0xF, true))
    CRAG_SHL_(1);
    CRAG_SHL_(2);
    CRAG_SHL_(3);
    CRAG_SHL_(4);
    CRAG_SHL_(5);
    CRAG_SHL_(6);
    CRAG_SHL_(7);
#undef CRAG_SHL_
    return d;
}

__device__ __forceinline__ float canonical_qinv(const f32x4 v, bool real_query, double *sh) {
    double ss = ((double)v[0] * v[0] + (double)v[1] * v[1]) + ((double)v[2] * v[2] + (double)v[3] * v[3]);
    // butterfly in the order xor 32, 16, 8, 4, 2, 1 (the pairing decides the rounding: it is part of the result)
    ss = lane_xor_add_f64<32>(ss);
    ss = lane_xor_add_f64<16>(ss);
    ss = lane_xor_add_f64<8>(ss);
    ss = lane_xor_add_f64<4>(ss);
    ss = lane_xor_add_f64<2>(ss);
    ss = lane_xor_add_f64<1>(ss);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0 && wv < 4) sh[wv] = ss;
    __syncthreads();
    const double tot = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const bool ok = real_query && (tot > 0.0) && (tot < 1.0e300) && (tot == tot);
    float qinv = ok ? (float)(1.0 / sqrt(tot)) : 0.f;
    if (!(qinv < 3.0e38f)) qinv = 0.f;
    return qinv;
}

// score -> key for one owned (query, row) pair
// (the pipelined kernels' and the selection kernel's expression, so that all of them produce the same bits:
// scale = 1/||row|| * 1/||q||, or 0 when the pair is not eligible)
__device__ __forceinline__ void make_key(float dot, float scale, int64_t row, uint32_t &khi, uint32_t &klo) {
    float sc = dot * scale;
    sc = __builtin_amdgcn_fmed3f(sc, -1.f, 1.f);  // pgvector clamps the similarity to [-1, 1]
    const bool ok = (scale > 0.f) && (sc == sc);
    khi = ok ? f2ord(sc) : 0u;
    klo = ok ? ~(uint32_t)row : 0u;
}

// One 128-dim slice of the exact dot product: the query slice comes from LDS (fragment order), the row's 32
// float4 are fetched first, all of them (32 independent 16-byte loads in flight, four per 64-byte piece of the
// row: latency is everything here), then the fmaf chain runs in the scan's k order:
// s = 0..15, then component, then lane half (k = 0, 1 of one 32x32x2 MFMA).
template <int PS>
__device__ __forceinline__ float exact_slice_dot(const f32x4 *qslice /* [16][2] float4 in LDS */,
                                                 const f32x4 *ctile /* tile base + slice */, int jrow) {
    f32x4 c0[16], c1[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        // float4 kq = 2s (and 2s + 1) of the slice: piece kq >> PS of the row
        c0[s] = ctile[(((2 * s) >> PS) * 32 + jrow) * (1 << PS) + ((2 * s) & ((1 << PS) - 1))];
        c1[s] = ctile[(((2 * s) >> PS) * 32 + jrow) * (1 << PS) + ((2 * s) & ((1 << PS) - 1)) + 1];
    }
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const f32x4 q0 = qslice[2 * s], q1 = qslice[2 * s + 1];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            acc = __builtin_fmaf(q0[cc], c0[s][cc], acc);
            acc = __builtin_fmaf(q1[cc], c1[s][cc], acc);
        }
    }
    return acc;
}

// exact_slice_dot in two halves, for a kernel that scores one row against many queries (crag_group.hip): the fetch of
// the row's 32 float4 -- the same addresses, c0[s] / c1[s] = float4 2s / 2s + 1 of the slice -- and the fmaf chain in
// the same order over a slice that is already in registers.  exact_slice_fma(q, fetched row) is exact_slice_dot(q, row)
// bit for bit.
template <int PS>
__device__ __forceinline__ void exact_slice_fetch(const f32x4 *ctile /* tile base + slice */, int jrow, f32x4 (&c0)[16],
                                                  f32x4 (&c1)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        c0[s] = ctile[(((2 * s) >> PS) * 32 + jrow) * (1 << PS) + ((2 * s) & ((1 << PS) - 1))];
        c1[s] = ctile[(((2 * s) >> PS) * 32 + jrow) * (1 << PS) + ((2 * s) & ((1 << PS) - 1)) + 1];
    }
}

// (the query slice is read from LDS eight float4 -- four steps s -- ahead of the chain that uses them, in two register
// sets used in turn: a kernel that keeps a whole row slice in registers runs at two waves per SIMD, where a read that the
// chain waits for costs its whole latency; the scheduling fences keep the compiler from sinking the reads to their uses)
__device__ __forceinline__ void slice_query_read(const f32x4 *qslice, int h, f32x4 (&q)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = qslice[8 * h + i];
}
__device__ __forceinline__ float slice_query_fma(float acc, int h, const f32x4 (&q)[8], const f32x4 (&c0)[16],
                                                 const f32x4 (&c1)[16]) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        const f32x4 q0 = q[2 * s4], q1 = q[2 * s4 + 1];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            acc = __builtin_fmaf(q0[cc], c0[4 * h + s4][cc], acc);
            acc = __builtin_fmaf(q1[cc], c1[4 * h + s4][cc], acc);
        }
    }
    return acc;
}
__device__ __forceinline__ float exact_slice_fma(const f32x4 *qslice /* [16][2] float4 in LDS */, const f32x4 (&c0)[16],
                                                 const f32x4 (&c1)[16]) {
    f32x4 qa[8], qb[8];
    slice_query_read(qslice, 0, qa);
    slice_query_read(qslice, 1, qb);
    __builtin_amdgcn_sched_barrier(0);
    float acc = slice_query_fma(0.f, 0, qa, c0, c1);   // s = 0..3
    __builtin_amdgcn_sched_barrier(0);
    slice_query_read(qslice, 2, qa);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_query_fma(acc, 1, qb, c0, c1);         // s = 4..7
    __builtin_amdgcn_sched_barrier(0);
    slice_query_read(qslice, 3, qb);
    __builtin_amdgcn_sched_barrier(0);
    acc = slice_query_fma(acc, 2, qa, c0, c1);         // s = 8..11
    acc = slice_query_fma(acc, 3, qb, c0, c1);         // s = 12..15
    return acc;
}

}  // namespace crag
