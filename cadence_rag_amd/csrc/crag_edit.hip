// crag_edit.hip -- in-place edits of the device corpus: remove rows, insert rows whose ids lie between stored ones.
//
// The contract: after an edit the index holds, bit for bit, what crag_index_add would have stored from
// the same rows in id order.  A row that stays is therefore COPIED -- its fp32 pieces, its 128 mirror pieces, its
// 1/||row|| and its id -- never recomputed, and a row that comes in is written by store_row (crag_layout.h), the
// arithmetic of store_rows_kernel.
//
// Moving in place: a removal moves rows to lower positions only, an insertion to higher positions only, but inside
// one launch a workgroup may write a row that another one still has to read.  The host (crag_api_store.hip) therefore
// works in chunks of C destination rows through a bounce buffer laid out like C rows of the index: source positions
// of the chunk -> gather into the bounce buffer -> write to the destination, in stream order; chunks ascend for a
// removal and descend for an insertion, so that no chunk overwrites a row a later chunk reads.  Rows in front of the
// first changed position are never touched.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {

// ---- which row goes where ------------------------------------------------------------------------------------------

// Binary search of each of the n given ids in the ascending stored ids.  pos (nullable) receives the number of stored
// ids below it (+ its own index j with add_index: the row's position after an insertion of the ascending list);
// drop (nullable, one bit per row position, 32 rows per word) gets the bit of every id that is stored; found
// (nullable) counts them.
__global__ __launch_bounds__(256) void lookup_ids_kernel(const int64_t *stored, int64_t size, const int64_t *ids, int64_t n,
                                                         int64_t *pos, int add_index, uint32_t *drop,
                                                         unsigned long long *found) {
    unsigned long long c = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t id = ids[j];
        const int64_t lo = lower_bound_asc(stored, 0, size, id);
        const bool hit = lo < size && stored[lo] == id;
        if (pos) pos[j] = lo + (add_index ? j : 0);
        if (hit) {
            if (drop) atomicOr(&drop[lo >> 5], 1u << (lo & 31));
            ++c;
        }
    }
    if (found) {
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(found, c);
    }
}

// Removal: destination position d0 + i holds the (d0 + i)-th kept row.  prefix[w] = kept rows in front of word w
// (n_words + 1 entries, computed on the host).
__global__ __launch_bounds__(256) void remove_srcpos_kernel(const uint32_t *keep, const uint32_t *prefix, int64_t n_words,
                                                            int64_t d0, int64_t m, int64_t *srcpos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t d = (uint32_t)(d0 + i);
    int64_t lo = 0, hi = n_words;   // first word whose prefix is > d; the row sits in the word before it
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= d) lo = mid + 1;
        else hi = mid;
    }
    const int64_t w = lo - 1;
    uint32_t x = keep[w];
    for (uint32_t r = d - prefix[w]; r > 0; --r) x &= x - 1;   // drop the kept rows in front of ours
    srcpos[i] = w * 32 + (__ffs((int)x) - 1);
}

// Insertion: newpos[j] (ascending) = position of new row j afterwards.  Destination d0 + i is either one of them
// (srcpos = -1: the scattered store fills it) or the old row that has as many new rows in front of it.
__global__ __launch_bounds__(256) void insert_srcpos_kernel(const int64_t *newpos, int64_t n_new, int64_t d0, int64_t m,
                                                            int64_t *srcpos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t d = d0 + i;
    int64_t lo = 0, hi = n_new;   // number of new rows at positions <= d
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (newpos[mid] <= d) lo = mid + 1;
        else hi = mid;
    }
    srcpos[i] = (lo > 0 && newpos[lo - 1] == d) ? -1 : d - lo;
}

// ---- the move ------------------------------------------------------------------------------------------------------

// Everything a row owns, from position s of `src` to position d of `dst`: one 256-thread block per row, thread kq
// its kq-th float4 (the 8 x 512 B or 64 x 64 B fp32 pieces), threads 0..127 one 16-byte mirror piece each, thread
// 255 the norm and the id.
template <int PS>
__device__ __forceinline__ void copy_row(const RowStore &src, int64_t s, const RowStore &dst, int64_t d) {
    const int kq = threadIdx.x;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(src.corpus + row_f4_offset<PS>(s, kq));
    u32x4 h = {0u, 0u, 0u, 0u};
    const bool mir = PS == PS_BIG && kq < 128;
    if (mir) h = *reinterpret_cast<const u32x4 *>(src.mirror + row_mirror_piece_offset(s, kq));
    *reinterpret_cast<f32x4 *>(dst.corpus + row_f4_offset<PS>(d, kq)) = v;
    if (mir) *reinterpret_cast<u32x4 *>(dst.mirror + row_mirror_piece_offset(d, kq)) = h;
    if (kq == 255) {
        dst.inv_norm[d] = src.inv_norm[s];
        dst.ids[d] = src.ids[s];
    }
}

// gather: index row srcpos[i] -> bounce row i.   A negative source position (a slot an insertion fills) is skipped.
template <int PS>
__global__ __launch_bounds__(256) void gather_rows_kernel(RowStore index, RowStore bounce, const int64_t *srcpos) {
    const int64_t i = blockIdx.x;
    const int64_t s = srcpos[i];
    if (s < 0) return;
    copy_row<PS>(index, s, bounce, i);
}

// bounce row i -> index row d0 + i
template <int PS>
__global__ __launch_bounds__(256) void spread_rows_kernel(RowStore bounce, RowStore index, const int64_t *srcpos, int64_t d0) {
    const int64_t i = blockIdx.x;
    if (srcpos[i] < 0) return;
    copy_row<PS>(bounce, i, index, d0 + i);
}

// ---- around the move -----------------------------------------------------------------------------------------------

// new rows at listed positions: store_rows_kernel's arithmetic (store_row) + the id
template <int PS>
__global__ __launch_bounds__(256) void store_rows_at_kernel(const float *rows, int dim, const int64_t *dstpos,
                                                            const int64_t *new_ids, RowStore index, uint32_t *irregular) {
    const int64_t i = blockIdx.x;
    const int64_t row = dstpos[i];
    store_row<PS>(rows + (size_t)i * dim, dim, row, index.corpus, index.inv_norm, irregular, index.mirror);
    if (threadIdx.x == 0) index.ids[row] = new_ids[i];
}

// vacated positions back to what crag_index_create leaves: fp32 row 0, mirror 0, 1/||row|| 0, id 0
template <int PS>
__global__ __launch_bounds__(256) void clear_rows_kernel(RowStore index, int64_t pos) {
    const int64_t row = pos + blockIdx.x;
    const int kq = threadIdx.x;
    *reinterpret_cast<f32x4 *>(index.corpus + row_f4_offset<PS>(row, kq)) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (PS == PS_BIG && kq < 128)
        *reinterpret_cast<u32x4 *>(index.mirror + row_mirror_piece_offset(row, kq)) = u32x4{0u, 0u, 0u, 0u};
    if (kq == 255) {
        index.inv_norm[row] = 0.f;
        index.ids[row] = 0;
    }
}

// store_rows_kernel's condition over the rows that are left
__global__ __launch_bounds__(256) void irregular_flag_kernel(const float *inv_norm, int64_t n, uint32_t *flag) {
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        any |= irregular_inv_norm(inv_norm[i]);
    if (any) *flag = 1u;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
static unsigned grid_for(int64_t n, int64_t cap) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < cap ? b : cap);
}

hipError_t launch_lookup_ids(const int64_t *stored, int64_t size, const int64_t *ids, int64_t n, int64_t *pos,
                             int add_index, uint32_t *drop, unsigned long long *found, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lookup_ids_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, st, stored, size, ids, n, pos, add_index,
                       drop, found);
    return hipGetLastError();
}

hipError_t launch_remove_srcpos(const uint32_t *keep, const uint32_t *prefix, int64_t n_words, int64_t d0, int64_t m,
                                int64_t *srcpos, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(remove_srcpos_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, keep, prefix, n_words, d0,
                       m, srcpos);
    return hipGetLastError();
}

hipError_t launch_insert_srcpos(const int64_t *newpos, int64_t n_new, int64_t d0, int64_t m, int64_t *srcpos,
                                hipStream_t st) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(insert_srcpos_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, newpos, n_new, d0, m,
                       srcpos);
    return hipGetLastError();
}

hipError_t launch_move_rows(const RowStore &index, const RowStore &bounce, const int64_t *srcpos, int64_t d0, int64_t m,
                            hipStream_t st) {
    if (m <= 0) return hipSuccess;
    const dim3 grid((unsigned)m), block(256);
    if (index.mirror) {
        hipLaunchKernelGGL(gather_rows_kernel<PS_BIG>, grid, block, 0, st, index, bounce, srcpos);
        hipLaunchKernelGGL(spread_rows_kernel<PS_BIG>, grid, block, 0, st, bounce, index, srcpos, d0);
    } else {
        hipLaunchKernelGGL(gather_rows_kernel<PS_SMALL>, grid, block, 0, st, index, bounce, srcpos);
        hipLaunchKernelGGL(spread_rows_kernel<PS_SMALL>, grid, block, 0, st, bounce, index, srcpos, d0);
    }
    return hipGetLastError();
}

hipError_t launch_store_rows_at(const float *rows, int dim, const int64_t *dstpos, const int64_t *new_ids, int64_t n,
                                const RowStore &index, uint32_t *irregular, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)n), block(256);
    if (index.mirror) hipLaunchKernelGGL(store_rows_at_kernel<PS_BIG>, grid, block, 0, st, rows, dim, dstpos, new_ids, index, irregular);
    else hipLaunchKernelGGL(store_rows_at_kernel<PS_SMALL>, grid, block, 0, st, rows, dim, dstpos, new_ids, index, irregular);
    return hipGetLastError();
}

hipError_t launch_clear_rows(const RowStore &index, int64_t pos, int64_t n, hipStream_t st) {
    const int64_t STEP = (int64_t)1 << 24;   // rows per launch (one block each)
    for (int64_t o = 0; o < n; o += STEP) {
        const int64_t m = n - o < STEP ? n - o : STEP;
        if (index.mirror) hipLaunchKernelGGL(clear_rows_kernel<PS_BIG>, dim3((unsigned)m), dim3(256), 0, st, index, pos + o);
        else hipLaunchKernelGGL(clear_rows_kernel<PS_SMALL>, dim3((unsigned)m), dim3(256), 0, st, index, pos + o);
    }
    return hipGetLastError();
}

hipError_t launch_irregular_flag(const float *inv_norm, int64_t n, uint32_t *flag, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(irregular_flag_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, st, inv_norm, n, flag);
    return hipGetLastError();
}

}  // namespace crag
