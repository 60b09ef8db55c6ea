// crag_ngram.hip -- the character-trigram field of the BM25 lane: its postings are built on the GPU (gfx950).
// Stands in for the reference's `pdb.ngram(3,3)` aliases (alembic/versions/0005_add_bm25_ngram.py, 0006_add_artifact_chunks.py).
// The rule is this tree's own and is written down in include/crag_dense.h (crag_ngram_extract); scoring is the word
// lane's crag_bm25_lane_host over the arrays built here.
//
// The build is three steps around a sort and a scan the CALLER runs (cadence_rag_amd.ngram uses torch.sort(stable=True)
// and torch.cumsum; nothing here depends on how they work inside):
//   1. ngram_extract_kernel: one workgroup per NG_TILE bytes of the concatenated text.  The tile and a forward halo of
//      16 bytes (a gram of three 4-byte sequences that starts on the tile's last byte ends 11 bytes behind it) go to LDS
//      with coalesced 16-byte loads.  EVERY byte position gets a slot (key, row): the gram's key where one starts,
//      CRAG_NGRAM_NO_KEY -- above every real key -- elsewhere.  No compaction: in text about four positions of five start
//      a gram, so a count/scan/emit pass would save a fifth of the sort at the price of reading the text twice, and the
//      slots are written position by position in full 512-byte and 256-byte runs per wave.  A gram can start only on a
//      byte that is not 10xxxxxx, and every such byte is a point where decoding resumes whatever precedes it, so no
//      backward look is needed: the three forward decodes decide.  The row of a position is found in text_ptr between
//      the rows of the tile's first and last byte.  doc_len is counted with integer atomics, one per wave where the
//      wave's 64 positions lie in one row.
//   (the caller sorts the slots by key, stable: positions ascend, so rows ascend inside a key; the first n_grams sorted
//    slots are the grams)
//   2. ngram_heads_kernel: per sorted gram 1 if it opens a (key, row) run, + 2^32 if it opens a key run.
//   (the caller takes the inclusive prefix sum: low word = postings so far, high word = terms so far)
//   3. ngram_emit_kernel scatters the heads (keys, post_ptr, post_pos and the run's first index), ngram_tf_kernel turns
//      neighbouring first indices into the saturated tf.
// All global writes are ordinary vector stores; every written index is checked against the caller's sizes.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_host.h"

namespace crag {
namespace {

constexpr int NG_THREADS = 256;
constexpr int NG_TILE = CRAG_NGRAM_TILE;
constexpr int NG_HALO = 16;
constexpr int NG_PER = NG_TILE / NG_THREADS;   // positions per thread, NG_THREADS apart: a wave stores 64 consecutive slots
constexpr int NG_VECS = (NG_TILE + NG_HALO) / 16;
constexpr int64_t NG_NO_KEY = CRAG_NGRAM_NO_KEY;
constexpr int NG_TF_MAX = 65535;

static_assert(NG_TILE % (16 * NG_THREADS) == 0 && NG_HALO >= 11, "whole 16-byte vectors, and the halo covers a gram");

// largest r in [lo, hi] with ptr[r] <= pos (ptr ascending, ptr[lo] <= pos): of equal entries the last, so never an empty row
__device__ __forceinline__ int64_t row_of(const int64_t *ptr, int64_t lo, int64_t hi, int64_t pos) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (ptr[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One sequence at s[i], the row ending at s[end]: its length and the folded code point in `cp` when it is a gram
// character, 0 for a separator of any kind (malformed, cut off, F8..FF, a stray continuation, other ASCII).
__device__ __forceinline__ int gram_char(const uint8_t *s, int i, int end, uint32_t &cp) {
    const uint32_t b = s[i];
    int len = 1;
    uint32_t v = b;
    if (b >= 0x80u) {
        len = b >= 0xF8u ? 0 : b >= 0xF0u ? 4 : b >= 0xE0u ? 3 : b >= 0xC0u ? 2 : 0;
        if (len == 0 || i + len > end) return 0;
        v = b & (0xFFu >> (len + 1));
        for (int j = 1; j < len; ++j) {
            const uint32_t c = s[i + j];
            if ((c & 0xC0u) != 0x80u) return 0;
            v = (v << 6) | (c & 0x3Fu);
        }
        if (v > 0x10FFFFu) return 0;
    }
    if (v - 'A' < 26u) v += 32u;
    if (v < 0x80u && !(v - '0' < 10u || v - 'a' < 26u)) return 0;
    cp = v;
    return len;
}

__global__ __launch_bounds__(NG_THREADS) void ngram_extract_kernel(const uint8_t *text, int64_t n_bytes,
                                                                   const int64_t *text_ptr, int64_t n_rows,
                                                                   int64_t *slot_keys, int32_t *slot_rows,
                                                                   int32_t *doc_len) {
    __shared__ alignas(16) uint8_t s_txt[NG_TILE + NG_HALO];
    __shared__ int64_t s_row[2];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * NG_TILE;
    for (int v = tid; v < NG_VECS; v += NG_THREADS) {
        const int64_t off = base + (int64_t)v * 16;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (off + 16 <= n_bytes) {
            w = *(const uint4 *)(text + off);
        } else if (off < n_bytes) {   // the text's last, partial vector: byte by byte, nothing behind n_bytes is read
            uint32_t parts[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < (int)(n_bytes - off); ++j) parts[j >> 2] |= (uint32_t)text[off + j] << ((j & 3) * 8);
            w = make_uint4(parts[0], parts[1], parts[2], parts[3]);
        }
        ((uint4 *)s_txt)[v] = w;
    }
    if (tid < 2) {
        const int64_t last = (base + NG_TILE < n_bytes ? base + NG_TILE : n_bytes) - 1;
        s_row[tid] = row_of(text_ptr, 0, n_rows - 1, tid == 0 ? base : last);
    }
    __syncthreads();
    const int64_t r_lo = s_row[0], r_hi = s_row[1];
#pragma unroll 1
    for (int j = 0; j < NG_PER; ++j) {
        const int li = j * NG_THREADS + tid;
        const int64_t pos = base + li;
        const bool valid = pos < n_bytes;
        int64_t key = NG_NO_KEY;
        int32_t row = -1;
        if (valid) {
            const int64_t r = row_of(text_ptr, r_lo, r_hi, pos);
            row = (int32_t)r;
            const int64_t row_end = text_ptr[r + 1] - base;
            const int end = row_end < NG_TILE + NG_HALO ? (int)row_end : NG_TILE + NG_HALO;
            uint32_t c0, c1, c2;
            const int l0 = gram_char(s_txt, li, end, c0);
            if (l0 && li + l0 < end) {
                const int l1 = gram_char(s_txt, li + l0, end, c1);
                if (l1 && li + l0 + l1 < end && gram_char(s_txt, li + l0 + l1, end, c2))
                    key = (int64_t)(((uint64_t)c0 << 42) | ((uint64_t)c1 << 21) | (uint64_t)c2);
            }
            slot_keys[pos] = key;
            slot_rows[pos] = row;
        }
        // dl: one atomic per wave when its positions share a row (lanes ascend with the position: lane 0 is valid
        // whenever any lane is)
        const bool has = key != NG_NO_KEY;
        const uint64_t grams = __ballot(has);
        const int32_t row0 = __shfl(row, 0);
        if (__all(!has || row == row0)) {
            if ((tid & 63) == 0 && grams) atomicAdd(&doc_len[row0], (int32_t)__popcll(grams));
        } else if (has) {
            atomicAdd(&doc_len[row], 1);
        }
    }
}

// *flag = 1 unless text_ptr is 0 = ptr[0] <= ptr[1] <= ... <= ptr[n_rows] = n_bytes (the caller zeroes it first)
__global__ __launch_bounds__(256) void ngram_check_ptr_kernel(const int64_t *text_ptr, int64_t n_rows, int64_t n_bytes,
                                                              int32_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = first == 0 && (text_ptr[0] != 0 || text_ptr[n_rows] != n_bytes);
    for (int64_t i = first; i < n_rows; i += stride) bad |= text_ptr[i + 1] < text_ptr[i];
    if (bad) *flag = 1;
}

__global__ __launch_bounds__(256) void ngram_heads_kernel(const int64_t *keys, const int32_t *rows, int64_t n,
                                                          int64_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool term = i == 0 || keys[i - 1] != keys[i];
    const bool post = term || rows[i - 1] != rows[i];
    flags[i] = (int64_t)post | ((int64_t)term << 32);
}

__global__ __launch_bounds__(256) void ngram_emit_kernel(const int64_t *keys, const int32_t *rows, const int64_t *scan,
                                                         int64_t n, int64_t n_terms, int64_t nnz, int64_t *out_keys,
                                                         int64_t *post_ptr, int32_t *post_pos, int32_t *run_first) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) post_ptr[n_terms] = nnz;
    if (i >= n) return;
    const int64_t c = scan[i], d = c - (i ? scan[i - 1] : 0);
    if ((d & 0xffffffffll) == 0) return;
    const int64_t p = (c & 0xffffffffll) - 1;
    if (p < 0 || p >= nnz) return;   // (a scan that is not the heads' prefix sum)
    post_pos[p] = rows[i];
    run_first[p] = (int32_t)i;
    if (d >> 32) {
        const int64_t t = (c >> 32) - 1;
        if (t < 0 || t >= n_terms) return;
        out_keys[t] = keys[i];
        post_ptr[t] = p;
    }
}

__global__ __launch_bounds__(256) void ngram_tf_kernel(const int32_t *run_first, int64_t nnz, int64_t n,
                                                       uint16_t *post_tf) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int64_t len = (p + 1 < nnz ? (int64_t)run_first[p + 1] : n) - run_first[p];
    post_tf[p] = (uint16_t)(len < NG_TF_MAX ? len : NG_TF_MAX);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace crag

extern "C" {

int64_t crag_ngram_scratch_bytes(int64_t n_bytes, int64_t n_rows) {
    if (n_bytes < 0 || n_rows < 0 || n_rows > INT32_MAX) return CRAG_EINVAL;
    if (n_bytes > INT32_MAX) return CRAG_E2BIG;
    // the check flag's 256 bytes | run_first [nnz <= n_bytes] int32
    return 256 + ((n_bytes * 4 + 255) & ~(int64_t)255);
}

int crag_ngram_extract(const uint8_t *d_text, int64_t n_bytes, const int64_t *d_text_ptr, int64_t n_rows,
                       int64_t *d_slot_keys, int32_t *d_slot_rows, int32_t *d_doc_len, void *d_scratch,
                       int64_t scratch_bytes, void *stream) {
    // the argument checks come before the first HIP call
    if (n_bytes < 0 || n_rows < 0 || n_rows > INT32_MAX)
        return fail(CRAG_EINVAL, "ngram_extract: n_bytes / n_rows out of range");
    if (n_bytes > INT32_MAX)
        return fail(CRAG_E2BIG, "ngram_extract: %lld bytes of text; one build takes at most 2^31 - 1 (split the corpus)",
                    (long long)n_bytes);
    if (!d_text_ptr || !d_scratch || (n_bytes > 0 && (!d_text || !d_slot_keys || !d_slot_rows)) || (n_rows > 0 && !d_doc_len))
        return fail(CRAG_EINVAL, "ngram_extract: NULL pointer argument");
    if (((uintptr_t)d_text & 15) != 0 || ((uintptr_t)d_scratch & 7) != 0)
        return fail(CRAG_EINVAL, "ngram_extract: the text must be 16-byte aligned, the scratch 8-byte aligned");
    if (scratch_bytes < crag_ngram_scratch_bytes(n_bytes, n_rows))
        return fail(CRAG_EINVAL, "ngram_extract: scratch too small (crag_ngram_scratch_bytes)");
    if (n_rows == 0 && n_bytes > 0) return fail(CRAG_EINVAL, "ngram_extract: text without rows");
    hipStream_t st = (hipStream_t)stream;
    int32_t *d_flag = (int32_t *)d_scratch;
    HIP_TRY(hipMemsetAsync(d_flag, 0, 4, st));
    const unsigned check_blocks = n_rows / 256 + 1 < 1024 ? (unsigned)(n_rows / 256 + 1) : 1024u;
    hipLaunchKernelGGL(crag::ngram_check_ptr_kernel, dim3(check_blocks), dim3(256), 0, st, d_text_ptr, n_rows, n_bytes,
                       d_flag);
    int rc = launch_ok("ngram_check_ptr_kernel");
    if (rc) return rc;
    int32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad)
        return fail(CRAG_EINVAL, "ngram_extract: text_ptr must ascend from 0 to n_bytes (rows may be empty)");
    if (n_rows > 0) HIP_TRY(hipMemsetAsync(d_doc_len, 0, (size_t)n_rows * 4, st));
    if (n_bytes == 0) return CRAG_OK;
    const unsigned tiles = (unsigned)((n_bytes + crag::NG_TILE - 1) / crag::NG_TILE);
    hipLaunchKernelGGL(crag::ngram_extract_kernel, dim3(tiles), dim3(crag::NG_THREADS), 0, st, d_text, n_bytes,
                       d_text_ptr, n_rows, d_slot_keys, d_slot_rows, d_doc_len);
    return launch_ok("ngram_extract_kernel");
}

int crag_ngram_heads(const int64_t *d_sorted_keys, const int32_t *d_sorted_rows, int64_t n_grams, int64_t *d_flags,
                     void *stream) {
    if (n_grams < 0 || n_grams > INT32_MAX) return fail(CRAG_EINVAL, "ngram_heads: n_grams out of range");
    if (n_grams == 0) return CRAG_OK;
    if (!d_sorted_keys || !d_sorted_rows || !d_flags) return fail(CRAG_EINVAL, "ngram_heads: NULL pointer argument");
    hipLaunchKernelGGL(crag::ngram_heads_kernel, dim3(crag::blocks_for(n_grams)), dim3(256), 0, (hipStream_t)stream,
                       d_sorted_keys, d_sorted_rows, n_grams, d_flags);
    return launch_ok("ngram_heads_kernel");
}

int crag_ngram_emit(const int64_t *d_sorted_keys, const int32_t *d_sorted_rows, const int64_t *d_scan, int64_t n_grams,
                    int64_t n_terms, int64_t nnz, int64_t *d_keys, int64_t *d_post_ptr, int32_t *d_post_pos,
                    uint16_t *d_post_tf, void *d_scratch, int64_t scratch_bytes, void *stream) {
    if (n_grams < 0 || n_grams > INT32_MAX || n_terms < 0 || n_terms > nnz || nnz > n_grams || (n_grams > 0 && nnz == 0) ||
        (nnz > 0 && n_terms == 0))
        return fail(CRAG_EINVAL, "ngram_emit: need n_terms <= nnz <= n_grams <= 2^31 - 1 (and none zero unless all are)");
    if (!d_post_ptr || !d_scratch || (n_grams > 0 && (!d_sorted_keys || !d_sorted_rows || !d_scan || !d_keys || !d_post_pos ||
                                                      !d_post_tf)))
        return fail(CRAG_EINVAL, "ngram_emit: NULL pointer argument");
    if (((uintptr_t)d_scratch & 7) != 0 || scratch_bytes < 256 + nnz * 4)
        return fail(CRAG_EINVAL, "ngram_emit: scratch misaligned or too small (crag_ngram_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    int32_t *run_first = (int32_t *)((char *)d_scratch + 256);
    hipLaunchKernelGGL(crag::ngram_emit_kernel, dim3(n_grams ? crag::blocks_for(n_grams) : 1u), dim3(256), 0, st,
                       d_sorted_keys, d_sorted_rows, d_scan, n_grams, n_terms, nnz, d_keys, d_post_ptr, d_post_pos,
                       run_first);
    if (nnz > 0)
        hipLaunchKernelGGL(crag::ngram_tf_kernel, dim3(crag::blocks_for(nnz)), dim3(256), 0, st, run_first, nnz, n_grams,
                           d_post_tf);
    return launch_ok("ngram_emit_kernel");
}

}  // extern "C"
