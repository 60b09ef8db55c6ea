// crag_group.hip -- exact cosine top-k under "at most per_group rows per group" on the GPU (gfx950), DESIGN.md 4.12.
//
// Per query: rank the eligible rows by (score descending, id ascending), walk the ranking, keep a row iff its group holds
// fewer than per_group kept rows, stop at k -- equivalently the top-k of the union of every group's own top-per_group.
// Scores and eligibility are crag_index_search's: the arithmetic is crag_exact.h's (the canonical 1/||q||, the fmaf chain
// of exact_slice_dot per K slice, the eight slice sums added in wave order 0..7, make_key), one (query, row) pair at a
// time, so a pair's score depends on nothing else.
//
// Three launches in stream order:
//  1. group_prep_kernel: zeroes the (query, group) table in the caller's scratch and writes the canonical 1/||q|| of
//     every query behind it -- once per query, not once per workgroup of the score kernel.
//  2. group_score_kernel<PS>, grid ceil(size / 64), 512 threads: a workgroup owns 64 consecutive row POSITIONS, 8 lanes
//     per row (lane `sub` = K slice).  Each lane fetches its slice of the row (32 float4) into registers ONCE and keeps
//     it there while the workgroup walks over all queries in blocks of GQ_BLOCK held in LDS: the table is read once per
//     call, whatever nq.  A pair that counts folds its key (f2ord(score) << 32) | ~pos into the per_group sorted slots
//     of (query, group) with a cascade of atomic maxima (group_insert_finish); what a pair needs from memory is asked
//     for a query ahead and the cascade's first answer is used a query later, so the arithmetic hides both.
//  3. group_select_kernel, one workgroup per query: the k largest of the query's n_groups * per_group slots -- streamed
//     through LDS in chunks under a running k-th key --, written with their ids, scores and groups.
// Every key is unique (it holds the row position), so the table and the outputs depend on the set of inserted keys only,
// not on the order the atomics arrive in.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_exact.h"
#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {
namespace {

constexpr int GS_ROWS = SCAN_THREADS / 8;    // row positions per workgroup of the score kernel: 8 lanes each
constexpr int GQ_BLOCK = 16;                 // queries held in LDS at a time
// float4 per K slice of a query in LDS: 32 + 1 of padding.  The 8 lanes of a row read 8 different slices, the lanes of
// different rows the same ones (a broadcast); 33 float4 apart the eight 16-byte reads fall into disjoint banks, 32
// apart (512 bytes) they would all start at the same one.
constexpr int GQ_SLICE_F4 = 33;
constexpr int SEL_BUF = 4096;                // keys the select kernel holds in LDS
constexpr int SEL_CHUNK = 2048;              // table slots it reads between two looks at the buffer

static_assert(GS_ROWS == 64, "the grid is ceil(size / 64)");
static_assert(GQ_BLOCK * SCAN_WAVES * GQ_SLICE_F4 * 16 <= 80 * 1024, "two blocks of queries fit the LDS of a CU");
static_assert((SEL_BUF & (SEL_BUF - 1)) == 0 && SEL_CHUNK + CRAG_MAX_K <= SEL_BUF, "the k best and a chunk fit the buffer");

__global__ __launch_bounds__(SCAN_THREADS) void group_prep_kernel(GroupParams p, int64_t table_words) {
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < p.nq) {   // (the same for every thread of the workgroup: canonical_qinv has barriers)
        const f32x4 v = load_query_quad(p.queries, p.dim, blockIdx.x, p.nq, tid);
        const float qinv = canonical_qinv(v, true, sh);
        if (tid == 0) p.qinv[blockIdx.x] = qinv;
    }
    for (int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + tid; i < table_words; i += (int64_t)gridDim.x * SCAN_THREADS)
        p.table[i] = 0ull;
}

// A key (non-zero) enters the per sorted slots of its (query, group) by a cascade of atomic maxima: the maximum on slot j
// leaves the larger of (slot, v) in the slot and hands the smaller one on to slot j + 1.  Whatever the interleaving, slot
// j therefore ends as the largest key that ever reached it and every other key that reached it goes on exactly once: by
// induction over j the slots end as the group's per largest keys in descending order.  Slots only grow, so a key that is
// not above the last slot -- even a stale value of it -- is not among them and is dropped without an atomic (the caller
// compares with a value it asked for earlier).
// The cascade is cut in two so that nothing waits for memory: the score kernel issues the maximum on slot 0 and keeps
// what the slot held unread; group_insert_finish -- called after the arithmetic of the NEXT query, when that value has
// arrived -- carries on.  The last slot hands nothing on: its maximum needs no return value.
__device__ __forceinline__ uint64_t slot_max(uint64_t *slot, uint64_t v) {
    return __hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void group_insert_finish(uint64_t *slot, int per, uint64_t v, uint64_t old) {
    if (old < v) v = old;   // slot 0 took the larger of the two
    for (int j = 1; j < per && v != 0ull; ++j) {
        if (j == per - 1) {
            (void)slot_max(slot + j, v);
            break;
        }
        old = slot_max(slot + j, v);
        if (old < v) v = old;
    }
}

// What lane 0 of a row needs from memory for one query: the mask word of the row and the last (smallest) slot of the
// row's group.  Asked for one query ahead, so that the loads travel during the arithmetic of the query before.
struct PairGate {
    uint32_t mword;   // 0 for a lane that owns no pair
    uint64_t last;
};
__device__ __forceinline__ uint64_t *group_slots(const GroupParams &p, int q, int32_t g) {
    return p.table + ((size_t)q * (size_t)p.n_groups + (size_t)g) * (size_t)p.per_group;
}
__device__ __forceinline__ PairGate ask_gate(const GroupParams &p, bool owner, int q, int64_t pos, int32_t g) {
    PairGate r = {0u, ~0ull};
    if (owner) {
        r.mword = p.mask ? p.mask[(size_t)q * (size_t)p.mask_stride_w + (size_t)(pos >> 5)] : 0xffffffffu;
        r.last = __hip_atomic_load(group_slots(p, q, g) + p.per_group - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return r;
}

// (the row slice takes 128 registers: two waves per SIMD = one workgroup per CU.  Two would need the slice in 64, i.e.
// the row fetched in halves and once per block of queries instead of once per call -- DESIGN.md 4.12)
template <int PS>
__global__ __launch_bounds__(SCAN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void group_score_kernel(GroupParams p) {
    __shared__ f32x4 qs[GQ_BLOCK][SCAN_WAVES][GQ_SLICE_F4];   // per query and K slice: float4 2s + half, as exact_slice_fma reads it
    __shared__ float qinv_sh[GQ_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 3, sub = tid & 7;
    const int64_t pos = (int64_t)blockIdx.x * GS_ROWS + grp;
    const bool stored = pos < p.rows.size;

    f32x4 c0[16], c1[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) c0[s] = c1[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float inv_row = 0.f;
    int32_t g = -1;
    if (stored) {
        if (sub == 0) {
            inv_row = p.rows.inv_norm[pos];
            g = p.row_group[pos];
        }
        const f32x4 *ctile = reinterpret_cast<const f32x4 *>(p.rows.corpus + (size_t)(pos >> 5) * TILE_FLOATS) + (size_t)sub * 32 * 32;
        exact_slice_fetch<PS>(ctile, (int)(pos & 31), c0, c1);
    }
    // lane 0 of a row owns its pairs; a group number outside [0, n_groups) is never used as an index
    const bool owner = sub == 0 && stored && g >= 0 && (int64_t)g < p.n_groups;

    uint64_t *pend_slots = nullptr;   // a cascade in flight: slot 0 was given pend_v and answers pend_old
    uint64_t pend_v = 0ull, pend_old = 0ull;
    // one query of the block in LDS against the row in registers; `gate` was asked for a query ago
    auto score_one = [&](int q0, int qi, const PairGate &gate) {
        const float qinv = qinv_sh[qi];
        if (!(qinv > 0.f)) return;   // a zero / non-finite query scores nothing (the same for the whole workgroup)
        const float part = exact_slice_fma(&qs[qi][sub][0], c0, c1);
        // the 8 slice sums in wave order 0..7 (the scan kernels' split-K reduction order)
        float d = __shfl(part, (lane & ~7) | 0);
#pragma unroll
        for (int ww = 1; ww < 8; ++ww) d += __shfl(part, (lane & ~7) | ww);
        if (pend_slots) {
            group_insert_finish(pend_slots, p.per_group, pend_v, pend_old);
            pend_slots = nullptr;
        }
        if ((gate.mword >> (pos & 31)) & 1u) {
            uint32_t khi, klo;
            make_key(d, inv_row * qinv, pos, khi, klo);
            const uint64_t key = mk64(khi, klo);
            if (key > gate.last) {   // (above the last slot as it was a query ago; an ignored pair has key 0)
                uint64_t *slots = group_slots(p, q0 + qi, g);
                if (p.per_group == 1) {
                    (void)slot_max(slots, key);
                } else {
                    pend_old = slot_max(slots, key);
                    pend_v = key;
                    pend_slots = slots;
                }
            }
        }
    };
    for (int q0 = 0; q0 < p.nq; q0 += GQ_BLOCK) {
        const int nb = p.nq - q0 < GQ_BLOCK ? p.nq - q0 : GQ_BLOCK;
        // two gates used in turn (a copy from "next" to "current" would wait for the loads where it stands)
        PairGate even = ask_gate(p, owner, q0, pos, g), odd = {0u, ~0ull};
        __syncthreads();   // the last block of queries has been read
        for (int i = tid; i < nb * 256; i += SCAN_THREADS) {
            const int qi = i >> 8, t = i & 255;   // t holds dims 4t .. 4t + 3: float4 t & 31 of slice t >> 5
            qs[qi][t >> 5][t & 31] = load_query_quad(p.queries, p.dim, q0 + qi, p.nq, t);
        }
        if (tid < nb) qinv_sh[tid] = p.qinv[q0 + tid];
        __syncthreads();
        for (int qi = 0; qi < nb; qi += 2) {
            // (asked without a condition around the assignment: keeping the old value would read it, i.e. wait for it)
            odd = ask_gate(p, owner && qi + 1 < nb, q0 + qi + 1, pos, g);
            score_one(q0, qi, even);
            even = ask_gate(p, owner && qi + 2 < nb, q0 + qi + 2, pos, g);
            if (qi + 1 < nb) score_one(q0, qi + 1, odd);
        }
    }
    if (pend_slots) group_insert_finish(pend_slots, p.per_group, pend_v, pend_old);
}

// The n (<= SEL_BUF) keys of the buffer in descending order; returns how many of them stay: min(n, k).
__device__ __forceinline__ int sort_and_cut(uint64_t *keys, int n, int k) {
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + threadIdx.x; i < P; i += SCAN_THREADS) keys[i] = 0ull;
    __syncthreads();
    sort_keys_desc(keys, P);
    return n < k ? n : k;
}

__global__ __launch_bounds__(SCAN_THREADS) void group_select_kernel(GroupParams p) {
    __shared__ uint64_t keys[SEL_BUF];
    __shared__ int n_sh;
    const int q = blockIdx.x, tid = threadIdx.x, k = p.k;
    const int64_t slots = p.n_groups * p.per_group;
    const uint64_t *mine = p.table + (size_t)q * (size_t)slots;
    uint64_t bar = 0ull;   // the k-th key so far: nothing at or below it can be among the k best (0: the empty slots)
    if (tid == 0) n_sh = 0;
    __syncthreads();
    for (int64_t base = 0; base < slots; base += SEL_CHUNK) {
        int n = n_sh;
        __syncthreads();
        if (n + SEL_CHUNK > SEL_BUF) {   // no room for another chunk: keep the k best, raise the bar
            n = sort_and_cut(keys, n, k);
            if (n == k) bar = keys[k - 1];
            if (tid == 0) n_sh = n;
            __syncthreads();
        }
        for (int i = tid; i < SEL_CHUNK && base + i < slots; i += SCAN_THREADS) {
            const uint64_t key = mine[base + i];
            if (key > bar) keys[atomicAdd(&n_sh, 1)] = key;   // (the sort undoes the arrival order)
        }
        __syncthreads();
    }
    const int n_out = sort_and_cut(keys, n_sh, k);
    for (int r = tid; r < k; r += SCAN_THREADS) {
        const size_t o = (size_t)q * k + r;
        if (r < n_out) {
            const uint64_t key = keys[r];
            const uint32_t pos = ~(uint32_t)key;
            p.out_scores[o] = ord2f((uint32_t)(key >> 32));
            p.out_ids[o] = p.rows.stored[pos];
            if (p.out_groups) p.out_groups[o] = p.row_group[pos];
        } else {
            p.out_scores[o] = __uint_as_float(0x7fc00000u);
            p.out_ids[o] = -1;
            if (p.out_groups) p.out_groups[o] = -1;
        }
    }
    if (tid == 0) p.out_counts[q] = n_out;
}

int64_t table_words(int nq, int64_t n_groups, int per_group) {
    return (int64_t)(nq > 1 ? nq : 1) * (n_groups > 1 ? n_groups : 1) * (per_group > 1 ? per_group : 1);
}

}  // namespace

int64_t group_scratch_bytes(int nq, int64_t n_groups, int per_group) {
    return table_words(nq, n_groups, per_group) * (int64_t)sizeof(uint64_t) +
           ((int64_t)(nq > 1 ? nq : 1) * (int64_t)sizeof(float) + 7) / 8 * 8;
}

hipError_t launch_grouped(const GroupParams &p, hipStream_t st) {
    if (p.nq <= 0) return hipSuccess;
    const int64_t words = (int64_t)p.nq * p.n_groups * p.per_group;
    int64_t clear_blocks = (words + SCAN_THREADS - 1) / SCAN_THREADS;
    if (clear_blocks > 2048) clear_blocks = 2048;
    const unsigned prep_blocks = (unsigned)(clear_blocks > p.nq ? clear_blocks : p.nq);
    hipLaunchKernelGGL(group_prep_kernel, dim3(prep_blocks), dim3(SCAN_THREADS), 0, st, p, words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (p.rows.size > 0) {
        const dim3 grid((unsigned)((p.rows.size + GS_ROWS - 1) / GS_ROWS));
        if (p.rows.piece_shift == PS_BIG) hipLaunchKernelGGL(group_score_kernel<PS_BIG>, grid, dim3(SCAN_THREADS), 0, st, p);
        else hipLaunchKernelGGL(group_score_kernel<PS_SMALL>, grid, dim3(SCAN_THREADS), 0, st, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(group_select_kernel, dim3(p.nq), dim3(SCAN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag
