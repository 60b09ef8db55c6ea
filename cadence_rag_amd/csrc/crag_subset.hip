// crag_subset.hip -- exact cosine top-k and scores over LISTED rows on the GPU (gfx950), DESIGN.md 4.11.
//
// Per query: a list of up to CRAG_SUBSET_MAX_WIDTH row ids (a set: order and repeats change nothing).  Only the listed
// rows are read -- 4 KiB each -- where a masked search streams the whole table.  The result is what the masked search
// returns under a mask whose set bits are the positions of the listed ids, bit for bit: the arithmetic is the selection
// kernel's own (crag_exact.h) -- the canonical 1/||q||, exact_slice_dot per K slice, the eight slice sums added in wave
// order 0..7, make_key -- and it sees one (query, row) pair at a time, so a pair's score depends on nothing else (not
// on the slot, the width, nq, k, shared or per-query lists, the row's position or the row layout).
//
// Two launches in stream order:
//  1. subset_score_kernel, grid (ceil(width / 64), nq), 512 threads: a workgroup scores 64 slots of one query, 8 lanes
//     per slot (lane `sub` = K slice).  It loads the query (load_query_quad -> canonical_qinv -> LDS in fragment order
//     [slice][s][half]) while its 64 ids are on their way, resolves the ids to positions in the ascending stored ids
//     (lower_bound_asc_x8 of crag_rows.h: the 8 lanes of a slot probe 8 points per round -- 7 dependent round trips at
//     a million rows instead of 20; this path is latency-bound), then fetches stored[pos], 1/||row|| and
//     the row's 32 float4 per lane in flight together, and writes the key (f2ord(score) << 32) | ~pos per slot into the
//     scratch (0: ignored) and the slot's score if asked for.
//  2. subset_select_kernel, one workgroup per query: the query's keys into LDS (32 KiB at 4096), padded with zeros to
//     the next power of two at or above the count, a bitonic sort in descending order, equal neighbours dropped (an
//     equal key is the same row: the set semantics), the first k written with their ids.  The output depends on the key
//     set only.
#include "crag_arch.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crag_dense.h"
#include "crag_exact.h"
#include "crag_kernels.h"
#include "crag_layout.h"

namespace crag {
namespace {

constexpr int SS_SLOTS = SCAN_THREADS / 8;   // slots per workgroup of the score kernel: 8 lanes each
constexpr int SS_W = CRAG_SUBSET_MAX_WIDTH;

static_assert(SS_SLOTS == 64, "the grid is ceil(width / 64) x nq");
static_assert((SS_W & (SS_W - 1)) == 0 && SS_W >= SCAN_THREADS, "the select kernel sorts a power of two of keys in LDS");

// (two to three waves per SIMD: left to itself the compiler holds the kernel to 64 registers and fetches a row in
// batches of a few float4; with ~160 the loads of a row are in flight together, which is all this kernel waits for)
template <int PS>
__global__ __launch_bounds__(SCAN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 3))) void subset_score_kernel(SubsetParams p) {
    __shared__ f32x4 qs[SCAN_WAVES][16][2];   // the query in fragment order: [slice][s][lane half]
    __shared__ double sh[4];
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, grp = tid >> 3, sub = tid & 7;
    const int slot = (int)blockIdx.x * SS_SLOTS + grp;
    const int count = clamp_count(p.counts[p.list_stride ? q : 0], p.width);
    const bool listed = slot < count;
    // the slot's id (the 8 lanes of a slot read the same word) is on its way while the query is prepared
    const int64_t id = listed ? p.ids[(size_t)q * p.list_stride + slot] : -1;
    const f32x4 v = load_query_quad(p.queries, p.dim, q, p.nq, tid);
    const float qinv = canonical_qinv(v, true, sh);
    if (tid < 256) qs[tid >> 5][(tid >> 1) & 15][tid & 1] = v;
    __syncthreads();

    // ---- id -> first position whose stored id is >= id, the slot's 8 lanes together ----
    const bool wanted = listed && id != -1 && qinv > 0.f;   // (a zero / non-finite query scores nothing: no row is read)
    const int64_t lo = lower_bound_asc_x8(p.rows.stored, 0, wanted ? p.rows.size : 0, id, lane);

    // ---- the row at that position, its id and 1/||row|| in flight together; the pair counts if the id is the one ----
    const bool live = wanted && lo < p.rows.size;
    float part = 0.f, inv_row = 0.f;
    int64_t found = -1;
    if (live) {
        if (sub == 0) {
            found = p.rows.stored[lo];
            inv_row = p.rows.inv_norm[lo];
        }
        const f32x4 *ctile = reinterpret_cast<const f32x4 *>(p.rows.corpus + (size_t)(lo >> 5) * TILE_FLOATS) + (size_t)sub * 32 * 32;
        part = exact_slice_dot<PS>(&qs[sub][0][0], ctile, (int)(lo & 31));
    }
    // the 8 slice sums in wave order 0..7 (the scan kernels' split-K reduction order)
    float d = __shfl(part, (lane & ~7) | 0);
#pragma unroll
    for (int ww = 1; ww < 8; ++ww) d += __shfl(part, (lane & ~7) | ww);
    if (sub == 0 && slot < p.width) {
        const bool hit = live && found == id;
        uint32_t khi, klo;
        make_key(d, hit ? inv_row * qinv : 0.f, lo, khi, klo);
        const size_t o = (size_t)q * p.width + slot;
        p.keys[o] = mk64(khi, klo);
        if (p.out_slot_scores) p.out_slot_scores[o] = khi ? ord2f(khi) : __uint_as_float(0x7fc00000u);
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void subset_select_kernel(SubsetParams p) {
    __shared__ uint64_t keys[SS_W];
    __shared__ int wave_tot[SCAN_WAVES];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = p.k;
    const int count = clamp_count(p.counts[p.list_stride ? q : 0], p.width);
    int P = 1;
    while (P < count) P <<= 1;   // <= SS_W: width <= SS_W
    const uint64_t *mine = p.keys + (size_t)q * p.width;
    for (int i = tid; i < P; i += SCAN_THREADS) keys[i] = i < count ? mine[i] : 0ull;
    __syncthreads();
    sort_keys_desc(keys, P);   // bitonic, descending
    // the distinct non-zero keys, in order: thread t owns the contiguous run [t * per, t * per + per)
    const int per = (P + SCAN_THREADS - 1) / SCAN_THREADS, i0 = tid * per;
    int n_mine = 0;
    for (int i = i0; i < i0 + per && i < P; ++i) n_mine += (keys[i] != 0ull && (i == 0 || keys[i] != keys[i - 1])) ? 1 : 0;
    int incl = n_mine;   // inclusive scan over the wave, then the waves' totals in wave order
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int rank = incl - n_mine, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
        if (w < wave) rank += wave_tot[w];
        total += wave_tot[w];
    }
    for (int i = i0; i < i0 + per && i < P && rank < k; ++i) {
        const uint64_t key = keys[i];
        if (key != 0ull && (i == 0 || key != keys[i - 1])) {
            p.out_scores[(size_t)q * k + rank] = ord2f((uint32_t)(key >> 32));
            p.out_ids[(size_t)q * k + rank] = p.rows.stored[~(uint32_t)key];
            ++rank;
        }
    }
    const int n_out = total < k ? total : k;
    for (int r = n_out + tid; r < k; r += SCAN_THREADS) {
        p.out_scores[(size_t)q * k + r] = __uint_as_float(0x7fc00000u);
        p.out_ids[(size_t)q * k + r] = -1;
    }
    if (tid == 0) p.out_counts[q] = n_out;
}

}  // namespace

int64_t subset_scratch_bytes(int nq, int width) {
    return (int64_t)(nq > 1 ? nq : 1) * (width > 1 ? width : 1) * (int64_t)sizeof(uint64_t);
}

hipError_t launch_subset(const SubsetParams &p, hipStream_t st) {
    if (p.nq <= 0) return hipSuccess;
    const dim3 grid((p.width + SS_SLOTS - 1) / SS_SLOTS, p.nq);
    if (p.rows.piece_shift == PS_BIG) hipLaunchKernelGGL(subset_score_kernel<PS_BIG>, grid, dim3(SCAN_THREADS), 0, st, p);
    else hipLaunchKernelGGL(subset_score_kernel<PS_SMALL>, grid, dim3(SCAN_THREADS), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(subset_select_kernel, dim3(p.nq), dim3(SCAN_THREADS), 0, st, p);
    return hipGetLastError();
}

}  // namespace crag
