// crag_rows.h -- what the operators on LISTED rows of the dense index share (crag_dedupe.hip, crag_mmr.hip,
// crag_subset.hip, crag_group.hip, the id lookup of crag_edit.hip): the view of the stored rows their parameter blocks
// carry, the count clamp, and the one place an id becomes a row position -- the lower-bound search in ascending values,
// scalar and nine-way, and dedupe's eligibility rule on top of it.  The BM25 kernels search their ascending postings with
// the same scalar routine.  The host fills a RowView with row_view() (crag_host.h); the functions are device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crag {

struct RowView {
    const float *corpus;        // tile32 layout (crag_layout.h)
    const float *inv_norm;      // [size] 1/||row||, 0: never eligible
    const int64_t *stored;      // [size] ids, ascending with the position
    int64_t size;
    int piece_shift;            // layout of the fp32 rows: crag_piece_shift(index has the fp16 mirror)
};

// a list's count as the kernels use it: clamped to [0, width]
__device__ __forceinline__ int clamp_count(int c, int width) { return c < 0 ? 0 : (c > width ? width : c); }

// first position in [lo, hi) whose value is >= x, hi if there is none; a[lo, hi) ascends
template <class T>
__device__ __forceinline__ int64_t lower_bound_asc(const T *a, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The same answer nine-way: first position whose stored id is >= id; the eight lanes of a slot call it together.
// A slot is lanes 8g .. 8g + 7 of a wave, which pass the same id and bounds; every lane of the wave must be in the call
// (it votes), a slot with nothing to find passes hi = lo.  8 probes per round -- 7 dependent round trips at a million
// rows instead of 20, for callers that are bound by latency.
// invariant: the answer lies in [lo, hi].  Lane `sub` = lane & 7 probes the last position of the (sub + 1)-th of nine
// parts; the ids ascend, so the probes below the id are a prefix of the eight: their number c picks the part.
__device__ __forceinline__ int64_t lower_bound_asc_x8(const int64_t *stored, int64_t lo, int64_t hi, int64_t id, int lane) {
    const int sub = lane & 7;
    while (__any(lo < hi)) {
        const int64_t step = (hi - lo + 8) / 9;
        const int64_t m = lo + (sub + 1) * step - 1;
        const bool below = lo < hi && m < hi && stored[m] < id;
        const unsigned long long b = __ballot(below);
        const int c = __popc((unsigned)(b >> (lane & ~7)) & 0xffu);
        if (lo < hi) {
            const int64_t mc = lo + (c + 1) * step - 1;   // the first probe that is not below the id, if there is one
            if (c < 8 && mc < hi) hi = mc;
            lo += c * step;
        }
    }
    return lo;
}

// Dedupe's eligibility rule, MMR's "comparable": the id is not the -1 pad, it is stored, and its row has 1/||row|| > 0.
// Then pos = its row position and inv = that 1/||row||; else pos = -1, inv = 0.
__device__ __forceinline__ bool comparable_row(const RowView &v, int64_t id, int64_t &pos, float &inv) {
    pos = -1;
    inv = 0.f;
    const int64_t lo = lower_bound_asc(v.stored, 0, v.size, id);
    if (id != -1 && lo < v.size && v.stored[lo] == id) {
        const float x = v.inv_norm[lo];
        if (x > 0.f) {
            pos = lo;
            inv = x;
        }
    }
    return pos >= 0;
}

}  // namespace crag
