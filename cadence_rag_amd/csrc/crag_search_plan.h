// crag_search_plan.h — which kernels a search takes and how large its buffers are, as a function of plain numbers:
// no HIP call, no allocation, no index.  search_device (crag_api_search.hip) consumes the plan; crag_search_plan_
// exposes it to host tests, which is how the dispatch of every (size, nq, k) class is pinned without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "crag_kernels.h"

// developer switches that bear on the plan (read from the environment once, when the index is created)
struct SearchSwitches {
    int no_wide = 0;          // CRAG_NO_WIDE
    int no_prefilter = 0;     // CRAG_NO_PREFILTER
    int no_rsplit = 0;        // CRAG_NO_RSPLIT: one selection block per query for any k
    int pf_derive_lag = 2, pf_read_lag = 4;   // CRAG_PF_LAGS="d,r" (developer tuning; r <= 4 = the stashed tiles)
    int pf_nt = -1;           // CRAG_PF_NT=0/1 forces the cache policy of the prefilter scan
    int64_t nt_above_bytes = 1536ll << 20;    // mirror bytes above which its loads stream (measured: no gain below ~1 GB)
    int pf_waits = -1;        // CRAG_PF_WAITS=tile|fragment forces the wait schedule of the mirror scan (PfWaits)
};

struct SearchPlan {   // all int32: crag_search_plan_ hands it to ctypes as it is
    int wide;         // the 64-queries-per-pass kernels (two query blocks share every corpus fragment)
    int q_blocks;     // 32-query blocks
    int nq_pad;
    int G;            // scan workgroups
    int prefilter;    // fp16 prefilter scan + exact rescoring; 0: the plain fp32 scan
    int cap;          // candidates per query; a fuller list sends the search to the exact fallback
    int rsplit;       // selection blocks per query
    int nb;           // global-bound buckets in use (fp32 scan)
    int pub_rank;     // rank of the key a workgroup publishes (fp32 scan)
    int sets;         // class sets of the prefilter bound
    int pub0;         // rows of a workgroup's first tile that publish their score per query
    int derive_lag, read_lag;   // exchange lags in tiles: publish -> delegates derive -> every wave reads
    int nt;           // streaming cache policy for the mirror's loads
    int fb_blocks;    // workgroups of the selection launch that stand by for the exact fallback
    int window_too_large;   // a workgroup's corpus window reaches the buffer-descriptor / OOB-marker limit
};

inline SearchPlan plan_search(int64_t size, int n_cu, int nq, int k, bool has_mirror, bool irregular,
                              const SearchSwitches &sw) {
    SearchPlan pl;
    // more than 32 queries: two query blocks share every corpus fragment (64 queries per pass)
    pl.wide = (nq > 32 && !sw.no_wide) ? 1 : 0;
    pl.q_blocks = pl.wide ? ((nq + 63) / 64) * 2 : (nq + 31) / 32;
    pl.nq_pad = pl.q_blocks * 32;
    // one workgroup per CU; never more workgroups than 8-row groups
    pl.G = (int)std::max<int64_t>(1, std::min<int64_t>(n_cu, (size + 7) / 8));
    // the fp16 prefilter + exact rescoring path needs a few tiles per workgroup for its bounds to form;
    // small corpora take the plain fp32 scan (they are latency-, not bandwidth-bound anyway)
    pl.prefilter = (!sw.no_prefilter && !irregular && size >= (int64_t)pl.G * crag::PF_MIN_ROWS_PER_GROUP &&
                    (pl.wide || nq <= 32)) ? 1 : 0;
    // k > 104 (k_s = 27 .. 32 of a set's 32 class maxima: a weak bound) passes several thousand rows per query on a
    // 1M-row corpus
    pl.cap = (k > 104 && pl.nq_pad <= 128) ? 32768 : 8192;
    // large k: several selection blocks per query share the exact rescoring (see finalize_fb_kernel)
    pl.rsplit = (k <= 32 || sw.no_rsplit) ? 1 : (nq <= 16 ? 8 : (nq <= 128 ? 4 : 1));
    pl.nb = k < crag::GB_CELLS ? k : crag::GB_CELLS;
    pl.pub_rank = (k + pl.nb - 1) / pl.nb - 1;
    // class sets (32 * sets >= k; the bound is the k_s-th largest of a set's 32 class maxima, k_s = k / sets).  Two
    // sets up to k = 56 (k_s <= 28): measured at k = 50 against four sets (k_s = 12-13), 100 000 x 64: 78.9 vs
    // 82.3 us per step -- the half-wave sorts of every exchange cost more than the tighter bound returns
    pl.sets = k <= 24 ? 1 : (k <= 56 ? 2 : 4);
    pl.pub0 = (k + pl.sets - 1) / pl.sets >= 27 ? 8 : pl.sets;
    // Mirror scan 2 / 4; the scan of the fp32 rows (twice the time per tile, two stashed tiles) 1 / 2
    pl.derive_lag = has_mirror ? sw.pf_derive_lag : 1;
    pl.read_lag = has_mirror ? sw.pf_read_lag : 2;
    // streaming cache policy for a mirror far larger than the Infinity Cache (see prefilter_kernel)
    pl.nt = !has_mirror ? 0 : (sw.pf_nt >= 0 ? sw.pf_nt : (size * (int64_t)crag::DIM * 2 > sw.nt_above_bytes ? 1 : 0));
    // the fallback of a search whose candidate list overflows scans 32 queries per pass
    pl.fb_blocks = pl.G * ((nq + 31) / 32);
    const int64_t rows_per_g = (size + pl.G - 1) / pl.G + 64;
    pl.window_too_large = rows_per_g * (int64_t)(crag::DIM * 4) >= (int64_t)0x7ff00000 ? 1 : 0;
    return pl;
}

// Wait schedule of the mirror scan's corpus loads (crag::PfWaits; see prefilter_body).  Kept out of SearchPlan, whose
// layout host tests pin: search_device asks with the plan's nt.  The per-fragment schedule exists for the mirror with
// plain loads only; the switch (-1: by size) cannot force it onto another kernel.
inline int pf_waits_for(int64_t mirror_bytes, bool has_mirror, int nt, int pf_waits_switch) {
    if (!has_mirror || nt) return crag::PF_WAITS_TILE;
    if (pf_waits_switch >= 0) return pf_waits_switch ? crag::PF_WAITS_FRAGMENT : crag::PF_WAITS_TILE;
    return mirror_bytes <= crag::PF_FRAG_WAITS_MAX_BYTES ? crag::PF_WAITS_FRAGMENT : crag::PF_WAITS_TILE;
}
