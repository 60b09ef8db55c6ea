// crag_api_search.hip — the search calls of the C ABI: the launch sequence prep_queries -> scan -> selection on a
// per-stream workspace (what each search takes is decided in crag_search_plan.h), the pipelined form and its join, and
// the calls that work on ranked lists (dedupe, listed rows) and the search with a cap per group.  No exceptions cross
// the ABI.

#include "crag_index.h"

namespace {

struct SearchArgs {   // what the caller of a search passes, all on the device
    const float *queries;
    int nq, k;
    const uint8_t *mask;
    int64_t mask_stride;
    int64_t *out_ids;
    float *out_scores;
    int32_t *out_counts;
};

// The workspace of stream `st`: its own, else a free one, else the least recently used one of another stream.
int acquire_workspace(crag_index *ix, hipStream_t st, Workspace **out) {
    Workspace *ws = nullptr;
    for (auto &w : ix->ws)
        if (w.in_use && w.stream == st) ws = &w;
    if (!ws)
        for (auto &w : ix->ws)
            if (!w.in_use) {
                w.in_use = true;
                w.stream = st;
                ws = &w;
                // the last free workspace: the next new stream takes one over, so from now on every search records
                // its workspace's completion event (until then: no event packet per search -- it cost a step 4-7 us
                // for every caller with two to four streams, and for crag_index_search_pipelined)
                if (&w == &ix->ws[crag_index::MAX_WS - 1]) ix->record_done = true;
                break;
            }
    if (!ws) {
        // every workspace belongs to some other stream: take the least recently used one and make this
        // stream wait for the last search that used it (its owner may even be gone by now)
        for (auto &w : ix->ws)
            if (!ws || w.last_use < ws->last_use) ws = &w;
        if (ws->done_recorded && !ws->dirty) {   // (a failed search recorded no event)
            HIP_TRY(hipStreamWaitEvent(st, ws->done, 0));
        } else {
            // its last search predates the moment the workspaces ran out (no event was recorded then): wait for the device
            HIP_TRY(hipDeviceSynchronize());
        }
        ix->record_done = true;
        ws->stream = st;
    }
    ws->last_use = ++ix->use_clock;
    *out = ws;
    return CRAG_OK;
}

// Every allocation and memset of the search happens HERE, in front of its first launch: an allocation that fails
// between the scan and the selection launch would leave the scan's per-query state behind (and a hipFree /
// hipMalloc between two launches synchronises the device).
int reserve_workspace(const crag_index *ix, Workspace *ws, const SearchPlan &pl, int k, hipStream_t st) {
    DevBuf *b = ws->buf;
    const size_t nq_pad = (size_t)pl.nq_pad;
    int rc;
    if ((rc = b[Workspace::PARTIAL].ensure((size_t)pl.q_blocks * pl.G * 32 * (size_t)k * sizeof(uint2)))) return rc;
    // (re)allocated buffers start zeroed; merge re-zeroes after use
    if ((rc = b[Workspace::GBOUND].ensure_zeroed((size_t)pl.q_blocks * 32 * crag::GB_CELLS * sizeof(uint32_t), st))) return rc;
    if ((rc = b[Workspace::A32].ensure(nq_pad * crag::DIM * sizeof(float)))) return rc;
    if ((rc = b[Workspace::QINV].ensure(nq_pad * sizeof(float)))) return rc;
    if (!pl.prefilter) return CRAG_OK;
    if ((rc = b[Workspace::A16].ensure(nq_pad * crag::DIM * 2))) return rc;
    // n_cu idle records of zeros that nothing ever writes (zeroed once, when the buffer is allocated; at the FRONT, so
    // that no later search with fewer queries finds an old query record there), then the queries' bound records (left
    // zeroed by the selection kernel of every search)
    if ((rc = b[Workspace::PF_GBOUND].ensure_zeroed((ix->n_cu + nq_pad) * crag::PF_BOUND_CELLS * sizeof(uint32_t), st))) return rc;
    if ((rc = b[Workspace::PF_CAND].ensure(nq_pad * pl.cap * sizeof(uint2)))) return rc;
    if (pl.rsplit > 1) {   // scratch of the selection blocks that share a query (k > 32)
        const size_t slots = nq_pad * 8;
        if ((rc = b[Workspace::PF_XKEYS].ensure(slots * CRAG_MAX_K * sizeof(uint64_t)))) return rc;
        if ((rc = b[Workspace::PF_XIDS].ensure(slots * CRAG_MAX_K * sizeof(int64_t)))) return rc;
        if ((rc = b[Workspace::PF_XCOUNT].ensure(slots * sizeof(uint2)))) return rc;
        if ((rc = b[Workspace::PF_XTICKET].ensure_zeroed(nq_pad * sizeof(uint32_t), st))) return rc;
    }
    // per-query candidate counts and the overflow / ticket words: zero when allocated, kept clean by the kernels
    if ((rc = b[Workspace::PF_COUNT].ensure_zeroed(nq_pad * sizeof(uint32_t), st))) return rc;
    if ((rc = b[Workspace::PF_FLAGS].ensure_zeroed(4 * sizeof(uint32_t), st))) return rc;
    if (ws->dirty) {  // the last search on this workspace died between scan and selection: nothing cleaned up
        for (int i = Workspace::KEPT_ZERO_FIRST; i < Workspace::KEPT_ZERO_END; ++i)
            if (b[i].p) HIP_TRY(hipMemsetAsync(b[i].p, 0, b[i].bytes, st));
        ws->dirty = false;
    }
    return CRAG_OK;
}

// (the sampled search is the one in the MIDDLE of every window of N: with a caller that synchronises every N searches
// the first of a window starts on an idle GPU and is not the typical one)
int profile_begin(crag_index *ix, hipStream_t st, EvSet **out) {
    *out = nullptr;
    if (!(ix->profiling > 0 && (ix->prof_calls++ % ix->profiling) == ix->profiling / 2)) return CRAG_OK;
    if (ix->ev_used == ix->ev_pool.size()) {
        EvSet t;
        for (hipEvent_t *e : {&t.e0, &t.e1a, &t.e1, &t.e2, &t.e3}) HIP_TRY(hipEventCreate(e));
        ix->ev_pool.push_back(t);
    }
    *out = &ix->ev_pool[ix->ev_used++];
    HIP_TRY(hipEventRecord((*out)->e0, st));
    return CRAG_OK;
}

// K0: 1/||q||, the queries in A-fragment order, reset of the prefilter state
crag::PrepParams prep_params(const crag_index *ix, const Workspace *ws, const SearchPlan &pl, const SearchArgs &a) {
    // (the fp32 fragments are the fp32 scan's operand; the prefilter path's selection blocks read the raw queries)
    return crag::PrepParams{a.queries, a.nq, ix->dim, ws->at<float>(Workspace::QINV),
                            pl.prefilter ? nullptr : ws->at<float>(Workspace::A32),
                            pl.prefilter ? ws->at<_Float16>(Workspace::A16) : nullptr};
}

crag::ScanParams scan_params(const crag_index *ix, const Workspace *ws, const SearchPlan &pl, const SearchArgs &a,
                             int reverse) {
    crag::ScanParams sp;
    sp.wide = pl.wide;
    sp.corpus = ix->corpus;
    sp.inv_norm = ix->inv_norm;
    sp.queries = a.queries;
    sp.a32 = ws->at<const float>(Workspace::A32);
    sp.qinv = ws->at<const float>(Workspace::QINV);
    sp.gate = nullptr;
    sp.dim = ix->dim;
    sp.mask = (const uint32_t *)a.mask;
    sp.mask_stride_w = a.mask_stride / 4;
    sp.partial = ws->at<uint2>(Workspace::PARTIAL);
    sp.gbound = ws->at<uint32_t>(Workspace::GBOUND);
    sp.n_rows = ix->size;
    sp.cap_rows = ix->cap_rows;
    sp.nq = a.nq;
    sp.k = a.k;
    sp.G = pl.G;
    sp.nb = pl.nb;
    sp.pub_rank = pl.pub_rank;
    sp.reverse = reverse;
    sp.unpipelined = (ix->env_unpipelined && !pl.prefilter) ? 1 : 0;
    sp.piece_shift = crag::crag_piece_shift(ix->corpus16 != nullptr);
    return sp;
}

crag::MergeParams merge_params(const crag_index *ix, const Workspace *ws, const SearchPlan &pl, const SearchArgs &a) {
    crag::MergeParams mp;
    mp.partial = ws->at<const uint2>(Workspace::PARTIAL);
    mp.ids = ix->ids;
    mp.gbound = ws->at<uint32_t>(Workspace::GBOUND);
    mp.id_base = 0;
    mp.out_ids = a.out_ids;
    mp.out_scores = a.out_scores;
    mp.out_counts = a.out_counts;
    mp.k = a.k;
    mp.G = pl.G;
    return mp;
}

// K1: fp16 scan -> candidates
crag::PfParams pf_params(const crag_index *ix, const Workspace *ws, const SearchPlan &pl, const SearchArgs &a,
                         int reverse) {
    crag::PfParams fp;
    fp.corpus = ix->corpus;
    fp.corpus16 = ix->corpus16;
    fp.inv_norm = ix->inv_norm;
    fp.a16 = ws->at<const _Float16>(Workspace::A16);
    fp.qinv = ws->at<const float>(Workspace::QINV);
    fp.mask = (const uint32_t *)a.mask;
    fp.mask_stride_w = a.mask_stride / 4;
    fp.gbound_idle = ws->at<const uint32_t>(Workspace::PF_GBOUND);
    fp.gbound = ws->at<uint32_t>(Workspace::PF_GBOUND) + (size_t)ix->n_cu * crag::PF_BOUND_CELLS;
    fp.cand = ws->at<uint2>(Workspace::PF_CAND);
    fp.count = ws->at<uint32_t>(Workspace::PF_COUNT);
    fp.flags = ws->at<uint32_t>(Workspace::PF_FLAGS);
    fp.seq = ws->seq;
    fp.n_rows = ix->size;
    fp.nq = a.nq;
    fp.k = a.k;
    fp.G = pl.G;
    fp.reverse = reverse;
    fp.sets = pl.sets;
    fp.pub0 = pl.pub0;
    fp.cap = pl.cap;
    fp.derive_lag = pl.derive_lag;
    fp.read_lag = pl.read_lag;
    fp.nt = pl.nt;
    return fp;
}

// K2: exact rescoring + selection, and -- workgroups of the same launch that end at once unless a candidate list
// overflowed -- the fp32 fallback scan + merge
crag::FinParams fin_params(const crag_index *ix, const Workspace *ws, const SearchPlan &pl, const SearchArgs &a,
                           const crag::PfParams &fp, crag::ScanParams sp, const crag::MergeParams &mp) {
    crag::FinParams fin;
    fin.corpus = ix->corpus;
    fin.inv_norm = ix->inv_norm;
    fin.qinv = ws->at<const float>(Workspace::QINV);
    fin.cand = ws->at<const uint2>(Workspace::PF_CAND);
    fin.count = ws->at<uint32_t>(Workspace::PF_COUNT);
    fin.gbound = fp.gbound;
    fin.flags = ws->at<const uint32_t>(Workspace::PF_FLAGS);
    fin.seq = fp.seq;
    fin.ids = ix->ids;
    fin.out_ids = a.out_ids;
    fin.out_scores = a.out_scores;
    fin.out_counts = a.out_counts;
    // statistics records: one block of PF_STAT_SLOTS / MAX_WS records per workspace, so that searches overlapping
    // on several streams never share a record (queries beyond a block's size fold onto it: counts may be lost
    // there, results never depend on them)
    fin.stats = ix->pf_stats + (size_t)(ws - ix->ws) * (crag::PF_STAT_SLOTS / crag_index::MAX_WS) * 3;
    fin.k = a.k;
    fin.cap = pl.cap;
    fin.merge = mp;
    fin.nq = a.nq;
    fin.rsplit = pl.rsplit;
    const bool shared = pl.rsplit > 1;   // several selection blocks per query: their exchange scratch
    fin.xkeys = shared ? ws->at<uint64_t>(Workspace::PF_XKEYS) : nullptr;
    fin.xids = shared ? ws->at<int64_t>(Workspace::PF_XIDS) : nullptr;
    fin.xcount = shared ? ws->at<uint2>(Workspace::PF_XCOUNT) : nullptr;
    fin.xticket = shared ? ws->at<uint32_t>(Workspace::PF_XTICKET) : nullptr;
    // the fallback of a search whose candidate list overflows: the self-contained generic scan (32 queries per
    // pass) inside the same launch, see finalize_fb_kernel
    sp.wide = 0;
    sp.gate = nullptr;
    sp.unpipelined = 1;
    fin.scan = sp;
    fin.fb_blocks = pl.fb_blocks;
    fin.fb_done = ws->at<uint32_t>(Workspace::PF_FLAGS) + 1;
    fin.trace = ix->phase_trace;
    return fin;
}

int search_device(crag_index *ix, const SearchArgs &a, hipStream_t st) {
    if (a.nq <= 0) return CRAG_OK;
    const SearchPlan pl = plan_search(ix->size, ix->n_cu, a.nq, a.k, ix->corpus16 != nullptr, ix->irregular, ix->sw);
    int rc;
    Workspace *ws = nullptr;
    if ((rc = acquire_workspace(ix, st, &ws))) return rc;
    if ((rc = reserve_workspace(ix, ws, pl, a.k, st))) return rc;
    if (pl.window_too_large)
        return fail(CRAG_EINVAL, "index too large for one device scan window (%lld rows)", (long long)ix->size);
    EvSet *ev = nullptr;
    if ((rc = profile_begin(ix, st, &ev))) return rc;

    HIP_TRY(crag::launch_prep_queries(prep_params(ix, ws, pl, a), pl.nq_pad, st));
    const int reverse = ix->env_no_reverse ? 0 : ix->pass_parity;
    ix->pass_parity ^= 1;
    const crag::ScanParams sp = scan_params(ix, ws, pl, a, reverse);
    const crag::MergeParams mp = merge_params(ix, ws, pl, a);
    if (ev) {
        HIP_TRY(hipEventRecord(ev->e1a, st));
        HIP_TRY(hipEventRecord(ev->e1, st));
    }
    if (pl.prefilter) {
        if (++ws->seq == 0u) ws->seq = 1u;
        const crag::PfParams fp = pf_params(ix, ws, pl, a, reverse);
        const int nqb = pl.wide ? 2 : 1;
        ws->dirty = true;   // until the selection launch is in the stream
        const int waits = pf_waits_for(ix->size * (int64_t)crag::DIM * 2, ix->corpus16 != nullptr, pl.nt, ix->sw.pf_waits);
        HIP_TRY(crag::launch_prefilter(fp, nqb, pl.nq_pad / (32 * nqb), waits == crag::PF_WAITS_FRAGMENT, st,
                                       &ix->last_scan_kernel));
        ix->last_scan_waits = waits == crag::PF_WAITS_FRAGMENT ? "fragment" : "tile";
        if (ix->env_fail_after_scan > 0 && ++ix->pf_searches == ix->env_fail_after_scan)
            return fail(CRAG_EHIP, "injected failure behind the scan launch (CRAG_TEST_FAIL_AFTER_SCAN)");
        if (ev) HIP_TRY(hipEventRecord(ev->e2, st));
        HIP_TRY(crag::launch_finalize(fin_params(ix, ws, pl, a, fp, sp, mp), st));
        ws->dirty = false;
    } else {
        HIP_TRY(crag::launch_scan(sp, pl.q_blocks, st, &ix->last_scan_kernel));
        ix->last_scan_waits = "tile";
        if (ev) HIP_TRY(hipEventRecord(ev->e2, st));
        HIP_TRY(crag::launch_merge_partials(mp, a.nq, st));
    }
    if (ev) HIP_TRY(hipEventRecord(ev->e3, st));
    // what a stream that later takes this workspace over waits for.  Recorded only once every workspace has an owner:
    // callers with up to MAX_WS streams (the pipelined form's three included) pay no event packet per search.
    ws->done_recorded = ix->record_done;
    if (ix->record_done) HIP_TRY(hipEventRecord(ws->done, st));
    return CRAG_OK;
}

int check_search_args(const crag_index *ix, const SearchArgs &a) {   // (pointers on either side)
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (a.nq < 0) return fail(CRAG_EINVAL, "nq must be >= 0 (got %d)", a.nq);
    if (a.k <= 0 || a.k > CRAG_MAX_K) return fail(CRAG_EINVAL, "k must be in [1, %d] (got %d)", CRAG_MAX_K, a.k);
    if (a.nq > 0 && (!a.queries || !a.out_ids || !a.out_scores || !a.out_counts))
        return fail(CRAG_EINVAL, "queries / out_ids / out_scores / out_counts must not be NULL");
    if (a.mask) {
        const int64_t need = ((ix->size + 31) / 32) * 4;
        if (a.mask_stride != 0 && (a.mask_stride % 4 != 0 || a.mask_stride < need))
            return fail(CRAG_EINVAL, "mask_stride must be 0 or a multiple of 4 >= %lld (got %lld)",
                        (long long)need, (long long)a.mask_stride);
        if (((uintptr_t)a.mask) & 3) return fail(CRAG_EINVAL, "row_mask must be 4-byte aligned");
    }
    return CRAG_OK;
}

}  // namespace

extern "C" {

int crag_search_plan_(int64_t size, int n_cu, int nq, int k, int has_mirror, int irregular, int no_wide,
                      int no_prefilter, int no_rsplit, int pf_derive_lag, int pf_read_lag, int pf_nt,
                      int64_t nt_above_bytes, SearchPlan *out) {
    const SearchSwitches sw = {no_wide, no_prefilter, no_rsplit, pf_derive_lag, pf_read_lag, pf_nt, nt_above_bytes};
    if (out) *out = plan_search(size, n_cu, nq, k, has_mirror != 0, irregular != 0, sw);
    return (int)sizeof(SearchPlan);
}

int crag_pf_waits_(int64_t mirror_bytes, int has_mirror, int nt, int pf_waits_switch) {
    return pf_waits_for(mirror_bytes, has_mirror != 0, nt, pf_waits_switch);
}

int64_t crag_pf_frag_waits_max_bytes_(void) { return crag::PF_FRAG_WAITS_MAX_BYTES; }

int crag_index_search_async(crag_index *ix, const float *d_queries, int nq, int k,
                            const uint8_t *d_row_mask, int64_t mask_stride, int64_t *d_out_ids,
                            float *d_out_scores, int32_t *d_out_counts, void *stream) {
    const SearchArgs a = {d_queries, nq, k, d_row_mask, mask_stride, d_out_ids, d_out_scores, d_out_counts};
    int rc = check_search_args(ix, a);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    return search_device(ix, a, (hipStream_t)stream);
}

int crag_index_search_pipelined(crag_index *ix, const float *d_queries, int nq, int k,
                                const uint8_t *d_row_mask, int64_t mask_stride, int64_t *d_out_ids,
                                float *d_out_scores, int32_t *d_out_counts, void *stream, int flags) {
    const SearchArgs a = {d_queries, nq, k, d_row_mask, mask_stride, d_out_ids, d_out_scores, d_out_counts};
    int rc = check_search_args(ix, a);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    for (int i = 0; i < ix->n_pipe; ++i) {   // created on first use; a creation that failed is tried again, not skipped
        if (!ix->pipe[i]) HIP_TRY(hipStreamCreateWithFlags(&ix->pipe[i], hipStreamNonBlocking));
        if (!ix->pipe_fork[i]) HIP_TRY(hipEventCreateWithFlags(&ix->pipe_fork[i], hipEventDisableTiming));
        if (!ix->pipe_done[i]) HIP_TRY(hipEventCreateWithFlags(&ix->pipe_done[i], hipEventDisableTiming));
    }
    // Overlap pays for the searches whose small kernels are a large share of the step -- k <= 24 (one class set): 100 000
    // x 64, k = 10: 40.2 us per step on three streams against 47.7 in order; 1M: 316 against 322 -- and costs for larger k,
    // whose scans disturb each other's bound exchange (k = 100 at 100 000 rows: 74-80 us against 71).  Those run in
    // stream order on the caller's stream (the join then has nothing to wait for).
    if (k > 24 || ix->n_pipe <= 1) return search_device(ix, a, (hipStream_t)stream);
    const int i = (int)(ix->pipe_next++ % (unsigned)ix->n_pipe);
    if (!(flags & CRAG_PIPE_INPUTS_READY)) {
        HIP_TRY(hipEventRecord(ix->pipe_fork[i], (hipStream_t)stream));
        HIP_TRY(hipStreamWaitEvent(ix->pipe[i], ix->pipe_fork[i], 0));
    }
    rc = search_device(ix, a, ix->pipe[i]);
    if (rc) return rc;
    ix->pipe_pending[i] = true;   // (its completion event is recorded by the join: one per fence and stream, not per search)
    return CRAG_OK;
}

int crag_index_join(crag_index *ix, void *stream) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    for (int i = 0; i < ix->n_pipe; ++i)
        if (ix->pipe_pending[i]) {
            HIP_TRY(hipEventRecord(ix->pipe_done[i], ix->pipe[i]));
            HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ix->pipe_done[i], 0));
            ix->pipe_pending[i] = false;
        }
    return CRAG_OK;
}

int crag_index_search(crag_index *ix, const float *queries, int nq, int k, const uint8_t *row_mask,
                      int64_t mask_stride, int64_t *out_ids, float *out_scores, int32_t *out_counts) {
    int rc = check_search_args(ix, {queries, nq, k, row_mask, mask_stride, out_ids, out_scores, out_counts});
    if (rc) return rc;
    if (nq == 0) return CRAG_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);

    const float *dq = nullptr;
    if ((rc = stage_in(ix->stage_q, queries, (size_t)nq * ix->dim * sizeof(float), &dq))) return rc;
    const uint8_t *dm = nullptr;
    int64_t dstride = 0;
    if ((rc = stage_row_masks(ix, row_mask, mask_stride, nq, &dm, &dstride))) return rc;
    const bool ids_dev = is_device_ptr(out_ids), sc_dev = is_device_ptr(out_scores),
               ct_dev = is_device_ptr(out_counts);
    const size_t b_ids = (size_t)nq * k * sizeof(int64_t), b_sc = (size_t)nq * k * sizeof(float),
                 b_ct = (size_t)nq * sizeof(int32_t);
    if ((rc = ix->stage_out.ensure(b_ids + b_sc + b_ct + 64))) return rc;
    char *so = (char *)ix->stage_out.p;
    int64_t *d_ids = ids_dev ? out_ids : (int64_t *)so;
    float *d_sc = sc_dev ? out_scores : (float *)(so + b_ids);
    int32_t *d_ct = ct_dev ? out_counts : (int32_t *)(so + b_ids + b_sc);

    rc = search_device(ix, {dq, nq, k, dm, dstride, d_ids, d_sc, d_ct}, 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    if (!ids_dev) HIP_TRY(hipMemcpy(out_ids, d_ids, b_ids, hipMemcpyDeviceToHost));
    if (!sc_dev) HIP_TRY(hipMemcpy(out_scores, d_sc, b_sc, hipMemcpyDeviceToHost));
    if (!ct_dev) HIP_TRY(hipMemcpy(out_counts, d_ct, b_ct, hipMemcpyDeviceToHost));
    return CRAG_OK;
}

int crag_index_dedupe_async(crag_index *ix, const int64_t *d_ids, const int32_t *d_counts, int nq, int width,
                            float threshold, int64_t *d_out_ids, int32_t *d_out_counts, int32_t *d_out_dup_of,
                            float *d_out_sim, void *stream) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (nq < 0) return fail(CRAG_EINVAL, "nq must be >= 0 (got %d)", nq);
    if (width < 1 || width > CRAG_DEDUPE_MAX_WIDTH)
        return fail(CRAG_EINVAL, "width must be in [1, %d] (got %d)", CRAG_DEDUPE_MAX_WIDTH, width);
    if (!(threshold > -1.f && threshold <= 1.f))   // (NaN fails both)
        return fail(CRAG_EINVAL, "threshold must be finite, in (-1, 1] (got %g)", (double)threshold);
    if (!d_ids || !d_counts || !d_out_ids || !d_out_counts)
        return fail(CRAG_EINVAL, "ids / counts / out_ids / out_counts must not be NULL");
    if (nq == 0) return CRAG_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    crag::DedupeParams p;
    p.rows = row_view(ix);
    p.ids = d_ids;
    p.counts = d_counts;
    p.width = width;
    p.threshold = threshold;
    p.out_ids = d_out_ids;
    p.out_counts = d_out_counts;
    p.out_dup_of = d_out_dup_of;
    p.out_sim = d_out_sim;
    HIP_TRY(crag::launch_dedupe(p, nq, (hipStream_t)stream));
    return CRAG_OK;
}

int64_t crag_index_search_ids_scratch_bytes(int nq, int width) { return crag::subset_scratch_bytes(nq, width); }

int crag_index_search_ids_async(crag_index *ix, const float *d_queries, int nq, const int64_t *d_ids,
                                const int32_t *d_counts, int width, int64_t list_stride, int k, int64_t *d_out_ids,
                                float *d_out_scores, int32_t *d_out_counts, float *d_out_slot_scores, void *d_scratch,
                                int64_t scratch_bytes, void *stream) {
    if (!ix) return fail(CRAG_EINVAL, "search_ids: index is NULL");
    if (int rc = check_nq("search_ids", nq)) return rc;
    if (width < 1) return fail(CRAG_EINVAL, "search_ids: width must be >= 1 (got %d)", width);
    if (k < 1 || k > CRAG_MAX_K) return fail(CRAG_EINVAL, "search_ids: k must be in [1, %d] (got %d)", CRAG_MAX_K, k);
    if (list_stride != 0 && list_stride != width)
        return fail(CRAG_EINVAL, "search_ids: list_stride must be 0 (one shared list) or width (got %lld)",
                    (long long)list_stride);
    if (!d_queries || !d_ids || !d_counts || !d_out_ids || !d_out_scores || !d_out_counts || !d_scratch)
        return fail(CRAG_EINVAL, "search_ids: queries / ids / counts / outputs / scratch must not be NULL");
    if (width > CRAG_SUBSET_MAX_WIDTH)
        return fail(CRAG_E2BIG, "search_ids: width %d exceeds CRAG_SUBSET_MAX_WIDTH (%d): use the row_mask route", width,
                    CRAG_SUBSET_MAX_WIDTH);
    if (int rc = check_scratch("search_ids", d_scratch, scratch_bytes, crag::subset_scratch_bytes(nq, width),
                               "crag_index_search_ids_scratch_bytes"))
        return rc;
    if (nq == 0) return CRAG_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    crag::SubsetParams p;
    p.rows = row_view(ix);
    p.queries = d_queries;
    p.nq = nq;
    p.dim = ix->dim;
    p.k = k;
    p.ids = d_ids;
    p.counts = d_counts;
    p.width = width;
    p.list_stride = list_stride;
    p.keys = (uint64_t *)d_scratch;
    p.out_ids = d_out_ids;
    p.out_scores = d_out_scores;
    p.out_counts = d_out_counts;
    p.out_slot_scores = d_out_slot_scores;
    HIP_TRY(crag::launch_subset(p, (hipStream_t)stream));
    return CRAG_OK;
}

int64_t crag_index_mmr_scratch_bytes(int nq, int width) { return crag::mmr_scratch_bytes(nq, width); }

int crag_index_mmr_async(crag_index *ix, const int64_t *d_ids, const float *d_rel, const int32_t *d_counts, int nq,
                         int width, float lambda, int k, int64_t *d_out_ids, float *d_out_rel, float *d_out_value,
                         int32_t *d_out_slots, float *d_out_sim_rows, int32_t *d_out_counts, void *d_scratch,
                         int64_t scratch_bytes, void *stream) {
    if (!ix) return fail(CRAG_EINVAL, "mmr: index is NULL");
    if (int rc = check_nq("mmr", nq)) return rc;
    if (width < 1 || width > CRAG_MMR_MAX_WIDTH)
        return fail(CRAG_EINVAL, "mmr: width must be in [1, %d] (got %d)", CRAG_MMR_MAX_WIDTH, width);
    if (k < 1 || k > CRAG_MMR_MAX_WIDTH) return fail(CRAG_EINVAL, "mmr: k must be in [1, %d] (got %d)", CRAG_MMR_MAX_WIDTH, k);
    if (!(lambda >= 0.f && lambda <= 1.f))   // (NaN fails both)
        return fail(CRAG_EINVAL, "mmr: lambda must be finite, in [0, 1] (got %g)", (double)lambda);
    if (!d_ids || !d_rel || !d_counts || !d_out_ids || !d_out_rel || !d_out_counts || !d_scratch)
        return fail(CRAG_EINVAL, "mmr: ids / rel / counts / out_ids / out_rel / out_counts / scratch must not be NULL");
    if (int rc = check_scratch("mmr", d_scratch, scratch_bytes, crag::mmr_scratch_bytes(nq, width),
                               "crag_index_mmr_scratch_bytes"))
        return rc;
    if (nq == 0) return CRAG_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    crag::MmrParams p;
    p.rows = row_view(ix);
    p.ids = d_ids;
    p.rel = d_rel;
    p.counts = d_counts;
    p.nq = nq;
    p.width = width;
    p.k = k;
    p.lambda = lambda;
    p.mu = 1.0f - lambda;
    p.gram = (float *)d_scratch;
    p.out_ids = d_out_ids;
    p.out_rel = d_out_rel;
    p.out_value = d_out_value;
    p.out_slots = d_out_slots;
    p.out_sim_rows = d_out_sim_rows;
    p.out_counts = d_out_counts;
    HIP_TRY(crag::launch_mmr(p, (hipStream_t)stream));
    return CRAG_OK;
}

int64_t crag_index_search_grouped_scratch_bytes(int nq, int64_t n_groups, int per_group) {
    return crag::group_scratch_bytes(nq, n_groups, per_group);
}

int crag_index_search_grouped_async(crag_index *ix, const float *d_queries, int nq, int k, const int32_t *d_row_group,
                                    int64_t n_groups, int per_group, const uint8_t *d_row_mask, int64_t mask_stride,
                                    int64_t *d_out_ids, float *d_out_scores, int32_t *d_out_groups, int32_t *d_out_counts,
                                    void *d_scratch, int64_t scratch_bytes, void *stream) {
    if (!ix) return fail(CRAG_EINVAL, "search_grouped: index is NULL");
    if (int rc = check_nq("search_grouped", nq)) return rc;
    if (k < 1 || k > CRAG_MAX_K) return fail(CRAG_EINVAL, "search_grouped: k must be in [1, %d] (got %d)", CRAG_MAX_K, k);
    if (per_group < 1 || per_group > CRAG_GROUP_MAX_PER)
        return fail(CRAG_EINVAL, "search_grouped: per_group must be in [1, %d] (got %d)", CRAG_GROUP_MAX_PER, per_group);
    if (n_groups < 1 || n_groups >= ((int64_t)1 << 31))
        return fail(CRAG_EINVAL, "search_grouped: n_groups must be in [1, 2^31) (got %lld)", (long long)n_groups);
    if (!d_queries || !d_row_group || !d_out_ids || !d_out_scores || !d_out_counts || !d_scratch)
        return fail(CRAG_EINVAL, "search_grouped: queries / row_group / out_ids / out_scores / out_counts / scratch must not be NULL");
    if (d_row_mask) {   // what check_search_args refuses
        const int64_t need = ((ix->size + 31) / 32) * 4;
        if (mask_stride != 0 && (mask_stride % 4 != 0 || mask_stride < need))
            return fail(CRAG_EINVAL, "search_grouped: mask_stride must be 0 or a multiple of 4 >= %lld (got %lld)",
                        (long long)need, (long long)mask_stride);
        if (((uintptr_t)d_row_mask) & 3) return fail(CRAG_EINVAL, "search_grouped: row_mask must be 4-byte aligned");
    }
    if (int rc = check_scratch("search_grouped", d_scratch, scratch_bytes, crag::group_scratch_bytes(nq, n_groups, per_group),
                               "crag_index_search_grouped_scratch_bytes"))
        return rc;
    if (nq == 0) return CRAG_OK;
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    crag::GroupParams p;
    p.rows = row_view(ix);
    p.queries = d_queries;
    p.nq = nq;
    p.dim = ix->dim;
    p.k = k;
    p.row_group = d_row_group;
    p.n_groups = n_groups;
    p.per_group = per_group;
    p.mask = (const uint32_t *)d_row_mask;
    p.mask_stride_w = mask_stride / 4;
    p.table = (uint64_t *)d_scratch;
    p.qinv = (float *)(p.table + (size_t)nq * (size_t)n_groups * (size_t)per_group);
    p.out_ids = d_out_ids;
    p.out_scores = d_out_scores;
    p.out_groups = d_out_groups;
    p.out_counts = d_out_counts;
    HIP_TRY(crag::launch_grouped(p, (hipStream_t)stream));
    return CRAG_OK;
}

}  // extern "C"
