// crag_api.hip — host side of the C ABI declared in include/crag_dense.h: the error message, the index's life cycle,
// introspection, profiling and the cross-shard merge.  The index owns the device corpus (tile32 layout, see
// crag_search.hip) and the workspaces; searches are in crag_api_search.hip, rows and edits in crag_api_store.hip.
// No exceptions cross the ABI.

#include <stdlib.h>

#include <new>

#include "crag_index.h"

namespace {

thread_local char g_err[512] = "";

// everything crag_index_create sets up behind the allocation of the index itself; on failure the caller destroys it
int init_index(crag_index *ix) {
    const size_t cbytes = (size_t)ix->cap_rows * crag::DIM * sizeof(float);
    hipError_t e;
    if ((e = hipMalloc((void **)&ix->corpus, cbytes)) != hipSuccess ||
        (e = hipMalloc((void **)&ix->inv_norm, (size_t)ix->cap_rows * sizeof(float))) != hipSuccess ||
        (e = hipMalloc((void **)&ix->ids, (size_t)ix->cap_rows * sizeof(int64_t))) != hipSuccess)
        return fail(CRAG_ENOMEM, "hipMalloc for %lld rows failed: %s", (long long)ix->cap_rows, hipGetErrorString(e));
    // padding rows of the last tile must read as "never eligible" and finite
    if ((e = hipMemset(ix->inv_norm, 0, (size_t)ix->cap_rows * sizeof(float))) != hipSuccess ||
        (e = hipMemset(ix->corpus, 0, cbytes)) != hipSuccess)
        return fail(CRAG_EHIP, "hipMemset failed: %s", hipGetErrorString(e));
    for (auto &w : ix->ws)
        if ((e = hipEventCreateWithFlags(&w.done, hipEventDisableTiming)) != hipSuccess)
            return fail(CRAG_EHIP, "hipEventCreate failed: %s", hipGetErrorString(e));
    ix->sw.no_wide = getenv("CRAG_NO_WIDE") != nullptr;
    ix->env_no_reverse = getenv("CRAG_NO_REVERSE") != nullptr;
    ix->env_unpipelined = getenv("CRAG_UNPIPELINED") != nullptr;
    ix->sw.no_prefilter = getenv("CRAG_NO_PREFILTER") != nullptr;
    ix->sw.no_rsplit = getenv("CRAG_NO_RSPLIT") != nullptr;
    if (const char *v = getenv("CRAG_PF_NT")) ix->sw.pf_nt = atoi(v) ? 1 : 0;
    if (const char *v = getenv("CRAG_PF_WAITS")) {
        if (!strcmp(v, "tile")) ix->sw.pf_waits = crag::PF_WAITS_TILE;
        else if (!strcmp(v, "fragment")) ix->sw.pf_waits = crag::PF_WAITS_FRAGMENT;
    }
    if (const char *v = getenv("CRAG_PF_LAGS")) {
        int d = 0, r = 0;
        if (sscanf(v, "%d,%d", &d, &r) == 2 && d >= 1 && r > d && r <= 4) {
            ix->sw.pf_derive_lag = d;
            ix->sw.pf_read_lag = r;
        }
    }
    if (const char *v = getenv("CRAG_TEST_FAIL_AFTER_SCAN")) ix->env_fail_after_scan = atoll(v);
    if (const char *v = getenv("CRAG_PIPE_STREAMS")) {
        const int n = atoi(v);
        if (n >= 1 && n <= crag_index::MAX_PIPE) ix->n_pipe = n;
    }
    if (const char *v = getenv("CRAG_EDIT_CHUNK_ROWS")) {   // developer switch: tests cross chunk boundaries on small tables
        const long long c = atoll(v);
        if (c >= 32 && c % 32 == 0 && c <= ((long long)1 << 24)) ix->edit_chunk_rows = c;
    }
    if (const char *v = getenv("CRAG_PF_NT_ABOVE_MB")) ix->sw.nt_above_bytes = (int64_t)atoll(v) << 20;
    if (!ix->sw.no_prefilter && getenv("CRAG_NO_FP16_MIRROR") == nullptr) {
        // + 2 KiB per row beside the 4 KiB fp32 row: the prefilter scan then streams half the bytes.  Padding rows
        // read as zeros (their positions are beyond every workgroup's row range anyway).
        const size_t mbytes = (size_t)ix->cap_rows * crag::DIM * sizeof(_Float16);
        if ((e = hipMalloc((void **)&ix->corpus16, mbytes)) != hipSuccess ||
            (e = hipMemset(ix->corpus16, 0, mbytes)) != hipSuccess)
            return fail(CRAG_ENOMEM, "hipMalloc for the fp16 mirror of %lld rows failed: %s", (long long)ix->cap_rows,
                        hipGetErrorString(e));
    }
    if ((e = hipMalloc((void **)&ix->irregular_dev, sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc((void **)&ix->pf_stats, crag::PF_STAT_SLOTS * 3 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(ix->irregular_dev, 0, sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemset(ix->pf_stats, 0, crag::PF_STAT_SLOTS * 3 * sizeof(unsigned long long))) != hipSuccess)
        return fail(CRAG_ENOMEM, "hipMalloc for the index state failed: %s", hipGetErrorString(e));
    if (getenv("CRAG_PHASE_TRACE") != nullptr) {
        if ((e = hipMalloc((void **)&ix->phase_trace, 128 * sizeof(unsigned long long))) != hipSuccess ||
            (e = hipMemset(ix->phase_trace, 0, 128 * sizeof(unsigned long long))) != hipSuccess)
            return fail(CRAG_ENOMEM, "hipMalloc for the phase trace failed: %s", hipGetErrorString(e));
    }
    return CRAG_OK;
}

// what the two crag_merge_topk* calls check alike
int check_merge_args(bool any_null, int n_lists, int nq, int k) {
    if (any_null) return fail(CRAG_EINVAL, "NULL pointer argument");
    if (n_lists <= 0 || nq < 0 || k <= 0 || k > CRAG_MAX_K)
        return fail(CRAG_EINVAL, "bad sizes n_lists=%d nq=%d k=%d", n_lists, nq, k);
    if ((int64_t)n_lists * k > 4096) return fail(CRAG_EINVAL, "n_lists*k must be <= 4096");
    return CRAG_OK;
}

// p: the lists and their strides; the rest of the block is filled here
int merge_lists(int device, crag::XMergeParams &p, int n_lists, int nq, int k, int64_t *d_out_ids, float *d_out_scores,
                int32_t *d_out_counts, void *stream) {
    DeviceGuard guard(device);
    if (!guard.ok) return fail(CRAG_EHIP, "hipSetDevice(%d) failed", device);
    p.out_ids = d_out_ids;
    p.out_scores = d_out_scores;
    p.out_counts = d_out_counts;
    p.n_lists = n_lists;
    p.nq = nq;
    p.k = k;
    HIP_TRY(crag::launch_merge_results(p, (hipStream_t)stream));
    return CRAG_OK;
}

}  // namespace

extern "C" {

const char *crag_last_error(void) { return g_err; }

// how every translation unit of the library reports an error (crag_host.h: fail)
void crag_set_error_(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg ? msg : ""); }

const char *crag_version(void) { return "cadence-rag_amd dense lane 0.1 (gfx950)"; }

int crag_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int crag_index_create(int device, int dim, int64_t capacity, crag_index **out) {
    if (!out) return fail(CRAG_EINVAL, "out is NULL");
    *out = nullptr;
    if (dim <= 0 || dim > CRAG_DIM) return fail(CRAG_EINVAL, "dim must be in [1, %d] (got %d)", CRAG_DIM, dim);
    if (capacity <= 0) return fail(CRAG_EINVAL, "capacity must be > 0 (got %lld)", (long long)capacity);
    int ndev = crag_device_count();
    if (ndev <= 0) return fail(CRAG_ENODEV, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(CRAG_EINVAL, "device %d out of range [0, %d)", device, ndev);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(CRAG_EHIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CRAG_ENODEV, "device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);
    crag_index *ix = new (std::nothrow) crag_index();
    if (!ix) return fail(CRAG_ENOMEM, "out of host memory");
    ix->device = device;
    ix->dim = dim;
    ix->capacity = capacity;
    ix->cap_rows = ((capacity + 31) / 32) * 32;
    ix->n_cu = prop.multiProcessorCount;
    int rc = init_index(ix);
    if (rc) {
        crag_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return CRAG_OK;
}

int crag_index_destroy(crag_index *ix) {
    if (!ix) return CRAG_OK;
    DeviceGuard guard(ix->device);
    (void)hipDeviceSynchronize();
    for (auto &t : ix->ev_pool)
        for (hipEvent_t e : {t.e0, t.e1a, t.e1, t.e2, t.e3}) (void)hipEventDestroy(e);
    for (int i = 0; i < crag_index::MAX_PIPE; ++i) {
        if (ix->pipe_fork[i]) (void)hipEventDestroy(ix->pipe_fork[i]);
        if (ix->pipe_done[i]) (void)hipEventDestroy(ix->pipe_done[i]);
        if (ix->pipe[i]) (void)hipStreamDestroy(ix->pipe[i]);
    }
    for (void *p : {(void *)ix->irregular_dev, (void *)ix->phase_trace, (void *)ix->pf_stats, (void *)ix->corpus,
                    (void *)ix->corpus16, (void *)ix->inv_norm, (void *)ix->ids})
        if (p) (void)hipFree(p);
    for (auto &w : ix->ws) {
        for (auto &b : w.buf) b.release();
        if (w.done) (void)hipEventDestroy(w.done);
    }
    for (DevBuf *b : {&ix->stage_q, &ix->stage_rows, &ix->stage_ids, &ix->stage_mask, &ix->stage_out, &ix->scratch,
                      &ix->edit_bounce, &ix->edit_srcpos, &ix->edit_mask, &ix->edit_prefix, &ix->edit_newpos})
        b->release();
    delete ix;
    return CRAG_OK;
}

int64_t crag_index_size(const crag_index *ix) { return ix ? ix->size : -1; }
int64_t crag_index_capacity(const crag_index *ix) { return ix ? ix->capacity : -1; }
int crag_index_dim(const crag_index *ix) { return ix ? ix->dim : -1; }

int crag_merge_topk(int device, const int64_t *d_ids, const float *d_scores, const int32_t *d_counts,
                    int n_lists, int nq, int k, int64_t *d_out_ids, float *d_out_scores,
                    int32_t *d_out_counts, void *stream) {
    int rc = check_merge_args(!d_ids || !d_scores || !d_counts || !d_out_ids || !d_out_scores || !d_out_counts, n_lists,
                              nq, k);
    if (rc || nq == 0) return rc;
    crag::XMergeParams p;
    p.ids = d_ids;
    p.scores = d_scores;
    p.counts = d_counts;
    p.stride_ids = (int64_t)nq * k;
    p.stride_scores = (int64_t)nq * k;
    p.stride_counts = nq;
    return merge_lists(device, p, n_lists, nq, k, d_out_ids, d_out_scores, d_out_counts, stream);
}

int64_t crag_result_record_bytes(int nq, int k) {
    if (nq < 0 || k <= 0) return -1;
    const int64_t b = (int64_t)nq * k * 8 + (int64_t)nq * k * 4 + (int64_t)nq * 4;
    return (b + 7) & ~(int64_t)7;
}

int crag_merge_topk_packed(int device, const void *d_records, int n_lists, int nq, int k, int64_t *d_out_ids,
                           float *d_out_scores, int32_t *d_out_counts, void *stream) {
    int rc = check_merge_args(!d_records || !d_out_ids || !d_out_scores || !d_out_counts, n_lists, nq, k);
    if (rc || nq == 0) return rc;
    const int64_t rec = crag_result_record_bytes(nq, k);
    const char *base = (const char *)d_records;
    crag::XMergeParams p;
    p.ids = (const int64_t *)base;
    p.scores = (const float *)(base + (int64_t)nq * k * 8);
    p.counts = (const int32_t *)(base + (int64_t)nq * k * 12);
    p.stride_ids = rec / 8;
    p.stride_scores = rec / 4;
    p.stride_counts = rec / 4;
    return merge_lists(device, p, n_lists, nq, k, d_out_ids, d_out_scores, d_out_counts, stream);
}

int crag_index_profile_enable(crag_index *ix, int enabled) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->profiling = enabled > 0 ? enabled : 0;
    ix->prof_calls = 0;
    ix->ev_used = 0;
    return CRAG_OK;
}

int crag_index_profile_read_ex(crag_index *ix, int64_t *n_launches, double *scan_ms_total,
                               double *merge_ms_total, double *event_pair_ms_total) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    double scan = 0.0, merge = 0.0, pair = 0.0;
    for (size_t i = 0; i < ix->ev_used; ++i) {
        float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
        HIP_TRY(hipEventSynchronize(ix->ev_pool[i].e3));
        HIP_TRY(hipEventElapsedTime(&a, ix->ev_pool[i].e0, ix->ev_pool[i].e1a));
        HIP_TRY(hipEventElapsedTime(&d, ix->ev_pool[i].e1a, ix->ev_pool[i].e1));
        HIP_TRY(hipEventElapsedTime(&b, ix->ev_pool[i].e1, ix->ev_pool[i].e2));
        HIP_TRY(hipEventElapsedTime(&c, ix->ev_pool[i].e2, ix->ev_pool[i].e3));
        scan += b;
        merge += a + c;
        pair += d;
    }
    if (n_launches) *n_launches = (int64_t)ix->ev_used;
    if (scan_ms_total) *scan_ms_total = scan;
    if (merge_ms_total) *merge_ms_total = merge;
    if (event_pair_ms_total) *event_pair_ms_total = pair;
    ix->ev_used = 0;
    return CRAG_OK;
}

int crag_index_profile_read(crag_index *ix, int64_t *n_launches, double *scan_ms_total,
                            double *merge_ms_total) {
    return crag_index_profile_read_ex(ix, n_launches, scan_ms_total, merge_ms_total, nullptr);
}

int crag_index_prefilter_stats(crag_index *ix, int64_t *searches, int64_t *candidates, int64_t *rescored_rows) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    unsigned long long v[3] = {0, 0, 0};
    std::vector<unsigned long long> rec((size_t)crag::PF_STAT_SLOTS * 3);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(rec.data(), ix->pf_stats, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(ix->pf_stats, 0, rec.size() * sizeof(unsigned long long)));
    for (size_t i = 0; i < rec.size(); ++i) v[i % 3] += rec[i];
    if (candidates) *candidates = (int64_t)v[0];
    if (rescored_rows) *rescored_rows = (int64_t)v[1];
    if (searches) *searches = (int64_t)v[2];
    return CRAG_OK;
}

int crag_index_phase_trace(crag_index *ix, uint64_t *out128) {
    if (!ix || !out128) return fail(CRAG_EINVAL, "index / out is NULL");
    if (!ix->phase_trace) return fail(CRAG_EINVAL, "the index was not created with CRAG_PHASE_TRACE=1");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out128, ix->phase_trace, 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return CRAG_OK;
}

const char *crag_index_last_scan_kernel(const crag_index *ix) { return ix ? ix->last_scan_kernel : ""; }
const char *crag_index_scan_waits(const crag_index *ix) { return ix ? ix->last_scan_waits : ""; }

int64_t crag_index_prefilter_row_bytes(const crag_index *ix) {
    if (!ix || ix->sw.no_prefilter) return 0;
    return (int64_t)crag::DIM * (ix->corpus16 ? 2 : 4);
}

int crag_index_scan_geometry(const crag_index *ix, int nq, int *workgroups, int *threads,
                             int *query_blocks, int64_t *algorithmic_bytes_per_launch) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    const int qb = (nq + 31) / 32;
    if (workgroups) *workgroups = plan_search(ix->size, ix->n_cu, nq, 1, false, false, ix->sw).G;
    if (threads) *threads = crag::SCAN_THREADS;
    if (query_blocks) *query_blocks = qb;
    // N*D*4 (corpus streamed once per query batch) + Q*D*4.  A batch of more than
    // 32 queries re-streams the corpus once per 32-query block; that is NOT counted here.
    if (algorithmic_bytes_per_launch)
        *algorithmic_bytes_per_launch = ix->size * (int64_t)ix->dim * 4 + (int64_t)nq * ix->dim * 4;
    return CRAG_OK;
}

}  // extern "C"
