// crag_index.h — the index behind the opaque crag_index of include/crag_dense.h, shared by the host units of the C ABI:
// crag_api.hip (life cycle, introspection, profiling), crag_api_search.hip, crag_api_store.hip (rows and edits).
#pragma once
#include <mutex>
#include <vector>

#include "crag_host.h"
#include "crag_kernels.h"
#include "crag_search_plan.h"

#pragma GCC visibility push(hidden)   // internal types and helpers: nothing of them is exported

// A host row mask (one shared, or nq of them mask_stride bytes apart) in stage_mask, each padded with zeros to whole
// words; a device mask as it is.  (crag_api_store.hip)
int stage_row_masks(struct crag_index *ix, const uint8_t *row_mask, int64_t mask_stride, int nq, const uint8_t **d_mask,
                    int64_t *d_stride);

struct EvSet {  // around one profiled search: start, before / after the scan kernel, end
    hipEvent_t e0, e1a, e1, e2, e3;  // e1a, e1: recorded back to back (what an event pair measures with nothing between)
};

// One search's scratch.  Search workspaces are per stream (up to MAX_WS streams): searches enqueued on different
// streams may overlap on the GPU, same-stream searches are ordered by the stream itself.
struct Workspace {
    enum Buf {
        PARTIAL, GBOUND,
        // prepared queries (fragment order) and the prefilter path's per-query state
        A32, A16, QINV, PF_CAND, PF_XKEYS, PF_XIDS, PF_XCOUNT,
        // the per-query state the selection kernel leaves zeroed (class maxima, candidate counts, flags, tickets)
        PF_GBOUND, PF_COUNT, PF_FLAGS, PF_XTICKET,
        N_BUF,
        KEPT_ZERO_FIRST = PF_GBOUND, KEPT_ZERO_END = N_BUF
    };
    DevBuf buf[N_BUF];   // allocated on the workspace's first search that needs them
    template <class T> T *at(Buf b) const { return (T *)buf[b].p; }
    hipStream_t stream = nullptr;
    bool in_use = false;
    hipEvent_t done = nullptr;   // created with the index, recorded after every search that used this workspace
    uint32_t seq = 0;            // sequence number of the last prefilter search on this workspace (never 0 in use)
    bool done_recorded = false;  // ... once every workspace has an owner (until then nobody can take one over)
    // a search failed between its scan launch and its selection launch: the KEPT_ZERO buffers may hold the failed
    // search's values -- the next search on this workspace re-zeroes them first
    bool dirty = false;
    uint64_t last_use = 0;
};

#pragma GCC visibility pop

struct crag_index {
    int device = 0;
    int dim = 0;
    int64_t capacity = 0;   // rows requested
    int64_t cap_rows = 0;   // padded to a multiple of 32
    int64_t size = 0;
    int n_cu = 0;
    float *corpus = nullptr;
    _Float16 *corpus16 = nullptr;  // fp16 mirror of the unit rows for the prefilter scan (CRAG_NO_FP16_MIRROR=1: none)
    float *inv_norm = nullptr;
    int64_t *ids = nullptr;
    static constexpr int MAX_WS = 8;   // (= crag::PF_STAT_WS)
    Workspace ws[MAX_WS];
    // crag_index_search_pipelined: streams of the index's own, used in turn (3 by default; CRAG_PIPE_STREAMS=1..4)
    static constexpr int MAX_PIPE = 4;
    int n_pipe = 3;
    hipStream_t pipe[MAX_PIPE] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t pipe_fork[MAX_PIPE] = {nullptr, nullptr, nullptr, nullptr}, pipe_done[MAX_PIPE] = {nullptr, nullptr, nullptr, nullptr};
    bool pipe_pending[MAX_PIPE] = {false, false, false, false};
    unsigned pipe_next = 0;
    uint64_t use_clock = 0;
    bool record_done = false;   // every workspace has an owner: from now on a search records its workspace's event
    int64_t last_id = INT64_MIN;  // largest id stored so far (ids are strictly ascending with the row position)
    // developer switches, read from the environment once, when the index is created
    SearchSwitches sw;
    bool env_no_reverse = false, env_unpipelined = false;
    // a stored row whose norm lies outside [1e-30, 1e30]: the fp16 prefilter's error bound assumes normalised
    // rows in fp32's comfortable range, so such an index always takes the plain fp32 scan
    bool irregular = false;
    uint32_t *irregular_dev = nullptr;
    unsigned long long *pf_stats = nullptr;  // device: PF_STAT_SLOTS x {candidates, rescored rows, searches}
    unsigned long long *phase_trace = nullptr;  // device, 128 words; only with CRAG_PHASE_TRACE=1 (developer probe)
    const char *last_scan_kernel = "";  // name of the scan kernel the most recent search launched
    const char *last_scan_waits = "";   // wait schedule of that scan's corpus loads: "tile" or "fragment"
    DevBuf stage_q, stage_rows, stage_ids, stage_mask, stage_out, scratch;
    // in-place edits (crag_index_remove / compact / insert): destination rows per chunk (CRAG_EDIT_CHUNK_ROWS; the default
    // keeps the bounce buffer, 6 156 bytes per row, below 128 MiB), the bounce buffer (held only during an edit), the
    // chunk's source positions, the keep mask + its popcount prefix, the new rows' positions
    int64_t edit_chunk_rows = 16384;
    DevBuf edit_bounce, edit_srcpos, edit_mask, edit_prefix, edit_newpos;
    std::mutex mu;
    int pass_parity = 0;  // alternate scan direction between searches (Infinity Cache reuse)
    int64_t env_fail_after_scan = 0;  // CRAG_TEST_FAIL_AFTER_SCAN=n (tests): the n-th prefilter search returns CRAG_EHIP
    int64_t pf_searches = 0;          // between its scan launch and its selection launch
    int profiling = 0;      // 0 = off, N = record HIP events around every N-th search
    int64_t prof_calls = 0;
    std::vector<EvSet> ev_pool;
    size_t ev_used = 0;
};

static_assert(crag_index::MAX_WS == crag::PF_STAT_WS, "one block of statistics records per workspace");

// the stored rows as the kernels of the list operators see them (crag_rows.h)
inline crag::RowView row_view(const crag_index *ix) {
    return {ix->corpus, ix->inv_norm, ix->ids, ix->size, crag::crag_piece_shift(ix->corpus16 != nullptr)};
}
