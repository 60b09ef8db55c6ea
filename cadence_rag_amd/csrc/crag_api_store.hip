// crag_api_store.hip — row storage of the C ABI: add, update, read back, count, and the in-place edits (kernels:
// crag_search.hip for the stores, crag_edit.hip for the moves).  Everything here runs on the default stream and
// returns with its work done.  No exceptions cross the ABI.

#include "crag_index.h"

int stage_row_masks(crag_index *ix, const uint8_t *row_mask, int64_t mask_stride, int nq, const uint8_t **d_mask,
                    int64_t *d_stride) {
    *d_mask = row_mask;
    *d_stride = mask_stride;
    if (!row_mask || is_device_ptr(row_mask)) return CRAG_OK;
    const size_t row_b = (size_t)((ix->size + 31) / 32) * 4;
    const int nmask = mask_stride ? nq : 1;
    int rc = ix->stage_mask.ensure(row_b * nmask);
    if (rc) return rc;
    HIP_TRY(hipMemset(ix->stage_mask.p, 0, row_b * nmask));
    // the caller's buffer may end at ceil(size/8) bytes: copy only that much
    const size_t have = (size_t)((ix->size + 7) / 8);
    if (mask_stride == 0) {
        HIP_TRY(hipMemcpy(ix->stage_mask.p, row_mask, have, hipMemcpyHostToDevice));
    } else {
        HIP_TRY(hipMemcpy2D(ix->stage_mask.p, row_b, row_mask, (size_t)mask_stride, have, nq, hipMemcpyHostToDevice));
        *d_stride = (int64_t)row_b;
    }
    *d_mask = (const uint8_t *)ix->stage_mask.p;
    return CRAG_OK;
}

namespace {

constexpr int64_t UPLOAD_CHUNK = 65536;   // rows per staged chunk: host staging stays bounded (256 MiB at dim 1024)

int read_irregular(crag_index *ix) {
    uint32_t flag = 0;
    HIP_TRY(hipMemcpy(&flag, ix->irregular_dev, sizeof(flag), hipMemcpyDeviceToHost));
    ix->irregular = flag != 0;
    return CRAG_OK;
}

// the irregular flag from the rows that are stored now (irregular_flag_kernel: store_row's own condition)
int recompute_irregular(crag_index *ix) {
    HIP_TRY(hipMemsetAsync(ix->irregular_dev, 0, sizeof(uint32_t), 0));
    HIP_TRY(crag::launch_irregular_flag(ix->inv_norm, ix->size, ix->irregular_dev, 0));
    return read_irregular(ix);
}

// rows [0, n) of the caller's host or device table, chunk by chunk: store(device rows, offset, count) enqueues a chunk
template <class Store> int upload_rows(crag_index *ix, const float *rows, int64_t n, Store store) {
    for (int64_t o = 0; o < n; o += UPLOAD_CHUNK) {
        const int64_t m = (n - o < UPLOAD_CHUNK) ? (n - o) : UPLOAD_CHUNK;
        const float *src = rows + (size_t)o * ix->dim;
        const float *d = nullptr;
        int rc = stage_in(ix->stage_rows, src, (size_t)m * ix->dim * sizeof(float), &d);
        if (rc) return rc;
        HIP_TRY(store(d, o, m));
        if (d != src) HIP_TRY(hipStreamSynchronize(0));  // staging buffer is reused by the next chunk
    }
    HIP_TRY(hipStreamSynchronize(0));
    return CRAG_OK;
}

int store_rows_locked(crag_index *ix, int64_t pos, const float *rows, int64_t n) {
    int rc = upload_rows(ix, rows, n, [&](const float *src, int64_t o, int64_t m) {
        return crag::launch_store_rows(src, ix->dim, pos + o, m, ix->corpus, ix->inv_norm, ix->irregular_dev, ix->corpus16, 0);
    });
    if (rc) return rc;
    // the store kernel can only raise the flag.  Set, it stays right while rows are appended; whoever may have taken
    // an irregular row away (crag_index_update, the edits) recomputes it over the stored rows (recompute_irregular)
    return ix->irregular ? CRAG_OK : read_irregular(ix);
}

int check_room(const crag_index *ix, int64_t n) {
    if (ix->size + n > ix->capacity)
        return fail(CRAG_ENOMEM, "capacity exceeded: size %lld + %lld > %lld", (long long)ix->size,
                    (long long)n, (long long)ix->capacity);
    if (ix->size + n >= (int64_t)0xfffffff0ll) return fail(CRAG_ENOMEM, "more than 2^32 rows per index");
    return CRAG_OK;
}

// ---- in-place edits (kernels: crag_edit.hip) ----

crag::RowStore index_rows(crag_index *ix) { return crag::RowStore{ix->corpus, ix->corpus16, ix->inv_norm, ix->ids}; }

// the bounce buffer as a RowStore of `rows` (a multiple of 32) rows, and room for as many source positions
int bounce_rows(crag_index *ix, int64_t rows, crag::RowStore *out) {
    const size_t b32 = (size_t)rows * crag::DIM * sizeof(float), b16 = ix->corpus16 ? (size_t)rows * crag::DIM * 2 : 0,
                 binv = (size_t)rows * sizeof(float), bid = (size_t)rows * sizeof(int64_t);
    int rc = ix->edit_bounce.ensure(b32 + b16 + bid + binv);
    if (!rc) rc = ix->edit_srcpos.ensure((size_t)rows * sizeof(int64_t));
    if (rc) return rc;
    char *p = (char *)ix->edit_bounce.p;
    out->corpus = (float *)p;
    out->mirror = ix->corpus16 ? (_Float16 *)(p + b32) : nullptr;
    out->ids = (int64_t *)(p + b32 + b16);
    out->inv_norm = (float *)(p + b32 + b16 + bid);
    return CRAG_OK;
}

int64_t edit_chunk(const crag_index *ix, int64_t moved) {
    const int64_t want = ((moved + 31) / 32) * 32;
    return want < ix->edit_chunk_rows ? want : ix->edit_chunk_rows;
}

// after an edit: last_id from the last stored row, the irregular flag from the rows that are left
int refresh_after_edit(crag_index *ix) {
    ix->last_id = INT64_MIN;
    if (ix->size > 0)
        HIP_TRY(hipMemcpy(&ix->last_id, ix->ids + (ix->size - 1), sizeof(int64_t), hipMemcpyDeviceToHost));
    int rc = recompute_irregular(ix);
    ix->edit_bounce.release();
    return rc;
}

// keep: one bit per stored row (bits beyond size already cleared), a cleared bit drops the row
int compact_locked(crag_index *ix, const std::vector<uint32_t> &keep) {
    const int64_t n = ix->size, nw = (n + 31) / 32;
    std::vector<uint32_t> prefix((size_t)nw + 1);
    int64_t first = -1, total = 0;
    for (int64_t w = 0; w < nw; ++w) {
        prefix[w] = (uint32_t)total;
        const uint32_t gone = ~keep[w] & (w == nw - 1 ? tail_mask(n) : 0xffffffffu);
        if (first < 0 && gone) first = w * 32 + __builtin_ctz(gone);
        total += __builtin_popcount(keep[w]);
    }
    prefix[nw] = (uint32_t)total;
    const int64_t new_size = total;
    if (new_size == n) return CRAG_OK;
    const crag::RowStore index = index_rows(ix);
    crag::RowStore bounce{};
    const int64_t C = edit_chunk(ix, new_size - first);
    int rc;
    if (new_size > first) {   // every allocation in front of the first move
        if ((rc = bounce_rows(ix, C, &bounce))) return rc;
        if ((rc = ix->edit_mask.ensure((size_t)nw * 4))) return rc;
        if ((rc = ix->edit_prefix.ensure(((size_t)nw + 1) * 4))) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());   // every search in flight on this index, whichever stream it runs on
    if (new_size > first) {
        HIP_TRY(hipMemcpy(ix->edit_mask.p, keep.data(), (size_t)nw * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ix->edit_prefix.p, prefix.data(), ((size_t)nw + 1) * 4, hipMemcpyHostToDevice));
        int64_t *srcpos = (int64_t *)ix->edit_srcpos.p;
        for (int64_t d0 = first; d0 < new_size; d0 += C) {   // rows move down: ascending chunks
            const int64_t m = new_size - d0 < C ? new_size - d0 : C;
            HIP_TRY(crag::launch_remove_srcpos((const uint32_t *)ix->edit_mask.p, (const uint32_t *)ix->edit_prefix.p, nw, d0, m,
                                               srcpos, 0));
            HIP_TRY(crag::launch_move_rows(index, bounce, srcpos, d0, m, 0));
        }
    }
    HIP_TRY(crag::launch_clear_rows(index, new_size, n - new_size, 0));
    HIP_TRY(hipStreamSynchronize(0));
    ix->size = new_size;
    return refresh_after_edit(ix);
}

}  // namespace

extern "C" {

int crag_index_add(crag_index *ix, const float *rows, const int64_t *ids, int64_t n) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (n < 0) return fail(CRAG_EINVAL, "n must be >= 0");
    if (n == 0) return CRAG_OK;
    if (!rows) return fail(CRAG_EINVAL, "rows is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    int rc = check_room(ix, n);
    if (rc) return rc;
    DeviceGuard guard(ix->device);
    const int64_t pos = ix->size;
    // ids must grow with the row position: that is what makes "equal scores by ascending position" inside
    // the scan the same order as "equal scores by ascending id"  and as the cross-shard merge
    int64_t new_last;
    if (!ids) {
        if (pos <= ix->last_id)
            return fail(CRAG_EINVAL, "implicit ids would start at %lld, not above the largest stored id %lld",
                        (long long)pos, (long long)ix->last_id);
        new_last = pos + n - 1;
    } else if (is_device_ptr(ids)) {
        if ((rc = ix->scratch.ensure(sizeof(unsigned long long)))) return rc;
        HIP_TRY(hipMemsetAsync(ix->scratch.p, 0, sizeof(unsigned long long), 0));
        HIP_TRY(crag::launch_check_ids(ids, n, ix->last_id, (unsigned long long *)ix->scratch.p, 0));
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, ix->scratch.p, sizeof(bad), hipMemcpyDeviceToHost));
        if (bad)
            return fail(CRAG_EINVAL, "ids must be strictly ascending and above the largest stored id %lld "
                        "(%llu of %lld are not)", (long long)ix->last_id, bad, (long long)n);
        HIP_TRY(hipMemcpy(&new_last, ids + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost));
    } else {
        int64_t prev = ix->last_id;
        for (int64_t i = 0; i < n; ++i) {
            if (ids[i] <= prev)
                return fail(CRAG_EINVAL, "ids must be strictly ascending and above the largest stored id: "
                            "ids[%lld] = %lld follows %lld", (long long)i, (long long)ids[i], (long long)prev);
            prev = ids[i];
        }
        new_last = prev;
    }
    if ((rc = store_rows_locked(ix, pos, rows, n))) return rc;
    if (ids) {
        HIP_TRY(hipMemcpy(ix->ids + pos, ids, (size_t)n * sizeof(int64_t),
                          is_device_ptr(ids) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    } else {
        HIP_TRY(crag::launch_fill_ids(ix->ids, pos, n, pos, 0));
        HIP_TRY(hipStreamSynchronize(0));
    }
    ix->size = pos + n;
    ix->last_id = new_last;
    return CRAG_OK;
}

int crag_index_update(crag_index *ix, int64_t pos, const float *rows, int64_t n) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (n < 0 || pos < 0) return fail(CRAG_EINVAL, "pos and n must be >= 0");
    if (n == 0) return CRAG_OK;
    if (!rows) return fail(CRAG_EINVAL, "rows is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (pos + n > ix->size)
        return fail(CRAG_EINVAL, "update range [%lld, %lld) exceeds size %lld", (long long)pos,
                    (long long)(pos + n), (long long)ix->size);
    DeviceGuard guard(ix->device);
    const bool was_irregular = ix->irregular;
    int rc = store_rows_locked(ix, pos, rows, n);
    if (rc) return rc;
    // the overwritten rows may have been the irregular ones: as after an edit, the flag follows the rows stored now.
    // (A clear flag needs nothing more: the store kernel has raised it if a new row is irregular.)
    return was_irregular ? recompute_irregular(ix) : CRAG_OK;
}

int crag_index_remove(crag_index *ix, const int64_t *ids, int64_t n, int64_t *out_removed) {
    if (out_removed) *out_removed = 0;
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (n < 0) return fail(CRAG_EINVAL, "n must be >= 0");
    if (n == 0) return CRAG_OK;
    if (!ids) return fail(CRAG_EINVAL, "ids is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->size == 0) return CRAG_OK;
    DeviceGuard guard(ix->device);
    const int64_t *d_ids = nullptr;
    int rc;
    if ((rc = stage_in(ix->stage_ids, ids, (size_t)n * sizeof(int64_t), &d_ids))) return rc;
    const int64_t nw = (ix->size + 31) / 32;
    if ((rc = ix->edit_mask.ensure((size_t)nw * 4))) return rc;
    HIP_TRY(hipMemsetAsync(ix->edit_mask.p, 0, (size_t)nw * 4, 0));
    HIP_TRY(crag::launch_lookup_ids(ix->ids, ix->size, d_ids, n, nullptr, 0, (uint32_t *)ix->edit_mask.p, nullptr, 0));
    std::vector<uint32_t> keep((size_t)nw);
    HIP_TRY(hipMemcpy(keep.data(), ix->edit_mask.p, (size_t)nw * 4, hipMemcpyDeviceToHost));
    int64_t removed = 0;
    for (int64_t w = 0; w < nw; ++w) {   // (the lookup marks stored positions only: no bit beyond size)
        removed += __builtin_popcount(keep[w]);
        keep[w] = ~keep[w] & (w == nw - 1 ? tail_mask(ix->size) : 0xffffffffu);
    }
    if (removed == 0) return CRAG_OK;
    if ((rc = compact_locked(ix, keep))) return rc;
    if (out_removed) *out_removed = removed;
    return CRAG_OK;
}

int crag_index_compact(crag_index *ix, const uint8_t *keep_mask, int64_t *out_size) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (!keep_mask) return fail(CRAG_EINVAL, "keep_mask is NULL");
    if (((uintptr_t)keep_mask) & 3) return fail(CRAG_EINVAL, "keep_mask must be 4-byte aligned");
    if (is_device_ptr(keep_mask)) return fail(CRAG_EINVAL, "keep_mask must be a host pointer");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    const int64_t nw = (ix->size + 31) / 32;
    std::vector<uint32_t> keep((size_t)nw);
    if (nw) {
        memcpy(keep.data(), keep_mask, (size_t)nw * 4);
        keep[nw - 1] &= tail_mask(ix->size);
        int rc = compact_locked(ix, keep);
        if (rc) return rc;
    }
    if (out_size) *out_size = ix->size;
    return CRAG_OK;
}

int crag_index_insert(crag_index *ix, const float *rows, const int64_t *ids, int64_t n) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (n < 0) return fail(CRAG_EINVAL, "n must be >= 0");
    if (n == 0) return CRAG_OK;
    if (!rows) return fail(CRAG_EINVAL, "rows is NULL");
    if (!ids) return fail(CRAG_EINVAL, "ids is NULL (an insertion needs explicit ids)");
    std::unique_lock<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    std::vector<int64_t> h_ids;
    if (is_device_ptr(ids)) {
        h_ids.resize((size_t)n);
        HIP_TRY(hipMemcpy(h_ids.data(), ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    const int64_t *hid = h_ids.empty() ? ids : h_ids.data();
    for (int64_t i = 1; i < n; ++i)
        if (hid[i] <= hid[i - 1])
            return fail(CRAG_EINVAL, "ids must be strictly ascending: ids[%lld] = %lld follows %lld", (long long)i,
                        (long long)hid[i], (long long)hid[i - 1]);
    if (hid[0] > ix->last_id) {   // nothing stored lies behind the new rows: exactly the crag_index_add route
        lk.unlock();
        return crag_index_add(ix, rows, ids, n);
    }
    int rc;
    if ((rc = check_room(ix, n))) return rc;
    const int64_t *d_ids = nullptr;
    if ((rc = stage_in(ix->stage_ids, ids, (size_t)n * sizeof(int64_t), &d_ids))) return rc;
    // where each new row lands (stored ids below it + new ids below it), and that none of them is stored already
    if ((rc = ix->edit_newpos.ensure((size_t)n * sizeof(int64_t)))) return rc;
    if ((rc = ix->scratch.ensure(sizeof(unsigned long long)))) return rc;
    int64_t *newpos = (int64_t *)ix->edit_newpos.p;
    HIP_TRY(hipMemsetAsync(ix->scratch.p, 0, sizeof(unsigned long long), 0));
    HIP_TRY(crag::launch_lookup_ids(ix->ids, ix->size, d_ids, n, newpos, 1, nullptr, (unsigned long long *)ix->scratch.p, 0));
    unsigned long long dup = 0;
    HIP_TRY(hipMemcpy(&dup, ix->scratch.p, sizeof(dup), hipMemcpyDeviceToHost));
    if (dup) return fail(CRAG_EINVAL, "%llu of the %lld ids are stored already (crag_index_update re-embeds in place)", dup,
                         (long long)n);
    int64_t first = 0;
    HIP_TRY(hipMemcpy(&first, newpos, sizeof(first), hipMemcpyDeviceToHost));
    const int64_t new_size = ix->size + n;
    const crag::RowStore index = index_rows(ix);
    crag::RowStore bounce{};
    const int64_t C = edit_chunk(ix, new_size - first);
    if ((rc = bounce_rows(ix, C, &bounce))) return rc;
    // (every allocation in front of the first move: the upload then finds its staging buffer large enough)
    if (!is_device_ptr(rows) &&
        (rc = ix->stage_rows.ensure((size_t)(n < UPLOAD_CHUNK ? n : UPLOAD_CHUNK) * ix->dim * sizeof(float))))
        return rc;
    HIP_TRY(hipDeviceSynchronize());   // every search in flight on this index, whichever stream it runs on
    int64_t *srcpos = (int64_t *)ix->edit_srcpos.p;
    for (int64_t hi = new_size; hi > first; hi -= C) {   // rows move up: descending chunks
        const int64_t d0 = hi - C > first ? hi - C : first;
        HIP_TRY(crag::launch_insert_srcpos(newpos, n, d0, hi - d0, srcpos, 0));
        HIP_TRY(crag::launch_move_rows(index, bounce, srcpos, d0, hi - d0, 0));
    }
    rc = upload_rows(ix, rows, n, [&](const float *src, int64_t o, int64_t m) {
        return crag::launch_store_rows_at(src, ix->dim, newpos + o, d_ids + o, m, index, ix->irregular_dev, 0);
    });
    if (rc) return rc;
    ix->size = new_size;
    return refresh_after_edit(ix);
}

int crag_index_get_rows(crag_index *ix, int64_t pos, int64_t n, float *rows, int64_t *ids) {
    if (!ix) return fail(CRAG_EINVAL, "index is NULL");
    if (n < 0 || pos < 0) return fail(CRAG_EINVAL, "pos and n must be >= 0");
    if (n == 0) return CRAG_OK;
    if (!rows) return fail(CRAG_EINVAL, "rows is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    if (pos + n > ix->size)
        return fail(CRAG_EINVAL, "range [%lld, %lld) exceeds size %lld", (long long)pos,
                    (long long)(pos + n), (long long)ix->size);
    DeviceGuard guard(ix->device);
    const bool dev = is_device_ptr(rows);
    for (int64_t o = 0; o < n; o += UPLOAD_CHUNK) {
        const int64_t m = (n - o < UPLOAD_CHUNK) ? (n - o) : UPLOAD_CHUNK;
        float *dst = rows + (size_t)o * ix->dim;
        float *ddst = dst;
        if (!dev) {
            int rc = ix->stage_rows.ensure((size_t)m * ix->dim * sizeof(float));
            if (rc) return rc;
            ddst = (float *)ix->stage_rows.p;
        }
        HIP_TRY(crag::launch_load_rows(ix->corpus, ix->dim, pos + o, m, ddst, crag::crag_piece_shift(ix->corpus16 != nullptr), 0));
        if (!dev)
            HIP_TRY(hipMemcpy(dst, ddst, (size_t)m * ix->dim * sizeof(float), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipStreamSynchronize(0));
    if (ids)
        HIP_TRY(hipMemcpy(ids, ix->ids + pos, (size_t)n * sizeof(int64_t),
                          is_device_ptr(ids) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return CRAG_OK;
}

int crag_index_count_eligible(crag_index *ix, const uint8_t *row_mask, int64_t *out_count) {
    if (!ix || !out_count) return fail(CRAG_EINVAL, "index / out_count is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    DeviceGuard guard(ix->device);
    *out_count = 0;
    if (ix->size == 0) return CRAG_OK;
    if (((uintptr_t)row_mask) & 3) return fail(CRAG_EINVAL, "row_mask must be 4-byte aligned");
    const uint8_t *dmask = nullptr;
    int64_t dstride = 0;
    int rc = stage_row_masks(ix, row_mask, 0, 1, &dmask, &dstride);
    if (rc) return rc;
    if ((rc = ix->scratch.ensure(sizeof(unsigned long long)))) return rc;
    HIP_TRY(hipMemset(ix->scratch.p, 0, sizeof(unsigned long long)));
    HIP_TRY(crag::launch_count_eligible(ix->inv_norm, ix->size, (const uint32_t *)dmask, (unsigned long long *)ix->scratch.p, 0));
    unsigned long long c = 0;
    HIP_TRY(hipMemcpy(&c, ix->scratch.p, sizeof(c), hipMemcpyDeviceToHost));
    *out_count = (int64_t)c;
    return CRAG_OK;
}

}  // extern "C"
