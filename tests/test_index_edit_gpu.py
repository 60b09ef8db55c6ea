"""In-place index edits (crag_edit.hip; crag_index_remove / compact / insert) against the contract of DESIGN.md 4.8:
after any edit the index is indistinguishable from a SECOND INDEX BUILT FRESH, with add, from the rows and ids
tests/index_edit_oracle.py says are left -- size, ids, get_rows, every search (ids, score bits, counts), the scan
kernel chosen and count_eligible.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest

from tests import index_edit_oracle as ox
from tests.helpers import unit_rows
from tests.index_compare import MODES, _assert_same, _bits, _build, _env

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def small():
    """300 rows x 1024 with gaps between the ids (absent ids exist everywhere), 4 queries; never modified."""
    rng = np.random.default_rng(4801)
    rows = rng.standard_normal((N, 1024)).astype(np.float32) * rng.uniform(0.2, 5.0, (N, 1)).astype(np.float32)
    ids = 1000 + 3 * np.arange(N, dtype=np.int64)
    queries = rng.standard_normal((4, 1024)).astype(np.float32)
    for a in (rows, ids, queries):
        a.setflags(write=False)
    return rows, ids, queries


@pytest.fixture(scope="module")
def big():
    """40 000 unit rows x 1024 (the prefilter path), ids with gaps, 8 queries, + 1 000 more rows to insert."""
    rng = np.random.default_rng(4802)
    rows = unit_rows(rng, 41_000)
    ids = 2 * np.arange(40_000, dtype=np.int64)
    queries = rng.standard_normal((8, 1024)).astype(np.float32)
    for a in (rows, ids, queries):
        a.setflags(write=False)
    return rows[:40_000], ids, queries, rows[40_000:]


def _remove_cases(ids):
    return {
        "first": ids[:1],
        "last": ids[-1:],
        "tile": ids[32:64],
        "every_second": ids[::2],
        "all_but_one": np.delete(ids, 137),
        "all": ids,
        "none": np.array([1, 1001, 1002, 5000], dtype=np.int64),
        "repeats_and_absent": np.array([ids[5], 7, ids[5], ids[290], 1001, ids[64], ids[290], ids[63]], dtype=np.int64),
        "single_beyond_256": ids[270:271],
    }


def _run_remove(rows, ids, queries, drop, as_device=False, as_compact=False):
    want_ids, want_rows, want_removed = ox.remove(ids, rows, drop)
    edited = _build(rows, ids, capacity=len(ids))
    fresh = _build(want_rows, want_ids, capacity=len(ids))
    try:
        before = edited.get_rows(0, 256)
        if as_compact:
            assert edited.compact(np.isin(ids, want_ids)) == want_ids.size
        elif as_device:
            import torch
            assert edited.remove(torch.from_numpy(np.array(drop, dtype=np.int64)).cuda()) == want_removed
        else:
            assert edited.remove(drop) == want_removed
        _assert_same(edited, fresh, queries)
        first_gone = int(np.flatnonzero(~np.isin(ids, want_ids))[0]) if want_removed else len(ids)
        if first_gone >= 256:   # rows in front of the first change are where they were
            after = edited.get_rows(0, 256)
            assert np.array_equal(before[1], after[1]) and np.array_equal(_bits(before[0]), _bits(after[0]))
        if want_ids.size == 0:  # an emptied index takes ids from any value again
            edited.add(rows[:40], ids=np.arange(40, dtype=np.int64))
            fresh.add(rows[:40], ids=np.arange(40, dtype=np.int64))
            _assert_same(edited, fresh, queries)
    finally:
        edited.close()
        fresh.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["first", "last", "tile", "every_second", "all_but_one", "all", "none",
                                  "repeats_and_absent", "single_beyond_256"])
def test_remove_layout_edges(gpu, monkeypatch, small, case, mode):
    rows, ids, queries = small
    _env(monkeypatch, mode)
    _run_remove(rows, ids, queries, _remove_cases(ids)[case])


@pytest.mark.parametrize("mode", list(MODES))
def test_remove_ids_from_a_device_tensor_and_by_keep_mask(gpu, monkeypatch, small, mode):
    rows, ids, queries = small
    _env(monkeypatch, mode)
    drop = _remove_cases(ids)["repeats_and_absent"]
    _run_remove(rows, ids, queries, drop, as_device=True)
    _run_remove(rows, ids, queries, ids[1::3], as_compact=True)


def test_remove_at_dim_768(gpu, monkeypatch, small):
    rows, ids, queries = small
    _env(monkeypatch)
    _run_remove(np.ascontiguousarray(rows[:, :768]), ids, np.ascontiguousarray(queries[:, :768]), ids[::2])


def test_vacated_tail_is_clean(gpu, monkeypatch, small):
    """Remove 40 of 100 rows, add 40 new rows with larger ids: the positions the removal vacated are what a new
    index has there."""
    rows, ids, queries = small
    _env(monkeypatch)
    drop = ids[np.random.default_rng(5).choice(100, 40, replace=False)]
    left_ids, left_rows, _ = ox.remove(ids[:100], rows[:100], drop)
    new_ids = 5000 + np.arange(40, dtype=np.int64)
    edited = _build(rows[:100], ids[:100])
    fresh = _build(np.concatenate([left_rows, rows[200:240]]), np.concatenate([left_ids, new_ids]))
    try:
        assert edited.remove(drop) == 40
        edited.add(rows[200:240], ids=new_ids)
        _assert_same(edited, fresh, queries)
    finally:
        edited.close()
        fresh.close()


def test_special_rows_travel(gpu, monkeypatch, small):
    """A zero row, a NaN row and a pair of duplicate rows behind the removed ones: copied, not recomputed."""
    rows, ids, queries = small
    _env(monkeypatch)
    rows = rows[:100].copy()
    ids = ids[:100]
    rows[50] = 0.0
    rows[60, 17] = np.nan
    rows[80] = rows[70]
    drop = ids[0:40:2]
    want_ids, want_rows, _ = ox.remove(ids, rows, drop)
    edited, fresh = _build(rows, ids), _build(want_rows, want_ids)
    try:
        assert edited.remove(drop) == 20
        q = np.concatenate([rows[70][None], queries])
        _assert_same(edited, fresh, q, ks=(10, 128))
        got_ids, got_scores, counts = edited.search(q, 128)
        assert got_ids[0, :2].tolist() == [ids[70], ids[80]] and got_scores[0, 0] == got_scores[0, 1]
        assert np.all(counts == 78) and edited.count_eligible() == 78
        assert ids[50] not in got_ids and ids[60] not in got_ids
    finally:
        edited.close()
        fresh.close()


def test_irregular_flag_follows_the_rows_that_are_left(gpu, monkeypatch, big):
    """One row scaled by 1e-35 keeps the index on the fp32 scans; once it is removed the index returns to the
    prefilter path (default chunk size)."""
    rows, ids, queries, _ = big
    _env(monkeypatch, chunk=None)
    n = 33_000
    mine = rows[:n].copy()
    mine[12_345] *= np.float32(1e-35)
    edited = _build(mine, ids[:n])
    want_ids, want_rows, _ = ox.remove(ids[:n], mine, ids[12_345:12_346])
    fresh = _build(want_rows, want_ids, capacity=n)
    try:
        edited.search(queries, 10)
        assert "scan" in edited.last_scan_kernel() and "prefilter" not in edited.last_scan_kernel()
        assert edited.remove(ids[12_345:12_346]) == 1
        _assert_same(edited, fresh, queries)
        assert "prefilter_kernel" in edited.last_scan_kernel()
    finally:
        edited.close()
        fresh.close()


@pytest.mark.parametrize("mode", ["mirror", "no_prefilter"])
def test_prefilter_path_and_mirror_after_remove_and_insert(gpu, monkeypatch, big, mode):
    """40 000 rows, default chunk size: remove 2 000 scattered rows, then insert 1 000 rows with ids spread through the
    range; after each step everything equals the fresh index, the rescored-row count (a function of
    corpus, query, k and mask alone) included."""
    rows, ids, queries, extra = big
    _env(monkeypatch, mode, chunk=None)
    rng = np.random.default_rng(77)
    drop = ids[rng.choice(40_000, 2_000, replace=False)]
    new_ids = np.sort(rng.choice(40_000, 1_000, replace=False)).astype(np.int64) * 2 + 1
    stats = mode == "mirror"
    edited = _build(rows, ids)
    ids1, rows1, removed = ox.remove(ids, rows, drop)
    fresh = _build(rows1, ids1, capacity=40_000)
    try:
        assert edited.remove(drop) == removed == 2_000
        _assert_same(edited, fresh, queries, ks=(10, 100), stats=stats)
        if stats:
            assert "prefilter_kernel" in edited.last_scan_kernel()
        fresh.close()
        ids2, rows2 = ox.insert(ids1, rows1, new_ids, extra)
        fresh = _build(rows2, ids2, capacity=40_000)
        edited.insert(extra, new_ids)
        _assert_same(edited, fresh, queries, ks=(10, 100), stats=stats)
    finally:
        edited.close()
        fresh.close()


def _run_insert(rows, ids, queries, new_rows, new_ids, capacity, as_device=False):
    want_ids, want_rows = ox.insert(ids, rows, new_ids, new_rows)
    edited, fresh = _build(rows, ids, capacity=capacity), _build(want_rows, want_ids, capacity=capacity)
    try:
        if as_device:
            import torch
            edited.insert(torch.from_numpy(np.array(new_rows)).cuda(), torch.from_numpy(np.array(new_ids)).cuda())
        else:
            edited.insert(new_rows, new_ids)
        _assert_same(edited, fresh, queries)
        # the index accepts the same next add
        more = np.array([want_ids[-1] + 5], dtype=np.int64)
        edited.add(rows[:1], ids=more)
        fresh.add(rows[:1], ids=more)
        _assert_same(edited, fresh, queries)
    finally:
        edited.close()
        fresh.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["in_front", "between_every_pair", "tile_boundary", "above_last_id", "cuda_tensor"])
def test_insert_edges(gpu, monkeypatch, small, case, mode):
    rows, ids, queries = small
    _env(monkeypatch, mode)
    if case == "in_front":
        _run_insert(rows[:290], ids[:290], queries, rows[290:293], np.array([1, 2, 3], dtype=np.int64), 300)
    elif case == "between_every_pair":   # 150 -> 299
        _run_insert(rows[:150], ids[:150], queries, rows[150:299], ids[:149] + 1, 300)
    elif case == "tile_boundary":        # new rows land on positions 32 and 64 of a table of full tiles
        _run_insert(rows[:288], ids[:288], queries, rows[288:290], np.array([ids[31] + 1, ids[62] + 1], dtype=np.int64), 300)
    elif case == "above_last_id":        # the crag_index_add route
        _run_insert(rows[:200], ids[:200], queries, rows[200:260], ids[200:260], 300)
    else:
        _run_insert(rows[:200], ids[:200], queries, rows[200:260], ids[:60] + 2, 300, as_device=True)


def test_insert_refusals_leave_the_index_unchanged(gpu, monkeypatch, small):
    rows, ids, queries = small
    _env(monkeypatch)
    with _build(rows[:200], ids[:200], capacity=210) as ix:
        before = ix.get_rows(0, 200)
        with pytest.raises(Exception, match=r"code -1\).*stored already"):        # CRAG_EINVAL
            ix.insert(rows[200:203], np.array([ids[3] + 1, ids[7], ids[9] + 1], dtype=np.int64))
        with pytest.raises(Exception, match=r"code -3\)"):                         # CRAG_ENOMEM
            ix.insert(rows[200:211], ids[:11] + 1)
        with pytest.raises(Exception, match=r"code -1\).*strictly ascending"):
            ix.insert(rows[200:202], np.array([ids[9] + 1, ids[3] + 1], dtype=np.int64))
        after = ix.get_rows(0, 200)
        assert len(ix) == 200
        assert np.array_equal(before[1], after[1]) and np.array_equal(_bits(before[0]), _bits(after[0]))
        ix.insert(rows[200:210], ids[:10] + 1)                                    # exactly up to the capacity
        assert len(ix) == 210


def test_order_of_chunks(gpu, monkeypatch, small):
    """Chunk 64: removing row 0 of 300 shifts every row down by one across five chunks, inserting one row at position
    0 shifts every row up by one.  A wrong chunk direction or a move without the bounce buffer duplicates rows."""
    rows, ids, queries = small
    _env(monkeypatch)
    _run_remove(rows, ids, queries, ids[:1])
    # capacity 301: _run_insert adds one more row after the insert has filled all 300 positions
    _run_insert(rows[:299], ids[:299], queries, rows[299:300], np.array([5], dtype=np.int64), 301)


def test_abi_refusals(gpu, monkeypatch, small):
    rows, ids, queries = small
    _env(monkeypatch)
    lib = gpu
    removed, size = ctypes.c_int64(-5), ctypes.c_int64(-5)
    host_ids = np.ascontiguousarray(ids[:4])
    assert lib.crag_index_remove(None, host_ids.ctypes.data, 4, ctypes.byref(removed)) == -1
    assert lib.crag_index_compact(None, host_ids.ctypes.data, ctypes.byref(size)) == -1
    assert lib.crag_index_insert(None, rows.ctypes.data, host_ids.ctypes.data, 4) == -1
    with _build(rows[:100], ids[:100], capacity=200) as ix:
        h = ix._h
        assert lib.crag_index_remove(h, None, 3, ctypes.byref(removed)) == -1 and removed.value == 0
        assert lib.crag_index_remove(h, host_ids.ctypes.data, -1, None) == -1
        assert lib.crag_index_remove(h, None, 0, None) == 0                        # n == 0 is CRAG_OK
        assert lib.crag_index_insert(h, None, None, 0) == 0
        assert lib.crag_index_insert(h, None, host_ids.ctypes.data, 2) == -1
        assert lib.crag_index_insert(h, rows.ctypes.data, None, 2) == -1
        unsorted = np.array([ids[5] + 1, ids[2] + 1], dtype=np.int64)
        assert lib.crag_index_insert(h, rows.ctypes.data, unsorted.ctypes.data, 2) == -1
        keep = np.full(20, 0xFF, dtype=np.uint8)
        base = keep.ctypes.data
        off = 1 if base % 4 == 0 else (4 - base % 4) + 1
        assert lib.crag_index_compact(h, base + off, ctypes.byref(size)) == -1      # misaligned
        assert lib.crag_index_compact(h, None, ctypes.byref(size)) == -1
        assert len(ix) == 100
        aligned = base + (-base % 4)
        assert lib.crag_index_compact(h, aligned, ctypes.byref(size)) == 0 and size.value == 100   # bits beyond size ignored
        assert lib.crag_index_remove(h, host_ids.ctypes.data, 4, None) == 0 and len(ix) == 96      # out_removed is nullable


def test_dense_table_delete_and_late_inserts(gpu, monkeypatch):
    """DenseTable.delete_calls / delete / insert keep index, columns, timestamps, tokens and the two lanes one table:
    every lane answers exactly like a backend over a freshly built table, and the index object stays the same one
    while its capacity suffices."""
    from datetime import datetime
    from uuid import UUID

    from cadence_rag_amd import retrieve as rt
    _env(monkeypatch)
    rng = np.random.default_rng(31)
    vecs = unit_rows(rng, 260)
    all_ids = list(range(1000, 1520, 2))

    def cols(ids):
        ids = list(ids)
        return {"chunk_id": ids, "call_id": [UUID(int=1 + (i // 2) % 4) for i in ids], "speaker": ["S"] * len(ids),
                "start_ts_ms": [0] * len(ids), "end_ts_ms": [1] * len(ids),
                "text": [f"row {i} timeout in shard {i % 7}" for i in ids],
                "tech_tokens": [["ECONNRESET"] if i % 10 == 0 else [f"TOK-{i}"] for i in ids]}

    def started(ids):
        return [datetime(2024, 1, 1 + (i % 20)) for i in ids]

    def table_of(idx, capacity=400):
        t = rt.DenseTable("chunks", "chunk_id", dim=1024, capacity=capacity)
        ids = [all_ids[i] for i in idx]
        t.add(vecs[idx], cols(ids), call_started_at=started(ids))
        return t

    def backend(t):
        return rt.GpuRetrieveBackend(t, t, tech_chunks=t.build_tech_lane([list(x) for x in cols(t.columns["chunk_id"])["tech_tokens"]]),
                                     bm25_chunks=t.build_bm25_lane("text"))

    def answers(be, q):
        f = rt.RetrieveFilters(date_from=datetime(2024, 1, 5), date_to=datetime(2024, 1, 15))
        return (be.fetch_chunks_dense(q, None, None, "exact", 20), be.fetch_chunks_dense(q, f, None, "exact", 20),
                be.fetch_chunks_tech(["ECONNRESET"], None, None, 50), be.fetch_chunks_tech(["ECONNRESET"], f, None, 50),
                be.fetch_chunks_bm25("timeout shard 3", None, None, 20), be.fetch_chunks_bm25("timeout shard 3", f, None, 20))

    early = np.arange(0, 200)
    table = table_of(early)
    fresh = None
    try:
        be = backend(table)
        answers(be, vecs[3])                                   # the lanes exist and were used before the delete
        index_before, gen, n_before = table.index, table.generation, len(table)
        gone_call = UUID(int=2)
        n_gone = sum(1 for c in table.call_ids if c == gone_call)
        assert table.delete_calls([gone_call]) == n_gone > 0
        assert len(table) == n_before - n_gone == len(table.columns["chunk_id"]) == len(table.tech_tokens)
        assert table.generation > gen and gone_call not in set(table.call_ids) and table.index is index_before
        left = np.array([i for i in early if UUID(int=1 + (all_ids[i] // 2) % 4) != gone_call])
        fresh = table_of(left)
        got, want = answers(be, vecs[3]), answers(backend(fresh), vecs[3])
        assert got == want
        gone_ids = {all_ids[i] for i in early} - set(table.columns["chunk_id"])
        for lane_rows in got:
            assert lane_rows and not gone_ids.intersection(r["chunk_id"] for r in lane_rows)
        assert be._tech["chunks"].n == len(table) and len(be._bm25["chunks"]) == len(table)
        # delete by id, absent ids ignored
        assert table.delete([all_ids[left[0]], all_ids[left[5]], 7]) == 2
        left = np.delete(left, [0, 5])
        # late rows through sink(): below, between and above the stored ids, two batches, unsorted inside a batch
        late = np.array([i for i in early if i not in set(left)][:30] + list(range(200, 230)))
        sink = table.sink(lambda ids: dict(cols(ids), call_started_at=started(ids)))
        for part in (late[:25][::-1], late[25:]):
            sink.add(vecs[part].tolist(), ids=[all_ids[i] for i in part])
        assert table.index is index_before                     # no rebuild while the capacity suffices
        fresh.close()
        fresh = table_of(np.sort(np.concatenate([left, late])))
        assert table.columns["chunk_id"] == fresh.columns["chunk_id"]
        assert np.array_equal(table.call_started_at, fresh.call_started_at)
        assert answers(be, vecs[210]) == answers(backend(fresh), vecs[210])
        a, b = table.index.get_rows(0, len(table)), fresh.index.get_rows(0, len(fresh))
        assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    finally:
        table.close()
        if fresh is not None:
            fresh.close()
