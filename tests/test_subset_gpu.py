"""The search over listed rows (crag_index_search_ids_async) against the masked search it must equal bit for bit: for the
same queries and k, under a mask whose set bits are the positions of the listed ids, ids, score bits and counts are the
same -- whatever the width, k, nq, the counts, the order of a list, repeats, ids that are not stored, rows and queries
that score nothing, the row layout, the dim or the path the masked search takes (fp32 scan at 200 rows, prefilter at
40 000).  Then the per-slot scores, edits, argument errors and the route through DenseTable / GpuRetrieveBackend."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import settings
from cadence_rag_amd.dense_index import DenseIndex
from helpers import assert_topk_matches

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_ROWS = 200          # six full tiles and a ragged seventh
N_BIG = 40000         # the masked search takes the prefilter path here (tests/helpers.py)
KS = (1, 32, 33, 128)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Data:
    """n rows, ids 10 + 3 * position; a duplicated row pair (tie -> ascending id), a zero row and a NaN row."""

    def __init__(self, n: int, dim: int, seed: int) -> None:
        rng = np.random.default_rng(seed)
        rows = rng.standard_normal((n, dim)).astype(np.float32) * rng.uniform(0.2, 5.0, size=(n, 1)).astype(np.float32)
        self.twin_pos, self.zero_pos, self.nan_pos = (17, n - 3), 40, 77
        rows[self.twin_pos[1]] = rows[self.twin_pos[0]]
        rows[self.zero_pos] = 0.0
        rows[self.nan_pos, dim // 2] = np.nan
        self.rows, self.n, self.dim, self.rng = rows, n, dim, rng
        self.ids = 10 + 3 * np.arange(n, dtype=np.int64)
        # between stored ids, below the first, above the last, far above
        self.unstored = np.asarray([11, 12, 10 + 3 * 50 + 1, 5, -9, 10 + 3 * n + 5, 2 ** 40], dtype=np.int64)
        self.twins = [int(self.ids[p]) for p in self.twin_pos]
        self.zero, self.nan = int(self.ids[self.zero_pos]), int(self.ids[self.nan_pos])

    def queries(self, nq: int) -> np.ndarray:
        q = self.rng.standard_normal((nq, self.dim)).astype(np.float32)
        q[0] = self.rows[self.twin_pos[0]] * 0.5          # the twins tie at the top of this query
        if nq >= 3:
            q[1] = 0.0                                    # a zero query
            q[2, 0] = np.nan                              # a non-finite query
        return q

    def random_list(self, count: int) -> np.ndarray:
        """ids drawn with repeats, with unstored ids, -1, the zero row, the NaN row and the twins among them"""
        pool = np.concatenate([self.ids, self.unstored, np.asarray([-1, self.zero, self.nan] + self.twins, dtype=np.int64)])
        out = self.rng.choice(pool, size=count, replace=True)
        special = np.concatenate([self.unstored, np.asarray([-1, self.zero, self.nan] + self.twins + self.twins[:1])])
        if count >= 2 * special.size:   # a list with room for them holds every special id
            out[self.rng.choice(count, size=special.size, replace=False)] = special
        return out.astype(np.int64)


def build(data: Data, mirror: bool = True, rows=None, ids=None, extra: int = 8) -> DenseIndex:
    old = os.environ.pop("CRAG_NO_FP16_MIRROR", None)
    try:
        if not mirror:
            os.environ["CRAG_NO_FP16_MIRROR"] = "1"     # read once, at crag_index_create
        ix = DenseIndex(data.dim, capacity=data.n + extra, device=0)
    finally:
        os.environ.pop("CRAG_NO_FP16_MIRROR", None)
        if old is not None:
            os.environ["CRAG_NO_FP16_MIRROR"] = old
    ix.add(data.rows if rows is None else rows, data.ids if ids is None else ids)
    return ix


@pytest.fixture(scope="module")
def data(gpu):
    return Data(N_ROWS, 1024, 5)


@pytest.fixture(scope="module")
def index(data):
    ix = build(data)
    assert ix.prefilter_row_bytes() == 2048
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def index_rows_only(data):
    ix = build(data, mirror=False)
    assert ix.prefilter_row_bytes() == 4096
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def big(gpu):
    d = Data(N_BIG, 1024, 11)
    ix = build(d)
    yield d, ix
    ix.close()


def listed(ix: DenseIndex, queries, lists, k: int, width: int, counts=None, shared: bool = False, slot: bool = True):
    """-> ids [nq, k], scores [nq, k], counts [nq], slot scores [nq, width] (None without), through the async entry
    with sentinel-filled outputs.  counts: what the entry is GIVEN (default: the lists' lengths)."""
    nq = int(queries.shape[0])
    h = np.full((len(lists), width), -1, dtype=np.int64)
    for q, l in enumerate(lists):
        h[q, :len(l)] = l
    d_ids = torch.from_numpy(h[0] if shared else h).to(DEV)
    d_ct = torch.tensor([len(l) for l in lists] if counts is None else list(counts), dtype=torch.int32, device=DEV)
    out_ids = torch.full((nq, k), -7, dtype=torch.int64, device=DEV)
    out_sc = torch.full((nq, k), -7.0, dtype=torch.float32, device=DEV)
    out_ct = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    sl = torch.full((nq, width), -7.0, dtype=torch.float32, device=DEV) if slot else None
    ix.search_ids_async(torch.from_numpy(queries).to(DEV), d_ids, d_ct, k, out_ids, out_sc, out_ct, sl, shared=shared,
                        stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    return out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_ct.cpu().numpy(), None if sl is None else sl.cpu().numpy()


def masked(ix: DenseIndex, stored_ids, queries, lists, k: int):
    """The reference: the masked search under the positions of the listed ids."""
    mask = np.zeros((len(lists), len(stored_ids)), dtype=bool)
    for q, l in enumerate(lists):
        l = np.asarray(l, dtype=np.int64)
        l = l[l != -1]
        pos = np.searchsorted(stored_ids, l)
        ok = (pos < len(stored_ids)) & (stored_ids[np.minimum(pos, len(stored_ids) - 1)] == l)
        mask[q, pos[ok]] = True
    return ix.search(queries, k, row_mask=DenseIndex.pack_mask(mask))


def assert_same(got, want, note=""):
    assert np.array_equal(got[2], want[2]), (note, got[2], want[2])
    assert np.array_equal(got[0], want[0]), note
    assert np.array_equal(bits(got[1]), bits(want[1])), note


def ragged(data: Data, width: int, nq: int):
    """lists and the counts GIVEN to the entry: full, empty, a few, above the width (clamped), then random"""
    given = [width, 0, min(3, width), width + 7, width // 2][:nq]
    given += [int(c) for c in data.rng.integers(0, width + 1, size=nq - len(given))]
    lists = [data.random_list(min(c, width)) for c in given]
    return lists, given


@pytest.mark.parametrize("mirror", [True, False])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 200])
def test_widths_k_and_layouts(data, index, index_rows_only, width, mirror):
    ix = index if mirror else index_rows_only
    queries = data.queries(6)
    lists, given = ragged(data, width, 6)
    some = False
    for k in KS:
        got = listed(ix, queries, lists, k, width, counts=given)
        want = masked(ix, data.ids, queries, lists, k)
        assert_same(got, want, (width, k))
        assert got[2][1] == 0 and got[2][2] == 0          # the zero and the non-finite query
        some = some or int(got[2].max()) > 1
    assert some or width == 1


@pytest.mark.parametrize("nq", [1, 33, 70])
def test_batches(data, index, nq):
    queries = data.queries(nq)
    lists, given = ragged(data, 65, nq)
    for k in (33, 128):
        assert_same(listed(index, queries, lists, k, 65, counts=given), masked(index, data.ids, queries, lists, k), (nq, k))


def test_layouts_agree_bit_for_bit(data, index, index_rows_only):
    queries = data.queries(5)
    lists, _ = ragged(data, 200, 5)
    a, b = listed(index, queries, lists, 50, 200), listed(index_rows_only, queries, lists, 50, 200)
    assert_same(a, b)
    assert np.array_equal(bits(a[3]), bits(b[3]))


@pytest.mark.parametrize("dim", [260, 7])
def test_small_dims(gpu, dim):
    d = Data(N_ROWS, dim, 20 + dim)
    with build(d) as ix:
        queries = d.queries(7)
        lists, given = ragged(d, 200, 7)
        for k in (1, 33, 128):
            assert_same(listed(ix, queries, lists, k, 200, counts=given), masked(ix, d.ids, queries, lists, k), (dim, k))


def test_prefilter_sized_index_and_the_widest_list(big):
    d, ix = big
    queries = d.queries(4)
    lists = [d.random_list(2000) for _ in range(4)]
    for k in (32, 128):
        got = listed(ix, queries, lists, k, 4096)
        assert_same(got, masked(ix, d.ids, queries, lists, k), k)
        assert got[2][0] == k and got[0][0, :2].tolist() == d.twins       # the tie: ascending id
    lists, given = ragged(d, 200, 4)
    assert_same(listed(ix, queries, lists, 33, 200, counts=given), masked(ix, d.ids, queries, lists, 33))


def test_a_list_is_a_set(data, index):
    queries = data.queries(4)
    base = [data.random_list(90) for _ in range(4)]
    want = listed(index, queries, base, 50, 90)
    shuffled = [data.rng.permutation(l) for l in base]
    doubled = [np.repeat(l, 2) for l in base]
    assert_same(listed(index, queries, shuffled, 50, 90), want)
    assert_same(listed(index, queries, doubled, 50, 180), want)
    assert_same(listed(index, queries, doubled, 50, 200), want)           # ... and the width changes nothing either


def test_shared_list(data, index):
    queries = data.queries(9)
    lst = data.random_list(130)
    shared = listed(index, queries, [lst], 33, 130, shared=True)
    each = listed(index, queries, [lst] * 9, 33, 130)
    assert_same(shared, each)
    assert np.array_equal(bits(shared[3]), bits(each[3]))
    assert_same(shared, masked(index, data.ids, queries, [lst] * 9, 33))
    host = index.search_ids(queries, lst.tolist(), 33, slot_scores=True)    # the host form: a flat list is shared
    assert_same(host, shared)
    assert np.array_equal(bits(host[3]), bits(shared[3]))
    ragged_host = index.search_ids(queries[:2], [lst[:5].tolist(), []], 4)
    assert_same(ragged_host, masked(index, data.ids, queries[:2], [lst[:5], []], 4))
    with pytest.raises(ValueError):
        index.search_ids(queries[:1], list(range(4097)), 5)


def test_against_the_fp64_oracle(data, index):
    import oracle
    clean = np.setdiff1d(np.arange(N_ROWS), [data.zero_pos, data.nan_pos, data.twin_pos[1]])
    pos = np.sort(data.rng.choice(clean, size=120, replace=False))
    queries = data.rng.standard_normal((5, 1024)).astype(np.float32)
    got = listed(index, queries, [data.rng.permutation(data.ids[pos])] * 5, 20, 120)
    want = oracle.exact_topk(queries, data.rows[pos], 20, ids=data.ids[pos], mode=oracle.F64)
    assert_topk_matches(got[0], got[1], got[2], *want)


def test_slot_scores(data, index):
    queries = data.queries(5)
    lists = [data.random_list(c) for c in (100, 64, 1, 0, 37)]
    lists[0][[3, 50]] = data.ids[5]                                        # a repeated id: both slots are filled
    width = 110
    got = listed(index, queries, lists, 128, width)
    want = masked(index, data.ids, queries, lists, 128)
    assert_same(got, want)
    for q, l in enumerate(lists):
        score_of = {int(i): s for i, s in zip(want[0][q, :want[2][q]], bits(want[1][q, :want[2][q]]))}
        assert want[2][q] < 128                                            # every eligible id of the list was returned
        for s in range(width):
            b = bits(got[3][q, s:s + 1])[0]
            if s < len(l) and int(l[s]) in score_of:
                assert b == score_of[int(l[s])], (q, s)
            else:
                assert np.isnan(got[3][q, s]), (q, s)
    assert not np.isnan(got[3][0, 3]) and bits(got[3][0, 3:4]) == bits(got[3][0, 50:51])
    bare = listed(index, queries, lists, 128, width, slot=False)
    assert_same(bare, got)


def test_after_remove_and_insert(data):
    late = np.asarray([30, 31, 95, 150])
    gone_pos = np.asarray([3, 40, 41, 97, 160])
    start = np.setdiff1d(np.arange(N_ROWS), late)
    ix = build(data, rows=data.rows[start], ids=data.ids[start])
    try:
        queries = data.queries(4)
        lists = [np.concatenate([data.random_list(80), data.ids[gone_pos], data.ids[late]]) for _ in range(4)]
        stored = data.ids[start]
        assert_same(listed(ix, queries, lists, 50, 100), masked(ix, stored, queries, lists, 50), "before")
        ix.remove(data.ids[gone_pos])
        stored = np.setdiff1d(stored, data.ids[gone_pos])
        got = listed(ix, queries, lists, 50, 100)
        assert_same(got, masked(ix, stored, queries, lists, 50), "removed")
        assert not np.isin(got[0], data.ids[gone_pos]).any()
        ix.insert(data.rows[late], data.ids[late])                         # rows between stored ids
        stored = np.sort(np.concatenate([stored, data.ids[late]]))
        got = listed(ix, queries, lists, 128, 100)
        assert_same(got, masked(ix, stored, queries, lists, 128), "inserted")
        assert np.isin(data.ids[late], got[0][3]).all()
    finally:
        ix.close()


def test_an_empty_index(gpu):
    with DenseIndex(1024, capacity=64, device=0) as ix:
        q = np.ones((2, 1024), dtype=np.float32)
        got = listed(ix, q, [[10, 13, -1], [2 ** 40]], 5, 3)
        assert got[2].tolist() == [0, 0] and (got[0] == -1).all() and np.isnan(got[1]).all() and np.isnan(got[3]).all()


def test_argument_errors_enqueue_nothing(gpu, data, index):
    nq, width, k = 2, 8, 5
    d_q = torch.from_numpy(data.queries(3)[:nq].copy()).to(DEV)   # query 1: the zero query
    d_ids = torch.full((nq, 4100), int(data.ids[0]), dtype=torch.int64, device=DEV)
    d_ct = torch.full((nq,), 8, dtype=torch.int32, device=DEV)
    outs = [torch.full((nq, 128), -7, dtype=torch.int64, device=DEV), torch.full((nq, 128), -7.0, dtype=torch.float32, device=DEV),
            torch.full((nq,), -7, dtype=torch.int32, device=DEV), torch.full((nq, 4100), -7.0, dtype=torch.float32, device=DEV)]
    scratch = torch.zeros(nq * 4100 * 8 + 8, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(**kw):
        a = dict(ix=index._h, q=d_q.data_ptr(), nq=nq, ids=d_ids.data_ptr(), ct=d_ct.data_ptr(), width=width, stride=None,
                 k=k, o0=outs[0].data_ptr(), o1=outs[1].data_ptr(), o2=outs[2].data_ptr(), o3=outs[3].data_ptr(),
                 scratch=scratch.data_ptr(), nbytes=int(scratch.numel()))
        a.update(kw)
        stride = a["width"] if a["stride"] is None else a["stride"]
        return gpu.crag_index_search_ids_async(a["ix"], a["q"], a["nq"], a["ids"], a["ct"], a["width"], stride, a["k"], a["o0"],
                                               a["o1"], a["o2"], a["o3"], a["scratch"], a["nbytes"], st)

    assert scratch.data_ptr() % 8 == 0
    for kw in (dict(ix=None), dict(q=None), dict(ids=None), dict(ct=None), dict(o0=None), dict(o1=None), dict(o2=None),
               dict(scratch=None), dict(nq=-1), dict(width=0), dict(k=0), dict(k=129), dict(stride=4), dict(stride=-8),
               dict(nbytes=nq * width * 8 - 1), dict(scratch=scratch.data_ptr() + 4)):
        assert call(**kw) == -1, kw
        assert gpu.crag_last_error(), kw
    assert call(width=4097) == -5 and gpu.crag_last_error()
    assert call(nq=0) == 0
    torch.cuda.synchronize(DEV)
    assert bool((outs[0] == -7).all()) and bool((outs[1] == -7.0).all()) and bool((outs[2] == -7).all())
    assert bool((outs[3] == -7.0).all())
    assert call() == 0 and call(o3=None) == 0                              # the same arguments, valid: it runs
    torch.cuda.synchronize(DEV)
    assert outs[2].tolist() == [1, 0]                                      # (query 1 is the zero query)


def test_through_the_table_and_the_backend(gpu, data, monkeypatch):
    from datetime import datetime, timedelta
    from uuid import UUID
    clean = np.setdiff1d(np.arange(N_ROWS), [data.zero_pos, data.nan_pos])
    n, t0 = len(clean), datetime(2026, 3, 1)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(20)]
    cols = {"chunk_id": [int(data.ids[p]) for p in clean], "call_id": [calls[(i * 7) % 20]["call_id"] for i in range(n)],
            "text": [f"row {int(p)}" for p in clean], "speaker": ["S%d" % (i % 3) for i in range(n)],
            "start_ts_ms": [i * 10 for i in range(n)], "end_ts_ms": [i * 10 + 9 for i in range(n)]}
    chunks = rt.DenseTable("chunks", "chunk_id", dim=1024, capacity=n + 64)
    arts = rt.DenseTable("artifact_chunks", "artifact_chunk_id", dim=1024, capacity=8)
    taken = []
    real = DenseIndex.search_ids

    def spy(self, queries, ids, k, slot_scores=False):
        taken.append(len(ids[0]))
        return real(self, queries, ids, k, slot_scores)

    monkeypatch.setattr(DenseIndex, "search_ids", spy)
    try:
        chunks.add(data.rows[clean], cols, call_started_at=[t0 + timedelta(days=i % 6) if i % 11 else None for i in range(n)],
                   call_tags={c["call_id"]: ["billing"] if i % 2 else ["outage", "renewal"] for i, c in enumerate(calls)})
        be = rt.GpuRetrieveBackend(chunks, arts, calls=calls)
        q = data.queries(1)[0]
        ids5 = [c["call_id"] for c in calls[:5]]
        F = rt.RetrieveFilters
        scoped = [(F(), ids5), (F(), ids5[:1]), (F(date_from=t0 + timedelta(days=2)), ids5),
                  (F(date_from=t0 + timedelta(days=1), date_to=t0 + timedelta(days=4)), ids5),
                  (F(call_tags=["billing"]), ids5), (F(call_tags=["outage"], date_to=t0 + timedelta(days=3)), ids5),
                  (F(), ids5 + [UUID(int=999)]), (F(), [])]
        unscoped = [(None, None), (F(), None), (F(date_from=t0 + timedelta(days=2)), None), (None, ids5)]
        first = None
        for limit in (50, 3):
            monkeypatch.setattr(settings, "embeddings_exact_scan_threshold", 2000)
            on = [be.fetch_chunks_dense(q, f, c, "exact", limit) for f, c in scoped]
            assert len(taken) == len(scoped) - 1 and min(taken) >= 1       # ([] needs no search at all)
            del taken[:]
            monkeypatch.setattr(settings, "embeddings_exact_scan_threshold", 0)
            off = [be.fetch_chunks_dense(q, f, c, "exact", limit) for f, c in scoped]
            assert not taken
            assert on == off and len(on[0]) == limit and on[-1] == [] and len(on[1]) >= 1
            assert all(set(r) == set(rt.CHUNK_SELECT) | {"score"} for r in on[0])
            first = first or on[0]
        monkeypatch.setattr(settings, "embeddings_exact_scan_threshold", 2000)
        for f, c in unscoped:
            assert len(be.fetch_chunks_dense(q, f, c, "ann", 10)) == 10
        assert not taken
        monkeypatch.setattr(settings, "embeddings_exact_scan_threshold", 20)   # below the rows of the five calls
        assert be.fetch_chunks_dense(q, F(), ids5, "exact", 50) == first
        assert not taken
    finally:
        chunks.close(); arts.close()
