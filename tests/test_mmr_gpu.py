"""MMR on the GPU (crag_index_mmr_async) through the C ABI and its wrappers: DenseIndex, DenseTable, GpuRetrieveBackend,
retrieve_evidence.

The walk is checked with no tolerance: cadence_rag_amd.mmr.mmr_host, fed the kernel's own similarity rows, must reproduce
every output bit.  The similarity rows are checked on their own: within 1e-4 of the fp64 cosine (the project's score bar),
NaN exactly where the oracle says "not comparable", symmetric, the bits of crag_index_dedupe_async, unchanged by nq, width,
k, lambda, the row layout and edits.  Against the fp64 oracle of mmr_oracle.py the picks must agree exactly on lists whose
decision gaps are >= 1e-3 by construction (asserted on the oracle first)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import settings
from cadence_rag_amd.dense_index import DenseIndex
from cadence_rag_amd.mmr import MmrParams, mmr_host
from mmr_oracle import candidate_slots, crafted, crafted_query, mmr_oracle, pair_cosines

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_ROWS = 200          # six full tiles and a ragged seventh
N_CLUSTERS, PER_CLUSTER = 12, 15
CRAFTED = ((0.5, 12, 1), (0.7, 40, 0), (0.3, 20, 11))   # lambda, k, seed (tests/test_mmr_host.py)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


class Data:
    """test_dedupe_gpu.py's recipe: 200 rows in shuffled order (members of a cluster lie in different tiles), clusters at
    ~0.99, a zero row and a NaN row, ids 10 + 3 * position; lists draw stored ids (repeats included), unstored ids and -1."""

    def __init__(self, dim: int, seed: int) -> None:
        rng = np.random.default_rng(seed)

        def unit(n):
            a = rng.standard_normal((n, dim))
            return a / np.linalg.norm(a, axis=1, keepdims=True)

        rows = []
        for base in unit(N_CLUSTERS):   # base + noise of length 0.1: in-cluster cosines ~0.99
            rows += [(base + 0.1 * e) * rng.uniform(0.2, 5.0) for e in unit(PER_CLUSTER)]
        twin = unit(1)[0] * 1.7
        special = [twin, twin, np.zeros(dim), np.full(dim, np.nan)]
        rows += special + list(unit(N_ROWS - len(rows) - len(special)))
        rows = np.asarray(rows, dtype=np.float32)
        perm = rng.permutation(N_ROWS)
        self.rows = np.ascontiguousarray(rows[perm])
        self.ids = 10 + 3 * np.arange(N_ROWS, dtype=np.int64)
        where = np.empty(N_ROWS, dtype=np.int64)
        where[perm] = np.arange(N_ROWS)
        n_cl = N_CLUSTERS * PER_CLUSTER
        self.zero, self.nan = int(self.ids[where[n_cl + 2]]), int(self.ids[where[n_cl + 3]])
        self.unstored = [11, 12, 10 + 3 * N_ROWS + 5, 5, 2 ** 40]
        self.rng = rng

    def random_list(self, count: int) -> np.ndarray:
        pool = np.concatenate([self.ids, self.ids, np.asarray(self.unstored + [-1], dtype=np.int64)])
        return self.rng.choice(pool, size=count, replace=count > pool.size // 2)

    def random_rel(self, count: int) -> np.ndarray:
        """Half from a short grid (ties, -0.0 among them), half uniform; a few NaN / inf."""
        grid = self.rng.choice(np.asarray([-0.5, -0.0, 0.0, 0.25, 0.5, 0.75], dtype=np.float32), size=count)
        rel = np.where(self.rng.random(count) < 0.5, grid, self.rng.uniform(-1, 1, size=count).astype(np.float32))
        odd = self.rng.random(count) < 0.03
        rel[odd] = self.rng.choice(np.asarray([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(odd.sum()))
        return rel.astype(np.float32)

    def batch(self, nq: int, width: int):
        """Ragged lists: the first is full, one is empty when there is room for it."""
        counts = [width] + [int(c) for c in self.rng.integers(0, width + 1, size=nq - 1)]
        if nq > 2:
            counts[1] = 0
        return [self.random_list(c) for c in counts], [self.random_rel(c) for c in counts]


def build(data: Data, monkeypatch=None, mirror=True, rows=None, ids=None) -> DenseIndex:
    if monkeypatch is not None:
        if mirror:
            monkeypatch.delenv("CRAG_NO_FP16_MIRROR", raising=False)
        else:
            monkeypatch.setenv("CRAG_NO_FP16_MIRROR", "1")
    ix = DenseIndex(data.rows.shape[1], capacity=N_ROWS + 8, device=0)
    ix.add(data.rows if rows is None else rows, data.ids if ids is None else ids)
    return ix


@pytest.fixture(scope="module")
def data(gpu):
    return Data(1024, 5)


@pytest.fixture(scope="module")
def index(data):
    ix = build(data)
    yield ix
    ix.close()


def run(ix: DenseIndex, lists, rels, width: int, lam: float, k: int, aux: bool = True):
    """-> dict of host arrays: ids / rel [nq, k], counts [nq], and with aux value / slots [nq, k], sim [nq, k, width].
    Every output is prefilled with -7."""
    nq = len(lists)
    h_ids = np.full((nq, width), -1, dtype=np.int64)
    h_rel = np.full((nq, width), 0.5, dtype=np.float32)     # (finite beyond the count: the count alone must cut there)
    for q, (l, r) in enumerate(zip(lists, rels)):
        h_ids[q, :len(l)] = l
        h_rel[q, :len(r)] = r
    d_ids, d_rel = torch.from_numpy(h_ids).to(DEV), torch.from_numpy(h_rel).to(DEV)
    d_ct = torch.tensor([len(l) for l in lists], dtype=torch.int32, device=DEV)
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device=DEV)   # noqa: E731
    out = {"ids": full((nq, k), torch.int64), "rel": full((nq, k), torch.float32), "counts": full((nq,), torch.int32)}
    if aux:
        out.update(value=full((nq, k), torch.float32), slots=full((nq, k), torch.int32),
                   sim=full((nq, k, width), torch.float32))
    ix.mmr_async(d_ids, d_rel, d_ct, lam, k, out["ids"], out["rel"], out["counts"], out.get("value"), out.get("slots"),
                 out.get("sim"), stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    return {name: t.cpu().numpy() for name, t in out.items()}


def replay(out, lists, rels, lam: float, k: int) -> None:
    """mmr_host on the input rel and the kernel's own similarity rows reproduces every output exactly, padding included."""
    for q, (l, r) in enumerate(zip(lists, rels)):
        n = len(l)
        rows = out["sim"][q]
        slots, values = mmr_host(r, lambda p, t: rows[t, :n], lam, k, l)
        c = slots.size
        where = (q, n, lam, k)
        assert out["counts"][q] == c == min(k, int(candidate_slots(r, l).sum())), where
        assert np.array_equal(out["slots"][q, :c], slots) and np.all(out["slots"][q, c:] == -1), where
        assert np.array_equal(out["ids"][q, :c], np.asarray(l, dtype=np.int64)[slots]) and np.all(out["ids"][q, c:] == -1), where
        assert np.array_equal(bits(out["rel"][q, :c]), bits(np.asarray(r, dtype=np.float32)[slots])), where
        assert np.array_equal(bits(out["value"][q, :c]), bits(values)), where
        assert np.all(np.isnan(out["rel"][q, c:])) and np.all(np.isnan(out["value"][q, c:])), where
        assert np.all(np.isnan(rows[c:])) and np.all(np.isnan(rows[:, n:])), where


def check_sim_rows(out, lists, rels, stored_ids, stored_rows) -> None:
    """Every finite cell within 1e-4 of the fp64 cosine; NaN exactly where the pair is not comparable or the slot ignored."""
    for q, (l, r) in enumerate(zip(lists, rels)):
        n, c = len(l), int(out["counts"][q])
        if c == 0:
            continue
        cos = pair_cosines(stored_ids, stored_rows, l)
        cand = candidate_slots(r, l)
        want = cos[out["slots"][q, :c]]
        want[:, ~cand] = np.nan
        got = out["sim"][q, :c, :n]
        assert np.array_equal(np.isnan(got), np.isnan(want)), q
        ok = ~np.isnan(want)
        if ok.any():
            assert np.max(np.abs(got[ok] - want[ok])) <= 1e-4, q


def pair_bits(out, lists) -> dict:
    """(id a, id b) -> the bits of every finite cell (pick a, slot of b)."""
    seen = {}
    for q, l in enumerate(lists):
        for t in range(int(out["counts"][q])):
            a = int(out["ids"][q, t])
            row = out["sim"][q, t, :len(l)]
            for s in np.flatnonzero(~np.isnan(row)):
                b = int(l[s])
                v = int(bits(row[s:s + 1])[0])
                assert seen.setdefault((a, b), v) == v, (a, b)
    return seen


@pytest.mark.parametrize("width", [1, 2, 31, 32, 33, 64, 65, 255, 256])
def test_replay_with_no_tolerance(data, index, width):
    for nq in (1, 3, 65):
        lists, rels = data.batch(nq, width)
        for k in sorted({1, 2, width}):
            for lam in (0.0, 0.3, 0.7, 1.0):
                out = run(index, lists, rels, width, lam, k)
                replay(out, lists, rels, lam, k)
        check_sim_rows(out, lists, rels, data.ids, data.rows)     # (the last run: k = width, lambda = 1)


def test_dim_768(gpu):
    d768 = Data(768, 6)
    ix = build(d768)
    try:
        lists, rels = d768.batch(3, 100)
        for lam, k in ((0.4, 100), (1.0, 7)):
            out = run(ix, lists, rels, 100, lam, k)
            replay(out, lists, rels, lam, k)
            check_sim_rows(out, lists, rels, d768.ids, d768.rows)
    finally:
        ix.close()


def test_similarity_is_symmetric_and_dedupes_bits(data, index):
    """k = width picks every candidate: cell (pick a, slot of b) and cell (pick b, slot of a) hold the same bits, and they
    are the bits crag_index_dedupe_async reports for the two-item list [b, a] at threshold -0.999999."""
    width = 130
    lists, rels = [data.random_list(width)], [data.rng.uniform(-1, 1, size=width).astype(np.float32)]
    out = run(index, lists, rels, width, 0.5, width)
    seen = pair_bits(out, lists)
    assert len(seen) > 2000 and all(seen[(b, a)] == v for (a, b), v in seen.items())
    pairs = [p for p in seen if p[0] != p[1]]
    pairs = [pairs[i] for i in data.rng.choice(len(pairs), size=64, replace=False)]
    d_ids = torch.tensor([[b, a] for a, b in pairs], dtype=torch.int64, device=DEV)
    d_ct = torch.full((len(pairs),), 2, dtype=torch.int32, device=DEV)
    o_ids, o_ct = torch.empty_like(d_ids), torch.empty_like(d_ct)
    o_sim = torch.empty(len(pairs), 2, dtype=torch.float32, device=DEV)
    index.dedupe_async(d_ids, d_ct, -0.999999, o_ids, o_ct, None, o_sim, stream=torch.cuda.current_stream(DEV).cuda_stream)
    sim = o_sim.cpu().numpy()
    assert not np.isnan(sim[:, 1]).any()
    assert bits(sim[:, 1]).tolist() == [seen[p] for p in pairs]


def test_similarity_bits_do_not_depend_on_the_call(data, index, monkeypatch):
    lists, rels = data.batch(3, 256)
    want = pair_bits(run(index, lists, rels, 256, 0.5, 256), lists)
    # other nq / width / k / lambda: shorter lists of the same ids in another order, other relevances
    for nq, width, k, lam in ((1, 97, 97, 0.0), (5, 64, 20, 0.9), (2, 33, 33, 1.0)):
        short = [data.rng.permutation(lists[q % 3])[:min(width, len(lists[q % 3]))] for q in range(nq)]
        other = [data.random_rel(len(l)) for l in short]
        got = pair_bits(run(index, short, other, width, lam, k), short)
        assert len(got) > 50 and all(want[p] == v for p, v in got.items() if p in want)
        assert sum(p in want for p in got) > 50
    # the other row layout
    ix = build(data, monkeypatch, mirror=False)
    try:
        assert ix.prefilter_row_bytes() == 4096 and index.prefilter_row_bytes() == 2048
        assert pair_bits(run(ix, lists, rels, 256, 0.5, 256), lists) == want
    finally:
        ix.close()


@pytest.mark.parametrize("mirror", [True, False])
def test_after_edits_equals_a_fresh_build(data, monkeypatch, mirror):
    gone = data.ids[[3, 40, 41, 97, 160]]
    final = np.setdiff1d(np.arange(N_ROWS), [3, 40, 41, 97, 160])
    late = np.sort(data.rng.choice(final, size=9, replace=False))
    start = np.setdiff1d(np.arange(N_ROWS), late)
    edited = build(data, monkeypatch, mirror, rows=data.rows[start], ids=data.ids[start])
    edited.remove(gone)
    edited.insert(data.rows[late], data.ids[late])
    fresh = build(data, monkeypatch, mirror, rows=data.rows[final], ids=data.ids[final])
    try:
        lists, rels = data.batch(3, 200)
        lists[2] = np.concatenate([gone, lists[2]])[:200]       # removed ids: stored no longer, picked by rel alone
        rels[2] = data.random_rel(len(lists[2]))
        got, want = run(edited, lists, rels, 200, 0.5, 200), run(fresh, lists, rels, 200, 0.5, 200)
        replay(got, lists, rels, 0.5, 200)
        check_sim_rows(got, lists, rels, data.ids[final], data.rows[final])
    finally:
        edited.close(); fresh.close()
    for name in ("ids", "slots", "counts"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("rel", "value", "sim"):
        assert np.array_equal(bits(got[name]), bits(want[name])), name


def test_lambda_one_is_search_ids(data, index):
    """rel = search_ids' slot scores, lambda = 1: the ids, score bits and counts of crag_index_search_ids_async."""
    nq, width = 5, 150
    lists = [data.random_list(c) for c in (150, 0, 77, 150, 3)]
    queries = data.rng.standard_normal((nq, 1024)).astype(np.float32)
    for k in (1, 10, 128):
        ids, scores, counts, slot = index.search_ids(queries, lists, k, slot_scores=True)
        rels = [slot[q, :len(l)] for q, l in enumerate(lists)]
        out = run(index, lists, rels, width, 1.0, k)
        assert np.array_equal(out["counts"], counts) and np.array_equal(out["ids"], ids)
        assert np.array_equal(bits(out["rel"]), bits(scores)) and np.array_equal(bits(out["value"]), bits(scores))
    assert counts[0] > 100 and counts[1] == 0


@pytest.mark.parametrize("lam,k,seed", CRAFTED)
def test_against_the_fp64_oracle_on_crafted_lists(gpu, lam, k, seed):
    rows, ids, rel = crafted(seed)
    cos = pair_cosines(ids, rows, ids)
    slots, values, gaps = mmr_oracle(rel, cos, lam, k, ids)
    assert slots.size == k and gaps.min() >= 1e-3                # an assertion on the construction, not a skip
    assert not np.array_equal(slots, mmr_oracle(rel, cos, 1.0, k, ids)[0])
    with DenseIndex(1024, capacity=64, device=0) as ix:
        ix.add(rows, ids)
        out = run(ix, [ids, ids[::-1].copy()], [rel, rel[::-1].copy()], 40, lam, k)
    assert out["counts"].tolist() == [k, k]
    assert np.array_equal(out["slots"][0], slots) and np.array_equal(out["ids"][0], ids[slots])
    assert np.array_equal(out["ids"][1], ids[slots]) and np.array_equal(out["slots"][1], 39 - slots)   # a list is a set
    assert np.max(np.abs(out["value"][0] - values)) <= 1e-4 and np.array_equal(bits(out["value"][0]), bits(out["value"][1]))


def test_nullable_outputs_errors_and_an_empty_index(gpu, data, index):
    lists, rels = data.batch(3, 130)
    full, bare = run(index, lists, rels, 130, 0.4, 50), run(index, lists, rels, 130, 0.4, 50, aux=False)
    assert set(bare) == {"ids", "rel", "counts"}
    assert np.array_equal(full["ids"], bare["ids"]) and np.array_equal(full["counts"], bare["counts"])
    assert np.array_equal(bits(full["rel"]), bits(bare["rel"]))
    # argument errors enqueue nothing: outputs prefilled with -7 stay -7
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    d_ids = torch.from_numpy(np.stack([data.random_list(8), data.random_list(8)])).to(DEV)
    d_rel = torch.rand(2, 8, device=DEV)
    d_ct = torch.tensor([8, 5], dtype=torch.int32, device=DEV)
    outs = [torch.full((2, 4), -7, dtype=torch.int64, device=DEV), torch.full((2, 4), -7.0, dtype=torch.float32, device=DEV),
            torch.full((2,), -7, dtype=torch.int32, device=DEV)]
    scratch = torch.empty(DenseIndex.mmr_scratch_bytes(2, 8), dtype=torch.uint8, device=DEV)

    def call(nq=2, width=8, lam=0.5, k=4, scratch_bytes=int(scratch.numel()), counts=d_ct.data_ptr()):
        return gpu.crag_index_mmr_async(index._h, d_ids.data_ptr(), d_rel.data_ptr(), counts, nq, width, lam, k,
                                        outs[0].data_ptr(), outs[1].data_ptr(), None, None, None, outs[2].data_ptr(),
                                        scratch.data_ptr(), scratch_bytes, st)

    for bad in (dict(width=257), dict(width=0), dict(k=0), dict(k=257), dict(lam=1.5), dict(lam=float("nan")), dict(nq=-1),
                dict(scratch_bytes=int(scratch.numel()) - 1), dict(counts=None)):
        assert call(**bad) == -1 and b"mmr" in gpu.crag_last_error(), bad
    torch.cuda.synchronize(DEV)
    assert all(bool((o == -7).all()) for o in outs)
    assert call(nq=0) == 0
    torch.cuda.synchronize(DEV)
    assert all(bool((o == -7).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize(DEV)
    assert outs[2].tolist() == [min(4, int(candidate_slots(d_rel[0].cpu().numpy(), d_ids[0].cpu().numpy()).sum())),
                                min(4, int(candidate_slots(d_rel[1, :5].cpu().numpy(), d_ids[1, :5].cpu().numpy()).sum()))]
    # an empty index: nothing is comparable, the picks go by rel alone
    with DenseIndex(1024, capacity=64, device=0) as empty:
        l, r = [np.asarray([7, 3, -1, 9, 3, 12], dtype=np.int64)], [np.asarray([0.2, 0.9, 1.0, 0.2, 1.0, np.nan], dtype=np.float32)]
        out = run(empty, l, r, 6, 0.25, 6)
        assert out["counts"].tolist() == [3] and out["ids"][0].tolist() == [3, 7, 9, -1, -1, -1]
        assert out["slots"][0].tolist() == [1, 0, 3, -1, -1, -1] and np.all(np.isnan(out["sim"]))
        replay(out, l, r, 0.25, 6)


def test_host_convenience(data, index):
    lists, rels = data.batch(3, 90)
    want = run(index, lists, rels, 90, 0.6, 25)
    ids, rel, value, slots = index.mmr(lists, rels, 0.6, 25)
    for q in range(3):
        c = int(want["counts"][q])
        assert np.array_equal(ids[q], want["ids"][q, :c]) and np.array_equal(slots[q], want["slots"][q, :c])
        assert np.array_equal(bits(rel[q]), bits(want["rel"][q, :c])) and np.array_equal(bits(value[q]), bits(want["value"][q, :c]))
    one = index.mmr(lists[0], rels[0], 0.6, 25)
    assert np.array_equal(one[0], ids[0]) and np.array_equal(one[3], slots[0])
    assert index.mmr([], [], 0.6, 5)[0].size == 0
    for bad in (dict(k=0), dict(k=257), dict(lam=1.5), dict(lam=-0.1)):
        args = dict(lam=0.5, k=5)
        args.update(bad)
        with pytest.raises(ValueError):
            index.mmr(lists[0], rels[0], args["lam"], args["k"])
    with pytest.raises(ValueError):
        index.mmr(list(range(257)), [0.5] * 257, 0.5, 5)
    with pytest.raises(ValueError):
        index.mmr([1, 2, 3], [0.5, 0.5], 0.5, 2)


TABLE_SEED = 5   # crafted(5) with crafted_query(.., 5): every gap of the first ten picks >= 1e-3 at lambda 0.5 and 0.7


def make_tables():
    """The 40 crafted rows as chunks of 8 calls (one cluster does not follow one call), the first 10 of them as artifact chunks too."""
    from datetime import datetime
    from uuid import UUID
    rows, ids, _ = crafted(TABLE_SEED)
    q = crafted_query(rows, TABLE_SEED)
    n, t0 = len(rows), datetime(2026, 3, 1)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(8)]
    cols = {"chunk_id": ids.tolist(), "call_id": [calls[i % 8]["call_id"] for i in range(n)],
            "text": [f"row {i}" for i in range(n)], "speaker": ["S%d" % (i % 3) for i in range(n)],
            "start_ts_ms": [i * 10 for i in range(n)], "end_ts_ms": [i * 10 + 9 for i in range(n)]}
    chunks = rt.DenseTable("chunks", "chunk_id", dim=1024, capacity=n + 64)
    arts = rt.DenseTable("artifact_chunks", "artifact_chunk_id", dim=1024, capacity=64)
    chunks.add(rows, cols, call_started_at=[t0] * n)
    arts.add(rows[:10], {"artifact_chunk_id": list(range(500, 510)), "call_id": [calls[0]["call_id"]] * 10,
                         "artifact_id": [i // 3 for i in range(10)], "kind": ["summary"] * 10,
                         "content": [f"artifact {i}" for i in range(10)]}, call_started_at=[t0] * 10)
    return chunks, arts, calls, rows, ids, q


def test_through_the_table(gpu):
    """fetch_dense(mmr=) == search -> mmr_host over oracle cosines, composed on the host, under the guard."""
    chunks, arts, calls, rows, ids, q = make_tables()
    try:
        plain = chunks.fetch_dense(q, None, None, "ann", 40, rt.CHUNK_SELECT)
        assert len(plain) == 40
        rel = np.asarray([r["score"] for r in plain], dtype=np.float32)
        listed = np.asarray([r["chunk_id"] for r in plain], dtype=np.int64)
        cos = pair_cosines(ids, rows, listed)
        for lam in (0.5, 0.7):
            slots, _, gaps = mmr_oracle(rel, cos, lam, 10, listed)
            assert gaps.min() >= 1e-3                                       # an assertion on the construction
            host, _ = mmr_host(rel, cos.astype(np.float32), lam, 10, listed)
            assert np.array_equal(host, slots) and not np.array_equal(slots, np.arange(10))
            got = chunks.fetch_dense(q, None, None, "ann", 10, rt.CHUNK_SELECT, mmr=MmrParams(lam=lam))   # fetch 40
            assert [r["chunk_id"] for r in got] == listed[slots].tolist()
            assert np.array_equal(bits([r["score"] for r in got]), bits(rel[slots]))
            assert all(set(r) == set(rt.CHUNK_SELECT) | {"score"} for r in got)
        # lambda = 1 and a fetch of exactly the limit: the plain lane
        same = chunks.fetch_dense(q, None, None, "ann", 10, rt.CHUNK_SELECT, mmr=MmrParams(lam=1.0, fetch=10))
        assert same == plain[:10]
        # the other routes: under a per-call cap the picks come from the capped rows; a small call scope lists its rows
        capped = chunks.fetch_dense(q, None, None, "ann", 8, rt.CHUNK_SELECT, per_call=1, mmr=MmrParams(lam=0.5))
        assert len(capped) == 8 and len({r["call_id"] for r in capped}) == 8
        scoped = chunks.fetch_dense(q, rt.RetrieveFilters(), [calls[0]["call_id"]], "exact", 3, rt.CHUNK_SELECT,
                                    mmr=MmrParams(lam=0.5))
        assert len(scoped) == 3 and all(r["call_id"] == calls[0]["call_id"] for r in scoped)
        assert chunks.fetch_dense(q, rt.RetrieveFilters(), [], "exact", 3, rt.CHUNK_SELECT, mmr=MmrParams(lam=0.5)) == []
    finally:
        chunks.close(); arts.close()


def test_retrieve_evidence_and_the_knob(gpu, monkeypatch):
    from cadence_rag_amd import embeddings
    chunks, arts, calls, rows, ids, q = make_tables()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[q.tolist() for _ in texts], model="m"))
    monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.0)
    monkeypatch.setattr(settings, "dense_per_call_cap", 0)
    monkeypatch.setattr(settings, "rerank_base_url", "")
    monkeypatch.setattr(settings, "dense_mmr_fetch", 0)

    class Before(rt.GpuRetrieveBackend):
        """the dense lanes as they were before the knob existed"""
        def fetch_chunks_dense(self, query_embedding, filters, call_ids, mode, limit):
            return rt._fetch_chunks_dense(self.tables["chunks"], query_embedding, filters, call_ids, mode, limit)

        def fetch_artifacts_dense(self, query_embedding, filters, call_ids, mode, limit):
            return rt._fetch_artifacts_dense(self.tables["artifact_chunks"], query_embedding, filters, call_ids, mode, limit)

    def response(backend):
        out = rt.retrieve_evidence(rt.RetrieveRequest(query="why did the renewal slip", debug=True), backend=backend)
        out.pop("query_id")
        return out

    try:
        be = rt.GpuRetrieveBackend(chunks, arts, calls=calls)
        monkeypatch.setattr(settings, "dense_mmr_lambda", 1.0)
        off = response(be)
        assert off == response(Before(chunks, arts, calls=calls))          # key for key what it was
        assert "dense_mmr_lambda" not in off["notes"]["retrieval"]
        monkeypatch.setattr(settings, "dense_mmr_lambda", 0.5)
        on = response(be)
        assert on["notes"]["retrieval"]["dense_mmr_lambda"] == 0.5
        for side, key in (("chunks", "chunk_id"), ("artifacts", "artifact_chunk_id")):
            a, b = off["debug"]["lanes"][side]["dense"], on["debug"]["lanes"][side]["dense"]
            assert sorted(r[key] for r in a) == sorted(r[key] for r in b) and [r[key] for r in a] != [r[key] for r in b]
            assert {r[key]: r["score"] for r in a} == {r[key]: r["score"] for r in b}     # each row's score is its cosine
            assert a[0][key] == b[0][key]                                                 # the first pick has no penalty
        lane = on["debug"]["lanes"]["chunks"]["dense"]
        rel = np.asarray([r["score"] for r in off["debug"]["lanes"]["chunks"]["dense"]], dtype=np.float32)
        listed = np.asarray([r["chunk_id"] for r in off["debug"]["lanes"]["chunks"]["dense"]], dtype=np.int64)
        slots, _, gaps = mmr_oracle(rel, pair_cosines(ids, rows, listed), 0.5, 10, listed)
        assert gaps.min() >= 1e-3 and [r["chunk_id"] for r in lane[:10]] == listed[slots].tolist()
        on["notes"]["retrieval"].pop("dense_mmr_lambda")
        assert set(on) == set(off) and on["notes"] == off["notes"]
    finally:
        chunks.close(); arts.close()
