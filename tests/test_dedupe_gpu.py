"""Near-duplicate suppression on the GPU (crag_index_dedupe_async) against the fp64 oracle of dedupe_oracle.py, through
the C ABI and its wrappers: DenseIndex, HybridSearcher, DenseTable / GpuRetrieveBackend / retrieve_evidence.

The data keeps every examined pair far from the threshold (clusters at >= 0.97, a rotation chain at 0.95 / 0.805,
everything else <= 0.3; threshold 0.9), each case asserts that on the oracle's matrix first, and under that guard keep,
dup_of and the counts must equal the oracle's exactly; |sim - oracle| <= 1e-4 (the project's score bar)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import settings
from cadence_rag_amd.dense_index import DenseIndex
from dedupe_oracle import dedupe_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TAU = 0.9
N_ROWS = 200          # six full tiles and a ragged seventh
N_CLUSTERS, PER_CLUSTER = 12, 15


class Data:
    """200 rows in shuffled order (members of a cluster lie in different tiles), ids 10 + 3 * position."""

    def __init__(self, dim: int, seed: int) -> None:
        rng = np.random.default_rng(seed)

        def unit(n):
            a = rng.standard_normal((n, dim))
            return a / np.linalg.norm(a, axis=1, keepdims=True)

        rows = []
        for base in unit(N_CLUSTERS):   # base + noise of length 0.1: in-cluster cosines ~0.99
            rows += [(base + 0.1 * e) * rng.uniform(0.2, 5.0) for e in unit(PER_CLUSTER)]
        u, v = unit(2)
        v = v - (v @ u) * u
        v /= np.linalg.norm(v)
        t = np.arccos(0.95)
        chain = [3.0 * u, 0.5 * (np.cos(t) * u + np.sin(t) * v), np.cos(2 * t) * u + np.sin(2 * t) * v]
        twin = unit(1)[0] * 1.7
        special = chain + [twin, twin, np.zeros(dim), np.full(dim, np.nan)]
        rows += special + list(unit(N_ROWS - len(rows) - len(special)))
        rows = np.asarray(rows, dtype=np.float32)
        n_cl = N_CLUSTERS * PER_CLUSTER
        perm = rng.permutation(N_ROWS)
        self.rows = np.ascontiguousarray(rows[perm])
        self.ids = 10 + 3 * np.arange(N_ROWS, dtype=np.int64)
        where = np.empty(N_ROWS, dtype=np.int64)
        where[perm] = np.arange(N_ROWS)
        idof = lambda k: int(self.ids[where[k]])   # noqa: E731
        self.cluster0 = [idof(i) for i in range(5)]
        self.chain = [idof(n_cl + i) for i in range(3)]
        self.twins = [idof(n_cl + 3), idof(n_cl + 4)]
        self.zero, self.nan = idof(n_cl + 5), idof(n_cl + 6)
        self.unstored = [11, 12, 10 + 3 * N_ROWS + 5, 5, 2 ** 40]
        self.rng = rng

    def random_list(self, count: int) -> np.ndarray:
        pool = np.concatenate([self.ids, self.ids, np.asarray(self.unstored + [-1], dtype=np.int64)])
        return self.rng.choice(pool, size=count, replace=count > pool.size // 2)


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


def run(ix: DenseIndex, lists, width: int, tau: float = TAU, with_aux: bool = True):
    """-> out_ids [nq, width], out_counts [nq], dup_of [nq, width], sim [nq, width] (host; the last two None without)"""
    nq = len(lists)
    h = np.full((nq, width), -1, dtype=np.int64)
    for q, l in enumerate(lists):
        h[q, :len(l)] = l
    d_ids = torch.from_numpy(h).to(DEV)
    d_ct = torch.tensor([len(l) for l in lists], dtype=torch.int32, device=DEV)
    out_ids = torch.full((nq, width), -7, dtype=torch.int64, device=DEV)
    out_ct = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    dup = torch.full((nq, width), -7, dtype=torch.int32, device=DEV) if with_aux else None
    sim = torch.full((nq, width), -7.0, dtype=torch.float32, device=DEV) if with_aux else None
    ix.dedupe_async(d_ids, d_ct, tau, out_ids, out_ct, dup, sim, stream=torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    return (out_ids.cpu().numpy(), out_ct.cpu().numpy(), None if dup is None else dup.cpu().numpy(),
            None if sim is None else sim.cpu().numpy())


def guard(cos: np.ndarray, tau: float = TAU) -> None:
    """No examined pair within 1e-3 of the threshold (an assertion on the construction, not a skip)."""
    c = cos[np.isfinite(cos)]
    assert not np.any(np.abs(c - tau) <= 1e-3), "the test data put a pair at the threshold"


def check(ix, stored_ids, rows, lists, width, tau: float = TAU):
    out_ids, out_ct, dup, sim = run(ix, lists, width, tau)
    for q, l in enumerate(lists):
        keep, w_dup, w_sim, cos = dedupe_oracle(stored_ids, rows, l, tau)
        guard(cos, tau)
        n, kept = len(l), np.asarray(l, dtype=np.int64)[keep]
        assert out_ct[q] == kept.size, (q, out_ct[q], kept.size)
        assert np.array_equal(out_ids[q, :kept.size], kept) and np.all(out_ids[q, kept.size:] == -1)
        assert np.array_equal(dup[q, :n], w_dup) and np.all(dup[q, n:] == -1)
        assert np.array_equal(np.isnan(sim[q, :n]), keep) and np.all(np.isnan(sim[q, n:]))
        if (~keep).any():
            assert np.max(np.abs(sim[q, :n][~keep] - w_sim[~keep])) <= 1e-4
    return out_ids, out_ct, dup, sim


@pytest.mark.parametrize("width", [1, 2, 31, 32, 33, 64, 65, 255, 256])
def test_widths(data, index, width):
    lists = [data.random_list(width), data.random_list(max(width - 1, 0)), data.random_list(width // 2)]
    _, out_ct, _, _ = check(index, data.ids, data.rows, lists, width)
    if width >= 64:
        assert out_ct[0] < width    # something was dropped


@pytest.mark.parametrize("nq", [1, 3, 65])
def test_batches_with_ragged_counts(data, index, nq):
    width = 96
    counts = [width, 0, 1, 33, 95][:nq] + [int(c) for c in data.rng.integers(0, width + 1, size=max(nq - 5, 0))]
    check(index, data.ids, data.rows, [data.random_list(c) for c in counts], width)


def test_dim_768(gpu):
    d = Data(768, 9)
    with build(d) as ix:
        check(ix, d.ids, d.rows, [d.random_list(150), d.chain, d.random_list(40)], 150)


def test_chain_is_greedy_over_the_kept_set(data, index):
    a, b, c = data.chain
    _, _, dup, sim = check(index, data.ids, data.rows, [[a, b, c], [c, b, a], [b, a, c], [a, c, b]], 3)
    assert dup[0].tolist() == [-1, 0, -1] and dup[1].tolist() == [-1, 0, -1]   # "any earlier item" would drop c too
    assert dup[2].tolist() == [-1, 0, 0] and dup[3].tolist() == [-1, -1, 0]
    assert abs(sim[0, 1] - 0.95) <= 1e-4


def test_ineligible_items_stay_and_never_suppress(data, index):
    x = data.cluster0[0]
    lst = [data.unstored[0], data.zero, -1, data.nan, x, data.unstored[0], data.zero, data.nan, -1, 2 ** 40, x]
    out_ids, out_ct, dup, _ = check(index, data.ids, data.rows, [lst], 16)
    assert out_ct[0] == 10 and dup[0, :11].tolist() == [-1] * 10 + [4]
    assert out_ids[0, :10].tolist() == lst[:10]


def test_identical_rows_and_repeats(data, index):
    t0, t1 = data.twins
    _, _, dup, sim = check(index, data.ids, data.rows, [[t0, t1], [t1, t1, t0]], 4)
    assert dup[0, 1] == 0 and sim[0, 1] >= 1 - 1e-6
    assert dup[1, :3].tolist() == [-1, 0, 0] and sim[1, 1] >= 1 - 1e-6


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_sim_bits_do_not_depend_on_the_launch(data, index):
    lst = data.random_list(100)
    alone = run(index, [lst], 100)
    many = run(index, [data.random_list(int(c)) for c in data.rng.integers(0, 101, size=40)] + [lst] +
               [data.random_list(100) for _ in range(24)], 100)
    wide = run(index, [lst], 256)
    assert (~np.isnan(alone[3][0])).sum() >= 10
    for other, q in ((many, 40), (wide, 0)):
        assert np.array_equal(alone[2][0], other[2][q, :100])
        assert np.array_equal(bits(alone[3][0]), bits(other[3][q, :100]))
    # deeper in the list: the pair moves to other blocks and lanes
    shifted = run(index, [np.concatenate([np.full(37, 2 ** 40, dtype=np.int64), lst])], 137)
    assert np.array_equal(bits(alone[3][0]), bits(shifted[3][0, 37:]))
    # cos(a, b) and cos(b, a)
    for a in data.cluster0:
        for b in data.cluster0:
            if a != b:
                ab, ba = run(index, [[a, b]], 2), run(index, [[b, a]], 2)
                assert ab[2][0, 1] == 0 and ba[2][0, 1] == 0
                assert bits(ab[3][0, 1]) == bits(ba[3][0, 1])


def test_both_layouts_bit_for_bit(data, index, monkeypatch):
    lists = [data.random_list(256), data.random_list(77), data.chain]
    want = run(index, lists, 256)
    ix = build(data, monkeypatch, mirror=False)
    try:
        assert ix.prefilter_row_bytes() == 4096 and index.prefilter_row_bytes() == 2048
        got = run(ix, lists, 256)
    finally:
        ix.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(bits(got[3]), bits(want[3]))


@pytest.mark.parametrize("mirror", [True, False])
def test_after_edits_equals_a_fresh_build(data, monkeypatch, mirror):
    gone = data.ids[[3, 40, 41, 97, 160]]
    late = np.sort(data.rng.choice(np.setdiff1d(np.arange(N_ROWS), [3, 40, 41, 97, 160]), size=9, replace=False))
    start = np.setdiff1d(np.arange(N_ROWS), late)
    edited = build(data, monkeypatch, mirror, rows=data.rows[start], ids=data.ids[start])
    edited.remove(gone)
    edited.insert(data.rows[late], data.ids[late])
    final = np.setdiff1d(np.arange(N_ROWS), [3, 40, 41, 97, 160])
    fresh = build(data, monkeypatch, mirror, rows=data.rows[final], ids=data.ids[final])
    try:
        lists = [data.random_list(256), data.random_list(90), list(gone) + data.chain]
        got = check(edited, data.ids[final], data.rows[final], lists, 256)
        want = run(fresh, lists, 256)
    finally:
        edited.close(); fresh.close()
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert np.array_equal(bits(got[3]), bits(want[3]))


def test_nullable_outputs(data, index):
    lists = [data.random_list(130), data.random_list(0), data.random_list(64)]
    full, bare = run(index, lists, 130), run(index, lists, 130, with_aux=False)
    assert np.array_equal(full[0], bare[0]) and np.array_equal(full[1], bare[1])


def test_host_convenience(data, index):
    a, b, c = data.chain
    keep, dup, sim = index.dedupe([a, b, c], TAU)
    assert keep.tolist() == [0, 2] and dup.tolist() == [-1, 0, -1] and abs(sim[1] - 0.95) <= 1e-4
    keeps, dups, _ = index.dedupe([[a, b, c], [], data.twins], TAU)
    assert [k.tolist() for k in keeps] == [[0, 2], [], [0]] and dups[2].tolist() == [-1, 0]
    with pytest.raises(ValueError):
        index.dedupe(list(range(257)), TAU)


@pytest.mark.parametrize("width, tau", [(0, TAU), (257, TAU), (8, float("nan")), (8, -1.0), (8, 1.5), (8, float("inf"))])
def test_argument_errors_enqueue_nothing(gpu, data, index, width, tau):
    alloc = max(width, 8)
    d_ids = torch.full((2, alloc), int(data.ids[0]), dtype=torch.int64, device=DEV)
    d_ct = torch.full((2,), min(alloc, 8), dtype=torch.int32, device=DEV)
    outs = [torch.full((2, alloc), -7, dtype=torch.int64, device=DEV), torch.full((2,), -7, dtype=torch.int32, device=DEV),
            torch.full((2, alloc), -7, dtype=torch.int32, device=DEV), torch.full((2, alloc), -7.0, dtype=torch.float32, device=DEV)]
    st = torch.cuda.current_stream(DEV).cuda_stream
    rc = gpu.crag_index_dedupe_async(index._h, d_ids.data_ptr(), d_ct.data_ptr(), 2, width, tau, outs[0].data_ptr(),
                                     outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), ctypes.c_void_p(st))
    assert rc == -1
    torch.cuda.synchronize(DEV)
    assert all(bool((o == -7).all()) for o in outs)
    for kw in ({"nq": -1}, {"ids": None}, {"counts": None}, {"out_ids": None}, {"out_counts": None}):
        args = {"ids": d_ids.data_ptr(), "counts": d_ct.data_ptr(), "nq": 2, "out_ids": outs[0].data_ptr(),
                "out_counts": outs[1].data_ptr()}
        args.update(kw)
        assert gpu.crag_index_dedupe_async(index._h, args["ids"], args["counts"], args["nq"], 8, TAU, args["out_ids"],
                                           args["out_counts"], None, None, ctypes.c_void_p(st)) == -1
    assert gpu.crag_index_dedupe_async(index._h, d_ids.data_ptr(), d_ct.data_ptr(), 0, 8, TAU, outs[0].data_ptr(),
                                       outs[1].data_ptr(), None, None, ctypes.c_void_p(st)) == 0
    torch.cuda.synchronize(DEV)
    assert all(bool((o == -7).all()) for o in outs)


def test_hybrid_searcher(data, index):
    from cadence_rag_amd.fusion import HybridSearcher
    nq = 5
    qv = torch.from_numpy(np.nan_to_num(data.rows[[0, 17, 60, 111, 150]]).astype(np.float32)).to(DEV)
    bm_ids = torch.from_numpy(np.stack([data.random_list(40) for _ in range(nq)])).to(DEV)
    bm_ct = torch.tensor([40, 0, 13, 40, 1], dtype=torch.int32, device=DEV)
    plain = HybridSearcher(index, None, dense_k=50)
    deduped = HybridSearcher(index, None, dense_k=50, dedupe_cosine=TAU)
    st = torch.cuda.current_stream(DEV).cuda_stream
    base = {k: v.cpu().numpy() for k, v in plain.search(qv, bm25=(bm_ids, bm_ct), stream=st).items()}
    got = {k: v.cpu().numpy() for k, v in deduped.search(qv, bm25=(bm_ids, bm_ct), stream=st).items()}
    assert set(base) == {"ids", "scores", "lanes", "counts", "dense_ids", "dense_scores", "dense_counts"}
    assert set(got) == set(base) | {"dup_of", "dup_sim"}
    assert got["ids"].shape == base["ids"].shape == (nq, 90)
    dropped = 0
    for q in range(nq):
        n = int(base["counts"][q])
        keep, dup_of, sim, cos = dedupe_oracle(data.ids, data.rows, base["ids"][q, :n], TAU)
        guard(cos)
        m = int(keep.sum())
        dropped += n - m
        assert got["counts"][q] == m
        assert np.array_equal(got["ids"][q, :m], base["ids"][q, :n][keep]) and np.all(got["ids"][q, m:] == -1)
        assert np.array_equal(got["scores"][q, :m], base["scores"][q, :n][keep]) and np.all(np.isnan(got["scores"][q, m:]))
        assert np.array_equal(got["lanes"][q, :m], base["lanes"][q, :n][keep]) and np.all(got["lanes"][q, m:] == 0)
        assert np.array_equal(got["dup_of"][q, :n], dup_of) and np.all(got["dup_of"][q, n:] == -1)
        assert np.all(np.abs(got["dup_sim"][q, :n][~keep] - sim[~keep]) <= 1e-4)
    assert dropped >= 20
    for key in ("dense_ids", "dense_scores", "dense_counts"):
        assert np.array_equal(got[key], base[key], equal_nan=True)
    again = {k: v.cpu().numpy() for k, v in plain.search(qv, bm25=(bm_ids, bm_ct), stream=st).items()}
    assert all(np.array_equal(again[k], base[k], equal_nan=True) for k in base)
    with pytest.raises(ValueError):
        HybridSearcher(index, None, dense_k=50, dedupe_cosine=TAU).search(qv, bm25=(bm_ids, bm_ct), out_k=257, stream=st)


def test_retrieve_evidence_end_to_end(gpu, data, monkeypatch):
    """retrieve_evidence over GpuRetrieveBackend with the knob at 0.9 == the same request over a CPU composition whose
    dense rows come from the scan oracle and whose dedupe comes from the dedupe oracle; at 0.0 == without the feature."""
    from datetime import datetime, timedelta
    from uuid import UUID

    import oracle as scan_oracle
    from cadence_rag_amd import embeddings
    clean = np.flatnonzero(np.isfinite(data.rows).all(axis=1) & (np.abs(data.rows).sum(axis=1) > 0))
    t0 = datetime(2026, 3, 1)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(40)]

    def make(name, id_field, body, pos, extra):
        n = len(pos)
        cols = {id_field: [int(data.ids[p]) for p in pos], "call_id": [calls[i % 40]["call_id"] for i in range(n)],
                body: [f"{name} row {int(p)}" for p in pos]}
        cols.update(extra(n))
        table = rt.DenseTable(name, id_field, dim=1024, capacity=n + 64)
        table.add(data.rows[pos], cols, call_started_at=[t0 + timedelta(days=i % 6) for i in range(n)])
        return table

    cpos, apos = clean[:150], clean[150:]
    chunks = make("chunks", "chunk_id", "text", cpos, lambda n: {
        "speaker": ["S%d" % (i % 3) for i in range(n)], "start_ts_ms": [i * 10 for i in range(n)],
        "end_ts_ms": [i * 10 + 9 for i in range(n)]})
    arts = make("artifact_chunks", "artifact_chunk_id", "content", apos, lambda n: {
        "artifact_id": [i // 3 for i in range(n)], "kind": ["summary"] * n})
    qvec = (data.rows[cpos[0]] / np.linalg.norm(data.rows[cpos[0]]) +
            data.rows[apos[0]] / np.linalg.norm(data.rows[apos[0]])).astype(np.float32)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec.tolist() for _ in texts], model="m"))
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(settings, "rerank_base_url", "")

    def lexical(table, select, order):   # a fixed "bm25" ranking shared by both backends
        pos_of = table._positions()
        ids = [table.columns[table.id_field][i] for i in order]
        return lambda q, f, c, k: [{col: table.columns[col][pos_of[i]] for col in select} | {"score": 1.0} for i in ids][:k]

    lex_c = lexical(chunks, rt.CHUNK_SELECT, list(range(149, 100, -1)))
    lex_a = lexical(arts, rt.ARTIFACT_SELECT, list(range(len(apos) - 1, -1, -2)))
    dedupe_calls = []

    class CpuBackend(rt.RetrieveBackend):
        def __init__(self, allow_dedupe=True): self.allow = allow_dedupe
        def fetch_chunks_bm25(self, q, f, c, k): return lex_c(q, f, c, k)
        def fetch_artifacts_bm25(self, q, f, c, k): return lex_a(q, f, c, k)
        def estimate_dense_candidates(self, name, f, c): return len(chunks if name == "chunks" else arts)

        def _dense(self, table, pos, select, e, k):
            ids, sc, ct = scan_oracle.exact_topk(rt._parse_vector(e)[None], data.rows[pos], k, mode=scan_oracle.F64)
            return [{col: table.columns[col][int(p)] for col in select} | {"score": float(s)}
                    for p, s in zip(ids[0, :ct[0]], sc[0, :ct[0]])]

        def fetch_chunks_dense(self, e, f, c, mode, k): return self._dense(chunks, cpos, rt.CHUNK_SELECT, e, k)
        def fetch_artifacts_dense(self, e, f, c, mode, k): return self._dense(arts, apos, rt.ARTIFACT_SELECT, e, k)

        def dedupe(self, name, ids, threshold):
            assert self.allow
            pos = cpos if name == "chunks" else apos
            keep, dup_of, sim, cos = dedupe_oracle(data.ids[pos], data.rows[pos], ids, threshold)
            guard(cos, threshold)
            dedupe_calls.append((name, int((~keep).sum())))
            return [(None, None) if k else (int(d), float(s)) for k, d, s in zip(keep, dup_of, sim)]

    class Approx(float):
        def __eq__(self, other): return abs(float(self) - float(other)) <= 1e-4
        __hash__ = float.__hash__

    def rounded(resp):
        resp.pop("query_id")
        for lanes in resp.get("debug", {}).get("lanes", {}).values():
            for row in lanes.get("dense", []):
                row["score"] = Approx(row["score"])
        for pairs in resp.get("debug", {}).get("dedupe", {}).values():
            for pair in pairs:
                pair["cosine"] = Approx(pair["cosine"])
        return resp

    cases = [rt.RetrieveRequest(query="what happened?", debug=True),
             rt.RetrieveRequest(query="what happened?", return_style="ids_only"),
             rt.RetrieveRequest(query="what happened?", debug=True, budget=rt.Budget(max_evidence_items=30, max_total_chars=4000))]
    try:
        gpu_be = rt.GpuRetrieveBackend(chunks, arts, calls=calls, bm25_chunks=lex_c, bm25_artifacts=lex_a)
        monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.0)
        off = [rounded(rt.retrieve_evidence(req, gpu_be)) for req in cases]
        assert off == [rounded(rt.retrieve_evidence(req, CpuBackend(allow_dedupe=False))) for req in cases]
        assert "dedupe" not in off[0]["debug"] and "dedupe_cosine" not in off[0]["notes"]["retrieval"]
        monkeypatch.setattr(settings, "evidence_dedupe_cosine", TAU)
        for req, before in zip(cases, off):
            got, want = rounded(rt.retrieve_evidence(req, gpu_be)), rounded(rt.retrieve_evidence(req, CpuBackend()))
            assert got == want, req
            assert got != before
        assert sum(n for _, n in dedupe_calls) >= 10
        on = rt.retrieve_evidence(cases[0], gpu_be)
        assert on["notes"]["retrieval"]["dedupe_cosine"] == TAU
        assert sum(on["notes"]["retrieval"]["dedupe_dropped"].values()) == sum(len(v) for v in on["debug"]["dedupe"].values()) > 0
        assert chunks.dedupe([], TAU) == [] and chunks.dedupe([7], TAU) == [(None, None)]
    finally:
        chunks.close(); arts.close()
