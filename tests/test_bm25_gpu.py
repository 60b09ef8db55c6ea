"""BM25 lane on the GPU (crag_bm25_lane_host / Bm25Index) against tests/bm25_oracle.py.

Every result is also compared exactly (ids, counts, score bits) with tests/bm25_replay.py, the fp32 restatement of the
header's formula.  Tolerance against the fp64 oracle (derived, not measured): |dscore| <= 2 * (T + 9) * 2^-24 * score, T = distinct known terms of the query; ids
equal the oracle's except for permutations inside a window of that same relative width; exact ties (identical tf..., dl)
come out in ascending id order with identical bits.  See bm25_oracle.tolerance / assert_matches."""
import ctypes

import numpy as np
import pytest
import torch

from bm25_oracle import Bm25Oracle, assert_matches
from bm25_replay import assert_equals_replay, replay_index
from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import RANGE_ROWS, Bm25Index
from cadence_rag_amd.dense_index import DenseIndex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def host(t):
    return [x.cpu().numpy() for x in t]


def check(index, oracle, queries, k, eligible=None, **kw):
    """eligible: None, bool [N] (shared) or bool [nq, N].  Two legs: the fp64 oracle inside its tolerance window (the
    check of the formula), then ids, counts and score bits equal to the fp32 replay (the check of the header's contract:
    one rounding per operation, terms in ascending id) -- every query, no window."""
    mask = stride = None
    if eligible is not None:
        packed = DenseIndex.pack_mask(eligible)
        mask = torch.from_numpy(packed).to(DEV)
        stride = packed.shape[-1] if packed.ndim == 2 else 0
    ids, sc, ct = host(index.search(queries, k, row_mask=mask, mask_stride=stride or 0, **kw))
    assert ids.shape == (len(queries), k) and sc.shape == (len(queries), k) and ct.shape == (len(queries),)
    worst = 0.0
    for q, text in enumerate(queries):
        el = None if eligible is None else (eligible[q] if np.ndim(eligible) == 2 else eligible)
        worst = max(worst, assert_matches(oracle, text, k, ids[q], sc[q], ct[q], el))
    assert_equals_replay(replay_index(index, *index.query_terms(queries), k, eligible), ids, sc, ct, f"k={k}")
    return ids, sc, ct, worst


def zipf_corpus(seed, n_rows, n_terms, lo, hi):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_terms + 1)
    p /= p.sum()
    lens = rng.integers(lo, hi + 1, size=n_rows)
    flat = rng.choice(n_terms, size=int(lens.sum()), p=p)
    words = np.array([f"w{t}" for t in range(n_terms)])
    texts, o = [], 0
    for n in lens:
        texts.append(" ".join(words[flat[o:o + n]]))
        o += n
    return rng, texts, words, p


@pytest.fixture(scope="module")
def zipf(gpu):
    rng, texts, words, p = zipf_corpus(2024, 20000, 5000, 5, 120)
    ids = np.arange(20000, dtype=np.int64) * 3 + 100
    queries = [" ".join(rng.choice(words, size=int(rng.integers(1, 33)), p=p)) for _ in range(64)]
    index = Bm25Index(texts, ids, DEV)
    yield index, Bm25Oracle(texts, ids), queries, texts, ids
    index.close()


REFERENCE_ROWS = ["We saw ECONNRESET in api-gateway.", "Let's roll back version 1.2.3.", "Action item: file ticket ABC-123.",
                  "We saw ECONNRESET in api-gateway and planned rollback."]


def test_reference_sentences(gpu):
    ids = [11, 12, 13, 40]
    index, oracle = Bm25Index(REFERENCE_ROWS, ids, DEV), Bm25Oracle(REFERENCE_ROWS, ids)
    query = "Where did we discuss ECONNRESET in api-gateway?"
    got_ids, got_sc, got_ct, _ = check(index, oracle, [query, "rollback version", "file a ticket"], 10)
    assert got_ids[0, 0] == 11 and got_ct[0] == 2 and got_ids[0, 1] == 40       # the shorter row wins
    assert got_ids[2, 0] == 13 and got_ct[2] == 1
    # through the C ABI directly: the same bits
    lib = _native.load()
    q_ptr, terms, w = index.query_terms([query])
    out_ids = torch.empty(1, 10, dtype=torch.int64, device=DEV)
    out_sc = torch.empty(1, 10, dtype=torch.float32, device=DEV)
    out_ct = torch.empty(1, dtype=torch.int32, device=DEV)
    nbytes = lib.crag_bm25_scratch_bytes(4, 1, 10)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    slot = lib.crag_upload_slot_create()
    try:
        rc = lib.crag_bm25_lane_host(index.d_post_ptr.data_ptr(), index.d_post_pos.data_ptr(), index.d_post_tf.data_ptr(),
                                     index.d_doc_len.data_ptr(), index.d_ids.data_ptr(), 4, index.n_terms,
                                     ctypes.c_float(index.avgdl), q_ptr.ctypes.data, terms.ctypes.data, w.ctypes.data, 1, 10,
                                     None, 0, slot, scratch.data_ptr(), nbytes, out_ids.data_ptr(), out_sc.data_ptr(),
                                     out_ct.data_ptr(), None)
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        lib.crag_upload_slot_destroy(slot)
    assert np.array_equal(out_ids.cpu().numpy()[0], got_ids[0])
    assert np.array_equal(out_sc.cpu().numpy()[0].view(np.uint32), got_sc[0].view(np.uint32))
    assert int(out_ct[0]) == 2
    index.close()


@pytest.mark.parametrize("k", [1, 10, 50, 128])
def test_zipf_corpus_against_the_oracle(zipf, k):
    index, oracle, queries, _, _ = zipf
    *_, worst = check(index, oracle, queries, k)
    print(f"k={k}: worst score error = {worst:.3f} of the single bound (T + 9) * 2^-24")


def test_identical_rows_tie_in_id_order_with_identical_bits(gpu):
    rng, texts, words, p = zipf_corpus(5, 3000, 300, 5, 40)
    twin = "w3 w3 w17 w40 w250 filler filler"
    spots = np.sort(rng.choice(3000, size=200, replace=False))
    for s in spots:
        texts[s] = twin
    ids = np.arange(3000, dtype=np.int64) + 7
    index, oracle = Bm25Index(texts, ids, DEV), Bm25Oracle(texts, ids)
    got_ids, got_sc, got_ct, _ = check(index, oracle, ["w3 w250 w17", "w40"], 128)
    for q in range(2):
        in_list = [j for j in range(int(got_ct[q])) if got_ids[q, j] - 7 in set(spots.tolist())]
        assert len(in_list) >= 100
        assert np.all(np.diff(got_ids[q, in_list]) > 0), "identical rows must ascend by id"
        assert in_list == list(range(in_list[0], in_list[0] + len(in_list))), "identical rows are one run"
        assert len(set(got_sc[q, in_list].view(np.uint32).tolist())) == 1, "identical rows, identical bits"
    index.close()


def test_masks(zipf):
    index, oracle, queries, _, _ = zipf
    rng = np.random.default_rng(9)
    n, qs = 20000, queries[:16]
    check(index, oracle, qs, 50, None)
    check(index, oracle, qs, 50, rng.random(n) < 0.3)
    check(index, oracle, qs, 50, rng.random((16, n)) < 0.5)
    window = np.zeros(n, dtype=bool)
    window[6000:17001] = True                                   # a date filter: one contiguous range of positions
    check(index, oracle, qs, 50, window)
    _, _, ct, _ = check(index, oracle, qs, 50, np.zeros(n, dtype=bool))
    assert np.all(ct == 0)


def test_short_lists_unknown_terms_and_term_counts(zipf):
    index, oracle, queries, texts, ids = zipf
    rare = min(index.vocab, key=lambda tok: index.df[index.vocab[tok]])
    got_ids, got_sc, got_ct, _ = check(index, oracle, [rare, "nosuchterm zzz", "", "?!", rare + " nosuchterm"], 128)
    assert 0 < got_ct[0] < 128 and got_ct[1] == 0 and got_ct[2] == 0 and got_ct[3] == 0 and got_ct[4] == got_ct[0]
    # a repeated query token doubles that term's contribution (qtf = 2): exactly, a power of two
    one = host(index.search(["w7"], 20))
    two = host(index.search(["w7 w7"], 20))
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1] * np.float32(2.0), two[1], equal_nan=True)
    check(index, oracle, ["w7 w7 w9", "w9 w7 w9 w9"], 20)
    # 200 distinct terms in one query; beside it a one-term query
    long_q = " ".join(f"w{t}" for t in range(40, 240))
    check(index, oracle, [long_q, "w5", long_q + " " + long_q], 50)
    check(index, oracle, [" ".join(f"w{t}" for t in range(0, 600))], 128)     # more than one round of terms
    # a term with df = N
    every = [t + " common" for t in texts[:3000]]
    ix2, or2 = Bm25Index(every, ids[:3000], DEV), Bm25Oracle(every, ids[:3000])
    assert ix2.df[ix2.vocab["common"]] == 3000
    check(ix2, or2, ["common", "common w1"], 50)
    ix2.close()


@pytest.mark.parametrize("n", [RANGE_ROWS - 1, RANGE_ROWS, RANGE_ROWS + 1, 3 * RANGE_ROWS + 5])
def test_range_edges(gpu, n):
    """The only matches sit at the first and the last position of every range."""
    texts = ["pad filler"] * n
    planted = sorted({p for r in range(0, n, RANGE_ROWS) for p in (r, min(r + RANGE_ROWS, n) - 1)})
    for j, p in enumerate(planted):
        texts[p] = "needle " * (1 + j % 3) + "x" * (j % 2)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    index, oracle = Bm25Index(texts, ids, DEV), Bm25Oracle(texts, ids)
    got_ids, _, got_ct, _ = check(index, oracle, ["needle", "needle pad"], 16)
    assert got_ct[0] == len(planted) and sorted(got_ids[0, :got_ct[0]].tolist()) == [2 * p + 1 for p in planted]
    last_only = np.zeros(n, dtype=bool)
    last_only[n - 1] = True
    got_ids, _, got_ct, _ = check(index, oracle, ["needle"], 16, last_only)
    assert got_ct[0] == 1 and got_ids[0, 0] == 2 * (n - 1) + 1
    index.close()


@pytest.mark.parametrize("nq", [1, 7, 64])
def test_determinism(zipf, nq):
    index, oracle, queries, _, _ = zipf
    first = host(index.search(queries[:nq], 50))
    again = host(index.search(queries[:nq], 50))
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    a = index.search(queries[:nq], 50, stream=s1.cuda_stream)
    b = index.search(queries[:nq], 50, stream=s2.cuda_stream)
    s1.synchronize(); s2.synchronize()
    whole = host(index.search(queries, 50))
    for other in (again, host(a), host(b), [x[:nq] for x in whole]):     # the batch size does not change a bit either
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[2], other[2])
        assert np.array_equal(first[1].view(np.uint32), other[1].view(np.uint32))


def test_extend_equals_a_fresh_index(zipf):
    _, _, queries, texts, ids = zipf
    grown = Bm25Index(texts[:9000], ids[:9000], DEV)
    before = host(grown.search(queries, 50))
    grown.extend(texts[9000:17000], ids[9000:17000])
    grown.extend(texts[17000:], ids[17000:])
    fresh = Bm25Index(texts, ids, DEV)
    assert grown.vocab == fresh.vocab and grown.avgdl == fresh.avgdl
    got, want = host(grown.search(queries, 50)), host(fresh.search(queries, 50))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert not np.array_equal(before[0], got[0])
    grown.close(); fresh.close()


def test_retrieve_and_hybrid_end_to_end(gpu, monkeypatch):
    """retrieve_evidence over GpuRetrieveBackend with native BM25 lanes == the same request over a CPU composition
    whose BM25 rows come from the oracle (with the dense lane, and lexical-only); HybridSearcher(bm25_index=...) ==
    HybridSearcher fed the oracle's ids."""
    from datetime import datetime, timedelta
    from uuid import UUID

    import oracle as scan_oracle
    from cadence_rag_amd import embeddings
    from cadence_rag_amd.fusion import HybridSearcher
    from helpers import unit_rows
    rng, texts, words, p = zipf_corpus(31, 790, 400, 5, 40)
    t0 = datetime(2026, 3, 1)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(6)]

    def make(name, id_field, body, rows, extra):
        n = len(rows)
        vecs = unit_rows(rng, n)
        cols = {id_field: [1000 + 2 * i for i in range(n)], "call_id": [calls[i % 6]["call_id"] for i in range(n)], body: rows}
        cols.update(extra(n))
        table = rt.DenseTable(name, id_field, dim=1024, capacity=n + 64)
        table.add(vecs, cols, call_started_at=[t0 + timedelta(days=i % 6) for i in range(n)],
                  call_tags={c["call_id"]: ["t%d" % (i % 2)] for i, c in enumerate(calls)})
        return table, vecs

    chunks, cvec = make("chunks", "chunk_id", "text", texts[:700], lambda n: {
        "speaker": ["S%d" % (i % 3) for i in range(n)], "start_ts_ms": [i * 10 for i in range(n)],
        "end_ts_ms": [i * 10 + 9 for i in range(n)]})
    arts, avec = make("artifact_chunks", "artifact_chunk_id", "content", texts[700:], lambda n: {
        "artifact_id": [i // 3 for i in range(n)], "kind": ["summary"] * n})
    qvec = (cvec[77] + 0.5 * avec[5]).astype(np.float32)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec.tolist() for _ in texts], model="m"))
    oracles = {}

    def oracle_of(table, body):   # follows the table (rows are appended below)
        key = (table.name, len(table))
        if key not in oracles:
            oracles[key] = Bm25Oracle(table.columns[body], table.columns[table.id_field])
        return oracles[key]

    class CpuBackend(rt.RetrieveBackend):
        def resolve_call_ids(self, filters): return rt._resolve_call_ids(calls, filters)

        def _mask(self, table, f, c):
            m = table.filter_mask(f, c)
            return np.ones(len(table), bool) if m is None else m

        def _bm25(self, table, body, select, q, f, c, k):
            ids, sc, n = oracle_of(table, body).topk(q, k, self._mask(table, f, c))
            pos = table._positions()
            return [{col: table.columns[col][pos[int(i)]] for col in select} | {"score": float(s)}
                    for i, s in zip(ids[:n], sc[:n])]

        def fetch_chunks_bm25(self, q, f, c, k): return self._bm25(chunks, "text", rt.CHUNK_SELECT, q, f, c, k)
        def fetch_artifacts_bm25(self, q, f, c, k): return self._bm25(arts, "content", rt.ARTIFACT_SELECT, q, f, c, k)

        def estimate_dense_candidates(self, name, f, c):
            return int(self._mask(chunks if name == "chunks" else arts, f, c).sum())

        def _dense(self, table, vecs, select, e, f, c, k):
            ids, sc, ct = scan_oracle.exact_topk(rt._parse_vector(e)[None], vecs, k,
                                                 mask=np.packbits(self._mask(table, f, c), bitorder="little"),
                                                 mode=scan_oracle.F64)
            return [{col: table.columns[col][int(p)] for col in select} | {"score": float(s)}
                    for p, s in zip(ids[0, :ct[0]], sc[0, :ct[0]])]

        def fetch_chunks_dense(self, e, f, c, mode, k): return self._dense(chunks, cvec, rt.CHUNK_SELECT, e, f, c, k)
        def fetch_artifacts_dense(self, e, f, c, mode, k): return self._dense(arts, avec, rt.ARTIFACT_SELECT, e, f, c, k)

    class Approx(float):
        """A lane score in a debug listing: fp32 on the GPU side, fp64 on the other."""
        def __eq__(self, other): return abs(float(self) - float(other)) <= 1e-5 * max(abs(float(self)), 1.0)
        __hash__ = float.__hash__

    def rounded(resp):
        resp.pop("query_id")
        for lanes in resp.get("debug", {}).get("lanes", {}).values():
            for lane in ("dense", "bm25"):
                for row in lanes.get(lane, []):
                    row["score"] = Approx(row["score"])
        return resp

    try:
        gpu_be = rt.GpuRetrieveBackend(chunks, arts, calls=calls, bm25_chunks=chunks.build_bm25_lane("text"),
                                       bm25_artifacts=arts.build_bm25_lane("content"))
        cases = [
            rt.RetrieveRequest(query="what about w3 and w17 in w40?", debug=True),
            rt.RetrieveRequest(query="w1 w2 w5 w8", return_style="ids_only"),
            rt.RetrieveRequest(query="w11 w2 status", debug=True, return_style="ids_only",
                               filters=rt.RetrieveFilters(call_ids=[calls[1]["call_id"], calls[4]["call_id"]])),
            rt.RetrieveRequest(query="w9 w30 w4", debug=True,
                               filters=rt.RetrieveFilters(date_from=t0 + timedelta(days=2), call_tags=["t1"]),
                               budget=rt.Budget(max_evidence_items=5, max_total_chars=300)),
            rt.RetrieveRequest(query="nothing from the vocabulary", debug=True),
        ]
        for dense_on in (True, False):
            monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: dense_on)
            for req in cases:
                got, want = rounded(rt.retrieve_evidence(req, gpu_be)), rounded(rt.retrieve_evidence(req, CpuBackend()))
                assert got == want, (dense_on, req)
            if not dense_on:   # the reference's lexical-only operating mode
                resp = rt.retrieve_evidence(cases[0], gpu_be)
                assert resp["notes"]["retrieval"]["planner"] == "lexical_only" and resp["quotes"]
        # rows appended behind the lane's: the backend extends it
        more = [f"w3 w17 w40 fresh row {i}" for i in range(5)]
        chunks.add(unit_rows(rng, 5), {"chunk_id": [5000 + i for i in range(5)], "call_id": [calls[0]["call_id"]] * 5,
                                       "text": more, "speaker": ["S0"] * 5, "start_ts_ms": [0] * 5, "end_ts_ms": [9] * 5},
                   call_started_at=[t0] * 5)
        cvec = np.concatenate([cvec, np.zeros((5, 1024), np.float32)])   # (lexical-only below: the vectors are not read)
        lane_before = gpu_be._bm25["chunks"]
        got, want = rounded(rt.retrieve_evidence(cases[0], gpu_be)), rounded(rt.retrieve_evidence(cases[0], CpuBackend()))
        assert got == want and gpu_be._bm25["chunks"] is lane_before and len(lane_before) == 705
        assert any(q["chunk_id"] >= 5000 for q in got["quotes"])

        # HybridSearcher: the native lane beside the other two == the oracle's ids handed in
        qtexts = ["w3 w17 w40", "w1 w2", "nothing known", "w9 w9 w30 w4 w100 w7"]
        qv = torch.from_numpy(unit_rows(rng, 4)).to(DEV)
        orc = oracle_of(chunks, "text")
        want_ids = np.stack([orc.topk(t, 50)[0] for t in qtexts])
        want_ct = np.array([orc.topk(t, 50)[2] for t in qtexts], dtype=np.int32)
        native = HybridSearcher(chunks.index, None, dense_k=50, bm25_index=gpu_be._bm25["chunks"], bm25_k=50)
        fed = HybridSearcher(chunks.index, None, dense_k=50)
        a = {k: v.cpu().numpy() for k, v in native.search(qv, query_texts=qtexts).items()}
        b = {k: v.cpu().numpy() for k, v in fed.search(qv, bm25=(torch.from_numpy(want_ids).to(DEV),
                                                                torch.from_numpy(want_ct).to(DEV))).items()}
        assert np.array_equal(a["bm25_ids"], want_ids) and np.array_equal(a["bm25_counts"], want_ct)
        for key in ("ids", "lanes", "counts", "dense_ids"):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a["scores"], b["scores"], equal_nan=True)
        # a `bm25` handed in wins over the native lane
        c = native.search(qv, query_texts=qtexts, bm25=(torch.from_numpy(want_ids[:, :5].copy()).to(DEV),
                                                        torch.from_numpy(np.minimum(want_ct, 5)).to(DEV)))
        assert "bm25_ids" not in c and c["ids"].shape[1] == 55
    finally:
        for lane in (getattr(locals().get("gpu_be"), "_bm25", {}) or {}).values():
            if hasattr(lane, "close"):
                lane.close()
        chunks.close(); arts.close()
