"""The clause syntax of the BM25 lane end to end on the GPU: Bm25Index.search_query against the fp32
replay (tests/bm25_replay.py) of the scored bag under the clause oracle's mask (tests/bm25_clause_oracle.py), and
retrieve_evidence over a GpuRetrieveBackend with settings.bm25_query_syntax on and off.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from bm25_clause_oracle import ClauseOracle, arrays_from_rows, clauses_of, random_corpus, random_queries
from bm25_replay import NAN_BITS, assert_equals_replay, replay_index
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.bm25 import Bm25Index, parse_query, tokenize
from cadence_rag_amd.dense_index import DenseIndex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

WORDS = ["connection", "reset", "timeout", "staging", "prod", "deploy", "rollback", "gateway", "error", "retry", "the", "a",
         "we", "saw", "after", "in"]
TEXT_QUERIES = ['"connection reset" -staging', '+timeout -staging "connection reset"', 'connection reset',
                '+gateway error retry', '-the deploy rollback', '"we saw" "the gateway" error', '-"connection reset" reset',
                '"connection reset" "reset connection"', 'plain words only', '+deploy +rollback -prod -"a the"',
                '"saw the error" retry', '-staging -prod', '+nosuchword timeout', '-nosuchword timeout',
                '"timeout nosuchword" timeout', '"retry"']


def text_corpus(n=200, seed=8):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(WORDS) + 1) ** 0.7
    p /= p.sum()
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 13)), p=p)) for _ in range(n)]
    texts[17] = "we saw a connection reset in prod"
    texts[18] = "connection was reset in staging after the connection reset"
    texts[19] = "reset the connection"
    return texts


@pytest.fixture(scope="module")
def text_index(gpu):
    texts = text_corpus()
    ids = np.arange(len(texts), dtype=np.int64) * 2 + 500
    ix = Bm25Index(texts, ids, DEV, positions=True)
    yield ix, ClauseOracle([[ix.vocab[t] for t in tokenize(text)] for text in texts]), TEXT_QUERIES
    ix.close()


@pytest.fixture(scope="module")
def random_index(gpu):
    rows = random_corpus()
    row_ptr, terms, tfs, pair_off, pair_where = arrays_from_rows(rows)
    ix = Bm25Index.from_arrays(row_ptr, terms, tfs, 50, np.arange(len(rows), dtype=np.int64) * 3 + 7, DEV,
                               pair_off=pair_off, pair_where=pair_where)
    yield ix, ClauseOracle(rows), random_queries(rows)
    ix.close()


def check(ix, oracle, queries, k, eligible=None):
    """search_query == the replay of the scored bag with eligible = the oracle's mask (and the filter)."""
    parsed = [parse_query(q) for q in queries]
    want_mask = oracle.mask([clauses_of(p, ix.vocab.get) for p in parsed], eligible)
    mask = stride = None
    if eligible is not None:
        pk = DenseIndex.pack_mask(eligible)
        mask, stride = torch.from_numpy(pk).to(DEV), (pk.shape[-1] if pk.ndim == 2 else 0)
    ids, sc, ct = [x.cpu().numpy() for x in ix.search_query(queries, k, row_mask=mask, mask_stride=stride or 0)]
    assert ids.shape == (len(queries), k) and sc.shape == (len(queries), k) and ct.shape == (len(queries),)
    bags = ix.query_terms([" ".join(p.bag) for p in parsed])
    assert_equals_replay(replay_index(ix, *bags, k, want_mask), ids, sc, ct, f"k={k}")
    bits = sc.view(np.uint32)
    for q in range(len(queries)):
        assert np.all(ids[q, ct[q]:] == -1) and np.all(bits[q, ct[q]:] == NAN_BITS)
    return ids, sc, ct


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("which", ["text", "random"])
def test_search_query_equals_the_replay_under_the_oracles_mask(text_index, random_index, which, k):
    ix, oracle, queries = text_index if which == "text" else random_index
    rng = np.random.default_rng(k)
    _, _, ct = check(ix, oracle, queries, k)
    assert (ct > 0).sum() >= len(queries) // 2
    check(ix, oracle, queries, k, rng.random(len(ix)) < 0.6)                      # a shared filter mask
    check(ix, oracle, queries, k, rng.random((len(queries), len(ix))) < 0.6)      # one per query
    check(ix, oracle, queries[:1], k)


def test_queries_without_syntax_are_search(text_index, monkeypatch):
    ix, _, _ = text_index

    def no_clause_launch(parsed):
        raise AssertionError("a batch without constraints must not reach the clause launch")
    monkeypatch.setattr(ix, "clause_arrays", no_clause_launch)
    queries = ["connection reset", "the gateway error-retry", "nothing known here", "", "field:staging (deploy)*"]
    mask = torch.from_numpy(DenseIndex.pack_mask(np.arange(len(ix)) % 3 != 0)).to(DEV)
    for kw in (dict(), dict(row_mask=mask, mask_stride=0)):
        a = [x.cpu().numpy() for x in ix.search_query(queries, 20, **kw)]
        b = [x.cpu().numpy() for x in ix.search(queries, 20, **kw)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_excluded_only_and_unknown_required_return_nothing(text_index):
    ix, _, _ = text_index
    ids, sc, ct = [x.cpu().numpy() for x in ix.search_query(['-staging -"connection reset"', '+nosuchword connection reset',
                                                             '"connection nosuchword" reset', 'connection -nosuchword'], 10)]
    assert ct.tolist()[:3] == [0, 0, 0] and ct[3] > 0
    assert np.all(ids[:3] == -1) and np.all(sc[:3].view(np.uint32) == NAN_BITS)
    plain = ix.search(["connection"], 10)
    assert np.array_equal(ids[3], plain[0].cpu().numpy()[0])                      # the excluded unknown token is dropped
    assert np.array_equal(sc[3].view(np.uint32), plain[1].cpu().numpy()[0].view(np.uint32))


def test_a_phrase_needs_positions(gpu):
    ix = Bm25Index(text_corpus(40), np.arange(40), DEV)
    try:
        with pytest.raises(ValueError, match="positions"):
            ix.search_query(['"connection reset"'], 5)
        ids, _, ct = ix.search_query(["+connection -reset"], 5)                   # term clauses do not
        assert int(ct[0]) == int((ids[0] >= 0).sum())
    finally:
        ix.close()


def test_extend_keeps_the_positions_on_the_device(gpu):
    texts = text_corpus(120)
    grown = Bm25Index(texts[:70], np.arange(70), DEV, positions=True)
    fresh = Bm25Index(texts, np.arange(120), DEV, positions=True)
    try:
        grown.search_query(TEXT_QUERIES[:4], 10)                                  # (allocates the stream's mask buffer)
        grown.extend(texts[70:], np.arange(70, 120))
        a = [x.cpu().numpy() for x in grown.search_query(TEXT_QUERIES, 10)]
        b = [x.cpu().numpy() for x in fresh.search_query(TEXT_QUERIES, 10)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    finally:
        grown.close(); fresh.close()


# ---- retrieve_evidence ------------------------------------------------------------------------------------------------
def test_retrieve_evidence_with_the_syntax_on_and_off(gpu, monkeypatch):
    """retrieve_evidence over a GpuRetrieveBackend with native word lanes == the same request over a CPU composition
    whose BM25 rows are the fp32 replay's: under the oracle's clause mask with the syntax on, the plain bag with it off."""
    from datetime import datetime, timedelta
    from uuid import UUID

    import oracle as scan_oracle
    from cadence_rag_amd import embeddings
    from helpers import unit_rows
    rng = np.random.default_rng(21)
    texts = text_corpus(200)
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

    chunks, cvec = make("chunks", "chunk_id", "text", texts[:150], lambda n: {
        "speaker": ["S%d" % (i % 3) for i in range(n)], "start_ts_ms": [i * 10 for i in range(n)],
        "end_ts_ms": [i * 10 + 9 for i in range(n)]})
    arts, avec = make("artifact_chunks", "artifact_chunk_id", "content", texts[150:], lambda n: {
        "artifact_id": [i // 3 for i in range(n)], "kind": ["summary"] * n})
    qvec = (cvec[77] + 0.5 * avec[5]).astype(np.float32)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec.tolist() for _ in texts], model="m"))
    gpu_be = None
    try:
        gpu_be = rt.GpuRetrieveBackend(chunks, arts, calls=calls, bm25_chunks=chunks.build_bm25_lane("text", positions=True),
                                       bm25_artifacts=arts.build_bm25_lane("content", positions=True))
        lanes = {"chunks": gpu_be._bm25["chunks"], "artifact_chunks": gpu_be._bm25["artifact_chunks"]}
        assert all(lane.positions for lane in lanes.values())
        oracles = {name: ClauseOracle([[lane.vocab[t] for t in tokenize(text)]
                                       for text in (chunks if name == "chunks" else arts).columns[lane.text_column]])
                   for name, lane in lanes.items()}
        syntax = {"on": False}

        class CpuBackend(rt.RetrieveBackend):
            def resolve_call_ids(self, filters): return rt._resolve_call_ids(calls, filters)

            def _mask(self, table, f, c):
                m = table.filter_mask(f, c)
                return np.ones(len(table), bool) if m is None else m

            def _bm25(self, table, select, q, f, c, k):
                lane, eligible, bag = lanes[table.name], self._mask(table, f, c), q
                if syntax["on"]:
                    try:
                        parsed = parse_query(q)
                        eligible = oracles[table.name].passes(clauses_of(parsed, lane.vocab.get), eligible)
                        bag = " ".join(parsed.bag)
                    except ValueError:            # over the limits: the bag reading of the raw string
                        pass
                ids, bits, n = replay_index(lane, *lane.query_terms([bag]), k, eligible)
                pos = table._positions()
                return [{col: table.columns[col][pos[int(i)]] for col in select} | {"score": float(s)}
                        for i, s in zip(ids[0, :n[0]], bits[0, :n[0]].view(np.float32))]

            def fetch_chunks_bm25(self, q, f, c, k): return self._bm25(chunks, rt.CHUNK_SELECT, q, f, c, k)
            def fetch_artifacts_bm25(self, q, f, c, k): return self._bm25(arts, rt.ARTIFACT_SELECT, q, f, c, k)

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
            """A dense lane score in a debug listing: fp32 on the GPU side, fp64 on the other."""
            def __eq__(self, other): return abs(float(self) - float(other)) <= 1e-5 * max(abs(float(self)), 1.0)
            __hash__ = float.__hash__

        def rounded(resp):
            resp.pop("query_id")
            for by_lane in resp.get("debug", {}).get("lanes", {}).values():
                for row in by_lane.get("dense", []):
                    row["score"] = Approx(row["score"])
            return resp

        over = " ".join(f"+{w}" for w in WORDS) + " +connection"                  # 17 required terms
        cases = [
            rt.RetrieveRequest(query='"connection reset" -staging', debug=True),
            rt.RetrieveRequest(query='+timeout -the gateway error', debug=True, return_style="ids_only"),
            rt.RetrieveRequest(query='"we saw" retry -prod', debug=True,
                               filters=rt.RetrieveFilters(call_ids=[calls[1]["call_id"], calls[4]["call_id"]])),
            rt.RetrieveRequest(query='-"the gateway" gateway deploy', debug=True,
                               filters=rt.RetrieveFilters(date_from=t0 + timedelta(days=2), call_tags=["t1"])),
            rt.RetrieveRequest(query="plain words about the connection", debug=True),
            rt.RetrieveRequest(query=over, debug=True),
        ]
        responses = {}
        for on in (True, False):
            monkeypatch.setattr(rt.settings, "bm25_query_syntax", on)
            syntax["on"] = on
            for dense_on in (True, False):
                monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: dense_on)
                for i, req in enumerate(cases):
                    got, want = rounded(rt.retrieve_evidence(req, gpu_be)), rounded(rt.retrieve_evidence(req, CpuBackend()))
                    assert got == want, (on, dense_on, req)
                    responses[on, dense_on, i] = got
        # the syntax changes the answer where the query uses it, and only there
        assert responses[True, False, 0] != responses[False, False, 0]
        ids_on = [q["chunk_id"] for q in responses[True, False, 0]["quotes"]]
        assert ids_on and all("connection reset" in texts[(i - 1000) // 2] and "staging" not in texts[(i - 1000) // 2]
                              for i in ids_on)
        assert responses[True, False, 4] == responses[False, False, 4]
        assert responses[True, False, 5] == responses[False, False, 5]            # over the clause limit: the bag response
    finally:
        for lane in (getattr(gpu_be, "_bm25", {}) or {}).values():
            if hasattr(lane, "close"):
                lane.close()
        chunks.close(); arts.close()
