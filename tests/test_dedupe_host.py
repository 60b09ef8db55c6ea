"""Near-duplicate suppression without a GPU: the oracle on hand-checkable cases, the C entry point's NULL check and the
dedupe stage of retrieve_evidence over a fake backend."""
from __future__ import annotations

from uuid import UUID

import numpy as np
import pytest

from cadence_rag_amd import reranker, retrieve
from cadence_rag_amd.config import Settings, settings
from dedupe_oracle import dedupe_oracle

TAU = 0.9


def chain_rows(dim=8):
    """a, b, c: a unit vector rotated in a plane by 0, t and 2t with cos t = 0.95 (cos 2t = 0.805)."""
    t = np.arccos(0.95)
    u, v = np.eye(dim)[0], np.eye(dim)[1]
    return np.stack([np.cos(k * t) * u + np.sin(k * t) * v for k in range(3)])


def test_oracle_chain_keeps_the_ends():
    rows = chain_rows()
    keep, dup_of, sim, cos = dedupe_oracle([5, 6, 7], rows, [5, 6, 7], TAU)
    assert cos[0, 1] == pytest.approx(0.95) and cos[1, 2] == pytest.approx(0.95) and cos[0, 2] == pytest.approx(0.805)
    assert keep.tolist() == [True, False, True] and dup_of.tolist() == [-1, 0, -1]
    assert sim[1] == pytest.approx(0.95) and np.isnan(sim[0]) and np.isnan(sim[2])
    # c first: b is its duplicate, a stays
    keep, dup_of, _, _ = dedupe_oracle([5, 6, 7], rows, [7, 6, 5], TAU)
    assert keep.tolist() == [True, False, True] and dup_of.tolist() == [-1, 0, -1]
    # b first: it takes both neighbours
    keep, dup_of, _, _ = dedupe_oracle([5, 6, 7], rows, [6, 5, 7], TAU)
    assert keep.tolist() == [True, False, False] and dup_of.tolist() == [-1, 0, 0]


def test_oracle_unstored_zero_and_repeats():
    rows = np.concatenate([chain_rows(), np.zeros((1, 8)), np.full((1, 8), np.nan)])
    stored = [5, 6, 7, 8, 9]
    # unstored ids and the pad are kept, even repeated, and suppress nothing
    keep, dup_of, sim, cos = dedupe_oracle(stored, rows, [100, 5, -1, 100, -1, 6], TAU)
    assert keep.tolist() == [True, True, True, True, True, False] and dup_of[5] == 1
    assert np.isnan(cos[0]).all() and np.isnan(cos[:, 2]).all()
    # a zero row and a NaN row: kept, never a suppressor, also of themselves
    keep, dup_of, _, _ = dedupe_oracle(stored, rows, [8, 9, 8, 9, 5], TAU)
    assert keep.all() and (dup_of == -1).all()
    # a stored, eligible row repeated has cosine 1 with itself; scaling a row changes nothing
    rows[2] *= 1e-3
    keep, dup_of, sim, _ = dedupe_oracle(stored, rows, [7, 5, 7, 7], TAU)
    assert keep.tolist() == [True, True, False, False] and dup_of.tolist() == [-1, -1, 0, 0]
    assert sim[2] == pytest.approx(1.0, abs=1e-12)
    assert dedupe_oracle(stored, rows, [], TAU)[0].size == 0


def test_null_index_is_einval(native_lib):
    assert native_lib.crag_index_dedupe_async(None, None, None, 1, 8, 0.9, None, None, None, None, None) == -1
    assert b"NULL" in native_lib.crag_last_error()


def test_setting_default_and_env(monkeypatch):
    assert Settings().evidence_dedupe_cosine == 0.0
    monkeypatch.setenv("EVIDENCE_DEDUPE_COSINE", "0.92")
    assert Settings.from_env().evidence_dedupe_cosine == 0.92


# ---- retrieve_evidence ------------------------------------------------------------------------------------------
def _chunk(i):   # (a call each: the per-call quota stays out of the way)
    return {"chunk_id": i, "call_id": UUID(int=i), "speaker": "S", "start_ts_ms": i, "end_ts_ms": i + 1, "text": f"chunk {i}"}


def _artifact(i):
    return {"artifact_chunk_id": i, "artifact_id": i // 2, "call_id": UUID(int=i), "kind": "summary", "content": f"artifact {i}"}


class _FakeBackend(retrieve.RetrieveBackend):
    """bm25 lanes only; `dedupe` says that chunk 12 restates chunk 11."""

    def __init__(self):
        self.dedupe_calls = []

    def fetch_chunks_bm25(self, query, filters, call_ids, limit):
        return [dict(_chunk(i), score=1.0 / i) for i in (10, 11, 12, 13)]

    def fetch_artifacts_bm25(self, query, filters, call_ids, limit):
        return [dict(_artifact(i), score=1.0 / i) for i in (20, 21)]

    def dedupe(self, table_name, ids, threshold):
        self.dedupe_calls.append((table_name, list(ids), threshold))
        return [(ids.index(11), 0.97) if i == 12 else (None, None) for i in ids]


class _Stub:
    def __init__(self):
        self.docs = []

    def rerank(self, query, documents):
        self.docs.append(list(documents))
        scores = [1.0 - 0.01 * i for i in range(len(documents))]
        return np.asarray(scores, dtype=np.float32), list(range(len(documents))), "stub"


@pytest.fixture
def no_dense(monkeypatch):
    from cadence_rag_amd import embeddings
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: False)


def test_retrieve_drops_the_duplicate_in_front_of_the_reranker(monkeypatch, no_dense):
    monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.9)
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    stub = _Stub()
    reranker.set_reranker(stub)
    try:
        be = _FakeBackend()
        resp = retrieve.retrieve_evidence(retrieve.RetrieveRequest(query="anything", debug=True), be)
        ids_only = retrieve.retrieve_evidence(retrieve.RetrieveRequest(query="anything", return_style="ids_only"), be)
    finally:
        reranker.set_reranker(None)
    assert [q["chunk_id"] for q in resp["quotes"]] == [10, 11, 13]
    assert [a["artifact_chunk_id"] for a in resp["artifacts"]] == [20, 21]
    assert "chunk:12" not in ids_only["retrieved_ids"] and "chunk:11" in ids_only["retrieved_ids"]
    assert len(ids_only["retrieved_ids"]) == 5
    assert all("chunk 12" not in docs for docs in stub.docs) and any("chunk 11" in docs for docs in stub.docs)
    notes = resp["notes"]["retrieval"]
    assert notes["dedupe_cosine"] == 0.9 and notes["dedupe_dropped"] == {"chunks": 1, "artifact_chunks": 0}
    assert notes["reranked_from"] == 5
    assert resp["debug"]["dedupe"] == {"chunks": [{"dropped": 12, "kept": 11, "cosine": 0.97}], "artifacts": []}
    assert ("chunks", [10, 11, 12, 13], 0.9) in be.dedupe_calls and ("artifact_chunks", [20, 21], 0.9) in be.dedupe_calls


def test_retrieve_with_the_knob_off_is_untouched(monkeypatch, no_dense):
    monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.0)
    monkeypatch.setattr(settings, "rerank_base_url", "")
    be = _FakeBackend()
    resp = retrieve.retrieve_evidence(retrieve.RetrieveRequest(query="anything", debug=True), be)
    assert be.dedupe_calls == []
    assert [q["chunk_id"] for q in resp["quotes"]] == [10, 11, 12, 13]
    assert "dedupe_cosine" not in resp["notes"]["retrieval"] and "dedupe_dropped" not in resp["notes"]["retrieval"]
    assert "dedupe" not in resp["debug"]


def test_only_the_first_256_rows_are_examined(monkeypatch, no_dense):
    monkeypatch.setattr(settings, "evidence_dedupe_cosine", 0.9)
    monkeypatch.setattr(settings, "rerank_base_url", "")

    class Many(_FakeBackend):
        def fetch_chunks_bm25(self, query, filters, call_ids, limit):
            return [dict(_chunk(i), score=1.0) for i in range(1, 301)]

        def fetch_artifacts_bm25(self, query, filters, call_ids, limit):
            return []

    be = Many()
    ids = retrieve.retrieve_evidence(retrieve.RetrieveRequest(query="q", return_style="ids_only"), be)["retrieved_ids"]
    assert [c for c in be.dedupe_calls if c[0] == "chunks"][0][1] == list(range(1, 257))
    assert len(ids) == 299 and "chunk:12" not in ids and ids[-1] == "chunk:300"


def test_default_backend_drops_nothing():
    assert retrieve.RetrieveBackend().dedupe("chunks", [1, 2, 3], 0.9) == [(None, None)] * 3
