"""Host side of the reranker: the model card's token ids, the shared-prefix plan, the parent-aware batch layout,
the client seam (native and HTTP), POST /rerank and the rerank stage of retrieve_evidence.  No GPU."""
from __future__ import annotations

import json
from pathlib import Path
from uuid import UUID

import numpy as np
import pytest
import torch

from cadence_rag_amd import reranker, retrieve
from cadence_rag_amd.config import Settings, settings
from cadence_rag_amd.encoder import rerank as R
from cadence_rag_amd.encoder.qwen3 import PackedBatch
from cadence_rag_amd.reranker import RerankClientError

QUERY = "why did the api gateway fail after the upgrade?"
DOCS = ["the customer called about a failed deployment of the api gateway",
        "  leading whitespace: we saw ECONNRESET errors",
        ", a comma first",
        "<Document>: looks like a marker",
        "yes",
        ""]


@pytest.fixture(scope="module")
def tok():
    from tiny_reranker_checkpoint import build_tokenizer
    return build_tokenizer()


def _card_ids(tok, query, docs, instruction=R.DEFAULT_INSTRUCTION, max_length=1024):
    """The Qwen3-Reranker model card's process_inputs, applied with the tokenizer directly."""
    prefix_tokens = tok.encode(R.PREFIX, add_special_tokens=False)
    suffix_tokens = tok.encode(R.SUFFIX, add_special_tokens=False)
    pairs = [f"<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {d}" for d in docs]
    inputs = tok(pairs, padding=False, truncation="longest_first", return_attention_mask=False,
                 max_length=max_length - len(prefix_tokens) - len(suffix_tokens))
    return [prefix_tokens + ele + suffix_tokens for ele in inputs["input_ids"]]


def test_template_strings_are_the_model_cards():
    assert R.PREFIX == ("<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and "
                        "the Instruct provided. Note that the answer can only be \"yes\" or \"no\".<|im_end|>\n"
                        "<|im_start|>user\n")
    assert R.SUFFIX == "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
    assert R.DEFAULT_INSTRUCTION == "Given a web search query, retrieve relevant passages that answer the query"


def test_token_ids_follow_the_model_card(tok):
    assert R.canonical_ids(tok, QUERY, DOCS, R.DEFAULT_INSTRUCTION, 1024) == _card_ids(tok, QUERY, DOCS)
    assert R.canonical_ids(tok, QUERY, DOCS, "find errors", 1024) == _card_ids(tok, QUERY, DOCS, "find errors")
    ids = R.canonical_ids(tok, QUERY, DOCS, R.DEFAULT_INSTRUCTION, 1024)
    assert ids[0][0] == tok.get_vocab()["<|im_start|>"]


def test_truncation_cuts_the_document_tail_deterministically(tok):
    long_doc = " ".join(["the agent confirmed the refund and scheduled a call back"] * 200)
    max_length = 300
    a = R.canonical_ids(tok, QUERY, [long_doc], R.DEFAULT_INSTRUCTION, max_length)
    b = R.canonical_ids(tok, QUERY, [long_doc], R.DEFAULT_INSTRUCTION, max_length)
    assert a == b == _card_ids(tok, QUERY, [long_doc], max_length=max_length)
    assert len(a[0]) == max_length
    n_pre = len(tok.encode(R.PREFIX, add_special_tokens=False))
    n_suf = len(tok.encode(R.SUFFIX, add_special_tokens=False))
    full_pair = tok.encode(f"<Instruct>: {R.DEFAULT_INSTRUCTION}\n<Query>: {QUERY}\n<Document>: {long_doc}",
                           add_special_tokens=False)
    body = a[0][n_pre:len(a[0]) - n_suf]
    assert body == full_pair[:len(body)]          # the head of the pair (instruction, query) is intact; the tail went
    assert a[0][-n_suf:] == tok.encode(R.SUFFIX, add_special_tokens=False)


@pytest.mark.parametrize("docs", [DOCS, DOCS[1:3], [" x"], ["?!"], ["a", "a"], ["same doc", "same doc", "same dog"]])
def test_shared_prefix_is_the_longest_common_id_prefix(tok, docs):
    ids = R.canonical_ids(tok, QUERY, docs, R.DEFAULT_INSTRUCTION, 1024)
    p = R.shared_prefix_len(ids)
    assert all(p < len(tl) for tl in ids)                         # every child keeps a token
    assert all(ids[0][:p] + tl[p:] == tl for tl in ids)           # prefix + child == canonical
    if len(ids) > 1 and p < min(len(tl) for tl in ids) - 1:       # not capped: the next id differs somewhere
        assert len({tl[p] for tl in ids}) > 1
    if len(ids) == 1:
        assert p == len(ids[0]) - 1


def test_shared_prefix_on_plain_lists():
    assert R.shared_prefix_len([[1, 2, 3], [1, 2, 4], [1, 2]]) == 1      # capped by the 2-token list
    assert R.shared_prefix_len([[5, 6], [7, 6]]) == 0
    assert R.shared_prefix_len([[1, 2, 3, 4]]) == 3
    assert R.shared_prefix_len([[1, 2, 3], [1, 2, 3]]) == 2


def test_prefixed_batch_layout():
    b = PackedBatch.build_prefixed([40, 3, 33, 1], [-1, 0, 0, 0], "cpu")
    assert b.parent.tolist() == [-1, 0, 0, 0]
    assert b.cu.tolist() == [0, 40, 43, 76, 77]
    assert b.cu_pad.tolist() == [0, 64, 96, 160, 192]
    pos = b.positions.tolist()
    assert pos[:40] == list(range(40)) and pos[40:43] == [40, 41, 42] and pos[43:76] == list(range(40, 73))
    assert pos[76:] == [40]
    assert b.last_tok.tolist() == [42, 75, 76]                    # the children's last rows only
    tok_of_pad = b.tok_of_pad.tolist()
    assert tok_of_pad[64:67] == [40, 41, 42] and tok_of_pad[67:96] == [-1] * 29
    # every q block once; longest first counting the parent's key tiles
    blocks = list(zip(b.blk_seq.tolist(), b.blk_q0.tolist()))
    assert sorted(blocks) == [(0, 0), (0, 32), (1, 0), (2, 0), (2, 32), (3, 0)]
    walk = [q0 + (64 if s > 0 else 0) for s, q0 in blocks]
    assert walk == sorted(walk, reverse=True) and blocks[0] == (2, 32)


def test_prefixed_batch_of_roots_is_the_plain_layout():
    lens = [5, 64, 33]
    a, b = PackedBatch.build(lens, "cpu"), PackedBatch.build_prefixed(lens, [-1, -1, -1], "cpu")
    for f in ("cu", "cu_pad", "positions", "tok_of_pad", "blk_seq", "blk_q0", "last_tok"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_prefixed_batch_rejects_bad_parents():
    for parent in ([0, -1], [-1, 5], [-1, 0, 1], [-2, -1]):
        with pytest.raises(ValueError):
            PackedBatch.build_prefixed([3] * len(parent), parent, "cpu")


@pytest.mark.parametrize("budget", [1, 50, 100, 333, 65536])
def test_token_budget_splits_cover_every_pair_once(budget):
    rng = np.random.default_rng(budget)
    lengths = rng.integers(20, 120, size=57).tolist()
    p = 17
    groups = R.split_forwards(lengths, p, budget)
    assert [i for g in groups for i in g] == list(range(len(lengths)))
    for g in groups:
        assert len(g) == 1 or p + sum(lengths[i] - p for i in g) <= budget
    assert R.split_forwards([10, 10, 10], 0, 20) == [[0, 1], [2]]
    assert R.split_forwards([10, 10, 10], 4, 16) == [[0, 1], [2]]


def test_settings_defaults_and_env(monkeypatch):
    s = Settings()
    assert (s.rerank_base_url, s.rerank_model_id, s.rerank_timeout_s) == ("", "Qwen/Qwen3-Reranker-4B", 180.0)
    assert (s.rerank_max_chars_per_doc, s.rerank_topn_in, s.rerank_topm_out, s.rerank_max_length) == (0, 40, 12, 1024)
    assert s.rerank_device == s.embeddings_device == 0
    monkeypatch.setenv("rerank_base_url", "native")
    monkeypatch.setenv("RERANK_TOPN_IN", "20")
    monkeypatch.setenv("Rerank_TopM_Out", "5")
    monkeypatch.setenv("EMBEDDINGS_DEVICE", "3")
    s = Settings.from_env()
    assert (s.rerank_base_url, s.rerank_topn_in, s.rerank_topm_out) == ("native", 20, 5)
    assert s.rerank_device == 3
    monkeypatch.setenv("RERANK_DEVICE", "1")
    assert Settings.from_env().rerank_device == 1


class _StubReranker:
    """Deterministic scores: a document's score is its value in `table` (default: its length / 1000)."""

    def __init__(self, table=None, fail=None):
        self.table, self.fail, self.calls = table or {}, fail, []

    def rerank(self, query, documents):
        self.calls.append((query, list(documents)))
        if self.fail:
            raise self.fail
        scores = [float(self.table.get(d, len(d) / 1000.0)) for d in documents]
        return np.asarray(scores, dtype=np.float32), R.stable_order(scores), "stub-reranker"


@pytest.fixture
def native_stub(monkeypatch):
    stub = _StubReranker({"a": 0.1, "b": 0.9, "c": 0.5})
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    reranker.set_reranker(stub)
    yield stub
    reranker.set_reranker(None)


def test_rerank_texts_native_path(native_stub):
    res = reranker.rerank_texts("  q  ", ["a", "b", "c"])
    assert res.order == [1, 2, 0] and res.model == "stub-reranker"
    assert res.scores == pytest.approx([0.1, 0.9, 0.5])
    assert native_stub.calls[-1] == ("q", ["a", "b", "c"])


def test_rerank_texts_validates_and_wraps_errors(monkeypatch, native_stub):
    for query, docs, msg in (("", ["a"], "non-empty query"), ("   ", ["a"], "non-empty query"),
                             ("q", [], "at least one document"), ("q", "abc", "at least one document"),
                             ("q", ["a", 3], "must be strings")):
        with pytest.raises(RerankClientError, match=msg):
            reranker.rerank_texts(query, docs)
    monkeypatch.setattr(settings, "rerank_max_chars_per_doc", 2)
    reranker.rerank_texts("q", ["abcdef"])
    assert native_stub.calls[-1] == ("q", ["ab"])
    reranker.set_reranker(_StubReranker(fail=RuntimeError("device lost")))
    with pytest.raises(RerankClientError, match="native reranker failed: device lost"):
        reranker.rerank_texts("q", ["a"])

    class _Bad:
        def __init__(self, scores, order):
            self.out = (scores, order, "m")

        def rerank(self, q, d):
            return self.out

    for scores, order, msg in (([0.5], None, "count mismatch"), ([float("nan"), 1.0], None, "non-finite"),
                               ([0.1, 0.2], [0, 0], "permutation"), ([0.1, 0.2], [0, 1], "follow the scores"),
                               (["x", 0.2], None, "not numbers")):
        reranker.set_reranker(_Bad(scores, order))
        with pytest.raises(RerankClientError, match=msg):
            reranker.rerank_texts("q", ["a", "b"])
    reranker.set_reranker(None)
    with pytest.raises(RerankClientError, match="not loaded"):
        reranker.rerank_texts("q", ["a"])
    monkeypatch.setattr(settings, "rerank_base_url", "")
    assert not reranker.rerank_enabled()
    with pytest.raises(RerankClientError, match="not configured"):
        reranker.rerank_texts("q", ["a"])


class _Resp:
    def __init__(self, status, payload):
        self.status_code, self._payload = status, payload
        self.text = json.dumps(payload)

    def json(self):
        return self._payload


class _Client:
    def __init__(self, resp, log):
        self._resp, self._log = resp, log

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return None

    def post(self, url, json):
        self._log.append({"url": url, "payload": json})
        return self._resp


def test_http_path_speaks_the_rerank_contract(monkeypatch):
    import httpx
    log = []
    monkeypatch.setattr(settings, "rerank_base_url", "http://rerank.local/")
    good = _Resp(200, {"scores": [0.2, 0.7], "order": [1, 0], "model": "remote-rr"})
    monkeypatch.setattr(httpx, "Client", lambda *a, **k: _Client(good, log))
    res = reranker.rerank_texts("q", ["a", "b"])
    assert (res.scores, res.order, res.model) == ([0.2, 0.7], [1, 0], "remote-rr")
    assert log[0] == {"url": "http://rerank.local/rerank",
                      "payload": {"query": "q", "documents": ["a", "b"], "model": settings.rerank_model_id}}
    no_order = _Resp(200, {"scores": [0.2, 0.7, 0.2]})
    monkeypatch.setattr(httpx, "Client", lambda *a, **k: _Client(no_order, log))
    res = reranker.rerank_texts("q", ["a", "b", "c"])
    assert res.order == [1, 0, 2] and res.model == settings.rerank_model_id
    for resp, msg in ((_Resp(500, {"detail": "x" * 500}), "rerank service returned 500"),
                      (_Resp(200, {"model": "m"}), "missing 'scores'"),
                      (_Resp(200, {"scores": [1.0]}), "count mismatch")):
        monkeypatch.setattr(httpx, "Client", lambda *a, _r=resp, **k: _Client(_r, log))
        with pytest.raises(RerankClientError, match=msg):
            reranker.rerank_texts("q", ["a", "b"])

    def refuse(*a, **k):
        raise httpx.ConnectError("connection refused")

    monkeypatch.setattr(httpx, "Client", refuse)
    with pytest.raises(RerankClientError, match="rerank HTTP request failed"):
        reranker.rerank_texts("q", ["a"])


def test_post_rerank_route():
    from fastapi.testclient import TestClient

    from cadence_rag_amd import gateway
    client = TestClient(gateway.app)
    reranker.set_reranker(None)
    assert client.post("/rerank", json={"query": "q", "documents": ["a"]}).status_code == 502
    reranker.set_reranker(_StubReranker({"a": 0.1, "b": 0.9, "c": 0.5}))
    try:
        r = client.post("/rerank", json={"query": "q", "documents": ["a", "b", "c"]})
        assert r.status_code == 200
        body = r.json()
        assert body["order"] == [1, 2, 0] and body["model"] == "stub-reranker"
        assert body["scores"] == pytest.approx([0.1, 0.9, 0.5])
        assert client.post("/rerank", json={"query": "q", "documents": ["a"], "model": "x"}).json()["model"] == "x"
        assert client.post("/rerank", json={"query": " ", "documents": ["a"]}).status_code == 400
        assert client.post("/rerank", json={"query": "q", "documents": []}).status_code == 400
        reranker.set_reranker(_StubReranker(fail=RuntimeError("boom")))
        assert client.post("/rerank", json={"query": "q", "documents": ["a"]}).status_code == 502
    finally:
        reranker.set_reranker(None)


# ---- retrieve_evidence with the rerank stage ------------------------------------------------------------------
def _gold():
    return json.loads((Path(__file__).parent / "golden" / "reference_retrieve_evidence.json").read_text())


def _request(sc):
    pl = dict(sc["payload"])
    if "filters" in pl:
        f = dict(pl["filters"])
        if f.get("call_ids"):
            f["call_ids"] = [UUID(c) for c in f["call_ids"]]
        pl["filters"] = retrieve.RetrieveFilters(**f)
    if "budget" in pl:
        pl["budget"] = retrieve.Budget(**pl["budget"])
    return retrieve.RetrieveRequest(**pl)


def _dense(monkeypatch, sc):
    from cadence_rag_amd import embeddings
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: sc["dense"] != "off")

    def fake_embed(texts):
        if sc["dense"] == "error":
            raise embeddings.EmbeddingClientError("embedding request failed: connection refused")
        return embeddings.EmbeddingResult(vectors=[[0.25] * 1024 for _ in texts], model="Qwen/Qwen3-Embedding-4B")

    monkeypatch.setattr(embeddings, "embed_texts", fake_embed)


@pytest.mark.parametrize("idx", range(10))
def test_goldens_unchanged_with_the_reranker_off(monkeypatch, idx):
    from test_host_logic import _ReplayBackend
    gold = _gold()
    sc = gold["scenarios"][idx]
    monkeypatch.setattr(settings, "rerank_base_url", "")
    stub = _StubReranker()
    reranker.set_reranker(stub)       # registered but not configured: never called
    try:
        _dense(monkeypatch, sc)
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(gold["lanes"], sc))
    finally:
        reranker.set_reranker(None)
    assert UUID(resp.pop("query_id"))
    assert resp == sc["response"], sc["name"]
    assert stub.calls == []


def _scenario(name):
    gold = _gold()
    return gold, next(s for s in gold["scenarios"] if s["name"] == name)


def _fused_bodies(gold, sc, monkeypatch):
    """The fused rows of both sides as the RRF stage orders them (reranker off)."""
    from test_host_logic import _ReplayBackend
    monkeypatch.setattr(settings, "rerank_base_url", "")
    _dense(monkeypatch, sc)
    req = _request(sc)
    req.return_style = "ids_only"
    return retrieve.retrieve_evidence(req, _ReplayBackend(gold["lanes"], sc))["retrieved_ids"]


def test_rerank_reorders_each_side_and_keeps_budgets(monkeypatch):
    from test_host_logic import _ReplayBackend
    gold, sc = _scenario("evidence_pack_dense")
    _dense(monkeypatch, sc)
    lanes = gold["lanes"]
    bodies = {}
    for lane, rows in lanes.items():
        for r in rows:
            bodies[r.get("text", r.get("content"))] = r
    # score = the reverse of the chunk / artifact id: the RRF order is overturned
    table = {body: 1.0 / (1 + (r.get("chunk_id") or r.get("artifact_chunk_id"))) for body, r in bodies.items()}
    stub = _StubReranker(table)
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    monkeypatch.setattr(settings, "rerank_topn_in", 40)
    monkeypatch.setattr(settings, "rerank_topm_out", 12)
    reranker.set_reranker(stub)
    try:
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(lanes, sc))
        ids = retrieve.retrieve_evidence(retrieve.RetrieveRequest(query=sc["payload"]["query"],
                                                                  return_style="ids_only"),
                                         _ReplayBackend(lanes, sc))
    finally:
        reranker.set_reranker(None)
    assert len(stub.calls) == 2 and stub.calls[0][0] == sc["payload"]["query"].strip()
    docs = stub.calls[0][1]
    notes = resp["notes"]["retrieval"]
    assert notes["reranked_from"] == len(docs) and notes["rerank_model_id"] == "stub-reranker"
    assert notes["rerank_error"] is None
    # full bodies were scored, not the clipped snippets
    assert max(len(d) for d in docs) > retrieve.DEFAULT_SNIPPET_CHARS
    quotes = [q["chunk_id"] for q in resp["quotes"]]
    assert quotes == sorted(quotes)                        # lowest id = highest score first
    arts = [a["artifact_chunk_id"] for a in resp["artifacts"]]
    assert arts == sorted(arts)
    assert len(resp["artifacts"]) + len(resp["quotes"]) <= resp["budget"]["max_evidence_items"]
    assert sum(len(x["snippet"]) for x in resp["artifacts"] + resp["quotes"]) <= resp["budget"]["max_total_chars"]
    per_call = {}
    for q in resp["quotes"]:
        per_call[q["call_id"]] = per_call.get(q["call_id"], 0) + 1
    assert max(per_call.values()) <= retrieve.DEFAULT_MAX_QUOTES_PER_CALL
    # ids_only: (-score, side rank, id)
    got = ids["retrieved_ids"]
    body_of = {(("artifact_chunk" if "artifact_chunk_id" in r else "chunk"),
                r.get("artifact_chunk_id", r.get("chunk_id"))): r.get("text", r.get("content"))
               for rows in lanes.values() for r in rows}

    def key(s):
        tag, rid = s.split(":")
        return (-table[body_of[(tag, int(rid))]], 0 if tag == "artifact_chunk" else 1, int(rid))

    keyed = sorted(got, key=key)
    assert got == keyed and len(got) == len(docs)


def test_rerank_topn_and_topm_cut_each_side(monkeypatch):
    from test_host_logic import _ReplayBackend
    gold, sc = _scenario("evidence_pack_dense")
    fused = _fused_bodies(gold, sc, monkeypatch)
    n_chunks = sum(s.startswith("chunk:") for s in fused)
    n_arts = len(fused) - n_chunks
    stub = _StubReranker()
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    monkeypatch.setattr(settings, "rerank_topn_in", 3)
    monkeypatch.setattr(settings, "rerank_topm_out", 2)
    reranker.set_reranker(stub)
    try:
        req = _request(sc)
        req.return_style = "ids_only"
        got = retrieve.retrieve_evidence(req, _ReplayBackend(gold["lanes"], sc))["retrieved_ids"]
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(gold["lanes"], sc))
    finally:
        reranker.set_reranker(None)
    assert len(stub.calls[0][1]) == min(3, n_arts) + min(3, n_chunks)
    assert sum(s.startswith("chunk:") for s in got) == min(2, n_chunks)
    assert len(got) == min(2, n_arts) + min(2, n_chunks)
    assert resp["notes"]["retrieval"]["reranked_from"] == min(3, n_arts) + min(3, n_chunks)
    assert len(resp["quotes"]) <= 2 and len(resp["artifacts"]) <= 2


def test_rerank_ties_keep_the_rrf_order(monkeypatch):
    from test_host_logic import _ReplayBackend
    gold, sc = _scenario("evidence_pack_dense")
    _dense(monkeypatch, sc)
    stub = _StubReranker()
    stub.rerank = lambda q, d: ([0.5] * len(d), list(range(len(d))), "flat")
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    reranker.set_reranker(stub)
    try:
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(gold["lanes"], sc))
    finally:
        reranker.set_reranker(None)
    # equal scores: every side keeps its RRF order, so the pack is the one without the reranker
    resp.pop("query_id")
    notes = resp["notes"]["retrieval"]
    assert notes.pop("rerank_model_id") == "flat" and notes.pop("rerank_error") is None
    assert notes["reranked_from"] > 0
    notes["reranked_from"] = None
    assert resp == sc["response"]


def test_rerank_fails_open(monkeypatch):
    from test_host_logic import _ReplayBackend
    gold, sc = _scenario("evidence_pack_dense")
    _dense(monkeypatch, sc)
    monkeypatch.setattr(settings, "rerank_base_url", "native")
    reranker.set_reranker(_StubReranker(fail=RuntimeError("device lost")))
    try:
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(gold["lanes"], sc))
    finally:
        reranker.set_reranker(None)
    resp.pop("query_id")
    notes = resp["notes"]["retrieval"]
    assert notes.pop("rerank_error") == "native reranker failed: device lost"
    assert notes.pop("rerank_model_id") is None and notes["reranked_from"] is None
    assert resp == sc["response"]                 # the RRF order stands
