"""/answer on the host: the citation validator, the bounded repair loop over stub LLMs, the evidence that is dropped when a
prompt does not fit, the http client with its posting function replaced (no socket), the gateway route, and the retrieve
goldens unchanged beside it."""
from __future__ import annotations

import json
from uuid import UUID

import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerClientError, AnswerRequest, validate_citations
from cadence_rag_amd.config import settings

IDS = ["Q-12", "A-45", "Q-7"]


# ---- the validator ----------------------------------------------------------------------------------------------
def test_validator_accepts_citations_before_and_after_the_full_stop():
    for text in ("The rollback was agreed [Q-12].",
                 "The rollback was agreed.[Q-12]",
                 "The rollback was agreed. [Q-12]",
                 "The rollback was agreed [Q-12]. It ships next week.[A-45]",
                 "Was it agreed? [Q-12] Yes it was! [A-45]",
                 "The rollback was agreed [Q-12]"):
        rep = validate_citations(text, IDS)
        assert rep["valid"] and not rep["uncited"] and not rep["unknown_ids"], (text, rep)
    rep = validate_citations("The rollback was agreed [Q-12]. It ships next week.[A-45]", IDS)
    assert rep["sentences"] == 2 and rep["cited"] == ["Q-12", "A-45"]


def test_validator_two_ids_on_one_sentence_and_order_of_first_use():
    rep = validate_citations("Both say so [A-45][Q-12]. Again [Q-12] [Q-7].", IDS)
    assert rep["valid"] and rep["sentences"] == 2 and rep["cited"] == ["A-45", "Q-12", "Q-7"]
    rep = validate_citations("Both say so.[A-45][Q-12] And this [Q-007].", IDS)
    assert rep["valid"] and rep["cited"] == ["A-45", "Q-12", "Q-7"]


def test_validator_reports_an_uncited_sentence():
    rep = validate_citations("The rollback was agreed [Q-12]. It ships next week. The customer is happy [A-45].", IDS)
    assert not rep["valid"] and rep["uncited"] == ["It ships next week."] and rep["unknown_ids"] == []
    rep = validate_citations("Nothing is cited here", IDS)
    assert not rep["valid"] and rep["uncited"] == ["Nothing is cited here"]
    # a trailing group belongs to the sentence before it, not to the one after
    rep = validate_citations("First.[Q-12] Second.", IDS)
    assert rep["uncited"] == ["Second."]


def test_validator_reports_an_unknown_id():
    rep = validate_citations("The rollback was agreed [Q-13]. It ships [A-45][A-46].", IDS)
    assert not rep["valid"] and rep["unknown_ids"] == ["Q-13", "A-46"] and rep["uncited"] == []
    assert rep["cited"] == ["A-45"]
    # the pattern is \[(Q|A)-\d+\]: anything else is no citation
    assert validate_citations("Agreed [q-12].", IDS)["uncited"] == ["Agreed [q-12]."]
    assert validate_citations("Agreed (Q-12).", IDS)["uncited"] == ["Agreed (Q-12)."]
    assert validate_citations("Agreed [X-12].", IDS)["uncited"] == ["Agreed [X-12]."]


def test_validator_blank_lines_and_list_markers_are_not_sentences():
    text = "\n\n- The rollback was agreed [Q-12].\n\n* It ships next week [A-45].\n1. Version v1.2.3 is the target [Q-7].\n2)\n-\n"
    rep = validate_citations(text, IDS)
    assert rep["valid"] and rep["sentences"] == 3, rep
    assert answer.split_sentences("Version v1.2.3 is out [Q-7]. Done!")[0] == "Version v1.2.3 is out [Q-7]."
    assert not validate_citations("", IDS)["valid"] and not validate_citations("   \n", IDS)["valid"]
    assert not validate_citations("[Q-12]", IDS)["valid"]          # ids without a sentence


# ---- answer_question over stub LLMs -----------------------------------------------------------------------------
def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    """retrieve_evidence replaced by a fixed pack (one artifact, then n quotes); records the request it was given."""
    state = {"quotes": 3, "requests": []}

    def fake(request, backend=None):
        state["requests"].append(request)
        art = {"evidence_id": "A-45", "call_id": "call-9", "artifact_id": 4, "artifact_chunk_id": 45, "kind": "summary",
               "snippet": "the summary", "why_relevant": "dense"}
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [art] if state["quotes"] else [], "quotes": _items(state["quotes"]), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    yield state
    answer.set_llm(None)


class _StubLLM:
    model_id = "stub-llm"

    def __init__(self, replies, too_long_above=None):
        self.replies, self.calls, self.too_long_above = list(replies), [], too_long_above

    def generate_text(self, messages, max_new_tokens):
        if self.too_long_above is not None and messages[1]["content"].count("\n[") > self.too_long_above:
            raise ValueError("a prompt of 9000 tokens does not fit: max_context 8192 - max_new_tokens 512 leaves 7680")
        self.calls.append([dict(m) for m in messages])
        return self.replies[min(len(self.calls) - 1, len(self.replies) - 1)]


def test_one_repair_then_ok(pack):
    llm = _StubLLM(["The rollback was agreed.", "The rollback was agreed [Q-11]. The summary says so [A-45]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what was agreed?"))
    assert out["status"] == "ok" and out["repairs"] == 1 and len(llm.calls) == 2 and out["model"] == "stub-llm"
    assert out["answer"] == "The rollback was agreed [Q-11]. The summary says so [A-45]."
    assert out["citations"] == [{"evidence_id": "Q-11", "call_id": "call-1"}, {"evidence_id": "A-45", "call_id": "call-9"}]
    assert "evidence_pack" not in out
    first, second = llm.calls
    assert [m["role"] for m in first] == ["system", "user"] and "INSUFFICIENT_EVIDENCE" in first[0]["content"]
    assert "[A-45] summary: the summary\n[Q-10] agent: fact number 0" in first[1]["content"]
    assert [m["role"] for m in second] == ["system", "user", "assistant", "user"]
    assert "The rollback was agreed." in second[3]["content"] and "[Q-10]" in second[3]["content"]
    assert pack["requests"][0].return_style == "evidence_pack_json"


def test_never_cites_fails_closed(pack):
    llm = _StubLLM(["It was agreed. Trust me [Q-99]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what was agreed?", echo_evidence=True))
    assert len(llm.calls) == settings.answer_max_repairs + 1 == 3
    assert out["status"] == "citation_check_failed" and out["answer"] is None and out["citations"] == []
    assert out["repairs"] == 2 and out["notes"]["validator"]["unknown_ids"] == ["Q-99"]
    assert out["evidence_pack"]["quotes"] == _items(3)


def test_empty_pack_never_calls_the_llm(pack):
    pack["quotes"] = 0
    llm = _StubLLM(["anything [Q-10]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what was agreed?"))
    assert llm.calls == [] and out["answer"] is None and out["status"] == "insufficient_evidence"
    assert out["citations"] == [] and out["notes"]["llm_calls"] == 0


def test_insufficient_evidence_reply_maps_to_the_status(pack):
    for reply in ("INSUFFICIENT_EVIDENCE", " INSUFFICIENT_EVIDENCE.\n"):
        llm = _StubLLM([reply])
        answer.set_llm(llm)
        out = answer.answer_question(AnswerRequest(query="what is the weather?"))
        assert out["status"] == "insufficient_evidence" and out["answer"] is None and len(llm.calls) == 1


def test_evidence_is_dropped_from_the_tail_when_the_prompt_does_not_fit(pack):
    pack["quotes"] = 6                       # 7 items with the artifact; the stub takes at most 4
    llm = _StubLLM(["Fact [Q-10]. Gone [Q-15]."], too_long_above=4)
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="q"))
    assert out["notes"]["dropped_evidence"] == 3
    body = llm.calls[0][1]["content"]
    assert "[A-45]" in body and "[Q-12]" in body and "[Q-13]" not in body and "[Q-15]" not in body
    # a dropped item is no longer citable
    assert out["status"] == "citation_check_failed" and out["notes"]["validator"]["unknown_ids"] == ["Q-15"]
    llm = _StubLLM(["x"], too_long_above=0)
    answer.set_llm(llm)
    with pytest.raises(AnswerClientError, match="does not fit"):
        answer.answer_question(AnswerRequest(query="q"))


def test_failures_are_answer_client_errors(pack, monkeypatch):
    answer.set_llm(None)
    with pytest.raises(AnswerClientError, match="not loaded"):
        answer.answer_question(AnswerRequest(query="q"))

    class Boom:
        model_id = "boom"

        def generate_text(self, messages, max_new_tokens):
            raise RuntimeError("device lost")

    answer.set_llm(Boom())
    with pytest.raises(AnswerClientError, match="native LLM failed: device lost"):
        answer.answer_question(AnswerRequest(query="q"))
    monkeypatch.setattr(settings, "llm_base_url", "")
    with pytest.raises(AnswerClientError, match="LLM_BASE_URL is not configured"):
        answer.answer_question(AnswerRequest(query="q"))
    assert not answer.llm_enabled()


def test_settings_use_the_reference_names():
    from cadence_rag_amd.config import Settings
    s = Settings()
    assert (s.llm_base_url, s.llm_api_key, s.llm_model, s.llm_timeout_s) == ("", "", "Qwen/Qwen3-4B-Instruct-2507", 180.0)
    assert (s.llm_max_new_tokens, s.llm_max_context, s.answer_max_repairs) == (512, 8192, 2)
    assert s.llm_device == s.embeddings_device and Settings(llm_device=3).llm_device == 3


# ---- the http client: the one posting function replaced, no socket ----------------------------------------------
def test_http_path_speaks_chat_completions(pack, monkeypatch):
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.local/v1/")
    monkeypatch.setattr(settings, "llm_api_key", "sekret")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 77)
    log = []

    def post(url, headers, body, timeout_s):
        log.append((url, headers, body, timeout_s))
        return 200, json.dumps({"model": "remote-llm", "choices": [{"message": {"role": "assistant",
                                                                                "content": "Agreed [Q-10]."}}]})

    monkeypatch.setattr(answer, "_post_json", post)
    out = answer.answer_question(AnswerRequest(query="what was agreed?"))
    assert out["status"] == "ok" and out["model"] == "remote-llm" and out["answer"] == "Agreed [Q-10]."
    url, headers, body, timeout_s = log[0]
    assert url == "http://llm.local/v1/chat/completions" and headers == {"Authorization": "Bearer sekret"}
    assert timeout_s == settings.llm_timeout_s
    assert body["model"] == settings.llm_model and body["temperature"] == 0 and body["max_tokens"] == 77
    assert [m["role"] for m in body["messages"]] == ["system", "user"]
    monkeypatch.setattr(settings, "llm_api_key", "")
    answer.answer_question(AnswerRequest(query="what was agreed?"))
    assert log[1][1] == {}
    for reply, msg in (((500, "x" * 500), "LLM service returned 500"), ((200, "not json"), "not a chat completion"),
                       ((200, json.dumps({"choices": []})), "not a chat completion"),
                       ((200, json.dumps({"choices": [{"message": {"content": None}}]})), "holds no text")):
        monkeypatch.setattr(answer, "_post_json", lambda *a, _r=reply: _r)
        with pytest.raises(AnswerClientError, match=msg):
            answer.answer_question(AnswerRequest(query="q"))


def test_post_answer_route(pack, monkeypatch):
    from fastapi.testclient import TestClient

    from cadence_rag_amd import gateway
    client = TestClient(gateway.app)
    assert client.get("/health").json()["llm_loaded"] is False
    assert client.post("/answer", json={"query": "q"}).status_code == 502          # native, nothing registered
    answer.set_llm(_StubLLM(["Agreed [Q-10]."]))
    assert client.get("/health").json()["llm_loaded"] is True
    r = client.post("/answer", json={"query": "what was agreed?", "echo_evidence": True})
    assert r.status_code == 200
    body = r.json()
    assert body["status"] == "ok" and body["citations"] == [{"evidence_id": "Q-10", "call_id": "call-0"}]
    assert body["evidence_pack"]["artifacts"][0]["evidence_id"] == "A-45"
    assert isinstance(pack["requests"][-1], retrieve.RetrieveRequest) and pack["requests"][-1].query == "what was agreed?"

    def no_backend(request, backend=None):
        raise RuntimeError("retrieve_evidence: no backend registered (set_backend)")

    monkeypatch.setattr(retrieve, "retrieve_evidence", no_backend)
    assert client.post("/answer", json={"query": "q"}).status_code == 503


# ---- nothing existing changes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(10))
def test_goldens_unchanged_and_answer_over_them(monkeypatch, idx):
    """With LLM_BASE_URL="" retrieve_evidence answers the ten reference scenarios as before and answer_question refuses;
    with a stub LLM the answer's pack is the scenario's own."""
    from test_host_logic import _ReplayBackend
    from test_rerank_host import _dense, _gold, _request
    gold = _gold()
    sc = gold["scenarios"][idx]
    monkeypatch.setattr(settings, "llm_base_url", "")
    monkeypatch.setattr(settings, "rerank_base_url", "")
    llm = _StubLLM(["INSUFFICIENT_EVIDENCE"])
    answer.set_llm(llm)         # registered but not configured: never called
    try:
        _dense(monkeypatch, sc)
        resp = retrieve.retrieve_evidence(_request(sc), _ReplayBackend(gold["lanes"], sc))
        assert UUID(resp.pop("query_id"))
        assert resp == sc["response"], sc["name"]
        req = _request(sc)
        fields = {k: getattr(req, k) for k in ("query", "intent", "filters", "budget", "return_style", "debug")}
        with pytest.raises(AnswerClientError, match="not configured"):
            answer.answer_question(AnswerRequest(**fields), _ReplayBackend(gold["lanes"], sc))
        assert llm.calls == []
        monkeypatch.setattr(settings, "llm_base_url", "native")
        fields["return_style"], fields["debug"] = "evidence_pack_json", False
        out = answer.answer_question(AnswerRequest(**fields, echo_evidence=True), _ReplayBackend(gold["lanes"], sc))
        items = out["evidence_pack"].get("artifacts", []) + out["evidence_pack"].get("quotes", [])
        assert len(llm.calls) == (1 if items else 0) and out["status"] == "insufficient_evidence"
        if sc["payload"].get("return_style", "evidence_pack_json") == "evidence_pack_json" and not sc["payload"].get("debug"):
            pack = dict(out["evidence_pack"])
            pack.pop("query_id")
            assert pack == sc["response"]
    finally:
        answer.set_llm(None)
