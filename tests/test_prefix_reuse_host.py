"""Prefix reuse on the host: plan_reuse's truth table, the reused-token count answer_question keeps for an LLM that
reports one, and the LLM_PREFIX_CACHE setting."""
from __future__ import annotations

import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerRequest
from cadence_rag_amd.config import Settings, settings
from cadence_rag_amd.encoder.generate import PREFIX_MIN_REUSE, plan_reuse


def test_plan_reuse_truth_table():
    assert PREFIX_MIN_REUSE == 32
    ids = list(range(100, 200))
    assert plan_reuse(ids, ids, 32) == 99                       # identical: one row is left to compute
    assert plan_reuse(ids[:60], ids, 32) == 60                  # the slot holds less than the prompt: all of it
    assert plan_reuse(ids, ids[:60], 32) == 59                  # the slot holds more: the prompt less one row
    assert plan_reuse(ids[:99], ids, 32) == 99 and plan_reuse(ids, ids[:33], 32) == 32
    for at, want in ((0, 0), (31, 0), (32, 32), (33, 33), (99, 99)):
        other = list(ids)
        other[at] = -5
        assert plan_reuse(ids, other, 32) == want, at            # the common prefix ends at `at`
        assert plan_reuse(other, ids, 32) == want, at
    assert plan_reuse([], ids, 32) == 0 and plan_reuse(ids, [], 32) == 0 and plan_reuse(ids, ids[:1], 1) == 0
    assert plan_reuse(ids[:40], ids, 41) == 0 and plan_reuse(ids[:40], ids, 40) == 40 and plan_reuse(ids[:5], ids, 1) == 5
    assert plan_reuse(ids[:31], ids) == 0 and plan_reuse(ids[:32], ids) == 32       # the default is PREFIX_MIN_REUSE
    assert plan_reuse(tuple(ids), ids, 0) == 99 and plan_reuse([-1] * 50, ids, 1) == 0


@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        quotes = [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i}", "chunk_id": 10 + i, "speaker": "agent",
                   "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(3)]
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": quotes, "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    yield
    answer.set_llm(None)


class _Stub:
    model_id = "stub-llm"

    def __init__(self, replies, reuse=None):
        self.replies, self.reuse, self.calls = list(replies), reuse, 0
        if reuse is not None:
            self.last_reuse = None

    def generate_text(self, messages, max_new_tokens):
        self.calls += 1
        if self.reuse is not None:
            self.last_reuse = {"reused": [self.reuse[self.calls - 1]], "computed": [7]}
        return self.replies[min(self.calls, len(self.replies)) - 1]


def test_answer_adds_up_the_reused_tokens_of_every_call(pack):
    llm = _Stub(["Not cited.", "Still not cited.", "Fact zero holds [Q-10]."], reuse=[0, 410, 530])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok" and out["repairs"] == 2 and llm.calls == 3
    assert out["notes"]["prefix_reused_tokens"] == 940 and out["notes"]["llm_calls"] == 3
    llm = _Stub(["Fact zero holds [Q-10]."], reuse=[0])
    answer.set_llm(llm)
    assert answer.answer_question(AnswerRequest(query="what holds?"))["notes"]["prefix_reused_tokens"] == 0


def test_an_llm_without_last_reuse_leaves_the_notes_alone(pack):
    llm = _Stub(["Not cited.", "Fact zero holds [Q-10]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok" and "prefix_reused_tokens" not in out["notes"]
    assert sorted(out["notes"]) == ["dropped_evidence", "evidence_items", "llm_calls", "validator"]


def test_the_prefix_cache_setting(monkeypatch):
    monkeypatch.delenv("LLM_PREFIX_CACHE", raising=False)
    assert Settings().llm_prefix_cache is True and Settings.from_env().llm_prefix_cache is True
    for raw, want in (("0", False), ("false", False), ("1", True), ("on", True)):
        monkeypatch.setenv("LLM_PREFIX_CACHE", raw)
        assert Settings.from_env().llm_prefix_cache is want, raw
