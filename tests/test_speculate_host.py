"""Speculative decoding on the host: the prompt-lookup drafter and the accepted prefix (pure functions), and /answer's
`speculate` -- ANSWER_SPECULATE and the request field, their bounds, that the value reaches only a native model with
supports_speculation, notes.speculation, and that with 0 the response and the notes are those of today."""
from __future__ import annotations

import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerRequest, AnswerRequestError
from cadence_rag_amd.config import settings
from cadence_rag_amd.speculate import MAX_SPECULATE, accepted_prefix, propose_drafts

GOOD = "The rollback was agreed [Q-11]. The summary says so [A-45]."


# ---- the drafter ------------------------------------------------------------------------------------------------
def test_no_match_gives_no_draft():
    assert propose_drafts([1, 2, 3, 4], 4) == []
    assert propose_drafts([], 4) == [] and propose_drafts([7], 4) == []
    assert propose_drafts([1, 2, 3, 1, 2], 4, min_ngram=3) == []          # a 2-gram matches, 3 are asked for


def test_the_longest_ngram_wins_over_a_later_shorter_one():
    # suffix (8, 9): the 2-gram occurs at 0 (followed by 5); the 1-gram 9 occurs later, at 4 (followed by 6)
    ids = [8, 9, 5, 0, 9, 6, 0, 8, 9]
    assert propose_drafts(ids, 1) == [5]
    assert propose_drafts(ids, 1, max_ngram=1) == [6]
    assert propose_drafts(ids, 3) == [5, 0, 9]


def test_the_latest_occurrence_wins():
    ids = [1, 2, 30, 1, 2, 40, 1, 2]
    assert propose_drafts(ids, 2) == [40, 1]
    assert propose_drafts([5, 5, 5], 4) == [5]                           # occurrences may overlap the suffix


def test_the_continuation_is_clipped_at_the_end():
    ids = [1, 2, 3, 4, 1, 2]
    assert propose_drafts(ids, 7) == [3, 4, 1, 2]
    assert propose_drafts(ids, 2) == [3, 4]


def test_no_draft_is_asked_for_or_an_id_is_unknown():
    ids = [1, 2, 3, 1, 2]
    assert propose_drafts(ids, 3) == [3, 1, 2]
    assert propose_drafts(ids, 0) == [] and propose_drafts(ids, -2) == []
    assert propose_drafts([-1, 2, 3, 1, 2], 3) == []                     # a forked slot's ids are unknown (-1)


def test_accepted_prefix_over_all_prefix_lengths():
    drafts = [4, 5, 6, 7]
    for right in range(len(drafts) + 1):
        picks = drafts[:right] + [99] * (len(drafts) + 1 - right)        # one pick per row: the drafts' rows and one more
        assert accepted_prefix(drafts, picks) == right
    assert accepted_prefix([], [3]) == 0
    assert accepted_prefix([4, 5], [4]) == 1                              # picking stopped early (a stop id, the budget)
    assert accepted_prefix([4, 5, 6], [9, 5, 6]) == 0                     # a right draft behind a wrong one does not count
    assert MAX_SPECULATE == 7


# ---- /answer ----------------------------------------------------------------------------------------------------
@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        quote = {"evidence_id": "Q-11", "call_id": "call-1", "chunk_id": 11, "speaker": "agent", "start_ts_ms": 0,
                 "end_ts_ms": 1, "snippet": "the rollback was agreed", "why_relevant": "bm25"}
        art = {"evidence_id": "A-45", "call_id": "call-9", "artifact_id": 4, "artifact_chunk_id": 45, "kind": "summary",
               "snippet": "the summary", "why_relevant": "dense"}
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [art], "quotes": [quote], "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 0)
    yield
    answer.set_llm(None)


class _Plain:
    """A native model that knows nothing of speculation: an unknown keyword would be a TypeError."""
    model_id = "stub-llm"

    def __init__(self):
        self.calls = []

    def generate_text(self, messages, max_new_tokens, grammar=None):
        self.calls.append({})
        return GOOD


class _Speculating(_Plain):
    supports_speculation = True
    last_speculation = None

    def generate_text(self, messages, max_new_tokens, grammar=None, **kw):
        self.calls.append(dict(kw))
        k = kw.get("speculate", 0)
        self.last_speculation = {"forwards": 5, "drafted": [4 * k], "accepted": [3 * k]} if k else None
        return GOOD


def _ask(llm, **fields):
    answer.set_llm(llm)
    return answer.answer_question(AnswerRequest(query="what was agreed?", **fields))


def test_the_request_field_reaches_a_model_that_speculates(pack):
    llm = _Speculating()
    out = _ask(llm, speculate=3)
    assert llm.calls == [{"speculate": 3}] and out["answer"] == GOOD
    assert out["notes"]["speculation"] == {"forwards": 5, "drafted": [12], "accepted": [9]}


def test_the_setting_supplies_the_default_and_the_request_overrides_it(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_speculate", 5)
    llm = _Speculating()
    assert _ask(llm)["notes"]["speculation"]["drafted"] == [20]
    assert _ask(llm, speculate=1)["notes"]["speculation"]["drafted"] == [4]
    assert "speculation" not in _ask(llm, speculate=0)["notes"]               # the request turns it off
    assert llm.calls == [{"speculate": 5}, {"speculate": 1}, {}]


def test_a_model_without_the_attribute_never_sees_it(pack):
    llm = _Plain()
    out = _ask(llm, speculate=4)
    assert llm.calls == [{}] and out["answer"] == GOOD and out["notes"]["speculation"] == {"applied": False}


def test_an_http_backend_never_sees_it(pack, monkeypatch):
    import json
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.invalid/v1")
    bodies = []

    def post(url, headers, body, timeout_s):
        bodies.append(body)
        return 200, json.dumps({"choices": [{"message": {"content": GOOD}}], "model": "served"})

    monkeypatch.setattr(answer, "_post_json", post)
    llm = _Speculating()                                                        # registered, but the backend is not native
    out = _ask(llm, speculate=4)
    assert out["answer"] == GOOD and out["notes"]["speculation"] == {"applied": False} and llm.calls == []
    assert all("speculate" not in body for body in bodies)


def test_with_zero_the_response_and_the_notes_are_those_of_today(pack):
    want = _ask(_Plain())
    for llm, fields in ((_Speculating(), {}), (_Speculating(), {"speculate": 0}), (_Plain(), {"speculate": 0})):
        got = _ask(llm, **fields)
        assert got == want and llm.calls == [{}]
    assert set(want["notes"]) == {"evidence_items", "dropped_evidence", "llm_calls", "validator"}


def test_values_out_of_range_are_refused(pack, monkeypatch):
    for bad in (-1, 8, 2.0, "3", True):
        with pytest.raises(AnswerRequestError, match="speculate"):
            _ask(_Speculating(), speculate=bad)
    monkeypatch.setattr(settings, "answer_speculate", 9)
    with pytest.raises(AnswerRequestError, match="speculate"):
        _ask(_Speculating())
    assert _ask(_Speculating(), speculate=7)["notes"]["speculation"]["drafted"] == [28]


def test_the_setting_reads_the_environment(monkeypatch):
    from cadence_rag_amd.config import Settings
    assert Settings().answer_speculate == 0
    monkeypatch.setenv("ANSWER_SPECULATE", "4")
    assert Settings.from_env().answer_speculate == 4


def test_the_generator_declares_it():
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    assert Qwen3Generator.supports_speculation is True
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="speculate"):
            Qwen3Generator._check_speculate(bad)
