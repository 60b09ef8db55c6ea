"""Repetition control on the host: the rule (penalties.adjust_host) on hand-computed rows, clause by clause and all
together; PenaltyParams' ranges, `neutral` and `echo`; bias_list and exempt_ids; and the /answer plumbing over stub LLMs
and a replaced posting function (no socket)."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerRequest, AnswerRequestError
from cadence_rag_amd.config import settings
from cadence_rag_amd.grammar import TokenTable
from cadence_rag_amd.penalties import (CITATION_ALPHABET, PenaltyParams, active, adjust_host, banned_continuations,
                                       bias_list, exempt_ids, exempt_words)

F = np.float32
INF = math.inf


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32).tolist()


# ---- the rule ---------------------------------------------------------------------------------------------------
def test_repetition_sign_branch_and_specials():
    """l / rp above 0, l * rp at and below it: +0, -0, -inf and NaN take the else arm; +inf the division."""
    row = [2.6, -2.6, 0.0, -0.0, INF, -INF, math.nan, 1.0]
    out, token = adjust_host(row, [0, 1, 2, 3, 4, 5, 6], 7, PenaltyParams(repetition_penalty=1.3))
    want = [F(2.6) / F(1.3), F(-2.6) * F(1.3), F(0.0) * F(1.3), F(-0.0) * F(1.3), INF, -INF, math.nan, 1.0]
    assert _bits(out[:6]) == _bits(want[:6]) and math.isnan(out[6]) and out[7] == 1.0
    assert np.signbit(out[3]) and not np.signbit(out[2]) and token == 4
    # a penalty below 1 rewards repetition: the same two arms
    out, _ = adjust_host([2.0, -2.0], [0, 1], 0, PenaltyParams(repetition_penalty=0.5))
    assert out.tolist() == [4.0, -1.0]
    # rp == 1 touches nothing, not even through the other clauses' zeros
    out, _ = adjust_host(row, [0, 1, 2, 3, 4, 5, 6], 0, PenaltyParams(no_repeat_ngram=8))
    assert _bits(out[:6]) == _bits(row[:6])


def test_presence_and_frequency_count_the_output_only():
    p = PenaltyParams(presence_penalty=0.5, frequency_penalty=0.25, repetition_penalty=2.0)
    #          prompt: 0 0 5 | output: 1 2 2 2
    out, token = adjust_host([4.0] * 6, [0, 0, 5, 1, 2, 2, 2], 3, p)
    assert out.tolist() == [2.0, (2.0 - 0.25) - 0.5, (2.0 - 0.75) - 0.5, 4.0, 4.0, 2.0]   # c = 1 against c = 3
    assert token == 3                                     # the lowest id among the untouched maxima
    # three roundings: fp32(f * fp32(c)), then the two subtractions
    p = PenaltyParams(presence_penalty=0.3, frequency_penalty=0.1)
    out, _ = adjust_host([1.0, 1.0], [1, 1, 1], 0, p)
    want = F(F(1.0) - F(F(0.1) * F(3.0))) - F(0.3)
    assert _bits(out) == _bits([1.0, want])
    # with the whole history as prompt nothing is counted
    out, _ = adjust_host([1.0, 1.0], [1, 1, 1], 3, p)
    assert out.tolist() == [1.0, 1.0]


def test_ngram_ban_at_the_edges_of_the_output():
    n = 3
    p = PenaltyParams(no_repeat_ngram=n)
    row = [1.0] * 8
    for output, banned in (([5], []),                      # |O| = n - 2: no tail yet
                           ([5, 6], []),                   # |O| = n - 1: a tail, but no j with j + n - 1 < |O|
                           ([5, 6, 7], []),                # |O| = n: the only window is not the tail (6 7)
                           ([5, 5, 5], [5]),               # |O| = n: the window 5 5 at j = 0 is the tail 5 5
                           ([5, 6, 7, 5, 6], [7]),
                           ([5, 6, 7, 5, 6, 1, 5, 6], [1, 7]),
                           ([4, 4, 4, 4], [4])):           # overlapping self-match
        assert banned_continuations(output, n) == banned, output
        out, _ = adjust_host(row, [5, 6, 2] + output, 3, p)    # the prompt's own 5 6 2 bans nothing
        assert sorted(np.nonzero(out == -INF)[0].tolist()) == banned, output
    # n = 2: every id that ever followed the last id
    assert banned_continuations([3, 1, 3, 2, 3], 2) == [1, 2]
    # an id outside the row takes part in the match and is ignored as a target
    out, _ = adjust_host(row, [900, 1, 900], 0, PenaltyParams(no_repeat_ngram=2))
    assert np.nonzero(out == -INF)[0].tolist() == [1]
    out, _ = adjust_host(row, [1, 900, 1], 0, PenaltyParams(no_repeat_ngram=2))
    assert not (out == -INF).any()


def test_exempt_ids_are_untouched_but_biased_and_all_clauses_together():
    p = PenaltyParams(repetition_penalty=2.0, presence_penalty=1.0, frequency_penalty=0.5, no_repeat_ngram=2,
                      logit_bias={2: 3.0, 3: -INF, 4: -1.5})
    row = [4.0, 4.0, 4.0, 4.0, 4.0, -4.0]
    hist = [0, 5, 1, 2, 1]            # prompt 0 5 | output 1 2 1: the bigram ban takes 2
    out, token = adjust_host(row, hist, 2, p)
    assert out.tolist() == [2.0, (2.0 - 1.0) - 1.0, -INF, -INF, 2.5, -8.0] and token == 4
    mask = np.array([False, True, True, False, False, False])
    out, token = adjust_host(row, hist, 2, p, exempt=mask)
    assert out.tolist() == [2.0, 4.0, 7.0, -INF, 2.5, -8.0] and token == 2
    assert adjust_host(row, hist, 2, p, exempt=[1, 2])[0].tolist() == out.tolist()       # ids instead of a mask
    # an explicit bias list takes the place of logit_bias
    out, _ = adjust_host(row, hist, 2, p, bias=[(0, 1.0)])
    assert out.tolist() == [3.0, 0.0, -INF, 4.0, 4.0, -8.0]
    # `total` cuts the history
    assert adjust_host(row, hist, 2, p, total=3)[0].tolist() == adjust_host(row, hist[:3], 2, p)[0].tolist()


def test_ties_go_to_the_lowest_id_and_all_nan_gives_minus_one():
    out, token = adjust_host([3.0, 6.0, 3.0, 1.0], [1], 0, PenaltyParams(repetition_penalty=2.0))
    assert out.tolist() == [3.0, 3.0, 3.0, 1.0] and token == 0
    assert adjust_host([math.nan, 1.0, math.nan], [], 0, PenaltyParams())[1] == 1
    assert adjust_host([math.nan] * 3, [0], 0, PenaltyParams(repetition_penalty=2.0))[1] == -1
    assert adjust_host([-INF, -INF], [], 0, PenaltyParams())[1] == 0      # -inf is a candidate, as in lm_head
    assert adjust_host([1.0, 2.0], [], 0, PenaltyParams(logit_bias={1: -INF}))[1] == 0


# ---- the parameters ---------------------------------------------------------------------------------------------
def test_penalty_params_ranges_neutral_and_echo():
    assert PenaltyParams().neutral and active(PenaltyParams()) is None and active(None) is None
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=-0.5), dict(frequency_penalty=2.0),
               dict(no_repeat_ngram=2), dict(logit_bias={7: 0.0}), dict(min_new_tokens=1)):
        p = PenaltyParams(**kw)
        assert not p.neutral and active(p) is p, kw
    for kw in (dict(repetition_penalty=0.1), dict(repetition_penalty=10), dict(presence_penalty=2), dict(no_repeat_ngram=8),
               dict(logit_bias={i: -100.0 for i in range(256)}), dict(logit_bias={"12": "-inf"})):
        PenaltyParams(**kw)
    for kw in (dict(repetition_penalty=0.09), dict(repetition_penalty=10.5), dict(repetition_penalty=math.nan),
               dict(presence_penalty=2.1), dict(presence_penalty=math.nan), dict(frequency_penalty=-2.1),
               dict(no_repeat_ngram=1), dict(no_repeat_ngram=9), dict(no_repeat_ngram=-2), dict(no_repeat_ngram=2.0),
               dict(no_repeat_ngram=True), dict(min_new_tokens=-1), dict(min_new_tokens=1.5),
               dict(logit_bias={i: 0.0 for i in range(257)}), dict(logit_bias={3: 100.5}), dict(logit_bias={3: INF}),
               dict(logit_bias={3: math.nan}), dict(logit_bias={-1: 0.0}), dict(logit_bias={"x": 0.0}),
               dict(logit_bias={1.5: 0.0}), dict(logit_bias={3: "much"}), dict(logit_bias=[(3, 1.0)]),
               dict(logit_bias={3: 1.0, "3": 2.0})):
        with pytest.raises(ValueError):
            PenaltyParams(**kw)
    p = PenaltyParams(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=-0.25, no_repeat_ngram=3,
                      logit_bias={"9": -INF, 4: 2}, min_new_tokens=5)
    assert p.logit_bias == {4: 2.0, 9: -INF} and list(p.logit_bias) == [4, 9]        # integer keys, ascending
    assert p.echo() == {"repetition_penalty": 1.2, "presence_penalty": 0.5, "frequency_penalty": -0.25,
                        "no_repeat_ngram": 3, "logit_bias": {"4": 2.0, "9": "-inf"}, "min_new_tokens": 5}
    json.dumps(p.echo())
    assert hash(p) == hash(PenaltyParams(1.2, 0.5, -0.25, 3, {9: -INF, 4: 2.0}, 5))


def test_bias_list_holds_the_stop_ids_below_min_new_tokens():
    p = PenaltyParams(logit_bias={7: 1.0, 2: -3.0, 500: 4.0}, min_new_tokens=2)
    assert bias_list(p, 0, [9, 2]) == [(2, -INF), (7, 1.0), (9, -INF), (500, 4.0)]
    assert bias_list(p, 1, [9], vocab=100) == [(2, -3.0), (7, 1.0), (9, -INF)]
    assert bias_list(p, 2, [9, 2]) == [(2, -3.0), (7, 1.0), (500, 4.0)]
    with pytest.raises(ValueError):
        bias_list(PenaltyParams(logit_bias={i: 0.0 for i in range(256)}, min_new_tokens=1), 0, [300])


def test_exempt_ids_and_words():
    table = TokenTable.from_bytes([b"[", b"Q-", b"12]", b"", None, b"Q x", b" [", b"A", b"the", b"-0123456789"], stop_ids=[3])
    assert exempt_ids(table, CITATION_ALPHABET).tolist() == [0, 1, 2, 7, 9]
    assert exempt_ids(table, b"").tolist() == [] and exempt_ids(table, b"the").tolist() == [8]
    words = exempt_words([0, 31, 32, 69, 70, -1], 70)
    assert words.dtype == np.uint32 and words.tolist() == [(1 << 31) | 1, 1, 1 << 5]


# ---- /answer ----------------------------------------------------------------------------------------------------
def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": _items(3), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 0)
    yield
    answer.set_llm(None)


REPLY = "The rollback was agreed [Q-11]."


class _PlainLLM:
    model_id = "stub-llm"

    def __init__(self):
        self.calls = []

    def generate_text(self, messages, max_new_tokens):
        self.calls.append({})
        return REPLY


class _PenaltyLLM:
    model_id = "stub-llm"
    supports_penalties = True

    def __init__(self):
        self.calls = []

    def generate_text(self, messages, max_new_tokens, **kw):
        self.calls.append(kw)
        return REPLY

    def token_table(self):
        return TokenTable.from_bytes([b"[", b"Q-", b"the", b"11]"])


def test_penalties_for_merges_the_request_over_the_settings(monkeypatch):
    assert answer.penalties_for(AnswerRequest(query="q")) is None
    assert answer.penalties_for(AnswerRequest(query="q", repetition_penalty=1.0, logit_bias={})) is None
    got = answer.penalties_for(AnswerRequest(query="q", presence_penalty=0.5, logit_bias={"3": -100}))
    assert got == PenaltyParams(presence_penalty=0.5, logit_bias={3: -100.0})
    monkeypatch.setattr(settings, "answer_repetition_penalty", 1.3)
    monkeypatch.setattr(settings, "answer_logit_bias", '{"8": -5}')
    monkeypatch.setattr(settings, "answer_min_new_tokens", 4)
    got = answer.penalties_for(AnswerRequest(query="q", no_repeat_ngram=3))
    assert got == PenaltyParams(repetition_penalty=1.3, no_repeat_ngram=3, logit_bias={8: -5.0}, min_new_tokens=4)
    assert answer.penalties_for(AnswerRequest(query="q", repetition_penalty=1.0, logit_bias={}, min_new_tokens=0)) is None
    for kw in (dict(repetition_penalty=11.0), dict(presence_penalty=-3.0), dict(no_repeat_ngram=1),
               dict(logit_bias={"x": 1.0}), dict(logit_bias={"3": 101.0}), dict(min_new_tokens=-1)):
        with pytest.raises(AnswerRequestError):
            answer.penalties_for(AnswerRequest(query="q", **kw))
    monkeypatch.setattr(settings, "answer_logit_bias", "not json")
    with pytest.raises(AnswerRequestError):
        answer.penalties_for(AnswerRequest(query="q"))


def test_native_model_with_penalties_receives_them_and_the_exemption(pack):
    llm = _PenaltyLLM()
    answer.set_llm(llm)
    assert answer.native_penalties()
    out = answer.answer_question(AnswerRequest(query="what was agreed?", repetition_penalty=1.2, no_repeat_ngram=3,
                                               logit_bias={"2": -INF}, min_new_tokens=2))
    want = PenaltyParams(repetition_penalty=1.2, no_repeat_ngram=3, logit_bias={2: -INF}, min_new_tokens=2)
    assert out["status"] == "ok" and out["notes"]["penalties"] == want.echo()
    assert "penalties_ignored" not in out["notes"]
    (kw,) = llm.calls
    assert kw["penalties"] == want and np.asarray(kw["penalty_exempt"]).tolist() == [0, 1, 3]
    json.dumps(out)


def test_native_model_without_penalties_says_so(pack):
    llm = _PlainLLM()
    answer.set_llm(llm)
    assert not answer.native_penalties()
    out = answer.answer_question(AnswerRequest(query="what was agreed?", frequency_penalty=0.5))
    assert out["status"] == "ok" and llm.calls == [{}]
    assert out["notes"]["penalties"] == dict(PenaltyParams(frequency_penalty=0.5).echo(), applied=False)


def test_a_response_without_the_fields_is_unchanged(pack):
    for llm in (_PenaltyLLM(), _PlainLLM()):
        answer.set_llm(llm)
        out = answer.answer_question(AnswerRequest(query="what was agreed?"))
        assert llm.calls == [{}]
        assert out == {"query_id": "00000000-0000-0000-0000-000000000001", "answer": REPLY, "status": "ok",
                       "citations": [{"evidence_id": "Q-11", "call_id": "call-1"}], "repairs": 0, "model": "stub-llm",
                       "notes": {"evidence_items": 3, "dropped_evidence": 0, "llm_calls": 1,
                                 "validator": {"valid": True, "sentences": 1, "uncited": [], "unknown_ids": [],
                                               "cited": ["Q-11"]}}}
    # a neutral value named in the request is no different
    out = answer.answer_question(AnswerRequest(query="what was agreed?", repetition_penalty=1.0, presence_penalty=0.0))
    assert "penalties" not in out["notes"] and llm.calls[-1] == {}


def test_http_body_carries_the_three_standard_knobs(pack, monkeypatch):
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.local/v1")
    bodies = []

    def post(url, headers, body, timeout_s):
        bodies.append(body)
        return 200, json.dumps({"choices": [{"message": {"content": REPLY}}], "model": "served"})

    monkeypatch.setattr(answer, "_post_json", post)
    out = answer.answer_question(AnswerRequest(query="what was agreed?"))
    assert set(bodies[0]) == {"model", "messages", "temperature", "max_tokens"} and "penalties" not in out["notes"]
    out = answer.answer_question(AnswerRequest(query="what was agreed?", presence_penalty=0.5, frequency_penalty=-0.25,
                                               logit_bias={"7": -INF, "9": 3.5}))
    body = bodies[1]
    assert body["presence_penalty"] == 0.5 and body["frequency_penalty"] == -0.25
    assert body["logit_bias"] == {"7": -100.0, "9": 3.5}
    assert "penalties_ignored" not in out["notes"] and out["notes"]["penalties"]["presence_penalty"] == 0.5
    out = answer.answer_question(AnswerRequest(query="what was agreed?", repetition_penalty=1.3, no_repeat_ngram=2,
                                               min_new_tokens=3))
    body = bodies[2]
    assert body["presence_penalty"] == 0.0 and body["frequency_penalty"] == 0.0 and "logit_bias" not in body
    assert "repetition_penalty" not in body and "no_repeat_ngram" not in body and "min_new_tokens" not in body
    assert out["notes"]["penalties_ignored"] == ["repetition_penalty", "no_repeat_ngram", "min_new_tokens"]
    assert out["status"] == "ok" and out["model"] == "served"


def test_gateway_route_takes_the_fields(pack):
    from fastapi.testclient import TestClient
    from cadence_rag_amd import gateway
    llm = _PenaltyLLM()
    answer.set_llm(llm)
    client = TestClient(gateway.app)
    r = client.post("/answer", json={"query": "what was agreed?", "repetition_penalty": 1.5, "logit_bias": {"2": -50}})
    assert r.status_code == 200, r.text
    assert r.json()["notes"]["penalties"]["repetition_penalty"] == 1.5
    assert llm.calls[0]["penalties"] == PenaltyParams(repetition_penalty=1.5, logit_bias={2: -50.0})
    assert client.post("/answer", json={"query": "q", "repetition_penalty": 11}).status_code == 422
    assert client.post("/answer", json={"query": "q", "no_repeat_ngram": 1}).status_code == 422
    assert client.post("/answer", json={"query": "q", "logit_bias": {"2": 500}}).status_code == 422
