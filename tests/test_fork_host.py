"""Several candidates per /answer attempt, on the host: the selection rule over a stub model that draws n replies in one
call (its four branches, the noise streams a * n + i, notes.samples), one sample = the responses of today, the refusal
of n greedy copies before anything is retrieved, the fall-back to one candidate, and the gateway model's bounds."""
from __future__ import annotations

import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerRequest, AnswerRequestError
from cadence_rag_amd.config import settings

GOOD = "The rollback was agreed [Q-11]. The summary says so [A-45]."
GOOD2 = "It was agreed [Q-10]."
BAD = "The rollback was agreed."
BAD2 = "Trust me [Q-99]."
NONE = "INSUFFICIENT_EVIDENCE"


def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    """retrieve_evidence replaced by a fixed pack (one artifact, three quotes); records the requests it was given."""
    state = {"requests": []}

    def fake(request, backend=None):
        state["requests"].append(request)
        art = {"evidence_id": "A-45", "call_id": "call-9", "artifact_id": 4, "artifact_chunk_id": 45, "kind": "summary",
               "snippet": "the summary", "why_relevant": "dense"}
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [art], "quotes": _items(3), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    yield state
    answer.set_llm(None)


class _OneReply:
    """A sampling model without generate_text_samples: call k returns replies[k] (the last one again afterwards)."""
    model_id = "stub-llm"
    supports_sampling = True

    def __init__(self, replies):
        self.replies, self.calls = list(replies), []

    def generate_text(self, messages, max_new_tokens, **kw):
        self.calls.append({"messages": [dict(m) for m in messages], **kw})
        return self.replies[min(len(self.calls) - 1, len(self.replies) - 1)]


class _Samples(_OneReply):
    """... with it: `batches[k]` are the candidates of call k.  last_reuse as Qwen3Generator.generate_samples leaves it."""
    supports_samples = True

    def __init__(self, batches, replies=(GOOD,), reused=0):
        super().__init__(replies)
        self.batches, self.sample_calls, self.reused, self.last_reuse = [list(b) for b in batches], [], reused, None

    def generate_text_samples(self, messages, n, max_new_tokens, grammar=None, sampling=None, streams=None):
        self.sample_calls.append({"messages": [dict(m) for m in messages], "n": n, "sampling": sampling,
                                  "streams": list(streams), "grammar": grammar})
        self.last_reuse = {"reused": [self.reused] * n, "computed": [100 - self.reused] * n}
        batch = self.batches[min(len(self.sample_calls) - 1, len(self.batches) - 1)]
        assert len(batch) == n
        return list(batch)


def _ask(llm, **fields):
    answer.set_llm(llm)
    return answer.answer_question(AnswerRequest(query="what was agreed?", **fields))


def test_the_first_valid_candidate_is_the_answer(pack):
    llm = _Samples([[BAD, NONE, GOOD, GOOD2]], reused=40)
    out = _ask(llm, samples=4, temperature=0.8, seed=5)
    assert out["status"] == "ok" and out["answer"] == GOOD and out["repairs"] == 0
    assert out["citations"] == [{"evidence_id": "Q-11", "call_id": "call-1"}, {"evidence_id": "A-45", "call_id": "call-9"}]
    assert out["notes"]["samples"] == {"drawn": 4, "valid": 2, "chosen": 2}
    assert out["notes"]["llm_calls"] == 1 and out["notes"]["validator"]["valid"]
    assert out["notes"]["prefix_reused_tokens"] == 40          # the prompt's rows were reused once, not once per candidate
    assert llm.calls == [] and len(llm.sample_calls) == 1
    call = llm.sample_calls[0]
    assert call["n"] == 4 and call["streams"] == [0, 1, 2, 3]
    assert call["sampling"].temperature == 0.8 and call["sampling"].seed == 5
    assert out["notes"]["sampling"]["temperature"] == 0.8


def test_every_candidate_insufficient_is_insufficient_evidence(pack):
    llm = _Samples([[NONE, NONE + ".", "**" + NONE + "**"]])
    out = _ask(llm, samples=3, temperature=1.0)
    assert out["status"] == "insufficient_evidence" and out["answer"] is None and out["repairs"] == 0
    assert out["notes"]["samples"] == {"drawn": 3, "valid": 0, "chosen": None}
    assert out["notes"]["llm_calls"] == 1 and out["notes"]["validator"] is None


def test_the_repair_turn_quotes_the_first_failing_candidate_that_is_not_insufficient(pack):
    llm = _Samples([[NONE, BAD, BAD2], [BAD2, GOOD2, NONE]])
    out = _ask(llm, samples=3, temperature=1.0)
    assert out["status"] == "ok" and out["answer"] == GOOD2 and out["repairs"] == 1
    assert out["notes"]["samples"] == {"drawn": 3, "valid": 1, "chosen": 1}     # of the last attempt
    assert out["notes"]["llm_calls"] == 2                                       # calls, not candidates
    first, second = llm.sample_calls
    assert [m["role"] for m in first["messages"]] == ["system", "user"]
    assert [m["role"] for m in second["messages"]] == ["system", "user", "assistant", "user"]
    assert second["messages"][2]["content"] == BAD                              # not NONE (index 0), not BAD2 (index 2)
    assert BAD in second["messages"][3]["content"]
    assert first["streams"] == [0, 1, 2] and second["streams"] == [3, 4, 5]     # attempt a draws on a * n + i


def test_no_candidate_ever_passes_fails_closed(pack):
    llm = _Samples([[BAD2, NONE]])
    out = _ask(llm, samples=2, temperature=1.0)
    assert out["status"] == "citation_check_failed" and out["answer"] is None and out["repairs"] == 2
    assert [c["streams"] for c in llm.sample_calls] == [[0, 1], [2, 3], [4, 5]]
    assert out["notes"]["samples"] == {"drawn": 2, "valid": 0, "chosen": None}
    assert out["notes"]["validator"]["unknown_ids"] == ["Q-99"] and out["notes"]["llm_calls"] == 3


def test_one_sample_is_the_response_of_today(pack, monkeypatch):
    """samples unset, samples = 1 and ANSWER_SAMPLES = 1 go through generate_text with the same keywords and give the
    same response, key for key; no notes.samples."""
    outs, calls = [], []
    for fields in ({}, {"samples": 1}):
        llm = _Samples([[GOOD]], replies=[BAD, GOOD])
        outs.append(_ask(llm, temperature=0.7, **fields))
        assert llm.sample_calls == []
        calls.append(llm.calls)
    assert outs[0] == outs[1] and calls[0] == calls[1]
    assert outs[0]["status"] == "ok" and outs[0]["repairs"] == 1
    assert [c["stream"] for c in calls[0]] == [0, 1]
    assert sorted(outs[0]["notes"]) == ["dropped_evidence", "evidence_items", "llm_calls", "sampling", "validator"]
    greedy = _ask(_Samples([[GOOD]], replies=[GOOD]), samples=1)                # greedy: no sampling keyword at all
    assert sorted(greedy["notes"]) == ["dropped_evidence", "evidence_items", "llm_calls", "validator"]
    assert set(answer.get_llm().calls[0]) == {"messages"}


def test_the_setting_supplies_the_default_and_the_request_overrides_it(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_samples", 3)
    llm = _Samples([[GOOD, GOOD, GOOD]])
    assert _ask(llm, temperature=0.5)["notes"]["samples"] == {"drawn": 3, "valid": 3, "chosen": 0}
    llm = _Samples([[GOOD, GOOD]])
    assert _ask(llm, temperature=0.5, samples=2)["notes"]["samples"]["drawn"] == 2
    assert "samples" not in _ask(_Samples([[GOOD]]), temperature=0.5, samples=1)["notes"]


def test_greedy_copies_and_counts_out_of_range_are_refused_before_retrieval(pack, monkeypatch):
    answer.set_llm(_Samples([[GOOD, GOOD]]))
    for fields in ({"samples": 2}, {"samples": 2, "temperature": 0.0}, {"samples": 0, "temperature": 0.5},
                   {"samples": 9, "temperature": 0.5}, {"samples": -1}):
        with pytest.raises(AnswerRequestError):
            answer.answer_question(AnswerRequest(query="q", **fields))
    monkeypatch.setattr(settings, "answer_samples", 4)                          # the default alone, greedy
    with pytest.raises(AnswerRequestError):
        answer.answer_question(AnswerRequest(query="q"))
    assert pack["requests"] == [] and answer.get_llm().sample_calls == []
    assert answer.samples_for(AnswerRequest(query="q", temperature=0.5)) == 4
    assert answer.samples_for(AnswerRequest(query="q", samples=1)) == 1


def test_a_model_without_the_attribute_gives_one_candidate(pack):
    llm = _OneReply([GOOD])
    out = _ask(llm, samples=4, temperature=0.8)
    assert out["status"] == "ok" and out["notes"]["samples"] == {"applied": False}
    assert len(llm.calls) == 1 and llm.calls[0]["stream"] == 0


def test_an_http_backend_gives_one_candidate(pack, monkeypatch):
    import json
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.invalid/v1")
    posted = []

    def post(url, headers, body, timeout_s):
        posted.append(body)
        return 200, json.dumps({"choices": [{"message": {"content": GOOD}}], "model": "remote"})

    monkeypatch.setattr(answer, "_post_json", post)
    answer.set_llm(_Samples([[GOOD, GOOD]]))                                    # registered, but the backend is not native
    out = answer.answer_question(AnswerRequest(query="q", samples=2, temperature=0.8))
    assert out["status"] == "ok" and out["model"] == "remote" and out["notes"]["samples"] == {"applied": False}
    assert len(posted) == 1 and posted[0]["temperature"] == 0.8 and answer.get_llm().sample_calls == []


def test_kv_cache_fork_is_host_bookkeeping():
    """KvCache.fork on a CPU cache: what the children hold, the logical rows of keys / values, the refusals, and the rule
    that empties the children of a slot whose shared rows go."""
    import torch

    from cadence_rag_amd.encoder.generate import KvCache
    cache = KvCache(1, 5, 2, 16, "cpu")
    cache.k.copy_(torch.arange(cache.k.numel()).view_as(cache.k) % 251)
    cache.v.copy_(cache.k + 1)
    assert cache.parent == [0, 1, 2, 3, 4] and cache.shared == [0] * 5
    cache.lens[0] = 6
    plain = cache.keys(0, 0)
    assert plain.data_ptr() == cache.k[0, 0].data_ptr() and plain.shape == (6, 2, 128)      # not forked: the view it was
    cache.fork(0, [2, 3])
    assert cache.lens == [6, 0, 6, 6, 0] and cache.parent == [0, 1, 0, 0, 4] and cache.shared == [0, 0, 6, 6, 0]
    assert cache.children(0) == [2, 3] and cache.forked(2) and not cache.forked(0)
    cache.lens[2] = 9                                                                       # three rows of its own
    want = torch.cat([cache.k[0, 0, :, :6], cache.k[0, 2, :, 6:9]], dim=1).transpose(0, 1)
    assert torch.equal(cache.keys(0, 2), want) and torch.equal(cache.values(0, 2), want + 1)
    for src, dsts in ((0, [0]), (0, [1, 1]), (1, [0]), (0, [5]), (2, [4])):                 # (2: a child with own rows)
        with pytest.raises(ValueError):
            cache.fork(src, dsts)
    cache.fork(3, [4])                                                                      # a child without rows of its
    assert cache.parent[4] == 0 and cache.shared[4] == 6 and cache.lens[4] == 6             # own: one deep, under slot 0
    cache.release(0, 6)                                                                     # rows 6.. go: nobody shares
    assert cache.children(0) == [2, 3, 4]
    cache.release(0, 5)
    assert cache.children(0) == [] and cache.lens == [6, 0, 0, 0, 0] and cache.parent == [0, 1, 2, 3, 4]
    cache.fork(1, [2])                                                                      # an empty source: nothing shared
    assert not cache.forked(2) and cache.lens[2] == 0


def test_gateway_bounds(pack):
    pytest.importorskip("fastapi")
    from pydantic import ValidationError

    from cadence_rag_amd import gateway
    assert gateway.AnswerRequestModel(query="q").samples is None
    assert gateway.AnswerRequestModel(query="q", samples=8).samples == 8
    for bad in (0, 9, -3):
        with pytest.raises(ValidationError):
            gateway.AnswerRequestModel(query="q", samples=bad)
    from fastapi.testclient import TestClient
    client = TestClient(gateway.app)
    answer.set_llm(_Samples([[BAD, GOOD2]]))
    body = client.post("/answer", json={"query": "what was agreed?", "samples": 2, "temperature": 0.9}).json()
    assert body["status"] == "ok" and body["answer"] == GOOD2 and body["notes"]["samples"]["chosen"] == 1
    assert client.post("/answer", json={"query": "q", "samples": 2}).status_code == 422     # greedy copies
    assert client.post("/answer", json={"query": "q", "samples": 9, "temperature": 0.9}).status_code == 422
