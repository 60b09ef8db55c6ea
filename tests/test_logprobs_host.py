"""Token log-probabilities on the host: logprobs_host -- the rule crag_enc_logprobs is tested against -- held to a plain
fp64 log-softmax and to hand-made edge rows; and /answer's use of the records over a stub model: ranking candidates by
mean token log-probability, the notes, the defaults that change nothing, the refusal, the HTTP backend."""
from __future__ import annotations

import json
import math

import numpy as np
import pytest

from cadence_rag_amd import answer, retrieve
from cadence_rag_amd.answer import AnswerRequest, AnswerRequestError
from cadence_rag_amd.config import settings
from cadence_rag_amd.logprobs import MAX_TOP, TokenLogprob, error_bar, logprobs_host, mean_logprob, summarise


# ---- the rule -----------------------------------------------------------------------------------------------------------
def _log_softmax(row: np.ndarray) -> np.ndarray:
    x = row.astype(np.float64)
    return x - math.log(float(np.exp(x).sum()))       # no maximum taken out: small rows, moderate values


@pytest.mark.parametrize("v", [1, 2, 17, 300])
def test_against_a_plain_log_softmax(v):
    rng = np.random.default_rng(v)
    for _ in range(5):
        row = (rng.standard_normal(v) * 2).astype(np.float32)
        want = _log_softmax(row)
        token = int(rng.integers(0, v))
        n_top = min(MAX_TOP, v)
        got = logprobs_host(row, token, None, n_top)
        assert got.logprob == pytest.approx(want[token], abs=1e-12)
        assert got.lse_all == pytest.approx(math.log(float(np.exp(row.astype(np.float64)).sum())), abs=1e-12)
        assert got.lse_allowed == got.lse_all and got.allowed_logmass == 0.0
        assert got.rank == 1 + int((row > row[token]).sum())
        order = sorted(range(v), key=lambda i: (-float(row[i]), i))[:n_top]
        assert got.top_id.tolist() == order
        assert np.allclose(got.top_logprob, want[order], atol=1e-12, rtol=0)
        assert math.exp(got.logprob) <= 1.0 + 1e-12


def test_nan_entries_are_no_candidates_and_minus_inf_entries_are():
    row = np.array([1.0, np.nan, -np.inf, 2.0, np.nan, 0.5], np.float32)
    got = logprobs_host(row, 3, None, 6)
    z = math.exp(1.0) + math.exp(2.0) + math.exp(0.5)
    assert got.lse_all == pytest.approx(math.log(z), abs=1e-12) and got.rank == 1
    assert got.top_id.tolist() == [3, 0, 5, 2, -1, -1]
    assert got.top_logprob[3] == -math.inf and np.isnan(got.top_logprob[4:]).all()
    on_inf = logprobs_host(row, 2)
    assert on_inf.logprob == -math.inf and on_inf.rank == 4
    on_nan = logprobs_host(row, 1)
    assert math.isnan(on_nan.logprob) and on_nan.rank == 0


def test_infinite_maxima_empty_sets_and_tokens_outside_the_row():
    row = np.array([0.0, np.inf, 3.0, np.inf], np.float32)
    got = logprobs_host(row, 2, None, 3)
    assert got.lse_all == math.inf and got.logprob == -math.inf and got.rank == 3       # finite - inf
    assert got.top_id.tolist() == [1, 3, 2] and math.isnan(got.top_logprob[0]) and got.top_logprob[2] == -math.inf
    on_max = logprobs_host(row, 3)
    assert math.isnan(on_max.logprob) and on_max.rank == 1                              # inf - inf, still a rank
    nothing = logprobs_host(np.full(4, np.nan, np.float32), 0, None, 2)
    assert nothing.lse_all == -math.inf and math.isnan(nothing.logprob) and nothing.rank == 0
    assert nothing.top_id.tolist() == [-1, -1] and np.isnan(nothing.top_logprob).all()
    only_minus_inf = logprobs_host(np.full(3, -np.inf, np.float32), 1, None, 1)
    assert only_minus_inf.lse_all == -math.inf and math.isnan(only_minus_inf.logprob) and only_minus_inf.rank == 1
    fine = np.array([0.5, 1.5], np.float32)
    for token in (-1, 2):
        out = logprobs_host(fine, token, None, 1)
        assert math.isnan(out.logprob) and out.rank == 0 and out.top_id.tolist() == [1]
    with pytest.raises(ValueError):
        logprobs_host(fine, 0, None, 3)
    with pytest.raises(ValueError):
        logprobs_host(np.zeros(40, np.float32), 0, None, MAX_TOP + 1)


def test_signed_zeros_tie_in_rank_and_equal_logits_go_lowest_id_first():
    row = np.array([0.0, -0.0, 1.0, -0.0, 0.0, 1.0, -1.0], np.float32)
    for token in (0, 1, 3, 4):
        assert logprobs_host(row, token).rank == 3            # only the two 1.0 lie strictly above a zero of either sign
    assert logprobs_host(row, 6).rank == 7 and logprobs_host(row, 5).rank == 1
    got = logprobs_host(row, 0, None, 7)
    assert got.top_id.tolist() == [2, 5, 0, 1, 3, 4, 6]
    assert got.top_logprob[2] == got.top_logprob[3] == got.top_logprob[5]


def test_allowed_logmass_on_a_hand_made_mask():
    row = np.log(np.array([0.1, 0.2, 0.3, 0.4], np.float64)).astype(np.float32)
    mask = np.array([True, False, True, False])
    got = logprobs_host(row, 1, mask, 2)
    assert got.allowed_logmass == pytest.approx(math.log(0.4), abs=1e-6)     # 0.1 + 0.3 of the mass is allowed
    assert got.logprob == pytest.approx(math.log(0.2), abs=1e-6)             # the model's own, mask or not
    assert got.top_id.tolist() == [3, 2]                                     # over all ids, not the allowed ones
    assert logprobs_host(row, 1, np.zeros(4, bool)).lse_allowed == -math.inf
    # allowed ids 50 below the maximum: relative to their own maximum, so the value is finite and exact
    far = np.array([0.0, -50.0, -50.0], np.float32)
    low = logprobs_host(far, 0, np.array([False, True, True]))
    assert low.lse_allowed == pytest.approx(-50.0 + math.log(2.0), abs=1e-12)
    assert low.allowed_logmass == pytest.approx(-50.0 + math.log(2.0) - low.lse_all, abs=1e-12) and low.allowed_logmass < 0
    assert error_bar(-3.0, 10.0, 2.0) == 2.0 ** -24 * (24 + 8 + 10 + 3)


def test_summaries():
    recs = [TokenLogprob(5, -0.5, 1, -0.1, []), TokenLogprob(6, -1.5, 3, -0.3, [])]
    assert mean_logprob(recs) == -1.0 and mean_logprob([]) is None
    assert summarise(recs) == {"tokens": 2, "mean_logprob": -1.0, "min_logprob": -1.5,
                               "mean_allowed_logmass": pytest.approx(-0.2), "min_allowed_logmass": -0.3}
    assert summarise([TokenLogprob(5, -0.5, 1, None, [])]) == {"tokens": 1, "mean_logprob": -0.5, "min_logprob": -0.5}


# ---- /answer ------------------------------------------------------------------------------------------------------------
GOOD = "The rollback was agreed [Q-11]. The summary says so [A-45]."
GOOD2 = "It was agreed [Q-10]."
GOOD3 = "Agreed it was [Q-12]."
BAD = "The rollback was agreed."
BAD2 = "Trust me [Q-99]."
NONE = "INSUFFICIENT_EVIDENCE"


def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        art = {"evidence_id": "A-45", "call_id": "call-9", "artifact_id": 4, "artifact_chunk_id": 45, "kind": "summary",
               "snippet": "the summary", "why_relevant": "dense"}
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [art], "quotes": _items(3), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    yield
    answer.set_llm(None)


def _records(mean: float, n: int = 4, mass=None):
    return [TokenLogprob(7 + k, mean + (0.25 if k % 2 else -0.25), 1 + k, mass, []) for k in range(n)]


class _Scored:
    """A stub of Qwen3Generator's text interface with canned candidates and canned records: batches[k] = [(text, mean
    token logprob)] of call k.  It takes logprobs= only because it says supports_logprobs."""
    model_id = "stub-llm"
    supports_sampling = supports_samples = supports_logprobs = True

    def __init__(self, batches, mass=None):
        self.batches, self.calls, self.mass, self.last_logprobs = [list(b) for b in batches], [], mass, None

    def _next(self, n, kw):
        batch = self.batches[min(len(self.calls), len(self.batches) - 1)]
        self.calls.append(dict(kw, n=n))
        assert len(batch) == n
        self.last_logprobs = [_records(m, mass=self.mass) for _, m in batch] if kw.get("logprobs") is not None else None
        return [t for t, _ in batch]

    def generate_text_samples(self, messages, n, max_new_tokens, **kw):
        return self._next(n, dict(kw, messages=[dict(m) for m in messages]))

    def generate_text(self, messages, max_new_tokens, **kw):
        return self._next(1, dict(kw, messages=[dict(m) for m in messages]))[0]


class _Plain(_Scored):
    supports_logprobs = False

    def generate_text_samples(self, messages, n, max_new_tokens, grammar=None, sampling=None, streams=None):
        return self._next(n, {})

    def generate_text(self, messages, max_new_tokens, grammar=None, sampling=None, stream=0):
        return self._next(1, {})[0]


def _ask(llm, **fields):
    answer.set_llm(llm)
    return answer.answer_question(AnswerRequest(query="what was agreed?", **fields))


FOUR = [(GOOD2, -2.0), (BAD, -0.125), (GOOD, -0.5), (GOOD3, -1.0)]


def test_logprob_ranking_takes_the_best_scoring_valid_candidate_and_first_takes_index_0(pack):
    first = _ask(_Scored([FOUR]), samples=4, temperature=0.8)
    assert first["answer"] == GOOD2 and first["notes"]["samples"] == {"drawn": 4, "valid": 3, "chosen": 0}
    llm = _Scored([FOUR])
    out = _ask(llm, samples=4, temperature=0.8, sample_rank="logprob")
    assert out["status"] == "ok" and out["answer"] == GOOD       # -0.5: the best VALID one; BAD scores higher and fails
    assert out["notes"]["samples"] == {"drawn": 4, "valid": 3, "chosen": 2, "scores": [-2.0, -0.125, -0.5, -1.0],
                                       "ranked": True}
    assert "logprobs" not in out["notes"]                         # ranking alone: the option is off
    assert llm.calls[0]["logprobs"] == 0 and llm.calls[0]["n"] == 4


def test_equal_scores_go_to_the_lower_index(pack):
    out = _ask(_Scored([[(BAD, -0.125), (GOOD3, -0.5), (GOOD, -0.5), (GOOD2, -0.5)]]), samples=4, temperature=0.8,
               sample_rank="logprob")
    assert out["answer"] == GOOD3 and out["notes"]["samples"]["chosen"] == 1


def test_the_repair_turn_quotes_the_best_scoring_candidate_that_tried(pack):
    llm = _Scored([[(NONE, -0.01), (BAD, -3.0), (BAD2, -1.0)], [(GOOD, -1.0), (GOOD2, -0.2), (NONE, -0.1)]])
    out = _ask(llm, samples=3, temperature=1.0, sample_rank="logprob")
    assert out["status"] == "ok" and out["answer"] == GOOD2 and out["repairs"] == 1
    assert llm.calls[1]["messages"][2]["content"] == BAD2         # -1.0 beats -3.0; NONE did not try
    assert out["notes"]["samples"]["chosen"] == 1


def test_the_logprobs_note(pack):
    out = _ask(_Scored([[(GOOD, -0.75)]]), logprobs=True)
    assert out["answer"] == GOOD
    assert out["notes"]["logprobs"] == {"tokens": 4, "mean_logprob": -0.75, "min_logprob": -1.0}
    assert "samples" not in out["notes"]
    grammar = _ask(_Scored([FOUR], mass=-0.125), samples=4, temperature=0.8, sample_rank="logprob", logprobs=True)
    assert grammar["notes"]["logprobs"] == {"tokens": 4, "mean_logprob": -0.5, "min_logprob": -0.75,
                                            "mean_allowed_logmass": -0.125, "min_allowed_logmass": -0.125}
    json.dumps(grammar)                                           # the response stays plain JSON


def test_the_setting_turns_it_on(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_logprobs", True)
    monkeypatch.setattr(settings, "answer_sample_rank", "logprob")
    out = _ask(_Scored([FOUR]), samples=4, temperature=0.8)
    assert out["answer"] == GOOD and out["notes"]["logprobs"]["tokens"] == 4
    off = _ask(_Scored([FOUR]), samples=4, temperature=0.8, logprobs=False, sample_rank="first")
    assert off["answer"] == GOOD2 and "logprobs" not in off["notes"] and "ranked" not in off["notes"]["samples"]


def test_the_defaults_change_nothing(pack):
    """Options absent (a request object that does not even have the fields) against options at their defaults: the same
    bytes, and the model is never handed logprobs=."""
    class Old:   # the request of before: no `logprobs`, no `sample_rank`
        def __init__(self, **kw):
            self.__dict__.update(AnswerRequest(query="what was agreed?", **kw).__dict__)
            del self.logprobs, self.sample_rank

    for fields in (dict(samples=4, temperature=0.8, seed=3), dict()):
        batch = FOUR if fields else [FOUR[2]]
        old_llm, new_llm = _Scored([batch]), _Scored([batch])
        answer.set_llm(old_llm)
        old = answer.answer_question(Old(**fields))
        new = _ask(new_llm, **fields)
        assert json.dumps(old, sort_keys=True) == json.dumps(new, sort_keys=True)
        assert "logprobs" not in new["notes"] and "scores" not in json.dumps(new)
        assert all("logprobs" not in c for c in old_llm.calls + new_llm.calls)


def test_a_bad_sample_rank_is_refused_before_anything_runs(pack):
    llm = _Scored([FOUR])
    for bad in ("best", "", 1, "LOGPROB"):
        with pytest.raises(AnswerRequestError):
            _ask(llm, samples=4, temperature=0.8, sample_rank=bad)
    assert llm.calls == []


def test_logprob_ranking_without_the_means_behaves_as_first(pack):
    one = _ask(_Scored([[(GOOD, -0.75)]]), sample_rank="logprob")                  # one sample
    assert one["answer"] == GOOD and one["notes"]["samples"] == {"ranked": False}
    plain = _ask(_Plain([FOUR]), samples=4, temperature=0.8, sample_rank="logprob", logprobs=True)   # no capability
    assert plain["answer"] == GOOD2
    assert plain["notes"]["samples"] == {"drawn": 4, "valid": 3, "chosen": 0, "ranked": False}
    assert plain["notes"]["logprobs"] == {"applied": False}


def test_the_http_backend_says_not_applied(pack, monkeypatch):
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.invalid/v1")
    sent = []

    def post(url, headers, body, timeout_s):
        sent.append(body)
        return 200, json.dumps({"choices": [{"message": {"content": GOOD}}], "model": "remote"})

    monkeypatch.setattr(answer, "_post_json", post)
    answer.set_llm(_Scored([FOUR]))                               # registered, but the backend is not native
    out = answer.answer_question(AnswerRequest(query="what was agreed?", logprobs=True, sample_rank="logprob"))
    assert out["answer"] == GOOD and out["notes"]["logprobs"] == {"applied": False}
    assert out["notes"]["samples"] == {"ranked": False}
    assert len(sent) == 1 and "logprobs" not in sent[0]


def test_the_gateway_model_carries_the_fields():
    from cadence_rag_amd.gateway import AnswerRequestModel
    m = AnswerRequestModel(query="q", logprobs=True, sample_rank="logprob")
    assert m.logprobs is True and m.sample_rank == "logprob"
    d = AnswerRequestModel(query="q")
    assert d.logprobs is None and d.sample_rank is None
