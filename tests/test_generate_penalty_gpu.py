"""Repetition control in the generator, on the tiny checkpoint: a neutral PenaltyParams is the plain code path; a
penalised run -- greedy, sampled, under the citation grammar -- equals a hand loop of prefill / step with the host rule
(penalties.adjust_host) on the downloaded logits, and differs from its unpenalised twin; speculate=4 returns the ids of
speculate=0 whatever is drafted; generate_samples equals separate generate calls on the same streams; no_repeat_ngram=2
leaves no bigram twice; logprobs keeps scoring the raw logits; /answer echoes the parameters."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from cadence_rag_amd.grammar import KIND_STOP, TokenGrammar, allowed_tokens_host, argmax_host, citation_grammar, next_state_host
from cadence_rag_amd.penalties import CITATION_ALPHABET, PenaltyParams, adjust_host, bias_list, exempt_ids
from cadence_rag_amd.sampling import SamplingParams

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEW = 32
TEXTS = ["the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
         "gateway and the billing service after the upgrade",
         "ticket ABC-123 tracks the rollback to version v1.2.3 and the follow up call next week, the agent confirmed the "
         "refund and scheduled a call back for tuesday morning"]
STRONG = PenaltyParams(repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=1.0, no_repeat_ngram=3,
                       logit_bias={101: -100.0, 7: 2.0}, min_new_tokens=6)


@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """The tiny checkpoint (2 random layers, byte-level BPE of 384 ids), its embedding table as the head."""
    from tiny_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    root = tmp_path_factory.mktemp("penalty_tiny")
    build_checkpoint(root)
    enc = Qwen3Encoder.from_pretrained(str(root), DEV, max_length=2048)
    return Qwen3Generator(enc, enc.embed, enc.tokenizer, max_context=2048, max_seqs=4, model_id="tiny")


@pytest.fixture(scope="module")
def prompts(generator):
    return [generator.tokenizer.encode(t, add_special_tokens=False) for t in TEXTS]


def _grammar(gen):
    return TokenGrammar(citation_grammar(["Q-12", "A-45"]), gen.token_table())


def hand_loop(gen, prompts, params, stop, new=NEW, draw=None, streams=None, g=None, exempt=None, keep_logits=False):
    """generate(penalties=params) by hand: prefill / step, every row downloaded, adjusted by the host rule over the
    prompt and the ids picked so far, and picked on the adjusted row -- the host argmax, ops.sample on the uploaded
    adjusted rows, or the host argmax over the tokens the automaton allows.  Returns (ids, the raw rows of every pick)."""
    from cadence_rag_amd.encoder import ops
    n, vocab = len(prompts), gen.cfg.vocab_size
    logits = gen.prefill(prompts)
    hist = [list(p) for p in prompts]
    out, live = [[] for _ in range(n)], list(range(n))
    state = [g.dfa.start if g else 0] * n
    raw = [[] for _ in range(n)]
    for j in range(new):
        rows = logits.float().cpu().numpy()
        adjusted, picked = [], []
        for k, b in enumerate(live):
            adj, tok = adjust_host(rows[k], hist[b], len(prompts[b]), params, exempt=exempt,
                                   bias=bias_list(params, j, stop, vocab))
            if g is not None and draw is None:
                tok = argmax_host(adj, allowed_tokens_host(g.dfa, g.table, state[b]))
            adjusted.append(adj)
            picked.append(tok)
            raw[b].append(rows[k])
        if draw is not None:
            token = torch.empty(len(live), dtype=torch.int32, device=DEV)
            ops.sample(torch.from_numpy(np.stack(adjusted)).to(DEV), draw, j, [streams[b] for b in live], token)
            picked = token.tolist()
        feed, keep = [], []
        for b, t in zip(live, picked):
            if g is not None and t >= 0 and g.table.kind[t] == KIND_STOP:
                continue
            if t < 0 or t in stop:
                continue
            if g is not None:
                state[b] = next_state_host(g.dfa, g.table, state[b], t)
            out[b].append(int(t))
            hist[b].append(int(t))
            if len(out[b]) < new:
                keep.append(b)
                feed.append(int(t))
        live = keep
        if not live:
            break
        _, logits = gen.step(feed, slots=live)
    gen.live = []
    return out, raw


def test_a_neutral_value_is_the_plain_code_path(gpu, generator, prompts, monkeypatch):
    from cadence_rag_amd.encoder import ops
    gen = generator
    assert gen.supports_penalties is True
    calls = []
    real = ops.adjust_logits
    monkeypatch.setattr(ops, "adjust_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain = gen.generate(prompts, NEW, gen.stop_ids())
    assert gen.generate(prompts, NEW, gen.stop_ids(), penalties=PenaltyParams()) == plain
    assert gen.generate(prompts, NEW, gen.stop_ids(), penalties=[PenaltyParams(), None]) == plain
    assert gen.generate(prompts, NEW, gen.stop_ids(), penalties=PenaltyParams(repetition_penalty=1.0, logit_bias={}),
                        penalty_exempt=[1, 2, 3]) == plain
    assert not calls and "_adjust_bufs" not in gen.__dict__          # nothing launched, nothing allocated
    gen.generate(prompts, 2, gen.stop_ids(), penalties=STRONG)
    assert len(calls) == 2
    with pytest.raises(ValueError):
        gen.generate(prompts, 2, penalties=[STRONG])
    with pytest.raises(ValueError):
        gen.generate(prompts, 2, penalties="strong")
    with pytest.raises(ValueError):
        gen.generate_samples(prompts[0], 2, 2, penalties=[STRONG, STRONG])


def test_a_penalised_greedy_run_equals_the_hand_loop(gpu, generator, prompts):
    gen, stop = generator, generator.stop_ids()
    plain = gen.generate(prompts, NEW, stop)
    got = gen.generate(prompts, NEW, stop, penalties=STRONG)
    by_hand, _ = hand_loop(gen, prompts, STRONG, stop)
    assert got == by_hand
    assert all(a != b for a, b in zip(got, plain)), "the penalties changed nothing"
    assert all(len(o) >= STRONG.min_new_tokens and 101 not in o for o in got)
    # one value per prompt, a neutral one among them (without stop ids both rows run to the end in every call: the
    # same batch shapes); and the exempt ids
    mixed = gen.generate(prompts, NEW, penalties=[None, STRONG])
    assert mixed == [gen.generate(prompts, NEW)[0], gen.generate(prompts, NEW, penalties=STRONG)[1]]
    exempt = sorted(set(got[0][:8]) | set(prompts[0][:10]))
    freed = gen.generate(prompts, NEW, stop, penalties=STRONG, penalty_exempt=exempt)
    assert freed == hand_loop(gen, prompts, STRONG, stop, exempt=exempt)[0] and freed != got


def test_a_penalised_sampled_run_equals_the_hand_loop(gpu, generator, prompts):
    gen, stop = generator, generator.stop_ids()
    draw = SamplingParams(temperature=0.8, top_k=30, top_p=0.95, seed=11)
    streams = [4, 9]
    plain = gen.generate(prompts, NEW, stop, sampling=draw, streams=streams)
    got = gen.generate(prompts, NEW, stop, sampling=draw, streams=streams, penalties=STRONG)
    by_hand, _ = hand_loop(gen, prompts, STRONG, stop, draw=draw, streams=streams)
    assert got == by_hand
    assert all(a != b for a, b in zip(got, plain)), "the penalties changed nothing"


def test_a_penalised_run_under_the_grammar_equals_the_hand_loop(gpu, generator, prompts):
    gen, stop, g = generator, generator.stop_ids(), _grammar(generator)
    params = PenaltyParams(repetition_penalty=1.8, presence_penalty=1.5, frequency_penalty=1.0, no_repeat_ngram=2)
    plain = gen.generate(prompts, NEW, stop, grammar=g)
    got = gen.generate(prompts, NEW, stop, grammar=g, penalties=params)
    by_hand, _ = hand_loop(gen, prompts, params, stop, g=g)
    assert got == by_hand
    assert all(a != b for a, b in zip(got, plain)), "the penalties changed nothing"
    # with the citation alphabet exempt the brackets and digits are never penalised
    exempt = exempt_ids(g.table, CITATION_ALPHABET)
    assert exempt.size > 0
    freed = gen.generate(prompts, NEW, stop, grammar=g, penalties=params, penalty_exempt=exempt)
    assert freed == hand_loop(gen, prompts, params, stop, g=g, exempt=exempt)[0]


def test_speculation_returns_the_ids_of_the_plain_loop(gpu, generator, prompts):
    gen, stop, prompt = generator, generator.stop_ids(), prompts[1]
    ref = gen.generate([prompt], NEW, stop, penalties=STRONG)[0]
    assert len(ref) > 8

    def knows(ids, max_draft):      # the continuation itself: every draft is right
        at = len(ids) - len(prompt)
        return list(ref[at:at + max_draft])

    def wrong(ids, max_draft):
        at = len(ids) - len(prompt)
        return [(t + 1) % gen.cfg.vocab_size for t in ref[at:at + max_draft]]

    assert gen.generate([prompt], NEW, stop, penalties=STRONG, speculate=4, drafter=knows) == [ref]
    stats = gen.last_speculation
    assert stats["accepted"][0] > 0 and stats["forwards"] < len(ref), stats
    assert gen.generate([prompt], NEW, stop, penalties=STRONG, speculate=4, drafter=wrong) == [ref]
    assert gen.last_speculation["accepted"][0] == 0 and gen.last_speculation["drafted"][0] > 0
    # both prompts at once, the default prompt-lookup drafter
    both = gen.generate(prompts, NEW, stop, penalties=STRONG)
    assert gen.generate(prompts, NEW, stop, penalties=STRONG, speculate=4) == both


def test_generate_samples_equals_separate_generate_calls(gpu, generator, prompts):
    gen, stop, prompt = generator, generator.stop_ids(), prompts[0]
    draw = SamplingParams(temperature=1.0, top_k=40, seed=3)
    streams = [5, 1, 8]
    got = gen.generate_samples(prompt, 3, NEW, stop, sampling=draw, streams=streams, penalties=STRONG)
    want = [gen.generate([prompt], NEW, stop, sampling=draw, streams=[s], penalties=STRONG)[0] for s in streams]
    assert got == want and len({tuple(o) for o in got}) == 3
    assert got != gen.generate_samples(prompt, 3, NEW, stop, sampling=draw, streams=streams)


def test_no_bigram_twice(gpu, generator, prompts):
    gen = generator
    draw = SamplingParams(temperature=0.3, seed=2)
    plain = gen.generate(prompts, NEW)
    assert any(len(set(zip(o, o[1:]))) < len(o) - 1 for o in plain), "the unpenalised run repeats no bigram"
    for kw in ({}, {"sampling": draw}):
        for o in gen.generate(prompts, NEW, penalties=PenaltyParams(no_repeat_ngram=2), **kw):
            pairs = list(zip(o, o[1:]))
            assert len(o) == NEW and len(set(pairs)) == len(pairs)


def test_logprobs_score_the_raw_logits(gpu, generator, prompts):
    from cadence_rag_amd.encoder.generate import score_rows
    gen, stop = generator, generator.stop_ids()
    got = gen.generate(prompts, NEW, stop, penalties=STRONG, logprobs=3)
    records = gen.last_logprobs
    by_hand, raw = hand_loop(gen, prompts, STRONG, stop)
    assert got == by_hand and [[r.token for r in recs] for recs in records] == got
    for b, recs in enumerate(records):
        rows = torch.from_numpy(np.stack(raw[b][:len(recs)])).to(DEV)
        for lo in range(0, len(recs), 8):
            token = torch.tensor(got[b][lo:lo + 8], dtype=torch.int32).to(DEV)
            want = score_rows(rows[lo:lo + 8].contiguous(), token, 3)
            assert recs[lo:lo + 8] == want, f"prompt {b}, tokens {lo}.."
    # a penalised token is not always the model's first choice
    assert any(r.rank > 1 for recs in records for r in recs)


def test_answer_echoes_the_parameters(gpu, generator, monkeypatch):
    from cadence_rag_amd import answer, retrieve
    from cadence_rag_amd.config import settings
    from cadence_rag_amd.encoder import ops
    items = [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
              "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(3)]

    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": [dict(i) for i in items], "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 16)
    monkeypatch.setattr(settings, "answer_max_repairs", 0)
    monkeypatch.setattr(settings, "answer_constrained", True)
    calls = []
    real = ops.adjust_logits
    monkeypatch.setattr(ops, "adjust_logits", lambda *a, **k: (calls.append(k.get("exempt_bits")), real(*a, **k))[1])
    answer.set_llm(generator)
    try:
        assert answer.native_penalties()
        plain = answer.answer_question(answer.AnswerRequest(query="what holds?"))
        assert "penalties" not in plain["notes"] and not calls
        out = answer.answer_question(answer.AnswerRequest(query="what holds?", repetition_penalty=1.4, no_repeat_ngram=3,
                                                          frequency_penalty=0.5, min_new_tokens=4))
    finally:
        answer.set_llm(None)
    want = PenaltyParams(repetition_penalty=1.4, no_repeat_ngram=3, frequency_penalty=0.5, min_new_tokens=4)
    assert out["notes"]["penalties"] == want.echo() and "penalties_ignored" not in out["notes"]
    assert calls and all(bits is not None for bits in calls)          # the citation alphabet went along as exempt
    print(f"plain {plain['status']}: {plain['answer']!r}; penalised {out['status']}: {out['answer']!r}")
