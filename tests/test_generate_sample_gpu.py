"""Qwen3Generator.generate(sampling=...) on the tiny checkpoint: temperature 0 is the greedy path (with and without a
grammar, with reuse_prefix); a sampled run equals a hand loop of prefill / step / ops.sample; seeds repeat and differ;
under the citation grammar every drawn token is one the tracked state allows and accepted outputs pass the validator,
and a sampled run equals a hand loop of prefill / step / ops.grammar_argmax / ops.sample / ops.grammar_advance;
/answer reports the parameters."""
from __future__ import annotations

import pytest
import torch

from cadence_rag_amd import grammar
from cadence_rag_amd.grammar import TokenGrammar, allowed_tokens_host, citation_grammar, next_state_host
from cadence_rag_amd.sampling import SamplingParams

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEW = 32
TEXTS = ["the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
         "gateway and the billing service after the upgrade",
         "ticket ABC-123 tracks the rollback to version v1.2.3 and the follow up call next week, the agent confirmed the "
         "refund and scheduled a call back for tuesday morning, latency went from forty milliseconds to nine hundred",
         "please send the transcript and the action items to the account team, the speaker asked whether the embedding "
         "backfill had finished for all chunks"]
PRIMED = 40


@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """The tiny checkpoint (2 random layers, byte-level BPE of 384 ids), its embedding table as the head."""
    from tiny_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    root = tmp_path_factory.mktemp("sample_tiny")
    build_checkpoint(root)
    enc = Qwen3Encoder.from_pretrained(str(root), DEV, max_length=2048)
    return Qwen3Generator(enc, enc.embed, enc.tokenizer, max_context=2048, max_seqs=4, model_id="tiny")


@pytest.fixture(scope="module")
def prompts(generator):
    return [generator.tokenizer.encode(t, add_special_tokens=False) for t in TEXTS]


def test_temperature_zero_is_the_greedy_path(gpu, generator, prompts):
    gen = generator
    assert gen.supports_sampling is True
    greedy = SamplingParams(temperature=0, top_k=5, top_p=0.5, seed=99)
    want = gen.generate(prompts, NEW)
    assert gen.generate(prompts, NEW, sampling=greedy) == want
    assert gen.generate(prompts, NEW, sampling=[greedy] * 3, streams=[5, 6, 7]) == want
    g = TokenGrammar(citation_grammar(["Q-12", "A-45"]), gen.token_table())
    want_g = gen.generate(prompts, NEW, gen.stop_ids(), grammar=g)
    accepted = gen.last_grammar
    assert gen.generate(prompts, NEW, gen.stop_ids(), grammar=g, sampling=greedy) == want_g
    assert gen.last_grammar == accepted and want_g != want
    gen.prefill([p[:PRIMED] for p in prompts])
    assert gen.generate(prompts, NEW, reuse_prefix=True, sampling=greedy) == want
    assert gen.last_reuse["reused"] == [PRIMED] * 3
    gen.prefill([p[:PRIMED] for p in prompts])
    assert gen.generate(prompts, NEW, gen.stop_ids(), reuse_prefix=True, grammar=g, sampling=greedy) == want_g


def test_a_sampled_run_equals_the_hand_loop(gpu, generator, prompts):
    from cadence_rag_amd.encoder import ops
    gen = generator
    params = [SamplingParams(0.8, top_k=40, seed=7), SamplingParams(1.0, top_p=0.9, seed=7),
              SamplingParams(0.6, min_p=0.05, seed=7)]
    streams = [3, 0, 11]
    got = gen.generate(prompts, 12, sampling=params, streams=streams)
    assert [len(o) for o in got] == [12] * 3
    logits = gen.prefill(prompts)
    by_hand = [[] for _ in prompts]
    token = torch.empty(3, dtype=torch.int32, device=DEV)
    for j in range(12):
        ops.sample(logits, params, j, streams, token)
        for s, t in zip(by_hand, token.tolist()):
            s.append(int(t))
        if j < 11:
            _, logits = gen.step([s[-1] for s in by_hand])
    gen.live = []
    assert got == by_hand
    # the default stream is the prompt's index
    assert gen.generate(prompts, 6, sampling=params[0]) == gen.generate(prompts, 6, sampling=params[0], streams=[0, 1, 2])
    with pytest.raises(ValueError, match="one seed"):
        gen.generate(prompts, 4, sampling=[SamplingParams(1.0, seed=1), SamplingParams(1.0, seed=2), SamplingParams(1.0)])
    with pytest.raises(ValueError, match="one SamplingParams"):
        gen.generate(prompts, 4, sampling=params[:2])


def test_seeds_repeat_and_differ(gpu, generator, prompts):
    gen = generator
    a = gen.generate(prompts, NEW, sampling=SamplingParams(1.0, seed=1))
    assert gen.generate(prompts, NEW, sampling=SamplingParams(1.0, seed=1)) == a
    b = gen.generate(prompts, NEW, sampling=SamplingParams(1.0, seed=2))
    assert all(x != y for x, y in zip(a, b))                      # two seeds part within 32 tokens, for every prompt
    c = gen.generate(prompts, NEW, sampling=SamplingParams(1.0, seed=1), streams=[7, 8, 9])
    assert all(x != y for x, y in zip(a, c))                      # and so do two streams of one seed
    assert a != gen.generate(prompts, NEW)


def test_under_the_grammar_every_drawn_token_is_allowed(gpu, generator, prompts):
    from cadence_rag_amd.answer import validate_citations
    gen = generator
    ids = ["Q-12", "A-45"]
    g = TokenGrammar(citation_grammar(ids), gen.token_table())
    accepted_any = False
    for seed in (1, 2, 3):
        outs = gen.generate(prompts, 48, gen.stop_ids(), grammar=g, sampling=SamplingParams(0.9, top_p=0.95, seed=seed))
        for b, out in enumerate(outs):
            state = g.dfa.start
            for t in out:
                assert allowed_tokens_host(g.dfa, g.table, state)[t] and g.table.kind[t] == grammar.KIND_ORDINARY, (seed, b, t)
                state = next_state_host(g.dfa, g.table, state, t)
            text = b"".join(g.table.token_bytes(t) for t in out).decode("utf-8", "replace")
            print(f"seed {seed} prompt {b}: accepted {gen.last_grammar['accepted'][b]}, {len(out)} tokens, {text!r}")
            if gen.last_grammar["accepted"][b]:
                accepted_any = True
                assert bool(g.dfa.accept[state])
                assert text == "INSUFFICIENT_EVIDENCE" or validate_citations(text, ids)["valid"], text
            else:
                assert len(out) == 48
    print(f"accepted any: {accepted_any}")


def test_a_sampled_run_under_the_grammar_equals_the_hand_loop(gpu, generator, prompts):
    """The fourth selection mode, token for token: grammar_argmax hands out the bits on a copy of the states, sample draws
    under them with step = the token's index and the prompt's stream, grammar_advance moves the states."""
    from cadence_rag_amd.encoder import ops
    gen, two, new, streams = generator, prompts[:2], 12, [3, 5]
    g = TokenGrammar(citation_grammar(["Q-12", "A-45"]), gen.token_table())
    params = SamplingParams(temperature=1.0, top_k=20, seed=11)
    stop = set(gen.stop_ids())
    got = gen.generate(two, new, gen.stop_ids(), grammar=g, sampling=params, streams=streams)
    got_accepted = gen.last_grammar["accepted"]

    tables = g.table.to(DEV) + g.dfa.to(DEV)
    state = torch.full((2,), int(g.dfa.start), dtype=torch.int32, device=DEV)
    by_hand, accepted, live = [[], []], [False, False], [0, 1]
    logits = gen.prefill(two)
    for j in range(new):
        idx = torch.tensor(live, dtype=torch.int64).to(DEV)
        cur = state.index_select(0, idx)
        token = torch.empty(len(live), dtype=torch.int32, device=DEV)
        bits = torch.empty(len(live), (g.table.vocab + 31) // 32, dtype=torch.int32, device=DEV)
        ops.grammar_argmax(logits, *tables, cur.clone(), token, allowed_bits=bits)
        ops.sample(logits, params, j, [streams[b] for b in live], token, allowed_bits=bits)
        ops.grammar_advance(*tables[:5], cur, token)
        state.index_copy_(0, idx, cur)
        feed, keep = [], []
        for b, t in zip(live, token.tolist()):
            if t >= 0 and g.table.kind[t] == grammar.KIND_STOP:
                accepted[b] = True
            elif t >= 0 and t not in stop:
                by_hand[b].append(t)
                if len(by_hand[b]) < new:
                    keep.append(b)
                    feed.append(t)
        live = keep
        if not live:
            break
        _, logits = gen.step(feed, slots=live)
    gen.live = []
    print(f"by hand: {by_hand}, accepted {accepted}")
    assert got == by_hand and got_accepted == accepted
    assert any(by_hand) and by_hand != gen.generate(two, new, gen.stop_ids(), grammar=g)   # drawn, not the greedy run


def test_answer_reports_the_sampling_parameters(gpu, generator, monkeypatch):
    from cadence_rag_amd import answer, retrieve
    from cadence_rag_amd.config import settings
    items = [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
              "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(3)]

    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": [dict(i) for i in items], "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 16)
    monkeypatch.setattr(settings, "answer_max_repairs", 1)
    monkeypatch.setattr(settings, "answer_constrained", True)
    answer.set_llm(generator)
    try:
        plain = answer.answer_question(answer.AnswerRequest(query="what holds?"))
        out = answer.answer_question(answer.AnswerRequest(query="what holds?", temperature=0.8, top_p=0.9, seed=5))
        again = answer.answer_question(answer.AnswerRequest(query="what holds?", temperature=0.8, top_p=0.9, seed=5))
    finally:
        answer.set_llm(None)
    assert "sampling" not in plain["notes"]
    assert out["notes"]["sampling"] == {"temperature": 0.8, "top_k": 0, "top_p": 0.9, "min_p": 0.0, "seed": 5}
    assert out["notes"]["constrained"] is True and out["status"] in ("ok", "insufficient_evidence", "citation_check_failed")
    report = out["notes"]["validator"]
    assert report is None or report["unknown_ids"] == []
    assert (again["status"], again["answer"], again["notes"]["validator"]) == \
        (out["status"], out["answer"], out["notes"]["validator"])          # one seed, one answer
