"""Token log-probabilities in the generator, on tiny checkpoints: generate(logprobs=n) returns the ids it returned
without, in the four picking modes, under speculation and in generate_samples; its records equal the host rule
(logprobs.logprobs_host) on the logits each pick read -- prefill and step replayed by hand, the same tensors the kernel
read -- with rank and top ids exact and the floats inside logprobs.error_bar; under the grammar allowed_logmass is held
to the host mask; under speculation there is one record per returned token, scored on the row that verified it; and
score() gives the same records for text it is handed: against its own logits (the bar), against live decoding
(2 x LOGIT_BAR_CACHE of test_generate_gpu.py: a log-probability moves by at most twice the largest logit difference),
leaving the slots reusable.  /answer ranks four candidates of the tiny model by their mean."""
from __future__ import annotations

import math

import pytest
import torch

from cadence_rag_amd.grammar import TokenGrammar, allowed_tokens_host, citation_grammar, next_state_host
from cadence_rag_amd.logprobs import error_bar, logprobs_host, mean_logprob
from cadence_rag_amd.sampling import SamplingParams

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEW = 8
TOP = 5
TEXTS = ["the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
         "gateway and the billing service after the upgrade",
         "ticket ABC-123 tracks the rollback to version v1.2.3 and the follow up call next week, the agent confirmed the "
         "refund and scheduled a call back for tuesday morning"]


@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """The tiny checkpoint (2 random layers, byte-level BPE of 384 ids), its embedding table as the head."""
    from tiny_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    root = tmp_path_factory.mktemp("logprobs_tiny")
    build_checkpoint(root)
    enc = Qwen3Encoder.from_pretrained(str(root), DEV, max_length=2048)
    return Qwen3Generator(enc, enc.embed, enc.tokenizer, max_context=2048, max_seqs=4, model_id="tiny")


@pytest.fixture(scope="module")
def prompts(generator):
    return [generator.tokenizer.encode(t, add_special_tokens=False) for t in TEXTS]


def _grammar(gen):
    return TokenGrammar(citation_grammar(["Q-12", "A-45"]), gen.token_table())


def _modes(gen):
    draw = SamplingParams(temperature=0.9, top_k=40, top_p=0.95, seed=7)
    return {"greedy": {}, "grammar": {"grammar": _grammar(gen)}, "sampling": {"sampling": draw},
            "grammar+sampling": {"grammar": _grammar(gen), "sampling": draw}}


MODES = ["greedy", "grammar", "sampling", "grammar+sampling"]


def _near(got, want, lse, ln_z, what):
    if math.isnan(want) or math.isinf(want):
        assert (math.isnan(got) and math.isnan(want)) or got == want, f"{what}: {got} for {want}"
    else:
        assert abs(got - want) <= error_bar(want, lse, ln_z), f"{what}: {got} for {want}"


def _check_record(rec, row: torch.Tensor, token: int, n_top: int, allowed=None, what=""):
    """One TokenLogprob against the host rule on the logits row the kernel read."""
    want = logprobs_host(row.float().cpu().numpy(), token, allowed, n_top)
    assert rec.token == token and rec.rank == want.rank, f"{what}: token / rank"
    _near(rec.logprob, want.logprob, want.lse_all, want.ln_z_all, f"{what}: logprob")
    assert [i for i, _ in rec.top] == want.top_id.tolist(), f"{what}: top ids"
    for k, (_, lp) in enumerate(rec.top):
        _near(lp, float(want.top_logprob[k]), want.lse_all, want.ln_z_all, f"{what}: top logprob {k}")
    if allowed is None:
        assert rec.allowed_logmass is None
    else:   # the difference of two fp32 outputs, taken on the host: the two bars add up
        bar = error_bar(want.lse_all, want.lse_all, want.ln_z_all) + \
            error_bar(want.lse_allowed, want.lse_allowed, want.ln_z_allowed)
        assert abs(rec.allowed_logmass - want.allowed_logmass) <= bar, f"{what}: allowed_logmass"
        assert rec.allowed_logmass <= bar and allowed[token]


@pytest.mark.parametrize("mode", MODES)
def test_the_ids_do_not_depend_on_logprobs_and_the_records_equal_the_host_rule(gpu, generator, prompts, mode):
    gen, kw = generator, _modes(generator)[mode]
    stop = gen.stop_ids()
    plain = gen.generate(prompts, NEW, stop, **kw)
    assert gen.last_logprobs is None
    got = gen.generate(prompts, NEW, stop, logprobs=TOP, **kw)
    assert got == plain
    records = gen.last_logprobs
    assert [len(r) for r in records] == [len(o) for o in got] and any(got)
    assert [[r.token for r in recs] for recs in records] == got
    # prefill and step by hand, fed with the ids generate produced: pick j of generate read exactly these logits
    g = kw.get("grammar")
    state = [g.dfa.start if g else 0] * len(prompts)
    logits, live = gen.prefill(prompts), list(range(len(prompts)))
    for j in range(NEW):
        for k, b in enumerate(live):
            if len(got[b]) > j:
                allowed = allowed_tokens_host(g.dfa, g.table, state[b]) if g else None
                _check_record(records[b][j], logits[k], got[b][j], TOP, allowed, f"{mode}: prompt {b}, token {j}")
                if g:
                    state[b] = next_state_host(g.dfa, g.table, state[b], got[b][j])
        live = [b for b in live if len(got[b]) > j]
        if not live or j + 1 == NEW:
            break
        _, logits = gen.step([got[b][j] for b in live], slots=live)
    gen.live = []
    assert gen.generate(prompts, NEW, stop, logprobs=0, **kw) == plain and all(r.top == [] for r in gen.last_logprobs[0])


def test_generate_samples_keeps_its_ids(gpu, generator, prompts):
    gen = generator
    draw = SamplingParams(temperature=1.0, top_p=0.9, seed=3)
    plain = gen.generate_samples(prompts[0], 3, NEW, gen.stop_ids(), sampling=draw)
    got = gen.generate_samples(prompts[0], 3, NEW, gen.stop_ids(), sampling=draw, logprobs=2)
    assert got == plain and len(set(map(tuple, got))) > 1
    assert [[r.token for r in recs] for recs in gen.last_logprobs] == got
    for recs in gen.last_logprobs:
        for r in recs:
            assert r.logprob <= 0.0 and r.rank >= 1 and len(r.top) == 2
            assert r.top[0][1] >= r.top[1][1] and r.top[0][1] >= r.logprob and (r.rank > 1 or r.top[0][0] == r.token)
    # the first pick of every sample reads the one row the prefill gave
    first = gen.prefill([prompts[0]])
    for i, recs in enumerate(gen.last_logprobs):
        if recs:
            _check_record(recs[0], first[0], got[i][0], 2, None, f"sample {i}")
    gen.live = []


def test_speculation_scores_every_returned_token_on_the_row_that_verified_it(gpu, generator, prompts, monkeypatch):
    from cadence_rag_amd.encoder import generate as generate_module
    gen, prompt = generator, prompts[1]
    ref = gen.generate([prompt], 12)[0]

    def drafter(ids, max_draft):   # the plain run's next ids, the second one spoiled: accepted and rejected drafts
        at = len(ids) - len(prompt)
        drafts = list(ref[at:at + max_draft])
        if len(drafts) > 1:
            drafts[1] = (drafts[1] + 1) % gen.cfg.vocab_size
        return drafts

    plain = gen.generate([prompt], 12, speculate=3, drafter=drafter)
    seen = []
    real = generate_module.score_rows

    def spy(logits, token, n_top, bits=None):
        out = real(logits, token, n_top, bits)
        seen.append((logits.clone(), out))
        return out

    monkeypatch.setattr(generate_module, "score_rows", spy)
    got = gen.generate([prompt], 12, speculate=3, drafter=drafter, logprobs=TOP)
    stats = gen.last_speculation
    assert got == plain
    assert stats["accepted"][0] >= 1 and stats["drafted"][0] > stats["accepted"][0], stats
    recs = gen.last_logprobs[0]
    assert [r.token for r in recs] == got[0]                       # one per returned token, none for a rejected draft
    assert len(seen) >= len(recs) and all(lg.shape[0] == 1 for lg, _ in seen)
    by_id = {id(out[0]): lg for lg, out in seen}
    for j, r in enumerate(recs):
        _check_record(r, by_id[id(r)][0], got[0][j], TOP, None, f"token {j}")
    assert stats["forwards"] < len(got[0])                         # several tokens came out of one forward


def test_score_against_its_own_logits_in_blocks_of_eight(gpu, generator, prompts):
    gen = generator
    conts = [prompts[1][:6], prompts[0][:7]]                       # 13 rows: a block of 8 and one of 5
    records = gen.score(prompts, conts, top=TOP, keep_logits=True)
    assert [len(r) for r in records] == [6, 7] and [t.shape for t in gen.last_score_logits] == \
        [(6, gen.cfg.vocab_size), (7, gen.cfg.vocab_size)]
    for b, recs in enumerate(records):
        for j, r in enumerate(recs):
            _check_record(r, gen.last_score_logits[b][j], conts[b][j], TOP, None, f"sequence {b}, token {j}")
    # afterwards the slots hold prompt + continuation as after a prefill
    for b in range(2):
        assert gen.resident(b) == list(prompts[b]) + list(conts[b]) and gen.cache.lens[b] == len(prompts[b]) + len(conts[b])
    longer = [list(prompts[b]) + list(conts[b]) + [5, 6, 7] for b in range(2)]
    gen.generate(longer, 2, reuse_prefix=True)
    assert gen.last_reuse["reused"] == [len(p) - 3 for p in longer]   # everything score left, only the new ids computed
    again = gen.score(prompts[:1], conts[:1])                      # one sequence, no top entries, no logits kept
    assert [r.token for r in again[0]] == conts[0] and all(r.top == [] for r in again[0])
    assert gen.last_score_logits is None
    gen.live = []


def test_score_refuses_what_prefill_refuses(gpu, generator, prompts):
    from cadence_rag_amd.encoder.generate import PromptTooLong
    gen = generator
    with pytest.raises(PromptTooLong):
        gen.score([list(range(5)) * 400], [[1] * 60])
    for bad in (dict(prompts=[prompts[0]], continuations=[[]]), dict(prompts=[[]], continuations=[[1]]),
                dict(prompts=prompts, continuations=[[1]]), dict(prompts=[prompts[0]], continuations=[[1]], top=17)):
        with pytest.raises(ValueError):
            gen.score(**bad)
    with pytest.raises(ValueError):
        gen.generate([prompts[0]], 2, logprobs=17)


def test_score_against_live_decoding(gpu, tmp_path_factory):
    """generate's records, read behind steps over the cache, against score's, read behind one prefill of the whole text:
    the logits of the two differ by at most LOGIT_BAR_CACHE (measured in test_generate_gpu.py on these prompts), and
    logprob = l_t - lse moves by at most twice the largest logit difference."""
    from test_generate_gpu import LOGIT_BAR_CACHE, PROMPTS
    from tiny_reranker_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    root = tmp_path_factory.mktemp("logprobs_live")
    _, tok = build_checkpoint(root, tied=False, heads=(8, 2))
    gen = Qwen3Generator.from_pretrained(str(root), DEV, max_context=512, max_seqs=4)
    ids = [tok.encode(p, add_special_tokens=False) for p in PROMPTS]
    out = gen.generate(ids, 16, logprobs=0)
    live = gen.last_logprobs
    scored = gen.score(ids, out)
    worst = 0.0
    for b in range(len(ids)):
        assert [r.token for r in scored[b]] == out[b] == [r.token for r in live[b]]
        for a, s in zip(live[b], scored[b]):
            worst = max(worst, abs(a.logprob - s.logprob))
    print(f"largest |logprob(step) - logprob(score)| = {worst:.3e}, bound {2 * LOGIT_BAR_CACHE:.3e}")
    assert worst <= 2 * LOGIT_BAR_CACHE


def test_answer_ranks_the_candidates_by_their_mean_logprob(gpu, generator, monkeypatch):
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
    monkeypatch.setattr(settings, "answer_max_repairs", 0)
    monkeypatch.setattr(settings, "answer_constrained", True)
    drawn = []
    real = generator.generate_samples

    def spy(*a, **kw):
        drawn.append(real(*a, **kw))
        return drawn[-1]

    monkeypatch.setattr(generator, "generate_samples", spy)
    answer.set_llm(generator)
    try:
        out = answer.answer_question(answer.AnswerRequest(query="what holds?", temperature=0.9, seed=5, samples=4,
                                                          sample_rank="logprob", logprobs=True))
    finally:
        answer.set_llm(None)
    notes = out["notes"]
    scores = notes["samples"]["scores"]
    assert notes["samples"]["drawn"] == 4 and notes["samples"]["ranked"] is True
    assert len(scores) == 4 and all(math.isfinite(s) and s <= 0.0 for s in scores)
    assert scores == [mean_logprob(r) for r in generator.last_logprobs]
    ids = drawn[-1]
    tok = generator.tokenizer
    texts = [tok.decode(x, skip_special_tokens=True).strip() for x in ids]
    evidence = [i["evidence_id"] for i in items]
    insufficient = [t.strip(" .\"'`*") == answer.INSUFFICIENT for t in texts]
    valid = [not n and answer.validate_citations(t, evidence)["valid"] for t, n in zip(texts, insufficient)]
    by_score = sorted(range(4), key=lambda i: -scores[i])          # stable: the lower index among equals
    want = next((i for i in by_score if valid[i]), None)
    assert notes["samples"]["chosen"] == want and notes["samples"]["valid"] == sum(valid)
    judged = want if want is not None else next((i for i in by_score if not insufficient[i]), by_score[0])
    assert notes["logprobs"]["tokens"] == len(ids[judged])
    assert notes["logprobs"]["mean_logprob"] == scores[judged]
    assert "mean_allowed_logmass" in notes["logprobs"] and notes["logprobs"]["min_allowed_logmass"] <= 1e-5
    if want is not None:
        assert out["status"] == "ok" and out["answer"] == texts[want]
    print(f"scores {scores}, valid {valid}, chosen {want}, status {out['status']}")
