"""Speculative decoding end to end on the GPU: Qwen3Generator.step_rows and generate(speculate=k).

(a) The small_gemm path (2 random layers at the 4B widths, vocabulary 4096 -- the model of
test_generate_gpu.test_small_gemm_decode_path_at_4b_widths): every row of a forward depends on that row alone, so
step_rows' logits are step's to the bit and generate(speculate=k) returns the ids of generate() in all four picking modes,
whatever the drafter proposes.
(b) The library path (the tiny checkpoint): GEMMs of other heights round differently, so teacher-forced logits are held
to LOGIT_BAR_CACHE, the bar tests/test_generate_gpu.py measured for forwards of different heights, and generate keeps
its invariants."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
VOCAB = 4096
NEW = 24
LOGIT_BAR_CACHE = 4.74e-2     # tests/test_generate_gpu.py: forwards of different heights over the same tokens


# ---- (a) the small_gemm path ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen4b():
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder
    cfg = Qwen3Config(num_layers=2, vocab_size=VOCAB, max_length=512)
    enc = Qwen3Encoder.random_init(cfg, seed=9, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    lm = (torch.randn(VOCAB, cfg.hidden_size, generator=g, device=DEV) * 0.02).to(BF)
    return Qwen3Generator(enc, lm, max_context=512, max_seqs=4)


@pytest.fixture(scope="module")
def prompts():
    rng = np.random.default_rng(1)
    return [rng.integers(0, VOCAB, n).tolist() for n in (40, 131)]


def _grammar():
    """A synthetic grammar over the 4096 ids, its tables built as tests/test_sample_gpu.py builds them: token id is the
    one byte 'A' + id % 3; three states, state s forbids the byte 'A' + s and every other byte moves the state, so what is
    allowed depends on every token emitted so far.  A fifth of the ids never appear; two are stop tokens."""
    from cadence_rag_amd.grammar import DEAD, KIND_NEVER, KIND_STOP, ByteDfa, TokenGrammar, TokenTable
    rng = np.random.default_rng(3)
    kind = np.where(rng.random(VOCAB) < 0.2, KIND_NEVER, 0).astype(np.uint8)
    kind[[7, 1000]] = KIND_STOP
    table = TokenTable(np.arange(VOCAB + 1, dtype=np.int32), (65 + np.arange(VOCAB) % 3).astype(np.uint8), kind)
    class_of = np.zeros(256, np.uint8)
    class_of[[65, 66, 67]] = [0, 1, 2]
    trans = np.array([[DEAD if c == s else (s + c + 1) % 3 for c in range(3)] for s in range(3)], np.uint16)
    return TokenGrammar(ByteDfa(class_of, trans, np.ones(3, np.uint8)), table)


def _modes():
    from cadence_rag_amd.sampling import SamplingParams
    draw = SamplingParams(0.9, top_k=40, seed=7)
    return {"greedy": {}, "sampled": {"sampling": draw}, "grammar": {"grammar": _grammar()},
            "grammar+sampled": {"grammar": _grammar(), "sampling": draw}}


def drafter_from(runs, how):
    """A drafter that knows the plain runs [(prompt, ids)]: `ids` is a prompt and the first j ids of its run.  right: the
    next ids of the run; wrong: each of them + 1; partly: right for j % (max_draft + 1) ids, then wrong."""
    def draft(ids, max_draft):
        for prompt, out in runs:
            j = len(ids) - len(prompt)
            if list(ids[:len(prompt)]) == list(prompt) and list(ids[len(prompt):]) == list(out[:j]):
                right = list(out[j:j + max_draft])
                wrong = [(t + 1) % VOCAB for t in right]
                keep = {"right": len(right), "wrong": 0, "partly": j % (max_draft + 1)}[how]
                return right[:keep] + wrong[keep:]
        return []
    return draft


def _held(gen, n):
    return list(gen.cache.lens[:n]), [list(gen.resident(b)) for b in range(n)]


def test_step_rows_logits_are_steps_logits_to_the_bit(gpu, gen4b, prompts):
    gen = gen4b
    feed = np.random.default_rng(2).integers(0, VOCAB, (8, 2)).tolist()
    gen.prefill(prompts)
    want, tokens = [], []
    for toks in feed:
        token, logits = gen.step(toks, slots=[0, 1])
        want.append(logits.clone())
        tokens.append(token.clone())
    assert gen.last_path == "small_gemm"
    want, tokens = torch.stack(want), torch.stack(tokens)         # [step, sequence, vocab]
    held = _held(gen, 2)
    gen.prefill(prompts)
    token, logits = gen.step_rows([[f[0] for f in feed[:4]], [f[1] for f in feed[:4]]], slots=[0, 1])
    assert gen.last_path == "small_gemm" and logits.shape == (8, VOCAB)
    assert torch.equal(logits[:4], want[:4, 0]) and torch.equal(logits[4:], want[:4, 1])
    assert torch.equal(token[:4], tokens[:4, 0]) and torch.equal(token[4:], tokens[:4, 1])
    # the next rows behind them: 1 + 3, then a plain step -- the cache rows step_rows appended are step's
    token, logits = gen.step_rows([[feed[4][0]], [f[1] for f in feed[4:7]]], slots=[0, 1])
    assert torch.equal(logits[0], want[4, 0]) and torch.equal(logits[1:], want[4:7, 1])
    gen.step_rows([[f[0] for f in feed[5:8]]], slots=[0])
    token, logits = gen.step([feed[7][1]], slots=[1])
    assert torch.equal(logits[0], want[7, 1])
    assert _held(gen, 2) == held
    # eight rows of one sequence
    gen.prefill(prompts)
    token, logits = gen.step_rows([[f[1] for f in feed]], slots=[1])
    assert torch.equal(logits, want[:, 1]) and torch.equal(token, tokens[:, 1])
    with pytest.raises(ValueError, match="at most 8"):
        gen.step_rows([[1] * 5, [2] * 4], slots=[0, 1])
    with pytest.raises(ValueError, match="at least one"):
        gen.step_rows([[1], []], slots=[0, 1])
    gen.live = []


@pytest.mark.parametrize("mode", ["greedy", "sampled", "grammar", "grammar+sampled"])
def test_speculation_returns_the_plain_ids(gpu, gen4b, prompts, mode):
    """k in {1, 3, 7} x three drafters made from the plain run, over both prompts in one call (at most 3 drafts each)
    and over the longer one alone (up to 7)."""
    gen, kw = gen4b, _modes()[mode]
    for batch in (prompts, prompts[1:]):
        n = len(batch)
        want = gen.generate(batch, NEW, **kw)
        assert gen.last_path == "small_gemm" and gen.last_speculation is None
        held, ended = _held(gen, n), gen.last_grammar
        assert "grammar" in kw or [len(o) for o in want] == [NEW] * n
        runs = list(zip(batch, want))
        for k in (1, 3, 7):
            cap = min(k, 8 // n - 1)
            for how in ("right", "wrong", "partly"):
                got = gen.generate(batch, NEW, speculate=k, drafter=drafter_from(runs, how), **kw)
                spec = gen.last_speculation
                assert got == want, (mode, n, k, how, spec)
                assert _held(gen, n) == held and gen.last_grammar == ended and gen.live == []
                assert all(0 <= a <= d for a, d in zip(spec["accepted"], spec["drafted"]))
                assert sum(spec["drafted"]) > 0 or max(len(o) for o in want) <= 1      # (a stop token at once)
                if how == "right":
                    assert spec["accepted"] == spec["drafted"]
                if how == "wrong":
                    assert spec["accepted"] == [0] * n
                if "grammar" not in kw:      # nobody stops early: every sequence makes NEW picks, the first on the prefill
                    if how == "right":       # a forward yields cap + 1 tokens
                        assert spec["forwards"] == math.ceil((NEW - 1) / (cap + 1))
                        assert spec["drafted"] == [NEW - 1 - spec["forwards"]] * n
                    if how == "wrong":       # one forward per token
                        assert spec["forwards"] == NEW - 1


def test_samples_stops_and_budgets(gpu, gen4b, prompts):
    from cadence_rag_amd.sampling import SamplingParams
    gen, draw = gen4b, SamplingParams(0.9, top_k=40, seed=7)
    # two samples of one prompt, forked: the children read the prompt's rows in slot 0
    want = gen.generate_samples(prompts[1], 2, NEW, sampling=draw, streams=[4, 9])
    held = _held(gen, 2)
    assert want[0] != want[1]
    for how in ("right", "partly"):
        drafter = drafter_from([(prompts[1], want[0]), (prompts[1], want[1])], how)
        got = gen.generate_samples(prompts[1], 2, NEW, sampling=draw, streams=[4, 9], speculate=3, drafter=drafter)
        assert got == want and _held(gen, 2) == held
        assert gen.cache.lens[1] == 0 and not gen.cache.forked(1) and sum(gen.last_speculation["accepted"]) > 0
    # two prompts that stop at different times, the stop id inside a run of right drafts
    plain = gen.generate(prompts, NEW)
    stop = plain[0][5]
    want = gen.generate(prompts, NEW, [stop])
    held = _held(gen, 2)
    assert len(want[0]) <= 5 and len(want[0]) != len(want[1])
    for how in ("right", "wrong", "partly"):
        got = gen.generate(prompts, NEW, [stop], speculate=3, drafter=drafter_from(list(zip(prompts, plain)), how))
        assert got == want and _held(gen, 2) == held, how
    # a budget that ends inside an accepted run: the drafter knows 24 ids, 6 are allowed
    want = gen.generate(prompts[:1], 6)
    held = _held(gen, 1)
    assert want[0] == plain[0][:6]
    got = gen.generate(prompts[:1], 6, speculate=7, drafter=drafter_from([(prompts[0], plain[0])], "right"))
    assert got == want and _held(gen, 1) == held
    assert gen.last_speculation == {"forwards": 1, "drafted": [4], "accepted": [4]}
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="speculate"):
            gen.generate(prompts[:1], 6, speculate=bad)


def test_prompt_lookup_on_a_repeated_cycle(gpu, gen4b):
    """The default drafter (propose_drafts) on a prompt that repeats five ids: it always finds a draft; the ids are the
    plain run's whether the model goes on with the cycle or not."""
    gen = gen4b
    prompt = [11, 222, 3333, 44, 555] * 8
    want = gen.generate([prompt], NEW)
    held = _held(gen, 1)
    for k in (3, 7):
        assert gen.generate([prompt], NEW, speculate=k) == want and _held(gen, 1) == held
        spec = gen.last_speculation
        print(f"cycle prompt, speculate={k}: {spec}")
        assert spec["drafted"][0] > 0 and spec["forwards"] <= NEW - 1


# ---- (b) the library path ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_gen(tmp_path_factory):
    from tiny_reranker_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    root = tmp_path_factory.mktemp("speculate_tiny")
    build_checkpoint(root, tied=False, heads=(8, 2))
    return Qwen3Generator.from_pretrained(str(root), DEV, max_context=512, max_seqs=4)


TEXTS = ["the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
         "gateway and the billing service after the upgrade", "what did the agent promise about the refund?"]


def test_library_path_logits_stay_within_the_bar(gpu, tiny_gen):
    gen = tiny_gen
    ids = [gen.tokenizer.encode(t, add_special_tokens=False) for t in TEXTS]
    vocab = gen.cfg.vocab_size
    feed = np.random.default_rng(4).integers(0, vocab, (8, 2)).tolist()
    gen.prefill(ids)
    want = torch.stack([gen.step(toks, slots=[0, 1])[1].clone() for toks in feed])
    assert gen.last_path == "library"
    worst = 0.0
    for rows in ([[f[0] for f in feed[:4]], [f[1] for f in feed[:4]]], [[f[0] for f in feed]], [[feed[0][0]], [feed[0][1]]]):
        gen.prefill(ids)
        _, logits = gen.step_rows(rows, slots=list(range(len(rows))))
        assert gen.last_path == "library"
        ref = torch.cat([want[:len(r), b] for b, r in enumerate(rows)])
        worst = max(worst, float((logits - ref).abs().max()))
    print(f"library path: step_rows vs successive steps max |dlogit| = {worst:.3e} (std {float(want.std()):.2f})")
    assert worst <= LOGIT_BAR_CACHE, worst
    gen.live = []


def test_library_path_generate_keeps_its_invariants(gpu, tiny_gen):
    """Greedy, speculate=3, a drafter that is right about half the time (it knows the plain run): every emitted token is
    the greedy pick of this run's own logits at the row behind the tokens emitted before it; the slot holds what was
    emitted; the counts add up."""
    gen = tiny_gen
    prompt = gen.tokenizer.encode(TEXTS[0], add_special_tokens=False)
    plain = gen.generate([prompt], NEW)[0]
    record = []
    real_rows, real_step, real_prefill = gen.step_rows, gen.step, gen.prefill

    def step_rows(token_rows, *a, **k):
        token, logits = real_rows(token_rows, *a, **k)
        record.append((list(token_rows[0]), token.tolist(), logits.argmax(dim=1).tolist()))
        return token, logits

    def step(tokens, *a, **k):
        token, logits = real_step(tokens, *a, **k)
        record.append(([tokens[0]], token.tolist(), logits.argmax(dim=1).tolist()))
        return token, logits

    def prefill(*a, **k):
        logits = real_prefill(*a, **k)
        record.append(([], gen.last_tokens.tolist(), logits.argmax(dim=1).tolist()))
        return logits

    gen.step_rows, gen.step, gen.prefill = step_rows, step, prefill
    try:
        out = gen.generate([prompt], NEW, speculate=3, drafter=drafter_from([(prompt, plain)], "partly"))[0]
    finally:
        del gen.step_rows, gen.step, gen.prefill
    spec = gen.last_speculation
    print(f"library path, speculate=3: {spec}; {sum(a == b for a, b in zip(out, plain))} of {NEW} ids are the plain run's")
    emitted, accepted, drafted = [], 0, 0
    for fed, token, top in record:
        assert token == top                                       # the pick is the maximum of the row's own logits
        assert fed[:1] == emitted[-1:]                            # the pending token is the last one emitted
        drafted += max(len(fed) - 1, 0)
        for i, t in enumerate(token):
            emitted.append(t)
            if len(emitted) == NEW or i + 1 >= len(fed) or fed[i + 1] != t:
                break
            accepted += 1
    assert out == emitted and len(out) == NEW
    assert spec == {"forwards": len(record) - 1, "drafted": [drafted], "accepted": [accepted]}
    assert gen.cache.lens[0] == len(prompt) + NEW - 1 and gen.resident(0) == (list(prompt) + out)[:-1]
    assert gen.live == []
