"""Continuing cached sequences in Qwen3Generator on the GPU: extend() against prefill() of the whole text and against
transformers' Qwen3ForCausalLM, generate(reuse_prefix=True) over a resident prefix (what it reuses, what it leaves
alone in the cache, what it computes), and answer_question's repair round over a generator with a prefix cache."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# The bars tests/test_generate_gpu.py measured on these same tiny checkpoints for two bf16 forwards that round
# differently (a step over the cache against a prefill of the longer prefix: 2.92e-2 untied, 3.16e-2 tied; a step against
# Qwen3ForCausalLM in fp32 on the CPU: 3.71e-2 / 3.88e-2; each bar 1.5 x the larger value).  extend() against prefill()
# is such a pair too: other query blocks and key tiles in the attention, library GEMMs of other heights.
LOGIT_BAR_CACHE = 4.74e-2
LOGIT_BAR_HF = 5.83e-2


@pytest.fixture(scope="module", params=[False, True], ids=["untied", "tied"])
def tiny(request, tmp_path_factory):
    from tiny_reranker_checkpoint import build_checkpoint
    tied = request.param
    root = tmp_path_factory.mktemp("reuse_tied" if tied else "reuse_untied")
    # untied: 8 q / 2 kv heads (GROUP 4, the 4B model's); tied: 4 / 2 (GROUP 2, the 0.6B model's)
    hf, tok = build_checkpoint(root, tied=tied, heads=(4, 2) if tied else (8, 2))
    return root, hf, tok


def _fresh(tiny, **kw):
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    kw.setdefault("max_seqs", 3)
    return Qwen3Generator.from_pretrained(str(tiny[0]), DEV, max_context=512, **kw)


def _ids(rng, tiny, n):
    return rng.integers(0, tiny[1].config.vocab_size, n).tolist()


def _rows(gen, slot, n):
    """The first n cache rows of a slot in the first and the last layer, keys and values."""
    last = gen.cfg.num_layers - 1
    return [t[layer, slot, :, :n].clone() for t in (gen.cache.k, gen.cache.v) for layer in (0, last)]


def test_extend_against_prefill_and_transformers(gpu, tiny):
    """prefill(A) then extend(B) in slot 0, and extend(A + B) from the empty slot 2: the logits behind A + B against (a)
    prefill(A + B) in slot 1 and (b) Qwen3ForCausalLM in fp32 on the CPU.  A 45 tokens, B 57: the cached rows end inside a
    key tile and the new rows fill one query block and part of a second."""
    from cadence_rag_amd.encoder.generate import PromptTooLong
    gen, hf = _fresh(tiny), tiny[1]
    rng = np.random.default_rng(3)
    a, b = _ids(rng, tiny, 45), _ids(rng, tiny, 57)
    with torch.no_grad():
        want_hf = hf(torch.tensor([a + b])).logits[0, -1]
    gen.prefill([a], slots=[0])
    before = _rows(gen, 0, len(a))
    got = gen.extend([b], slots=[0]).cpu()[0]
    assert gen.cache.lens[0] == len(a) + len(b) and gen.resident(0) == a + b and gen.live == [0]
    assert all(torch.equal(x, y) for x, y in zip(before, _rows(gen, 0, len(a))))      # A's rows are read, not written
    no_cache = gen.prefill([a + b], slots=[1]).cpu()[0]
    empty = gen.extend([a + b], slots=[2]).cpu()[0]
    assert gen.cache.lens[2] == len(a) + len(b) and gen.resident(2) == a + b
    worst = {"extend vs prefill": float((got - no_cache).abs().max()), "extend vs hf": float((got - want_hf).abs().max()),
             "empty-slot extend vs prefill": float((empty - no_cache).abs().max()),
             "empty-slot extend vs hf": float((empty - want_hf).abs().max())}
    print("max |dlogit|: " + ", ".join(f"{k} = {v:.3e}" for k, v in worst.items()))
    assert worst["extend vs prefill"] <= LOGIT_BAR_CACHE and worst["empty-slot extend vs prefill"] <= LOGIT_BAR_CACHE, worst
    assert worst["extend vs hf"] <= LOGIT_BAR_HF and worst["empty-slot extend vs hf"] <= LOGIT_BAR_HF, worst
    # two sequences in one call, one of them behind a truncated slot: what each gave alone (the library GEMMs run at
    # another height, so within the bar rather than bit for bit)
    gen.truncate(0, len(a))
    assert gen.cache.lens[0] == len(a) and gen.resident(0) == a
    gen.truncate(2, 0)
    both = gen.extend([a + b, b], slots=[2, 0]).cpu()
    assert gen.live == [2, 0] and gen.cache.lens[0] == gen.cache.lens[2] == len(a) + len(b)
    d_both = max(float((both[0] - empty).abs().max()), float((both[1] - got).abs().max()))
    print(f"max |dlogit| two sequences in one call vs each alone = {d_both:.3e}")
    assert d_both <= LOGIT_BAR_CACHE, d_both
    with pytest.raises(PromptTooLong):
        gen.extend([_ids(rng, tiny, 512 - len(a) - len(b))], slots=[0])
    with pytest.raises(ValueError):
        gen.extend([[]], slots=[1])
    with pytest.raises(ValueError):
        gen.truncate(1, len(a) + len(b) + 1)


def test_reuse_in_generate(gpu, tiny):
    g1, g2 = _fresh(tiny, max_seqs=2), _fresh(tiny, max_seqs=2)
    rng = np.random.default_rng(8)
    p = _ids(rng, tiny, 60)
    # nothing is resident: the same prefill, token for token
    out = g1.generate([p], 16, reuse_prefix=True)
    assert out == g2.generate([p], 16) and len(out[0]) == 16
    assert g1.last_reuse == {"reused": [0], "computed": [60]} and g2.last_reuse is None
    assert g1.resident(0) == p + out[0][:-1]                       # the last token was never fed

    seen = []
    inner = g1.extend
    g1.extend = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]     # keeps the logits generate() does not return

    # the chat goes on: everything the slot holds is the head of the new prompt
    p2 = p + out[0] + _ids(rng, tiny, 20)
    held = len(p) + len(out[0]) - 1
    before = _rows(g1, 0, held)
    out2 = g1.generate([p2], 16, reuse_prefix=True)
    assert g1.last_reuse == {"reused": [held], "computed": [len(p2) - held]} and len(seen) == 1
    assert all(torch.equal(x, y) for x, y in zip(before, _rows(g1, 0, held)))
    scratch = g2.prefill([p2]).cpu()[0]
    d_chat = float((seen[0].cpu()[0] - scratch).abs().max())
    assert g1.resident(0) == p2 + out2[0][:-1] and g1.cache.lens[0] == len(p2) + 15

    # fewer than 32 shared tokens: nothing is reused, the plain path bit for bit
    p3 = p2[:20] + _ids(rng, tiny, 50)
    out3 = g1.generate([p3], 16, reuse_prefix=True)
    assert g1.last_reuse == {"reused": [0], "computed": [70]} and len(seen) == 1
    assert out3 == g2.generate([p3], 16)
    assert all(torch.equal(x, y) for x, y in zip(_rows(g1, 0, len(p3) + 15), _rows(g2, 0, len(p3) + 15)))

    # a divergence in the middle: the first 50 tokens stay, the slot then holds the new prompt only
    p4 = p3[:50] + _ids(rng, tiny, 30)
    before = _rows(g1, 0, 50)
    out4 = g1.generate([p4], 16, reuse_prefix=True)
    assert g1.last_reuse == {"reused": [50], "computed": [30]} and len(seen) == 2
    assert all(torch.equal(x, y) for x, y in zip(before, _rows(g1, 0, 50)))
    assert g1.resident(0) == p4 + out4[0][:-1] and g1.cache.lens[0] == len(p4) + 15
    scratch = g2.prefill([p4]).cpu()[0]
    d_mid = float((seen[1].cpu()[0] - scratch).abs().max())
    g1.truncate(0, len(p4))                                         # ... and continuing from it: one more token on both
    _, l1 = g1.step([p[0]], slots=[0])
    _, l2 = g2.step([p[0]], slots=[0])
    d_step = float((l1 - l2).abs().max())
    print(f"max |dlogit| reuse vs from scratch: chat {d_chat:.3e}, divergence {d_mid:.3e}, the step behind it {d_step:.3e}")
    assert max(d_chat, d_mid, d_step) <= LOGIT_BAR_CACHE, (d_chat, d_mid, d_step)


def test_answer_repair_round_reuses_the_prompt(gpu, tiny, monkeypatch):
    """answer_question over the GPU retrieve backend and a generator with prefix_cache=True whose first reply is
    replaced by an uncited sentence: the repair round finds the system rules and the evidence pack in the cache."""
    from datetime import datetime, timedelta
    from uuid import UUID

    from cadence_rag_amd import answer, embeddings
    from cadence_rag_amd import retrieve as rt
    from cadence_rag_amd.config import settings
    from test_rerank_gpu import DOCS, QUERY
    rng = np.random.default_rng(5)
    calls = [{"call_id": UUID(int=i + 1), "external_id": f"ext-{i}", "external_source": "zoom"} for i in range(4)]
    t0 = datetime(2026, 3, 1)

    def make(name, id_field, n, extra):
        vecs = rng.standard_normal((n, 1024)).astype(np.float32)
        vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
        cols = {id_field: [100 + i for i in range(n)], "call_id": [calls[i % 4]["call_id"] for i in range(n)]}
        cols.update(extra(n))
        table = rt.DenseTable(name, id_field, dim=1024, capacity=n)
        table.add(vecs, cols, call_started_at=[t0 + timedelta(days=i % 4) for i in range(n)])
        return table, vecs

    chunks, cvec = make("chunks", "chunk_id", 40, lambda n: {
        "speaker": ["S"] * n, "start_ts_ms": list(range(n)), "end_ts_ms": list(range(1, n + 1)),
        "text": [DOCS[i % 7] + f" #{i}" for i in range(n)]})
    arts, avec = make("artifact_chunks", "artifact_chunk_id", 8, lambda n: {
        "artifact_id": list(range(n)), "kind": ["summary"] * n, "content": [DOCS[(3 * i) % 7] for i in range(n)]})
    qvec = (cvec[3] + avec[2]).tolist()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec for _ in texts], model="m"))
    be = rt.GpuRetrieveBackend(chunks, arts, calls=calls)
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    gen = Qwen3Generator.from_pretrained(str(tiny[0]), DEV, max_context=2048, max_seqs=1, prefix_cache=True)
    assert gen.prefix_cache is True
    replies, reuse = [], []

    class FirstReplyUncited:
        model_id = gen.model_id

        @property
        def last_reuse(self):
            return gen.last_reuse

        def generate_text(self, messages, max_new_tokens):
            replies.append(gen.generate_text(messages, max_new_tokens))
            reuse.append(dict(gen.last_reuse))
            return "The rollback was agreed on the call." if len(replies) == 1 else replies[-1]

    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 24)
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    answer.set_llm(FirstReplyUncited())
    try:
        out = answer.answer_question(answer.AnswerRequest(
            query=QUERY, budget=rt.Budget(max_evidence_items=4, max_total_chars=500), echo_evidence=True), be)
    finally:
        answer.set_llm(None)
        chunks.close()
        arts.close()
    pack = out["evidence_pack"]
    ids = [i["evidence_id"] for i in pack["artifacts"] + pack["quotes"]]
    print(f"status {out['status']}, {len(replies)} LLM calls, reuse per call {reuse}, notes {out['notes']['prefix_reused_tokens']}")
    assert 2 <= len(replies) <= settings.answer_max_repairs + 1 and out["repairs"] >= 1
    assert reuse[0]["reused"] == [0] and reuse[1]["reused"][0] >= 32
    assert out["notes"]["prefix_reused_tokens"] == sum(r["reused"][0] for r in reuse) > 0
    assert out["status"] in ("ok", "insufficient_evidence", "citation_check_failed")
    if out["status"] == "ok":
        assert answer.validate_citations(out["answer"], ids)["valid"]
    else:
        assert out["answer"] is None and out["citations"] == []
