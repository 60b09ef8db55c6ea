"""Qwen3Generator on the GPU: decoding with the KV cache against decoding without one and against transformers'
Qwen3ForCausalLM (teacher forcing), greedy tokens against transformers' own continuation, generate() against stepping
by hand, the small_gemm decode path at the 4B widths against the library path, the embedder and the reranker left
alone, and answer_question end to end over the GPU retrieve backend."""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16

PROMPTS = ["ticket ABC-123 tracks the rollback to version v1.2.3", "the customer called about a failed deployment"]
NEW = 48

# Teacher forcing, 48 steps behind each of the two prompts, both tiny checkpoints.  Measured on MI355X, max |dlogit| over
# all steps and the whole vocabulary (logit standard deviation 0.8):
#   step (cache) against prefill of the longer prefix (no cache), same generator: 2.92e-2 (untied), 3.16e-2 (tied)
#   step against Qwen3ForCausalLM in fp32 on the CPU:                             3.71e-2 (untied), 3.88e-2 (tied)
# Both sides of the first line are bf16 forwards that round differently (P in bf16 tiles in the flash kernel, in fp32 in
# the decode kernel; library GEMMs of other heights), so it is as large as the bf16-vs-fp32 error of either.
# Bars: 1.5 x the larger measured value.  2 x LOGIT_BAR_HF = 0.117 is above the 0.1 the issue hoped for: the greedy
# test compares 70 % (untied) and 80 % (tied) of the steps at that margin, still above its 60 % floor.
LOGIT_BAR_CACHE = 4.74e-2
LOGIT_BAR_HF = 5.83e-2
# 2 random layers at the 4B widths, vocabulary 4096: the small_gemm decode path against the library path over 8 steps of
# three sequences, measured 3.37e-2 (logit standard deviation 1.02); bar 1.5 x
LOGIT_BAR_4B = 5.06e-2


@pytest.fixture(scope="module", params=[False, True], ids=["untied", "tied"])
def tiny(request, tmp_path_factory):
    from tiny_reranker_checkpoint import build_checkpoint
    tied = request.param
    root = tmp_path_factory.mktemp("gen_tied" if tied else "gen_untied")
    # untied: 8 q / 2 kv heads (GROUP 4, the 4B model's); tied: 4 / 2 (GROUP 2, the 0.6B model's)
    hf, tok = build_checkpoint(root, tied=tied, heads=(4, 2) if tied else (8, 2))
    return root, hf, tok


@pytest.fixture(scope="module")
def generator(tiny):
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    gen = Qwen3Generator.from_pretrained(str(tiny[0]), DEV, max_context=512, max_seqs=4)
    assert gen.lm_head.shape == (tiny[1].config.vocab_size, tiny[1].config.hidden_size)
    tied = tiny[1].config.tie_word_embeddings
    assert (gen.lm_head.data_ptr() == gen.encoder.embed.data_ptr()) == bool(tied)
    return gen


@pytest.fixture(scope="module")
def hf_greedy(tiny):
    """transformers' own greedy continuation of each prompt (a full fp32 forward per step on the CPU): per prompt the
    prompt ids, the 48 tokens, and the logits [48, vocab] each token was picked from."""
    _, hf, tok = tiny
    out = []
    with torch.no_grad():
        for text in PROMPTS:
            ids = tok.encode(text, add_special_tokens=False)
            seq, toks, logits = list(ids), [], []
            for _ in range(NEW):
                row = hf(torch.tensor([seq])).logits[0, -1]
                toks.append(int(row.argmax()))
                logits.append(row)
                seq.append(toks[-1])
            out.append((ids, toks, torch.stack(logits)))
    return out


def test_cache_against_no_cache_and_transformers(gpu, tiny, generator, hf_greedy):
    """Teacher forcing: after prefill(prompt), step i is fed the i-th given token; its logits against (a) prefill of the
    longer prefix by the same generator (slot 1) and (b) transformers in fp32 (one causal forward over the whole text)."""
    _, hf, _ = tiny
    gen = generator
    worst_cache = worst_hf = 0.0
    for ids, given, first_logits in hf_greedy:
        with torch.no_grad():
            want = hf(torch.tensor([ids + given])).logits[0]          # row p: the logits behind the prefix [: p + 1]
        got0 = gen.prefill([ids], slots=[0]).cpu()[0]
        worst_hf = max(worst_hf, float((got0 - want[len(ids) - 1]).abs().max()))
        assert float((first_logits[0] - want[len(ids) - 1]).abs().max()) < 1e-4
        for i, tok in enumerate(given):
            _, logits = gen.step([tok], slots=[0])
            got = logits.cpu()[0]
            prefix = ids + given[: i + 1]
            assert gen.cache.lens[0] == len(prefix)
            no_cache = gen.prefill([prefix], slots=[1]).cpu()[0]
            worst_cache = max(worst_cache, float((got - no_cache).abs().max()))
            worst_hf = max(worst_hf, float((got - want[len(prefix) - 1]).abs().max()))
    print(f"max |dlogit|: cache vs no cache = {worst_cache:.3e}, vs transformers fp32 = {worst_hf:.3e}")
    assert worst_cache <= LOGIT_BAR_CACHE, worst_cache
    assert worst_hf <= LOGIT_BAR_HF, worst_hf


def test_greedy_tokens_follow_transformers(gpu, generator, hf_greedy):
    """Fed transformers' own continuation, the native greedy token equals transformers' at every step where its top-1
    minus top-2 logit exceeds 2 x LOGIT_BAR_HF; at least 60 % of the steps are such steps."""
    gen = generator
    compared = total = 0
    for ids, toks, logits in hf_greedy:
        top2 = logits.topk(2, dim=-1).values
        margin = (top2[:, 0] - top2[:, 1]).tolist()
        gen.prefill([ids])
        native = [int(gen.last_tokens[0])]
        for t in toks[:-1]:
            token, _ = gen.step([t])
            native.append(int(token[0]))
        for i in range(NEW):
            total += 1
            if margin[i] > 2 * LOGIT_BAR_HF:
                compared += 1
                assert native[i] == toks[i], (i, margin[i], native[i], toks[i])
    share = compared / total
    print(f"compared {compared} of {total} steps ({share:.2f})")
    assert share >= 0.6, share


def test_generate_equals_stepping_by_hand(gpu, tiny, generator):
    gen, tok = generator, tiny[2]
    prompts = [tok.encode(p, add_special_tokens=False) for p in PROMPTS]
    frozen = [list(p) for p in prompts]
    gen.prefill(prompts)                                      # by hand: both sequences side by side, as generate runs them
    prefix_keys = [gen.cache.keys(0, b).clone() for b in range(2)]
    by_hand = [[int(t)] for t in gen.last_tokens.tolist()]
    while len(by_hand[0]) < NEW:
        token, _ = gen.step([s[-1] for s in by_hand])
        for s, t in zip(by_hand, token.tolist()):
            s.append(int(t))
    both = gen.generate(prompts, NEW)
    assert both == by_hand and prompts == frozen
    assert [len(s) for s in both] == [NEW, NEW] and gen.live == []
    for b in range(2):                                        # the prompt's own cache rows are as prefill left them
        assert gen.cache.lens[b] == len(prompts[b]) + NEW - 1
        assert torch.equal(gen.cache.keys(0, b)[: len(prompts[b])], prefix_keys[b])
    assert gen.generate(prompts, 5) == [s[:5] for s in by_hand]            # the token budget
    stop = by_hand[0][7]
    cut = by_hand[0].index(stop)
    got = gen.generate(prompts, NEW, stop_ids=[stop])                        # a stop id ends its own sequence only
    assert got[0] == by_hand[0][:cut] and stop not in got[0] and stop not in got[1]
    if stop not in by_hand[1][: cut + 1]:
        assert got[1][: cut + 1] == by_hand[1][: cut + 1] and len(got[1]) > cut + 1
    from cadence_rag_amd.encoder.generate import PromptTooLong
    with pytest.raises(ValueError, match=r"max_context 512 - max_new_tokens 500") as exc:
        gen.generate(prompts, 500)
    assert isinstance(exc.value, PromptTooLong)
    text = gen.generate_text([{"role": "system", "content": "be brief"}, {"role": "user", "content": PROMPTS[0]}], 8)
    assert isinstance(text, str)
    ids = gen.chat_ids([{"role": "user", "content": "hi"}])
    assert tok.decode(ids) == "<|im_start|>user\nhi<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
    assert tok.get_vocab()["<|im_end|>"] in gen.stop_ids() and tok.eos_token_id in gen.stop_ids()


def test_small_gemm_decode_path_at_4b_widths(gpu):
    """2 random layers at the 4B widths (32 q / 8 kv heads, hidden 2560, ffn 9728), vocabulary 4096: step() takes the
    small_gemm path (16 padded rows); forced onto the library GEMMs the same steps give the same logits within
    LOGIT_BAR_4B."""
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder
    cfg = Qwen3Config(num_layers=2, vocab_size=4096, max_length=512)
    enc = Qwen3Encoder.random_init(cfg, seed=9, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    lm = (torch.randn(4096, cfg.hidden_size, generator=g, device=DEV) * 0.02).to(BF)
    gen = Qwen3Generator(enc, lm, max_context=512, max_seqs=4)
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, 4096, n).tolist() for n in (40, 131, 7)]
    feed = rng.integers(0, 4096, (8, 3)).tolist()
    gen.prefill(prompts)
    k0, v0, lens0 = gen.cache.k.clone(), gen.cache.v.clone(), list(gen.cache.lens)
    runs = {}
    for force in (False, True):
        gen.cache.k.copy_(k0)
        gen.cache.v.copy_(v0)
        gen.cache.lens[:] = lens0
        gen.force_library = force
        rows = []
        for toks in feed:
            _, logits = gen.step(toks, slots=[0, 1, 2])
            rows.append(logits.cpu())
        runs[gen.last_path] = torch.stack(rows)
    assert set(runs) == {"small_gemm", "library"}
    assert 0.5 < float(runs["library"].std()) and bool(torch.isfinite(runs["small_gemm"]).all())
    err = float((runs["small_gemm"] - runs["library"]).abs().max())
    print(f"4B widths: small_gemm vs library max |dlogit| = {err:.3e} (std {float(runs['library'].std()):.2f})")
    assert err <= LOGIT_BAR_4B, err


def test_embedder_and_reranker_unaffected_by_the_generator(gpu, tiny, tmp_path):
    from tiny_checkpoint import build_checkpoint as build_embedder
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker
    build_embedder(tmp_path / "emb")
    enc = Qwen3Encoder.from_pretrained(str(tmp_path / "emb"), DEV)
    rr = Qwen3Reranker.from_pretrained(str(tiny[0]), DEV, max_length=256)
    texts = PROMPTS + ["a short query", "x" * 600]
    emb_before = enc.encode_device(texts)[0].clone()
    rr_before = rr.rerank(PROMPTS[0], texts)[0].copy()
    gen = Qwen3Generator.from_pretrained(str(tiny[0]), DEV, max_context=256, max_seqs=2)
    gen.generate([tiny[2].encode(p, add_special_tokens=False) for p in PROMPTS], 12)
    assert torch.equal(emb_before, enc.encode_device(texts)[0])
    assert np.array_equal(rr_before, rr.rerank(PROMPTS[0], texts)[0])


def test_answer_question_end_to_end(gpu, tiny, monkeypatch):
    """The gate over a real (random, tiny) LLM: the status is one of the three, the LLM is called at most
    answer_max_repairs + 1 times, and no answer that fails validate_citations comes back."""
    from datetime import datetime, timedelta
    from uuid import UUID

    from cadence_rag_amd import answer, embeddings
    from cadence_rag_amd import retrieve as rt
    from cadence_rag_amd.config import settings
    from cadence_rag_amd.encoder.generate import Qwen3Generator
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
    gen = Qwen3Generator.from_pretrained(str(tiny[0]), DEV, max_context=2048, max_seqs=1)
    replies = []

    class Recording:
        model_id = gen.model_id

        def generate_text(self, messages, max_new_tokens):
            replies.append(gen.generate_text(messages, max_new_tokens))
            return replies[-1]

    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 24)
    monkeypatch.setattr(settings, "answer_max_repairs", 2)
    answer.set_llm(Recording())
    try:
        out = answer.answer_question(answer.AnswerRequest(
            query=QUERY, budget=rt.Budget(max_evidence_items=4, max_total_chars=500), echo_evidence=True), be)
    finally:
        answer.set_llm(None)
        chunks.close()
        arts.close()
    pack = out["evidence_pack"]
    ids = [i["evidence_id"] for i in pack["artifacts"] + pack["quotes"]]
    print(f"status {out['status']}, {len(replies)} LLM calls, dropped {out['notes']['dropped_evidence']}, replies {replies!r}")
    assert len(ids) > 1 and out["status"] in ("ok", "insufficient_evidence", "citation_check_failed")
    assert 1 <= len(replies) <= settings.answer_max_repairs + 1 and out["model"] == gen.model_id
    if out["status"] == "ok":
        assert answer.validate_citations(out["answer"], ids)["valid"]
        assert [c["evidence_id"] for c in out["citations"]] == answer.validate_citations(out["answer"], ids)["cited"]
    else:
        assert out["answer"] is None and out["citations"] == []
