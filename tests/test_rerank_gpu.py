"""The reranker on the GPU: crag_enc_attention_prefixed and crag_enc_rerank_head against torch fp32, Qwen3Reranker
end to end against transformers' Qwen3ForCausalLM with the model card's recipe, shared against unshared forwards,
the embedder left alone, and the rerank stage of retrieve_evidence over the GPU backend."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16

QUERY = "why did the api gateway fail after the upgrade?"
DOCS = ["the customer called about a failed deployment of the api gateway",
        "we saw ECONNRESET errors between the gateway and the billing service after the upgrade",
        "  ticket ABC-123 tracks the rollback to version v1.2.3",
        "the agent confirmed the refund and scheduled a call back for tuesday morning",
        ", latency went from forty milliseconds to nine hundred during the incident window",
        "yes",
        "no",
        " ".join(["please send the transcript and the action items to the account team"] * 40)]


def _bf(t):
    return t.to(BF).to(DEV).contiguous()


def _attn_ref(qkv, lens, parent, hq, hkv):
    """fp32: segment b's queries see every key of segment parent[b], then their own keys causally."""
    f = qkv.float().cpu()
    d = 128
    q = f[:, : hq * d].view(-1, hq, d)
    k = f[:, hq * d: (hq + hkv) * d].view(-1, hkv, d)
    v = f[:, (hq + hkv) * d:].view(-1, hkv, d)
    cu = np.concatenate([[0], np.cumsum(lens)])
    out = torch.zeros(int(cu[-1]), hq, d)
    g = hq // hkv
    for b, n in enumerate(lens):
        s = slice(cu[b], cu[b + 1])
        kk, vv = k[s], v[s]
        mask = torch.ones(n, n).tril().bool()
        if parent[b] >= 0:
            ps = slice(cu[parent[b]], cu[parent[b] + 1])
            kk, vv = torch.cat([k[ps], kk]), torch.cat([v[ps], vv])
            mask = torch.cat([torch.ones(n, lens[parent[b]]).bool(), mask], dim=1)
        for h in range(hq):
            sc = (q[s, h] @ kk[:, h // g].T) / math.sqrt(d)
            sc = sc.masked_fill(~mask, float("-inf"))
            out[s, h] = torch.softmax(sc, dim=-1) @ vv[:, h // g]
    return out


def _run_prefixed(lens, parent, hq, hkv, seed):
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.qwen3 import PackedBatch
    g = torch.Generator().manual_seed(seed)
    t = sum(lens)
    qkv = torch.randn(t + 32, (hq + 2 * hkv) * 128, generator=g)
    qkv[t:] = float("nan")
    qkv = _bf(qkv)
    batch = PackedBatch.build_prefixed(lens, parent, DEV)
    vt = torch.empty(hkv, 128, batch.t_pad, dtype=BF, device=DEV)
    ops.v_transpose(qkv, vt, batch.tok_of_pad, hq, hkv)
    out = torch.full((t, hq * 128), float("nan"), dtype=BF, device=DEV)
    ops.attention_prefixed(qkv, vt, out, batch.cu, batch.cu_pad, batch.blk_seq, batch.blk_q0, batch.parent, hq, hkv,
                           1 / math.sqrt(128))
    torch.cuda.synchronize()
    got = out.float().cpu().view(t, hq, 128)
    return got, _attn_ref(qkv[:t], lens, parent, hq, hkv)


@pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])
@pytest.mark.parametrize("plen", [1, 31, 32, 33, 95])
def test_attention_prefixed_matches_fp32(gpu, heads, plen):
    """A prefix root, children of 1 / 17 / 300 / 1000 tokens, and a root without children in one batch (the tolerance
    of test_attention_property_random_lengths_and_groups)."""
    hq, hkv = heads
    lens = [45, plen, 1, 17, 300, 1000, 33]
    parent = [-1, -1, 1, 1, 1, 1, -1]
    got, ref = _run_prefixed(lens, parent, hq, hkv, seed=plen * 7 + hq)
    assert torch.isfinite(got).all()
    assert torch.allclose(got, ref, atol=2e-2, rtol=2e-2), (heads, plen, (got - ref).abs().max())


@pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])
def test_attention_prefixed_roots_equal_the_plain_kernel(gpu, heads):
    """All roots: the prefixed kernel computes what crag_enc_attention computes."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.qwen3 import PackedBatch
    hq, hkv = heads
    lens = [1, 31, 64, 97, 200]
    got, ref = _run_prefixed(lens, [-1] * len(lens), hq, hkv, seed=11)
    assert torch.allclose(got, ref, atol=2e-2, rtol=2e-2), (got - ref).abs().max()
    g = torch.Generator().manual_seed(11)
    t = sum(lens)
    qkv = torch.randn(t + 32, (hq + 2 * hkv) * 128, generator=g)
    qkv[t:] = float("nan")
    qkv = _bf(qkv)
    batch = PackedBatch.build(lens, DEV)
    vt = torch.empty(hkv, 128, batch.t_pad, dtype=BF, device=DEV)
    ops.v_transpose(qkv, vt, batch.tok_of_pad, hq, hkv)
    plain = torch.empty(t, hq * 128, dtype=BF, device=DEV)
    ops.attention(qkv, vt, plain, batch.cu, batch.cu_pad, batch.blk_seq, batch.blk_q0, hq, hkv, 1 / math.sqrt(128))
    assert torch.allclose(plain.float().cpu().view(t, hq, 128), got, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("tied", [False, True], ids=["untied", "tied"])
def test_rerank_head_matches_torch(gpu, tied):
    from cadence_rag_amd.encoder import ops
    g = torch.Generator().manual_seed(3 + tied)
    hidden, rows_total, eps = 2560, 50, 1e-6
    hs = _bf(torch.randn(rows_total, hidden, generator=g))
    delta = _bf(torch.randn(rows_total, hidden, generator=g) * 0.5)
    w = _bf(1 + 0.1 * torch.randn(hidden, generator=g))
    table = torch.randn(300, hidden, generator=g) * 0.05
    # tied: the rows come out of the embedding table; untied: a separate lm_head
    lm = _bf(table[[17, 230]] if tied else torch.randn(2, hidden, generator=g) * 0.05)
    rows = torch.tensor([49, 0, 7, 7, 23], dtype=torch.int64, device=DEV)
    out = torch.empty(5, 3, dtype=torch.float32, device=DEV)
    ops.rerank_head(hs, w, rows, lm, out, eps, delta=delta)
    x = (hs.float() + delta.float()).to(BF).float()[rows]
    normed = (w.float() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)).to(BF).float()).to(BF).float()
    logits = normed @ lm.float().T
    score = torch.log_softmax(logits[:, [1, 0]], dim=-1)[:, 1].exp()
    got = out.cpu()
    assert torch.allclose(got[:, 0], logits[:, 0].cpu(), atol=2e-4, rtol=1e-4)
    assert torch.allclose(got[:, 1], logits[:, 1].cpu(), atol=2e-4, rtol=1e-4)
    assert torch.allclose(got[:, 2], score.cpu(), atol=1e-5)


# ---- end to end on tiny checkpoints ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["untied", "tied"])
def tiny(request, tmp_path_factory):
    from tiny_reranker_checkpoint import build_checkpoint
    tied = request.param
    root = tmp_path_factory.mktemp("rr_tied" if tied else "rr_untied")
    # untied: 8 q / 2 kv heads (GROUP 4, the 4B model's); tied: 4 / 2 (GROUP 2, the 0.6B model's)
    hf, tok = build_checkpoint(root, tied=tied, heads=(4, 2) if tied else (8, 2))
    return root, hf, tok


def _hf_scores(hf, tok, token_lists):
    yes, no = tok.get_vocab()["yes"], tok.get_vocab()["no"]
    out = []
    with torch.no_grad():
        for ids in token_lists:
            logits = hf(torch.tensor([ids])).logits[0, -1]
            pair = torch.stack([logits[no], logits[yes]])
            out.append(float(torch.log_softmax(pair, dim=0)[1].exp()))
    return np.asarray(out)


# measured on MI355X: max |dscore| 3.1e-3 (untied) and 4.8e-3 (tied) over the 8 pairs; the bar is 1.5x the larger
SCORE_BAR = 7.3e-3
# shared against unshared: the same ids and keys, but a child's keys are walked in tiles aligned to the prefix segment's
# end rather than to the pair's start, so the online softmax rounds P to bf16 at other running maxima.  Measured on
# MI355X: 3.3e-3 (tiny, tied; the model's own bf16-vs-fp32 error above is 4.8e-3) and 7.5e-3 at 2 layers of the 4B
# widths with random weights (near-uniform attention over random V: the output is a mean of cancelling vectors, so
# its relative rounding noise is that of P itself).  Bars: 1.5x measured.  A call split over several forwards keeps the
# layout of every pair and stays within 2e-3.
SHARED_BAR_TINY = 5e-3
SHARED_BAR_4B = 1.2e-2
SPLIT_BAR = 2e-3


def test_end_to_end_matches_transformers(gpu, tiny):
    """Qwen3Reranker.from_pretrained on the tiny checkpoint against Qwen3ForCausalLM in fp32 with the model card's
    recipe.  |dscore| < SCORE_BAR (measured, x1.5: see above); the order is the reference's wherever its neighbouring
    scores differ by more than the bar."""
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker, canonical_ids
    root, hf, tok = tiny
    rr = Qwen3Reranker.from_pretrained(str(root), DEV, max_length=256)
    ids = canonical_ids(tok, QUERY, DOCS, rr.instruction, 256)
    assert rr.token_lists(QUERY, DOCS) == ids and max(len(i) for i in ids) == 256
    want = _hf_scores(hf, tok, ids)
    scores, order, model = rr.rerank(QUERY, DOCS)
    assert scores.dtype == np.float32 and scores.shape == (len(DOCS),)
    err = float(np.max(np.abs(scores - want)))
    print(f"max |dscore| = {err:.3e}")
    assert err < SCORE_BAR, err
    want_order = sorted(range(len(DOCS)), key=lambda i: (-want[i], i))
    assert order == sorted(range(len(DOCS)), key=lambda i: (-float(scores[i]), i))
    for a, b in zip(want_order, want_order[1:]):
        if want[a] - want[b] > SCORE_BAR:
            assert order.index(a) < order.index(b), (a, b, want[a], want[b])
    assert rr.head.shape == (2, hf.config.hidden_size)
    assert rr.encoder.__dict__.get("_skinny") is None and rr.encoder.__dict__.get("_wide") is None


def test_shared_equals_unshared_and_split_equals_whole(gpu, tiny):
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker
    root, _, _ = tiny
    rr = Qwen3Reranker.from_pretrained(str(root), DEV, max_length=256)
    lists = rr.token_lists(QUERY, DOCS)
    shared = rr.score_token_lists(lists, share_prefix=True)
    st = dict(rr.last_stats)
    assert st["prefix_tokens"] > 50 and st["forwards"] == 1
    assert st["executed_tokens"] == st["real_tokens"] - (len(DOCS) - 1) * st["prefix_tokens"]
    unshared = rr.score_token_lists(lists, share_prefix=False)
    assert rr.last_stats["executed_tokens"] == rr.last_stats["real_tokens"]
    err = float(np.max(np.abs(shared[:, 2] - unshared[:, 2])))
    print(f"shared vs unshared max |dscore| = {err:.3e}")
    assert err <= SHARED_BAR_TINY
    rr.token_budget = 400
    split = rr.score_token_lists(lists, share_prefix=True)
    assert rr.last_stats["forwards"] > 1
    assert np.max(np.abs(split[:, 2] - shared[:, 2])) <= SPLIT_BAR
    one = rr.score_token_lists(lists[:1], share_prefix=True)      # one pair: a prefix segment and a 1-token child
    assert abs(float(one[0, 2]) - float(unshared[0, 2])) <= SHARED_BAR_TINY


def test_shared_equals_unshared_at_4b_width(gpu):
    """2 layers of the 4B model's widths (32 q / 8 kv heads, hidden 2560, ffn 9728), random weights: 16 pairs of an
    80-token shared head and 350 document tokens (bar: see SHARED_BAR_4B)."""
    from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker
    cfg = Qwen3Config(num_layers=2, vocab_size=4096, max_length=1024)
    enc = Qwen3Encoder.random_init(cfg, seed=9, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    lm = (torch.randn(2, cfg.hidden_size, generator=g, device=DEV) * 0.02).to(BF)
    rr = Qwen3Reranker(enc, lm)
    rng = np.random.default_rng(1)
    head = rng.integers(0, 4096, 80).tolist()
    lists = [head + rng.integers(0, 4096, 350).tolist() for _ in range(16)]
    shared = rr.score_token_lists(lists, share_prefix=True)
    assert rr.last_stats["prefix_tokens"] >= 80
    unshared = rr.score_token_lists(lists, share_prefix=False)
    assert 0.02 < float(np.std(unshared[:, 0] - unshared[:, 1])) and np.all(np.isfinite(shared))
    err = float(np.max(np.abs(shared[:, 2] - unshared[:, 2])))
    print(f"4B width shared vs unshared max |dscore| = {err:.3e}")
    assert err <= SHARED_BAR_4B, np.abs(shared - unshared).max(0)


def test_embedder_unaffected_by_the_reranker(gpu, tiny, tmp_path):
    from tiny_checkpoint import build_checkpoint as build_embedder
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker
    build_embedder(tmp_path / "emb")
    enc = Qwen3Encoder.from_pretrained(str(tmp_path / "emb"), DEV)
    texts = DOCS + ["a short query", "x" * 600]
    before = enc.encode_device(texts)[0].clone()
    rr = Qwen3Reranker.from_pretrained(str(tiny[0]), DEV, max_length=256)
    rr.rerank(QUERY, DOCS)
    rr.rerank(QUERY, DOCS, share_prefix=False)
    after = enc.encode_device(texts)[0]
    assert torch.equal(before, after)


def test_retrieve_evidence_with_the_native_reranker(gpu, tiny, monkeypatch):
    from datetime import datetime, timedelta
    from uuid import UUID

    from cadence_rag_amd import embeddings, reranker
    from cadence_rag_amd import retrieve as rt
    from cadence_rag_amd.config import settings
    from cadence_rag_amd.encoder.rerank import Qwen3Reranker
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

    chunks, cvec = make("chunks", "chunk_id", 60, lambda n: {
        "speaker": ["S"] * n, "start_ts_ms": list(range(n)), "end_ts_ms": list(range(1, n + 1)),
        "text": [DOCS[i % len(DOCS)] + f" #{i}" for i in range(n)]})
    arts, avec = make("artifact_chunks", "artifact_chunk_id", 12, lambda n: {
        "artifact_id": list(range(n)), "kind": ["summary"] * n, "content": [DOCS[(3 * i) % len(DOCS)] for i in range(n)]})
    qvec = (cvec[3] + avec[2]).tolist()
    monkeypatch.setattr(embeddings, "embeddings_enabled", lambda: True)
    monkeypatch.setattr(embeddings, "embed_texts",
                        lambda texts: embeddings.EmbeddingResult(vectors=[qvec for _ in texts], model="m"))
    be = rt.GpuRetrieveBackend(chunks, arts, calls=calls)
    rr = Qwen3Reranker.from_pretrained(str(tiny[0]), DEV, max_length=256)
    seen = {}

    class Recording:
        def rerank(self, query, documents):
            scores, order, model = rr.rerank(query, documents)
            seen.update(zip(documents, scores.tolist()))
            return scores, order, model

    monkeypatch.setattr(settings, "rerank_base_url", "native")
    reranker.set_reranker(Recording())
    try:
        resp = rt.retrieve_evidence(rt.RetrieveRequest(query=QUERY, budget=rt.Budget(max_evidence_items=20,
                                                                                    max_total_chars=20000)), be)
    finally:
        reranker.set_reranker(None)
        chunks.close()
        arts.close()
    notes = resp["notes"]["retrieval"]
    assert notes["reranked_from"] > 0
    assert notes["rerank_error"] is None and notes["rerank_model_id"] == rr.model_id
    body = {c: r for c, r in zip(chunks.columns["chunk_id"], chunks.columns["text"])}
    quote_scores = [seen[body[q["chunk_id"]]] for q in resp["quotes"]]
    assert len(quote_scores) > 1 and quote_scores == sorted(quote_scores, reverse=True)
