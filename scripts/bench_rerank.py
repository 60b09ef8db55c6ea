"""Reranker throughput: Qwen3Reranker forwards with random weights at the Qwen3-Reranker-4B and -0.6B widths.

For every shape (pairs x document tokens, a ~20-token query) one JSON line: ms per call with the shared prefix and
without, pairs/s, real and executed tokens, and the fraction of the 2.5 PF/s dense bf16 MFMA peak reached on the
executed FLOPs (Qwen3Config.flops_per_token at the pairs' mean length, minus the last layer's skipped rows).  A last
line per model times crag_enc_attention_prefixed beside crag_enc_attention on the same unshared 80 x 350 batch.

    python scripts/bench_rerank.py [--model 4b|0.6b|both] [--reps 3] [--shapes 16x350,80x350,...]
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cadence_rag_amd.encoder import ops  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import PackedBatch, Qwen3Config, Qwen3Encoder  # noqa: E402
from cadence_rag_amd.encoder.rerank import Qwen3Reranker  # noqa: E402

PEAK_FLOPS = 2.5e15
# token counts of the model card's template with the Qwen3 tokenizer, rounded: system prompt + instruction + a 20-token
# query before the document (all pairs of a call share them), the assistant suffix after it
HEAD_TOKENS = 82
SUFFIX_TOKENS = 13
MODELS = {
    "4b": Qwen3Config(hidden_size=2560, num_layers=36, num_heads=32, num_kv_heads=8, intermediate_size=9728,
                      vocab_size=151669, max_length=1024, model_id="Qwen/Qwen3-Reranker-4B"),
    "0.6b": Qwen3Config(hidden_size=1024, num_layers=28, num_heads=16, num_kv_heads=8, intermediate_size=3072,
                        vocab_size=151669, max_length=1024, model_id="Qwen/Qwen3-Reranker-0.6B"),
}


def token_lists(n_pairs: int, doc_tokens: int, vocab: int, seed: int):
    rng = np.random.default_rng(seed)
    head = rng.integers(0, vocab, HEAD_TOKENS).tolist()
    suffix = rng.integers(0, vocab, SUFFIX_TOKENS).tolist()
    return [head + rng.integers(0, vocab, doc_tokens).tolist() + suffix for _ in range(n_pairs)]


def time_call(rr: Qwen3Reranker, lists, share: bool, reps: int) -> float:
    rr.score_token_lists(lists, share_prefix=share)          # warm-up (library GEMM selection)
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rr.score_token_lists(lists, share_prefix=share)       # returns host scores: the call is complete
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def executed_flops(cfg: Qwen3Config, stats, lists) -> float:
    avg_ctx = float(np.mean([len(tl) for tl in lists]))
    rows_out = stats["pairs"]
    return cfg.flops_per_token(avg_ctx) * stats["executed_tokens"] - cfg.flops_skipped_in_last_layer(
        stats["executed_tokens"], rows_out)


def attention_compare(cfg: Qwen3Config, lists, reps: int = 20):
    """Per-launch time of crag_enc_attention and crag_enc_attention_prefixed on the same unshared batch, and of the
    prefixed kernel on the shared layout of the same pairs."""
    dev = torch.device("cuda", 0)
    hq, hkv = cfg.num_heads, cfg.num_kv_heads
    lens = [len(tl) for tl in lists]
    p = HEAD_TOKENS
    out = {}
    for name, lengths, parent in (("unshared", lens, [-1] * len(lens)),
                                  ("shared", [p] + [n - p for n in lens], [-1] + [0] * len(lens))):
        t = sum(lengths)
        qkv = (torch.randn(t + 32, (hq + 2 * hkv) * 128, device=dev)).to(torch.bfloat16)
        batch = PackedBatch.build_prefixed(lengths, parent, dev)
        vt = torch.empty(hkv, 128, batch.t_pad, dtype=torch.bfloat16, device=dev)
        ops.v_transpose(qkv, vt, batch.tok_of_pad, hq, hkv)
        o = torch.empty(t, hq * 128, dtype=torch.bfloat16, device=dev)
        runs = {"attention_prefixed": lambda: ops.attention_prefixed(qkv, vt, o, batch.cu, batch.cu_pad, batch.blk_seq,
                                                                     batch.blk_q0, batch.parent, hq, hkv,
                                                                     1 / math.sqrt(128))}
        if name == "unshared":
            plain = PackedBatch.build(lengths, dev)
            runs["attention"] = lambda: ops.attention(qkv, vt, o, plain.cu, plain.cu_pad, plain.blk_seq, plain.blk_q0,
                                                      hq, hkv, 1 / math.sqrt(128))
        for kname, fn in runs.items():
            fn()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fn()
            end.record()
            end.synchronize()
            out[f"{kname}_{name}_us"] = round(start.elapsed_time(end) * 1e3 / reps, 1)
        out[f"tokens_{name}"] = t
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=["4b", "0.6b", "both"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="16x350,16x600,80x350,80x600,160x350,160x600")
    ap.add_argument("--budget", type=int, default=65536)
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    dev = torch.device("cuda", 0)
    for key in (["4b", "0.6b"] if args.model == "both" else [args.model]):
        cfg = MODELS[key]
        enc = Qwen3Encoder.random_init(cfg, seed=0, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        lm = (torch.randn(2, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        rr = Qwen3Reranker(enc, lm, token_budget=args.budget, model_id=cfg.model_id)
        for n_pairs, doc in shapes:
            lists = token_lists(n_pairs, doc, cfg.vocab_size, seed=n_pairs * 1000 + doc)
            line = {"bench": "rerank", "model": cfg.model_id, "pairs": n_pairs, "doc_tokens": doc,
                    "query_head_tokens": HEAD_TOKENS}
            for share in (True, False):
                ms = time_call(rr, lists, share, args.reps)
                st = rr.last_stats
                tag = "shared" if share else "unshared"
                line[f"ms_{tag}"] = round(ms, 2)
                line[f"pairs_per_s_{tag}"] = round(n_pairs / (ms / 1e3), 1)
                line[f"executed_tokens_{tag}"] = st["executed_tokens"]
                line[f"forwards_{tag}"] = st["forwards"]
                line[f"mfma_fraction_{tag}"] = round(executed_flops(cfg, st, lists) / (ms / 1e3) / PEAK_FLOPS, 4)
                line["real_tokens"] = st["real_tokens"]
                line["prefix_tokens"] = st["prefix_tokens"] if share else line.get("prefix_tokens")
            line["time_ratio"] = round(line["ms_shared"] / line["ms_unshared"], 4)
            line["token_ratio"] = round(line["executed_tokens_shared"] / line["executed_tokens_unshared"], 4)
            print(json.dumps(line), flush=True)
        att = attention_compare(cfg, token_lists(80, 350, cfg.vocab_size, seed=80350))
        print(json.dumps({"bench": "rerank_attention", "model": cfg.model_id, "pairs": 80, "doc_tokens": 350, **att}),
              flush=True)
        del rr, enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
