"""Time of one decode step of Qwen3Generator at the 4B config (random_init: time does not depend on the values) at cache
lengths 128, 1024 and 4096 for 1 and 8 sequences -- HIP events around 50 steps, the median of three windows -- and of the
two new entries alone (crag_enc_decode_attention for one layer, crag_enc_lm_head).  Beside each the byte model
(weights + 2 * layers * hkv * len * 256 per sequence) and its time at 8 TB/s.  Prints one JSON line per measurement.

  python scripts/probes/decode_time.py [--out profiles/decode_bench.jsonl] [--layers 36] [--steps 50]"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd.encoder import ops  # noqa: E402
from cadence_rag_amd.encoder.generate import Qwen3Generator  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder  # noqa: E402

HBM_TBPS = 8.0
LENGTHS = (128, 1024, 4096)


def window(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    max_context = max(LENGTHS) + 4 * args.steps + 64
    cfg = Qwen3Config(num_layers=args.layers, max_length=max_context)
    enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
    g = torch.Generator(device=dev).manual_seed(2)
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    gen = Qwen3Generator(enc, lm, max_context=max_context)
    stream = torch.cuda.current_stream(dev)
    per_layer = cfg.hidden_size * (cfg.q_size + 2 * cfg.kv_size) + cfg.q_size * cfg.hidden_size \
        + 3 * cfg.hidden_size * cfg.intermediate_size
    weight_bytes = 2 * (cfg.num_layers * per_layer + cfg.vocab_size * cfg.hidden_size)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n in (1, 8):
        slots = list(range(n))
        tokens = [11 + i for i in range(n)]
        for length in LENGTHS:
            def steps(k):
                for s in slots:
                    gen.cache.lens[s] = length
                return window(lambda: gen.step(tokens, slots=slots), k, stream)
            steps(5)                                          # warm: library handles, the re-tiled weights
            ms = statistics.median(steps(args.steps) for _ in range(3))
            cache_bytes = n * 2 * cfg.num_layers * cfg.num_kv_heads * (length + args.steps // 2) * 256
            floor_ms = (weight_bytes + cache_bytes) / (HBM_TBPS * 1e12) * 1e3
            emit({"what": "step", "path": gen.last_path, "layers": cfg.num_layers, "n_seqs": n, "cache_len": length,
                  "ms_per_step": round(ms, 4), "weight_bytes": weight_bytes, "cache_bytes": cache_bytes,
                  "floor_ms_at_8TBps": round(floor_ms, 4), "fraction_of_byte_model": round(floor_ms / ms, 4)})
    # the two entries alone
    c = cfg
    kc, vc = gen.cache.layer(0)
    scale = 1.0 / math.sqrt(c.head_dim)
    for n in (1, 8):
        qkv = torch.randn(n, c.q_size + 2 * c.kv_size, device=dev).to(torch.bfloat16)
        out = torch.empty(n, c.q_size, dtype=torch.bfloat16, device=dev)
        L0 = enc.layers[0]
        for length in LENGTHS:
            fn = lambda: ops.decode_attention(qkv, L0["q_norm"], L0["k_norm"], enc._cos_sin, kc, vc, list(range(n)),  # noqa: E731
                                              [length] * n, out, c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale,
                                              gen._workspace)
            window(fn, 20, stream)
            us = statistics.median(window(fn, 200, stream) for _ in range(3)) * 1e3
            nbytes = n * 2 * c.num_kv_heads * (length + 1) * 256
            emit({"what": "decode_attention", "n_seqs": n, "cache_len": length, "us": round(us, 2), "kv_bytes": nbytes,
                  "floor_us_at_8TBps": round(nbytes / (HBM_TBPS * 1e12) * 1e6, 3), "launches": 3})
        hs = torch.randn(n, c.hidden_size, device=dev).to(torch.bfloat16)
        logits = torch.empty(n, c.vocab_size, dtype=torch.float32, device=dev)
        token = torch.empty(n, dtype=torch.int32, device=dev)
        fn = lambda: ops.lm_head(hs, enc.final_norm, lm, logits, token, c.rms_norm_eps)  # noqa: E731
        window(fn, 10, stream)
        us = statistics.median(window(fn, 100, stream) for _ in range(3)) * 1e3
        nbytes = 2 * c.vocab_size * c.hidden_size
        emit({"what": "lm_head", "rows": n, "vocab": c.vocab_size, "us": round(us, 2), "weight_bytes": nbytes,
              "floor_us_at_8TBps": round(nbytes / (HBM_TBPS * 1e12) * 1e6, 2),
              "fraction_of_byte_model": round(nbytes / (HBM_TBPS * 1e12) * 1e6 / us, 4), "launches": 2})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
