"""Time to the first token of a repair-round-shaped call of Qwen3Generator at the 4B config (random_init: time does not
depend on the values): a prompt of PREFIX + 256 tokens whose first PREFIX tokens the slot already holds, with
generate(reuse_prefix=True) (the slot keeps the prefix, extend() computes the 256) against reuse_prefix=False (prefill of
the whole prompt: the path generate had before extend existed).  HIP events around generate(..., max_new_tokens=1), the
median of three windows.  Then crag_enc_extend_attention alone for one layer (32 / 8 heads) at cache lengths 1024 / 4096 /
8000 with 32 / 256 new rows, beside the K and V bytes it has to read once at 8 TB/s.  Prints one JSON line
per measurement.

  python scripts/probes/extend_time.py [--out profiles/extend_bench.jsonl] [--layers 36] [--iters 3]"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd import _native  # noqa: E402
from cadence_rag_amd.encoder import ops  # noqa: E402
from cadence_rag_amd.encoder.generate import Qwen3Generator  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder  # noqa: E402

HBM_TBPS = 8.0
PREFIXES = (1024, 4096)
SUFFIX = 256
CACHE_LENS = (1024, 4096, 8000)
NEW_ROWS = (32, 256)
SPLIT, SPLIT_ROWS = _native.CRAG_EXTEND_SPLIT, _native.CRAG_EXTEND_SPLIT_ROWS


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
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    max_context = max(CACHE_LENS) + max(NEW_ROWS) + 64
    cfg = Qwen3Config(num_layers=args.layers, max_length=max_context)
    enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
    g = torch.Generator(device=dev).manual_seed(2)
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    gen = Qwen3Generator(enc, lm, max_context=max_context, max_seqs=1)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    cpu = torch.Generator().manual_seed(3)
    for prefix in PREFIXES:
        head = torch.randint(0, cfg.vocab_size, (prefix,), generator=cpu).tolist()
        # two suffixes that differ in their first token: each call finds exactly the prefix resident
        tails = [[7 + k] + torch.randint(0, cfg.vocab_size, (SUFFIX - 1,), generator=cpu).tolist() for k in range(2)]
        turn = [0]

        def call(reuse):
            turn[0] ^= 1
            gen.generate([head + tails[turn[0]]], 1, reuse_prefix=reuse)

        ms = {}
        for reuse in (False, True):
            call(reuse)                                        # warm: library handles; the slot holds the prefix
            call(reuse)
            ms[reuse] = statistics.median(window(lambda: call(reuse), args.iters, stream) for _ in range(3))
            if reuse:
                assert gen.last_reuse == {"reused": [prefix], "computed": [SUFFIX]}, gen.last_reuse
        emit({"what": "first_token", "layers": cfg.num_layers, "prefix": prefix, "suffix": SUFFIX,
              "ms_prefill_whole_prompt": round(ms[False], 3), "ms_reuse_prefix": round(ms[True], 3),
              "speedup": round(ms[False] / ms[True], 2)})
    # the attention entry alone, one layer
    c = cfg
    kc, vc = gen.cache.layer(0)
    scale = 1.0 / math.sqrt(c.head_dim)
    L0 = enc.layers[0]
    for rows in NEW_ROWS:
        qkv = torch.randn(rows, c.q_size + 2 * c.kv_size, device=dev).to(torch.bfloat16)
        out = torch.empty(rows, c.q_size, dtype=torch.bfloat16, device=dev)
        ws = ops.extend_workspace(1, c.num_heads, rows, max_context, dev)
        for length in CACHE_LENS:
            fn = lambda: ops.extend_attention(qkv, L0["q_norm"], L0["k_norm"], enc._cos_sin, kc, vc, [0], [length],  # noqa: E731
                                              [rows], out, c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale, ws)
            window(fn, 20, stream)
            us = statistics.median(window(fn, 200, stream) for _ in range(3)) * 1e3
            nbytes = 2 * c.num_kv_heads * (length + rows) * 256
            # a sequence of at most SPLIT_ROWS new rows cuts each query block's keys into splits of SPLIT keys
            splits = [-(-(length + min(q0 + 32, rows)) // SPLIT) if rows <= SPLIT_ROWS else 1 for q0 in range(0, rows, 32)]
            emit({"what": "extend_attention", "cache_len": length, "new_rows": rows, "us": round(us, 2),
                  "workgroups": c.num_kv_heads * sum(splits), "kv_bytes": nbytes,
                  "floor_us_at_8TBps": round(nbytes / (HBM_TBPS * 1e12) * 1e6, 3), "launches": 3 if max(splits) > 1 else 2})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
