"""What forking one prefill saves, at the 4B config (random_init: time does not depend on the values), in one process on
one GPU -- HIP events, the median of three windows, the windows' spread beside it.  The baseline is always the path of
the commit before forks, run here: private copies of the rows, the duplicated prompt.

  (a) one layer's crag_enc_decode_attention_shared over n = 2, 4, 8 children of one parent (outside the call) at 1024 and
      4096 shared keys plus 64 private ones, against crag_enc_decode_attention over n slots that each hold all the rows;
  (b) generate_samples(p, 8, 64) against generate([p] * 8, 64) at prompts of 1024 and 4096 tokens: the whole call, the
      prefill alone (prefill([p]) against prefill([p] * 8)), and the steps as the difference.

Prints one JSON line per measurement and appends them to --out.

  python scripts/probes/fork_time.py [--out profiles/fork_bench.jsonl] [--layers 36] [--new 64]"""
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
from cadence_rag_amd.encoder.generate import KvCache, Qwen3Generator  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder  # noqa: E402

SHARED = (1024, 4096)
PRIVATE = 64


def window(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms


def three(fn, iters, stream):
    """(median, lowest, highest) of three windows."""
    w = sorted(window(fn, iters, stream) for _ in range(3))
    return w[1], w[0], w[2]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--skip-generate", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    max_context = max(SHARED) + max(args.new, PRIVATE) + 64
    cfg = Qwen3Config(num_layers=args.layers, max_length=max_context)
    enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    # (a) one layer: children of slot 8 in slots 0..n-1, or the same rows held by every slot
    c = cfg
    cache = KvCache(1, 9, c.num_kv_heads, max_context, dev)
    cache.k.normal_()
    cache.v.normal_()
    kc, vc = cache.layer(0)
    ws = ops.decode_workspace(8, c.num_heads, max_context, dev)
    scale = 1.0 / math.sqrt(c.head_dim)
    L0 = enc.layers[0]
    for n in (2, 4, 8):
        qkv = torch.randn(n, c.q_size + 2 * c.kv_size, device=dev).to(torch.bfloat16)
        out = torch.empty(n, c.q_size, dtype=torch.bfloat16, device=dev)
        slots = list(range(n))
        for shared in SHARED:
            lens = [shared + PRIVATE] * n
            private = lambda: ops.decode_attention(qkv, L0["q_norm"], L0["k_norm"], enc._cos_sin, kc, vc, slots, lens,  # noqa: E731
                                                   out, c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale, ws)
            forked = lambda: ops.decode_attention_shared(qkv, L0["q_norm"], L0["k_norm"], enc._cos_sin, kc, vc, slots,  # noqa: E731
                                                         lens, [8] * n, [shared] * n, out, c.num_heads, c.num_kv_heads,
                                                         c.rms_norm_eps, scale, ws)
            rec = {"what": "decode_attention_shared", "children": n, "shared_keys": shared, "private_keys": PRIVATE}
            for name, fn in (("private_copies", private), ("forked", forked)):
                window(fn, 20, stream)
                med, lo, hi = three(fn, 200, stream)
                rec[name + "_us"] = round(med * 1e3, 2)
                rec[name + "_spread_us"] = [round(lo * 1e3, 2), round(hi * 1e3, 2)]
            rec["kv_bytes_private"] = n * 2 * c.num_kv_heads * (shared + PRIVATE + 1) * 256
            rec["kv_bytes_forked"] = 2 * c.num_kv_heads * (shared + n * (PRIVATE + 1)) * 256
            emit(rec)
    del cache, kc, vc

    # (b) eight continuations of one prompt
    if not args.skip_generate:
        g = torch.Generator(device=dev).manual_seed(2)
        lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        gen = Qwen3Generator(enc, lm, max_context=max_context)
        for length in SHARED:
            prompt = [11 + (7 * i) % 1000 for i in range(length)]
            runs = {"duplicated_prompt": (lambda: gen.generate([prompt] * 8, args.new), lambda: gen.prefill([prompt] * 8)),
                    "forked": (lambda: gen.generate_samples(prompt, 8, args.new), lambda: gen.prefill([prompt]))}
            rec = {"what": "generate_samples", "n": 8, "prompt_tokens": length, "new_tokens": args.new,
                   "layers": cfg.num_layers}
            for name, (whole, prefill) in runs.items():
                whole()                                          # warm: library handles, the re-tiled weights
                total, lo, hi = three(whole, 1, stream)
                pre, plo, phi = three(prefill, 1, stream)
                rec[name] = {"total_ms": round(total, 2), "total_spread_ms": [round(lo, 2), round(hi, 2)],
                             "prefill_ms": round(pre, 2), "prefill_spread_ms": [round(plo, 2), round(phi, 2)],
                             "steps_ms": round(total - pre, 2), "step_path": gen.last_path}
            emit(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with Path(args.out).open("a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
