"""What a multi-row decode step costs, at the 4B config (random_init: time does not depend on the values), in one process
on one GPU -- HIP events, the median of three windows, the windows' spread beside it.  The baseline is always the path
of the commit before step_rows, run here: step(), crag_enc_decode_attention.

  (a) one layer's crag_enc_decode_attention_rows over R = 1, 2, 4, 8 rows of one sequence at 128, 1024 and 4096 cached
      tokens, and over two sequences of four rows, against crag_enc_decode_attention with one row per sequence.  The rows
      one workgroup serves is ROWS_UNIT_MEMBERS of crag_decode.hip (1, 2, 4 or 8): build one library per
      size, point CRAG_DENSE_LIB at it and name the size with --unit-rows; one process per library.
  (b) Qwen3Generator.step_rows over the same shapes against step(), and the break-even acceptance t_rows(R) / t_step - 1:
      the accepted drafts per forward above which speculation is faster than plain decoding.

Prints one JSON line per measurement and appends them to --out.

  python scripts/probes/speculate_time.py [--out profiles/speculate_bench.jsonl] [--layers 36] [--unit-rows N]
                                          [--skip-attention] [--skip-model]"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd.encoder import ops  # noqa: E402
from cadence_rag_amd.encoder.generate import KvCache, Qwen3Generator  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder  # noqa: E402

CACHED = (128, 1024, 4096)
SHAPES = [(1, 1), (1, 2), (1, 4), (1, 8), (2, 4)]     # (sequences, rows of each)


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
    ap.add_argument("--unit-rows", type=int, default=None, help="ROWS_UNIT_MEMBERS of the loaded library (a label)")
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    max_context = max(CACHED) + 64
    cfg = Qwen3Config(num_layers=1 if args.skip_model else args.layers, max_length=max_context)
    enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        if args.unit_rows is not None:
            rec["unit_rows"] = args.unit_rows
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(rec, name, fn, iters, unit=1e3, suffix="_us"):
        window(fn, max(iters // 10, 2), stream)
        med, lo, hi = three(fn, iters, stream)
        rec[name + suffix] = round(med * unit, 2)
        rec[name + "_spread" + suffix] = [round(lo * unit, 2), round(hi * unit, 2)]
        return med

    c = cfg
    if not args.skip_attention:   # (a) one layer
        cache = KvCache(1, 2, c.num_kv_heads, max_context, dev)
        cache.k.normal_()
        cache.v.normal_()
        kc, vc = cache.layer(0)
        ws = ops.decode_workspace(8, c.num_heads, max_context, dev)
        scale = 1.0 / math.sqrt(c.head_dim)
        L0 = enc.layers[0]
        qkv = torch.randn(8, c.q_size + 2 * c.kv_size, device=dev).to(torch.bfloat16)
        out = torch.empty(8, c.q_size, dtype=torch.bfloat16, device=dev)
        head = (qkv, L0["q_norm"], L0["k_norm"], enc._cos_sin, kc, vc)
        tail = (c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale, ws)
        for cached in CACHED:
            for n, r in SHAPES:
                slots, lens = list(range(n)), [cached] * n
                rec = {"what": "decode_attention_rows", "sequences": n, "rows_each": r, "cached_tokens": cached}
                timed(rec, "one_row_entry", lambda: ops.decode_attention(*head, slots, lens, out, *tail), 200)
                timed(rec, "rows_entry", lambda: ops.decode_attention_rows(*head, slots, lens, [r] * n, out, *tail), 200)
                emit(rec)
        del cache, kc, vc

    if not args.skip_model:       # (b) the whole step
        g = torch.Generator(device=dev).manual_seed(2)
        lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        gen = Qwen3Generator(enc, lm, max_context=max_context, max_seqs=2)

        def at(cached, n, fn):
            def run():
                gen.cache.lens[:n] = [cached] * n     # the step before grew them; the rows' values do not matter
                fn()
            return run

        for cached in CACHED:
            base = {}
            for n, r in SHAPES:
                slots = list(range(n))
                rec = {"what": "step_rows", "sequences": n, "rows_each": r, "cached_tokens": cached,
                       "layers": cfg.num_layers}
                if n not in base:
                    base[n] = timed(rec, "step", at(cached, n, lambda: gen.step([5] * n, slots=slots)), 30, 1.0, "_ms")
                    rec["step_path"] = gen.last_path
                t = timed(rec, "step_rows", at(cached, n, lambda: gen.step_rows([[5] * r] * n, slots=slots)), 30, 1.0, "_ms")
                rec["step_rows_path"] = gen.last_path
                rec["step_baseline_ms"] = round(base[n], 3)
                rec["break_even_accepted_per_forward"] = round(t / base[n] - 1.0, 3)
                emit(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with Path(args.out).open("a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
