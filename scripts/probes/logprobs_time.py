"""Cost of scoring a token (crag_enc_logprobs) at the 4B model's vocabulary, beside crag_enc_sample on the same rows, and
of generate(logprobs=n) per generated token at the 4B config (random_init: time does not depend on the values).

  kernel     us per call at 1 and 8 rows with n_top 0 and 16, with and without allowed_bits, on sample_time.py's flat
             and peaked rows, and on a row of equal logits (more than 4096 candidates reach the top: n_top rounds over
             the row instead of a count inside LDS); crag_enc_sample (T = 1, and T = 0.7 top_k = 50) on the same rows.
             HIP events around 200 calls, the median of three windows.
  generate   ms per generated token of generate(prompt of 128 ids, 32 new tokens, 1 and 8 sequences) without logprobs,
             with logprobs=0 and with logprobs=16, greedy and sampled: the three variants alternate inside one process,
             HIP events around each call, the median of three rounds.  The difference is the kernel plus the two
             device-to-host copies of a step's records.

  python scripts/probes/logprobs_time.py [--out profiles/logprobs_bench.jsonl] [--rows 1,8] [--iters 200] [--layers 36]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd.encoder import ops  # noqa: E402
from cadence_rag_amd.encoder.generate import Qwen3Generator  # noqa: E402
from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder  # noqa: E402
from cadence_rag_amd.sampling import SamplingParams  # noqa: E402

VOCAB = 151_936
PROMPT, NEW = 128, 32


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
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--no-generate", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def median_us(fn):
        window(fn, 20, stream)
        return round(statistics.median(window(fn, args.iters, stream) for _ in range(3)) * 1e3, 2)

    g = torch.Generator(device=dev).manual_seed(2)
    rng = np.random.default_rng(5)
    for n in [int(r) for r in args.rows.split(",")]:
        flat = torch.randn(n, VOCAB, generator=g, device=dev) * 3
        peaked = flat.clone()
        hot = torch.from_numpy(rng.choice(VOCAB, 200, replace=False)).to(dev)
        peaked[:, hot] += torch.linspace(8, 14, 200, device=dev)
        equal = torch.full((n, VOCAB), 1.5, device=dev)
        words = (VOCAB + 31) // 32
        bits = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (n, words), dtype=np.int64).astype(np.int32)).to(dev)
        bits[:, -1] = 0     # vocab is a multiple of 32; kept zero for a vocabulary that is not
        token = torch.from_numpy(rng.integers(0, VOCAB, n).astype(np.int32)).to(dev)
        drawn = torch.empty(n, dtype=torch.int32, device=dev)
        lp, la, lw = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        rank = torch.empty(n, dtype=torch.int32, device=dev)
        for shape, logits in (("flat", flat), ("peaked", peaked), ("equal", equal)):
            for n_top in (0, 16):
                tid = torch.empty(n, n_top, dtype=torch.int32, device=dev) if n_top else None
                tlp = torch.empty(n, n_top, dtype=torch.float32, device=dev) if n_top else None
                for with_bits in (False, True):
                    us = median_us(lambda: ops.logprobs(logits, token, lp, allowed_bits=bits if with_bits else None,
                                                        lse_all=la, lse_allowed=lw if with_bits else None, rank=rank,
                                                        top_id=tid, top_logprob=tlp))
                    emit({"what": "logprobs", "rows": n, "vocab": VOCAB, "logits": shape, "n_top": n_top,
                          "allowed_bits": with_bits, "us": us})
            if shape != "equal":
                for name, params in (("T=1", SamplingParams(1.0)), ("T=0.7 top_k=50", SamplingParams(0.7, top_k=50))):
                    us = median_us(lambda: ops.sample(logits, params, 3, list(range(n)), drawn))
                    emit({"what": "sample", "rows": n, "vocab": VOCAB, "logits": shape, "config": name, "us": us})
    if not args.no_generate:
        cfg = Qwen3Config(num_layers=args.layers, max_length=PROMPT + NEW + 64)
        enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
        lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        gen = Qwen3Generator(enc, lm, max_context=PROMPT + NEW + 64)
        for n in [int(r) for r in args.rows.split(",")]:
            prompts = [rng.integers(0, cfg.vocab_size, PROMPT).tolist() for _ in range(n)]
            for mode, sampling in (("greedy", None), ("sampled", SamplingParams(0.8, top_p=0.95, seed=1))):
                variants = (("off", None), ("logprobs=0", 0), ("logprobs=16", 16))
                times = {name: [] for name, _ in variants}
                for rnd in range(4):        # round 0 warms every shape
                    for name, k in variants:
                        ms = window(lambda: gen.generate(prompts, NEW, sampling=sampling, logprobs=k), 1, stream)
                        if rnd:
                            times[name].append(ms)
                base = statistics.median(times["off"])
                for name, _ in variants:
                    ms = statistics.median(times[name])
                    emit({"what": "generate", "path": gen.last_path, "layers": cfg.num_layers, "n_seqs": n, "mode": mode,
                          "logprobs": name, "prompt": PROMPT, "new_tokens": NEW, "ms_per_call": round(ms, 3),
                          "ms_per_token_over_off": round((ms - base) / NEW, 4),
                          "ms_per_step_incl_prefill": round(ms / NEW, 4)})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
