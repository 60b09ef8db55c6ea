"""Cost of repetition control (crag_enc_adjust_logits) at the 4B model's vocabulary, beside crag_enc_lm_head on the same
rows in the same run, and of generate(penalties=...) per generated token at the 4B config (random_init: time does not
depend on the values).

  kernel     us per call at 1 and 8 rows with histories of 512 and 4096 ids (a quarter of them prompt), every clause on,
             with and without a bias list of 256 entries; and with a neutral rule over an empty history: the zeroing and
             the vocabulary walk alone.  crag_enc_lm_head (hidden 2560) for the same rows, and the ratio of the two.
             HIP events around 200 calls, the median of three windows.
  generate   ms per generated token of generate(prompt of 128 ids, 32 new tokens, 1 and 8 sequences) without and with
             penalties, greedy and sampled: the variants alternate inside one process, HIP events around each call, the
             median of three rounds.  The difference is the kernel plus the append of the picked tokens to the log.

  python scripts/probes/penalty_time.py [--out profiles/penalty_bench.jsonl] [--rows 1,8] [--iters 200] [--layers 36]
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
from cadence_rag_amd.penalties import PenaltyParams  # noqa: E402
from cadence_rag_amd.sampling import SamplingParams  # noqa: E402

VOCAB = 151_936
HIDDEN = 2560
PROMPT, NEW = 128, 32
EVERY = PenaltyParams(repetition_penalty=1.2, presence_penalty=0.4, frequency_penalty=0.2, no_repeat_ngram=3)


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
    lm = (torch.randn(VOCAB, HIDDEN, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    norm_w = torch.ones(HIDDEN, dtype=torch.bfloat16, device=dev)
    for n in [int(r) for r in args.rows.split(",")]:
        hs = torch.randn(n, HIDDEN, generator=g, device=dev).to(torch.bfloat16)
        logits = torch.empty(n, VOCAB, dtype=torch.float32, device=dev)
        token = torch.empty(n, dtype=torch.int32, device=dev)
        head_us = median_us(lambda: ops.lm_head(hs, norm_w, lm, logits, token, 1e-6))
        emit({"what": "lm_head", "rows": n, "vocab": VOCAB, "hidden": HIDDEN, "us": head_us})
        out = torch.empty_like(logits)
        ws = ops.adjust_workspace(n, VOCAB, dev)
        ids = torch.from_numpy(np.sort(rng.choice(VOCAB, 256, replace=False)).astype(np.int32)).to(dev)
        bias = dict(bias_ids=ids.repeat(n), bias_values=torch.full((256 * n,), -1.0, device=dev),
                    bias_offsets=[256 * r for r in range(n + 1)])
        cases = [("walk only", PenaltyParams(), 0, {})]
        for length in (512, 4096):
            cases += [(f"history {length}", EVERY, length, {}), (f"history {length} + 256 bias", EVERY, length, bias)]
        for name, params, length, extra in cases:
            log = torch.from_numpy(rng.integers(0, 4000, (n, max(length, 1))).astype(np.int32)).to(dev)
            us = median_us(lambda: ops.adjust_logits(logits, out, log, list(range(n)), [length // 4] * n, [length] * n,
                                                     params, token, ws, **extra))
            emit({"what": "adjust_logits", "rows": n, "vocab": VOCAB, "case": name, "us": us,
                  "lm_head_us": head_us, "ratio_to_lm_head": round(us / head_us, 4)})
    if not args.no_generate:
        del lm
        cfg = Qwen3Config(num_layers=args.layers, max_length=PROMPT + NEW + 64)
        enc = Qwen3Encoder.random_init(cfg, seed=1, device=dev)
        lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        gen = Qwen3Generator(enc, lm, max_context=PROMPT + NEW + 64)
        for n in [int(r) for r in args.rows.split(",")]:
            prompts = [rng.integers(0, cfg.vocab_size, PROMPT).tolist() for _ in range(n)]
            for mode, sampling in (("greedy", None), ("sampled", SamplingParams(0.8, top_p=0.95, seed=1))):
                variants = (("off", None), ("penalties", EVERY))
                times = {name: [] for name, _ in variants}
                for rnd in range(4):        # round 0 warms every shape
                    for name, p in variants:
                        ms = window(lambda: gen.generate(prompts, NEW, sampling=sampling, penalties=p), 1, stream)
                        if rnd:
                            times[name].append(ms)
                base = statistics.median(times["off"])
                for name, _ in variants:
                    ms = statistics.median(times[name])
                    emit({"what": "generate", "path": gen.last_path, "layers": cfg.num_layers, "n_seqs": n, "mode": mode,
                          "penalties": name, "prompt": PROMPT, "new_tokens": NEW, "ms_per_call": round(ms, 3),
                          "ms_per_token_over_off": round((ms - base) / NEW, 4),
                          "ms_per_step_incl_prefill": round(ms / NEW, 4)})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
