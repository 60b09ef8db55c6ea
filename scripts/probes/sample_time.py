"""Cost of a sampled token selection (crag_enc_sample) at the 4B model's vocabulary, beside the head it follows
(crag_enc_lm_head: lm_head_kernel + lm_argmax_kernel), the greedy selection alone (lm_argmax's time = lm_head minus its
GEMM is not separable by events, so the T = 0 row of crag_enc_sample -- the same single pass -- stands beside it) and
crag_enc_grammar_argmax with allowed_bits, all from the same run.  Logits: Gaussian with sd 3 (a flat row: the widest
kept sets) and a peaked row (sd 3 plus 200 ids raised by 8..14, closer to a language model's).  HIP events around 200
calls, the median of three windows.  Prints one JSON line per measurement.

  python scripts/probes/sample_time.py [--out profiles/sample_bench.jsonl] [--rows 1,8] [--iters 200]
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
from cadence_rag_amd.grammar import ByteDfa, TokenTable  # noqa: E402
from cadence_rag_amd.sampling import SamplingParams  # noqa: E402

VOCAB = 151_936
HIDDEN = 2560
CONFIGS = [("T=0", SamplingParams(0.0)), ("T=1", SamplingParams(1.0)), ("T=0.7 top_k=50", SamplingParams(0.7, top_k=50)),
           ("T=0.7 top_p=0.9", SamplingParams(0.7, top_p=0.9)),
           ("T=1 top_p=0.9 min_p=0.05", SamplingParams(1.0, top_p=0.9, min_p=0.05))]


def window(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def median_us(fn):
        window(fn, 20, stream)
        return round(statistics.median(window(fn, args.iters, stream) for _ in range(3)), 2)

    g = torch.Generator(device=dev).manual_seed(2)
    rng = np.random.default_rng(5)
    # the bits of a permissive automaton state: 94 % of the ids allowed (the citation grammar's start state)
    kind = np.where(rng.random(VOCAB) < 0.06, 2, 0).astype(np.uint8)
    table = TokenTable(np.arange(VOCAB + 1, dtype=np.int32), np.full(VOCAB, 65, np.uint8), kind)
    dfa = ByteDfa(np.zeros(256, np.uint8), np.zeros((1, 1), np.uint16), np.ones(1, np.uint8))
    tables = table.to(dev) + dfa.to(dev)
    for n in [int(r) for r in args.rows.split(",")]:
        flat = torch.randn(n, VOCAB, generator=g, device=dev) * 3
        peaked = flat.clone()
        hot = torch.from_numpy(rng.choice(VOCAB, 200, replace=False)).to(dev)
        peaked[:, hot] += torch.linspace(8, 14, 200, device=dev)
        token = torch.empty(n, dtype=torch.int32, device=dev)
        kept = torch.empty(n, dtype=torch.int32, device=dev)
        state = torch.zeros(n, dtype=torch.int32, device=dev)
        bits = torch.empty(n, (VOCAB + 31) // 32, dtype=torch.int32, device=dev)
        us = median_us(lambda: ops.grammar_argmax(flat, *tables, state, token, allowed_bits=bits))
        emit({"what": "grammar_argmax", "rows": n, "vocab": VOCAB, "allowed_bits": True, "allowed_share": 0.94, "us": us})
        us = median_us(lambda: ops.grammar_advance(*tables[:5], state, token))
        emit({"what": "grammar_advance", "rows": n, "us": us})
        for shape, logits in (("flat", flat), ("peaked", peaked)):
            for name, params in CONFIGS:
                for with_bits in (False, True):
                    us = median_us(lambda: ops.sample(logits, params, 3, list(range(n)), token,
                                                      allowed_bits=bits if with_bits else None, kept=kept))
                    emit({"what": "sample", "rows": n, "vocab": VOCAB, "logits": shape, "config": name,
                          "allowed_bits": with_bits, "us": us, "kept_row0": int(kept[0].item())})
    lm = (torch.randn(VOCAB, HIDDEN, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    w = torch.ones(HIDDEN, dtype=torch.bfloat16, device=dev)
    for n in [int(r) for r in args.rows.split(",")]:
        hs = torch.randn(n, HIDDEN, generator=g, device=dev).to(torch.bfloat16)
        logits = torch.empty(n, VOCAB, dtype=torch.float32, device=dev)
        token = torch.empty(n, dtype=torch.int32, device=dev)
        us = median_us(lambda: ops.lm_head(hs, w, lm, logits, token, 1e-6))
        emit({"what": "lm_head", "rows": n, "vocab": VOCAB, "hidden": HIDDEN, "us": us, "launches": 2})
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
