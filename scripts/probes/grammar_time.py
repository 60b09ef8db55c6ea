"""Cost of the selection under a citation grammar (crag_enc_grammar_argmax) at the 4B model's vocabulary, beside the
head it follows (crag_enc_lm_head: lm_head_kernel + lm_argmax_kernel) from the same run.  The vocabulary is synthetic --
the 256 single bytes, then seeded strings whose lengths follow a byte-level BPE's (1..16 bytes, most of them 3..7, one of
48) -- because only the byte lengths and the share of refused tokens matter to the walk.  States: the start of the
grammar of 12 ids (most tokens allowed), inside a sentence, and behind `[` (two tokens in a thousand allowed, so every
thread walks every one of its tokens).  HIP events around 200 calls, the median of three windows; each call is preceded
by the 32-byte copy that puts the states back, timed alone as well.  Prints one JSON line per measurement.

  python scripts/probes/grammar_time.py [--out profiles/grammar_bench.jsonl] [--only grammar|head] [--rows 1,8]

Kernel times proper: run it under `rocprofv3 --kernel-trace --stats -- python scripts/probes/grammar_time.py --rows 1
--states start` (and --rows 8), which keeps one shape per kernel name."""
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
from cadence_rag_amd.grammar import TokenTable, allowed_tokens_host, citation_grammar, walk  # noqa: E402

VOCAB = 151_936
HIDDEN = 2560


def window(fn, iters, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def synthetic_table(seed: int = 1) -> TokenTable:
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxz" * 3 + b"ETAOINSHR0123456789" + b"   .,!?-_[]()\"'\n:;/", dtype=np.uint8)
    lengths = np.clip(rng.poisson(4.0, VOCAB) + 1, 1, 16)
    tokens = [bytes([b]) for b in range(256)]
    for n in lengths[256:]:
        body = alphabet[rng.integers(0, alphabet.size, int(n))].tobytes()
        tokens.append((b" " + body[1:]) if rng.random() < 0.5 and n > 1 else body)
    tokens[1000] = b" " * 48
    stops = [VOCAB - 300, VOCAB - 299]
    for s in stops:
        tokens[s] = b"<stop>"
    for i in range(VOCAB - 298, VOCAB):      # the padded tail of a model's vocabulary: no bytes
        tokens[i] = None
    return TokenTable.from_bytes(tokens, stop_ids=stops)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["grammar", "head"], default=None)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--states", default="start,sentence,bracket")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    rows_list = [int(r) for r in args.rows.split(",")]
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def median_us(fn):
        window(fn, 20, stream)
        return round(statistics.median(window(fn, args.iters, stream) for _ in range(3)), 2)

    g = torch.Generator(device=dev).manual_seed(2)
    if args.only != "head":
        dfa = citation_grammar([f"Q-{100 + 7 * i}" for i in range(9)] + ["A-3", "A-45", "A-46"])
        table = synthetic_table()
        tables = table.to(dev) + dfa.to(dev)
        named = {"start": dfa.start, "sentence": walk(dfa, dfa.start, b"The rollback was agreed"),
                 "bracket": walk(dfa, dfa.start, b"The rollback was agreed [")}
        for n in rows_list:
            logits = torch.randn(n, VOCAB, generator=g, device=dev)
            token = torch.empty(n, dtype=torch.int32, device=dev)
            bits = torch.empty(n, (VOCAB + 31) // 32, dtype=torch.int32, device=dev)
            for name in args.states.split(","):
                state0 = torch.full((n,), int(named[name]), dtype=torch.int32, device=dev)
                state = state0.clone()
                copy_us = median_us(lambda: state.copy_(state0))
                share = float(allowed_tokens_host(dfa, table, named[name]).mean())
                for with_bits in (False, True):
                    def fn():
                        state.copy_(state0)
                        ops.grammar_argmax(logits, *tables, state, token, allowed_bits=bits if with_bits else None)
                    us = median_us(fn)
                    emit({"what": "grammar_argmax", "rows": n, "vocab": VOCAB, "state": name, "n_states": dfa.n_states,
                          "n_classes": dfa.n_classes, "allowed_share": round(share, 4), "allowed_bits": with_bits,
                          "us_with_state_copy": us, "state_copy_us": copy_us})
    if args.only != "grammar":
        lm = (torch.randn(VOCAB, HIDDEN, generator=g, device=dev) * 0.02).to(torch.bfloat16)
        w = torch.ones(HIDDEN, dtype=torch.bfloat16, device=dev)
        for n in rows_list:
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
