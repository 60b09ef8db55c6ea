"""What the snippet windows of the BM25 lane cost at the lane's batch: 64 queries x 50 rows of 600-token
chunks, 5-term queries, window 120.  The corpus is seeded: `rows` chunks of 600 tokens from the Zipf(1) vocabulary of
scripts/bench_bm25.py; a query's rows are the top 50 of its own search, the rows /retrieve would cut snippets from.

Two JSON lines per corpus size, measured in the same run:

    search    Bm25Index.search(queries, 50), the bag reading       (the step the snippet launch follows)
    snippets  Bm25Index.snippet_windows_terms over the 3 200 pairs  (one upload, one launch)

ms per call (HIP events around `reps` back-to-back calls, the median of three rounds; the host share -- argument checks,
the upload -- is inside for both), the positions the launch reads (2 bytes each) and how many pairs took the LDS path.

    python scripts/bench_snippets.py [--rows 20000] [--terms 5] [--window 120] [--reps 50] [--out profiles/snippets.jsonl]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_bm25 import DEV, K, NQ, VOCAB, timed  # noqa: E402
from cadence_rag_amd.bm25 import SNIPPET_STAGE, Bm25Index  # noqa: E402

CHUNK_TOKENS = 600


def chunk_rows(rng, n_rows: int):
    """`n_rows` chunks of CHUNK_TOKENS Zipf(1) tokens as the arguments of Bm25Index.from_arrays, positions included."""
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    terms = np.searchsorted(np.cumsum(p), rng.random(n_rows * CHUNK_TOKENS)).clip(0, VOCAB - 1).astype(np.int64)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), CHUNK_TOKENS)
    pos = np.tile(np.arange(CHUNK_TOKENS, dtype=np.int64), n_rows)
    key = np.sort((rows * VOCAB + terms) * CHUNK_TOKENS + pos)              # by row, then term, then position
    pair_of = key // CHUNK_TOKENS
    pairs, tf = np.unique(pair_of, return_counts=True)
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs // VOCAB, minlength=n_rows), out=row_ptr[1:])
    pair_off = np.zeros(pairs.size + 1, dtype=np.int64)
    np.cumsum(tf, out=pair_off[1:])
    return row_ptr, (pairs % VOCAB).astype(np.int32), tf, pair_off, (key % CHUNK_TOKENS).astype(np.uint16), p


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="20000")
    ap.add_argument("--terms", type=int, default=5)
    ap.add_argument("--window", type=int, default=120)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for n_rows in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(20261 + n_rows % 997)
        row_ptr, row_terms, row_tf, pair_off, pair_where, p = chunk_rows(rng, n_rows)
        index = Bm25Index.from_arrays(row_ptr, row_terms, row_tf, VOCAB, np.arange(n_rows, dtype=np.int64), DEV,
                                      pair_off=pair_off, pair_where=pair_where)
        queries = [" ".join(str(int(t)) for t in rng.choice(VOCAB, size=args.terms, replace=False, p=p)) for _ in range(NQ)]
        ids, _, counts = index.search(queries, K)
        ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
        lists = [ids[q, :counts[q]] for q in range(NQ)]
        r_ptr = np.zeros(NQ + 1, dtype=np.int32)
        np.cumsum(counts, out=r_ptr[1:])
        rows = np.concatenate(lists).astype(np.int32)                        # (ids are row positions here)
        q_ptr, terms, weights = index.snippet_terms(queries)
        start, _, _, covered = index.snippet_windows_terms(q_ptr, terms, weights, r_ptr, rows, args.window)
        # the positions every pair reads: the tf of the query's terms in the row
        per_pair = np.zeros(rows.size, dtype=np.int64)
        for q in range(NQ):
            for t in terms[q_ptr[q]:q_ptr[q + 1]]:
                for i in range(r_ptr[q], r_ptr[q + 1]):
                    a, b = row_ptr[rows[i]], row_ptr[rows[i] + 1]
                    j = a + np.searchsorted(row_terms[a:b], t)
                    if j < b and row_terms[j] == t:
                        per_pair[i] += row_tf[j]
        base = {"bench": "bm25_snippets", "rows": n_rows, "chunk_tokens": CHUNK_TOKENS, "nq": NQ, "k": K,
                "terms_per_query": args.terms, "vocab": VOCAB, "window": args.window, "pairs": int(rows.size)}
        ms_search = timed(lambda: index.search(queries, K), args.reps)
        lines.append({**base, "case": "search", "ms_per_call": round(ms_search, 4),
                      "scored_postings_bytes": int(index.df[terms].sum()) * 6})
        ms = timed(lambda: index.snippet_windows_terms(q_ptr, terms, weights, r_ptr, rows, args.window), args.reps)
        lines.append({**base, "case": "snippets", "ms_per_call": round(ms, 4), "ms_over_search": round(ms - ms_search, 4),
                      "positions_read": int(per_pair.sum()), "positions_per_pair_max": int(per_pair.max(initial=0)),
                      "pairs_staged_in_lds": int((per_pair <= SNIPPET_STAGE).sum()),
                      "pairs_placed": int((start >= 0).sum().item()),
                      "slots_covered_mean": round(float(np.mean([bin(int(c) & (2 ** 64 - 1)).count("1")
                                                                 for c in covered.cpu().numpy()])), 2)})
        for line in lines[-2:]:
            print(json.dumps(line), flush=True)
        index.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
