"""What the clause syntax of the BM25 lane costs, on the seeded Zipf corpus of scripts/bench_bm25.py:
rows x 64 queries of 4-12 terms, k = 50.  Token positions are synthesised by laying each row's tokens out in a seeded
order.  Five cases over the SAME scored bag per query:

    plain     Bm25Index.search                                  (the yardstick, measured in the same run)
    required  search_query, the bag's most frequent term carries a `+`
    excluded  search_query, one `-term` (a frequent term outside the bag) appended
    phrase    search_query, the bag's two most frequent terms quoted as a phrase
    two_required  search_query, those two terms as `+a +b`: what the phrase costs before compaction and verification

One JSON line per corpus size and case: ms per call (HIP events around `reps` back-to-back calls, the median of three
rounds; the host share -- parsing, weights, uploads -- is inside, as it is for `plain`), ms of the clause-mask launch alone
(the C entry with prepared arrays), and the cost-model bytes that launch adds: 4 per posting of every clause term, plus,
for a phrase, 8 + 2 * tf per verified candidate row and member term.

    python scripts/bench_bm25_syntax.py [--rows 100000,1000000] [--reps 50] [--out profiles/bm25_syntax_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_bm25 import DEV, K, NQ, VOCAB, timed, zipf_rows  # noqa: E402
from cadence_rag_amd import _native  # noqa: E402
from cadence_rag_amd.bm25 import Bm25Index, parse_query  # noqa: E402


def synth_positions(rng, row_ptr, row_tf):
    """pair_off / pair_where of Bm25Index.from_arrays: every row's tokens (term t, tf times) laid out in a seeded order."""
    n_rows = row_ptr.size - 1
    pair_row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(row_ptr))
    tok_pair = np.repeat(np.arange(row_tf.size, dtype=np.int64), row_tf)      # the (row, term) pair of every token
    tok_row = pair_row[tok_pair]
    order = np.lexsort((rng.random(tok_pair.size), tok_row))                  # a seeded order inside every row
    first = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(tok_row, minlength=n_rows), out=first[1:])
    pos = np.empty(tok_pair.size, dtype=np.int64)
    pos[order] = np.arange(tok_pair.size) - first[tok_row[order]]
    back = np.lexsort((pos, tok_pair))                                        # by pair, positions ascending
    pair_off = np.zeros(row_tf.size + 1, dtype=np.int64)
    np.cumsum(row_tf, out=pair_off[1:])
    return pair_off, pos[back].astype(np.uint16)


def model_bytes(index, post, parsed_list):
    """Cost-model bytes of one clause launch: 4 per posting of every clause term; per phrase, 8 + 2 * tf per candidate
    row (the rows that hold every member) and member."""
    post_ptr, post_pos, post_tf = post
    total = verified = 0
    for parsed in parsed_list:
        for kind, toks in parsed.clauses:
            ids = [index.vocab.get(t) for t in toks]
            if any(t is None for t in ids):
                continue
            total += 4 * sum(int(index.df[t]) for t in ids)
            if len(ids) > 1:
                cand = None
                for t in set(ids):
                    rows = post_pos[post_ptr[t]:post_ptr[t + 1]]
                    cand = rows if cand is None else np.intersect1d(cand, rows, assume_unique=True)
                verified += int(cand.size)
                for t in ids:
                    a, b = post_ptr[t], post_ptr[t + 1]
                    tf = post_tf[a:b][np.searchsorted(post_pos[a:b], cand)]
                    total += 8 * int(cand.size) + 2 * int(tf.astype(np.int64).sum())
    return total, verified


def mask_launch(index, parsed_list):
    """The clause launch alone, through the C entry, with the arrays prepared: () -> None."""
    lib = _native.load()
    c_ptr, c_kind, ct_ptr, ct_terms = index.clause_arrays(parsed_list)
    stride = (index.n + 31) // 32 * 4
    out = torch.empty(NQ * stride, dtype=torch.uint8, device=DEV)

    def run():
        rc = lib.crag_bm25_clause_masks_host(
            index.d_post_ptr.data_ptr(), index.d_post_pos.data_ptr(), index.d_post_off.data_ptr(),
            index.d_post_where.data_ptr(), index.n, index.n_terms, c_ptr.ctypes.data, c_kind.ctypes.data, ct_ptr.ctypes.data,
            ct_terms.ctypes.data, len(parsed_list), None, 0, index._slot(0), out.data_ptr(), stride, ctypes.c_void_p(0))
        _native.check(rc, "crag_bm25_clause_masks_host")
    return run, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for n_rows in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(20260 + n_rows % 997)
        row_ptr, row_terms, row_tf, p = zipf_rows(rng, n_rows)
        pair_off, pair_where = synth_positions(rng, row_ptr, row_tf)
        index = Bm25Index.from_arrays(row_ptr, row_terms, row_tf, VOCAB, np.arange(n_rows, dtype=np.int64), DEV,
                                      pair_off=pair_off, pair_where=pair_where)
        post = index.host_csr()
        bags = [sorted(int(t) for t in rng.choice(VOCAB, size=int(rng.integers(4, 13)), p=p)) for _ in range(NQ)]
        floors = rng.integers(0, 20, size=NQ)                       # a frequent term outside the bag
        outside = [next(t for t in range(int(lo), VOCAB) if t not in bag) for bag, lo in zip(bags, floors)]
        text = lambda ts: " ".join(str(t) for t in ts)

        def two_in_front(bag, form):
            """The bag with its two most frequent distinct terms (the lowest ids) in front, as `form` writes them."""
            d = sorted(set(bag))
            a, b = (d[0], d[1]) if len(d) > 1 else (bag[0], bag[1])
            rest = list(bag)
            rest.remove(a)
            rest.remove(b)
            return form.format(a=a, b=b) + " " + text(rest)
        cases = {
            "plain": [text(bag) for bag in bags],
            "required": ["+" + text(bag) for bag in bags],
            "excluded": [text(bag) + f" -{x}" for bag, x in zip(bags, outside)],
            "phrase": [two_in_front(bag, '"{a} {b}"') for bag in bags],
            # the phrase's two terms as required terms: its bitmap phase without compaction and verification
            "two_required": [two_in_front(bag, "+{a} +{b}") for bag in bags],
        }
        want_bag = index.query_terms(cases["plain"])
        ms_plain = None
        for name, queries in cases.items():
            parsed = [parse_query(q) for q in queries]
            got_bag = index.query_terms([" ".join(pq.bag) for pq in parsed])
            assert all(np.array_equal(a, b) for a, b in zip(got_bag, want_bag)), "the cases must score the same bag"
            line = {"bench": "bm25_syntax", "case": name, "rows": n_rows, "nq": NQ, "k": K, "vocab": VOCAB,
                    "nnz": int(row_terms.size), "tokens": int(pair_where.size),
                    "positions_bytes": int(pair_where.size) * 2 + int(row_terms.size + 1) * 8}
            if name == "plain":
                ms_plain = ms = timed(lambda: index.search(queries, K), args.reps)
            else:
                ms = timed(lambda: index.search_query(queries, K), args.reps)
                run, out = mask_launch(index, parsed)
                line["ms_clause_launch_alone"] = round(timed(run, args.reps), 4)
                line["mask_bytes_written"] = int(out.numel())
                line["model_bytes_clause_launch"], line["phrase_candidates_verified"] = model_bytes(index, post, parsed)
                line["rows_passing_mean"] = round(float(np.unpackbits(out.cpu().numpy(), bitorder="little").sum()) / NQ, 1)
                _, _, counts = index.search_query(queries, K)
                line["queries_with_results"] = int((counts > 0).sum())
                line["ms_over_plain"] = round(ms - ms_plain, 4)
            line["ms_per_call"] = round(ms, 4)
            line["scored_postings_bytes"] = int(index.df[want_bag[1]].sum()) * 6
            lines.append(line)
            print(json.dumps(line), flush=True)
        index.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
