"""What prefix and fuzzy items of the BM25 lane cost.

Part 1, the expansion alone: seeded vocabularies of 50 000 and 1 000 000 words (3-12 letters a-z, df 0-4), and 1, 8 and
64 patterns of each kind (prefix: the first three letters of a vocabulary word; fuzzy: a vocabulary word with one or two
letters replaced).  Per case one JSON line: ms of crag_bm25_expand_host alone (HIP events around `reps` back-to-back calls
of the C entry with prepared arrays, the median of three rounds), wall ms of Bm25Index.expand (launches, the stream
synchronisation and the read-back), wall ms of the same rule on the host (numpy over a padded code-point matrix, once),
and the cost-model bytes: the dictionary once per call (8 per term of term_ptr, the terms' bytes, 8 per term of post_ptr
for the matches' df is an upper bound: 16 per term + bytes) plus the per-slice lists written and read (2 * 520 bytes per
slice and pattern).

Part 2, the query: the Zipf corpus of scripts/bench_bm25_syntax.py (decimal vocabulary), 64 queries, k = 50: `search`,
`search_query(expand=True)` without an operator (the same calls), with one optional prefix item per query (`12*`), with
one required fuzzy item (`+1234~`).

    python scripts/bench_bm25_expand.py [--vocab 50000,1000000] [--rows 100000] [--reps 20] [--out profiles/bm25_expand_bench.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_bm25 import DEV, K, NQ, VOCAB, timed, zipf_rows  # noqa: E402
from cadence_rag_amd import _native  # noqa: E402
from cadence_rag_amd.bm25 import BM25_EXPAND_SLICE, FUZZY1, FUZZY2, MAX_EXPANSIONS, PREFIX, Bm25Index  # noqa: E402

KIND_NAME = {PREFIX: "prefix", FUZZY1: "fuzzy1", FUZZY2: "fuzzy2"}


def seeded_vocabulary(rng, v):
    """v distinct words of 3-12 letters."""
    words, seen = [], set()
    while len(words) < v:
        lens = rng.integers(3, 13, size=v)
        letters = rng.integers(97, 123, size=int(lens.sum()), dtype=np.uint8).tobytes().decode("ascii")
        at = 0
        for n in lens.tolist():
            w = letters[at:at + n]
            at += n
            if w not in seen:
                seen.add(w)
                words.append(w)
                if len(words) == v:
                    break
    return words


def vocabulary_index(rng, words):
    """An index whose term t is words[t] with df in 0 .. 4 (term t is held by the rows below df[t])."""
    df = rng.integers(0, 5, size=len(words))
    per_row = [np.flatnonzero(df > r).astype(np.int32) for r in range(4)]
    row_ptr = np.zeros(5, dtype=np.int64)
    np.cumsum([r.size for r in per_row], out=row_ptr[1:])
    row_terms = np.concatenate(per_row)
    return Bm25Index.from_arrays(row_ptr, row_terms, np.ones(row_terms.size, dtype=np.int64), len(words),
                                 np.arange(4, dtype=np.int64), DEV, vocab={w: i for i, w in enumerate(words)})


def make_patterns(rng, words, kind, count):
    out = []
    for w in (words[int(i)] for i in rng.integers(0, len(words), size=count)):
        if kind == PREFIX:
            out.append((kind, w[:3]))
        else:
            chars = list(w)
            for at in rng.choice(len(chars), size=min(kind, len(chars)), replace=False):
                chars[int(at)] = chr(int(rng.integers(97, 123)))
            out.append((kind, "".join(chars)))
    return out


class HostRule:
    """The rule in numpy: the vocabulary as a padded matrix of code points, one banded recurrence over all terms."""

    def __init__(self, words, df):
        self.len = np.fromiter(map(len, words), dtype=np.int32, count=len(words))
        self.width = int(self.len.max())
        self.mat = np.zeros((len(words), self.width + 1), dtype=np.uint32)
        for w in range(1, self.width + 1):
            rows = np.flatnonzero(self.len >= w)
            self.mat[rows, w - 1] = np.fromiter((ord(words[r][w - 1]) for r in rows), dtype=np.uint32, count=rows.size)
        self.df = np.asarray(df, dtype=np.int64)

    def kept(self, kind, pattern):
        pat = np.fromiter(map(ord, pattern), dtype=np.uint32, count=len(pattern))
        m = pat.size
        if kind == PREFIX:
            cand = np.flatnonzero(self.len >= m)
            cand = cand[np.all(self.mat[cand, :m] == pat, axis=1)] if m <= self.width else cand[:0]
            dist = np.zeros(cand.size, dtype=np.int64)
        else:
            cand = np.flatnonzero(np.abs(self.len - m) <= kind)
            sub, n = self.mat[cand], self.len[cand]
            prev = np.tile(np.arange(m + 1, dtype=np.int64), (cand.size, 1))
            final = prev[:, m].copy()
            final[n != 0] = 1 << 20
            for i in range(1, min(self.width, m + kind) + 1):
                cur = np.empty_like(prev)
                cur[:, 0] = i
                cost = (sub[:, i - 1:i] != pat[None, :]).astype(np.int64)
                for j in range(1, m + 1):
                    cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + cost[:, j - 1])
                final = np.where(n == i, cur[:, m], final)
                prev = cur
            ok = final <= kind
            cand, dist = cand[ok], final[ok]
        order = np.lexsort((cand, -self.df[cand], dist))[:MAX_EXPANSIONS]
        return cand[order], dist[order], int(cand.size)


def entry_alone(index, patterns):
    """crag_bm25_expand_host with prepared arrays: () -> None."""
    lib = _native.load()
    enc = [tok.encode("utf-8") for _, tok in patterns]
    npat = len(patterns)
    pat_ptr = np.zeros(npat + 1, dtype=np.int32)
    np.cumsum([len(e) for e in enc], out=pat_ptr[1:])
    pat_bytes = np.frombuffer(b"".join(enc), dtype=np.uint8)
    pat_kind = np.asarray([k for k, _ in patterns], dtype=np.int32)
    d_term_ptr, d_term_bytes = index._device_dictionary()
    need = int(lib.crag_bm25_expand_scratch_bytes(index.n_terms, npat))
    scratch = torch.empty(max(need // 8, 1), dtype=torch.int64, device=DEV)
    terms = torch.empty(npat * MAX_EXPANSIONS, dtype=torch.int32, device=DEV)
    dist = torch.empty_like(terms)
    kept = torch.empty(npat, dtype=torch.int32, device=DEV)
    total = torch.empty(npat, dtype=torch.int64, device=DEV)

    def run():
        rc = lib.crag_bm25_expand_host(d_term_ptr.data_ptr(), d_term_bytes.data_ptr(), index.d_post_ptr.data_ptr(),
                                       index.n_terms, pat_ptr.ctypes.data, pat_bytes.ctypes.data, pat_kind.ctypes.data, npat,
                                       index._slot(0), scratch.data_ptr(), scratch.numel() * 8, terms.data_ptr(),
                                       dist.data_ptr(), kept.data_ptr(), total.data_ptr(), ctypes.c_void_p(0))
        _native.check(rc, "crag_bm25_expand_host")
    return run, int(d_term_bytes.numel())


def wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", default="50000,1000000")
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    for v in (int(x) for x in args.vocab.split(",")):
        rng = np.random.default_rng(4700 + v % 991)
        words = seeded_vocabulary(rng, v)
        index = vocabulary_index(rng, words)
        host = HostRule(words, index.df)
        n_slices = (v + BM25_EXPAND_SLICE - 1) // BM25_EXPAND_SLICE
        for kind in (PREFIX, FUZZY1, FUZZY2):
            for count in (1, 8, 64):
                patterns = make_patterns(rng, words, kind, count)
                run, dict_bytes = entry_alone(index, patterns)
                got = index.expand(patterns)
                t0 = time.perf_counter()
                want = [host.kept(k, tok) for k, tok in patterns]
                host_ms = (time.perf_counter() - t0) * 1e3
                for (gi, gd, gt), (wi, wd, wt) in zip(got, want):
                    assert gi.tolist() == wi.tolist() and gd.tolist() == wd.tolist() and gt == wt, "device != host rule"
                model = 16 * (v + 1) + dict_bytes + 2 * n_slices * count * (MAX_EXPANSIONS * 8 + 4)
                ms = timed(run, args.reps)
                emit({"bench": "bm25_expand", "vocab": v, "kind": KIND_NAME[kind], "patterns": count,
                      "ms_entry_alone": round(ms, 4), "ms_expand_wall": round(wall_ms(lambda: index.expand(patterns), args.reps), 4),
                      "ms_host_numpy": round(host_ms, 2), "dictionary_bytes": dict_bytes, "model_bytes": model,
                      "model_gb_per_s": round(model / ms / 1e6, 1), "matches_total": int(sum(t for _, _, t in got)),
                      "kept_total": int(sum(len(i) for i, _, _ in got))})
        index.close()

    rng = np.random.default_rng(20260 + args.rows % 997)
    row_ptr, row_terms, row_tf, p = zipf_rows(rng, args.rows)
    index = Bm25Index.from_arrays(row_ptr, row_terms, row_tf, VOCAB, np.arange(args.rows, dtype=np.int64), DEV)
    bags = [sorted(int(t) for t in rng.choice(VOCAB, size=int(rng.integers(4, 13)), p=p)) for _ in range(NQ)]
    plain = [" ".join(str(t) for t in bag) for bag in bags]
    cases = {"search": lambda: index.search(plain, K),
             "search_query_expand_no_operator": lambda: index.search_query(plain, K, expand=True),
             "optional_prefix_item": lambda: index.search_query([f"{q} {100 + i}*" for i, q in enumerate(plain)], K, expand=True),
             "required_fuzzy_item": lambda: index.search_query([f"{q} +{1000 + 7 * i}~" for i, q in enumerate(plain)], K,
                                                               expand=True)}
    for name, fn in cases.items():
        emit({"bench": "bm25_expand_query", "case": name, "rows": args.rows, "nq": NQ, "k": K, "vocab": VOCAB,
              "ms_per_call_events": round(timed(fn, args.reps), 4), "ms_per_call_wall": round(wall_ms(fn, args.reps), 4)})
    index.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
