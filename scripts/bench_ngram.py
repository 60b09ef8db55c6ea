"""Trigram field of the BM25 lane on a seeded synthetic corpus: what building the postings on the GPU costs against the
host rule, and what a search over the field costs beside the word lane over the same rows.

Rows are 8-24 words drawn from a Zipf(1) vocabulary of 20 000 pronounceable pseudo-words (3-10 letters; every 50th word
carries a 2-, 3- or 4-byte character), joined by spaces.  Queries are 64 strings of 20-60 characters cut from rows, with
one letter in eight replaced (the misspelt query the field exists for).

Line "ngram_build": ms of NgramIndex.from_bytes (upload, extraction kernel, torch.sort, heads, torch.cumsum, emit; HIP
events around the whole build, median of `--build-reps`), the same split into the extraction kernel alone
(crag_ngram_extract, HIP events) and the rest, bytes of text, grams, nnz, V, and the seconds of ngram_csr_host on the
same rows (plain Python: one interpreter thread).
Line "ngram_search": ms per NgramIndex.search_terms call and per Bm25Index.search_terms call for the same 64 queries at
k = 50 (HIP events over `--reps` calls enqueued back to back, median of three), the postings each touches, and the host
preparation (query_terms) of both.

    python scripts/bench_ngram.py [--rows 100000] [--reps 50] [--build-reps 3] [--no-host] [--out profiles/ngram_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cadence_rag_amd import _native  # noqa: E402
from cadence_rag_amd.bm25 import Bm25Index  # noqa: E402
from cadence_rag_amd.ngram import NgramIndex, ngram_csr_host  # noqa: E402

VOCAB = 20_000
NQ, K = 64, 50
DEV = torch.device("cuda", 0)


def pseudo_words(rng):
    cons, vow = "bcdfghjklmnprstvwz", "aeiou"
    wide = ["é", "ü", "ß", "€", "中", "😀"]
    words = []
    for i in range(VOCAB):
        n = int(rng.integers(3, 11))
        w = "".join((cons if j % 2 == 0 else vow)[int(rng.integers(0, 18 if j % 2 == 0 else 5))] for j in range(n))
        if i % 50 == 49:
            w = w[:2] + wide[(i // 50) % len(wide)] + w[2:]
        words.append(w)
    return np.array(words)


def corpus(rng, n_rows):
    words = pseudo_words(rng)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    lens = rng.integers(8, 25, size=n_rows)
    flat = words[np.searchsorted(np.cumsum(p), rng.random(int(lens.sum()))).clip(0, VOCAB - 1)]
    texts, o = [], 0
    for n in lens:
        texts.append(" ".join(flat[o:o + n]))
        o += n
    return texts


def noisy_queries(rng, texts):
    out = []
    for _ in range(NQ):
        t = texts[int(rng.integers(0, len(texts)))]
        n = int(rng.integers(20, 61))
        a = int(rng.integers(0, max(len(t) - n, 1)))
        chars = list(t[a:a + n])
        for i in range(len(chars)):
            if chars[i] != " " and rng.random() < 0.125:
                chars[i] = "aeioubcdfg"[int(rng.integers(0, 10))]
        out.append("".join(chars))
    return out


def events(fn, reps):
    """ms per call: `reps` calls between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return float(np.median([events(fn, reps) for _ in range(3)]))


def extract_alone(index, reps):
    """The extraction kernel's share: crag_ngram_extract over the index's text (with its pointer check and memsets)."""
    lib = _native.load()
    n, n_bytes = len(index), int(index.text.size)
    text, ptr = torch.from_numpy(index.text).to(DEV), torch.from_numpy(index.text_ptr).to(DEV)
    keys, rows = torch.empty(n_bytes, dtype=torch.int64, device=DEV), torch.empty(n_bytes, dtype=torch.int32, device=DEV)
    dl = torch.empty(n, dtype=torch.int32, device=DEV)
    scratch = torch.empty(int(lib.crag_ngram_scratch_bytes(n_bytes, n)) // 8, dtype=torch.int64, device=DEV)

    def run():
        _native.check(lib.crag_ngram_extract(text.data_ptr(), n_bytes, ptr.data_ptr(), n, keys.data_ptr(), rows.data_ptr(),
                                             dl.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, None), "extract")
    return timed(run, reps)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--build-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rng = np.random.default_rng(20261)
    texts = corpus(rng, args.rows)
    rows_bytes = [t.encode() for t in texts]
    ids = np.arange(args.rows, dtype=np.int64)
    queries = noisy_queries(rng, texts)

    NgramIndex.from_bytes(rows_bytes[:1000], ids[:1000], DEV).close()        # (library load, allocator warm-up)
    build_ms = []
    index = None
    for _ in range(args.build_reps):
        if index is not None:
            index.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = NgramIndex.from_bytes(rows_bytes, ids, DEV)
        torch.cuda.synchronize()
        build_ms.append((time.perf_counter() - t0) * 1e3)
    device_ms = []
    for _ in range(args.build_reps):                                          # the device's share: no joining of rows
        torch.cuda.synchronize()
        device_ms.append(events(index._build, 1))
    line = {"bench": "ngram_build", "rows": args.rows, "text_bytes": int(index.text.size), "grams": index.n_grams,
            "nnz": index.nnz, "n_terms": index.n_terms, "avgdl": round(index.avgdl, 2),
            "ms_from_bytes_wall": round(float(np.median(build_ms)), 2),
            "ms_build_device_events": round(float(np.median(device_ms)), 2),
            "ms_extract_call": round(extract_alone(index, 10), 4)}
    line["text_GBps_extract"] = round(line["text_bytes"] / line["ms_extract_call"] / 1e6, 1)
    if not args.no_host:
        t0 = time.perf_counter()
        want = ngram_csr_host(rows_bytes)
        line["host_rule_s"] = round(time.perf_counter() - t0, 2)
        post_ptr, post_pos, post_tf = index.host_csr()
        line["equal_to_host_rule"] = bool(
            np.array_equal(index.keys, want["keys"]) and np.array_equal(post_ptr, want["post_ptr"])
            and np.array_equal(post_pos, want["post_pos"]) and np.array_equal(post_tf, want["post_tf"])
            and np.array_equal(index.doc_len, want["doc_len"]))
    lines = [line]
    print(json.dumps(line), flush=True)

    words = Bm25Index(texts, ids, DEV)
    g_terms, w_terms = index.query_terms(queries), words.query_terms(queries)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        index.query_terms(queries)
    g_prep = (time.perf_counter() - t0) / args.reps * 1e3
    t0 = time.perf_counter()
    for _ in range(args.reps):
        words.query_terms(queries)
    w_prep = (time.perf_counter() - t0) / args.reps * 1e3
    line = {"bench": "ngram_search", "rows": args.rows, "nq": NQ, "k": K,
            "ngram_query_terms": int(g_terms[1].size), "ngram_postings": int(index.df[g_terms[1]].sum()),
            "ngram_ms_prepared_terms": round(timed(lambda: index.search_terms(*g_terms, K), args.reps), 4),
            "ngram_ms_host_query_terms": round(g_prep, 4),
            "ngram_queries_with_hits": int((index.search_terms(*g_terms, K)[2] > 0).sum()),
            "word_query_terms": int(w_terms[1].size), "word_postings": int(words.df[w_terms[1]].sum()),
            "word_ms_prepared_terms": round(timed(lambda: words.search_terms(*w_terms, K), args.reps), 4),
            "word_ms_host_query_terms": round(w_prep, 4),
            "word_queries_with_hits": int((words.search_terms(*w_terms, K)[2] > 0).sum())}
    lines.append(line)
    print(json.dumps(line), flush=True)
    index.close()
    words.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.writelines(json.dumps(entry) + "\n" for entry in lines)


if __name__ == "__main__":
    main()
