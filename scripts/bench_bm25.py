"""BM25 lane throughput on a synthetic Zipf corpus (seeded): rows x 64 queries of 4-12 terms, k = 50.

One JSON line per corpus size: ms per Bm25Index.search call (host share included: tokenising the queries, the weights,
one upload), ms per call with the term ids and weights prepared (`search_terms`: the upload and the two kernels -- the
roofline figures use this one), the bytes of postings the call touches (6 per posting of every query term), the doc_len gathers (4 per
posting) and the partial lists, the fraction of the 8 TB/s HBM peak those bytes per second are, and the time of the same
job on the host (scipy.sparse when installed, else numpy; 16 threads over the queries).  A second line per size times
one HybridSearcher step (dense top-50 + BM25 top-50 -> RRF) with the native lane and the same step fed ready-made BM25
ids: the difference is what the lane costs inside a real step.

    python scripts/bench_bm25.py [--rows 100000,1000000] [--reps 50] [--no-hybrid] [--out profiles/bm25_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from cadence_rag_amd.bm25 import B, K1, RANGE_ROWS, Bm25Index  # noqa: E402
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402
from cadence_rag_amd.fusion import HybridSearcher  # noqa: E402

HBM_PEAK = 8.0e12
VOCAB = 50_000
NQ, K = 64, 50
DEV = torch.device("cuda", 0)


def zipf_rows(rng, n_rows: int):
    """Rows of 10-50 tokens drawn from a Zipf(1) vocabulary, as (row_ptr, row_terms, row_tf)."""
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    lens = rng.integers(10, 51, size=n_rows)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    terms = np.searchsorted(np.cumsum(p), rng.random(rows.size)).clip(0, VOCAB - 1)
    pairs, tf = np.unique(rows * VOCAB + terms, return_counts=True)       # sorted by row, then term
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs // VOCAB, minlength=n_rows), out=row_ptr[1:])
    return row_ptr, (pairs % VOCAB).astype(np.int32), tf, p


def host_job(index: Bm25Index, queries):
    """The same job on the host: per query the contributions of its terms' postings added into a dense fp32 vector,
    then the k best by (-score, position)."""
    post_ptr, post_pos, post_tf = index.host_csr()
    norm = (K1 * (1.0 - B + B * index.doc_len / np.float32(index.avgdl))).astype(np.float32)
    q_ptr, terms, w = index.query_terms(queries)
    try:
        import scipy.sparse as sp
        how = "scipy.sparse"
        tfm = sp.csc_matrix((post_tf.astype(np.float32), post_pos, post_ptr), shape=(index.n, index.n_terms))
    except ImportError:
        how, tfm = "numpy", None

    def one(q):
        acc = np.zeros(index.n, dtype=np.float32)
        for i in range(q_ptr[q], q_ptr[q + 1]):
            t = terms[i]
            if tfm is not None:
                col = tfm.getcol(int(t))
                pos, tf = col.indices, col.data
            else:
                pos = post_pos[post_ptr[t]:post_ptr[t + 1]]
                tf = post_tf[post_ptr[t]:post_ptr[t + 1]].astype(np.float32)
            acc[pos] += w[i] * tf / (tf + norm[pos])
        top = np.argpartition(-acc, K)[:K]
        return top[np.lexsort((top, -acc[top]))]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(len(queries))))
    return how, (time.perf_counter() - t0) * 1e3


def timed(fn, reps: int) -> float:
    """ms per call: `reps` calls enqueued back to back between two events (three rounds, the median)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-hybrid", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for n_rows in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(20260 + n_rows % 997)
        row_ptr, row_terms, row_tf, p = zipf_rows(rng, n_rows)
        index = Bm25Index.from_arrays(row_ptr, row_terms, row_tf, VOCAB, np.arange(n_rows, dtype=np.int64), DEV)
        queries = [" ".join(str(t) for t in rng.choice(VOCAB, size=int(rng.integers(4, 13)), p=p)) for _ in range(NQ)]
        ms_call = timed(lambda: index.search(queries, K), args.reps)
        q_ptr, terms, weights = index.query_terms(queries)
        ms = timed(lambda: index.search_terms(q_ptr, terms, weights, K), args.reps)    # the device's share
        t0 = time.perf_counter()
        for _ in range(args.reps):
            index.query_terms(queries)
        ms_prepare = (time.perf_counter() - t0) / args.reps * 1e3
        postings = int(index.df[terms].sum())
        n_ranges = -(-n_rows // RANGE_ROWS)
        partial = 2 * (NQ * n_ranges * (K * 8 + 4))          # written by the ranges, read by the merge (upper bound)
        total = postings * 6 + postings * 4 + partial
        line = {"bench": "bm25_lane", "rows": n_rows, "nq": NQ, "k": K, "vocab": VOCAB, "nnz": int(row_terms.size),
                "query_terms": int(terms.size), "postings": postings, "ms_per_call": round(ms_call, 4),
                "ms_prepared_terms": round(ms, 4), "ms_host_query_terms": round(ms_prepare, 4),
                "postings_bytes": postings * 6, "doc_len_gather_bytes": postings * 4, "partial_list_bytes": partial,
                "bytes_per_call": total, "GBps": round(total / ms / 1e6, 1),
                "hbm_fraction": round(total / (ms * 1e-3) / HBM_PEAK, 4),
                "hbm_fraction_postings_only": round(postings * 6 / (ms * 1e-3) / HBM_PEAK, 4)}
        if not args.no_host:
            how, host_ms = host_job(index, queries)
            line["host_backend"], line["host_ms_per_call"] = how + ", 16 threads", round(host_ms, 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
        if not args.no_hybrid:
            g = torch.Generator(device=DEV).manual_seed(1234)
            dense = DenseIndex(1024, capacity=n_rows)
            for lo in range(0, n_rows, 100_000):
                m = min(100_000, n_rows - lo)
                dense.add(torch.randn(m, 1024, generator=g, device=DEV),
                          torch.arange(lo, lo + m, dtype=torch.int64, device=DEV))
            qv = torch.randn(NQ, 1024, generator=g, device=DEV)
            native = HybridSearcher(dense, None, dense_k=50, bm25_index=index, bm25_k=K)
            fed = HybridSearcher(dense, None, dense_k=50)
            ids, _, counts = index.search(queries, K)
            ready = (ids.clone(), counts.clone())
            ms_fed = timed(lambda: fed.search(qv, bm25=ready), args.reps)
            ms_native = timed(lambda: native.search(qv, query_texts=queries), args.reps)
            ms_fed2 = timed(lambda: fed.search(qv, bm25=ready), args.reps)
            line = {"bench": "hybrid_step_dense50_bm25", "rows": n_rows, "nq": NQ, "k": K,
                    "ms_native_bm25_lane": round(ms_native, 4), "ms_ready_made_ids": round(min(ms_fed, ms_fed2), 4),
                    "ms_ready_made_ids_runs": [round(ms_fed, 4), round(ms_fed2, 4)],
                    "lane_cost_ms": round(ms_native - min(ms_fed, ms_fed2), 4)}
            lines.append(line)
            print(json.dumps(line), flush=True)
            dense.close()
        index.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
