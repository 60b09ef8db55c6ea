"""Kernel time of crag_index_dedupe_async (64 queries x width 150 and x 256 over a 100 000-row index) and the
HybridSearcher step with and without dedupe_cosine: HIP events on one stream, warm.  Prints one JSON line.

  python scripts/probes/dedupe_time.py [--rows 100000] [--nq 64] [--iters 200]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402
from cadence_rag_amd.fusion import HybridSearcher  # noqa: E402

SCAN_TBPS = 6.8   # what the scan reaches: the bandwidth the byte floor is taken at


def timed(fn, iters, stream):
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    # clusters of 8 near-duplicates, as overlapping transcript chunks give
    base = rng.standard_normal((args.rows // 8 + 1, 1024), dtype=np.float32)
    rows = np.repeat(base, 8, axis=0)[:args.rows] + 0.15 * rng.standard_normal((args.rows, 1024), dtype=np.float32) / 32
    out = {"rows": args.rows, "nq": args.nq}
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    with DenseIndex(1024, capacity=args.rows, device=0) as ix, torch.cuda.stream(stream):
        ix.add(rows)
        for width in (150, 256):
            ids = np.stack([rng.choice(args.rows, size=width, replace=False) for _ in range(args.nq)]).astype(np.int64)
            d_ids = torch.from_numpy(ids).to(dev)
            d_ct = torch.full((args.nq,), width, dtype=torch.int32, device=dev)
            o_ids, o_ct = torch.empty_like(d_ids), torch.empty_like(d_ct)
            o_dup = torch.empty(args.nq, width, dtype=torch.int32, device=dev)
            o_sim = torch.empty(args.nq, width, dtype=torch.float32, device=dev)
            us = timed(lambda: ix.dedupe_async(d_ids, d_ct, 0.9, o_ids, o_ct, o_dup, o_sim, stream=st), args.iters, stream)
            nbytes = args.nq * width * (4096 + 8 + 8 + 4 + 4)
            floor_us = nbytes / (SCAN_TBPS * 1e12) * 1e6
            out[f"dedupe_w{width}_us"] = round(us, 2)
            out[f"dedupe_w{width}_bytes"] = nbytes
            out[f"dedupe_w{width}_floor_us"] = round(floor_us, 2)
            out[f"dedupe_w{width}_fraction_of_floor"] = round(floor_us / us, 4)
        # the hybrid step: dense top-100 + a given 50-wide lexical lane -> fused width 150
        qv = torch.from_numpy(rows[rng.choice(args.rows, size=args.nq, replace=False)]).to(dev)
        bm = torch.from_numpy(np.stack([rng.choice(args.rows, size=50, replace=False) for _ in range(args.nq)]).astype(np.int64)).to(dev)
        bm_ct = torch.full((args.nq,), 50, dtype=torch.int32, device=dev)
        for name, kw in (("hybrid_step_us", {}), ("hybrid_step_dedupe_us", {"dedupe_cosine": 0.9})):
            hs = HybridSearcher(ix, None, dense_k=100, **kw)
            out[name] = round(timed(lambda: hs.search(qv, bm25=(bm, bm_ct), stream=st), args.iters, stream), 2)
        res = hs.search(qv, bm25=(bm, bm_ct), stream=st)
        stream.synchronize()
        out["hybrid_mean_kept_of_150"] = round(float(res["counts"].float().mean()), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
