"""Time of crag_index_mmr_async -- both launches, the Gram kernel and the walk -- for 64 queries x (width 64, k 12),
(150, 12) and (256, 50) over a 100 000-row index, with the dedupe kernel at the same widths beside it: HIP events on one
stream, warm.  The same call with k = 1 is printed too: one pick, so all but the Gram launch's share is gone.  Prints one
JSON line.

  python scripts/probes/mmr_time.py [--rows 100000] [--nq 64] [--iters 200]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402


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
        for width, k in ((64, 12), (150, 12), (256, 50)):
            ids = np.stack([rng.choice(args.rows, size=width, replace=False) for _ in range(args.nq)]).astype(np.int64)
            d_ids = torch.from_numpy(ids).to(dev)
            d_rel = torch.from_numpy(np.sort(rng.uniform(0.2, 0.9, size=(args.nq, width)).astype(np.float32))[:, ::-1].copy()).to(dev)
            d_ct = torch.full((args.nq,), width, dtype=torch.int32, device=dev)
            for kk, tag in ((k, f"mmr_w{width}_k{k}"), (1, f"mmr_w{width}_k1")):
                o_ids = torch.empty(args.nq, kk, dtype=torch.int64, device=dev)
                o_rel = torch.empty(args.nq, kk, dtype=torch.float32, device=dev)
                o_ct = torch.empty(args.nq, dtype=torch.int32, device=dev)
                out[tag + "_us"] = round(timed(lambda: ix.mmr_async(d_ids, d_rel, d_ct, 0.5, kk, o_ids, o_rel, o_ct, stream=st),
                                               args.iters, stream), 2)
            out[f"mmr_w{width}_scratch_bytes"] = DenseIndex.mmr_scratch_bytes(args.nq, width)
            out[f"mmr_w{width}_row_bytes"] = args.nq * width * 4096
            x_ids, x_ct = torch.empty_like(d_ids), torch.empty_like(d_ct)
            out[f"dedupe_w{width}_us"] = round(timed(lambda: ix.dedupe_async(d_ids, d_ct, 0.9, x_ids, x_ct, stream=st),
                                                     args.iters, stream), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
