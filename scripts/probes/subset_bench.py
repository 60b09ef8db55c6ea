"""The search over listed rows against the masked search it equals: per size (100 000 and 1 000 000
rows over about 20 000 calls), batch (1 and 64 queries, each with its own list) and listed count (64, 500, 2000, 4096:
whole calls drawn at random until the count is reached), k = 50, the stream time of
  * DenseIndex.search_ids_async over the lists (two launches), and
  * DenseIndex.search_async under the equivalent per-query masks (the route every scoped search took before),
HIP events on one stream around `--iters` calls back to back after `--warmup` calls, the two routes alternating
`--blocks` times; the median block and the spread (min, max) are kept.  Both routes must return the same ids, score bits
and counts before anything is timed.  The floor quoted is (listed rows x 4 KiB) / 8 TB/s per query -- lists this small
are latency-bound and partly cache-resident (the repeats re-read the same rows), not HBM-bound: the floor says how far
from the bytes the time is, not what is reachable.  Appends one JSON line per (rows, nq, count) to
profiles/subset_bench.jsonl.

  python scripts/probes/subset_bench.py [--rows 100000 1000000] [--calls 20000] [--iters 200] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402

HBM_TBPS = 8.0
K = 50


def build_index(n, dev):
    ix = DenseIndex(1024, capacity=n, device=dev.index)
    step = 65536
    for lo in range(0, n, step):
        m = min(step, n - lo)
        ix.add(torch.randn(m, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(lo + 1)),
               ids=np.arange(lo, lo + m, dtype=np.int64) * 2 + 7)
    return ix


def scoped_positions(rows_of_call, count, rng):
    """positions of whole calls drawn at random until `count` rows are listed (cut at the count)"""
    pos, have = [], 0
    for c in rng.permutation(len(rows_of_call)):
        pos.append(rows_of_call[int(c)])
        have += pos[-1].size
        if have >= count:
            break
    return np.sort(np.concatenate(pos)[:count])


def timed(fn, stream, warmup, iters):
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            fn()
        b.record(stream)
        b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--counts", type=int, nargs="+", default=[64, 500, 2000, 4096])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "subset_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    for n in args.rows:
        ix = build_index(n, dev)
        try:
            call_of = rng.integers(0, args.calls, n)
            order = np.argsort(call_of, kind="stable")
            rows_of_call = np.split(order, np.cumsum(np.bincount(call_of, minlength=args.calls))[:-1])
            stride = ((n + 31) // 32) * 4
            for nq in args.queries:
                d_q = torch.randn(nq, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
                for count in args.counts:
                    pos = [scoped_positions(rows_of_call, count, rng) for _ in range(nq)]
                    h_ids = np.stack([p * 2 + 7 for p in pos]).astype(np.int64)
                    mask = np.zeros((nq, n), dtype=bool)
                    for q, p in enumerate(pos):
                        mask[q, p] = True
                    d_ids = torch.from_numpy(h_ids).to(dev)
                    d_ct = torch.full((nq,), count, dtype=torch.int32, device=dev)
                    d_mask = torch.from_numpy(DenseIndex.pack_mask(mask)).to(dev)
                    assert d_mask.shape == (nq, stride)
                    scratch = torch.empty(DenseIndex.search_ids_scratch_bytes(nq, count), dtype=torch.uint8, device=dev)
                    outs = [[torch.empty(nq, K, dtype=torch.int64, device=dev), torch.empty(nq, K, dtype=torch.float32, device=dev),
                             torch.empty(nq, dtype=torch.int32, device=dev)] for _ in range(2)]

                    def listed():
                        ix.search_ids_async(d_q, d_ids, d_ct, K, *outs[0], scratch=scratch, stream=st)

                    def masked():
                        ix.search_async(d_q, K, *outs[1], d_row_mask=d_mask, mask_stride=stride, stream=st)

                    with torch.cuda.stream(stream):
                        listed()
                        masked()
                    stream.synchronize()
                    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2]), "ids differ"
                    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), "score bits differ"
                    t = {"listed": [], "masked": []}
                    for _ in range(args.blocks):
                        t["listed"].append(timed(listed, stream, args.warmup, args.iters))
                        t["masked"].append(timed(masked, stream, args.warmup, args.iters))
                    rec = {"rows": n, "calls": args.calls, "nq": nq, "count": count, "k": K, "warmup": args.warmup,
                           "iters": args.iters, "blocks": args.blocks,
                           "floor_us": round(nq * count * 4096 / (HBM_TBPS * 1e12) * 1e6, 3), "floor_tbps": HBM_TBPS}
                    for name, v in t.items():
                        rec[f"{name}_us"] = round(float(np.median(v)), 2)
                        rec[f"{name}_us_min_max"] = [round(float(min(v)), 2), round(float(max(v)), 2)]
                    rec["masked_over_listed"] = round(rec["masked_us"] / rec["listed_us"], 2)
                    print(json.dumps(rec), flush=True)
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps(rec) + "\n")
        finally:
            ix.close()


if __name__ == "__main__":
    main()
