"""The grouped search against the plain search of the same index: 100 000 x 1024 rows in 2 000 groups
dealt out at random, per_group = 2, k = 50, for 1 and 64 queries -- the stream time per call of
  * DenseIndex.search_grouped_async (three launches: clear + 1/||q||, score, select), and
  * DenseIndex.search_async with k = 50 on the same index in the same process (the comparator: the mirror scan),
HIP events on one stream around `--iters` calls back to back after `--warmup` calls, the two alternating `--blocks` times;
the median block and the spread (min, max) are kept.  Before anything is timed the grouped result is checked against a
walk over the plain search's top-128 where that walk ends inside the list.  Appends one JSON line per batch size to
profiles/grouped_search.jsonl.

  python scripts/probes/grouped_search.py [--rows 100000] [--groups 2000] [--per-group 2] [--iters 200] [--out FILE]"""
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

K = 50


def build_index(n, dev):
    ix = DenseIndex(1024, capacity=n, device=dev.index)
    step = 65536
    for lo in range(0, n, step):
        m = min(step, n - lo)
        ix.add(torch.randn(m, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(lo + 1)),
               ids=np.arange(lo, lo + m, dtype=np.int64) * 2 + 7)
    return ix


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


def walk(ids, counts, group_of_id, k, per_group):
    """the capped walk over a plain ranking; None where it does not end inside the list"""
    out = []
    for q in range(ids.shape[0]):
        kept, held = [], {}
        for rid in ids[q, :counts[q]].tolist():
            g = group_of_id(rid)
            if held.get(g, 0) < per_group:
                held[g] = held.get(g, 0) + 1
                kept.append(rid)
                if len(kept) == k:
                    break
        out.append(kept if len(kept) == k else None)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--groups", type=int, default=2000)
    ap.add_argument("--per-group", type=int, default=2)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grouped_search.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, n_groups, per = args.rows, args.groups, args.per_group
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    group_of = np.random.default_rng(11).integers(0, n_groups, n).astype(np.int32)
    d_group = torch.from_numpy(group_of).to(dev)
    ix = build_index(n, dev)
    try:
        for nq in args.queries:
            d_q = torch.randn(nq, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
            scratch = torch.empty(DenseIndex.search_grouped_scratch_bytes(nq, n_groups, per), dtype=torch.uint8, device=dev)
            g_out = [torch.empty(nq, K, dtype=torch.int64, device=dev), torch.empty(nq, K, dtype=torch.float32, device=dev),
                     torch.empty(nq, dtype=torch.int32, device=dev)]
            p_out = [torch.empty(nq, K, dtype=torch.int64, device=dev), torch.empty(nq, K, dtype=torch.float32, device=dev),
                     torch.empty(nq, dtype=torch.int32, device=dev)]
            wide = [torch.empty(nq, 128, dtype=torch.int64, device=dev), torch.empty(nq, 128, dtype=torch.float32, device=dev),
                    torch.empty(nq, dtype=torch.int32, device=dev)]

            def grouped():
                ix.search_grouped_async(d_q, K, d_group, n_groups, per, *g_out, scratch=scratch, stream=st)

            def plain():
                ix.search_async(d_q, K, *p_out, stream=st)

            with torch.cuda.stream(stream):
                grouped()
                ix.search_async(d_q, 128, *wide, stream=st)
            stream.synchronize()
            want = walk(wide[0].cpu().numpy(), wide[2].cpu().numpy(), lambda rid: int(group_of[(rid - 7) // 2]), K, per)
            got = g_out[0].cpu().numpy()
            checked = 0
            for q, w in enumerate(want):
                if w is not None:
                    assert got[q].tolist() == w, f"query {q}: the grouped result differs from the walk over the top-128"
                    checked += 1
            t = {"grouped": [], "plain": []}
            for _ in range(args.blocks):
                t["grouped"].append(timed(grouped, stream, args.warmup, args.iters))
                t["plain"].append(timed(plain, stream, args.warmup, args.iters))
            rec = {"rows": n, "n_groups": n_groups, "per_group": per, "nq": nq, "k": K, "warmup": args.warmup,
                   "iters": args.iters, "blocks": args.blocks, "queries_checked": checked,
                   "plain_kernel": ix.last_scan_kernel()}
            for name, v in t.items():
                rec[f"{name}_us"] = round(float(np.median(v)), 2)
                rec[f"{name}_us_min_max"] = [round(float(min(v)), 2), round(float(max(v)), 2)]
            rec["grouped_over_plain"] = round(rec["grouped_us"] / rec["plain_us"], 2)
            print(json.dumps(rec), flush=True)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    finally:
        ix.close()


if __name__ == "__main__":
    main()
