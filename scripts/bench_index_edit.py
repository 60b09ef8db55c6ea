"""In-place index edits (crag_index_remove / crag_index_insert) against the routes they replace, on one MI355X.

For 100 000 and 1 000 000 rows x 1024 (seeded, generated on the device), four edits:
  remove_1pct_scattered   1 % of the rows, spread over the table: nearly every row moves down
  remove_1pct_tail        the last 1 % of the rows: nothing moves, the tail is cleared
  remove_1000_near_end    1 000 rows that start 10 000 rows in front of the end: 9 000 rows move, whatever the table
  insert_1pct_scattered   1 % new rows with ids spread through the range: nearly every row moves up
One JSON line per size and edit: wall ms of the edit (device synchronised around the call; a fresh index per trial,
the median of --trials), the rows that moved, the bytes the move had to touch -- moved rows x (6 156 B read + 6 156 B
written), twice: into the bounce buffer and out of it --, the fraction of the 8 TB/s HBM peak that is, and the wall
ms of the route the edit replaces:
  insert: DenseTable._rebuild(order=, extra=) as it stood before the in-place insert -- read every row out, concatenate
          the new ones, permute with a torch gather, add everything to a second index;
  remove: there was none; "reload the remaining rows into a new index with add" (read out, gather the kept rows, add).

    python scripts/bench_index_edit.py [--rows 100000,1000000] [--trials 3] [--out profiles/index_edit_bench.jsonl]
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

from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402

HBM_PEAK = 8.0e12
ROW_BYTES = 4096 + 2048 + 4 + 8      # fp32 row + fp16 mirror + 1/||row|| + id
DEV = torch.device("cuda", 0)
STEP = 100_000


def build(n_rows: int, capacity: int, seed: int) -> DenseIndex:
    """Rows with the even ids 0, 2, 4, ... (odd ids are free for the insertion)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ix = DenseIndex(1024, capacity=capacity)
    for lo in range(0, n_rows, STEP):
        m = min(STEP, n_rows - lo)
        ix.add(torch.randn(m, 1024, generator=g, device=DEV), 2 * torch.arange(lo, lo + m, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    return ix


def wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def reload_route(old: DenseIndex, keep_pos: np.ndarray) -> DenseIndex:
    """No removal existed: the remaining rows go into a new index with add."""
    new = DenseIndex(old.dim, capacity=old.capacity)
    keep = torch.as_tensor(keep_pos, device=DEV)
    for lo in range(0, len(old), STEP):
        m = min(STEP, len(old) - lo)
        buf = torch.empty(m, old.dim, dtype=torch.float32, device=DEV)
        ids = old.get_rows_into(lo, m, buf)
        sel = keep[(keep >= lo) & (keep < lo + m)] - lo
        if sel.numel():
            new.add(buf[sel], ids=ids[sel.cpu().numpy()])
    return new


def rebuild_route(old: DenseIndex, new_rows, new_ids: np.ndarray) -> DenseIndex:
    """DenseTable._rebuild(order=, extra=) as it stood before DenseIndex.insert existed."""
    n_old = len(old)
    new = DenseIndex(old.dim, capacity=old.capacity)
    rows = torch.empty(n_old, old.dim, dtype=torch.float32, device=DEV)
    ids = old.get_rows_into(0, n_old, rows)
    rows = torch.cat([rows, new_rows])
    ids = np.concatenate([ids, new_ids])
    order = np.argsort(ids, kind="stable")
    rows = rows[torch.as_tensor(order, device=DEV)]
    new.add(rows, ids=ids[order])
    return new


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    box = torch.cuda.get_device_properties(0).name
    for n in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(4100 + n % 991)
        pct = n // 100
        scattered = np.sort(rng.choice(n, pct, replace=False))
        near_end = np.arange(n - 10_000, n - 9_000)
        g = torch.Generator(device=DEV).manual_seed(99)
        new_rows = torch.randn(pct, 1024, generator=g, device=DEV)
        new_ids = 2 * scattered.astype(np.int64) + 1
        d_new_ids = torch.as_tensor(new_ids, device=DEV)
        edits = {
            "remove_1pct_scattered": ("remove", scattered, n - pct - int(scattered[0])),
            "remove_1pct_tail": ("remove", np.arange(n - pct, n), 0),
            "remove_1000_near_end": ("remove", near_end, 9_000),
            "insert_1pct_scattered": ("insert", None, n - 1 - int(scattered[0])),
        }
        for name, (kind, pos, moved) in edits.items():
            ms = []
            for t in range(args.trials):
                ix = build(n, n + pct, seed=7)
                if kind == "remove":
                    d_ids = torch.as_tensor(2 * pos.astype(np.int64), device=DEV)
                    ms.append(wall_ms(lambda: ix.remove(d_ids)))
                    assert len(ix) == n - pos.size
                else:
                    ms.append(wall_ms(lambda: ix.insert(new_rows, d_new_ids)))
                    assert len(ix) == n + pct
                ix.close()
            ix = build(n, n + pct, seed=7)
            made = []
            if kind == "remove":
                keep = np.setdiff1d(np.arange(n), pos)
                ms_old = wall_ms(lambda: made.append(reload_route(ix, keep)))
                old_route = "reload the remaining rows into a new index with add"
            else:
                ms_old = wall_ms(lambda: made.append(rebuild_route(ix, new_rows, new_ids)))
                old_route = "DenseTable._rebuild(order=, extra=) of the parent commit"
            made[0].close()
            ix.close()
            t_ms = float(np.median(ms))
            touched = moved * ROW_BYTES * 2 * 2
            line = {"bench": "index_edit", "box": box, "rows": n, "edit": name, "edited_rows": int(pct if pos is None else pos.size),
                    "moved_rows": int(moved), "ms": round(t_ms, 3), "ms_trials": [round(v, 3) for v in ms],
                    "bytes_touched": int(touched), "GBps": round(touched / t_ms / 1e6, 1),
                    "hbm_fraction": round(touched / (t_ms * 1e-3) / HBM_PEAK, 4),
                    "replaced_route": old_route, "ms_replaced_route": round(ms_old, 3),
                    "speedup": round(ms_old / t_ms, 2)}
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
