"""Attribute masks on the GPU against the host route: per size (100 000 and 1 000 000 rows, about 4
attributes per row: a speaker and three entities on average) and batch (1 and 64 queries of 2 clauses: one entity filter
and a speakers list)
  * stream time of one crag_attr_masks_host call (its one upload + the kernel; HIP events on one stream, warm, median of
    three runs) without an input mask and in place over a per-query mask, and the fraction of its byte floor
    (8 (n + 1) + 4 nnz read, the input mask read, nq * stride written);
  * stream time of crag_filter_masks_host alone on the same rows and batch size (date bounds + 200 call ids per query);
  * host time of the route a caller without the kernel takes: DenseTable.filter_mask + pack_mask + upload, per query
    (measured on the first queries of the batch: the host rule walks every row once per query).
The tables are host columns only (no vectors).  Appends one JSON line per size to profiles/attr_mask_bench.jsonl.

  python scripts/probes/attr_filter_time.py [--rows 100000 1000000] [--iters 50] [--host-queries 2] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from datetime import datetime, timedelta
from pathlib import Path
from uuid import UUID

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from cadence_rag_amd import filters as fl  # noqa: E402
from cadence_rag_amd import retrieve as rt  # noqa: E402
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402

HBM_TBPS = 6.29   # measured copy bandwidth of the part: the rate the byte floor is taken at
T0 = datetime(2024, 1, 1)
N_CALLS, N_SPEAKERS, N_ORGS, N_PEOPLE = 20000, 40, 50, 20000


class _Rows:
    def __init__(self, n):
        self.n, self.device = n, 0

    def __len__(self):
        return self.n


def make_table(n, calls, rng):
    """The host side of a chunks table: filter_mask and the column builders read nothing else."""
    table = object.__new__(rt.DenseTable)
    table.name, table.id_field, table.index, table.generation = "chunks", "chunk_id", _Rows(n), 0
    call_of = rng.integers(0, len(calls), n)
    table.call_ids = np.asarray([calls[int(c)] for c in call_of], dtype=object)
    table.call_started_at = (np.datetime64(T0, "us") + call_of.astype("timedelta64[m]")).astype("datetime64[us]")
    table.call_tags = {}
    speakers, orgs, people = rng.integers(0, N_SPEAKERS, n), rng.integers(0, N_ORGS, n), rng.integers(0, N_PEOPLE, n)
    extra = rng.integers(0, 5, n)        # 0-4 further entities: 3 per row on average with the org
    table.columns = {"chunk_id": list(range(n)), "speaker": [f"speaker {int(s)}" for s in speakers]}
    table.entities = [[("org", f"org {int(o)}")] + [("person", f"person {int(p) + j}") for j in range(int(e))]
                      for o, p, e in zip(orgs, people, extra)]
    return table


def batch_of(nq, calls, rng):
    out = []
    for q in range(nq):
        ids = [calls[int(i)] for i in rng.choice(len(calls), size=200, replace=False)]
        out.append((rt.RetrieveFilters(date_from=T0 + timedelta(minutes=100 * q), date_to=T0 + timedelta(minutes=15000),
                                       call_ids=ids, entity_filters=[{"label": "org", "value": f"org {int(rng.integers(0, N_ORGS))}"}],
                                       speakers=[f"speaker {int(s)}" for s in rng.integers(0, N_SPEAKERS, 4)]), ids))
    return out


def stream_us(stream, call, iters):
    """Median of three warm runs of `iters` calls between two events on `stream`, per call."""
    with torch.cuda.stream(stream):
        for _ in range(10):
            call()
        runs = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(iters):
                call()
            b.record(stream)
            b.synchronize()
            runs.append(a.elapsed_time(b) / iters * 1e3)
    return float(np.median(runs))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attr_mask_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    calls = [UUID(int=i + 1) for i in range(N_CALLS)]
    stream = torch.cuda.Stream(device=dev)
    for n in args.rows:
        table = make_table(n, calls, rng)
        t = time.perf_counter()
        acols = fl.AttributeColumns(table._row_attrs(), device=dev)
        build_s = time.perf_counter() - t
        fcols = fl.FilterColumns(table.call_started_at, table.call_ids, device=dev)
        nnz = int(acols.attr_ids.size)
        rec = {"rows": n, "attrs": nnz, "dictionary": acols.n_attrs, "floor_tbps": HBM_TBPS, "build_columns_s": round(build_s, 2)}
        stride = fl.mask_bytes(n)
        try:
            for nq in (1, 64):
                batch = batch_of(nq, calls, rng)
                t = time.perf_counter()
                attrs = fl.compile_attr_predicates(acols, batch)
                rec[f"compile_q{nq}_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                rec[f"keys_q{nq}"] = int(attrs[0].size)
                compiled = fl.compile_predicates(fcols, table.call_tags, batch)
                with torch.cuda.stream(stream):
                    out = torch.empty((nq, stride), dtype=torch.uint8, device=dev)
                    base = torch.empty((nq, stride), dtype=torch.uint8, device=dev)
                s = stream.cuda_stream
                us = stream_us(stream, lambda: acols.masks(attrs, out=out, stream=s), args.iters)
                floor = 8 * (n + 1) + 4 * nnz + nq * stride
                rec[f"attr_call_q{nq}_us"] = round(us, 2)
                rec[f"attr_fraction_of_floor_q{nq}"] = round(floor / (HBM_TBPS * 1e12) * 1e6 / us, 4)
                rec[f"filter_call_q{nq}_us"] = round(stream_us(stream, lambda: fcols.masks(*compiled, out=base, stream=s), args.iters), 2)
                # in place over the filter kernel's masks (repeating it only clears bits: the time does not depend on them)
                us = stream_us(stream, lambda: acols.masks(attrs, in_mask=base, in_stride=stride, out=base, stream=s), args.iters)
                rec[f"attr_in_place_q{nq}_us"] = round(us, 2)
                rec[f"attr_in_place_fraction_of_floor_q{nq}"] = round((floor + nq * stride) / (HBM_TBPS * 1e12) * 1e6 / us, 4)
                with torch.cuda.stream(stream):
                    fcols.masks(*compiled, out=base, stream=s)
                    acols.masks(attrs, in_mask=base, in_stride=stride, out=base, stream=s)
                stream.synchronize()
                m = min(nq, args.host_queries)
                t = time.perf_counter()
                host = torch.stack([torch.from_numpy(DenseIndex.pack_mask(table.filter_mask(f, c))).to(dev) for f, c in batch[:m]])
                torch.cuda.synchronize(dev)
                rec[f"host_route_per_query_q{nq}_ms"] = round((time.perf_counter() - t) * 1e3 / m, 2)
                assert torch.equal(host, base[:m]), "the device masks differ from the host route's"
                rec[f"rows_passing_q{nq}"] = int(np.unpackbits(base.cpu().numpy()).sum())
        finally:
            acols.close()
            fcols.close()
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
