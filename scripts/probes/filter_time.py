"""Filter masks on the GPU against the host route they replace: per size (100 000 and 1 000 000 rows,
20 000 calls) and batch (1 and 64 queries)
  * stream time of one crag_filter_masks_host call (its one upload + the kernel; HIP events on one stream, warm) and
    the fraction of its byte floor (12 n + 8 n_calls read, nq * stride written);
  * host time of the route every caller took before: DenseTable.filter_mask + pack_mask + upload, per batch;
and per size the wall time of one scoped retrieve_evidence request (dense lanes of two tables: chunks of n rows,
artifact chunks of n / 10; four mask uses) with the device mask and with filter_mask_device replaced by that host route,
alternating.  Appends one JSON line per size to profiles/filter_mask_bench.jsonl.

  python scripts/probes/filter_time.py [--rows 100000 1000000] [--calls 20000] [--iters 100] [--out FILE]"""
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
from cadence_rag_amd import embeddings  # noqa: E402
from cadence_rag_amd import filters as fl  # noqa: E402
from cadence_rag_amd import retrieve as rt  # noqa: E402
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402

HBM_TBPS = 6.29   # measured copy bandwidth of the part: the rate the byte floor is taken at
T0 = datetime(2024, 1, 1)


def make_table(name, id_field, n, calls, rng, dev):
    table = rt.DenseTable(name, id_field, dim=1024, capacity=n)
    body = "text" if id_field == "chunk_id" else "content"
    call_of = rng.integers(0, len(calls), n)
    step = 65536
    for lo in range(0, n, step):
        m = min(step, n - lo)
        vecs = torch.randn(m, 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(lo + 1))
        cols = {id_field: list(range(lo, lo + m)), "call_id": [calls[int(c)] for c in call_of[lo:lo + m]],
                body: ["row"] * m}
        if id_field == "chunk_id":
            cols.update(speaker=["S"] * m, start_ts_ms=[0] * m, end_ts_ms=[1] * m)
        else:
            cols.update(artifact_id=[0] * m, kind=["summary"] * m)
        started = [T0 + timedelta(minutes=int(c)) for c in call_of[lo:lo + m]]
        table.add(vecs, cols, call_started_at=started,
                  call_tags={c: ["outage"] if i % 3 == 0 else ["billing"] for i, c in enumerate(calls)} if lo == 0 else None)
    return table


def batch_of(nq, calls, rng):
    out = []
    for q in range(nq):
        ids = [calls[int(i)] for i in rng.choice(len(calls), size=200, replace=False)]
        out.append((rt.RetrieveFilters(date_from=T0 + timedelta(minutes=100 * q), date_to=T0 + timedelta(minutes=15000),
                                       call_ids=ids), ids))
    return out


def host_route(table, filters, call_ids):
    mask = rt.DenseTable.filter_mask(table, filters, call_ids)
    return None if mask is None else torch.from_numpy(DenseIndex.pack_mask(mask)).to(torch.device("cuda", table.index.device))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filter_mask_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    calls = [UUID(int=i + 1) for i in range(args.calls)]
    stream = torch.cuda.Stream(device=dev)
    for n in args.rows:
        rec = {"rows": n, "calls": args.calls, "floor_tbps": HBM_TBPS}
        chunks = make_table("chunks", "chunk_id", n, calls, rng, dev)
        arts = make_table("artifact_chunks", "artifact_chunk_id", max(n // 10, 1), calls, rng, dev)
        try:
            cols = chunks.filter_columns()
            for nq in (1, 64):
                batch = batch_of(nq, calls, rng)
                t = time.perf_counter()
                compiled = fl.compile_predicates(cols, chunks.call_tags, batch)
                rec[f"compile_q{nq}_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                stride = fl.mask_bytes(n)
                with torch.cuda.stream(stream):
                    out = torch.empty((nq, stride), dtype=torch.uint8, device=dev)
                    for _ in range(20):
                        cols.masks(*compiled, out=out, stream=stream.cuda_stream)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(args.iters):
                        cols.masks(*compiled, out=out, stream=stream.cuda_stream)
                    b.record(stream)
                    b.synchronize()
                us = a.elapsed_time(b) / args.iters * 1e3
                nbytes = 12 * n + 8 * cols.n_calls + nq * stride
                rec[f"device_call_q{nq}_us"] = round(us, 2)
                rec[f"bytes_q{nq}"] = nbytes
                rec[f"fraction_of_floor_q{nq}"] = round(nbytes / (HBM_TBPS * 1e12) * 1e6 / us, 4)
                t = time.perf_counter()
                host = torch.stack([host_route(chunks, f, c) for f, c in batch])
                torch.cuda.synchronize(dev)
                rec[f"host_route_q{nq}_ms"] = round((time.perf_counter() - t) * 1e3, 2)
                assert torch.equal(host, out), "the device masks differ from the host route's"
            # one scoped request, dense lanes only (no lexical lanes attached), alternating the two routes
            qvec = torch.randn(1024, generator=torch.Generator().manual_seed(5)).tolist()
            embeddings_enabled, embed_texts = embeddings.embeddings_enabled, embeddings.embed_texts
            embeddings.embeddings_enabled = lambda: True
            embeddings.embed_texts = lambda texts: embeddings.EmbeddingResult(vectors=[qvec for _ in texts], model="probe")
            be = rt.GpuRetrieveBackend(chunks, arts)
            device_route = rt.DenseTable.filter_mask_device
            walls = {"device": [], "host": []}
            try:
                for rep in range(6):
                    f, _ = batch_of(1, calls, rng)[0]      # fresh predicates: the memo serves the lanes of ONE request
                    for name, route in (("device", device_route), ("host", host_route)):
                        rt.DenseTable.filter_mask_device = route
                        torch.cuda.synchronize(dev)
                        t = time.perf_counter()
                        resp = rt.retrieve_evidence(rt.RetrieveRequest(query="scoped probe", filters=f), be)
                        walls[name].append((time.perf_counter() - t) * 1e3)
                        walls[name + "_rows"] = resp["notes"]["retrieval"]["dense_candidate_rows"]
            finally:
                rt.DenseTable.filter_mask_device = device_route
                embeddings.embeddings_enabled, embeddings.embed_texts = embeddings_enabled, embed_texts
            assert walls["device_rows"] == walls["host_rows"]
            rec["request_device_ms"] = round(float(np.median(walls["device"][1:])), 3)   # (the first repeat warms up)
            rec["request_host_route_ms"] = round(float(np.median(walls["host"][1:])), 3)
            rec["request_candidate_rows"] = walls["device_rows"]
        finally:
            chunks.close()
            arts.close()
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
