"""Facet counts on the GPU beside two yardsticks measured in the same run.  Per size (100 000 and
1 000 000 rows: one speaker of 8, one kind of 6 and 0-3 entities of one label from a Zipf-like pool of 50 000) and batch
(1 and 64 queries), requesting "speaker", "kind" and "entity:SERVICE" with top 10:
  * stream time of one FacetColumns.counts call (HIP events on one stream, warm, median of three runs) without masks
    (unfiltered) and under per-query date masks, and the bytes such a call must touch -- the requested postings (8 bytes
    each), the masks read and the query sets written and read (masked calls), the count table zeroed, added to and read
    -- over that time as a fraction of the HBM rate;
  * the phases of the masked call, from calls that run a part of it: masks without namespaces (the transpose alone) and
    namespaces without masks (count + select); of the unfiltered call its two kinds of namespace apart: "speaker" +
    "kind" (a few values over every row) and the entity label (the long tail);
  * yardstick 1: the attribute-mask launch (crag_attr_masks_host) on the same table and batch size, one entity clause and
    a speakers clause per query (the method of attr_filter_time.py);
  * yardstick 2: filters.facets_host on the CPU for ONE query (it walks every row in Python), whose answer the device
    answer of query 0 must equal.
Appends one JSON line per case to profiles/facet_bench.jsonl.

  python scripts/probes/facet_time.py [--rows 100000 1000000] [--iters 30] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from cadence_rag_amd import filters as fl  # noqa: E402
from cadence_rag_amd import retrieve as rt  # noqa: E402

HBM_TBPS = 6.29   # measured copy bandwidth of the part: the rate the byte count is taken at
NAMES = ["speaker", "kind", "entity:SERVICE"]
N_SPEAKERS, N_KINDS, POOL, TOP = 8, 6, 50000, 10
DAY_US = 86400 * 10 ** 6


def make_rows(n, rng):
    speakers, kinds = rng.integers(0, N_SPEAKERS, n), rng.integers(0, N_KINDS, n)
    how_many = rng.integers(0, 4, n)
    picks = np.minimum(rng.zipf(1.2, (n, 3)) - 1, POOL - 1)
    return [[("speaker", f"speaker {s}"), ("kind", f"kind {k}")] + [("entity:SERVICE", f"svc-{v:05d}") for v in p[:m]]
            for s, k, m, p in zip(speakers.tolist(), kinds.tolist(), how_many.tolist(), picks.tolist())]


def stream_us(stream, call, iters):
    """Median of three warm runs of `iters` calls between two events on `stream`, per call."""
    with torch.cuda.stream(stream):
        for _ in range(5):
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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "facet_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(14)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    for n in args.rows:
        rows = make_rows(n, rng)
        acols = fl.AttributeColumns(rows, device=dev)
        t = time.perf_counter()
        cols = fl.FacetColumns(acols, device=dev)
        build_s = time.perf_counter() - t
        started = rng.integers(0, 365, n).astype(np.int64) * DAY_US
        fcols = fl.FilterColumns(started.astype("datetime64[us]"), [0] * n, device=dev)
        lo, hi = cols.requested(NAMES)
        width = int((hi - lo).sum())
        postings = int(sum(cols.post_ptr[h] - cols.post_ptr[l] for l, h in zip(lo, hi)))
        stride = fl.mask_bytes(n)
        try:
            for nq in (1, 64):
                date_from = (np.arange(nq, dtype=np.int64) * 5 + 30) * DAY_US          # the last 335 .. 20 days
                date_to = np.full(nq, fl.NO_UPPER, dtype=np.int64)
                F = rt.RetrieveFilters
                attrs = fl.compile_attr_predicates(acols, [
                    (F(entity_filters=[{"label": "service", "value": f"svc-{q:05d}"}], speakers=[f"speaker {q % 8}", "speaker 3"]), None)
                    for q in range(nq)])
                with torch.cuda.stream(stream):
                    masks = fcols.masks(None, date_from, date_to, stream=s)
                    out = torch.empty((nq, stride), dtype=torch.uint8, device=dev)
                    work = torch.empty(8 * n + 4 * nq * width, dtype=torch.uint8, device=dev)
                mask_us = stream_us(stream, lambda: acols.masks(attrs, out=out, stream=s), args.iters)
                t = time.perf_counter()
                want = fl.facets_host(rows, None, NAMES, TOP)
                host_ms = (time.perf_counter() - t) * 1e3
                for case, m in (("unfiltered", None), ("date_filtered", masks)):
                    call = lambda: cols.counts(NAMES, masks=m, nq=nq, top=TOP, stream=s, workspace=work)
                    us = stream_us(stream, call, args.iters)
                    table = 4 * nq * width
                    touched = 8 * postings + 3 * table + (nq * stride + 16 * n if m is not None else 0)
                    rec = {"case": case, "rows": n, "nq": nq, "top": TOP, "namespaces": NAMES, "postings": postings,
                           "width": width, "build_columns_s": round(build_s, 2), "facet_call_us": round(us, 2),
                           "bytes_touched": touched, "floor_tbps": HBM_TBPS,
                           "fraction_of_hbm_rate": round(touched / (HBM_TBPS * 1e12) * 1e6 / us, 4),
                           "attr_mask_call_us": round(mask_us, 2), "times_the_mask_call": round(us / mask_us, 2),
                           "facets_host_one_query_ms": round(host_ms, 1)}
                    if m is None:
                        # the two kinds of namespace apart: a few values over every row, and the long tail
                        rec["hot_namespaces_only_us"] = round(stream_us(
                            stream, lambda: cols.counts(NAMES[:2], nq=nq, top=TOP, stream=s, workspace=work), args.iters), 2)
                        rec["entity_namespace_only_us"] = round(stream_us(
                            stream, lambda: cols.counts(NAMES[2:], nq=nq, top=TOP, stream=s, workspace=work), args.iters), 2)
                        with torch.cuda.stream(stream):
                            got = cols.counts(NAMES, nq=nq, top=TOP, stream=s, workspace=work)
                        stream.synchronize()
                        listed = cols.lists(NAMES, *(x.cpu().numpy() for x in got))[0]
                        assert listed["rows"] == want[0], "the device rows differ from facets_host"
                        for ns in NAMES:
                            assert ([(v["value"], v["count"]) for v in listed["facets"][ns]["values"]], listed["facets"][ns]["distinct"]) \
                                == want[1][ns], f"the device list of {ns} differs from facets_host"
                    else:
                        rec["transpose_alone_us"] = round(stream_us(
                            stream, lambda: cols.counts([], masks=m, top=TOP, stream=s, workspace=work), args.iters), 2)
                        rec["count_and_select_no_masks_us"] = round(stream_us(
                            stream, lambda: cols.counts(NAMES, nq=nq, top=TOP, stream=s, workspace=work), args.iters), 2)
                    print(json.dumps(rec), flush=True)
                    with open(args.out, "a") as fh:
                        fh.write(json.dumps(rec) + "\n")
        finally:
            acols.close()
            fcols.close()


if __name__ == "__main__":
    main()
