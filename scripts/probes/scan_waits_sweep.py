"""Developer probe: the two wait schedules of the mirror scan (CRAG_PF_WAITS=tile|fragment) side by side over corpus
sizes.  Per shape two indices over the same rows, one per schedule; the timed rounds alternate between them and the
median per schedule is reported (step time of the in-order search, no profiling events in the stream), then the scan
kernel's own time from the library's events.  One JSON line per shape.
   python scripts/probes/scan_waits_sweep.py [--out FILE] [--rounds 7] [--steps 400] 100000,64,10 ..."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from cadence_rag_amd.dense_index import DenseIndex  # noqa: E402

SCHEDULES = ("tile", "fragment")


def build(rows: int, schedule: str, dev) -> DenseIndex:
    os.environ["CRAG_PF_WAITS"] = schedule   # read once, when the index is created
    try:
        index = DenseIndex(1024, capacity=rows)
    finally:
        del os.environ["CRAG_PF_WAITS"]
    g = torch.Generator(device=dev).manual_seed(1234)
    for lo in range(0, rows, 131072):
        m = min(131072, rows - lo)
        c = torch.randn(m, 1024, generator=g, device=dev)
        index.add(c / c.norm(dim=1, keepdim=True))
    return index


def run(rows: int, nq: int, k: int, rounds: int, steps: int) -> dict:
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(4321)
    q = torch.randn(nq, 1024, generator=g, device=dev)
    q = q / q.norm(dim=1, keepdim=True)
    st = torch.cuda.current_stream().cuda_stream
    ix = {s: build(rows, s, dev) for s in SCHEDULES}
    out = {s: (torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, dtype=torch.float32, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev)) for s in SCHEDULES}

    def steps_of(s: str, n: int) -> float:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ix[s].search_async(q, k, *out[s], stream=st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    times = {s: [] for s in SCHEDULES}
    for r in range(rounds + 1):   # round 0 warms both up and is dropped
        for s in (SCHEDULES if r % 2 == 0 else SCHEDULES[::-1]):
            steps_of(s, 50)       # the other index's rows have just been through the cache: this one's back in
            t = steps_of(s, steps)
            if r:
                times[s].append(t)
    rec = {"rows": rows, "nq": nq, "k": k, "mirror_mib": round(rows * 2048 / 2**20, 1), "steps": steps, "rounds": rounds}
    for s in SCHEDULES:
        ix[s].prefilter_stats()
        ix[s].profile_enable(4)
        steps_of(s, steps)
        n, scan_ms, rest_ms = ix[s].profile_read()
        ix[s].profile_enable(0)
        stats = ix[s].prefilter_stats()
        rec[s] = {"step_us_median": round(statistics.median(times[s]), 2), "step_us_min": round(min(times[s]), 2),
                  "step_us_max": round(max(times[s]), 2), "step_us_rounds": [round(t, 2) for t in times[s]],
                  "scan_us_events": round(scan_ms / max(n, 1) * 1e3, 2), "rest_us_events": round(rest_ms / max(n, 1) * 1e3, 2),
                  "kernel": ix[s].last_scan_kernel(), "ran_with_waits": ix[s].scan_waits(),   # (nt kernels: tile only)
                  "rescored_per_search": stats["rescored_rows"] / max(stats["searches"], 1)}
    same = all(torch.equal(a, b) for a, b in zip(out["tile"], out["fragment"]))
    rec["outputs_equal"] = bool(same)
    rec["fragment_minus_tile_us"] = round(rec["fragment"]["step_us_median"] - rec["tile"]["step_us_median"], 2)
    for s in SCHEDULES:
        ix[s].close()
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = a.shapes or ["50000,64,10", "100000,64,10", "100000,64,100", "112000,64,10", "125000,64,10", "150000,64,10",
                          "250000,64,10", "500000,64,10", "1000000,64,10"]
    for s in shapes:
        r, nq, k = (int(v) for v in s.split(","))
        steps = a.steps if r <= 250_000 else max(a.steps // 4, 50)
        line = json.dumps(run(r, nq, k, a.rounds, steps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
